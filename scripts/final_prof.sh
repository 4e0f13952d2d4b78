#!/bin/bash
# Run on the GPU box: the full bench line (--full), then the same command under rocprofv3 (kernel trace + stats).
# usage: scripts/final_prof.sh <round tag, e.g. r02> [output dir, default bench_out]   -> <dir>/<tag>_bench_line.json, <dir>/<tag>_prof/.../*kernel_stats.csv
tag=${1:-r02}
cd "$(dirname "$0")/.."
mkdir -p "${2:-bench_out}"; out=$(cd "${2:-bench_out}" && pwd)
python bench.py --full > $out/${tag}_bench_line.json 2> $out/${tag}_bench_line.err
tail -1 $out/${tag}_bench_line.json | cut -c1-600
R=$PWD
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof -- python $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-parity --no-secondary > $out/${tag}_prof.json 2> $out/${tag}_prof.err
cd $R
rm -f $out/${tag}_prof/*/*kernel_trace.csv; ls $out/${tag}_prof/*/ | head
