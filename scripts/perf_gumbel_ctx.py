"""Timing of the Gumbel-key generation, fixed key against context-keyed, on one GPU.

    python scripts/perf_gumbel_ctx.py gen   [--ngrams 0,1,4] [--runs 5]   RAR-XL, batch 64 under guidance, 256 positions: ms / step
    python scripts/perf_gumbel_ctx.py eager [--runs 5]                    gumbel_sample with distinct hashes: device rows against host builds
    python scripts/perf_gumbel_ctx.py trace [--ngrams 1]                  one warm generation per ngram (run it under a kernel trace)

`gen` alternates the ngrams inside every run, so that drift of the box hits them alike.  WMAR_ROOT=<another checkout> times that
checkout's fixed-key path with `--ngrams 0` (the comparison against the parent commit)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("WMAR_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _stat(xs):
    return f"median {statistics.median(xs):.4f}  min {min(xs):.4f}  max {max(xs):.4f}  (n = {len(xs)})"


def gen(ngrams, runs, trace=False):
    from wmar_amd.models.rar_wrapper import RarARMMWrapper
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    B = 64
    m = RarARMMWrapper.synthetic(max_batch=B)
    L = m.model.cfg.image_seq_len
    cond = torch.arange(B) * 13 % 1000
    wms = {n: (GumbelWatermark(1024, seed=1234, device="cuda", ngram=n) if n else GumbelWatermark(1024, seed=1234, device="cuda"))
           for n in ngrams}
    noise = {}
    for n in ngrams:                     # warm-up: code objects, the unconditional adaLN table, the captured graph's shapes
        m.set_watermarker(wms[n])
        torch.manual_seed(1)
        noise[n] = m.draw_gumbel_noise(B, n) if n else None
        m.sample(cond, None, True, q=noise[n])
    torch.cuda.synchronize()
    ms = {n: [] for n in ngrams}
    codes = {}
    for r in range(1 if trace else runs):
        for n in ngrams:
            m.set_watermarker(wms[n])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = m.sample(cond, None, True, q=noise[n])
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / L * 1e3)
            assert n not in codes or torch.equal(codes[n], c)
            codes[n] = c
    for n in ngrams:
        rows = len({tuple(r) for r in codes[n].cpu().tolist()})
        print(f"gen ngram={n}: ms/step {_stat(ms[n])}  distinct rows {rows}/{B}  p_median {float(wms[n].detect(codes[n]).median()):.2e}",
              flush=True)


def eager(runs):
    from wmar_amd.watermarking import gumbel_watermark as G

    def host_rows(h, V):                 # what the parent commit did: one host build and three copies per distinct hash
        G._KEYS.clear()
        return torch.stack([G.key_for(int(x), V, "cuda")[1] for x in h.tolist()]).contiguous()

    for B, V in ((128, 1024), (5, 16384)):
        g = torch.Generator().manual_seed(B)
        lg = (torch.randn(B, V, generator=g) * 4).cuda()
        h = torch.randint(0, 2 ** 31 - 1, (B,), generator=g)
        assert len(set(h.tolist())) == B
        out = torch.empty(B, dtype=torch.int64, device="cuda")
        t_dev, t_host = [], []
        for r in range(runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a = G.gumbel_sample(lg, h, True, 1.0, 0.0, 0)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            key = host_rows(h, V)
            G._lib.check(G._lib.load().wmar_gumbel_sample(lg.data_ptr(), B, V, key.data_ptr(), V, 1, 1.0, 0.0, 0, out.data_ptr(),
                                                          G._lib.stream_ptr(lg.device)))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert torch.equal(a, out)
            if r:                        # the first pass loads code objects
                t_dev.append((t1 - t0) * 1e3)
                t_host.append((t2 - t1) * 1e3)
        print(f"eager gumbel_sample B={B} V={V}: device rows ms/call {_stat(t_dev)} | host builds ms/call {_stat(t_host)}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["gen", "eager", "trace"])
    ap.add_argument("--ngrams", default="0,1,4")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.mode == "eager":
        eager(a.runs)
    else:
        gen([int(x) for x in a.ngrams.split(",")], a.runs, trace=a.mode == "trace")
