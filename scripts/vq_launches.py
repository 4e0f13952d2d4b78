"""The ordered kernel launches of one encode + decode of a tokenizer's inference engine at its small test config, for comparing two builds
launch by launch (profiles/vq_plan_launches_*.csv).  WMAR_ROOT=<another checkout or build_alt snapshot> runs that build.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/vq_launches.py run taming|mvq
    python scripts/vq_launches.py table DIR OUT.csv      # (kernel, grid, workgroup) in start order, from the first layout kernel on
"""
import csv
import glob
import os
import sys


def run(net):
    sys.path.insert(0, os.environ.get("WMAR_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from wmar_amd.models.engine import MaskgitVQEngine, VQGANEngine
    from wmar_amd.utils import synth
    if net == "taming":
        cfg = synth.VQConfig(**synth.HARNESS_VQ)
        sd, Eng, n_codes = synth.synth_vq_state(cfg, 5, "cpu"), VQGANEngine, cfg.n_embed
    else:
        cfg = synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16, num_embeddings=512)
        sd, Eng, n_codes = synth.synth_maskgit_state(cfg, 5, "cpu"), MaskgitVQEngine, cfg.num_embeddings
    eng = Eng(cfg, {k: v.detach().to("cuda", torch.float32).contiguous() for k, v in sd.items()}, max_batch=2)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 3, cfg.resolution, cfg.resolution, generator=g) * 2 - 1).cuda()
    codes = torch.randint(0, n_codes, (2, cfg.codes_size ** 2), generator=g).cuda()
    torch.cuda.synchronize()
    c = eng.encode(x)
    img = eng.decode(codes)
    torch.cuda.synchronize()
    print("ok", net, int(c.sum()), float(img.sum()))


def table(trace_dir, out):
    files = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    key = {k.lower(): k for k in rows[0]}
    rows.sort(key=lambda r: int(r[key["start_timestamp"]]))
    name = lambda n: n.split("(")[0].strip().replace("void ", "").replace("wmar::", "")
    seq = [(name(r[key["kernel_name"]]),) + tuple(r[key[c]] for c in ("grid_size_x", "grid_size_y", "grid_size_z", "workgroup_size_x")) for r in rows]
    start = next(i for i, s in enumerate(seq) if s[0].startswith("k_nchw_to_nhwc"))      # create-time packing lies in front of it
    seq = [s for s in seq[start:] if s[0].startswith("k_")]
    with open(out, "w") as f:
        f.write("kernel,grid_x,grid_y,grid_z,workgroup_x\n")
        for s in seq:
            f.write(",".join(s) + "\n")
    print(out, len(seq), "launches")


if __name__ == "__main__":
    run(sys.argv[2]) if sys.argv[1] == "run" else table(sys.argv[2], sys.argv[3])
