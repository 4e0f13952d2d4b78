"""Cost of the hooked generation mode against the fused loops ("Hooked generation"), on one GPU.

    python scripts/perf_hook.py [--configs taming64,taming5,taming1,rar64,cham16] [--runs 5]
    python scripts/perf_hook.py --configs taming64 --trace          one warm hooked generation (run it under a kernel trace)

Full-size models with synthetic weights.  Timing method of DESIGN.md section 6: host clock around one whole generation (256 steps;
Chameleon: 1024 image tokens behind the prompt) ending in one device synchronise, `--runs` runs, median (min - max) in ms per step,
one process.  Per configuration:
    (i)   fused loop, no watermark              (iii) fused loop, greenlist key table
    (ii)  hooked, identity processor            (iv)  hooked, the greenlist written in torch (tests/hook_processors.greenlist_from_table)
(i) and (iii) are the loops this mode leaves untouched: the comparator.  The four are alternated inside every run, so that drift of
the box hits them alike; (iv) must return the tokens of (iii), (ii) those of (i)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests import hook_processors as HP  # noqa: E402


def _stat(xs):
    return f"{statistics.median(xs):.4f} ({min(xs):.4f} - {max(xs):.4f})"


def _gentime(m, V, h=1, seed="linear"):
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    return GentimeWatermark(m.get_vq(), V, SeedStrategy(seed), SplitStrategy.RANDOM_STRATIFIED, h, 2.0, 0.25, device="cuda")


def build(name):
    """(model, conditioning, gen_params, steps, watermarker, noise)"""
    from wmar_amd.utils import synth
    if name.startswith("taming"):
        from wmar_amd.models.taming_wrapper import TamingARMMWrapper
        B = int(name[len("taming"):])
        m = TamingARMMWrapper.synthetic(synth.TAMING_GPT, synth.TAMING_VQ, seed=0, max_batch=B)
        steps = m.codes_size ** 2
        torch.manual_seed(1)
        return m, (torch.arange(B) * 37 % 1000).tolist(), {"temperature": 1.0, "top_k": 250, "top_p": 0.92}, steps, \
            _gentime(m, m.get_total_vocab_size()), m.draw_noise(steps, B)
    if name.startswith("rar"):
        from wmar_amd.models.rar_wrapper import RarARMMWrapper
        B = int(name[len("rar"):])
        m = RarARMMWrapper.synthetic(max_batch=B)
        torch.manual_seed(1)
        return m, (torch.arange(B) * 13 % 1000).tolist(), None, m.model.cfg.image_seq_len, _gentime(m, 1024), m.draw_noise(B)
    from wmar_amd.models.chameleon_wrapper import ChameleonARMMWrapper
    B = int(name[len("cham"):])
    m = ChameleonARMMWrapper.synthetic(seed=0, max_batch=B)
    text = m.vocab.text_tokens
    cond = [(c, [text[(c * 37 + j * 11) % len(text)] for j in range(12 + c % 5)]) for c in range(B)]
    torch.manual_seed(1)
    # FIXED seeding: one table row (a LINEAR key over 65536 entries is a 512 MiB table the torch processor would index per step)
    return m, cond, {"temperature": 1.0, "top_p": 0.9}, m.n_image_tokens, _gentime(m, m.get_total_vocab_size(), 0, "fixed"), m.draw_noise(B)


def run(name, runs, trace):
    m, cond, gp, steps, wm, q = build(name)
    green = HP.greenlist_from_table(wm)
    m.set_watermarker(wm)
    modes = {"i fused": dict(apply_watermark=False), "ii hooked identity": dict(logit_processor=HP.identity),
             "iii fused greenlist": dict(apply_watermark=True), "iv hooked greenlist": dict(logit_processor=green)}
    if trace:
        modes = {"iv hooked greenlist": modes["iv hooked greenlist"]}
    codes = {k: m.sample(cond, gp, q=q, **kw) for k, kw in modes.items()}       # warm-up: code objects, graphs, tables
    torch.cuda.synchronize()
    if not trace:
        assert torch.equal(codes["ii hooked identity"], codes["i fused"]) and torch.equal(codes["iv hooked greenlist"], codes["iii fused greenlist"])
    ms = {k: [] for k in modes}
    for r in range(1 if trace else runs):
        for k, kw in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = m.sample(cond, gp, q=q, **kw)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
            assert torch.equal(c, codes[k])
    for k in modes:
        print(f"{name:9s} {k:20s} ms/step {_stat(ms[k])}", flush=True)
    if not trace:
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(f"{name:9s} hooked - fused: identity {1e3 * (med['ii hooked identity'] - med['i fused']):+.1f} us/step, "
              f"greenlist {1e3 * (med['iv hooked greenlist'] - med['iii fused greenlist']):+.1f} us/step", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="taming64,taming5,taming1,rar64,cham16")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    for name in a.configs.split(","):
        run(name, a.runs, a.trace)
