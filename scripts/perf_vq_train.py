"""Times the trainable Taming VQGAN on one MI355X at TAMING_VQ, B = 4 (synthetic weights): encode forward + backward, decode forward +
backward, one full rcc_loss step -- and the same restated network under PyTorch-ROCm fp32 autograd on the same GPU as the reference
point.  Events around each call, 2 warm-up runs, median of 5.  Prints one line per figure and device_bytes.

    python scripts/perf_vq_train.py [--config taming|harness] [--batch 4] [--no-torch]

The share of the wgrad launches comes from a separate run under `rocprofv3 --kernel-trace --stats -- python scripts/perf_vq_train.py
--no-torch` (kernels k_wgrad<3>, k_wgrad<1>, k_fold_splits in the table it writes)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="taming", choices=["taming", "harness"])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from tests import vq_grad_reference as G
    from wmar_amd import finetune as ft
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = synth.TAMING_VQ if args.config == "taming" else synth.VQConfig(**synth.HARNESS_VQ)
    B, S, R = args.batch, cfg.codes_size, cfg.resolution
    state = {k: v.contiguous() for k, v in synth.synth_vq_state_fast(cfg, 0, "cuda").items()}
    tok = TrainableTokenizer(cfg, state, max_batch=B)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(B, 3, R, R, device="cuda", generator=g) * 2 - 1
    z = torch.randn(B, cfg.embed_dim, S, S, device="cuda", generator=g)
    rx, rz = torch.randn_like(x), torch.randn_like(z)
    codes = torch.randint(0, cfg.n_embed, (B, S * S), device="cuda", generator=g)

    def clear(params):
        for p in params:
            p.grad = None

    def enc(t, params):
        clear(params)
        xi = x.clone().requires_grad_(True)
        (t.encode_prequant(xi) * rz).sum().backward()

    def dec(t, params):
        clear(params)
        zi = z.clone().requires_grad_(True)
        (t.decode(zi) * rx).sum().backward()

    def rcc(t, params):
        clear(params)
        ft.rcc_loss(t, codes, [], loss_weight=1.0, orig=None)[0].backward()

    rows = []
    params = list(tok.parameters())
    for name, fn in (("encode fwd+bwd", enc), ("decode fwd+bwd", dec), ("rcc_loss step", rcc)):
        rows.append(("hip", name) + timed(lambda: fn(tok, params)))
    print("device_bytes %d (%.2f GB)" % (tok.device_bytes, tok.device_bytes / 2 ** 30), flush=True)
    if not args.no_torch:
        ref = G.TorchTokenizer(cfg, {k: v.detach().cpu() for k, v in state.items()})
        ref.state = {k: v.detach().cuda().requires_grad_(not k.startswith("quantize.")) for k, v in ref.state.items()}
        rparams = list(ref.parameters())
        for name, fn in (("encode fwd+bwd", enc), ("decode fwd+bwd", dec), ("rcc_loss step", rcc)):
            rows.append(("torch fp32 autograd", name) + timed(lambda: fn(ref, rparams)))
    for who, name, med, lo, hi in rows:
        print("PERF %-20s %-16s median %9.2f ms  (min %.2f, max %.2f)  config=%s B=%d" % (who, name, med, lo, hi, args.config, B), flush=True)


if __name__ == "__main__":
    main()
