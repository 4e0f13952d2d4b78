"""Times LPIPS on one MI355X at full width, 256 x 256, B = 4 (synthetic weights): forward + backward of the native engine, the same loss
restated in torch (tests/lpips_reference.py) under PyTorch-ROCm fp32 autograd on the same GPU, and one rcc_loss step of the Taming
tokenizer (TAMING_VQ) with the L1 regulariser alone and with the reference's L1 + LPIPS.  Events around each call, 2 warm-up runs,
median of 5.  Prints one PERF line per figure, device_bytes at max_batch 1 and B, and the per-image difference (the tape).

    python scripts/perf_lpips.py [--batch 4] [--resolution 256] [--lpips-only] [--no-torch]

The per-kernel shares come from a separate run under `rocprofv3 --kernel-trace --stats -- python scripts/perf_lpips.py --lpips-only
--no-torch`."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.perf_vq_train import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--lpips-only", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from tests import lpips_reference as LR
    from wmar_amd import finetune as ft
    from wmar_amd.lpips import LPIPS
    from wmar_amd.utils import synth
    B, R = args.batch, args.resolution
    state = synth.synth_lpips_state(seed=0)
    one = LPIPS(state, resolution=R, max_batch=1)
    lp = LPIPS(state, resolution=R, max_batch=B)
    b1, bB = one.device_bytes, lp.device_bytes
    print("device_bytes max_batch=1 %d  max_batch=%d %d  per image %d (%.1f MB)" % (b1, B, bB, (bB - b1) // max(B - 1, 1),
                                                                                   (bB - b1) / max(B - 1, 1) / 1e6), flush=True)
    del one
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(B, 3, R, R, device="cuda", generator=g) * 2 - 1
    t = (x + 0.1 * torch.randn(B, 3, R, R, device="cuda", generator=g)).clamp(-1, 1)

    def native():
        xi = x.clone().requires_grad_(True)
        lp(xi, t).sum().backward()

    rows = []

    def record(who, name, fn):
        rows.append((who, name) + timed(fn))
        print("PERF %-20s %-20s median %9.2f ms  (min %.2f, max %.2f)  R=%d B=%d" % (rows[-1] + (R, B)), flush=True)

    record("hip", "LPIPS fwd+bwd", native)
    if not args.no_torch:
        dstate = {k: v.cuda() for k, v in state.items()}

        def restated():
            xi = x.clone().requires_grad_(True)
            LR.lpips(dstate, xi, t, torch.float32)[0].sum().backward()

        record("torch fp32 autograd", "LPIPS fwd+bwd", restated)
    if not args.lpips_only:
        from wmar_amd.models.tokenizer_train import TrainableTokenizer
        cfg = synth.TAMING_VQ
        assert cfg.resolution == R, "the step is timed at the tokenizer's resolution"
        vstate = {k: v.contiguous() for k, v in synth.synth_vq_state_fast(cfg, 0, "cuda").items()}
        tok = TrainableTokenizer(cfg, vstate, max_batch=B)
        orig = TrainableTokenizer(cfg, {k: (v.detach() + 0.01 * v.detach().std() * torch.randn_like(v)).contiguous() for k, v in vstate.items()}, max_batch=B)
        codes = torch.randint(0, cfg.n_embed, (B, cfg.codes_size ** 2), device="cuda", generator=g)
        params = list(tok.parameters())

        def step(rec):
            for p in params:
                p.grad = None
            ft.rcc_loss(tok, codes, [], loss_weight=1.0, orig=orig, rec_loss=rec)[0].backward()

        record("hip", "rcc step, L1", lambda: step(None))
        rec = ft.reference_rec_loss(lp, 1.0)
        record("hip", "rcc step, L1+LPIPS", lambda: step(rec))


if __name__ == "__main__":
    main()
