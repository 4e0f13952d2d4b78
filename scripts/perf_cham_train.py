"""Measures tokenizer training at Chameleon's VQGAN layout and the validation pass on one MI355X (synthetic weights):

  * at CHAMELEON_VQ (512 x 512), per batch size: device_bytes of the taped and of the forward-only ("frozen") engine handle, the time
    of one rcc_loss step (forward + backward, no regulariser) and of the same restated network under PyTorch-ROCm fp32 autograd on the
    same GPU.  A batch whose engines or whose torch graph do not fit is reported as such and the next one is tried;
  * at TAMING_VQ, B = 4: one validation pass over one batch with the weak-stage curriculum (wmar_amd.finetune.validate: 1 + the
    stage's (transform, parameter) pairs forwards) against one training step with the frozen original decoder.

Events around each call, 1 warm-up run, median of 3.  Lines start with PERF.

    python scripts/perf_cham_train.py [--batches 1,8] [--no-torch] [--skip-validation]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup=1, reps=3):
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


def clear(params):
    for p in params:
        p.grad = None


def chameleon(B, with_torch):
    from tests import vq_grad_reference as G
    from wmar_amd import _lib
    from wmar_amd import finetune as ft
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = synth.CHAMELEON_VQ
    S = cfg.codes_size
    torch.cuda.reset_peak_memory_stats()
    state = {k: v.contiguous() for k, v in synth.synth_vq_state_fast(cfg, 0, "cuda").items()}
    codes = torch.randint(0, cfg.n_embed, (B, S * S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    try:
        frozen = TrainableTokenizer(cfg, {k: v.detach().clone() for k, v in state.items()}, max_batch=B, frozen=True)
        tok = TrainableTokenizer(cfg, state, max_batch=B)
    except _lib.WmarError as e:
        print("PERF chameleon B=%d engines do not fit: %s" % (B, e), flush=True)
        return False
    gb = 2 ** 30
    print("PERF chameleon B=%d device_bytes taped %d (%.2f GB)  frozen %d (%.2f GB)  ratio %.1f" % (
        B, tok._train.device_bytes, tok._train.device_bytes / gb, frozen.device_bytes, frozen.device_bytes / gb,
        tok._train.device_bytes / frozen.device_bytes), flush=True)
    params = list(tok.parameters())

    def step(t, prm, orig):
        clear(prm)
        ft.rcc_loss(t, codes, [], loss_weight=1.0, orig=orig)[0].backward()

    print("PERF chameleon B=%d hip rcc_loss step (no regulariser)      median %9.2f ms (min %.2f, max %.2f)" % ((B,) + timed(lambda: step(tok, params, None))),
          flush=True)
    print("PERF chameleon B=%d hip rcc_loss step (frozen orig decoder) median %9.2f ms (min %.2f, max %.2f)" % ((B,) + timed(lambda: step(tok, params, frozen))),
          flush=True)
    with torch.no_grad():
        print("PERF chameleon B=%d hip frozen decode + encode              median %9.2f ms (min %.2f, max %.2f)" % (
            (B,) + timed(lambda: frozen.encode_prequant(frozen.decode(frozen.embed(codes))))), flush=True)
    print("PERF chameleon B=%d torch.cuda.max_memory_allocated %.2f GB (tensors of the loss tail, outside the engines)" % (
        B, torch.cuda.max_memory_allocated() / gb), flush=True)
    del tok, frozen
    if with_torch:
        ref = G.TorchTokenizer(cfg, {k: v.detach().cpu() for k, v in state.items()})
        ref.state = {k: v.detach().cuda().requires_grad_(not k.startswith("quantize.")) for k, v in ref.state.items()}
        rparams = list(ref.parameters())
        try:
            torch.cuda.reset_peak_memory_stats()
            print("PERF chameleon B=%d torch fp32 autograd rcc_loss step      median %9.2f ms (min %.2f, max %.2f)" % (
                (B,) + timed(lambda: step(ref, rparams, None))), flush=True)
            print("PERF chameleon B=%d torch fp32 autograd peak memory %.2f GB" % (B, torch.cuda.max_memory_allocated() / gb), flush=True)
        except torch.OutOfMemoryError as e:
            print("PERF chameleon B=%d torch fp32 autograd does not fit: %s" % (B, str(e).splitlines()[0]), flush=True)
        del ref, rparams
        torch.cuda.empty_cache()
    return True


def validation(B=4):
    from wmar_amd import finetune as ft
    from wmar_amd.augmentations import finetune_schedule
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = synth.TAMING_VQ
    S = cfg.codes_size
    state = {k: v.contiguous() for k, v in synth.synth_vq_state_fast(cfg, 0, "cuda").items()}
    orig = TrainableTokenizer(cfg, {k: v.detach().clone() for k, v in state.items()}, max_batch=B, frozen=True)
    tok = TrainableTokenizer(cfg, state, max_batch=B)
    codes = torch.randint(0, cfg.n_embed, (B, S * S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    entries = finetune_schedule("all+geom", "0,1", 1)[0]           # the weak stage: 16 (transform, parameter) pairs
    n = 1 + sum(len(p) for _, p in entries)
    params = list(tok.parameters())

    def step():
        clear(params)
        ft.rcc_loss(tok, codes, [], loss_weight=1.0, orig=orig)[0].backward()

    t_step = timed(step)
    t_val = timed(lambda: ft.validate(tok, orig, codes, entries, B, 1.0))
    print("PERF taming B=%d training step (rcc_loss + backward, frozen orig)  median %9.2f ms (min %.2f, max %.2f)" % ((B,) + t_step), flush=True)
    print("PERF taming B=%d validation pass, weak stage: %d records, 1 batch  median %9.2f ms (min %.2f, max %.2f)  = %.1f training steps" % (
        (B, n) + t_val + (t_val[0] / t_step[0],)), flush=True)
    print("PERF taming B=%d device_bytes taped %d  no-grad (frozen) %d  orig (frozen) %d" % (
        B, tok._train.device_bytes, tok._eval.device_bytes, orig.device_bytes), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,4,2", help="batch sizes at CHAMELEON_VQ, in the order tried; after B = 1 the first that fits ends the list")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--skip-validation", action="store_true")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",") if b]
    for i, B in enumerate(batches):
        ok = chameleon(B, not args.no_torch)
        torch.cuda.empty_cache()
        if ok and B != 1:
            break
    if not args.skip_validation:
        validation()


if __name__ == "__main__":
    main()
