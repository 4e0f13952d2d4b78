"""CPU: the fine-tuning step's reference (tests/rcc_chain_reference.py) before tests/test_gpu_rcc_chain.py relies on it.

  * with the three discrete decisions taken from the CPU modules themselves, the injected chain IS plain ``rcc_loss`` on the same
    stand-ins: loss, logged values, intermediates and every weight gradient are bit-equal, in float64 and in fp32, for all six classes
    of the curriculum, and the patched forwards are gone afterwards;
  * for the committed seeds of every case of the GPU test, the float64 run keeps every clamp margin and the L1 sign margin at 1e-5 or
    more (the noise case here with the CPU generator's draws; the GPU test asserts it again for the device's), the cases cover what
    they are there for (pixels outside [-1, 1] on Taming, saturated pixels on MaskGIT, a sub-grid for Rotate and the crop), and the
    fp32 budget |g32 - g64|_inf is finite and non-zero for every tensor the GPU test gates."""
import functools

import pytest
import torch

from tests import rcc_chain_reference as C
from wmar_amd import finetune as ft
from wmar_amd.augmentations.geometric import Rotate
from wmar_amd.augmentations.valuemetric import JPEG, GaussianNoise

SIX = [("JPEG", 20), ("GaussianBlur", 9), ("GaussianNoise", 0.1), ("Brightness", 1.3), ("Rotate", 3), ("Rotate", -3),
       ("UpperLeftCropWithPadBack", 0.5)]
TENSORS = ("rec_x", "rec_x_maybe_augmented", "rec_z", "rec_x_grad")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["taming", "maskgit"])
@pytest.mark.parametrize("aug", SIX, ids=[C.case_id(a) for a in SIX])
def test_injected_chain_is_plain_rcc_loss_bit_for_bit(aug, name, dtype):
    shipped = {cls: cls.__dict__["forward"] for cls in (Rotate, JPEG, GaussianNoise)}
    tok, orig, rec = C.standins(name, dtype)
    idx, a = C.codes(name), C.resolve(aug)
    plain = C.run(tok, orig, idx, a, None, rec)
    decisions = C.cpu_decisions(tok, idx, a, dtype)
    assert bool(decisions) == (a[0] in shipped)
    again = C.run(tok, orig, idx, a, decisions, rec)
    assert all(cls.__dict__["forward"] is fn for cls, fn in shipped.items()), "a patched forward outlived the reference run"
    assert torch.equal(plain["loss"], again["loss"]) and plain["log"] == again["log"]
    for k in TENSORS:
        assert torch.equal(plain[k], again[k]), k
    assert set(plain["grads"]) == set(again["grads"])
    # quarter turns: rot90's backward hands a strided gradient on, and torch's CPU reductions sum a strided tensor in another order than
    # a contiguous one.  There the weight gradients are the same sums of the same bits (rec_x_grad above) up to that order.
    slack = 0.0 if not (a[0] is Rotate and a[1] < 0) else 2.0 ** (-40 if dtype == torch.float64 else -14)
    for k, g in plain["grads"].items():
        assert float((g - again["grads"][k]).abs().max()) <= slack * float(g.abs().max()), k
    if a[0] is Rotate:          # the decision is really taken from the map: another map, another loss
        other = C.run(tok, orig, idx, a, {"rotate_map": C.identity_map(tok.cfg.resolution)}, rec)
        assert not torch.equal(other["rec_x_maybe_augmented"], plain["rec_x_maybe_augmented"])
        assert torch.equal(other["rec_x_maybe_augmented"], 2.0 * (0.5 * plain["rec_x"] + 0.5) - 1.0)


def test_gather_follows_the_map_and_fills_with_zero():
    img = torch.arange(1.0, 13.0, dtype=torch.float64).view(1, 1, 3, 4).requires_grad_(True)
    imap = torch.tensor([[0, 1, 1, 12], [5, 0, 7, 8], [9, 10, 2, 0]])
    out = C.gather(img, imap)
    assert out.tolist() == [[[[0, 1, 1, 12], [5, 0, 7, 8], [9, 10, 2, 0]]]]
    out.sum().backward()
    assert img.grad.view(-1).tolist() == [2, 1, 0, 0, 1, 0, 1, 1, 1, 1, 0, 1]
    assert torch.equal(C.gather(img.detach(), C.identity_map(4)[:3]), img.detach())


@functools.lru_cache(maxsize=None)
def _pair(name, aug, step):
    tok, _, _ = C.standins(name, torch.float64, step)
    decisions = C.cpu_decisions(tok, C.codes(name, step), C.resolve(aug), torch.float64)
    return C.reference(name, aug, torch.float64, decisions, step), C.reference(name, aug, torch.float32, decisions, step)


@pytest.mark.parametrize("name,aug,step", C.cases(), ids=["%s-%s-step%d" % (n, C.case_id(a), s) for n, a, s in C.cases()])
def test_committed_seeds_meet_the_margins_and_the_fp32_budget_is_usable(name, aug, step):
    r64, r32 = _pair(name, aug, step)
    m = r64["margins"]
    assert m["clamp"] >= C.MARGIN and m["l1"] >= C.MARGIN, m
    x = r64["rec_x"]
    if name == "maskgit":
        assert 0.3 <= m["saturated"] <= 0.7 and float(x.min()) == -1.0 and float(x.max()) == 1.0
    else:
        assert m["saturated"] == 0.0
    if name == "taming":
        assert float((x.abs() > 1).double().mean()) >= 0.05, "the transform clamps must really block"
    S = r64["rec_z"].shape[-1]
    r = ft.idempotence_region(S, C.resolve(aug))
    if aug is not None and aug[0] == "Rotate":
        assert r == C.ROTATE_REGION[name] and r != slice(0, S)
    if aug is not None and aug[0] == "UpperLeftCropWithPadBack":
        assert 0 < r.stop < S
    assert r64["log"]["rec_loss"] > 0 and ("rec_loss_perceptual_component" in r64["log"]) == (name == "lpips")
    pairs = [(k, r32[k], r64[k]) for k in TENSORS] + [(k, r32["grads"][k], g) for k, g in r64["grads"].items()]
    assert len(pairs) > len(TENSORS)
    for k, a32, a64 in pairs:
        b = float((a32.double() - a64).abs().max())
        assert torch.isfinite(a32).all() and torch.isfinite(a64).all() and 0.0 < b < float("inf"), (k, b)
        if float(a64.abs().max()) > 1e-9:      # a tensor that is not analytically zero: fp32 stays a small fraction of it
            assert b <= 1e-3 * float(a64.abs().max()), (k, b)
