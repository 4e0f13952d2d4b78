"""MI355X: the fine-tuning step finetune.py runs -- ``rcc_loss``: decode -> transform -> re-encode on a taped tokenizer, a distinct
``frozen=True`` original decoder, the L1 (+ 0.5 x LPIPS) regulariser, ``idempotence_region``'s sub-grid, backward to every encoder and
decoder weight -- against the same ``rcc_loss`` on float64 stand-ins (tests/rcc_chain_reference.py), under every class of the
augmentation curriculum, on all three tokenizers, and again after a weight change at a smaller batch.

The three discrete decisions of the chain are taken from the device run and injected into the float64 run and into the fp32 budget
run alike: Rotate's index map (an index image through ``Rotate()`` under no_grad), JPEG's coded image (what ``device_ops.jpeg`` returned
inside the step) and GaussianNoise's draws (the device generator reseeded, ``randn_like`` redrawn).

Gates (none measured on the code under test):
  gradients      per tensor |got - g64|_inf <= 8 x |g32 - g64|_inf, g32 the fp32 CPU chain under the same decisions (GATE of
                 tests/test_gpu_vq_train.py / test_gpu_mvq_train.py, NET_GATE of tests/test_gpu_lpips.py), in absolute form so that the
                 conv biases in front of a GroupNorm, whose float64 gradient is analytically zero, get a bound too;
  intermediates  rec_x, rec_x_maybe_augmented, rec_z and the gradient that lands on rec_x: the same inequality;
  logged values  loss, rec_loss, idem_loss and the perceptual component: 1e-5 relative;
  JPEG           the coded image equals the host PIL path applied to the device's own clamped xrec, bit for bit;
  margins        in the float64 run every clamp of the chain and the sign of every L1 term stay 1e-5 or more from their edge, and the
                 device's rec_x and rec_x_orig_decoder lie within half the smallest margin of the reference's: no mask and no sign
                 differs, so nothing is excluded.  On MaskGIT the set of pixels at exactly +-1 equals the reference's.
The worst ratio of every case is printed on a line starting with RCCSTEP (run with -s).

Measured 2026-10-20 on one MI355X, worst ratio over the tensors and cases of a tokenizer (gate 8):
  Taming HARNESS_VQ            5.97 (GaussianNoise 0.1, decoder.conv_out.bias); the other 16 cases 2.30 - 4.07; second step 2.04
  HARNESS128 + narrow LPIPS    4.51 (none, decoder.up.2.block.1.conv2.bias)
  MaskGIT small                2.92 (JPEG 20, encoder.down.0.block.0.norm2.weight); second step 5.39 (decoder.conv_out.bias)
  CHAMELEON_SMALL_VQ           5.47 (GaussianBlur 9, decoder.up.4.block.1.norm1.weight)
Logged values within 4.3e-7 relative.  The device's rec_x lies 4.5e-6 (Taming) to 1.0e-5 (Chameleon small) from the reference's, the
smallest margins are 3.0e-5 and 2.9e-5 there."""
import functools
import random

import pytest
import torch

from tests import rcc_chain_reference as C

pytestmark = pytest.mark.gpu

GATE = 8.0
VALUE_GATE = 1e-5
TENSORS = ("rec_x", "rec_x_maybe_augmented", "rec_z", "rec_x_grad")


def _classes(name):
    from wmar_amd.models.tokenizer_train import MaskgitTrainableTokenizer, TrainableTokenizer
    return MaskgitTrainableTokenizer if name == "maskgit" else TrainableTokenizer


def _handles(name):
    """(taped tokenizer, frozen original on the perturbed weights, rec_loss or None) on the device, from the states the stand-ins get."""
    from wmar_amd import finetune as ft
    sd, orig = C.states(name, 1)
    cls = _classes(name)
    tok = cls(C.config(name), {k: v.clone().cuda().contiguous() for k, v in sd.items()}, max_batch=2)
    frozen = cls(C.config(name), {k: v.clone().cuda().contiguous() for k, v in orig.items()}, max_batch=2, frozen=True)
    rec = None
    if name == "lpips":
        from wmar_amd.lpips import LPIPS
        rec = ft.reference_rec_loss(LPIPS(C.lpips_state(), resolution=128, max_batch=2, chns=C.NARROW), C.PERCEPTUAL_WEIGHT)
    return tok, frozen, rec


_device = functools.lru_cache(maxsize=None)(_handles)


class _jpeg_spy:
    """Records every call of ``device_ops.jpeg`` (input, quality, passthrough, result) while the step runs."""

    def __enter__(self):
        from wmar_amd.augmentations import device_ops as D
        self.calls, self._D, self._jpeg = [], D, D.jpeg

        def spy(image, quality, pm1=False, passthrough=True):
            out = self._jpeg(image, quality, pm1=pm1, passthrough=passthrough)
            self.calls.append((image.detach().clone(), quality, pm1, passthrough, out.detach().clone()))
            return out
        D.jpeg = spy
        return self

    def __exit__(self, *exc):
        self._D.jpeg = self._jpeg
        return False


def _device_step(name, handles, aug, step=1):
    """One step on the device, and the decisions it took."""
    from wmar_amd.augmentations.geometric import Rotate
    from wmar_amd.augmentations.valuemetric import JPEG, GaussianNoise, jpeg_compress
    tok, frozen, rec = handles
    a = C.resolve(aug)
    idx = C.codes(name, step).cuda()
    with _jpeg_spy() as spy:
        got = C.run(tok, frozen, idx, a, None, rec)
    assert frozen.frozen and frozen is not tok and frozen.state is not tok.state
    decisions = {}
    R = C.config(name).resolution
    if a is not None and a[0] is Rotate:
        with torch.no_grad():
            decisions["rotate_map"] = Rotate()(C.index_image(R).cuda(), a[1]).cpu().round().long().view(R, R)
        assert int(decisions["rotate_map"].min()) >= 0 and int(decisions["rotate_map"].max()) <= R * R
    if a is not None and a[0] is JPEG:
        assert len(spy.calls) == 1, "the step codes its image once"
        image, quality, pm1, passthrough, coded = spy.calls[0]
        assert quality == a[1] and not pm1 and not passthrough
        assert torch.equal(image, (0.5 * got["rec_x"] + 0.5).clamp(0, 1)), "the coded image is the step's own clamped xrec"
        host = torch.stack([jpeg_compress(one, quality) for one in image.cpu()])
        assert torch.equal(coded.cpu(), host), "device JPEG differs from the host PIL path on the device's own xrec"
        decisions["jpeg_coded"] = coded.cpu()
    else:
        assert not spy.calls
    if a is not None and a[0] is GaussianNoise:
        torch.manual_seed(C.NOISE_SEED)
        decisions["noise"] = torch.randn_like(got["rec_x"]).cpu()
    return got, decisions


_DECISIONS = {}


@functools.lru_cache(maxsize=None)
def _references(name, aug, step):
    """The float64 chain and the fp32 budget chain under the decisions of this case's device run."""
    d = _DECISIONS[(name, aug, step)]
    return C.reference(name, aug, torch.float64, d, step), C.reference(name, aug, torch.float32, d, step)


def _inf(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _check(name, aug, step, got, decisions):
    _DECISIONS[(name, aug, step)] = decisions
    r64, r32 = _references(name, aug, step)
    case = "%s %s step=%d" % (name, C.case_id(aug), step)
    m = r64["margins"]
    half = 0.5 * min(m["clamp"], m["l1"])
    e_x, e_o = _inf(got["rec_x"], r64["rec_x"]), _inf(got["rec_x_orig_decoder"], r64["rec_x_orig_decoder"])
    print("RCCSTEP %s margins clamp=%.3g l1=%.3g u=%.3g saturated=%.3f rec_x_err=%.3g rec_x_orig_err=%.3g" % (
        case, m["clamp"], m["l1"], m["u"], m["saturated"], e_x, e_o), flush=True)
    assert m["clamp"] >= C.MARGIN and m["l1"] >= C.MARGIN, "the inputs of %s do not keep the margins: %s" % (case, m)
    assert e_x <= half and e_o <= half, "%s: rec_x off by %.3g / %.3g, half the smallest margin is %.3g" % (case, e_x, e_o, half)
    if name == "maskgit":
        sat, want = got["rec_x"].cpu().abs() == 1.0, r64["rec_x"].abs() == 1.0
        assert torch.equal(sat, want), "%s: %d pixels are saturated on one side only" % (case, int((sat != want).sum()))
        assert 0.3 <= float(sat.double().mean()) <= 0.7
    logged = ["loss", "rec_loss", "idem_loss"] + (["rec_loss_perceptual_component"] if name == "lpips" else [])
    assert set(logged) <= set(got["log"]) and got["log"]["loss_weight"] == C.LOSS_WEIGHT
    assert ("rec_loss_perceptual_component" in got["log"]) == (name == "lpips")
    bad_values = []
    for k in logged:
        rel = abs(got["log"][k] - r64["log"][k]) / abs(r64["log"][k])
        print("RCCSTEP %s %s=%.9g ref=%.9g rel=%.3g" % (case, k, got["log"][k], r64["log"][k], rel), flush=True)
        if not rel <= VALUE_GATE:
            bad_values.append((k, rel))
    assert set(got["grads"]) == set(r64["grads"]) == set(r32["grads"])
    rows = [(k, got[k], r64[k], r32[k]) for k in TENSORS] + [(k, g, r64["grads"][k], r32["grads"][k]) for k, g in got["grads"].items()]
    bad, worst = [], (0.0, "")
    for k, a, e64, e32 in rows:
        assert torch.isfinite(a).all(), k
        e, b = _inf(a, e64), _inf(e32, e64)
        assert b > 0, k
        worst = max(worst, (e / b, k))
        if not e <= GATE * b:
            bad.append((k, e, b, e / b))
    print("RCCSTEP %s worst_ratio=%.3g at %s" % (case, worst[0], worst[1]), flush=True)
    assert not bad_values, "%s: logged values beyond %g relative: %s" % (case, VALUE_GATE, bad_values)
    assert not bad, "%s: beyond %g x the fp32 chain: %s" % (case, GATE, bad)
    return r64


FIRST_STEPS = [(n, a) for n, a, s in C.cases() if s == 1]


@pytest.mark.parametrize("name,aug", FIRST_STEPS, ids=["%s-%s" % (n, C.case_id(a)) for n, a in FIRST_STEPS])
def test_step_against_the_float64_chain(name, aug):
    """a (Taming HARNESS_VQ, every class at its first weak and last strong parameter), b (HARNESS128 + narrow LPIPS at weight 0.5),
    c (MaskGIT small) and d (CHAMELEON_SMALL_VQ): B = 2, max_batch = 2, p = 1, loss_weight = 2."""
    from wmar_amd import finetune as ft
    got, decisions = _device_step(name, _device(name), aug)
    R, S = C.config(name).resolution, C.config(name).codes_size
    if aug is not None and aug[0] == "Rotate":
        assert ft.idempotence_region(S, C.resolve(aug)) == C.ROTATE_REGION[name]
        same = torch.equal(decisions["rotate_map"], C.identity_map(R))
        if abs(aug[1]) == 1:      # no pixel of 32 moves by half a pixel: the case differs from "none" by the region alone
            assert R == 32 and same, "Rotate %d moved a pixel at 32 x 32" % aug[1]
            assert torch.equal(got["rec_x_maybe_augmented"], 2.0 * (0.5 * got["rec_x"] + 0.5) - 1.0)
        else:
            assert not same and int((decisions["rotate_map"] == 0).sum()) > 0
    _check(name, aug, 1, got, decisions)


@pytest.mark.parametrize("name", C.SECOND_STEP)
def test_second_step_after_a_weight_change_at_a_smaller_batch(name):
    """e: Rotate 3 at B = 2 with its backward, then the same seeded change added in place to every weight (the device side must repack),
    then UpperLeftCropWithPadBack 0.5 at B = 1 on the same handles."""
    handles = _handles(name)
    tok = handles[0]
    first, _ = _device_step(name, handles, C.FIRST, 1)
    assert set(k for k, _ in tok.named_parameters()) == set(C.step_delta(name))
    with torch.no_grad():
        for k, p in tok.named_parameters():
            p.add_(C.step_delta(name)[k].cuda())
    for k, v in C.states(name, 2)[0].items():
        assert torch.equal(tok.state[k].detach().cpu(), v), k
    got, decisions = _device_step(name, handles, C.SECOND, 2)
    assert got["rec_x"].shape[0] == 1 and not decisions
    assert not torch.equal(got["rec_x"], first["rec_x"][:1]), "the weight change did not reach the device"
    r64 = _check(name, C.SECOND, 2, got, decisions)
    S = C.config(name).codes_size
    assert r64["rec_z"].shape[-1] == S and int(S * 0.5) == S // 2


def test_device_path_consumes_pythons_random_as_the_cpu_path_does(monkeypatch):
    """f: twenty ``rcc_loss`` calls at p = 0.5 over the whole weak table after one ``random.seed(0)``: the device handles and the CPU
    stand-in see the same (was_augmented, class, parameter) sequence."""
    from wmar_amd import finetune as ft
    from wmar_amd.augmentations import finetune_schedule
    weak = finetune_schedule("all+geom", "0,1,0,0", 1)[0]
    assert {cls for cls, _ in weak} == set(C.CLASSES.values())
    seen = []
    shipped = ft.apply_random_augmentation

    def recording(x, augmentations, p=0.5):
        out, applied = shipped(x, augmentations, p=p)
        seen.append(applied)
        return out, applied

    monkeypatch.setattr(ft, "apply_random_augmentation", recording)
    tok_cpu, orig_cpu, _ = C.standins("taming", torch.float32)
    tok, frozen, _ = _device("taming")
    sequences = []
    for t, o, idx in ((tok_cpu, orig_cpu, C.codes("taming")), (tok, frozen, C.codes("taming").cuda())):
        seen.clear()
        flags = []
        random.seed(0)
        torch.manual_seed(C.NOISE_SEED)
        for _ in range(20):
            _, _, _, was = ft.rcc_loss(t, idx, weak, p=0.5, loss_weight=C.LOSS_WEIGHT, orig=o)
            flags.append(was)
        assert len(seen) == 20
        sequences.append((list(zip(flags, seen)), random.random()))
    (cpu, cpu_next), (dev, dev_next) = sequences
    print("RCCSTEP draw order: %s" % [(w, a and (a[0].__name__, a[1])) for w, a in dev], flush=True)
    assert cpu == dev and cpu_next == dev_next
    assert 5 <= sum(w for w, _ in dev) <= 15 and len({a[0] for _, a in dev if a}) >= 3
