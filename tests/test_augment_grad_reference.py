"""CPU checks of what training through the transforms rests on: the reference gradients of tests/augment_grad_reference.py against
dense Jacobians, the two fine-tuning helpers (wmar/utils/utils.py:25-44, finetune.py:323-359), and the argument checks of
wmar_augment_backward, which run before the library touches a device."""
import random

import pytest
import torch

from tests import augment_grad_reference as R

H, W = 7, 9


def _jacobian(op, p0, p1, noise, index_map):
    """dense Jacobian of T: column i = T(e_i) - T(0) (every T is affine)"""
    zero = torch.zeros(1, 1, H, W, dtype=torch.float64)
    t0 = R.transform(op, zero, p0, p1, noise, index_map).view(-1)
    cols = []
    for i in range(H * W):
        e = zero.clone().view(-1)
        e[i] = 1.0
        cols.append(R.transform(op, e.view(1, 1, H, W), p0, p1, noise, index_map).view(-1) - t0)
    return torch.stack(cols, dim=1)            # [outputs, inputs]


CASES = [(R.IDENTITY, 0, 0), (R.BLUR, 3, 0), (R.BLUR, 9, 0), (R.NOISE, 0.2, 0), (R.BRIGHTNESS, 2.0, 0), (R.FLIP_H, 0, 0),
         (R.CROP_RESIZE, 4, 6), (R.CROP_RESIZE, 6, 8), (R.CROP_PAD, 4, 6), (R.ROTATE, 0, 20), (R.ROTATE, 2, 0), (R.ROTATE, 2, 70)]


@pytest.mark.parametrize("pm1", [False, True])
@pytest.mark.parametrize("op,p0,p1", CASES)
def test_reference_gradient_is_the_transposed_jacobian(op, p0, p1, pm1):
    gen = torch.Generator().manual_seed(op * 10 + int(pm1))
    span = 4.0 if op == R.BLUR else 1.6                                              # blurred pixels leave [0, 1] too
    u = torch.rand(1, 1, H, W, generator=gen, dtype=torch.float64) * span - (span - 1.0) / 2
    g = torch.rand(1, 1, H, W, generator=gen, dtype=torch.float64) * 2 - 1
    noise = torch.randn(1, 1, H, W, generator=gen, dtype=torch.float64) if op == R.NOISE else None
    imap = R.torch_index_map(H, W, p0, p1) if op == R.ROTATE else None
    x = u * 2.0 - 1.0 if pm1 else u
    ref = R.reference(op, x, g, p0, p1, noise, pm1, imap)
    J = _jacobian(op, p0, p1, noise, imap)
    t = R.transform(op, x / 2.0 + 0.5 if pm1 else x, p0, p1, noise, imap)
    assert torch.equal(t, ref.t)
    mask = ((t >= 0) & (t <= 1)).double() if (pm1 or op in R.CLAMPING) else torch.ones_like(t)
    want = J.t() @ ((2.0 if pm1 else 1.0) * g * mask).view(-1) * (0.5 if pm1 else 1.0)
    assert torch.allclose(ref.grad.view(-1), want, rtol=0, atol=1e-14), float((ref.grad.view(-1) - want).abs().max())
    if pm1 or op in R.CLAMPING:
        assert 0 < int(mask.sum()) < mask.numel()                                   # the mask blocks some pixels and passes others
    A = ref.adjoint_abs(ref.gm).view(-1)
    assert torch.allclose(A, J.abs().t() @ (g * mask).abs().view(-1), rtol=0, atol=1e-14)


def test_clamp_passes_the_gradient_at_both_bounds():
    x = torch.tensor([[[[0.0, 0.5, 1.0]]]], dtype=torch.float64)
    ref = R.reference(R.BRIGHTNESS, x, torch.ones_like(x), 2.0)
    assert ref.t.view(-1).tolist() == [0.0, 1.0, 2.0] and ref.grad.view(-1).tolist() == [2.0, 2.0, 0.0]


def test_rotation_reference_scatters_through_the_index_map():
    imap = R.torch_index_map(H, W, 0, 20)
    reads = torch.bincount(imap.view(-1), minlength=H * W + 1)[1:]
    assert int(reads.max()) <= 2 and int((reads == 0).sum()) > 0
    g = torch.rand(1, 1, H, W, dtype=torch.float64)
    ref = R.reference(R.ROTATE, torch.rand(1, 1, H, W, dtype=torch.float64), g, 0, 20, index_map=imap)
    want = torch.zeros(H * W + 1, dtype=torch.float64).index_add_(0, imap.view(-1), g.view(-1))[1:]
    assert torch.equal(ref.grad.view(-1), want)


# ------------------------------------------------------------------------------------------------------------------ the two helpers
def _weak():
    from wmar_amd.augmentations import finetune_schedule
    return finetune_schedule("all+geom", "0,1,0,0", 1)[0]


class _Recorder(torch.nn.Module):
    calls = []

    def forward(self, image, param):
        type(self).calls.append((image, param))
        return image * 0.5


class _Other(_Recorder):
    pass


def test_apply_random_augmentation_replays_the_reference_draw_order():
    from wmar_amd.augmentations.geometric import Identity
    from wmar_amd.utils.utils import apply_random_augmentation
    table = [(_Recorder, [1, 2, 3]), (Identity, [0]), (_Other, [4, 5, 6, 7])]
    x = torch.rand(2, 3, 8, 8) * 2 - 1
    for seed in range(5):
        for p in (0.5, 1.0):
            random.seed(seed)
            x_t, info = apply_random_augmentation(x, table, p)
            random.seed(seed)                                           # the documented order: random(), choice(augs), choice(params)
            if random.random() < p:
                cls, params = random.choice(table)
                want = None if cls is Identity else (cls, random.choice(params))
            else:
                want = None
            assert info == want, (seed, p)
            if want is None:
                assert x_t is x
            else:
                image, param = _Recorder.calls[-1]
                assert param == want[1] and torch.equal(image, x / 2.0 + 0.5) and torch.equal(x_t, (image * 0.5) * 2.0 - 1.0)
            after = random.random()
            random.seed(seed)
            apply_random_augmentation(x, table, p)
            assert random.random() == after                             # no draw beyond those three
    assert apply_random_augmentation(x, [], 1.0) == (x, None)
    out, info = apply_random_augmentation(x, [(Identity, [0])], 1.0)
    assert out is x and info is None


def test_jpeg_is_straight_through(monkeypatch):
    from wmar_amd.augmentations import valuemetric
    from wmar_amd.utils.utils import apply_random_augmentation

    class StubJPEG(torch.nn.Module):                                    # a codec with a gradient of its own, which must not be used
        def forward(self, image, quality):
            return (image * 255).round() / 255 * 0.25

    monkeypatch.setattr(valuemetric, "JPEG", StubJPEG)
    x = (torch.rand(1, 3, 8, 8) * 2 - 1).requires_grad_(True)
    x_t, info = apply_random_augmentation(x, [(StubJPEG, [50])], 1.0)
    assert info == (StubJPEG, 50)
    assert torch.equal(x_t.detach(), x.detach() + (((x.detach() / 2.0 + 0.5) * 255).round() / 255 * 0.25 * 2.0 - 1.0 - x.detach()))
    g = torch.rand(1, 3, 8, 8)
    x_t.backward(g)
    assert torch.equal(x.grad, g)                                       # exactly 1


def test_finetune_schedule_tables_lengths_and_assertion():
    from wmar_amd.augmentations import finetune_schedule
    from wmar_amd.augmentations.geometric import Rotate, UpperLeftCropWithPadBack
    from wmar_amd.augmentations.valuemetric import JPEG, Brightness, GaussianBlur, GaussianNoise
    none = finetune_schedule("none", "1,2,3,4", 7)
    assert sorted(none) == list(range(7)) and all(v == [] for v in none.values())
    sched = finetune_schedule("all+geom", "1,2,3,4", 10)
    assert sorted(sched) == list(range(10)) and sched == finetune_schedule("all+geom", [1, 2, 3, 4], 10)
    assert sched[0] == []
    order = [JPEG, GaussianBlur, GaussianNoise, Brightness, Rotate, UpperLeftCropWithPadBack]
    for epochs in ((1, 2), (3, 4, 5), (6, 7, 8, 9)):
        assert all(sched[e] is sched[epochs[0]] for e in epochs) and [c for c, _ in sched[epochs[0]]] == order
    assert dict(sched[1]) == {JPEG: [90, 80, 70], GaussianBlur: [1, 3], GaussianNoise: [0.005, 0.01, 0.015, 0.02],
                              Brightness: [1.0, 1.1, 1.2], Rotate: [-1, 1], UpperLeftCropWithPadBack: [0.8, 0.9]}
    assert dict(sched[3]) == {JPEG: [80, 60, 40], GaussianBlur: [3, 5], GaussianNoise: [0.02, 0.04, 0.06], Brightness: [1.2, 1.3, 1.4],
                              Rotate: [-3, -2, -1, 1, 2, 3], UpperLeftCropWithPadBack: [0.5, 0.6, 0.7, 0.8, 0.9]}
    assert dict(sched[9]) == {JPEG: [40, 30, 20], GaussianBlur: [5, 7, 9], GaussianNoise: [0.06, 0.08, 0.1], Brightness: [1.4, 1.7, 2.0],
                              Rotate: [-3, -2, -1, 1, 2, 3], UpperLeftCropWithPadBack: [0.5, 0.6, 0.7, 0.8, 0.9]}
    with pytest.raises(AssertionError, match="covers 10 epochs, the run has 11"):
        finetune_schedule("all+geom", "1,2,3,4", 11)
    with pytest.raises(ValueError):
        finetune_schedule("all", "1,2,3,4", 10)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_backward_entry_point_checks_its_arguments_before_any_launch():
    """no device here: a call that got as far as a launch would return the HIP status, not WMAR_EINVAL"""
    from wmar_amd import _lib
    L = _lib.load()
    a, b, c, n, ws = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000            # never dereferenced on the host

    def call(op, x=a, g=b, gin=c, noise=None, work=None, B=2, C=3, Hh=8, Ww=8, pm1=0, p0=0.0, p1=0.0):
        rc = L.wmar_augment_backward(op, x, g, gin, noise, work, B, C, Hh, Ww, pm1, p0, p1, None)
        return rc, L.wmar_last_error().decode()

    for kw in (dict(x=None), dict(g=None), dict(gin=None), dict(B=0), dict(C=0), dict(Hh=0), dict(Ww=0)):
        rc, msg = call(0, **kw)
        assert rc == -1 and "bad argument" in msg, kw
    for op in (-1, 8, 99):
        rc, msg = call(op)
        assert rc == -1 and "unknown transform" in msg, op
    assert call(1, p0=3.0)[1].endswith("floats") and call(1, p0=3.0)[0] == -1                  # blur without a workspace
    assert call(1, p0=4.0, work=ws) == (-1, "augment_backward: blur kernel size 4 (odd, 1..63)")
    assert call(1, p0=19.0, work=ws)[0] == -1 and "does not fit" in call(1, p0=19.0, work=ws)[1]
    assert call(1, p0=3.0, work=c)[0] == -1 and "overlaps" in call(1, p0=3.0, work=c)[1]
    assert call(2, p0=0.1)[0] == -1 and "normal draws" in call(2, p0=0.1)[1]
    assert call(4, Hh=8, Ww=12, p0=1.0)[0] == -1 and "square" in call(4, Hh=8, Ww=12, p0=1.0)[1]
    for op in (6, 7):
        assert call(op, p0=9.0, p1=4.0)[0] == -1 and "crop 9 x 4" in call(op, p0=9.0, p1=4.0)[1]
    for op in (1, 4, 5, 6):                                             # the gathering transforms cannot write over their own input
        rc, msg = call(op, gin=b, work=ws, p0=3.0, p1=3.0)
        assert rc == -1 and "in place" in msg, op
