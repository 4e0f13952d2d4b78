"""Training through the device transforms on the MI355X: wmar_augment_backward (wmar_amd/csrc/augment.hip) reached through autograd
from device_ops.run / fused and the transform modules, against the float64 reference gradients of tests/augment_grad_reference.py.

  * identity, flip, crop + pad, brightness, noise and every rotation are BIT-EQUAL to the fp32 reference (a rotated pixel has at most
    two addends, asserted from the kernel's own index map first);
  * blur and crop + resize stay within |got - ref64| <= c 2^-24 A per pixel, A the float64 adjoint applied to |g mask|.  The smallest c
    at which torch's own fp32 autograd through the restatements, run on the device, meets the float64 reference at these shapes was
    measured as C_TORCH = 4.872 (blur) and 217.896 (crop + resize) -- printed again by every run; the kernels, which measured 4.050
    and 217.896, are allowed twice that, which covers another summation order.
    g is zeroed at output pixels whose float64 t lies within 1e-5 of a clamp bound (fp32 and fp64 may clip differently there): at
    most 1 % of the pixels;
  * the graph: requires_grad, .grad on the device, no graph and today's bits under no_grad; two runs give the same bits; 3-D and
    non-contiguous inputs; apply_random_augmentation end to end; fused() equals the unfused module sequence bit for bit.

Shapes are the smallest at which the kernels can go wrong: planes 2 x 3; blur 21 x 19 (k = 3, 9: ragged 16 x 16 tiles), 5 x 5 with
k = 9 (both reflections of one source), 40 x 40 with k = 19 (halo larger than the tile); rotation 17 x 17 and 12 x 20."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import augment_grad_reference as R  # noqa: E402
from wmar_amd.augmentations import device_ops as D  # noqa: E402

# smallest c for torch's fp32 autograd on the device (MI355X, these shapes, the two input sets of the issue; the extra "wide" blur
# inputs are held to the same bound and do not enter it).  The kernels measured 4.050 and 217.896.  The resize figure is large for both
# because both compute the triangle weights in fp32 from `j - scale * (i + 0.5) + 0.5`, which cancels up to 31 pixels of coordinate.
# Every run measures torch again and checks it against the recorded figure, so that a change of torch's own error cannot silently
# change what the bound means.
C_TORCH = {"blur": 4.872, "resize": 217.896}

BC = (2, 3)


def _inputs(H, W, seed, exact=False):
    """u in [0, 1] terms: uniform in [-0.3, 1.3], unclamped, so the mask really blocks -- or (exact) uniform in [-0.02, 1.02] clamped
    to [0, 1], which plants exact 0.0 and 1.0 pixels -- or (exact == "wide") uniform in [-1.9, 2.9]: a blurred pixel is an average
    and leaves [0, 1] only from such inputs; g uniform in [-1, 1]"""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(*BC, H, W, generator=gen)
    u = u * 4.8 - 1.9 if exact == "wide" else (u * 1.04 - 0.02).clamp(0, 1) if exact else u * 1.6 - 0.3
    g = torch.rand(*BC, H, W, generator=gen) * 2 - 1
    return u, g


def _x(u, pm1):
    return u * 2.0 - 1.0 if pm1 else u          # exact 0.0 / 1.0 stay exact: -1 / 1 map back to 0 / 1 in the kernel


def _device_grad(op, x, g, p0=0.0, p1=0.0, noise=None, pm1=False):
    xd = x.cuda().requires_grad_(True)
    out = D.run(op, xd, p0, p1, noise=None if noise is None else noise.cuda(), pm1=pm1)
    out.backward(g.cuda())
    return out.detach(), xd.grad


def _torch_device_grad(op, x, g, p0, p1, pm1):
    """torch's own fp32 autograd through the restatement, on the device"""
    xd = x.cuda().requires_grad_(True)
    u = xd / 2.0 + 0.5 if pm1 else xd
    t = R.transform(op, u, p0, p1)
    c = t.clamp(0, 1) if (pm1 or op in R.CLAMPING) else t
    (c * 2.0 - 1.0 if pm1 else c).backward(g.cuda())
    return xd.grad


# ------------------------------------------------------------------------------------------------------------------ the graph
def test_output_joins_the_graph_and_no_grad_is_todays_launch():
    u, g = _inputs(21, 19, 1)
    x = u.cuda().requires_grad_(True)
    for op, p0, p1 in ((D.BLUR, 3, 0), (D.BRIGHTNESS, 1.5, 0), (D.ROTATE, 0, 20), (D.FLIP_H, 0, 0), (D.CROP_RESIZE, 10, 9),
                       (D.CROP_PAD, 10, 9), (D.IDENTITY, 0, 0)):
        x.grad = None
        out = D.run(op, x, p0, p1)
        assert out.requires_grad and out.grad_fn is not None, op
        out.backward(g.cuda())
        assert x.grad is not None and x.grad.device == x.device and x.grad.shape == x.shape, op
        with torch.no_grad():
            plain = D.run(op, x, p0, p1)
        assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, out.detach()), op
        assert torch.equal(plain, D.run(op, x.detach(), p0, p1)) and not D.run(op, x.detach(), p0, p1).requires_grad, op


# ------------------------------------------------------------------------------------------------------------------ bit-equal transforms
@pytest.mark.parametrize("pm1", [False, True])
@pytest.mark.parametrize("exact", [False, True])
def test_pointwise_transforms_are_bit_equal_to_the_fp32_reference(pm1, exact):
    u, g = _inputs(16, 16, 2, exact)
    x = _x(u, pm1)
    noise = torch.randn(u.shape, generator=torch.Generator().manual_seed(3))
    for op, p0, p1, nz in ((D.IDENTITY, 0, 0, None), (D.FLIP_H, 0, 0, None), (D.CROP_PAD, 8, 8, None), (D.BRIGHTNESS, 2.0, 0, None),
                           (D.BRIGHTNESS, 1.3, 0, None), (D.NOISE, 0.1, 0, noise)):
        _, got = _device_grad(op, x, g, p0, p1, nz, pm1)
        ref = R.reference(op, x, g, p0, p1, nz, pm1, dtype=torch.float32)
        assert torch.equal(got.cpu(), ref.grad), (op, p0)
        if not exact and ref.clamps:                                    # the mask really blocks
            assert bool((ref.grad == 0).any()), (op, p0)


@pytest.mark.parametrize("pm1", [False, True])
def test_brightness_mask_includes_both_bounds(pm1):
    """f = 2: t is exactly 0, exactly 1 and above 1 at known pixels; the gradient is f g at both bounds and 0 above"""
    u, g = _inputs(16, 16, 4)
    u[..., 0, 0], u[..., 0, 1], u[..., 0, 2], u[..., 0, 3] = 0.0, 0.5, 0.75, -0.25
    _, got = _device_grad(D.BRIGHTNESS, _x(u, pm1), g, 2.0, pm1=pm1)
    got = got.cpu()
    assert torch.equal(got[..., 0, 0], 2.0 * g[..., 0, 0]) and torch.equal(got[..., 0, 1], 2.0 * g[..., 0, 1])
    assert not bool(got[..., 0, 2].any()) and not bool(got[..., 0, 3].any())


ROTATIONS = [(17, 17, q, rest) for q in range(4) for rest in (0, 5, 70)] + [(12, 20, 0, 20), (12, 20, 2, 0), (12, 20, 2, 20)]


@pytest.mark.parametrize("pm1", [False, True])
def test_rotation_follows_the_forwards_own_index_map(pm1):
    for H, W, q, rest in ROTATIONS:
        u, g = _inputs(H, W, 5)
        x = _x(u, pm1)
        with torch.no_grad():
            imap = D.run(D.ROTATE, R.index_image(H, W).cuda(), q, rest).cpu().round().long().view(H, W)
        reads = torch.bincount(imap.view(-1), minlength=H * W + 1)[1:]
        assert int(reads.max()) <= (2 if rest else 1), (H, W, q, rest, int(reads.max()))      # at most two addends: any order is exact
        out, got = _device_grad(D.ROTATE, x, g, q, rest, pm1=pm1)
        ref = R.reference(D.ROTATE, x, g, q, rest, pm1=pm1, index_map=imap, dtype=torch.float32)
        assert torch.equal(out.cpu(), ref.out), (H, W, q, rest)
        assert torch.equal(got.cpu(), ref.grad), (H, W, q, rest)
        if rest:
            assert int((reads == 0).sum()) > 0 and int((reads == 2).sum()) > 0, (H, W, q, rest)


# ------------------------------------------------------------------------------------------------------------------ the two stencils
def _stencil_cases():
    cases = [("blur", D.BLUR, H, W, k, 0) for H, W, k in ((21, 19, 3), (21, 19, 9), (5, 5, 9), (40, 40, 19))]
    cases += [("resize", D.CROP_RESIZE, 23, 31, int(f * 23), int(f * 31)) for f in (0.5, 0.95)]
    cases += [("resize", D.CROP_RESIZE, 23, 31, 10, 25)]
    return cases


def _measure(kind):
    """(c of the kernels, c of torch's fp32 autograd on the device, largest tie fraction) over every case of `kind`"""
    c_kernel = c_torch = worst_ties = 0.0
    for name, op, H, W, p0, p1 in _stencil_cases():
        if name != kind:
            continue
        for pm1 in (False, True):
            for exact in (False, True) + (("wide",) if kind == "blur" else ()):
                u, g = _inputs(H, W, 6 + H, exact)
                x = _x(u, pm1)
                g, ties = R.zero_ties(op, x, g, p0=p0, p1=p1, pm1=pm1)
                ref = R.reference(op, x, g, p0, p1, pm1=pm1)
                assert exact != "wide" or 0.0 < float((ref.gm == 0).double().mean()) < 1.0, (H, W, p0)        # the mask blocks and passes
                _, got = _device_grad(op, x, g.float(), p0, p1, pm1=pm1)
                ck, ct = R.smallest_c(got, ref), R.smallest_c(_torch_device_grad(op, x, g.float(), p0, p1, pm1), ref)
                print(f"{name} {H}x{W} p=({p0},{p1}) pm1={int(pm1)} inputs={exact}: c_kernel {ck:.3f} c_torch {ct:.3f} ties {ties:.2e}")
                c_kernel, c_torch, worst_ties = max(c_kernel, ck), max(c_torch, ct if exact != "wide" else 0.0), max(worst_ties, ties)
    print(f"{kind}: c_kernel {c_kernel:.3f}, c_torch {c_torch:.3f} (recorded {C_TORCH[kind]}), ties <= {worst_ties:.2e}")
    return c_kernel, c_torch, worst_ties


@pytest.mark.parametrize("kind", ["blur", "resize"])
def test_stencil_gradients_within_twice_torchs_own_fp32_error(kind):
    c_kernel, c_torch, ties = _measure(kind)
    assert ties <= 0.01, ties
    assert c_torch <= 2.0 * C_TORCH[kind], (c_torch, C_TORCH[kind])     # loose: the recorded constant is still about torch's own
    assert c_kernel <= 2.0 * C_TORCH[kind], (c_kernel, C_TORCH[kind])


def test_two_backward_runs_give_the_same_bits():
    for op, H, W, p0, p1 in ((D.BLUR, 40, 40, 19, 0), (D.BLUR, 21, 19, 9, 0), (D.ROTATE, 17, 17, 1, 70), (D.CROP_RESIZE, 23, 31, 11, 15)):
        u, g = _inputs(H, W, 7)
        a, b = _device_grad(op, _x(u, True), g, p0, p1, pm1=True)[1], _device_grad(op, _x(u, True), g, p0, p1, pm1=True)[1]
        assert torch.equal(a, b), op


# ------------------------------------------------------------------------------------------------------------------ shapes, modules
def test_3d_and_non_contiguous_inputs_get_their_own_gradient_layout():
    u, g = _inputs(21, 19, 8)
    _, want = _device_grad(D.BLUR, u, g, 9)
    one = u[0].cuda().requires_grad_(True)                              # [3, H, W]
    out = D.run(D.BLUR, one, 9)
    assert out.shape == one.shape
    out.backward(g[0].cuda())
    assert one.grad.shape == one.shape and torch.equal(one.grad, want[0])
    base = u.permute(0, 1, 3, 2).contiguous().cuda().requires_grad_(True)      # the image is a transposed view of this leaf
    view = base.permute(0, 1, 3, 2)
    assert not view.is_contiguous()
    D.run(D.BLUR, view, 9).backward(g.cuda())
    assert base.grad.shape == base.shape and base.grad.stride() == base.stride()
    assert torch.equal(base.grad.permute(0, 1, 3, 2), want)


def test_apply_random_augmentation_trains_through_every_weak_class():
    from wmar_amd.augmentations import finetune_schedule
    from wmar_amd.utils.utils import apply_random_augmentation
    weak = finetune_schedule("all+geom", "0,1,0,0", 1)[0]
    gen = torch.Generator().manual_seed(9)
    for entry in weak:
        random.seed(0)
        x = (torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1).cuda().requires_grad_(True)
        x_t, info = apply_random_augmentation(x, [entry], p=1.0)
        assert info is not None and info[0] is entry[0] and x_t.requires_grad, entry
        (x_t ** 2).sum().backward()
        assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any()), entry


def test_fused_is_differentiable_and_equals_the_unfused_sequence():
    from wmar_amd.augmentations import AugmentationManager
    u, g = _inputs(32, 32, 10)
    x = _x(u, True)
    for name, fn, params in AugmentationManager(False, False, True).augs:
        if name == "jpeg":                                              # straight-through inside the module; fused() has no graph for it
            continue
        for p in params[:3]:
            a = x.cuda().requires_grad_(True)
            b = x.cuda().requires_grad_(True)
            torch.manual_seed(11)
            fused = D.fused(name, a, p)
            torch.manual_seed(11)
            unfused = fn(b / 2.0 + 0.5, p).clamp(0, 1) * 2.0 - 1.0
            assert fused.requires_grad and torch.equal(fused, unfused), (name, p)
            fused.backward(g.cuda())
            unfused.backward(g.cuda())
            assert torch.equal(a.grad, b.grad), (name, p)
