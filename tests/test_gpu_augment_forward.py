"""The forward transform kernels (wmar_augment: k_aug_blur, k_aug_point<op>; wmar_amd/csrc/augment.hip) on the MI355X, each held alone to
the references of tests/augment_forward_reference.py -- the gates that file's float32 models pass, and its planted errors fail, on the CPU:

  * rotation: the kernel's index map, read with an image holding 1 .. H W per plane, equals the FLOAT64 map on every decidable pixel
    (on every pixel where the map has no undecidable one, which is asserted on the reference before the kernel is looked at); an
    undecidable pixel shows one of its candidates; the pm1 form carries the same map on a random image with saturated pixels;
  * blur and crop + resize: per pixel |got - t64| <= c 2^-24 A with c_kernel <= 2 max(c_torch, c_chain) -- torch's fp32 restatement on the
    device in the same test and the sequential float32 model; single-tap cases are bit-equal;
  * identity, flip, crop + pad, brightness and noise: bit-equal to the numpy float32 restatement, special values planted;
  * the ABI: in-place calls, non-contiguous, 3-D and one-channel inputs, two runs of every case with the same bits, and the plane limit
    of the blur launch.

Shapes are the smallest at which the kernels can go wrong (ragged 16 x 16 tiles, halos wider than the tile and as wide as the image,
non-square images, single-tap windows); planes are 2 x 3 with different content per plane.  Every test prints what it measured on lines
starting with AUGFWD (DESIGN.md section 4 records them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import augment_forward_reference as R  # noqa: E402
from wmar_amd import _lib  # noqa: E402
from wmar_amd.augmentations import device_ops as D  # noqa: E402
from wmar_amd.augmentations.geometric import Rotate  # noqa: E402


def _report(line):
    print("AUGFWD " + line)


def _run(op, x, p0=0.0, p1=0.0, noise=None, pm1=False):
    """the launch through device_ops.run, twice: two runs of every case give the same bits"""
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).cuda()
    nd = None if noise is None else torch.from_numpy(np.array(noise, dtype=np.float32)).cuda()
    a, b = D.run(op, xd, p0, p1, noise=nd, pm1=pm1), D.run(op, xd, p0, p1, noise=nd, pm1=pm1)
    assert a.shape == xd.shape and a.data_ptr() != xd.data_ptr()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (op, p0, p1, pm1)
    return a.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ rotation
ROTATION_GROUPS = {f"sweep-{S}": [c for c in R.ROTATION_SWEEP if c[0] == S] for S in (16, 17, 50, 64)}
ROTATION_GROUPS.update({"rect": R.ROTATION_RECT, "ties": list(R.ROTATION_TIES), "thin": R.ROTATION_THIN, "quarters": R.ROTATION_QUARTERS})
assert sorted(sum(ROTATION_GROUPS.values(), [])) == sorted(set(R.ROTATION_CASES) | set(R.ROTATION_TIES))


@pytest.mark.parametrize("group", sorted(ROTATION_GROUPS))
def test_rotation_map_equals_the_float64_map(group):
    for case in ROTATION_GROUPS[group]:
        R.gate_rotation(_run, *case, report=_report)


def test_pure_quarter_turns_are_bit_equal_to_rot90():
    for H, W, q, _ in R.ROTATION_QUARTERS:
        for pm1 in (False, True):
            x = R.saturated_image(H, W, pm1)
            want = torch.rot90(torch.from_numpy(R.model(R.IDENTITY, x, pm1=pm1)), q, dims=(-2, -1)).numpy()
            R.assert_bits(_run(D.ROTATE, x, q, 0, pm1=pm1), want, (H, W, q, pm1))
        xd = torch.from_numpy(R.saturated_image(H, W, False)).cuda()
        assert torch.equal(Rotate()(xd, 90 * q), torch.rot90(xd, q, dims=(-2, -1))), (H, W, q)


def test_rotation_through_the_module():
    """Rotate() on the device: negative angles (three quarter turns + 70), 185 and 200 degrees on a non-square image (two quarter turns
    + a remainder), a 3-D image"""
    for H, W, angle in ((17, 17, -20), (17, 17, 20), (16, 16, -5), (12, 20, 185), (12, 20, 200), (33, 47, 200)):
        q, rest = divmod(angle, 90)
        n = R.assert_cap(H, W, q % 4, rest)
        idx = R.index_image(H, W)
        got = Rotate()(torch.from_numpy(idx).cuda(), angle).cpu().numpy()
        assert R.check_rotation(got, idx, 0.0, H, W, q % 4, rest) == n == 0
        one = Rotate()(torch.from_numpy(idx[1]).cuda(), angle)
        assert one.shape == (3, H, W) and np.array_equal(one.cpu().numpy(), got[1])
        _report(f"rotation module {H}x{W} angle={angle}: undecidable {n} of {H * W}")


# ------------------------------------------------------------------------------------------------------------------ blur, crop + resize
@pytest.mark.parametrize("H,W,k", R.BLUR_CASES)
def test_blur_within_twice_the_references_own_fp32_error(H, W, k):
    R.gate_stencil(_run, R.BLUR, H, W, k, 0, torch_device="cuda", report=_report)


@pytest.mark.parametrize("H,W,nh,nw", R.RESIZE_CASES)
def test_crop_resize_within_twice_the_references_own_fp32_error(H, W, nh, nw):
    R.gate_stencil(_run, R.CROP_RESIZE, H, W, nh, nw, torch_device="cuda", report=_report)


def test_single_tap_stencils_are_bit_equal():
    """k = 1 is the clamp alone; a crop that keeps the whole image returns the input's bits"""
    for H, W, k in R.BLUR_EXACT:
        R.gate_exact_stencil(_run, R.BLUR, H, W, k, 0)
    for H, W, nh, nw in R.RESIZE_EXACT:
        R.gate_exact_stencil(_run, R.CROP_RESIZE, H, W, nh, nw)


def test_fused_crop_factors_of_the_sweep():
    """the eleven upperleft-crop factors of the table on 50 x 50 through device_ops.fused (pm1 form; 1.0 is the identity launch)"""
    for f in R.CROP_FACTORS:
        n = int(f * 50)
        fused = lambda op, x, p0, p1, noise, pm1, f=f: D.fused("upperleft-crop", torch.from_numpy(np.array(x)).cuda(), f).cpu().numpy()  # noqa: E731
        if n == 50:
            x = R.stencil_input(50, 50, "plain", True)
            R.assert_bits(fused(None, x, n, n, None, True), R.model(R.IDENTITY, x, pm1=True), f)
        else:
            R.gate_stencil(fused, R.CROP_RESIZE, 50, 50, n, n, torch_device="cuda", report=_report, forms=(True,))


# ------------------------------------------------------------------------------------------------------------------ pointwise
@pytest.mark.parametrize("H,W", [(16, 16), (7, 37), (5, 1)])
def test_pointwise_transforms_are_bit_equal_to_the_float32_restatement(H, W):
    """every brightness factor and noise sigma of the table, identity, flip (W = 1 included), crop + pad with nh != nw"""
    R.gate_pointwise(_run, H, W)
    _report(f"pointwise {H}x{W}: {2 * len(R.pointwise_calls(H, W))} calls bit-equal")


# ------------------------------------------------------------------------------------------------------------------ shapes, ABI
CALLS = [(D.IDENTITY, 0, 0), (D.BLUR, 9, 0), (D.NOISE, 0.1, 0), (D.BRIGHTNESS, 1.75, 0), (D.ROTATE, 2, 20), (D.FLIP_H, 0, 0),
         (D.CROP_RESIZE, 10, 25), (D.CROP_PAD, 10, 25)]


def test_one_channel_3d_and_non_contiguous_inputs():
    """planes are independent: a C = 1 batch, a 3-D image and a non-contiguous view give the bits of the same planes in the 2 x 3 batch"""
    H, W = 21, 29
    noise = torch.randn(*R.BC, H, W, generator=torch.Generator().manual_seed(5))
    for pm1 in (False, True):
        x = torch.from_numpy(R.stencil_input(H, W, "plain", pm1))
        for op, p0, p1 in CALLS:
            nz = noise if op == D.NOISE else None
            full = _run(op, x.numpy(), p0, p1, None if nz is None else nz.numpy(), pm1)
            one = D.run(op, x[:, 1:2].cuda(), p0, p1, noise=None if nz is None else nz[:, 1:2].cuda(), pm1=pm1)
            assert one.shape == (2, 1, H, W) and np.array_equal(one.cpu().numpy().view(np.int32), full[:, 1:2].view(np.int32)), (op, pm1)
            img = D.run(op, x[1].cuda(), p0, p1, noise=None if nz is None else nz[1].cuda(), pm1=pm1)
            assert img.shape == (3, H, W) and np.array_equal(img.cpu().numpy().view(np.int32), full[1].view(np.int32)), (op, pm1)
            view = x.permute(0, 1, 3, 2).contiguous().cuda().permute(0, 1, 3, 2)          # same pixels, transposed strides
            assert not view.is_contiguous()
            got = D.run(op, view, p0, p1, noise=None if nz is None else nz.cuda(), pm1=pm1)
            assert np.array_equal(got.cpu().numpy().view(np.int32), full.view(np.int32)), (op, pm1)


def _call(op, src, dst, noise, shape, pm1, p0, p1=0.0):
    B, C, H, W = shape
    return _lib.load().wmar_augment(int(op), src.data_ptr(), dst.data_ptr(), noise.data_ptr() if noise is not None else None, B, C, H, W,
                                    1 if pm1 else 0, float(p0), float(p1), _lib.stream_ptr(src.device))


def test_in_place_calls_give_the_bits_of_the_out_of_place_call():
    """the ABI allows in_dev == out_dev for noise, brightness and identity (one thread reads and writes its own element)"""
    H, W = 7, 37
    noise = torch.randn(*R.BC, H, W, generator=torch.Generator().manual_seed(6)).cuda()
    for pm1 in (False, True):
        x = torch.from_numpy(R.pointwise_input(H, W, pm1)).cuda()
        for op, p0 in ((D.NOISE, 0.125), (D.BRIGHTNESS, 2.0), (D.BRIGHTNESS, 1.25), (D.IDENTITY, 0)):
            nz = noise if op == D.NOISE else None
            out, buf = torch.empty_like(x), x.clone()
            _lib.check(_call(op, x, out, nz, x.shape, pm1, p0))
            _lib.check(_call(op, buf, buf, nz, x.shape, pm1, p0))
            assert torch.equal(out.view(torch.int32), buf.view(torch.int32)), (op, p0, pm1)
            R.assert_bits(out.cpu().numpy(), R.model(op, x.cpu().numpy(), p0, 0, None if nz is None else nz.cpu().numpy(), pm1), (op, p0, pm1))
    for op in (D.BLUR, D.ROTATE, D.FLIP_H, D.CROP_RESIZE, D.CROP_PAD):                    # every gathering transform refuses
        buf = torch.rand(*R.BC, H, W, device="cuda")
        keep = buf.clone()
        assert _call(op, buf, buf, None, buf.shape, False, 3, 3) != 0 and torch.equal(buf, keep), op


def test_blur_refuses_more_planes_than_the_launch_can_take():
    """planes are gridDim.z of the blur launches: B C = 65536 planes of 1 x 1 with k = 1 return the error before any launch"""
    L = _lib.load()
    n = 65536
    x = torch.rand(n, 1, 1, 1, device="cuda")
    out = torch.full_like(x, -7.0)
    assert _call(D.BLUR, x, out, None, x.shape, False, 1) != 0
    assert "planes" in L.wmar_last_error().decode()
    g, gin, ws = torch.ones_like(x), torch.full_like(x, -7.0), torch.full_like(x, -7.0)
    rc = L.wmar_augment_backward(int(D.BLUR), x.data_ptr(), g.data_ptr(), gin.data_ptr(), None, ws.data_ptr(), n, 1, 1, 1, 0, 1.0, 0.0,
                                 _lib.stream_ptr(x.device))
    assert rc != 0 and "planes" in L.wmar_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((gin == -7.0).all()) and bool((ws == -7.0).all())      # nothing ran
    with pytest.raises(_lib.WmarError, match="planes"):
        D.run(D.BLUR, x, 1)
    ok = D.run(D.BLUR, x[:65535], 1)                                                      # the largest legal count still runs
    assert torch.equal(ok, x[:65535])
