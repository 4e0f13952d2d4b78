"""MI355X: LPIPS on the device (wmar_amd/csrc/lpips.h, wmar_amd/lpips.py) -- every new layer alone through the wmar_lpips_probe_* entries,
VGG16's convolution shapes through the existing convolution probes, the whole net against the reference module's float64 results
(tests/golden/lpips_vectors.npz, written by tests/golden/make_lpips_vectors.py) and a narrow net against the float64 restatement
(tests/lpips_reference.py), determinism, autograd, ``rcc_loss`` and the finetune CLI.

Gates (none measured on the code under test):
  exact layers   the input edge, ReLU, ReLU + max-pool and their backwards are bit-equal to torch's fp32 CPU result.
  head           value error normalised by the value, gradient error normalised by max|g| per image: <= 4 x the same figure of torch's
                 fp32 CPU autograd on the same data against float64, floor 4 x 2^-24 (the GroupNorm / attention gate of
                 tests/test_gpu_vq_grad_layers.py).  The gradient at an all-zero feature vector is exactly 0.  Shapes: 8 x 8 (one pixel
                 chunk), 8 x 25 (three chunks of 66 / 67 / 67 pixels) and 128 x 130 (HW / 64 = 260 chunks cut to the cap 256), with
                 zero vectors in the first, the last and a middle chunk and next to the chunk boundaries.
  convolutions   the dense gate of tests/vq_layer_checks.py, forward and input gradient: <= 2 x a sequential fp32 chain.
  whole net      values <= 1e-5 relative; input gradient per image |got - g64|_inf / |g64|_inf <= 8 x the same figure of the fp32 CPU
                 restatement on the same data (the two gates of tests/test_gpu_vq_train.py).

The measured figures are printed on lines starting with LPIPS (run with -s)."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_reference as LR
from tests import vq_grad_reference as G
from tests import vq_layer_checks as K
from tests import vq_layer_reference as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TORCH_FACTOR = 4.0
FLOOR = 4.0 * R.U24
VALUE_GATE = 1e-5
NET_GATE = 8.0
NARROW = (8, 16, 32, 32, 32)


def _say(what, case, **figs):
    print("LPIPS %s %s %s" % (what, case, " ".join("%s=%.4g" % kv for kv in figs.items())), flush=True)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _nhwc(x, extra=0, fill=None):
    """torch NCHW (cpu) -> cuda NHWC with `extra` more stored channels holding `fill`."""
    B, Cc, H, W = x.shape
    out = torch.zeros(B, H, W, Cc + extra)
    if extra:
        out[..., Cc:] = fill
    out[..., :Cc] = x.permute(0, 2, 3, 1)
    return out.cuda().contiguous()


def _nchw(t, Cc):
    return t.cpu()[..., :Cc].permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ the input edge
@pytest.mark.parametrize("hw", [8, 16])
def test_input_edge_forward_and_backward_are_bit_equal_to_torch(hw):
    lib, L = K._lib()
    from wmar_amd.utils.synth import LPIPS_SCALE, LPIPS_SHIFT
    B = 3
    g = torch.Generator().manual_seed(hw)
    x = (torch.rand(B, 3, hw, hw, generator=g) * 2 - 1).requires_grad_(True)
    shift, scale = torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1), torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1)
    want = (x - shift) / scale
    gy = torch.randn(B, 3, hw, hw, generator=g)
    want.backward(gy)
    xd, sh, sc = x.detach().cuda().contiguous(), shift.cuda().contiguous(), scale.cuda().contiguous()
    y = torch.full((B, hw, hw, 8), float("nan"), device="cuda")
    lib.check(L.wmar_lpips_probe_input(xd.data_ptr(), sh.data_ptr(), sc.data_ptr(), B, hw * hw, y.data_ptr(), lib.stream_ptr()))
    assert _same_bits(_nchw(y, 3), want)
    assert torch.all(y[..., 3:] == 0), "padding channels of the scaled image must be 0"
    gd = _nhwc(gy, 5, torch.randn(B, hw, hw, 5, generator=g) * 1e6)          # garbage in the padding channels
    gx = torch.full((B, 3, hw, hw), float("nan"), device="cuda")
    lib.check(L.wmar_lpips_probe_input_backward(gd.data_ptr(), sc.data_ptr(), B, hw * hw, gx.data_ptr(), lib.stream_ptr()))
    assert _same_bits(gx, x.grad)


# ------------------------------------------------------------------------------------------------ ReLU + max-pool
def _pool_input(Cc, seed, B=3, H=16):
    """Normal values with, planted per image: equal positive values in every pair of window positions (and in all four), windows whose
    maximum is shared with a smaller value elsewhere, exact zeros, -0.0, all-negative and all-zero windows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cc, H, H, generator=g)
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1, 2, 3), (1, 2, 3), (0, 2, 3)]
    pos = [(0, 0), (0, 1), (1, 0), (1, 1)]
    n = 0
    for b in range(B):
        for c in range(Cc):
            for k, tie in enumerate(pairs):
                wy, wx = (c + k) % (H // 2), (b + c + 2 * k + 3 * (k // 8)) % (H // 2)      # nine different windows per plane
                x[b, c, 2 * wy:2 * wy + 2, 2 * wx:2 * wx + 2] = -0.25         # the others lose
                for i in tie:
                    x[b, c, 2 * wy + pos[i][0], 2 * wx + pos[i][1]] = 1.5 + k
                n += 1
    x[:, :, 4:6, 6:8] = 0.0                                                      # an all-zero window
    x[:, :, 6, 2] = -0.0
    x[:, :, 7, 3] = 0.0
    x[:, ::2, 10:12, 10:12] = -torch.rand(B, (Cc + 1) // 2, 2, 2, generator=g) - 0.1      # all negative
    x[:, :, 12, 12] = -0.0
    x[:, :, 12, 13] = -0.0
    x[:, :, 13, 12] = -3.0
    x[:, :, 13, 13] = -0.0                                                      # a window of -0.0 and a negative
    assert n == B * Cc * len(pairs)
    return x, g


@pytest.mark.parametrize("Cc", [8, 40])
def test_relu_maxpool_forward_and_backward_are_bit_equal_to_torch(Cc):
    lib, L = K._lib()
    B, H = 3, 16
    x, g = _pool_input(Cc, 100 + Cc)
    xt = x.clone().requires_grad_(True)
    y = F.relu(xt)
    p = F.max_pool2d(y, 2, 2)
    gp, gt = torch.randn(p.shape, generator=g), torch.randn(y.shape, generator=g)
    ((p * gp).sum() + (y * gt).sum()).backward()
    outs = []
    for extra in (0, 8):                       # 8 more stored channels of garbage must change no bit of the real ones
        fill = torch.randn(B, H, H, extra, generator=g) * 1e6 if extra else None
        fill2 = torch.randn(B, H // 2, H // 2, extra, generator=g) * 1e6 if extra else None
        Cs = Cc + extra
        xd = _nhwc(x, extra, fill)
        yd = torch.full((B, H, H, Cs), float("nan"), device="cuda")
        pd = torch.full((B, H // 2, H // 2, Cs), float("nan"), device="cuda")
        lib.check(L.wmar_lpips_probe_relu_pool(xd.data_ptr(), B, H, H, Cs, yd.data_ptr(), pd.data_ptr(), lib.stream_ptr()))
        assert _same_bits(_nchw(yd, Cc), y) and _same_bits(_nchw(pd, Cc), p)
        ip = xd.clone()                        # in place, as the engine runs it
        lib.check(L.wmar_lpips_probe_relu_pool(ip.data_ptr(), B, H, H, Cs, ip.data_ptr(), pd.data_ptr(), lib.stream_ptr()))
        assert torch.equal(ip.view(torch.int32), yd.view(torch.int32))
        gpd, gtd = _nhwc(gp, extra, fill2), _nhwc(gt, extra, fill)
        gx = torch.full((B, H, H, Cs), float("nan"), device="cuda")
        lib.check(L.wmar_lpips_probe_relu_pool_backward(yd.data_ptr(), gpd.data_ptr(), gtd.data_ptr(), B, H, H, Cs, gx.data_ptr(), lib.stream_ptr()))
        assert _same_bits(_nchw(gx, Cc), xt.grad), "ReLU + max-pool backward (first maximum, tap gradient added, ReLU mask)"
        lib.check(L.wmar_lpips_probe_relu_pool_backward(yd.data_ptr(), gpd.data_ptr(), gtd.data_ptr(), B, H, H, Cs, gtd.data_ptr(), lib.stream_ptr()))
        assert torch.equal(gtd.view(torch.int32), gx.view(torch.int32)), "in place over the tap gradient"
        outs.append(_nchw(gx, Cc))
    assert _same_bits(outs[0], outs[1])


@pytest.mark.parametrize("Cc", [8, 40])
def test_relu_alone_forward_and_backward_are_bit_equal_to_torch(Cc):
    lib, L = K._lib()
    B, H = 3, 16
    x, g = _pool_input(Cc, 200 + Cc)
    xt = x.clone().requires_grad_(True)
    y = F.relu(xt)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    xd = _nhwc(x)
    lib.check(L.wmar_lpips_probe_relu_pool(xd.data_ptr(), B, H, H, Cc, xd.data_ptr(), None, lib.stream_ptr()))
    assert _same_bits(_nchw(xd, Cc), y)
    gd = _nhwc(gy)
    lib.check(L.wmar_lpips_probe_relu_pool_backward(xd.data_ptr(), None, gd.data_ptr(), B, H, H, Cc, gd.data_ptr(), lib.stream_ptr()))
    assert _same_bits(_nchw(gd, Cc), xt.grad)


# ------------------------------------------------------------------------------------------------ the head of one tap
def _head_data(Cc, seed, B=3, H=8, W=None, zero0=None):
    """zero0: (image, y, x) of the all-zero feature vectors planted in the first operand."""
    W = H if W is None else W
    g = torch.Generator().manual_seed(seed)
    f0, f1 = F.relu(torch.randn(B, Cc, H, W, generator=g) + 0.3), F.relu(torch.randn(B, Cc, H, W, generator=g) + 0.3)
    zero0 = [(0, 0, 0), (0, 3, 5), (1, 7, 7), (2, 4, 4), (2, 0, 7)] if zero0 is None else zero0
    zero1 = [(0, 1, 1), (1, 2, 6), zero0[3]]                       # zero0[3]: both operands
    for b, yy, xx in zero0:
        f0[b, :, yy, xx] = 0.0
    for b, yy, xx in zero1:
        f1[b, :, yy, xx] = 0.0
    w = torch.rand(Cc, generator=g) / Cc
    gv = torch.rand(B, generator=g) + 0.5
    return f0, f1, w, gv, zero0


def _head_torch(f0, f1, w, gv, dtype):
    a = f0.to(dtype).requires_grad_(True)
    v = LR.head(a, f1.to(dtype), w.to(dtype))
    (v * gv.to(dtype)).sum().backward()
    return v.detach(), a.grad


@pytest.mark.parametrize("Cc", [8, 64, 512])
def test_head_value_and_gradient_within_four_times_torch_fp32(Cc):
    _check_head(Cc, 8, 8, None)


def _pixels(W, plan):
    return [(b, p // W, p % W) for b, p in plan]


@pytest.mark.parametrize("H,W,chunks,zeros", [
    # 200 pixels: lp_chunks = 3, chunks [0, 66) [66, 133) [133, 200) -- zero vectors at both ends and on both sides of each boundary
    (8, 25, 3, [(0, 0), (0, 199), (1, 100), (2, 65), (2, 66), (1, 132), (0, 133)]),
    # 16 640 pixels: HW / 64 = 260 is cut to the cap 256, 65 pixels per chunk -- first, last and a middle chunk, and a chunk's last pixel
    (128, 130, 256, [(0, 0), (0, 16639), (1, 128 * 65), (2, 128 * 65 - 1), (2, 64), (1, 16575)]),
], ids=["8x25", "128x130"])
def test_head_with_uneven_and_capped_pixel_chunks(H, W, chunks, zeros):
    assert chunks == min(max(H * W // 64, 1), 256)               # lp_chunks restated
    _check_head(64, H, W, _pixels(W, zeros))


def _check_head(Cc, H, W, zero0):
    lib, L = K._lib()
    B = 3
    f0, f1, w, gv, zero0 = _head_data(Cc, 300 + Cc + (0 if H == W == 8 else H * W), B, H, W, zero0)
    v64, g64 = _head_torch(f0, f1, w, gv, torch.float64)
    v32, g32 = _head_torch(f0, f1, w, gv, torch.float32)
    nz = torch.ones(B, 1, H, W, dtype=torch.bool)
    for b, yy, xx in zero0:
        nz[b, 0, yy, xx] = False
        assert torch.isnan(g64[b, :, yy, xx]).all(), "float64 autograd on the bare head has no gradient at an all-zero vector"
    assert torch.isfinite(g64[nz.expand_as(g64)]).all()
    f0d, f1d, wd, gvd = _nhwc(f0), _nhwc(f1), w.cuda(), gv.cuda()
    val = torch.full((B,), float("nan"), device="cuda")
    lib.check(L.wmar_lpips_probe_head(f0d.data_ptr(), f1d.data_ptr(), wd.data_ptr(), B, H * W, Cc, val.data_ptr(), lib.stream_ptr()))
    g0 = torch.full((B, H, W, Cc), float("nan"), device="cuda")
    lib.check(L.wmar_lpips_probe_head_backward(f0d.data_ptr(), f1d.data_ptr(), wd.data_ptr(), gvd.data_ptr(), B, H * W, Cc, g0.data_ptr(),
                                               lib.stream_ptr()))
    again = torch.full((B, H, W, Cc), float("nan"), device="cuda")
    lib.check(L.wmar_lpips_probe_head_backward(f0d.data_ptr(), f1d.data_ptr(), wd.data_ptr(), gvd.data_ptr(), B, H * W, Cc, again.data_ptr(),
                                               lib.stream_ptr()))
    assert torch.equal(g0.view(torch.int32), again.view(torch.int32)), "two runs differ"
    got = _nchw(g0, Cc).double()
    e_v = float(((val.cpu().double() - v64).abs() / v64).max())
    b_v = float(((v32.double() - v64).abs() / v64).max())
    keep = nz.expand_as(g64)
    z = torch.zeros_like(g64)
    d_got, d_32, ref = torch.where(keep, got - g64, z), torch.where(keep, g32.double() - g64, z), torch.where(keep, g64, z)
    scale = ref.abs().amax((1, 2, 3))
    e_g = float((d_got.abs().amax((1, 2, 3)) / scale).max())
    b_g = float((d_32.abs().amax((1, 2, 3)) / scale).max())
    _say("head", "C=%d %dx%d" % (Cc, H, W), value_err=e_v, value_torch_fp32=b_v, grad_err=e_g, grad_torch_fp32=b_g)
    assert torch.isfinite(got).all()
    for b, yy, xx in zero0:
        assert torch.all(g0[b, yy, xx] == 0), "the gradient at an all-zero feature vector must be exactly 0"
    assert e_v <= max(TORCH_FACTOR * b_v, FLOOR), "head C=%d %dx%d value: error %.3g against torch fp32's %.3g" % (Cc, H, W, e_v, b_v)
    assert e_g <= max(TORCH_FACTOR * b_g, FLOOR), "head C=%d %dx%d gradient: error %.3g against torch fp32's %.3g" % (Cc, H, W, e_g, b_g)


# ------------------------------------------------------------------------------------------------ VGG16's convolution shapes
VGG_CONVS = [(3, 64, 16), (64, 64, 16), (64, 128, 16), (128, 128, 16), (128, 256, 8), (256, 256, 8), (256, 512, 8), (512, 512, 8)]


@pytest.mark.parametrize("cin,cout,hw", VGG_CONVS, ids=["%dto%d-%d" % c for c in VGG_CONVS])
def test_vgg_conv_shapes_forward_and_input_gradient(cin, cout, hw):
    from tests.test_gpu_vq_grad_layers import probe_conv_backward
    B = 2
    rng = np.random.default_rng(cin * 131 + cout)
    x0 = R.realistic_activations(rng, (B, cin, hw, hw))
    w0 = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    kernel = K.probe_conv(w0, np.zeros(cout, dtype=np.float32), x0)[3]["conv"]        # the dispatch's own report names the case
    case = K.ConvCase(kernel, cin, cout, 3, hw, res=False, B=B)
    K.check_dense(case)
    K.check_epilogue(case)
    x, w, g = x0, w0, (rng.standard_normal((B, cout, hw, hw)) * 0.05).astype(np.float32)
    gx, gxpad, _, _, info = probe_conv_backward(w, x, g)
    print("LPIPS conv %dto%d-%d forward=%s %s" % (cin, cout, hw, kernel, info["dgrad"]), flush=True)
    ex, ax = G.conv2d_backward(x, w, g)[0], G.conv2d_backward_abs(x, w, g)[0]
    cx = G.conv2d_dgrad_chain(x.shape, w, g)
    e, e_chain = G.normalised_error(gx, ex, ax), G.normalised_error(cx, ex, ax)
    _say("conv_dgrad", "%dto%d-%d %s" % (cin, cout, hw, info["dgrad"]), err=e, chain=e_chain, ratio=e / e_chain)
    assert np.all(np.isfinite(gx)) and np.all(gxpad == 0)
    assert e <= K.DENSE_GATE * e_chain, "input gradient %dto%d: normalised error %.3g is %.2f x the fp32 chain's %.3g" % (cin, cout, e, e / e_chain, e_chain)


# ------------------------------------------------------------------------------------------------ the whole net
@functools.lru_cache(maxsize=None)
def _fixture():
    v = dict(np.load(os.path.join(HERE, "golden", "lpips_vectors.npz")))
    v["grad_input"] = np.load(os.path.join(HERE, "golden", "lpips_vectors_grad.npz"))["grad_input"]
    return v


@functools.lru_cache(maxsize=None)
def _full():
    """The fixture's state, its inputs, and the fp32 CPU restatement's gradient on them (the budget)."""
    from wmar_amd.lpips import LPIPS
    from wmar_amd.utils.synth import synth_lpips_state
    v = _fixture()
    state = synth_lpips_state(seed=int(v["seed"]))
    h = hashlib.sha256()
    for k in state:
        h.update(k.encode())
        h.update(state[k].numpy().tobytes())
    assert h.hexdigest() == str(v["weights_sha256"]), "synth_lpips_state drifted from the fixture's weights: regenerate the fixture"
    x, t = torch.from_numpy(v["input"]), torch.from_numpy(v["target"])
    _, _, g32, _ = LR.value_and_grad(state, x, t, torch.float32)
    return LPIPS(state, resolution=128, max_batch=2), x, t, g32.double()


@functools.lru_cache(maxsize=None)
def _narrow():
    from wmar_amd.lpips import LPIPS
    from wmar_amd.utils.synth import synth_lpips_state
    state = synth_lpips_state(NARROW, seed=1)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 3, 128, 128, generator=g) * 2 - 1
    t = (x + 0.1 * torch.randn(3, 3, 128, 128, generator=g)).clamp(-1, 1)
    gv = torch.rand(3, generator=g) + 0.5
    r64 = LR.value_and_grad(state, x, t, torch.float64, gv)
    r32 = LR.value_and_grad(state, x, t, torch.float32, gv)
    return LPIPS(state, resolution=128, max_batch=4, chns=NARROW), x, t, gv, r64, r32


def _run(lp, x, t, gv=None):
    xd = x.cuda().requires_grad_(True)
    val = lp(xd, t.cuda())
    per_tap = lp.last_per_tap.clone()
    (val.reshape(-1) * (1.0 if gv is None else gv.cuda())).sum().backward()
    return val.detach().reshape(-1), per_tap, xd.grad


def _net_gates(name, val, per_tap, grad, v64, pt64, g64, g32):
    e_v = float(((val.cpu().double() - v64).abs() / v64.abs()).max())
    e_t = float(((per_tap.cpu().double() - pt64).abs() / pt64.abs()).max())
    scale = g64.abs().amax((1, 2, 3))
    e_g = (grad.cpu().double() - g64).abs().amax((1, 2, 3)) / scale
    b_g = (g32 - g64).abs().amax((1, 2, 3)) / scale
    _say("net", name, value_err=e_v, per_tap_err=e_t, grad_err=float(e_g.max()), grad_torch_fp32=float(b_g.max()),
         worst_ratio=float((e_g / b_g).max()))
    assert torch.isfinite(grad).all()
    assert e_v <= VALUE_GATE, "%s: value off by %.3g relative" % (name, e_v)
    assert e_t <= VALUE_GATE, "%s: a per-tap term off by %.3g relative" % (name, e_t)
    assert torch.all(e_g <= NET_GATE * b_g), "%s: input gradient error %s against the fp32 restatement's %s" % (name, e_g.tolist(), b_g.tolist())


def test_full_width_net_against_the_reference_module():
    lp, x, t, g32 = _full()
    v = _fixture()
    val, per_tap, grad = _run(lp, x, t)
    _net_gates("full S=128 B=2", val, per_tap, grad, torch.from_numpy(v["value"]), torch.from_numpy(v["per_tap"]),
               torch.from_numpy(v["grad_input"]), g32)


def test_narrow_net_with_all_zero_feature_vectors():
    lp, x, t, gv, r64, r32 = _narrow()
    assert max(r64[3]) >= 1, "the narrow case must keep covering the all-zero feature vector rule"
    assert torch.isfinite(r64[2]).all()
    xd = x.cuda().requires_grad_(True)
    val = lp(xd, t.cuda())
    per_tap = lp.last_per_tap.clone()
    (val.reshape(-1) * gv.cuda()).sum().backward()
    _net_gates("narrow S=128 B=3 zero_vectors=%s" % r64[3], val.detach().reshape(-1), per_tap, xd.grad, r64[0], r64[1], r64[2], r32[2].double())


def test_two_runs_give_the_same_bits_and_a_replaced_tape_is_refused():
    lp, x, t, gv, _, _ = _narrow()
    a, b = _run(lp, x, t, gv), _run(lp, x, t, gv)
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), "two runs differ"
    xd = x.cuda().requires_grad_(True)
    first = lp(xd, t.cuda())
    second = lp(xd.detach().flip(0).requires_grad_(True), t.cuda())           # replaces the tape
    with pytest.raises(RuntimeError, match="does not belong to the last forward"):
        first.sum().backward()
    with torch.no_grad():
        lp(x.cuda(), t.cuda())                                                 # keeps no tape
    with pytest.raises(RuntimeError, match="does not belong to the last forward"):
        second.sum().backward()
    assert torch.equal(_run(lp, x, t, gv)[2].view(torch.int32), a[2].view(torch.int32)), "the engine stays usable"


def test_engine_refuses_a_backward_without_a_tape_and_bad_shapes():
    import ctypes as C
    from wmar_amd import _lib
    from wmar_amd.lpips import LPIPS
    from wmar_amd.utils.synth import synth_lpips_state
    lp, x, t, gv, _, _ = _narrow()
    with torch.no_grad():
        lp(x.cuda(), t.cuda())
    gi = torch.empty(3, 3, 128, 128, device="cuda")
    g = torch.ones(3, device="cuda")
    with pytest.raises(_lib.WmarError, match="no tape"):
        _lib.check(lp._L.wmar_lpips_backward(lp._h, g.data_ptr(), 3, gi.data_ptr(), _lib.stream_ptr()))
    with pytest.raises(ValueError, match="max_batch"):
        lp(torch.zeros(5, 3, 128, 128, device="cuda"), torch.zeros(5, 3, 128, 128, device="cuda"))
    with pytest.raises(ValueError, match="input` only"):
        lp(x.cuda(), t.cuda().requires_grad_(True))
    with pytest.raises(ValueError, match="multiple of 128"):
        LPIPS(synth_lpips_state(NARROW, seed=1), resolution=192, chns=NARROW)
    cfg = _lib.LpipsConfig()
    for i, c in enumerate(NARROW):
        cfg.chns[i] = c
    cfg.resolution, cfg.max_batch = 64, 1
    h = C.c_void_p()
    names, ptrs, n = _lib.tensor_table({k: v.cuda() for k, v in synth_lpips_state(NARROW, seed=1).items()})
    with pytest.raises(_lib.WmarError, match="multiple of 128"):
        _lib.check(lp._L.wmar_lpips_create(C.byref(cfg), names, ptrs, n, _lib.stream_ptr(), C.byref(h)))
    assert lp.device_bytes > 0


# ------------------------------------------------------------------------------------------------ autograd, rcc_loss, CLI
def test_autograd_fills_the_input_gradient_only():
    lp, x, t, _, r64, _ = _narrow()
    xd, td = x.cuda().requires_grad_(True), t.cuda()
    out = lp(xd, td)
    assert out.shape == (3, 1, 1, 1) and out.requires_grad
    out.sum().backward()
    assert xd.grad is not None and xd.grad.shape == xd.shape and float(xd.grad.abs().max()) > 0 and td.grad is None
    with torch.no_grad():
        assert not lp(xd, td).requires_grad
    assert torch.equal(lp(x.cuda(), td), out.detach())


HARNESS128 = dict(ch=32, ch_mult=(1, 2, 2), num_res_blocks=1, attn_resolutions=(8,), resolution=128, z_channels=16, embed_dim=8, n_embed=16384)


def test_rcc_loss_with_the_reference_regulariser_moves_the_decoder_gradients():
    """The harness Taming shape has resolution 32, below what LPIPS takes: the same shape at 128 x 128, the smallest multiple of 128."""
    from wmar_amd import finetune as ft
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = synth.VQConfig(**HARNESS128)
    sd = synth.synth_vq_state(cfg, 5, "cpu")
    tok = TrainableTokenizer(cfg, {k: v.to("cuda", torch.float32).contiguous() for k, v in sd.items()}, max_batch=2)
    orig = TrainableTokenizer(cfg, {k: (v + 0.01 * torch.randn(v.shape, generator=torch.Generator().manual_seed(1))).to("cuda", torch.float32).contiguous()
                                    for k, v in sd.items()}, max_batch=2)
    lp, _, _, _, _, _ = _narrow()
    idx = torch.randint(0, cfg.n_embed, (2, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(11)).cuda()
    grads, logs = [], []
    for rec in (None, ft.reference_rec_loss(lp, 1.0)):
        for p in tok.parameters():
            p.grad = None
        loss, _, log, _ = ft.rcc_loss(tok, idx, [], p=0.0, loss_weight=1.0, orig=orig, rec_loss=rec)
        loss.backward()
        grads.append({k: p.grad.clone() for k, p in tok.named_parameters("decoder.")})
        logs.append(log)
    assert "rec_loss_perceptual_component" not in logs[0] and logs[1]["rec_loss_perceptual_component"] > 0
    assert abs(logs[1]["rec_loss"] - logs[0]["rec_loss"] - logs[1]["rec_loss_perceptual_component"]) <= 1e-5 * logs[1]["rec_loss"]
    moved = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert len(moved) == len(grads[0]), "every decoder gradient sees the perceptual term"
    assert all(torch.isfinite(g).all() for g in grads[1].values())


def test_finetune_cli_with_synthetic_lpips_is_reproducible_and_differs_from_l1_only(tmp_path):
    """``--synthetic_config harness`` has resolution 32, which LPIPS refuses (a multiple of 128 is needed); the CLI's ``harness128`` is the
    same shape at 128 x 128.  Two optimizer steps, not one: at the first step the trained decoder IS the frozen one, so the regulariser
    and its gradient are exactly 0 with or without LPIPS (the log line says ``rec_loss: 0.0``) and one step cannot tell the runs apart."""
    import finetune as cli
    base = ("--model taming --synthetic --synthetic_config harness128 --dataset_size 4 --batch_size_per_gpu 2 --nb_epochs 1 --augs none "
            "--max_steps 2 --seed 0")
    with pytest.raises(SystemExit, match="multiple of 128"):
        cli.main(f"--model taming --synthetic --synthetic_config harness --synthetic_lpips --max_steps 1 --outdir {tmp_path / 'no'}".split())
    outs = {}
    for name, extra in (("a", "--synthetic_lpips"), ("b", "--synthetic_lpips"), ("l1", "")):
        out = tmp_path / name
        assert cli.main(f"{base} {extra} --outdir {out}".split()) == 0
        outs[name] = {f: open(out / f, "rb").read() for f in ("encoder_ft_delta.pth", "decoder_ft_delta.pth")}
    assert outs["a"] == outs["b"], "two runs with LPIPS write different delta files"
    assert outs["a"]["decoder_ft_delta.pth"] != outs["l1"]["decoder_ft_delta.pth"], "the LPIPS term did not reach the decoder"
