"""GPU: the WAM extractor on the device (wmar_wamx_detect and its probes, wmar_amd/csrc/wam_extractor.h) against what the
reference's own modules computed in float64 (tests/golden/wam_extractor_*.npz) and against the float64 restatement
(tests/wam_extractor_reference.py, itself held to the fixture to 1e-10 by tests/test_wam_extractor_reference.py).

Gates, none of them measured on the code under test.  Whole calls: the device error against the reference's float64 run must stay
within 4 x (rms) and 8 x (max) of the error of the reference's OWN float32 run against that float64 run, as the fixture records it
(``*_preds_err``), on pred_subset; and over the full arrays the sign of every logit must be the recorded one at every pixel that is
not ``near`` (some channel within MARGIN_MULT = 8 x that max error of zero: a device inside its max gate cannot flip a sign outside
that margin; at most NEAR_CAP = 1 % of an image is near).  Stages: bounds derived from the roundings of the stage, in the comments at
each test.  The measured ratios are printed on lines starting WAMEXTRACT.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wam_extractor_cases as XC
from tests import wam_extractor_reference as XR
from wmar_amd.utils import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24                                   # half an ulp of 1 in float32
RMS_GATE, MAX_GATE = 4.0, 8.0
E, P = XR.E, XR.P


@functools.lru_cache(maxsize=None)
def fx():
    return XC.load()


@functools.lru_cache(maxsize=None)
def state(which):
    cfg, seed = (synth.WAMX_SMALL, XC.SMALL_SEED) if which == "small" else (synth.WAMX_RELEASED, XC.RELEASED_SEED)
    return cfg, synth.synth_wamx_state(cfg, seed)


@functools.lru_cache(maxsize=None)
def engine(which, max_batch):
    from wmar_amd.watermarking.wam_extractor import WamExtractor
    cfg, st = state(which)
    return WamExtractor(cfg, st, DEV, max_batch=max_batch)


@functools.lru_cache(maxsize=None)
def images(which):
    cfg, _ = state(which)
    seed, B = (XC.SMALL_SEED, XC.SMALL_B) if which == "small" else (XC.RELEASED_SEED, XC.RELEASED_B)
    return torch.from_numpy(XC.images_norm(seed, B, cfg.img_size)).to(DEV)


@functools.lru_cache(maxsize=None)
def state64():
    return XR.to_dtype(state("small")[1], torch.float64)


def _lib():
    from wmar_amd import _lib
    return _lib, _lib.load()


def nhwc(a, Cs=None):
    """float64 / float32 [B, C, H, W] -> float32 [B, H, W, pad8(C)] on the device, padding channels zero"""
    t = torch.as_tensor(a).permute(0, 2, 3, 1).to(torch.float32)
    C = t.shape[-1]
    Cs = Cs or (C + 7) // 8 * 8
    return F.pad(t, (0, Cs - C)).contiguous().to(DEV)


def gate(tag, got, want64, ref_err):
    """rms <= 4 x, max <= 8 x the reference's own float32 error (max, rms) against the same float64 array"""
    d = np.abs(np.asarray(got, dtype=np.float64) - want64)
    mx, rms = float(d.max()), float(np.sqrt(np.mean(d * d)))
    print(f"WAMEXTRACT {tag}: max {mx:.3g} = {mx / ref_err[0]:.2f} x reference fp32 ({ref_err[0]:.3g}), "
          f"rms {rms:.3g} = {rms / ref_err[1]:.2f} x ({ref_err[1]:.3g})")
    assert rms <= RMS_GATE * ref_err[1], (tag, rms, ref_err[1])
    assert mx <= MAX_GATE * ref_err[0], (tag, mx, ref_err[0])


def within(tag, got, want64, bound):
    d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want64))
    r = float((d / np.maximum(bound, 1e-300)).max())
    print(f"WAMEXTRACT {tag}: max error {float(d.max()):.3g}, at most {r:.3f} of its bound")
    assert np.all(d <= bound), (tag, float(d.max()), r)


# ---------------------------------------------------------------------------------------------------------------- whole calls
def _whole(tag, which, preds, b0=0):
    g = fx()
    cfg, _ = state(which)
    R, n = cfg.img_size, preds.shape[0]
    sub = XC.pred_subset(R)
    got = preds.cpu().numpy()
    assert got.shape == (n, cfg.nbits + 1, R, R) and got.dtype == np.float32
    t = which[0]
    gate(tag, got[:, :, sub, :][:, :, :, sub], g[f"{t}_preds64_sub"][b0:b0 + n], g[f"{t}_preds_err"])
    B = g[f"{t}_near_share"].shape[0]
    signs = np.unpackbits(g[f"{t}_signs"])[:B * (cfg.nbits + 1) * R * R].reshape(B, cfg.nbits + 1, R, R).astype(bool)[b0:b0 + n]
    near = np.unpackbits(g[f"{t}_near"])[:B * R * R].reshape(B, R, R).astype(bool)[b0:b0 + n]
    assert float(near.reshape(n, -1).mean(axis=1).max()) <= XC.NEAR_CAP
    wrong = ((got > 0) != signs) & ~near[:, None]
    print(f"WAMEXTRACT {tag}: {int(((got > 0) != signs).sum())} signs differ in all, {int(wrong.sum())} outside the near pixels "
          f"({near.mean():.4%} of the pixels are near)")
    assert not wrong.any()


@pytest.mark.parametrize("max_batch", [2, 1])
def test_small_detect_against_float64(max_batch):
    # 3 images: groups of 2 + 1, or three of 1
    _whole(f"small mb{max_batch}", "small", engine("small", max_batch).detect(images("small"))["preds"])


def test_released_detect_against_float64():
    _whole("released B1", "released", engine("released", 1).detect(images("released"))["preds"])


# ---------------------------------------------------------------------------------------------------------------- invariance
def test_two_runs_batch_position_and_chunking_change_no_bit():
    x = images("small")
    a = engine("small", 2).detect(x)["preds"]
    assert torch.equal(a, engine("small", 2).detect(x)["preds"])
    # image 1 of the batch of 3 against the single-image call
    assert torch.equal(a[1:2], engine("small", 2).detect(x[1:2])["preds"])
    for mb in (1, 16):
        assert torch.equal(a, engine("small", mb).detect(x)["preds"]), mb


# ---------------------------------------------------------------------------------------------------------------- stages, small
def test_patch_embedding_probe():
    """tokens0 = conv + bias + pos_embed.  K = 3 * 16 * 16 = 768 products summed in float32 in some order: at most (K - 1) roundings of
    partial sums, each below half an ulp of sum |w| |x|, one per product, two for the bias and pos_embed additions, one for the input
    taken from float32 as it is: (K + 4) 2^-24 (sum |w| |x| + |b| + |pos|)."""
    L_, L = _lib()
    cfg, st = state("small")
    x = images("small")
    w, b, pos = (st[E + k].to(DEV).contiguous() for k in ("patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed"))
    g = cfg.grid
    out = torch.full((3, g, g, cfg.embed_dim), -7.0, device=DEV)
    L_.check(L.wmar_wamx_probe_patch_embed(x.data_ptr(), 3, cfg.img_size, cfg.patch_size, w.data_ptr(), b.data_ptr(), pos.data_ptr(),
                                           cfg.embed_dim, out.data_ptr(), L_.stream_ptr(DEV)))
    s64 = state64()
    mag = F.conv2d(x.cpu().double().abs(), s64[E + "patch_embed.proj.weight"].abs(), s64[E + "patch_embed.proj.bias"].abs(),
                   stride=cfg.patch_size).permute(0, 2, 3, 1) + s64[E + "pos_embed"].abs()
    within("patch embedding", out.cpu().numpy(), fx()["s_tokens0"], (3 * cfg.patch_size ** 2 + 4) * EPS * mag.numpy())


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_block_probe(i):
    """Block i (0, 2 windowed; 1, 3 global) from the fixture's tokens before it to the fixture's tokens after it.  A block chains two
    LayerNorms, four Linears, a softmax and a GELU, so its bound is taken the way the whole call's is: the error of the SAME block
    evaluated by PyTorch in float32 on the CPU (the restatement, float32 weights, the same float32 input) against the float64 fixture,
    times 4 (rms) and 8 (max).  Nothing of it comes from the device."""
    L_, L = _lib()
    cfg, st = state("small")
    g = fx()
    x32 = torch.from_numpy(g[f"s_tokens{i}"]).float()
    with torch.no_grad():
        ref32 = XR.block(st, cfg, i, x32).double().numpy()
    d = np.abs(ref32 - g[f"s_tokens{i + 1}"])
    ref_err = (float(d.max()), float(np.sqrt(np.mean(d * d))))
    e = engine("small", 2)
    for b0, n in ((0, 2), (2, 1)):
        xin = x32[b0:b0 + n].contiguous().to(DEV)
        out = torch.full_like(xin, -7.0)
        L_.check(L.wmar_wamx_probe_block(e._h, i, xin.data_ptr(), n, out.data_ptr(), L_.stream_ptr(DEV)))
        gate(f"block {i} images {b0}..{b0 + n - 1}", out.cpu().numpy(), g[f"s_tokens{i + 1}"][b0:b0 + n], ref_err)
    big = torch.zeros(3, cfg.grid, cfg.grid, cfg.embed_dim, device=DEV)
    assert L.wmar_wamx_probe_block(e._h, i, big.data_ptr(), 3, big.data_ptr(), L_.stream_ptr(DEV)) == -1      # above max_batch


def _attn64(q, k, v, rh, rw, g, S):
    """float64 attention of [B, g, g, nh, hd] tensors in windows of S"""
    B, _, _, nh, hd = q.shape
    nw = g // S

    def win(t):
        return t.view(B, nw, S, nw, S, nh, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(B * nw * nw * nh, S * S, hd)
    o = XR.attention_core(win(q), win(k), win(v), rh, rw, S)
    return o.view(B, nw, nw, nh, S, S, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, g, g, nh * hd)


@pytest.mark.parametrize("g,S,nh,hd,qscale", [(8, 4, 3, 32, 1.0), (8, 8, 3, 32, 1.0), (16, 16, 2, 64, 1.0), (16, 8, 2, 64, 1.0),
                                              (8, 8, 3, 32, 30.0), (16, 16, 2, 64, 30.0)])
def test_attention_probe(g, S, nh, hd, qscale):
    """Windowed (16 tokens) and global (64 tokens) at head width 32, global (256 tokens) and windowed (64) at head width 64, on random
    q, k, v; q scaled by 30 makes scores of +-100 and more, where a softmax without max subtraction overflows.
    Each score is three float32 dot products of hd terms (q k scaled, q Rh, q Rw) and two additions: its absolute error is at most
    ds = (hd + 4) 2^-24 (|q| . |k| scale + |q| . |Rh| + |q| . |Rw|), maximised over the keys of a query.  exp (2 ulp), the sum of N
    terms and the division give each weight a relative error of at most 2 ds + (N + 6) 2^-24 -- the error of the maximum cancels between
    numerator and denominator -- and the product with V adds N more roundings: |do| <= (2 ds + (2 N + 8) 2^-24) sum_j p_j |v_j|."""
    L_, L = _lib()
    B, D = 2, nh * hd
    rng = np.random.Generator(np.random.PCG64(100 + g + S + hd))
    qkv = torch.from_numpy(rng.standard_normal((B, g, g, 3, nh, hd)).astype(np.float32))
    qkv[:, :, :, 0] *= qscale
    rh = torch.from_numpy((0.2 * rng.standard_normal((2 * S - 1, hd))).astype(np.float32))
    rw = torch.from_numpy((0.2 * rng.standard_normal((2 * S - 1, hd))).astype(np.float32))
    out = torch.full((B, g, g, D), -7.0, device=DEV)
    dq, dh, dw = qkv.reshape(B, g, g, 3 * D).contiguous().to(DEV), rh.to(DEV), rw.to(DEV)
    L_.check(L.wmar_wamx_probe_attn(dq.data_ptr(), B, g, S, nh, hd, dh.data_ptr(), dw.data_ptr(), out.data_ptr(), L_.stream_ptr(DEV)))
    q, k, v = (qkv[:, :, :, j].double() for j in range(3))
    want = _attn64(q, k, v, rh.double(), rw.double(), g, S)
    # the scores' error from magnitudes, maximised over the keys; sum_j p_j |v_j| replaced by max_j |v_j| of the window
    N = S * S
    qa = q.abs().view(B, g // S, S, g // S, S, nh, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, N, hd)
    ka = k.abs().view(B, g // S, S, g // S, S, nh, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, N, hd)
    va = v.abs().view(B, g // S, S, g // S, S, nh, hd).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, N, hd)
    s_mag = (qa @ ka.transpose(-2, -1)).amax(dim=-1) * hd ** -0.5 + (qa @ rh.double().abs().t()).amax(dim=-1) + (qa @ rw.double().abs().t()).amax(dim=-1)
    ds = (hd + 4) * EPS * s_mag                                                    # [windows, N]
    bound = (2 * ds + (2 * N + 8) * EPS)[:, :, None] * va.amax(dim=1, keepdim=True)  # sum_j p_j |v_j| <= max_j |v_j|
    bound = bound.view(B, g // S, g // S, nh, S, S, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, g, g, D)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    within(f"attention g{g} S{S} hd{hd} q x{qscale:g}", got, want.numpy(), bound.numpy())


@pytest.mark.parametrize("C", [96, 12])
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_layernorm_probe(C, eps):
    """(mean, rstd) per token; rows of tiny variance (a constant + 1e-4 noise: variance 1e-8, where eps 1e-5 and 1e-6 give 316 and 995)
    and ordinary rows.  The sums are float64 over float32 inputs, so what remains is the cancellation in E[x^2] - mean^2 -- the two
    sums carry at most C roundings of 2^-53 of E[x^2] each, relative to (variance + eps) -- and the roundings of the result to float32
    and of its reciprocal square root (three Newton steps in float64): mean within 2 * 2^-24 |mean|, rstd within
    (4 * 2^-24 + 2 C 2^-53 E[x^2] / (variance + eps)) rstd.  C = 12 is stored in 16 channels; the padding holds zeros and is not counted."""
    L_, L = _lib()
    rng = np.random.Generator(np.random.PCG64(7 + C))
    n = 37
    x = rng.standard_normal((n, C))
    x[:12] = rng.uniform(-2, 2, (12, 1)) + 1e-4 * rng.standard_normal((12, C))
    x = x.astype(np.float32)
    Cs = (C + 7) // 8 * 8
    xd = F.pad(torch.from_numpy(x), (0, Cs - C)).contiguous().to(DEV)
    mr = torch.full((n, 2), -7.0, device=DEV)
    L_.check(L.wmar_wamx_probe_layernorm(xd.data_ptr(), n, C, eps, mr.data_ptr(), L_.stream_ptr(DEV)))
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=1)
    var = ((x64 - mean[:, None]) ** 2).mean(axis=1)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    got = mr.cpu().numpy()
    within(f"layernorm C{C} eps{eps:g} mean", got[:, 0], mean, 2 * EPS * np.abs(mean) + 1e-30)
    within(f"layernorm C{C} eps{eps:g} rstd", got[:, 1], rstd, (4 * EPS + 2 * C * 2.0 ** -53 * (x64 ** 2).mean(axis=1) / (var + eps)) * rstd)
    if eps == 1e-6:        # the two eps differ visibly on the tiny-variance rows
        assert np.all(got[:12, 1] > 900.0) and np.all(got[:12, 1] < 1000.0)
    else:
        assert np.all(got[:12, 1] > 310.0) and np.all(got[:12, 1] < 317.0)


def _upstage(x_nchw, w, f, gamma=None, beta=None, gelu=0):
    L_, L = _lib()
    B, Cin, Hs, _ = x_nchw.shape
    Cout = w.shape[0]
    xd, wd = nhwc(x_nchw), w.to(torch.float32).contiguous().to(DEV)
    out = torch.full((B, Hs * f, Hs * f, (Cout + 7) // 8 * 8), -7.0, device=DEV)
    gd = gamma.float().contiguous().to(DEV) if gamma is not None else None
    bd = beta.float().contiguous().to(DEV) if beta is not None else None
    L_.check(L.wmar_wamx_probe_upstage(xd.data_ptr(), B, Hs, Cin, f, gd.data_ptr() if gd is not None else None,
                                       bd.data_ptr() if bd is not None else None, gelu, wd.data_ptr(), Cout, out.data_ptr(), L_.stream_ptr(DEV)))
    out = out.cpu()
    assert bool((out[..., Cout:] == 0).all())                 # the padding channels
    return out[..., :Cout].permute(0, 3, 1, 2).numpy()


def _up64(x, f):
    return F.pad(XR.upsample_bilinear(x, f), (1, 1, 1, 1), mode="reflect")


@pytest.mark.parametrize("f", [4, 2])
def test_upsample_probe_ramp_and_corner_are_exact(f):
    """A linear ramp with integer slopes and an image that is zero except one corner pixel: every interpolated value is a multiple of
    1 / 64 below 2^10, so products and sums are exact in float32 whatever their order, and a conv whose weight is one 1 in one tap
    copies the upsampled, reflected tensor: the device must return the float64 values EXACTLY.  A wrong half-pixel offset moves the
    ramp by a fraction of its slope, a reflection off by one shows in the first and last row and column of the edge taps."""
    H, C = 8, 8
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
    x = torch.zeros(2, C, H, H, dtype=torch.float64)
    for c in range(C):
        x[0, c] = (c + 1) * yy - (2 * c + 1) * xx + c
    x[1, :, 0, 0] = torch.arange(1, C + 1, dtype=torch.float64)            # one corner pixel, another value per channel
    x[1, :, H - 1, H - 1] = -8.0
    u = _up64(x, f)
    # in the interior the ramp's upsampled value is the ramp at the source coordinate (d + 0.5) / f - 0.5
    d = torch.arange(f, H * f - f, dtype=torch.float64)
    src = (d + 0.5) / f - 0.5
    assert torch.equal(u[0, 2, 1 + f:1 + H * f - f, 1 + f:1 + H * f - f], 3 * src[:, None] - 5 * src[None, :] + 2)
    for tap in ((1, 1), (0, 0), (2, 2), (0, 2), (2, 1)):
        w = torch.zeros(C, C, 3, 3, dtype=torch.float64)
        for c in range(C):
            w[c, (c + 3) % C, tap[0], tap[1]] = 1.0                         # output channel c copies input channel c + 3 at this tap
        want = F.conv2d(u, w).numpy()
        got = _upstage(x, w, f)
        assert np.array_equal(got.astype(np.float64), want), (f, tap, float(np.abs(got - want).max()))


def _conv_bound(u64, w64, extra):
    """(K + extra) 2^-24 sum |w| |u| of a 3 x 3 conv on the padded tensor u64: K = 9 Cin float32 products in some order"""
    K = 9 * w64.shape[1]
    return (K + extra) * EPS * F.conv2d(u64.abs(), w64.abs())


def _ln_gelu_after(tag, raw, e_raw, gamma, beta, want64):
    """The stage's own LayerNorm(eps 1e-6) + GELU, which the device leaves to the next conv, applied here in float64 to the device's raw
    conv output; e_raw bounds the raw error per element.  y = g (r - u) / sd + b: an error e on every channel moves r - u by at most
    2 max e and sd by at most max e, so |dy| <= |g| / sd (2 + |r - u| / sd) max_c e; GELU's slope is below 1.13."""
    r = torch.from_numpy(raw).double()
    got = XR.gelu(XR.layer_norm_cf(r, gamma, beta, 1e-6))
    u = r.mean(1, keepdim=True)
    sd = torch.sqrt(((r - u) ** 2).mean(1, keepdim=True) + 1e-6)
    bound = 1.13 * gamma.abs()[None, :, None, None] / sd * (2 + (r - u).abs() / sd) * e_raw.amax(dim=1, keepdim=True)
    within(tag, got.numpy(), want64, bound.numpy())


def test_upstage_probe_on_the_fixture_stages():
    """neck -> up0 (factor 4, 96 -> 24 channels, three images), up0 -> up1 (factor 2, 24 -> 12, image 0), up1 -> up2 (factor 2, 12 -> 6:
    stored in 16 and 8 channels).  The input is the fixture's float64 array rounded to float32 (one rounding); an interpolated value is
    four products and three sums of values below max |x|: 8 roundings at most; the conv as _conv_bound: (9 Cin + 10) 2^-24 sum |w| |u|."""
    g, s64 = fx(), state64()
    chain = [("s_neck", "s_up0", 4, slice(0, 3)), ("s_up0", "s_up1_img0", 2, slice(0, 1)), ("s_up1_img0", "s_up2_img0", 2, slice(0, 1))]
    for j, (src, dst, f, sl) in enumerate(chain):
        p = f"{P}output_upscaling.{j}.upsample_block."
        x = torch.from_numpy(g[src])[sl]
        w = s64[p + "2.weight"]
        raw = _upstage(x, w, f)
        _ln_gelu_after(f"upscaling stage {j} (x{f}, {w.shape[1]} -> {w.shape[0]})", raw, _conv_bound(_up64(x, f), w, 10), s64[p + "3.weight"],
                       s64[p + "3.bias"], g[dst][sl] if dst == "s_up0" else g[dst])


def test_upstage_probe_normalises_its_input_while_staging():
    """The form the engine runs: the previous stage's RAW conv output, its LayerNorm + GELU applied to the four source pixels of every
    patch pixel.  Stage 1 on the float64 restatement's raw stage-0 output of image 0.  On top of the bound above, the staged value
    carries the float32 LayerNorm (mean and rstd good to 4 * 2^-24 of themselves, see the probe above; (x - u) rstd g + b: four more
    roundings; |x - u| rstd <= sqrt(C); the input rounded to float32 once) and erff (4 ulp): below (12 + 4 sqrt(C)) 2^-24
    (|g| sqrt(C) + |b|) per value, and the conv sums 9 Cin of them weighted by |w|."""
    g, s64 = fx(), state64()
    p0, p1 = f"{P}output_upscaling.0.upsample_block.", f"{P}output_upscaling.1.upsample_block."
    neck = torch.from_numpy(g["s_neck"])[:1]
    raw0 = F.conv2d(_up64(neck, 4), s64[p0 + "2.weight"])                     # float64, before LayerNorm + GELU
    assert float((XR.gelu(XR.layer_norm_cf(raw0, s64[p0 + "3.weight"], s64[p0 + "3.bias"])) - torch.from_numpy(g["s_up0"])[:1]).abs().max()) < 1e-10
    w = s64[p1 + "2.weight"]
    raw1 = _upstage(raw0, w, 2, s64[p0 + "3.weight"], s64[p0 + "3.bias"], gelu=1)
    C = raw0.shape[1]
    stage_err = float((12 + 4 * C ** 0.5) * EPS * (s64[p0 + "3.weight"].abs().max() * C ** 0.5 + s64[p0 + "3.bias"].abs().max()))
    u = _up64(torch.from_numpy(g["s_up0"])[:1], 2)
    e_raw = _conv_bound(u, w, 10) + stage_err * F.conv2d(torch.ones_like(u), w.abs())
    _ln_gelu_after("upscaling stage 1 with LayerNorm + GELU while staging", raw1, e_raw, s64[p1 + "3.weight"], s64[p1 + "3.bias"], g["s_up1_img0"])


def test_last_layer_probe():
    """up2 of image 0 (6 channels, stored in 8) -> the 33 logits, NCHW: 6 products, a bias, the input rounded once: (6 + 3) 2^-24
    (sum |w| |x| + |b|).  Compared on pred_subset with the fixture, and in full with the float64 restatement of the layer."""
    L_, L = _lib()
    g, s64 = fx(), state64()
    cfg, st = state("small")
    x = torch.from_numpy(g["s_up2_img0"])
    R, C, n = cfg.img_size, x.shape[1], cfg.nbits + 1
    w, b = st[P + "last_layer.weight"].contiguous().to(DEV), st[P + "last_layer.bias"].contiguous().to(DEV)
    xd = nhwc(x)
    out = torch.full((1, n, R, R), -7.0, device=DEV)
    L_.check(L.wmar_wamx_probe_last(xd.data_ptr(), 1, R, C, None, None, 0, w.data_ptr(), b.data_ptr(), n, out.data_ptr(), L_.stream_ptr(DEV)))
    want = XR.last_layer(s64, x)
    bound = (C + 3) * EPS * F.conv2d(x.abs(), s64[P + "last_layer.weight"].abs(), s64[P + "last_layer.bias"].abs())
    got = out.cpu().numpy()
    within("last layer (restatement, in full)", got, want.numpy(), bound.numpy())
    sub = XC.pred_subset(R)
    within("last layer (fixture subset)", got[:, :, sub, :][:, :, :, sub], g["s_preds64_sub"][:1], bound.numpy()[:, :, sub, :][:, :, :, sub] + 1e-10)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_a_wrong_size_is_refused_and_the_output_untouched():
    L_, L = _lib()
    e = engine("small", 2)
    with pytest.raises(ValueError, match=r"128 x 128.*64, 64"):
        e.detect(torch.zeros(1, 3, 64, 64, device=DEV))
    with pytest.raises(ValueError, match="GPU"):
        e.detect(torch.zeros(1, 3, 128, 128))
    sentinel = 123.25
    out = torch.full((1, 33, 128, 128), sentinel, device=DEV)
    small = torch.zeros(1, 3, 64, 64, device=DEV)
    assert L.wmar_wamx_detect(e._h, small.data_ptr(), 1, 64, out.data_ptr(), L_.stream_ptr(DEV)) == -1
    assert b"64 x 64" in L.wmar_last_error() and b"128 x 128" in L.wmar_last_error()
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


@pytest.mark.parametrize("bad,text", [
    (dict(window_size=3), "no multiple of window_size"),                   # a grid of 8 in windows of 3: needs window padding
    (dict(img_size=64), "8 x 8 conv tile"),                                # a grid of 4
    (dict(num_heads=5), "not divisible by num_heads"),
    (dict(num_heads=1), "head width 96"),                                  # above what the attention kernel takes
    (dict(out_chans=104), "not divisible by the product of the stages"),
    (dict(nbits=65), "1..64"),
])
def test_create_refuses_with_a_text(bad, text):
    from wmar_amd._lib import WmarError
    from wmar_amd.watermarking.wam_extractor import WamExtractor
    cfg = dataclasses.replace(synth.WAMX_SMALL, **bad)
    with pytest.raises(WmarError, match=text):
        WamExtractor(cfg, synth.synth_wamx_state(cfg, 0), DEV, max_batch=2)


def test_create_refuses_a_missing_tensor_and_an_interpolated_table():
    from wmar_amd._lib import WmarError
    from wmar_amd.watermarking.wam_extractor import WamExtractor
    cfg, st = state("small")
    less = {k: v for k, v in st.items() if k != E + "blocks.2.mlp.lin1.bias"}
    with pytest.raises(WmarError, match=r"image_encoder\.blocks\.2\.mlp\.lin1\.bias.*missing"):
        WamExtractor(cfg, less, DEV, max_batch=2)
    longer = dict(st)
    longer[E + "blocks.1.attn.rel_pos_w"] = torch.zeros(27, cfg.head_dim)       # a table made for a 14 x 14 grid
    with pytest.raises(ValueError, match=r"rel_pos_w.*2 S - 1 = 15 rows"):
        WamExtractor(cfg, longer, DEV, max_batch=2)


# ---------------------------------------------------------------------------------------------------------------- composition
class _Through:
    """A WAM-like object whose detect is the device extractor: what the existing remove_sync is run with"""

    def __init__(self, e):
        self.e = e

    def detect(self, imgs):
        return self.e.detect(imgs)


def test_remove_sync_with_the_extractor_equals_the_same_call_through_wam():
    from wmar_amd.watermarking.synchronization import WamSync
    e = engine("small", 2)
    pm1 = torch.from_numpy(np.clip(XC.WC.images_pm1(XC.SMALL_SEED, 3, 128), -1, 1)).to(DEV)
    a = WamSync(None, DEV, wam=object(), extractor=e).remove_sync(pm1, return_info=True)
    b = WamSync(None, DEV, wam=_Through(e)).remove_sync(pm1, return_info=True)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])
    assert a[0].shape == pm1.shape


def test_sync_natives_from_a_synthetic_checkpoint_without_a_checkout(tmp_path):
    """--sync true --sync_embedder native --sync_extractor native: both networks from the checkpoint's tensors; nothing of a WAM
    checkout can be imported."""
    import importlib
    import generate
    from wmar_amd import cli
    from wmar_amd.watermarking.wam_extractor import WamExtractor
    # the embedder read from a checkpoint works at 256 x 256: the small extractor's widths on a 16 x 16 grid (global blocks of 256 tokens)
    cfg = dataclasses.replace(synth.WAMX_SMALL, img_size=256)
    st = synth.synth_wamx_state(cfg, 4)
    ckpt = {"embedder." + k: v for k, v in synth.synth_wam_state(synth.WAM_RELEASED, 3).items()}
    ckpt.update({"detector." + k: v for k, v in st.items()})
    path = tmp_path / "wam_mit_synth.pth"
    torch.save(ckpt, path)
    with pytest.raises(ImportError):
        importlib.import_module("deps.watermark_anything.utils.inference_utils")
    args = generate.get_parser().parse_args(["--sync", "true", "--syncpath", str(path), "--sync_embedder", "native", "--sync_extractor", "native"])
    generate.check_wm_args(args)
    mgr = cli.build_sync_manager(args, DEV)
    assert mgr.sync.extractor.cfg == cfg and mgr.sync.embedder.cfg == synth.WAM_RELEASED and mgr.sync._wam is None
    pm1 = torch.from_numpy(XC.WC.images_pm1(XC.SMALL_SEED, 2, 256)).to(DEV)
    out = mgr.add_sync(pm1)
    back = mgr.remove_sync(out)
    assert out.shape == pm1.shape and back.shape == pm1.shape and mgr.sync._wam is None
    x = mgr.sync.normalize(out)
    assert torch.equal(mgr.sync.extractor.detect(x)["preds"], WamExtractor(cfg, st, DEV, max_batch=2).detect(x)["preds"])
