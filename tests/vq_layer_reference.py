"""Float64 references for single VQGAN layers, and the accuracy yardsticks the layer tests gate on (tests/test_gpu_vq_layers.py).

Conventions are the engine's (wmar_amd/csrc/vqgan.hip, deps/taming/modules/diffusionmodules/model.py): 3 x 3 stride 1 pads 1 on every
side; stride 2 pads (0, 1, 0, 1) -- right and bottom only; `up` doubles the input by nearest-neighbour repetition in front of the
conv; GroupNorm has 32 groups and eps 1e-6; the attention core is softmax(q k^T C^-1/2) v.  Everything is written out in plain
numpy: tests/test_vq_layer_reference.py pins it against torch.nn.functional in float64 on the CPU.

The yardstick for a convolution is a sequential fp32 multiply-add chain over the K = Cin ks^2 products of an output (tap-major,
channels inside), restated as in tests/test_bx_split_math.py: fp64 multiply-add, rounded to fp32 after every step.  Errors are
normalised by sum|w x| + |bias| + |res|, the quantity a rounding-error bound of a contraction is proportional to."""
import numpy as np

F64 = np.float64
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ references (float64, NCHW)
def _prepare(x, ks, stride, up):
    x = np.asarray(x, dtype=F64)
    if up:
        x = x.repeat(2, axis=2).repeat(2, axis=3)
    if ks == 3 and stride == 1:
        x = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    elif stride == 2:
        x = np.pad(x, ((0, 0), (0, 0), (0, 1), (0, 1)))
    return x


def _out_size(x, ks, stride, up):
    H, W = x.shape[2] * (2 if up else 1), x.shape[3] * (2 if up else 1)
    return (H // 2, W // 2) if stride == 2 else (H, W)


def conv2d(x, w, bias=None, res=None, stride=1, up=False):
    """x [B, Cin, H, W], w [Cout, Cin, ks, ks] -> [B, Cout, Ho, Wo] in float64."""
    w = np.asarray(w, dtype=F64)
    ks = w.shape[2]
    Ho, Wo = _out_size(x, ks, stride, up)
    xp = _prepare(x, ks, stride, up)
    y = np.zeros((xp.shape[0], w.shape[0], Ho, Wo), dtype=F64)
    for dy in range(ks):
        for dx in range(ks):
            win = xp[:, :, dy:dy + stride * Ho:stride, dx:dx + stride * Wo:stride]
            y += np.einsum("bchw,oc->bohw", win, w[:, :, dy, dx])
    if bias is not None:
        y += np.asarray(bias, dtype=F64)[None, :, None, None]
    if res is not None:
        y += np.asarray(res, dtype=F64)
    return y


def conv2d_abs(x, w, bias=None, res=None, stride=1, up=False):
    """sum |w x| + |bias| + |res| per output: the denominator of the normalised error."""
    return conv2d(np.abs(x), np.abs(w), None if bias is None else np.abs(bias), None if res is None else np.abs(res), stride, up)


def group_stats(x):
    """x [B, C, H, W] -> (mean, rstd) [B, 32] of GroupNorm(32, eps 1e-6) in float64 (biased variance)."""
    x = np.asarray(x, dtype=F64)
    B, C = x.shape[:2]
    g = x.reshape(B, 32, -1)
    mean = g.mean(-1)
    var = ((g - mean[..., None]) ** 2).mean(-1)
    return mean, 1.0 / np.sqrt(var + 1e-6)


def group_norm(x, gamma, beta, swish):
    x = np.asarray(x, dtype=F64)
    B, C = x.shape[:2]
    mean, rstd = group_stats(x)
    cpg = C // 32
    m = np.repeat(mean, cpg, axis=1)[:, :, None, None]
    r = np.repeat(rstd, cpg, axis=1)[:, :, None, None]
    y = (x - m) * r * np.asarray(gamma, dtype=F64)[None, :, None, None] + np.asarray(beta, dtype=F64)[None, :, None, None]
    if swish:
        y = y / (1.0 + np.exp(-y))
    return y


def attention(q, k, v):
    """q, k, v [B, N, C] -> softmax(q k^T C^-1/2) v in float64."""
    q, k, v = (np.asarray(t, dtype=F64) for t in (q, k, v))
    s = np.einsum("bic,bjc->bij", q, k) * (q.shape[-1] ** -0.5)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bij,bjc->bic", p, v)


def sq_distances(z, e):
    """z [P, E], e [N, E] -> |z - e|^2 [P, N] in float64, as the sum of squared differences (no cancellation)."""
    z, e = np.asarray(z, dtype=F64), np.asarray(e, dtype=F64)
    out = np.empty((z.shape[0], e.shape[0]), dtype=F64)
    for i in range(0, z.shape[0], 64):
        d = z[i:i + 64, None, :] - e[None, :, :]
        out[i:i + 64] = (d * d).sum(-1)
    return out


# ------------------------------------------------------------------------------------------------ yardstick: sequential fp32 chain
def conv2d_chain(x, w, bias=None, res=None, stride=1, up=False):
    """The same convolution as ONE sequential fp32 fused-multiply-add chain per output (taps outside, input channels inside), then
    + bias, + res, each rounded to fp32.  x, w, bias, res are fp32 values."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    ks = w.shape[2]
    Ho, Wo = _out_size(x, ks, stride, up)
    xp = _prepare(x, ks, stride, up)                       # float64 copies of fp32 values
    acc = np.zeros((xp.shape[0], Ho, Wo, w.shape[0]), dtype=np.float32)
    for dy in range(ks):
        for dx in range(ks):
            win = xp[:, :, dy:dy + stride * Ho:stride, dx:dx + stride * Wo:stride]
            for c in range(w.shape[1]):
                acc = (acc.astype(F64) + win[:, c, :, :, None] * w[None, None, None, :, c, dy, dx].astype(F64)).astype(np.float32)
    if bias is not None:
        acc = (acc.astype(F64) + np.asarray(bias, dtype=np.float32).astype(F64)).astype(np.float32)
    y = acc.transpose(0, 3, 1, 2)
    if res is not None:
        y = (y.astype(F64) + np.asarray(res, dtype=np.float32).astype(F64)).astype(np.float32)
    return np.ascontiguousarray(y)


def normalised_error(y, exact, denom):
    """max |y - exact| / denom over the outputs with a non-zero denominator (an output that sees only padding is exactly 0)."""
    y, exact, denom = np.asarray(y, dtype=F64), np.asarray(exact, dtype=F64), np.asarray(denom, dtype=F64)
    ok = denom > 0
    return float((np.abs(y - exact)[ok] / denom[ok]).max())


# ------------------------------------------------------------------------------------------------ CPU model of the bf16-piece kernels
def bf16_rne(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    h = bf16_rne(x)
    r = (x - h).astype(np.float32)
    m = bf16_rne(r)
    return h, m, bf16_rne((r - m).astype(np.float32))


# accumulation order of k_conv_bx (WMAR_CONVBX_ROUND6): the small products first; names are (weight piece, input piece)
BX_PRODUCTS = ("lh", "hl", "mm", "mh", "hm", "hh")


def bx_model_dot(x, w, drop=None):
    """Dot products [N, K] as k_conv_bx accumulates them: per 16 products, six piece products (each exact in fp32), every one of the
    six MFMA results added into the fp32 accumulator with one rounding.  drop = one of BX_PRODUCTS: a kernel that forgets that
    product (what the layer tests must catch)."""
    xs = dict(zip("hml", (p.astype(F64) for p in split3(x))))
    ws = dict(zip("hml", (p.astype(F64) for p in split3(w))))
    acc = np.zeros(np.asarray(x).shape[0], dtype=np.float32)
    K = np.asarray(x).shape[1]
    for k0 in range(0, K, 16):
        for name in BX_PRODUCTS:
            if name == drop:
                continue
            part = (ws[name[0]][:, k0:k0 + 16] * xs[name[1]][:, k0:k0 + 16]).sum(-1)
            acc = (acc.astype(F64) + part).astype(np.float32)
    return acc


def chain_dot(x, w):
    """Sequential fp32 multiply-add chain of dot products [N, K]."""
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    acc = np.zeros(x.shape[0], dtype=np.float32)
    for k in range(x.shape[1]):
        acc = (acc.astype(F64) + x[:, k].astype(F64) * w[:, k].astype(F64)).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------ test operands
def full_significand(rng, n, lo=-20, hi=20):
    """fp32 values with all 24 significand bits in use (odd last bit), both signs, magnitudes 2^lo .. 2^hi."""
    mant = (rng.integers(1 << 22, 1 << 23, n, dtype=np.int64) * 2 + 1).astype(F64)          # odd 24-bit integers
    v = mant * 2.0 ** -23 * 2.0 ** rng.integers(lo, hi, n).astype(F64) * rng.choice([-1.0, 1.0], n)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(F64), v)
    return out


def bf16_exact(rng, n, lo=-20, hi=20):
    """fp32 values that are exactly representable in bf16 (8 significand bits), both signs, magnitudes 2^lo .. 2^hi."""
    mant = rng.integers(128, 256, n).astype(F64)
    v = mant * 2.0 ** -7 * 2.0 ** rng.integers(lo, hi, n).astype(F64) * rng.choice([-1.0, 1.0], n)
    return v.astype(np.float32)


def realistic_activations(rng, shape):
    """swish of a normal variable (the spread a ResnetBlock's conv sees) with a few values at 2^+-20."""
    a = rng.standard_normal(shape)
    a = (a / (1.0 + np.exp(-a))).astype(np.float32)
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, size=max(2, flat.size // 2000), replace=False)
    flat[idx[::2]] = np.float32(2.0 ** 20) * rng.choice([-1.0, 1.0], idx[::2].size).astype(np.float32)
    flat[idx[1::2]] = np.float32(2.0 ** -20) * rng.choice([-1.0, 1.0], idx[1::2].size).astype(np.float32)
    return a
