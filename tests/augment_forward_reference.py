"""References for the FORWARD of the device transforms (wmar_augment: k_aug_blur, k_aug_point<op>; wmar_amd/csrc/augment.hip), in plain
numpy / torch on the CPU.  Shared by tests/test_augment_forward_reference.py (CPU) and tests/test_gpu_augment_forward.py; the two old
rotation assertions (tests/test_augmentations_algorithms.py, tests/test_gpu_augment_kernels.py) use the rotation rule as well.

The launch computes  out = S(clamp(T(R(x))))  with R(x) = x / 2 + 0.5 and S(c) = 2 c - 1 in `pm1` mode (identities otherwise); the clamp
is there always in `pm1` mode and otherwise for blur, noise and brightness.  Three kinds of yardstick:

  * FLOAT64 references of T: the rotation index map (`rotation_map64`), the blur (`blur64`) and the antialiased resize (`resize64`,
    weights `aa_weights`).  Nothing here is tuned to a kernel.
  * FLOAT32 MODELS, one per kernel, written from the kernel's own expressions (`model`).  They are a second yardstick for the summing
    transforms (`c_chain`: one sequential fp32 summation of the same taps), the bit-exact expectation for the pointwise transforms, and --
    with a `fault` planted -- the subject of the CPU mutation check, which shows that the gates below can see a subtle error.
  * GATES (`gate_rotation`, `gate_stencil`, `gate_pointwise`): what a forward must satisfy.  They take a callable
    `run(op, x, p0, p1, noise, pm1) -> float32 array`, which is a model on the CPU and the kernel launch on the GPU.

Rotation rule.  With (fx, fy) the float64 source coordinates of an output pixel, the pixel is DECIDABLE unless fx or fy lies within
delta = 4 (H + W) 2^-24 of a half-integer.  delta covers the fp32 evaluation of the map: two products of magnitude <= max(H, W) / 2 with
coefficients rounded to float and three additions at magnitude <= max(H, W), about 2.5 (H + W) 2^-24 together; 4 leaves a margin.  A
decidable pixel must equal the float64 map exactly; an undecidable one must take one of the candidate sources on either side of the
boundary (fill where a candidate lies outside).

Error constant of a summing transform.  `smallest_c(got, t64, A)` is the smallest c with |got - t64| <= c 2^-24 A per pixel, A the
float64 transform applied to |u| (the sum of w |u| of that pixel); where A is 0 the two must agree exactly."""
import functools
import math

import numpy as np
import torch

from wmar_amd.augmentations.geometric import resize_bilinear
from wmar_amd.augmentations.valuemetric import gaussian_blur

IDENTITY, BLUR, NOISE, BRIGHTNESS, ROTATE, FLIP_H, CROP_RESIZE, CROP_PAD = range(8)
CLAMPING = (BLUR, NOISE, BRIGHTNESS)        # the transforms that clamp without pm1
F32 = np.float32
EPS = 2.0 ** -24
BC = (2, 3)                                 # planes of every case: 2 x 3, different content per plane

SWEEP_ANGLES = (-20, -15, -10, -5, 5, 10, 15, 20)       # the rotation entries of the AugmentationManager table (0 is the identity)
SWEEP_RESTS = (5, 10, 15, 20, 70, 75, 80, 85)           # their remainders: -20 = three quarter turns + 70


def clamps(op, pm1):
    return bool(pm1) or op in CLAMPING


# ---------------------------------------------------------------------------------------------------------------- rotation, float64
def rotation_delta(H, W):
    return 4.0 * (H + W) * EPS


def rotation_map64(H, W, quarters, rest):
    """(imap, undecidable, cands) of `quarters` counter-clockwise quarter turns followed by a rotation by `rest` degrees, on the canvas
    after the quarter turns: imap[y, x] is the 1-based raster index of the ORIGINAL pixel that output (y, x) shows, 0 for fill;
    cands[y, x, :] are the four (per axis: lower / upper neighbour of the boundary) candidates of an undecidable pixel, all equal to
    imap where the pixel is decidable."""
    base = np.rot90(np.arange(1, H * W + 1, dtype=np.int64).reshape(H, W), quarters % 4)
    Hc, Wc = base.shape
    if rest == 0:
        return base.copy(), np.zeros((Hc, Wc), bool), np.repeat(base[..., None], 4, axis=-1)
    th = math.radians(rest)
    c, s = math.cos(th), math.sin(th)
    dx = np.arange(Wc, dtype=np.float64)[None, :] + 0.5 - 0.5 * Wc
    dy = np.arange(Hc, dtype=np.float64)[:, None] + 0.5 - 0.5 * Hc
    fx = c * dx - s * dy + Wc / 2 - 0.5
    fy = s * dx + c * dy + Hc / 2 - 0.5

    def pick(ix, iy):
        ix, iy = ix.astype(np.int64), iy.astype(np.int64)
        inside = (ix >= 0) & (ix < Wc) & (iy >= 0) & (iy < Hc)
        return np.where(inside, base[np.clip(iy, 0, Hc - 1), np.clip(ix, 0, Wc - 1)], 0)

    delta = rotation_delta(H, W)
    ux = np.abs(fx - np.floor(fx) - 0.5) < delta
    uy = np.abs(fy - np.floor(fy) - 0.5) < delta
    rx, ry = np.rint(fx), np.rint(fy)                   # round half to even
    xa, xb = np.where(ux, np.floor(fx), rx), np.where(ux, np.floor(fx) + 1, rx)
    ya, yb = np.where(uy, np.floor(fy), ry), np.where(uy, np.floor(fy) + 1, ry)
    cands = np.stack([pick(xa, ya), pick(xb, ya), pick(xa, yb), pick(xb, yb)], axis=-1)
    return pick(rx, ry), ux | uy, cands


def undecidable_count(H, W, quarters, rest):
    return int(rotation_map64(H, W, quarters, rest)[1].sum())


def check_rotation(got, src, fill, H, W, quarters, rest):
    """`got` [..., Hc, Wc] against the float64 map applied to `src` [..., H, W] (`fill` outside): every decidable pixel equal, every
    undecidable pixel equal to one of its candidates.  Returns the number of undecidable pixels of the map."""
    imap, und, cands = rotation_map64(H, W, quarters, rest)
    got = np.asarray(got)
    src = np.asarray(src)
    assert got.shape[-2:] == imap.shape and got.shape[:-2] == src.shape[:-2], (got.shape, src.shape, imap.shape)
    table = np.concatenate([np.full(src.shape[:-2] + (1,), fill, src.dtype), src.reshape(src.shape[:-2] + (H * W,))], axis=-1)
    want = table[..., imap]
    wrong = (got != want) & ~und
    assert not wrong.any(), f"rotation {H}x{W} q={quarters} rest={rest}: {int(wrong.sum())} decidable pixels differ from the float64 map, " \
                            f"first at {tuple(int(v) for v in np.argwhere(wrong)[0])}"
    one_of = (got[..., None] == table[..., cands]).any(-1)
    assert one_of[..., und].all(), f"rotation {H}x{W} q={quarters} rest={rest}: an undecidable pixel shows none of its candidates"
    return int(und.sum())


def index_image(H, W):
    """[2, 3, H, W]: plane p holds p H W + (1 .. H W), exact in fp32, so that a read from another plane shows; 0 stays free for fill"""
    n = BC[0] * BC[1]
    assert n * H * W < 2 ** 24
    return (np.arange(1, H * W + 1, dtype=F32).reshape(1, H, W) + F32(H * W) * np.arange(n, dtype=F32).reshape(n, 1, 1)).reshape(*BC, H, W)


# ---------------------------------------------------------------------------------------------------------------- blur, resize: float64
def blur_weights64(k):
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    taps = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    w = np.exp(-0.5 * (taps / sigma) ** 2)
    return w / w.sum()


def reflect_index(n, p, include_edge=False):
    """source index of the padded positions -p .. n - 1 + p (reflection about the edge pixel's centre; p <= n - 1)"""
    i = np.arange(-p, n + p)
    if include_edge:                                    # the planted error: reflection about the image border
        return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def blur64(u, k):
    u = np.asarray(u, np.float64)
    H, W = u.shape[-2:]
    w, p = blur_weights64(k), k // 2
    xp = u[..., reflect_index(H, p), :][..., reflect_index(W, p)]
    rows = sum(w[j] * xp[..., :, j:j + W] for j in range(k))
    return sum(w[i] * rows[..., i:i + H, :] for i in range(k))


def aa_weights(n_in, n_out):
    """resize(antialias=True) along one axis: the triangle filter of support max(scale, 1) about scale (i + 0.5), normalised per output"""
    scale = n_in / n_out
    support = max(scale, 1.0)
    W = np.zeros((n_out, n_in))
    for i in range(n_out):
        center = scale * (i + 0.5)
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        ws = [max(0.0, 1.0 - abs((j - center + 0.5) / max(scale, 1.0))) for j in range(lo, hi)]
        W[i, lo:hi] = np.array(ws) / sum(ws)
    return W


def resize64(u, nh, nw):
    u = np.asarray(u, np.float64)
    H, W = u.shape[-2:]
    return np.einsum("oi,...ij,pj->...op", aa_weights(nh, H), u[..., :nh, :nw], aa_weights(nw, W))


def transform64(op, u, p0, p1):
    return blur64(u, int(p0)) if op == BLUR else resize64(u, int(p0), int(p1))


def smallest_c(got, t64, A, clamp=False, pm1=False):
    """the smallest c with |got - t64| <= c 2^-24 A at every pixel; inf where A is 0 and the two differ.  `got` is the launch's output:
    with `clamp` the reference is clamped too (the clamp is 1-Lipschitz, so the bound survives it); in `pm1` mode `got` = fl(2 c - 1),
    which is allowed one extra rounding of 2^-24 and then halved back into [0, 1] terms."""
    ref = np.clip(t64, 0.0, 1.0) if clamp else t64
    d = np.abs(np.asarray(got, np.float64) - (ref * 2.0 - 1.0 if pm1 else ref))
    if pm1:
        d = np.where(A > 0, np.maximum(d - EPS, 0.0) * 0.5, d)
    if ((A == 0) & (d > 0)).any():
        return float("inf")
    return float(np.where(A > 0, d / (np.where(A > 0, A, 1.0) * EPS), 0.0).max())


# ---------------------------------------------------------------------------------------------------------------- the float32 models
FAULTS = {
    "blur-reflect-edge": BLUR,          # reflection that includes the edge pixel
    "blur-sigma-k": BLUR,               # sigma from k instead of k - 1
    "rot-centre": ROTATE,               # centre at (W - 1) / 2 - 1/2 on the x axis
    "rot-border": ROTATE,               # the border test admits fx == W
    "rot-quarters": ROTATE,             # quarter turns 1 and 3 swapped
    "rot-sign": ROTATE,                 # sign of sn flipped
    "resize-centre": CROP_RESIZE,       # centre without the + 1/2
    "resize-unnormalised": CROP_RESIZE,  # weights not divided by their sum
    "pm1-noclamp": None,                # the clamp of the pm1 form dropped (every transform)
    "plane-stride": None,               # plane stride W W instead of H W (the gathering transforms: flip, rotation)
}


def to_unit(x, pm1):
    """aug_in: fl(v * 0.5 + 0.5), one rounding (v * 0.5 is exact)"""
    x = np.asarray(x, F32)
    return x * F32(0.5) + F32(0.5) if pm1 else x


def from_unit(t, clamp, pm1, fault=None):
    """aug_out: clamp (always in pm1 mode), then fl(c * 2 - 1), one rounding"""
    t = np.asarray(t, F32)
    if (clamp or pm1) and not (pm1 and fault == "pm1-noclamp"):
        t = np.minimum(np.maximum(t, F32(0)), F32(1))
    return t * F32(2) - F32(1) if pm1 else t


def fma32(a, b, c):
    """fmaf: the product of two floats is exact in float64; the sum is rounded to float64 and then to float (double rounding differs from
    fmaf in the last bit on rare inputs, which a model used as an error yardstick can afford)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def blur_weights32(k, fault=None):
    """the host loop of wmar_augment, in float"""
    km = k if fault == "blur-sigma-k" else k - 1
    sigma = F32(0.3) * (F32(km) * F32(0.5) - F32(1)) + F32(0.8)
    w = np.zeros(k, F32)
    total = F32(0)
    for i in range(k):
        x = -F32(k - 1) * F32(0.5) + F32(i)
        w[i] = F32(math.exp(float(F32(-0.5) * (x / sigma) * (x / sigma))))
        total = total + w[i]
    return w / total


def _blur_model(u, k, fault):
    H, W = u.shape[-2:]
    w, p = blur_weights32(k, fault), k // 2
    edge = fault == "blur-reflect-edge"
    xp = u[..., reflect_index(H, p, edge), :][..., reflect_index(W, p, edge)]
    acc = np.zeros(u.shape, F32)
    for i in range(k):
        for j in range(k):
            acc = fma32(w[i] * w[j], xp[..., i:i + H, j:j + W], acc)
    return acc


def resize_weights32(n_in, n_out, fault=None):
    """[n_out, n_in] float weights of one axis as k_aug_point<AUG_CROP_RESIZE> forms them: window, sequential weight sum, one division
    per tap; 0 outside the window"""
    sc = F32(n_in) / F32(n_out)
    sp = max(sc, F32(1))
    Wm = np.zeros((n_out, n_in), F32)
    for o in range(n_out):
        c = sc * (F32(o) if fault == "resize-centre" else F32(o) + F32(0.5))
        lo, hi = max(int(c - sp + F32(0.5)), 0), min(int(c + sp + F32(0.5)), n_in)
        ws = [max(F32(0), F32(1) - abs((F32(j) - c + F32(0.5)) / sp)) for j in range(lo, hi)]
        total = F32(0)
        for v in ws:
            total = total + v
        for j, v in zip(range(lo, hi), ws):
            Wm[o, j] = v if fault == "resize-unnormalised" else v / total
    return Wm


def _resize_model(u, nh, nw, fault):
    H, W = u.shape[-2:]
    Wy, Wx = resize_weights32(nh, H, fault), resize_weights32(nw, W, fault)
    row = np.zeros(u.shape[:-2] + (nh, W), F32)        # a tap of weight 0 leaves the chain unchanged, so the window need not be cut out
    for j in range(nw):
        row = fma32(Wx[:, j], u[..., :nh, j:j + 1], row)
    acc = np.zeros(u.shape, F32)
    for i in range(nh):
        acc = fma32(Wy[:, i][:, None], row[..., i:i + 1, :], acc)
    return acc


def _gather(u, plane, sy, sx, fault):
    """u[plane, sy, sx] through the kernel's flat index plane * H * W + sy * W + sx"""
    H, W = u.shape[-2:]
    stride = W * W if fault == "plane-stride" else H * W
    return u.reshape(-1).take(plane * stride + sy * W + sx, mode="clip")


def _rot90_px(u, plane, q, y, x, fault):
    H, W = u.shape[-2:]
    if fault == "rot-quarters":
        q = {1: 3, 3: 1}.get(q, q)
    sy, sx = ((y, x), (x, W - 1 - y), (H - 1 - y, W - 1 - x), (H - 1 - x, y))[q]
    return _gather(u, plane, sy + 0 * x, sx + 0 * y, fault)


def _rotate_model(u, q, rest, fault):
    H, W = u.shape[-2:]
    assert H == W or q % 2 == 0
    P = u.size // (H * W)
    plane = np.arange(P).reshape(P, 1, 1)
    y, x = np.arange(H).reshape(1, H, 1), np.arange(W).reshape(1, 1, W)
    if rest == 0:
        return _rot90_px(u, plane, q, y, x, fault).reshape(u.shape)
    rad = rest * 3.14159265358979323846 / 180.0
    cs, sn = F32(math.cos(rad)), F32(math.sin(rad))
    if fault == "rot-sign":
        sn = -sn
    half_w, half_h = F32(0.5) * F32(W), F32(0.5) * F32(H)
    dx, dy = x.astype(F32) + F32(0.5) - half_w, y.astype(F32) + F32(0.5) - half_h
    sx, sy = cs * dx - sn * dy, sn * dx + cs * dy
    fx = np.rint(sx + (F32(0.5) * F32(W - 1) if fault == "rot-centre" else half_w) - F32(0.5))
    fy = np.rint(sy + half_h - F32(0.5))
    inside = (fx >= 0) & ((fx <= F32(W)) if fault == "rot-border" else (fx < F32(W))) & (fy >= 0) & (fy < F32(H))
    iy, ix = np.where(inside, fy, 0).astype(np.int64), np.where(inside, fx, 0).astype(np.int64)
    return np.where(inside, _rot90_px(u, plane, q, iy, ix, fault), F32(0)).reshape(u.shape)


def model(op, x, p0=0.0, p1=0.0, noise=None, pm1=False, fault=None):
    """the launch wmar_augment(op, ...) on a [..., H, W] float array, in numpy float32; `fault` plants one of FAULTS"""
    u = to_unit(x, pm1)
    H, W = u.shape[-2:]
    if op == IDENTITY:
        t = u
    elif op == BLUR:
        t = _blur_model(u, int(p0), fault)
    elif op == NOISE:
        t = u + F32(p0) * np.asarray(noise, F32)
    elif op == BRIGHTNESS:
        t = u * F32(p0)
    elif op == ROTATE:
        t = _rotate_model(u, int(p0) % 4, p1, fault)
    elif op == FLIP_H:
        P = u.size // (H * W)
        t = _gather(u, np.arange(P).reshape(P, 1, 1), np.arange(H).reshape(1, H, 1), W - 1 - np.arange(W).reshape(1, 1, W), fault).reshape(u.shape)
    elif op == CROP_RESIZE:
        t = _resize_model(u, int(p0), int(p1), fault)
    elif op == CROP_PAD:
        keep = (np.arange(H)[:, None] < int(p0)) & (np.arange(W)[None, :] < int(p1))
        t = np.where(keep, u, F32(0))
    else:
        raise ValueError(op)
    return from_unit(t, op in CLAMPING, pm1, fault)


def torch_restatement(op, x, p0, p1, pm1, device="cpu"):
    """torch's own fp32 evaluation of the published algorithm (valuemetric.gaussian_blur, geometric.resize_bilinear) on `device`"""
    xt = torch.from_numpy(np.array(x, dtype=F32)).to(device)
    u = xt / 2.0 + 0.5 if pm1 else xt
    H, W = u.shape[-2:]
    t = gaussian_blur(u, int(p0)) if op == BLUR else resize_bilinear(u[..., :int(p0), :int(p1)], (H, W))
    c = t.clamp(0, 1) if clamps(op, pm1) else t
    return (c * 2.0 - 1.0 if pm1 else c).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- cases
# rotation through the launch: (H, W, quarters, rest)
ROTATION_SWEEP = [(S, S) + divmod(a, 90) for S in (16, 17, 50, 64) for a in SWEEP_ANGLES]
ROTATION_SWEEP = [(H, W, q % 4, r) for H, W, q, r in ROTATION_SWEEP]
ROTATION_RECT = [(H, W, q, r) for H, W in ((12, 20), (33, 47)) for q in (0, 2) for r in (5, 20, 70)]
ROTATION_TIES = {(16, 16, 0, 45): 32, (17, 17, 0, 30): 16, (12, 20, 0, 45): 24}        # exact float64 ties: undecidable pixels
ROTATION_THIN = [(1, 7, 0, 20), (7, 1, 0, 20)]
ROTATION_QUARTERS = [(17, 17, 1, 0), (17, 17, 2, 0), (17, 17, 3, 0), (12, 20, 2, 0)]
ROTATION_CASES = ROTATION_SWEEP + ROTATION_RECT + [c for c in ROTATION_TIES if c[0] != 12] + ROTATION_THIN + ROTATION_QUARTERS
SMALL_SHAPES = ((16, 16), (17, 17), (12, 20), (20, 12), (50, 50), (64, 64), (33, 47))   # no undecidable pixel at any sweep remainder
LARGE_CAP = 0.002                                                                       # other shapes: at most 0.2 % undecidable


def expected_undecidable(H, W, q, rest):
    """what the float64 map alone must show before a forward is compared with it: the exact count for the cases of this file, None
    (the 0.2 % cap) for any other shape"""
    if (H, W, q, rest) in ROTATION_TIES:
        return ROTATION_TIES[(H, W, q, rest)]
    if rest == 0 or ((H, W) in SMALL_SHAPES and rest in SWEEP_RESTS) or (H, W, q, rest) in ROTATION_THIN:
        return 0
    return None


def assert_cap(H, W, q, rest):
    """the cap on what a rotation test may leave out -- a condition on the reference alone"""
    n, want = undecidable_count(H, W, q, rest), expected_undecidable(H, W, q, rest)
    if want is None:
        assert n <= LARGE_CAP * H * W, (H, W, q, rest, n)
    else:
        assert n == want, (H, W, q, rest, n, want)
    return n


BLUR_CASES = [(21, 19, 3), (21, 19, 9), (5, 5, 9), (40, 40, 19), (33, 70, 63), (32, 32, 63), (17, 33, 5)]
BLUR_EXACT = [(16, 16, 1), (1, 1, 1)]                   # k = 1: the clamp alone
RESIZE_CASES = [(23, 31, 10, 9), (23, 31, 22, 30), (20, 20, 10, 10), (17, 40, 9, 39), (50, 50, 47, 47), (64, 64, 60, 35),
                (23, 31, 1, 1), (23, 31, 1, 31), (23, 31, 23, 9)]
RESIZE_EXACT = [(23, 31, 23, 31)]                       # the whole image: the input's bits
RESIZE_FLOOR = (4.0, 8.0)       # torch's figure below 4 -> the gate is 8: one rounding per weight division and per fmaf on a 2 x 2-tap window
BRIGHTNESS_FACTORS = (1, 1.25, 1.5, 1.75, 2, 2.25, 2.5, 2.75, 3)
NOISE_SIGMAS = (0, 0.025, 0.05, 0.075, 0.1, 0.125, 0.15, 0.175, 0.2)
CROP_FACTORS = (1.0, 0.95, 0.9, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6, 0.55, 0.5)


def stencil_input(H, W, inputs, pm1, planes=BC):
    """what the launch reads: u uniform in [-0.3, 1.3] ("plain") or [-1.9, 2.9] ("wide": blurred pixels really clip), as x = 2 u - 1 in
    pm1 form"""
    gen = torch.Generator().manual_seed(1000 * H + W)
    u = torch.rand(*planes, H, W, generator=gen)
    u = (u * 4.8 - 1.9 if inputs == "wide" else u * 1.6 - 0.3).numpy()
    return (u * F32(2) - F32(1)) if pm1 else u


def saturated_image(H, W, pm1, seed=0):
    """a random image with saturated pixels: exact 0 / 1 (pm1: -1 / 1) on about a sixth of the pixels"""
    gen = torch.Generator().manual_seed(7000 + 100 * H + W + seed)
    u = (torch.rand(*BC, H, W, generator=gen) * 1.4 - 0.2).clamp(0, 1).numpy()
    return (u * F32(2) - F32(1)) if pm1 else u


@functools.lru_cache(maxsize=None)
def stencil_reference(op, H, W, p0, p1, inputs, pm1):
    """(x, t64, A, c_chain) of a case: computed once and shared; callers leave the arrays unchanged"""
    x = stencil_input(H, W, inputs, pm1)
    u = to_unit(x, pm1).astype(np.float64)              # pm1: the reference starts from the fp32 value fl(v * 0.5 + 0.5)
    t64, A = transform64(op, u, p0, p1), transform64(op, np.abs(u), p0, p1)
    for a in (x, t64, A):
        a.setflags(write=False)
    chain = smallest_c(model(op, x, p0, p1, pm1=pm1), t64, A, clamps(op, pm1), pm1)
    return x, t64, A, chain


# ---------------------------------------------------------------------------------------------------------------- gates
def gate_rotation(run, H, W, q, rest, report=None):
    """plain form on the index image (reads the map itself), pm1 form on a random image with saturated pixels (the value path)"""
    n = assert_cap(H, W, q, rest)                       # before the forward's output is looked at
    idx = index_image(H, W)
    assert check_rotation(run(ROTATE, idx, q, rest, None, False), idx, F32(0), H, W, q, rest) == n
    x = saturated_image(H, W, True)
    check_rotation(run(ROTATE, x, q, rest, None, True), model(IDENTITY, x, pm1=True), F32(-1), H, W, q, rest)
    if report:
        report(f"rotation {H}x{W} q={q} rest={rest}: undecidable {n} of {H * W}")
    return n


def gate_stencil(run, op, H, W, p0, p1, torch_device="cpu", report=None, forms=(False, True)):
    """c_kernel <= 2 max(c_torch, c_chain) for both input sets in both forms; the factor 2 covers another summation order"""
    name = "blur" if op == BLUR else "resize"
    for inputs in ("plain", "wide") if op == BLUR else ("plain",):
        for pm1 in forms:
            x, t64, A, c_chain = stencil_reference(op, H, W, p0, p1, inputs, pm1)
            cl = clamps(op, pm1)
            if inputs == "wide" and p0 <= 9:            # blurred pixels really clip, and some do not (a wider blur averages the excess away)
                assert 0.0 < float(((t64 < 0) | (t64 > 1)).mean()) < 1.0, (H, W, p0)
            c_torch = smallest_c(torch_restatement(op, x, p0, p1, pm1, torch_device), t64, A, cl, pm1)
            c_kernel = smallest_c(run(op, x, p0, p1, None, pm1), t64, A, cl, pm1)
            bound = 2.0 * max(c_torch, c_chain)
            if op == CROP_RESIZE and c_torch < RESIZE_FLOOR[0]:
                bound = RESIZE_FLOOR[1]
            if report:
                report(f"{name} {H}x{W} p=({p0},{p1}) pm1={int(pm1)} inputs={inputs}: c_kernel {c_kernel:.3f} c_torch {c_torch:.3f} "
                       f"c_chain {c_chain:.3f} bound {bound:.3f}")
            assert c_kernel <= bound, (name, H, W, p0, p1, pm1, inputs, c_kernel, c_torch, c_chain)


def canon(a):
    """the bits of a float array with -0.0 folded into +0.0 (fmaxf(-0.0, 0.0) may return either zero)"""
    return (np.asarray(a, F32) + F32(0)).view(np.int32)


def assert_bits(got, want, what):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape and np.array_equal(canon(got), canon(want)), \
        (what, int((canon(got) != canon(want)).sum()) if got.shape == want.shape else (got.shape, want.shape))


def gate_exact_stencil(run, op, H, W, p0, p1):
    """the cases in which a summing transform has one tap of weight 1: the bits of the range change and the clamp alone"""
    for inputs in ("plain", "wide"):
        for pm1 in (False, True):
            x = stencil_input(H, W, inputs, pm1)
            assert_bits(run(op, x, p0, p1, None, pm1), from_unit(to_unit(x, pm1), op in CLAMPING, pm1), (op, H, W, p0, p1, inputs, pm1))


SPECIALS = (-1.0, 1.0, -0.0, 0.0, 1e-40, 0.5, float(np.nextafter(F32(0.5), F32(1))), 2.0 ** -23, 0.75, float(np.nextafter(F32(0.75), F32(1))),
            0.4, 1.0 / 3.0)


def pointwise_input(H, W, pm1):
    """random pixels with the special values planted at the start of every plane: -1, +1, -0.0, a denormal, and u with f u exactly 1
    (0.5 at f = 2; pm1: x = 0) and just above (the next float; pm1: x = 2^-23), among others"""
    x = stencil_input(H, W, "plain", pm1).copy()
    flat = x.reshape(*BC, -1)
    n = min(len(SPECIALS), flat.shape[-1])
    flat[..., :n] = np.array(SPECIALS[:n], F32)
    return x


def pointwise_calls(H, W):
    calls = [(IDENTITY, 0, 0), (FLIP_H, 0, 0), (CROP_PAD, max(H // 2, 1), max(W - 3, 1)), (CROP_PAD, H, W), (CROP_PAD, 1, 1)]
    calls += [(BRIGHTNESS, f, 0) for f in BRIGHTNESS_FACTORS] + [(NOISE, s, 0) for s in NOISE_SIGMAS]
    return calls


def gate_pointwise(run, H, W):
    """identity, flip, crop + pad, brightness and noise are bit-equal to the numpy float32 restatement"""
    noise = torch.randn(*BC, H, W, generator=torch.Generator().manual_seed(H + W)).numpy()
    for pm1 in (False, True):
        x = pointwise_input(H, W, pm1)
        for op, p0, p1 in pointwise_calls(H, W):
            nz = noise if op == NOISE else None
            assert_bits(run(op, x, p0, p1, nz, pm1), model(op, x, p0, p1, nz, pm1), (op, H, W, p0, p1, pm1))
