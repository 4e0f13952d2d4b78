"""MI355X: thin wrappers of the wmar_vq_probe_* entries (include/wmar_hip.h) and the checks tests/test_gpu_vq_layers.py runs on one
kernel variant at a time.  Kept in a module of its own because the variants behind a process-wide switch (WMAR_CONV_NO_BX,
WMAR_VQ_NO_SPLIT) run the same checks in a child process.

Layout helpers: the probes take the engine's activation layout (NHWC fp32, channels zero-padded to a multiple of 8); the permutes
and the padding are done here with torch, so no layout kernel sits between a test and the kernel under test.

Every check returns the figures it measured and prints them on a line starting with "VQLAYER" before it asserts."""
import ctypes as C

import numpy as np
import torch

from tests import vq_layer_reference as R

IMPULSE_GATE = 2.0 ** -21     # <= six fp32 accumulations + the 2^-24 truncation of bx_split.h = 7 x 2^-24; fp32 kernels round once
DENSE_GATE = 2.0              # x the sequential fp32 chain's normalised error on the same data
EXPF_MARGIN = 4.0             # x torch's fp32 CPU error: __expf's argument scaling costs up to |r| ulp


def pad8(c):
    return (c + 7) & ~7


def _lib():
    from wmar_amd import _lib
    return _lib, _lib.load()


def to_nhwc(x, fill=None):
    """numpy NCHW -> cuda NHWC fp32 with channels padded to a multiple of 8 (zeros, or `fill` values for the padding channels)."""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    B, Cc, H, W = x.shape
    out = torch.zeros(B, H, W, pad8(Cc), dtype=torch.float32)
    if fill is not None and pad8(Cc) > Cc:
        out[..., Cc:] = torch.from_numpy(np.asarray(fill, dtype=np.float32))
    out[..., :Cc] = x.permute(0, 2, 3, 1)
    return out.cuda().contiguous()


def from_nhwc(t):
    return t.cpu().permute(0, 3, 1, 2).contiguous().numpy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _info(buf):
    return dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))


def probe_conv(w, bias, x, res=None, gn=None, stride=1, up=False, arm_stats=False, want_mr=False, in_fill=None):
    """w [Cout, Cin, ks, ks], bias [Cout] or None, x NCHW, res NCHW or None, gn = (gamma, beta, swish) or None.
    Returns (y NCHW with the real channels, y_pad NCHW with the padding channels, mr [B, 32, 2] or None, info dict)."""
    lib, L = _lib()
    cout, cin, ks, _ = w.shape
    B, _, Hs, Ws = x.shape
    Hc, Wc = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    Ho, Wo = (Hc // 2, Wc // 2) if stride == 2 else (Hc, Wc)
    wd, bd, xd = _dev(w), _dev(bias), to_nhwc(x, in_fill)
    rd = None if res is None else to_nhwc(res)
    gd = (None, None) if gn is None else (_dev(gn[0]), _dev(gn[1]))
    y = torch.full((B, Ho, Wo, pad8(cout)), float("nan"), dtype=torch.float32, device="cuda")
    mr = torch.full((B, 32, 2), float("nan"), dtype=torch.float32, device="cuda") if want_mr else None
    buf = C.create_string_buffer(256)
    lib.check(L.wmar_vq_probe_conv(_ptr(wd), _ptr(bd), cout, cin, ks, _ptr(xd), _ptr(rd), _ptr(gd[0]), _ptr(gd[1]),
                                   int(gn[2]) if gn else 0, B, Hs, Ws, stride, int(up), int(arm_stats), _ptr(y), _ptr(mr), buf, 256,
                                   lib.stream_ptr()))
    torch.cuda.synchronize()
    yn = from_nhwc(y)
    return yn[:, :cout], yn[:, cout:], None if mr is None else mr.cpu().numpy(), _info(buf)


def probe_attn(q, k, v, H, W):
    """q, k, v numpy [B, H * W, C] -> (o, info)."""
    lib, L = _lib()
    B, N, Cc = q.shape
    assert N == H * W
    qd, kd, vd = _dev(q), _dev(k), _dev(v)
    o = torch.full((B, N, Cc), float("nan"), dtype=torch.float32, device="cuda")
    buf = C.create_string_buffer(256)
    lib.check(L.wmar_vq_probe_attn(_ptr(qd), _ptr(kd), _ptr(vd), B, H, W, Cc, _ptr(o), buf, 256, lib.stream_ptr()))
    torch.cuda.synchronize()
    return o.cpu().numpy(), _info(buf)


def probe_argmin(z, emb):
    lib, L = _lib()
    P, E = z.shape
    zd, ed = _dev(z), _dev(emb)
    codes = torch.full((P,), -1, dtype=torch.int64, device="cuda")
    buf = C.create_string_buffer(256)
    lib.check(L.wmar_vq_probe_argmin(_ptr(zd), P, E, _ptr(ed), emb.shape[0], _ptr(codes), buf, 256, lib.stream_ptr()))
    torch.cuda.synchronize()
    return codes.cpu().numpy(), buf.value.decode()


# ------------------------------------------------------------------------------------------------ convolution checks
class ConvCase:
    def __init__(self, kernel, cin, cout, ks, hw, stride=1, up=False, res=True, B=2):
        self.kernel, self.cin, self.cout, self.ks, self.stride, self.up, self.B = kernel, cin, cout, ks, stride, up, B
        self.H, self.W = (hw, hw) if isinstance(hw, int) else hw
        self.res = res                       # whether the dense / epilogue checks hand the kernel a residual
        self.seed = (cin * 131 + cout * 17 + ks * 7 + self.H * 3 + stride + 2 * int(up)) & 0xffff

    @property
    def id(self):
        return "%s-%dto%d-k%d-s%d-up%d-%dx%d" % (self.kernel, self.cin, self.cout, self.ks, self.stride, int(self.up), self.H, self.W)

    def out_hw(self):
        Hc, Wc = (2 * self.H, 2 * self.W) if self.up else (self.H, self.W)
        return (Hc // 2, Wc // 2) if self.stride == 2 else (Hc, Wc)

    def __repr__(self):
        return self.id


def _say(what, case, **figs):
    print("VQLAYER %s %s %s" % (what, case, " ".join("%s=%.4g" % kv for kv in figs.items())), flush=True)


def check_kernel(case, info):
    assert info["conv"] == case.kernel, "dispatch launched %s, this case is meant to cover %s" % (info["conv"], case.kernel)


def _gather(case, xp, c, dy, dx):
    """xp = R._prepare(x): x[b, c, oy * s + dy - pad, ox * s + dx - pad] of the (upsampled, zero-padded) input for every output
    pixel -> [B, Ho, Wo]."""
    Ho, Wo = case.out_hw()
    s = case.stride
    return xp[:, c, dy:dy + s * Ho:s, dx:dx + s * Wo:s]


def check_impulse(case, gn=None):
    """One non-zero weight per output channel; over the passes every (input channel, tap) pair is hit.  Every output is a single
    product (gate 2^-21 relative, derived in the module docstring of the test) or an exact zero where the tap falls into the padding.
    The last pass uses bf16-exact operands: the product is then exact in every kernel."""
    rng = np.random.default_rng(case.seed)
    T = case.ks * case.ks
    pairs = case.cin * T
    passes = -(-pairs // case.cout)
    x = R.full_significand(rng, case.B * case.cin * case.H * case.W).reshape(case.B, case.cin, case.H, case.W)
    worst, seen, n_zero = 0.0, set(), 0
    for p in range(passes + 1):
        exact_pass = p == passes
        xs = R.bf16_exact(rng, x.size).reshape(x.shape) if exact_pass else x
        vals = R.bf16_exact(rng, case.cout) if exact_pass else R.full_significand(rng, case.cout)
        w = np.zeros((case.cout, case.cin, case.ks, case.ks), dtype=np.float32)
        idx = [((p * case.cout + o) * (1 if not exact_pass else 7)) % pairs for o in range(case.cout)]
        for o, i in enumerate(idx):
            c, tap = i // T, i % T
            w[o, c, tap // case.ks, tap % case.ks] = vals[o]
            if not exact_pass:
                seen.add(i)
        y, ypad, _, info = probe_conv(w, None, xs, stride=case.stride, up=case.up)
        check_kernel(case, info)
        xp = R._prepare(xs, case.ks, case.stride, case.up)
        for o, i in enumerate(idx):
            c, tap = i // T, i % T
            want = vals[o].astype(np.float64) * _gather(case, xp, c, tap // case.ks, tap % case.ks)
            got = y[:, o].astype(np.float64)
            zero = want == 0
            n_zero += int(zero.sum())
            assert np.all(got[zero] == 0), "%s pass %d cout %d: padding output is not exactly 0" % (case, p, o)
            rel = np.abs(got - want)[~zero] / np.abs(want)[~zero]
            if exact_pass:
                assert np.all(rel == 0), "%s: bf16-exact product of cout %d (cin %d, tap %d) is off by %.3g" % (case, o, c, tap, rel.max())
            else:
                worst = max(worst, float(rel.max()))
                assert rel.max() <= IMPULSE_GATE, "%s pass %d: cout %d (cin %d, tap %d) off by %.2f x 2^-24 relative" % (
                    case, p, o, c, tap, rel.max() / R.U24)
        assert np.all(ypad == 0)
    assert len(seen) == pairs, "impulse passes covered %d of %d (channel, tap) pairs" % (len(seen), pairs)
    if case.ks == 3:
        assert n_zero > 0, "no output fell into the padding"
    _say("impulse", case, passes=passes + 1, worst_rel_in_ulp24=worst / R.U24)
    return worst


def dense_data(case, rng):
    x = R.realistic_activations(rng, (case.B, case.cin, case.H, case.W))
    w = (rng.standard_normal((case.cout, case.cin, case.ks, case.ks)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(case.cout) * 0.1).astype(np.float32)
    Ho, Wo = case.out_hw()
    res = R.realistic_activations(rng, (case.B, case.cout, Ho, Wo)) if case.res else None
    return x, w, b, res


def check_dense(case):
    """Random weights, bias, residual: max normalised error against float64 at most DENSE_GATE x the sequential fp32 chain's."""
    rng = np.random.default_rng(case.seed + 1)
    x, w, b, res = dense_data(case, rng)
    y, ypad, _, info = probe_conv(w, b, x, res, stride=case.stride, up=case.up)
    check_kernel(case, info)
    exact = R.conv2d(x, w, b, res, case.stride, case.up)
    den = R.conv2d_abs(x, w, b, res, case.stride, case.up)
    chain = R.conv2d_chain(x, w, b, res, case.stride, case.up)
    e_chain = R.normalised_error(chain, exact, den)
    e = R.normalised_error(y, exact, den)
    # An output that sees one of the 2^20 values pushes the chain towards its worst case (every later product is rounded at the big
    # term's ulp), which would leave the gate over ALL outputs 5 to 10 times looser than on ordinary data -- loose enough for a lost
    # piece product to pass.  The same gate is therefore also applied to the outputs that see no such value, against the chain's
    # maximum over the same outputs (the yardstick holds for any set of outputs; these are at least 3/4 of them).
    big = R.conv2d((np.abs(x) >= 2.0 ** 19).astype(np.float64), np.ones((1, case.cin, case.ks, case.ks)), stride=case.stride, up=case.up) > 0
    big = np.broadcast_to(big, exact.shape) | (False if res is None else np.abs(res) >= 2.0 ** 19)
    plain = np.where(big, 0.0, den)
    e_plain, e_chain_plain = R.normalised_error(y, exact, plain), R.normalised_error(chain, exact, plain)
    _say("dense", case, K=case.cin * case.ks ** 2, kernel_err=e, chain_err=e_chain, ratio=e / e_chain, plain_share=float((~big).mean()),
         plain_kernel_err=e_plain, plain_chain_err=e_chain_plain, plain_ratio=e_plain / e_chain_plain)
    assert np.all(np.isfinite(y)) and np.all(ypad == 0)
    assert e <= DENSE_GATE * e_chain, "%s: normalised error %.3g is %.2f x the fp32 chain's %.3g" % (case, e, e / e_chain, e_chain)
    assert e_plain <= DENSE_GATE * e_chain_plain, "%s: outputs without a 2^20 operand: normalised error %.3g is %.2f x the fp32 chain's %.3g" % (
        case, e_plain, e_plain / e_chain_plain, e_chain_plain)
    return e / e_chain, e_plain / e_chain_plain


def check_epilogue(case):
    """All-zero weights: y is bit-equal to fl32(bias + res); the padding output channels are exactly 0."""
    rng = np.random.default_rng(case.seed + 2)
    x, w, b, res = dense_data(case, rng)
    y, ypad, _, info = probe_conv(np.zeros_like(w), b, x, res, stride=case.stride, up=case.up)
    check_kernel(case, info)
    want = np.broadcast_to(b[None, :, None, None], y.shape).astype(np.float32)
    if res is not None:
        want = (want.astype(np.float64) + res.astype(np.float64)).astype(np.float32)
    assert np.array_equal(y.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), "%s: epilogue is not fl32(bias + res)" % case
    assert np.all(ypad == 0) and ypad.shape[1] == pad8(case.cout) - case.cout


def check_input_padding(case):
    """Finite garbage in the input's padding channels (cin .. cin_s) must not change a bit of the output."""
    assert pad8(case.cin) > case.cin
    rng = np.random.default_rng(case.seed + 3)
    x, w, b, res = dense_data(case, rng)
    y0, p0, _, info = probe_conv(w, b, x, res, stride=case.stride, up=case.up)
    check_kernel(case, info)
    fill = (rng.standard_normal((case.B, case.H, case.W, pad8(case.cin) - case.cin)) * 1e6).astype(np.float32)
    y1, p1, _, _ = probe_conv(w, b, x, res, stride=case.stride, up=case.up, in_fill=fill)
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32)) and np.array_equal(p0, p1)


# ------------------------------------------------------------------------------------------------ fused GroupNorm checks
def gn_input(rng, B, Cc, H, W, offset_sigmas=0.0):
    """Normal values clipped to +-3.5 sigma (|normalised value| stays below 8 with the gammas used here); offset_sigmas moves
    every group's mean to that many standard deviations."""
    x = np.clip(rng.standard_normal((B, Cc, H, W)), -3.5, 3.5)
    scale = rng.uniform(0.5, 2.0, (B, 32)).repeat(Cc // 32, axis=1)[:, :, None, None]
    shift = rng.uniform(-1.0, 1.0, (B, 32)).repeat(Cc // 32, axis=1)[:, :, None, None]
    x = x * scale + shift + offset_sigmas * scale
    gamma = rng.uniform(0.5, 1.5, Cc) * rng.choice([-1.0, 1.0], Cc)
    beta = rng.uniform(-0.5, 0.5, Cc)
    return x.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32)


def torch_fp32_gn(x, gamma, beta, swish):
    import torch.nn.functional as F
    y = F.group_norm(torch.from_numpy(x), 32, torch.from_numpy(gamma), torch.from_numpy(beta), eps=1e-6)
    return (F.silu(y) if swish else y).numpy()


def check_fused_gn_identity(kernel, Cc, hw, swish, offset_sigmas=0.0, ks=3):
    """Identity weight (one tap, 1.0): y is exactly the activation the patch loader staged.  Elementwise against float64
    swish(GN(x)); tolerance EXPF_MARGIN x the error of torch's fp32 CPU silu(group_norm(x)) on the same input."""
    case = ConvCase(kernel, Cc, Cc, ks, hw, res=False)
    rng = np.random.default_rng(case.seed + 11 + swish)
    x, gamma, beta = gn_input(rng, case.B, Cc, hw, hw, offset_sigmas)
    w = np.zeros((Cc, Cc, ks, ks), dtype=np.float32)
    w[np.arange(Cc), np.arange(Cc), ks // 2, ks // 2] = 1.0
    y, _, _, info = probe_conv(w, None, x, gn=(gamma, beta, swish))
    check_kernel(case, info)
    assert info["gn_in"] == "k_gn_partial+k_gn_finalize"
    exact = R.group_norm(x, gamma, beta, swish)
    assert np.abs((x.astype(np.float64) - np.repeat(R.group_stats(x)[0], Cc // 32, 1)[:, :, None, None])
                  * np.repeat(R.group_stats(x)[1], Cc // 32, 1)[:, :, None, None]).max() <= 8.0
    budget = float(np.abs(torch_fp32_gn(x, gamma, beta, swish) - exact).max())
    e = float(np.abs(y - exact).max())
    _say("fused_gn", "%s C=%d HW=%d swish=%d mean/std=%g" % (kernel, Cc, hw * hw, swish, offset_sigmas), kernel_err=e, torch_fp32_err=budget,
         ratio=e / budget)
    assert e <= EXPF_MARGIN * budget, "C=%d HW=%d swish=%d: error %.3g is %.2f x torch fp32's %.3g" % (Cc, hw * hw, swish, e, e / budget, budget)
    return e / budget


def check_fused_gn_dense(kernel, Cc, cout, hw, swish=1, ks=3):
    """A dense conv behind a fused GroupNorm: the dense gate plus sum|w| x the activation budget of the identity check."""
    case = ConvCase(kernel, Cc, cout, ks, hw, res=True)
    rng = np.random.default_rng(case.seed + 21)
    x, gamma, beta = gn_input(rng, case.B, Cc, hw, hw)
    _, w, b, res = dense_data(case, rng)
    y, _, _, info = probe_conv(w, b, x, res, gn=(gamma, beta, swish))
    check_kernel(case, info)
    a64 = R.group_norm(x, gamma, beta, swish)
    a32 = a64.astype(np.float32)
    budget = EXPF_MARGIN * float(np.abs(torch_fp32_gn(x, gamma, beta, swish) - a64).max())
    exact, den = R.conv2d(a64, w, b, res), R.conv2d_abs(a64, w, b, res)
    e_chain = R.normalised_error(R.conv2d_chain(a32, w, b, res), R.conv2d(a32, w, b, res), R.conv2d_abs(a32, w, b, res))
    sum_w = R.conv2d(np.ones_like(a64), np.abs(w))
    allowed = DENSE_GATE * e_chain * den + sum_w * budget
    err = np.abs(y - exact)
    _say("fused_gn_dense", case, chain_err=e_chain, worst_over_allowed=float((err / allowed).max()))
    assert np.all(err <= allowed), "%s behind GroupNorm: %.3g x the allowed error" % (case, (err / allowed).max())


# ------------------------------------------------------------------------------------------------ statistics checks
def check_stats(kernel, cin, cout, ks, hw, with_res, B=3):
    """(mean, rstd) of the conv's output as the next GroupNorm gets them -- through the conv epilogue + k_gn_finalize_tiles when
    the tracker is armed and the shape qualifies, through k_gn_partial + k_gn_finalize otherwise -- against float64 statistics
    of the stored fp32 tensor.  The sums are fp64: only the final roundings to fp32 remain."""
    case = ConvCase(kernel, cin, cout, ks, hw, res=with_res, B=B)
    rng = np.random.default_rng(case.seed + 31)
    x, w, b, res = dense_data(case, rng)
    x = np.clip(x, -4, 4)                                   # statistics of a tensor with 2^20 outliers test nothing but the outlier
    res = None if res is None else np.clip(res, -4, 4)
    b = (b + rng.uniform(-3, 3, cout)).astype(np.float32)   # group means away from zero
    out = {}
    for armed in (1, 0):
        y, _, mr, info = probe_conv(w, b, x, res, arm_stats=bool(armed), want_mr=True)
        check_kernel(case, info)
        want_path = "k_gn_finalize_tiles" if armed and cout // 32 in (4, 8, 16) and cout % 32 == 0 else "k_gn_partial+k_gn_finalize"
        assert info["stats"] == want_path, (info, want_path)
        mean, rstd = R.group_stats(y)
        std = 1.0 / rstd
        assert np.all(np.abs(mean) / std <= 1e3)
        em = np.abs(mr[:, :, 0] - mean) / np.maximum(np.abs(mean), std)
        er = np.abs(mr[:, :, 1] - rstd) / rstd
        _say("stats", "%s path=%s res=%d" % (case, info["stats"], with_res), mean_err_ulp23=em.max() / 2.0 ** -23, rstd_err_ulp22=er.max() / 2.0 ** -22)
        assert em.max() <= 2.0 ** -23, (case, info["stats"], em.max())
        assert er.max() <= 2.0 ** -22, (case, info["stats"], er.max())
        out[armed] = (y, mr)
    assert np.array_equal(out[0][0], out[1][0]), "the statistics epilogue changed the conv's output"
    m0, m1 = out[0][1].astype(np.float64), out[1][1].astype(np.float64)
    mean, rstd = R.group_stats(out[0][0])
    assert np.all(np.abs(m0[:, :, 0] - m1[:, :, 0]) <= 2.0 ** -23 * np.maximum(np.abs(mean), 1.0 / rstd))
    assert np.all(np.abs(m0[:, :, 1] - m1[:, :, 1]) <= 2.0 ** -22 * rstd)


# ------------------------------------------------------------------------------------------------ attention checks
def attn_inputs(N, Cc, seed):
    """B = 2, different K and V per image, score std about 3; image 1 row 3 has one dominant key (score gap 60), image 1 row 7 has
    all scores equal (q = 0); V of image 1 has a positive mean so that 'the plain mean of V' has a scale."""
    rng = np.random.default_rng(seed)
    s = 3.0 ** 0.5
    q = (rng.standard_normal((2, N, Cc)) * s).astype(np.float32)
    k = (rng.standard_normal((2, N, Cc)) * s).astype(np.float32)
    v = rng.standard_normal((2, N, Cc)).astype(np.float32)
    v[1] = (1.0 + 0.3 * v[1]).astype(np.float32)
    kj = k[1, 5].astype(np.float64)
    others = np.delete(k[1].astype(np.float64) @ kj, 5)
    t = 60.0 * Cc ** 0.5 / (kj @ kj - others.max())
    q[1, 3] = (t * kj).astype(np.float32)
    q[1, 7] = 0.0
    return q, k, v


def check_attention(N, Cc, hw, path, kernel):
    q, k, v = attn_inputs(N, Cc, 1000 + N + Cc)
    sc = np.einsum("ic,jc->ij", q[1].astype(np.float64), k[1].astype(np.float64)) * Cc ** -0.5
    row = np.sort(sc[3])
    assert 59.0 <= row[-1] - row[-2] <= 61.0 and np.argmax(sc[3]) == 5 and 2.5 < np.delete(sc, [3, 7], 0).std() < 3.5
    o, info = probe_attn(q, k, v, hw, hw)
    assert info["path"] == path and info["scores"] == kernel[0] and info["pv"] == kernel[1], info
    exact = R.attention(q, k, v)
    tq, tk, tv = (torch.from_numpy(t) for t in (q, k, v))
    t32 = (torch.softmax(tq @ tk.transpose(1, 2) * (Cc ** -0.5), dim=-1) @ tv).numpy()
    budget = float(np.abs(t32 - exact).max())
    e = float(np.abs(o - exact).max())
    mean_v = v[1].astype(np.float64).mean(0)
    e_mean = float((np.abs(o[1, 7] - mean_v) / np.abs(v[1].astype(np.float64)).mean(0)).max())
    _say("attention", "N=%d C=%d %s" % (N, Cc, info), kernel_err=e, torch_fp32_err=budget, ratio=e / budget, equal_row_err_ulp24=e_mean / R.U24)
    assert np.all(np.isfinite(o))
    assert np.abs(o[1, 3] - v[1, 5]).max() <= 1e-6, "the dominant key (score gap 60) must own its row"
    assert e <= EXPF_MARGIN * budget, "attention N=%d C=%d: error %.3g is %.2f x torch fp32's %.3g" % (N, Cc, e, e / budget, budget)
    assert e_mean <= 2.0 ** -21, "equal scores: off the plain mean of V by %.2f x 2^-24" % (e_mean / R.U24)
    return e / budget


# ------------------------------------------------------------------------------------------------ nearest-code search checks
def argmin_inputs(P, E, N, seed):
    """Random z and codebook; duplicated codebook rows in another 32-code tile, in the last code split and in the other lane half
    (a lane half holds the codes with bit 2 of the index clear / set); z rows bit-equal to codebook rows, duplicated ones included."""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((N, E)).astype(np.float32)
    z = rng.standard_normal((P, E)).astype(np.float32)
    dups = [(1, 33), (6, 70), (2, N - 30), (5, N - 2), (40, N - 57), (N // 2 + 3, N // 2 + 39)]       # (lower, higher)
    for lo, hi in dups:
        assert lo < hi < N and lo // 32 != hi // 32
        emb[hi] = emb[lo]
    on_rows = [lo for lo, _ in dups] + [hi for _, hi in dups][:2] + [N - 1, 0, 31, 32]
    pix = rng.choice(P, size=len(on_rows), replace=False)
    for p, r in zip(pix, on_rows):
        z[p] = emb[r]
    first = {hi: lo for lo, hi in dups}
    expect = {int(p): first.get(r, r) for p, r in zip(pix, on_rows)}
    return z, emb, expect


def check_argmin(P, E, N, want_path, seed=5):
    z, emb, expect = argmin_inputs(P, E, N, seed + P + E + N)
    codes, path = probe_argmin(z, emb)
    assert path == want_path, (path, want_path)
    assert codes.min() >= 0 and codes.max() < N
    d = R.sq_distances(z, emb)
    zn, en = (z.astype(np.float64) ** 2).sum(-1), (emb.astype(np.float64) ** 2).sum(-1)
    chosen = d[np.arange(P), codes]
    slack = 8 * R.U24 * (zn + en[codes])
    worst = float(((chosen - d.min(-1)) / slack).max())
    _say("argmin", "P=%d E=%d N=%d %s" % (P, E, N, path), worst_excess_over_slack=worst, not_the_fp64_argmin=float((codes != d.argmin(-1)).sum()))
    assert np.all(chosen <= d.min(-1) + slack), "a chosen code is %.2f x the rounding slack away from the nearest" % worst
    for p, r in expect.items():
        assert codes[p] == r, "pixel %d sits exactly on row %d (lowest duplicate) but got %d" % (p, r, codes[p])
    return codes
