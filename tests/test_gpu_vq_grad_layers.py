"""MI355X: the backward of every VQGAN layer alone against a float64 reference (wmar_amd/csrc/vq_grad.h through the
wmar_vq_probe_*_backward entries).  Every case asserts the kernels the dispatch reports.

Gates (the forward's, tests/test_gpu_vq_layers.py; none of them measured on the code under test):
  impulse   every output is ONE product: |got - a b| <= 2^-21 |a b| (six fp32 accumulations of piece products + the 2^-24 truncation
            on the bf16-piece path, one rounding on the fp32 paths); bf16-exact operands give the exact product; outputs that see
            only padding are exactly 0.  The input gradient gets a weight with one non-zero per input channel (with `up`, a
            gradient on one parity class of pixels, so that the 2 x 2 sum has one term); the weight gradient gets an output
            gradient with one non-zero per output channel, which also makes the bias gradient that value.
  dense     max |got - exact| / sum|terms| <= 2 x the same figure of a sequential fp32 chain over the same terms
            (tests/vq_grad_reference.py; tests/test_vq_grad_reference.py shows that a weight gradient which drops a tap or an image
            is 1000 x beyond it).
  padding   garbage in the padding channels of either operand changes no bit.
  GroupNorm g_x error normalised by max|g_x| per (image, group), dgamma / dbeta by sum|terms|: <= 4 x the same figure of torch's
            fp32 CPU autograd on the same data (the forward file's GroupNorm factor), floor 4 x 2^-24.
  attention per output tensor, error normalised by its max: <= 4 x torch's fp32 CPU autograd, same floor.
  determinism  every probe run twice gives the same bits (no floating-point atomics anywhere).

The measured ratios are printed on lines starting with VQGRAD (run with -s) and tabulated in DESIGN.md."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vq_grad_reference as G
from tests import vq_layer_checks as K
from tests import vq_layer_reference as R

pytestmark = pytest.mark.gpu

IMPULSE_GATE = K.IMPULSE_GATE
DENSE_GATE = K.DENSE_GATE
TORCH_FACTOR = 4.0
FLOOR = 4.0 * R.U24


def _say(what, case, **figs):
    print("VQGRAD %s %s %s" % (what, case, " ".join("%s=%.4g" % kv for kv in figs.items())), flush=True)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ probes
def probe_conv_backward(w, x, g, stride=1, up=False, x_fill=None, g_fill=None):
    """w [Cout, Cin, ks, ks], x NCHW (the conv's input), g NCHW (gradient of its output) ->
    (g_x NCHW real channels, g_x padding channels, g_w, g_b, info)."""
    lib, L = K._lib()
    cout, cin, ks, _ = w.shape
    B, _, Hs, Ws = x.shape
    wd, xd, gd = K._dev(w), K.to_nhwc(x, x_fill), K.to_nhwc(g, g_fill)
    gx = torch.full((B, Hs, Ws, K.pad8(cin)), float("nan"), dtype=torch.float32, device="cuda")
    gw = torch.full((cout, cin, ks, ks), float("nan"), dtype=torch.float32, device="cuda")
    gb = torch.full((cout,), float("nan"), dtype=torch.float32, device="cuda")
    buf = C.create_string_buffer(256)
    lib.check(L.wmar_vq_probe_conv_backward(K._ptr(wd), cout, cin, ks, K._ptr(xd), K._ptr(gd), B, Hs, Ws, stride, int(up), K._ptr(gx),
                                            K._ptr(gw), K._ptr(gb), buf, 256, lib.stream_ptr()))
    torch.cuda.synchronize()
    gxn = K.from_nhwc(gx)
    return gxn[:, :cin], gxn[:, cin:], gw.cpu().numpy(), gb.cpu().numpy(), K._info(buf)


def probe_gn_backward(x, g, mr, gamma, beta, swish):
    lib, L = K._lib()
    B, Cc, H, W = x.shape
    xd, gd = K.to_nhwc(x), K.to_nhwc(g)
    md, gad, bed = K._dev(mr), K._dev(gamma), K._dev(beta)
    gx = torch.full((B, H, W, Cc), float("nan"), dtype=torch.float32, device="cuda")
    dg = torch.full((Cc,), float("nan"), dtype=torch.float32, device="cuda")
    db = torch.full((Cc,), float("nan"), dtype=torch.float32, device="cuda")
    buf = C.create_string_buffer(256)
    lib.check(L.wmar_vq_probe_gn_backward(K._ptr(xd), K._ptr(gd), K._ptr(md), K._ptr(gad), K._ptr(bed), B, H * W, Cc, int(swish), K._ptr(gx),
                                          K._ptr(dg), K._ptr(db), buf, 256, lib.stream_ptr()))
    torch.cuda.synchronize()
    return K.from_nhwc(gx), dg.cpu().numpy(), db.cpu().numpy(), K._info(buf)


def probe_attn_backward(q, k, v, go, H, W):
    lib, L = K._lib()
    B, N, Cc = q.shape
    ds = [K._dev(t) for t in (q, k, v, go)]
    outs = [torch.full((B, N, Cc), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    buf = C.create_string_buffer(256)
    lib.check(L.wmar_vq_probe_attn_backward(*[K._ptr(t) for t in ds], B, H, W, Cc, *[K._ptr(t) for t in outs], buf, 256, lib.stream_ptr()))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs], K._info(buf)


# ------------------------------------------------------------------------------------------------ convolution
class Case:
    def __init__(self, cin, cout, ks, hw, dgrad, stride=1, up=False):
        self.cin, self.cout, self.ks, self.H, self.stride, self.up, self.dgrad = cin, cout, ks, hw, stride, up, dgrad
        self.seed = (cin * 131 + cout * 17 + ks * 7 + hw * 3 + stride + 2 * int(up)) & 0xffff

    @property
    def id(self):
        return "%dto%d-k%d-s%d-up%d-%d" % (self.cin, self.cout, self.ks, self.stride, int(self.up), self.H)

    def out_hw(self):
        return self.H * (2 if self.up else 1) // self.stride

    def splits(self, B):
        """The documented rule of run_conv_wgrad: slices of at least 256 products per weight, at most as many as bring the launch to
        1024 waves, at most 64."""
        Kp = B * self.out_hw() ** 2
        tiles = -(-self.cout // 32) * -(-self.cin // 32)
        return max(1, min(-(-Kp // 256), -(-1024 // tiles), 64))

    def check_info(self, info, B):
        assert info["dgrad"] == self.dgrad, "dgrad launched %s, this case is meant to cover %s" % (info["dgrad"], self.dgrad)
        assert info["wgrad"] == "k_wgrad<%d>" % self.ks, info
        assert int(info["splits"]) == self.splits(B), (info, self.splits(B))
        assert info["bgrad"] == "k_bgrad_partial", info

    def __repr__(self):
        return self.id


CASES = [
    Case(32, 32, 3, 8, "flip+k_conv_bx<1,3>"),
    Case(32, 32, 1, 8, "flip+k_conv_bx<1,1>"),
    Case(64, 128, 3, 16, "flip+k_conv_bx<2,3>"),
    Case(128, 64, 1, 8, "flip+k_conv_bx<4,1>"),
    Case(64, 64, 3, 24, "flip+k_conv_bx<2,3>"),                         # odd tile counts
    Case(32, 32, 3, 16, "k_dgrad_s2", stride=2),
    Case(32, 128, 3, 16, "k_dgrad_s2", stride=2),
    Case(64, 64, 3, 4, "flip+k_conv_bx<2,3>+k_sum2x2", up=True),
    Case(128, 128, 3, 8, "flip+k_conv_bx<4,3,4>+k_sum2x2", up=True),
    Case(3, 32, 3, 8, "flip+k_conv_bx<1,3>"),                           # conv_in: a 3-channel input gradient
    Case(32, 3, 3, 16, "flip+k_conv<1>"),                               # conv_out: a 3-channel output gradient
]
_ids = [c.id for c in CASES]
BATCHES = [1, 3]


def test_the_cases_cover_one_and_several_wgrad_splits():
    by = {c.id: c for c in CASES}
    assert by["32to32-k3-s1-up0-8"].splits(1) == 1 and by["32to32-k3-s1-up0-8"].splits(3) == 1        # K = 64, 192
    assert by["64to128-k3-s1-up0-16"].splits(1) == 1 and by["64to128-k3-s1-up0-16"].splits(3) == 3    # K = 256 (exactly one), 768
    assert by["64to64-k3-s1-up0-24"].splits(1) == 3 and by["64to64-k3-s1-up0-24"].splits(3) == 7      # K = 576, 1728: uneven slices


def _rel(got, want):
    nz = want != 0
    return (np.abs(got.astype(np.float64) - want)[nz] / np.abs(want)[nz]).max() if nz.any() else 0.0


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_conv_dgrad_impulse_response(case, B):
    """One non-zero weight per input channel, tap and output channel moving with the pass: every g_x is one product or exactly 0."""
    rng = np.random.default_rng(case.seed)
    T, Ho = case.ks ** 2, case.out_hw()
    x = np.zeros((B, case.cin, case.H, case.H), dtype=np.float32)
    worst, n_zero = 0.0, 0
    for p in range(T + 1):
        exact_pass = p == T
        gen = R.bf16_exact if exact_pass else R.full_significand
        g = gen(rng, B * case.cout * Ho * Ho).reshape(B, case.cout, Ho, Ho)
        if case.up:                                      # one parity class of pixels: one term per 2 x 2 sum
            mask = np.zeros((Ho, Ho), dtype=np.float32)
            mask[(p >> 1) & 1::2, p & 1::2] = 1
            g = g * mask
        vals = gen(rng, case.cin)
        w = np.zeros((case.cout, case.cin, case.ks, case.ks), dtype=np.float32)
        for ci in range(case.cin):
            tap = (ci + p) % T
            w[(ci * 7 + p) % case.cout, ci, tap // case.ks, tap % case.ks] = vals[ci]
        gx, gxpad, _, _, info = probe_conv_backward(w, x, g, case.stride, case.up)
        case.check_info(info, B)
        want = G.conv2d_backward(x, w, g, case.stride, case.up)[0]      # a single product per element: exact in float64
        zero = want == 0
        n_zero += int(zero.sum())
        assert np.all(gx[zero] == 0), "%s pass %d: an element that sees only padding is not exactly 0" % (case, p)
        assert np.all(gxpad == 0)
        rel = _rel(gx, want)
        if exact_pass:
            assert rel == 0, "%s: bf16-exact products are off by %.3g" % (case, rel)
        else:
            worst = max(worst, rel)
            assert rel <= IMPULSE_GATE, "%s pass %d: off by %.2f x 2^-24 relative" % (case, p, rel / R.U24)
    if case.ks == 3:
        assert n_zero > 0
    _say("dgrad_impulse", "%s B=%d %s" % (case, B, case.dgrad), worst_rel_in_ulp24=worst / R.U24)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_conv_wgrad_impulse_response(case, B):
    """One non-zero output gradient per output channel, at a pixel and image moving with the channel and the pass: every g_w is one
    product or exactly 0 (the tap fell into the padding), g_b is that value."""
    rng = np.random.default_rng(case.seed + 1)
    Ho = case.out_hw()
    w = np.zeros((case.cout, case.cin, case.ks, case.ks), dtype=np.float32)
    worst, n_zero = 0.0, 0
    corners = [(0, 0), (0, Ho - 1), (Ho - 1, 0), (Ho - 1, Ho - 1)]
    for p in range(5):
        exact_pass = p == 4
        gen = R.bf16_exact if exact_pass else R.full_significand
        x = gen(rng, B * case.cin * case.H * case.H).reshape(B, case.cin, case.H, case.H)
        vals = gen(rng, case.cout)
        g = np.zeros((B, case.cout, Ho, Ho), dtype=np.float32)
        for co in range(case.cout):
            oy, ox = corners[(co + p) % 4] if co % 3 == 0 else ((co * 5 + p * 3) % Ho, (co * 11 + p * 7) % Ho)
            g[(co + p) % B, co, oy, ox] = vals[co]
        _, _, gw, gb, info = probe_conv_backward(w, x, g, case.stride, case.up)
        case.check_info(info, B)
        _, want, wantb = G.conv2d_backward(x, w, g, case.stride, case.up)
        zero = want == 0
        n_zero += int(zero.sum())
        assert np.all(gw[zero] == 0), "%s pass %d: a weight whose tap saw only padding is not exactly 0" % (case, p)
        assert np.array_equal(gb.astype(np.float64), wantb), "%s: the bias gradient of a single term is that term" % case
        rel = _rel(gw, want)
        if exact_pass:
            assert rel == 0, "%s: bf16-exact products are off by %.3g" % (case, rel)
        else:
            worst = max(worst, rel)
            assert rel <= IMPULSE_GATE, "%s pass %d: off by %.2f x 2^-24 relative" % (case, p, rel / R.U24)
    if case.ks == 3:
        assert n_zero > 0
    _say("wgrad_impulse", "%s B=%d splits=%s" % (case, B, info["splits"]), worst_rel_in_ulp24=worst / R.U24)


def _dense(case, B, rng):
    Ho = case.out_hw()
    x = R.realistic_activations(rng, (B, case.cin, case.H, case.H))
    w = (rng.standard_normal((case.cout, case.cin, case.ks, case.ks)) * 0.05).astype(np.float32)
    g = (rng.standard_normal((B, case.cout, Ho, Ho)) * 0.05).astype(np.float32)
    return x, w, g


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_conv_backward_dense_within_twice_an_fp32_chain_and_bit_reproducible(case, B):
    rng = np.random.default_rng(case.seed + 2)
    x, w, g = _dense(case, B, rng)
    gx, gxpad, gw, gb, info = probe_conv_backward(w, x, g, case.stride, case.up)
    case.check_info(info, B)
    again = probe_conv_backward(w, x, g, case.stride, case.up)
    for a, b in zip((gx, gxpad, gw, gb), again[:4]):
        assert np.array_equal(_bits(a), _bits(b)), "%s: two runs differ" % case
    ex, ew, eb = G.conv2d_backward(x, w, g, case.stride, case.up)
    ax, aw, ab = G.conv2d_backward_abs(x, w, g, case.stride, case.up)
    cw, cb = G.conv2d_wgrad_chain(x, g, case.ks, case.stride, case.up)
    cx = G.conv2d_dgrad_chain(x.shape, w, g, case.stride, case.up)
    figs = {}
    for name, got, exact, den, chain in (("gx", gx, ex, ax, cx), ("gw", gw, ew, aw, cw), ("gb", gb, eb, ab, cb)):
        e, e_chain = G.normalised_error(got, exact, den), G.normalised_error(chain, exact, den)
        figs[name + "_err"], figs[name + "_chain"], figs[name + "_ratio"] = e, e_chain, e / e_chain
    _say("dense", "%s B=%d %s splits=%s" % (case, B, case.dgrad, info["splits"]), **figs)
    assert np.all(np.isfinite(gx)) and np.all(np.isfinite(gw)) and np.all(np.isfinite(gb)) and np.all(gxpad == 0)
    for name in ("gx", "gw", "gb"):
        assert figs[name + "_err"] <= DENSE_GATE * figs[name + "_chain"], "%s %s: normalised error %.3g is %.2f x the fp32 chain's %.3g" % (
            case, name, figs[name + "_err"], figs[name + "_ratio"], figs[name + "_chain"])


@pytest.mark.parametrize("case", [c for c in CASES if c.cin % 8 or c.cout % 8], ids=[c.id for c in CASES if c.cin % 8 or c.cout % 8])
def test_conv_backward_ignores_padding_channels(case):
    B = 3
    rng = np.random.default_rng(case.seed + 3)
    x, w, g = _dense(case, B, rng)
    Ho = case.out_hw()
    base = probe_conv_backward(w, x, g, case.stride, case.up)
    xf = (rng.standard_normal((B, case.H, case.H, K.pad8(case.cin) - case.cin)) * 1e6).astype(np.float32) if case.cin % 8 else None
    gf = (rng.standard_normal((B, Ho, Ho, K.pad8(case.cout) - case.cout)) * 1e6).astype(np.float32) if case.cout % 8 else None
    dirty = probe_conv_backward(w, x, g, case.stride, case.up, x_fill=xf, g_fill=gf)
    for a, b in zip(base[:4], dirty[:4]):
        assert np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ GroupNorm (+ swish)
@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("Cc", [32, 64, 128, 256, 512])      # 1, 2, 4, 8 and 16 channels per group
def test_group_norm_backward(Cc, swish):
    _check_group_norm_backward(Cc, swish, 8, 1)


def test_group_norm_backward_two_pixel_chunks():
    _check_group_norm_backward(64, 1, 24, 2)                 # 576 pixels: the per-channel sums are folded over two chunks


def _check_group_norm_backward(Cc, swish, H, chunks):
    B = 2
    rng = np.random.default_rng(4000 + Cc + swish)
    x, gamma, beta = K.gn_input(rng, B, Cc, H, H)
    g = rng.standard_normal(x.shape).astype(np.float32)
    mean, rstd = R.group_stats(x)
    mr = np.stack([mean, rstd], -1).astype(np.float32)                 # the tape: what the forward's statistics pass rounds to
    gx, dg, db, info = probe_gn_backward(x, g, mr, gamma, beta, swish)
    assert info["path"] == "k_gnb_partial+k_gnb_apply" and int(info["chunks"]) == chunks, info
    again = probe_gn_backward(x, g, mr, gamma, beta, swish)
    for a, b in zip((gx, dg, db), again[:3]):
        assert np.array_equal(_bits(a), _bits(b)), "two runs differ"
    ex, edg, edb, adg, adb = G.group_norm_backward(x, gamma, beta, swish, g)
    tx, tg, tb = (torch.from_numpy(t).requires_grad_(True) for t in (x, gamma, beta))
    y = F.group_norm(tx, 32, tg, tb, eps=1e-6)
    (F.silu(y) if swish else y).backward(torch.from_numpy(g))

    def gx_err(a):
        scale = np.abs(ex).reshape(B, 32, -1).max(-1)
        return float((np.abs(a - ex).reshape(B, 32, -1).max(-1) / scale).max())

    figs = dict(gx=gx_err(gx), gx_torch=gx_err(tx.grad.numpy()),
                dgamma=G.normalised_error(dg, edg, adg), dgamma_torch=G.normalised_error(tg.grad.numpy(), edg, adg),
                dbeta=G.normalised_error(db, edb, adb), dbeta_torch=G.normalised_error(tb.grad.numpy(), edb, adb))
    _say("groupnorm", "C=%d swish=%d" % (Cc, swish), **figs, **{n + "_ratio": figs[n] / max(figs[n + "_torch"], R.U24) for n in ("gx", "dgamma", "dbeta")})
    for n in ("gx", "dgamma", "dbeta"):
        assert figs[n] <= max(TORCH_FACTOR * figs[n + "_torch"], FLOOR), "C=%d swish=%d %s: error %.3g against torch fp32's %.3g" % (
            Cc, swish, n, figs[n], figs[n + "_torch"])


# ------------------------------------------------------------------------------------------------ attention core
@pytest.mark.parametrize("hw,Cc,path,forward", [(8, 64, "bf16_pipe", "bf16_pipe"), (4, 32, "plain", "scalar")])
def test_attention_backward(hw, Cc, path, forward):
    N = hw * hw
    q, k, v = K.attn_inputs(N, Cc, 2000 + N + Cc)
    go = np.random.default_rng(N + Cc).standard_normal(q.shape).astype(np.float32)
    got, info = probe_attn_backward(q, k, v, go, hw, hw)
    assert info["path"] == path and info["forward"] == forward, info
    again, _ = probe_attn_backward(q, k, v, go, hw, hw)
    exact = G.attention_backward(q, k, v, go)
    tq, tk, tv = (torch.from_numpy(t).requires_grad_(True) for t in (q, k, v))
    (torch.softmax(tq @ tk.transpose(1, 2) * (Cc ** -0.5), dim=-1) @ tv).backward(torch.from_numpy(go))
    for name, a, b, e64, t32 in zip(("gq", "gk", "gv"), got, again, exact, (tq.grad, tk.grad, tv.grad)):
        assert np.array_equal(_bits(a), _bits(b)), "%s: two runs differ" % name
        scale = np.abs(e64).max()
        e, budget = float(np.abs(a - e64).max() / scale), float(np.abs(t32.numpy() - e64).max() / scale)
        _say("attention", "N=%d C=%d %s %s" % (N, Cc, path, name), kernel_err=e, torch_fp32_err=budget, ratio=e / budget)
        assert np.all(np.isfinite(a))
        assert e <= max(TORCH_FACTOR * budget, FLOOR), "attention %s N=%d C=%d: error %.3g is %.2f x torch fp32's %.3g" % (
            name, N, Cc, e, e / budget, budget)
