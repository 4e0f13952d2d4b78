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

The measured ratios are printed on lines starting with VQGRAD (run with -s) and tabulated in DESIGN.md.

Shapes.  The first eleven conv cases are the smallest that reach every dgrad instantiation.  The rest are what a production run
(128 - 512 channels, 256^2 or 512^2 images, attention over 256 or 1024 tokens) launches and the small cases do not, each the
smallest shape that reaches its branch; sizes are (H, W) with H != W wherever the kernels index with both:
  3->128 16x16          the flipped conv has 3 outputs and a size that is a multiple of 16: k_conv_few<3> (8 x 8 stays on k_conv_bx)
  4->32 16x32           k_conv_few<4>
  128->3 16x16          the flipped conv has 8 stored inputs and 4 output tiles: fp32 k_conv<4>;  64->3 16x24: k_conv<2>
  32->32 k3 128x136     K = 17 408 > 64 x 256: wgrad_splits is cut to its cap 64 (one 32 x 32 tile, so the 1024-wave term is far off)
  32->32 k1 256x264     K = 67 584: the same cap, and K / 512 = 132 bias chunks cut to their cap 128
  32->32 k1 136x136     K = 18 496 under the 64 cap: slices of 290 with a last one of 226, 36 bias chunks of 513 or 514 pixels
  256->256 k1 64x72     64 tiles reach 1024 waves with 16 slices although K / 256 = 18: the fill cap; slices of 288, not 256
  512->512 k1 32x40     256 tiles: the fill cap at 4 (K / 256 = 5), slices of 320
  512->512 k3 8x16      16 rounds of 32 input channels through the wide dgrad kernel (two pixel tiles across), 16 x 16 wgrad tiles
  256->128 k3 32x40     five pixel tiles across, an odd count: k_conv_bx<4,3> instead of the wide kernel; 4 x 8 wgrad tiles, 5 slices
  128->128 s2 16x24, 32->256 s2 16x16    k_dgrad_s2 with a 128- and a 256-term inner chain
  256->256 up 8x12      k_sum2x2 and the dgrad at 16 x 24 with H != W
  64->64 k3 8x24, 24x8  the same layer and its transpose
Cases wider than 128 channels run at B = 1 only, which keeps each float64 reference and fp32 chain at a few seconds.
GroupNorm: C = 96, 160, 1024 (thread layouts of k_gnb_partial that are not a power of two / have one pixel row); 1000 pixels (chunks
of 333, 333, 334), 16 640 pixels (the cap of 64 chunks), C = 512 over two chunks.  Attention: 256 and 1024 tokens (k_attn_softmax_bwd
walks a row in 4 and 16 steps of 64 lanes), 8 x 16, and the two ways onto the plain path (C < 64, N < 64)."""
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
def probe_conv_backward(w, x, g, stride=1, up=False, x_fill=None, g_fill=None, bias=True):
    """w [Cout, Cin, ks, ks], x NCHW (the conv's input), g NCHW (gradient of its output) ->
    (g_x NCHW real channels, g_x padding channels, g_w, g_b, info).  bias=False: a bias-free conv, the probe gets a null g_b (and
    fails if the bias part of its workspace was written); g_b comes back as None."""
    lib, L = K._lib()
    cout, cin, ks, _ = w.shape
    B, _, Hs, Ws = x.shape
    wd, xd, gd = K._dev(w), K.to_nhwc(x, x_fill), K.to_nhwc(g, g_fill)
    gx = torch.full((B, Hs, Ws, K.pad8(cin)), float("nan"), dtype=torch.float32, device="cuda")
    gw = torch.full((cout, cin, ks, ks), float("nan"), dtype=torch.float32, device="cuda")
    gb = torch.full((cout,), float("nan"), dtype=torch.float32, device="cuda") if bias else None
    buf = C.create_string_buffer(256)
    lib.check(L.wmar_vq_probe_conv_backward(K._ptr(wd), cout, cin, ks, K._ptr(xd), K._ptr(gd), B, Hs, Ws, stride, int(up), K._ptr(gx),
                                            K._ptr(gw), K._ptr(gb), buf, 256, lib.stream_ptr()))
    torch.cuda.synchronize()
    gxn = K.from_nhwc(gx)
    return gxn[:, :cin], gxn[:, cin:], gw.cpu().numpy(), None if gb is None else gb.cpu().numpy(), K._info(buf)


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
    """hw: the conv's input size, an int (square) or (H, W).  dgrad: the path run_conv_dgrad must report.  batches: the batch sizes
    the case runs at."""

    def __init__(self, cin, cout, ks, hw, dgrad, stride=1, up=False, batches=(1, 3)):
        self.cin, self.cout, self.ks, self.stride, self.up, self.dgrad, self.batches = cin, cout, ks, stride, up, dgrad, tuple(batches)
        self.square = isinstance(hw, int)
        self.H, self.W = (hw, hw) if self.square else hw
        self.seed = (cin * 131 + cout * 17 + ks * 7 + (hw * 3 if self.square else self.H * 3 + self.W * 5) + stride + 2 * int(up)) & 0xffff

    @property
    def id(self):
        size = "%d" % self.H if self.square else "%dx%d" % (self.H, self.W)
        return "%dto%d-k%d-s%d-up%d-%s" % (self.cin, self.cout, self.ks, self.stride, int(self.up), size)

    def out_hw(self):
        m = 2 if self.up else 1
        return self.H * m // self.stride, self.W * m // self.stride

    def K(self, B):
        Ho, Wo = self.out_hw()
        return B * Ho * Wo

    def split_terms(self, B):
        """The three terms of run_conv_wgrad's documented rule: slices of at least 256 products per weight, at most as many as bring
        the launch to 1024 waves, at most 64."""
        tiles = -(-self.cout // 32) * -(-self.cin // 32)
        return -(-self.K(B) // 256), -(-1024 // tiles), 64

    def splits(self, B):
        return max(1, min(self.split_terms(B)))

    def slice_len(self, B):
        """Products per K slice: the even number at or above K / S."""
        return (-(-self.K(B) // self.splits(B)) + 1) & ~1

    def bias_chunks(self, B):
        return min(max(self.K(B) // 512, 1), 128)

    def check_info(self, info, B, bias=True):
        assert info["dgrad"] == self.dgrad, "dgrad launched %s, this case is meant to cover %s" % (info["dgrad"], self.dgrad)
        assert info["wgrad"] == "k_wgrad<%d>" % self.ks, info
        assert int(info["splits"]) == self.splits(B), (info, self.splits(B))
        assert info["bgrad"] == ("k_bgrad_partial" if bias else "none"), info

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
    # ---- what a production run launches (module docstring: why each is the smallest shape that reaches its branch)
    Case(3, 128, 3, 16, "flip+k_conv_few<3>"),                          # conv_in at a multiple of 16: the flipped conv has 3 outputs
    Case(4, 32, 3, (16, 32), "flip+k_conv_few<4>", batches=(1,)),
    Case(128, 3, 3, 16, "flip+k_conv<4>"),                              # conv_out: the flipped conv has 8 stored inputs, 4 cout tiles
    Case(64, 3, 3, (16, 24), "flip+k_conv<2>", batches=(1,)),
    Case(32, 32, 3, (128, 136), "flip+k_conv_bx<1,3>", batches=(1,)),   # K = 17 408: the 64 cap, 34 bias chunks
    Case(32, 32, 1, (256, 264), "flip+k_conv_bx<1,1>", batches=(1,)),   # K = 67 584: the 64 cap, bias chunks at their cap 128
    Case(32, 32, 1, 136, "flip+k_conv_bx<1,1>", batches=(1,)),          # K = 18 496: the 64 cap, short last slice, uneven bias chunks
    Case(256, 256, 1, (64, 72), "flip+k_conv_bx<4,1>", batches=(1,)),   # 64 tiles: the fill cap 16
    Case(512, 512, 1, (32, 40), "flip+k_conv_bx<4,1>", batches=(1,)),   # 256 tiles: the fill cap 4
    Case(512, 512, 3, (8, 16), "flip+k_conv_bx<4,3,4>", batches=(1,)),  # 16 input rounds on the wide dgrad kernel, 16 x 16 wgrad tiles
    Case(256, 128, 3, (32, 40), "flip+k_conv_bx<4,3>", batches=(1,)),   # odd tiles_x: not the wide kernel; CT != CIT; S = 5
    Case(128, 128, 3, (16, 24), "k_dgrad_s2", stride=2),
    Case(32, 256, 3, 16, "k_dgrad_s2", stride=2, batches=(1,)),
    Case(256, 256, 3, (8, 12), "flip+k_conv_bx<4,3>+k_sum2x2", up=True, batches=(1,)),     # 16 x 24 behind the upsampling: tiles_x = 3
    Case(64, 64, 3, (8, 24), "flip+k_conv_bx<2,3>", batches=(3,)),
    Case(64, 64, 3, (24, 8), "flip+k_conv_bx<2,3>", batches=(3,)),      # the same layer transposed
]
_ids = [c.id for c in CASES]
RUNS = [(c, B) for c in CASES for B in c.batches]
_run_ids = ["%s-%d" % (c.id, B) for c, B in RUNS]


def test_the_cases_cover_one_and_several_wgrad_splits():
    by = {c.id: c for c in CASES}
    assert len(by) == len(CASES)
    assert by["32to32-k3-s1-up0-8"].splits(1) == 1 and by["32to32-k3-s1-up0-8"].splits(3) == 1        # K = 64, 192
    assert by["64to128-k3-s1-up0-16"].splits(1) == 1 and by["64to128-k3-s1-up0-16"].splits(3) == 3    # K = 256 (exactly one), 768
    assert by["64to64-k3-s1-up0-24"].splits(1) == 3 and by["64to64-k3-s1-up0-24"].splits(3) == 7      # K = 576, 1728: uneven slices
    assert by["3to128-k3-s1-up0-16"].splits(1) == 1 and by["3to128-k3-s1-up0-16"].splits(3) == 3
    assert by["128to3-k3-s1-up0-16"].splits(1) == 1 and by["128to3-k3-s1-up0-16"].splits(3) == 3
    # the 64 cap binds: more than 64 slices of 256 products, few tiles
    c = by["32to32-k3-s1-up0-128x136"]
    assert c.split_terms(1) == (68, 1024, 64) and c.splits(1) == 64 and c.slice_len(1) == 272 and c.bias_chunks(1) == 34
    c = by["32to32-k1-s1-up0-256x264"]
    assert c.split_terms(1) == (264, 1024, 64) and c.splits(1) == 64 and c.slice_len(1) == 1056
    assert c.K(1) // 512 == 132 and c.bias_chunks(1) == 128                                           # the bias chunks' own cap
    c = by["32to32-k1-s1-up0-136"]
    assert c.split_terms(1) == (73, 1024, 64) and c.splits(1) == 64 and c.slice_len(1) == 290
    assert c.K(1) - 63 * 290 == 226                                                                   # a short last slice under the cap
    assert c.bias_chunks(1) == 36 and c.K(1) % 36 != 0                                                # bias chunks of 513 and 514 pixels
    # the fill cap binds: 1024 waves are reached with fewer slices than K / 256
    c = by["256to256-k1-s1-up0-64x72"]
    assert c.split_terms(1) == (18, 16, 64) and c.splits(1) == 16 and c.slice_len(1) == 288
    c = by["512to512-k1-s1-up0-32x40"]
    assert c.split_terms(1) == (5, 4, 64) and c.splits(1) == 4 and c.slice_len(1) == 320
    c = by["512to512-k3-s1-up0-8x16"]
    assert c.split_terms(1) == (1, 4, 64) and c.splits(1) == 1
    c = by["256to128-k3-s1-up0-32x40"]
    assert c.split_terms(1) == (5, 32, 64) and c.splits(1) == 5 and c.slice_len(1) == 256             # no cap: 5 slices of exactly 256
    assert by["128to128-k3-s2-up0-16x24"].splits(3) == 2 and by["128to128-k3-s2-up0-16x24"].slice_len(3) == 144
    for a, b in (("64to64-k3-s1-up0-8x24", "64to64-k3-s1-up0-24x8"),):
        assert by[a].splits(3) == by[b].splits(3) == 3 and (by[a].H, by[a].W) == (by[b].W, by[b].H)


def _rel(got, want):
    nz = want != 0
    return (np.abs(got.astype(np.float64) - want)[nz] / np.abs(want)[nz]).max() if nz.any() else 0.0


@pytest.mark.parametrize("case,B", RUNS, ids=_run_ids)
def test_conv_dgrad_impulse_response(case, B):
    """One non-zero weight per input channel, tap and output channel moving with the pass: every g_x is one product or exactly 0."""
    rng = np.random.default_rng(case.seed)
    T, (Ho, Wo) = case.ks ** 2, case.out_hw()
    x = np.zeros((B, case.cin, case.H, case.W), dtype=np.float32)
    worst, n_zero = 0.0, 0
    for p in range(T + 1):
        exact_pass = p == T
        gen = R.bf16_exact if exact_pass else R.full_significand
        g = gen(rng, B * case.cout * Ho * Wo).reshape(B, case.cout, Ho, Wo)
        if case.up:                                      # one parity class of pixels: one term per 2 x 2 sum
            mask = np.zeros((Ho, Wo), dtype=np.float32)
            mask[(p >> 1) & 1::2, p & 1::2] = 1
            g = g * mask
        vals = gen(rng, case.cin)
        w = np.zeros((case.cout, case.cin, case.ks, case.ks), dtype=np.float32)
        for ci in range(case.cin):
            tap = (ci + p) % T
            w[(ci * 7 + p) % case.cout, ci, tap // case.ks, tap % case.ks] = vals[ci]
        gx, gxpad, _, _, info = probe_conv_backward(w, x, g, case.stride, case.up)
        case.check_info(info, B)
        want = G.conv2d_dgrad(x.shape, w, g, case.stride, case.up)      # a single product per element: exact in float64
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


@pytest.mark.parametrize("case,B", RUNS, ids=_run_ids)
def test_conv_wgrad_impulse_response(case, B):
    """One non-zero output gradient per output channel, at a pixel and image moving with the channel and the pass: every g_w is one
    product or exactly 0 (the tap fell into the padding), g_b is that value."""
    rng = np.random.default_rng(case.seed + 1)
    Ho, Wo = case.out_hw()
    w = np.zeros((case.cout, case.cin, case.ks, case.ks), dtype=np.float32)
    worst, n_zero = 0.0, 0
    corners = [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1)]
    for p in range(5):
        exact_pass = p == 4
        gen = R.bf16_exact if exact_pass else R.full_significand
        x = gen(rng, B * case.cin * case.H * case.W).reshape(B, case.cin, case.H, case.W)
        vals = gen(rng, case.cout)
        g = np.zeros((B, case.cout, Ho, Wo), dtype=np.float32)
        for co in range(case.cout):
            oy, ox = corners[(co + p) % 4] if co % 3 == 0 else ((co * 5 + p * 3) % Ho, (co * 11 + p * 7) % Wo)
            g[(co + p) % B, co, oy, ox] = vals[co]
        _, _, gw, gb, info = probe_conv_backward(w, x, g, case.stride, case.up)
        case.check_info(info, B)
        want, wantb = G.conv2d_wgrad(x, g, case.ks, case.stride, case.up), g.astype(np.float64).sum((0, 2, 3))
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
    Ho, Wo = case.out_hw()
    x = R.realistic_activations(rng, (B, case.cin, case.H, case.W))
    w = (rng.standard_normal((case.cout, case.cin, case.ks, case.ks)) * 0.05).astype(np.float32)
    g = (rng.standard_normal((B, case.cout, Ho, Wo)) * 0.05).astype(np.float32)
    return x, w, g


@pytest.mark.parametrize("case,B", RUNS, ids=_run_ids)
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
    B = case.batches[-1]
    rng = np.random.default_rng(case.seed + 3)
    x, w, g = _dense(case, B, rng)
    Ho, Wo = case.out_hw()
    base = probe_conv_backward(w, x, g, case.stride, case.up)
    case.check_info(base[4], B)
    xf = (rng.standard_normal((B, case.H, case.W, K.pad8(case.cin) - case.cin)) * 1e6).astype(np.float32) if case.cin % 8 else None
    gf = (rng.standard_normal((B, Ho, Wo, K.pad8(case.cout) - case.cout)) * 1e6).astype(np.float32) if case.cout % 8 else None
    dirty = probe_conv_backward(w, x, g, case.stride, case.up, x_fill=xf, g_fill=gf)
    for a, b in zip(base[:4], dirty[:4]):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("cid,B", [("32to32-k3-s1-up0-8", 1), ("64to64-k3-s1-up0-24", 3), ("256to256-k1-s1-up0-64x72", 1)])
def test_bias_free_conv_backward_gives_the_same_bits_and_leaves_the_bias_workspace_alone(cid, B):
    """The MaskGIT plan's bias-free convs call run_conv_wgrad without a bias gradient.  With one, several and a capped number of K
    slices: g_x and g_w are bit-equal to the call with a bias, no bias kernel is reported, and the probe -- which gives the workspace
    the size a bias needs and fills it with a sentinel -- would fail the call had the bias part been written."""
    case = {c.id: c for c in CASES}[cid]
    x, w, g = _dense(case, B, np.random.default_rng(case.seed + 4))
    gx, gxpad, gw, gb, info = probe_conv_backward(w, x, g, case.stride, case.up)
    case.check_info(info, B)
    fx, fxpad, fw, fb, finfo = probe_conv_backward(w, x, g, case.stride, case.up, bias=False)
    case.check_info(finfo, B, bias=False)
    assert fb is None and np.all(np.isfinite(gb))
    assert {k: v for k, v in finfo.items() if k != "bgrad"} == {k: v for k, v in info.items() if k != "bgrad"}
    for a, b in ((gx, fx), (gxpad, fxpad), (gw, fw)):
        assert np.array_equal(_bits(a), _bits(b)), "%s: the bias-free call changed a bit" % case


# ------------------------------------------------------------------------------------------------ GroupNorm (+ swish)
@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("Cc", [32, 64, 128, 256, 512, 96, 160, 1024])
def test_group_norm_backward(Cc, swish):
    """1, 2, 4, 8 and 16 channels per group; then the thread layouts of k_gnb_partial (col = tid % (C / 4), 256 / (C / 4) pixel rows)
    that are not a power of two or leave one row: C = 96 (24 columns, 10 rows, 16 idle threads), C = 160 (5 channels per group: a
    float4 straddles two groups), C = 1024 (256 columns, one row: the widest run_gn_backward admits)."""
    _check_group_norm_backward(Cc, swish, 8, 1)


def test_group_norm_backward_two_pixel_chunks():
    _check_group_norm_backward(64, 1, 24, 2)                 # 576 pixels: the per-channel sums are folded over two chunks


@pytest.mark.parametrize("Cc,hw,chunks", [(64, (25, 40), 3), (32, (128, 130), 64), (512, (24, 24), 2)], ids=["C64-1000px", "C32-16640px", "C512-576px"])
def test_group_norm_backward_uneven_and_capped_pixel_chunks(Cc, hw, chunks):
    """1000 pixels: three chunks of 333 / 333 / 334 (chunk * HW / nchunk with a remainder).  16 640 pixels: HW / 256 = 65 is cut to
    the cap 64, 260 pixels per chunk.  C = 512 over 576 pixels: two pixel rows per workgroup pass, two chunks."""
    _check_group_norm_backward(Cc, 1, hw, chunks)


def _check_group_norm_backward(Cc, swish, hw, chunks):
    B = 2
    H, W = (hw, hw) if isinstance(hw, int) else hw
    rng = np.random.default_rng(4000 + Cc + swish)
    x, gamma, beta = K.gn_input(rng, B, Cc, H, W)
    g = rng.standard_normal(x.shape).astype(np.float32)
    mean, rstd = R.group_stats(x)
    mr = np.stack([mean, rstd], -1).astype(np.float32)                 # the tape: what the forward's statistics pass rounds to
    gx, dg, db, info = probe_gn_backward(x, g, mr, gamma, beta, swish)
    assert chunks == min(max(H * W // 256, 1), 64)                     # gnb_chunks restated
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
    _say("groupnorm", "C=%d HW=%d chunks=%d swish=%d" % (Cc, H * W, chunks, swish), **figs, **{n + "_ratio": figs[n] / max(figs[n + "_torch"], R.U24) for n in ("gx", "dgamma", "dbeta")})
    for n in ("gx", "dgamma", "dbeta"):
        assert figs[n] <= max(TORCH_FACTOR * figs[n + "_torch"], FLOOR), "C=%d swish=%d %s: error %.3g against torch fp32's %.3g" % (
            Cc, swish, n, figs[n], figs[n + "_torch"])


# ------------------------------------------------------------------------------------------------ attention core
@pytest.mark.parametrize("hw,Cc,path,forward", [(8, 64, "bf16_pipe", "bf16_pipe"), (4, 32, "plain", "scalar")])
def test_attention_backward(hw, Cc, path, forward):
    _check_attention_backward(hw, hw, Cc, 2, path, forward)


@pytest.mark.parametrize("H,W,Cc,B,path,forward", [
    (16, 16, 512, 1, "bf16_pipe", "bf16_pipe"),      # Taming's attention: 256 tokens, k_attn_softmax_bwd's row loop runs 4 times
    (32, 32, 64, 1, "bf16_pipe", "bf16_pipe"),       # 1024 tokens (Chameleon's count): the row loop runs 16 times
    (8, 16, 64, 2, "bf16_pipe", "bf16_pipe"),        # non-square on the matrix path
    (16, 16, 32, 2, "plain", "scalar"),              # C < 64: k_bmm_plain over 256 tokens, the row loop runs 4 times
    (4, 4, 64, 2, "plain", "scalar"),                # N < 64 alone sends a 64-channel block to the plain path
], ids=["16x16-C512", "32x32-C64", "8x16-C64", "16x16-C32", "4x4-C64"])
def test_attention_backward_at_production_token_counts(H, W, Cc, B, path, forward):
    _check_attention_backward(H, W, Cc, B, path, forward)


def _check_attention_backward(H, W, Cc, B, path, forward):
    """K.attn_inputs' second image has a query row of zeros (row 7): all its scores are equal, P = 1 / N, and its dS row is
    scale (dP - mean(dP)) / N.  dS is seen through dQ = dS K: that row of dQ is held to the gate on its own, normalised by its own
    largest element (it is far smaller than the rows with a peaked softmax, which set the tensor's maximum)."""
    N = H * W
    q, k, v = K.attn_inputs(N, Cc, 2000 + N + Cc)
    if B == 1:
        q, k, v = (np.ascontiguousarray(t[1:]) for t in (q, k, v))
    go = np.random.default_rng(N + Cc).standard_normal(q.shape).astype(np.float32)
    got, info = probe_attn_backward(q, k, v, go, H, W)
    assert info["path"] == path and info["forward"] == forward, info
    again, _ = probe_attn_backward(q, k, v, go, H, W)
    exact = G.attention_backward(q, k, v, go)
    tq, tk, tv = (torch.from_numpy(t).requires_grad_(True) for t in (q, k, v))
    (torch.softmax(tq @ tk.transpose(1, 2) * (Cc ** -0.5), dim=-1) @ tv).backward(torch.from_numpy(go))
    for name, a, b, e64, t32 in zip(("gq", "gk", "gv"), got, again, exact, (tq.grad, tk.grad, tv.grad)):
        assert np.array_equal(_bits(a), _bits(b)), "%s: two runs differ" % name
        scale = np.abs(e64).max()
        e, budget = float(np.abs(a - e64).max() / scale), float(np.abs(t32.numpy() - e64).max() / scale)
        _say("attention", "%dx%d N=%d C=%d B=%d %s %s" % (H, W, N, Cc, B, path, name), kernel_err=e, torch_fp32_err=budget, ratio=e / budget)
        assert np.all(np.isfinite(a))
        assert e <= max(TORCH_FACTOR * budget, FLOOR), "attention %s N=%d C=%d: error %.3g is %.2f x torch fp32's %.3g" % (
            name, N, Cc, e, e / budget, budget)
    b, row = B - 1, 7
    assert not q[b, row].any()
    dp = v[b].astype(np.float64) @ go[b, row].astype(np.float64)
    want = (Cc ** -0.5) * ((dp - dp.mean()) / N) @ k[b].astype(np.float64)
    top = np.abs(want).max()
    assert np.abs(exact[0][b, row] - want).max() <= 1e-10 * top, "the float64 reference disagrees with the closed form of an equal-score row"
    e, budget = float(np.abs(got[0][b, row] - want).max() / top), float(np.abs(tq.grad[b, row].numpy() - want).max() / top)
    _say("attention", "%dx%d N=%d C=%d B=%d %s equal_score_row" % (H, W, N, Cc, B, path), kernel_err=e, torch_fp32_err=budget,
         ratio=e / max(budget, R.U24), row_over_tensor_max=top / np.abs(exact[0]).max())
    assert e <= max(TORCH_FACTOR * budget, FLOOR), "equal-score row N=%d C=%d: error %.3g against torch fp32's %.3g" % (N, Cc, e, budget)
