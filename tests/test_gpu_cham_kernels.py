"""Every launch of a Chameleon decode step alone, through a live engine's own plan and buffers (wmar_cham_probe_run /
wmar_cham_probe_copy / wmar_cham_probe_plan), against the float64 statement of that one operation in
tests/cham_kernel_reference.py.  Engines have one block and are created from bf16-exact fp32 tensors (tensors_bf16 = 0), so
the operands the kernels multiply are known exactly and most expectations are bits, not tolerances.

Every test asserts the kernel instantiations and the stream-K decomposition (C, U, G) the plan reports and prints its figures
on lines starting CHAMK (run with -s).  Measured on an MI355X: 259 cases, 57 .. 60 s.

Not reachable through an engine, so covered on the CPU only (tests/test_cham_kernel_reference.py): weight rows past N in the
last tile of k_bpack (wmar_cham_create rejects widths that are no multiple of 32)."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cham_oracle as CO  # noqa: E402
from tests import cham_kernel_reference as R  # noqa: E402
from tests.conftest import REPO  # noqa: E402
from tests.engine_probe import EngineProbe, dev, parse_plan, say  # noqa: E402
from tests.test_gpu_chameleon_parity import SWEEP, _cham_cfg, decomposition  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402

WIDTHS = [(1024, 8, 8, 1024, 64), (1536, 12, 4, 2080, 64), (320, 5, 1, 1056, 16)]
assert all(w in SWEEP for w in WIDTHS)
# (max_rows, M): all four MT templates; M = 1, 31, 32, 33, 32 MT - 1 where they fit, and 5 of 128 (three wholly empty row tiles)
ROWS = [(R_, M) for R_, Ms in ((32, (1, 31, 32)), (64, (1, 31, 32, 33, 63)), (96, (1, 31, 32, 33, 95)), (128, (1, 5, 31, 32, 33, 127)))
        for M in Ms]
_ID = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))

_say = say("CHAMK", 34)


class Probe(EngineProbe):
    """One wmar_cham engine and stage access to it."""
    ENGINE = "cham"
    DTYPES = {"x": torch.int16, "y": torch.int16, "hbuf": torch.int16, "slabs": torch.float32, "big_slabs": torch.float32, "ssq": torch.float64,
              "kcache": torch.int16, "vcache": torch.int16, "rope": torch.float32, "wqkv": torch.int16, "wo": torch.int16, "w13": torch.int16,
              "w2": torch.int16, "whead": torch.int16}

    def __init__(self, cfg, sd, max_rows, max_seq_len=16, src_bf16=False):
        from wmar_amd import _lib
        self.cfg, self.max_rows, self.MT, self.T = cfg, max_rows, (max_rows + 31) // 32, max_seq_len
        self.Mpad = 32 * self.MT
        c = _lib.ChamConfig(cfg.dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size, cfg.ffn_hidden, cfg.norm_eps,
                            cfg.rope_theta, int(cfg.qk_normalization), 0, max_rows, max_seq_len, int(src_bf16))
        self._create(c, sd, dtype=torch.bfloat16 if src_bf16 else torch.float32)

    def run(self, first, last, M, tok=None, pos=None, want_logits=False):
        return self._call(self._run, M, self.cfg.vocab_size, dev(tok), dev(pos, torch.int32), M, 0, first, last, want_logits=want_logits)

    def forward(self, tok, pos):
        return self._call(self.L.wmar_cham_forward_tokens, len(tok), self.cfg.vocab_size, dev(tok), dev(pos, torch.int32), len(tok))

    def plan(self, M):
        return parse_plan(self.plan_text(M, buflen=512), list_keys=(), ints=False)

    # ---- packed buffers as [Mpad, width] arrays
    def put_act(self, name, X):
        self.put(name, R.pack_act(R.bf_bits(X), self.MT))

    def get_act(self, name, K):
        return R.bits_f32(R.unpack_act(self.get(name), self.MT, K))

    def get_pieces(self, name, N):
        """[BG_MAXP][Mpad, N] in tile order; a piece's stride is the producing GEMM's own width"""
        flat = self.get(name)
        stride = N * self.Mpad
        return R.unpack_slab(flat[:R.BG_MAXP * stride].reshape(R.BG_MAXP, stride), self.MT, N)

    def put_pieces(self, name, P):
        self.put_front(name, np.stack([R.pack_slab(P[p], self.MT) for p in range(R.BG_MAXP)]).reshape(-1).astype(np.float32))


def _sks(cfg):
    D, Dkv, F = cfg.dim, cfg.n_kv_heads * cfg.head_dim, cfg.ffn_hidden
    return {"sk_qkv": R._sk_for((D + 2 * Dkv) // 32, D // 16, False), "sk_o": R._sk_for(D // 32, D // 16, False),
            "sk_13": R._sk_for(F // 16, D // 16, False), "sk_2": R._sk_for(D // 32, F // 16, False),
            "sk_head": R._sk_for(cfg.vocab_size // 32, D // 16, True)}


def _assert_plan(pr, M, nwa=2):
    """the dispatch launches the instantiations this test is about, on the decomposition the references restate"""
    plan = pr.plan(M)
    assert plan["MT"] == str(pr.MT)
    for name, k in _sks(pr.cfg).items():
        assert plan[name] == "%d,%d,%d" % k, (name, plan[name], k)
    assert plan["kernels"] == "k_bgemm<%d,SLAB>;k_bgemm<%d,LOGITS>;k_cham_attn<%d,%d>" % (pr.MT, pr.MT, pr.cfg.head_dim, nwa), plan["kernels"]
    return plan


def _gemms(cfg):
    """name -> (stage, input buffer, K, weight key, gamma key, pack mode, slab buffer, tile-order width, sk name, packed weight)"""
    D, Dkv, F = cfg.dim, cfg.n_kv_heads * cfg.head_dim, cfg.ffn_hidden
    p = "layers.0."
    return {"qkv": (R.QKV, "x", D, p + "attention.wqkv.weight", p + "attention_norm.weight", 0, "big_slabs", D + 2 * Dkv, "sk_qkv", "wqkv"),
            "wo": (R.WO, "y", D, p + "attention.wo.weight", None, 0, "slabs", D, "sk_o", "wo"),
            "w13": (R.W13, "x", D, p + "feed_forward.w13.weight", p + "ffn_norm.weight", 1, "big_slabs", 2 * F, "sk_13", "w13"),
            "w2": (R.W2, "hbuf", F, p + "feed_forward.w2.weight", None, 0, "slabs", D, "sk_2", "w2")}


def _tile(cfg, sd, name):
    _, _, _, wk, gk, mode, _, _, _, _ = _gemms(cfg)[name]
    return R.tile_weight(sd[wk], sd[gk] if gk else None, mode, cfg.ffn_hidden)


def _int_state(cfg, seed):
    """integer weights in -4..4, gammas powers of two, embedding rows in -8..8 (row 1 all zero): every product and partial sum is an
    integer below 2^24"""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in synth.chameleon_shapes(cfg).items():
        if k.endswith("norm.weight"):
            sd[k] = (2.0 ** rs.randint(-1, 2, size=shp)).astype(np.float32)
        elif k == "tok_embeddings.weight":
            sd[k] = rs.randint(-8, 9, size=shp).astype(np.float32)
            sd[k][1] = 0
        else:
            sd[k] = rs.randint(-4, 5, size=shp).astype(np.float32)
    return sd


def _dense_state(cfg, seed):
    return {k: v.float().numpy() for k, v in synth.synth_chameleon_state(cfg, seed=seed, logit_scale=4.0).items()}


@functools.lru_cache(maxsize=2)
def _engine(shape, max_rows, kind, max_seq_len=16, qk=False):
    cfg = _cham_cfg(*shape, layers=1, qk=qk)
    sd = _int_state(cfg, sum(shape)) if kind == "int" else _dense_state(cfg, sum(shape))
    return Probe(cfg, sd, max_rows, max_seq_len), sd


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _engine.cache_clear()


# ------------------------------------------------------------------------------------------------------------------ k_bpack
@pytest.mark.parametrize("src_bf16", [0, 1])
@pytest.mark.parametrize("shape", WIDTHS, **_ID)
def test_weight_packing_is_bit_exact(shape, src_bf16):
    """wqkv, wo, w13 (mode 1), w2, whead of a random engine == the numpy pack of bf16(W * gamma), from fp32 and from bf16 sources"""
    cfg = _cham_cfg(*shape, layers=1, qk=False)
    sd = _dense_state(cfg, 3)
    if not src_bf16:        # fp32 sources that are NOT bf16 values: the pack-time rounding of W * gamma is part of the check
        rs = np.random.RandomState(5)
        sd = {k: (v * (1 + 2.0 ** -10 * rs.randn(*v.shape))).astype(np.float32) if v.ndim == 2 and k != "tok_embeddings.weight" else v
              for k, v in sd.items()}
    pr = Probe(cfg, sd, 32, 16, bool(src_bf16))
    _assert_plan(pr, 1)
    n = 0
    for name in _gemms(cfg):
        n += R.check_pack(pr.get(_gemms(cfg)[name][9]), _tile(cfg, sd, name))
    n += R.check_pack(pr.get("whead"), R.tile_weight(sd["output.weight"], sd["norm.weight"]))
    _say("pack %s bf16=%d" % ("x".join(map(str, shape[:3])), src_bf16), differing_bits=n)


# ------------------------------------------------------------------------------------------------------------------ k_bgemm<MT, SLAB>
@pytest.mark.parametrize("rows", ROWS, **_ID)
@pytest.mark.parametrize("shape", WIDTHS, **_ID)
def test_gemm_pieces_exact_and_padding(shape, rows):
    """Integer operands: each piece of each group equals the integer partial sum over exactly its k-blocks bit for bit; slots of
    pieces past sk_count(g) and rows >= M keep the sentinel written before the launch.  Then NaN in rows >= M of the packed input
    changes no bit."""
    max_rows, M = rows
    pr, sd = _engine(shape, max_rows, "int")
    cfg = pr.cfg
    plan = _assert_plan(pr, M)
    rs = np.random.RandomState(M)
    bad = 0
    for name, (stage, inp, K, _, _, _, slabs, N, skn, _) in _gemms(cfg).items():
        k = _sks(cfg)[skn]
        Wt = _tile(cfg, sd, name)
        X = rs.randint(-8, 9, size=(pr.Mpad, K)).astype(np.float32)
        pr.put_act(inp, X)
        pr.fill(slabs, float(R.SENTINEL))
        pr.run(stage, stage, M)
        got = pr.get_pieces(slabs, N)
        bad += R.check_gemm_exact(got, Wt, X, k, M)
        if M < pr.Mpad:
            Xn = X.copy()
            Xn[M:] = np.nan
            pr.put_act(inp, Xn)
            pr.fill(slabs, float(R.SENTINEL))
            pr.run(stage, stage, M)
            d = R.diff_bits(pr.get_pieces(slabs, N), got)
            assert d == 0, "%s: NaN in the padding rows of the input changed %d floats" % (name, d)
    _say("gemm exact %s R%d M%d" % ("x".join(map(str, shape[:3])), max_rows, M), differing_bits=bad, plan=";".join(plan[s] for s in _sks(cfg)))


@pytest.mark.parametrize("rows", ROWS, **_ID)
@pytest.mark.parametrize("shape", WIDTHS, **_ID)
def test_gemm_pieces_dense(shape, rows):
    """Random bf16 operands: per piece, max |got - exact| / sum |terms| <= DENSE_GATE x the same figure of a sequential fp32 chain
    over the same terms, measured in the same run on the CPU."""
    max_rows, M = rows
    pr, sd = _engine(shape, max_rows, "dense")
    cfg = pr.cfg
    _assert_plan(pr, M)
    rs = np.random.RandomState(M + 1)
    for name, (stage, inp, K, _, _, _, slabs, N, skn, _) in _gemms(cfg).items():
        k = _sks(cfg)[skn]
        X = np.zeros((pr.Mpad, K), dtype=np.float32)
        X[:M] = R.bf(rs.randn(M, K).astype(np.float32))
        pr.put_act(inp, X)
        pr.run(stage, stage, M)
        e, ec, worst = R.check_gemm_dense(pr.get_pieces(slabs, N), _tile(cfg, sd, name), X, k, M)
        _say("gemm dense %s %s R%d M%d" % (name, "x".join(map(str, shape[:3])), max_rows, M), err=e, chain=ec, worst_ratio=worst)


# ------------------------------------------------------------------------------------------------------------------ consumers
@pytest.mark.parametrize("rows", ROWS, **_ID)
@pytest.mark.parametrize("shape", WIDTHS, **_ID)
def test_embed_resid_swiglu(shape, rows):
    """EMBED: gathered rows (tokens 0 and V - 1 among them), zero padding rows, ssq.  RESID_ATTN / RESID_FFN: x' == bf(x + bf(fp32
    sum of the pieces in piece order)) and ssq, with NaN in the padding rows of the slabs and of x.  SWIGLU: each output is
    bf(v) of the float64 value v in front of every rounding, or one of the two neighbours where v is within delta of a midpoint.

    delta (tests/cham_kernel_reference.py, DELTA_RSTD and DELTA_SILU), relative, from the documented bounds of HIP's rsqrtf and
    expf (1 ulp each) plus one fp32 rounding per arithmetic step: u = bf(rstd * acc): 2^-24 (rounded mean and + eps, halved by the
    square root) + 2 * 2^-24 (rsqrtf) + 2^-24 (product) = 4 * 2^-24; silu(u) = u / (1 + expf(-u)): 2 * 2^-24 (expf, through 1 + e) +
    2^-24 (the sum) + 5 * 2^-24 (a division bound of 2.5 ulp) = 8 * 2^-24; bf(silu) * u3 is exact in fp32.  Both candidates of an
    undecided u1 and of an undecided bf(silu(u1)) are propagated."""
    max_rows, M = rows
    pr, sd = _engine(shape, max_rows, "dense")
    cfg = pr.cfg
    D, F, V, eps = cfg.dim, cfg.ffn_hidden, cfg.vocab_size, cfg.norm_eps
    _assert_plan(pr, M)
    sks = _sks(cfg)
    rs = np.random.RandomState(M + 2)
    tok = rs.randint(0, V, size=M)
    tok[0] = 0
    tok[-1] = V - 1
    if M > 2:
        tok[1] = V - 1
    pr.fill("x", 0x7fc0)                           # NaN everywhere: EMBED must write every row, the padding rows as zeros
    pr.run(R.EMBED, R.EMBED, M, tok, np.zeros(M, dtype=np.int32))
    x = pr.get_act("x", D)
    want = R.embed_ref(R.bf(sd["tok_embeddings.weight"]), tok, pr.Mpad)
    bad = R.diff_bits(x, want)
    assert bad == 0, "EMBED: %d elements differ" % bad
    figs = {"embed_bits": bad, "embed_ssq": R.check_ssq(pr.get("ssq").reshape(-1, pr.Mpad), x, M)}
    # residual updates behind wo (sk_o) and behind w2 (sk_2)
    for stage_g, stage_r, inp, K, skn, tag in ((R.WO, R.RESID_ATTN, "y", D, "sk_o", "resid_attn"), (R.W2, R.RESID_FFN, "hbuf", F, "sk_2", "resid_ffn")):
        A = np.zeros((pr.Mpad, K), dtype=np.float32)
        A[:M] = R.bf(rs.randn(M, K).astype(np.float32))
        pr.put_act(inp, A)
        pr.run(stage_g, stage_g, M)
        pieces = pr.get_pieces("slabs", D)
        x_old = pr.get_act("x", D)
        if M < pr.Mpad:
            pn, xn = pieces.copy(), x_old.copy()
            pn[:, M:] = np.nan
            xn[M:] = np.nan
            pr.put_pieces("slabs", pn)
            pr.put_act("x", xn)
        pr.run(stage_r, stage_r, M)
        x_new = pr.get_act("x", D)
        b, s = R.check_resid(x_new, pr.get("ssq").reshape(-1, pr.Mpad), x_old, pieces, R.pieces_of(sks[skn], D // 32), M)
        figs[tag + "_bits"], figs[tag + "_ssq"] = b, s
        if M < pr.Mpad:                         # leave finite padding rows behind for the next stage
            xf = x_new.copy()
            xf[M:] = 0
            pr.put_act("x", xf)
    # SwiGLU on the w13 pieces of the current x and its statistics
    pr.run(R.W13, R.W13, M)
    pieces = pr.get_pieces("big_slabs", 2 * F)
    ssq = pr.get("ssq").reshape(-1, pr.Mpad)
    pr.run(R.SWIGLU, R.SWIGLU, M)
    figs["swiglu_undecided"] = R.check_swiglu(pr.get_act("hbuf", F), pieces, R.pieces_of(sks["sk_13"], F // 16), ssq, D, eps, F, M)
    _say("consumers %s R%d M%d" % ("x".join(map(str, shape[:3])), max_rows, M), **figs)


@pytest.mark.parametrize("rows", ROWS, **_ID)
@pytest.mark.parametrize("shape", WIDTHS, **_ID)
def test_head_integer_operands(shape, rows):
    """HEAD (k_bgemm<MT, LOGITS>) with integer operands: the accumulator is exact, so each logit is bf(rstd * acc) under the
    undecided rule (delta = 4 * 2^-24, as for u above).  Token 1 embeds to an all-zero row: its logits are exact zeros whatever
    rsqrtf returns -- the one construction in which 1/rms is irrelevant to exactness (rsqrtf is documented to 1 ulp even at powers
    of four, so no non-zero row can be required to be exact).  NaN in the padding rows of x changes nothing.  With random operands
    the accumulator of this epilogue is not known exactly (it never leaves the registers), and a bound on it from the fp32 chain
    would leave well over 1 % of the logits undecided: the rule is applied with integer operands only."""
    max_rows, M = rows
    pr, sd = _engine(shape, max_rows, "int")
    cfg = pr.cfg
    D, V, eps = cfg.dim, cfg.vocab_size, cfg.norm_eps
    _assert_plan(pr, M)
    rs = np.random.RandomState(M + 3)
    tok = rs.randint(2, V, size=M)
    tok[M // 2] = 1
    pr.run(R.EMBED, R.EMBED, M, tok, np.zeros(M, dtype=np.int32))
    x = pr.get_act("x", D)
    ssq = pr.get("ssq").reshape(-1, pr.Mpad)
    if M < pr.Mpad:
        xn = x.copy()
        xn[M:] = np.nan
        pr.put_act("x", xn)
    lg = pr.run(R.HEAD, R.HEAD, M, want_logits=True)
    Wt = R.tile_weight(sd["output.weight"], sd["norm.weight"])
    acc = x[:M].astype(np.float64) @ Wt.astype(np.float64).T
    assert np.abs(x[:M].astype(np.float64)) .max() * np.abs(Wt).sum(1).max() < 2 ** 24
    share = R.check_head(lg, acc.astype(np.float32), ssq, D, eps, M)
    assert not lg[M // 2].any(), "the all-zero row's logits"
    _say("head int %s R%d M%d" % ("x".join(map(str, shape[:3])), max_rows, M), undecided=share, zero_row_bits=int(np.count_nonzero(lg[M // 2])))


# ------------------------------------------------------------------------------------------------------------------ k_rope_table
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_table(hd):
    """(cos, sin) of every position up to 1100 against float64 cos / sin of the float64 angle: |d| <= |angle| * c * 2^-24 +
    2 * 2^-24, c = 12.5 from powf (1 ulp) on a once-rounded exponent (9.22 = ln 10000), the fp32 product and sincosf (1 ulp):
    the derivation stands at ROPE_C in tests/cham_kernel_reference.py."""
    cfg = _cham_cfg(256 if hd == 64 else 512, 4, 4, 1024, layers=1, qk=False)
    pr = Probe(cfg, _int_state(cfg, hd), 32, 1100)
    _assert_plan(pr, 1)
    tab = pr.get("rope").reshape(1100, hd // 2, 2)
    ref, ang = R.rope_table_ref(1100, hd, cfg.rope_theta)
    err = np.abs(tab.astype(np.float64) - ref)
    bound = (np.abs(ang) * R.ROPE_C * 2.0 ** -24 + 2 * 2.0 ** -24)[..., None]
    _say("rope table hd%d" % hd, worst_err=float(err.max()), worst_of_bound=float((err / bound).max()))
    assert np.all(err <= bound), "RoPE table: %.3g of its bound at the worst entry" % float((err / bound).max())


# ------------------------------------------------------------------------------------------------------------------ attention
ATT = {"hd64": (256, 4, 4), "hd128": (512, 4, 4), "hd64_gqa3": (192, 3, 1), "hd64_gqa5": (320, 5, 1), "hd128_gqa3": (384, 3, 1)}
TMAX = 1100


def _att_cfg(key, qk):
    dim, H, Hkv = ATT[key]
    return _cham_cfg(dim, H, Hkv, 1024, layers=1, qk=qk)


def _att_state(cfg, seed, wk_mode):
    """random bf16 weights; every q head of a kv group shares one wq block (the group then shares q, so one cached K row can be
    the winner of all of them).  wk_mode "zero": the new token's K row is zero; a float c: wk = c * wq of the group."""
    sd = _dense_state(cfg, seed)
    H, Hkv, hd, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.dim
    w = sd["layers.0.attention.wqkv.weight"].copy()
    rep = H // Hkv
    for h in range(H):
        w[h * hd:(h + 1) * hd] = w[(h // rep) * rep * hd:((h // rep) * rep + 1) * hd]
    for hk in range(Hkv):
        w[D + hk * hd:D + (hk + 1) * hd] = 0 if wk_mode == "zero" else R.bf(np.float32(wk_mode) * w[hk * rep * hd:(hk * rep + 1) * hd])
    sd["layers.0.attention.wqkv.weight"] = w
    return sd


def _v_pattern(Mr, Hkv, T, hd):
    """distinct bf16 patterns: elements 0 and 1 of a row spell its position, the rest mix in row, head and element (on the device)"""
    m = torch.arange(Mr, device="cuda").view(Mr, 1, 1, 1)
    hk = torch.arange(Hkv, device="cuda").view(1, Hkv, 1, 1)
    t = torch.arange(T, device="cuda").view(1, 1, T, 1)
    d = torch.arange(hd, device="cuda").view(1, 1, 1, hd)
    low = ((t >> (8 * (d & 1))) + 37 * (d >> 1) + 11 * m + 5 * hk) & 0xff
    return (0x3c00 | low | ((d & 3) << 8)).to(torch.int16)


def _v_rows(m, hk, t, hd):
    """the same pattern on the host for given (m, hk, t) arrays -> float32 [.., hd]"""
    m, hk, t = (np.asarray(a)[..., None] for a in (m, hk, t))
    d = np.arange(hd)
    low = ((t >> (8 * (d & 1))) + 37 * (d >> 1) + 11 * m + 5 * hk) & 0xff
    return R.bits_f32((0x3c00 | low | ((d & 3) << 8)).astype(np.uint16))


def _lengths(hd):
    E = 16 if hd == 128 else 32                     # ROWS of k_cham_attn: cached rows per chunk
    return [2, E - 1, E, E + 1, 2 * E - 1, 2 * E + 1, 4 * E - 1, 4 * E + 1, 8 * E + 3, TMAX]


def _q_rows(pr, sd, M, pos, tab):
    """the test's estimate of the rotated q of every (row, head) from the QKV pieces the engine just wrote, and the folded sums"""
    cfg = pr.cfg
    D, Dkv, H, hd = cfg.dim, cfg.n_kv_heads * cfg.head_dim, cfg.n_heads, cfg.head_dim
    pieces = pr.get_pieces("big_slabs", D + 2 * Dkv)
    acc = R.fold_pieces(pieces[:, :M], R.pieces_of(_sks(cfg)["sk_qkv"], (D + 2 * Dkv) // 32))
    ssq = pr.get("ssq").reshape(-1, pr.Mpad)
    rstd = R.rstd64(ssq[:, :M], D, cfg.norm_eps)
    u = R.bf((rstd[:, None] * acc).astype(np.float32))
    q = u[:, :D].reshape(M, H, hd).astype(np.float64)
    cs, sn = tab[pos, :, 0].astype(np.float64)[:, None], tab[pos, :, 1].astype(np.float64)[:, None]
    return R.bf(R.rope_rotate(q, cs, sn)[0].astype(np.float32)), acc, rstd


def _onehot_launches(hd, Hkv, full):
    """(P, t*) for every (row, kv head) of ragged 128-row launches: every cached position of every length, or (GQA engines) the
    chunk edges of every length"""
    jobs = []
    for T in _lengths(hd):
        P = T - 1
        E = 16 if hd == 128 else 32
        ts = range(P) if full else sorted({t for t in (0, 1, E - 1, E, E + 1, 2 * E - 1, 2 * E, 4 * E, 8 * E - 1, 8 * E, P - 2, P - 1) if 0 <= t < P})
        ts = list(ts)
        for i in range(0, len(ts), Hkv):
            grp = ts[i:i + Hkv]
            jobs.append((P, grp + [grp[-1]] * (Hkv - len(grp))))
    return [jobs[i:i + 128] for i in range(0, len(jobs), 128)]


def _run_onehot(pr, sd, key, full, winners=1):
    """runs the sweep; returns per launch (P [M], t* [M, Hkv], t2 [M, Hkv] or None, y [M, D])"""
    cfg = pr.cfg
    D, H, Hkv, hd = cfg.dim, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    rep = H // Hkv
    tab = pr.get("rope").reshape(TMAX, hd // 2, 2)
    vdev = _v_pattern(pr.max_rows, Hkv, TMAX, hd)
    pr.put("vcache", vdev)
    rs = np.random.RandomState(hd + Hkv)
    out = []
    for jobs in _onehot_launches(hd, Hkv, full):
        M = len(jobs)
        P = np.array([j[0] for j in jobs])
        ts = np.array([j[1] for j in jobs])
        t2 = None
        if winners == 2:
            t2 = (ts + 1 + rs.randint(0, 1 << 20, size=ts.shape) % np.maximum(P[:, None] - 1, 1)) % np.maximum(P[:, None], 1)
            t2 = np.where(P[:, None] >= 2, t2, ts)
        tok = rs.randint(0, cfg.vocab_size, size=M)
        pr.run(R.EMBED, R.QKV, M, tok, P)
        q, _, _ = _q_rows(pr, sd, M, P, tab)
        qg = q[:, ::rep]                                                         # one q per kv group
        lam = 200.0 * np.sqrt(hd) / (qg.astype(np.float64) ** 2).sum(-1)
        krow = R.bf((lam[..., None] * qg).astype(np.float32))
        assert ((krow.astype(np.float64) * qg).sum(-1) / np.sqrt(hd) > 190).all()
        kc = torch.zeros(pr.max_rows, Hkv, TMAX, hd, dtype=torch.int16, device="cuda")
        kb = torch.from_numpy(R.bf_bits(krow).view(np.int16).reshape(M, Hkv, hd)).cuda()
        mi, hi = torch.arange(M, device="cuda")[:, None].expand(M, Hkv), torch.arange(Hkv, device="cuda")[None].expand(M, Hkv)
        kc[mi, hi, torch.from_numpy(ts).cuda()] = kb
        if t2 is not None:
            kc[mi, hi, torch.from_numpy(t2).cuda()] = kb
        pr.put("kcache", kc)
        pr.put("vcache", vdev)
        pr.run(R.ATTN, R.ATTN, M)
        out.append((P, ts, t2, pr.get_act("y", D)[:M]))
        del kc
    return out


def _check_onehot(cfg, runs):
    H, Hkv, hd = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    rep = H // Hkv
    bad = n = 0
    for P, ts, t2, y in runs:
        M = len(P)
        m = np.arange(M)[:, None].repeat(Hkv, 1)
        hk = np.arange(Hkv)[None].repeat(M, 0)
        want = _v_rows(m, hk, ts, hd)
        if t2 is not None:
            want = R.bf(((want.astype(np.float64) + _v_rows(m, hk, t2, hd).astype(np.float64)) * 0.5).astype(np.float32))
        want = np.repeat(want, rep, axis=1)                                     # every q head of the group
        bad += R.check_onehot(y.reshape(M, H, hd), want)
        n += M * H
    return bad, n


@pytest.mark.parametrize("key", list(ATT))
def test_attention_one_hot_sweep(key):
    """One cached K row t* = bf(lambda q) scores ~200, every other row and the new token (wk = 0) score 0, exp(-200) is 0 in fp32:
    the output of that (row, head) is V[t*] bit for bit.  t* sweeps every cached position of T = P + 1 in {2, E-1, E, E+1, 2E+-1,
    4E+-1, 8E+3, max_seq_len} (E = cached rows per chunk; GQA engines: the chunk edges of each), a different (P, t*) in every
    (row, kv head) of ragged 128-row launches.  Then two equal winners: bf of the mean of the two V rows, which is exact."""
    cfg = _att_cfg(key, False)
    sd = _att_state(cfg, 11, "zero")
    pr = Probe(cfg, sd, 128, TMAX)
    _assert_plan(pr, 128)
    t0 = time.perf_counter()
    runs = _run_onehot(pr, sd, key, full=cfg.n_kv_heads > 1)
    bad, n = _check_onehot(cfg, runs)
    runs2 = _run_onehot(pr, sd, key, full=False, winners=2)
    bad2, n2 = _check_onehot(cfg, runs2)
    _say("attn one-hot %s" % key, launches=len(runs), cases=n, differing_bits=bad, two_winner_cases=n2, two_winner_bits=bad2,
         seconds=time.perf_counter() - t0)


@pytest.mark.parametrize("key", list(ATT))
def test_attention_new_token_dominates(key):
    """wk = c wq: the new row's score is the large one, so the output is the V row the kernel itself wrote to the cache at P
    (T = 1 included).  The K / V rows written at P follow the float64 replay under the undecided rule (V: bf(rstd * acc), delta
    4 * 2^-24; K: the rotation of both candidates, one fp32 rounding per product and one for the sum, with the table entries the
    kernel reads); no other cache row changes and positions >= P + 1 keep their sentinel."""
    cfg = _att_cfg(key, False)
    D, H, Hkv, hd = cfg.dim, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    Dkv, rep = Hkv * hd, H // Hkv
    sd = _att_state(cfg, 13, 64.0)
    pr = Probe(cfg, sd, 128, TMAX)
    _assert_plan(pr, 128)
    rs = np.random.RandomState(hd)
    Ls = [1] + _lengths(hd)
    P = np.array([Ls[i % len(Ls)] - 1 for i in range(128)])
    M = 128
    tab = pr.get("rope").reshape(TMAX, hd // 2, 2)
    vdev = _v_pattern(128, Hkv, TMAX, hd)
    kdev = torch.zeros_like(vdev)
    kdev[:, :, :, 0] = 0x7fc0                                                    # NaN in element 0 of every K row: sentinel past P, stale at P
    for m in range(M):
        kdev[m, :, :P[m]] = 0
    pr.put("kcache", kdev)
    pr.put("vcache", vdev)
    pr.run(R.EMBED, R.ATTN, M, rs.randint(0, cfg.vocab_size, size=M), P)
    q, acc, rstd = _q_rows(pr, sd, M, P, tab)
    k_after, v_after = pr.get_dev("kcache").view(128, Hkv, TMAX, hd), pr.get_dev("vcache").view(128, Hkv, TMAX, hd)
    mi = torch.arange(M, device="cuda")
    Pd = torch.from_numpy(P).cuda()
    k_new = R.bits_f32(k_after[mi, :, Pd].cpu().numpy().view(np.uint16))         # [M, Hkv, hd]
    v_new = R.bits_f32(v_after[mi, :, Pd].cpu().numpy().view(np.uint16))
    keep = torch.ones(128, Hkv, TMAX, dtype=torch.bool, device="cuda")
    keep[mi, :, Pd] = False
    changed = int(((k_after != kdev).any(-1) & keep).sum()) + int(((v_after != vdev).any(-1) & keep).sum())
    assert changed == 0, "%d cache rows other than the appended ones changed" % changed
    # the appended rows against the float64 replay
    rr = np.repeat(rstd, Hkv)
    lo, hi, und = R.norm_candidates(acc[:, D + Dkv:].reshape(M * Hkv, hd), rr)
    v_share = R.check_candidates(v_new.reshape(M * Hkv, hd), [lo, hi], und, "appended V row")
    cs, sn = np.repeat(tab[P, :, 0], Hkv, axis=0), np.repeat(tab[P, :, 1], Hkv, axis=0)
    cands, und = R.rope_k_candidates(acc[:, D:D + Dkv].reshape(M * Hkv, hd), rr, cs, sn)
    k_share = R.check_candidates(k_new.reshape(M * Hkv, hd), cands, und, "appended K row")
    score = (k_new.astype(np.float64)[:, :, None] * q.reshape(M, Hkv, rep, hd)).sum(-1) / np.sqrt(hd)
    assert score.min() > 100, "the new token must dominate (score %.1f)" % score.min()
    y = pr.get_act("y", D)[:M].reshape(M, Hkv, rep, hd)
    bad = R.check_onehot(y, np.broadcast_to(v_new[:, :, None], y.shape))
    _say("attn new token %s" % key, differing_bits=bad, k_undecided=k_share, v_undecided=v_share, other_rows_changed=changed, min_score=float(score.min()))


def _dense_inputs(key, qk, M, seed):
    """deterministic on the host (the variant child rebuilds the same): positions, tokens, caches [M, Hkv, 1024, hd] as bf16 values"""
    cfg = _att_cfg(key, qk)
    Hkv, hd = cfg.n_kv_heads, cfg.head_dim
    rs = np.random.RandomState(seed)
    E = 16 if hd == 128 else 32
    pos = rs.randint(32, 1024, size=M)
    pos[:6] = [1023, 8 * E, 8 * E - 1, 4 * E + 1, 300, 32]
    tok = rs.randint(0, cfg.vocab_size, size=M)
    g = torch.Generator().manual_seed(seed)
    kc = torch.randn(M, Hkv, 1024, hd, generator=g).to(torch.bfloat16)
    vc = torch.randn(M, Hkv, 1024, hd, generator=g).to(torch.bfloat16)
    return cfg, pos, tok, kc, vc


def _run_dense(pr, pos, tok, kc, vc):
    M = len(pos)
    Hkv, hd = pr.cfg.n_kv_heads, pr.cfg.head_dim
    for name, c in (("kcache", kc), ("vcache", vc)):
        full = torch.zeros(pr.max_rows, Hkv, pr.T, hd, dtype=torch.int16, device="cuda")
        full[:M, :, :1024] = c.view(torch.int16).cuda()
        pr.put(name, full)
    pr.run(R.EMBED, R.ATTN, M, tok, pos)
    return pr.get_act("y", pr.cfg.dim)[:M], pr.get_act("x", pr.cfg.dim)[:M]


def _bf64(v):
    return R.bf_candidates(v, -1.0)[0].astype(np.float64)


def _check_dense(cfg, sd, pos, kc, vc, x, y):
    """ref64: the QKV + ATTN stage in float64 with the stage's bf16 rounding points; the yardstick: oracle/cham_oracle.py's fp32
    evaluation of the same stage on the same data"""
    M = len(pos)
    D, H, Hkv, hd = cfg.dim, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    Dkv, rep = Hkv * hd, H // Hkv
    Wt = R.tile_weight(sd["layers.0.attention.wqkv.weight"], sd["layers.0.attention_norm.weight"]).astype(np.float64)
    x64 = x.astype(np.float64)
    rstd = 1.0 / np.sqrt((x64 ** 2).mean(1) + np.float64(np.float32(cfg.norm_eps)))
    u = _bf64(rstd[:, None] * (x64 @ Wt.T))
    q, k, v = u[:, :D].reshape(M, H, hd), u[:, D:D + Dkv].reshape(M, Hkv, hd), u[:, D + Dkv:].reshape(M, Hkv, hd)
    if cfg.qk_normalization:
        def ln(a, w, b):
            mu = a.mean(-1, keepdims=True)
            return _bf64((a - mu) / np.sqrt(((a - mu) ** 2).mean(-1, keepdims=True) + np.float64(np.float32(1e-5))) * w.astype(np.float64) + b.astype(np.float64))
        p = "layers.0.attention."
        q = ln(q, sd[p + "q_normalization.weight"], sd[p + "q_normalization.bias"])
        k = ln(k, sd[p + "k_normalization.weight"], sd[p + "k_normalization.bias"])
    tab, _ = R.rope_table_ref(1024, hd, cfg.rope_theta)
    cs, sn = tab[pos, :, 0][:, None], tab[pos, :, 1][:, None]
    q, k = _bf64(R.rope_rotate(q, cs, sn)[0]), _bf64(R.rope_rotate(k, cs, sn)[0])
    kc64, vc64 = kc.float().numpy().astype(np.float64), vc.float().numpy().astype(np.float64)
    ref = np.empty((M, H, hd))
    for m in range(M):
        for h in range(H):
            hk = h // rep
            ref[m, h] = R.attn_ref(q[m, h], np.concatenate([kc64[m, hk, :pos[m]], k[m, hk][None]]),
                                   np.concatenate([vc64[m, hk, :pos[m]], v[m, hk][None]]), hd ** -0.5)
    cache = CO.Cache(1, M)
    for m in range(M):
        cache.k[0][m] = kc[m, :, :pos[m]].float().transpose(0, 1).contiguous()
        cache.v[0][m] = vc[m, :, :pos[m]].float().transpose(0, 1).contiguous()
    tsd = {k_: torch.from_numpy(v_) for k_, v_ in sd.items()}
    fp32 = CO.attention_stage(tsd, cfg, 0, torch.from_numpy(x), torch.from_numpy(pos), cache, fold=True).numpy().reshape(M, H, hd)
    return R.check_attn_dense(y.reshape(M, H, hd), ref, fp32)


@pytest.mark.parametrize("qk", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("key", list(ATT))
def test_attention_dense(key, qk):
    """Random caches, positions up to 1023 (the chunk and loop edges among them): per (row, head), max |got - ref64| / max |ref64|
    <= TORCH_FACTOR (4) x the same figure of oracle/cham_oracle.py's fp32 evaluation of the stage, measured in the same run."""
    M = 64
    cfg, pos, tok, kc, vc = _dense_inputs(key, qk, M, 21)
    sd = _dense_state(cfg, 17)
    pr = Probe(cfg, sd, 64, 1024)
    _assert_plan(pr, M)
    y, x = _run_dense(pr, pos, tok, kc, vc)
    e, eo, worst = _check_dense(cfg, sd, pos, kc, vc, x, y)
    _say("attn dense %s qk=%d" % (key, qk), err=e, oracle_fp32=eo, worst_ratio=worst)


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from tests import test_gpu_cham_kernels as T
T.variant_child(sys.argv[1], int(sys.argv[2]))
print("CHILD OK")
"""


def variant_child(path, nwa):
    """in a process started with WMAR_CHAM_NWA set: the one-hot sweep and the dense cases of head_dim 128, outputs to `path`"""
    key = "hd128"
    cfg = _att_cfg(key, False)
    sd = _att_state(cfg, 11, "zero")
    pr = Probe(cfg, sd, 128, TMAX)
    _assert_plan(pr, 128, nwa)
    out = {}
    for i, (P, ts, _, y) in enumerate(_run_onehot(pr, sd, key, full=True)):
        out["oh_P%d" % i], out["oh_t%d" % i], out["oh_y%d" % i] = P, ts, y
    del pr
    for qk in (0, 1):
        cfg, pos, tok, kc, vc = _dense_inputs(key, bool(qk), 64, 21)
        pr = Probe(cfg, _dense_state(cfg, 17), 64, 1024)
        _assert_plan(pr, 64, nwa)
        out["dense_y%d" % qk], out["dense_x%d" % qk] = _run_dense(pr, pos, tok, kc, vc)
        del pr
    np.savez(path, **out)


@pytest.mark.parametrize("nwa", [1, 4])
def test_attention_wave_count_variants(nwa, tmp_path):
    """WMAR_CHAM_NWA = 1 / 4 (read once per process: one fresh child each) select k_cham_attn<128,1> / <128,4>: the one-hot sweep
    and the dense cases; the child asserts the plan and saves its outputs, the comparing is done here."""
    path = tmp_path / "variant.npz"
    res = subprocess.run([sys.executable, "-c", _CHILD % REPO, str(path), str(nwa)], env=dict(os.environ, WMAR_CHAM_NWA=str(nwa)),
                         capture_output=True, text=True, timeout=300, cwd=REPO)
    assert res.returncode == 0 and "CHILD OK" in res.stdout, (res.stdout[-1500:], res.stderr[-2500:])
    z = np.load(path)
    cfg = _att_cfg("hd128", False)
    n_l = len([k for k in z.files if k.startswith("oh_P")])
    assert n_l == len(_onehot_launches(128, 4, True))
    bad, n = _check_onehot(cfg, [(z["oh_P%d" % i], z["oh_t%d" % i], None, z["oh_y%d" % i]) for i in range(n_l)])
    figs = {"cases": n, "differing_bits": bad}
    for qk in (0, 1):
        cfg, pos, tok, kc, vc = _dense_inputs("hd128", bool(qk), 64, 21)
        e, eo, worst = _check_dense(cfg, _dense_state(cfg, 17), pos, kc, vc, z["dense_x%d" % qk], z["dense_y%d" % qk])
        figs["dense_qk%d" % qk], figs["oracle_qk%d" % qk], figs["ratio_qk%d" % qk] = e, eo, worst
    _say("attn variant <128,%d>" % nwa, **figs)


# ------------------------------------------------------------------------------------------------------------------ engine level
def test_small_batch_after_large_batch_is_bit_identical():
    """k_bgemm never stores padding rows: a slab slot keeps "the finite sums an earlier, larger batch left there".  Two steps at
    M = 126, then the same tokens at M = 5: logits and cache rows of the 5 rows are bit-equal to a fresh engine's that only
    ever saw M = 5."""
    shape = (1024, 8, 8, 1024, 64)
    cfg = _cham_cfg(*shape, layers=1, qk=True)
    assert "workgroup boundary inside a group" in decomposition(cfg)
    sd = _dense_state(cfg, 23)
    rs = np.random.RandomState(23)
    tok = rs.randint(0, cfg.vocab_size, size=(2, 126))
    used, fresh = Probe(cfg, sd, 128, 16), Probe(cfg, sd, 128, 16)
    _assert_plan(used, 126)
    _assert_plan(fresh, 5)
    for t in range(2):
        used.forward(tok[t], np.full(126, t))
    bad = 0
    for t in range(2):
        a, b = used.forward(tok[t, :5], np.full(5, t)), fresh.forward(tok[t, :5], np.full(5, t))
        bad += R.diff_bits(a, b)
    Hkv, hd = cfg.n_kv_heads, cfg.head_dim
    for name in ("kcache", "vcache"):
        a, b = (p.get(name).reshape(128, Hkv, 16, hd)[:5, :, :2] for p in (used, fresh))
        bad += int(np.count_nonzero(a != b))
    _say("small after large batch", differing_bits=bad)
    assert bad == 0
