"""The launches of a Taming minGPT decode step one at a time, through a live engine's own StepPlan and buffers (wmar_gpt_probe_run /
wmar_gpt_probe_copy / wmar_gpt_probe_plan), against the numpy statement of that one operation in tests/gpt_kernel_reference.py.
Every case asserts the kernel names and integers the probe plan reports and prints its figures on lines starting GPTK (run with -s).

Engines (synthetic weights, n_layer 2 unless noted; "int": integer weights in -4..4, one-hot FC1 / head weights, LayerNorm weights
powers of two, integer embeddings and proj / FC2 biases -- every partial sum is an integer below 2^24; "dense": full-significand):
  A   n_embd 1536, 24 heads, max_batch 128: k_qkvx<1,.> (13 / 31 / 32 rows), k_qkvx_bx + k_bx_xr + k_fc1x + FC2 with fc2_hi + the
      two-tile head (33 / 63 / 64), k_resid_stats + k_gemm QKV + the four-row-tile FC1 (65 / 127 / 128); the small-batch plan at 1..12
      rows; with WMAR_NO_XR=1: k_bx<1,6> at 4 slices + k_resid_stats
  B   768 wide, 6 heads of 128: k_bx at 2 slices, k_fc1x, attention at head_dim 128
  C   256 wide, 8 heads of 32, vocabulary 16384: k_gemm projection, k_gemm<EPI_GELU> at one and two row tiles, the head as 2 and 4
      launches; with WMAR_NO_BX=1: k_qkvx<2,.>
  D   160 wide, 5 heads: RESID_IN + k_gemm QKV at one and two row tiles, k-splits of 5 k-blocks per wave (tail path only)
  E   2176 wide, 17 heads of 128, one block: 17 statistics chunks (the second round of ln_row_stats) in FC1, HEAD and ATTN

Measured on an MI355X (159 cases, 19 s): 0 differing bits in every exact case; dense pieces 0.22 .. 1.11 x the chain; one-hot FC1 /
head 0.32 .. 0.64 of the derived distance (small-batch plan 0.58 .. 0.81); dense head 0.30 .. 0.45 x the fp32 algebra, FC1 0.64 .. 1.82 x
torch; DESIGN.md section 4 has the table and the off-centre figures.

Rules this file applies, and why:
  * the outputs of the LayerNorm-fused launches are fp32, where 4 x 2^-24 |v| spans several values at every v: there is no pair of
    candidates to choose from, so every element is held to that distance (plus the rounding of the final addition) and none is exempt;
  * dense attention: every output within a worst-case distance derived from the launch's own steps (correct kernels use 0.3 .. 2.4 %
    of it: it catches a missing chunk, nothing subtle), the largest error of a launch within 4 x the largest of an fp32 numpy
    evaluation (the gate that bites), and the K / V rows the prologue appends within 2 x an fp32 evaluation of the prologue's algebra
    on rows with |mean| of the order of sigma.  4 x per single (row, head) is not asserted: a correct k_attn_decode measures 9 .. 13 x
    at its worst pair (test_dense_attention_meets_the_fp32_bound says why);
  * the number of QKV pieces S is the plan's (7, 8, 1 on these engines): the probe runs the engine's own plan, so S cannot be set per
    case; at 31 rows of engine B the 186 (row, head) pairs do not reach every cached position of the two longest lengths;
  * composition runs the step stage by stage on the engine that ran wmar_gpt_decode_step, after every work buffer and the cache rows
    the walk has to append were overwritten with a sentinel (the step is a function of the tokens, the position and the cache rows
    below it);
  * a case is skipped only where the DEVICE cannot run k_bx_xr (xcd_ok = 0 in the probe plan, measured at engine creation); a plan that
    leaves the fused launch on an eligible device, or a barrier that fell back, fails;
  * the head never runs on four row tiles per workgroup: its launches hold at most 128 column tiles at > 64 rows, and the dispatch
    takes that path only above 256 workgroups of two row tiles (head_tiles in the plan pins it; fc1_tiles = 4 pins the FC1 of A).

The RAR-only variants of these kernels (k_attn_decode80, attention mode 1, k_modulate, k_resid_mod, k_bx with GELU / XF / four row
tiles) are held stage by stage in tests/test_gpu_rar_kernels.py, through wmar_rar_probe_*."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpt_kernel_reference as R  # noqa: E402
from tests.engine_probe import EngineCache, EngineProbe, dev, parse_plan, say  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402

SENT = float(R.SENTINEL)
GARBAGE = 3.0e30


_say = say("GPTK", 40)


# ------------------------------------------------------------------------------------------------------------------- engines
SHAPES = {  # name: (n_embd, n_head, vocab, block, n_layer, max_batch)
    "A": (1536, 24, 512, 256, 2, 128), "A12": (1536, 24, 512, 256, 2, 12), "B": (768, 6, 512, 256, 2, 64), "C": (256, 8, 16384, 256, 2, 128),
    "D": (160, 5, 512, 32, 2, 64), "E": (2176, 17, 512, 16, 1, 128),
}


def _cfg(name):
    D, H, V, T, L, _ = SHAPES[name]
    return synth.GPTConfig(vocab_size=V, block_size=T, n_layer=L, n_head=H, n_embd=D)


def _int_state(cfg, seed):
    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in synth.gpt_shapes(cfg).items():
        leaf = k.rsplit(".", 1)[-1]
        if any(t in k for t in ("ln1.", "ln2.", "ln_f.")):
            sd[k] = (2.0 ** rs.randint(-1, 2, size=shp) if leaf == "weight" else 0.05 * rs.randn(*shp)).astype(np.float32)
        elif k in ("tok_emb.weight", "pos_emb"):
            sd[k] = rs.randint(-4, 5, size=shp).astype(np.float32)
        elif k.endswith("mlp.0.weight") or k == "head.weight":                     # one-hot, every k hit
            N, K = shp
            w = np.zeros(shp, dtype=np.float32)
            kn = np.concatenate([rs.permutation(K) for _ in range(-(-N // K))])[:N]
            w[np.arange(N), kn] = rs.randint(1, 5, size=N) * rs.choice([-1.0, 1.0], size=N)
            sd[k] = w
        elif leaf == "weight":
            sd[k] = rs.randint(-4, 5, size=shp).astype(np.float32)
        elif k.endswith("proj.bias") or k.endswith("mlp.2.bias"):
            sd[k] = rs.randint(-2, 3, size=shp).astype(np.float32)
        else:
            sd[k] = (0.5 * rs.randn(*shp)).astype(np.float32)
    return sd


def _dense_state(cfg, seed):
    return {k: v.float().numpy() for k, v in synth.synth_gpt_state(cfg, seed=seed, logit_scale=4.0).items()}


class Probe(EngineProbe):
    """One wmar_gpt engine and stage access to it."""
    ENGINE = "gpt"
    DTYPES = {"stats": torch.float64, "stats_q": torch.float64, "yq": torch.int16}

    def __init__(self, name, kind, env=()):
        self.name, self.kind = name, kind
        self.D, self.H, self.V, self.T, self.nl, self.Bmax = SHAPES[name]
        self.hd = self.D // self.H
        self.cfg = _cfg(name)
        self.sd = _int_state(self.cfg, 11 + self.D) if kind == "int" else _dense_state(self.cfg, 11 + self.D)
        from wmar_amd import _lib
        self._create(_lib.GptConfig(self.V, self.T, self.nl, self.H, self.D, self.Bmax), self.sd, env)

    # ---- stages
    def run(self, first, last, B, pos=0, layer=0, tok=None, want_logits=False):
        return self._call(self._run, B, self.V, dev(tok), B, pos, layer, first, last, want_logits=want_logits)

    def decode_step(self, tok, pos):
        return self._call(self.L.wmar_gpt_decode_step, len(tok), self.V, dev(tok), len(tok), pos)

    def plan(self, B, kv_len=1):
        out = parse_plan(self.plan_text(B, kv_len))
        for k in ("small", "MT", "S_qx", "nkeep", "S_qkv", "S_proj", "S_fc2", "fc2_hi", "nch", "nch_ln2", "pingpong", "attn_waves", "rowmajor", "fc1_tiles", "head_tiles",
                  "xcd_ok", "xr_eligible", "barrier_fallbacks"):
            assert isinstance(out[k], int), (k, out[k])
        return out

    def waves(self, nwa):
        big = 1 << 30
        t1, t2 = {0: (-1, -1), 1: (big, big), 2: (0, big), 4: (0, 0)}[nwa]
        self._lib.check(self.L.wmar_gpt_set_attention_phases(self.h, t1, t2))

    # ---- packed buffers as [Mpad, width] arrays of the step's MT
    def put_act(self, name, X, MT):
        """X [32 MT, K] into the front of a packed buffer sized for max_batch"""
        self.put_front(name, R.pack_act(X.astype(np.float32), MT))

    def get_act(self, name, MT, K):
        return R.unpack_act(self.get(name)[:32 * MT * K], MT, K)

    def put_x(self, X, MT):
        self.put_act("x", X, MT)
        self.put_act("x2", X, MT)

    def cur(self, plan, stage, layer):
        """the residual stream buffer a stage reads (include/wmar_hip.h)"""
        if not plan["pingpong"] or stage == R.EMBED:
            return "x"
        if stage >= R.RESID_OUT:
            layer = self.nl - 1
        return "x2" if (layer + (1 if stage > R.QKV else 0)) & 1 else "x"

    def put_stats(self, name, st, MT):
        """st [nch][32 MT][2] into the front of the statistics buffer"""
        self.put_front(name, st.reshape(-1).astype(np.float64), rest=1e300)       # chunks past the plan's count must not be read

    def get_stats(self, name, nch, MT):
        return self.get(name)[:nch * 32 * MT * 2].reshape(nch, 32 * MT, 2)

    def w(self, key, layer=None):
        return self.sd[key if layer is None else "blocks.%d.%s" % (layer, key)]


_ENGINES = EngineCache()


def _probe(name, kind, env=()):
    """the module's engines, created on first use (one per shape, weights and environment) and destroyed when the module ends"""
    return _ENGINES.get((name, kind, env), lambda: Probe(name, kind, env))


@pytest.fixture(scope="module", autouse=True)
def engines():
    yield _ENGINES
    _ENGINES.close_all()
    torch.cuda.empty_cache()


ENGINES = [("A", ()), ("A", ("WMAR_NO_XR",)), ("B", ()), ("C", ()), ("C", ("WMAR_NO_BX",)), ("D", ()), ("E", ())]
_EID = dict(ids=str)

# (engine, env, B) -> what the plan must report: integers and kernel names
PLANS = {
    ("A", (), 31): dict(MT=1, S_qx=7, S_proj=5, S_fc2=5, fc2_hi=0, nch=12, nch_ln2=12, proj="gemm", head="1,256", qkv="k_qkvx<1,5>", fc1="k_gemm<EPI_GELU"),
    ("A", (), 63): dict(MT=2, S_qx=7, nkeep=4, S_proj=4, S_fc2=5, fc2_hi=16, nch=12, nch_ln2=16, proj="bx_xr", head="ntw2", qkv="k_qkvx_bx<6>", fc1="k_fc1x", rowmajor=1),
    ("A", (), 127): dict(MT=4, S_qx=0, S_qkv=1, S_proj=5, S_fc2=4, fc2_hi=0, nch=12, nch_ln2=12, proj="gemm", head="1,128", qkv="k_gemm<EPI_PACKED>", fc1="k_gemm<EPI_GELU"),
    ("A", (), 13): dict(MT=1, S_qx=7, S_proj=5, S_fc2=5, fc2_hi=0, nch=12, nch_ln2=12, proj="gemm", head="1,256", qkv="k_qkvx<1,5>", fc1="k_gemm<EPI_GELU"),
    ("A", (), 32): dict(MT=1, S_qx=7, S_proj=5, S_fc2=5, fc2_hi=0, nch=12, nch_ln2=12, proj="gemm", head="1,256", qkv="k_qkvx<1,5>", fc1="k_gemm<EPI_GELU"),
    ("A", (), 33): dict(MT=2, S_qx=7, nkeep=4, S_proj=4, S_fc2=5, fc2_hi=16, nch=12, nch_ln2=16, proj="bx_xr", head="ntw2", qkv="k_qkvx_bx<6>", fc1="k_fc1x", rowmajor=1),
    ("A", (), 64): dict(MT=2, S_qx=7, nkeep=4, S_proj=4, S_fc2=5, fc2_hi=16, nch=12, nch_ln2=16, proj="bx_xr", head="ntw2", qkv="k_qkvx_bx<6>", fc1="k_fc1x", rowmajor=1),
    ("A", (), 65): dict(MT=4, S_qx=0, S_qkv=1, S_proj=5, S_fc2=4, fc2_hi=0, nch=12, nch_ln2=12, proj="gemm", head="1,128", qkv="k_gemm<EPI_PACKED>", fc1="k_gemm<EPI_GELU"),
    ("A", (), 128): dict(MT=4, S_qx=0, S_qkv=1, S_proj=5, S_fc2=4, fc2_hi=0, nch=12, nch_ln2=12, proj="gemm", head="1,128", qkv="k_gemm<EPI_PACKED>", fc1="k_gemm<EPI_GELU"),
    ("A", ("WMAR_NO_XR",), 63): dict(MT=2, S_qx=7, nkeep=4, S_proj=4, S_fc2=5, fc2_hi=16, nch=12, nch_ln2=12, proj="bx", head="ntw2", qkv="k_qkvx_bx<6>", fc1="k_fc1x", projk="k_bx<1,6>"),
    ("B", (), 31): dict(MT=1, S_qx=8, S_proj=3, S_fc2=8, fc2_hi=0, nch=6, nch_ln2=6, proj="gemm", head="1,256", qkv="k_qkvx<1,8>", fc1="k_gemm<EPI_GELU"),
    ("B", (), 64): dict(MT=2, S_qx=8, nkeep=4, S_proj=2, S_fc2=4, fc2_hi=0, nch=6, nch_ln2=6, proj="bx", head="ntw2", qkv="k_qkvx_bx<4>", fc1="k_fc1x", projk="k_bx<1,6>", rowmajor=1),
    ("C", (), 5): dict(MT=1, S_qx=8, S_proj=1, S_fc2=4, fc2_hi=0, nch=2, nch_ln2=2, proj="gemm", head="2,256", qkv="k_qkvx<1,4>", fc1="k_gemm<EPI_GELU"),
    ("C", (), 32): dict(MT=1, S_qx=8, S_proj=1, S_fc2=4, fc2_hi=0, nch=2, nch_ln2=2, proj="gemm", head="2,256", qkv="k_qkvx<1,4>", fc1="k_gemm<EPI_GELU"),
    ("C", (), 33): dict(MT=2, S_qx=8, nkeep=4, S_proj=1, S_fc2=4, fc2_hi=0, nch=2, nch_ln2=2, proj="gemm", head="ntw2", qkv="k_qkvx_bx<4>", fc1="k_gemm<EPI_GELU", rowmajor=1),
    ("C", (), 127): dict(MT=4, S_qx=0, S_qkv=1, S_proj=1, S_fc2=4, fc2_hi=0, nch=2, nch_ln2=2, proj="gemm", head="4,128", qkv="k_gemm<EPI_PACKED>", fc1="k_gemm<EPI_GELU"),
    ("C", ("WMAR_NO_BX",), 63): dict(MT=2, S_qx=8, S_proj=1, S_fc2=4, fc2_hi=0, nch=2, nch_ln2=2, proj="gemm", head="ntw2", qkv="k_qkvx<2,4>", fc1="k_gemm<EPI_GELU", rowmajor=0),
    ("D", (), 13): dict(MT=1, S_qx=0, S_qkv=1, S_proj=1, S_fc2=2, fc2_hi=0, nch=2, nch_ln2=2, proj="gemm", head="1,256", qkv="k_gemm<EPI_PACKED>", fc1="k_gemm<EPI_GELU"),
    ("D", (), 33): dict(MT=2, S_qx=0, S_qkv=1, S_proj=1, S_fc2=2, fc2_hi=0, nch=2, nch_ln2=2, proj="gemm", head="ntw2", qkv="k_gemm<EPI_PACKED>", fc1="k_gemm<EPI_GELU"),
    ("E", (), 13): dict(MT=1, nch=17, nch_ln2=17, head="1,256", fc1="k_gemm<EPI_GELU"),
    ("E", (), 65): dict(MT=4, S_qx=0, S_qkv=1, nch=17, nch_ln2=17, qkv="k_gemm<EPI_PACKED>"),
}
_MFMA_STAGES = {True: ["EMBED", "QKV", "ATTN", "PROJ", "RESID_ATTN", "FC1", "FC2", "RESID_OUT", "HEAD"],
                False: ["EMBED", "RESID_IN", "QKV", "ATTN", "PROJ", "RESID_ATTN", "FC1", "FC2", "RESID_OUT", "HEAD"]}


def _plan(pr, env, B, kv_len=1):
    """the plan for B rows, held to PLANS (a dispatch change cannot silently move a case to another kernel)"""
    plan = pr.plan(B, kv_len)
    want = PLANS[(pr.name if pr.name != "A12" else "A", env, B)]
    if want.get("proj") == "bx_xr" and not plan["xcd_ok"]:     # a property of the device, measured at engine creation -- not the dispatch
        pytest.skip("this device does not place blocks with equal blockIdx % 8 on one XCD or does not hold the grid: k_bx_xr cannot run")
    assert plan["barrier_fallbacks"] == 0, "an in-launch barrier gave up: the engine left the fused projection launch"
    assert plan["small"] == 0
    # row tiles per workgroup of the k_gemm that runs FC1 (0: k_fc1x) -- the four-row-tile FC1 is A at > 64 rows
    if "fc1" in want:
        tiles = 0 if want["fc1"] == "k_fc1x" else {1: 1, 2: 2, 4: {"A": 4, "C": 2, "E": 4}.get(pr.name, 2)}[want["MT"]]
        assert plan["fc1_tiles"] == tiles, (plan["fc1_tiles"], tiles)
    if "head" in want:
        assert plan["head_tiles"] == {1: 1, 2: 2, 4: 2}[want["MT"]], plan["head_tiles"]
    for k, v in want.items():
        if k in ("qkv", "fc1"):
            assert v in plan["roles"][k], (k, plan["roles"][k])
        elif k == "projk":
            assert v in plan["roles"]["proj"], plan["roles"]["proj"]
        else:
            assert plan[k] == v, (k, plan[k], v)
    stages = list(_MFMA_STAGES[plan["S_qx"] > 0])
    if plan["proj"] == "bx_xr":
        stages.remove("RESID_ATTN")
    if pr.nl == 1 and "RESID_IN" in stages:
        stages.remove("RESID_IN")
    assert plan["stages"] == stages, plan["stages"]
    assert "k_attn_decode<%d," % pr.hd in plan["roles"]["attn"]
    return plan


def _rows(Mpad, M, K, rs, kind="int"):
    """[Mpad, K] input rows: integers in -8..8 (or full-significand values) in the live rows, large finite garbage in the padding rows"""
    X = rs.randint(-8, 9, size=(Mpad, K)).astype(np.float32) if kind == "int" else rs.randn(Mpad, K).astype(np.float32)
    X[M:] = GARBAGE * rs.choice([-1.0, 1.0], size=(Mpad - M, K))
    return X


def _zero_sum_rows(Mpad, M, K, rs):
    """integer rows whose sum is exactly 0 (mean = 0: the fused LayerNorm algebra has no cancelling term); padding rows: finite garbage"""
    X = rs.randint(-8, 9, size=(Mpad, K)).astype(np.float32)
    X[:, -1] -= X.sum(1)
    X[:, -2] -= X.sum(1)
    assert np.all(X.sum(1) == 0)
    X[M:] = 1.0e15 * rs.choice([-1.0, 1.0], size=(Mpad - M, K))            # (finite sums of squares for the planted statistics)
    return X


# ------------------------------------------------------------------------------------------------------------------- plans, packs
@pytest.mark.parametrize("case", sorted(PLANS, key=str), ids=lambda c: "%s%s-%d" % (c[0], "+" + "+".join(c[1]) if c[1] else "", c[2]))
def test_plan_reports_the_kernels_and_integers(case):
    name, env, B = case
    pr = _probe(name, "dense", env)
    plan = _plan(pr, env, B)
    # a stage the plan does not have is rejected, and so is the EMBED stage without tokens
    absent = [s for s in range(10) if R.STAGES[s] not in plan["stages"]]
    for s in absent:
        assert pr.L.wmar_gpt_probe_run(pr.h, None, B, 0, pr.nl - 1, s, s, None, pr._lib.stream_ptr()) != 0
    assert pr.L.wmar_gpt_probe_run(pr.h, None, B, 0, 0, R.EMBED, R.EMBED, None, pr._lib.stream_ptr()) != 0
    _say("plan %s%s B=%d" % (name, "".join(env), B), **{k: plan[k] for k in ("MT", "S_qx", "S_proj", "S_fc2", "fc2_hi", "nch_ln2", "proj", "head")})


def test_small_plan_is_reported_at_1_to_12_rows():
    pr = _probe("A", "dense")
    for B in range(1, 13):
        plan = pr.plan(B)
        assert plan["small"] == 1 and plan["stages"] == ["EMBED", "QKV", "ATTN", "PROJ", "FC1", "FC2", "HEAD"] and plan["head"] == "small"
        assert "k_sgemv<QKV>" in plan["roles"]["qkv"] and "k_sattn" in plan["roles"]["attn"]
        for s in (R.RESID_IN, R.RESID_ATTN, R.RESID_OUT):
            assert pr.L.wmar_gpt_probe_run(pr.h, None, B, 0, 1, s, s, None, pr._lib.stream_ptr()) != 0


@pytest.mark.parametrize("eng", ENGINES, **_EID)
def test_weight_packs_and_folded_vectors_are_bit_exact(eng):
    name, env = eng
    pr = _probe(name, "dense", env)
    D, n, shares = pr.D, 0, []
    for l in range(pr.nl):
        g1, b1, g2, b2 = (pr.w(k, l) for k in ("ln1.weight", "ln1.bias", "ln2.weight", "ln2.bias"))
        Wqkv = np.concatenate([pr.w("attn.%s.weight" % k, l) for k in ("query", "key", "value")])
        bq = np.concatenate([pr.w("attn.%s.bias" % k, l) for k in ("query", "key", "value")])
        Wp, W1, W2 = pr.w("attn.proj.weight", l), pr.w("mlp.0.weight", l), pr.w("mlp.2.weight", l)
        n += R.check_pack(pr.get("wqkv", l), R.pack_linear(R.fold_gamma(Wqkv, g1)), "wqkv") + 1
        n += R.check_pack(pr.get("wproj", l), R.pack_linear(Wp), "wproj") + 1
        n += R.check_pack(pr.get("wfc1", l), R.pack_linear(R.fold_gamma(W1, g2)), "wfc1") + 1
        n += R.check_pack(pr.get("wfc2", l), R.pack_linear(W2), "wfc2") + 1
        if pr.has("wqkvx_bx"):
            n += R.check_pack(pr.get("wqkvx_bx", l), R.pack_bx(R.fold_gamma(Wqkv, g1)), "wqkvx_bx") + 1
        if pr.has("wproj_bx"):
            n += R.check_pack(pr.get("wproj_bx", l), R.pack_bx(Wp), "wproj_bx") + 1
        if pr.has("wfc1x16"):
            w16, w8 = R.pack_fc1x(R.fold_gamma(W1, g2))
            n += R.check_pack(pr.get("wfc1x16", l), w16, "wfc1x16") + R.check_pack(pr.get("wfc1x8", l), w8, "wfc1x8") + 2
        for got, W, v, b, what in (("bqkv", Wqkv, b1, bq, "bqkv"), ("cqkv", Wqkv, g1, None, "cqkv"), ("bfc1", W1, b2, pr.w("mlp.0.bias", l), "bfc1"),
                                   ("cfc1", W1, g2, None, "cfc1")):
            shares.append(R.check_fold_vec(pr.get(got, l), *R.fold_vec(W, v, b), what))
        R.check_exact(pr.get("bproj", l), pr.w("attn.proj.bias", l), "bproj")
        R.check_exact(pr.get("bfc2", l), pr.w("mlp.2.bias", l), "bfc2")
    Wh = pr.w("head.weight")
    n += R.check_pack(pr.get("whead"), R.pack_linear(R.fold_gamma(Wh, pr.w("ln_f.weight"))), "whead") + 1
    shares.append(R.check_fold_vec(pr.get("bhead"), *R.fold_vec(Wh, pr.w("ln_f.bias")), "bhead"))
    shares.append(R.check_fold_vec(pr.get("chead"), *R.fold_vec(Wh, pr.w("ln_f.weight")), "chead"))
    assert (name in ("A", "B")) == pr.has("wproj_bx") and (name in ("A", "B")) == pr.has("wfc1x16") and (name != "D") == pr.has("wqkvx_bx")
    _say("packs %s%s" % (name, "".join(env)), packs=n, differing_bits=0, fold_vectors=len(shares), near_midpoint_share=float(max(shares)))


# ------------------------------------------------------------------------------------------------------------------- composition
def _stage_walk(pr, plan, tok, pos):
    B = len(tok)
    ids = [R.STAGES.index(s) for s in plan["stages"]]
    per_layer = [s for s in ids if R.EMBED < s < R.RESID_OUT and s != R.RESID_IN]
    pr.run(R.EMBED, R.EMBED, B, pos, 0, tok=tok)
    for l in range(pr.nl):
        for s in ([R.RESID_IN] if (R.RESID_IN in ids and l > 0) else []) + per_layer:
            pr.run(s, s, B, pos, l)
    if R.RESID_OUT in ids:
        pr.run(R.RESID_OUT, R.RESID_OUT, B, pos, pr.nl - 1)
    return pr.run(R.HEAD, R.HEAD, B, pos, pr.nl - 1, want_logits=True)


def _compose(pr, plan, B, seed):
    """decode_step at positions 0..2, then position 2 again stage by stage on the same engine (the step is a function of the tokens,
    the position and the cache rows below it): logits and appended cache rows bit-equal"""
    rs = np.random.RandomState(seed)
    toks = rs.randint(0, pr.V, size=(3, B))
    for p in range(3):
        lg = pr.decode_step(toks[p], p)
    caches = [(pr.get_dev("kcache", l).clone(), pr.get_dev("vcache", l).clone()) for l in range(pr.nl)]
    for l in range(pr.nl):                                       # the rows the walk has to append again
        for nm, t in zip(("kcache", "vcache"), caches[l]):
            z = t.clone().view(pr.Bmax, pr.H, pr.T, pr.hd)
            z[:B, :, 2] = SENT
            pr.put(nm, z, l)
    # no work buffer keeps what decode_step left: a stage that writes nothing, or to the wrong buffer, shows
    for nm in ("x", "x2", "y", "hbuf", "slabs", "qkv_slabs", "xs", "ys", "hs", "qs"):
        if pr.has(nm):
            pr.fill(nm, SENT)
    for nm in ("stats", "stats_q"):
        pr.fill(nm, 1e300)
    if pr.has("yq"):
        pr.fill("yq", 0)
    lg2 = _stage_walk(pr, plan, toks[2], 2)
    bad = R.diff_bits(lg2, lg)
    for l in range(pr.nl):
        for nm, t in zip(("kcache", "vcache"), caches[l]):
            bad += int((pr.get_dev(nm, l).view(torch.int32) != t.view(torch.int32)).sum())
    assert bad == 0, "stage walk and decode_step differ in %d floats" % bad
    assert np.isfinite(lg).all()
    return bad


@pytest.mark.parametrize("case", [("A", (), 13), ("A", (), 64), ("A", (), 128), ("A", ("WMAR_NO_XR",), 63), ("B", (), 64), ("C", (), 32), ("C", (), 127),
                                  ("C", ("WMAR_NO_BX",), 63), ("D", (), 33)], ids=str)
def test_stage_walk_equals_decode_step(case):
    name, env, B = case
    pr = _probe(name, "dense", env)
    plan = _plan(pr, env, B, 3)
    _compose(pr, plan, B, 5)
    _say("composition %s%s B=%d" % (name, "".join(env), B), stages=len(plan["stages"]), differing_bits=0)


def test_stage_walk_equals_decode_step_on_the_small_plan_and_after_127_then_5_rows():
    pr = _probe("A", "dense")
    rs = np.random.RandomState(6)
    pr.decode_step(rs.randint(0, pr.V, size=127), 0)                 # 127 rows leave their garbage in every work buffer
    for B in (5, 1, 12):
        plan = pr.plan(B, 3)
        assert plan["small"] == 1
        _compose(pr, plan, B, 7 + B)
    _say("composition A small plan", rows="5,1,12", differing_bits=0)


# ------------------------------------------------------------------------------------------------------------------- split GEMMs
def _int_weight(pr, key, layer, gamma_key=None):
    W = np.concatenate([pr.w("attn.%s.weight" % k, layer) for k in ("query", "key", "value")]) if key == "qkv" else pr.w(key, layer)
    return R.fold_gamma(W, pr.w(gamma_key, layer) if gamma_key else None)


def _qkv_ranges(plan, KB, NT):
    if plan["rowmajor"]:
        return R.uniform_ranges(NT, lambda s: R.qkvx_bx_kblocks(KB, plan["S_qx"], s), plan["S_qx"])
    if plan["S_qx"] > 0:
        return R.uniform_ranges(NT, lambda s: R.qkvx_kblocks(KB, plan["S_qx"], s), plan["S_qx"])
    return R.gemm_ranges(KB, NT, plan["S_qkv"])


def _fc2_slabs(pr, plan, rs, M, Mpad, kind):
    """planted FC2 slabs of the previous block: S_fc2 (+ 1 below fc2_hi) pieces, SENTINEL where a tile owns no last slab and behind"""
    D, S, hi = pr.D, plan["S_fc2"], plan["fc2_hi"]
    n = S + (1 if hi > 0 else 0)
    P = (rs.randint(-1, 2, size=(n, Mpad, D)) if kind == "int" else rs.randn(n, Mpad, D)).astype(np.float32)
    P[:, M:] = GARBAGE
    if hi > 0:
        P[n - 1, :, hi * 32:] = SENT
    flat = np.full(pr.size("slabs") // 4, SENT, dtype=np.float32)
    pr.put("slabs", R.put_pieces(flat, P, plan["MT"]))
    return [P[i] for i in range(n)]


GEMM_CASES = [("A", (), 13), ("A", (), 31), ("A", (), 32), ("A", (), 33), ("A", (), 63), ("A", (), 64), ("A", (), 65), ("A", (), 127), ("A", (), 128), ("A", ("WMAR_NO_XR",), 63), ("B", (), 31),
              ("B", (), 64), ("C", (), 5), ("C", (), 33), ("C", (), 127), ("C", ("WMAR_NO_BX",), 63), ("D", (), 13), ("D", (), 33)]


@pytest.mark.parametrize("case", GEMM_CASES, ids=str)
def test_qkv_pieces_fold_and_statistics_are_exact_with_integers(case):
    """QKV of block 1: the fold of block 0's FC2 inside k_qkvx / k_qkvx_bx (x', statistics per K slice), every piece the integer
    partial sum over exactly its k-blocks, pieces past the plan's count untouched, padding-row garbage in no live row"""
    name, env, B = case
    pr = _probe(name, "int", env)
    plan = _plan(pr, env, B)
    MT, D, KB = plan["MT"], pr.D, pr.D // 8
    Mpad, rs = 32 * MT, np.random.RandomState(B)
    Wg = _int_weight(pr, "qkv", 1, "ln1.weight")
    X = _rows(Mpad, B, D, rs)
    pr.put_x(X, MT)
    ranges = _qkv_ranges(plan, KB, 3 * D // 32)
    pr.fill("qkv_slabs", SENT)
    pr.fill("stats_q", 1e300)
    bad = 0
    if plan["S_qx"] > 0:
        slabs = _fc2_slabs(pr, plan, rs, B, Mpad, "int")
        src = pr.cur(plan, R.QKV, 1)
        dst = "x2" if src == "x" else "x"
        pr.fill(dst, SENT)
        pr.run(R.QKV, R.QKV, B, 0, 1)
        Xn = R.resid_ref(X[:B], pr.w("mlp.2.bias", 0), [s[:B] for s in slabs], plan["fc2_hi"])
        assert np.abs(Xn).max() <= 16
        bad += R.check_exact(pr.get_act(dst, MT, D)[:B], Xn, "x' of the fused fold")
        bad += R.check_exact(pr.get_act(src, MT, D)[:B], X[:B], "the buffer the fold reads")
        chunks = R.chunk_lists(KB, "qkvx_bx", S=plan["S_qx"], nkeep=plan["nkeep"]) if plan["rowmajor"] else R.chunk_lists(KB, "qkvx", S=plan["S_qx"])
        R.check_stats(pr.get_stats("stats_q", len(chunks), MT), np.concatenate([Xn, X[B:]]), chunks, B, exact=True)
        assert np.all(pr.get("stats_q")[len(chunks) * Mpad * 2:] == 1e300), "statistics chunks past the plan's count were written"
        Xin = np.concatenate([Xn, X[B:]])
    else:
        pr.run(R.QKV, R.QKV, B, 0, 1)
        Xin = X
    got = R.get_pieces(pr.get("qkv_slabs"), R.MAX_SLABS, MT, 3 * D, bool(plan["rowmajor"]))
    bad += R.check_gemm_exact(got, Wg, Xin, ranges, B)
    _say("QKV int %s%s B=%d" % (name, "".join(env), B), kernel=plan["roles"]["qkv"].split(" ")[0], pieces=len(ranges), differing_bits=bad)


@pytest.mark.parametrize("case", GEMM_CASES, ids=str)
def test_proj_and_fc2_pieces_are_exact_with_integers(case):
    name, env, B = case
    pr = _probe(name, "int", env)
    plan = _plan(pr, env, B)
    MT, D = plan["MT"], pr.D
    Mpad, rs = 32 * MT, np.random.RandomState(100 + B)
    # ---- PROJ: k_gemm on y, k_bx / k_bx_xr on the bf16 planes yq
    Wp = _int_weight(pr, "attn.proj.weight", 1)
    Y = _rows(Mpad, B, D, rs)
    if plan["proj"] == "gemm":
        pr.put_act("y", Y, MT)
        ranges = R.gemm_ranges(D // 8, D // 32, plan["S_proj"])
    else:
        pr.put("yq", R.pack_planes(Y, 2))                         # (the planes always hold 64 rows)
        ranges = R.uniform_ranges(D // 32, R.bx_kblocks, plan["S_proj"])
    pr.fill("slabs", SENT)
    xr = plan["proj"] == "bx_xr"
    if xr:
        X = _rows(Mpad, B, D, rs)
        pr.put_x(X, MT)
        pr.fill("stats", 1e300)
    pr.run(R.PROJ, R.PROJ, B, 0, 1)
    got = R.get_pieces(pr.get("slabs"), R.MAX_SLABS, MT, D)
    bad = R.check_gemm_exact(got, Wp, Y, ranges, B)
    if xr:                                                         # phase 2: x += bproj + (s0 + s1 + s2 + s3), statistics chunks 2 g + half
        cur = pr.cur(plan, R.PROJ, 1)
        Xn = R.resid_ref(X[:B], pr.w("attn.proj.bias", 1), [got[s, :B] for s in range(4)])
        xg = pr.get_act(cur, MT, D)
        bad += R.check_exact(xg[:B], Xn, "x after k_bx_xr")
        R.check_stats(pr.get_stats("stats", 16, MT), xg, R.chunk_lists(D // 8, "xr"), B, exact=True)
    # ---- FC2: S_fc2 slices, one more for the first fc2_hi column tiles
    W2 = _int_weight(pr, "mlp.2.weight", 1)
    Hh = _rows(Mpad, B, 4 * D, rs)
    pr.put_act("hbuf", Hh, MT)
    pr.fill("slabs", SENT)
    pr.run(R.FC2, R.FC2, B, 0, 1)
    r2 = R.gemm_ranges(4 * D // 8, D // 32, plan["S_fc2"], plan["fc2_hi"])
    bad += R.check_gemm_exact(R.get_pieces(pr.get("slabs"), R.MAX_SLABS, MT, D), W2, Hh, r2, B)
    _say("PROJ+FC2 int %s%s B=%d" % (name, "".join(env), B), proj=plan["roles"]["proj"].split(" ")[0], S_proj=plan["S_proj"], S_fc2=plan["S_fc2"],
         fc2_hi=plan["fc2_hi"], differing_bits=bad)


DENSE_CASES = [("A", (), 32), ("A", (), 64), ("A", (), 128), ("A", ("WMAR_NO_XR",), 63), ("B", (), 64), ("C", (), 33), ("C", ("WMAR_NO_BX",), 63), ("D", (), 33)]


@pytest.mark.parametrize("case", DENSE_CASES, ids=str)
def test_dense_gemm_pieces_meet_the_chain_bound(case):
    """random full-significand operands: every piece of QKV (block 0: no fold), PROJ and FC2 within 2 x the normalised error of a
    sequential fp32 chain over the same terms"""
    name, env, B = case
    pr = _probe(name, "dense", env)
    plan = _plan(pr, env, B)
    MT, D, KB = plan["MT"], pr.D, pr.D // 8
    Mpad, rs = 32 * MT, np.random.RandomState(200 + B)
    figs = {}
    X = _rows(Mpad, B, D, rs, "dense")
    X[B:] = 0.5
    pr.put_x(X, MT)
    pr.run(R.QKV, R.QKV, B, 0, 0)
    got = R.get_pieces(pr.get("qkv_slabs"), R.MAX_SLABS, MT, 3 * D, bool(plan["rowmajor"]))
    figs["qkv"] = R.check_gemm_dense(got, _int_weight(pr, "qkv", 0, "ln1.weight"), X, _qkv_ranges(plan, KB, 3 * D // 32), B)[2]
    Y = _rows(Mpad, B, D, rs, "dense")
    Y[B:] = 0.5
    if plan["proj"] == "gemm":
        pr.put_act("y", Y, MT)
        ranges = R.gemm_ranges(KB, D // 32, plan["S_proj"])
    else:
        pr.put("yq", R.pack_planes(Y, 2))
        ranges = R.uniform_ranges(D // 32, R.bx_kblocks, plan["S_proj"])
    pr.put_x(X, MT)
    pr.run(R.PROJ, R.PROJ, B, 0, 0)
    figs["proj"] = R.check_gemm_dense(R.get_pieces(pr.get("slabs"), R.MAX_SLABS, MT, D), pr.w("attn.proj.weight", 0), Y, ranges, B)[2]
    Hh = _rows(Mpad, B, 4 * D, rs, "dense")
    Hh[B:] = 0.5
    pr.put_act("hbuf", Hh, MT)
    pr.run(R.FC2, R.FC2, B, 0, 0)
    figs["fc2"] = R.check_gemm_dense(R.get_pieces(pr.get("slabs"), R.MAX_SLABS, MT, D), pr.w("mlp.2.weight", 0), Hh,
                                     R.gemm_ranges(4 * KB, D // 32, plan["S_fc2"], plan["fc2_hi"]), B)[2]
    _say("dense GEMM %s%s B=%d" % (name, "".join(env), B), **{"worst_x_chain_" + k: float(v) for k, v in figs.items()})


# ------------------------------------------------------------------------------------------------------------------- residual launches
RESID_CASES = [("A", (), 13), ("A", (), 64), ("A", (), 127), ("A", ("WMAR_NO_XR",), 63), ("B", (), 64), ("C", (), 33), ("C", ("WMAR_NO_BX",), 63),
               ("D", (), 13), ("D", (), 33), ("E", (), 13)]


@pytest.mark.parametrize("kind", ["dense", "int"])
@pytest.mark.parametrize("case", RESID_CASES, ids=str)
def test_residual_updates_are_exact_and_statistics_meet_their_bound(case, kind):
    """EMBED, RESID_IN (where the plan has it), the fold inside QKV (where it has not), RESID_ATTN or phase 2 of k_bx_xr, RESID_OUT on
    full-significand data: x' = x + (bias + (s0 + s1 + ..)) in fp32 in slab order bit for bit, the short slab of tiles at or past
    fc2_hi never added, statistics within K 2^-53 sum x^2 of float64; and on the integer engine (inputs of at most 16 significant
    bits: every square and every sum is exact in fp64) the statistics of every one of these launches bit for bit"""
    name, env, B = case
    pr = _probe(name, kind, env)
    exact = kind == "int"

    def rnd(*shape):
        return (rs.randint(-8, 9, size=shape) if exact else rs.randn(*shape)).astype(np.float32)
    plan = _plan(pr, env, B)
    MT, D, KB = plan["MT"], pr.D, pr.D // 8
    Mpad, rs = 32 * MT, np.random.RandomState(300 + B)
    rchunks = R.chunk_lists(KB, "resid", nch=plan["nch"])
    bad, worst = 0, 0.0
    # EMBED
    tok, pos = rs.randint(0, pr.V, size=B), 3
    pr.fill("x", SENT)
    pr.fill("stats", 1e300)
    pr.run(R.EMBED, R.EMBED, B, pos, 0, tok=tok)
    xe = R.embed_ref(pr.w("tok_emb.weight"), pr.w("pos_emb")[0], tok, pos, Mpad)
    xg = pr.get_act("x", MT, D)
    bad += R.check_exact(xg, xe, "embedding")
    worst = max(worst, R.check_stats(pr.get_stats("stats", plan["nch"], MT), xe, rchunks, B, exact=exact))
    L1 = pr.nl - 1

    def fold_stage(stage, layer, bias, slabs, n_hi, chunks, stats_name):
        nonlocal bad, worst
        X = _rows(Mpad, B, D, rs, kind)
        X[B:] = 0.25
        pr.put_x(X, MT)
        pr.fill(stats_name, 1e300)
        pr.run(stage, stage, B, 0, layer)
        cur = pr.cur(plan, stage, layer)
        if stage == R.QKV:
            cur = "x2" if cur == "x" else "x"
        xg = pr.get_act(cur, MT, D)
        bad += R.check_resid(xg, X, bias, slabs, n_hi, B)
        worst = max(worst, R.check_stats(pr.get_stats(stats_name, len(chunks), MT), xg, chunks, B, exact=exact))

    if pr.nl > 1:
        slabs = _fc2_slabs(pr, plan, rs, B, Mpad, kind)
        if plan["S_qx"] > 0:
            qch = R.chunk_lists(KB, "qkvx_bx", S=plan["S_qx"], nkeep=plan["nkeep"]) if plan["rowmajor"] else R.chunk_lists(KB, "qkvx", S=plan["S_qx"])
            fold_stage(R.QKV, 1, pr.w("mlp.2.bias", 0), slabs, plan["fc2_hi"], qch, "stats_q")
        else:
            fold_stage(R.RESID_IN, 1, pr.w("mlp.2.bias", 0), slabs, plan["fc2_hi"], rchunks, "stats")
    slabs = _fc2_slabs(pr, plan, rs, B, Mpad, kind)
    fold_stage(R.RESID_OUT, L1, pr.w("mlp.2.bias", L1), slabs, plan["fc2_hi"], rchunks, "stats")
    if "RESID_ATTN" in plan["stages"]:
        P = rnd(plan["S_proj"], Mpad, D)
        P[:, B:] = GARBAGE
        pr.put("slabs", R.put_pieces(np.full(pr.size("slabs") // 4, SENT, dtype=np.float32), P, MT))
        fold_stage(R.RESID_ATTN, L1, pr.w("attn.proj.bias", L1), [P[i] for i in range(plan["S_proj"])], 0,
                   R.chunk_lists(KB, "resid", nch=plan["nch_ln2"]), "stats")
    else:                                                          # k_bx_xr: its own slabs, then the fold (dense operands)
        Y = rnd(Mpad, D)
        pr.put("yq", R.pack_planes(Y, 2))
        X = rnd(Mpad, D)
        pr.put_x(X, MT)
        pr.fill("stats", 1e300)
        pr.run(R.PROJ, R.PROJ, B, 0, L1)
        got = R.get_pieces(pr.get("slabs"), 4, MT, D)
        xg = pr.get_act(pr.cur(plan, R.PROJ, L1), MT, D)
        bad += R.check_resid(xg, X, pr.w("attn.proj.bias", L1), [got[s] for s in range(4)], 0, B)
        worst = max(worst, R.check_stats(pr.get_stats("stats", 16, MT), xg, R.chunk_lists(KB, "xr"), B, exact=exact))
    _say("residual %s %s%s B=%d" % (kind, name, "".join(env), B), differing_bits=bad, stats_worst_of_bound=float(worst))


# ------------------------------------------------------------------------------------------------------------------- LayerNorm-fused launches
def _ln_stats_name_and_chunks(pr, plan, stage):
    KB = pr.D // 8
    if stage == R.FC1:
        return "stats", (R.chunk_lists(KB, "xr") if plan["proj"] == "bx_xr" else R.chunk_lists(KB, "resid", nch=plan["nch_ln2"]))
    return "stats", R.chunk_lists(KB, "resid", nch=plan["nch"])


LN_CASES = [("A", (), 13), ("A", (), 31), ("A", (), 33), ("A", (), 63), ("A", (), 64), ("A", (), 65), ("A", (), 127), ("A", (), 128), ("A", ("WMAR_NO_XR",), 63), ("B", (), 64), ("C", (), 5),
            ("C", (), 32), ("C", (), 33), ("C", (), 127), ("D", (), 13), ("D", (), 33), ("E", (), 13)]


@pytest.mark.parametrize("case", LN_CASES, ids=str)
def test_fc1_and_head_with_one_hot_weights_and_zero_mean_rows(case):
    """one-hot integer FC1 / head weights, integer rows of sum exactly 0: the pre-activation is rstd x[k(n)] gamma[k(n)] w + b; every
    element within 4.25 x 2^-24 (+ the final rounding; through gelu_erf for FC1) of the float64 value, no element exempt"""
    name, env, B = case
    pr = _probe(name, "int", env)
    plan = _plan(pr, env, B)
    MT, D = plan["MT"], pr.D
    Mpad, rs = 32 * MT, np.random.RandomState(400 + B)
    L1 = pr.nl - 1
    figs = {}
    for stage, Wk, gk, bk, wb, N in ((R.FC1, "blocks.%d.mlp.0.weight" % L1, "blocks.%d.ln2.weight" % L1, "blocks.%d.ln2.bias" % L1,
                                      "blocks.%d.mlp.0.bias" % L1, 4 * D), (R.HEAD, "head.weight", "ln_f.weight", "ln_f.bias", None, pr.V)):
        X = _zero_sum_rows(Mpad, B, D, rs)
        pr.put_x(X, MT)
        sname, chunks = _ln_stats_name_and_chunks(pr, plan, stage)
        st = R.stats_ref(X, chunks)
        pr.put_stats(sname, st, MT)
        Wg = R.fold_gamma(pr.w(Wk), pr.w(gk))
        acc = (X[:B].astype(np.float64) @ Wg.astype(np.float64).T).astype(np.float32)
        b = pr.get("bfc1", L1) if stage == R.FC1 else pr.get("bhead")
        mean, rstd = R.mean_rstd64(st[:, :B], D)
        assert np.all(mean == 0)
        if stage == R.FC1:
            pr.fill("hbuf", SENT)
            pr.run(R.FC1, R.FC1, B, 0, L1)
            got = pr.get_act("hbuf", MT, 4 * D)
            figs["fc1"], _ = R.check_ln_onehot(got, acc, rstd, b, B, "FC1", gelu=True)
        else:
            got = pr.run(R.HEAD, R.HEAD, B, 0, L1, want_logits=True)
            figs["head"], figs["head_not_rn"] = R.check_ln_onehot(got, acc, rstd, b, B, "head")
    _say("LN one-hot %s%s B=%d" % (name, "".join(env), B), fc1_kernel=plan["roles"]["fc1"].split(" ")[0], head=plan["head"],
         **{k + "_worst_of_bound": float(v) for k, v in figs.items()})


@pytest.mark.parametrize("case", [("A", (), 64), ("A", (), 128), ("C", (), 32), ("C", (), 127), ("D", (), 33), ("E", (), 13)], ids=str)
def test_dense_head_and_fc1_meet_their_bounds(case):
    """random operands: the head within 2 x an fp32 numpy evaluation of the same algebra (normalised by rstd (sum |w' x| + |mean c1|) +
    |b|); FC1 after GELU within 4 x torch's CPU fp32 gelu(linear(layer_norm(x))), both against float64"""
    name, env, B = case
    pr = _probe(name, "dense", env)
    plan = _plan(pr, env, B)
    MT, D = plan["MT"], pr.D
    Mpad, rs = 32 * MT, np.random.RandomState(500 + B)
    L1 = pr.nl - 1
    X = (rs.randn(Mpad, D) * 1.5 + 0.3).astype(np.float32)
    pr.put_x(X, MT)
    figs = _ln_dense(pr, plan, X, B, L1)
    _say("LN dense %s B=%d" % (name, B), **figs)


def _ln_dense(pr, plan, X, B, L1, gate=True):
    MT, D = plan["MT"], pr.D
    figs = {}
    # head
    sname, chunks = _ln_stats_name_and_chunks(pr, plan, R.HEAD)
    st = R.stats_ref(X, chunks)
    pr.put_stats(sname, st, MT)
    got = pr.run(R.HEAD, R.HEAD, B, 0, L1, want_logits=True)
    Wh, g, be = pr.w("head.weight"), pr.w("ln_f.weight"), pr.w("ln_f.bias")
    Wg, c1, b = R.fold_gamma(Wh, g), pr.get("chead"), pr.get("bhead")
    mean, rstd = R.mean_rstd64(st[:, :B], D)
    ref = R.ln_ref64(Wh, g, be, None, X[:B])
    norm = R.ln_normaliser(Wg, X[:B], mean, rstd, c1, b)
    yard = R.ln_algebra32(Wg, X[:B], st[:, :B], c1, b, D)
    e = float((np.abs(got.astype(np.float64) - ref) / norm).max())
    ey = float((np.abs(yard.astype(np.float64) - ref) / norm).max())
    t = torch.from_numpy(X[:B])
    ref_form = torch.nn.functional.linear(torch.nn.functional.layer_norm(t, (D,), torch.from_numpy(g), torch.from_numpy(be), 1e-5), torch.from_numpy(Wh)).numpy()
    er = float((np.abs(ref_form.astype(np.float64) - ref) / norm).max())
    if gate:
        R.check_ln_dense(got, ref, norm, yard, B, "head")
    figs.update(head_err=e, head_x_yardstick=e / ey, head_x_reference_form=e / er, head_abs=float(np.abs(got - ref).max()),
                head_bound_abs=float(R.DENSE_GATE * ey * norm.max()), head_reference_form_abs=float(np.abs(ref_form - ref).max()))
    # FC1
    sname, chunks = _ln_stats_name_and_chunks(pr, plan, R.FC1)
    st = R.stats_ref(X, chunks)
    pr.put_stats(sname, st, MT)
    pr.run(R.FC1, R.FC1, B, 0, L1)
    got = pr.get_act("hbuf", MT, 4 * D)[:B]
    W1, g2, b2, bb = (pr.w(k, L1) for k in ("mlp.0.weight", "ln2.weight", "ln2.bias", "mlp.0.bias"))
    pre = R.ln_ref64(W1, g2, b2, bb, X[:B])
    ref = R.gelu64(pre)
    tt = torch.nn.functional.gelu(torch.nn.functional.linear(torch.nn.functional.layer_norm(t, (D,), torch.from_numpy(g2), torch.from_numpy(b2), 1e-5),
                                                              torch.from_numpy(W1), torch.from_numpy(bb))).numpy()
    mean, rstd = R.mean_rstd64(st[:, :B], D)
    norm = R.ln_normaliser(R.fold_gamma(W1, g2), X[:B], mean, rstd, pr.get("cfc1", L1), pr.get("bfc1", L1))
    e = float((np.abs(got.astype(np.float64) - ref) / norm).max())
    et = float((np.abs(tt.astype(np.float64) - ref) / norm).max())
    if gate:
        assert e <= R.TORCH_FACTOR * et, "FC1: normalised error %.3g is %.2f x torch's fp32 %.3g" % (e, e / et, et)
    # ... and, gated or not, to the derived normaliser: gelu is 1.13-Lipschitz and rounds to 2^-23 of |v| <= the normaliser itself
    ypre = R.ln_algebra32(R.fold_gamma(W1, g2), X[:B], st[:, :B], pr.get("cfc1", L1), pr.get("bfc1", L1), D)
    eyp = float((np.abs(ypre.astype(np.float64) - pre) / norm).max())
    assert e <= R.DENSE_GATE * R.GELU_LIP * eyp + 2.0 ** -22, "FC1: normalised error %.3g against the fp32 algebra's %.3g before GELU" % (e, eyp)
    figs.update(fc1_err=e, fc1_x_torch=e / et, fc1_x_yardstick=e / (R.GELU_LIP * eyp))
    return figs


@pytest.mark.parametrize("case", [("A", (), 64), ("C", (), 32)], ids=str)
def test_off_centre_rows_are_measured(case):
    """rows with mean / sigma = 10, 100, 1000: rstd (x W'^T - mean c1) + b cancels, the reference form (normalise, then the Linear) does
    not.  Asserted: the derived normaliser only (error <= 2 x the fp32 evaluation of the same algebra); printed: the ratio to the
    reference form in fp32, for DESIGN section 4"""
    name, env, B = case
    pr = _probe(name, "dense", env)
    plan = _plan(pr, env, B)
    MT, D = plan["MT"], pr.D
    Mpad, rs = 32 * MT, np.random.RandomState(600 + B)
    for ratio in (10.0, 100.0, 1000.0):
        X = (rs.randn(Mpad, D) + ratio).astype(np.float32)
        pr.put_x(X, MT)
        figs = _ln_dense(pr, plan, X, B, pr.nl - 1, gate=False)
        assert figs["head_x_yardstick"] <= R.DENSE_GATE
        _say("off-centre %s B=%d mean/sigma=%g" % (name, B, ratio), **figs)


# ------------------------------------------------------------------------------------------------------------------- attention
ATTN_CASES = [("A", (), 13, 1), ("A", (), 13, 2), ("A", (), 64, 1), ("A", (), 64, 4), ("A", (), 65, 2), ("B", (), 64, 1), ("B", (), 64, 2), ("B", (), 64, 4),
              ("B", (), 31, 4), ("C", (), 32, 1), ("C", (), 32, 2), ("C", (), 32, 4), ("C", (), 33, 2), ("C", ("WMAR_NO_BX",), 63, 4), ("C", (), 127, 1)]


def _attn_setup(pr, plan, B, T, rs, gen, winners, S, layer):
    """plants statistics (mean 0, variance 1), integer q / k / v pieces (q leads to the winner's K row by ~200), the caches; returns
    what the launch must produce"""
    MT, D, H, hd = plan["MT"], pr.D, pr.H, pr.hd
    Mpad = 32 * MT
    k0 = np.float32(np.ceil(5.0 * np.sqrt(hd)))
    acc = np.zeros((3, Mpad, D), dtype=np.float32)                     # q | k | v sums, all integers
    acc[0].reshape(Mpad, H, hd)[:, :, 0] = 40.0
    acc[2] = rs.randint(-8, 9, size=(Mpad, D))
    kc = torch.zeros(pr.Bmax, H, pr.T, hd, device="cuda")
    vc = torch.randn(pr.Bmax, H, pr.T, hd, device="cuda", generator=gen)
    kc[:, :, T - 1:] = 0                                                # row T - 1 is replaced from registers, rows behind it never read:
    kc[:, :, T - 1:, 0] = 1000.0                                        # a K row that would win by far if it were, with a sentinel for V
    vc[:, :, T - 1:] = SENT
    bi, hi = np.divmod(np.arange(B * H), H)
    w1 = winners[:B * H]
    new = w1 == T - 1
    kc[torch.from_numpy(bi[~new]).cuda(), torch.from_numpy(hi[~new]).cuda(), torch.from_numpy(w1[~new]).cuda(), 0] = float(k0)
    acc[1].reshape(Mpad, H, hd)[bi[new], hi[new], 0] = k0              # a dominating new token
    P = np.zeros((S, Mpad, 3 * D), dtype=np.float32)
    P[0][:, :D], P[S - 1][:, D:2 * D], P[S // 2][:, 2 * D:] = acc[0], acc[1], acc[2]
    P[:, B:] = GARBAGE
    flat = np.full(pr.size("qkv_slabs") // 4, SENT, dtype=np.float32)    # pieces at index >= S carry the sentinel
    pr.put("qkv_slabs", R.put_pieces(flat, P, MT, bool(plan["rowmajor"])))
    if plan["S_qx"] > 0:
        sname, nchk = "stats_q", (plan["S_qx"] * plan["nkeep"] if plan["rowmajor"] else plan["S_qx"])
    else:
        sname, nchk = "stats", plan["nch"]
    st = np.zeros((nchk, Mpad, 2))
    st[:, :, 1] = float(D) / nchk * (1.0 - 1e-5)
    st[:, B:] = 1e30
    pr.put_stats(sname, st, MT)
    pr.put("kcache", kc, layer)
    pr.put("vcache", vc, layer)
    return acc, kc, vc, bi, hi, w1, st


@pytest.mark.parametrize("case", ATTN_CASES, ids=str)
def test_attention_one_hot_sweep(case):
    """1 / 2 / 4 waves, packed and row-major pieces: (row, head) pair p attends to cached position p % T with a lead of ~200 and must
    return that V row bit for bit, at every length with a wave or chunk edge; the new token's K / V rows are appended within the
    derived distance, no other cache row changes, y / yq carry the values"""
    name, env, B, nwa = case
    pr = _probe(name, "dense", env)
    layer, H, hd, D = pr.nl - 1, pr.H, pr.hd, pr.D
    rs = np.random.RandomState(700 + B + nwa)
    gen = torch.Generator(device="cuda").manual_seed(B + nwa)
    pr.waves(nwa)
    try:
        n_pairs, worst, t0 = 0, 0.0, time.time()
        for T in R.attn_lengths(hd, nwa):
            plan = _plan(pr, env, B, T)
            assert plan["attn_waves"] == nwa
            MT, S = plan["MT"], (plan["S_qx"] if plan["S_qx"] > 0 else plan["S_qkv"])
            winners = (np.arange(pr.Bmax * H) + rs.randint(0, T)) % T
            acc, kc, vc, bi, hi, w1, st = _attn_setup(pr, plan, B, T, rs, gen, winners, S, layer)
            use_yq = plan["proj"] != "gemm"
            if use_yq:
                pr.fill("yq", 0)
            else:
                pr.fill("y", SENT)
            pr.run(R.ATTN, R.ATTN, B, T - 1, layer)
            ka, va = pr.get_dev("kcache", layer).view(pr.Bmax, H, pr.T, hd), pr.get_dev("vcache", layer).view(pr.Bmax, H, pr.T, hd)
            # appended rows: rstd * acc + b within the derived distance; nothing else changed
            mean, rstd = R.mean_rstd64(st[:, :B], D)
            bq = pr.get("bqkv", layer)
            for which, cache in ((1, ka), (2, va)):
                gotrow = cache[:B, :, T - 1].reshape(B, D).cpu().numpy()
                worst = max(worst, R.check_ln_onehot(gotrow, acc[which], rstd, bq[which * D:(which + 1) * D], B, "appended %s row" % "qkv"[which])[0])
            for before, after in ((kc, ka), (vc, va)):
                b2, a2 = before.clone(), after.clone()
                b2[:B, :, T - 1] = 0
                a2[:B, :, T - 1] = 0
                assert torch.equal(b2.view(torch.int32), a2.view(torch.int32)), "a cache row outside the appended ones changed"
            # the output: the winner's V row (the appended one for the new token)
            vfull = va.clone()
            want = vfull[torch.from_numpy(bi).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(w1).cuda()].reshape(B, D).cpu().numpy()
            if use_yq:
                h, m, l = R.unpack_planes(pr.get("yq"), 2, D)
                y = (h.astype(np.float64) + m + l).astype(np.float32)
            else:
                y = pr.get_act("y", MT, D)
            R.check_onehot(y[:B], want)
            n_pairs += B * H
        # two equal winners (first and last cached row of the longest length that keeps them in different chunks) return their mean
        T = min(4 * R.attn_chunk_rows(hd) * nwa + 1, pr.T)
        plan = _plan(pr, env, B, T)
        S = plan["S_qx"] if plan["S_qx"] > 0 else plan["S_qkv"]
        winners = np.zeros(pr.Bmax * H, dtype=np.int64)
        acc, kc, vc, bi, hi, w1, st = _attn_setup(pr, plan, B, T, rs, gen, winners, S, layer)
        kc[:, :, T - 2, 0] = kc[0, 0, 0, 0]
        pr.put("kcache", kc, layer)
        pr.run(R.ATTN, R.ATTN, B, T - 1, layer)
        want = ((vc[:B, :, 0] + vc[:B, :, T - 2]) * 0.5).reshape(B, D).cpu().numpy()
        if plan["proj"] != "gemm":
            h, m, l = R.unpack_planes(pr.get("yq"), 2, D)
            y = (h.astype(np.float64) + m + l).astype(np.float32)
        else:
            y = pr.get_act("y", plan["MT"], D)
        R.check_onehot(y[:B], want, "two winners")
    finally:
        pr.waves(0)
    _say("attention one-hot %s%s B=%d nwa=%d" % (name, "".join(env), B, nwa), kernel="k_attn_decode<%d,%d,rm=%d>" % (hd, nwa, plan["rowmajor"]),
         lengths=len(R.attn_lengths(hd, nwa)), pairs=n_pairs, differing_bits=0, appended_worst_of_bound=float(worst), seconds=time.time() - t0)


@pytest.mark.parametrize("case", [("A", (), 64, 1), ("B", (), 64, 2), ("C", (), 32, 4), ("E", (), 65, 1)], ids=str)
def test_dense_attention_meets_the_fp32_bound(case):
    """random q / k / v and caches at 32..block_size rows, against float64: every output within the distance derived from the launch's
    own steps (tests/gpt_kernel_reference.py), and the largest error of a launch within 4 x the largest error of an fp32 numpy
    evaluation of softmax V.  The same 4 x per single (row, head) is not met by this kernel (measured 9.4 .. 13.3 x at the worst
    pair of 256-row caches, 6.1 x at 16 rows, while the launch maxima are 0.8 .. 1.6 x): the quotient of two rounding errors of one
    pair has no bound -- the fp32 evaluation lands within 1e-7 of float64 on some pairs -- and __expf (exp2 of the scaled argument,
    (2 + 1.16 |x|) ulp) and the 1 ulp of rsqrtf in q move every weight by more than numpy's exp does.  The per-pair quotient is printed."""
    name, env, B, nwa = case
    pr = _probe(name, "dense", env)
    layer, H, hd, D = pr.nl - 1, pr.H, pr.hd, pr.D
    rs = np.random.RandomState(800 + B)
    gen = torch.Generator(device="cuda").manual_seed(B)
    pr.waves(nwa)
    try:
        worst, x32, emax, e32max, xmax, xapp = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
        for T in sorted({min(32, pr.T), min(97, pr.T), pr.T}):
            plan = _plan(pr, env, B, T)
            MT, S = plan["MT"], (plan["S_qx"] if plan["S_qx"] > 0 else plan["S_qkv"])
            Mpad = 32 * MT
            P = rs.randn(S, Mpad, 3 * D).astype(np.float32)
            P[:, B:] = 0.5
            pr.put("qkv_slabs", R.put_pieces(np.full(pr.size("qkv_slabs") // 4, SENT, dtype=np.float32), P, MT, bool(plan["rowmajor"])))
            if plan["S_qx"] > 0:
                sname, nchk = "stats_q", (plan["S_qx"] * plan["nkeep"] if plan["rowmajor"] else plan["S_qx"])
            else:
                sname, nchk = "stats", plan["nch"]
            st = np.zeros((nchk, Mpad, 2))
            m_row, v_row = (0.5 + rs.rand(Mpad)) * rs.choice([-1.0, 1.0], size=Mpad), 0.5 + rs.rand(Mpad)    # |mean| of the order of sigma
            wc, wq = rs.rand(nchk, Mpad) + 0.5, rs.rand(nchk, Mpad) + 0.5        # uneven over the chunks, the row's totals as drawn
            st[:, :, 0] = float(D) * m_row[None, :] * wc / wc.sum(0)
            st[:, :, 1] = float(D) * (m_row ** 2 + v_row)[None, :] * wq / wq.sum(0)
            pr.put_stats(sname, st, MT)
            kc = torch.randn(pr.Bmax, H, pr.T, hd, device="cuda", generator=gen)
            vc = torch.randn(pr.Bmax, H, pr.T, hd, device="cuda", generator=gen)
            pr.put("kcache", kc, layer)
            pr.put("vcache", vc, layer)
            pr.run(R.ATTN, R.ATTN, B, T - 1, layer)
            if plan["proj"] != "gemm":
                h, m, l = R.unpack_planes(pr.get("yq"), 2, D)
                y = (h.astype(np.float64) + m + l).astype(np.float32)[:B]
            else:
                y = pr.get_act("y", MT, D)[:B]
            # the K / V rows the prologue appends: rstd (sum of the pieces - mean c1) + b within 2 x an fp32 numpy evaluation of it
            v64, nrm, y32 = R.ln_pieces(P[:, :B], st[:, :B], pr.get("cqkv", layer), pr.get("bqkv", layer), D)
            ka = pr.get_dev("kcache", layer).view(pr.Bmax, H, pr.T, hd)[:B, :, T - 1].reshape(B, D).cpu().numpy()
            va = pr.get_dev("vcache", layer).view(pr.Bmax, H, pr.T, hd)[:B, :, T - 1].reshape(B, D).cpu().numpy()
            for got_row, sl, what in ((ka, slice(D, 2 * D), "appended K row"), (va, slice(2 * D, 3 * D), "appended V row")):
                xapp = max(xapp, R.check_ln_dense(got_row, v64[:, sl], nrm[:, sl], y32[:, sl], B, what)[2])
            # q / k / v of the new token in float64 from the pieces, with the distance the prologue's fp32 algebra may be off by
            acc, amag = P.astype(np.float64).sum(0)[:B], np.abs(P.astype(np.float64)).sum(0)[:B]
            mean, rstd = R.mean_rstd64(st[:, :B], D)
            c1, bq = pr.get("cqkv", layer).astype(np.float64), pr.get("bqkv", layer).astype(np.float64)
            qkv = rstd[:, None] * (acc - mean[:, None] * c1[None, :]) + bq[None, :]
            dqkv = (R.DELTA_RSTD + (S + 1) * R.HALF_ULP) * rstd[:, None] * (amag + np.abs(mean[:, None] * c1[None, :])) + R.HALF_ULP * np.abs(qkv)
            K = kc[:B, :, :T].double().cpu().numpy()
            V = vc[:B, :, :T].double().cpu().numpy()
            K[:, :, T - 1] = qkv[:, D:2 * D].reshape(B, H, hd)
            V[:, :, T - 1] = qkv[:, 2 * D:].reshape(B, H, hd)
            q, dq, dk, dv = (a.reshape(B, H, hd) for a in (qkv[:, :D], dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]))
            ref, tol = R.attn_dense_bound(q, dq, K, dk, V, dv, 1.0 / np.sqrt(hd), R.attn_chunk_rows(hd), nwa)
            worst = max(worst, R.check_attn_dense(y.reshape(B, H, hd), ref, tol))
            e32 = np.abs(R.attn_fp32(q, K, V, 1.0 / np.sqrt(hd)).astype(np.float64) - ref).max(-1) / np.abs(ref).max(-1)
            ek = np.abs(y.reshape(B, H, hd).astype(np.float64) - ref).max(-1) / np.abs(ref).max(-1)
            # ... and over the launch: the largest error of any (row, head) within 4 x the largest of the fp32 evaluation
            assert ek.max() <= R.TORCH_FACTOR * e32.max(), "attention at %d rows: max error %.3g is %.2f x the fp32 evaluation's %.3g" % (
                T, ek.max(), ek.max() / e32.max(), e32.max())
            x32, emax, e32max = max(x32, float((ek / np.maximum(e32, 1e-300)).max())), max(emax, float(ek.max())), max(e32max, float(e32.max()))
            xmax = max(xmax, float(ek.max() / e32.max()))
    finally:
        pr.waves(0)
    _say("attention dense %s B=%d nwa=%d" % (name, B, nwa), appended_rows_x_fp32_algebra=float(xapp), worst_of_derived_bound=float(worst), max_err_x_fp32_evaluation=xmax,
         worst_pair_x_fp32_evaluation=x32, max_err=emax, max_err_fp32_evaluation=e32max)


# ------------------------------------------------------------------------------------------------------------------- small-batch plan
@pytest.mark.parametrize("B", list(range(1, 13)))
def test_small_plan_stages(B):
    """k_sembed, PROJ and FC2 with integers exact (the residual added in place); QKV / FC1 / HEAD on zero-mean integer rows within the
    derived distance; k_sattn returns the winner's V row; rows at index >= B of xs / ys / hs / qs untouched"""
    pr = _probe("A12", "int")
    plan = pr.plan(B)
    assert plan["small"] == 1 and "k_sgemv<FC2>" in plan["roles"]["fc2"]
    D, H, hd, L1 = pr.D, pr.H, pr.hd, 1
    rs = np.random.RandomState(900 + B)
    gen = torch.Generator(device="cuda").manual_seed(B)
    bad = 0

    def rows(width, kind="int"):
        a = np.full((R.SG_MAX_ROWS, width), SENT, dtype=np.float32)
        a[:B] = rs.randint(-8, 9, size=(B, width)) if kind == "int" else _zero_sum_rows(B, B, width, rs)
        return a
    # EMBED
    tok = rs.randint(0, pr.V, size=B)
    pr.fill("xs", SENT)
    pr.run(R.EMBED, R.EMBED, B, 5, 0, tok=tok)
    xs = pr.get("xs").reshape(R.SG_MAX_ROWS, D)
    bad += R.check_exact(xs[:B], pr.w("tok_emb.weight")[tok] + pr.w("pos_emb")[0][5][None, :], "k_sembed")
    assert np.all(xs[B:] == R.SENTINEL)
    # PROJ and FC2: x += in W^T + b in place
    for stage, inp, width, Wk, bk in ((R.PROJ, "ys", D, "attn.proj.weight", "attn.proj.bias"), (R.FC2, "hs", 4 * D, "mlp.2.weight", "mlp.2.bias")):
        X, Y = rows(D), rows(width)
        pr.put("xs", X)
        pr.put(inp, Y)
        pr.run(stage, stage, B, 0, L1)
        want = X[:B].astype(np.float64) + Y[:B].astype(np.float64) @ pr.w(Wk, L1).astype(np.float64).T + pr.w(bk, L1)[None, :]
        assert np.abs(want).max() < 2 ** 24
        xs = pr.get("xs").reshape(R.SG_MAX_ROWS, D)
        bad += R.check_exact(xs[:B], want.astype(np.float32), "k_sgemv<%s>" % R.STAGES[stage])
        assert np.all(xs[B:] == R.SENTINEL) and np.all(pr.get(inp).reshape(R.SG_MAX_ROWS, width) == Y)
    # QKV / FC1 / HEAD on zero-mean rows
    worst = 0.0
    X = rows(D, "zero")
    pr.put("xs", X)
    x64 = X[:B].astype(np.float64)
    rstd = 1.0 / np.sqrt((x64 ** 2).sum(1) / D + np.float64(R.LN_EPS))
    Wqkv = np.concatenate([pr.w("attn.%s.weight" % k, L1) for k in ("query", "key", "value")])
    acc = (x64 @ R.fold_gamma(Wqkv, pr.w("ln1.weight", L1)).astype(np.float64).T).astype(np.float32)
    pr.fill("qs", SENT)
    kb4, vb4 = pr.get_dev("kcache", L1).clone(), pr.get_dev("vcache", L1).clone()
    pr.run(R.QKV, R.QKV, B, 9, L1)
    bq = pr.get("bqkv", L1)
    qs = pr.get("qs").reshape(R.SG_MAX_ROWS, D)
    ka, va = pr.get_dev("kcache", L1), pr.get_dev("vcache", L1)
    worst = max(worst, R.check_ln_onehot(qs, acc[:, :D], rstd, bq[:D], B, "k_sgemv<QKV> q")[0])
    for which, c in ((1, ka), (2, va)):
        row = c.view(pr.Bmax, H, pr.T, hd)[:B, :, 9].reshape(B, D).cpu().numpy()
        worst = max(worst, R.check_ln_onehot(row, acc[:, which * D:(which + 1) * D], rstd, bq[which * D:(which + 1) * D], B, "k_sgemv<QKV> cache row")[0])
    R.check_cache_untouched(ka.cpu().numpy(), kb4.cpu().numpy(), B, 9, H, pr.T, hd)
    R.check_cache_untouched(va.cpu().numpy(), vb4.cpu().numpy(), B, 9, H, pr.T, hd)
    assert np.all(qs[B:] == R.SENTINEL)
    pr.fill("hs", SENT)
    pr.run(R.FC1, R.FC1, B, 0, L1)
    acc1 = (x64 @ R.fold_gamma(pr.w("mlp.0.weight", L1), pr.w("ln2.weight", L1)).astype(np.float64).T).astype(np.float32)
    hs = pr.get("hs").reshape(R.SG_MAX_ROWS, 4 * D)
    worst = max(worst, R.check_ln_onehot(hs, acc1, rstd, pr.get("bfc1", L1), B, "k_sgemv<FC1>", gelu=True)[0])
    assert np.all(hs[B:] == R.SENTINEL)
    lg = pr.run(R.HEAD, R.HEAD, B, 0, L1, want_logits=True)
    acch = (x64 @ R.fold_gamma(pr.w("head.weight"), pr.w("ln_f.weight")).astype(np.float64).T).astype(np.float32)
    worst = max(worst, R.check_ln_onehot(lg, acch, rstd, pr.get("bhead"), B, "k_sgemv<HEAD>")[0])
    # k_sattn: the one-hot sweep over the lengths with a unit (4 rows) or wave edge
    for T in (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256):
        q = np.full((R.SG_MAX_ROWS, D), SENT, dtype=np.float32)
        q[:B] = 0
        q[:B].reshape(B, H, hd)[:, :, 0] = 40.0
        kc = torch.zeros(pr.Bmax, H, pr.T, hd, device="cuda")
        vc = torch.randn(pr.Bmax, H, pr.T, hd, device="cuda", generator=gen)
        kc[:, :, T:] = 0                                                     # rows past the cache would win if they were read
        kc[:, :, T:, 0] = 1000.0
        vc[:, :, T:] = SENT
        bi, hi = np.divmod(np.arange(B * H), H)
        w1 = (np.arange(B * H) * 7 + T // 2) % T
        kc[torch.from_numpy(bi).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(w1).cuda(), 0] = 40.0
        pr.put("qs", q)
        pr.put("kcache", kc, L1)
        pr.put("vcache", vc, L1)
        pr.fill("ys", SENT)
        pr.run(R.ATTN, R.ATTN, B, T - 1, L1)
        ys = pr.get("ys").reshape(R.SG_MAX_ROWS, D)
        want = vc[torch.from_numpy(bi).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(w1).cuda()].reshape(B, D).cpu().numpy()
        bad += R.check_onehot(ys[:B], want, "k_sattn")
        assert np.all(ys[B:] == R.SENTINEL)
        assert torch.equal(pr.get_dev("kcache", L1).view(torch.int32), kc.view(-1).view(torch.int32))
    _say("small plan B=%d" % B, differing_bits=bad, ln_worst_of_bound=float(worst))
