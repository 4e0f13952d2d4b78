"""The two-slab FC2 / QKV seam of 33..64-row decode steps (WMAR_GPT_OPT_FC2X, wmar_gpt_create_opt): k_fc2x, k_qkvx_bx<2> and the
two-slab RESID_OUT through a live engine's own StepPlan (wmar_gpt_probe_*), in the way of tests/test_gpu_gpt_kernels.py and against
the same numpy statements (tests/gpt_kernel_reference.py).  Figures are printed on lines starting FC2X (run with -s).

Engines (2 blocks, vocabulary 512, block size 64), each once with the option and once without (wmar_gpt_create):
  P   n_embd 1536, 24 heads, max_batch 128: the production width; fused projection (k_bx_xr), k_fc1x; 48 K units per wave of k_fc2x
  Q   n_embd 384, 6 heads, max_batch 64: the smallest width the variant admits; each wave of k_fc2x walks 12 units (three trips of
      the four-unit ring), the projection is k_bx, FC1 is k_gemm
Rows 33, 63, 64; padding rows of every planted operand hold large finite garbage.

Bounds, and where they come from:
  * integer operands (|x| <= 8, |w| <= 4, K <= 6144: every partial sum is an integer below 2^24): each slab equals the numpy partial
    sum over its K half bit for bit; x', the QKV pieces and the statistics chunks behind two planted slabs likewise;
  * dense operands: each slab within DENSE_GATE x the normalised error of a sequential fp32 chain over the same terms (the rule of
    test_dense_gemm_pieces_meet_the_chain_bound);
  * logits with the option against logits without it, same weights and tokens: the two steps differ in FC2's summation order only, so
    their distance is held to what the existing file allows the head launch alone against float64 -- DENSE_GATE x the normalised
    error of an fp32 numpy evaluation of the head's algebra on the residual stream the default engine left (check_ln_dense)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpt_kernel_reference as R  # noqa: E402
from tests import test_gpu_gpt_kernels as K  # noqa: E402  (its engine class, operand makers and stage walk)
from tests.engine_probe import EngineCache, say  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402

SENT, GARBAGE = K.SENT, K.GARBAGE
_say = say("FC2X", 36)

SHAPES = {"P": (1536, 24, 512, 64, 2, 128), "Q": (384, 6, 512, 64, 2, 64)}      # n_embd, n_head, vocab, block, n_layer, max_batch
ROWS = (33, 63, 64)
# what wmar_gpt_probe_plan / wmar_gpt_plan_info say at 33..64 rows WITHOUT the option (the plan tests/test_gpu_gpt_kernels.py pins)
TODAY = {"P": dict(S_fc2=5, fc2_hi=16, qkv="k_qkvx_bx<6> (bf16 pipe, 7 K slices)", fc2="k_gemm<EPI_PACKED> (fp32 MFMA, 5/+1 K slices)"),
         "Q": dict(S_fc2=4, fc2_hi=0, qkv="k_qkvx_bx<4> (bf16 pipe, 8 K slices)", fc2="k_gemm<EPI_PACKED> (fp32 MFMA, 4 K slices)")}


class Probe(K.Probe):
    """One wmar_gpt engine of SHAPES, created through wmar_gpt_create_opt (fc2x) or wmar_gpt_create (the default plan)."""

    def __init__(self, name, kind, fc2x):
        self.name, self.kind, self.fc2x = name, kind, fc2x
        self.D, self.H, self.V, self.T, self.nl, self.Bmax = SHAPES[name]
        self.hd = self.D // self.H
        self.cfg = synth.GPTConfig(vocab_size=self.V, block_size=self.T, n_layer=self.nl, n_head=self.H, n_embd=self.D)
        self.sd = K._int_state(self.cfg, 11 + self.D) if kind == "int" else K._dense_state(self.cfg, 11 + self.D)
        from wmar_amd import _lib
        self._lib, self.L = _lib, _lib.load()
        self._copy, self._run, self._plan, self._destroy = (getattr(self.L, "wmar_gpt_%s" % f) for f in ("probe_copy", "probe_run", "probe_plan", "destroy"))
        tensors = {k: torch.as_tensor(v).to("cuda", torch.float32).contiguous() for k, v in self.sd.items()}
        names, ptrs, n = _lib.tensor_table(tensors)
        cfg = _lib.GptConfig(self.V, self.T, self.nl, self.H, self.D, self.Bmax)
        h = C.c_void_p()
        if fc2x:
            _lib.check(self.L.wmar_gpt_create_opt(C.byref(cfg), _lib.GPT_OPT_FC2X, names, ptrs, n, _lib.stream_ptr(), C.byref(h)))
        else:
            _lib.check(self.L.wmar_gpt_create(C.byref(cfg), names, ptrs, n, _lib.stream_ptr(), C.byref(h)))
        torch.cuda.synchronize()
        self.h = h

    def device_bytes(self):
        return int(self.L.wmar_gpt_device_bytes(self.h))


_ENGINES = EngineCache()


def _probe(name, kind, fc2x=True):
    return _ENGINES.get((name, kind, fc2x), lambda: Probe(name, kind, fc2x))


@pytest.fixture(scope="module", autouse=True)
def engines():
    yield _ENGINES
    _ENGINES.close_all()
    torch.cuda.empty_cache()


def _plan_on(pr, B, kv_len=1):
    """the plan with the option, held to what the variant must report"""
    plan = pr.plan(B, kv_len)
    if pr.name == "P" and not plan["xcd_ok"]:
        pytest.skip("this device does not place blocks with equal blockIdx % 8 on one XCD or does not hold the grid: k_bx_xr cannot run")
    assert plan["barrier_fallbacks"] == 0 and plan["small"] == 0 and plan["MT"] == 2
    assert plan["S_fc2"] == 2 and plan["fc2_hi"] == 0, (plan["S_fc2"], plan["fc2_hi"])
    assert plan["roles"]["fc2"].startswith("k_fc2x "), plan["roles"]["fc2"]
    assert plan["roles"]["qkv"].startswith("k_qkvx_bx<2> "), plan["roles"]["qkv"]
    assert plan["rowmajor"] == 1 and plan["pingpong"] == 1
    assert plan["proj"] == ("bx_xr" if pr.name == "P" else "bx")
    return plan


def _halves(D):
    """slab s of k_fc2x: K half s of every column tile"""
    KB = 4 * D // 8
    return R.uniform_ranges(D // 32, lambda s: (s * KB // 2, (s + 1) * KB // 2), 2)


CASES = [(n, B) for n in ("P", "Q") for B in ROWS]
_IDS = dict(ids=lambda c: "%s-%d" % c)


# ------------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("case", CASES, **_IDS)
def test_plan_with_and_without_the_option(case):
    name, B = case
    on, off = _probe(name, "dense", True), _probe(name, "dense", False)
    plan = _plan_on(on, B)
    today = TODAY[name]
    poff = off.plan(B)
    assert poff["S_fc2"] == today["S_fc2"] and poff["fc2_hi"] == today["fc2_hi"]
    assert poff["roles"]["qkv"] == today["qkv"] and poff["roles"]["fc2"] == today["fc2"]
    assert plan["stages"] == poff["stages"], (plan["stages"], poff["stages"])
    # nothing else in the text moves: the option's four items put back give the default engine's text, character for character
    text = on.plan_text(B, 1)
    for a, b in (("S_fc2=2 fc2_hi=0", "S_fc2=%d fc2_hi=%d" % (today["S_fc2"], today["fc2_hi"])), (plan["roles"]["qkv"], today["qkv"]),
                 (plan["roles"]["fc2"], today["fc2"])):
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    assert text == off.plan_text(B, 1)
    _say("plan %s B=%d" % (name, B), S_fc2=plan["S_fc2"], fc2_hi=plan["fc2_hi"], fc2=plan["roles"]["fc2"].split(" ")[0], qkv=plan["roles"]["qkv"].split(" ")[0])


@pytest.mark.parametrize("name", ["P", "Q"])
def test_other_row_counts_and_the_memory_bill(name):
    on, off = _probe(name, "dense", True), _probe(name, "dense", False)
    for B in (13, 32) + ((65, 128) if SHAPES[name][5] > 64 else ()):
        assert on.plan_text(B, 1) == off.plan_text(B, 1), B
    D, nl = on.D, on.nl
    assert on.device_bytes() - off.device_bytes() == nl * 16 * D * D          # the second packing of mlp.2.weight, and nothing else
    assert on.has("wfc2x16") and on.has("wfc2x8") and not off.has("wfc2x16") and not off.has("wfc2x8")
    n = 0
    for l in range(nl):
        w16, w8 = R.pack_fc1x(on.w("mlp.2.weight", l))
        n += R.check_pack(on.get("wfc2x16", l), w16, "wfc2x16") + R.check_pack(on.get("wfc2x8", l), w8, "wfc2x8") + 2
    # an unknown option bit is refused
    from wmar_amd import _lib
    cfg, h = _lib.GptConfig(512, 64, 1, 6, 384, 64), C.c_void_p()
    assert on.L.wmar_gpt_create_opt(C.byref(cfg), 2, None, None, 0, _lib.stream_ptr(), C.byref(h)) != 0 and not h
    _say("packs %s" % name, packs=n, differing_bits=0, extra_bytes=nl * 16 * D * D)


# ------------------------------------------------------------------------------------------------------------------- FC2 alone
@pytest.mark.parametrize("case", CASES, **_IDS)
def test_fc2x_slabs_are_exact_with_integers(case):
    """each of the two slabs is the integer partial sum over its K half bit for bit on every live row; pieces 2..7 of the slab buffer
    keep the sentinel in every row, padding rows included; padding-row garbage reaches no live row"""
    name, B = case
    pr = _probe(name, "int")
    plan = _plan_on(pr, B)
    MT, D = plan["MT"], pr.D
    Mpad, rs = 32 * MT, np.random.RandomState(700 + B)
    bad = 0
    for layer in range(pr.nl):
        W2 = pr.w("mlp.2.weight", layer)
        Hh = K._rows(Mpad, B, 4 * D, rs)
        pr.put_act("hbuf", Hh, MT)
        pr.fill("slabs", SENT)
        pr.run(R.FC2, R.FC2, B, 0, layer)
        got = R.get_pieces(pr.get("slabs"), R.MAX_SLABS, MT, D)
        bad += R.check_gemm_exact(got, W2, Hh, _halves(D), B)
        assert np.all(pr.get("slabs")[2 * Mpad * D:] == SENT), "k_fc2x wrote behind slab 1"
    _say("FC2 int %s B=%d" % (name, B), slabs=2, differing_bits=bad)


@pytest.mark.parametrize("case", [("P", 64), ("P", 33), ("Q", 63)], **_IDS)
def test_fc2x_dense_slabs_meet_the_chain_bound(case):
    name, B = case
    pr = _probe(name, "dense")
    plan = _plan_on(pr, B)
    MT, D = plan["MT"], pr.D
    Mpad, rs = 32 * MT, np.random.RandomState(800 + B)
    Hh = K._rows(Mpad, B, 4 * D, rs, "dense")
    pr.put_act("hbuf", Hh, MT)
    pr.fill("slabs", SENT)
    pr.run(R.FC2, R.FC2, B, 0, 0)
    got = R.get_pieces(pr.get("slabs"), R.MAX_SLABS, MT, D)
    e, ec, worst = R.check_gemm_dense(got, pr.w("mlp.2.weight", 0), Hh, _halves(D), B)
    assert np.all(got[2:] == SENT)
    _say("FC2 dense %s B=%d" % (name, B), err=e, chain_err=ec, worst_x_chain=worst)


# ------------------------------------------------------------------------------------------------------------------- the consumers of two slabs
@pytest.mark.parametrize("case", CASES, **_IDS)
def test_qkv_and_resid_out_fold_two_planted_slabs_exactly(case):
    """QKV of block 1 behind two planted slabs (integers): x', every piece and every statistics chunk exact, pieces and chunks past the
    plan's count untouched; RESID_OUT with two slabs: x' and its statistics exact"""
    name, B = case
    pr = _probe(name, "int")
    plan = _plan_on(pr, B)
    MT, D, KB = plan["MT"], pr.D, pr.D // 8
    Mpad, rs = 32 * MT, np.random.RandomState(900 + B)
    Wg = K._int_weight(pr, "qkv", 1, "ln1.weight")
    X = K._rows(Mpad, B, D, rs)
    pr.put_x(X, MT)
    pr.fill("qkv_slabs", SENT)
    pr.fill("stats_q", 1e300)
    slabs = K._fc2_slabs(pr, plan, rs, B, Mpad, "int")
    assert len(slabs) == 2
    src = pr.cur(plan, R.QKV, 1)
    dst = "x2" if src == "x" else "x"
    pr.fill(dst, SENT)
    pr.run(R.QKV, R.QKV, B, 0, 1)
    Xn = R.resid_ref(X[:B], pr.w("mlp.2.bias", 0), [s[:B] for s in slabs], 0)
    bad = R.check_exact(pr.get_act(dst, MT, D)[:B], Xn, "x' of the fused fold")
    bad += R.check_exact(pr.get_act(src, MT, D)[:B], X[:B], "the buffer the fold reads")
    chunks = R.chunk_lists(KB, "qkvx_bx", S=plan["S_qx"], nkeep=plan["nkeep"])
    Xin = np.concatenate([Xn, X[B:]])
    R.check_stats(pr.get_stats("stats_q", len(chunks), MT), Xin, chunks, B, exact=True)
    assert np.all(pr.get("stats_q")[len(chunks) * Mpad * 2:] == 1e300), "statistics chunks past the plan's count were written"
    got = R.get_pieces(pr.get("qkv_slabs"), R.MAX_SLABS, MT, 3 * D, True)
    ranges = R.uniform_ranges(3 * D // 32, lambda s: R.qkvx_bx_kblocks(KB, plan["S_qx"], s), plan["S_qx"])
    bad += R.check_gemm_exact(got, Wg, Xin, ranges, B)
    # RESID_OUT
    L1 = pr.nl - 1
    X = K._rows(Mpad, B, D, rs)
    X[B:] = 0.25
    pr.put_x(X, MT)
    slabs = K._fc2_slabs(pr, plan, rs, B, Mpad, "int")
    pr.fill("stats", 1e300)
    pr.run(R.RESID_OUT, R.RESID_OUT, B, 0, L1)
    xg = pr.get_act(pr.cur(plan, R.RESID_OUT, L1), MT, D)
    bad += R.check_resid(xg, X, pr.w("mlp.2.bias", L1), slabs, 0, B)
    rchunks = R.chunk_lists(KB, "resid", nch=plan["nch"])
    R.check_stats(pr.get_stats("stats", plan["nch"], MT), xg, rchunks, B, exact=True)
    _say("QKV + RESID_OUT int %s B=%d" % (name, B), pieces=len(ranges), chunks=len(chunks), differing_bits=bad)


# ------------------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("case", [("P", 33), ("P", 64), ("Q", 63), ("Q", 64)], **_IDS)
def test_stage_walk_equals_decode_step_with_the_option(case):
    name, B = case
    pr = _probe(name, "dense")
    plan = _plan_on(pr, B, 3)
    K._compose(pr, plan, B, 5)
    _say("composition %s B=%d" % (name, B), stages=len(plan["stages"]), differing_bits=0)


@pytest.mark.parametrize("case", [("P", 64), ("Q", 33)], **_IDS)
def test_logits_with_and_without_the_option_meet_the_head_bound(case):
    """the same tokens through both engines, positions 0..40: at positions 0, 1 and 40 the two logit matrices are within the distance
    the head launch alone is allowed against float64 (module docstring); arg-max agreement is printed"""
    name, B = case
    on, off = _probe(name, "dense", True), _probe(name, "dense", False)
    _plan_on(on, B)
    poff = off.plan(B)
    rs = np.random.RandomState(40 + B)
    toks = rs.randint(0, on.V, size=(41, B))
    Wh, g, be = off.w("head.weight"), off.w("ln_f.weight"), off.w("ln_f.bias")
    Wg, c1, b = R.fold_gamma(Wh, g), off.get("chead"), off.get("bhead")
    figs = {}
    for p in range(41):
        lg_on, lg_off = on.decode_step(toks[p], p), off.decode_step(toks[p], p)
        if p not in (0, 1, 40):
            continue
        X = off.get_act(off.cur(poff, R.HEAD, off.nl - 1), 2, off.D)
        st = off.get_stats("stats", poff["nch"], 2)
        mean, rstd = R.mean_rstd64(st[:, :B], off.D)
        ref = R.ln_ref64(Wh, g, be, None, X[:B])
        norm = R.ln_normaliser(Wg, X[:B], mean, rstd, c1, b)
        yard = R.ln_algebra32(Wg, X[:B], st[:, :B], c1, b, off.D)
        ey = float((np.abs(yard.astype(np.float64) - ref) / norm).max())
        e = float((np.abs(lg_on.astype(np.float64) - lg_off.astype(np.float64)) / norm).max())
        agree = float(np.mean(lg_on.argmax(1) == lg_off.argmax(1)))
        _say("logits on/off %s B=%d pos=%d" % (name, B, p), dist=e, head_yardstick=ey, x_bound=e / (R.DENSE_GATE * ey),
             abs_max=float(np.abs(lg_on - lg_off).max()), argmax_agreement=agree)
        figs[p] = (e, ey)
    for p, (e, ey) in figs.items():
        assert e <= R.DENSE_GATE * ey, "position %d: option on / off logits differ by %.3g of the normaliser, %.2f x the fp32 head yardstick's %.3g" % (
            p, e, e / ey, ey)


# ------------------------------------------------------------------------------------------------------------------- determinism, wrapper
def test_generation_is_deterministic_and_the_wrapper_opts_in(monkeypatch):
    """GPTEngine asks for the variant (WMAR_NO_FC2X in the environment keeps the default plan); a 16-step generation at 64 rows: 5
    eager passes and 3 graph replays give the same tokens and the same logits bit for bit"""
    from wmar_amd.models.engine import GPTEngine
    D, H, V, T, nl, _ = SHAPES["P"]
    cfg = synth.GPTConfig(vocab_size=V, block_size=T, n_layer=nl, n_head=H, n_embd=D)
    state = synth.synth_gpt_state(cfg, seed=3, logit_scale=4.0)
    monkeypatch.setenv("WMAR_NO_FC2X", "1")
    eng0 = GPTEngine(cfg, state, max_batch=64)
    assert not eng0.fc2x and eng0.plan_info(64)["fc2"] == TODAY["P"]["fc2"]
    del eng0
    monkeypatch.delenv("WMAR_NO_FC2X")
    eng = GPTEngine(cfg, state, max_batch=64)
    if not GPTEngine.DEFAULT_FC2X:
        assert not eng.fc2x
        eng = GPTEngine(cfg, state, max_batch=64, fc2x=True)
    info = eng.plan_info(64)
    assert eng.fc2x and info["fc2"].startswith("k_fc2x ") and info["qkv"].startswith("k_qkvx_bx<2> "), info
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.empty(16, 64, V, device="cuda").exponential_(1, generator=g)
    cond = (torch.arange(64) * 7 % V).cuda()
    ref_tok, ref_lg = eng.generate(cond, 16, q, 1.0, 100, 0.95, None, use_graph=False, trace_logits=True)
    bad = 0
    for use_graph, n in ((False, 4), (True, 3)):
        for _ in range(n):
            tok, lg = eng.generate(cond, 16, q, 1.0, 100, 0.95, None, use_graph=use_graph, trace_logits=True)
            bad += int((tok != ref_tok).sum()) + int((lg.view(torch.int32) != ref_lg.view(torch.int32)).sum())
    assert bad == 0, "%d tokens / logits differ between passes" % bad
    assert torch.isfinite(ref_lg).all()
    _say("determinism P B=64", eager_passes=5, graph_replays=3, steps=16, differing=bad)
