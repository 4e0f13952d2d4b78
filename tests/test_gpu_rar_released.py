"""The plans the released RAR sizes select, and attention over caches of full length.

RarARMMWrapper ships RAR-B / -L / -XL / -XXL (768 / 1024 / 1280 / 1408 wide, 16 heads of 48 / 64 / 80 / 88); the stage files ran toy
widths and the XL width only.  This file runs the BODIES of tests/test_gpu_rar_kernels.py (same checks, same gates, nothing new) on
one-block engines of the other three widths, and a sweep of its own over the attention launch at up to 258 cached rows.

1. Released widths, stage by stage (engines RB / RL / RXXL at 20 / 64 / 97 / 127 / 128 rows; P16 / P20, 256 wide with F 8192 / 6400, at
   97 / 128 rows for k_bx<2,16,4> and <2,20,4>; vocabulary 256, 8 classes, 18 positions, max_batch 64).  Every case asserts the probe
   plan against rar_kernel_reference.expected_plan AND against released_pins(), the table written down by hand: k_bx<2,8,4> as FC2 of
   RB (6 slabs) and RL (8 slabs), QKV pieces in 3 / 4 slabs into the head_dim 48 / 64 prologue, yq planes out of k_attn_decode<48> /
   <64>, 11 / 44 statistics chunks and the four-row-tile GELU GEMM at 1408.  Integer GEMM stages: 0 differing floats, pieces past the
   plan untouched; dense pieces and the head under DENSE_GATE; FC1 through GELU (planes, four and two row tiles); k_resid_mod at S = 3,
   4, 5, 6, 8 (integer fold bit-exact, dense per element, published sums, every other buffer byte for byte); k_modulate / k_rar_embed at
   6 / 8 / 11 chunks; attention mode 1 and the appended rows at 128 rows; the stage walk against wmar_rar_forward_position and the
   shared_u walk against the plain walk: 0 differing bits.
   Composition: positions 0..5 at 128 rows through wmar_rar_forward_position against rar_kernel_reference.position64 (float64).  The
   gate is measured, not fixed: TORCH_FACTOR = 4 x the largest logit error of oracle.rar_oracle.rar_position evaluated in float32 on
   the CPU against position64 on the same inputs (the margin the stage files give an fp32 evaluation: the engine sums in another order
   and uses __expf).

2. Full-length caches, MODE 1 attention alone (engines A32 .. A128: 4 heads of 32 / 48 / 64 / 80 / 88 / 128, one block, 258 positions,
   max_batch 32 = 64 rows = 256 (row, head) pairs; A80R: head_dim 80 at max_batch 64 = 128 rows for k_attn_decode80<1> rowmajor).
   E = cached rows per chunk (8 at head_dim 80, else attn_chunk_rows).  Lengths: every T in 1 .. 4 E + 1 (every phase of the appended
   row in both buffers, both parities of the chunk count), 8 E - 1 / 8 E / 8 E + 1, 255 / 256 / 257 / 258; A80R: E + 3, 4 E + 1, 257, 258.
   One-hot: the output is the winner's V row bit for bit, every cached position the winner of at least one pair (two launches at 258),
   rows at and past T - 1 hold 3e30 before the launch; the appended V row bit for bit, the appended k-normed row within prologue_tol; no
   other cache row and no work buffer other than y / yq changes.  Dense at E + 3, 4 E + 1, 97, 257, 258: the derived distance per output
   (attn_dense_bound) and 4 x an fp32 numpy evaluation per launch.  Two equal winners (first and last cached row of 257): their mean.
   The caches live on the device: a length clones the engine's base cache there, poisons the rows from T - 1 on and scatters the
   winners' rows; only q-sized arrays cross the bus.

tests/test_rar_kernel_reference.py plants the faults these checks exist for (a k_bx that stops behind step 4 at PER 8, slab 6 of 8, the
third QKV piece, buffer B's refill, the last chunk of an odd count, a stale appended row at phase 2..5, the wrong tail quad) on the CPU.

Measured on an MI355X (290 cases, 25 s for the whole file, none skipped; tests/test_gpu_rar_kernels.py: 365 cases, 35 s at its merge).
  plans: all 19 (engine, rows) equal to expected_plan and to the hand-written table, plain and shared_u, fallbacks 0.
  exact: integer QKV / PROJ / FC2 / HEAD / adaLN pieces 0 differing floats in all 19 cases (k_bx<2,8,4> at 6 and 8 slabs, <2,16,4>,
      <2,20,4>, 3 / 4 QKV slabs), pieces past the plan untouched; integer gated fold at S = 1, 3, 4, 5, 6, 8: 0 differing bits, sums
      bit-exact; stage walk (19) and shared_u walk (5): 0 differing bits in logits, x, h, caches; 0 bytes changed in buffers a launch
      does not own.
  gated: dense pieces 0.23 .. 0.37 / 0.22 .. 0.55 / 0.29 .. 0.54, adaLN GEMM 0.27 .. 0.40, head 0.30 .. 0.49 x the fp32 chain (gate 2);
      GELU 0.25 of its distance on exact pre-activations, 0.12 .. 0.18 on dense ones; dense fold <= 0.98, dense sums <= 1.0e-15 of their
      scale; k_resid_mod h 0.81 .. 0.99 and k_modulate 0.78 .. 0.96 of the per-element distance (fp32 numpy the same); embedding
      statistics <= 1.9e-15, SiLU 0.15 .. 0.36 of its distance (fp32 numpy 0.25 .. 0.50); attention at 128 rows: dense <= 0.005 of the
      derived distance, 1.02 .. 1.31 x the fp32 evaluation (gate 4); appended k rows 1.00 .. 1.09 x the fp32 algebra (gate 2), 0.30 / 0.60 / 0.11
      of prologue_tol on RB / RL / RXXL.
  composition, positions 0..5 at 128 rows, logits up to 5.8 .. 6.9 in magnitude: largest logit error of the engine / of the oracle's
      fp32 evaluation against position64 -- RB 2.94e-06 / 3.05e-06 (0.96 x), RL 3.27e-06 / 3.25e-06 (1.01 x), RXXL 4.60e-06 / 3.03e-06
      (1.52 x); gate 4 x.
  full-length caches: 61 440 + 2 048 (row, head) pairs over 72 / 40 / 40 / 40 / 24 / 24 / 4 lengths (A32 .. A128, A80R), every phase
      of a chunk: 0 differing bits, 0 cache floats outside the appended rows changed, 0 bytes of other buffers changed; appended V rows
      bit-exact, appended k rows 0.05 .. 0.09 of prologue_tol; dense at 5 lengths per engine <= 0.0056 of the derived distance, 0.75 ..
      1.19 x the fp32 evaluation (gate 4; per launch 1.3e-07 .. 7.0e-07 against 2.4e-07 .. 8.6e-07); two equal winners: the mean,
      0 differing bits.
  FOUND AND FIXED: RL at 128 rows feeds the head_dim-64 prologue FOUR QKV pieces, and with a plain fp32 piece sum its worst appended
      k-normed element was 1.08 x prologue_tol at 1 cached row and 1.06 x at 7 (RB, three pieces: 0.64; one piece: 0.05 .. 0.11; an
      fp32 numpy evaluation in the same order missed by the same 1.08 x / 1.07 x).  Where an element cancels in the piece sum
      (sum |pieces| 1.12 against v = -0.0018) the roundings of the partial sums survive and the per-head norm scales them by rstd.
      The prologue of k_attn_decode<.., MODE 1> now carries the rounding errors of the q and k piece additions along
      (two_sum / csum4_add in decoder_kernels.h; same order, v and MODE 0 untouched, one piece gives the bits it gave);
      rar_kernel_reference.piece_sum32c states it.  Figures behind the fix: DESIGN.md section 4 (ATTN_AFTER_FIX).  k_attn_decode80 keeps the plain sum: RAR-XL tokens are
      pinned one by one against the oracle, and a change of rounding there flipped one near-tie."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rar_kernel_reference as R  # noqa: E402
from tests import test_gpu_rar_kernels as K  # noqa: E402

SENT, GARBAGE, V, NCLS = K.SENT, K.GARBAGE, K.V, K.NCLS
TORCH_FACTOR = 4.0
_say = K._say
_T0 = [None]

WIDTHS = ("RB", "RL", "RXXL")
ROWS = (20, 64, 97, 127, 128)            # 20 = the reference's 10 x 2
CASES = [(n, M) for n in WIDTHS for M in ROWS] + [(n, M) for n in ("P16", "P20") for M in (97, 128)]


@pytest.fixture(scope="module", autouse=True)
def engines():
    _T0[0] = time.time()
    _LONG.clear()
    yield K._ENGINES
    _LONG.clear()
    K._ENGINES.close_all()
    torch.cuda.empty_cache()
    print("RARK released file                                seconds=%.1f" % (time.time() - _T0[0]))


# ------------------------------------------------------------------------------------------------ 1. released widths: the stage file's bodies
@pytest.mark.parametrize("name,M", CASES, ids=str)
def test_released_plan_is_the_pinned_one(name, M):
    """the probe plan against expected_plan and the hand-written table (K.Probe.plan asserts both), plain and under guidance"""
    pr = K._probe(name, "dense")
    assert (name, M) in K.HEADLINE
    plan = pr.plan(M)
    if M % 2 == 0:
        pr.plan(M, M // 2, 1)
    _say("plan %s M=%d" % (name, M), bx=plan["bx"], S="%d/%d/%d" % (plan["S_qkv"], plan["S_proj"], plan["S_fc2"]),
         PER="%d/%d/%d" % (plan["PER_qkv"], plan["PER_proj"], plan["PER_fc2"]), nch=plan["nch"], nrm=plan["nrm"], fc2=plan["roles"]["fc2"],
         fc1=plan["roles"]["fc1"], resid_mlp=plan["roles"]["resid_mlp"], attn=plan["roles"]["attn"])


@pytest.mark.parametrize("name,M", CASES, ids=str)
def test_released_gemm_stages_on_integer_operands(name, M):
    K.test_gemm_stages_on_integer_operands(name, (), M, 0)


@pytest.mark.parametrize("name,M", CASES, ids=str)
def test_released_gemm_pieces_and_head_dense(name, M):
    K.test_gemm_pieces_and_head_dense(name, (), M)


@pytest.mark.parametrize("name,M", CASES, ids=str)
@pytest.mark.parametrize("stage", [R.RESID_ATTN, R.RESID_MLP], ids=["RESID_ATTN", "RESID_MLP"])
@pytest.mark.parametrize("integer", [True, False], ids=["int", "dense"])
def test_released_resid_mod_against_float64(name, M, stage, integer):
    K.test_resid_mod_against_float64(name, M, 0, stage, integer)


@pytest.mark.parametrize("name", WIDTHS)
@pytest.mark.parametrize("stage", [R.RESID_ATTN, R.RESID_MLP], ids=["RESID_ATTN", "RESID_MLP"])
def test_released_resid_mod_shared_u(name, stage):
    K.test_resid_mod_against_float64(name, 128, 64, stage, False)


@pytest.mark.parametrize("name,M,Bhalf", [(n, M, 0) for n, M in CASES] + [(n, 128, 64) for n in WIDTHS], ids=str)
def test_released_modulate_against_float64(name, M, Bhalf):
    K.test_modulate_against_float64(name, M, Bhalf)


@pytest.mark.parametrize("name,M,Bhalf", [(n, M, B) for n in WIDTHS for M, B in ((20, 0), (128, 0), (128, 64))], ids=str)
@pytest.mark.parametrize("p", [0, 1, 2, 9])
@pytest.mark.parametrize("kind", ["int", "dense"])
def test_released_embedding_both_forms(name, M, Bhalf, p, kind):
    K.test_embedding_both_forms(name, M, Bhalf, p, kind)


@pytest.mark.parametrize("name", WIDTHS)
@pytest.mark.parametrize("mode", ["onehot", "dense"])
def test_released_attention_mode1(name, mode):
    """RB / RL: S = 3 / 4 packed pieces (S < RPI at head_dim 48), yq planes out, y untouched; RXXL: one piece, head_dim 88.
    RL (four pieces) is the case that found the plain fp32 piece sum of q and k outside prologue_tol (1.08 x); the prologue now
    carries the additions' rounding errors along (module docstring)."""
    K.test_attention_mode1(name, 128, mode)


@pytest.mark.parametrize("name", WIDTHS)
def test_released_appended_rows(name):
    K.test_appended_rows_within_twice_the_fp32_algebra(name, 128)


@pytest.mark.parametrize("name,M", CASES, ids=str)
def test_released_stage_walk_equals_forward_position(name, M):
    K.test_stage_walk_equals_forward_position(name, (), M)


@pytest.mark.parametrize("name,Bhalf", [("RB", 64), ("RB", 49), ("RL", 64), ("RL", 49), ("RXXL", 64)], ids=str)
def test_released_shared_u_walk_equals_plain_walk(name, Bhalf):
    K.test_shared_u_walk_equals_plain_walk(name, Bhalf)


@pytest.mark.parametrize("name", WIDTHS)
def test_released_composition_against_float64(name):
    """positions 0..5 at 128 rows: the engine's largest logit error against position64 within TORCH_FACTOR x that of the oracle's fp32
    evaluation of the same positions (each evaluation keeps its own caches, as it would in a run)"""
    from oracle.rar_oracle import rar_position
    from wmar_amd.utils.synth import RARConfig
    pr = K._probe(name, "dense")
    M = 128
    pr.plan(M)
    cfg = RARConfig(hidden_size=pr.D, num_hidden_layers=pr.nl, num_attention_heads=pr.H, intermediate_size=pr.F, image_seq_len=pr.SEQ,
                    codebook_size=V, condition_num_classes=NCLS)
    sd32 = {k: torch.from_numpy(v) for k, v in pr.sd.items()}
    rs = np.random.RandomState(pr.D)
    cond = K._conds(rs, M)
    for l in range(pr.nl):
        pr.fill("kcache", GARBAGE, l); pr.fill("vcache", GARBAGE, l)
    kc32 = vc32 = kcn = vcn = None
    e_eng, e_orc, per_pos = 0.0, 0.0, []
    for p in range(6):
        tk = np.full(M, -1) if p == 0 else (cond if p == 1 else rs.randint(0, V, size=M))
        lg = pr.forward_position(tk, cond, p)
        te = sd32["cls_token"][0, 0].expand(M, -1) if p == 0 else sd32["embeddings.weight"][torch.from_numpy(np.asarray(tk))]
        ce = sd32["embeddings.weight"][torch.from_numpy(cond)]
        with torch.no_grad():
            l32, kc32, vc32 = rar_position(sd32, cfg, te, ce, p, kc32, vc32)
        ref, kcn, vcn = R.position64(pr.sd, cfg, tk, cond, p, kcn, vcn)
        a, b = float(np.abs(lg.astype(np.float64) - ref).max()), float(np.abs(l32.numpy().astype(np.float64) - ref).max())
        per_pos.append("%.2g/%.2g" % (a, b))
        e_eng, e_orc = max(e_eng, a), max(e_orc, b)
        assert np.isfinite(lg).all()
    _say("composition %s M=%d" % (name, M), engine=e_eng, oracle_fp32=e_orc, ratio=e_eng / e_orc, gate=TORCH_FACTOR, logit_scale=float(np.abs(ref).max()),
         per_position=",".join(per_pos))
    assert e_eng <= TORCH_FACTOR * e_orc, "largest logit error %.3g against the float64 composition; the oracle's fp32 evaluation: %.3g (gate %g x)" % (
        e_eng, e_orc, TORCH_FACTOR)


# ------------------------------------------------------------------------------------------------ 2. full-length caches, attention alone
LONG = ["A32", "A48", "A64", "A80", "A88", "A128", "A80R"]
_LONG = {}


def _rows_per_chunk(hd):
    return 8 if hd == 80 else R.attn_chunk_rows(hd)


def _sweep_lengths(name, E, T):
    if name == "A80R":
        return [E + 3, 4 * E + 1, 257, 258]
    return sorted(set(range(1, 4 * E + 2)) | {8 * E - 1, 8 * E, 8 * E + 1, 255, 256, 257, 258})


def _dense_lengths(E):
    return [E + 3, 4 * E + 1, 97, 257, 258]


class Long:
    """One 258-position engine set up for ATTN launches: the QKV pieces (the same for every length: q, and the rows the launch appends,
    are a function of them alone) and every work buffer are loaded once; the base caches stay on the device."""

    def __init__(self, name):
        pr = self.pr = K._probe(name, "dense")
        self.M = M = pr.Mmax
        self.plan = plan = pr.plan(M)
        H, hd, D, MT = pr.H, pr.hd, pr.D, plan["MT"]
        assert pr.T == 258 and plan["attn_waves"] == 1
        assert ("k_attn_decode80<1>" if hd == 80 else "k_attn_decode<%d,1,1>" % hd) in plan["roles"]["attn"]
        assert plan["rowmajor"] == (1 if name == "A80R" else 0) and plan["bx"] == plan["rowmajor"]
        self.E = _rows_per_chunk(hd)
        self.scale = 1.0 / np.sqrt(hd)
        rs = np.random.RandomState(hd + M)
        S = plan["S_qkv"]
        P = (rs.standard_normal((S, 32 * MT, 3 * D)) * (0.7 / np.sqrt(S))).astype(np.float32)
        self.pro = R.attn_prologue(P[:, :M], pr.w("attn.qkv.bias", 0), pr.w("attn.q_norm.weight", 0), pr.w("attn.q_norm.bias", 0),
                                   pr.w("attn.k_norm.weight", 0), pr.w("attn.k_norm.bias", 0), H, hd)
        q32 = self.pro[1][0]
        pr.sentinel_work()
        buf = np.full(pr.size("qkv_slabs") // 4, SENT, dtype=np.float32)
        pr.put("qkv_slabs", R.put_pieces(buf, P, MT, bool(plan["rowmajor"])))
        self.ybuf = "yq" if plan["bx"] else "y"
        self.snap = pr.snapshot()
        self.shape = (pr.Mmax, H, pr.T, hd)
        self.k_host = rs.standard_normal(self.shape).astype(np.float32)
        self.v_host = rs.standard_normal(self.shape).astype(np.float32)
        self.k_dev, self.v_dev = torch.from_numpy(self.k_host).cuda(), torch.from_numpy(self.v_host).cuda()
        self.ks_dev = self.k_dev * 0.01                            # the one-hot sweep's losers
        # the winner's row: aligned with q, 400 ahead of every other score (|q . knew| / sqrt(hd) <= sqrt(hd) (1 + ..) stays below 20)
        n2 = np.maximum((q32.astype(np.float64) ** 2).sum(-1, keepdims=True), 1e-12)
        self.win_dev = torch.from_numpy((q32 * (400.0 / self.scale) / n2).astype(np.float32)).cuda()
        self.mi = torch.arange(M, device="cuda")[:, None].expand(M, H)
        self.hi = torch.arange(H, device="cuda")[None, :].expand(M, H)
        self.cache_floats_changed = 0

    def caches(self, Tn, onehot, winners=()):
        """the base caches with 3e30 from row Tn - 1 on; one-hot: losers scaled down, the winners' rows scattered in"""
        kc, vc = (self.ks_dev if onehot else self.k_dev).clone(), self.v_dev.clone()
        for w in winners:
            kc[self.mi, self.hi, w] = self.win_dev
        kc[:, :, Tn - 1:] = GARBAGE
        vc[:, :, Tn - 1:] = GARBAGE
        return kc, vc

    def launch(self, Tn, kc, vc):
        """one ATTN launch at Tn cached rows (the new one included): asserts what must not change, returns (y [M, H, hd], the
        appended k row, the appended v row) on the host"""
        pr, M, plan = self.pr, self.M, self.plan
        pr.put("kcache", kc); pr.put("vcache", vc)
        pr.fill(self.ybuf, 0x7f7f if plan["bx"] else SENT)
        pr.run(R.ATTN, R.ATTN, M, pos=Tn - 1, layer=0)
        pr.assert_unowned_unchanged(self.snap, {self.ybuf})
        out = []
        for nme, before in (("kcache", kc), ("vcache", vc)):
            after = pr.get_dev(nme).view(self.shape)
            out.append(after[:M, :, Tn - 1].cpu().numpy())
            rest = after.clone()
            rest[:M, :, Tn - 1] = before[:M, :, Tn - 1]
            changed = int((rest.view(torch.int32) != before.view(torch.int32)).sum())
            self.cache_floats_changed += changed
            assert changed == 0, "%s at %d rows: %d floats outside the appended rows changed" % (nme, Tn, changed)
        if plan["bx"]:
            y = R.check_planes_consistent(pr.get("yq")[:pr.D // 16 * plan["MT"] * 3 * 64 * 8], plan["MT"], pr.D, M, "yq planes")
            assert torch.equal(pr.get_dev("y"), self.snap["y"]), "y written on the bx plan"
        else:
            y = pr.get_act("y", plan["MT"], pr.D)
        return y[:M].reshape(M, pr.H, pr.hd), out[0], out[1]

    def check_appended(self, Tn, kg, vg, late):
        """the appended V row bit for bit; the k-normed row per element as a multiple of prologue_tol (a miss goes to `late`, which the
        caller asserts empty behind its loop, so that every length is still run)"""
        (q64, k64, v64), (q32, k32, v32), (nq, nk, nv) = self.pro
        kerr = np.abs(kg.astype(np.float64) - k64) / R.prologue_tol(nk, self.pr.hd)
        if not np.all(kerr <= 1.0):
            late.append("%d rows: worst element %.3g x the derived distance" % (Tn, float(kerr.max())))
        R.check_exact(vg, v32, "appended V row at %d rows" % Tn)
        return float(kerr.max())


def _long(name):
    if name not in _LONG:
        _LONG[name] = Long(name)
    return _LONG[name]


@pytest.mark.parametrize("name", LONG)
def test_full_length_one_hot_sweep(name):
    """every length of the sweep; pair j of a launch attends to cached position (j + offset) mod (T - 1), so that every cached position
    of the length is the winner of at least one (row, head) pair -- two launches where there are more positions than pairs"""
    lc = _long(name)
    pr, M, H = lc.pr, lc.M, lc.pr.H
    t0, pairs, launches, worst, late = time.time(), 0, 0, 0.0, []
    lengths = _sweep_lengths(name, lc.E, pr.T)
    phases = set()
    pair = torch.arange(M * H, device="cuda").view(M, H)
    for Tn in lengths:
        phases.add((Tn - 1) % lc.E)
        npos = Tn - 1
        if npos == 0:
            y, kg, vg = lc.launch(Tn, *lc.caches(Tn, True))
            worst = max(worst, lc.check_appended(Tn, kg, vg, late))
            R.check_onehot(y, vg, "new-token attention")
            launches += 1
            continue
        seen = np.zeros(npos, dtype=bool)
        for first in range(0, npos, M * H):
            win = (pair + (first + 7 * Tn)) % npos
            seen[win.cpu().numpy().reshape(-1)] = True
            kc, vc = lc.caches(Tn, True, [win])
            y, kg, vg = lc.launch(Tn, kc, vc)
            worst = max(worst, lc.check_appended(Tn, kg, vg, late))
            R.check_onehot(y, lc.v_dev[lc.mi, lc.hi, win].cpu().numpy(), "one-hot attention at %d rows" % Tn)
            pairs += M * H
            launches += 1
        assert seen.all(), "%d cached positions of length %d were never a winner" % (int((~seen).sum()), Tn)
    assert name == "A80R" or phases == set(range(lc.E)), "the appended row did not land on every phase of a chunk"
    _say("long one-hot %s M=%d" % (name, M), kernel=lc.plan["roles"]["attn"], E=lc.E, lengths=len(lengths), launches=launches, pairs=pairs, differing_bits=0,
         appended_of_distance=worst, cache_floats_changed=lc.cache_floats_changed, seconds=time.time() - t0)
    assert not late, "appended K row at " + "; ".join(late)


@pytest.mark.parametrize("name", LONG)
def test_full_length_dense(name):
    """dense caches at E + 3, 4 E + 1, 97, 257, 258 rows: the derived distance per output, 4 x an fp32 numpy evaluation per launch"""
    lc = _long(name)
    pr, M, hd = lc.pr, lc.M, lc.pr.hd
    (q64, k64, v64), (q32, k32, v32), (nq, nk, nv) = lc.pro
    t0, figs, late = time.time(), dict(dist=0.0, fp32=0.0, kdist=0.0), []
    for Tn in _dense_lengths(lc.E):
        y, kg, vg = lc.launch(Tn, *lc.caches(Tn, False))
        figs["kdist"] = max(figs["kdist"], lc.check_appended(Tn, kg, vg, late))
        # the cache's new row is what the kernel itself wrote (held above); q is held through the bound's dq
        K64 = np.concatenate([lc.k_host[:M, :, :Tn - 1].astype(np.float64), kg[:, :, None].astype(np.float64)], 2)
        V64 = np.concatenate([lc.v_host[:M, :, :Tn - 1].astype(np.float64), vg[:, :, None].astype(np.float64)], 2)
        ref, tol = R.attn_dense_bound(q64, R.prologue_tol(nq, hd), K64, np.zeros_like(q64), V64, np.zeros_like(q64), lc.scale, lc.E, 1)
        figs["dist"] = max(figs["dist"], R.check_attn_dense(y, ref, tol))
        y32 = R.attn_fp32(q32, K64, V64, lc.scale)
        e, e32 = float(np.abs(y - ref).max()), float(np.abs(y32 - ref).max())
        print("RARK   dense %s T=%d: launch maximum %.3g, fp32 evaluation %.3g" % (name, Tn, e, e32))
        assert e <= 4.0 * e32, "attention at %d rows: largest error %.3g against the fp32 evaluation's %.3g (gate 4 x)" % (Tn, e, e32)
        if e32 > 0:
            figs["fp32"] = max(figs["fp32"], e / e32)
    _say("long dense %s M=%d" % (name, M), kernel=lc.plan["roles"]["attn"], lengths=len(_dense_lengths(lc.E)), of_distance=figs["dist"], x_fp32=figs["fp32"],
         appended_of_distance=figs["kdist"], cache_floats_changed=lc.cache_floats_changed, seconds=time.time() - t0)
    assert not late, "appended K row at " + "; ".join(late)


@pytest.mark.parametrize("name", LONG)
def test_full_length_two_equal_winners(name):
    """the first and the last cached row of 257 hold the same winning K row (chunk 0 of buffer A and the last full chunk): the output
    is the mean of their V rows -- one fp32 addition and an exact halving, whatever the order"""
    lc = _long(name)
    M, H = lc.M, lc.pr.H
    Tn = 257
    first, last = torch.zeros(M, H, dtype=torch.long, device="cuda"), torch.full((M, H), Tn - 2, dtype=torch.long, device="cuda")
    kc, vc = lc.caches(Tn, True, [first, last])
    y, kg, vg = lc.launch(Tn, kc, vc)
    late = []
    lc.check_appended(Tn, kg, vg, late)
    want = ((lc.v_dev[:M, :, 0] + lc.v_dev[:M, :, Tn - 2]) * 0.5).cpu().numpy()
    R.check_onehot(y, want, "two winners")
    _say("long two winners %s M=%d" % (name, M), rows=Tn, differing_bits=0, cache_floats_changed=lc.cache_floats_changed)
    assert not late, "appended K row at " + "; ".join(late)
