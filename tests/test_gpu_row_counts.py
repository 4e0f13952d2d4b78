"""Decode parity at the row counts BETWEEN the pinned ends, production width, deep caches.

The decode engines choose another set of kernels for almost every range of row counts.  test_gpu_small_batch.py pins 1..12 rows and
test_gpu_prod_shapes.py pins 64 (and 33 at two positions); this file walks the ranges in between on the same 2-layer engines and the
same fixture (tests/golden/prod_vectors.npz: 64 independent rows of the reference's own run, so rows [:B] are the reference's answer
for batch B and a batch above 64 is those rows repeated).

Taming GPT (wmar_amd/csrc/gpt.hip StepPlan; mt_for() in decoder_host.h), n_embd 1536, 24 heads, max_batch 128, as plan_info reports:

  rows B    what runs
  13..21    one 32-row MFMA tile: k_qkvx<1,..>, k_gemm proj / FC1 / FC2; B * H < 512, so att_phase() picks 2 attention waves up to
            128 cached rows and 4 beyond
  22..32    the same tile, one attention wave at every cache length
  33..64    two tiles on the bf16 pipe: k_qkvx_bx, k_bx_xr (k_bx<1,..> where the XCD grouping probe fails), k_fc1x; padded rows
            33..63 inside every tile
  65..128   MT = 4: S_qx = 0, so k_resid_stats + k_gemm<EPI_PACKED> QKV, head in 128-row launches

RAR (wmar_amd/csrc/rar.hip RarPlan), hidden 1280, M = 2B rows under guidance: tiles change at B = 16 / 32, the bf16 pipe starts at
M > 64, the adaLN GEMM of a guided run works on mt_for(B) tiles and the conditional / unconditional split falls inside a row tile
whenever B is not a multiple of 32.

References:
  * the reference fixture at its 12 positions / 23 steps, gate ATOL = 5e-4 (the project's gate at this width and depth);
  * for Taming a FULL comparison: one float64 pass of oracle.model_oracle.gpt_prefix over the 64 fixture rows, every logit of every
    row at every position under the same 5e-4 (compared on the device against a float32 copy: its rounding, 2e-6 at |logit| 30, is
    far below the gate);
  * an arg-max may differ from the reference's only at the REFERENCE's own near ties: the (row, position) pairs whose top-two gap
    in the float64 oracle logits is below 2 * ATOL.  The set is computed from the oracle (never from the engine's logits), must
    have at most 8 members, and a flip there must land on the oracle's top or runner-up token;
  * sampling loops against model_oracle.sample_with_past / rar_oracle.generate on the same noise, compared with
    test_gpu_depth._compare_tokens: a row may leave the oracle's path only at a race closer than 4 * ATOL (16 * ATOL for the guided
    mix, which multiplies logit differences by up to 7), at most one such row per run."""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model_oracle as M  # noqa: E402
from oracle import rar_oracle as R  # noqa: E402
from oracle import wm_oracle as W  # noqa: E402
from tests.conftest import REPO  # noqa: E402
from tests.test_gpu_depth import _compare_tokens  # noqa: E402
from tests.test_gpu_prod_shapes import ATOL, GCFG, RCFG  # noqa: E402
from tests.test_gpu_watermark import _wm  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402

GPT_ROWS = [13, 16, 20, 21, 22, 31, 32, 33, 34, 47, 48, 63, 64, 65, 96, 127, 128]
RAR_ROWS = [5, 10, 16, 17, 20, 32, 33, 40, 63]
T_ALL = 256


@pytest.fixture(scope="module")
def pv():
    return np.load(os.path.join(REPO, "tests", "golden", "prod_vectors.npz"))


# ------------------------------------------------------------------------------------------------------------------ Taming

@pytest.fixture(scope="module")
def gsd():
    return synth.synth_gpt_state(GCFG, seed=9, logit_scale=10.0)


@pytest.fixture(scope="module")
def gpt(gsd):
    from wmar_amd.models.engine import GPTEngine
    return GPTEngine(GCFG, gsd, max_batch=128)


class _Oracle:
    """float64 logits of the 64 fixture rows at all 256 positions (float32 copy on the device, [T, 64, V]), the oracle's top and
    runner-up token per (row, position) and the near-tie set."""


def gpt_oracle(pv, gsd):
    """(host part of the `orc` fixture: runs without a GPU)"""
    sd64 = {k: v.double() for k, v in gsd.items() if v.is_floating_point()}
    seq = torch.from_numpy(pv["gpt_seq"].astype(np.int64))
    ref = torch.empty(T_ALL, 64, GCFG.vocab_size, dtype=torch.float32)
    top = np.zeros((64, T_ALL), np.int64)
    second = np.zeros((64, T_ALL), np.int64)
    gap = np.zeros((64, T_ALL), np.float64)
    t0 = time.perf_counter()
    for r0 in range(0, 64, 8):          # 8 rows per pass: 270 MB of float64 logits at a time
        lg = M.gpt_prefix(sd64, GCFG.n_head, seq[r0:r0 + 8])               # [8, T, V] float64
        v, i = lg.topk(2, dim=-1)
        top[r0:r0 + 8], second[r0:r0 + 8] = i[..., 0].numpy(), i[..., 1].numpy()
        gap[r0:r0 + 8] = (v[..., 0] - v[..., 1]).numpy()
        ref[:, r0:r0 + 8] = lg.transpose(0, 1).float()
    t_cpu = time.perf_counter() - t0
    o = _Oracle()
    o.top, o.second, o.near = top, second, gap < 2 * ATOL
    pairs = [(int(r), int(t)) for r, t in zip(*np.nonzero(o.near))]
    assert len(pairs) <= 8, pairs       # a changed fixture cannot quietly widen the exception
    # the oracle against the reference's own numbers: logits at the fixture positions, the arg-max everywhere but at a near tie
    d = max(float(np.abs(ref[int(p)][:, ::64].numpy() - pv["gpt_logits"][i]).max()) for i, p in enumerate(pv["gpt_pos"]))
    assert d < ATOL, d
    ref_am = pv["gpt_argmax"].astype(np.int64).T                           # [64, T]
    off = ref_am != top
    assert not (off & ~o.near).any() and (ref_am[off] == second[off]).all()
    o.ref, o.ref_am, o.seq = ref, ref_am, seq
    print(f"float64 oracle prefix pass over 64 rows x {T_ALL} positions: {t_cpu:.1f} s; against the fixture {d:.2e}; "
          f"near ties (gap < {2 * ATOL:g}): {pairs}, minimum gap {gap.min():.2e}")
    return o


@pytest.fixture(scope="module")
def orc(pv, gsd):
    o = gpt_oracle(pv, gsd)
    o.ref, o.seq = o.ref.cuda(), o.seq.cuda()
    o.fix = torch.from_numpy(pv["gpt_logits"].astype(np.float32)).cuda()   # [12, 64, 256]
    o.fix_pos = {int(p): i for i, p in enumerate(pv["gpt_pos"])}
    return o


def _check_plan(gpt, B):
    """plan_info names the plan of the table in the module docstring"""
    info = gpt.plan_info(B)
    print(f"{B} rows: qkv={info['qkv']}; attn={info['attn']}; proj={info['proj']}; fc1={info['fc1']}; fc2={info['fc2']}")
    assert not any("k_sgemv" in v for v in info.values()), info
    if B <= 32:
        assert "k_qkvx<1" in info["qkv"], info
        assert "k_gemm<EPI_PACKED>" in info["proj"] and "k_gemm<EPI_GELU,LN>" in info["fc1"], info
    elif B <= 64:
        assert "k_qkvx_bx" in info["qkv"] and "bf16 pipe" in info["qkv"], info
        assert ("k_bx_xr" in info["proj"] or "k_bx<" in info["proj"]) and "bf16 pipe" in info["proj"], info
        assert "k_fc1x" in info["fc1"], info
    else:
        assert "k_gemm<EPI_PACKED>" in info["qkv"] and "k_resid_stats" in info["qkv"], info
        assert "k_gemm<EPI_PACKED>" in info["proj"] and "k_gemm<EPI_GELU,LN>" in info["fc1"], info
    if B <= 21:
        assert info["attn"].startswith("k_attn_decode<64,2>") and "2 / 2 / 4 waves at 1 / 128 / 256 cached rows" in info["attn"], info
    else:
        assert info["attn"] == "k_attn_decode<64,1>", info


def _teacher_forced(gpt, orc, rows, T, full_at=None):
    """Engine row j = fixture row rows[j], teacher-forced over positions 0..T-1.  Every logit against the float64 oracle at the
    positions `full_at` (None: all), every 64th against the reference fixture at its own positions, the arg-max of every row at every
    position.  The maxima stay on the device until the pass is over (one copy, not one per step)."""
    rows = np.asarray(rows, np.int64)
    B = len(rows)
    ridx = torch.from_numpy(rows).cuda()
    seq = orc.seq.index_select(0, ridx)
    d_full = torch.zeros(T, device="cuda")
    d_fix = torch.zeros(T, device="cuda")
    am = torch.empty(T, B, dtype=torch.int64, device="cuda")
    for t in range(T):
        lg = gpt.decode_step(seq[:, t], t)
        am[t] = lg.argmax(-1)
        if full_at is None or t in full_at:
            d_full[t] = (lg - orc.ref[t].index_select(0, ridx)).abs().max()
        if t in orc.fix_pos:
            d_fix[t] = (lg[:, ::64] - orc.fix[orc.fix_pos[t]].index_select(0, ridx)).abs().max()
    d_full, d_fix, am = d_full.cpu().numpy(), d_fix.cpu().numpy(), am.cpu().numpy().T          # am [B, T]
    print(f"{B} rows, {T} positions: max |dlogit| {d_full.max():.2e} over all {GCFG.vocab_size} logits vs the float64 oracle, "
          f"{d_fix.max():.2e} vs the reference fixture", end="")
    bad = ~(d_full < ATOL)          # (a NaN fails)
    assert not bad.any(), (B, "oracle", [(int(t), float(d_full[t])) for t in np.nonzero(bad)[0][:8]])
    bad = ~(d_fix < ATOL)
    assert not bad.any(), (B, "fixture", [(int(t), float(d_fix[t])) for t in np.nonzero(bad)[0][:8]])
    want = orc.ref_am[rows, :T]
    flips = set()
    for j, t in zip(*np.nonzero(am != want)):
        r = int(rows[j])
        assert orc.near[r, t], f"{B} rows: arg-max of row {j} (fixture row {r}) at position {t} is {am[j, t]}, the reference's {want[j, t]}"
        assert am[j, t] in (orc.top[r, t], orc.second[r, t]), (B, j, r, t)
        flips.add((r, int(t)))
    print(f"; arg-max near-tie flips: {sorted(flips)}")


@pytest.mark.parametrize("B", GPT_ROWS)
def test_gpt_1536_rows_teacher_forced_256_positions(gpt, orc, B):
    """every logit of every row at all 256 positions within 5e-4 of the float64 oracle, every 64th logit at the fixture's 12 positions
    within 5e-4 of the reference's, the arg-max of every row at every position the reference's (near ties of the reference excepted)"""
    _check_plan(gpt, B)
    _teacher_forced(gpt, orc, np.arange(B) % 64, T_ALL)


def test_gpt_1536_one_engine_changing_row_counts(gpt, orc):
    """128 -> 13 -> 64 -> 33 -> 21 -> 65 rows on one engine, positions 0..139 each (across the 128-row attention switch).  Consecutive
    runs hold DIFFERENT fixture rows in every row slot (rolled by 7 on every other run), so whatever a larger batch leaves behind in
    padded rows, caches, statistics or slabs is wrong data for the next one."""
    for k, B in enumerate((128, 13, 64, 33, 21, 65)):
        rows = (np.arange(B) + 7 * (k % 2)) % 64
        _teacher_forced(gpt, orc, rows, 140, full_at=(0, 127, 128, 139))


def _loop_inputs(B, steps, seed, device):
    cond = torch.tensor([(i * 37 + 3) % 1000 for i in range(B)])
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.empty(steps, B, GCFG.vocab_size, device=device).exponential_(1, generator=g)
    return cond, q


def test_gpt_1536_generate_20_64_20_rows_bit_equal(gpt, kat):
    """generate() with 20, then 64, then 20 rows again on one engine (captured graphs; 160 steps: the 20-row attention schedule and
    with it the captured graph changes at 128 cached rows): the two 20-row runs equal bit for bit, and equal to an eager 20-row run
    (the same kernels)."""
    wm = _wm(kat["keys"]["taming"])
    steps = 160
    cond, q = _loop_inputs(64, steps, 2064, "cuda")
    q20 = q[:, :20].contiguous()

    def run(c, qq, graph):
        return gpt.generate(c.cuda(), steps, qq, 1.0, 250, 0.92, wm.wm_ctx(), use_graph=graph).clone()

    a = run(cond[:20], q20, True)
    run(cond.roll(7), q, True)          # other conditioning tokens in every row slot
    b = run(cond[:20], q20, True)
    c = run(cond[:20], q20, False)
    assert torch.equal(a, b), f"rows that differ after the 64-row run: {np.nonzero((a != b).any(1).cpu().numpy())[0]}"
    assert torch.equal(a, c), f"graph / eager rows that differ: {np.nonzero((a != c).any(1).cpu().numpy())[0]}"


@pytest.mark.parametrize("B,steps", [(13, 160), (21, 160), (33, 64), (48, 64), (96, 64)])
def test_gpt_1536_watermarked_loop_vs_oracle(gpt, gsd, kat, key_factory, B, steps):
    """greenlist delta 2, top-k 250, top-p 0.92, graph and eager, token for token against model_oracle.sample_with_past on the same noise;
    the detector's p-values of the engine's tokens equal the oracle detector's on the same tokens"""
    wm = _wm(kat["keys"]["taming"])
    key = key_factory(kat["keys"]["taming"])
    cond, q = _loop_inputs(B, steps, 3000 + B, "cpu")
    rec = []
    t0 = time.perf_counter()
    ref = M.sample_with_past(gsd, GCFG.n_head, cond.view(-1, 1), steps, 1.0, 250, 0.92, key, 2.0,
                             q_source=lambda n, b, v: q[n], record=rec, static_cache=True).numpy()
    t_cpu = time.perf_counter() - t0
    qd = q.cuda()
    for graph in (True, False):
        toks = gpt.generate(cond.cuda(), steps, qd, 1.0, 250, 0.92, wm.wm_ctx(), use_graph=graph)
        got = toks.cpu().numpy()
        near = _compare_tokens(got, ref, rec, 4 * ATOL)
        print(f"{B} rows, {'graph' if graph else 'eager'}: {int((got == ref).all(1).sum())} of {B} rows equal over {steps} steps, "
              f"{near} near-tie divergences; oracle loop {t_cpu:.1f} s")
        assert near <= 1, near
        p = wm.detect(toks).cpu().numpy()
        rp, _, _ = W.detect(key, got)
        assert np.allclose(p, rp, rtol=1e-9, atol=0, equal_nan=True)


# --------------------------------------------------------------------------------------------------------------------- RAR

@pytest.fixture(scope="module")
def rsd():
    return synth.synth_rar_state(RCFG, seed=12, logit_scale=8.0)


@pytest.fixture(scope="module")
def rar(rsd):
    from wmar_amd.models.engine import RAREngine
    return RAREngine(RCFG, rsd, max_batch=64)


def _both(cond):
    ids = cond + RCFG.codebook_size + 1
    return torch.cat([ids, torch.full_like(ids, RCFG.none_condition_id)])


@pytest.mark.parametrize("B", RAR_ROWS)
def test_rar_1280_rows_teacher_forced_256_steps(pv, rar, B):
    """M = 2B rows (conditional rows, then unconditional rows: rows [:B] and [64:64+B] of the fixture), all 256 steps: every 8th logit
    at the fixture's 23 steps within 5e-4 of the reference's"""
    toks = torch.from_numpy(pv["rar_tokens"].astype(np.int64))[:B]
    rows = torch.cat([torch.arange(B), 64 + torch.arange(B)]).cuda()
    both = _both(torch.from_numpy(pv["rar_cond"].astype(np.int64))[:B]).cuda()
    fix = torch.from_numpy(pv["rar_logits"].astype(np.float32)).cuda()
    want = {int(s): i for i, s in enumerate(pv["rar_steps"])}
    tok2 = torch.cat([toks, toks]).cuda()                                   # [2B, 256]
    rar.forward_position(torch.full((2 * B,), -1, dtype=torch.int64).cuda(), both, 0)
    d = torch.zeros(256, device="cuda")
    tok = both
    for n in range(256):
        lg = rar.forward_position(tok, both, n + 1)
        if n in want:
            d[n] = (lg[:, ::8] - fix[want[n]].index_select(0, rows)).abs().max()
        tok = tok2[:, n]
    d = d.cpu().numpy()
    print(f"RAR {B} conditions ({2 * B} rows): max |dlogit| over {len(want)} steps: {d.max():.2e}")
    bad = ~(d < ATOL)
    assert not bad.any(), (B, [(int(n), float(d[n])) for n in np.nonzero(bad)[0][:8]])


@pytest.mark.parametrize("Mrows", [33, 65])
def test_rar_1280_odd_row_counts_vs_oracle(pv, rar, rsd, Mrows):
    """forward_position takes any row count: the first M of the 128 guided rows at positions 0..3 against rar_oracle.rar_position"""
    toks = torch.from_numpy(pv["rar_tokens"].astype(np.int64))
    both = _both(torch.from_numpy(pv["rar_cond"].astype(np.int64)))[:Mrows]
    tok2 = torch.cat([toks, toks])[:Mrows]
    ce = rsd["embeddings.weight"][both]
    kc = vc = None
    worst = 0.0
    for p in range(4):
        if p == 0:
            emb, tok = rsd["cls_token"][0, 0].expand(Mrows, -1), torch.full((Mrows,), -1, dtype=torch.int64)
        else:
            tok = both if p == 1 else tok2[:, p - 2]
            emb = rsd["embeddings.weight"][tok]
        with torch.no_grad():
            ref, kc, vc = R.rar_position(rsd, RCFG, emb, ce, p, kc, vc)
        lg = rar.forward_position(tok.cuda(), both.cuda(), p).cpu().numpy()
        d = float(np.abs(lg - ref.numpy()).max())
        worst = max(worst, d)
        assert d < ATOL, (Mrows, p, d)
    print(f"RAR {Mrows} rows: max |dlogit| at positions 0..3: {worst:.2e}")


def _rar_inputs(B, seed):
    cond = torch.tensor([(i * 13 + 1) % 1000 for i in range(B)])
    q = torch.empty(RCFG.image_seq_len, B, RCFG.codebook_size).exponential_(1, generator=torch.Generator().manual_seed(seed))
    return cond, q


@pytest.mark.parametrize("B", [10, 20, 33, 40])
def test_rar_1280_guided_loop_vs_oracle(rar, rsd, kat, key_factory, B):
    """generate() under guidance 4.0 with the watermark (the adaLN split between conditional and unconditional rows inside a row
    tile), graph and eager, against rar_oracle.generate, then the logits of the first 32 steps teacher-forced on the oracle's tokens.
    The tokens are compared over ALL 256 steps, not only the first 32: the guided loop exposes no logits, so a small error in one row's
    modulation shows only where it moves a sampled token (tried on a scratch build: the last conditional row of 33 taking the
    unconditional table in layer 0's first modulation alone went unnoticed over 32 steps; in every modulation it fails at step 0)."""
    wm = _wm(kat["keys"]["rar"])
    key = key_factory(kat["keys"]["rar"])
    steps, steps_lg = RCFG.image_seq_len, 32
    cond, q = _rar_inputs(B, 4000 + B)
    rec = []
    ref = R.generate(rsd, RCFG, cond, guidance_scale=4.0, guidance_scale_pow=0.0, key=key, delta=2.0,
                     q_source=lambda n, b, v: q[n], record=rec, draw_drop_mask=False).numpy()
    qd = q.cuda()
    for graph in (True, False):
        got = rar.generate(cond.cuda(), qd, R.cfg_scales(RCFG.image_seq_len, 4.0, 0.0), 1.0, wm.wm_ctx(), use_graph=graph).cpu().numpy()
        assert got.shape == (B, RCFG.image_seq_len)
        near = _compare_tokens(got[:, :steps], ref, rec, 16 * ATOL)
        print(f"RAR {B} conditions, {'graph' if graph else 'eager'}: {int((got[:, :steps] == ref).all(1).sum())} of {B} rows equal over "
              f"{steps} steps, {near} near-tie divergences")
        assert near <= 1, near
    both = _both(cond).cuda()
    rar.forward_position(torch.full((2 * B,), -1, dtype=torch.int64).cuda(), both, 0)
    tok = both
    worst = 0.0
    for n in range(steps_lg):
        lg = rar.forward_position(tok, both, n + 1).cpu().numpy()
        d = float(np.abs(lg - np.concatenate([rec[n]["cond_logits"], rec[n]["uncond_logits"]])).max())
        worst = max(worst, d)
        assert d < ATOL, (B, n, d)
        t = torch.from_numpy(ref[:, n])
        tok = torch.cat([t, t]).cuda()
    print(f"RAR {B} conditions: max |dlogit| over {steps_lg} steps x {2 * B} rows x {RCFG.codebook_size} logits: {worst:.2e}")


def test_rar_1280_generate_40_10_40_rows_bit_equal(rar, kat):
    """generate() with 40, then 10, then 40 conditions again on one engine: the first and the last run equal bit for bit"""
    wm = _wm(kat["keys"]["rar"])
    cond, q = _rar_inputs(40, 4140)
    qd = q.cuda()
    q10 = qd[:, :10].contiguous()
    sc = R.cfg_scales(RCFG.image_seq_len, 4.0, 0.0)
    a = rar.generate(cond.cuda(), qd, sc, 1.0, wm.wm_ctx()).clone()
    rar.generate(cond.roll(7)[:10].cuda(), q10, sc, 1.0, wm.wm_ctx())
    b = rar.generate(cond.cuda(), qd, sc, 1.0, wm.wm_ctx()).clone()
    assert torch.equal(a, b), f"rows that differ after the 10-row run: {np.nonzero((a != b).any(1).cpu().numpy())[0]}"
