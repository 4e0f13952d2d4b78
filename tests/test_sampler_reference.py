"""The float64 restatement of the sampling stage (tests/sampler_reference.py) against the reference's own float32 chain
(transformers' warpers + torch.softmax) and against the C oracle, on the CPU; the detector's p-values against scipy.

The oracle and the HIP kernels share include/wmar_math.h, so "HIP == oracle" cannot see an error in that header.  This file is
the outside check of the oracle; tests/test_gpu_sampler_paths.py then ties every kernel path to the oracle bit for bit."""
import numpy as np
import pytest
import torch

from oracle import wm_oracle as W
from tests import sampler_reference as R


@pytest.fixture(scope="module")
def matrix():
    """Every (case, rows, noise, reference decision) of the matrix, computed once."""
    out = []
    rows = {V: R.matrix_rows(V) for V in R.VOCABS}
    for V, T, tk, tp in R.matrix_cases():
        lg, q = rows[V]
        out.append(((V, T, tk, tp), lg, q, R.sample_reference_rows(lg, q, T, tk, tp)))
    return out


def _f32_gap(lg, T, tk, tp):
    """Largest |float32 - float64| over torch's softmax and cumsum of the sorted row that top-p sees (the reference's arithmetic)."""
    gap = 0.0
    for row in lg:
        x = torch.from_numpy(row) / np.float32(T)
        if tk:
            x = x[x >= torch.topk(x, min(tk, x.numel()))[0][-1]]
        x = torch.sort(x[x > -np.inf])[0]
        p32 = torch.softmax(x, -1)
        p64 = torch.softmax(x.double(), -1)
        gap = max(gap, float((p32.double() - p64).abs().max()), float((p32.cumsum(-1).double() - p64.cumsum(-1)).abs().max()))
    return gap


def test_eps_and_undecidable_share(matrix):
    gap = max(_f32_gap(lg, T, tk, tp) for (V, T, tk, tp), lg, q, _ in matrix if tp is not None)
    n = sum(len(ref[2]) for *_, ref in matrix)
    und = sum(int((~ref[2]).sum()) for *_, ref in matrix)
    print(f"float32 - float64 gap of torch softmax / cumsum over the matrix: {gap:.3e}; EPS = {R.EPS:g} (8 x gap = {8 * gap:.3e}); "
          f"undecidable rows: {und} of {n} ({100.0 * und / n:.2f} %)")
    assert 8 * gap <= R.EPS
    assert gap >= R.EPS / 80, "EPS is more than ten times wider than 8 x the measured gap: measure again"
    assert und <= 0.02 * n


def test_reference_equals_oracle_on_the_full_matrix(matrix):
    """Tokens on every decidable row; the kept sets too (the oracle's ``xs`` is finite exactly where an entry is kept)."""
    bad, bad_kept, n_dec, n_exact = [], [], 0, 0
    for (V, T, tk, tp), lg, q, ref in matrix:
        tok, kept, dec, inner, outer = ref
        otok, xs, _ = W.sample_rows(lg, q, T, tk, tp, return_all=True)
        for b in np.nonzero(dec)[0]:
            n_dec += 1
            if otok[b] != tok[b]:
                bad.append((V, T, tk, tp, R.ROW_KINDS[b], int(otok[b]), int(tok[b])))
            n_exact += int(np.array_equal(inner[b], outer[b]))
            if not R.kept_set_agrees(np.isfinite(xs[b]), ref, b):
                bad_kept.append((V, T, tk, tp, R.ROW_KINDS[b], int(np.isfinite(xs[b]).sum()), int(kept[b].sum())))
    print(f"oracle vs float64 reference: {len(bad)} token and {len(bad_kept)} kept-set mismatches on {n_dec} decidable rows "
          f"({n_exact} with a kept set that no moved threshold changes: compared for equality)")
    assert not bad, bad[:8]
    assert not bad_kept, bad_kept[:8]


REDUCED = [(V, T, tk, tp) for (V, T, tk, tp) in R.matrix_cases() if V in (33, 1000, 1025, 16385, 65537)]


def test_reference_equals_the_hf_float32_chain(matrix):
    """transformers' TopKLogitsWarper / TopPLogitsWarper + torch.softmax in float32, token = argmax(p / q).  torch.sort orders
    equal values arbitrarily, so a row whose top-p cut falls inside a tie group is compared only when the reference's kept set
    shows no such cut (the same exception tests/test_sampler_bulk.py documents)."""
    tr = pytest.importorskip("transformers")
    n = skipped = 0
    for (V, T, tk, tp), lg, q, (tok, kept, dec, _, _) in matrix:
        if (V, T, tk, tp) not in REDUCED:
            continue
        x = torch.from_numpy(lg) / np.float32(T)
        if tk:
            x = tr.TopKLogitsWarper(tk)(None, x)
        if tp is not None:
            x = tr.TopPLogitsWarper(tp)(None, x) if 0.0 < tp < 1.0 else _top_p_edge(x, tp)
        p = torch.softmax(x, -1)
        hf = torch.argmax(p / torch.from_numpy(q), -1).numpy()
        for b in np.nonzero(dec)[0]:
            xb = lg[b].astype(np.float64)
            removed = ~kept[b] & np.isfinite(xb)
            if tp is not None and removed.any() and xb[removed].max() == xb[kept[b]].min():
                skipped += 1
                continue
            n += 1
            assert hf[b] == tok[b], (V, T, tk, tp, R.ROW_KINDS[b], int(hf[b]), int(tok[b]))
    print(f"HF float32 chain vs float64 reference: {n} rows equal, {skipped} with the top-p cut inside a tie group left out")
    assert n > 250


def _top_p_edge(x, tp):
    """TopPLogitsWarper's body for top_p = 0.0 and 1.0, which its constructor refuses but the build's ABI takes (transformers
    logits_process.py: sort ascending, softmax, cumsum, remove cum <= 1 - top_p, keep the last)."""
    sl, si = torch.sort(x, descending=False)
    rem = sl.softmax(-1).cumsum(-1) <= (1 - tp)
    rem[..., -1:] = False
    return x.masked_fill(rem.scatter(1, si, rem), -float("inf"))


# ------------------------------------------------------------------------------------------------------------ signed zeros
# Expected tokens are literals taken from torch (see each test): -0.0 and +0.0 are one value to every comparison of the reference.
def test_signed_zero_top_k():
    row = np.array([-0.0] * 10 + [0.0] * 10 + [-5.0] * 44, dtype=np.float32)
    q = np.ones(64, dtype=np.float32)
    q[0] = 1e-3
    x = torch.from_numpy(row)
    x = x.masked_fill(x < torch.topk(x, 5)[0][-1], -float("inf"))          # TopKLogitsWarper
    assert int(torch.argmax(torch.softmax(x, -1) / torch.from_numpy(q))) == 0
    tok, kept, dec, _, _ = R.sample_reference(row, q, 1.0, 5, None)
    assert (tok, dec, int(kept.sum())) == (0, True, 20)
    otok, xs, _ = W.sample_rows(row[None], q[None], 1.0, 5, None, return_all=True)
    assert int(np.isfinite(xs[0]).sum()) == 20
    assert int(otok[0]) == 0


def test_signed_zero_greedy_gumbel():
    row = np.full(64, -3.0, dtype=np.float32)
    row[0], row[5] = -0.0, 0.0
    assert int(torch.argmax(torch.from_numpy(row))) == 0
    assert int(np.argmax(row.astype(np.float64))) == 0
    assert int(W.gumbel_sample(row[None], [7], use_sampling=False)[0]) == 0


def test_signed_zero_top_p_order_is_by_index():
    """Four zeros of mixed sign and nothing else: ascending (value, index) order is 0, 1, 2, 3 whatever the signs, so
    top_p = 0.5 (remove cum <= 0.5) removes entries 0 and 1 and keeps 2 and 3; the noise makes entry 2 win.  With -0.0 ordered
    below +0.0 the order would be 1, 3, 0, 2, entries 1 and 3 would go and entry 0 would win."""
    row = np.array([0.0, -0.0, 0.0, -0.0], dtype=np.float32)
    q = np.array([1e-3, 1.0, 1e-2, 1.0], dtype=np.float32)
    tok, kept, dec, _, _ = R.sample_reference(row, q, 1.0, None, 0.5)
    assert (tok, dec, kept.tolist()) == (2, True, [False, False, True, True])
    otok, xs, _ = W.sample_rows(row[None], q[None], 1.0, None, 0.5, return_all=True)
    assert np.isfinite(xs[0]).tolist() == [False, False, True, True]
    assert int(otok[0]) == 2


# ---------------------------------------------------------------------------------------------------- float32 stages
def test_restated_stages_against_torch_float32():
    rs = np.random.RandomState(4)
    c, u, im = (rs.randn(3, 70).astype(np.float32) * 5 for _ in range(3))
    tc, tu, ti = torch.from_numpy(c), torch.from_numpy(u), torch.from_numpy(im)
    assert np.array_equal(R.restate_stages(c, uncond=u, scale=4.5), (tu + (tc - tu) * 4.5).numpy())
    assert np.array_equal(R.restate_stages(c, uncond=u, img=im, g_text=3.0, g_image=1.2), (tu + 1.2 * (ti - tu) + 3.0 * (tc - ti)).numpy())
    green = rs.rand(3, 70) < 0.25
    allow = rs.rand(70) < 0.5
    ids = np.nonzero(allow)[0]
    exp = tc.clone()
    exp[torch.from_numpy(green)] += 2.0
    exp[:, torch.from_numpy(~allow)] = -float("inf")
    assert np.array_equal(R.restate_stages(c, green=green, delta=2.0, allow=allow, gather=ids), exp[:, torch.from_numpy(ids)].numpy())
    words = np.array([0x80000001, 0x3], dtype=np.uint32)
    assert np.nonzero(R.bits_to_mask(words, 40))[0].tolist() == [0, 31, 32, 33]


# ------------------------------------------------------------------------------------------------ detector p-values
@pytest.mark.parametrize("ns,ng,gamma", [(1, 1, 0.25), (1, 0, 0.25), (3, 2, 0.25), (1023, 1023, 0.25), (1008, 1008, 0.25), (1022, 0, 0.25),
                                         (15, 9, 0.25), (9, 4, 0.5), (961, 300, 0.25), (300, 120, 0.25), (1, 1, 0.5), (299, 299, 0.5),
                                         (1023, 700, 0.25)])
def test_oracle_p_values_against_scipy(ns, ng, gamma):
    """The counts that the detector cases of tests/test_gpu_sampler_paths.py produce (single n-gram, all green, none green,
    underflow, small spatial grids) against scipy.special.betainc(n_green, 1 + n_scored - n_green, gamma)."""
    sp = pytest.importorskip("scipy.special")
    got, exp = W.betainc_int(ng, 1 + ns - ng, gamma), float(sp.betainc(ng, 1 + ns - ng, gamma))
    if np.isnan(exp):
        assert np.isnan(got)
    elif exp == 0.0:
        assert got == 0.0
    else:
        assert abs(got - exp) <= 1e-9 * exp, (got, exp)
