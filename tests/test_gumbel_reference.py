"""The Gumbel-key sampler's second and third link, on the CPU: the C oracle (built from include/wmar_math.h,
as k_gumbel_sample is) against the float64 restatement tests/gumbel_reference.py, and that restatement against the reference's own
recorded decisions -- the 5 940 tokens of tests/golden/gumbel_bulk.npz (engine.py's gumbel_sample run by make_golden.py
--only gumbelbulk) and the 144 of gumbel_vectors.npz.

Measured here (printed by the tests, -s): 4 of the 5 940 bulk rows are undecidable (0.07 %; three plain top-k 250 rows at
V = 16383 / 16384 and one top-p row at V = 37); the oracle equals float64 on all 5 936 others and on the 4 as well.  964 rows have
their top-p / top-k cut inside a group of exactly equal probabilities (all among the half-integer and bf16-valued rows); the
reference resolved 18 of them the other way, and equals float64 on every decidable row outside that class.  The float32 softmax /
cumsum gap on the top-p rows of this matrix is 6.1e-6, so 8 x gap = 4.9e-5 <= EPS holds with EPS unchanged.

No window hash makes every candidate underflow, ties two winning scores exactly or puts a score at the underflow bound, so three
of the planted faults below would pass on hashed keys alone.  The oracle and float64 therefore also meet on CONSTANT key rows
(rs = 0, 0.5, 0.2, 0.02 for every entry) over the V = 16384, scale 1 chunks: every candidate in the lowest class (the first in
order must win: by rank under top-p, by index otherwise) and maxima on either side of log 2^-150."""
import os

import numpy as np
import pytest
import torch

from oracle import wm_oracle as W
from tests import gumbel_reference as G
from tests.conftest import REPO
from tests.sampler_reference import EPS

G.bulk_chunk(0)                                     # puts tests/golden on the path
from bulk_inputs import GUM_BULK_CHUNKS, GUM_BULK_ROWS, GUM_BULK_V, gumbel_bulk_case  # noqa: E402

CONST_KEYS = (0.0, 0.5, 0.2, 0.02)
CONST_CHUNKS = [c for c in range(GUM_BULK_CHUNKS) if gumbel_bulk_case(c)[:2] == (16384, 1.0)]


def oracle_rows(lg, rs, T, top_p, top_k):
    """wmo_gumbel_sample_row over rows with the key given as rs ([V] or [B, V])."""
    lg = np.ascontiguousarray(lg, dtype=np.float32)
    rs = np.broadcast_to(np.asarray(rs, dtype=np.float32), lg.shape)
    return np.array([W.lib().wmo_gumbel_sample_row(lg[b], lg.shape[1], np.ascontiguousarray(rs[b]), 1, float(T), float(top_p),
                                                   int(top_k)) for b in range(len(lg))], dtype=np.int64)


@pytest.fixture(scope="module")
def ref_tokens():
    return np.load(os.path.join(REPO, "tests", "golden", "gumbel_bulk.npz"))["tokens"].astype(np.int64)


@pytest.fixture(scope="module")
def f64():
    return G.bulk_decisions()


@pytest.fixture(scope="module")
def oracle_tokens():
    out = np.zeros((GUM_BULK_CHUNKS, GUM_BULK_ROWS), dtype=np.int64)
    for c in range(GUM_BULK_CHUNKS):
        lg, _, rs, (T, top_p, top_k) = G.bulk_chunk(c)
        out[c] = oracle_rows(lg, rs, T, top_p, top_k)
    return out


@pytest.fixture(scope="module")
def const_rows():
    """{(chunk, key): (oracle token, float64 token, decidable)} of the constant-key rows."""
    out = {}
    for c in CONST_CHUNKS:
        lg, _, _, (T, top_p, top_k) = G.bulk_chunk(c)
        for key in CONST_KEYS:
            rs = np.full(lg.shape[1], key, dtype=np.float32)
            tok, dec, _ = G.decide(lg, T, top_p, top_k, rs=rs)
            out[c, key] = (oracle_rows(lg, rs, T, top_p, top_k), tok, dec)
    return out


def test_fixture_shape(ref_tokens):
    assert ref_tokens.shape == (GUM_BULK_CHUNKS, GUM_BULK_ROWS) and ref_tokens.min() >= 0
    for c in range(GUM_BULK_CHUNKS):
        assert ref_tokens[c].max() < gumbel_bulk_case(c)[0]
    assert GUM_BULK_V == (37, 1000, 1024, 16383, 16384)


def test_oracle_equals_float64_on_every_decidable_bulk_row(f64, oracle_tokens):
    tok, dec, _ = f64
    bad = np.argwhere((oracle_tokens != tok) & dec)
    print(f"oracle vs float64: {len(bad)} differences on {int(dec.sum())} decidable rows; "
          f"{int(((oracle_tokens != tok) & ~dec).sum())} on the {int((~dec).sum())} undecidable ones")
    assert len(bad) == 0, [(int(c), int(b), gumbel_bulk_case(c)) for c, b in bad[:8]]


def test_reference_equals_float64_outside_its_unspecified_ties(f64, ref_tokens):
    tok, dec, amb = f64
    diff = (ref_tokens != tok) & dec
    unexplained = np.argwhere(diff & ~amb)
    print(f"reference vs float64: {int(amb.sum())} rows with the cut inside a group of equal probabilities, the reference resolved "
          f"{int((diff & amb).sum())} of them the other way; {len(unexplained)} unexplained differences in {tok.size} decisions")
    assert len(unexplained) == 0, [(int(c), int(b), gumbel_bulk_case(c)) for c, b in unexplained[:8]]
    assert int((dec & ~amb).sum()) >= 4500                  # the link is held on most of the matrix, not on a remainder


def test_undecidable_share(f64):
    _, dec, _ = f64
    share = float((~dec).mean())
    print(f"undecidable: {int((~dec).sum())} of {dec.size} rows ({100 * share:.2f} %)")
    assert share <= 0.01


def test_constant_key_rows(const_rows):
    """Lowest-class ties and maxima around the underflow bound: the oracle equals float64 on every decidable row."""
    n = bad = 0
    for (c, key), (otok, tok, dec) in const_rows.items():
        n += int(dec.sum())
        bad += int(((otok != tok) & dec).sum())
    print(f"constant keys: {n} decidable rows of {len(const_rows) * GUM_BULK_ROWS}")
    assert bad == 0 and n >= 0.8 * len(const_rows) * GUM_BULK_ROWS


def test_eps_covers_the_float32_chain():
    """8 x (largest gap between torch's float32 softmax / cumsum of the sorted row and float64, over the top-p chunks) <= EPS."""
    gap = 0.0
    for c in range(GUM_BULK_CHUNKS):
        T, top_p, _ = gumbel_bulk_case(c)[3]
        if top_p <= 0.0:
            continue
        lg = torch.from_numpy(G.bulk_chunk(c)[0])
        x = lg / T
        ps32, _ = torch.sort(torch.softmax(x, dim=-1), dim=-1, descending=True)
        cum32 = torch.cumsum(ps32, dim=-1)
        ps64 = -np.sort(-torch.softmax(x.double(), dim=-1).numpy(), axis=-1)
        gap = max(gap, float(np.abs(ps32.numpy() - ps64).max()), float(np.abs(cum32.numpy() - np.cumsum(ps64, axis=-1)).max()))
    print(f"float32 softmax / cumsum gap on the Gumbel bulk matrix: {gap:.3g}; 8 x gap = {8 * gap:.3g}, EPS = {EPS:.3g}")
    assert 8 * gap <= EPS


@pytest.mark.parametrize("hname", ["same", "rows"])
def test_gumbel_vectors_three_ways(hname):
    """The 12 rows x 6 settings of gumbel_vectors.npz: reference, oracle and float64."""
    gv = np.load(os.path.join(REPO, "tests", "golden", "gumbel_vectors.npz"))
    lg, h = gv["gum_logits"], gv["gum_hash_" + hname]
    rs = G.key_rows(h, lg.shape[1])
    n = 0
    for (t, p, k), name in zip(gv["gum_cases"], gv["gum_case_names"]):
        tok, dec, amb = G.decide(lg, t, p, int(k), rs=rs)
        assert np.array_equal(oracle_rows(lg, rs, t, p, int(k))[dec], tok[dec]), name
        ok = dec & ~amb
        assert np.array_equal(gv[f"gum_tok_{hname}_{name}"][ok], tok[ok]), name
        n += int(ok.sum())
    assert n >= 70
    assert np.array_equal(G.greedy(lg), gv[f"gum_tok_{hname}_greedy"])


def test_score_restatement():
    gv = np.load(os.path.join(REPO, "tests", "golden", "gumbel_vectors.npz"))
    rs = G.key_rows(gv["gum_hash_rows"], 1024)
    s = np.array([G.score(rs[b], t) for b, t in enumerate(gv["gum_score_tokens"])])
    assert np.array_equal(s.astype(np.float32).astype(np.int64), gv["gum_score_rows"])


# fault -> (which settings show it, whether it needs the constant-key rows)
PLANTED = {
    "cut_on_cum": (lambda T, p, k: p > 0.0, False),
    "fill_outside_norm": (lambda T, p, k: p == 0.0 and 0 < k < 16384, True),
    "ties_by_index": (lambda T, p, k: p > 0.0, True),
    "score_times_p": (lambda T, p, k: True, False),
    "temperature_after_softmax": (lambda T, p, k: T != 1.0 and p > 0.0, False),
    "top_k_first": (lambda T, p, k: p > 0.0 and k > 0, False),
    "no_underflow_class": (lambda T, p, k: p == 0.0, True),
}


@pytest.mark.parametrize("fault", G.FAULTS)
def test_planted_fault_is_noticed(fault, f64, oracle_tokens, const_rows):
    """Each misreading, planted in a copy of the restatement, breaks "oracle == float64 on the decidable rows" on these rows."""
    touches, constant = PLANTED[fault]
    hits = 0
    if constant:
        for (c, key), (otok, _, dec) in const_rows.items():
            lg, _, _, (T, top_p, top_k) = G.bulk_chunk(c)
            if touches(T, top_p, top_k):
                tok = G.decide(lg, T, top_p, top_k, rs=np.full(lg.shape[1], key, dtype=np.float32), fault=fault)[0]
                hits += int(((tok != otok) & dec).sum())
    else:
        _, dec, _ = f64
        for c in range(GUM_BULK_CHUNKS):
            lg, _, rs, (T, top_p, top_k) = G.bulk_chunk(c)
            if touches(T, top_p, top_k):
                hits += int(((G.decide(lg, T, top_p, top_k, rs=rs, fault=fault)[0] != oracle_tokens[c]) & dec[c]).sum())
            if hits >= 3:
                break
    print(f"{fault}: {hits} decidable rows notice it")
    assert hits >= 1
