"""Independent restatement of the sampling stage, in plain numpy: float64 for the decisions, float32 for the single-rounding stages
in front of them.  It shares NOTHING with include/wmar_math.h (the arithmetic that both the HIP kernels and the C oracle are
built from): no ordering keys, no fixed-point sums, no polynomial exp -- it does not import ``oracle``.

What it restates (deps/taming/modules/transformer/mingpt.py:351-363 and the two HF warpers it calls):

    x      = row / T                                   float64, T rounded to float32 first (the build holds T as a float)
    top-k  : keep every entry >= the k-th largest VALUE (TopKLogitsWarper: ``scores < topk(scores, k)[0][..., -1]`` is removed;
             a float comparison, so -0.0 and +0.0 are one value and a tie group at the threshold survives whole)
    top-p  : TopPLogitsWarper -- sort ascending, softmax, cumulative sum, remove ``cum <= float32(1 - top_p)``, always keep the
             last entry.  Equal values are ordered by ascending index (the build's documented rule; torch.sort leaves it open)
    race   : softmax over the kept set, token = argmax(p / q), first index on ties (torch.multinomial's exponential race)

DECIDABLE rows.  The float32 chain of the reference and the pinned arithmetic of the build both round; a row whose decision
hangs on less than their rounding error has no single right answer.  ``sample_reference`` therefore repeats the decision with
the top-p threshold moved by -EPS / +EPS (absolute: cumulative probabilities are O(1)) and with the top-k threshold VALUE moved
by -EPS / +EPS relative -- entries EQUAL to the k-th value stay kept under either move: equal inputs are equal in every
precision, so a tie group at the threshold is an exact decision, not a rounding one -- and looks at the race margin.  A row is
decidable when all five tokens are the same and the winning ratio exceeds the runner-up by more than EPS relative, or equals
it exactly (an exact tie is decided by index).  The kept SET is more fragile than the token: a cumulative sum may land on the
threshold itself (500 x 0.001 against 0.5) without the token caring.  ``kept_set_agrees`` asks for equality where no moved
threshold changes the reference's own kept set and for "between the two moved sets" where one does.

EPS.  Measured on the CPU over the whole matrix below (tests/test_sampler_reference.py::test_eps_and_undecidable_share prints
it): the largest absolute difference between torch's own float32 ``softmax`` / ``cumsum`` of the sorted row that top-p sees and
the float64 values is 1.4e-5 (the cumulative sum of the 7e4 equal terms of the all-zero row; 1e-6 on the gaussian rows).
EPS = 8 x that = 1.2e-4.  With it 8 of the 870 rows of the matrix are undecidable (0.92 %; the bound is 2 %): the all-zero row
under top_p = 0.0 at seven sizes, where the float sum of V equal terms does or does not reach the threshold 1, and one rounded
row.  The oracle disagrees with this file on none of the other 862, in token or kept set.

The matrix has ten rows per case, one of each kind in ROW_KINDS (three plain gaussians of scale 1, 2, 3 among them).

NaN logits are out of scope: ``sample_reference`` raises.
"""
import numpy as np

EPS = 1.2e-4                       # 8 x 1.4e-5 (see above); the CPU test measures the gap again and asserts 8 x gap <= EPS

# ------------------------------------------------------------------------------------------------------------- the matrix
VOCABS = (1, 33, 1000, 1023, 1025, 16383, 16384, 16385, 20000, 65535, 65536, 65537, 70001)
# (T, top_k, top_p); None = off
SETTINGS = ((1.0, 250, 0.92), (1.3, 1024, 0.8), (0.9, None, 0.95), (1.0, 1025, None), (0.7, 1, 0.5), (1.0, None, 0.0),
            (1.0, 3000, 1.0), (1.0, None, None))
ROW_KINDS = ("gauss1", "gauss2", "gauss3", "rounded", "zeros", "plateau", "dominant_last", "upper_half_neg_inf", "winner_first",
             "winner_last")
MATRIX_SEED = 20240


def matrix_cases():
    """(V, T, top_k, top_p) of the matrix; a top_k >= V is the same decision as no top-k and is left out."""
    return [(V, T, tk, tp) for V in VOCABS for (T, tk, tp) in SETTINGS if tk is None or tk < V]


def matrix_rows(V, seed=MATRIX_SEED):
    """The rows of one vocabulary size, one per ROW_KINDS entry: (logits float32 [B, V], noise float32 [B, V])."""
    rs = np.random.RandomState(seed + V)
    B = len(ROW_KINDS)
    lg = rs.randn(B, V).astype(np.float32)
    lg[0] *= 1.0
    lg[1] *= 2.0
    lg[2] *= 3.0
    lg[3] = np.round(lg[3] * 3.0)                    # integers: many ties, -0.0 among them (np.round of a small negative)
    lg[4] = 0.0
    lg[5] *= 3.0
    lg[5, : V // 3] = 9.0                            # a plateau that straddles the top-k / top-p boundaries
    lg[6] *= 3.0
    lg[6, V - 1] = 24.0                              # one dominant entry, last
    lg[7] *= 3.0
    lg[7, max(1, V // 2):] = -np.inf
    lg[8] *= 3.0
    lg[9] *= 3.0
    q = rs.exponential(size=(B, V)).astype(np.float32)
    q = np.maximum(q, np.float32(1e-6))
    # the winner forced to an end of the row: the row maximum sits there (kept by every warper) under a tiny noise value
    lg[8, 0] = lg[8].max() + np.float32(1.0)
    q[8, 0] = 1e-20
    lg[9, V - 1] = lg[9].max() + np.float32(1.0)
    q[9, V - 1] = 1e-20
    return lg, q


# ---------------------------------------------------------------------------------------------------- float64 decisions
def _kept_top_k(x, top_k, shift):
    if not top_k or top_k <= 0:
        return np.ones(x.shape, dtype=bool), None
    k = min(int(top_k), x.size)
    kth = np.partition(x, x.size - k)[x.size - k]
    thr = kth + shift * abs(kth) if np.isfinite(kth) else kth
    keep = x >= thr
    keep |= x == kth                                 # entries EQUAL to the k-th value stay: equality is exact in every precision
    return keep, kth


def _decide(x, q, top_k, top_p, k_shift=0.0, p_shift=0.0):
    """One pass of the chain.  Returns (token, kept mask, best ratio, runner-up ratio)."""
    V = x.size
    alive, _ = _kept_top_k(x, top_k, k_shift)
    alive &= x > -np.inf
    m = x[alive].max()
    kept = alive.copy()
    if top_p is not None:
        idx = np.nonzero(alive)[0]
        order = idx[np.lexsort((idx, x[idx]))]       # ascending value, equal values (-0.0 == +0.0) by ascending index
        e = np.exp(x[order] - m)
        cum = np.cumsum(e / e.sum())
        thr = np.float64(np.float32(1.0 - top_p)) + p_shift
        remove = cum <= thr
        remove[-1] = False
        kept[order[remove]] = False
    e = np.where(kept, np.exp(np.where(kept, x, 0.0) - m), 0.0)
    p = e / e.sum()
    with np.errstate(divide="ignore", over="ignore"):
        r = p / q
    tok = int(np.argmax(r))
    best = r[tok]
    if V > 1:
        r2 = r.copy()
        r2[tok] = -np.inf
        second = r2.max()
    else:
        second = 0.0
    return tok, kept, best, second


def sample_reference(row, q, T=1.0, top_k=None, top_p=None, eps=EPS):
    """row: float32 [V] after bias / guidance / allow-list, q: its noise row.
    Returns (token, kept mask bool [V], decidable, kept_inner, kept_outer): the last two are the intersection and the union of
    the kept sets under the moved thresholds -- an entry outside ``inner`` and inside ``outer`` is one whose membership hangs on
    less than EPS (a cumulative sum that lands ON the threshold, as 500 x 0.001 against 0.5 does), and a correct kept set lies
    between the two; where they coincide it IS ``kept``."""
    row = np.asarray(row)
    if np.isnan(row).any():
        raise ValueError("NaN logits are outside the reference")
    x = row.astype(np.float64) / np.float64(np.float32(T))
    qq = np.asarray(q).astype(np.float64)
    tok, kept, best, second = _decide(x, qq, top_k, top_p)
    decidable = bool(best > second * (1.0 + eps) or best == second)
    moved = []
    if top_p is not None:
        moved += [_decide(x, qq, top_k, top_p, p_shift=s) for s in (-eps, eps)]
    if top_k and 0 < top_k < x.size:
        moved += [_decide(x, qq, top_k, top_p, k_shift=s) for s in (-eps, eps)]
    inner, outer = kept.copy(), kept.copy()
    for t2, k2, _, _ in moved:
        decidable = decidable and t2 == tok
        inner &= k2
        outer |= k2
    return tok, kept, decidable, inner, outer


def sample_reference_rows(rows, q, T=1.0, top_k=None, top_p=None, eps=EPS):
    out = [sample_reference(r, qq, T, top_k, top_p, eps) for r, qq in zip(rows, q)]
    return (np.array([o[0] for o in out], dtype=np.int64), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=bool),
            np.stack([o[3] for o in out]), np.stack([o[4] for o in out]))


def kept_set_agrees(kept_got, ref, b):
    """The kept set of row b against the reference's (``ref`` = what sample_reference_rows returned): equal to ``kept`` where the
    reference's kept set does not move under the shifted thresholds, and between ``inner`` and ``outer`` where it does."""
    _, kept, _, inner, outer = ref
    if np.array_equal(inner[b], outer[b]):
        return np.array_equal(kept_got, kept[b])
    return bool(np.all(kept_got[inner[b]]) and not np.any(kept_got[~outer[b]]))


# ------------------------------------------------------------------------------------- float32 stages in front of the sampler
def bits_to_mask(words, V):
    """uint32 key / allow words, bit j of word w = entry 32 w + j  ->  bool [V]."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:V].astype(bool)


def restate_stages(cond, *, uncond=None, img=None, scale=None, g_text=None, g_image=None, green=None, delta=0.0, allow=None,
                   gather=None):
    """The single-rounding float32 stages, in the build's order, one operation per statement (numpy rounds each to float32):

        guidance   two streams:   u + (c - u) * s                            (RAR.generate)
                   three streams: u + g_image * (im - u) + g_text * (c - im)  (InBatchInstructCFG)
        bias       + delta where the row's key bit is set (``green``: bool [B, V] or None; a None ROW is a skipped row)
        allow-list -inf outside ``allow`` (bool [V])
        gather     the columns ``gather`` (source ids), in that order

    Everything is compared bit for bit: there is no tolerance to choose."""
    f = np.float32
    c = np.asarray(cond, dtype=f)
    if img is not None:
        u, im = np.asarray(uncond, dtype=f), np.asarray(img, dtype=f)
        d1 = im - u
        t1 = f(g_image) * d1
        s1 = u + t1
        d2 = c - im
        t2 = f(g_text) * d2
        x = s1 + t2
    elif uncond is not None:
        u = np.asarray(uncond, dtype=f)
        d = c - u
        sc = d * f(scale)
        x = u + sc
    else:
        x = c.copy()
    assert x.dtype == f
    if green is not None:
        for b in range(x.shape[0]):
            if green[b] is not None:
                x[b] = np.where(green[b], x[b] + f(delta), x[b])
    if allow is not None:
        x = np.where(np.asarray(allow, dtype=bool)[None, :], x, f(-np.inf))
    if gather is not None:
        x = x[:, np.asarray(gather, dtype=np.int64)]
    return np.ascontiguousarray(x, dtype=f)


def divide_by_temperature(x, T):
    """float32 x / float32 T: what the sampler exports as its row."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, dtype=np.float32) / np.float32(T)).astype(np.float32)
