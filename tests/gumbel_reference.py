"""Independent restatement of the Gumbel-key sampler (wmar_audio/watermark/engine.py:29-75, ``gumbel_sample``) and of its
detector score (:123-134, ``gumbel_score_tok``) in plain numpy: float64 for the decisions, float32 for the two single-rounding
stages in front of them.  Like tests/sampler_reference.py it shares NOTHING with include/wmar_math.h (the arithmetic that
k_gumbel_sample and the C oracle are both built from): no ordering keys, no fixed-point sums, no polynomial exp -- it does not
import ``oracle``.

What it restates:

    mix     u + (x - u) * s                       float32, one rounding per operation (RAR.generate's guidance; ``mix``)
    x       row / float32(T)                      float32 (``scale_by_temperature``)
    p       softmax(x)                            float64 from here on
    top-p   (top_p > 0) sort descending, equal values by ascending index; drop where cum - p > float32(top_p); renormalise
    top-k   (else, top_k > 0) keep the first min(k, V) of that same order, every other entry becomes float32(1e-6); renormalise
    race    token = argmax log(rs) / p -- the monotone image of the reference's rs ** (1 / p).  Candidates are ordered by sorted
            rank under top-p (the reference races the sorted row and maps the winner back) and by index otherwise; scores below
            log 2^-150 (the reference's float32 pow rounds to exactly 0 there) and entries with p = 0 form ONE lowest class; the
            first candidate in order wins a tie, as torch.argmax does.

``decide`` takes the key as ``rs`` (what torch.rand gives) or as a ``log_rs`` row directly (what the kernel reads).

UNDECIDABLE rows.  The reference's float32 chain and the build's pinned arithmetic both round; a row whose token hangs on less
than their rounding error has no single right answer.  A row is undecidable when
  * the token changes when the top-p threshold moves by -EPS / +EPS (absolute: cumulative probabilities are O(1));
  * the k-th and (k+1)-th probabilities differ by less than EPS relative without being equal;
  * the winner leads the runner-up by no more than EPS max(1, |s|) without tying it exactly;
  * the winning score lies in [log 2^-150, log 2^-126): the reference's float32 pow is subnormal there and has lost its bits;
  * every candidate is in the lowest class, but one of them is within that margin of the bound log 2^-150.
A row whose candidates ALL lie below the bound by more than the margin is decidable: the reference's pow is exactly 0 for each of
them and its argmax returns the first -- there is nothing left to round.

AMBIGUOUS rows (in the reference, not in the build).  Where the top-p or top-k cut falls strictly inside a group of exactly equal
probabilities, ``torch.sort`` / ``torch.topk`` keep whichever tied entries they happen to put first.  The build breaks the tie by
index and is held to this file there; only the reference's own token is not.

EPS is sampler_reference.EPS; tests/test_gumbel_reference.py measures, on the bulk matrix, the largest gap between torch's
float32 softmax / cumsum of the sorted row and float64, and asserts 8 x gap <= EPS.

NaN logits and rows without a finite entry are out of scope: ``decide`` raises.
"""
import numpy as np

from tests.sampler_reference import EPS

LOG_POW_ZERO = -150.0 * np.log(2.0)        # below: float32 pow(rs, 1 / p) is exactly 0
LOG_POW_SUBNORMAL = -126.0 * np.log(2.0)   # below: it is subnormal
FILL = np.float64(np.float32(1e-6))        # torch.full_like(probs, 1e-6) of a float32 tensor

FAULTS = ("cut_on_cum", "fill_outside_norm", "ties_by_index", "score_times_p", "temperature_after_softmax", "top_k_first",
          "no_underflow_class")


def mix(cond, uncond, scale):
    """Guidance in float32, one rounding per operation: u + (c - u) * s."""
    f = np.float32
    c, u = np.asarray(cond, dtype=f), np.asarray(uncond, dtype=f)
    d = c - u
    sc = d * f(scale)
    out = u + sc
    assert out.dtype == f
    return out


def scale_by_temperature(rows, T):
    """float32 row / float32 T."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(rows, dtype=np.float32) / np.float32(T)).astype(np.float32)


def greedy(rows):
    """use_sampling = False or temp <= 0: torch.argmax of the row as it is (first index of the maximum; -0.0 == +0.0)."""
    return np.argmax(np.asarray(rows, dtype=np.float32), axis=-1).astype(np.int64)


def _pass(x, lr, top_p, top_k, eps, p_shift=0.0, fault=None, T=1.0):
    """One pass over rows x float64 [B, V] (already divided by T) with key rows lr = log(rs) float64 [B, V].
    Returns (token int64 [B], fragile bool [B], ambiguous bool [B])."""
    B, V = x.shape
    idx = np.broadcast_to(np.arange(V), (B, V))
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    if fault == "temperature_after_softmax":
        p = p / np.float64(np.float32(T))
    order = np.lexsort((idx, -p), axis=-1)              # descending probability, equal ones by ascending index
    ps = np.take_along_axis(p, order, axis=-1)
    fragile = np.zeros(B, dtype=bool)
    ambiguous = np.zeros(B, dtype=bool)
    use_top_p = top_p > 0.0 and not (fault == "top_k_first" and top_k > 0)
    by_rank = use_top_p
    if use_top_p:
        cum = np.cumsum(ps, axis=-1)
        thr = np.float64(np.float32(top_p)) + p_shift
        drop = (cum if fault == "cut_on_cum" else cum - ps) > thr
        if V > 1:
            edge = drop[:, 1:] & ~drop[:, :-1]
            ambiguous = (edge & (ps[:, 1:] == ps[:, :-1])).any(axis=-1)
        kept = np.where(drop, 0.0, ps)
        with np.errstate(invalid="ignore", divide="ignore"):
            kept = kept / kept.sum(axis=-1, keepdims=True)
        kept = np.where(np.isnan(kept), 0.0, kept)
        p = np.empty_like(p)
        np.put_along_axis(p, order, kept, axis=-1)
    elif top_k > 0:
        k = min(int(top_k), V)
        if k < V:
            a, b = ps[:, k - 1], ps[:, k]
            ambiguous = a == b
            fragile |= ~ambiguous & ((a - b) < eps * a)
        q = np.full_like(p, FILL)
        np.put_along_axis(q, order[:, :k], ps[:, :k], axis=-1)
        norm = ps[:, :k].sum(axis=-1, keepdims=True) if fault == "fill_outside_norm" else q.sum(axis=-1, keepdims=True)
        p = q / norm
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        raw = lr * p if fault == "score_times_p" else lr / p
    raw = np.where((p == 0.0) | np.isnan(raw), -np.inf, raw)
    s = raw if fault == "no_underflow_class" else np.where(raw < LOG_POW_ZERO, -np.inf, raw)
    if by_rank and fault != "ties_by_index":
        first = np.argmax(np.take_along_axis(s, order, axis=-1), axis=-1)
        tok = order[np.arange(B), first]
    else:
        tok = np.argmax(s, axis=-1)
    best = s[np.arange(B), tok]
    rest = s.copy()
    rest[np.arange(B), tok] = -np.inf
    second = rest.max(axis=-1) if V > 1 else np.full(B, -np.inf)
    with np.errstate(invalid="ignore"):
        lead = np.where(np.isfinite(best), best - second, np.inf)       # a winner in the lowest class ties everything: exact
        fragile |= (best != second) & (lead <= eps * np.maximum(1.0, np.abs(best)))
    fragile |= np.isfinite(best) & (best < LOG_POW_SUBNORMAL)
    near = (raw < LOG_POW_ZERO) & (raw >= LOG_POW_ZERO * (1.0 + eps))
    fragile |= ~np.isfinite(best) & near.any(axis=-1)
    return tok.astype(np.int64), fragile, ambiguous


def decide(rows, T=1.0, top_p=0.0, top_k=0, rs=None, log_rs=None, eps=EPS, fault=None):
    """rows float32 [B, V] (or [V]) after guidance; the key as ``rs`` or ``log_rs``, one row ([V]) or one per row ([B, V]).
    Returns (token int64 [B], decidable bool [B], ambiguous bool [B]).  ``fault``: one of FAULTS, a planted misreading that the
    tests use on a copy of the decision to show that their rows would notice it."""
    assert fault is None or fault in FAULTS
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float32))
    if np.isnan(rows).any() or not np.isfinite(rows).any(axis=-1).all():
        raise ValueError("NaN logits and rows without a finite entry are outside the reference")
    if not T > 0.0:
        raise ValueError("temp <= 0 is the greedy leg: use greedy()")
    x32 = rows if fault == "temperature_after_softmax" else scale_by_temperature(rows, T)
    x = x32.astype(np.float64)
    if (rs is None) == (log_rs is None):
        raise ValueError("give rs or log_rs")
    with np.errstate(divide="ignore"):
        lr = np.log(np.asarray(rs).astype(np.float64)) if log_rs is None else np.asarray(log_rs).astype(np.float64)
    lr = np.broadcast_to(np.atleast_2d(lr), x.shape)
    top_p, top_k = float(top_p), int(top_k)
    tok, fragile, ambiguous = _pass(x, lr, top_p, top_k, eps, fault=fault, T=T)
    if top_p > 0.0 and not (fault == "top_k_first" and top_k > 0):
        for shift in (-eps, eps):
            fragile |= _pass(x, lr, top_p, top_k, eps, p_shift=shift, fault=fault, T=T)[0] != tok
    return tok, ~fragile, ambiguous


def key_rows(hashes, V):
    """rs of engine.py:65-66 for window hashes int64 [B]: torch.rand(V) of the CPU generator seeded with each -> float32 [B, V]."""
    import torch
    g = torch.Generator(device="cpu")
    out = np.empty((len(hashes), V), dtype=np.float32)
    for b, h in enumerate(hashes):
        g.manual_seed(int(h))
        out[b] = torch.rand(V, generator=g).numpy()
    return out


_BULK = {}


def bulk_chunk(c):
    """Chunk c of tests/golden/bulk_inputs.gumbel_bulk_rows as numpy: (logits [B, V], hashes [B], rs [B, V], (T, top_p, top_k))."""
    import os
    import sys
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if golden not in sys.path:
        sys.path.insert(0, golden)
    from bulk_inputs import gumbel_bulk_rows
    lg, h, setting = gumbel_bulk_rows(c)
    return lg.numpy(), h.numpy(), key_rows(h.numpy(), lg.shape[1]), setting


def bulk_decisions():
    """``decide`` over every bulk chunk, once per process: (token, decidable, ambiguous), each [chunks, rows]."""
    if "all" not in _BULK:
        bulk_chunk(0)
        from bulk_inputs import GUM_BULK_CHUNKS
        out = []
        for c in range(GUM_BULK_CHUNKS):
            lg, _, rs, (T, top_p, top_k) = bulk_chunk(c)
            out.append(decide(lg, T, top_p, top_k, rs=rs))
        _BULK["all"] = tuple(np.stack([o[i] for o in out]) for i in range(3))
    return _BULK["all"]


def score(rs, tokens):
    """gumbel_score_tok: -log(1 - rs)[token] in float64 (the reference rounds it to float32, then truncates to int64)."""
    rs = np.asarray(rs, dtype=np.float32)
    return -np.log1p(-rs.astype(np.float64))[..., np.asarray(tokens, dtype=np.int64)]
