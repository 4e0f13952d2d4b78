"""k_gumbel_sample against the float64 restatement tests/gumbel_reference.py and the reference's recorded tokens
(tests/golden/gumbel_bulk.npz), through wmar_gumbel_sample and the probe entry wmar_gumbel_probe_sample (the decode loop's
argument set: unconditional logits, a device scale table, device step / length counters, strided token rows, past_append).

The key goes in as log_rs rows: derived from window hashes on the device for the bulk rows (as the product does), given
directly for the constructed rows, where float64 takes the same row."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gumbel_reference as G  # noqa: E402
from tests.conftest import REPO  # noqa: E402
from tests.test_gumbel_reference import oracle_rows  # noqa: E402

G.bulk_chunk(0)                                     # puts tests/golden on the path
from bulk_inputs import GUM_BULK_CHUNKS, GUM_BULK_KINDS, GUM_BULK_ROWS, gumbel_bulk_case  # noqa: E402

SENTINEL = -777
NEG_INF = np.float32(-np.inf)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def sample(lg, log_rs, T=1.0, top_p=0.0, top_k=0, use_sampling=1):
    """wmar_gumbel_sample with the key as log_rs ([V]: shared, stride 0; [B, V]: one row each)."""
    from wmar_amd import _lib
    lg_d, lr_d = _dev(lg, np.float32), _dev(log_rs, np.float32)
    B, V = lg_d.shape
    out = torch.full((B,), SENTINEL, dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().wmar_gumbel_sample(lg_d.data_ptr(), B, V, lr_d.data_ptr(), V if lr_d.dim() == 2 else 0, int(use_sampling),
                                              float(T), float(top_p), int(top_k), out.data_ptr(), _lib.stream_ptr(lg_d.device)))
    return out.cpu().numpy()


def probe(lg, log_rs, T=1.0, top_p=0.0, top_k=0, use_sampling=1, uncond=None, table=None, step=None, t=None, tok_stride=1,
          past_stride=0, raw=False):
    """wmar_gumbel_probe_sample.  Returns (tok_out [B, tok_stride], past [B, past_stride] or None), both filled with SENTINEL
    first; ``raw``: the status code instead of an exception."""
    from wmar_amd import _lib
    lg_d, lr_d = _dev(lg, np.float32), _dev(log_rs, np.float32)
    B, V = lg_d.shape
    un_d = _dev(uncond, np.float32) if uncond is not None else None
    tb_d = _dev(table, np.float32) if table is not None else None
    st_d = _dev([step], np.int32) if step is not None else None
    t_d = _dev([t], np.int32) if t is not None else None
    tok = torch.full((B, tok_stride), SENTINEL, dtype=torch.int64, device="cuda")
    past = torch.full((B, past_stride), SENTINEL, dtype=torch.int64, device="cuda") if past_stride else None
    ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    rc = _lib.load().wmar_gumbel_probe_sample(lg_d.data_ptr(), ptr(un_d), ptr(tb_d), len(table) if table is not None else 1, ptr(st_d),
                                              ptr(t_d), B, V, lr_d.data_ptr(), V if lr_d.dim() == 2 else 0, int(use_sampling), float(T),
                                              float(top_p), int(top_k), tok.data_ptr(), tok_stride, ptr(past), past_stride,
                                              _lib.stream_ptr(lg_d.device))
    if raw:
        torch.cuda.synchronize()
        return rc, tok.cpu().numpy(), None if past is None else past.cpu().numpy()
    _lib.check(rc)
    return tok.cpu().numpy(), None if past is None else past.cpu().numpy()


def log_key(rs):
    """(float) log((double) rs): what wmar_gumbel_key_build hands the kernel."""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(rs, dtype=np.float32).astype(np.float64)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ bulk rows
@pytest.fixture(scope="module")
def bulk():
    """(float64 token, decidable, ambiguous, reference token, oracle token, kernel token), each [chunks, rows]."""
    from wmar_amd.watermarking.gumbel_watermark import gumbel_sample
    tok, dec, amb = G.bulk_decisions()
    ref = np.load(os.path.join(REPO, "tests", "golden", "gumbel_bulk.npz"))["tokens"].astype(np.int64)
    orc, got = np.zeros_like(tok), np.zeros_like(tok)
    for c in range(GUM_BULK_CHUNKS):
        lg, h, rs, (T, top_p, top_k) = G.bulk_chunk(c)
        orc[c] = oracle_rows(lg, rs, T, top_p, top_k)
        got[c] = gumbel_sample(torch.from_numpy(lg).cuda(), torch.from_numpy(h), True, T, top_p, top_k).cpu().numpy()
    return tok, dec, amb, ref, orc, got


@pytest.mark.parametrize("kind", GUM_BULK_KINDS)
def test_bulk_rows(bulk, kind):
    tok, dec, amb, ref, orc, got = bulk
    rows = np.array([gumbel_bulk_case(c)[2] == kind for c in range(GUM_BULK_CHUNKS)])[:, None] & np.ones_like(dec)
    assert rows.sum() == GUM_BULK_CHUNKS // len(GUM_BULK_KINDS) * GUM_BULK_ROWS
    assert np.array_equal(got[rows], orc[rows])                                  # the first link, undecidable rows included
    bad = np.argwhere(rows & dec & (got != tok))                                  # ambiguous rows included: the index rule
    assert len(bad) == 0, [(int(c), int(b), gumbel_bulk_case(c)) for c, b in bad[:8]]
    bad = np.argwhere(rows & dec & ~amb & (got != ref))
    assert len(bad) == 0, [(int(c), int(b), gumbel_bulk_case(c)) for c, b in bad[:8]]
    print(f"{kind}: {int((rows & dec).sum())} decidable rows, {int((rows & dec & amb).sum())} of them ambiguous in the reference, "
          f"which gave another token on {int((rows & dec & amb & (got != ref)).sum())}")


# ---------------------------------------------------------------------------------------------------------- ragged sizes
RAGGED_SETTINGS = ((1.0, 0.0, 0), (0.8, 0.9, 0), (1.0, 0.0, 7))


@pytest.mark.parametrize("V", [1, 37, 63, 64, 65, 1000, 1023, 1024, 1025, 2047, 2049, 16383, 16384])
def test_ragged_sizes(V):
    """The 1024-thread x 16-element layout and its tails; 1, 5 and 64 rows; one shared key (stride 0) and one key per row."""
    from wmar_amd.watermarking.gumbel_watermark import key_for, key_rows
    r = np.random.RandomState(4000 + V)
    lg = (r.randn(64, V) * 3).astype(np.float32)
    hashes = r.randint(0, 2 ** 31 - 1, size=64).astype(np.int64)
    rs_rows = G.key_rows(hashes, V)                                               # torch.rand on the host
    lr_rows = key_rows(torch.from_numpy(hashes), V, "cuda", (False, True, False))[1].cpu().numpy()
    lr_one = key_for(int(hashes[0]), V, "cuda")[1].cpu().numpy()
    n = 0
    for T, top_p, top_k in RAGGED_SETTINGS:
        for lr, rs in ((lr_one, rs_rows[0]), (lr_rows, rs_rows)):
            tok, dec, _ = G.decide(lg, T, top_p, top_k, rs=rs)
            orc = oracle_rows(lg, rs, T, top_p, top_k)
            for B in (1, 5, 64):
                got = sample(lg[:B], lr if lr.ndim == 1 else lr[:B], T, top_p, top_k)
                assert np.array_equal(got, orc[:B]), (T, top_p, top_k, B, lr.ndim)
                assert np.array_equal(got[dec[:B]], tok[:B][dec[:B]]), (T, top_p, top_k, B, lr.ndim)
                got2, _ = probe(lg[:B], lr if lr.ndim == 1 else lr[:B], T, top_p, top_k)
                assert np.array_equal(got2[:, 0], got)
            n += int(dec.sum())
    assert n >= 0.9 * 64 * 2 * len(RAGGED_SETTINGS)


def test_vocabulary_above_16384_is_refused():
    from wmar_amd import _lib
    lg = np.zeros((2, 16385), dtype=np.float32)
    lr = np.full(16385, -1.0, dtype=np.float32)
    with pytest.raises(_lib.WmarError) as e:
        sample(lg, lr)
    assert e.value.code == -1
    rc, tok, _ = probe(lg, lr, raw=True)
    assert rc == -1 and (tok == SENTINEL).all()                                   # nothing was launched
    lg_d, lr_d = _dev(lg, np.float32), _dev(lr, np.float32)
    out = torch.full((2,), SENTINEL, dtype=torch.int64, device="cuda")
    rc = _lib.load().wmar_gumbel_sample(lg_d.data_ptr(), 2, 16385, lr_d.data_ptr(), 0, 1, 1.0, 0.0, 0, out.data_ptr(),
                                        _lib.stream_ptr(out.device))
    torch.cuda.synchronize()
    assert rc == -1 and (out.cpu().numpy() == SENTINEL).all()


# --------------------------------------------------------------------------------------------------- constructed key rows
CV = 2049          # two elements on thread 0, one on every other


def _constructed():
    """name -> (logits [V], log_rs [V], [(T, top_p, top_k), ...])."""
    r = np.random.RandomState(99)
    V = CV
    plain = (r.randn(V) * 2).astype(np.float32)
    key = log_key(r.rand(V).astype(np.float32) * 0.999 + 0.0005)
    three = [(1.0, 0.0, 0), (0.9, 0.9, 0), (1.0, 0.0, 7)]
    out = {}
    out["all_neg_inf"] = (plain, np.full(V, NEG_INF), three)
    out["wholly_underflowed"] = (plain, np.full(V, -150.0, dtype=np.float32), three)
    lr = np.full(V, NEG_INF)
    lr[int(np.argsort(-plain)[3])] = -0.5                                         # a likely entry: kept by every cut of `three`
    out["one_finite"] = (plain, lr, three)
    lr = np.full(V, NEG_INF)
    lr[int(np.argsort(-plain)[600])] = -0.5                                       # an unlikely one: behind both cuts
    out["one_finite_cut_away"] = (plain, lr, three)
    lg = plain.copy()
    lg[V - 1] = plain.max() + np.float32(0.5)
    lr = np.full(V, NEG_INF)
    lr[V - 1] = -0.3
    out["survivor_last"] = (lg, lr, three)
    lg = (plain * 3).astype(np.float32)
    lr = key.copy()
    order = np.argsort(-lg, kind="stable")
    p = np.exp(lg[order].astype(np.float64) - lg.max())
    assert np.cumsum(p / p.sum())[38] > 0.6                                       # rank 40 onwards lies behind a 0.5 cut
    lr[order[40::2]] = np.float32(-0.0)
    lr[order[41::2]] = NEG_INF
    out["zero_p_behind_cut"] = (lg, lr, [(1.0, 0.5, 0), (0.7, 0.3, 0)])
    lg = np.where(np.arange(V) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    out["signed_zero_logits"] = (lg, key, [(1.0, 0.0, 0), (1.0, 0.3, 0), (1.0, 0.0, 7), (0.7, 1.0, 0)])
    out["all_equal"] = (np.full(V, 1.5, dtype=np.float32), key,
                        [(1.0, 0.3, 0), (1.0, 1.0, 0), (1.0, 0.0, 7), (1.0, 0.0, V), (1.0, 0.0, 10 ** 6)])
    # a tie group across the cut: three entries above, ten equal ones of which the index rule keeps the first few; the LAST of the
    # ten holds a key that wins wherever it is kept
    lg = (-np.abs(plain) - 1.0).astype(np.float32)
    tied = np.sort(r.choice(V, 13, replace=False))
    lg[tied[:3]] = 6.0
    lg[tied[3:]] = 5.0
    lr = key.copy()
    lr[tied[-1]] = -1e-4
    out["tie_group_across_cut"] = (lg, lr, [(1.0, 0.0, 7), (1.0, 0.6, 0), (1.0, 0.0, 12), (1.0, 0.0, 13)])
    return out


CONSTRUCTED = _constructed()


@pytest.mark.parametrize("name", sorted(CONSTRUCTED))
def test_constructed_key_rows(name):
    lg, lr, settings = CONSTRUCTED[name]
    # the same row three times: a batch exercises the shared key, and the per-row form must not differ
    for T, top_p, top_k in settings:
        tok, dec, amb = G.decide(lg, T, top_p, top_k, log_rs=lr)
        assert dec[0], (name, T, top_p, top_k)                                    # the rows are built to be decidable
        got = sample(np.stack([lg] * 3), lr, T, top_p, top_k)
        assert (got == tok[0]).all(), (name, T, top_p, top_k, got, tok)
        got = sample(np.stack([lg] * 3), np.stack([lr] * 3), T, top_p, top_k)
        assert (got == tok[0]).all(), (name, T, top_p, top_k, got, tok)
        if name == "tie_group_across_cut" and top_k in (0, 7, 12):
            assert amb[0]
    if name == "tie_group_across_cut":
        last = int(np.nonzero(lg == 5.0)[0][-1])
        assert G.decide(lg, 1.0, 0.0, 13, log_rs=lr)[0][0] == last                # kept whole, the planted key wins ...
        assert G.decide(lg, 1.0, 0.0, 12, log_rs=lr)[0][0] != last                # ... and the index rule cuts it away first
    if name == "signed_zero_logits":
        assert sample(lg[None], lr, use_sampling=0)[0] == 0


# ------------------------------------------------------------------------------------------------ the in-loop argument set
TABLE = np.array([0.0, 7.0, 7.0, 1.0, 7.0, 4.0], dtype=np.float32)               # read at step 0, 3 and 5: scales 0, 1, 4


@pytest.mark.parametrize("step", [0, 3, 5])
def test_in_loop_arguments(step):
    from wmar_amd.watermarking.gumbel_watermark import key_rows
    B, V, L, P = 5, 1025, len(TABLE), 11
    r = np.random.RandomState(700 + step)
    cond = (r.randn(B, V) * 3).astype(np.float32)
    uncond = (r.randn(B, V) * 3).astype(np.float32)
    hashes = r.randint(0, 2 ** 31 - 1, size=B).astype(np.int64)
    rs = G.key_rows(hashes, V)
    lr = key_rows(torch.from_numpy(hashes), V, "cuda", (False, True, False))[1].cpu().numpy()
    mixed = G.mix(cond, uncond, TABLE[step])
    t = step + 4
    for T, top_p, top_k in ((0.9, 0.0, 0), (1.0, 0.9, 0), (1.2, 0.0, 50)):
        tok, past = probe(cond, lr, T, top_p, top_k, uncond=uncond, table=TABLE, step=step, t=t, tok_stride=L, past_stride=P)
        plain = sample(mixed, lr, T, top_p, top_k)                                # unguided, on the float32 restatement of the mix
        assert np.array_equal(tok[:, step], plain)
        assert np.array_equal(past[:, t], plain)
        assert (np.delete(tok, step, axis=1) == SENTINEL).all() and (np.delete(past, t, axis=1) == SENTINEL).all()
        ref, dec, _ = G.decide(mixed, T, top_p, top_k, rs=rs)
        assert dec.sum() >= B - 1 and np.array_equal(plain[dec], ref[dec])
        tok2, past2 = probe(cond, lr, T, top_p, top_k, uncond=uncond, table=TABLE, step=step, t=t, tok_stride=L, past_stride=P)
        assert np.array_equal(tok, tok2) and np.array_equal(past, past2)
    # without the unconditional rows the table is not read; without past_append only the token row is written
    tok, past = probe(cond, lr, 0.9, 0.0, 0, step=step, tok_stride=L)
    assert past is None and np.array_equal(tok[:, step], sample(cond, lr, 0.9)) and (np.delete(tok, step, axis=1) == SENTINEL).all()


def test_probe_refuses_counters_outside_its_buffers():
    B, V = 2, 64
    lg, lr = np.zeros((B, V), dtype=np.float32), np.full(V, -1.0, dtype=np.float32)
    for kw in (dict(step=6, tok_stride=6), dict(step=-1, tok_stride=6), dict(step=0, t=11, tok_stride=6, past_stride=11),
               dict(step=3, tok_stride=6, uncond=lg, table=TABLE[:3])):
        rc, tok, past = probe(lg, lr, raw=True, **kw)
        assert rc == -1 and (tok == SENTINEL).all() and (past is None or (past == SENTINEL).all()), kw


# ------------------------------------------------------------------------------------------------------------ greedy leg
@pytest.mark.parametrize("use_sampling,T", [(0, 0.7), (1, 0.0), (1, -1.0), (0, 0.0)])
def test_greedy_leg(use_sampling, T):
    """torch.argmax of the row as it is: first index of the maximum, no division by the temperature (T = -1 would turn the
    order round, T = 0 would leave infinities and NaN)."""
    V = 2049
    r = np.random.RandomState(5)
    lg = (r.randn(6, V) * 3).astype(np.float32)
    lg[1, [7, 1500, 2048]] = lg[1].max() + np.float32(1.0)                        # a tied maximum: the first index
    lg[2] = np.where(np.arange(V) % 2 == 0, np.float32(-0.0), np.float32(0.0))    # -0.0 first: equal to +0.0, index 0
    lg[3] = -np.abs(lg[3]) - 1.0
    lg[3, [900, 901]] = [-0.0, 0.0]
    lg[4, V - 1] = lg[4].max() + np.float32(1.0)                                  # the maximum at the last index
    lg[5] = 1e-45                                                                 # subnormal rows survive: nothing is scaled
    lg[5, 1033] = 3e-45
    lr = log_key(r.rand(V).astype(np.float32) * 0.99 + 0.005)
    want = G.greedy(lg)
    assert want.tolist()[1:] == [7, 0, 900, V - 1, 1033]
    assert np.array_equal(sample(lg, lr, T, 0.9, 0, use_sampling), want)
    assert np.array_equal(sample(lg, lr, T, 0.0, 5, use_sampling), want)
    # guided: the maximum of the mixed row
    un = (r.randn(6, V) * 3).astype(np.float32)
    tok, _ = probe(lg, lr, T, 0.0, 0, use_sampling, uncond=un, table=TABLE, step=5, tok_stride=6)
    assert np.array_equal(tok[:, 5], G.greedy(G.mix(lg, un, TABLE[5])))
