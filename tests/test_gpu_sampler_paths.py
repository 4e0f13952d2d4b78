"""Every path of the fused sampler, the logit processor, the Gumbel sampler and the detector through the C ABI, each against
(a) the C oracle, bit for bit, and (c) the float64 restatement of tests/sampler_reference.py, which shares no arithmetic with
either; (b) the exported row against float32 ``biased / T``.

Which case reaches which path (derived from ``launch_sample_fused`` and ``k_sample_fused`` in wmar_amd/csrc/watermark.hip:
EPT/PLAIN from V and the optional streams, the tail from ``EPT > 0 && n_alive <= 1024`` where n_alive counts the keys >= the
top-k threshold and is "unbounded" without top-k, the top-p branch from the row):

  instantiation   reached by
  <16, PLAIN>     test_sample_fused_matrix V <= 16384 (wmar_sample_fused never passes gather / guidance / allow / trace)
  <16>            test_cham_sample allow_ids of length 1, 1000, 1025, 8192 (a.V = n_allow <= 16384, gather + guidance + allow)
  <64>            test_sample_fused_matrix V = 16385 .. 65536; test_cham_sample V = 65536 without ids (allow bitmap only) and
                  with 16385 ids (gather)
  <0>             test_sample_fused_matrix V = 65537, 70001; test_cham_sample V = 70001 without ids and with 65600 ids (gather)

  tail            reached by
  compacted       <16,PLAIN> and <64>: settings with top-k on rows without a wide tie group at the k-th value --
                  (1, 250, .92), (1.3, 1024, .8) [exactly 1024 survivors on the gaussian rows], (.7, 1, .5);
                  test_n_alive_boundary 1024 (every slot used).  <0> has no compacted tail.  <16> non-PLAIN has one, but
                  wmar_cham_sample has no top-k, so only the generation loops reach it (tests/test_gpu_rar.py under guidance)
  general         every setting without top-k; top_k = 1025, 3000; the "zeros" and "plateau" rows under any top-k (the tie
                  group at the k-th value is wider than 1024 from V = 3072 up); test_n_alive_boundary 1025; all of
                  test_cham_sample; everything at V > 65536

  top-p branch    reached by
  all_pass        top_p = 0.0 (threshold 1: every cumulative sum passes) -- general tail in the matrix, compacted tail in
                  test_n_alive_boundary[1024] with top_p = 0.0
  plain boundary  the gaussian / dominant / winner rows under top_p = .92, .8, .95, .5
  boundary in a   "rounded", "zeros", "plateau" rows (compacted: "rounded" under (1, 250, .92); general: "zeros", or any of
  tie group       them without top-k); test_index_tie_break (index bytes 1 and 2 of the boundary non-zero, <64> and <0>)

  ragged V        V = 33, 1000, 1023, 1025, 16383, 16385, 65535, 65537, 70001: inactive lanes of the last sweep, the clamped loads
                  of <16,PLAIN>, the partial last key word (V % 32 != 0) in the fused bias and in k_wm_bias
                  (test_process_logits_more_rows_than_cus)
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cham_oracle as CH  # noqa: E402
from oracle import wm_oracle as W  # noqa: E402
from tests import sampler_reference as R  # noqa: E402
from tests.test_gpu_watermark import _sample_fused  # noqa: E402

DELTA = 2.0
_WM = {}


def _watermark(V, seed, h, delta=DELTA, gamma=0.25):
    """(GentimeWatermark on the device, oracle KeyParams) for an arbitrary vocabulary, built once per module."""
    from wmar_amd.watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
    k = (V, seed, h, delta, gamma)
    if k not in _WM:
        alive = sorted(set(range(0, V, 2)) | set(range(1, V, 4)))
        dead = sorted(set(range(V)) - set(alive))
        vq = {"alive_ids": torch.tensor(alive, dtype=torch.int64), "dead_ids": torch.tensor(dead, dtype=torch.int64), "embedding": None}
        wm = GentimeWatermark(vq, V, SeedStrategy(seed), SplitStrategy.RANDOM_STRATIFIED, h, delta, gamma, device="cuda")
        _WM[k] = (wm, W.KeyParams(alive, dead, V, gamma, split="stratifiedrand", seed=seed, context_size=h))
    return _WM[k]


def _host_table(wm):
    if getattr(wm, "_host_table_cache", None) is None:
        wm._host_table_cache = wm.key_table_host()
    return wm._host_table_cache


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _green_rows(wm, ctx_rows, V):
    """bool [B, V] key rows from the product's own host table builder (checked against the oracle in test_gpu_watermark.py)."""
    tab = _host_table(wm)
    return np.stack([R.bits_to_mask(tab[r], V) for r in ctx_rows])


def _check_rows(tag, got, x_got, rows, q, T, tk, tp, src=None):
    """(a) oracle token, (b) exported row, (c) float64 token and kept set on the decidable rows.  ``rows`` is the float32 row
    the sampler sees (after bias / guidance / allow-list / gather), ``src`` maps its columns to token ids."""
    otok, xs, _ = W.sample_rows(rows, q, T, tk, tp, return_all=True)
    exp = otok if src is None else np.asarray(src)[otok]
    assert got.tolist() == exp.tolist(), (tag, "token != oracle")
    assert np.array_equal(_bits(x_got), _bits(R.divide_by_temperature(rows, T))), (tag, "exported row != float32 biased / T")
    ref = R.sample_reference_rows(rows, q, T, tk, tp)
    rtok = ref[0] if src is None else np.asarray(src)[ref[0]]
    for b in np.nonzero(ref[2])[0]:
        assert got[b] == rtok[b], (tag, int(b), "token != float64 reference", int(got[b]), int(rtok[b]))
        assert R.kept_set_agrees(np.isfinite(xs[b]), ref, b), (tag, int(b), "kept set != float64 reference")
    return int(ref[2].sum())


# ------------------------------------------------------------------------------------------------- wmar_sample_fused
@pytest.mark.parametrize("use_wm", [False, True], ids=["nowm", "wm"])
@pytest.mark.parametrize("V", R.VOCABS)
def test_sample_fused_matrix(V, use_wm):
    """The matrix of tests/sampler_reference.py.  Watermark: LINEAR h = 1 up to V = 20000 (a key row per context token), FIXED
    h = 0 above (one key row; a LINEAR table at 65536 would take 0.5 GB).  <16,PLAIN> / <64> / <0> by V, both tails, ragged V."""
    lg, q = R.matrix_rows(V)
    B = lg.shape[0]
    wm = past = None
    rows = lg
    if use_wm:
        linear = V <= 20000
        wm, key = _watermark(V, "linear" if linear else "fixed", 1 if linear else 0)
        past = np.random.RandomState(V).randint(0, V, size=(B, 3)).astype(np.int64)
        past[0, -1], past[1, -1] = V - 1, 0                                     # the last and the first key row
        rows = W.process_logits(key, past, lg, DELTA)
        green = _green_rows(wm, past[:, -1] if linear else [0] * B, V)
        assert np.array_equal(_bits(R.restate_stages(lg, green=green, delta=DELTA)), _bits(rows)), "float32 bias restatement != oracle"
        if not linear:
            past = None                                                         # FIXED needs no context
    n_dec = n = 0
    for T, tk, tp in R.SETTINGS:
        if tk is not None and tk >= V:
            continue
        got, x = _sample_fused(wm, lg, past, q, T, tk, tp)
        n_dec += _check_rows((V, use_wm, T, tk, tp), got, x, rows, q, T, tk, tp)
        n += B
    print(f"V = {V}: {n_dec} of {n} rows decidable")


def test_sample_fused_more_rows_than_cus():
    V, B = 1000, 300
    rs = np.random.RandomState(300)
    lg = (rs.randn(B, V) * 3).astype(np.float32)
    lg[::7] = np.round(lg[::7])
    q = rs.exponential(size=(B, V)).astype(np.float32)
    past = rs.randint(0, V, size=(B, 2)).astype(np.int64)
    wm, key = _watermark(V, "linear", 1)
    rows = W.process_logits(key, past, lg, DELTA)
    got, x = _sample_fused(wm, lg, past, q, 0.9, 250, 0.92)
    assert _check_rows("B=300", got, x, rows, q, 0.9, 250, 0.92) >= 0.98 * B


def _boundary_rows(n_ge, B=4, V=16384):
    """Rows with 900 distinct values above a tie group at 5.0 that is sized so that exactly ``n_ge`` entries are >= 5.0, the
    1000th largest value; everything else is below 4."""
    rs = np.random.RandomState(n_ge)
    lg = np.minimum(rs.randn(B, V) * 1.5, 3.9).astype(np.float32)
    for b in range(B):
        pos = rs.permutation(V)[:n_ge]
        lg[b, pos[:900]] = (5.5 + 3.0 * rs.rand(900)).astype(np.float32)
        lg[b, pos[900:]] = 5.0
    return lg, rs.exponential(size=(B, V)).astype(np.float32)


@pytest.mark.parametrize("top_p", [0.9, 0.0])
@pytest.mark.parametrize("n_ge", [1024, 1025])
def test_n_alive_boundary(n_ge, top_p):
    """top_k = 1000 at V = 16384 with exactly 1024 (compacted tail, every slot used) / 1025 (general tail) entries >= the k-th
    value; top_p = 0.0 adds the all_pass exit of each tail."""
    lg, q = _boundary_rows(n_ge)
    assert all(int((r >= np.partition(r, -1000)[-1000]).sum()) == n_ge for r in lg)
    got, x = _sample_fused(None, lg, None, q, 1.0, 1000, top_p)
    _check_rows((n_ge, top_p), got, x, lg, q, 1.0, 1000, top_p)


def _tie_rows(V, lo, hi, cuts):
    """One row per entry of ``cuts``: a tie group of zeros at indices lo .. hi - 1, fifty entries at 3.0 below ``lo``, -inf
    elsewhere, and a top_p (one per row, returned) whose cut falls inside the group so that index ``cut`` is the first one
    kept (the removed mass ends half an entry before it).  The noise has one tiny value three entries above the cut (kept: the
    winner) and a tinier one three entries below (removed: it wins if the cut is misplaced by more than three entries)."""
    rows, qs, tps = [], [], []
    rs = np.random.RandomState(V + lo)
    for cut in cuts:
        r = np.full(V, -np.inf, dtype=np.float32)
        r[lo:hi] = 0.0
        r[rs.permutation(lo)[:50]] = 3.0
        mass = (hi - lo) + 50 * np.exp(3.0)
        tps.append(1.0 - (cut - lo - 0.5) / mass)
        qq = (0.5 + rs.exponential(size=V)).astype(np.float32)
        qq[cut + 3], qq[cut - 3] = 1e-4, 1e-6
        rows.append(r)
        qs.append(qq)
    return np.stack(rows), np.stack(qs), tps


@pytest.mark.parametrize("V,lo,hi,cuts", [(70001, 65000, 67000, (65400, 65536, 65791, 66048, 66900)),
                                          (65536, 60000, 65536, (60160, 65024, 65279, 65280, 65500))],
                         ids=["V70001_<0>", "V65536_<64>"])
def test_index_tie_break(V, lo, hi, cuts):
    """The top-p cut inside a tie group, at indices whose second and third bytes are non-zero and next to 255/256 steps of
    the low byte: the four index-radix passes of the general tail (<0> and <64>)."""
    rows, q, tps = _tie_rows(V, lo, hi, cuts)
    for b, (cut, tp) in enumerate(zip(cuts, tps)):
        got, x = _sample_fused(None, rows[b:b + 1], None, q[b:b + 1], 1.0, None, tp)
        ref = R.sample_reference(rows[b], q[b], 1.0, None, tp)
        assert ref[2] and ref[0] == cut + 3 and abs(int(np.nonzero(ref[1])[0][np.nonzero(ref[1])[0] >= lo].min()) - cut) <= 1
        _check_rows((V, cut), got, x, rows[b:b + 1], q[b:b + 1], 1.0, None, tp)
        assert got[0] == cut + 3


# -------------------------------------------------------------------------------------------------- wmar_cham_sample
def _cham_sample(wm, lg3, past, T, tp, g_text, g_image, allow_words, ids, q, V):
    from wmar_amd import _lib
    B = lg3.shape[0] // 3
    d_lg = torch.from_numpy(lg3).cuda()
    d_q = torch.from_numpy(q).cuda()
    d_allow = torch.from_numpy(allow_words.view(np.int32)).cuda()
    d_ids = torch.from_numpy(ids.astype(np.int32)).cuda() if ids is not None else None
    d_past = torch.from_numpy(past).cuda() if past is not None else None
    out = torch.empty(B, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(B, V, device="cuda")
    ctx = wm.wm_ctx() if wm is not None else None
    _lib.check(_lib.load().wmar_cham_sample(
        C.byref(ctx) if ctx is not None else None, d_lg.data_ptr(), B, V, d_past.data_ptr() if d_past is not None else None,
        past.shape[1] if past is not None else 0, past.shape[1] if past is not None else 0, float(T), float(tp), float(g_text),
        float(g_image), d_allow.data_ptr(), d_ids.data_ptr() if d_ids is not None else None, len(ids) if ids is not None else 0,
        d_q.data_ptr(), scratch.data_ptr(), out.data_ptr(), _lib.stream_ptr()))
    n = len(ids) if ids is not None else V
    return out.cpu().numpy(), scratch.cpu().numpy().reshape(-1)[: B * n].reshape(B, n)


@pytest.mark.parametrize("use_wm", [False, True], ids=["nowm", "wm"])
@pytest.mark.parametrize("V,n_ids", [(65536, 0), (65536, 1), (65536, 1000), (65536, 1025), (65536, 8192), (65536, 16385), (70001, 0),
                                     (70001, 65600)])
def test_cham_sample(V, n_ids, use_wm):
    """Three DIFFERENT streams -> three-way guidance -> FIXED watermark (the bias follows the SOURCE id under gather) -> allow
    bitmap -> gather -> temperature -> top-p -> race, in one launch.  n_ids = 0: no gather, a bitmap of 30000 ids."""
    B, T, tp, g_text, g_image = 4, 0.9, 0.9, 3.0, 1.2
    rs = np.random.RandomState(V + n_ids)
    lg3 = (rs.randn(3 * B, V) * 2).astype(np.float32)
    lg3[B:2 * B] += (rs.randn(B, V) * 0.5).astype(np.float32)
    q = rs.exponential(size=(B, V)).astype(np.float32)
    ids = np.sort(rs.choice(V, size=n_ids if n_ids else 30000, replace=False)).astype(np.int64)
    if n_ids > 1:
        ids[-1] = V - 1                                                         # the last source id, in the partial key / allow word
        ids = np.unique(ids)
        n_ids = len(ids)
    allow = np.zeros(V, dtype=bool)
    allow[ids] = True
    words = np.zeros((V + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    wm = key = green = None
    if use_wm:
        wm, key = _watermark(V, "fixed", 0)
        green = _green_rows(wm, [0] * B, V)
    otok, olg = CH.sample_step(torch.from_numpy(lg3), q, T, tp, g_text, g_image, allow_ids=ids, key=key,
                               past_ids=np.zeros((B, 1), dtype=np.int64), delta=DELTA)
    full = R.restate_stages(lg3[:B], img=lg3[B:2 * B], uncond=lg3[2 * B:], g_text=g_text, g_image=g_image, green=green, delta=DELTA,
                            allow=allow)
    assert np.array_equal(_bits(full), _bits(olg)), "float32 restatement of guidance / bias / allow-list != oracle"
    gather = ids if n_ids else None
    rows = full[:, ids] if n_ids else full
    assert np.array_equal(_bits(rows), _bits(R.restate_stages(lg3[:B], img=lg3[B:2 * B], uncond=lg3[2 * B:], g_text=g_text,
                                                             g_image=g_image, green=green, delta=DELTA, allow=allow, gather=gather)))
    got, x = _cham_sample(wm, lg3, None, T, tp, g_text, g_image, words, gather, q, V)
    assert got.tolist() == otok.tolist(), "token != cham_oracle.sample_step"
    _check_rows((V, n_ids, use_wm), got, x, rows, q[:, ids] if n_ids else q, T, None, tp, src=ids if n_ids else None)


# ---------------------------------------------------------------------------------------------- wmar_wm_process_logits
@pytest.mark.parametrize("V", [33, 1000, 16385])
def test_process_logits_more_rows_than_cus(V):
    B = 300
    rs = np.random.RandomState(V)
    lg = rs.randn(B, V).astype(np.float32)
    for h, ts in ((1, (1, 3)), (2, (1, 2, 5))):                                 # h = 2, t = 1: every row's context is too short
        wm, key = _watermark(V, "linear", h, delta=1.5)
        for t in ts:
            past = rs.randint(0, V, size=(B, t)).astype(np.int64)
            past[0], past[1] = V - 1, 0
            got = wm._process_logits(torch.from_numpy(past).cuda(), torch.from_numpy(lg).clone().cuda()).cpu().numpy()
            exp = W.process_logits(key, past, lg, 1.5)
            assert np.array_equal(_bits(got), _bits(exp)), (V, h, t)
            assert (t < h) == np.array_equal(_bits(got), _bits(lg))
            if t >= h:
                green = _green_rows(wm, past[:, -h:].sum(1), V)
                assert np.array_equal(_bits(R.restate_stages(lg, green=green, delta=1.5)), _bits(got))


# ------------------------------------------------------------------------------------------------- wmar_gumbel_sample
SIGNED_ZERO_ROW = np.array([-0.0, -3, -3, -3, -3, 0.0] + [-3] * 58, dtype=np.float32)


@pytest.mark.parametrize("V", [1, 37, 64, 1025, 16383])
def test_gumbel_paths(V):
    from wmar_amd.watermarking.gumbel_watermark import gumbel_sample
    rs = np.random.RandomState(V)
    lg = (rs.randn(6, V) * 4).astype(np.float32)
    lg[1] = np.round(lg[1])
    lg[2] = 0.0
    lg[3] = 0.0
    lg[3, V // 2:] = -0.0                                                       # the maximum is shared by both zeros: index 0 wins
    if V == 64:
        lg[0] = SIGNED_ZERO_ROW
    h = torch.from_numpy(rs.randint(0, 2 ** 31, size=6).astype(np.int64))
    d = torch.from_numpy(lg).cuda()
    got = gumbel_sample(d, h, use_sampling=False).cpu().numpy()
    assert got.tolist() == W.gumbel_sample(lg, h.numpy(), False).tolist()
    assert got.tolist() == np.argmax(lg.astype(np.float64), axis=1).tolist()           # first index of the maximum, -0.0 == +0.0
    if V == 64:
        assert got[0] == 0
    for temp, top_p, top_k in [(1.0, 0.0, 0), (0.6, 0.0, 0), (1.0, 0.3, 0), (1.3, 0.95, 0), (1.0, 0.0, 7)]:
        got = gumbel_sample(d, h, True, temp, top_p, top_k).cpu().numpy()
        assert got.tolist() == W.gumbel_sample(lg, h.numpy(), True, temp, top_p, top_k).tolist(), (temp, top_p, top_k)


def test_signed_zero_rows_on_the_device():
    """The rows of tests/test_sampler_reference.py's signed-zero tests, through the kernels: tokens 0, 0 and 2 (torch's)."""
    row = np.array([-0.0] * 10 + [0.0] * 10 + [-5.0] * 44, dtype=np.float32)[None]
    q = np.ones((1, 64), dtype=np.float32)
    q[0, 0] = 1e-3
    got, x = _sample_fused(None, row, None, q, 1.0, 5, None)
    assert got[0] == 0 and np.array_equal(_bits(x), _bits(row))
    _check_rows("top-k zeros", got, x, row, q, 1.0, 5, None)
    row = np.array([[0.0, -0.0, 0.0, -0.0]], dtype=np.float32)
    q = np.array([[1e-3, 1.0, 1e-2, 1.0]], dtype=np.float32)
    got, x = _sample_fused(None, row, None, q, 1.0, None, 0.5)
    assert got[0] == 2 and np.array_equal(_bits(x), _bits(row))
    _check_rows("top-p zeros", got, x, row, q, 1.0, None, 0.5)


# ------------------------------------------------------------------------------------------------------------ detector
def _detect_case(wm, key, codes):
    codes = np.ascontiguousarray(codes, dtype=np.int64)
    pv, ns, ng, masks = wm.detect_counts(torch.from_numpy(codes).cuda(), return_masks=True)
    epv, ens, eng, emasks = W.detect(key, codes, return_masks=True)
    pv = pv.cpu().numpy()
    assert ns.cpu().numpy().tolist() == ens.tolist() and ng.cpu().numpy().tolist() == eng.tolist()
    assert [m[:len(r)] for m, r in zip(masks.cpu().tolist(), emasks)] == emasks
    for a, b in zip(pv, epv):
        if np.isnan(b):
            assert np.isnan(a)
        elif b == 0.0:
            assert a == 0.0
        else:
            assert abs(np.log10(a) - np.log10(b)) < 1e-9, (a, b)
    return pv, ens, eng


def _coloured(tab, V, h, L, green, rs):
    """A passage whose every target is green (or red) under the key row of the h tokens before it."""
    codes = list(rs.randint(0, V, size=h))
    for i in range(h, L):
        bits = R.bits_to_mask(tab[sum(codes[i - h:i])], V)
        codes.append(int(rs.choice(np.nonzero(bits == green)[0])))
    return codes


@pytest.mark.parametrize("h", [1, 2, 16])
def test_detector_linear_edges(h):
    V = 512
    wm, key = _watermark(V, "linear", h, delta=1.5)
    rs = np.random.RandomState(h)
    for L in (h + 1, 2 * h + 1):                                                # one n-gram; h + 1 n-grams
        _, ns, _ = _detect_case(wm, key, rs.randint(0, V, size=(3, L)))
        assert ns.max() <= L - h
    _, ns, _ = _detect_case(wm, key, np.full((2, 1024), 77))                    # one repeated n-gram: scored once
    assert ns.tolist() == [1, 1]
    tab = _host_table(wm)
    pv, ns, ng = _detect_case(wm, key, [_coloured(tab, V, h, 1024, True, rs)])
    assert ng[0] == ns[0] > 900 and pv[0] == 0.0                                # 0.25 ** 900 underflows
    pv, ns, ng = _detect_case(wm, key, [_coloured(tab, V, h, 1024, False, rs)])
    assert ng[0] == 0 and ns[0] > 900 and np.isnan(pv[0])


@pytest.mark.parametrize("h", [1, 3])
def test_detector_spatial_grids(h):
    V = 512
    wm, key = _watermark(V, "spatial", h, delta=1.5)
    rs = np.random.RandomState(10 + h)
    for L in (16, 1024):
        codes = rs.randint(0, V, size=(3, L))
        codes[1] = rs.randint(0, 3, size=L)                                     # heavy repetition
        codes[2, -1] = V - 1
        _detect_case(wm, key, codes)


def test_detector_fixed_h0_and_small_vocabulary():
    wm, key = _watermark(512, "fixed", 0, delta=1.5)
    rs = np.random.RandomState(20)
    _detect_case(wm, key, rs.randint(0, 512, size=(4, 1)))                      # L = 1: a single unigram
    _, ns, _ = _detect_case(wm, key, rs.choice([3, 4, 5, 500, 511], size=(3, 300)))
    assert ns.tolist() == [5, 5, 5]
    wm, key = _watermark(1000, "linear", 1, delta=1.5)
    codes = rs.randint(0, 1000, size=(3, 64))
    codes[0, ::5] = 999
    codes[1, -1] = codes[2, 0] = 999
    _detect_case(wm, key, codes)
