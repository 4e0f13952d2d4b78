"""CPU proof that the checks of tests/gpt_kernel_reference.py bite: each test plants ONE fault into otherwise correct data -- the
faults a 5e-4 logit gate behind a LayerNorm lets through -- and shows its check failing, and passing on the unmodified reference.
The "kernel outputs" here are numpy simulations built from the layout and decomposition statements of the reference module."""
import numpy as np
import pytest

from tests import gpt_kernel_reference as R

RS = np.random.RandomState


def _ints(rs, shape, lo, hi):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float32)


def _gemm_case(seed, M, Mpad, N, K):
    rs = RS(seed)
    W = _ints(rs, (N, K), -4, 4)
    gamma = (2.0 ** rs.randint(-1, 2, size=K)).astype(np.float32)
    X = _ints(rs, (Mpad, K), -8, 8)
    X[M:] = 3.0e30 * rs.choice([-1.0, 1.0], size=(Mpad - M, K))          # large finite garbage in the padding rows
    return R.fold_gamma(W, gamma), X


def _sim_slabs(Wg, X, ranges, P, shift=0, only=None):
    """what a correct split GEMM leaves in a sentinel-filled buffer of P pieces; shift: slice (s, nt) in `only` starts that many k-blocks late"""
    Mpad, N = X.shape[0], Wg.shape[0]
    out = np.full((P, Mpad, N), R.SENTINEL, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s, per_tile in enumerate(ranges):
            for nt, r in enumerate(per_tile):
                if r is None:
                    continue
                kb0 = r[0] + (shift if only is None or (s, nt) == only else 0)
                ks, cs = slice(kb0 * 8, r[1] * 8), slice(nt * 32, nt * 32 + 32)
                out[s, :, cs] = (X[:, ks].astype(np.float64) @ Wg[cs, ks].astype(np.float64).T).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------------- layouts
def test_layout_maps_round_trip():
    rs = RS(0)
    for MT, K in ((1, 32), (2, 160), (4, 64)):
        X = rs.randn(32 * MT, K).astype(np.float32)
        flat = R.pack_act(X, MT)
        m, k = np.meshgrid(np.arange(32 * MT), np.arange(K), indexing="ij")
        assert np.array_equal(flat[R.act_index(m, k, MT)], X)
        assert np.array_equal(R.unpack_act(flat, MT, K), X)
        P = rs.randn(3, 32 * MT, K).astype(np.float32)
        buf = np.zeros(5 * 32 * MT * K, dtype=np.float32)
        for rm in (False, True):
            assert np.array_equal(R.get_pieces(R.put_pieces(buf, P, MT, rm), 3, MT, K, rm), P)
        h, m_, l = R.unpack_planes(R.pack_planes(X, MT), MT, K) if K % 16 == 0 else (X, 0 * X, 0 * X)
        assert np.array_equal((h.astype(np.float64) + m_ + l).astype(np.float32), X)         # x == h + m + l exactly


def test_pack_statements_match_the_index_formulas_of_the_kernels():
    """each pack_* against a literal per-element transcription of its kernel's index arithmetic"""
    rs = RS(1)
    N, K = 96, 64
    Wg = rs.randn(N, K).astype(np.float32)
    lin = R.pack_linear(Wg).reshape(N // 32, K // 8, 64, 4)
    bx = R.pack_bx(Wg).reshape(N // 32, K // 16, 2, 64, 4)
    for nt, kb, lane, j in [(0, 0, 0, 0), (2, 7, 63, 3), (1, 3, 40, 1), (1, 5, 17, 2)]:
        assert lin[nt, kb, lane, j] == Wg[nt * 32 + (lane & 31), kb * 8 + 4 * (lane >> 5) + j]
    for nt, ku, hf, lane, j in [(0, 0, 0, 0, 0), (2, 3, 1, 63, 3), (1, 2, 0, 45, 2), (1, 1, 1, 9, 1)]:
        assert bx[nt, ku, hf, lane, j] == Wg[nt * 32 + (lane & 31), ku * 16 + 8 * (lane >> 5) + 4 * hf + j]
    W16, W8 = R.pack_fc1x(Wg)
    W16, W8 = W16.reshape(N // 24, K // 16, 64, 4), W8.reshape(N // 24, K // 16, 64, 2)
    for tile in range(N // 24):
        for kk in range(K // 16):
            for lane in range(64):
                for q in range(4):
                    blk = lane >> 4
                    pair = 2 * q + (blk & 1)
                    assert W16[tile, kk, lane, q] == Wg[tile * 24 + (lane & 15), kk * 16 + 8 * (pair >> 2) + (pair & 3) + 4 * (blk >> 1)]
                for g in range(2):
                    blk = lane >> 2
                    pair = blk & 7
                    assert W8[tile, kk, lane, g] == Wg[tile * 24 + 16 + 4 * g + (lane & 3), kk * 16 + 8 * (pair >> 2) + (pair & 3) + 4 * (blk >> 3)]
    # every (column, k) of the weight appears exactly once in W16 + W8
    ids = np.arange(N * K, dtype=np.float32).reshape(N, K)
    a, b = R.pack_fc1x(ids)
    assert np.array_equal(np.sort(np.concatenate([a, b])), ids.reshape(-1))


def test_pack_check_catches_a_swapped_k_pair_and_a_double_rounding():
    rs = RS(2)
    N, K = 96, 32
    W = rs.randn(N, K).astype(np.float32)
    gamma = (1.0 + 0.1 * rs.randn(K)).astype(np.float32)
    Wg = R.fold_gamma(W, gamma)
    W16, W8 = R.pack_fc1x(Wg)
    R.check_pack(W16, R.pack_fc1x(Wg)[0])
    bad = W16.reshape(N // 24, K // 16, 64, 4).copy()
    bad[:, :, :32], bad[:, :, 32:] = bad[:, :, 32:].copy(), bad[:, :, :32].copy()          # lanes of "k" <-> lanes of "k + 4"
    with pytest.raises(AssertionError):
        R.check_pack(bad, W16)
    # the product W * gamma formed in float64 and rounded once more is NOT what the kernel stores... unless it is the same single rounding
    assert np.array_equal(Wg, (W.astype(np.float64) * gamma.astype(np.float64)).astype(np.float32))
    with pytest.raises(AssertionError):
        R.check_pack(R.pack_linear(R.fold_gamma(W, R.bf(gamma))), R.pack_linear(Wg))


def test_decompositions():
    # k_gemm: the slices of a tile tile K; with n_hi on whole rounds of NW * 2 U = 32 k-blocks (24 rounds over 5 = 4, 5, 5, 5, 5)
    KB = 768
    for nt, S_t in ((0, 6), (20, 5)):
        r = [R.gemm_piece_kblocks(KB, 5, 16, nt, s) for s in range(6)]
        live = [x for x in r if x is not None]
        assert len(live) == S_t and live[0][0] == 0 and live[-1][1] == KB and all(a[1] == b[0] for a, b in zip(live, live[1:]))
        assert all((a % 32, b % 32) == (0, 0) for a, b in live)
        for s in range(S_t):
            ws = [R.gemm_wave_kblocks(KB, 5, 16, nt, s, w) for w in range(4)]
            assert ws[0][0] == live[s][0] and ws[-1][1] == live[s][1] and all(a[1] == b[0] for a, b in zip(ws, ws[1:]))
    assert [R.gemm_piece_kblocks(KB, 5, 16, 20, s) for s in range(5)] == [(0, 128), (128, 288), (288, 448), (448, 608), (608, 768)]
    # uneven k-splits (n_embd 160: 20 k-blocks over 2 slices x 4 waves)
    assert [R.gemm_wave_kblocks(20, 2, 0, 0, s, w) for s in range(2) for w in range(4)] == [(0, 2), (2, 5), (5, 7), (7, 10), (10, 12), (12, 15), (15, 17), (17, 20)]
    assert [R.qkvx_kblocks(192, 7, s) for s in (0, 6)] == [(0, 27), (164, 192)]
    assert [R.qkvx_bx_kblocks(192, 7, s) for s in (0, 1, 6)] == [(0, 26), (26, 54), (164, 192)]
    assert R.bx_kblocks(3) == (144, 192)
    # the statistics chunks of every producer tile the features exactly once
    for lists in (R.chunk_lists(192, "resid", nch=12), R.chunk_lists(20, "resid", nch=2), R.chunk_lists(192, "qkvx", S=7),
                  R.chunk_lists(192, "qkvx_bx", S=7, nkeep=4), R.chunk_lists(192, "xr"), R.chunk_lists(272, "resid", nch=17)):
        assert sorted(kb for l in lists for kb in l) == list(range(max(max(l) for l in lists if l) + 1))
    assert (R.attn_chunk_rows(32), R.attn_chunk_rows(64), R.attn_chunk_rows(128)) == (16, 8, 4)
    assert R.attn_lengths(64, 2) == [1, 2, 7, 8, 9, 31, 33, 63, 65, 255, 256]


# ------------------------------------------------------------------------------------------------------------------- split GEMMs
_SPLITS = {
    "k_gemm uneven": (160, lambda: R.gemm_ranges(20, 5, 2)),
    "k_gemm n_hi": (768, lambda: R.gemm_ranges(96, 3, 2, n_hi=1)),
    "k_qkvx": (256, lambda: R.uniform_ranges(4, lambda s: R.qkvx_kblocks(32, 3, s), 3)),
    "k_qkvx_bx": (224, lambda: R.uniform_ranges(4, lambda s: R.qkvx_bx_kblocks(28, 3, s), 3)),
    "k_bx": (768, lambda: R.uniform_ranges(2, R.bx_kblocks, 2)),
}


@pytest.mark.parametrize("name", list(_SPLITS))
def test_exact_gemm_check_catches_a_slice_that_starts_one_k_block_late(name):
    K, mk = _SPLITS[name]
    ranges = mk()
    NT = len(ranges[0])
    Wg, X = _gemm_case(3, 13, 32, 32 * NT, K)
    R.check_gemm_exact(_sim_slabs(Wg, X, ranges, 8), Wg, X, ranges, 13)
    last = len(ranges) - 1
    nt = next(i for i, r in enumerate(ranges[last]) if r is not None)
    with pytest.raises(AssertionError):
        R.check_gemm_exact(_sim_slabs(Wg, X, ranges, 8, shift=1, only=(last, nt)), Wg, X, ranges, 13)


def test_exact_gemm_check_catches_a_written_sentinel_a_leaking_padding_row_and_the_wrong_piece_layout():
    ranges = R.gemm_ranges(96, 3, 2, n_hi=1)
    Wg, X = _gemm_case(4, 33, 64, 96, 768)
    good = _sim_slabs(Wg, X, ranges, 8)
    R.check_gemm_exact(good, Wg, X, ranges, 33)
    bad = good.copy()
    bad[2, :, 32:] = 0.0                                    # tiles at or past n_hi own no third slab
    with pytest.raises(AssertionError):
        R.check_gemm_exact(bad, Wg, X, ranges, 33)
    bad = good.copy()
    bad[3, 50, 7] = 0.0                                     # a piece the plan does not write
    with pytest.raises(AssertionError):
        R.check_gemm_exact(bad, Wg, X, ranges, 33)
    Xs = X.copy()
    Xs[5, 0] = X[5, 0] + np.float32(1e-30) * X[40, 0]       # a padding row's garbage reaches a real row (here: scaled into sight)
    leak = _sim_slabs(Wg, Xs, ranges, 8)
    assert R.diff_bits(leak[:, :33], good[:, :33]) > 0
    with pytest.raises(AssertionError):
        R.check_gemm_exact(leak, Wg, X, ranges, 33)
    # packed pieces read as row-major ones (and the other way round)
    flat = R.put_pieces(np.full(8 * 64 * 96, R.SENTINEL, dtype=np.float32), good[:3], 2, rowmajor=False)
    R.check_gemm_exact(np.concatenate([R.get_pieces(flat, 3, 2, 96, False), good[3:]]), Wg, X, ranges, 33)
    with pytest.raises(AssertionError):
        R.check_gemm_exact(np.concatenate([R.get_pieces(flat, 3, 2, 96, True), good[3:]]), Wg, X, ranges, 33)


def _bx_products(Wg, X, drop=None):
    """the six piece products of the bf16 split (bx_split.h), summed in float64 and rounded once: a faithful stand-in for the kernel"""
    wh, wm, wl = (a.astype(np.float64) for a in R.bx_split(Wg))
    xh, xm, xl = (a.astype(np.float64) for a in R.bx_split(X))
    terms = {"lh": (wl, xh), "hl": (wh, xl), "mm": (wm, xm), "mh": (wm, xh), "hm": (wh, xm), "hh": (wh, xh)}
    return sum(x @ w.T for k, (w, x) in terms.items() if k != drop)


def test_dense_gemm_check_catches_a_dropped_second_order_product():
    rs = RS(5)
    K, N, M = 768, 64, 33
    Wg, X = (rs.randn(N, K) * 0.02).astype(np.float32), rs.randn(64, K).astype(np.float32)
    ranges = R.uniform_ranges(2, R.bx_kblocks, 2)

    def slabs(drop):
        out = np.zeros((2, 64, N), dtype=np.float32)
        for s in range(2):
            ks = slice(s * 384, s * 384 + 384)
            out[s] = _bx_products(Wg[:, ks], X[:, ks], drop).astype(np.float32)
        return out
    e, ec, worst = R.check_gemm_dense(slabs(None), Wg, X, ranges, M)
    assert worst < 1.0
    with pytest.raises(AssertionError):
        R.check_gemm_dense(slabs("mm"), Wg, X, ranges, M)
    # ... and the sequential chain itself sits at 1.0 x by construction
    assert R.check_gemm_dense(R.gemm_chain(Wg, X, ranges), Wg, X, ranges, M)[2] == 1.0


# ------------------------------------------------------------------------------------------------------------------- residual + statistics
def test_resid_check_catches_the_extra_slab_and_the_wrong_order():
    rs = RS(6)
    M, N = 33, 96
    x, bias = rs.randn(64, N).astype(np.float32), rs.randn(N).astype(np.float32)
    slabs = [rs.randn(64, N).astype(np.float32) for _ in range(3)]
    slabs[2][:, 32:] = R.SENTINEL                               # tiles >= n_hi = 1: the short slab carries the sentinel
    good = R.resid_ref(x, bias, slabs, n_hi=1)
    R.check_resid(good, x, bias, slabs, 1, M)
    assert np.isfinite(good).all() and np.abs(good).max() < 100
    with pytest.raises(AssertionError):
        R.check_resid(R.resid_ref(x, bias, slabs, n_hi=0), x, bias, slabs, 1, M)          # adds the slab it does not own
    wrong_order = ((x + bias[None, :]).astype(np.float32) + R.fold_slabs(slabs, 1)).astype(np.float32)
    assert R.diff_bits(wrong_order[:M], good[:M]) > 0
    with pytest.raises(AssertionError):
        R.check_resid(wrong_order, x, bias, slabs, 1, M)


@pytest.mark.parametrize("kind,kw,KB", [("resid", dict(nch=2), 20), ("resid", dict(nch=17), 272), ("qkvx", dict(S=7), 192),
                                       ("qkvx_bx", dict(S=7, nkeep=4), 192), ("xr", {}, 192)])
def test_stats_check_catches_the_neighbouring_row_and_a_missing_k_block(kind, kw, KB):
    rs = RS(7)
    M, Mpad = 13, 32
    chunks = R.chunk_lists(KB, kind, **kw)
    xi = _ints(rs, (Mpad, KB * 8), -8, 8)
    good = R.stats_ref(xi, chunks)
    R.check_stats(good, xi, chunks, M, exact=True)
    with pytest.raises(AssertionError):
        R.check_stats(np.roll(good, 1, axis=1), xi, chunks, M, exact=True)                # row m - 1's sums
    short = [l[:-1] if c == len(chunks) - 1 else l for c, l in enumerate(chunks)]
    with pytest.raises(AssertionError):
        R.check_stats(R.stats_ref(xi, short), xi, chunks, M, exact=True)                  # one k-block too few
    xf = rs.randn(Mpad, KB * 8).astype(np.float32)
    goodf = R.stats_ref(xf, chunks)
    R.check_stats(goodf, xf, chunks, M, exact=False)
    # sums of squares formed in fp32 are far outside K 2^-53 sum x^2
    f32 = goodf.copy()
    f32[:, :, 1] = f32[:, :, 1].astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_stats(f32, xf, chunks, M, exact=False)


def test_fold_vec_check():
    rs = RS(8)
    W, v, b = rs.randn(64, 1536).astype(np.float32), rs.randn(1536).astype(np.float32), rs.randn(64).astype(np.float32)
    lo, hi = R.fold_vec(W, v, b)
    share = R.check_fold_vec(((W.astype(np.float64) @ v.astype(np.float64)) + b).astype(np.float32), lo, hi, "fold")
    assert share < 0.01
    with pytest.raises(AssertionError):
        R.check_fold_vec((W @ v + b).astype(np.float32), lo, hi, "fold")                  # an fp32 accumulation
    with pytest.raises(AssertionError):
        R.check_fold_vec(np.roll(lo, 1), lo, hi, "fold")


# ------------------------------------------------------------------------------------------------------------------- LayerNorm-fused launches
def _onehot_case(seed, M, N, K):
    """one-hot integer weights that hit every k, integer rows of sum exactly 0"""
    rs = RS(seed)
    kn = np.concatenate([rs.permutation(K), rs.randint(0, K, size=max(0, N - K))])[:N]
    W = np.zeros((N, K), dtype=np.float32)
    W[np.arange(N), kn] = _ints(rs, N, 1, 4) * rs.choice([-1.0, 1.0], size=N)
    x = _ints(rs, (M, K), -8, 8)
    x[:, -1] -= x.sum(1)
    x[:, -2] -= x.sum(1)
    assert np.all(x.sum(1) == 0) and np.abs(x).max() < 2 ** 12
    b = rs.randn(N).astype(np.float32)
    return W, x, b


def _fp32_algebra(acc, stats, K, c1, b, rstd_ulps=0):
    mean64 = stats[:, :, 0].sum(0) / K
    var = (stats[:, :, 1].sum(0) / K - mean64 * mean64).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt(var + R.LN_EPS)).astype(np.float32)
    for _ in range(rstd_ulps):
        rstd = np.nextafter(rstd, np.float32(np.inf))
    return (rstd[:, None] * (acc - mean64.astype(np.float32)[:, None] * c1[None, :]) + b[None, :]).astype(np.float32)


def test_ln_onehot_check_holds_for_fp32_evaluations_and_catches_wrong_statistics_and_bias():
    M, N, K = 33, 256, 160
    W, x, b = _onehot_case(9, M, N, K)
    chunks = R.chunk_lists(K // 8, "resid", nch=2)
    stats = R.stats_ref(x, chunks)
    acc = (x.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    c1 = W.sum(1)
    mean, rstd = R.mean_rstd64(stats, K)
    assert np.all(mean == 0)
    for ulps in (0, 1):                                            # rsqrtf may be 1 ulp off: still inside
        worst, _ = R.check_ln_onehot(_fp32_algebra(acc, stats, K, c1, b, ulps), acc, rstd, b, M, "head")
        assert worst < 1.0
    with pytest.raises(AssertionError):                             # 3 ulp is not an rsqrtf any more
        R.check_ln_onehot(_fp32_algebra(acc, stats, K, c1, b, 3), acc, rstd, b, M, "head")
    with pytest.raises(AssertionError):                             # the neighbouring row's statistics
        R.check_ln_onehot(_fp32_algebra(acc, np.roll(stats, 1, axis=1), K, c1, b), acc, rstd, b, M, "head")
    with pytest.raises(AssertionError):                             # one statistics chunk too few
        R.check_ln_onehot(_fp32_algebra(acc, stats[:1], K, c1, b), acc, rstd, b, M, "head")
    with pytest.raises(AssertionError):                             # the bias of the neighbouring column tile
        R.check_ln_onehot(_fp32_algebra(acc, stats, K, c1, np.roll(b, 32)), acc, rstd, b, M, "head")
    # through GELU (exact-erf in float64, rounded once: what a correct kernel is close to)
    pre = _fp32_algebra(acc, stats, K, c1, b)
    R.check_ln_onehot(R.gelu64(pre).astype(np.float32), acc, rstd, b, M, "fc1", gelu=True)
    with pytest.raises(AssertionError):
        R.check_ln_onehot(R.gelu64(_fp32_algebra(acc, stats, K, c1, np.roll(b, 32))).astype(np.float32), acc, rstd, b, M, "fc1", gelu=True)
    tanh = (0.5 * pre * (1 + np.tanh(0.7978845608 * (pre + 0.044715 * pre ** 3)))).astype(np.float32)
    with pytest.raises(AssertionError):                             # the tanh approximation is not the exact-erf GELU
        R.check_ln_onehot(tanh, acc, rstd, b, M, "fc1", gelu=True)


def test_ln_dense_check_catches_c1_of_the_neighbouring_tile():
    rs = RS(10)
    M, N, K = 13, 128, 160
    W, gamma, beta = (rs.randn(N, K) * 0.05).astype(np.float32), (1 + 0.1 * rs.randn(K)).astype(np.float32), (0.1 * rs.randn(K)).astype(np.float32)
    x = (rs.randn(M, K) + 3.0).astype(np.float32)                  # a row mean the c1 term has to remove
    Wg = R.fold_gamma(W, gamma)
    c1 = (W.astype(np.float64) @ gamma.astype(np.float64)).astype(np.float32)
    b = (W.astype(np.float64) @ beta.astype(np.float64)).astype(np.float32)
    stats = R.stats_ref(x, R.chunk_lists(K // 8, "resid", nch=2))
    mean, rstd = R.mean_rstd64(stats, K)
    ref = R.ln_ref64(W, gamma, beta, None, x)
    norm = R.ln_normaliser(Wg, x, mean, rstd, c1, b)
    yard = R.ln_algebra32(Wg, x, stats, c1, b, K)
    e, ey, ratio = R.check_ln_dense(yard, ref, norm, yard, M, "head")
    assert ratio == 1.0 and ey < 2.0 ** -20
    with pytest.raises(AssertionError):
        R.check_ln_dense(R.ln_algebra32(Wg, x, stats, np.roll(c1, 32), b, K), ref, norm, yard, M, "head")


def test_appended_row_check_catches_c1_of_the_neighbouring_tile_and_a_mean_from_one_chunk_too_few():
    """the K / V rows the attention prologue appends, dense data, |mean| of the order of sigma"""
    rs = RS(14)
    M, N, K, S, nch = 13, 192, 256, 3, 4
    P = rs.randn(S, M, N).astype(np.float32)
    c1, b = (rs.randn(N) * 0.8).astype(np.float32), (rs.randn(N) * 0.05).astype(np.float32)
    m_row, v_row = 0.5 + rs.rand(M), 0.5 + rs.rand(M)
    st = np.zeros((nch, M, 2))
    st[:, :, 0], st[:, :, 1] = K / nch * m_row, K / nch * (m_row ** 2 + v_row)
    v, norm, y32 = R.ln_pieces(P, st, c1, b, K)
    assert R.check_ln_dense(y32, v, norm, y32, M, "appended rows")[2] == 1.0
    with pytest.raises(AssertionError):
        R.check_ln_dense(R.ln_pieces(P, st, np.roll(c1, 32), b, K)[2], v, norm, y32, M, "appended rows")
    with pytest.raises(AssertionError):
        R.check_ln_dense(R.ln_pieces(P, st[:3], c1, b, K)[2], v, norm, y32, M, "appended rows")
    with pytest.raises(AssertionError):                                  # a piece left out of the sum
        R.check_ln_dense(R.ln_pieces(P[:2], st, c1, b, K)[2], v, norm, y32, M, "appended rows")


# ------------------------------------------------------------------------------------------------------------------- attention
def _sim_attn(q, Kc, Vc, scale, hd, nwa, skip_chunk=None):
    """softmax(q K^T) V of one (row, head) over chunks of E rows dealt to nwa waves; skip_chunk: that chunk is never visited"""
    E = R.attn_chunk_rows(hd)
    T = Kc.shape[0]
    s = (Kc.astype(np.float64) @ q.astype(np.float64)) * scale
    if skip_chunk is not None:
        s[skip_chunk * E:(skip_chunk + 1) * E] = -np.inf
    w = np.exp(s - s.max())
    return ((w / w.sum()) @ Vc.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("hd,nwa", [(32, 1), (64, 2), (128, 4)])
def test_onehot_attention_check_catches_a_skipped_chunk(hd, nwa):
    rs = RS(11)
    E = R.attn_chunk_rows(hd)
    scale = 1.0 / np.sqrt(hd)
    for T in R.attn_lengths(hd, nwa):
        Vc = rs.randn(T, hd).astype(np.float32)
        for t in range(T):
            Kc = np.zeros((T, hd), dtype=np.float32)
            q = np.zeros(hd, dtype=np.float32)
            q[0], Kc[t, 0] = 40.0, 5.0 * np.sqrt(hd)                 # the winner leads by 200
            R.check_onehot(_sim_attn(q, Kc, Vc, scale, hd, nwa), Vc[t])
            if T > E:                                                # the chunk at a wave / chunk edge that holds the winner is skipped
                with pytest.raises(AssertionError):
                    R.check_onehot(_sim_attn(q, Kc, Vc, scale, hd, nwa, skip_chunk=t // E), Vc[t])
        if T >= 2:                                                   # two equal winners return their mean
            Kc = np.zeros((T, hd), dtype=np.float32)
            Kc[0, 0] = Kc[T - 1, 0] = 5.0 * np.sqrt(hd)
            R.check_onehot(_sim_attn(q, Kc, Vc, scale, hd, nwa), ((Vc[0].astype(np.float64) + Vc[T - 1]) / 2).astype(np.float32), "two winners")


def test_cache_check_catches_a_write_outside_the_appended_rows():
    rs = RS(12)
    H, Tmax, hd, Bmax = 3, 16, 32, 8
    before = rs.randn(Bmax * H * Tmax * hd).astype(np.float32)
    after = before.copy().reshape(Bmax, H, Tmax, hd)
    after[:5, :, 9] = 1.0
    R.check_cache_untouched(after.reshape(-1), before, 5, 9, H, Tmax, hd)
    after[5, 0, 9, 0] = 2.0                                          # a padding sequence's row
    with pytest.raises(AssertionError):
        R.check_cache_untouched(after.reshape(-1), before, 5, 9, H, Tmax, hd)
    assert R.cache_index(2, 1, 9, 4, H, Tmax, hd) == ((2 * H + 1) * Tmax + 9) * hd + 4


def test_dense_attention_check():
    rs = RS(13)
    hd, T = 64, 200
    q, Kc, Vc = (rs.randn(3, hd) * 2).astype(np.float64), rs.randn(3, T, hd), rs.randn(3, T, hd)
    z = np.zeros((3, hd))
    ref, tol = R.attn_dense_bound(q, 2.0 ** -22 * np.abs(q), Kc, z, Vc, z, 0.125, 8, 2)
    y32 = R.attn_fp32(q, Kc, Vc, 0.125)
    assert R.check_attn_dense(y32, ref, tol) < 0.5                      # a plain fp32 evaluation is well inside
    # weights from a fast exponential (exp2 of the rounded scaled argument) and a q that is 2 ulp off: still inside
    s32 = (np.einsum("bd,btd->bt", (q * (1 + 2.0 ** -22)).astype(np.float32), Kc.astype(np.float32)) * np.float32(0.125)).astype(np.float32)
    arg = ((s32 - s32.max(-1, keepdims=True)) * np.float32(1.4426950408889634)).astype(np.float32)
    w = np.exp2(arg.astype(np.float64)).astype(np.float32)
    fast = np.einsum("bt,btd->bd", (w / w.sum(-1, keepdims=True)).astype(np.float32), Vc.astype(np.float32)).astype(np.float32)
    assert R.check_attn_dense(fast, ref, tol) < 1.0
    for b in range(3):
        with pytest.raises(AssertionError):                                  # a skipped chunk of 8 rows
            R.check_attn_dense(_sim_attn(q[b], Kc[b], Vc[b], 0.125, hd, 2, skip_chunk=3)[None], ref[b:b + 1], tol[b:b + 1])
    # the bound follows the decomposition: more waves, fewer additions per lane
    assert np.all(R.attn_dense_bound(q, z, Kc, z, Vc, z, 0.125, 8, 4)[1] <= R.attn_dense_bound(q, z, Kc, z, Vc, z, 0.125, 8, 1)[1])
