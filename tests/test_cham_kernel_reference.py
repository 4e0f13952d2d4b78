"""The Chameleon stage references (tests/cham_kernel_reference.py) on the CPU: the layout maps round-trip, the stream-K piece
ranges tile every group, and every check of tests/test_gpu_cham_kernels.py fails on the fault it is there to catch.  Each test
builds what a correct kernel would leave (the check passes), plants one fault in a copy and shows the check failing."""
import numpy as np
import pytest

from tests import cham_kernel_reference as R
from tests.test_gpu_chameleon_parity import SWEEP, _cham_cfg

RS = np.random.RandomState


def _ints(rs, shape, lim):
    return rs.randint(-lim, lim + 1, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("MT", [1, 2, 3, 4])
def test_layout_maps_round_trip(MT):
    rs = RS(MT)
    X = rs.randn(32 * MT, 48).astype(np.float32)
    flat = R.pack_act(X, MT)
    assert np.array_equal(R.unpack_act(flat, MT, 48), X)
    m, k = np.meshgrid(np.arange(32 * MT), np.arange(48), indexing="ij")
    assert np.array_equal(flat[R.act_index(m, k, MT)], X)
    assert sorted(R.act_index(*np.meshgrid(np.arange(32 * MT), np.arange(48), indexing="ij"), MT).ravel()) == list(range(32 * MT * 48))
    S = rs.randn(32 * MT, 96).astype(np.float32)
    assert np.array_equal(R.unpack_slab(R.pack_slab(S, MT), MT, 96), S)
    m, n = np.meshgrid(np.arange(32 * MT), np.arange(96), indexing="ij")
    assert np.array_equal(R.pack_slab(S, MT)[R.slab_index(m, n, MT)], S)
    assert sorted(R.slab_index(m, n, MT).ravel()) == list(range(32 * MT * 96))
    assert np.array_equal(R.unpack_slab(np.stack([R.pack_slab(S, MT), R.pack_slab(2 * S, MT)]), MT, 96), np.stack([S, 2 * S]))
    Wt = R.bf(rs.randn(64, 32).astype(np.float32))
    assert np.array_equal(R.unpack_weight(R.pack_weight(Wt), 2, 32), Wt)
    assert sorted(R.row_feature(np.arange(32))) == list(range(32))


def test_packed_weight_layout_by_hand():
    """element by element from k_bpack's own index arithmetic"""
    rs = RS(0)
    N, K, Hd = 48, 32, 32
    W, gm = rs.randn(N, K).astype(np.float32), (2.0 ** rs.randint(-2, 3, size=K)).astype(np.float32)
    for mode, n_rows in ((0, N), (1, 2 * Hd)):
        Wm = W if mode == 0 else rs.randn(2 * Hd, K).astype(np.float32)
        bits = R.pack_weight(R.tile_weight(Wm, gm, mode, Hd))
        NT, KB = ((n_rows + 31) // 32, K // 16) if mode == 0 else (Hd // 16, K // 16)
        assert bits.size == NT * 32 * K
        for nt in range(NT):
            for kb in range(KB):
                for lane in range(64):
                    f = int(R.row_feature(lane & 31))
                    row = nt * 32 + f if mode == 0 else (nt * 16 + f if f < 16 else Hd + nt * 16 + f - 16)
                    k0 = kb * 16 + 8 * (lane >> 5)
                    want = R.bf_bits(Wm[row, k0:k0 + 8] * gm[k0:k0 + 8]) if row < n_rows else np.zeros(8, np.uint16)
                    assert np.array_equal(bits[((nt * KB + kb) * 64 + lane) * 8:][:8], want), (mode, nt, kb, lane)


def test_piece_ranges_tile_every_group():
    """the k-blocks of a group's pieces are disjoint, in order, and cover 0..KB-1, at every GEMM of the sweep widths"""
    for shape in SWEEP:
        cfg = _cham_cfg(*shape)
        D, Dkv, F = cfg.dim, cfg.n_kv_heads * cfg.head_dim, cfg.ffn_hidden
        for NT, KB, whole in (((D + 2 * Dkv) // 32, D // 16, False), (D // 32, D // 16, False), (F // 16, D // 16, False),
                              (D // 32, F // 16, False), (cfg.vocab_size // 32, D // 16, True)):
            k = R._sk_for(NT, KB, whole)
            for g in range(R.sk_groups(NT)):
                nxt = 0
                for p in range(R._count(k, g)):
                    a, b = R.piece_kblocks(k, g, p, KB)
                    assert a == nxt and b > a
                    nxt = b
                assert nxt == KB
                if whole:
                    assert R._count(k, g) == 1


def test_bf_candidates():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -8, -3.0 - 2.0 ** -7, 0.0, 255.5])
    lo, hi, und = R.bf_candidates(v, 2.0 ** -24 * np.abs(v))
    assert list(und) == [False, True, True, True, True, False, True]
    assert lo[0] == hi[0] == 1.0 and (lo[1], hi[1]) == (1.0, 1.0 + 2.0 ** -7) and (lo[4], hi[4]) == (-3.0 - 2.0 ** -6, -3.0)
    assert (lo[6], hi[6]) == (255.0, 256.0)
    x = RS(1).randn(4096).astype(np.float32)
    lo, hi, und = R.bf_candidates(x.astype(np.float64), 0.0)
    assert np.array_equal(lo, R.bf(x)) and np.array_equal(hi, R.bf(x))          # float32 inputs: the one-step rounding agrees
    assert np.array_equal(R.bits_f32(R.bf_bits(x)), R.bf(x))


# ------------------------------------------------------------------------------------------------------------------ GEMM pieces
def _gemm_case(seed=0, M=33, MT=2, shape=(320, 5, 1, 1056, 16), dense=False):
    """the w2 GEMM of the narrow sweep width: NT % 4 != 0 and a partial last K chunk"""
    cfg = _cham_cfg(*shape)
    D, F = cfg.dim, cfg.ffn_hidden
    rs = RS(seed)
    k = R._sk_for(D // 32, F // 16, False)
    if dense:
        Wt, X = R.tile_weight(rs.randn(D, F) / F ** 0.5, None), R.bf(rs.randn(32 * MT, F).astype(np.float32))
    else:
        Wt, X = R.tile_weight(_ints(rs, (D, F), 4), None), _ints(rs, (32 * MT, F), 8)
    return Wt, X, k, M, MT


def _slabs_from(pieces64, M, MT):
    """what the launch leaves in a sentinel-filled buffer"""
    got = np.full((R.BG_MAXP, 32 * MT, pieces64.shape[2]), R.SENTINEL, dtype=np.float32)
    used = ~np.isnan(pieces64)
    got[:, :M][used] = pieces64[used].astype(np.float32)
    return got


def test_gemm_exact_catches_piece_faults():
    Wt, X, k, M, MT = _gemm_case()
    KB = Wt.shape[1] // 16
    pieces, _ = R.gemm_pieces(Wt, X[:M], k)
    good = _slabs_from(pieces, M, MT)
    assert R.check_gemm_exact(good, Wt, X, k, M) == 0
    multi = [g for g in range(R.sk_groups(Wt.shape[0] // 32)) if R._count(k, g) > 1]
    assert multi, "the case must split a group"
    g = multi[0]
    c0, c1 = g * 128, min(Wt.shape[0], (g + 1) * 128)
    W64, X64 = Wt.astype(np.float64), X[:M].astype(np.float64)
    # a dropped k-block: the last one of piece 0
    a, b = R.piece_kblocks(k, g, 0, KB)
    ks = slice((b - 1) * 16, b * 16)
    bad = pieces.copy()
    bad[0, :, c0:c1] -= X64[:, ks] @ W64[c0:c1, ks].T
    with pytest.raises(AssertionError):
        R.check_gemm_exact(_slabs_from(bad, M, MT), Wt, X, k, M)
    # a unit given to the neighbouring piece: the group's total is unchanged, the pieces are not
    ks = slice((b - R.BG_KC) * 16, b * 16)
    moved = X64[:, ks] @ W64[c0:c1, ks].T
    assert np.abs(moved).max() > 0
    bad = pieces.copy()
    bad[0, :, c0:c1] -= moved
    bad[1, :, c0:c1] += moved
    assert np.array_equal(np.nansum(bad, 0), np.nansum(pieces, 0))
    with pytest.raises(AssertionError):
        R.check_gemm_exact(_slabs_from(bad, M, MT), Wt, X, k, M)
    # a padding row stored, an unused slot written
    bad = good.copy()
    bad[0, M, 0] = 0.0
    with pytest.raises(AssertionError):
        R.check_gemm_exact(bad, Wt, X, k, M)
    bad = good.copy()
    bad[R._count(k, g), 0, c0] = 1.0
    with pytest.raises(AssertionError):
        R.check_gemm_exact(bad, Wt, X, k, M)


def test_gemm_dense_catches_a_dropped_k_block_and_passes_a_blocked_sum():
    Wt, X, k, M, MT = _gemm_case(seed=3, dense=True)
    KB = Wt.shape[1] // 16
    pieces, _ = R.gemm_pieces(Wt, X[:M], k)
    good = _slabs_from(pieces, M, MT)                      # float32 of the exact sum: better than any fp32 accumulation
    e, ec, worst = R.check_gemm_dense(good, Wt, X, k, M)
    assert e < ec and worst <= 1.0
    a, b = R.piece_kblocks(k, 0, 0, KB)
    assert b - a >= 8, "one k-block of several"
    ks = slice(a * 16, a * 16 + 16)
    bad = pieces.copy()
    bad[0, :, :128] -= X[:M, ks].astype(np.float64) @ Wt[:128, ks].astype(np.float64).T
    with pytest.raises(AssertionError):
        R.check_gemm_dense(_slabs_from(bad, M, MT), Wt, X, k, M)


def test_pack_check_catches_swapped_rows():
    rs = RS(5)
    Wt = R.tile_weight(rs.randn(64, 48).astype(np.float32), (1 + 0.1 * rs.randn(48)).astype(np.float32))
    bits = R.pack_weight(Wt)
    assert R.check_pack(bits, Wt) == 0
    bad = bits.reshape(2, 3, 64, 8).copy()
    bad[1, :, [4, 5]] = bad[1, :, [5, 4]]                    # two rows of tile 1 (lanes 4 and 5: k 0..7 of each k-block)
    with pytest.raises(AssertionError):
        R.check_pack(bad, Wt)
    # and the integer GEMM sees the same swap through its outputs
    sw = R.unpack_weight(bad, 2, 48)
    X = _ints(rs, (32, 48), 8)
    k = R._sk_for(2, 3, False)
    got = _slabs_from(R.gemm_pieces(R.bf(np.rint(sw * 8)), X, k)[0], 32, 1)
    with pytest.raises(AssertionError):
        R.check_gemm_exact(got, R.bf(np.rint(Wt * 8)), X, k, 32)


# ------------------------------------------------------------------------------------------------------------------ consumers
def _fp32_swiglu(acc, rstd32, F, shift=0, rows=None):
    """k_cham_swiglu in numpy fp32; shift: x3 taken from `shift` features further on; rows: the row each row's 1/rms is read from"""
    M = acc.shape[0]
    a = acc.reshape(M, F // 16, 2, 16)
    a1, a3 = a[:, :, 0].reshape(M, F), np.roll(a[:, :, 1].reshape(M, F), -shift, axis=1)
    r = rstd32[np.arange(M) if rows is None else rows][:, None]
    u1, u3 = R.bf(r * a1), R.bf(r * a3)
    s = R.bf(u1 / (np.float32(1) + np.exp(-u1, dtype=np.float32)))
    return R.bf(s * u3)


def _consumer_case(seed=7, M=40, MT=2, D=128, F=64):
    rs = RS(seed)
    Wt = R.tile_weight(rs.randn(2 * F, D) / D ** 0.5, (1 + 0.1 * rs.randn(D)).astype(np.float32), 1, F)
    X = np.zeros((32 * MT, D), dtype=np.float32)
    X[:M] = R.bf(rs.randn(M, D).astype(np.float32) * (1 + rs.rand(M, 1).astype(np.float32)))
    k = R._sk_for(F // 16, D // 16, False)
    p64, _ = R.gemm_pieces(Wt, X[:M], k)
    pieces = np.zeros((R.BG_MAXP, 32 * MT, 2 * F), dtype=np.float32)
    pieces[:, :M] = np.nan_to_num(p64).astype(np.float32)
    counts = R.pieces_of(k, F // 16)
    ssq = np.zeros((D // 64, 32 * MT))
    ssq[:, :M] = R.ssq_chunks(X[:M])
    return X, pieces, counts, ssq, k


def test_swiglu_check_catches_x3_shift_and_wrong_row_rstd():
    M, MT, D, F, eps = 40, 2, 128, 64, 1e-5
    X, pieces, counts, ssq, _ = _consumer_case(M=M, MT=MT, D=D, F=F)
    acc = R.fold_pieces(pieces[:, :M], counts)
    rstd32 = (np.float32(1) / np.sqrt((ssq[:, :M].sum(0) / D).astype(np.float32) + np.float32(eps))).astype(np.float32)
    good = np.zeros((32 * MT, F), dtype=np.float32)
    good[:M] = _fp32_swiglu(acc, rstd32, F)
    assert R.check_swiglu(good, pieces, counts, ssq, D, eps, F, M) <= R.UNDECIDED_CAP
    for kw in (dict(shift=1), dict(rows=np.roll(np.arange(M), 1))):
        bad = good.copy()
        bad[:M] = _fp32_swiglu(acc, rstd32, F, **kw)
        with pytest.raises(AssertionError):
            R.check_swiglu(bad, pieces, counts, ssq, D, eps, F, M)
    # 1/rms over the wrong statistics chunk: the second chunk counted twice in place of the first
    bad = good.copy()
    r2 = (np.float32(1) / np.sqrt((2 * ssq[1, :M] / D).astype(np.float32) + np.float32(eps))).astype(np.float32)
    bad[:M] = _fp32_swiglu(acc, r2, F)
    with pytest.raises(AssertionError):
        R.check_swiglu(bad, pieces, counts, ssq, D, eps, F, M)


def test_resid_and_ssq_checks():
    M, MT, D = 40, 2, 128
    rs = RS(11)
    x = np.zeros((32 * MT, D), dtype=np.float32)
    x[:M] = R.bf(rs.randn(M, D).astype(np.float32))
    k = (2, 2, 2)                                           # one group, two pieces
    pieces = np.zeros((R.BG_MAXP, 32 * MT, D), dtype=np.float32)
    pieces[:2, :M] = rs.randn(2, M, D).astype(np.float32)
    counts = [2]
    xn = x.copy()
    xn[:M] = R.resid_ref(x[:M], pieces[0, :M] + pieces[1, :M])
    ssq = np.zeros((D // 64, 32 * MT))
    ssq[:, :M] = R.ssq_chunks(xn[:M])
    assert R.check_resid(xn, ssq, x, pieces, counts, M)[0] == 0
    bad = xn.copy()
    bad[:M] = R.resid_ref(x[:M], pieces[0, :M])             # the last piece not added
    with pytest.raises(AssertionError):
        R.check_resid(bad, ssq, x, pieces, counts, M)
    bad = xn.copy()
    bad[:M] = R.bf(x[:M] + (pieces[0, :M] + pieces[1, :M]))  # the branch not rounded on its own
    with pytest.raises(AssertionError):
        R.check_resid(bad, ssq, x, pieces, counts, M)
    s2 = ssq.copy()
    s2[1, 3] = np.float64(np.float32(s2[1, 3]))              # a statistic kept in fp32
    with pytest.raises(AssertionError):
        R.check_resid(xn, s2, x, pieces, counts, M)
    s2 = ssq.copy()
    s2[:, :M] = R.ssq_chunks(xn[np.roll(np.arange(M), 1)])   # statistics of the neighbouring row
    with pytest.raises(AssertionError):
        R.check_resid(xn, s2, x, pieces, counts, M)


def test_head_check_catches_wrong_row_rstd():
    M, D, eps = 20, 128, 1e-5
    rs = RS(13)
    x = _ints(rs, (32, D), 8)
    x[3] = 0                                                # a row with no signal: 1/rms is irrelevant, the logits are exact zeros
    Wt = R.tile_weight(_ints(rs, (64, D), 4), None)
    acc = (x.astype(np.float64) @ Wt.astype(np.float64).T).astype(np.float32)
    ssq = R.ssq_chunks(x)
    rstd32 = (np.float32(1) / np.sqrt((ssq.sum(0) / D).astype(np.float32) + np.float32(eps))).astype(np.float32)
    good = R.bf(rstd32[:, None] * acc)
    assert R.check_head(good, acc, ssq, D, eps, M) <= R.UNDECIDED_CAP
    assert not good[3].any()
    with pytest.raises(AssertionError):
        R.check_head(R.bf(np.roll(rstd32, 1)[:, None] * acc), acc, ssq, D, eps, M)


# ------------------------------------------------------------------------------------------------------------------ attention
def _fp32_attn(q, kc, vc, scale, drop=None, twice=None):
    """online-softmax-free fp32 attention of one (row, head); drop / twice: a cached row left out / counted twice"""
    idx = [t for t in range(len(kc)) if t != drop] + ([twice] if twice is not None else [])
    s = (kc[idx] @ q).astype(np.float32) * np.float32(scale)
    w = np.exp(s - s.max(), dtype=np.float32)
    return R.bf((w[:, None] * vc[idx]).sum(0, dtype=np.float32) / w.sum(dtype=np.float32))


def test_attention_checks_catch_row_faults():
    hd, T, scale = 64, 300, 64 ** -0.5
    rs = RS(17)
    q = R.bf(rs.randn(hd).astype(np.float32))
    # one-hot: row t* carries lambda q, every other K row (the new token's included) is zero; V rows are distinct bf16 patterns
    lam = 200.0 / (scale * float(q @ q))
    vc = R.bits_f32((0x3c00 + np.arange(T * hd).reshape(T, hd) % 0x700).astype(np.uint16))
    for ts in (0, 137, T - 2):
        kc = np.zeros((T, hd), dtype=np.float32)
        kc[ts] = R.bf(np.float32(lam) * q)
        assert float(kc[ts] @ q) * scale > 190
        assert R.check_onehot(_fp32_attn(q, kc, vc, scale), vc[ts]) == 0
        with pytest.raises(AssertionError):
            R.check_onehot(_fp32_attn(q, kc, vc, scale, drop=ts), vc[ts])          # the cached row dropped: nothing else can stand in
    # new token dominates (k_new = c q): a kernel that takes row P from the stale cache and not from its registers loses it
    kc = np.zeros((T, hd), dtype=np.float32)
    kc[T - 1] = R.bf(np.float32(lam) * q)
    assert R.check_onehot(_fp32_attn(q, kc, vc, scale), vc[T - 1]) == 0
    stale = kc.copy()
    stale[T - 1] = 0
    with pytest.raises(AssertionError):
        R.check_onehot(_fp32_attn(q, stale, vc, scale), vc[T - 1])
    # two equal winners: bf of the mean, exact; one of them counted twice moves the weights to 2/3 : 1/3
    kc = np.zeros((T, hd), dtype=np.float32)
    kc[5] = kc[250] = R.bf(np.float32(lam) * q)
    mean = R.bf((vc[5].astype(np.float64) + vc[250].astype(np.float64)).astype(np.float32) * np.float32(0.5))
    assert R.check_onehot(_fp32_attn(q, kc, vc, scale), mean) == 0
    with pytest.raises(AssertionError):
        R.check_onehot(_fp32_attn(q, kc, vc, scale, twice=5), mean)
    # dense: one cached row of 300 dropped or repeated is far outside 4 x the fp32 evaluation's error
    # (scores of spread 1, as behind the qk LayerNorm: every cached row carries weight)
    kc, vd = R.bf(rs.randn(T, hd).astype(np.float32) / np.float32(np.abs(q).max() * 8)), R.bf(rs.randn(T, hd).astype(np.float32))
    ref = R.attn_ref(q, kc, vd, scale)[None]
    fp32 = _fp32_attn(q, kc, vd, scale)[None]
    blocked = R.bf(R.attn_ref(q.astype(np.float64), kc, vd, scale).astype(np.float32))[None]
    R.check_attn_dense(blocked, ref, fp32)
    for kw in (dict(drop=123), dict(twice=123)):
        with pytest.raises(AssertionError):
            R.check_attn_dense(_fp32_attn(q, kc, vd, scale, **kw)[None], ref, fp32)


def test_k_row_check_catches_a_shifted_rope_slot_and_stale_statistics():
    hd, Rr, D, eps = 64, 24, 128, 1e-5
    rs = RS(19)
    acc = rs.randn(Rr, hd).astype(np.float32) * 8
    ssq = np.abs(rs.randn(D // 64, Rr)) * 64 + 32
    rstd = R.rstd64(ssq, D, eps)
    pos = rs.randint(1, 1000, size=Rr)
    tab, _ = R.rope_table_ref(1100, hd, 10000.0)
    tab32 = tab.astype(np.float32)

    def kernel(slot_shift=0, rstd_rows=None):
        r32 = rstd.astype(np.float32)[np.arange(Rr) if rstd_rows is None else rstd_rows]
        u = R.bf(r32[:, None] * acc)
        cs = np.roll(tab32[pos, :, 0], slot_shift, axis=1)
        sn = np.roll(tab32[pos, :, 1], slot_shift, axis=1)
        out = np.empty_like(u)
        out[:, 0::2], out[:, 1::2] = u[:, 0::2] * cs - u[:, 1::2] * sn, u[:, 0::2] * sn + u[:, 1::2] * cs
        return R.bf(out)

    cands, und = R.rope_k_candidates(acc, rstd, tab32[pos, :, 0], tab32[pos, :, 1])
    assert R.check_candidates(kernel(), cands, und, "K row") <= R.UNDECIDED_CAP
    for kw in (dict(slot_shift=1), dict(slot_shift=-1), dict(rstd_rows=np.roll(np.arange(Rr), 1))):
        with pytest.raises(AssertionError):
            R.check_candidates(kernel(**kw), cands, und, "K row")


def test_rope_table_reference_bound_holds_for_an_fp32_evaluation_and_catches_a_slot_shift():
    for hd in (64, 128):
        ref, ang = R.rope_table_ref(1100, hd, 10000.0)
        i = np.arange(hd // 2, dtype=np.float32)
        freq = np.power(np.float32(10000.0), np.float32(-2.0) * i / np.float32(hd)).astype(np.float32)
        a32 = np.arange(1100, dtype=np.float32)[:, None] * freq[None, :]
        got = np.stack([np.cos(a32.astype(np.float64)), np.sin(a32.astype(np.float64))], -1).astype(np.float32)
        bound = (np.abs(ang) * R.ROPE_C * 2.0 ** -24 + 2 * 2.0 ** -24)[..., None]
        assert np.all(np.abs(got - ref) <= bound)
        assert not np.all(np.abs(np.roll(got, 1, axis=1) - ref) <= bound)
