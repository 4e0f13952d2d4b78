"""Plain float64 statements of every launch of a Chameleon decode step (wmar_amd/csrc/cham_kernels.h), one per stage, and the
layout maps of the engine's buffers, taken from the kernels.  numpy only; tests/test_cham_kernel_reference.py shows on the CPU
that each check built from them catches the fault it is there for, tests/test_gpu_cham_kernels.py holds the kernels to them.

Values are float32 arrays holding bf16-exact numbers unless said otherwise; `bits` are uint16 bf16 patterns.

Layouts (Mpad = 32 MT rows, KB = K / 16 k-blocks):
  packed activation  [KB][MT][64][8] bf16: element (m, k) at kb = k >> 4, mt = m >> 5, lane = (m & 31) + 32 ((k >> 3) & 1), j = k & 7
  slab piece         [2 NT][MT][64][8] fp32: float (((nt 2 + b) MT + i) 64 + lane) 8 + j is row 32 i + (lane & 31), tile-order
                     column 32 nt + 16 b + 8 (lane >> 5) + j (so a piece, read as a packed [N/16][MT][64][8] array, is in the
                     packed activation layout of its N columns)
  packed weight      [NT][KB][64][8] bf16: lane carries tile row i = lane & 31, i.e. tile-order column 32 nt + row_feature(i), and
                     k = 16 kb + 8 (lane >> 5) + j; the value is bf16(fp32(W) * fp32(gamma))
  tile order         mode 0: column n is output feature n.  mode 1 (w13): tile nt holds x1 features 16 nt .. 16 nt + 15 in columns
                     32 nt .. 32 nt + 15 and the matching x3 features in columns 32 nt + 16 .. 32 nt + 31
"""
import numpy as np

from tests.test_gpu_chameleon_parity import BG_KC, BG_MAXP, BG_TG, _count, _sk_for, _wg_of  # noqa: F401  (the one restatement of sk_*)

STAT_KB = 4                                   # CHAM_STAT_KB: k-blocks per statistics chunk (64 features)
STAGES = ["EMBED", "QKV", "ATTN", "WO", "RESID_ATTN", "W13", "SWIGLU", "W2", "RESID_FFN", "HEAD"]
EMBED, QKV, ATTN, WO, RESID_ATTN, W13, SWIGLU, W2, RESID_FFN, HEAD = range(10)


# ------------------------------------------------------------------------------------------------------------------- bf16
def bf_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even (bf_round_bits)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bits_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf(x):
    """float32 -> nearest bf16 value, as float32."""
    return bits_f32(bf_bits(x))


def bf_candidates(v, delta_abs):
    """Where the bf16 rounding of a float32 evaluation of the float64 value `v` may land when that evaluation is within
    `delta_abs` of v: (lo, hi, undecided).  Away from a midpoint of two neighbouring bf16 values lo == hi == bf16(v) (round to
    nearest even done on the float64 itself, no double rounding); within delta_abs of one, lo and hi are the two neighbours."""
    v = np.asarray(v, dtype=np.float64)
    _, e = np.frexp(np.abs(v))
    ulp = np.ldexp(1.0, e - 8)                                   # bf16: 8 significant bits
    q = v / ulp
    fl = np.floor(q)
    und = np.abs(q - fl - 0.5) * ulp <= delta_abs
    near = np.rint(q) * ulp
    lo = np.where(und, fl * ulp, near)
    hi = np.where(und, (fl + 1) * ulp, near)
    return lo.astype(np.float32), hi.astype(np.float32), und


# ------------------------------------------------------------------------------------------------------------------- layouts
def row_feature(i):
    """cham_row_feature: MFMA row i of a 32-row weight tile carries this output feature of the tile."""
    i = np.asarray(i)
    g, h, r = i >> 3, (i >> 2) & 1, i & 3
    return 16 * (g >> 1) + 8 * h + 4 * (g & 1) + r


def act_index(m, k, MT):
    """index (in elements) of (row m, column k) in a packed [KB][MT][64][8] array"""
    m, k = np.asarray(m), np.asarray(k)
    return ((((k >> 4) * MT + (m >> 5)) * 64 + (m & 31) + 32 * ((k >> 3) & 1)) * 8) + (k & 7)


def pack_act(X, MT):
    """[32 MT, K] -> flat [KB][MT][64][8] (any dtype)"""
    Mpad, K = X.shape
    assert Mpad == 32 * MT and K % 16 == 0
    return np.ascontiguousarray(np.asarray(X).reshape(MT, 32, K // 16, 2, 8).transpose(2, 0, 3, 1, 4)).reshape(-1)


def unpack_act(flat, MT, K):
    """flat [.., KB][MT][64][8] -> [.., 32 MT, K] (leading dimensions, e.g. slab pieces, are kept)"""
    a = np.asarray(flat)
    lead = a.shape[:-1] if a.ndim > 1 else ()
    a = a.reshape(lead + (K // 16, MT, 2, 32, 8))
    n = len(lead)
    return np.ascontiguousarray(a.transpose(tuple(range(n)) + (n + 1, n + 3, n, n + 2, n + 4))).reshape(lead + (32 * MT, K))


def slab_index(m, n, MT):
    """float index of (row m, tile-order column n) inside one slab piece"""
    m, n = np.asarray(m), np.asarray(n)
    nt, b, hh, j = n >> 5, (n >> 4) & 1, (n >> 3) & 1, n & 7
    return ((((nt * 2 + b) * MT + (m >> 5)) * 64 + (m & 31) + 32 * hh) * 8) + j


def unpack_slab(piece, MT, N):
    """pieces (flat fp32, or [P, floats per piece]) -> [.., 32 MT, N] in tile order: 16 columns of a piece are one k-block of the
    packed activation layout (test_layout_maps_round_trip holds this to slab_index)"""
    return unpack_act(piece, MT, N)


def pack_slab(R, MT):
    return pack_act(R, MT)


def tile_rows(N, mode, Hd=0):
    """source row of W for every tile-order column (-1: a padding column of the last tile, packed as zeros)"""
    if mode == 0:
        NT = (N + 31) // 32
        r = np.arange(NT * 32)
        return np.where(r < N, r, -1)
    NT = Hd // 16
    c = np.arange(NT * 32)
    nt, f = c >> 5, c & 31
    return np.where(f < 16, nt * 16 + f, Hd + nt * 16 + (f - 16))


def tile_weight(W, gamma, mode=0, Hd=0):
    """[N, K] source weights (fp32 or bf16 values as fp32) and gamma [K] or None -> [32 NT, K] bf16 values in tile order:
    bf16(fp32(W) * fp32(gamma)), zero rows for padding columns.  A bf16 source is the same call on its fp32 values."""
    W = np.asarray(W, dtype=np.float32)
    rows = tile_rows(W.shape[0], mode, Hd)
    Wt = np.where(rows[:, None] >= 0, W[np.maximum(rows, 0)], np.float32(0))
    if gamma is not None:
        Wt = Wt * np.asarray(gamma, dtype=np.float32)[None, :]
    return bf(Wt)


def pack_weight(Wt):
    """tile-order bf16 values [32 NT, K] -> bits [NT][KB][64][8] as k_bpack stores them"""
    N32, K = Wt.shape
    NT, KB = N32 // 32, K // 16
    bits = bf_bits(Wt).reshape(NT, 32, KB, 2, 8)                         # [nt][feature][kb][h][j]
    lane = np.arange(64)
    src = bits[:, row_feature(lane & 31)]                                 # [nt][lane][kb][h][j]
    out = src[:, lane, :, lane >> 5, :]                                   # advanced indices first: [lane][nt][kb][j]
    return np.ascontiguousarray(out.transpose(1, 2, 0, 3)).reshape(-1)


def unpack_weight(bits, NT, K):
    """inverse of pack_weight: bits -> tile-order bf16 values [32 NT, K]"""
    KB = K // 16
    b = np.asarray(bits).reshape(NT, KB, 64, 8)
    out = np.empty((NT, 32, KB, 2, 8), dtype=np.uint16)
    lane = np.arange(64)
    out[:, row_feature(lane & 31), :, lane >> 5, :] = b.transpose(2, 0, 1, 3)
    return bits_f32(out.reshape(NT * 32, K))


# ------------------------------------------------------------------------------------------------------------------- stream-K
def sk_groups(NT):
    return -(-NT // BG_TG)


def piece_chunks(k, g, p):
    """k-chunks (of BG_KC k-blocks) that piece p of column group g covers: the units of workgroup sk_first(g) + p inside g"""
    C, U, G = k
    w = _wg_of(k, g * C) + p
    u0, u1 = w * U // G, (w + 1) * U // G
    return [u - g * C for u in range(max(u0, g * C), min(u1, (g + 1) * C))]


def piece_kblocks(k, g, p, KB):
    """(first, last + 1) k-block of piece p of group g"""
    ch = piece_chunks(k, g, p)
    assert ch and ch == list(range(ch[0], ch[-1] + 1))
    return ch[0] * BG_KC, min(KB, (ch[-1] + 1) * BG_KC)


def pieces_of(k, NT):
    return [_count(k, g) for g in range(sk_groups(NT))]


def gemm_pieces(Wt, X, k):
    """The partial sums k_bgemm<MT, SLAB> leaves: float64 [BG_MAXP][M, 32 NT] (tile order), piece p of group g = the sum over
    exactly the k-blocks piece_kblocks gives; slots past a group's piece count are NaN.  Also returns sum |terms| per slot."""
    N32, K = Wt.shape
    NT, KB = N32 // 32, K // 16
    M = X.shape[0]
    W64, X64 = Wt.astype(np.float64), X.astype(np.float64)
    out = np.full((BG_MAXP, M, N32), np.nan)
    mag = np.full((BG_MAXP, M, N32), np.nan)
    for g in range(sk_groups(NT)):
        c0, c1 = g * 32 * BG_TG, min(N32, (g + 1) * 32 * BG_TG)
        for p in range(_count(k, g)):
            kb0, kb1 = piece_kblocks(k, g, p, KB)
            ks = slice(kb0 * 16, kb1 * 16)
            out[p, :, c0:c1] = X64[:, ks] @ W64[c0:c1, ks].T
            mag[p, :, c0:c1] = np.abs(X64[:, ks]) @ np.abs(W64[c0:c1, ks]).T
    return out, mag


def gemm_chain(Wt, X, k):
    """The yardstick of the dense checks: the same pieces accumulated in fp32 one term after the other in k order (a product of
    two bf16 values is exact in fp32, so each step is one rounding).  fp32 [BG_MAXP][M, 32 NT], NaN in unused slots."""
    import torch
    N32, K = Wt.shape
    NT, KB = N32 // 32, K // 16
    M = X.shape[0]
    C = k[0]
    start, end = {}, {}                          # chunk -> [(piece, c0, c1)] of the pieces that begin / end with it
    for g in range(sk_groups(NT)):
        c0, c1 = g * 32 * BG_TG, min(N32, (g + 1) * 32 * BG_TG)
        for p in range(_count(k, g)):
            ch = piece_chunks(k, g, p)
            start.setdefault(ch[0], []).append((p, c0, c1))
            end.setdefault(ch[-1], []).append((p, c0, c1))
    xt, wt = torch.from_numpy(np.ascontiguousarray(X.T, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(Wt.T, dtype=np.float32))
    acc = torch.zeros(M, N32)
    seq = torch.full((BG_MAXP, M, N32), float("nan"))
    for c in range(C):
        for _, c0, c1 in start.get(c, []):
            acc[:, c0:c1] = 0
        for kk in range(c * BG_KC * 16, min(K, (c + 1) * BG_KC * 16)):
            acc += xt[kk][:, None] * wt[kk][None, :]
        for p, c0, c1 in end.get(c, []):
            seq[p, :, c0:c1] = acc[:, c0:c1]
    return seq.numpy()


def fold_pieces(pieces32, counts):
    """fp32 sum of a group's pieces in piece order, as every consumer forms it: [P][M, 32 NT] fp32 -> [M, 32 NT] fp32"""
    P, M, N32 = pieces32.shape
    acc = np.zeros((M, N32), dtype=np.float32)
    for g, np_ in enumerate(counts):
        c0, c1 = g * 32 * BG_TG, min(N32, (g + 1) * 32 * BG_TG)
        for p in range(np_):
            acc[:, c0:c1] = acc[:, c0:c1] + pieces32[p, :, c0:c1].astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------------------------- stages
def ssq_chunks(x):
    """[M, D] bf16 values -> float64 [ceil(D / 64)][M] sums of squares of each 64-feature chunk"""
    M, D = x.shape
    nch = -(-D // (16 * STAT_KB))
    x64 = x.astype(np.float64) ** 2
    return np.stack([x64[:, c * 64:(c + 1) * 64].sum(1) for c in range(nch)])


def rstd64(ssq, D, eps):
    """float64 1 / rms from the chunk sums: [nch][M] -> [M]"""
    return 1.0 / np.sqrt(ssq.sum(0) / D + np.float64(np.float32(eps)))


def resid_ref(x, acc32):
    """k_cham_resid<false>: x' = bf(x + bf(sum of pieces)) -- both additions' inputs are exact fp32, so this is bit exact"""
    return bf(x.astype(np.float32) + bf(acc32))


def embed_ref(emb, tok, Mpad):
    """k_cham_resid<true>: gathered rows, zero padding rows"""
    x = np.zeros((Mpad, emb.shape[1]), dtype=np.float32)
    x[:len(tok)] = emb[np.asarray(tok)]
    return x


# relative distance of a float32 evaluation of rstd * acc from the float64 value (acc exact, the chunk sums exact to 2^-53):
#   float(mean)        1/2 ulp                  2^-24      } the argument of rsqrtf is off by at most 2 * 2^-24,
#   + eps              1/2 ulp                  2^-24      } rsqrt halves a relative error:       2^-24
#   rsqrtf             1 ulp (HIP math API: rsqrtf max 1 ulp)                                      2 * 2^-24
#   rstd * acc         1/2 ulp                                                                     2^-24
# sum 4 * 2^-24; second-order terms are below 2^-46: 4.25 covers them.
DELTA_RSTD = 4.25 * 2.0 ** -24
# silu(u) = u / (1 + expf(-u)) on an exact bf16 u:
#   expf               1 ulp (HIP math API: expf max 1 ulp): e (1 +- 2 * 2^-24); 1 + e moves by at most e / (1 + e) * 2 * 2^-24 < 2 * 2^-24
#   1 + e              1/2 ulp                                                                     2^-24
#   u / ..             2.5 ulp, the bound of an fp32 division that is not correctly rounded (a correctly rounded one: 1/2 ulp)   5 * 2^-24
# sum 8 * 2^-24, 8.25 with the second-order terms.  The last step, bf(silu) * u3, is a product of two bf16 values: exact in fp32.
DELTA_SILU = 8.25 * 2.0 ** -24


def norm_candidates(acc32, rstd):
    """bf(rstd * acc) with the undecided rule: acc fp32 [M, N] exact, rstd float64 [M]"""
    v = rstd[:, None] * acc32.astype(np.float64)
    return bf_candidates(v, DELTA_RSTD * np.abs(v))


def swiglu_candidates(acc32, rstd, F):
    """k_cham_swiglu from the folded w13 sums (tile order [M, 2 F]): the set of outputs allowed per element, as a list of
    float32 arrays [M, F] (up to four: both candidates of u1, then both of bf(silu(u1)); u3's candidates multiply each), and
    the undecided mask [M, F]."""
    M = acc32.shape[0]
    a = acc32.reshape(M, F // 16, 2, 16)
    a1, a3 = a[:, :, 0].reshape(M, F), a[:, :, 1].reshape(M, F)
    u1 = norm_candidates(a1, rstd)
    u3 = norm_candidates(a3, rstd)
    outs, und = [], u1[2] | u3[2]
    for c1 in u1[:2]:
        s = c1.astype(np.float64) / (1.0 + np.exp(-c1.astype(np.float64)))
        s_lo, s_hi, s_und = bf_candidates(s, DELTA_SILU * np.abs(s))
        und = und | s_und
        for sc in (s_lo, s_hi):
            for c3 in u3[:2]:
                outs.append(bf(sc * c3))                    # exact product, one rounding
    return outs, und


def matches_any(got, cands):
    ok = np.zeros(got.shape, dtype=bool)
    for c in cands:
        ok |= bf_bits(got) == bf_bits(c)
    return ok


def rope_table_ref(T, hd, theta):
    """float64 (cos, sin) of the float64 angle p * theta^(-2 i / hd): [T, hd / 2, 2], and the angles"""
    i = np.arange(hd // 2, dtype=np.float64)
    ang = np.arange(T, dtype=np.float64)[:, None] * np.float64(np.float32(theta)) ** (-2.0 * i / hd)[None, :]
    return np.stack([np.cos(ang), np.sin(ang)], -1), ang


# |table - ref| <= |angle| * ROPE_C * 2^-24 + 2 * 2^-24, from k_rope_table's steps (theta = 10000 and 2 i are exact in fp32):
#   y = -2 i / hd       one fp32 division, 1/2 ulp: y (1 + r), |r| <= 2^-24; theta^(y r) moves the power by |y ln theta| |r|,
#                       and |y| < 1, ln 10000 = 9.22                                                     9.22 * 2^-24
#   powf                1 ulp (HIP math API: powf max 1 ulp)                                             2    * 2^-24
#   (float) p * freq    1/2 ulp                                                                          1    * 2^-24
# so the fp32 angle is within |angle| * 12.22 * 2^-24 of the float64 one (12.5 with the second-order terms) and cos, sin are
# 1-Lipschitz.  sincosf: 1 ulp (HIP math API) of a value of magnitude <= 1, at most 2^-23 = 2 * 2^-24 absolute.
ROPE_C = 12.5


def rope_rotate(x, cs, sn):
    """adjacent pairs: x [.., hd] float64, cs / sn [.., hd / 2] -> (value, sum of |products|) in float64"""
    x0, x1 = x[..., 0::2], x[..., 1::2]
    v = np.empty_like(x)
    mg = np.empty_like(x)
    v[..., 0::2], v[..., 1::2] = x0 * cs - x1 * sn, x0 * sn + x1 * cs
    mg[..., 0::2], mg[..., 1::2] = np.abs(x0 * cs) + np.abs(x1 * sn), np.abs(x0 * sn) + np.abs(x1 * cs)
    return v, mg


def attn_ref(q, kc, vc, scale):
    """decode attention of one (row, head): q [hd], kc / vc [T, hd] (the new token's row last) in float64"""
    s = (kc.astype(np.float64) @ q.astype(np.float64)) * scale
    w = np.exp(s - s.max())
    return (w / w.sum()) @ vc.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------- checks
# Shared by the GPU tests (on what the kernels left) and by tests/test_cham_kernel_reference.py (on planted faults).
DENSE_GATE = 2.0            # tests/vq_layer_checks.py: x the sequential fp32 chain's normalised error on the same data
TORCH_FACTOR = 4.0          # tests/test_gpu_vq_grad_layers.py: the attention factor against an fp32 evaluation of the same stage
UNDECIDED_CAP = 0.01        # share of elements the undecided rule may exempt from bit equality (expected: about 2^-10)
SENTINEL = np.float32(-7.0e30)


def diff_bits(got, want):
    """number of elements whose bit patterns differ (fp32 arrays; -0.0 and 0.0 count as equal)"""
    g, w = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return int(np.count_nonzero((g.view(np.uint32) != w.view(np.uint32)) & ~((g == 0) & (w == 0))))


def check_pack(got_bits, Wt):
    want = pack_weight(Wt)
    bad = int(np.count_nonzero(np.asarray(got_bits).reshape(-1) != want))
    assert bad == 0, "packed weight: %d of %d bf16 patterns differ" % (bad, want.size)
    return bad


def check_gemm_exact(got, Wt, X, k, M):
    """got fp32 [BG_MAXP][Mpad, 32 NT] (buffer prefilled with SENTINEL): integer operands, so every piece must equal the integer
    partial sum over exactly its k-blocks bit for bit; unused slots and rows >= M keep the sentinel."""
    want, mag = gemm_pieces(Wt, X[:M], k)
    assert np.nanmax(mag) < 2 ** 24, "operands too large for exact fp32 partial sums"
    used = ~np.isnan(want)
    exp = np.full(got.shape, SENTINEL, dtype=np.float32)
    exp[:, :M][used] = want[used].astype(np.float32)
    bad = diff_bits(got, exp)
    assert bad == 0, "%d of %d slab floats differ (live %d, sentinel region %d)" % (
        bad, exp.size, diff_bits(got[:, :M][used], exp[:, :M][used]), diff_bits(np.where(exp == SENTINEL, got, 0), np.where(exp == SENTINEL, exp, 0)))
    return bad


def check_gemm_dense(got, Wt, X, k, M):
    """per piece: max |got - exact| / sum |terms| <= DENSE_GATE x the same figure of the sequential fp32 chain"""
    want, mag = gemm_pieces(Wt, X[:M], k)
    seq = gemm_chain(Wt, X[:M], k)
    used = ~np.isnan(want)
    den = np.where(used & (mag > 0), mag, 1.0)
    e = np.where(used, np.abs(got[:, :M].astype(np.float64) - np.where(used, want, 0)) / den, 0.0)
    ec = np.where(used, np.abs(seq.astype(np.float64) - np.where(used, want, 0)) / den, 0.0)
    worst = 0.0
    for p in range(BG_MAXP):
        if used[p].any():
            ep, cp = float(e[p].max()), float(ec[p].max())
            assert ep <= DENSE_GATE * cp, "piece %d: normalised error %.3g is %.2f x the fp32 chain's %.3g" % (p, ep, ep / cp if cp else np.inf, cp)
            worst = max(worst, ep / cp if cp else 0.0)
    return float(e.max()), float(ec.max()), worst


def check_ssq(got, x, M):
    """each chunk within 4 * 2^-53 relative of the float64 sum of squares of its 64 features"""
    want = ssq_chunks(x[:M])
    err = np.abs(got[:, :M] - want)
    assert np.all(err <= 4 * 2.0 ** -53 * want), "ssq off by up to %.3g relative" % float((err / np.maximum(want, 1e-300)).max())
    return float((err / np.maximum(want, 1e-300)).max())


def check_resid(x_got, ssq_got, x_old, pieces32, counts, M):
    """x' == bf(x + bf(fp32 sum of the pieces in piece order)) bit for bit on the live rows; ssq of the new x"""
    want = resid_ref(x_old[:M], fold_pieces(pieces32[:, :M], counts))
    bad = diff_bits(x_got[:M], want)
    assert bad == 0, "residual update: %d of %d elements differ" % (bad, want.size)
    return bad, check_ssq(ssq_got, x_got, M)


def check_candidates(got, cands, und, what):
    """every element is one of its candidates; the undecided share (from the reference alone) stays under the cap"""
    share = float(np.mean(und))
    assert share <= UNDECIDED_CAP, "%s: %.3g of the elements are undecided" % (what, share)
    ok = matches_any(got, cands)
    assert ok.all(), "%s: %d of %d elements are none of their candidates (undecided share %.3g)" % (what, int((~ok).sum()), ok.size, share)
    return share


def check_swiglu(h_got, pieces32, counts, ssq, D, eps, F, M):
    acc = fold_pieces(pieces32[:, :M], counts)
    cands, und = swiglu_candidates(acc, rstd64(ssq[:, :M], D, eps), F)
    return check_candidates(h_got[:M], cands, und, "SwiGLU")


def check_head(lg_got, acc32, ssq, D, eps, M):
    """logits == bf(rstd * acc) under the undecided rule; acc must be exact (integer operands)"""
    lo, hi, und = norm_candidates(acc32[:M], rstd64(ssq[:, :M], D, eps))
    return check_candidates(lg_got[:M], [lo, hi], und, "head")


def rope_k_candidates(acc32, rstd, cs, sn):
    """the K row k_cham_attn appends without qk normalisation: bf(rope(bf(rstd * acc))).  acc [R, hd] fp32 exact, rstd [R], cs /
    sn [R, hd / 2] the fp32 table entries the kernel reads.  Both candidates of an undecided first rounding go through the
    rotation; the rotation's own fp32 error is one rounding per product and one for the sum (fused or not)."""
    u_lo, u_hi, und = norm_candidates(acc32, rstd)
    cands = []
    cs, sn = cs.astype(np.float64), sn.astype(np.float64)
    for a in (u_lo, u_hi):
        for b in (u_lo, u_hi):
            x = a.astype(np.float64).copy()
            x[..., 1::2] = b[..., 1::2]
            v, mg = rope_rotate(x, cs, sn)
            lo, hi, u2 = bf_candidates(v, 2.0 ** -24 * mg + 2.0 ** -24 * np.abs(v))
            und = und | u2
            cands += [lo, hi]
    return cands, und


def check_onehot(y_got, v_want):
    """attention output of a (row, head) whose winning score leads by ~200: exactly the winner's V row"""
    bad = diff_bits(y_got, v_want)
    assert bad == 0, "one-hot attention: %d of %d output elements differ from the selected V row" % (bad, v_want.size)
    return bad


def attn_rel_err(got, ref64):
    """per (row, head): max |got - ref64| / max |ref64| over head_dim; got / ref64 [.., hd]"""
    return np.abs(got.astype(np.float64) - ref64).max(-1) / np.abs(ref64).max(-1)


def check_attn_dense(y_got, ref64, y_fp32):
    e, eo = attn_rel_err(y_got, ref64), attn_rel_err(y_fp32, ref64)
    assert np.all(e <= TORCH_FACTOR * eo), "attention: error %.3g is %.2f x the fp32 evaluation's %.3g at the worst (row, head)" % (
        float(e[np.argmax(e / np.maximum(eo, 1e-300))]), float((e / np.maximum(eo, 1e-300)).max()), float(eo[np.argmax(e / np.maximum(eo, 1e-300))]))
    return float(e.max()), float(eo.max()), float((e / np.maximum(eo, 1e-300)).max())
