"""Plain numpy statements (float64, and float32 where the kernel's order fixes the bits) of the launches of a Taming minGPT decode
step (wmar_amd/csrc/decoder_kernels.h, decode_small.h), one per stage of wmar_gpt_probe_run, with the layout maps of the engine's
buffers and the K decompositions of its split GEMMs, taken from the kernels.  numpy only, nothing from wmar_amd/csrc.
tests/test_gpt_kernel_reference.py shows on the CPU that each check built from them catches the fault it is there for,
tests/test_gpu_gpt_kernels.py holds the kernels to them.

Everything is fp32 in HBM.  Mpad = 32 MT rows, MT = 1 / 2 / 4 row tiles for B <= 32 / 64 / 128, KB = K / 8 k-blocks.

Layouts
  packed activation  [KB][MT][64][4]: element (m, k) at kb = k >> 3, mt = m >> 5, lane = (m & 31) + 32 ((k >> 2) & 1), j = k & 3.
                     An output of N columns is the packed activation of the next GEMM (column n = its feature k).
  slab pieces        piece s of a split GEMM is one packed activation [N/8][MT][64][4] holding the partial sums over slice s of K;
                     pieces lie S * (N * 32 MT) floats apart (the stride follows the MT of the step, not of max_batch).
  row-major pieces   k_qkvx_bx writes its QKV pieces as [64 rows][3 D] instead (same piece stride).
  k_pack_linear      [NT][KB][64][4]: lane = (n & 31) + 32 ((k >> 2) & 1), value fp32(W[n][k] * gamma[k]) (ONE rounding; no gamma: W).
  k_pack_bx          [NT][K/16][2][64][4]: (ku, hf, lane) holds n = 32 nt + (lane & 31), k = 16 ku + 8 (lane >> 5) + 4 hf + 0..3.
  k_pack_fc1x        W16 [N/24][K/16][64][4]: register q of lane l (blk = l >> 4): pair = 2 q + (blk & 1), column 24 t + (l & 15),
                     k = 16 ku + 8 (pair >> 2) + (pair & 3) + 4 (blk >> 1);
                     W8 [N/24][K/16][64][2]: register g of lane l (blk = l >> 2): pair = blk & 7, column 24 t + 16 + 4 g + (l & 3),
                     k = 16 ku + 8 (pair >> 2) + (pair & 3) + 4 (blk >> 3).   ("pair" p covers k = 8 (p >> 2) + (p & 3) and k + 4.)
  bf16 planes        [K/16][MT][3][64][8] bf16 (bx_store_planes4): piece 0 / 1 / 2 = h, m, l with h = bf(x), m = bf(x - h),
                     l = bf((x - h) - m); lane = (m & 31) + 32 ((k >> 3) & 1), j = k & 7.
  statistics         [chunk][Mpad][2] fp64: (sum, sum of squares) of the chunk's features of row m.
  cache              [max_batch][H][block_size][head_dim] per block; row `pos` is appended by the attention launch (k_sgemv<QKV> on
                     the small-batch plan).
  small-batch plan   xs, ys, qs [12][D], hs [12][4 D] row-major; weights in the checkpoint's own [N][K] layout.
"""
import numpy as np

from tests.cham_kernel_reference import (DENSE_GATE, SENTINEL, TORCH_FACTOR, UNDECIDED_CAP, bf, bf_bits, bits_f32,  # noqa: F401
                                         diff_bits)

STAGES = ["EMBED", "RESID_IN", "QKV", "ATTN", "PROJ", "RESID_ATTN", "FC1", "FC2", "RESID_OUT", "HEAD"]
EMBED, RESID_IN, QKV, ATTN, PROJ, RESID_ATTN, FC1, FC2, RESID_OUT, HEAD = range(10)
MAX_SLABS = 8
QKV_SLABS_MAX = 8
STAT_CHUNKS_MAX = 64
GEMM_NW, GEMM_U = 4, 4            # waves per k_gemm workgroup, k-blocks per register stage (MTW 1 and 2)
QX_CK = 4                         # k-blocks per staged chunk of k_qkvx / k_qkvx_bx
BX_KSLICE = 384                   # k per K slice of k_bx / k_bx_xr
SG_MAX_ROWS = 12
LN_EPS = np.float32(1e-5)


def mt_for(B):
    return 1 if B <= 32 else (2 if B <= 64 else 4)


# ------------------------------------------------------------------------------------------------------------------- layouts
def act_index(m, k, MT):
    """float index of (row m, feature k) in a packed [KB][MT][64][4] array"""
    m, k = np.asarray(m), np.asarray(k)
    return ((((k >> 3) * MT + (m >> 5)) * 64 + (m & 31) + 32 * ((k >> 2) & 1)) * 4) + (k & 3)


def pack_act(X, MT):
    """[32 MT, K] -> flat [KB][MT][64][4] (any dtype)"""
    Mpad, K = X.shape
    assert Mpad == 32 * MT and K % 8 == 0
    return np.ascontiguousarray(np.asarray(X).reshape(MT, 32, K // 8, 2, 4).transpose(2, 0, 3, 1, 4)).reshape(-1)


def unpack_act(flat, MT, K):
    """flat [.., KB][MT][64][4] -> [.., 32 MT, K] (leading dimensions, e.g. slab pieces, are kept)"""
    a = np.asarray(flat)
    lead = a.shape[:-1] if a.ndim > 1 else ()
    a = a.reshape(lead + (K // 8, MT, 2, 32, 4))
    n = len(lead)
    return np.ascontiguousarray(a.transpose(tuple(range(n)) + (n + 1, n + 3, n, n + 2, n + 4))).reshape(lead + (32 * MT, K))


def get_pieces(flat, n_pieces, MT, N, rowmajor=False):
    """the first n_pieces pieces of a slab buffer -> [n_pieces][32 MT, N]"""
    stride = N * 32 * MT
    a = np.asarray(flat)[:n_pieces * stride].reshape(n_pieces, stride)
    return a.reshape(n_pieces, 32 * MT, N).copy() if rowmajor else unpack_act(a, MT, N)


def put_pieces(flat, P, MT, rowmajor=False):
    """writes pieces [n][32 MT, N] into the front of a flat slab buffer (in place)"""
    n, Mpad, N = P.shape
    stride = N * Mpad
    flat[:n * stride] = (P.reshape(n, -1) if rowmajor else np.stack([pack_act(P[p], MT) for p in range(n)])).reshape(-1)
    return flat


def fold_gamma(W, gamma):
    """fp32(W * gamma): the ONE rounding every pack kernel makes"""
    W = np.asarray(W, dtype=np.float32)
    return W if gamma is None else (W * np.asarray(gamma, dtype=np.float32)[None, :]).astype(np.float32)


def pack_linear(Wg):
    """[N, K] (gamma folded) -> flat [NT][KB][64][4] as k_pack_linear stores it"""
    N, K = Wg.shape
    return np.ascontiguousarray(Wg.reshape(N // 32, 32, K // 8, 2, 4).transpose(0, 2, 3, 1, 4)).reshape(-1)


def pack_bx(Wg):
    """[N, K] -> flat [NT][K/16][2][64][4] as k_pack_bx stores it"""
    N, K = Wg.shape
    a = Wg.reshape(N // 32, 32, K // 16, 2, 2, 4)             # [nt][n32][ku][lane >> 5][hf][j]
    return np.ascontiguousarray(a.transpose(0, 2, 4, 3, 1, 5)).reshape(-1)


def _fc1x_maps():
    lane = np.arange(64)[:, None]
    q = np.arange(4)[None, :]
    blk = lane >> 4
    pair = 2 * q + (blk & 1)
    n16, k16 = np.broadcast_to(lane & 15, (64, 4)), 8 * (pair >> 2) + (pair & 3) + 4 * (blk >> 1)
    g = np.arange(2)[None, :]
    blk8 = lane >> 2
    pair8 = np.broadcast_to(blk8 & 7, (64, 2))
    n8, k8 = 16 + 4 * g + (lane & 3), 8 * (pair8 >> 2) + (pair8 & 3) + 4 * np.broadcast_to(blk8 >> 3, (64, 2))
    return n16, k16, n8, k8


def pack_fc1x(Wg):
    """[N, K] -> (W16 flat [N/24][K/16][64][4], W8 flat [N/24][K/16][64][2]) as k_pack_fc1x stores them"""
    N, K = Wg.shape
    a = Wg.reshape(N // 24, 24, K // 16, 16)
    n16, k16, n8, k8 = _fc1x_maps()
    w16 = a[:, n16, :, k16]                                    # advanced indices first: [64][4][N/24][K/16]
    w8 = a[:, n8, :, k8]
    return (np.ascontiguousarray(w16.transpose(2, 3, 0, 1)).reshape(-1), np.ascontiguousarray(w8.transpose(2, 3, 0, 1)).reshape(-1))


def bx_split(x):
    """fp32 -> (h, m, l) bf16 values as fp32 with x == h + m + l (bx_split2: round to nearest even, exact subtractions)"""
    x = np.asarray(x, dtype=np.float32)
    h = bf(x)
    r = (x - h).astype(np.float32)
    m = bf(r)
    return h, m, bf((r - m).astype(np.float32))


def pack_planes(X, MT):
    """[32 MT, K] fp32 -> uint16 flat [K/16][MT][3][64][8] (bx_store_planes4)"""
    Mpad, K = X.shape
    out = np.empty((K // 16, MT, 3, 2, 32, 8), dtype=np.uint16)
    for p, piece in enumerate(bx_split(X)):
        b = bf_bits(piece).reshape(MT, 32, K // 16, 2, 8)       # [mt][m32][ku][lane >> 5][j]
        out[:, :, p] = b.transpose(2, 0, 3, 1, 4)
    return out.reshape(-1)


def unpack_planes(bits, MT, K):
    """inverse: uint16 planes -> the three pieces [3][32 MT, K] as fp32"""
    a = np.asarray(bits, dtype=np.uint16).reshape(K // 16, MT, 3, 2, 32, 8)
    return bits_f32(np.ascontiguousarray(a.transpose(2, 1, 4, 0, 3, 5)).reshape(3, 32 * MT, K))


def cache_index(b, h, t, d, H, Tmax, hd):
    return ((np.asarray(b) * H + h) * Tmax + t) * hd + d


# ------------------------------------------------------------------------------------------------------------------- decompositions
def gemm_piece_kblocks(KB, S, n_hi, nt, s, NW=GEMM_NW, U=GEMM_U):
    """k-blocks [kb0, kb1) that slab s of column tile nt holds (k_gemm<.., EPI_PACKED>), or None when the tile has no slab s.
    Tiles below n_hi are cut S + 1 ways.  With n_hi > 0 and KB a multiple of NW * 2 U the cuts of EVERY tile fall on whole pipeline
    rounds (NW waves x 2 U k-blocks)."""
    S_t = S + 1 if nt < n_hi else S
    if s >= S_t:
        return None
    if n_hi > 0 and KB % (NW * 2 * U) == 0:
        units = KB // (NW * 2 * U)
        return (s * units // S_t) * NW * 2 * U, ((s + 1) * units // S_t) * NW * 2 * U
    return (s * NW) * KB // (S_t * NW), ((s + 1) * NW) * KB // (S_t * NW)


def gemm_wave_kblocks(KB, S, n_hi, nt, s, w, NW=GEMM_NW, U=GEMM_U):
    """k-blocks of wave w inside that slab (the waves' partial sums meet in LDS in wave order)"""
    S_t = S + 1 if nt < n_hi else S
    if n_hi > 0 and KB % (NW * 2 * U) == 0:
        units = KB // (NW * 2 * U)
        u0, u1 = s * units // S_t, (s + 1) * units // S_t
        kb0 = (u0 * NW + w * (u1 - u0)) * 2 * U
        return kb0, kb0 + (u1 - u0) * 2 * U
    sl, slices = s * NW + w, S_t * NW
    return sl * KB // slices, (sl + 1) * KB // slices


def qkvx_kblocks(KB, S, s):
    """K slice s of k_qkvx (cut on k-blocks)"""
    return s * KB // S, (s + 1) * KB // S


def qkvx_bx_kblocks(KB, S, s):
    """K slice s of k_qkvx_bx (cut on 16-k steps)"""
    KU = KB // 2
    return 2 * (s * KU // S), 2 * ((s + 1) * KU // S)


def bx_kblocks(s):
    """K slice s of k_bx / k_bx_xr"""
    return s * BX_KSLICE // 8, (s + 1) * BX_KSLICE // 8


def stat_chunks(KB):
    n = (KB + 15) // 16
    return n


def resid_chunk_kblocks(KB, nch, c):
    """statistics chunk c of k_resid_stats"""
    return c * KB // nch, (c + 1) * KB // nch


def qkvx_bx_chunk_kblocks(KB, S, nkeep, c):
    """statistics chunk c = s nkeep + g of k_qkvx_bx: the staged chunks (4 k-blocks) j of slice s with j % nkeep == g -> list of k-blocks"""
    s, g = divmod(c, nkeep)
    kb0, kb1 = qkvx_bx_kblocks(KB, S, s)
    return [kb for kb in range(kb0, kb1) if ((kb - kb0) // QX_CK) % nkeep == g]


def xr_chunk_kblocks(KB, c):
    """statistics chunk c of 16 of k_bx_xr: XCD group c >> 1, half c & 1 of the group's k-blocks"""
    n = KB // 16
    return c * n, (c + 1) * n


def attn_chunk_rows(hd):
    """E: cached rows per chunk of k_attn_decode = 2 loads x 64 / LPR rows, LPR = lanes that cover a row (8, 16, 32)"""
    lpra = hd // 4
    lpr = 8 if lpra <= 8 else (16 if lpra <= 16 else 32)
    return 2 * 64 // lpr


def attn_lengths(hd, nwa):
    """the cache lengths of the one-hot sweep: every wave / chunk edge up to 256 rows"""
    E = attn_chunk_rows(hd)
    Ts = {1, 2, E - 1, E, E + 1, 2 * E * nwa - 1, 2 * E * nwa + 1, 4 * E * nwa - 1, 4 * E * nwa + 1, 255, 256}
    return sorted(t for t in Ts if 1 <= t <= 256)


def chunk_lists(KB, kind, **kw):
    """k-block lists of every statistics chunk: kind 'resid' (nch), 'qkvx' (S), 'qkvx_bx' (S, nkeep), 'xr'"""
    if kind == "resid":
        return [list(range(*resid_chunk_kblocks(KB, kw["nch"], c))) for c in range(kw["nch"])]
    if kind == "qkvx":
        return [list(range(*qkvx_kblocks(KB, kw["S"], s))) for s in range(kw["S"])]
    if kind == "qkvx_bx":
        return [qkvx_bx_chunk_kblocks(KB, kw["S"], kw["nkeep"], c) for c in range(kw["S"] * kw["nkeep"])]
    return [list(range(*xr_chunk_kblocks(KB, c))) for c in range(16)]


# ------------------------------------------------------------------------------------------------------------------- operations
def fold_vec(W, v, bias=None):
    """k_fold_bias: float32(bias + sum_k W[n][k] v[k]) with the sum in float64.  Returns (lo, hi): equal unless the sum is within
    K 2^-53 sum |w v| of a rounding midpoint (the kernel's fp64 sum runs in its own order); then the two neighbours.  The sum itself
    is formed in extended precision here (products of two floats are exact, 64-bit significand for the additions), so that this
    statement adds no error of its own."""
    ld = np.longdouble
    N, K = W.shape
    s, mag = np.empty(N, dtype=ld), np.empty(N, dtype=ld)
    v_ld = np.asarray(v, dtype=np.float32).astype(ld)
    for n0 in range(0, N, 512):
        prod = np.asarray(W[n0:n0 + 512], dtype=np.float32).astype(ld) * v_ld[None, :]
        s[n0:n0 + 512], mag[n0:n0 + 512] = prod.sum(1), np.abs(prod).sum(1)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float32).astype(ld)
        s, mag = s + b, mag + np.abs(b)
    slack = (K + 1) * ld(2.0) ** -53 * mag
    return (s - slack).astype(np.float32), (s + slack).astype(np.float32)


def embed_ref(tok_emb, pos_emb, tok, pos, Mpad):
    """k_resid_stats<embed>: x[m] = tok_emb[tok[m]] + pos_emb[pos] in fp32; padding rows read token 0"""
    t = np.zeros(Mpad, dtype=np.int64)
    t[:len(tok)] = tok
    return (tok_emb[t].astype(np.float32) + pos_emb[pos].astype(np.float32)[None, :]).astype(np.float32)


def fold_slabs(slabs, n_hi=0):
    """fp32 s0 + s1 + .. in slab order: [S][M, N] -> [M, N]; column tiles (32 columns) at or past n_hi have no last slab"""
    acc = slabs[0].astype(np.float32).copy()
    N = acc.shape[1]
    for s in range(1, len(slabs)):
        add = slabs[s].astype(np.float32)
        if n_hi > 0 and s == len(slabs) - 1:
            keep = (np.arange(N) // 32) < n_hi
            acc[:, keep] = (acc[:, keep] + add[:, keep]).astype(np.float32)
        else:
            acc = (acc + add).astype(np.float32)
    return acc


def resid_ref(x, bias, slabs, n_hi=0):
    """x' = x + (bias + (s0 + s1 + ..)) in fp32, in that order (k_resid_stats, the fold of k_qkvx / k_qkvx_bx, phase 2 of k_bx_xr)"""
    t = (np.asarray(bias, dtype=np.float32)[None, :] + fold_slabs(slabs, n_hi)).astype(np.float32)
    return (x.astype(np.float32) + t).astype(np.float32)


def stats_ref(x, chunks):
    """float64 [len(chunks)][M][2] (sum, sum of squares) over each chunk's k-blocks, and sum x^2 per chunk (the error scale)"""
    x64 = x.astype(np.float64)
    out = np.zeros((len(chunks), x.shape[0], 2))
    for c, kbs in enumerate(chunks):
        cols = (np.asarray(kbs, dtype=np.int64)[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
        out[c, :, 0] = x64[:, cols].sum(1)
        out[c, :, 1] = (x64[:, cols] ** 2).sum(1)
    return out


def mean_rstd64(stats, K):
    """float64 (mean, rstd) from the chunk sums [nch][M][2]"""
    mean = stats[:, :, 0].sum(0) / K
    var = stats[:, :, 1].sum(0) / K - mean * mean
    return mean, 1.0 / np.sqrt(var + np.float64(LN_EPS))


def gemm_pieces(Wg, X, ranges):
    """partial sums of X Wg^T: ranges[s][nt] = (kb0, kb1) or None -> float64 [S][M, N] (NaN where a tile has no slab s) and sum |terms|"""
    N, K = Wg.shape
    M = X.shape[0]
    W64, X64 = Wg.astype(np.float64), X.astype(np.float64)
    out = np.full((len(ranges), M, N), np.nan)
    mag = np.full((len(ranges), M, N), np.nan)
    for s, per_tile in enumerate(ranges):
        for nt, r in enumerate(per_tile):
            if r is None:
                continue
            ks, cs = slice(r[0] * 8, r[1] * 8), slice(nt * 32, nt * 32 + 32)
            out[s, :, cs] = X64[:, ks] @ W64[cs, ks].T
            mag[s, :, cs] = np.abs(X64[:, ks]) @ np.abs(W64[cs, ks]).T
    return out, mag


def gemm_chain(Wg, X, ranges):
    """the yardstick of the dense checks: each piece accumulated in fp32 one term after the other in k order (numpy; never the kernel)"""
    import torch
    N, K = Wg.shape
    M = X.shape[0]
    xt, wt = torch.from_numpy(np.ascontiguousarray(X.T, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(Wg.T, dtype=np.float32))
    out = torch.full((len(ranges), M, N), float("nan"))
    for s, per_tile in enumerate(ranges):
        groups = {}
        for nt, r in enumerate(per_tile):
            if r is not None:
                groups.setdefault(r, []).append(nt)
        for (kb0, kb1), nts in groups.items():
            cols = torch.tensor([nt * 32 + i for nt in nts for i in range(32)])
            acc = torch.zeros(M, len(cols))
            wsel = wt[:, cols]
            for k in range(kb0 * 8, kb1 * 8):
                acc += xt[k][:, None] * wsel[k][None, :]
            out[s][:, cols] = acc
    return out.numpy()


def uniform_ranges(NT, fn, S):
    """ranges for a GEMM whose slices do not depend on the column tile: fn(s) -> (kb0, kb1)"""
    return [[fn(s)] * NT for s in range(S)]


def gemm_ranges(KB, NT, S, n_hi=0):
    return [[gemm_piece_kblocks(KB, S, n_hi, nt, s) for nt in range(NT)] for s in range(S + (1 if n_hi > 0 else 0))]


def gelu64(v):
    from math import erf
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + np.vectorize(erf)(v * 0.70710678118654752440))


def attn_ref(q, kc, vc, scale):
    """decode attention of one (row, head): q [hd], kc / vc [T, hd] (the new token's row last) in float64"""
    s = (kc.astype(np.float64) @ q.astype(np.float64)) * scale
    w = np.exp(s - s.max())
    return (w / w.sum()) @ vc.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------- checks
# Shared by the GPU tests (on what the kernels left) and by tests/test_gpt_kernel_reference.py (on planted faults).

# A float32 evaluation of rstd * acc + b against the float64 value, acc exact and the row mean exactly 0 (so that the kernels'
# rstd * (acc - mean * c1) + b has no cancelling term):
#   float(var)           1/2 ulp            2^-24    } the argument of rsqrtf is off by at most 2 * 2^-24,
#   + 1e-5f              1/2 ulp            2^-24    } rsqrt halves a relative error:            2^-24
#   rsqrtf               1 ulp (HIP math API)                                                     2 * 2^-24
#   rstd * acc           1/2 ulp                                                                  2^-24
# = 4 * 2^-24 of |rstd acc| (the fp64 statistics' 2^-53 and the second-order terms are below 2^-46 and are not added), then + b:
# 1/2 ulp of the result (a fused multiply-add drops the product's rounding instead).  The outputs are fp32, so unlike the bf16 outputs
# of the Chameleon engine there is no "two candidate" form of this rule: 4 * 2^-24 |v| spans several fp32 values at every v.  Every
# element is held to the bound; none is exempt.
DELTA_RSTD = 4.0 * 2.0 ** -24
HALF_ULP = 2.0 ** -24
# gelu_erf(v) = 0.5 v (1 + erff(v / sqrt 2)) on an fp32 v: erff taken as 4 ulp of a value below 1 in magnitude, i.e. 4 * 2^-24 = 2^-22
# absolute on (1 + erf) and 2^-23 |v| on the result; the scaled argument's rounding moves erf by at most |erf'| |v| 2^-24 <= 2^-24
# * 0.49 (max of t exp(-t^2 / 2) sqrt(2 / pi)); the additions and two products add 3 * 2^-24 of the result.  |gelu'| <= 1.13 carries the
# pre-activation's own error.
GELU_LIP = 1.13


def check_exact(got, want, what):
    bad = diff_bits(got, want)
    assert bad == 0, "%s: %d of %d fp32 patterns differ" % (what, bad, np.asarray(want).size)
    return bad


def check_pack(got, want, what="packed weight"):
    g, w = np.ascontiguousarray(got, dtype=np.float32).reshape(-1), np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    assert g.size == w.size, "%s: %d floats, expected %d" % (what, g.size, w.size)
    bad = int(np.count_nonzero(g.view(np.uint32) != w.view(np.uint32)))
    assert bad == 0, "%s: %d of %d fp32 patterns differ" % (what, bad, w.size)
    return bad


def check_fold_vec(got, lo, hi, what):
    """got is float32 of SOME value within the slack of the sum: lo <= got <= hi (one float where the sum is clear of a midpoint; two
    neighbours at one; more only where the sum cancels so far that the slack itself exceeds a float32 ulp)"""
    g = np.ascontiguousarray(got, dtype=np.float32)
    ok = (g >= lo) & (g <= hi)
    assert ok.all(), "%s: %d of %d entries are not float32(float64 sum)" % (what, int((~ok).sum()), ok.size)
    return float(np.mean(lo.view(np.uint32) != hi.view(np.uint32)))


def check_gemm_exact(got, Wg, X, ranges, M):
    """got fp32 [P][Mpad, N] (buffer prefilled with SENTINEL; P >= len(ranges)): integer operands, so every piece equals the integer
    partial sum over exactly its k-blocks bit for bit on the live rows; slabs a tile does not own and pieces past the plan keep the
    sentinel.  Rows >= M of a written piece hold whatever the padding rows of the input gave: they are not compared."""
    want, mag = gemm_pieces(Wg, X[:M], ranges)
    assert np.nanmax(mag) < 2 ** 24, "operands too large for exact fp32 partial sums"
    used = ~np.isnan(want)                                       # [S][M, N]
    exp = np.full((got.shape[0], M, got.shape[2]), SENTINEL, dtype=np.float32)
    exp[:len(ranges)][used] = want[used].astype(np.float32)
    bad = diff_bits(got[:, :M], exp)
    col_used = np.zeros((got.shape[0], got.shape[2]), dtype=bool)
    col_used[:len(ranges)] = used[:, 0, :]
    pad_bad = int(np.count_nonzero(got[:, M:][:, :, :][np.broadcast_to(~col_used[:, None, :], got[:, M:].shape)] != SENTINEL))
    assert bad == 0 and pad_bad == 0, "%d of %d live slab floats differ (%d in pieces the plan does not write), %d sentinel floats of the padding rows overwritten" % (
        bad, exp.size, diff_bits(np.where(exp == SENTINEL, got[:, :M], 0), np.where(exp == SENTINEL, exp, 0)), pad_bad)
    return bad


def check_gemm_dense(got, Wg, X, ranges, M):
    """per piece: max |got - exact| / sum |terms| <= DENSE_GATE x the same figure of the sequential fp32 chain"""
    want, mag = gemm_pieces(Wg, X[:M], ranges)
    seq = gemm_chain(Wg, X[:M], ranges)
    used = ~np.isnan(want)
    den = np.where(used & (mag > 0), mag, 1.0)
    e = np.where(used, np.abs(got[:len(ranges), :M].astype(np.float64) - np.where(used, want, 0)) / den, 0.0)
    ec = np.where(used, np.abs(seq.astype(np.float64) - np.where(used, want, 0)) / den, 0.0)
    worst = 0.0
    for p in range(len(ranges)):
        ep, cp = float(e[p].max()), float(ec[p].max())
        assert ep <= DENSE_GATE * cp, "piece %d: normalised error %.3g is %.2f x the fp32 chain's %.3g" % (p, ep, ep / cp if cp else np.inf, cp)
        worst = max(worst, ep / cp if cp else 0.0)
    return float(e.max()), float(ec.max()), worst


def check_stats(got, x, chunks, M, exact):
    """got [>= len(chunks)][Mpad][2]: exact (inputs of <= 16 significant bits: every square and sum is exact in fp64) or within
    K 2^-53 sum x^2 (sum |x| for the plain sums)"""
    want = stats_ref(x[:M], chunks)
    g = got[:len(chunks), :M]
    if exact:
        bad = int(np.count_nonzero(g != want))
        assert bad == 0, "statistics: %d of %d chunk sums differ" % (bad, want.size)
        return 0.0
    x64 = np.abs(x[:M].astype(np.float64))
    worst = 0.0
    for c, kbs in enumerate(chunks):
        cols = (np.asarray(kbs, dtype=np.int64)[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
        n = len(cols)
        for j, scale in enumerate((x64[:, cols].sum(1), (x64[:, cols] ** 2).sum(1))):
            err = np.abs(g[c, :, j] - want[c, :, j])
            assert np.all(err <= n * 2.0 ** -53 * scale), "statistics chunk %d: off by %.3g of its scale" % (c, float((err / np.maximum(scale, 1e-300)).max()))
            worst = max(worst, float((err / np.maximum(scale, 1e-300)).max()))
    return worst


def check_resid(x_got, x_old, bias, slabs, n_hi, M):
    """x' == x + (bias + (s0 + s1 + ..)) in fp32 in slab order, bit for bit on the live rows"""
    want = resid_ref(x_old[:M], bias, [s[:M] for s in slabs], n_hi)
    return check_exact(x_got[:M], want, "residual update")


def ln_onehot_bound(acc, rstd, b):
    """(float64 value, allowed distance) of rstd * acc + b for rows of mean exactly 0: acc [M, N] exact, rstd [M] float64, b [N]"""
    t = rstd[:, None] * acc.astype(np.float64)
    v = t + np.asarray(b, dtype=np.float64)[None, :]
    return v, DELTA_RSTD * np.abs(t) + HALF_ULP * np.abs(v)


def check_ln_onehot(got, acc, rstd, b, M, what, gelu=False):
    """every live element within the derived distance of the float64 value (no element exempt); with gelu, through gelu_erf"""
    v, tol = ln_onehot_bound(acc[:M], rstd[:M], b)
    if gelu:
        tol = GELU_LIP * tol + (2.0 ** -23 + 0.49 * 2.0 ** -24 + 3 * 2.0 ** -24) * np.maximum(np.abs(v), np.abs(gelu64(v)))
        v = gelu64(v)
    err = np.abs(got[:M].astype(np.float64) - v)
    bad = err > tol
    assert not bad.any(), "%s: %d of %d elements are outside the derived distance (worst %.3g x it)" % (
        what, int(bad.sum()), bad.size, float((err / np.maximum(tol, 1e-300)).max()))
    return float((err / np.maximum(tol, 1e-300)).max()), float(np.mean(got[:M] != v.astype(np.float32)))


def ln_normaliser(Wg, x, mean, rstd, c1, b):
    """rstd (sum |w' x| + |mean c1|) + |b|: the scale of the fused-LayerNorm algebra  rstd (x W'^T - mean c1) + b"""
    return rstd[:, None] * (np.abs(x.astype(np.float64)) @ np.abs(Wg.astype(np.float64)).T + np.abs(mean[:, None] * c1[None, :].astype(np.float64))) + np.abs(
        np.asarray(b, dtype=np.float64))[None, :]


def ln_algebra32(Wg, x, stats, c1, b, K):
    """an fp32 numpy evaluation of the same algebra (sequential fp32 dot product): the yardstick of the LayerNorm-fused bounds"""
    import torch
    mean64 = stats[:, :, 0].sum(0) / K
    var64 = stats[:, :, 1].sum(0) / K - mean64 * mean64
    mu = mean64.astype(np.float32)
    rstd = (np.float32(1.0) / np.sqrt(var64.astype(np.float32) + LN_EPS)).astype(np.float32)
    xt, wt = torch.from_numpy(np.ascontiguousarray(x.T, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(Wg.T, dtype=np.float32))
    acc = torch.zeros(x.shape[0], Wg.shape[0])
    for k in range(x.shape[1]):
        acc += xt[k][:, None] * wt[k][None, :]
    acc = acc.numpy()
    return (rstd[:, None] * (acc - mu[:, None] * c1[None, :].astype(np.float32)) + np.asarray(b, dtype=np.float32)[None, :]).astype(np.float32)


def ln_pieces(P, stats, c1, b, K):
    """the attention prologue on dense data: q | k | v = rstd (sum of the pieces - mean c1) + b.  P [S][M, N] fp32 pieces, stats
    [nch][M][2] fp64.  Returns (float64 value, the normaliser rstd (sum_p |piece| + |mean c1|) + |b|, an fp32 numpy evaluation of the same
    algebra with the pieces added in piece order)"""
    mean, rstd = mean_rstd64(stats, K)
    c64, b64 = np.asarray(c1, dtype=np.float64), np.asarray(b, dtype=np.float64)
    P64 = P.astype(np.float64)
    v = rstd[:, None] * (P64.sum(0) - mean[:, None] * c64[None, :]) + b64[None, :]
    norm = rstd[:, None] * (np.abs(P64).sum(0) + np.abs(mean[:, None] * c64[None, :])) + np.abs(b64)[None, :]
    var32 = (stats[:, :, 1].sum(0) / K - mean * mean).astype(np.float32)
    rstd32 = (np.float32(1.0) / np.sqrt(var32 + LN_EPS)).astype(np.float32)
    acc = P[0].astype(np.float32).copy()
    for p in range(1, P.shape[0]):
        acc = (acc + P[p].astype(np.float32)).astype(np.float32)
    t = (acc - (mean.astype(np.float32)[:, None] * np.asarray(c1, dtype=np.float32)[None, :]).astype(np.float32)).astype(np.float32)
    y32 = ((rstd32[:, None] * t).astype(np.float32) + np.asarray(b, dtype=np.float32)[None, :]).astype(np.float32)
    return v, norm, y32


def ln_ref64(W, gamma, beta, bias, x):
    """the reference form: normalise first, then the Linear, in float64 (does not cancel)"""
    x64 = x.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(1, keepdims=True)
    xn = (x64 - mean) / np.sqrt(var + np.float64(LN_EPS)) * gamma.astype(np.float64)[None, :] + beta.astype(np.float64)[None, :]
    out = xn @ W.astype(np.float64).T
    return out if bias is None else out + bias.astype(np.float64)[None, :]


def check_ln_dense(got, ref64, norm, yard32, M, what, factor=DENSE_GATE):
    """max |got - ref| / normaliser <= factor x the same figure of the fp32 yardstick"""
    e = float((np.abs(got[:M].astype(np.float64) - ref64[:M]) / norm[:M]).max())
    ey = float((np.abs(yard32[:M].astype(np.float64) - ref64[:M]) / norm[:M]).max())
    assert e <= factor * ey, "%s: normalised error %.3g is %.2f x the fp32 yardstick's %.3g" % (what, e, e / ey if ey else np.inf, ey)
    return e, ey, e / ey if ey else 0.0


def check_onehot(y_got, v_want, what="one-hot attention"):
    """attention output of a (row, head) whose winning score leads by ~200: exactly the winner's V row (two equal winners: their mean)"""
    bad = diff_bits(y_got, v_want)
    assert bad == 0, "%s: %d of %d output elements differ from the selected V row" % (what, bad, np.asarray(v_want).size)
    return bad


def check_cache_untouched(after, before, b_rows, pos, H, Tmax, hd):
    """no cache row other than row `pos` of sequences < b_rows changed"""
    a, b = after.reshape(-1, H, Tmax, hd).copy(), before.reshape(-1, H, Tmax, hd).copy()
    a[:b_rows, :, pos] = 0
    b[:b_rows, :, pos] = 0
    bad = diff_bits(a, b)
    assert bad == 0, "cache: %d floats outside the appended rows changed" % bad
    return bad


# Dense attention against float64, derived (first order, worst case) from the launch's own steps -- the 4 x "fp32 evaluation of
# softmax V" gate of the VQGAN / Chameleon files does not hold for a CORRECT k_attn_decode: its weights are __expf(s - m), i.e.
# exp2 of the scaled argument, whose error grows with the argument ((2 + 1.16 |x|) ulp: the figure of the CUDA C Programming Guide's
# intrinsic table for __expf; HIP documents none for its __expf, the same construction, so it is taken over, not measured),
# and its q carries the 1 ulp of rsqrtf into every score in proportion to the score.  Per (row, head), weight t is off by the relative
#   rel_t = ds_t + eta_t,   ds_t  = scale (sum_i dq_i |k_ti| + |q_i| dk_ti) + (hd + 2) 2^-24 scale sum_i |q_i k_ti|    (the score)
#                           eta_t = (2 n_f + 1.16 (m - s_t)) 2^-23 + n_f 2^-24     (n_f exponential factors: its own, one per
#                                   increase of the wave's running maximum behind it, one in the merge of the waves; their arguments add
#                                   up to m - s_t; each factor multiplies the accumulators once)
# and y = sum_t p_t V_t / sum_t p_t moves by at most  sum_t p_t rel_t |V_t| + (sum_t p_t |V_t|) (sum_t p_t rel_t + 2 n_add 2^-24)
# + p_new dv_new, n_add = the additions of one lane's chain: 2 rows per chunk of its wave, the row-group shuffles, the waves' merge.
def attn_dense_bound(q, dq, K, dk_new, V, dv_new, scale, E, nwa):
    """q, dq [.., hd]; K, V [.., T, hd] float64 with the new token's row last; dk_new, dv_new [.., hd]: absolute error bounds of the
    prologue's fp32 q / k / v.  Returns (float64 reference [.., hd], allowed distance [.., hd])"""
    T, hd = K.shape[-2], K.shape[-1]
    aq, aK, aV = np.abs(q), np.abs(K), np.abs(V)
    s = np.einsum("...d,...td->...t", q, K) * scale
    ds = (hd + 2) * HALF_ULP * np.einsum("...d,...td->...t", aq, aK) * scale + scale * np.einsum("...d,...td->...t", dq, aK)
    ds[..., T - 1] += scale * (aq * dk_new).sum(-1)
    m = s.max(-1, keepdims=True)
    nchunk = -(-T // E)
    pad = np.full(s.shape[:-1] + (nchunk * E - T,), -np.inf)
    cm = np.concatenate([s, pad], -1).reshape(s.shape[:-1] + (nchunk, E)).max(-1)
    n_inc = np.zeros(s.shape[:-1])
    for w in range(nwa):
        c = cm[..., w::nwa]
        if c.shape[-1] > 1:
            run = np.maximum.accumulate(c, -1)
            n_inc = np.maximum(n_inc, (c[..., 1:] > run[..., :-1]).sum(-1))
    n_f = (2 + n_inc)[..., None]
    eta = (2 * n_f + 1.16 * (m - s)) * 2.0 ** -23 + n_f * HALF_ULP
    p = np.exp(s - m)
    p = p / p.sum(-1, keepdims=True)
    rel = ds + eta
    n_add = 2 * (-(-nchunk // nwa)) + int(np.log2(max(E // 2, 1))) + nwa + 2
    base = np.einsum("...t,...td->...d", p, aV)
    tol = np.einsum("...t,...td->...d", p * rel, aV) + base * ((p * rel).sum(-1, keepdims=True) + 2 * n_add * HALF_ULP) + p[..., T - 1:T] * dv_new
    return np.einsum("...t,...td->...d", p, V), 1.01 * tol


def check_attn_dense(y_got, ref64, tol):
    r = np.abs(y_got.astype(np.float64) - ref64) / tol
    assert np.all(r <= 1.0), "attention: %d of %d outputs are outside the derived distance (worst %.3g x it)" % (int((r > 1).sum()), r.size, float(r.max()))
    return float(r.max())


def attn_fp32(q, K, V, scale):
    """an fp32 numpy evaluation of softmax(q K^T) V (figures only)"""
    q32, K32, V32 = q.astype(np.float32), K.astype(np.float32), V.astype(np.float32)
    s32 = (np.einsum("...d,...td->...t", q32, K32) * np.float32(scale)).astype(np.float32)
    w32 = np.exp(s32 - s32.max(-1, keepdims=True)).astype(np.float32)
    return np.einsum("...t,...td->...d", (w32 / w32.sum(-1, keepdims=True)).astype(np.float32), V32).astype(np.float32)
