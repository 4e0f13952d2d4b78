"""Plain numpy statements (float64, and float32 where the kernel's order fixes the bits) of the launches of one RAR position
(wmar_amd/csrc/rar.hip and the decoder_kernels.h kernels it shares with the Taming engine), one per stage of wmar_rar_probe_run.
The packed layouts, the GEMM decompositions and the attention bounds are those of tests/gpt_kernel_reference.py and are imported
from there, not copied; this file adds what only RAR has.  numpy only, nothing from wmar_amd/csrc.
tests/test_rar_kernel_reference.py shows on the CPU that each check built from these statements catches the fault it is there
for (the `fault=` arguments below exist for that file alone); tests/test_gpu_rar_kernels.py and tests/test_gpu_rar_released.py hold the kernels to them.

M rows, MT = 1 / 2 / 4 row tiles for M <= 32 / 64 / 128, KB = D / 8 k-blocks, Ntot = 6 D L + 2 D adaLN columns.

Layouts RAR adds
  sc, mod            packed activations [KB resp. Ntot/8][MTsc][64][4] with MTsc = MTm = row tiles of the adaLN rows: MT, or
                     mt_for(Bhalf) under shared_u (rows at or past 32 MTsc take their modulation from the table).
  adaLN columns      block l at 6 D l: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp (D each);
                     the final layer at 6 D L: scale FIRST, then shift (FinalLayer, rar.py:132).
  mod_u              row-major [32 ceil(T / 32)][Ntot]: row p = the modulations of the "none" condition at position p.
  k_resid_mod        chunk c of nrm = ceil(KB / (4 KPW)) covers k-blocks [c KB / nrm, (c + 1) KB / nrm), KPW = 1 up to 2048 features, else 4;
                     row statistics: thread group gq = 0..7 adds the chunks gq, gq + 8, gq + 16, .. in that order, then the eight
                     groups are added in group order (fp64).  part: [site][nrm][32 MT][2] u64, site_words = nrm * 32 MT * 2.
  k_modulate / k_rar_embed   statistics chunks as k_resid_stats (stat_chunks(KB) of <= 16 k-blocks), summed in chunk order.
"""
import numpy as np

from tests.gpt_kernel_reference import (DENSE_GATE, HALF_ULP, SENTINEL, act_index, attn_chunk_rows, attn_dense_bound, attn_fp32,  # noqa: F401
                                        attn_ref, bf, bf_bits, bits_f32, bx_split, cache_index, check_attn_dense, check_cache_untouched,
                                        check_exact, check_gemm_dense, check_gemm_exact, check_ln_dense, check_onehot, check_pack,
                                        check_stats, diff_bits, fold_slabs, gelu64, gemm_chain, gemm_pieces, gemm_ranges, get_pieces, mt_for,
                                        pack_act, pack_bx, pack_linear, pack_planes, put_pieces, resid_chunk_kblocks, stat_chunks,
                                        stats_ref, uniform_ranges, unpack_act, unpack_planes)

STAGES = ["EMBED", "ADALN", "MOD_IN", "QKV", "ATTN", "PROJ", "RESID_ATTN", "FC1", "FC2", "RESID_MLP", "HEAD"]
EMBED, ADALN, MOD_IN, QKV, ATTN, PROJ, RESID_ATTN, FC1, FC2, RESID_MLP, HEAD = range(11)
LN_EPS = 1e-6                     # RAR's norm_layer and q_norm / k_norm
EPS32 = np.float32(1e-6)
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)
U = 2.0 ** -24                    # half an fp32 ulp, relative


# ------------------------------------------------------------------------------------------------------------------- layouts
def block_offsets(l, D):
    """feature offsets of block l's six adaLN chunks"""
    o = 6 * D * l
    return dict(shift_msa=o, scale_msa=o + D, gate_msa=o + 2 * D, shift_mlp=o + 3 * D, scale_mlp=o + 4 * D, gate_mlp=o + 5 * D)


def final_offsets(L, D, fault=None):
    """the final layer's two chunks: scale first, then shift"""
    o = 6 * D * L
    return dict(shift=o, scale=o + D) if fault == "final_swapped" else dict(scale=o, shift=o + D)


def pack_rows(X, MT):
    """[M, K] (M <= 32 MT, zero padded; rows past 32 MT dropped) -> flat packed activation of MT row tiles"""
    P = np.zeros((32 * MT, X.shape[1]), dtype=X.dtype)
    n = min(len(X), 32 * MT)
    P[:n] = X[:n]
    return pack_act(P, MT)


def rm_kpw(KB):
    return 1 if KB <= 256 else 4


def rm_chunks(KB):
    k = 4 * rm_kpw(KB)
    return (KB + k - 1) // k


def rm_chunk_lists(KB):
    n = rm_chunks(KB)
    return [list(range(c * KB // n, (c + 1) * KB // n)) for c in range(n)]


def stat_chunk_lists(KB):
    n = stat_chunks(KB)
    return [list(range(*resid_chunk_kblocks(KB, n, c))) for c in range(n)]


def site_words(KB, MT):
    return rm_chunks(KB) * MT * 32 * 2


def rm_row_sums(part, fault=None):
    """k_resid_mod's fixed order: part [nrm][M][2] fp64 -> [M][2]; groups gq + 8 i in i order, then the eight groups"""
    n = part.shape[0]
    tot = np.zeros(part.shape[1:])
    for gq in range(8):
        g = np.zeros(part.shape[1:])
        for c in range(gq, n, 8):
            if fault == "drop_chunk17" and c == 16:
                continue
            g = g + part[c]
        tot = tot + g
    return tot


def mod_row_sums(stats, fault=None):
    """k_modulate's order: the chunks one after the other (rounds of 16)"""
    tot = np.zeros(stats.shape[1:])
    for c in range(stats.shape[0]):
        if fault == "drop_chunk17" and c == 16:
            continue
        tot = tot + stats[c]
    return tot


def mean_rstd(sums, K, eps=LN_EPS):
    """float64 (mean, rstd) of rows from [M][2] (sum, sum of squares)"""
    mean = sums[:, 0] / K
    var = sums[:, 1] / K - mean * mean
    return mean, 1.0 / np.sqrt(var + eps)


# ------------------------------------------------------------------------------------------------------------------- embedding
def embed_tokens(tok, cond, ids, ids_stride, Bhalf, p, M, fault=None):
    """the token id every row embeds (-1: cls).  tok given: forward_position's form; None: generate's three cases"""
    if tok is not None:
        return np.asarray(tok, dtype=np.int64)[:M].copy()
    m = np.arange(M)
    if p == 0:
        return np.full(M, -1, dtype=np.int64)
    if p == 1:
        return np.asarray(cond, dtype=np.int64)[:M].copy()
    row = m if fault == "ids_by_m" else m % Bhalf
    return np.asarray(ids, dtype=np.int64).reshape(-1)[row * ids_stride + (p - 2)]


def embed_x(emb, cls, pos, tape, tk, p, fault=None, dtype=np.float32):
    """x = (token vector + pos_embed[p]) + target_aware_pos_embed[p + 1] for p >= 1, fp32 in that order: exact
    (dtype float64: the same sum without the roundings, for the composition)"""
    t = np.where((tk < 0)[:, None], cls[None, :], emb[np.maximum(tk, 0)]).astype(dtype)
    x = (t + pos[p][None, :].astype(dtype)).astype(dtype)
    arow = p if fault == "tape_at_p" else p + 1
    if p >= 1 or fault == "tape_at_0":
        x = (x + tape[arow][None, :].astype(dtype)).astype(dtype)
    return x


def cond_c(emb, tstep, cond, p, dtype=np.float32):
    """c = emb[cond] + timesteps[p]: ONE fp32 addition, exact"""
    return (emb[np.asarray(cond, dtype=np.int64)].astype(dtype) + tstep[p][None, :].astype(dtype)).astype(dtype)


def silu64(c):
    c = np.asarray(c, dtype=np.float64)
    return c / (1.0 + np.exp(-c))


def silu32(c):
    """an fp32 numpy evaluation of c / (1 + exp(-c)) (figures only)"""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (c / (np.float32(1.0) + np.exp(-c).astype(np.float32)).astype(np.float32)).astype(np.float32)


# c / (1 + expf(-c)) on an exact fp32 c: expf 1 ulp (HIP math API) = 2 U of e = exp(-c), which moves 1 + e by at most 2 U e / (1 + e)
# <= 2 U of it; the addition 1 U; the division at most 2 ulp = 4 U (1 U where it is correctly rounded): 7 U of the result.  Where
# exp(-c) overflows (c < -88.72) an fp32 evaluation gives -0 against a float64 value of at most 88.72 exp(-88.72) = 2.6e-37 < 2^-121:
# the absolute term covers that (and a flushed subnormal).
SILU_REL = 7 * U
SILU_ABS = 2.0 ** -121


def check_silu(got, c, what="SiLU"):
    """every element of fp32 `got` within the derived distance of silu64(c); returns (worst / bound, worst of the fp32 numpy
    evaluation / bound)"""
    v = silu64(c)
    tol = SILU_REL * np.abs(v) + SILU_ABS
    err = np.abs(np.asarray(got, dtype=np.float64) - v)
    bad = err > tol
    assert not bad.any(), "%s: %d of %d elements outside the derived distance (worst %.3g x it)" % (what, int(bad.sum()), bad.size, float((err / tol).max()))
    return float((err / tol).max()), float((np.abs(silu32(c).astype(np.float64) - v) / tol).max())


def check_planes(planes_bits, want32, MT, K, M, what="planes", fault=None):
    """the three bf16 planes [K/16][MT][3][64][8] of rows < M are bx_split of the fp32 values `want32` bit for bit (h + m + l == x)"""
    got = unpack_planes(planes_bits, MT, K)[:, :M]
    h, m, l = bx_split(want32[:M])
    want = np.stack([h, m, l])
    bad = diff_bits(got, want)
    assert bad == 0, "%s: %d of %d bf16 piece values differ from the split of the fp32 value" % (what, bad, want.size)
    return bad


def planes_value(planes_bits, MT, K):
    """fp32 h + m + l of unpacked planes (exact: the three pieces of one fp32 value)"""
    p = unpack_planes(planes_bits, MT, K).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):            # (padding rows may hold a sentinel)
        return (p[0] + p[1] + p[2]).astype(np.float32), unpack_planes(planes_bits, MT, K)


def check_planes_consistent(planes_bits, MT, K, M, what="planes"):
    """the planes of rows < M ARE a three-piece split: bx_split(h + m + l) gives them back bit for bit (a dropped third piece, a
    piece rounded the wrong way or a swapped pair does not)"""
    val, got = planes_value(planes_bits, MT, K)
    want = np.stack(bx_split(val[:M]))
    bad = diff_bits(got[:, :M], want)
    assert bad == 0, "%s: %d of %d bf16 piece values are not the split of their own sum" % (what, bad, want.size)
    return val


# ------------------------------------------------------------------------------------------------------------------- modulations
def uncond_table64(emb, tstep, none_id, T, Wada, bada):
    """float64 [T][Ntot]: SiLU(emb[none] + timesteps[p]) Wada^T + bada, and the magnitude sum |terms| + |bias|"""
    c = (emb[none_id][None, :].astype(np.float32) + tstep[:T].astype(np.float32)).astype(np.float32)
    s = silu64(c)
    W = Wada.astype(np.float64)
    return s @ W.T + bada.astype(np.float64)[None, :], np.abs(s) @ np.abs(W).T + np.abs(bada.astype(np.float64))[None, :], c


def effective_mod(mod_rows, mod_u, p, M, Bhalf, shared_u, fault=None):
    """[M][Ntot] the modulation every row takes: rows < Bhalf (all rows without shared_u) their own adaLN row, rows >= Bhalf row p of
    the table.  mod_rows [>= Bhalf or M][Ntot] unpacked with the right MTsc."""
    out = np.array(mod_rows[:M], dtype=mod_rows.dtype, copy=True) if len(mod_rows) >= M else np.concatenate(
        [mod_rows, np.zeros((M - len(mod_rows), mod_rows.shape[1]), dtype=mod_rows.dtype)])
    if shared_u:
        prow = p + 1 if fault == "table_pos_plus" else (p - 1 if fault == "table_pos_minus" else p)
        out[Bhalf:M] = mod_u[prow][None, :]
        if fault == "last_cond_row_uncond":
            out[Bhalf - 1] = mod_u[p]
    return out


def modulate64(x, mean, rstd, gamma, beta, scale, shift):
    """float64 h = ((x - mean) rstd gamma + beta) (1 + scale) + shift and the allowed distance of the kernels' fp32 evaluation:
         mu = float(mean)                 U |mean|
         x - mu                           U |x - mean|                         -> e_t = U (|mean| + |t|)
         rstd: float(var) U, + eps U (rsqrt halves both: U), rsqrtf 1 ulp = 2 U; the product t rstd U -> e_n = rstd e_t + 4 U |n|
         n gamma + beta                   U |n gamma| + U |a|                  -> e_a = |gamma| e_n + U (|n gamma| + |a|)
         1 + scale                        U |u|
         a u + shift                      U |a u| + U |h|                      -> e_h = |u| e_a + |a| U |u| + U (|a u| + |h|)
       (a fused multiply-add drops a product's rounding; second-order terms are not added.)  gamma None: no affine."""
    x = x.astype(np.float64)
    t = x - mean[:, None]
    n = t * rstd[:, None]
    e_t = U * (np.abs(mean)[:, None] + np.abs(t))
    e_n = rstd[:, None] * e_t + 4 * U * np.abs(n)
    if gamma is not None:
        g, b = gamma.astype(np.float64)[None, :], beta.astype(np.float64)[None, :]
        a = n * g + b
        e_a = np.abs(g) * e_n + U * (np.abs(n * g) + np.abs(a))
    else:
        a, e_a = n, e_n
    u = 1.0 + scale.astype(np.float64)
    h = a * u + shift.astype(np.float64)
    e_h = np.abs(u) * e_a + np.abs(a) * U * np.abs(u) + U * (np.abs(a * u) + np.abs(h))
    return h, e_h


def modulate32(x, mean, var, gamma, beta, scale, shift):
    """an fp32 numpy evaluation of the same algebra (figures only)"""
    f = np.float32
    mu = mean.astype(f)[:, None]
    rs = (f(1.0) / np.sqrt(var.astype(f) + EPS32)).astype(f)[:, None]
    r = ((x.astype(f) - mu).astype(f) * rs).astype(f)
    if gamma is not None:
        r = ((r * gamma.astype(f)[None, :]).astype(f) + beta.astype(f)[None, :]).astype(f)
    return ((r * (f(1.0) + scale.astype(f)).astype(f)).astype(f) + shift.astype(f)).astype(f)


def check_modulate(got, x, sums, K, gamma, beta, scale, shift, M, what="modulate"):
    """every live fp32 element of `got` within the derived distance (none exempt).  sums [M][2] in the kernel's order.
    Returns (worst / bound, worst of the fp32 numpy evaluation / bound)"""
    mean, rstd = mean_rstd(sums[:M], K)
    h, tol = modulate64(x[:M], mean, rstd, gamma, beta, scale[:M], shift[:M])
    err = np.abs(got[:M].astype(np.float64) - h)
    bad = err > tol
    assert not bad.any(), "%s: %d of %d elements outside the derived distance (worst %.3g x it; rows %s)" % (
        what, int(bad.sum()), bad.size, float((err / tol).max()), sorted(set(np.nonzero(bad)[0].tolist()))[:8])
    var = sums[:M, 1] / K - mean * mean
    y32 = modulate32(x[:M], mean, var, gamma, beta, scale[:M], shift[:M])
    return float((err / tol).max()), float((np.abs(y32.astype(np.float64) - h) / tol).max())


def gated_fold32(x, gate, bias, slabs, fault=None):
    """x' = x + gate (bias + (s0 + s1 + ..)) in fp32, slab order.  Exact on integer operands with power-of-two gates (every
    intermediate is an integer multiple of the gate below 2^24 of it), with or without a fused multiply-add."""
    use = slabs[:-1] if fault == "missing_slab" and len(slabs) > 1 else slabs
    if fault == "missing_slab6":                                  # slab 6 of 8 (the k_bx<2,8,4> FC2 of RAR-L leaves 8)
        use = [s for i, s in enumerate(slabs) if i != 5]
    acc = fold_slabs([s.astype(np.float32) for s in use])
    if fault == "missing_slab" and len(slabs) == 1:
        acc = np.zeros_like(acc)
    t = (bias.astype(np.float32)[None, :] + acc).astype(np.float32)
    return (x.astype(np.float32) + (gate.astype(np.float32) * t).astype(np.float32)).astype(np.float32)


def gated_fold64(x, gate, bias, slabs):
    """float64 value and the allowed distance of the fp32 fold: S - 1 slab additions, the bias, the product, the sum: each U of its
    result, bounded by the magnitudes"""
    S = len(slabs)
    s64 = [s.astype(np.float64) for s in slabs]
    acc = sum(s64)
    mag = sum(np.abs(s) for s in s64)
    b = bias.astype(np.float64)[None, :]
    g, x = gate.astype(np.float64), x.astype(np.float64)
    v = x + g * (b + acc)
    tol = U * ((S + 1) * np.abs(g) * (mag + np.abs(b)) + np.abs(g * (b + acc)) + np.abs(v))
    return v, tol


# ------------------------------------------------------------------------------------------------------------------- attention, mode 1
def attn_row_groups(hd):
    """RPI: row groups of a wave = 64 / (lanes a cache row is laid on: 8, 16 or 32)"""
    lpra = hd // 4
    return 64 // (8 if lpra <= 8 else (16 if lpra <= 16 else 32))


def piece_sum32(P, RPI):
    """the prologue's fp32 sum of the S pieces: piece p is held by row group p % RPI and added there in piece order; the groups
    meet in an xor butterfly (a balanced tree over the groups in their order)"""
    S = P.shape[0]
    groups = []
    for g in range(RPI):
        acc = np.zeros(P.shape[1:], dtype=np.float32)
        for p in range(g, S, RPI):
            acc = (acc + P[p].astype(np.float32)).astype(np.float32)
        groups.append(acc)
    while len(groups) > 1:
        groups = [(groups[i] + groups[i + 1]).astype(np.float32) for i in range(0, len(groups), 2)]
    return groups[0]


def two_sum32(a, b):
    """fp32 a + b and what the addition rounded away (Knuth's TwoSum, the kernels' two_sum)"""
    f = np.float32
    a, b = np.asarray(a, dtype=f), np.asarray(b, dtype=f)
    s = (a + b).astype(f)
    bb = (s - a).astype(f)
    return s, ((a - (s - bb).astype(f)).astype(f) + (b - bb).astype(f)).astype(f)


def piece_sum32c(P, RPI, bias):
    """the prologue's sum of the q and k pieces plus bias (MODE 1): the order of piece_sum32, every addition's rounding error
    carried along in a second fp32 value (csum4_add), both folded into the result behind the bias (csum4_finish)"""
    f = np.float32
    S = P.shape[0]
    groups = []
    for g in range(RPI):
        s, c = np.zeros(P.shape[1:], dtype=f), np.zeros(P.shape[1:], dtype=f)
        for p in range(g, S, RPI):
            s, e = two_sum32(s, P[p])
            c = (c + e).astype(f)
        groups.append((s, c))
    while len(groups) > 1:
        nxt = []
        for i in range(0, len(groups), 2):
            (s, c), (ps, pc) = groups[i], groups[i + 1]
            s, e = two_sum32(s, ps)
            nxt.append((s, (c + (pc + e).astype(f)).astype(f)))
        groups = nxt
    s, c = groups[0]
    t, e = two_sum32(s, np.broadcast_to(bias.astype(f), s.shape))
    return (t + (c + e).astype(f)).astype(f)


def head_sum32(v):
    """the prologue's fp32 sum over the hd values of a head: four values per lane ((a + b) + c) + d, the lanes (padded with zeros to
    8 / 16 / 32) in an xor butterfly.  [.., hd] -> [.., 1]"""
    f = np.float32
    hd = v.shape[-1]
    lanes = v.astype(f).reshape(v.shape[:-1] + (hd // 4, 4))
    s = lanes[..., 0]
    for j in range(1, 4):
        s = (s + lanes[..., j]).astype(f)
    lpr = 64 // attn_row_groups(hd)
    if lpr > hd // 4:
        s = np.concatenate([s, np.zeros(s.shape[:-1] + (lpr - hd // 4,), dtype=f)], -1)
    while s.shape[-1] > 1:
        s = (s[..., 0::2] + s[..., 1::2]).astype(f)
    return s


def attn_prologue(P, bias, qn_w, qn_b, kn_w, kn_b, H, hd, fault=None):
    """The prologue of k_attn_decode<.., MODE 1> / k_attn_decode80: r = (sum of the pieces) + bias, q and k LayerNorm-ed over the hd
    values of their head (eps 1e-6, affine), v as it is.  The q and k pieces are added with their rounding errors carried along
    (piece_sum32c: with several pieces an element that cancels would otherwise keep roundings the norm scales up), v plainly;
    at head_dim 80 (k_attn_decode80, RAR-XL: tokens pinned against the oracle) q and k take the plain sum as well.
    P [S][M, 3 D] fp32.
    Returns float64 (q, k, v) [M, H, hd], the same in an fp32 numpy evaluation, and the normalisers of q and k."""
    if fault == "drop_piece3":                                    # S = 3 on four row groups (head_dim 48): group 2's piece never added
        P = P[:2]
    S, M, N = P.shape
    D = N // 3
    r64 = P.astype(np.float64).sum(0) + bias.astype(np.float64)[None, :]
    r32 = (piece_sum32(P, attn_row_groups(hd)) + bias.astype(np.float32)[None, :]).astype(np.float32)       # v: the plain sum
    if hd != 80:                                                  # q, k: errors carried (k_attn_decode80 keeps the plain sum)
        r32[:, :2 * D] = piece_sum32c(P[:, :, :2 * D], attn_row_groups(hd), bias[:2 * D])
    out64, out32, norms = [], [], []
    for which, (w, b) in enumerate(((qn_w, qn_b), (kn_w, kn_b), (None, None))):
        if which == 1 and fault == "knorm_with_qnorm":
            w, b = qn_w, qn_b
        if which == 2 and fault == "v_normed":
            w, b = kn_w, kn_b
        v64 = r64[:, which * D:(which + 1) * D].reshape(M, H, hd)
        v32 = r32[:, which * D:(which + 1) * D].reshape(M, H, hd)
        if w is None or (which == 1 and fault == "k_cached_before_norm"):
            out64.append(v64); out32.append(v32); norms.append(np.abs(v64))
            continue
        eps = 1e-5 if fault == "eps_1e-5" else LN_EPS
        mean = v64.mean(-1, keepdims=True)
        dv = v64 - mean
        rs = 1.0 / np.sqrt((dv * dv).mean(-1, keepdims=True) + eps)
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        out64.append(dv * rs * w64 + b64)
        norms.append(rs * (np.abs(v64) + np.abs(mean)) * np.abs(w64) + np.abs(b64))
        f = np.float32
        m32 = (head_sum32(v32) * f(1.0 / hd)).astype(f)
        d32 = (v32 - m32).astype(f)
        rs32 = (f(1.0) / np.sqrt((head_sum32((d32 * d32).astype(f)) * f(1.0 / hd)).astype(f) + f(eps))).astype(f)
        out32.append((((d32 * rs32).astype(f) * w.astype(f)).astype(f) + b.astype(f)).astype(f))
    return out64, out32, norms


# the prologue's fp32 q / k against float64: hd additions for the mean and hd for the variance move either by at most hd U of its
# magnitude, the subtraction, rsqrtf (2 U), the two products and the addition a few U more: (2 hd + 8) U of the normaliser
def prologue_tol(norm, hd):
    return (2 * hd + 8) * U * norm


def check_appended(got, ref64, norm, yard32, what):
    """appended K / V rows: max |got - ref| / normaliser <= 2 x the same figure of the fp32 numpy evaluation of the prologue"""
    M = got.shape[0]
    return check_ln_dense(got.reshape(M, -1), ref64.reshape(M, -1), np.maximum(norm.reshape(M, -1), 1e-300), yard32.reshape(M, -1), M, what, factor=2.0)


def attn_mode1_ref(q64, K64, V64, hd, fault=None, E=None):
    """softmax(q K^T / sqrt(hd)) V in float64 over [.., T, hd] caches with the new row last"""
    if fault == "skip_chunk" and E is not None and K64.shape[-2] > E:
        keep = np.ones(K64.shape[-2], dtype=bool)
        keep[:E] = False
        K64, V64 = K64[..., keep, :], V64[..., keep, :]
    s = np.einsum("...d,...td->...t", q64, K64) / np.sqrt(hd)
    w = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("...t,...td->...d", w / w.sum(-1, keepdims=True), V64)


def attn_loop_rows(T, E, hd, fault=None):
    """The streaming loop of k_attn_decode<.., 1, 1> / k_attn_decode80<1> (one wave, two buffers) as the list of rows it weighs:
    chunk c holds rows c E .. c E + E - 1; buffer A takes the even chunks and buffer B the odd ones, each refilled two chunks ahead;
    loads clamp to row T - 1; the slot of row T - 1 is replaced by the new row from registers; slots at or past T are masked.
    Returns [(t, src, tail_src)]: row t weighed with the K / V of `src` (-1: the new row held in registers, else that cache row as it
    lies in front of the launch) and, at head_dim 80, the score's tail partial (floats 64..79) taken from `tail_src`.
    `fault` plants what tests/test_gpu_rar_released.py exists for (tests/test_rar_kernel_reference.py shows each caught)."""
    nchunk = -(-T // E)
    out = []
    for c in range(nchunk):
        if fault == "skip_last_odd" and nchunk % 2 == 1 and c == nchunk - 1:
            continue
        cs = 1 if (fault == "refill_b_chunk1" and c % 2 == 1 and c >= 3) else c         # buffer B's refill reads chunk 1 again
        for j in range(E):
            t = c * E + j
            if t >= T:
                continue
            stale = fault == "stale_append" and 2 <= (T - 1) % E <= 5
            src = -1 if (t >= T - 1 and not stale) else min(cs * E + j, T - 1)
            tail = src
            if fault == "tail_wrong_row" and hd == 80:                                  # quad u of the neighbouring 16-lane row
                j2 = 4 * (j // 4) + ((j % 4) ^ 1)
                t2 = c * E + j2
                tail = -1 if t2 >= T - 1 else min(cs * E + j2, T - 1)
            out.append((t, src, tail))
    return out


def attn_loop64(q, Kc, Vc, knew, vnew, T, hd, E, fault=None):
    """softmax(q K^T / sqrt(hd)) V in float64 over the rows of attn_loop_rows.  q, knew, vnew [.., hd]; Kc, Vc [.., Tmax, hd]: the
    cache in front of the launch (rows at or past T - 1 stale)."""
    rows = attn_loop_rows(T, E, hd, fault)
    f8 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    q, Kc, Vc, knew, vnew = f8(q), f8(Kc), f8(Vc), f8(knew), f8(vnew)
    pick = lambda C, new, r: new if r < 0 else C[..., r, :]  # noqa: E731
    nm = min(hd, 64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.stack([(q[..., :nm] * pick(Kc, knew, src)[..., :nm]).sum(-1) + (q[..., nm:] * pick(Kc, knew, tl)[..., nm:]).sum(-1)
                      for _, src, tl in rows], -1) / np.sqrt(hd)
        V = np.stack([pick(Vc, vnew, src) for _, src, _ in rows], -2)
        w = np.exp(s - s.max(-1, keepdims=True))
        return np.einsum("...t,...td->...d", w / w.sum(-1, keepdims=True), V)


# ------------------------------------------------------------------------------------------------------------------- GELU
def gelu_tanh64(v):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + np.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))


# gelu_erf on an fp32 pre-activation v (tests/gpt_kernel_reference.py derives it): erff 4 ulp of a value below 1, the scaled
# argument's rounding, three more roundings
GELU_REL = 2.0 ** -23 + 0.49 * U + 3 * U


def check_gelu(got, pre32, what="GELU", pre_tol=None):
    """fp32 `got` within the derived distance of gelu64(pre32); pre_tol: the pre-activation's own allowed error (carried by |gelu'| <= 1.13)"""
    v = pre32.astype(np.float64)
    g = gelu64(v)
    tol = GELU_REL * np.maximum(np.abs(v), np.abs(g)) + 2.0 ** -126
    if pre_tol is not None:
        tol = tol + 1.13 * pre_tol
    err = np.abs(np.asarray(got, dtype=np.float64) - g)
    bad = err > tol
    assert not bad.any(), "%s: %d of %d elements outside the derived distance (worst %.3g x it)" % (what, int(bad.sum()), bad.size, float((err / tol).max()))
    return float((err / tol).max())


# ------------------------------------------------------------------------------------------------------------------- bx GEMMs
def bx_ranges(NT, S, PER):
    """K slice s of a k_bx launch with PER 16-k steps per wave: 4 waves x PER x 16 = 64 PER features = 8 PER k-blocks"""
    return uniform_ranges(NT, lambda s: (s * 8 * PER, (s + 1) * 8 * PER), S)


def bx_pieces64(Wg, X, NT, S, PER, fault=None):
    """float64 pieces [S][M, N] of a k_bx launch.  A slab's 8 PER k-blocks go to four waves of PER 16-feature steps (2 PER k-blocks)
    each; fault "drop_steps_5_8": every wave stops behind its fourth step (what a PER 8 instance with a PER 4 loop would leave)."""
    if fault is None:
        return gemm_pieces(Wg, X, bx_ranges(NT, S, PER))[0]
    assert fault == "drop_steps_5_8" and PER >= 8
    out = 0.0
    for w in range(4):
        out = out + gemm_pieces(Wg, X, uniform_ranges(NT, lambda s: (s * 8 * PER + w * 2 * PER, s * 8 * PER + w * 2 * PER + 8), S))[0]
    return out


# ------------------------------------------------------------------------------------------------------------------- the plan
def _pick_split(tiles, KB, NW=4):
    best, best_eff = 1, 0.0
    for S in range(1, 9):
        if KB // (S * NW) < 8 and S > 1:
            break
        wgs = tiles * S
        eff = wgs / (((wgs + 255) // 256) * 256.0)
        if eff > best_eff + 0.02:
            best_eff, best = eff, S
    return best


def _bx_shape(tiles, KU):
    best = (0, 0)
    for per in (4, 5, 8, 10, 16, 20):
        if KU % (4 * per):
            continue
        S = KU // (4 * per)
        if S < 1 or S > 8 or tiles * S > 256:
            continue
        if tiles * S > tiles * best[0]:
            best = (S, per)
    return best


def _row_tiles(MT, NT):
    return 4 if (MT % 4 == 0 and NT * (MT // 2) > 256) else (2 if MT % 2 == 0 else 1)


def expected_plan(D, H, F, L, V, max_batch, M, Bhalf, shared_u, no_bx=False, fused=True):
    """The dispatch rules of rar.hip written down a second time (wmar_rar_create, RarPlan): what wmar_rar_probe_plan must report for
    M rows.  A change of the dispatch that moves a case to another kernel shows as a difference here."""
    hd = D // H
    MT, MTmax = mt_for(M), mt_for(2 * max_batch)
    MTc = mt_for(Bhalf) if shared_u else MT
    KBD, KBF, Ntot = D // 8, F // 8, 6 * D * L + 2 * D
    qkv = proj = fc2 = (0, 0)
    bx_ok = bx_fc1 = False
    if MTmax >= 4:
        qkv, proj, fc2 = _bx_shape(3 * D // 64, D // 16), _bx_shape(D // 32, D // 16), _bx_shape(D // 64, F // 16)
        bx_fc1 = D == 1280 and F // 32 <= 256
        bx_ok = D % 64 == 0 and 0 < qkv[0] <= 8 and proj[0] > 0 and fc2[0] > 0
    bx = MT == 4 and bx_ok and not no_bx
    tiles = (D // 32) * (MT // 2) if MT % 2 == 0 else (D // 32) * MT
    S_proj, S_fc2 = (proj[0], fc2[0]) if bx else (_pick_split(tiles, KBD), _pick_split(tiles, KBF))
    ada_bx = D == 1280 and Ntot % 128 == 0 and MTmax >= 2 and not no_bx and MTc == 2
    fc1_bx = bx and bx_fc1
    kpw = rm_kpw(KBD)
    mtw = 2 if MT % 2 == 0 else 1
    out = dict(MT=MT, MTc=MTc, bx=int(bx), ada_bx=int(ada_bx), fc1_bx=int(fc1_bx), rowmajor=int(bx and hd == 80), S_qkv=qkv[0] if bx else 1,
               S_proj=S_proj, S_fc2=S_fc2, PER_qkv=qkv[1] if bx else 0, PER_proj=proj[1] if bx else 0, PER_fc2=fc2[1] if bx else 0,
               nch=stat_chunks(KBD), nrm=rm_chunks(KBD), kpw=kpw, fused=int(fused), fallbacks=0,
               ada_tiles=0 if ada_bx else _row_tiles(MTc, Ntot // 32), fc1_tiles=0 if fc1_bx else _row_tiles(MT, F // 32),
               head_tiles=_row_tiles(MT, V // 32), attn_waves=1, stages=list(STAGES))
    rm = (lambda S: "k_resid_mod<%d,%d,0>" % (S, kpw)) if fused else (lambda S: "k_resid_mod<%d,%d,1>+k_resid_mod<%d,%d,2>" % (S, kpw, S, kpw))
    out["roles"] = dict(
        embed="k_rar_embed", adaln="k_bx<4,20,2>" if ada_bx else "k_gemm<%d,EPI_PACKED>" % out["ada_tiles"], mod_in="k_modulate",
        qkv=("k_bx<2,%d,4>%s" % (qkv[1], " rowmajor" if hd == 80 else "")) if bx else "k_gemm<%d,EPI_PACKED>" % mtw,
        attn=("k_attn_decode80<1>%s" % (" rowmajor" if bx else "")) if hd == 80 else "k_attn_decode<%d,1,1>" % hd,
        proj="k_bx<1,%d,4>" % proj[1] if bx else "k_gemm<%d,EPI_PACKED>" % mtw, resid_attn=rm(S_proj), resid_mlp=rm(S_fc2),
        fc1="k_bx<1,10,4,GELU,8,XF>" if fc1_bx else "k_gemm<%d,EPI_GELU>%s" % (out["fc1_tiles"], " planes" if bx else ""),
        fc2="k_bx<2,%d,4>" % fc2[1] if bx else "k_gemm<%d,EPI_PACKED>" % mtw, head="k_gemm<%d,EPI_LOGITS>" % out["head_tiles"])
    return out


# The released sizes of RarARMMWrapper (wmar_amd/models/rar_wrapper.py: _RAR_SIZES gives width, depth, F; 16 heads each) and two
# synthetic shapes that select the remaining launch_bx4 cases, as (D, H, F), and what their plans at max_batch 64 must say: written
# down by hand from the dispatch, NOT computed by expected_plan -- the CPU test holds expected_plan to it, the GPU tests the engine.
RELEASED_SHAPES = {"RB": (768, 16, 3072), "RL": (1024, 16, 4096), "RXL": (1280, 16, 5120), "RXXL": (1408, 16, 6144),
                   "P16": (256, 4, 8192), "P20": (256, 4, 6400)}
RELEASED_WRAPPER = {"rar_b": ("RB", 24), "rar_l": ("RL", 24), "rar_xl": ("RXL", 32), "rar_xxl": ("RXXL", 40)}


def released_pins():
    """{(engine, rows): facts}; `roles` holds kernel names by role"""
    pins = {}
    for M in (20, 64):
        mt = 1 if M <= 32 else 2
        for name, hd, Sp, Sf, nch in (("RB", 48, 3, 8, 6), ("RL", 64, 4, 8, 8), ("RXL", 80, 5, 6, 10), ("RXXL", 88, 5, 5, 11)):
            pins[(name, M)] = dict(bx=0, S_qkv=1, S_proj=Sp, S_fc2=Sf, nch=nch, nrm=4 * nch, roles=dict(
                fc2="k_gemm<%d,EPI_PACKED>" % mt, resid_attn="k_resid_mod<%d,1,0>" % Sp, resid_mlp="k_resid_mod<%d,1,0>" % Sf,
                fc1="k_gemm<%d,EPI_GELU>" % mt, attn="k_attn_decode80<1>" if hd == 80 else "k_attn_decode<%d,1,1>" % hd))
    for M in (97, 127, 128):
        pins[("RB", M)] = dict(bx=1, S_qkv=3, PER_qkv=4, S_proj=3, PER_proj=4, S_fc2=6, PER_fc2=8, nch=6, nrm=24, rowmajor=0, roles=dict(
            qkv="k_bx<2,4,4>", proj="k_bx<1,4,4>", fc2="k_bx<2,8,4>", resid_attn="k_resid_mod<3,1,0>", resid_mlp="k_resid_mod<6,1,0>",
            fc1="k_gemm<2,EPI_GELU> planes", attn="k_attn_decode<48,1,1>"))
        pins[("RL", M)] = dict(bx=1, S_qkv=4, PER_qkv=4, S_proj=4, PER_proj=4, S_fc2=8, PER_fc2=8, nch=8, nrm=32, rowmajor=0, roles=dict(
            qkv="k_bx<2,4,4>", proj="k_bx<1,4,4>", fc2="k_bx<2,8,4>", resid_attn="k_resid_mod<4,1,0>", resid_mlp="k_resid_mod<8,1,0>",
            fc1="k_gemm<2,EPI_GELU> planes", attn="k_attn_decode<64,1,1>"))
        pins[("RXL", M)] = dict(bx=1, fc1_bx=1, rowmajor=1, S_qkv=4, PER_qkv=5, S_proj=5, PER_proj=4, S_fc2=8, PER_fc2=10, nch=10, nrm=40,
                                roles=dict(qkv="k_bx<2,5,4> rowmajor", fc2="k_bx<2,10,4>", fc1="k_bx<1,10,4,GELU,8,XF>",
                                           resid_mlp="k_resid_mod<8,1,0>", attn="k_attn_decode80<1> rowmajor"))
        pins[("RXXL", M)] = dict(bx=0, S_qkv=1, S_proj=5, S_fc2=8, nch=11, nrm=44, roles=dict(
            qkv="k_gemm<2,EPI_PACKED>", fc2="k_gemm<2,EPI_PACKED>", resid_attn="k_resid_mod<5,1,0>", resid_mlp="k_resid_mod<8,1,0>",
            fc1="k_gemm<4,EPI_GELU>", attn="k_attn_decode<88,1,1>"))
        for name, S, PER in (("P16", 8, 16), ("P20", 5, 20)):
            pins[(name, M)] = dict(bx=1, S_qkv=1, PER_qkv=4, S_proj=1, PER_proj=4, S_fc2=S, PER_fc2=PER, roles=dict(
                fc2="k_bx<2,%d,4>" % PER, resid_mlp="k_resid_mod<%d,1,0>" % S, fc1="k_gemm<4,EPI_GELU> planes", attn="k_attn_decode<64,1,1>"))
    return pins


def check_pins(plan, pins, what=""):
    for k, v in pins.items():
        if k == "roles":
            for role, kern in v.items():
                assert plan["roles"][role] == kern, (what, role, plan["roles"][role], kern)
        else:
            assert plan[k] == v, (what, k, plan[k], v)


# ------------------------------------------------------------------------------------------------------------------- composition
def _gelu64_torch(v):
    """gelu64 through torch's float64 erf: the same values to a few 2^-53, without a Python call per element (the composition
    at released widths evaluates 128 x 6144 of them per position)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))).numpy()


def position64(sd, cfg, tk, cond, p, kc, vc):
    """One position in float64 numpy, composed of the statements above (the CPU test holds it to oracle.rar_oracle.rar_position).
    sd: numpy state dict with the checkpoint's keys; tk [M] token ids (-1 cls); kc / vc: per block [M, H, t, hd] or None."""
    d, H, hd, L = cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.num_hidden_layers
    M = len(tk)
    f8 = lambda k: sd[k].astype(np.float64)  # noqa: E731
    x = embed_x(sd["embeddings.weight"], sd["cls_token"][0, 0], sd["pos_embed"][0], sd["target_aware_pos_embed"][0], np.asarray(tk), p,
                dtype=np.float64)
    sc = silu64(cond_c(sd["embeddings.weight"], sd["timesteps_embeddings"][0], cond, p, dtype=np.float64))
    nk, nv = [], []

    def ln(x, gamma, beta, scale, shift):
        sums = np.stack([x.sum(1), (x * x).sum(1)], 1)
        mean, rstd = mean_rstd(sums, d)
        n = (x - mean[:, None]) * rstd[:, None]
        if gamma is not None:
            n = n * gamma[None, :] + beta[None, :]
        return n * (1.0 + scale) + shift

    for i in range(L):
        pre = "blocks.%d." % i
        mod = sc @ f8(pre + "adaLN_modulation.1.weight").T + f8(pre + "adaLN_modulation.1.bias")
        o = block_offsets(0, d)
        ch = {k: mod[:, v:v + d] for k, v in o.items()}
        h = ln(x, f8(pre + "norm1.weight"), f8(pre + "norm1.bias"), ch["scale_msa"], ch["shift_msa"])
        qkv = (h @ f8(pre + "attn.qkv.weight").T)[None]
        (q, k, v), _, _ = attn_prologue(qkv, sd[pre + "attn.qkv.bias"], sd[pre + "attn.q_norm.weight"], sd[pre + "attn.q_norm.bias"],
                                        sd[pre + "attn.k_norm.weight"], sd[pre + "attn.k_norm.bias"], H, hd)
        kk = k[:, :, None] if kc is None else np.concatenate([kc[i], k[:, :, None]], 2)
        vv = v[:, :, None] if vc is None else np.concatenate([vc[i], v[:, :, None]], 2)
        nk.append(kk); nv.append(vv)
        y = attn_mode1_ref(q, kk, vv, hd).reshape(M, d)
        x = x + ch["gate_msa"] * (y @ f8(pre + "attn.proj.weight").T + f8(pre + "attn.proj.bias"))
        h2 = ln(x, f8(pre + "norm2.weight"), f8(pre + "norm2.bias"), ch["scale_mlp"], ch["shift_mlp"])
        h2 = _gelu64_torch(h2 @ f8(pre + "mlp.fc1.weight").T + f8(pre + "mlp.fc1.bias"))
        x = x + ch["gate_mlp"] * (h2 @ f8(pre + "mlp.fc2.weight").T + f8(pre + "mlp.fc2.bias"))
    fm = sc @ f8("adaln_before_head.adaLN_modulation.1.weight").T + f8("adaln_before_head.adaLN_modulation.1.bias")
    fo = final_offsets(0, d)
    x = ln(x, None, None, fm[:, fo["scale"]:fo["scale"] + d], fm[:, fo["shift"]:fo["shift"] + d])
    return x @ f8("lm_head.weight").T + f8("lm_head.bias"), nk, nv
