"""CPU proof that the checks of tests/rar_kernel_reference.py bite: each test plants ONE fault into the numpy statement of a
kernel's output -- the faults a 5e-4 logit gate behind a LayerNorm lets through -- and shows its check failing, and passing on the
unmodified statement.  The "kernel outputs" are fp32 numpy evaluations built from the reference module's own statements.  The
composition of the float64 statements is held to oracle.rar_oracle.rar_position (head_dim 32, 48 and 88).  The plans of the four
released sizes are pinned against a table written down by hand, and the faults tests/test_gpu_rar_released.py exists for -- a k_bx
that stops behind step 4 at PER 8, slab 6 of 8, the third QKV piece, buffer B's refill, the last chunk of an odd count, a stale
appended row at chunk phase 2..5, the tail partial of the wrong lane row -- are planted into the loop statement attn_loop64."""
import numpy as np
import pytest
import torch

from tests import rar_kernel_reference as R

RS = np.random.RandomState
D, H, HD, L, NTOT = 64, 2, 32, 2, 6 * 64 * 2 + 2 * 64


def _fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ------------------------------------------------------------------------------------------------------------------- modulation
def _mod_case(seed, M=66, Bhalf=33, p=3, small_var=False):
    rs = RS(seed)
    x = (rs.standard_normal((M, D)) * (0.05 if small_var else 1.0) + rs.standard_normal((M, 1))).astype(np.float32)
    mod = (rs.standard_normal((R.mt_for(Bhalf) * 32, NTOT)) * 0.5).astype(np.float32)
    table = (rs.standard_normal((32, NTOT)) * 0.5).astype(np.float32)
    gamma, beta = (1 + 0.1 * rs.standard_normal(D)).astype(np.float32), (0.1 * rs.standard_normal(D)).astype(np.float32)
    st = R.stats_ref(x, R.stat_chunk_lists(D // 8))
    return x, mod, table, gamma, beta, R.mod_row_sums(st), M, Bhalf, p


def _sim_modulate(x, sums, gamma, beta, scale, shift, eps=None):
    mean = sums[:, 0] / D
    var = sums[:, 1] / D - mean * mean
    if eps is not None:                                           # a kernel with another eps: the same fp32 algebra, that eps
        f = np.float32
        rs = (f(1.0) / np.sqrt(var.astype(f) + f(eps))).astype(f)[:, None]
        r = ((x - mean.astype(f)[:, None]).astype(f) * rs).astype(f)
        r = ((r * gamma[None, :]).astype(f) + beta[None, :]).astype(f)
        return ((r * (f(1.0) + scale).astype(f)).astype(f) + shift).astype(f)
    return R.modulate32(x, mean, var, gamma, beta, scale, shift)


@pytest.mark.parametrize("fault", [None, "last_cond_row_uncond", "table_pos_plus", "table_pos_minus"])
def test_shared_rows_read_the_right_modulation(fault):
    """the row-33 escape (the last conditional row takes the unconditional table, in this one modulation only) and a table row off by one"""
    x, mod, table, gamma, beta, sums, M, Bhalf, p = _mod_case(1)
    o = R.block_offsets(1, D)
    good = R.effective_mod(mod, table, p, M, Bhalf, True)
    eff = R.effective_mod(mod, table, p, M, Bhalf, True, fault=fault)
    got = _sim_modulate(x, sums, gamma, beta, eff[:, o["scale_msa"]:o["scale_msa"] + D], eff[:, o["shift_msa"]:o["shift_msa"] + D])
    args = (got, x, sums, D, gamma, beta, good[:, o["scale_msa"]:o["scale_msa"] + D], good[:, o["shift_msa"]:o["shift_msa"] + D], M)
    if fault is None:
        r, r32 = R.check_modulate(*args)
        assert r <= 1.0 and r32 <= 1.0
    else:
        _fails(R.check_modulate, *args)
        if fault == "last_cond_row_uncond":                       # and the message names the row
            with pytest.raises(AssertionError, match=r"rows \[32\]"):
                R.check_modulate(*args)


def test_sc_is_indexed_with_its_own_row_tiles():
    """sc has MTsc row tiles under shared_u; a consumer (or producer) that uses MT reads other rows' values"""
    rs = RS(2)
    M, Bhalf = 66, 33
    MT, MTc = R.mt_for(M), R.mt_for(Bhalf)
    c = rs.standard_normal((32 * MTc, D)).astype(np.float32)
    sc = R.silu32(c)
    flat_good = R.pack_rows(sc, MTc)
    R.check_silu(R.unpack_act(flat_good, MTc, D)[:Bhalf], c[:Bhalf])
    flat_bad = R.pack_rows(sc, MT)[:flat_good.size]               # written with MT where MTsc belongs
    _fails(R.check_silu, R.unpack_act(flat_bad, MTc, D)[:Bhalf], c[:Bhalf])


@pytest.mark.parametrize("where", ["block", "final"])
def test_shift_and_scale_swapped(where):
    x, mod, table, gamma, beta, sums, M, Bhalf, p = _mod_case(3)
    eff = R.effective_mod(mod, table, p, M, Bhalf, True)
    if where == "block":
        o = R.block_offsets(0, D)
        sc0, sh0, g, b = o["scale_mlp"], o["shift_mlp"], gamma, beta
        bad = dict(scale=sh0, shift=sc0)
    else:
        o, g, b = R.final_offsets(L, D), None, None
        sc0, sh0 = o["scale"], o["shift"]
        bad = R.final_offsets(L, D, fault="final_swapped")
        assert o["scale"] < o["shift"], "FinalLayer: scale first"
    mean = sums[:, 0] / D
    var = sums[:, 1] / D - mean * mean
    args = lambda got: (got, x, sums, D, g, b, eff[:, sc0:sc0 + D], eff[:, sh0:sh0 + D], M)  # noqa: E731
    R.check_modulate(*args(R.modulate32(x, mean, var, g, b, eff[:, sc0:sc0 + D], eff[:, sh0:sh0 + D])))
    _fails(R.check_modulate, *args(R.modulate32(x, mean, var, g, b, eff[:, bad["scale"]:bad["scale"] + D], eff[:, bad["shift"]:bad["shift"] + D])))


def test_eps_is_1e_6():
    for small in (False, True):
        x, mod, table, gamma, beta, sums, M, Bhalf, p = _mod_case(4, small_var=small)
        eff = R.effective_mod(mod, table, p, M, Bhalf, True)
        sc, sh = eff[:, D:2 * D], eff[:, :D]
        R.check_modulate(_sim_modulate(x, sums, gamma, beta, sc, sh, eps=1e-6), x, sums, D, gamma, beta, sc, sh, M)
        _fails(R.check_modulate, _sim_modulate(x, sums, gamma, beta, sc, sh, eps=1e-5), x, sums, D, gamma, beta, sc, sh, M)


@pytest.mark.parametrize("kernel", ["k_modulate", "k_resid_mod"])
def test_the_17th_statistics_chunk(kernel):
    """2176 features: 17 chunks -- the second round of k_modulate's 16-wide loop, the third poll slot of k_resid_mod's group 0"""
    rs = RS(5)
    K, M = 2176, 5
    x = (rs.standard_normal((M, K)) + 0.5).astype(np.float32)
    chunks = R.stat_chunk_lists(K // 8) if kernel == "k_modulate" else R.rm_chunk_lists(K // 8)
    assert len(chunks) == 17 and (kernel == "k_modulate" or R.rm_kpw(K // 8) == 4)
    st = R.stats_ref(x, chunks)
    fn = R.mod_row_sums if kernel == "k_modulate" else R.rm_row_sums
    sums, bad = fn(st), fn(st, fault="drop_chunk17")
    z = np.zeros((M, K), dtype=np.float32)
    mean = sums[:, 0] / K
    good = R.modulate32(x, mean, sums[:, 1] / K - mean * mean, None, None, z, z)
    mb = bad[:, 0] / K
    R.check_modulate(good, x, sums, K, None, None, z, z, M)
    _fails(R.check_modulate, R.modulate32(x, mb, bad[:, 1] / K - mb * mb, None, None, z, z), x, sums, K, None, None, z, z, M)


def test_resid_mod_chunking_and_site_words():
    for KB, kpw, n in ((16, 1, 4), (40, 1, 10), (160, 1, 40), (256, 1, 64), (272, 4, 17), (1024, 4, 64)):
        assert (R.rm_kpw(KB), R.rm_chunks(KB)) == (kpw, n)
        ch = R.rm_chunk_lists(KB)
        assert sorted(sum(ch, [])) == list(range(KB)) and max(len(c) for c in ch) <= 4 * kpw
        assert R.site_words(KB, 2) == n * 64 * 2
    # the fixed order: groups gq + 8 i, then the eight groups -- differs from the plain chunk order in the last bits, not in value
    rs = RS(6)
    st = rs.standard_normal((40, 3, 2)) * 1e3
    a, b = R.rm_row_sums(st), R.mod_row_sums(st)
    assert np.allclose(a, b, rtol=1e-13) and np.array_equal(R.rm_row_sums(st[:8]), R.mod_row_sums(st[:8]))


# ------------------------------------------------------------------------------------------------------------------- the gated fold
@pytest.mark.parametrize("fault", ["missing_slab", "wrong_gate"])
def test_gated_fold(fault):
    rs = RS(7)
    M, S = 9, 3
    x = rs.randint(-64, 65, size=(M, D)).astype(np.float32)
    slabs = [rs.randint(-512, 513, size=(M, D)).astype(np.float32) for _ in range(S)]
    bias = rs.randint(-2, 3, size=D).astype(np.float32)
    mod = (2.0 ** rs.randint(-2, 3, size=(M, NTOT))).astype(np.float32)
    o = R.block_offsets(0, D)
    gate = mod[:, o["gate_msa"]:o["gate_msa"] + D]
    want = R.gated_fold32(x, gate, bias, slabs)
    v, tol = R.gated_fold64(x, gate, bias, slabs)
    assert np.array_equal(want.astype(np.float64), v), "integer operands with power-of-two gates: the fp32 fold is exact"
    R.check_exact(want, v.astype(np.float32), "gated fold")
    got = R.gated_fold32(x, gate, bias, slabs, fault="missing_slab") if fault == "missing_slab" else R.gated_fold32(
        x, mod[:, o["gate_mlp"]:o["gate_mlp"] + D], bias, slabs)            # the gate taken from the wrong sixth
    _fails(R.check_exact, got, want, "gated fold")
    assert np.any(np.abs(got.astype(np.float64) - v) > tol)
    # dense operands: the fp32 fold stays inside the derived distance
    xs, ss = rs.standard_normal((M, D)).astype(np.float32), [rs.standard_normal((M, D)).astype(np.float32) for _ in range(S)]
    gd = rs.standard_normal((M, D)).astype(np.float32)
    vd, td = R.gated_fold64(xs, gd, bias, ss)
    assert np.all(np.abs(R.gated_fold32(xs, gd, bias, ss).astype(np.float64) - vd) <= td)


# ------------------------------------------------------------------------------------------------------------------- the embedding
def _emb_case(seed):
    rs = RS(seed)
    emb = rs.randint(-4, 5, size=(40, D)).astype(np.float32)
    return rs, emb, rs.randint(-4, 5, size=D).astype(np.float32), rs.randint(-4, 5, size=(20, D)).astype(np.float32), rs.randint(-4, 5, size=(20, D)).astype(np.float32)


@pytest.mark.parametrize("fault,p", [("tape_at_p", 3), ("tape_at_0", 0), ("ids_by_m", 5)])
def test_embedding_faults(fault, p):
    rs, emb, cls, pos, tape = _emb_case(8)
    M, Bhalf, stride = 10, 5, 16
    cond = rs.randint(30, 40, size=M)
    ids = rs.randint(0, 30, size=(M, stride))
    tk = R.embed_tokens(None, cond, ids, stride, Bhalf, p, M)
    want = R.embed_x(emb, cls, pos, tape, tk, p)
    R.check_exact(R.embed_x(emb, cls, pos, tape, tk, p), want, "x")
    if fault == "ids_by_m":
        got = R.embed_x(emb, cls, pos, tape, R.embed_tokens(None, cond, ids, stride, Bhalf, p, M, fault=fault), p)
        assert np.array_equal(got[:Bhalf], want[:Bhalf])               # the conditional half cannot see it
    else:
        got = R.embed_x(emb, cls, pos, tape, tk, p, fault=fault)
    _fails(R.check_exact, got, want, "x")


def test_embedding_three_cases():
    rs, emb, cls, pos, tape = _emb_case(9)
    cond, ids = np.array([31, 32, 39, 39]), rs.randint(0, 30, size=(2, 16))
    assert np.all(R.embed_tokens(None, cond, ids, 16, 2, 0, 4) == -1)
    assert np.array_equal(R.embed_tokens(None, cond, ids, 16, 2, 1, 4), cond)
    assert np.array_equal(R.embed_tokens(None, cond, ids, 16, 2, 7, 4), ids[[0, 1, 0, 1], 5])
    x0 = R.embed_x(emb, cls, pos, tape, np.full(4, -1), 0)
    assert np.array_equal(x0, np.broadcast_to(cls + pos[0], (4, D)))


def test_silu_bound_holds_for_fp32_and_catches_a_wrong_activation():
    c = np.concatenate([np.linspace(-100, 30, 4001), RS(10).standard_normal(4000) * 3]).astype(np.float32)
    r, r32 = R.check_silu(R.silu32(c), c)
    assert r <= 1.0
    _fails(R.check_silu, (c * (1.0 / (1.0 + np.exp(-1.702 * c.astype(np.float64))))).astype(np.float32), c)       # the sigmoid GELU stand-in
    _fails(R.check_silu, R.bf(R.silu32(c)), c)                                                                     # one bf16 rounding


# ------------------------------------------------------------------------------------------------------------------- attention, mode 1
def _att_case(seed, M=7, S=3):
    rs = RS(seed)
    P = (rs.standard_normal((S, M, 3 * D)) * 0.5).astype(np.float32)
    vec = lambda s, o: (o + s * rs.standard_normal(HD)).astype(np.float32)  # noqa: E731
    return rs, P, (rs.standard_normal(3 * D) * 0.1).astype(np.float32), vec(0.1, 1), vec(0.1, 0), vec(0.1, 1), vec(0.1, 0)


@pytest.mark.parametrize("fault", ["knorm_with_qnorm", "k_cached_before_norm", "v_normed", "eps_1e-5"])
def test_prologue_faults(fault):
    rs, P, bias, qw, qb, kw, kb = _att_case(11)
    if fault == "eps_1e-5":
        P = P * np.float32(0.02)                                  # head variances of the order of 1e-4: eps shows
        bias = bias * np.float32(0.02)
    (q64, k64, v64), (q32, k32, v32), (nq, nk, nv) = R.attn_prologue(P, bias, qw, qb, kw, kb, H, HD)
    R.check_appended(k32, k64, nk, k32, "K row")
    R.check_exact(v32, v32, "V row")
    assert np.all(np.abs(q32 - q64) <= R.prologue_tol(nq, HD)) and np.all(np.abs(k32 - k64) <= R.prologue_tol(nk, HD))
    _, (fq, fk, fv), _ = R.attn_prologue(P, bias, qw, qb, kw, kb, H, HD, fault=fault)
    if fault == "v_normed":
        _fails(R.check_exact, fv, v32, "V row")
    else:
        _fails(R.check_appended, fk, k64, nk, k32, "K row")


def test_a_skipped_cache_chunk_and_the_one_hot_selection():
    rs = RS(12)
    M, Tn, E = 3, 19, 8
    q = rs.standard_normal((M, H, HD))
    K, Vv = rs.standard_normal((M, H, Tn, HD)), rs.standard_normal((M, H, Tn, HD))
    scale = 1.0 / np.sqrt(HD)
    zero = np.zeros_like(q)
    ref, tol = R.attn_dense_bound(q, zero, K, zero, Vv, zero, scale, E, 1)
    good = R.attn_fp32(q, K, Vv, scale)
    assert R.check_attn_dense(good, ref, tol) <= 1.0
    assert np.allclose(R.attn_mode1_ref(q, K, Vv, HD), ref, rtol=1e-12, atol=1e-14)
    bad = R.attn_mode1_ref(q, K, Vv, HD, fault="skip_chunk", E=E).astype(np.float32)
    _fails(R.check_attn_dense, bad, ref, tol)
    assert np.abs(bad - ref).max() > 4.0 * np.abs(good - ref).max()
    # one-hot: the winner's V row exactly; a neighbour's row is caught
    _fails(R.check_onehot, Vv[:, :, 4].astype(np.float32), Vv[:, :, 5].astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------- GELU, planes
def test_gelu_is_erf_not_tanh():
    v = np.linspace(-6, 6, 6001).astype(np.float32)
    f = np.float32
    from math import erf
    g32 = (f(0.5) * v * (f(1.0) + np.vectorize(erf)((v * f(0.70710678)).astype(f).astype(np.float64)).astype(f)).astype(f)).astype(f)
    assert R.check_gelu(g32, v) <= 1.0
    _fails(R.check_gelu, R.gelu_tanh64(v).astype(np.float32), v)


def test_the_third_bf16_piece():
    rs = RS(13)
    M, MT, K = 9, 1, 64
    X = np.zeros((32, K), dtype=np.float32)
    X[:M] = R.gelu64(rs.standard_normal((M, K)) * 2).astype(np.float32)
    bits = R.pack_planes(X, MT)
    val = R.check_planes_consistent(bits, MT, K, M)
    assert np.array_equal(val[:M], X[:M])
    R.check_planes(bits, X, MT, K, M)
    dropped = bits.reshape(K // 16, MT, 3, 64, 8).copy()
    dropped[:, :, 2] = 0
    _fails(R.check_planes, dropped.reshape(-1), X, MT, K, M)
    val2 = R.check_planes_consistent(dropped.reshape(-1), MT, K, M)      # h + m alone is a valid two-piece split of ANOTHER value ...
    assert not np.array_equal(val2[:M], X[:M])                            # ... which the value checks behind it reject
    swapped = bits.reshape(K // 16, MT, 3, 64, 8).copy()
    swapped[:, :, [0, 1]] = swapped[:, :, [1, 0]]
    _fails(R.check_planes_consistent, swapped.reshape(-1), MT, K, M)


# ------------------------------------------------------------------------------------------------------------------- the plan, composition
def test_expected_plan_pins_the_paths_of_the_test_engines():
    def p(shape, M, Bhalf=None, sh=0, **kw):
        Dm, Hm, F, Lm = shape
        return R.expected_plan(Dm, Hm, F, Lm, 256, 64, M, Bhalf or M, sh, **kw)
    r2, r3, r4 = (320, 4, 1280, 2), (1280, 16, 5120, 1), (2176, 17, 2176, 1)
    a = p(r2, 128)
    assert (a["bx"], a["rowmajor"], a["S_qkv"], a["PER_qkv"], a["S_proj"], a["PER_proj"], a["S_fc2"], a["PER_fc2"]) == (1, 1, 1, 5, 1, 5, 5, 4)
    assert p(r2, 64)["bx"] == 0 and p(r2, 128, no_bx=True)["bx"] == 0 and p(r2, 128, no_bx=True)["roles"]["attn"] == "k_attn_decode80<1>"
    b = p(r3, 128, 64, 1)
    assert (b["ada_bx"], b["fc1_bx"], b["MTc"], b["roles"]["adaln"], b["roles"]["fc1"]) == (1, 1, 2, "k_bx<4,20,2>", "k_bx<1,10,4,GELU,8,XF>")
    assert p(r3, 64, 32, 1)["ada_bx"] == 0 and p(r3, 66, 33, 1)["ada_bx"] == 1 and p(r3, 64)["ada_bx"] == 1
    c = p(r4, 65)
    assert (c["kpw"], c["nrm"], c["nch"], c["bx"]) == (4, 17, 17, 0) and c["roles"]["resid_mlp"].startswith("k_resid_mod<") and c["roles"]["attn"] == "k_attn_decode<128,1,1>"
    assert p((128, 4, 512, 2), 128, fused=False)["roles"]["resid_attn"] == "k_resid_mod<1,1,1>+k_resid_mod<1,1,2>"


@pytest.mark.parametrize("hidden,heads", [(64, 2), (96, 2), (176, 2)], ids=["hd32", "hd48", "hd88"])
def test_composition_against_the_oracle(hidden, heads):
    """the float64 statements composed into one position against oracle.rar_oracle.rar_position (head_dim 32, and 48 / 88 as in RAR-B /
    RAR-XXL: lanes padded to 16 / 32 in head_sum32).  The oracle is fp32 torch; the yardstick is what fp32 costs it: the same torch
    code evaluated in float64"""
    from oracle.rar_oracle import rar_position
    from wmar_amd.utils.synth import RARConfig, synth_rar_state
    cfg = RARConfig(hidden_size=hidden, num_hidden_layers=2, num_attention_heads=heads, intermediate_size=128, image_seq_len=8, codebook_size=32,
                    condition_num_classes=4)
    sd32 = synth_rar_state(cfg, seed=3, logit_scale=4.0)
    sd64 = {k: v.double() for k, v in sd32.items()}
    sdn = {k: v.numpy() for k, v in sd32.items()}
    M = 5
    rs = RS(14)
    cond = rs.randint(0, 4, size=M) + cfg.codebook_size + 1
    kc32 = vc32 = kc64 = vc64 = kcn = vcn = None
    for p in range(4):
        tk = np.full(M, -1) if p == 0 else (cond if p == 1 else rs.randint(0, cfg.codebook_size, size=M))
        te32 = sd32["cls_token"][0, 0].expand(M, -1) if p == 0 else sd32["embeddings.weight"][torch.from_numpy(tk)]
        ce32 = sd32["embeddings.weight"][torch.from_numpy(cond)]
        with torch.no_grad():
            l32, kc32, vc32 = rar_position(sd32, cfg, te32, ce32, p, kc32, vc32)
            l64, kc64, vc64 = rar_position(sd64, cfg, te32.double(), ce32.double(), p, kc64, vc64)
        ln, kcn, vcn = R.position64(sdn, cfg, tk, cond, p, kcn, vcn)
        cost = float((l32.double() - l64).abs().max())
        assert np.abs(ln - l64.numpy()).max() <= 1e-10, "the float64 statements and the oracle's code in float64 disagree at position %d" % p
        assert np.abs(ln - l32.numpy()).max() <= 2.0 * cost, (p, float(np.abs(ln - l32.numpy()).max()), cost)
        for i in range(cfg.num_hidden_layers):
            assert np.abs(kcn[i] - kc64[i].numpy()).max() <= 1e-11 and np.abs(vcn[i] - vc64[i].numpy()).max() <= 1e-11


# ------------------------------------------------------------------------------------------------------------------- the released sizes
def test_the_wrapper_still_ships_the_pinned_sizes():
    """the (width, depth, F) the pins below stand for are the ones RarARMMWrapper builds; 16 heads each"""
    from wmar_amd.models import rar_wrapper
    assert set(rar_wrapper._RAR_SIZES) == set(R.RELEASED_WRAPPER)
    for size, (name, depth) in R.RELEASED_WRAPPER.items():
        Dm, Hm, F = R.RELEASED_SHAPES[name]
        assert tuple(rar_wrapper._RAR_SIZES[size]) == (Dm, depth, F), size
        assert (Hm, Dm // Hm) == (16, {"RB": 48, "RL": 64, "RXL": 80, "RXXL": 88}[name])


PINS = R.released_pins()


@pytest.mark.parametrize("name,M", sorted(PINS), ids=str)
def test_expected_plan_pins_the_released_sizes(name, M):
    """the plan of every released size at 20 / 64 / 97 / 127 / 128 rows (max_batch 64, one block, vocabulary 256) and of the two
    synthetic k_bx<2,16,4> / <2,20,4> shapes, against the table written down by hand: a dispatch change shows without a GPU"""
    Dm, Hm, F = R.RELEASED_SHAPES[name]
    plan = R.expected_plan(Dm, Hm, F, 1, 256, 64, M, M, 0)
    R.check_pins(plan, PINS[(name, M)], (name, M))
    assert plan["kpw"] == 1 and plan["ada_bx"] == (1 if (name, M) == ("RXL", 64) else 0)
    # shared_u (guidance: 2 x 64 rows) changes the adaLN row tiles only
    if M == 128:
        sh = R.expected_plan(Dm, Hm, F, 1, 256, 64, 128, 64, 1)
        R.check_pins(sh, PINS[(name, M)], (name, M, "shared_u"))
        assert sh["MTc"] == 2


def test_the_pins_are_checked():
    plan = R.expected_plan(768, 16, 3072, 1, 256, 64, 128, 128, 0)
    _fails(R.check_pins, plan, dict(PINS[("RB", 128)], PER_fc2=4))
    _fails(R.check_pins, plan, dict(roles=dict(fc2="k_bx<2,4,4>")))
    _fails(R.check_pins, R.expected_plan(768, 16, 3072, 1, 256, 64, 128, 128, 0, no_bx=True), PINS[("RB", 128)])


# ------------------------------------------------------------------------------------------------------------------- released widths: planted faults
def _int_gemm(seed, N, K, M):
    rs = RS(seed)
    W = rs.randint(-4, 5, size=(N, K)).astype(np.float32)
    X = (rs.randint(-2, 3, size=(32, K)) * 0.25 * (rs.rand(32, K) < 1.0 / 16)).astype(np.float32)
    X[M:] = 3.0e30
    return W, X


def _as_slabs(P64, n_pieces, M):
    got = np.full((n_pieces, 32, P64.shape[2]), R.SENTINEL, dtype=np.float32)
    got[:P64.shape[0], :M] = P64.astype(np.float32)
    return got


def test_a_k_bx_that_stops_behind_step_4_at_per_8():
    """RAR-B's FC2 at 128 rows in small: k_bx at PER 8, S slabs of 64 k-blocks; the integer-operand check sees a wave that leaves
    its steps 5..8 out"""
    N, S, PER, M = 64, 2, 8, 9
    W, X = _int_gemm(20, N, S * 64 * PER, M)
    rng = R.bx_ranges(N // 32, S, PER)
    R.check_gemm_exact(_as_slabs(R.bx_pieces64(W, X[:M], N // 32, S, PER), S + 1, M), W, X, rng, M)
    _fails(R.check_gemm_exact, _as_slabs(R.bx_pieces64(W, X[:M], N // 32, S, PER, fault="drop_steps_5_8"), S + 1, M), W, X, rng, M)
    # a piece past the plan that was written is caught by the same check
    over = _as_slabs(R.bx_pieces64(W, X[:M], N // 32, S, PER), S + 1, M)
    over[S, :M] = 0.0
    _fails(R.check_gemm_exact, over, W, X, rng, M)


def test_slab_6_of_8_missing_in_the_fold():
    rs = RS(21)
    M, S = 9, 8
    x = rs.randint(-64, 65, size=(M, D)).astype(np.float32)
    slabs = [rs.randint(-512, 513, size=(M, D)).astype(np.float32) for _ in range(S)]
    bias = rs.randint(-2, 3, size=D).astype(np.float32)
    gate = (2.0 ** rs.randint(-2, 3, size=(M, D))).astype(np.float32)
    want = R.gated_fold32(x, gate, bias, slabs)
    R.check_exact(R.gated_fold32(x, gate, bias, slabs), want, "gated fold")
    _fails(R.check_exact, R.gated_fold32(x, gate, bias, slabs, fault="missing_slab6"), want, "gated fold")
    # dense: outside the derived distance as well
    ss = [rs.standard_normal((M, D)).astype(np.float32) for _ in range(S)]
    xs, gd = rs.standard_normal((M, D)).astype(np.float32), rs.standard_normal((M, D)).astype(np.float32)
    v, tol = R.gated_fold64(xs, gd, bias, ss)
    assert np.all(np.abs(R.gated_fold32(xs, gd, bias, ss).astype(np.float64) - v) <= tol)
    assert np.any(np.abs(R.gated_fold32(xs, gd, bias, ss, fault="missing_slab6").astype(np.float64) - v) > tol)


def test_the_third_qkv_piece_at_head_dim_48():
    """S = 3 pieces on the four row groups of a head_dim-48 prologue (S < RPI): the third piece dropped moves the plain v row (bit
    check) and the k-normed row (2 x the fp32 algebra, and the derived distance)"""
    hd, Hh = 48, 2
    Dm = hd * Hh
    assert R.attn_row_groups(hd) == 4 and R.attn_row_groups(64) == 4 and R.attn_row_groups(88) == 2 and R.attn_row_groups(32) == 8
    rs = RS(22)
    P = (rs.standard_normal((3, 7, 3 * Dm)) * 0.4).astype(np.float32)
    vec = lambda s, o: (o + s * rs.standard_normal(hd)).astype(np.float32)  # noqa: E731
    bias, qw, qb, kw, kb = (rs.standard_normal(3 * Dm) * 0.1).astype(np.float32), vec(0.1, 1), vec(0.1, 0), vec(0.1, 1), vec(0.1, 0)
    (q64, k64, v64), (q32, k32, v32), (nq, nk, nv) = R.attn_prologue(P, bias, qw, qb, kw, kb, Hh, hd)
    assert np.all(np.abs(k32 - k64) <= R.prologue_tol(nk, hd))
    _, (fq, fk, fv), _ = R.attn_prologue(P, bias, qw, qb, kw, kb, Hh, hd, fault="drop_piece3")
    _fails(R.check_exact, fv, v32, "V row")
    _fails(R.check_appended, fk, k64, nk, k32, "K row")
    assert np.any(np.abs(fk - k64) > R.prologue_tol(nk, hd))


def _loop_case(hd, T, seed=23, M=3, Hh=2):
    """a one-hot and a dense cache of T rows (the new one last) as the GPU sweep lays them out: 3e30 at and past row T - 1"""
    rs = RS(seed + T)
    q = rs.standard_normal((M, Hh, hd)).astype(np.float32)
    knew, vnew = rs.standard_normal((M, Hh, hd)).astype(np.float32), rs.standard_normal((M, Hh, hd)).astype(np.float32)
    Kd = rs.standard_normal((M, Hh, T + 2, hd)).astype(np.float32)
    Vc = rs.standard_normal((M, Hh, T + 2, hd)).astype(np.float32)
    Kd[:, :, T - 1:] = 3.0e30
    Vc[:, :, T - 1:] = 3.0e30
    return q, knew, vnew, Kd, Vc


def _onehot_caught(hd, T, E, fault):
    """does the one-hot sweep (every cached position the winner of some pair) see the fault at this length?"""
    q, knew, vnew, Kd, Vc = _loop_case(hd, T)
    scale = 1.0 / np.sqrt(hd)
    for win in range(T - 1):
        Ko = Kd.copy()
        Ko[:, :, :T - 1] *= 0.01
        Ko[:, :, win] = q * (400.0 / scale) / (q.astype(np.float64) ** 2).sum(-1, keepdims=True)
        y = R.attn_loop64(q, Ko, Vc, knew, vnew, T, hd, E, fault).astype(np.float32)
        if fault is None:
            R.check_onehot(y, Vc[:, :, win])
        elif R.diff_bits(y, Vc[:, :, win]):
            return True
    return False


def _dense_caught(hd, T, E, fault):
    q, knew, vnew, Kd, Vc = _loop_case(hd, T)
    scale = 1.0 / np.sqrt(hd)
    K64 = np.concatenate([Kd[:, :, :T - 1], knew[:, :, None]], 2).astype(np.float64)
    V64 = np.concatenate([Vc[:, :, :T - 1], vnew[:, :, None]], 2).astype(np.float64)
    zero = np.zeros(q.shape)
    ref, tol = R.attn_dense_bound(q.astype(np.float64), zero, K64, zero, V64, zero, scale, E, 1)
    y = R.attn_loop64(q, Kd, Vc, knew, vnew, T, hd, E, fault).astype(np.float32)
    if fault is None:
        assert R.check_attn_dense(y, ref, tol) <= 1.0
        assert np.allclose(y, R.attn_mode1_ref(q.astype(np.float64), K64, V64, hd), rtol=1e-5, atol=1e-6)
        return False
    return bool(np.any(np.abs(y - ref) > tol)) or not np.isfinite(y).all()


@pytest.mark.parametrize("hd,E", [(48, 8), (80, 8), (88, 4)])
def test_the_loop_statement_is_the_plain_softmax(hd, E):
    for T in (1, 2, E, E + 1, 3 * E + 2, 4 * E + 1):
        assert not _dense_caught(hd, T, E, None)
        if T > 1:
            assert not _onehot_caught(hd, T, E, None)


def test_buffer_b_refilled_from_chunk_1_again():
    """the refill `c + 3 NWA` of buffer B: first consumed in chunk 3, whose first slot is a cached row from 3 E + 2 rows on (at
    3 E + 1 it holds the new row, which comes from registers) -- 18 rows at E = 8 never get there"""
    hd, E = 80, 8
    assert R.attn_loop_rows(18, E, hd, "refill_b_chunk1") == R.attn_loop_rows(18, E, hd)           # the parent's longest cache: invisible
    for T in (3 * E + 2, 4 * E + 1, 8 * E):
        assert _onehot_caught(hd, T, E, "refill_b_chunk1") and _dense_caught(hd, T, E, "refill_b_chunk1")
    assert not _onehot_caught(hd, 3 * E + 1, E, "refill_b_chunk1") and not _dense_caught(hd, 3 * E + 1, E, "refill_b_chunk1")


def test_the_last_chunk_skipped_at_an_odd_chunk_count():
    """`if (c + NWA < nchunk)` guards buffer B; a loop that stops a pair early loses the last chunk of an odd count"""
    hd, E = 64, 8
    for T in (2 * E + 1, 2 * E + 2, 3 * E, 4 * E + 1, 4 * E + 3):          # 3, 3, 3, 5 and 5 chunks
        # (the last chunk of k E + 1 rows holds the new row alone: no cached winner lives there, the dense check is the one that sees it)
        assert _onehot_caught(hd, T, E, "skip_last_odd") == (T % E != 1)
        assert _dense_caught(hd, T, E, "skip_last_odd")
    assert not _dense_caught(hd, 4 * E, E, "skip_last_odd") and not _onehot_caught(hd, 4 * E, E, "skip_last_odd")


@pytest.mark.parametrize("hd,E", [(80, 8), (48, 8)])
def test_the_appended_row_taken_from_the_stale_cache_row(hd, E):
    """phases (T - 1) mod E = 2..5 of the appended row: the parent's lengths 1 / E - 1 / E / E + 1 / 2 E + 1 / 18 land on 0, 1, 6, 7
    only.  The sweep fills rows at and past T - 1 with 3e30, so a stale row wins (one-hot) or poisons the output (dense)"""
    assert sorted({(t - 1) % E for t in (1, E - 1, E, E + 1, 2 * E + 1, 18)}) == [0, 1, 6, 7]
    for ph in (2, 3, 4, 5):
        for T in (ph + 1, E + ph + 1, 3 * E + ph + 1):
            assert _dense_caught(hd, T, E, "stale_append")
            if T > 1:
                assert _onehot_caught(hd, T, E, "stale_append")
    for T in (1, E, E + 1, 2 * E + 1, 18):
        assert not _dense_caught(hd, T, E, "stale_append")


def test_the_tail_partial_of_the_wrong_lane_row_at_head_dim_80():
    """k_attn_decode80: the score of row 4 u + g16 takes its last 16 floats from quad u of ITS 16-lane row.  A neighbouring row's quad
    leaves every one-hot winner in place (the main 64 floats lead by far) -- the dense check is the one that sees it"""
    hd, E = 80, 8
    for T in (E + 3, 4 * E + 1, 97):
        assert _dense_caught(hd, T, E, "tail_wrong_row")
    assert not _onehot_caught(hd, E + 3, E, "tail_wrong_row")
    assert R.attn_loop_rows(33, 8, 48, "tail_wrong_row") == R.attn_loop_rows(33, 8, 48)            # other head_dims have no tail
