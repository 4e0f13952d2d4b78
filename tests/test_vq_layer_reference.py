"""CPU: the float64 layer references and yardsticks of tests/vq_layer_reference.py, pinned against torch.nn.functional in float64
and against the textbook bound of an fp32 chain -- and the proof that the gates of tests/test_gpu_vq_layers.py have teeth: a CPU
model of k_conv_bx's six-product accumulation passes them, the same model with any one second-order piece product removed fails
both the impulse gate and (up to K = 288) the dense gate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vq_layer_reference as R

IMPULSE_GATE = 2.0 ** -21          # the gates of tests/test_gpu_vq_layers.py
DENSE_GATE = 2.0


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("cin,cout,ks,stride,up,hw", [(3, 5, 3, 1, False, 8), (8, 6, 1, 1, False, 8), (5, 4, 3, 2, False, 8),
                                                       (4, 7, 3, 1, True, 4), (40, 9, 3, 1, False, 6)])
def test_conv_reference_matches_torch_float64(cin, cout, ks, stride, up, hw):
    rng = np.random.default_rng(cin * 100 + cout)
    x = rng.standard_normal((2, cin, hw, hw + 2))
    w = rng.standard_normal((cout, cin, ks, ks))
    b = rng.standard_normal(cout)
    Ho, Wo = R._out_size(x, ks, stride, up)
    res = rng.standard_normal((2, cout, Ho, Wo))
    xt = _t(x)
    if up:
        xt = F.interpolate(xt, scale_factor=2.0, mode="nearest")           # Upsample.forward
    if stride == 2:
        ref = F.conv2d(F.pad(xt, (0, 1, 0, 1)), _t(w), _t(b), stride=2, padding=0)      # Downsample.forward
    else:
        ref = F.conv2d(xt, _t(w), _t(b), stride=1, padding=1 if ks == 3 else 0)
    ref = ref + _t(res)
    got = R.conv2d(x, w, b, res, stride, up)
    assert got.shape == tuple(ref.shape)
    assert np.abs(got - ref.numpy()).max() <= 1e-12 * np.abs(ref.numpy()).max()
    den = R.conv2d_abs(x, w, b, res, stride, up)
    assert np.all(den >= np.abs(got) * (1 - 1e-12))


@pytest.mark.parametrize("C,swish", [(32, 0), (64, 1), (96, 1), (256, 0)])
def test_group_norm_reference_matches_torch_float64(C, swish):
    rng = np.random.default_rng(C)
    x = rng.standard_normal((2, C, 5, 7)) * 3 + 1.5
    g, b = rng.standard_normal(C), rng.standard_normal(C)
    ref = F.group_norm(_t(x), 32, _t(g), _t(b), eps=1e-6)
    if swish:
        ref = F.silu(ref)
    assert np.abs(R.group_norm(x, g, b, swish) - ref.numpy()).max() <= 1e-12
    mean, rstd = R.group_stats(x)
    grp = _t(x).reshape(2, 32, -1)
    assert np.allclose(mean, grp.mean(-1).numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(rstd, (grp.var(-1, unbiased=False) + 1e-6).rsqrt().numpy(), rtol=1e-13)


def test_attention_and_distance_references_match_torch_float64():
    rng = np.random.default_rng(1)
    q, k, v = (rng.standard_normal((2, 24, 16)) for _ in range(3))
    ref = torch.softmax(_t(q) @ _t(k).transpose(1, 2) * 16 ** -0.5, dim=-1) @ _t(v)
    assert np.abs(R.attention(q, k, v) - ref.numpy()).max() <= 1e-13
    z, e = rng.standard_normal((70, 8)), rng.standard_normal((96, 8))
    ref = torch.cdist(_t(z), _t(e), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    assert np.abs(R.sq_distances(z, e) - ref.numpy()).max() <= 1e-12


@pytest.mark.parametrize("cin,cout,ks,stride,up,hw", [(3, 4, 3, 1, False, 8), (32, 3, 3, 1, False, 8), (16, 8, 1, 1, False, 8),
                                                       (8, 4, 3, 2, False, 8), (8, 4, 3, 1, True, 4)])
def test_chain_yardstick_is_a_conv_and_stays_inside_its_textbook_bound(cin, cout, ks, stride, up, hw):
    """The chain computes the same convolution (to fp32 accuracy), and its normalised error stays below K 2^-24 (K roundings of at
    most half an ulp of a partial sum that never exceeds sum|w x|); bias and residual add one rounding each."""
    rng = np.random.default_rng(7 * cin + ks)
    x = R.realistic_activations(rng, (2, cin, hw, hw))
    w = (rng.standard_normal((cout, cin, ks, ks)) * 0.05).astype(np.float32)
    K = cin * ks * ks
    exact, den = R.conv2d(x, w, stride=stride, up=up), R.conv2d_abs(x, w, stride=stride, up=up)
    chain = R.conv2d_chain(x, w, stride=stride, up=up)
    assert chain.dtype == np.float32 and chain.shape == exact.shape
    e = R.normalised_error(chain, exact, den)
    assert 0 < e <= K * R.U24, (e, K * R.U24)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    res = R.realistic_activations(rng, exact.shape)
    e2 = R.normalised_error(R.conv2d_chain(x, w, b, res, stride, up), R.conv2d(x, w, b, res, stride, up), R.conv2d_abs(x, w, b, res, stride, up))
    assert 0 < e2 <= (K + 2) * R.U24
    # the chain helper over plain dot products is the same arithmetic
    if ks == 1 and not up:
        rows = x.transpose(0, 2, 3, 1).reshape(-1, cin)
        assert np.array_equal(R.chain_dot(rows, np.broadcast_to(w[0, :, 0, 0], rows.shape)), chain[:, 0].reshape(-1))


def test_operand_generators_do_what_the_gates_assume():
    rng = np.random.default_rng(2)
    v = R.full_significand(rng, 4096)
    assert np.all(v.view(np.uint32) & 1 == 1) and (v > 0).any() and (v < 0).any()
    assert np.abs(v).min() < 2.0 ** -18 and np.abs(v).max() > 2.0 ** 18 and np.abs(v).max() < 2.0 ** 21
    h, m, l = R.split3(v)
    assert np.all(m != 0) and np.array_equal(h.astype(np.float64) + m + l, v.astype(np.float64))
    b = R.bf16_exact(rng, 4096)
    assert np.array_equal(R.bf16_rne(b), b)
    a = R.realistic_activations(rng, (2, 32, 8, 8))
    assert (np.abs(a) == 2.0 ** 20).any() and (np.abs(a) == 2.0 ** -20).any()


def test_impulse_gate_passes_the_six_product_model_and_fails_every_five_product_model():
    """One product per output, full 24-bit significands: six exact piece products added into an fp32 accumulator one after the
    other.  All six: within 2 x 2^-24 of w x (six roundings of shrinking terms).  One second-order product missing: most outputs
    miss the 2^-21 gate."""
    rng = np.random.default_rng(11)
    n = 100000
    x, w = R.full_significand(rng, n).reshape(n, 1), R.full_significand(rng, n).reshape(n, 1)
    exact = x[:, 0].astype(np.float64) * w[:, 0].astype(np.float64)
    rel = np.abs(R.bx_model_dot(x, w) - exact) / np.abs(exact)
    assert rel.max() <= 2 * R.U24 < IMPULSE_GATE, rel.max() / R.U24
    for drop in ("mm", "hl", "lh"):
        rel = np.abs(R.bx_model_dot(x, w, drop=drop) - exact) / np.abs(exact)
        assert (rel > IMPULSE_GATE).mean() > 0.5, (drop, (rel > IMPULSE_GATE).mean())
        assert rel.max() > 64 * R.U24
    # bf16-exact operands: the product is a single exact piece product
    xb, wb = R.bf16_exact(rng, n).reshape(n, 1), R.bf16_exact(rng, n).reshape(n, 1)
    assert np.array_equal(R.bx_model_dot(xb, wb).astype(np.float64), xb[:, 0].astype(np.float64) * wb[:, 0])


@pytest.mark.parametrize("K", [32, 64, 288])
def test_dense_gate_passes_the_six_product_model_and_fails_every_five_product_model(K):
    """Dense dot products on swish-like activations and std-0.05 weights: the six-product model stays below the sequential chain's
    normalised error, every five-product model exceeds twice the chain's (the dense gate) at the contraction lengths of the small
    test shapes."""
    rng = np.random.default_rng(K)
    n = 20000
    a = rng.standard_normal((n, K))
    x = (a / (1 + np.exp(-a))).astype(np.float32)
    w = (rng.standard_normal((n, K)) * 0.05).astype(np.float32)
    p = x.astype(np.float64) * w.astype(np.float64)
    exact, den = p.sum(-1), np.abs(p).sum(-1)
    e_chain = (np.abs(R.chain_dot(x, w) - exact) / den).max()
    assert e_chain <= K * R.U24
    e_six = (np.abs(R.bx_model_dot(x, w) - exact) / den).max()
    assert e_six <= e_chain, (e_six, e_chain)
    for drop in ("mm", "hl", "lh"):
        e = (np.abs(R.bx_model_dot(x, w, drop=drop) - exact) / den).max()
        assert e > DENSE_GATE * e_chain, (drop, e / e_chain)
