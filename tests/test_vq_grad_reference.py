"""CPU: the float64 backward references of tests/vq_grad_reference.py against torch.autograd in float64, and a check that the
yardstick of the weight gradient means something (a wgrad that drops one tap, one image of the batch or the last K slice, or that
walks the image with H and W swapped, fails the dense gate).  The conv references are checked square and non-square."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vq_grad_reference as G
from tests import vq_layer_reference as R

DENSE_GATE = 2.0      # tests/vq_layer_checks.py

MAPS = [(3, 1, False), (1, 1, False), (3, 2, False), (3, 1, True)]


def _torch_conv(x, w, b, ks, stride, up):
    if up:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if stride == 2:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    return F.conv2d(x, w, b, padding=1 if ks == 3 else 0)


@pytest.mark.parametrize("ks,stride,up", MAPS)
def test_conv_backward_matches_autograd(ks, stride, up):
    rng = np.random.default_rng(ks * 10 + stride + int(up))
    B, cin, cout, H = 2, 5, 7, 6
    x, w = rng.standard_normal((B, cin, H, H)), rng.standard_normal((cout, cin, ks, ks))
    Ho = H * (2 if up else 1) // stride
    g = rng.standard_normal((B, cout, Ho, Ho))
    tx, tw, tb = (torch.tensor(t, requires_grad=True) for t in (x, w, np.zeros(cout)))
    y = _torch_conv(tx, tw, tb, ks, stride, up)
    assert np.allclose(y.detach().numpy(), R.conv2d(x, w, stride=stride, up=up), rtol=0, atol=1e-12)
    y.backward(torch.tensor(g))
    gx, gw, gb = G.conv2d_backward(x, w, g, stride, up)
    for got, want in ((gx, tx.grad), (gw, tw.grad), (gb, tb.grad)):
        assert got.shape == tuple(want.shape)
        assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("hw", [(4, 10), (10, 4)], ids=["4x10", "10x4"])
@pytest.mark.parametrize("ks,stride,up", MAPS)
def test_conv_backward_and_chains_at_non_square_shapes(ks, stride, up, hw):
    """The GPU probes run non-square layers: the float64 reference against autograd, and both fp32 chains against the reference, with
    H != W (a reference that mixed the two up would still pass every square check)."""
    H, W = hw
    rng = np.random.default_rng(ks * 10 + stride + int(up) + H)
    B, cin, cout = 2, 5, 7
    m = 2 if up else 1
    Ho, Wo = H * m // stride, W * m // stride
    x = rng.standard_normal((B, cin, H, W)).astype(np.float32)
    w = rng.standard_normal((cout, cin, ks, ks)).astype(np.float32)
    g = rng.standard_normal((B, cout, Ho, Wo)).astype(np.float32)
    tx, tw, tb = (torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (x, w, np.zeros(cout)))
    y = _torch_conv(tx, tw, tb, ks, stride, up)
    assert tuple(y.shape) == (B, cout, Ho, Wo)
    assert np.allclose(y.detach().numpy(), R.conv2d(x, w, stride=stride, up=up), rtol=0, atol=1e-12)
    y.backward(torch.tensor(g, dtype=torch.float64))
    gx, gw, gb = G.conv2d_backward(x, w, g, stride, up)
    for got, want in ((gx, tx.grad), (gw, tw.grad), (gb, tb.grad)):
        assert got.shape == tuple(want.shape)
        assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))
    ax, aw, ab = G.conv2d_backward_abs(x, w, g, stride, up)
    cw, cb = G.conv2d_wgrad_chain(x, g, ks, stride, up)
    cx = G.conv2d_dgrad_chain(x.shape, w, g, stride, up)
    K = B * Ho * Wo
    assert cx.shape == x.shape
    assert 0 < G.normalised_error(cw, gw, aw) <= K * R.U24
    assert G.normalised_error(cb, gb, ab) <= K * R.U24
    assert 0 < G.normalised_error(cx, gx, ax) <= (cout * ks * ks + 3) * R.U24


@pytest.mark.parametrize("ks,stride,up", MAPS)
def test_chains_are_fp32_accurate_versions_of_the_references(ks, stride, up):
    rng = np.random.default_rng(100 + ks + stride + int(up))
    B, cin, cout, H = 2, 4, 6, 4
    x = rng.standard_normal((B, cin, H, H)).astype(np.float32)
    w = rng.standard_normal((cout, cin, ks, ks)).astype(np.float32)
    Ho = H * (2 if up else 1) // stride
    g = rng.standard_normal((B, cout, Ho, Ho)).astype(np.float32)
    gx, gw, gb = G.conv2d_backward(x, w, g, stride, up)
    ax, aw, ab = G.conv2d_backward_abs(x, w, g, stride, up)
    cw, cb = G.conv2d_wgrad_chain(x, g, ks, stride, up)
    cx = G.conv2d_dgrad_chain(x.shape, w, g, stride, up)
    K = B * Ho * Ho
    assert cw.dtype == np.float32 and cx.dtype == np.float32 and cx.shape == x.shape
    assert 0 < G.normalised_error(cw, gw, aw) <= K * R.U24
    assert G.normalised_error(cb, gb, ab) <= K * R.U24
    assert 0 < G.normalised_error(cx, gx, ax) <= (cout * ks * ks + 3) * R.U24


@pytest.mark.parametrize("swish", [0, 1])
@pytest.mark.parametrize("C", [32, 64, 128])
def test_group_norm_backward_matches_autograd(C, swish):
    rng = np.random.default_rng(C + swish)
    x, g = rng.standard_normal((2, C, 4, 4)) * 2 + 0.5, rng.standard_normal((2, C, 4, 4))
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.uniform(-0.5, 0.5, C)
    tx, tg, tb = (torch.tensor(t, requires_grad=True) for t in (x, gamma, beta))
    y = F.group_norm(tx, 32, tg, tb, eps=1e-6)
    (F.silu(y) if swish else y).backward(torch.tensor(g))
    gx, dg, db, ag, ab = G.group_norm_backward(x, gamma, beta, swish, g)
    assert np.abs(gx - tx.grad.numpy()).max() <= 1e-11
    assert np.abs(dg - tg.grad.numpy()).max() <= 1e-11 and np.abs(db - tb.grad.numpy()).max() <= 1e-11
    assert np.all(ag >= np.abs(dg) - 1e-12) and np.all(ab >= np.abs(db) - 1e-12)


def test_attention_backward_matches_autograd():
    rng = np.random.default_rng(3)
    q, k, v, go = (rng.standard_normal((2, 16, 8)) for _ in range(4))
    tq, tk, tv = (torch.tensor(t, requires_grad=True) for t in (q, k, v))
    o = torch.softmax(tq @ tk.transpose(1, 2) * 8 ** -0.5, dim=-1) @ tv
    assert np.allclose(o.detach().numpy(), R.attention(q, k, v), rtol=0, atol=1e-12)
    o.backward(torch.tensor(go))
    for got, want in zip(G.attention_backward(q, k, v, go), (tq.grad, tk.grad, tv.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12


@pytest.mark.parametrize("broken", [dict(skip_tap=4), dict(skip_tap=8), dict(skip_image=1)])
def test_a_wgrad_that_drops_a_tap_or_an_image_fails_the_dense_gate(broken):
    rng = np.random.default_rng(7)
    B, cin, cout, H = 3, 8, 8, 8
    x = R.realistic_activations(rng, (B, cin, H, H))
    g = (rng.standard_normal((B, cout, H, H)) * 0.05).astype(np.float32)
    _, gw, _ = G.conv2d_backward(x, np.zeros((cout, cin, 3, 3)), g)
    _, aw, _ = G.conv2d_backward_abs(x, np.zeros((cout, cin, 3, 3)), g)
    good, _ = G.conv2d_wgrad_chain(x, g, 3)
    bad, _ = G.conv2d_wgrad_chain(x, g, 3, **broken)
    e_chain, e_bad = G.normalised_error(good, gw, aw), G.normalised_error(bad, gw, aw)
    assert e_chain > 0
    assert e_bad > 1e3 * DENSE_GATE * e_chain, (e_bad, e_chain)


def _slices(K, cout, cin):
    """run_conv_wgrad's K split (wmar_amd/csrc/vq_grad.h): (slices, products per slice)."""
    tiles = -(-cout // 32) * -(-cin // 32)
    S = max(1, min(-(-K // 256), -(-1024 // tiles), 64))
    return S, (-(-K // S) + 1) & ~1


@pytest.mark.parametrize("cin,cout,ks,H,W,S_want", [(32, 32, 3, 128, 136, 64), (512, 512, 1, 32, 40, 4)], ids=["S64", "S4"])
def test_a_wgrad_that_drops_the_last_k_slice_fails_the_dense_gate(cin, cout, ks, H, W, S_want):
    """The two capped shapes of tests/test_gpu_vq_grad_layers.py with the products of the last K slice (k >= (S - 1) Kc) left out.  The
    slice holds 1 / S of every weight's terms, the last rows of the image, so every weight loses mass (about sqrt(Kc) / K of its
    sum|terms|, 1e-3 to 1e-2), and the rows hold some of the 2^20 activations: a weight whose sum one of them dominates loses
    nearly all of it.  Measured: normalised error 0.92 at S = 64 (4.9e4 x the gate), 1.0 at S = 4 (1.3e5 x the gate)."""
    rng = np.random.default_rng(11 + S_want)
    K = H * W
    S, Kc = _slices(K, cout, cin)
    assert S == S_want and (S - 1) * Kc < K <= S * Kc
    x = R.realistic_activations(rng, (1, cin, H, W))
    g = (rng.standard_normal((1, cout, H, W)) * 0.05).astype(np.float32)
    gw, aw = G.conv2d_wgrad(x, g, ks), G.conv2d_wgrad(np.abs(x), np.abs(g), ks)
    good, _ = G.conv2d_wgrad_chain(x, g, ks)
    bad, _ = G.conv2d_wgrad_chain(x, g, ks, k_stop=(S - 1) * Kc)
    e_chain, e_bad = G.normalised_error(good, gw, aw), G.normalised_error(bad, gw, aw)
    print("VQGRAD control last_slice S=%d Kc=%d chain=%.3g dropped=%.3g over_gate=%.3g" % (S, Kc, e_chain, e_bad, e_bad / (DENSE_GATE * e_chain)))
    assert e_chain > 0
    assert e_bad > 1e3 * DENSE_GATE * e_chain, (e_bad, e_chain)


def test_a_wgrad_on_the_transposed_image_fails_the_dense_gate():
    """A kernel that swaps Ho and Wo walks the same memory as a W x H image: at 8 x 24 every tap but the centre then pairs a gradient
    with the wrong neighbour.  Measured: normalised error 49 (the wrong products are not bounded by the right ones' sum), 2.2e7 x the gate."""
    rng = np.random.default_rng(13)
    B, cin, cout, H, W = 3, 16, 16, 8, 24
    x = R.realistic_activations(rng, (B, cin, H, W))
    g = (rng.standard_normal((B, cout, H, W)) * 0.05).astype(np.float32)
    gw, aw = G.conv2d_wgrad(x, g, 3), G.conv2d_wgrad(np.abs(x), np.abs(g), 3)
    good, _ = G.conv2d_wgrad_chain(x, g, 3)
    bad, _ = G.conv2d_wgrad_chain(x.reshape(B, cin, W, H), g.reshape(B, cout, W, H), 3)
    e_chain, e_bad = G.normalised_error(good, gw, aw), G.normalised_error(bad, gw, aw)
    print("VQGRAD control transposed chain=%.3g swapped=%.3g over_gate=%.3g" % (e_chain, e_bad, e_bad / (DENSE_GATE * e_chain)))
    assert np.array_equal(good[:, :, 1, 1], bad[:, :, 1, 1]), "the centre tap pairs the same pixels either way"
    assert e_chain > 0
    assert e_bad > 1e3 * DENSE_GATE * e_chain, (e_bad, e_chain)


def test_walkers_float32_forward_equals_the_oracle_on_the_harness_config():
    from oracle import model_oracle as M
    from wmar_amd.utils import synth
    cfg = synth.VQConfig(**dict(synth.HARNESS_VQ, n_embed=512))
    sd = synth.synth_vq_state(cfg, 3, "cpu")
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, cfg.resolution, cfg.resolution, generator=g) * 2 - 1
    codes = torch.randint(0, cfg.n_embed, (2, cfg.codes_size ** 2), generator=g)
    with torch.no_grad():
        pre = G.encoder_prequant(sd, cfg, x)
        S = cfg.codes_size
        zq = sd["quantize.embedding.weight"][codes.reshape(-1)].view(2, S, S, cfg.embed_dim).permute(0, 3, 1, 2).contiguous()
        img = G.decode(sd, cfg, zq)
    assert torch.equal(pre.permute(0, 2, 3, 1).reshape(-1, cfg.embed_dim), M.encode_prequant(sd, cfg, x))
    assert torch.equal(img.clamp(-1, 1), M.codes_to_images(sd, cfg, codes))
    out, gx, grads = G.half_gradients(sd, cfg, 0, x, torch.ones_like(pre), torch.float64)
    assert gx.shape == x.shape and set(grads) == {k for k in sd if k.startswith(("encoder.", "quant_conv."))}
