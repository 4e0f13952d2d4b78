"""CPU: the float64 backward references of tests/vq_grad_reference.py against torch.autograd in float64, and a check that the
yardstick of the weight gradient means something (a wgrad that drops one tap or one image of the batch fails the dense gate)."""
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
