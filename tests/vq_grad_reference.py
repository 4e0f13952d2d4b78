"""Float64 references for the BACKWARD of single VQGAN layers, and the accuracy yardsticks tests/test_gpu_vq_grad_layers.py gates on.

Conventions are tests/vq_layer_reference.py's (and the engine's): the four index maps of `_prepare` -- 3 x 3 pad 1, 1 x 1, stride 2
with zero pad (0, 1, 0, 1), nearest x2 upsampling in front; GroupNorm has 32 groups and eps 1e-6; the attention core is
softmax(q k^T C^-1/2) v.  Everything is plain numpy written out from the forward's definition; tests/test_vq_grad_reference.py pins
each function against torch.autograd in float64 on the CPU.

Yardsticks: the weight gradient of a conv is a contraction over K = B Ho Wo products per weight, its input gradient one over (at
most) Cout ks^2 products per element.  `conv2d_wgrad_chain` / `conv2d_dgrad_chain` run each as ONE sequential fp32 multiply-add
chain (fp64 multiply-add rounded to fp32 after every step, as vq_layer_reference.conv2d_chain does); errors are normalised by the
sum of the absolute terms, which the `*_abs` functions return."""
import numpy as np

from tests import vq_layer_reference as R

F64 = np.float64


def _frame(x, ks, stride, up):
    """Shape of the (upsampled, zero-padded) frame the taps index, and the offset of the unpadded image inside it."""
    B, C, H, W = x.shape
    if up:
        H, W = 2 * H, 2 * W
    if ks == 3 and stride == 1:
        return (B, C, H + 2, W + 2), 1
    if stride == 2:
        return (B, C, H + 1, W + 1), 0
    return (B, C, H, W), 0


# ------------------------------------------------------------------------------------------------ convolution (float64, NCHW)
def _dgrad(x_shape, w, g, stride, up, step):
    """Scatter g through the taps into the frame, `acc_view = step(acc_view, g[:, co], w[co, :, dy, dx])` per (tap, co) --
    `step(None, shape, None)` makes the zero frame -- then cut the padding off.  With `up` the result is still 2H x 2W."""
    ks = w.shape[2]
    Ho, Wo = g.shape[2:]
    shape, off = _frame(np.empty(x_shape), ks, stride, up)
    acc = step(None, shape, None)
    for dy in range(ks):
        for dx in range(ks):
            for co in range(w.shape[0]):
                view = (slice(None), slice(None), slice(dy, dy + stride * Ho, stride), slice(dx, dx + stride * Wo, stride))
                acc[view] = step(acc[view], g[:, co, None], w[co, :, dy, dx][None, :, None, None])
    Hc, Wc = x_shape[2] * (2 if up else 1), x_shape[3] * (2 if up else 1)
    return acc[:, :, off:off + Hc, off:off + Wc]


def conv2d_wgrad(x, g, ks, stride=1, up=False):
    """g_w [Cout, Cin, ks, ks] in float64: per tap, the contraction of g with the window of the (upsampled, padded) input."""
    x, g = np.asarray(x, dtype=F64), np.asarray(g, dtype=F64)
    Ho, Wo = g.shape[2:]
    xp = R._prepare(x, ks, stride, up)
    gw = np.zeros((g.shape[1], x.shape[1], ks, ks), dtype=F64)
    for dy in range(ks):
        for dx in range(ks):
            win = xp[:, :, dy:dy + stride * Ho:stride, dx:dx + stride * Wo:stride]
            gw[:, :, dy, dx] = np.einsum("bohw,bchw->oc", g, win, optimize=True)
    return gw


def conv2d_dgrad(x_shape, w, g, stride=1, up=False):
    """g_x [B, Cin, H, W] in float64: per tap, g contracted with that tap's weights over the output channels and scattered into the
    frame; with `up` the 2 x 2 blocks are then summed.  (The same sum `_dgrad` forms one output channel at a time; written per tap
    so that the wide layers take a matrix product, not Cout ks^2 passes.)"""
    w, g = np.asarray(w, dtype=F64), np.asarray(g, dtype=F64)
    ks = w.shape[2]
    Ho, Wo = g.shape[2:]
    shape, off = _frame(np.empty(x_shape), ks, stride, up)
    acc = np.zeros(shape, dtype=F64)
    for dy in range(ks):
        for dx in range(ks):
            acc[:, :, dy:dy + stride * Ho:stride, dx:dx + stride * Wo:stride] += np.einsum("bohw,oc->bchw", g, w[:, :, dy, dx], optimize=True)
    Hc, Wc = x_shape[2] * (2 if up else 1), x_shape[3] * (2 if up else 1)
    gx = acc[:, :, off:off + Hc, off:off + Wc]
    if up:
        gx = gx[:, :, 0::2, 0::2] + gx[:, :, 0::2, 1::2] + gx[:, :, 1::2, 0::2] + gx[:, :, 1::2, 1::2]
    return gx


def conv2d_backward(x, w, g, stride=1, up=False):
    """x [B, Cin, H, W], w [Cout, Cin, ks, ks], g [B, Cout, Ho, Wo] = dL/dy -> (g_x, g_w, g_b) in float64."""
    g = np.asarray(g, dtype=F64)
    return conv2d_dgrad(np.shape(x), w, g, stride, up), conv2d_wgrad(x, g, np.shape(w)[2], stride, up), g.sum((0, 2, 3))


def conv2d_backward_abs(x, w, g, stride=1, up=False):
    """sum of the absolute terms of every g_x, g_w, g_b element: the denominators of the normalised errors."""
    return conv2d_backward(np.abs(x), np.abs(w), np.abs(g), stride, up)


def conv2d_wgrad_chain(x, g, ks, stride=1, up=False, skip_tap=None, skip_image=None, k_stop=None):
    """g_w as one sequential fp32 chain per weight over the K = B Ho Wo products in (b, oy, ox) order; also g_b the same way.
    skip_tap / skip_image / k_stop: a kernel that forgets that tap's weights / that image / every product k >= k_stop, k the
    position in (b, oy, ox) order -- the last K slice of run_conv_wgrad (what the dense gate must catch)."""
    x, g = np.asarray(x, dtype=np.float32), np.asarray(g, dtype=np.float32)
    B, Cout, Ho, Wo = g.shape
    xp = R._prepare(x, ks, stride, up)
    gw = np.zeros((Cout, x.shape[1], ks, ks), dtype=np.float32)
    gb = np.zeros(Cout, dtype=np.float32)
    g64 = g.astype(F64)
    for b in range(B):
        if b == skip_image:
            continue
        for oy in range(Ho):
            for ox in range(Wo):
                if k_stop is not None and (b * Ho + oy) * Wo + ox >= k_stop:
                    continue
                patch = xp[b, :, oy * stride:oy * stride + ks, ox * stride:ox * stride + ks]
                gw = (gw.astype(F64) + g64[b, :, oy, ox][:, None, None, None] * patch[None]).astype(np.float32)
                gb = (gb.astype(F64) + g64[b, :, oy, ox]).astype(np.float32)
    if skip_tap is not None:
        gw[:, :, skip_tap // ks, skip_tap % ks] = 0
    return gw, gb


def conv2d_dgrad_chain(x_shape, w, g, stride=1, up=False):
    """g_x as one sequential fp32 chain per input element (taps outside, output channels inside); with `up` the four elements of
    a 2 x 2 block are then added one after the other in fp32."""
    w32, g32 = np.asarray(w, dtype=np.float32).astype(F64), np.asarray(g, dtype=np.float32).astype(F64)

    def step(acc, a, b):
        return np.zeros(a, dtype=np.float32) if acc is None else (acc.astype(F64) + a * b).astype(np.float32)

    gx = _dgrad(tuple(x_shape), w32, g32, stride, up, step)
    if up:
        s = gx[:, :, 0::2, 0::2]
        for part in (gx[:, :, 0::2, 1::2], gx[:, :, 1::2, 0::2], gx[:, :, 1::2, 1::2]):
            s = (s.astype(F64) + part.astype(F64)).astype(np.float32)
        gx = s
    return np.ascontiguousarray(gx)


# ------------------------------------------------------------------------------------------------ GroupNorm (+ swish)
def group_norm_backward(x, gamma, beta, swish, g):
    """x, g [B, C, H, W] (g = dL/d swish(GN(x)) or dL/d GN(x)) -> (g_x, dgamma, dbeta, dgamma_abs, dbeta_abs) in float64; the
    last two are the sums of the absolute terms."""
    x, g = np.asarray(x, dtype=F64), np.asarray(g, dtype=F64)
    gamma, beta = np.asarray(gamma, dtype=F64)[None, :, None, None], np.asarray(beta, dtype=F64)[None, :, None, None]
    B, C = x.shape[:2]
    cpg = C // 32
    mean, rstd = R.group_stats(x)
    m = np.repeat(mean, cpg, axis=1)[:, :, None, None]
    r = np.repeat(rstd, cpg, axis=1)[:, :, None, None]
    xh = (x - m) * r
    dy = g
    if swish:
        y = xh * gamma + beta
        sg = 1.0 / (1.0 + np.exp(-y))
        dy = g * sg * (1.0 + y * (1.0 - sg))
    dxh = (dy * gamma).reshape(B, 32, -1)
    xg = xh.reshape(B, 32, -1)
    gx = (dxh - dxh.mean(-1, keepdims=True) - xg * (dxh * xg).mean(-1, keepdims=True)).reshape(x.shape) * r
    return gx, (dy * xh).sum((0, 2, 3)), dy.sum((0, 2, 3)), np.abs(dy * xh).sum((0, 2, 3)), np.abs(dy).sum((0, 2, 3))


# ------------------------------------------------------------------------------------------------ attention core
def attention_backward(q, k, v, go):
    """q, k, v, go [B, N, C] -> (g_q, g_k, g_v) of o = softmax(q k^T C^-1/2) v in float64."""
    q, k, v, go = (np.asarray(t, dtype=F64) for t in (q, k, v, go))
    scale = q.shape[-1] ** -0.5
    s = np.einsum("bic,bjc->bij", q, k) * scale
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    gv = np.einsum("bij,bic->bjc", p, go)
    dp = np.einsum("bic,bjc->bij", go, v)
    ds = scale * p * (dp - (dp * p).sum(-1, keepdims=True))
    return np.einsum("bij,bjc->bic", ds, k), np.einsum("bij,bic->bjc", ds, q), gv


def normalised_error(got, exact, denom):
    return R.normalised_error(got, exact, denom)


# ------------------------------------------------------------------------------------------------ whole halves, torch autograd
def _cast(sd, dtype):
    return {k: v.detach().to("cpu", dtype).requires_grad_(True) for k, v in sd.items() if not k.startswith("quantize.")}


def encoder_prequant(sd, cfg, x):
    """quant_conv(encoder(x)) [B, E, S, S] (vqgan.py:64-66) in torch with autograd on, in the dtype of `sd` and `x`: the oracle's
    encoder_forward restated without its no_grad (oracle.model_oracle; `sd` keys relative to first_stage_model.)."""
    import torch.nn.functional as F
    from oracle.model_oracle import _attn, _gn_swish, _resnet
    e = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    L = cfg.num_resolutions
    h = F.conv2d(x, e["conv_in.weight"], e["conv_in.bias"], padding=1)
    for lvl in range(L):
        for b in range(cfg.num_res_blocks):
            h = _resnet(e, f"down.{lvl}.block.{b}.", h)
            if f"down.{lvl}.attn.{b}.norm.weight" in e:
                h = _attn(e, f"down.{lvl}.attn.{b}.", h)
        if lvl != L - 1:
            h = F.conv2d(F.pad(h, (0, 1, 0, 1)), e[f"down.{lvl}.downsample.conv.weight"], e[f"down.{lvl}.downsample.conv.bias"], stride=2)
    h = _resnet(e, "mid.block_1.", h)
    h = _attn(e, "mid.attn_1.", h)
    h = _resnet(e, "mid.block_2.", h)
    h = _gn_swish(h, e["norm_out.weight"], e["norm_out.bias"])
    h = F.conv2d(h, e["conv_out.weight"], e["conv_out.bias"], padding=1)
    return F.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])


def decode(sd, cfg, z_q):
    """decoder(post_quant_conv(z_q)) [B, 3, R, R], not clamped (vqgan.py:70-73), the same way."""
    import torch.nn.functional as F
    from oracle.model_oracle import _attn, _gn_swish, _resnet
    d = {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}
    h = F.conv2d(z_q, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"])
    h = F.conv2d(h, d["conv_in.weight"], d["conv_in.bias"], padding=1)
    h = _resnet(d, "mid.block_1.", h)
    h = _attn(d, "mid.attn_1.", h)
    h = _resnet(d, "mid.block_2.", h)
    for lvl in reversed(range(cfg.num_resolutions)):
        for b in range(cfg.num_res_blocks + 1):
            h = _resnet(d, f"up.{lvl}.block.{b}.", h)
            if f"up.{lvl}.attn.{b}.norm.weight" in d:
                h = _attn(d, f"up.{lvl}.attn.{b}.", h)
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, d[f"up.{lvl}.upsample.conv.weight"], d[f"up.{lvl}.upsample.conv.bias"], padding=1)
    h = _gn_swish(h, d["norm_out.weight"], d["norm_out.bias"])
    return F.conv2d(h, d["conv_out.weight"], d["conv_out.bias"], padding=1)


def half_gradients(sd, cfg, half, x, r, dtype):
    """Gradients of (out * r).sum() for half 0 (encoder_prequant) or 1 (decode) by CPU autograd in `dtype`:
    (out, grad of x, {key: grad})."""
    import torch
    p = _cast(sd, dtype)
    xx = x.detach().to("cpu", dtype).requires_grad_(True)
    out = (encoder_prequant if half == 0 else decode)(p, cfg, xx)
    (out * r.detach().to("cpu", dtype)).sum().backward()
    return out.detach(), xx.grad, {k: v.grad for k, v in p.items() if v.grad is not None}


class TorchTokenizer:
    """The interface ``rcc_loss`` needs, in plain torch on the CPU."""

    def __init__(self, cfg, state, dtype=None):
        import torch
        dtype = dtype or torch.float32
        self.cfg = cfg
        self.state = {k: v.detach().clone().to(dtype) for k, v in state.items()}
        for k, v in self.state.items():
            v.requires_grad_(not k.startswith("quantize."))

    def named_parameters(self, prefix=None):
        return ((k, v) for k, v in self.state.items() if not k.startswith("quantize.") and (prefix is None or k.startswith(prefix)))

    def parameters(self, prefix=None):
        return (v for _, v in self.named_parameters(prefix))

    def embed(self, idx):
        S = self.cfg.codes_size
        return self.state["quantize.embedding.weight"].detach()[idx.reshape(-1, S * S)].view(-1, S, S, self.cfg.embed_dim).permute(0, 3, 1, 2).contiguous()

    def decode(self, z_q):
        return decode(self.state, self.cfg, z_q)

    def encode_prequant(self, x):
        return encoder_prequant(self.state, self.cfg, x)

    def quantize(self, z):
        z = z.detach()
        from oracle.model_oracle import quantize_argmin
        idx = quantize_argmin(self.state["quantize.embedding.weight"].detach(), z.permute(0, 2, 3, 1).reshape(-1, self.cfg.embed_dim))
        idx = idx.view(z.shape[0], -1)
        return self.embed(idx), idx
