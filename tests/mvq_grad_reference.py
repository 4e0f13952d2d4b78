"""Differentiable restatement of RAR's MaskGIT-VQGAN tokenizer as its fine-tuning uses it (deps/rar/modeling/modules/maskgit_vqgan.py,
deps/rar/modeling/titok.py:91-123), in plain torch on the CPU and in the dtype of the state it is handed: the float64 reference of
tests/test_gpu_mvq_train.py and the stand-in tokenizer of tests/test_mvq_train_cpu.py.

``oracle.rar_oracle.maskgit_*`` state the same network under ``no_grad``; tests/test_mvq_train_cpu.py pins these walkers' float32
forwards to them bit for bit.  What the network has that the Taming one (tests/vq_grad_reference.py) has not: bias-free block
convolutions and ``encoder.conv_in``, a 1 x 1 shortcut applied to the block OUTPUT, 2 x 2 average-pool downsampling, no attention, no
quant convolutions, and the range change / clamp inside the differentiated path."""
import torch
import torch.nn.functional as F


def _gn_swish(x, w, b):
    return F.silu(F.group_norm(x, 32, w, b, 1e-6))


def _block(sd, p, x):
    """ResnetBlock.forward (maskgit_vqgan.py:69-87): h = conv2(..conv1(..x)); out = h + nin_shortcut(h) when the block changes the
    channel count, else h + x."""
    h = F.conv2d(_gn_swish(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"]), sd[p + "conv1.weight"], None, padding=1)
    h = F.conv2d(_gn_swish(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), sd[p + "conv2.weight"], None, padding=1)
    if p + "nin_shortcut.weight" in sd:
        return h + F.conv2d(h, sd[p + "nin_shortcut.weight"], None)
    return h + x


def encoder_prequant(sd, cfg, x):
    """x [B, 3, R, R] in [-1, 1] -> encoder((x + 1) / 2) [B, z, S, S] (titok.py:98-100, maskgit_vqgan.py:173-185)."""
    h = F.conv2d((x + 1.0) / 2.0, sd["encoder.conv_in.weight"], None, padding=1)
    L = cfg.num_resolutions
    for lvl in range(L):
        for b in range(cfg.num_res_blocks):
            h = _block(sd, f"encoder.down.{lvl}.block.{b}.", h)
        if lvl != L - 1:
            h = F.avg_pool2d(h, kernel_size=2, stride=2)
    for b in range(cfg.num_res_blocks):
        h = _block(sd, f"encoder.mid.{b}.", h)
    h = _gn_swish(h, sd["encoder.norm_out.weight"], sd["encoder.norm_out.bias"])
    return F.conv2d(h, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"])


def decode_preclamp(sd, cfg, z_q):
    """z_q [B, z, S, S] -> decoder(z_q) [B, 3, R, R] in front of the clamp (maskgit_vqgan.py:222-237)."""
    h = F.conv2d(z_q, sd["decoder.conv_in.weight"], sd["decoder.conv_in.bias"], padding=1)
    for b in range(cfg.num_res_blocks):
        h = _block(sd, f"decoder.mid.{b}.", h)
    for lvl in reversed(range(cfg.num_resolutions)):
        for b in range(cfg.num_res_blocks):
            h = _block(sd, f"decoder.up.{lvl}.block.{b}.", h)
        if lvl != 0:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, sd[f"decoder.up.{lvl}.upsample_conv.weight"], sd[f"decoder.up.{lvl}.upsample_conv.bias"], padding=1)
    h = _gn_swish(h, sd["decoder.norm_out.weight"], sd["decoder.norm_out.bias"])
    return F.conv2d(h, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"], padding=1)


def decode(sd, cfg, z_q):
    """decode_like_taming (titok.py:106-109): clamp(decoder(z_q), 0, 1) * 2 - 1, images in [-1, 1]."""
    return torch.clamp(decode_preclamp(sd, cfg, z_q), 0.0, 1.0) * 2.0 - 1.0


def _cast(sd, dtype):
    return {k: v.detach().to("cpu", dtype).requires_grad_(True) for k, v in sd.items() if not k.startswith("quantize.")}


def half_gradients(sd, cfg, half, x, r, dtype):
    """Gradients of (out * r).sum() for half 0 (encoder_prequant) or 1 (decode) by CPU autograd in `dtype`:
    (out, grad of x, {key: grad}) -- the keys are the tensors of that half, a bias only where the network has one."""
    p = _cast(sd, dtype)
    xx = x.detach().to("cpu", dtype).requires_grad_(True)
    out = (encoder_prequant if half == 0 else decode)(p, cfg, xx)
    (out * r.detach().to("cpu", dtype)).sum().backward()
    return out.detach(), xx.grad, {k: v.grad for k, v in p.items() if v.grad is not None}


class TorchTokenizer:
    """The interface ``rcc_loss`` needs (embed, decode, encode_prequant, quantize, named_parameters / parameters), in plain torch."""

    def __init__(self, cfg, state, dtype=None):
        dtype = dtype or torch.float32
        self.cfg = cfg
        self.state = {k: v.detach().clone().to("cpu", dtype) for k, v in state.items()}
        for k, v in self.state.items():
            v.requires_grad_(not k.startswith("quantize."))

    def named_parameters(self, prefix=None):
        return ((k, v) for k, v in self.state.items() if not k.startswith("quantize.") and (prefix is None or k.startswith(prefix)))

    def parameters(self, prefix=None):
        return (v for _, v in self.named_parameters(prefix))

    def embed(self, idx):
        S = self.cfg.codes_size
        z = self.state["quantize.embedding.weight"].detach()[idx.reshape(-1, S * S)]
        return z.view(-1, S, S, self.cfg.z_channels).permute(0, 3, 1, 2).contiguous()

    def decode(self, z_q):
        return decode(self.state, self.cfg, z_q)

    def encode_prequant(self, x):
        return encoder_prequant(self.state, self.cfg, x)

    def quantize(self, z):
        """Nearest code, first minimum of |z|^2 + |e|^2 - 2 z.e (maskgit_vqgan.py:286-321); no gradient."""
        z = z.detach()
        e = self.state["quantize.embedding.weight"].detach()
        rows = z.permute(0, 2, 3, 1).reshape(-1, self.cfg.z_channels)
        d = (rows ** 2).sum(1, keepdim=True) + (e ** 2).sum(1)[None] - 2.0 * rows @ e.t()
        idx = torch.argmin(d, dim=1).view(z.shape[0], -1)
        return self.embed(idx), idx
