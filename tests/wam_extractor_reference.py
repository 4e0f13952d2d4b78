"""The WAM extractor (``Wam.detect`` without the resize: ``pixel_decoder(image_encoder(x))``) restated in plain torch from its
description: patch embedding + pos_embed, blocks with windowed / global attention and decomposed relative positions, the neck, the
bilinear upscaling stages and the last layer.  Works in the dtype of the weights it is handed: float64 in the tests (the truth the
device is held to, itself held to the reference's own modules by tests/golden/wam_extractor_*.npz), float32 on the GPU in
scripts/perf_sync.py (the baseline the native path is timed against).  Keys are the checkpoint's, relative to ``detector.``."""
import math

import torch
import torch.nn.functional as F

E, P = "image_encoder.", "pixel_decoder."


def layer_norm_tokens(x, w, b, eps):
    """Over the last axis, biased variance."""
    u = x.mean(-1, keepdim=True)
    s = ((x - u) ** 2).mean(-1, keepdim=True)
    return (x - u) / torch.sqrt(s + eps) * w + b


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def patch_embed(st, cfg, x):
    """[B, 3, R, R] -> tokens [B, g, g, D] (+ bias + pos_embed)."""
    t = F.conv2d(x, st[E + "patch_embed.proj.weight"], st[E + "patch_embed.proj.bias"], stride=cfg.patch_size)
    return t.permute(0, 2, 3, 1) + st[E + "pos_embed"]


def attention_core(q, k, v, rel_h, rel_w, S):
    """q, k, v [n, S * S, hd] of one window size S; rel_h / rel_w [2 S - 1, hd] -> [n, S * S, hd]."""
    n, N, hd = q.shape
    scores = (q * hd ** -0.5) @ k.transpose(-2, -1)
    # every query against every row of the two tables (the UNSCALED q), then the row a key needs is picked: for query (qy, qx) and
    # key (ky, kx) the rows qy - ky + S - 1 of rel_h and qx - kx + S - 1 of rel_w
    pos = torch.arange(S, device=q.device)
    qy, qx = pos.repeat_interleave(S), pos.repeat(S)     # [N]: row and column of token n = y * S + x
    row_h = qy[:, None] - qy[None, :] + (S - 1)          # [N queries, N keys]
    row_w = qx[:, None] - qx[None, :] + (S - 1)
    all_h, all_w = q @ rel_h.t(), q @ rel_w.t()          # [n, N, 2 S - 1]
    term_h = torch.gather(all_h, 2, row_h.expand(n, N, N))
    term_w = torch.gather(all_w, 2, row_w.expand(n, N, N))
    return ((scores + term_h) + term_w).softmax(dim=-1) @ v


def block(st, cfg, i, x):
    """One block: x + attn(norm1(x)), then x + lin2(gelu(lin1(norm2(x)))).  x [B, g, g, D]."""
    p = f"{E}blocks.{i}."
    B, g, _, D = x.shape
    nh, hd = cfg.num_heads, cfg.head_dim
    S = g if i in cfg.global_attn_indexes else cfg.window_size
    h = layer_norm_tokens(x, st[p + "norm1.weight"], st[p + "norm1.bias"], 1e-5)
    nw = g // S
    h = h.view(B, nw, S, nw, S, D).permute(0, 1, 3, 2, 4, 5).reshape(B * nw * nw, S * S, D)      # windows, after norm1
    qkv = (h @ st[p + "attn.qkv.weight"].t() + st[p + "attn.qkv.bias"]).reshape(-1, S * S, 3, nh, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.reshape(3, -1, S * S, hd).unbind(0)
    o = attention_core(q, k, v, st[p + "attn.rel_pos_h"], st[p + "attn.rel_pos_w"], S)
    o = o.view(-1, nh, S * S, hd).permute(0, 2, 1, 3).reshape(-1, S * S, D)
    o = o @ st[p + "attn.proj.weight"].t() + st[p + "attn.proj.bias"]
    o = o.view(B, nw, nw, S, S, D).permute(0, 1, 3, 2, 4, 5).reshape(B, g, g, D)
    x = x + o
    h = layer_norm_tokens(x, st[p + "norm2.weight"], st[p + "norm2.bias"], 1e-5)
    h = gelu(h @ st[p + "mlp.lin1.weight"].t() + st[p + "mlp.lin1.bias"])
    return x + (h @ st[p + "mlp.lin2.weight"].t() + st[p + "mlp.lin2.bias"])


def layer_norm_cf(x, w, b, eps=1e-6):
    """Channels-first LayerNorm of [B, C, H, W]."""
    return layer_norm_tokens(x.permute(0, 2, 3, 1), w, b, eps).permute(0, 3, 1, 2)


def neck(st, x):
    """tokens [B, g, g, D] -> [B, C, g, g]."""
    y = F.conv2d(x.permute(0, 3, 1, 2), st[E + "neck.0.weight"])
    y = layer_norm_cf(y, st[E + "neck.1.weight"], st[E + "neck.1.bias"])
    y = F.conv2d(y, st[E + "neck.2.weight"], padding=1)
    return layer_norm_cf(y, st[E + "neck.3.weight"], st[E + "neck.3.bias"])


def upsample_bilinear(x, f):
    """nn.Upsample(scale_factor=f, mode='bilinear', align_corners=False) of [B, C, H, W], written out: source coordinate
    max(0, (d + 0.5) / f - 0.5), upper neighbour clamped, lambda1 = src - floor(src), lambda0 = 1 - lambda1."""
    H = x.shape[-1]
    d = torch.arange(H * f, dtype=x.dtype, device=x.device)
    src = ((d + 0.5) / f - 0.5).clamp(min=0)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp(max=H - 1)
    l1 = src - i0.to(x.dtype)
    l0 = 1.0 - l1
    rows = x[:, :, i0, :] * l0[:, None] + x[:, :, i1, :] * l1[:, None]
    return rows[:, :, :, i0] * l0 + rows[:, :, :, i1] * l1


def upscale_stage(st, j, f, x, library=False):
    """Upsample('bilinear'): upsample, ReflectionPad2d(1) of the UPSAMPLED tensor, 3 x 3 conv without bias, LayerNorm, GELU.
    `library`: torch's own interpolation kernel instead of the written-out one (the timing baseline; same values to rounding)."""
    p = f"{P}output_upscaling.{j}.upsample_block."
    up = F.interpolate(x, scale_factor=f, mode="bilinear", align_corners=False) if library else upsample_bilinear(x, f)
    u = F.pad(up, (1, 1, 1, 1), mode="reflect")
    y = F.conv2d(u, st[p + "2.weight"])
    return gelu(layer_norm_cf(y, st[p + "3.weight"], st[p + "3.bias"]))


def last_layer(st, x):
    return F.conv2d(x, st[P + "last_layer.weight"], st[P + "last_layer.bias"])


def forward(st, cfg, x, stages=None, library=False):
    """preds [B, nbits + 1, R, R]; with a dict `stages`: tokens0, tokens{i + 1} after block i, neck, up{j}.  `library`: see
    upscale_stage."""
    t = patch_embed(st, cfg, x)
    if stages is not None:
        stages["tokens0"] = t
    for i in range(cfg.depth):
        t = block(st, cfg, i, t)
        if stages is not None:
            stages[f"tokens{i + 1}"] = t
    y = neck(st, t)
    if stages is not None:
        stages["neck"] = y
    for j, f in enumerate(cfg.upscale_stages):
        y = upscale_stage(st, j, f, y, library)
        if stages is not None:
            stages[f"up{j}"] = y
    return last_layer(st, y)


def to_dtype(state, dtype, device="cpu"):
    return {k: v.to(device=device, dtype=dtype) for k, v in state.items()}
