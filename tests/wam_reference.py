"""A float64 restatement of the WAM embedder on plain state dicts: the VAE encoder / decoder (ResnetBlock, stride-2 Downsample with
(0, 1, 0, 1) zero padding, nearest x2 Upsample, AttnBlock, GroupNorm(32, eps 1e-6), swish; decoder ending in tanh), the
"binary+concat" message processor, the JND heat map (Wu et al., "Enhanced just noticeable difference model for images with pattern
complexity", as the released model configures it: one luminance channel in, three out, optional blue weighting), the blend with
attenuation in [0, 1] space and the four-message grid of add_sync.  Written from the published architecture; torch is used as a
float64 array library (conv2d, group_norm), nothing of the reference's code is imported.

State keys are the checkpoint's, relative to ``embedder.``.  Every function takes and returns float64 torch tensors on the CPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).double().view(1, 3, 1, 1)      # the fp32 constants the network was trained with
STD = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).double().view(1, 3, 1, 1)
_M32, _S32 = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32), torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32)
# the inverse transform is a second normalisation whose two constants, -mean / std and 1 / std, are themselves computed in fp32
UMEAN, USTD = (-_M32 / _S32).double().view(1, 3, 1, 1), (1 / _S32).double().view(1, 3, 1, 1)
BLUE = torch.tensor([0.5, 0.5, 1.0], dtype=torch.float64).view(1, 3, 1, 1)


def state64(state):
    return {k: v.detach().cpu().double() for k, v in state.items()}


def normalize(u):
    return (u - MEAN) / STD


def unnormalize(x):
    return (x - UMEAN) / USTD


def _swish(x):
    return x * torch.sigmoid(x)


def _gn(s, p, x):
    return F.group_norm(x, 32, s[p + ".weight"], s[p + ".bias"], eps=1e-6)


def _conv(s, p, x, stride=1, padding=None):
    w = s[p + ".weight"]
    if padding is None:
        padding = w.shape[-1] // 2
    return F.conv2d(x, w, s[p + ".bias"], stride=stride, padding=padding)


def _res(s, p, x):
    h = _conv(s, p + "conv1", _swish(_gn(s, p + "norm1", x)))
    h = _conv(s, p + "conv2", _swish(_gn(s, p + "norm2", h)))
    if p + "nin_shortcut.weight" in s:
        x = _conv(s, p + "nin_shortcut", x)
    return x + h


def _attn(s, p, x):
    h = _gn(s, p + "norm", x)
    q, k, v = _conv(s, p + "q", h), _conv(s, p + "k", h), _conv(s, p + "v", h)
    b, c, hh, ww = q.shape
    w = torch.bmm(q.reshape(b, c, -1).permute(0, 2, 1), k.reshape(b, c, -1)) * (float(c) ** -0.5)
    w = torch.softmax(w, dim=2)
    o = torch.bmm(v.reshape(b, c, -1), w.permute(0, 2, 1)).reshape(b, c, hh, ww)
    return x + _conv(s, p + "proj_out", o)


def _levels(s, side, sub):
    lv = set()
    for k in s:
        if k.startswith(f"{side}.{sub}."):
            lv.add(int(k.split(".")[2]))
    return sorted(lv)


def _blocks(s, prefix):
    n = 0
    while f"{prefix}block.{n}.conv1.weight" in s:
        n += 1
    return n


def encoder(s, x):
    """normalised images [B, 3, R, R] -> latents [B, z, S, S]"""
    h = _conv(s, "encoder.conv_in", x)
    levels = _levels(s, "encoder", "down")
    for lvl in levels:
        p = f"encoder.down.{lvl}."
        for i in range(_blocks(s, p)):
            h = _res(s, f"{p}block.{i}.", h)
            if f"{p}attn.{i}.q.weight" in s:
                h = _attn(s, f"{p}attn.{i}.", h)
        if p + "downsample.conv.weight" in s:
            h = _conv(s, p + "downsample.conv", F.pad(h, (0, 1, 0, 1)), stride=2, padding=0)
    h = _res(s, "encoder.mid.block_1.", h)
    h = _attn(s, "encoder.mid.attn_1.", h)
    h = _res(s, "encoder.mid.block_2.", h)
    return _conv(s, "encoder.conv_out", _swish(_gn(s, "encoder.norm_out", h)))


def message_rows(s, msgs):
    """msgs integer [B, nbits] -> float64 [B, 2 nbits]: sum_j E[2 j + bit_j]"""
    E = s["msg_processor.msg_embeddings.weight"]
    msgs = torch.as_tensor(np.asarray(msgs)).long()
    idx = 2 * torch.arange(msgs.shape[1])[None] + msgs
    return E[idx].sum(dim=1)


def decoder_input(s, latents, msgs):
    m = message_rows(s, msgs)
    return torch.cat([latents, m[:, :, None, None].expand(-1, -1, latents.shape[-2], latents.shape[-1])], dim=1)


def decoder(s, z):
    """[B, z + 2 nbits, S, S] -> tanh(conv_out) [B, 3, R, R]"""
    h = _conv(s, "decoder.conv_in", z)
    h = _res(s, "decoder.mid.block_1.", h)
    h = _attn(s, "decoder.mid.attn_1.", h)
    h = _res(s, "decoder.mid.block_2.", h)
    for lvl in reversed(_levels(s, "decoder", "up")):
        p = f"decoder.up.{lvl}."
        for i in range(_blocks(s, p)):
            h = _res(s, f"{p}block.{i}.", h)
            if f"{p}attn.{i}.q.weight" in s:
                h = _attn(s, f"{p}attn.{i}.", h)
        if p + "upsample.conv.weight" in s:
            h = _conv(s, p + "upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
    return torch.tanh(_conv(s, "decoder.conv_out", _swish(_gn(s, "decoder.norm_out", h))))


LUM_K = torch.tensor([[1, 1, 1, 1, 1], [1, 2, 2, 2, 1], [1, 2, 0, 2, 1], [1, 2, 2, 2, 1], [1, 1, 1, 1, 1]], dtype=torch.float64).view(1, 1, 5, 5)
SOBEL_X = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=torch.float64).view(1, 1, 3, 3)
SOBEL_Y = torch.tensor([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=torch.float64).view(1, 1, 3, 3)
RGB = [float(np.float32(v)) for v in (0.299, 0.587, 0.114)]      # the weights are an fp32 tensor in the model


def luminance_average(u):
    """The value the two-branch curve is evaluated on: the 5 x 5 stencil of the luminance / 32, zero padded.  [B, 1, R, R]"""
    u = 255.0 * u
    lum = RGB[0] * u[:, 0:1] + RGB[1] * u[:, 1:2] + RGB[2] * u[:, 2:3]
    return F.conv2d(lum, LUM_K, padding=2) / 32.0, lum


def jnd_heat(u):
    """images in [0, 1] [B, 3, R, R] -> heat [B, 1, R, R] (one channel; the blue weights are applied by `blend`)"""
    la, lum = luminance_average(u)
    la = torch.where(la <= 127.0, 17.0 * (1.0 - torch.sqrt(la / 127.0 + 1e-5)), 3.0 / 128.0 * (la - 127.0) + 3.0)
    g = torch.sqrt(F.conv2d(lum, SOBEL_X, padding=1) ** 2 + F.conv2d(lum, SOBEL_Y, padding=1) ** 2)
    cm = 0.117 * (16.0 * g ** 2.4 / (g ** 2 + 26.0 ** 2))
    return torch.clamp_min(la + cm - 0.3 * torch.minimum(la, cm), 0.0) / 255.0


def la_excluded(u):
    """bool [B, R, R]: pixels whose la lies within wam_cases.LA_MARGIN of the switch at 127"""
    from tests import wam_cases
    la, _ = luminance_average(torch.as_tensor(u).double())
    return (la[:, 0] - 127.0).abs() < wam_cases.LA_MARGIN


def blend(x, preds_w, scaling_w=2.0, scaling_i=1.0, attenuation="jnd_1_3_blue"):
    """normalised images and tanh outputs -> watermarked images, normalised"""
    w = scaling_i * x + scaling_w * preds_w
    if attenuation == "none":
        return w
    u, uw = unnormalize(x), unnormalize(w)
    heat = jnd_heat(u).expand(-1, 3, -1, -1)
    if attenuation == "jnd_1_3_blue":
        heat = heat * BLUE
    return normalize(u + heat * (uw - u))


def embed(s, x, msgs, **kw):
    """Wam.embed at the network's own size: {"latents", "decoder_input", "preds_w", "imgs_w"}"""
    lat = encoder(s, x)
    zin = decoder_input(s, lat, msgs)
    preds = decoder(s, zin)
    return {"latents": lat, "decoder_input": zin, "preds_w": preds, "imgs_w": blend(x, preds, **kw)}


def grid_masks(R, n_msgs=4):
    """The 2 x 2 grid of add_sync: message k in the k-th square, a cross of 19 pixels (37 unless R is 256) left free.  [4, 1, R, R]"""
    m = torch.zeros(n_msgs, 1, R, R, dtype=torch.float64)
    q = R // 2
    for i in range(2):
        for j in range(2):
            m[i * 2 + j, 0, i * q:(i + 1) * q, j * q:(j + 1) * q] = 1
    leeway = 18 if R == 256 else 36
    a, b = R // 2 - leeway // 2, R // 2 + leeway // 2 + 1
    m[:, :, :, a:b] = 0
    m[:, :, a:b, :] = 0
    return m


def add_sync(s, imgs_pm1, msgs, masks, **kw):
    """images in [-1, 1], msgs [K, nbits], masks [K, 1, R, R] of 0 / 1 -> images in [-1, 1]"""
    x = normalize((imgs_pm1 + 1.0) / 2.0)
    lat = encoder(s, x)
    multi = x.clone()
    msgs = np.asarray(msgs)
    for k in range(msgs.shape[0]):
        preds = decoder(s, decoder_input(s, lat, np.repeat(msgs[k:k + 1], x.shape[0], axis=0)))
        multi = blend(x, preds, **kw) * masks[k] + multi * (1 - masks[k])
    return (unnormalize(multi) * 2.0 - 1.0).clamp(-1, 1)
