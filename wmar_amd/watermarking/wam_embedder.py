"""The WAM embedder on the device: ``Wam.embed`` and the reference's ``WamSync.add_sync`` as calls into libwmar_hip.so
(``wmar_wam_embed`` / ``wmar_wam_add_sync``, wmar_amd/csrc/wam.h), built from the ``embedder.*`` tensors of a WAM checkpoint.

Nothing of the WAM checkout is imported: the encoder / decoder run through the layer plan and kernels of the VQGAN engines, the
message processor, the JND attenuation and the blend are three kernels of their own.  Images must have the network's own size
(256 x 256 for the released checkpoint); other sizes are the PyTorch path's (the reference resizes them with torchvision).
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict

import torch

from .. import _lib
from ..models.engine import _Engine
from ..utils.synth import WamConfig

ATTENUATIONS = {"none": 0, "jnd_1_3": 1, "jnd_1_3_blue": 2}
PREFIX = "embedder."


def config_from_state(state: Dict[str, torch.Tensor], resolution: int = 256, **overrides) -> WamConfig:
    """ch, levels, num_res_blocks, z_channels and nbits from the tensor shapes and key names of ``embedder.*`` (prefix removed);
    scaling_w, scaling_i and the attenuation from the released params.json unless overridden."""
    def level_blocks(side):
        found = {}
        for k in state:
            m = re.match(rf"{side}\.(?:down|up)\.(\d+)\.block\.(\d+)\.conv1\.weight$", k)
            if m:
                found.setdefault(int(m.group(1)), {})[int(m.group(2))] = state[k].shape[0]
        return found
    enc = level_blocks("encoder")
    if not enc or "encoder.conv_in.weight" not in state or "msg_processor.msg_embeddings.weight" not in state:
        raise ValueError("not a WAM embedder: encoder.conv_in / encoder.down.*.block.* / msg_processor.msg_embeddings.weight are missing")
    ch = int(state["encoder.conv_in.weight"].shape[0])
    levels = sorted(enc)
    ch_mult = tuple(int(enc[lvl][0]) // ch for lvl in levels)
    nrb = len(enc[levels[0]])
    nbits = int(state["msg_processor.msg_embeddings.weight"].shape[0]) // 2
    z = int(state["encoder.conv_out.weight"].shape[0])
    if int(state["decoder.conv_in.weight"].shape[1]) != z + 2 * nbits:
        raise ValueError(f"decoder.conv_in takes {int(state['decoder.conv_in.weight'].shape[1])} channels, expected z_channels + 2 * nbits = "
                         f"{z + 2 * nbits} (msg_processor_type binary+concat)")
    attn = set()
    for side, sub in (("encoder", "down"), ("decoder", "up")):
        for k in state:
            m = re.match(rf"{side}\.{sub}\.(\d+)\.attn\.\d+\.q\.weight$", k)
            if m:
                attn.add(resolution >> int(m.group(1)))
    cfg = WamConfig(ch=ch, ch_mult=ch_mult, num_res_blocks=nrb, attn_resolutions=tuple(sorted(attn)), resolution=resolution,
                    z_channels=z, nbits=nbits)
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise TypeError(f"WamConfig has no field {k!r}")
        setattr(cfg, k, v)
    return cfg


class WamEmbedder(_Engine):
    _prefix = "wmar_wam"

    def __init__(self, cfg: WamConfig, state: Dict[str, torch.Tensor], device="cuda", max_batch: int = 16):
        if cfg.attenuation not in ATTENUATIONS:
            raise ValueError(f"attenuation {cfg.attenuation!r}: one of {sorted(ATTENUATIONS)}")
        self.cfg = cfg
        c = _lib.WamConfig()
        c.ch, c.num_res_blocks, c.resolution, c.z_channels, c.nbits = cfg.ch, cfg.num_res_blocks, cfg.resolution, cfg.z_channels, cfg.nbits
        c.n_levels = len(cfg.ch_mult)
        for i, m in enumerate(cfg.ch_mult):
            c.ch_mult[i] = m
        c.n_attn_res = len(cfg.attn_resolutions)
        for i, r in enumerate(cfg.attn_resolutions):
            c.attn_resolutions[i] = r
        c.max_batch = int(max_batch)
        c.scaling_w, c.scaling_i, c.attenuation = float(cfg.scaling_w), float(cfg.scaling_i), ATTENUATIONS[cfg.attenuation]
        self._create(c, state, lambda k: True, device, max_batch)

    @classmethod
    def from_checkpoint(cls, path, device="cuda", max_batch: int = 16, **overrides) -> "WamEmbedder":
        """``torch.load`` a WAM checkpoint (the state dict of ``Wam``, or a dict holding it under "model" / "state_dict") and keep
        its ``embedder.*`` tensors."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        for k in ("model", "state_dict"):
            if isinstance(ckpt, dict) and k in ckpt and isinstance(ckpt[k], dict):
                ckpt = ckpt[k]
        state = {k[len(PREFIX):]: v for k, v in ckpt.items() if k.startswith(PREFIX) and isinstance(v, torch.Tensor)}
        if not state:
            raise ValueError(f"{path}: no '{PREFIX}*' tensors -- not a WAM checkpoint")
        return cls(config_from_state(state, **overrides), state, device=device, max_batch=max_batch)

    # ---- arguments
    def _images(self, imgs, what):
        R = self.cfg.resolution
        if not isinstance(imgs, torch.Tensor) or imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[-1] != R or imgs.shape[-2] != R:
            shape = tuple(imgs.shape) if isinstance(imgs, torch.Tensor) else type(imgs).__name__
            raise ValueError(f"{what}: images must be [B, 3, {R}, {R}], the embedder's own size {R} x {R}; got {shape}")
        if not imgs.is_cuda:
            raise ValueError(f"{what}: images of size {R} x {R} must live on the GPU (the embedder has no CPU implementation)")
        if imgs.shape[0] < 1:
            raise ValueError(f"{what}: empty batch")
        return imgs.to(device=self.device, dtype=torch.float32).contiguous()

    def _msgs(self, msgs, rows, what):
        n = self.cfg.nbits
        if not isinstance(msgs, torch.Tensor) or msgs.dim() != 2 or msgs.shape[1] != n or (rows is not None and msgs.shape[0] != rows):
            shape = tuple(msgs.shape) if isinstance(msgs, torch.Tensor) else type(msgs).__name__
            raise ValueError(f"{what}: messages must be [{rows if rows is not None else 'K'}, {n}], got {shape}")
        if not msgs.is_cuda:
            raise ValueError(f"{what}: messages must live on the GPU")
        if bool(((msgs != 0) & (msgs != 1)).any()):
            raise ValueError(f"{what}: message bits must be 0 or 1")
        return msgs.to(device=self.device, dtype=torch.int32).contiguous()

    # ---- the two calls
    @torch.no_grad()
    def embed(self, imgs: torch.Tensor, msgs: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``Wam.embed`` (models/wam.py:147-192) in WAM-normalised space: {"msgs", "preds_w", "imgs_w"}."""
        x = self._images(imgs, "embed")
        B, R = x.shape[0], self.cfg.resolution
        m = self._msgs(msgs, B, "embed")
        imgs_w, preds_w = torch.empty_like(x), torch.empty_like(x)
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_wam_embed(self._h, x.data_ptr(), B, R, m.data_ptr(), imgs_w.data_ptr(), preds_w.data_ptr(),
                                              _lib.stream_ptr(self.device)))
        return {"msgs": msgs, "preds_w": preds_w, "imgs_w": imgs_w}

    @torch.no_grad()
    def add_sync(self, imgs_pm1: torch.Tensor, msgs: torch.Tensor, masks: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """The reference's ``WamSync.add_sync``: images in [-1, 1], msgs [K, nbits], masks [K, R, R] or [K, 1, R, R] of 0 / 1 ->
        images in [-1, 1] with message k where mask k is the last one set."""
        x = self._images(imgs_pm1, "add_sync")
        B, R = x.shape[0], self.cfg.resolution
        m = self._msgs(msgs, None, "add_sync")
        K = m.shape[0]
        if not 1 <= K <= 8:
            raise ValueError(f"add_sync: {K} messages, the device blend takes 1..8")
        if not isinstance(masks, torch.Tensor) or masks.numel() != K * R * R or masks.shape[0] != K or masks.shape[-1] != R or masks.shape[-2] != R:
            shape = tuple(masks.shape) if isinstance(masks, torch.Tensor) else type(masks).__name__
            raise ValueError(f"add_sync: masks must be [{K}, {R}, {R}] or [{K}, 1, {R}, {R}], got {shape}")
        if not masks.is_cuda:
            raise ValueError("add_sync: masks must live on the GPU")
        if bool(((masks != 0) & (masks != 1)).any()):
            raise ValueError("add_sync: masks must be 0 or 1 (the blend is a selection)")
        mk = masks.to(device=self.device).reshape(K, R, R).to(torch.uint8).contiguous()
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"add_sync: out must be a contiguous float32 {tuple(x.shape)} on {x.device}")
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_wam_add_sync(self._h, x.data_ptr(), B, R, m.data_ptr(), K, mk.data_ptr(), out.data_ptr(),
                                                 _lib.stream_ptr(self.device)))
        return out
