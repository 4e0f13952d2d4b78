"""The WAM extractor on the device: ``Wam.detect`` (models/wam.py:194-222, without its resize) as one call into libwmar_hip.so
(``wmar_wamx_detect``, wmar_amd/csrc/wam_extractor.h), built from the ``detector.*`` tensors of a WAM checkpoint.

Nothing of the WAM checkout is imported.  Images must have the network's own size (256 x 256 for the released checkpoint); other
sizes are the PyTorch path's (the reference resizes them with torchvision).
"""
from __future__ import annotations

import re
from typing import Dict

import torch

from .. import _lib
from ..models.engine import _Engine
from ..utils.synth import WamExtractorConfig, wamx_shapes

PREFIX = "detector."
E, P = "image_encoder.", "pixel_decoder."


def config_from_state(state: Dict[str, torch.Tensor]) -> WamExtractorConfig:
    """The configuration from the tensor shapes and key names of ``detector.*`` (prefix removed): depth from the block count, the
    global blocks from the length of their rel_pos tables, the window size from (rows + 1) / 2, num_heads from
    embed_dim / rel_pos.shape[1], the stages from the conv shapes, nbits from last_layer."""
    need = (E + "patch_embed.proj.weight", E + "pos_embed", E + "neck.0.weight", P + "last_layer.weight")
    if any(k not in state for k in need):
        raise ValueError(f"not a WAM extractor: {[k for k in need if k not in state]} missing")
    D, _, patch, _ = (int(v) for v in state[E + "patch_embed.proj.weight"].shape)
    grid = int(state[E + "pos_embed"].shape[1])
    blocks = sorted({int(m.group(1)) for m in (re.match(rf"{re.escape(E)}blocks\.(\d+)\.", k) for k in state) if m})
    if not blocks or blocks != list(range(len(blocks))):
        raise ValueError(f"not a WAM extractor: blocks {blocks}")
    rows = []
    for i in blocks:
        k = f"{E}blocks.{i}.attn.rel_pos_h"
        if k not in state:
            raise ValueError(f"block {i} has no rel_pos_h: the extractor is built for use_rel_pos only")
        rows.append(int(state[k].shape[0]))
    sizes = [(r + 1) // 2 for r in rows]
    glob = tuple(i for i in blocks if sizes[i] == grid)
    win = sorted({s for i, s in enumerate(sizes) if i not in glob})
    if len(win) > 1:
        raise ValueError(f"blocks with rel_pos tables for windows of {win}: one window size expected")
    window = win[0] if win else grid
    hd = int(state[f"{E}blocks.0.attn.rel_pos_h"].shape[1])
    stages, j, C = [], 0, int(state[E + "neck.0.weight"].shape[0])
    out_chans = C
    while f"{P}output_upscaling.{j}.upsample_block.2.weight" in state:
        co, ci = (int(v) for v in state[f"{P}output_upscaling.{j}.upsample_block.2.weight"].shape[:2])
        if ci != C or co < 1 or ci % co:
            raise ValueError(f"upscaling stage {j}: a conv of {ci} -> {co} channels behind {C}")
        stages.append(ci // co)
        C, j = co, j + 1
    nbits = int(state[P + "last_layer.weight"].shape[0]) - 1
    return WamExtractorConfig(img_size=grid * patch, patch_size=patch, embed_dim=D, depth=len(blocks), num_heads=D // hd, window_size=window,
                              global_attn_indexes=glob, out_chans=out_chans, upscale_stages=tuple(stages), nbits=nbits)


class WamExtractor(_Engine):
    _prefix = "wmar_wamx"

    def __init__(self, cfg: WamExtractorConfig, state: Dict[str, torch.Tensor], device="cuda", max_batch: int = 16):
        self.cfg = cfg
        if len(cfg.global_attn_indexes) > 16 or not 1 <= len(cfg.upscale_stages) <= 4:
            raise ValueError(f"{len(cfg.global_attn_indexes)} global blocks (at most 16), {len(cfg.upscale_stages)} upscaling stages (1..4)")
        # the C ABI carries no shapes: the table lengths are checked here (2 S - 1 rows: get_rel_pos never interpolates)
        for i in range(cfg.depth):
            S = cfg.grid if i in cfg.global_attn_indexes else cfg.window_size
            for name in ("rel_pos_h", "rel_pos_w"):
                t = state.get(f"{E}blocks.{i}.attn.{name}")
                if t is not None and (t.dim() != 2 or t.shape[0] != 2 * S - 1):
                    raise ValueError(f"blocks.{i}.attn.{name} is {tuple(t.shape)}: a table of 2 S - 1 = {2 * S - 1} rows is expected for "
                                     f"S = {S} (interpolated tables are not built)")
        # ... and so are all the others: the library reads each tensor at the size the configuration gives it
        for k, shp in wamx_shapes(cfg).items():
            if k in state and tuple(state[k].shape) != shp:
                raise ValueError(f"{k} is {tuple(state[k].shape)}, the configuration expects {shp}")
        c = _lib.WamxConfig()
        c.img_size, c.patch_size, c.embed_dim, c.depth, c.num_heads = cfg.img_size, cfg.patch_size, cfg.embed_dim, cfg.depth, cfg.num_heads
        c.window_size, c.out_chans, c.nbits, c.max_batch = cfg.window_size, cfg.out_chans, cfg.nbits, int(max_batch)
        c.n_global = len(cfg.global_attn_indexes)
        for i, b in enumerate(cfg.global_attn_indexes):
            c.global_attn_indexes[i] = b
        c.n_stages = len(cfg.upscale_stages)
        for i, f in enumerate(cfg.upscale_stages):
            c.upscale_stages[i] = f
        self._create(c, state, lambda k: True, device, max_batch)

    @classmethod
    def from_checkpoint(cls, path, device="cuda", max_batch: int = 16) -> "WamExtractor":
        """``torch.load`` a WAM checkpoint (the state dict of ``Wam``, or a dict holding it under "model" / "state_dict") and keep
        its ``detector.*`` tensors."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        for k in ("model", "state_dict"):
            if isinstance(ckpt, dict) and k in ckpt and isinstance(ckpt[k], dict):
                ckpt = ckpt[k]
        state = {k[len(PREFIX):]: v for k, v in ckpt.items() if k.startswith(PREFIX) and isinstance(v, torch.Tensor)}
        if not state:
            raise ValueError(f"{path}: no '{PREFIX}*' tensors -- not a WAM checkpoint")
        return cls(config_from_state(state), state, device=device, max_batch=max_batch)

    @torch.no_grad()
    def detect(self, imgs: torch.Tensor) -> Dict[str, torch.Tensor]:
        """``Wam.detect`` in WAM-normalised space: {"preds": [B, nbits + 1, R, R]} (mask logit, bit logits; no sigmoid)."""
        R = self.cfg.img_size
        if not isinstance(imgs, torch.Tensor) or imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[-1] != R or imgs.shape[-2] != R:
            shape = tuple(imgs.shape) if isinstance(imgs, torch.Tensor) else type(imgs).__name__
            raise ValueError(f"detect: images must be [B, 3, {R}, {R}], the extractor's own size {R} x {R}; got {shape}")
        if not imgs.is_cuda:
            raise ValueError(f"detect: images of size {R} x {R} must live on the GPU (the extractor has no CPU implementation)")
        if imgs.shape[0] < 1:
            raise ValueError("detect: empty batch")
        x = imgs.to(device=self.device, dtype=torch.float32).contiguous()
        B = x.shape[0]
        preds = torch.empty(B, self.cfg.nbits + 1, R, R, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_wamx_detect(self._h, x.data_ptr(), B, R, preds.data_ptr(), _lib.stream_ptr(self.device)))
        return {"preds": preds}
