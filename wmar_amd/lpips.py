"""LPIPS on the MI355X: the perceptual half of the reference's fine-tuning regulariser ``|x_orig_dec - x_rec| + LPIPS(x_orig_dec, x_rec)``
(deps/taming/modules/losses/vqperceptual.py:83-92, deps/rar/modeling/titok.py:113-115) over the native engine ``wmar_lpips_*``
(include/wmar_hip.h; wmar_amd/csrc/lpips.h).

``LPIPS(state)(input, target)`` is the reference module's ``forward`` in ``.eval()`` (deps/taming/modules/losses/lpips.py:41-54): a
frozen VGG16 on both images, five normalised feature taps, the lin heads, ``[B, 1, 1, 1]``.  It is a ``torch.autograd.Function``; the
gradient goes to ``input`` only and every weight is frozen.  ``state`` uses the reference module's own keys (``scaling_layer.shift``,
``net.slice1.0.weight`` .. ``net.slice5.28.bias``, ``lin0.model.1.weight`` ..); ``LPIPS.from_files`` builds it from the two files a user
of the reference has.  There is one tape: a backward must belong to the last forward, anything else raises.  No PyTorch fallback."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .models.engine import _require_cuda
from .utils.synth import LPIPS_CHNS, LPIPS_SCALE, LPIPS_SHIFT, LPIPS_SLICE_CONVS, lpips_shapes


def state_from_vgg_and_lin(vgg: Dict[str, torch.Tensor], lin: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """torchvision's VGG16 state dict (``features.N.weight`` / ``.bias``) plus the reference's ``vgg.pth`` (the ``lin*`` layers) -> the
    reference LPIPS module's layout, with the scaling constants of lpips.py:60-61."""
    out = {"scaling_layer.shift": torch.tensor(LPIPS_SHIFT, dtype=torch.float32).view(1, 3, 1, 1),
           "scaling_layer.scale": torch.tensor(LPIPS_SCALE, dtype=torch.float32).view(1, 3, 1, 1)}
    for k, idxs in enumerate(LPIPS_SLICE_CONVS):
        for i in idxs:
            for part in ("weight", "bias"):
                src = f"features.{i}.{part}"
                if src not in vgg:
                    raise KeyError(f"LPIPS: the VGG16 state has no '{src}' (expected torchvision's vgg16 state dict)")
                out[f"net.slice{k + 1}.{i}.{part}"] = vgg[src]
    for k in range(5):
        key = f"lin{k}.model.1.weight"
        if key not in lin:
            raise KeyError(f"LPIPS: the lin state has no '{key}' (expected the reference's vgg.pth)")
        out[key] = lin[key]
    return out


class _Lpips(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, inp, target):
        ctx.eng, ctx.dtype = eng, inp.dtype
        value, ctx.tape = eng._forward(eng._prepare(inp, "input"), target, True)
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return None, ctx.eng._backward(ctx.tape, g).to(ctx.dtype), None


class LPIPS:
    def __init__(self, state: Dict[str, torch.Tensor], resolution: int = 256, max_batch: int = 4, device="cuda",
                 chns: Sequence[int] = LPIPS_CHNS):
        self._L = _lib.load()
        self.device = torch.device(device)
        self.resolution, self.max_batch, self.chns = int(resolution), int(max_batch), tuple(int(c) for c in chns)
        if len(self.chns) != 5:
            raise ValueError(f"LPIPS: five slice widths expected, got {self.chns}")
        if self.resolution < 128 or self.resolution % 128:
            raise ValueError(f"LPIPS: resolution {self.resolution} is not a multiple of 128 (relu5_3 is resolution / 16 and the "
                             "convolutions work on 8 x 8 tiles)")
        tensors = {}
        for k, shp in lpips_shapes(self.chns).items():
            if k not in state:
                raise KeyError(f"LPIPS: state has no '{k}'")
            t = state[k].detach().to(self.device, torch.float32).contiguous()
            if tuple(t.shape) != shp:
                raise ValueError(f"LPIPS: {k} has shape {tuple(t.shape)}, expected {shp}")
            _require_cuda(t, k)
            tensors[k] = t
        cfg = _lib.LpipsConfig()
        for i, c in enumerate(self.chns):
            cfg.chns[i] = c
        cfg.resolution, cfg.max_batch = self.resolution, self.max_batch
        names, ptrs, n = _lib.tensor_table(tensors)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_lpips_create(C.byref(cfg), names, ptrs, n, _lib.stream_ptr(self.device), C.byref(h)))
        self._h = h
        self._serial, self._tape = 0, 0         # serial number of the forward the tape belongs to (0: none)
        self.last_per_tap = None                # [5, B]: the five terms of the last forward

    @classmethod
    def from_files(cls, vgg_path: str, lin_path: str, **kw) -> "LPIPS":
        """``vgg_path``: torchvision's VGG16 state dict; ``lin_path``: the reference's ``vgg.pth``."""
        vgg = torch.load(vgg_path, map_location="cpu")
        lin = torch.load(lin_path, map_location="cpu")
        return cls(state_from_vgg_and_lin(vgg, lin), **kw)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.wmar_lpips_destroy(h)
            self._h = None

    @property
    def device_bytes(self) -> int:
        return int(self._L.wmar_lpips_device_bytes(self._h))

    def _prepare(self, x: torch.Tensor, what: str) -> torch.Tensor:
        _require_cuda(x, what)
        R = self.resolution
        if x.ndim != 4 or tuple(x.shape[1:]) != (3, R, R):
            raise ValueError(f"LPIPS: {what}: expected [B, 3, {R}, {R}], got {tuple(x.shape)}")
        if x.shape[0] < 1 or x.shape[0] > self.max_batch:
            raise ValueError(f"batch {x.shape[0]} outside 1..max_batch={self.max_batch}: a tape holds one chunk, batches are not split")
        return x.detach().to(torch.float32).contiguous()

    def _forward(self, inp: torch.Tensor, target: torch.Tensor, keep_tape: bool):
        B = inp.shape[0]
        value = torch.empty(B, dtype=torch.float32, device=self.device)
        per_tap = torch.empty(5, B, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_lpips_forward(self._h, inp.data_ptr(), target.data_ptr(), B, int(keep_tape), value.data_ptr(),
                                                  per_tap.data_ptr(), _lib.stream_ptr(self.device)))
        self._serial += 1
        self._tape = self._serial if keep_tape else 0
        self.last_per_tap = per_tap
        return value.view(B, 1, 1, 1), self._serial

    def _backward(self, tape: int, g: torch.Tensor) -> torch.Tensor:
        if self._tape != tape:
            raise RuntimeError("LPIPS: this backward does not belong to the last forward (a later forward replaced the tape)")
        B, R = g.shape[0], self.resolution
        g = g.reshape(B).to(torch.float32).contiguous()
        gi = torch.empty(B, 3, R, R, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.wmar_lpips_backward(self._h, g.data_ptr(), B, gi.data_ptr(), _lib.stream_ptr(self.device)))
        return gi

    def __call__(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """``[B, 3, R, R]`` x 2 -> ``[B, 1, 1, 1]``; differentiable towards ``input``."""
        if target.requires_grad and torch.is_grad_enabled():
            raise ValueError("LPIPS: the gradient goes to `input` only: detach `target` (the reference passes the frozen decoder's image there)")
        a, b = self._prepare(input, "input"), self._prepare(target, "target")
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"LPIPS: input has batch {a.shape[0]}, target {b.shape[0]}")
        if torch.is_grad_enabled() and input.requires_grad:
            return _Lpips.apply(self, input, b)
        return self._forward(a, b, False)[0]
