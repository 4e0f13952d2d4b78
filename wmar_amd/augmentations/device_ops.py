"""The evaluation transforms as kernels of this build (``wmar_augment``, wmar_amd/csrc/augment.hip; ``wmar_jpeg``,
wmar_amd/csrc/jpeg.hip): what the transform modules run for tensors on the MI355X, and the harness's fused form -- one launch (two
for JPEG) that reads the decoder's [-1, 1] batch, transforms it in [0, 1], clamps and writes [-1, 1] for the encoder
(generate.py:146-150 around every (transform, parameter) pair; ~90 pairs per image).  CPU tensors keep the torch restatements in
valuemetric.py / geometric.py and PIL for JPEG (host-side utilities, as in the reference); so do JPEG inputs whose height or width is
not a multiple of 16."""
from __future__ import annotations

import os

import torch

from .. import _lib

IDENTITY, BLUR, NOISE, BRIGHTNESS, ROTATE, FLIP_H, CROP_RESIZE, CROP_PAD = range(8)


def eligible(image: torch.Tensor) -> bool:
    if os.environ.get("WMAR_AUG_TORCH"):        # A/B knob: the torch restatements on the device instead of the kernels
        return False
    return image.is_cuda and image.dtype == torch.float32 and image.dim() in (3, 4)


def _launch(op: int, x: torch.Tensor, p0: float, p1: float, noise, pm1: bool) -> torch.Tensor:
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    L = _lib.load()
    with torch.cuda.device(x.device):
        _lib.check(L.wmar_augment(int(op), x.data_ptr(), out.data_ptr(), noise.data_ptr() if noise is not None else None, B, C, H, W,
                                  1 if pm1 else 0, float(p0), float(p1), _lib.stream_ptr(x.device)))
    return out


class _Augment(torch.autograd.Function):
    """``wmar_augment`` with its vector-Jacobian product ``wmar_augment_backward`` (csrc/augment.hip): the gradient of the launch as
    it is implemented, range change and clamp included; the noise draws get none.  `x` is contiguous [B, C, H, W]."""

    @staticmethod
    def forward(ctx, x, op, p0, p1, noise, pm1):
        ctx.save_for_backward(x, noise)
        ctx.call = (op, p0, p1, pm1)
        return _launch(op, x, p0, p1, noise, pm1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, noise = ctx.saved_tensors
        op, p0, p1, pm1 = ctx.call
        B, C, H, W = x.shape
        g = grad_out.to(torch.float32).contiguous()
        grad_in = torch.empty_like(x)
        ws = torch.empty_like(x) if op == BLUR else None         # g * mask between the two blur launches
        L = _lib.load()
        with torch.cuda.device(x.device):
            _lib.check(L.wmar_augment_backward(int(op), x.data_ptr(), g.data_ptr(), grad_in.data_ptr(),
                                               noise.data_ptr() if noise is not None else None, ws.data_ptr() if ws is not None else None,
                                               B, C, H, W, 1 if pm1 else 0, float(p0), float(p1), _lib.stream_ptr(x.device)))
        return grad_in, None, None, None, None, None


def run(op: int, image: torch.Tensor, p0: float = 0.0, p1: float = 0.0, noise: torch.Tensor = None, pm1: bool = False) -> torch.Tensor:
    """One launch of transform `op` over the batch.  When a gradient is wanted of `image` the launch joins the autograd graph
    (`_Augment`; unsqueeze / contiguous are torch's own differentiable steps, so the gradient returns in the shape and strides of the
    original tensor); otherwise the launch alone."""
    x = image.unsqueeze(0) if image.dim() == 3 else image
    x = x.contiguous()
    if noise is not None:
        noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
        assert noise.numel() == x.numel()
    if torch.is_grad_enabled() and image.requires_grad:
        out = _Augment.apply(x, int(op), float(p0), float(p1), noise.detach() if noise is not None else None, bool(pm1))
    else:
        out = _launch(op, x, p0, p1, noise, pm1)
    return out[0] if image.dim() == 3 else out


def jpeg_supported(image: torch.Tensor) -> bool:
    """the device JPEG covers 3-channel images whose height and width are multiples of 16 (whole 4:2:0 MCUs, no edge padding)"""
    return eligible(image) and image.shape[-3] == 3 and image.shape[-2] % 16 == 0 and image.shape[-1] % 16 == 0


def jpeg(image: torch.Tensor, quality: int, pm1: bool = False, passthrough: bool = True) -> torch.Tensor:
    """``JPEG(passthrough=passthrough)(image, quality)`` of valuemetric.py for a [B, 3, H, W] / [3, H, W] tensor on the device, H and W
    multiples of 16: the pixels PIL's encoder + decoder return, bit for bit, without the host round trip (wmar_jpeg, two launches
    over the whole batch).  With `pm1` the pixels cross the call in [-1, 1] (the harness's fused form)."""
    x = image.unsqueeze(0) if image.dim() == 3 else image
    x = x.contiguous()
    if x.data_ptr() % 16:                       # a view at an odd offset: the kernels read and write 16-byte vectors
        x = x.clone()
    B, C, H, W = x.shape
    if C != 3:
        raise ValueError(f"jpeg: {C}-channel image (RGB only)")
    out = torch.empty_like(x)
    L = _lib.load()
    ws = torch.empty(int(L.wmar_jpeg_workspace_bytes(B, H, W)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.wmar_jpeg(x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, int(quality), 1 if pm1 else 0,
                               1 if passthrough else 0, _lib.stream_ptr(x.device)))
    return out[0] if image.dim() == 3 else out


def _rotation(angle):
    quarters, rest = divmod(angle, 90)          # floor division: -20 -> (-1, 70), as Rotate.forward
    return quarters % 4, rest


def fused(name: str, imgs_pm1: torch.Tensor, param):
    """`aug(imgs / 2 + 0.5, param).clamp(0, 1) * 2 - 1` of the AugmentationManager table entry `name` as ONE launch (jpeg: two), or
    None when the entry has no device form for this tensor (not eligible; jpeg: not 3 channels or a size that is not a multiple of
    16).  Bit-identical to the unfused sequence (tests/test_gpu_augment_kernels.py, tests/test_gpu_jpeg.py)."""
    if not eligible(imgs_pm1) or imgs_pm1.dim() != 4:
        return None
    H, W = imgs_pm1.shape[-2:]
    if name == "gaussian-blur":
        return run(IDENTITY if param == 0 else BLUR, imgs_pm1, param, pm1=True)
    if name == "gaussian-noise":
        return run(NOISE, imgs_pm1, param, noise=torch.randn_like(imgs_pm1), pm1=True)      # one randn draw, as GaussianNoise.forward
    if name == "brightness":
        return run(BRIGHTNESS, imgs_pm1, param, pm1=True)
    if name == "rotation":
        q, rest = _rotation(param)
        if q % 2 and H != W:
            return None
        return run(ROTATE, imgs_pm1, q, rest, pm1=True)
    if name == "flip-h":
        return run(FLIP_H if param else IDENTITY, imgs_pm1, pm1=True)
    if name == "upperleft-crop":
        oh, ow = int(param * H), int(param * W)
        return run(IDENTITY if (oh, ow) == (H, W) else CROP_RESIZE, imgs_pm1, oh, ow, pm1=True)
    if name == "jpeg":
        return jpeg(imgs_pm1, param, pm1=True) if jpeg_supported(imgs_pm1) else None
    return None
