"""Images of any size and mode -> the tensor the VQGAN sees: ``ImageTokenizer.img_tokens_from_pil`` up to the encoder
(deps/chameleon/inference/image_tokenizer.py:51-98).  ``_whiten_transparency`` (RGBA blended over white), ``_vqgan_input_from``
(PIL ``resize(LANCZOS)`` so that the short side equals the target, centre crop, ``u8 / 255 * 2 - 1``).

On a GPU the blend, the resize, the crop and the normalisation are one call for the whole batch (``wmar_image_ingest``,
wmar_amd/csrc/ingest.hip), bit for bit what PIL returns; the host only decodes the files and decides the mode.  For a CPU device the
same steps run through PIL itself, so the module works without a GPU.  EXIF orientation is ignored, as in the reference.
"""
from __future__ import annotations

import base64
import io
import os
from typing import List, Sequence, Tuple

import numpy as np
import torch

MAX_SIDE = 32768


def open_image(x):
    """A PIL image from a path, ``"file:<path>"``, ``"data:...;base64,..."`` (TokenManager.tokens_from_ui's two string forms,
    chameleon.py:150-160), a PIL image (returned as it is) or a uint8 HWC array (L, RGB or RGBA by its shape)."""
    from PIL import Image
    if isinstance(x, Image.Image):
        return x
    if isinstance(x, (str, os.PathLike)):
        s = os.fspath(x)
        if s.startswith("data:"):
            return Image.open(io.BytesIO(base64.b64decode(s.split(",", 1)[1])))
        if s.startswith("file:"):
            s = s.split(":", 1)[1]
        return Image.open(s)
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8 or x.ndim not in (2, 3) or (x.ndim == 3 and x.shape[2] not in (1, 3, 4)):
            raise ValueError(f"open_image: uint8 [H, W], [H, W, 3] or [H, W, 4] array expected, got {x.dtype} {x.shape}")
        return Image.fromarray(x[:, :, 0] if x.ndim == 3 and x.shape[2] == 1 else x)
    raise ValueError(f"open_image: cannot open a {type(x).__name__}")


def pixels_of(img) -> np.ndarray:
    """uint8 [H, W, 3 | 4] of anything ``open_image`` takes, as ``_whiten_transparency`` decides (image_tokenizer.py:51-70): RGB stays
    RGB; anything else is looked at as RGBA: without an alpha below 255 PIL's ``convert("RGB")`` is taken, otherwise the RGBA pixels,
    to be blended over white."""
    if isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (3, 4):
        # already pixels: the same decision without the round trip through PIL (its RGBA -> RGB conversion drops the alpha byte)
        if img.shape[2] == 3 or (img[:, :, 3] < 255).any():
            return img
        return np.ascontiguousarray(img[:, :, :3])
    img = open_image(img)
    if img.mode == "RGB":
        return np.asarray(img)
    rgba = np.asarray(img.convert("RGBA"))
    if not (rgba[:, :, 3] < 255).any():
        return np.asarray(img.convert("RGB"))
    return rgba


def whiten(rgba: np.ndarray) -> np.ndarray:
    """The blend of ``_whiten_transparency`` (float64, truncating cast) for uint8 [H, W, 4]."""
    alpha = rgba[:, :, 3] / 255.0
    return ((1 - alpha[:, :, np.newaxis]) * 255 + alpha[:, :, np.newaxis] * rgba[:, :, :3]).astype("uint8")


def plan(size: Tuple[int, int], target: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((new_width, new_height), (crop_x0, crop_y0)) of ``_vqgan_input_from`` (image_tokenizer.py:72-82) for a (width, height) image:
    Python's ``round`` (half to even) of the scaled sides, ``//`` for the crop origin."""
    s = min(size)
    scale = target / s
    new = (round(scale * size[0]), round(scale * size[1]))
    return new, ((new[0] - target) // 2, (new[1] - target) // 2)


def resize_plan(size: Tuple[int, int], target: int) -> Tuple[int, int]:
    """(new_width, new_height) of torchvision's ``Resize(target)`` for a (width, height) image (transforms/functional.py,
    ``_compute_resized_output_size``): the short side becomes ``target``, the long side ``int(target * long / short)``."""
    w, h = size
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(target * long / short)
    return (target, new_long) if w <= h else (new_long, target)


def random_crop_origin(new: Tuple[int, int], target: int, generator: torch.Generator) -> Tuple[int, int]:
    """(crop_x0, crop_y0) of torchvision's ``RandomCrop(target)`` on a (width, height) image (``RandomCrop.get_params``): no draw when
    both sides already equal ``target``, else the top ``i = randint(0, h - target + 1)`` and then the left ``j = randint(0, w - target +
    1)``, both from ``generator``."""
    w, h = new
    if w == target and h == target:
        return 0, 0
    i = int(torch.randint(0, h - target + 1, size=(1,), generator=generator).item())
    j = int(torch.randint(0, w - target + 1, size=(1,), generator=generator).item())
    return j, i


def _host_one(px: np.ndarray, target: int) -> np.ndarray:
    from PIL import Image
    img = Image.fromarray(whiten(px) if px.shape[2] == 4 else px, "RGB")
    new, (x0, y0) = plan(img.size, target)
    img = img.resize(new, Image.LANCZOS).crop((x0, y0, x0 + target, y0 + target))
    return np.array(img)


def ingest(images: Sequence, target: int, device="cuda", return_u8: bool = False):
    """float32 [n, 3, target, target] in [-1, 1] on ``device`` for ``images`` (anything ``open_image`` takes), one device call for the
    whole batch whatever the images' sizes.  ``return_u8``: also the cropped 8-bit images, uint8 [n, target, target, 3]."""
    device = torch.device(device)
    target = int(target)
    pix = [pixels_of(x) for x in images]
    n = len(pix)
    if n == 0:
        out = torch.empty(0, 3, target, target, dtype=torch.float32, device=device)
        return (out, torch.empty(0, target, target, 3, dtype=torch.uint8, device=device)) if return_u8 else out
    for p in pix:
        if max(p.shape[:2]) > MAX_SIDE:
            raise ValueError(f"ingest: {p.shape[1]} x {p.shape[0]} image (sides up to {MAX_SIDE})")
    if device.type != "cuda":
        u8 = torch.from_numpy(np.stack([_host_one(p, target) for p in pix]))
        out = (u8.to(torch.float64) / 255.0 * 2 - 1).permute(0, 3, 1, 2).to(torch.float32).contiguous().to(device)
        return (out, u8.to(device)) if return_u8 else out
    host, desc = pack(pix, target)
    return ingest_packed(host.to(device, non_blocking=True), desc, target, return_u8)


def pack(pix: List[np.ndarray], target: int, plans=None):
    """(uint8 host tensor holding the images back to back, each at a multiple of 4 bytes; the descriptor array of the C ABI).
    ``plans``: per image ``((new_width, new_height), (crop_x0, crop_y0))`` instead of ``plan``'s."""
    from .. import _lib
    offs, total = [], 0
    for p in pix:
        offs.append(total)
        total += (p.size + 3) // 4 * 4
    host = torch.empty(total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    flat = host.numpy()
    desc = (_lib.ImageDesc * len(pix))()
    for i, (p, o) in enumerate(zip(pix, offs)):
        flat[o:o + p.size] = p.reshape(-1)
        h, w, c = p.shape
        (nw, nh), (x0, y0) = plans[i] if plans is not None else plan((w, h), target)
        desc[i] = _lib.ImageDesc(o, w, h, c, nw, nh, x0, y0)
    return host, desc


def ingest_packed(pixels_dev: torch.Tensor, desc, target: int, return_u8: bool = False, filter: int = 1):
    """The device call on an uploaded pixel buffer (uint8, 1-D) and its descriptors (``pack``).  ``filter``: Pillow's number of the
    resampling filter, 1 = LANCZOS (the default: ``wmar_image_ingest``) or 2 = BILINEAR (``wmar_image_ingest_filtered``)."""
    from .. import _lib
    if not pixels_dev.is_cuda:
        raise RuntimeError("ingest_packed: the pixel buffer must be on the GPU")
    dev, n = pixels_dev.device, len(desc)
    out = torch.empty(n, 3, target, target, dtype=torch.float32, device=dev)
    u8 = torch.empty(n, target, target, 3, dtype=torch.uint8, device=dev) if return_u8 else None
    with torch.cuda.device(dev):
        if filter == _lib.RESAMPLE_LANCZOS:
            _lib.check(_lib.load().wmar_image_ingest(pixels_dev.data_ptr(), pixels_dev.numel(), desc, n, int(target), out.data_ptr(),
                                                     u8.data_ptr() if return_u8 else None, _lib.stream_ptr(dev)))
        else:
            _lib.check(_lib.load().wmar_image_ingest_filtered(pixels_dev.data_ptr(), pixels_dev.numel(), desc, n, int(target), out.data_ptr(),
                                                              u8.data_ptr() if return_u8 else None, int(filter), _lib.stream_ptr(dev)))
    return (out, u8) if return_u8 else out
