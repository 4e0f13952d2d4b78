"""Shapes, pixel patterns and the PIL path the image-ingest tests share (CPU and GPU)."""
import numpy as np
import torch
from PIL import Image

TARGETS = (64, 256, 512)


def shapes_for(T):
    """(width, height) inputs per target: degenerate, strips, the target itself, one pixel off, 1:3, a halving, photo sizes, an upscale."""
    return [(1, 1), (2, 3), (3, 2), (2000, 20), (20, 2000), (T, T), (T + 1, T), (T, T + 1), (T, 3 * T), (3 * T, T), (2 * T + 1, 2 * T),
            (1920, 1080), (1024, 1024), (4000, 3000), (T // 2 + 3, T - 7)]


# the two shapes whose resized long side is 153 600 pixels: only their crop window is ever computed
STRIPS = [(512, (1, 300)), (512, (300, 1))]
CASES = [(T, wh) for T in TARGETS for wh in shapes_for(T)] + STRIPS
PATTERNS = ("random", "checker", "binary")


def pattern(name, w, h, c=3, seed=0):
    rng = np.random.default_rng(seed + 7 * w + 13 * h)
    if name == "random":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if name == "checker":                       # 1-pixel checkerboard
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], c, axis=2)
    return (rng.integers(0, 2, (h, w, c), dtype=np.uint8) * 255).astype(np.uint8)       # random 0 / 255


def plan(size, target):
    s = min(size)
    scale = target / s
    new = (round(scale * size[0]), round(scale * size[1]))
    return new, ((new[0] - target) // 2, (new[1] - target) // 2)


def whiten_transparency(img):
    """ImageTokenizer._whiten_transparency, step for step."""
    if img.mode == "RGB":
        return img
    vals_rgba = np.array(img.convert("RGBA"))
    if not (vals_rgba[:, :, 3] < 255).any():
        return img.convert("RGB")
    alpha = vals_rgba[:, :, 3] / 255.0
    vals_rgb = (1 - alpha[:, :, np.newaxis]) * 255 + alpha[:, :, np.newaxis] * vals_rgba[:, :, :3]
    return Image.fromarray(vals_rgb.astype("uint8"), "RGB")


def pil_path(img, T):
    """(float32 [3, T, T], uint8 [T, T, 3]): _whiten_transparency + _vqgan_input_from through PIL itself."""
    img = whiten_transparency(img)
    s = min(img.size)
    scale = T / s
    new_size = (round(scale * img.size[0]), round(scale * img.size[1]))
    img = img.resize(new_size, Image.LANCZOS)
    x0, y0 = (img.width - T) // 2, (img.height - T) // 2
    img = img.crop((x0, y0, x0 + T, y0 + T))
    u8 = np.array(img)
    x = u8 / 255.0
    x = x * 2 - 1
    return torch.from_numpy(x).permute(2, 0, 1).float(), u8
