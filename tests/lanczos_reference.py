"""Pillow's 8-bit LANCZOS resample, restated in numpy (the steps wmar_amd/csrc/ingest.hip runs on the device), plus the reference's
transparency whitening and the centre-crop plan around it.  tests/test_ingest_reference.py pins this file to PIL byte for byte.

Per axis, from `in_size` to `out_size` pixels (Pillow: precompute_coeffs, normalize_coeffs_8bpc):
  scale = in / out, filterscale = max(scale, 1), support = 3 * filterscale, ksize = ceil(support) * 2 + 1
  output xx: center = (xx + 0.5) * scale, xmin = max(0, int(center - support + 0.5)),
             count = min(in, int(center + support + 0.5)) - xmin,
             k[x] = lanczos((x + xmin - center + 0.5) * (1 / filterscale)), divided by their sum
  fixed point: ki = int(k * 2^22 -+ 0.5) (half away from zero, truncating cast)
Output byte (the 8bpc horizontal / vertical passes): clip(((1 << 21) + sum pixel * ki) >> 22, 0, 255), arithmetic shift; the
horizontal pass runs first and its result is rounded to 8 bits before the vertical pass reads it.  An axis whose size does not change
is not filtered."""
import numpy as np

PRECISION_BITS = 22


def _sinc(x):
    px = np.where(x == 0.0, 1.0, x * np.pi)
    return np.where(x == 0.0, 1.0, np.sin(px) / px)


def lanczos(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where((x >= -3.0) & (x < 3.0), _sinc(x) * _sinc(x / 3.0), 0.0)


def coeffs(in_size, out_size, out0=0, n_out=None):
    """(xmin int32 [n], count int32 [n], k int32 [n, ksize], ksize) for the outputs [out0, out0 + n_out) of one axis."""
    n_out = out_size - out0 if n_out is None else n_out
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out0, out0 + n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = lanczos((x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / filterscale))
    w = np.where(x < count[:, None], w, 0.0)
    ww = _seq_sum(w)                             # left to right, as Pillow adds them (numpy's pairwise sum differs on long rows)
    k = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    ki = np.where(k < 0, -0.5 + k * (1 << PRECISION_BITS), 0.5 + k * (1 << PRECISION_BITS)).astype(np.int32)
    return xmin.astype(np.int32), count.astype(np.int32), ki, ksize


def _seq_sum(w):
    acc = np.zeros((w.shape[0], 1))
    for j in range(w.shape[1]):
        acc[:, 0] += w[:, j]
    return acc


def _pass(img, xmin, count, ki, axis):
    """One 8bpc pass along `axis` of uint8 [H, W, C]: int32 accumulators (wrapping like C), shift, clip."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(xmin),) + src.shape[1:], dtype=np.uint8)
    peak = 0
    for i in range(len(xmin)):
        a, n = int(xmin[i]), int(count[i])
        acc = np.tensordot(ki[i, :n].astype(np.int64), src[a:a + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        peak = max(peak, int(np.abs(acc).max()) if acc.size else 0)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    assert peak < 2 ** 31, "accumulator beyond int32"
    return np.moveaxis(out, 0, axis)


def resize_window(u8, new_size, box):
    """The pixels [x0, x1) x [y0, y1) of PIL's `Image.fromarray(u8).resize(new_size, LANCZOS)` for uint8 [H, W, C], computing only
    what the window needs (the window's columns, and the input rows its vertical taps touch)."""
    H, W = u8.shape[:2]
    nw, nh = new_size
    x0, y0, x1, y1 = box
    img = u8
    if nh != H:
        ymin, ycount, yk, _ = coeffs(H, nh, y0, y1 - y0)
        r0, r1 = int(ymin[0]), int(ymin[-1] + ycount[-1])
        img = img[r0:r1]
    else:
        img = img[y0:y1]
    if nw != W:
        xmin, xcount, xk, _ = coeffs(W, nw, x0, x1 - x0)
        img = _pass(img, xmin, xcount, xk, 1)
    else:
        img = img[:, x0:x1]
    if nh != H:
        img = _pass(img, ymin - r0, ycount, yk, 0)
    return np.ascontiguousarray(img)


def resize(u8, new_size):
    return resize_window(u8, new_size, (0, 0, new_size[0], new_size[1]))


def whiten(rgba):
    """ImageTokenizer._whiten_transparency's blend over white for uint8 [H, W, 4] (float64, truncating cast)."""
    alpha = rgba[:, :, 3] / 255.0
    return ((1 - alpha[:, :, np.newaxis]) * 255 + alpha[:, :, np.newaxis] * rgba[:, :, :3]).astype("uint8")


def plan(size, target):
    """(new_size, (x0, y0)) of ImageTokenizer._vqgan_input_from for a (width, height) image: Python's round (half to even), //."""
    s = min(size)
    scale = target / s
    new = (round(scale * size[0]), round(scale * size[1]))
    return new, ((new[0] - target) // 2, (new[1] - target) // 2)


def ingest(u8, target):
    """uint8 [H, W, 3 | 4] -> (float32 [3, T, T] in [-1, 1], uint8 [T, T, 3]): whiten, resize, centre crop, normalise."""
    if u8.shape[2] == 4:
        u8 = whiten(u8)
    new, (x0, y0) = plan((u8.shape[1], u8.shape[0]), target)
    crop = resize_window(u8, new, (x0, y0, x0 + target, y0 + target))
    return (crop / 255.0 * 2 - 1).transpose(2, 0, 1).astype(np.float32), crop
