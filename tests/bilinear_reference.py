"""Pillow's 8-bit BILINEAR resample in numpy: tests/lanczos_reference.py with the filter and its support swapped (Pillow's
bilinear_filter: the triangle 1 - |x| on |x| < 1, support 1.0) and nothing else changed -- the stretch by max(in / out, 1), the
left-to-right normalisation, the 22-bit rounding, the two integer passes with the 8-bit rounding in between, the unfiltered unchanged
axis.  What ``wmar_resample_coeffs_filtered(..., WMAR_RESAMPLE_BILINEAR)`` and ``wmar_image_ingest_filtered`` compute, plus torchvision's
``Resize(int)`` / ``RandomCrop.get_params`` arithmetic around it.  tests/test_bilinear_reference.py pins this file to PIL byte for byte."""
import numpy as np

from tests import lanczos_reference as R

PRECISION_BITS = R.PRECISION_BITS
SUPPORT = 1.0

# the shapes (width x height -> target) the device ingest is held to, at windows touching every edge
SHAPES = [((37, 53), 32), ((500, 375), 256), ((640, 427), 512), ((31, 17), 32), ((1024, 700), 256), ((256, 300), 256), ((97, 97), 128),
          ((33, 200), 32)]


def bilinear(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(x < 1.0, 1.0 - x, 0.0)


def coeffs(in_size, out_size, out0=0, n_out=None):
    """(xmin int32 [n], count int32 [n], k int32 [n, ksize], ksize) for the outputs [out0, out0 + n_out) of one axis."""
    n_out = out_size - out0 if n_out is None else n_out
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out0, out0 + n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = bilinear((x + xmin[:, None] - center[:, None] + 0.5) * (1.0 / filterscale))
    w = np.where(x < count[:, None], w, 0.0)
    ww = R._seq_sum(w)
    k = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    ki = np.where(k < 0, -0.5 + k * (1 << PRECISION_BITS), 0.5 + k * (1 << PRECISION_BITS)).astype(np.int32)
    return xmin.astype(np.int32), count.astype(np.int32), ki, ksize


def resize_window(u8, new_size, box):
    """The pixels [x0, x1) x [y0, y1) of PIL's ``Image.fromarray(u8).resize(new_size, BILINEAR)`` for uint8 [H, W, C]."""
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
        img = R._pass(img, xmin, xcount, xk, 1)
    else:
        img = img[:, x0:x1]
    if nh != H:
        img = R._pass(img, ymin - r0, ycount, yk, 0)
    return np.ascontiguousarray(img)


def resize(u8, new_size):
    return resize_window(u8, new_size, (0, 0, new_size[0], new_size[1]))


def resize_plan(size, target):
    """(new_width, new_height) of torchvision's Resize(target) for a (width, height) image: short side -> target, long side ->
    int(target * long / short)."""
    w, h = size
    if w <= h:
        return target, int(target * h / w)
    return int(target * w / h), target


def windows(new, target):
    """Crop origins (x0, y0) of target x target windows touching every edge of a (width, height) image, plus an inner one."""
    mx, my = new[0] - target, new[1] - target
    return sorted({(0, 0), (mx, 0), (0, my), (mx, my), (mx // 2, my // 3)})


def image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
