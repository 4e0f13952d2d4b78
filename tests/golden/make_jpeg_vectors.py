"""Generate tests/golden/jpeg_vectors.npz: uint8 RGB images and what PIL's JPEG encoder + decoder return for them.

Usage (build machine; the GPU box never runs this):
    python tests/golden/make_jpeg_vectors.py

Inputs (seeded): noise, a smooth gradient with noise, and an image of only 0 and 255 (exercises the decoder's range limits), at
64 x 64 and 48 x 80, each at the 11 qualities of the AugmentationManager table and at q = 1, 50, 100; one 256 x 256 smooth image at a
few qualities.  Keys: `<name>_in` [3, H, W], `<name>_q<q>` [3, H, W] (planar: the tensor layout, and it compresses better);
`qualities_<name>`; `pil_version`, `libjpeg_turbo_version`."""
import io
import os

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_QUALITIES = [100, 95, 85, 75, 65, 55, 45, 35, 25, 15, 5]


def pil_roundtrip(rgb, q):
    with io.BytesIO() as buf:
        Image.fromarray(rgb).save(buf, format="JPEG", quality=q)
        buf.seek(0)
        return np.asarray(Image.open(buf).convert("RGB"))


def images(rng, h, w, noise=2.0):
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    smooth = np.stack([200 * xx + 30, 180 * yy + 40, 120 * (xx + yy) + 10], -1) + rng.normal(0, noise, (h, w, 3))
    return {
        "noise": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
        "smooth": np.clip(smooth, 0, 255).astype(np.uint8),
        "binary": (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8),
    }


def main():
    rng = np.random.default_rng(2024)
    out = {"pil_version": np.array(PIL.__version__), "libjpeg_turbo_version": np.array(str(features.version("libjpeg_turbo")))}
    cases = []
    for h, w in ((64, 64), (48, 80)):
        for name, img in images(rng, h, w).items():
            cases.append((f"{name}_{h}x{w}", img, TABLE_QUALITIES + [1, 50]))
    cases.append(("smooth_256x256", images(rng, 256, 256, noise=0.5)["smooth"], [75, 10]))     # little noise: the file stays small
    for key, img, qs in cases:
        out[f"{key}_in"] = img.transpose(2, 0, 1)
        out[f"qualities_{key}"] = np.array(qs, dtype=np.int32)
        for q in qs:
            out[f"{key}_q{q}"] = pil_roundtrip(img, q).transpose(2, 0, 1)
    path = os.path.join(HERE, "jpeg_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
