"""Inputs the WAM embedder tests and tests/golden/make_wam_vectors.py share: seeded images, messages, and the constructed images
of the JND tests.  numpy only; nothing here is stored in the fixture."""
import numpy as np

SMALL_SEED, RELEASED_SEED = 11, 12        # synth_wam_state seeds of the two recorded networks
SMALL_B = 3
LA_MARGIN = 1e-3                          # pixels whose fp64 la (the 5 x 5 stencil / 32) lies this close to the switch at 127 are left out
LA_CAP = 1e-4                             # ... at most this share of an image

# WamSync.wm_msgs (wmar/watermarking/synchronization.py:33-40)
SYNC_MSGS = np.array([[0] * 32, [0] * 16 + [1] * 16, [1] * 16 + [0] * 16, [1] * 32], dtype=np.int32)


def images01(seed, B, R):
    """float32 [B, 3, R, R] in [0, 1]: a 16 x 16 PCG64 field upsampled (nearest) to R x R plus noise of sigma 0.03, clipped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    coarse = rng.random((B, 3, 16, 16))
    assert R % 16 == 0
    up = np.repeat(np.repeat(coarse, R // 16, axis=2), R // 16, axis=3)
    return np.clip(up + 0.03 * rng.standard_normal((B, 3, R, R)), 0.0, 1.0).astype(np.float32)


def images_pm1(seed, B, R):
    """The same images in [-1, 1] (float32, x * 2 - 1 in float32: what add_sync is handed)."""
    return (images01(seed, B, R) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


def messages(seed, B, nbits=32):
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    return rng.integers(0, 2, size=(B, nbits)).astype(np.int32)


def jnd_cases(R=32):
    """{name: float32 [3, R, R] in [0, 1]}: flat 0 and 1, a flat level either side of la = 127 (the luminance of a flat grey v is
    255 v and the stencil weights add up to 32, so la = 255 v inside the image), a vertical and a horizontal step, an impulse in each
    corner (the zero padding of the border)."""
    out = {"flat0": np.zeros((3, R, R), np.float32), "flat1": np.ones((3, R, R), np.float32)}
    out["below127"] = np.full((3, R, R), 126.0 / 255.0, np.float32)
    out["above127"] = np.full((3, R, R), 128.0 / 255.0, np.float32)
    v = np.full((3, R, R), 0.2, np.float32)
    v[:, :, R // 2:] = 0.8
    out["vstep"] = v
    h = np.full((3, R, R), 0.7, np.float32)
    h[:, R // 2:, :] = 0.1
    out["hstep"] = h
    for name, (y, x) in {"tl": (0, 0), "tr": (0, R - 1), "bl": (R - 1, 0), "br": (R - 1, R - 1)}.items():
        c = np.full((3, R, R), 0.25, np.float32)
        c[:, y, x] = (1.0, 0.5, 0.0)
        out["impulse_" + name] = c
    return out
