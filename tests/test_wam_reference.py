"""CPU: the float64 restatement of the WAM embedder (tests/wam_reference.py) against the arrays the reference's own modules produced in
float64 (tests/golden/wam_vectors*.npz, written by tests/golden/make_wam_vectors.py), the JND on constructed images, and the new
symbols of the C ABI.

Tolerance of the float64 comparison, from the operation count: a path through the embedder crosses at most 80 convolutions, norms and
attention products; the longest sum has 9 * 128 = 1152 products (a 3 x 3 convolution over 128 channels; the released attention adds
1024); activations stay below 2^4.  Every sum carries at most n * 2^-53 relative rounding whatever its order, so two correct float64
evaluations differ by less than 80 * 1152 * 2^-53 * 2^4 = 1.6e-10.  A wrong tap, pad, group or constant shows at 1e-3 and above.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import wam_cases as WC
from tests import wam_reference as WR
from wmar_amd.utils import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL64 = 80 * 1152 * 2.0 ** -53 * 2.0 ** 4


@functools.lru_cache(maxsize=None)
def gold(name):
    return dict(np.load(os.path.join(GOLD, name)))


@functools.lru_cache(maxsize=None)
def small_restated():
    s = WR.state64(synth.synth_wam_state(synth.WAM_SMALL, WC.SMALL_SEED))
    u = torch.from_numpy(WC.images01(WC.SMALL_SEED, WC.SMALL_B, 64)).double()
    x = WR.normalize(u)
    out = WR.embed(s, x, WC.messages(WC.SMALL_SEED, WC.SMALL_B))
    out["heat"] = WR.jnd_heat(WR.unnormalize(x))[:, 0]
    out["sync"] = WR.add_sync(s, torch.from_numpy(WC.images_pm1(WC.SMALL_SEED, WC.SMALL_B, 64)).double(), WC.SYNC_MSGS, WR.grid_masks(64))
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("mine,theirs", [("latents", "s_latents64"), ("decoder_input", "s_zin64"), ("preds_w", "s_preds64"),
                                         ("imgs_w", "s_imgs_w64"), ("heat", "s_heat64")])
def test_small_embed_matches_reference_float64(mine, theirs):
    a, b = small_restated()[mine], gold("wam_vectors.npz")[theirs]
    assert a.shape == b.shape and b.dtype == np.float64
    d = np.abs(a - b).max()
    print(f"WAMREF {mine}: max |restatement - reference float64| = {d:.3g} (bound {TOL64:.3g})")
    assert d <= TOL64


def test_small_add_sync_matches_reference_float64():
    a, b = small_restated()["sync"], gold("wam_vectors_f32.npz")["s_sync64"]
    assert a.shape == b.shape and b.dtype == np.float64
    assert np.abs(a - b).max() <= TOL64
    # the grid leaves a cross free: there the image comes back (through normalise / unnormalise), elsewhere it is changed
    x = WC.images_pm1(WC.SMALL_SEED, WC.SMALL_B, 64).astype(np.float64)
    free = WR.grid_masks(64).sum(dim=0)[0].numpy() == 0
    assert free.any() and (~free).any()
    assert np.abs(a - x)[:, :, free].max() < 1e-6 and np.abs(a - x)[:, :, ~free].max() > 1e-3


def test_released_add_sync_matches_reference_float64_subset():
    cfg = synth.WAM_RELEASED
    s = WR.state64(synth.synth_wam_state(cfg, WC.RELEASED_SEED))
    x = torch.from_numpy(WC.images_pm1(WC.RELEASED_SEED, 1, 256)).double()
    a = WR.add_sync(s, x, WC.SYNC_MSGS, WR.grid_masks(256)).numpy()
    g = gold("wam_vectors_released.npz")
    assert np.abs(a[:, :, ::4, ::4] - g["r_sync64_sub"]).max() <= TOL64
    # and the reference's own float32 run lies where its recorded error says
    d = np.abs(g["r_sync32"].astype(np.float64) - a)
    assert abs(d.max() - g["r_sync_err"][0]) <= TOL64 and abs(np.sqrt(np.mean(d * d)) - g["r_sync_err"][1]) <= TOL64


def test_fixture_holds_outputs_only_and_the_la_cap():
    for name in ("wam_vectors.npz", "wam_vectors_f32.npz", "wam_vectors_released.npz"):
        assert os.path.getsize(os.path.join(GOLD, name)) < (1 << 20)
        for k, v in gold(name).items():
            assert v.dtype in (np.float32, np.float64, np.int64), (name, k)
    ex = gold("wam_vectors_released.npz")["la_excluded"]
    assert ex[0] <= WC.LA_CAP * WC.SMALL_B * 64 * 64 and ex[1] <= WC.LA_CAP * 256 * 256


# ---- the JND on constructed images: closed forms
def _heat(img):
    return WR.jnd_heat(torch.from_numpy(img).double()[None])[0, 0].numpy()


def la_curve(la):
    return 17.0 * (1.0 - np.sqrt(la / 127.0 + 1e-5)) if la <= 127.0 else 3.0 / 128.0 * (la - 127.0) + 3.0


def test_jnd_flat_images():
    cases = WC.jnd_cases(32)
    lum_w = sum(WR.RGB)      # the three weights do not add up to exactly 1 in fp32
    for name, level in (("flat0", 0.0), ("flat1", 1.0), ("below127", 126.0 / 255.0), ("above127", 128.0 / 255.0)):
        h = _heat(cases[name])
        v = float(np.float32(level)) * 255.0 * lum_w
        # inside the image no gradient, la = the luminance (the 5 x 5 weights add up to 32): heat = curve(la) / 255
        assert np.allclose(h[2:-2, 2:-2], la_curve(v) / 255.0, rtol=0, atol=1e-15), name
    # the two branches either side of the switch: about 17 (1 - sqrt(126 / 127)) = 0.067 below, 3 + 3 / 128 above
    assert _heat(cases["below127"])[16, 16] * 255 < 0.1 and _heat(cases["above127"])[16, 16] * 255 > 3.0
    # flat 0: la = 17 (1 - sqrt(1e-5)) everywhere, the border included (zero padding of zeros)
    assert np.allclose(_heat(cases["flat0"]), 17.0 * (1.0 - np.sqrt(1e-5)) / 255.0, atol=1e-15)


def test_jnd_zero_padding_at_the_border():
    h = _heat(WC.jnd_cases(32)["flat1"])
    lum = 255.0 * sum(WR.RGB)
    # corner pixel: the 5 x 5 stencil keeps rows / columns 0..2 -> weights (0 + 2 + 1) + (2 + 2 + 1) + (1 + 1 + 1) = 11
    la = la_curve(lum * 11.0 / 32.0)
    # Sobel at the corner with zeros outside: gx = (0 + 2) lum + lum = 3 lum (right column weights 2 and 1), gy = -(2 + 1) lum
    g = np.sqrt(2.0) * 3.0 * lum
    cm = 0.117 * 16.0 * g ** 2.4 / (g ** 2 + 676.0)
    want = max(la + cm - 0.3 * min(la, cm), 0.0) / 255.0
    for y, x in ((0, 0), (0, 31), (31, 0), (31, 31)):
        assert abs(h[y, x] - want) < 1e-14


def test_jnd_steps_and_impulses():
    cases = WC.jnd_cases(32)
    v, hstep = _heat(cases["vstep"]), _heat(cases["hstep"])
    # a vertical step raises the heat in the two columns next to it and nowhere further inside; transposing the image transposes it
    assert v[16, 15] > 4 * v[16, 8] and v[16, 16] > 4 * v[16, 24]
    assert np.allclose(_heat(np.ascontiguousarray(cases["vstep"].transpose(0, 2, 1))), v.T, rtol=0, atol=1e-15)
    assert hstep[15, 16] > 4 * hstep[8, 16]
    base = _heat(np.full((3, 32, 32), 0.25, np.float32))
    for name, (y, x) in {"tl": (0, 0), "tr": (0, 31), "bl": (31, 0), "br": (31, 31)}.items():
        d = np.abs(_heat(cases["impulse_" + name]) - base)
        ys, xs = np.nonzero(d > 1e-12)
        # the impulse reaches the 5 x 5 neighbourhood that lies inside the image, and nothing else
        assert abs(ys - y).max() <= 2 and abs(xs - x).max() <= 2 and len(ys) >= 8, name
    # the four corners are mirror images of each other
    tl = _heat(cases["impulse_tl"])
    assert np.allclose(tl[:, ::-1], _heat(cases["impulse_tr"]), atol=1e-15) and np.allclose(tl[::-1, :], _heat(cases["impulse_bl"]), atol=1e-15)


def test_message_rows_are_table_sums():
    s = WR.state64(synth.synth_wam_state(synth.WAM_SMALL, WC.SMALL_SEED))
    E = s["msg_processor.msg_embeddings.weight"].numpy()
    m = WC.messages(3, 2)
    rows = WR.message_rows(s, m).numpy()
    for b in range(2):
        assert np.allclose(rows[b], sum(E[2 * j + m[b, j]] for j in range(32)), atol=1e-13)


def test_synth_state_is_the_released_embedder():
    s = synth.synth_wam_state(synth.WAM_RELEASED, 0)
    assert sum(v.numel() for v in s.values()) == 1105639
    assert s["decoder.conv_in.weight"].shape == (64, 68, 3, 3) and s["encoder.conv_out.weight"].shape == (4, 64, 3, 3)
    assert synth.WAM_SMALL.latent_size == 8 and synth.WAM_SMALL.ch == synth.WAM_RELEASED.ch
    from wmar_amd.watermarking.wam_embedder import config_from_state
    assert config_from_state(s) == synth.WAM_RELEASED


# ---- the C ABI
def test_new_symbols_declared_listed_and_exported():
    from wmar_amd import _lib
    names = ["wmar_wam_create", "wmar_wam_destroy", "wmar_wam_device_bytes", "wmar_wam_embed", "wmar_wam_add_sync", "wmar_wam_probe_jnd",
             "wmar_wam_probe_latent_msg", "wmar_wam_probe_tail"]
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "wmar_hip.h")).read()
    for n in names:
        assert n in _lib.SYMBOLS, n
        assert re.search(r"\b%s\(" % n, header), n
    assert "wmar_wam_config" in header and hasattr(_lib, "WamConfig")
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
