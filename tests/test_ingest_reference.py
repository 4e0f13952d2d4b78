"""CPU checks of the image ingest: tests/lanczos_reference.py (the steps the device kernels run) against PIL byte for byte; the
whitening table over all 65 536 (alpha, colour) pairs; wmar_resample_coeffs against the numpy tables entry for entry;
wmar_amd.utils.ingest on a CPU device against the PIL path; the round / // plan.  Exact everywhere: no tolerances."""
import base64
import ctypes as C
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import ingest_cases as K
from tests import lanczos_reference as R


def test_case_list():
    assert len(K.CASES) == 47 and len(set(K.CASES)) == 47
    assert [R.plan(wh, T)[0] for T, wh in K.STRIPS] == [(512, 153600), (153600, 512)]


@pytest.mark.parametrize("T", K.TARGETS)
def test_numpy_restatement_equals_pil(T):
    for w, h in K.shapes_for(T):
        new, (x0, y0) = R.plan((w, h), T)
        for name in K.PATTERNS:
            a = K.pattern(name, w, h)
            ref = np.array(Image.fromarray(a).resize(new, Image.LANCZOS))
            assert np.array_equal(R.resize(a, new), ref), (T, w, h, name)
            f, u8 = R.ingest(a, T)
            assert np.array_equal(u8, ref[y0:y0 + T, x0:x0 + T]), (T, w, h, name)
            assert torch.equal(torch.from_numpy(f), K.pil_path(Image.fromarray(a), T)[0]), (T, w, h, name)


@pytest.mark.parametrize("T,wh", K.STRIPS)
def test_window_of_a_153600_pixel_axis_equals_pil(T, wh):
    for name in K.PATTERNS:
        a = K.pattern(name, *wh)
        f, u8 = R.ingest(a, T)
        ref_f, ref_u8 = K.pil_path(Image.fromarray(a), T)
        assert np.array_equal(u8, ref_u8) and torch.equal(torch.from_numpy(f), ref_f), (wh, name)


def test_whitening_all_pairs():
    a, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.stack([c, c, c, a], axis=2)                                   # [256 alpha, 256 colour, 4]
    alpha = rgba[:, :, 3] / 255.0
    expect = ((1 - alpha[:, :, np.newaxis]) * 255 + alpha[:, :, np.newaxis] * rgba[:, :, :3]).astype("uint8")
    assert np.array_equal(R.whiten(rgba), expect)
    from wmar_amd.utils.ingest import whiten
    assert np.array_equal(whiten(rgba), expect)
    assert np.array_equal(np.array(K.whiten_transparency(Image.fromarray(rgba, "RGBA"))), expect)
    # an RGBA image through the whole reference path
    rng = np.random.default_rng(5)
    img = Image.fromarray(rng.integers(0, 256, (90, 130, 4), dtype=np.uint8), "RGBA")
    f, u8 = R.ingest(np.array(img), 64)
    ref_f, ref_u8 = K.pil_path(img, 64)
    assert np.array_equal(u8, ref_u8) and torch.equal(torch.from_numpy(f), ref_f)


def _c_coeffs(in_size, out_size, out0, n_out, capacity=None):
    from wmar_amd import _lib
    L = _lib.load()
    _, _, _, ksize = R.coeffs(in_size, out_size, out0, 1)
    cap = n_out * ksize if capacity is None else capacity
    xmin, cnt, k = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros(max(cap, 1), np.int32)
    ks = C.c_int32(0)
    rc = L.wmar_resample_coeffs(in_size, out_size, out0, n_out, xmin.ctypes.data, cnt.ctypes.data, k.ctypes.data, cap, C.byref(ks))
    return rc, xmin, cnt, k, ks.value


@pytest.mark.parametrize("case", [(100, 237, 0, 237), (237, 100, 0, 100), (4000, 683, 0, 683), (4000, 683, 85, 512), (1, 64, 0, 64),
                                  (300, 153600, 76544, 512), (3000, 512, 0, 512), (512, 512, 0, 512)])
def test_resample_coeffs_equal_the_numpy_tables(case):
    in_size, out_size, out0, n_out = case
    rc, xmin, cnt, k, ksize = _c_coeffs(*case)
    assert rc == 0
    rx, rc_, rk, rks = R.coeffs(in_size, out_size, out0, n_out)
    assert ksize == rks
    assert np.array_equal(xmin, rx) and np.array_equal(cnt, rc_)
    assert np.array_equal(k.reshape(n_out, ksize), rk)


def test_resample_coeffs_rejects_bad_arguments():
    from wmar_amd import _lib
    for bad in ((4000, 683, 0, 683, 683 * 37 - 1), (0, 64, 0, 64, None), (64, 0, 0, 1, None), (-3, 64, 0, 64, None),
                (100, 50, 40, 20, None), (100, 50, -1, 5, None)):
        rc = _c_coeffs(*bad[:4], capacity=bad[4])[0] if bad[0] > 0 and bad[1] > 0 else _lib.load().wmar_resample_coeffs(
            bad[0], bad[1], bad[2], bad[3], None, None, None, 0, None)
        assert rc == -1, bad
        with pytest.raises(_lib.WmarError):
            _lib.check(rc)


def _mode_images():
    rng = np.random.default_rng(11)
    rgb = Image.fromarray(rng.integers(0, 256, (70, 101, 3), dtype=np.uint8))
    rgba = Image.fromarray(rng.integers(0, 256, (83, 64, 4), dtype=np.uint8), "RGBA")
    opaque = np.array(rgba)
    opaque[:, :, 3] = 255
    pal = rgb.convert("P", palette=Image.ADAPTIVE, colors=17)
    palt = pal.copy()
    palt.info["transparency"] = 3
    return {"RGB": rgb, "RGBA": rgba, "RGBA_opaque": Image.fromarray(opaque, "RGBA"), "L": rgb.convert("L"), "P": pal,
            "P_transparent": palt, "LA": rgba.convert("LA")}


@pytest.mark.parametrize("T", [32, 64])
def test_cpu_ingest_equals_the_pil_path(T, tmp_path):
    from wmar_amd.utils.ingest import ingest, open_image
    imgs = _mode_images()
    got, u8 = ingest(list(imgs.values()), T, "cpu", return_u8=True)
    assert got.shape == (len(imgs), 3, T, T) and got.dtype == torch.float32
    for i, (name, img) in enumerate(imgs.items()):
        ref_f, ref_u8 = K.pil_path(img, T)
        assert torch.equal(got[i], ref_f) and np.array_equal(u8[i].numpy(), ref_u8), name
    # the ways in: path, file:, data:, array
    p = tmp_path / "a.png"
    imgs["RGBA"].save(p)
    buf = io.BytesIO()
    imgs["RGBA"].save(buf, format="PNG")
    data = "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()
    same = ingest([str(p), "file:" + str(p), data, np.array(imgs["RGBA"]), p], T, "cpu")
    for i in range(5):
        assert torch.equal(same[i], got[1]), i
    arrays = ingest([np.array(imgs[k]) for k in ("RGB", "RGBA", "RGBA_opaque")] + [np.array(imgs["L"])[:, :, None]], T, "cpu")
    for i, k in enumerate(("RGB", "RGBA", "RGBA_opaque", "L")):
        assert torch.equal(arrays[i], got[list(imgs).index(k)]), k
    with pytest.raises(ValueError):
        open_image(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        open_image(3.5)


def test_plan_rounds_half_to_even():
    from wmar_amd.utils.ingest import plan
    # scale * side exactly half way: 3 x 2 -> T = 1 gives 1.5 -> 2; 5 x 2 -> 2.5 -> 2; 2 x 7 at T = 1 gives 3.5 -> 4
    assert plan((3, 2), 1) == ((2, 1), (0, 0))
    assert plan((5, 2), 1) == ((2, 1), (0, 0))
    assert plan((2, 7), 1) == ((1, 4), (0, 1))
    assert plan((2, 9), 1) == ((1, 4), (0, 1))           # 4.5 -> 4
    assert plan((4, 6), 2) == ((2, 3), (0, 0))
    assert plan((4000, 3000), 512) == ((683, 512), (85, 0))
    assert plan((1, 300), 512) == ((512, 153600), (0, 76544))
    for size in [(3, 2), (5, 2), (2, 7), (2, 9), (1920, 1080), (1, 1), (7, 300)]:
        for T in (1, 2, 64, 512):
            assert plan(size, T) == K.plan(size, T) == R.plan(size, T)
            new, (x0, y0) = plan(size, T)
            assert 0 <= x0 and x0 + T <= new[0] and 0 <= y0 and y0 + T <= new[1]
