"""CPU checks of the BILINEAR ingest filter: tests/bilinear_reference.py against PIL byte for byte (full images and windows);
``wmar_resample_coeffs_filtered`` against the numpy tables entry for entry, and with LANCZOS against ``wmar_resample_coeffs``; the
Resize(int) / RandomCrop arithmetic of wmar_amd.utils.ingest.  Exact everywhere: no tolerances."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

from tests import bilinear_reference as BL
from tests import lanczos_reference as R

LANCZOS, BILINEAR = 1, 2


@pytest.mark.parametrize("wh,T", BL.SHAPES)
def test_numpy_restatement_equals_pil(wh, T):
    w, h = wh
    a = BL.image(w, h, w * 1000 + h)
    new = BL.resize_plan(wh, T)
    ref = np.array(Image.fromarray(a).resize(new, Image.BILINEAR))
    assert ref.shape[:2] == (new[1], new[0])
    assert np.array_equal(BL.resize(a, new), ref)
    for x0, y0 in BL.windows(new, T):
        assert np.array_equal(BL.resize_window(a, new, (x0, y0, x0 + T, y0 + T)), ref[y0:y0 + T, x0:x0 + T]), (x0, y0)


def _c_coeffs(in_size, out_size, out0, n_out, filt, ksize):
    from wmar_amd import _lib
    L = _lib.load()
    xmin, cnt, k = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros(n_out * ksize, np.int32)
    ks = C.c_int32(0)
    rc = L.wmar_resample_coeffs_filtered(in_size, out_size, out0, n_out, xmin.ctypes.data, cnt.ctypes.data, k.ctypes.data, n_out * ksize,
                                         C.byref(ks), filt)
    return rc, xmin, cnt, k.reshape(n_out, ksize), ks.value


CASES = [(100, 237, 0, 237), (237, 100, 0, 100), (4000, 683, 0, 683), (4000, 683, 85, 512), (1, 64, 0, 64), (3000, 512, 0, 512),
         (375, 256, 0, 256), (17, 32, 0, 32), (200, 193, 161, 32), (2, 3, 0, 3)]


@pytest.mark.parametrize("case", CASES)
def test_filtered_coeffs_equal_the_numpy_tables(case):
    in_size, out_size, out0, n_out = case
    rx, rc_, rk, rks = BL.coeffs(in_size, out_size, out0, n_out)
    rc, xmin, cnt, k, ksize = _c_coeffs(*case, BILINEAR, rks)
    assert rc == 0 and ksize == rks
    assert np.array_equal(xmin, rx) and np.array_equal(cnt, rc_) and np.array_equal(k, rk)
    assert cnt.min() >= 1


@pytest.mark.parametrize("case", CASES)
def test_filtered_coeffs_with_lanczos_are_the_existing_entry(case):
    from wmar_amd import _lib
    in_size, out_size, out0, n_out = case
    _, _, _, ksize = R.coeffs(in_size, out_size, out0, 1)
    rc, xmin, cnt, k, ks = _c_coeffs(*case, LANCZOS, ksize)
    xmin0, cnt0, k0 = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros(n_out * ksize, np.int32)
    ks0 = C.c_int32(0)
    rc0 = _lib.load().wmar_resample_coeffs(in_size, out_size, out0, n_out, xmin0.ctypes.data, cnt0.ctypes.data, k0.ctypes.data, n_out * ksize,
                                           C.byref(ks0))
    assert rc == 0 and rc0 == 0 and ks == ks0.value == ksize
    assert np.array_equal(xmin, xmin0) and np.array_equal(cnt, cnt0) and np.array_equal(k.reshape(-1), k0)
    rx, rc_, rk, _ = R.coeffs(in_size, out_size, out0, n_out)
    assert np.array_equal(xmin, rx) and np.array_equal(cnt, rc_) and np.array_equal(k, rk)


def test_filtered_coeffs_refuse_an_unknown_filter():
    from wmar_amd import _lib
    for filt in (0, 3, 5, -1):
        rc = _c_coeffs(100, 50, 0, 50, filt, 16)[0]
        assert rc == -1
        with pytest.raises(_lib.WmarError, match="filter"):
            _lib.check(rc)


def test_resize_and_random_crop_plans():
    from wmar_amd.utils.ingest import random_crop_origin, resize_plan
    assert resize_plan((500, 375), 256) == (341, 256) and resize_plan((375, 500), 256) == (256, 341)
    assert resize_plan((33, 200), 32) == (32, 193) and resize_plan((97, 97), 128) == (128, 128)
    assert resize_plan((640, 427), 512) == (int(512 * 640 / 427), 512)
    for wh, T in BL.SHAPES:
        assert resize_plan(wh, T) == BL.resize_plan(wh, T)
    # the draws: none for an exact fit, else top then left from the one generator
    g, ref = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    assert random_crop_origin((32, 32), 32, g) == (0, 0)
    assert torch.equal(g.get_state(), ref.get_state())
    x0, y0 = random_crop_origin((341, 256), 256, g)
    i = int(torch.randint(0, 256 - 256 + 1, size=(1,), generator=ref))
    j = int(torch.randint(0, 341 - 256 + 1, size=(1,), generator=ref))
    assert (x0, y0) == (j, i) and torch.equal(g.get_state(), ref.get_state())
    x0, y0 = random_crop_origin((32, 193), 32, g)
    i = int(torch.randint(0, 193 - 32 + 1, size=(1,), generator=ref))
    j = int(torch.randint(0, 1, size=(1,), generator=ref))
    assert (x0, y0) == (j, i) and 0 <= y0 <= 161
