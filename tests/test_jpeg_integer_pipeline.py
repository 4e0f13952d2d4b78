"""The specification the device JPEG (wmar_amd/csrc/jpeg.hip) is written against, pinned on the CPU: the integer restatement of
libjpeg-turbo's baseline path in tests/jpeg_reference.py equals PIL's encoder + decoder bit for bit -- on the committed fixture
(tests/golden/jpeg_vectors.npz, made by tests/golden/make_jpeg_vectors.py), on live PIL for random images of several sizes, and
through the float entry / exit steps of the JPEG module (x * 255 truncated to uint8, u / 255 in fp32, the straight-through form)."""
import os

import numpy as np
import pytest
import torch

from jpeg_reference import STD_CHROMINANCE, STD_LUMINANCE, pil_roundtrip, quant_tables, range_limit, roundtrip

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_QUALITIES = [100, 95, 85, 75, 65, 55, 45, 35, 25, 15, 5]


@pytest.fixture(scope="module")
def vectors():
    return np.load(os.path.join(HERE, "golden", "jpeg_vectors.npz"))


def _cases(v):
    for key in sorted(k[len("qualities_"):] for k in v.files if k.startswith("qualities_")):
        yield key, v[f"{key}_in"].transpose(1, 2, 0), [int(q) for q in v[f"qualities_{key}"]]


def test_fixture_covers_what_it_claims(vectors):
    keys = [k for k, _, _ in _cases(vectors)]
    assert {"noise_64x64", "smooth_48x80", "binary_64x64", "smooth_256x256"} <= set(keys)
    for key, img, qs in _cases(vectors):
        if key != "smooth_256x256":
            assert set(TABLE_QUALITIES + [1, 50, 100]) <= set(qs), key
    assert str(vectors["pil_version"]) and str(vectors["libjpeg_turbo_version"])


def test_restatement_equals_the_fixture(vectors):
    for key, img, qs in _cases(vectors):
        for q in qs:
            ref = vectors[f"{key}_q{q}"].transpose(1, 2, 0)
            got = roundtrip(img, q)
            assert np.array_equal(got, ref), (key, q, int((got != ref).sum()))


def test_restatement_equals_live_pil_on_the_fixture_inputs(vectors):
    for key, img, qs in _cases(vectors):
        for q in qs[::3]:
            assert np.array_equal(roundtrip(img, q), pil_roundtrip(img, q)), (key, q)


@pytest.mark.parametrize("hw", [(16, 16), (32, 48), (112, 64), (128, 144)])
def test_restatement_equals_live_pil_on_random_images(hw):
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    h, w = hw
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            np.clip(np.stack([xx * 3, yy * 2, xx + yy], -1) + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8),
            np.where(rng.random((h, w, 3)) < 0.5, 0, 255).astype(np.uint8)]
    for img in imgs:
        for q in (1, 2, 10, 33, 49, 50, 51, 77, 90, 99, 100):
            assert np.array_equal(roundtrip(img, q), pil_roundtrip(img, q)), (hw, q)


def test_tables_and_range_limit():
    assert all(np.array_equal(t, b) for t, b in zip(quant_tables(50), (STD_LUMINANCE, STD_CHROMINANCE)))
    assert all((t == 1).all() for t in quant_tables(100))
    assert (quant_tables(1)[1] == 255).all()
    v = np.arange(-1024, 2048)
    r = range_limit(v)
    assert r.min() == 0 and r.max() == 255
    assert np.array_equal(range_limit(np.arange(-128, 128)), np.arange(0, 256))      # in range: sample + 128


@pytest.mark.parametrize("passthrough", [True, False])
def test_module_float_steps_on_the_restatement(passthrough):
    """JPEG()(x, q) on a CPU tensor (PIL) = the restatement between u = (uint8)(clamp(x) * 255) and c = u / 255 (fp32), with
    x + (c - x) evaluated in fp32 for the straight-through form: the exact float contract of the device kernel"""
    from wmar_amd.augmentations.valuemetric import JPEG
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 3, 32, 48, generator=g) * 1.2 - 0.1)
    x[0, :, :4] = torch.tensor([1.0, 0.0, 254.99998 / 255, 3.0 / 255]).view(1, 4, 1)      # saturated and just-below-an-integer values
    for q in (5, 50, 95):
        got = JPEG(passthrough=passthrough)(x, q)
        xc = x.clamp(0, 1)
        u = (xc * 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
        c = torch.from_numpy(np.stack([roundtrip(one, q) for one in u]).astype(np.float32) / np.float32(255)).permute(0, 3, 1, 2)
        ref = (xc + (c - xc)).clamp(0, 1) if passthrough else c
        assert torch.equal(got, ref), q
