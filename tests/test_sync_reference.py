"""tests/sync_reference.py (numpy + scipy restatement of the synchronisation layer's fit and positions step) against the recorded
outputs of the reference (tests/golden/sync_vectors.npz), and its scipy-free spline rotation -- the arithmetic of
wmar_amd/csrc/sync.hip -- against scipy.ndimage.rotate."""
import os

import numpy as np
import pytest

pytest.importorskip("scipy")

from tests import sync_cases as SC  # noqa: E402
from tests import sync_reference as SR  # noqa: E402
from tests.conftest import REPO  # noqa: E402


@pytest.fixture(scope="module")
def sv():
    return np.load(os.path.join(REPO, "tests", "golden", "sync_vectors.npz"))


def _tuple(aug):
    return [aug[0], aug[1], aug[2], int(aug[3])]


@pytest.mark.parametrize("S", [256, 512, 128])
def test_fit_equals_the_reference(sv, S):
    cases = SC.label_cases(S)
    assert len(cases) == len(sv[f"fit{S}_aug"]) == {256: 15, 512: 3, 128: 1}[S]
    for n, (name, pos) in enumerate(cases):
        aug, total = SR.fit(pos)
        assert _tuple(aug) == sv[f"fit{S}_aug"][n].tolist(), name
        assert np.array_equal(total, sv[f"fit{S}_total"][n]), name


def test_rotated_maps_equal_the_reference(sv):
    cases = dict(SC.label_cases(256))
    for name in SC.ROT_CASES:
        wm = SR.labels_of(cases[name])
        for k, angle in enumerate(SC.ROT_ANGLES):
            assert np.array_equal(SR.rotate_wm(wm, angle), sv[f"rot_{name}"][k]), (name, angle)


def test_fixture_margin_and_documented_results(sv):
    assert float(sv["min_margin"]) > 1e-10
    names = [n for n, _ in SC.label_cases(256)]
    assert sv["fit256_aug"][names.index("all_minus1")].tolist() == [0, 128, 128, 0]
    assert np.all(sv["fit256_total"][names.index("all_minus1")] == 2e9)
    assert sv["fit128_aug"][0].tolist() == [0, 64, 64, 0] and np.all(sv["fit128_total"][0] == 2e9)      # no count reaches THRESH
    assert sv["fit256_aug"][names.index("flip")][3] == 1 and sv["fit256_aug"][names.index("rot-13")][0] == 13


def test_plain_spline_rotation_equals_scipy(sv):
    """The kernels' arithmetic (prefilter once, 16 taps per pixel) gives scipy's interpolated values to rounding, hence -- with the
    fixtures' margin -- the same thresholded maps."""
    from scipy import ndimage
    cases = dict(SC.label_cases(256))
    worst = 0.0
    for name, angles in (("rot+7", (-20, -7, 0, 1, 20)), ("random", (-20, 13))):
        mask = (cases[name] == 1) * 255
        coeffs = SR.spline_coefficients(mask)
        assert np.abs(coeffs - ndimage.spline_filter(mask.astype(np.float64), order=3, mode="constant")).max() < 1e-10
        for angle in angles:
            want = ndimage.rotate(mask.astype(np.float64), angle, reshape=False)
            worst = max(worst, float(np.abs(SR.spline_rotate_values(coeffs, angle) - want).max()))
    assert worst < 1e-10, worst
    wm = SR.labels_of(cases["flip_speckle"])
    for k, angle in enumerate(SC.ROT_ANGLES):
        assert np.array_equal(SR.rotate_wm_plain(wm, angle), sv["rot_flip_speckle"][k]), angle


def test_positions_equal_the_reference(sv):
    for k, (seed, S, angle, fails) in enumerate(SC.PRED_CASES):
        pos, sizes = SR.positions_from_preds(SC.preds(seed, S, angle, fails))
        assert np.array_equal(pos, sv[f"pred{k}_pos"]) and np.array_equal(sizes, sv[f"pred{k}_sizes"]), k
        assert SR.gate_fails(sizes, S) == fails
        aug = [0, S // 2, S // 2, 0] if fails else _tuple(SR.fit(pos)[0])
        assert aug == sv[f"pred{k}_aug"].tolist(), k
    # the planted mask logits: sigmoid(0) = sigmoid(-0) = sigmoid(5e-8) = 0.5 exactly in fp32 (not kept), sigmoid(2e-7) > 0.5
    pos = sv["pred0_pos"]
    for (y, x), v in SC.PLANTED:
        assert pos[y, x] == (0 if v == 2e-7 else -1), (y, x, v)


def test_e2e_tuples_equal_the_reference(sv):
    for n, pos in enumerate(SC.e2e_positions()):
        assert _tuple(SR.fit(pos)[0]) == sv["e2e_aug"][n].tolist(), SC.E2E[n]
