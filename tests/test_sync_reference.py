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


# ---- the edge fixtures (tests/golden/sync_edge_vectors.npz) and the census of what they reach ----------------------------------
@pytest.fixture(scope="module")
def ev():
    return np.load(os.path.join(REPO, "tests", "golden", "sync_edge_vectors.npz"))


@pytest.fixture(scope="module")
def edge_fits():
    """{(S, name): (aug, total, cuts, branches seen)} of every edge label case on the scipy path, computed once for the tests below."""
    out = {}
    for S in SC.EDGE_FIT_SIZES:
        for name, pos in SC.edge_label_cases(S):
            seen = set()
            out[S, name] = SR.fit_detail(pos, seen=seen) + (seen,)
    return out


def _assert_edge_fit(ev, S, n, name, got):
    aug, total, cuts = got[:3]
    assert _tuple(aug) == ev[f"efit{S}_aug"][n].tolist(), (S, name)
    assert np.array_equal(total, ev[f"efit{S}_total"][n]), (S, name)
    assert np.array_equal(cuts, ev[f"efit{S}_cuts"][n]), (S, name)


def test_edge_fit_equals_the_reference(ev, edge_fits):
    assert float(ev["min_margin"]) > 1e-10
    for S in SC.EDGE_FIT_SIZES:
        cases = SC.edge_label_cases(S)
        assert len(cases) == len(ev[f"efit{S}_aug"]) == {190: 9, 257: 9}.get(S, 8)
        for n, (name, _) in enumerate(cases):
            _assert_edge_fit(ev, S, n, name, edge_fits[S, name])
        if S in (96, 129):                              # the ragged sizes whose fit is trivial: no count reaches 80
            trivial = [n for n, (name, _) in enumerate(cases) if name != "rot-13_speckle"]
            assert np.all(ev[f"efit{S}_total"][trivial] == 2e9) and np.all(ev[f"efit{S}_cuts"][trivial] == [S // 2, S // 2, 0])


def test_edge_fit_on_the_plain_spline_path(ev):
    """The kernels' arithmetic instead of scipy's, at the sizes where it can go wrong alone: an odd size, a size with two columns
    per thread, and the two halves that were searched for."""
    for S, names in ((161, ("flip", "rot-13_speckle", "flip_left_half")), (190, ("rot+7.5",)), (257, ("half_even",)),
                     (300, ("rot+7",)), (96, ("identity",)), (129, ("rot-13_speckle",))):
        cases = SC.edge_label_cases(S)
        for n, (name, pos) in enumerate(cases):
            if name in names:
                _assert_edge_fit(ev, S, n, name, SR.fit_detail(pos, rotate=SR.PlainRotator()))


def test_edge_rotated_maps_equal_the_reference(ev):
    """Both paths, every recorded angle.  Beyond +-20 degrees the pixels whose source coordinate lies within 1e-9 of the border are
    left to the last bit of whoever computes it (at most 4 S of them)."""
    for name, pos, angles in SC.edge_rot_cases():
        S, wm, plain = pos.shape[-1], SR.labels_of(pos), SR.PlainRotator()
        assert ev[f"erot_{name}"].shape == (len(angles), S, S)
        for k, angle in enumerate(angles):
            want = ev[f"erot_{name}"][k]
            if S != 300 or angle in (0, 20):
                assert np.array_equal(SR.rotate_wm(wm, angle), want), (name, angle)
            skip = np.zeros((S, S), dtype=bool)
            if abs(angle) > 20:
                y, x = SR.source_coordinates(S, angle)
                for v in (y, x):
                    skip |= (np.abs(v) < 1e-9) | (np.abs(v - (S - 1)) < 1e-9)
                assert int(skip.sum()) <= 4 * S
            assert not np.any((plain(wm, angle) != want) & ~skip), (name, angle)


def test_edge_positions_equal_the_reference(ev):
    planted = SC.edge_planted()
    assert len(planted) == 12 + 4 + 7
    for S, batch in SC.edge_pred_cases():
        assert batch.shape == (3, 33, S, S) and ((S * S) % 64 != 0) == (S != 64)
        for k in range(3):
            pos, sizes = SR.positions_from_preds(batch[k])
            assert np.array_equal(pos, ev[f"epos{S}_pos"][k]) and np.array_equal(sizes, ev[f"epos{S}_sizes"][k]), (S, k)
            at = SC.edge_planted_at(S, k)
            assert len(set(at)) == len(planted)
            got = {what: int(pos.reshape(-1)[a]) for a, (_, _, what) in zip(at, planted)}
            for msg in range(4):                        # the Hamming gate: 6 differing bits are kept, 7 are not
                assert [got[f"msg{msg}+{f}"] for f in (5, 6, 7)] == [msg, msg, -1]
            assert [v for w, v in got.items() if w.startswith(("zero", "one"))] == [1, 1, 1, 1]
            assert [v for w, v in got.items() if w.startswith("mask")] == [-1, -1, -1, 0, 0, -1, -1]


def test_edge_e2e_512_tuples(sv, ev):
    """remove_sync beyond 256 pixels: the flipped and the cropped map are label_cases(512) entries, held above (27 s a fit)."""
    pos, cases = SC.e2e_positions(512), dict(SC.label_cases(512))
    assert np.array_equal(pos[1], cases["flip"]) and np.array_equal(pos[3], cases["crop0.7"])
    assert ev["e2e512_aug"][1].tolist() == sv["fit512_aug"][0].tolist() and ev["e2e512_aug"][3].tolist() == sv["fit512_aug"][2].tolist()
    assert ev["e2e512_aug"].tolist() == [[0, 255, 255, 0], [0, 255, 254, 1], [-10, 255, 255, 0], [0, 363, 367, 0]]
    assert _tuple(SR.fit(pos[2])[0]) == ev["e2e512_aug"][2].tolist()


CENSUS = (
    "only_L_normal_curve", "only_L_flipped_curve", "only_R_normal_curve", "only_R_flipped_curve",      # one side empty
    "both_normal_curve", "both_flipped_curve", "no_weight",
    "half_cut_floor_even", "half_cut_floor_odd",        # only the even floor separates half-to-even from half-up
    "votes_zero_dim0",
    "column_count_on_thresh", "row_count_on_thresh", "column_count_below_thresh", "row_count_below_thresh",
    "several_best_angles", "one_best_angle",
    "half_rotation",                                    # round((max + min) / 2) on a half
)


def test_edge_census(edge_fits):
    """What the union of the edge cases reaches on the host restatement, so that a change of seeds or layouts cannot silently empty
    the coverage of tests/test_gpu_sync_edges.py.  Measured: the shared fixture (50 fits, scipy path) takes 33 s on one core, the other edge tests of this file
    22 s together."""
    seen = set().union(*(v[3] for v in edge_fits.values()))
    missing = [item for item in CENSUS if item not in seen]
    assert not missing, missing
    # the pinned cases do what they were chosen for
    assert "half_cut_floor_even" in edge_fits[257, "half_even"][3] and edge_fits[257, "half_even"][0][1] == 128
    assert "half_rotation" in edge_fits[190, "rot+7.5"][3] and edge_fits[190, "rot+7.5"][0][0] == -8       # round(-7.5), not -7
    assert {"only_L_flipped_curve", "only_R_flipped_curve"} <= edge_fits[161, "flip"][3]
