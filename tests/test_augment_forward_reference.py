"""The forward references of tests/augment_forward_reference.py, without a GPU:

  * the references agree with one another: the float64 rotation map with the `_rotate_ref` loop and with `rotate_nearest` in fp32, the
    resize weights with torch's float64 `interpolate(bilinear, antialias=True)` within 1e-12, the blur with `_blur_ref`;
  * the caps on what a rotation test may leave out hold on the float64 map alone (the counts below were measured on it);
  * the float32 models of the kernels pass every gate that tests/test_gpu_augment_forward.py applies to the kernels;
  * every planted error (augment_forward_reference.FAULTS) fails at least one case of those gates, so the gates can see a subtle fault."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import augment_forward_reference as R
from tests.test_augmentations_algorithms import _blur_ref, _rotate_ref
from wmar_amd.augmentations.geometric import rotate_nearest


# ------------------------------------------------------------------------------------------------------ the references agree
@pytest.mark.parametrize("H,W", [(16, 16), (17, 17), (12, 20), (20, 12)])
def test_float64_map_agrees_with_the_rotate_ref_loop(H, W):
    x = R.saturated_image(H, W, False)
    for angle in R.SWEEP_ANGLES + (30, 45, 90, 180, 185, 200, 270):
        q, rest = divmod(angle, 90)
        got = _rotate_ref(x, angle)
        R.check_rotation(got, x, R.F32(0), H, W, q % 4, rest)


@pytest.mark.parametrize("H,W", [(16, 16), (17, 17), (12, 20), (20, 12), (50, 50), (64, 64), (33, 47), (96, 96), (256, 256)])
def test_float64_map_agrees_with_rotate_nearest_in_fp32(H, W):
    idx = torch.arange(1, H * W + 1, dtype=torch.float32).view(1, 1, H, W)
    for rest in R.SWEEP_RESTS + (1, 30, 45, 89):
        R.check_rotation(rotate_nearest(idx, rest).numpy(), idx.numpy(), R.F32(0), H, W, 0, rest)


@pytest.mark.parametrize("n_in,n_out", sorted({(c[2], c[0]) for c in R.RESIZE_CASES + R.RESIZE_EXACT} | {(c[3], c[1]) for c in R.RESIZE_CASES}))
def test_resize_weights_equal_torchs_float64_interpolate(n_in, n_out):
    Wm = R.aa_weights(n_in, n_out)
    eye = torch.eye(n_in, dtype=torch.float64).view(1, 1, n_in, n_in)          # resized along the rows only: the weight matrix itself
    ref = TF.interpolate(eye, size=(n_out, n_in), mode="bilinear", antialias=True, align_corners=False)[0, 0].numpy()
    assert np.abs(Wm - ref).max() <= 1e-12
    assert np.abs(Wm.sum(1) - 1).max() <= 1e-12
    assert np.abs(R.resize_weights32(n_in, n_out).astype(np.float64) - Wm).max() <= 64 * R.EPS     # the model restates the same filter


def test_resize_and_blur_references_agree_with_each_other():
    for H, W, nh, nw in R.RESIZE_CASES + R.RESIZE_EXACT:
        u = torch.from_numpy(R.stencil_input(H, W, "plain", False)).double()
        ref = TF.interpolate(u[..., :nh, :nw], size=(H, W), mode="bilinear", antialias=True, align_corners=False).numpy()
        assert np.abs(R.resize64(u.numpy(), nh, nw) - ref).max() <= 1e-12, (H, W, nh, nw)
    for H, W, k in R.BLUR_CASES + R.BLUR_EXACT:
        u = R.stencil_input(H, W, "wide", False).astype(np.float64)
        assert np.abs(np.clip(R.blur64(u, k), 0, 1) - _blur_ref(u, k)).max() <= 1e-12, (H, W, k)
        w32 = R.blur_weights32(k).astype(np.float64)
        assert np.abs(w32 - R.blur_weights64(k)).max() <= 8 * R.EPS, k


# ------------------------------------------------------------------------------------------------------ the caps, on the reference alone
def test_undecidable_counts_of_the_float64_map():
    for H, W in R.SMALL_SHAPES:
        for rest in R.SWEEP_RESTS:
            for q in range(4) if H == W else (0, 2):
                assert R.undecidable_count(H, W, q, rest) == 0, (H, W, q, rest)
    per_rest = {rest: R.undecidable_count(96, 96, 0, rest) for rest in R.SWEEP_RESTS}
    assert per_rest == {5: 0, 10: 4, 15: 0, 20: 0, 70: 0, 75: 0, 80: 4, 85: 0}, per_rest
    for S in (256, 512):
        for rest in R.SWEEP_RESTS:
            assert R.undecidable_count(S, S, 0, rest) <= R.LARGE_CAP * S * S, (S, rest)
    for case, n in R.ROTATION_TIES.items():
        assert R.undecidable_count(*case) == n, (case, R.undecidable_count(*case))
    for case in R.ROTATION_CASES:
        R.assert_cap(*case)


# ------------------------------------------------------------------------------------------------------ the models pass every gate
def _model_run(fault=None):
    return lambda op, x, p0, p1, noise, pm1: R.model(op, x, p0, p1, noise, pm1, fault)


def _rotation_gates(run):
    for case in R.ROTATION_CASES:
        yield lambda case=case: R.gate_rotation(run, *case)


def _blur_gates(run):
    for H, W, k in R.BLUR_EXACT:
        yield lambda H=H, W=W, k=k: R.gate_exact_stencil(run, R.BLUR, H, W, k, 0)
    for H, W, k in sorted(R.BLUR_CASES, key=lambda c: c[2]):
        yield lambda H=H, W=W, k=k: R.gate_stencil(run, R.BLUR, H, W, k, 0)


def _resize_gates(run):
    for H, W, nh, nw in R.RESIZE_EXACT:
        yield lambda H=H, W=W, nh=nh, nw=nw: R.gate_exact_stencil(run, R.CROP_RESIZE, H, W, nh, nw)
    for H, W, nh, nw in R.RESIZE_CASES:
        yield lambda H=H, W=W, nh=nh, nw=nw: R.gate_stencil(run, R.CROP_RESIZE, H, W, nh, nw)


def _pointwise_gates(run):
    for H, W in ((16, 16), (7, 37), (5, 1)):
        yield lambda H=H, W=W: R.gate_pointwise(run, H, W)


FAMILIES = {"rotation": _rotation_gates, "blur": _blur_gates, "resize": _resize_gates, "pointwise": _pointwise_gates}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_unmodified_models_pass_every_gate(family):
    for gate in FAMILIES[family](_model_run()):
        gate()


def _families_of(fault):
    op = R.FAULTS[fault]
    return {R.BLUR: ["blur"], R.ROTATE: ["rotation"], R.CROP_RESIZE: ["resize"], None: ["pointwise", "rotation", "blur", "resize"]}[op]


@pytest.mark.parametrize("fault", sorted(R.FAULTS))
def test_each_planted_error_fails_at_least_one_case(fault):
    failed = 0
    for family in _families_of(fault):
        for gate in FAMILIES[family](_model_run(fault)):
            try:
                gate()
            except AssertionError:
                failed += 1
                break
        if failed:
            break
    assert failed, f"no gate sees the planted error {fault}: the case list is too weak"


def test_the_rotation_errors_show_on_the_map_itself():
    """each rotation fault moves DECIDABLE pixels of the index image, i.e. it is the map that is held, not a fraction of it"""
    for fault in ("rot-centre", "rot-border", "rot-quarters", "rot-sign", "plane-stride"):
        seen = False
        for H, W, q, rest in R.ROTATION_CASES:
            idx = R.index_image(H, W)
            try:
                R.check_rotation(R.model(R.ROTATE, idx, q, rest, fault=fault), idx, R.F32(0), H, W, q, rest)
            except AssertionError:
                seen = True
                break
        assert seen, fault
