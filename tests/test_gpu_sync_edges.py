"""The synchronisation kernels (wmar_amd/csrc/sync.hip) where tests/test_gpu_sync.py does not reach: sizes other than 128 / 256 / 512
(odd, no multiple of the wave, two columns per thread with a ragged second one, 4 and 5 pixels), every branch of find_cut, cut
quotients on a half, counts on the threshold, the cuts of all 41 angles, rotations up to 180 degrees, the per-lane atomics of the
positions launch, the Hamming gate, and remove_sync beyond 256 pixels.  Expected values are the REFERENCE's, recorded in
tests/golden/sync_edge_vectors.npz (tests/golden/make_sync_vectors.py); inputs are rebuilt from seeds by tests/sync_cases.py;
tests/test_sync_reference.py keeps a census of the branches these inputs reach.  Everything is compared exactly, and every device
call is made twice and must return the same bytes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sync_cases as SC  # noqa: E402
from tests import sync_reference as SR  # noqa: E402
from tests.conftest import REPO  # noqa: E402

N_ANGLES = 41


@pytest.fixture(scope="module")
def ev():
    return np.load(os.path.join(REPO, "tests", "golden", "sync_edge_vectors.npz"))


@pytest.fixture(scope="module")
def ws():
    from tests.sync_standins import ColourWam
    from wmar_amd.watermarking.synchronization import WamSync
    return WamSync(None, "cuda", wam=ColourWam("cuda"))


def _twice(fn):
    """fn() -> tuple of numpy arrays; run twice, the bytes must not change."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "two identical calls returned different bytes"
    return a


def _fit_raw(maps, images_in_workspace=None):
    """wmar_sync_fit called directly: (aug [B, 4], total [B, 41], err [B, 41], cut [B, 41, 3]); the last two are read from the
    result region at the start of the caller's workspace (include/wmar_hip.h)."""
    from wmar_amd import _lib
    L = _lib.load()
    p = torch.from_numpy(np.stack(maps)).cuda().contiguous()
    B, S = p.shape[0], p.shape[-1]
    image = S * S * 4 * 8
    result = int(L.wmar_sync_workspace_bytes(B, S)) - B * image
    assert result >= B * N_ANGLES * 20
    n = B if images_in_workspace is None else images_in_workspace
    work = torch.zeros(result + n * image, dtype=torch.uint8, device="cuda")
    aug = torch.empty(B, 4, dtype=torch.int32, device="cuda")
    total = torch.empty(B, N_ANGLES, dtype=torch.float64, device="cuda")
    _lib.check(L.wmar_sync_fit(p.data_ptr(), B, S, aug.data_ptr(), total.data_ptr(), work.data_ptr(), work.numel(),
                               _lib.stream_ptr(p.device)))
    torch.cuda.synchronize()
    raw = work[:B * N_ANGLES * 20].cpu().numpy()
    err = raw[:B * N_ANGLES * 8].view(np.float64).reshape(B, N_ANGLES)
    cut = raw[B * N_ANGLES * 8:].view(np.int32).reshape(B, N_ANGLES, 3)
    return aug.cpu().numpy(), total.cpu().numpy(), err.copy(), cut.copy()


def _check_fit(got, ev, S, order, what):
    aug, total, err, cut = got
    names = [n for n, _ in SC.edge_label_cases(S)]
    for row, n in enumerate(order):
        tag = f"{names[n]}@{S}, {what}"
        assert aug[row].tolist() == ev[f"efit{S}_aug"][n].tolist(), tag
        assert np.array_equal(total[row], ev[f"efit{S}_total"][n]), tag
        assert np.array_equal(err[row], ev[f"efit{S}_total"][n]), tag
        bad = np.nonzero((cut[row] != ev[f"efit{S}_cuts"][n]).any(axis=1))[0]
        assert bad.size == 0, f"{tag}: (cut_i, cut_j, flipped) at angle {int(bad[0]) - 20}: {cut[row][bad[0]].tolist()}, " \
                              f"the reference has {ev[f'efit{S}_cuts'][n][bad[0]].tolist()}"


@pytest.mark.parametrize("S", SC.EDGE_FIT_SIZES)
def test_fit_and_cuts_of_every_angle(ev, S):
    maps = [m for _, m in SC.edge_label_cases(S)]
    B = len(maps)
    assert 8 <= B <= 16 and len(ev[f"efit{S}_aug"]) == B
    fwd = list(range(B))
    _check_fit(_twice(lambda: _fit_raw(maps)), ev, S, fwd, "one batched call")
    _check_fit(_twice(lambda: _fit_raw(maps[::-1])), ev, S, fwd[::-1], "reversed order")
    _check_fit(_twice(lambda: _fit_raw(maps, 1)), ev, S, fwd, "chunks of one image")
    n = 3 if B % 3 else 4
    assert B % n != 0
    _check_fit(_twice(lambda: _fit_raw(maps, n)), ev, S, fwd, f"chunks of {n} with a ragged last one")


def test_python_layer_at_ragged_sizes(ev, ws):
    """WamSync's own workspace sizing at a size that is no multiple of anything, against the same recorded tuples."""
    for S in (161, 300):
        p = torch.from_numpy(np.stack([m for _, m in SC.edge_label_cases(S)])).cuda()
        aug, total = _twice(lambda: (ws.fit_best_aug_batch(p).cpu().numpy(), ws.fit_total_error(p).cpu().numpy()))
        assert np.array_equal(aug, ev[f"efit{S}_aug"]) and np.array_equal(total, ev[f"efit{S}_total"]), S


def _border_pixels(S, angle):
    """Pixels whose fp64 source coordinate lies within 1e-9 of 0 or S - 1: the inside test hangs on the last bit there."""
    y, x = SR.source_coordinates(S, angle)
    near = np.zeros((S, S), dtype=bool)
    for v in (y, x):
        near |= (np.abs(v) < 1e-9) | (np.abs(v - (S - 1)) < 1e-9)
    return near


def test_rotated_maps_equal_the_reference(ev, ws):
    cases = SC.edge_rot_cases()
    assert len(cases) == 2 * len(SC.EDGE_ROT_SIZES)
    for S in SC.EDGE_ROT_SIZES:
        group = [c for c in cases if c[1].shape[-1] == S]
        angles = group[0][2]
        skip = {}
        for angle in angles:                            # what may be left out is settled before the device is consulted
            skip[angle] = _border_pixels(S, angle) if abs(angle) > 20 else np.zeros((S, S), dtype=bool)
            assert int(skip[angle].sum()) <= 4 * S, (S, angle)
        p = torch.from_numpy(np.stack([c[1] for c in group])).cuda()
        for k, angle in enumerate(angles):
            got, = _twice(lambda: (ws.rotated_labels(p, angle).cpu().numpy(),))
            for n, (name, _, _) in enumerate(group):
                want = ev[f"erot_{name}"][k]
                bad = int(((got[n] != want) & ~skip[angle]).sum())
                assert bad == 0, f"{name} at {angle} degrees: {bad} pixels differ"


def test_positions_sizes_and_planted_pixels(ev, ws):
    planted = SC.edge_planted()
    for S, batch in SC.edge_pred_cases():
        p = torch.from_numpy(batch).cuda()

        def call(t):
            pos, sizes = ws.positions_from_preds(t)
            return pos.cpu().numpy(), sizes.cpu().numpy()

        pos, sizes = _twice(lambda: call(p))
        assert np.array_equal(pos, ev[f"epos{S}_pos"]), S
        assert np.array_equal(sizes, ev[f"epos{S}_sizes"]), S
        for k in range(3):                              # image by image: the same bytes as in the batch
            one_pos, one_sizes = _twice(lambda: call(p[k:k + 1]))
            assert one_pos.tobytes() == pos[k].tobytes() and one_sizes.tobytes() == sizes[k].tobytes(), (S, k)
            flat = pos[k].reshape(-1)
            for at, (mask, _, what) in zip(SC.edge_planted_at(S, k), planted):
                if what.startswith("msg"):
                    want = -1 if what.endswith("+7") else int(what[3])
                elif what.startswith("mask"):
                    want = 0 if mask in (2e-7, np.inf) else -1
                else:
                    want = 1
                assert int(flat[at]) == want, (S, k, what)


class _NegatedMask:
    """ColourWam with the sign of every mask logit turned: no pixel is kept, the confidence gate fails."""

    def __init__(self, wam):
        self.wam = wam

    def detect(self, imgs):
        preds = self.wam.detect(imgs)["preds"].clone()
        preds[:, 0] = -preds[:, 0]
        return {"preds": preds}


def test_remove_sync_at_512(ev, ws):
    from wmar_amd.augmentations.geometric import HorizontalFlip, Rotate, resize_bilinear
    from wmar_amd.watermarking.synchronization import WamSync
    S = 512
    imgs = torch.from_numpy(SC.e2e_images(S)).cuda()
    want = ev["e2e512_aug"]
    calls = ws.wam.detect_calls

    def run():
        out, info, (pos, sizes) = ws.remove_sync(imgs, return_info=True)
        return out.cpu().numpy(), np.array([[a[0], a[1], a[2], int(a[3])] for a in info], dtype=np.int32), pos.cpu().numpy()

    out, info, pos = run()
    assert ws.wam.detect_calls == calls + 1                                   # one detect over the batch
    again = run()
    assert all(a.tobytes() == b.tobytes() for a, b in zip((out, info, pos), again))
    assert np.array_equal(pos, SC.e2e_positions(S))
    assert info.tolist() == want.tolist()
    x = ws.normalize(imgs)
    for n, a in enumerate(want.tolist()):               # the reference's revert_augmentation, beyond 256: PAD_THRESH 25
        if a[3]:
            expect = HorizontalFlip()(x[n:n + 1])
        elif abs(a[0]) >= 3:
            expect = Rotate()(x[n:n + 1], int(a[0]))
        else:
            pad_i = 2 * a[1] - S
            pad_i = 0 if pad_i < 25 else pad_i
            pad_j = max(0, 2 * a[2] - S)
            pad_j = 0 if pad_j < 25 else pad_j
            expect = x[n:n + 1]
            if pad_i or pad_j:
                expect = resize_bilinear(torch.nn.functional.pad(expect, (0, pad_j, 0, pad_i)), (S, S))
        assert np.array_equal(out[n:n + 1], ws.unnormalize(expect).cpu().numpy()), SC.E2E[n]
    assert want[1][3] == 1 and abs(int(want[2][0])) >= 3 and 2 * int(want[3][1]) - S >= 25      # a flip, a rotation and a padding ran
    # every mask logit negated: only the grey pixels outside the four squares are kept, far fewer than 0.75 of the image, so the
    # gate fails for the flipped, rotated and cropped image alike: the dummy estimate and no revert
    gated = WamSync(None, "cuda", wam=_NegatedMask(ws.wam))
    out, info, (pos, sizes) = gated.remove_sync(imgs, return_info=True)
    assert bool((sizes.sum(dim=1) < round(S * S * 0.75)).all()) and int(sizes.sum()) == int((pos >= 0).sum()) > 0
    assert info == [(0, S // 2, S // 2, False)] * 4
    assert torch.equal(out, ws.unnormalize(x))
