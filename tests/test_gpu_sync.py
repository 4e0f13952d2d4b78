"""The synchronisation layer on the device (wmar_amd/csrc/sync.hip, wmar_amd/watermarking/synchronization.py) against the outputs
of the REFERENCE's WamSync recorded in tests/golden/sync_vectors.npz (tests/golden/make_sync_vectors.py); inputs are rebuilt from
seeds by tests/sync_cases.py.  Everything is compared exactly: the fixtures keep every interpolated value 1e-10 away from the
threshold, far more than a different summation order can move it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sync_cases as SC  # noqa: E402
from tests.conftest import REPO  # noqa: E402


@pytest.fixture(scope="module")
def sv():
    return np.load(os.path.join(REPO, "tests", "golden", "sync_vectors.npz"))


@pytest.fixture(scope="module")
def ws():
    from tests.sync_standins import ColourWam
    from wmar_amd.watermarking.synchronization import WamSync
    return WamSync(None, "cuda", wam=ColourWam("cuda"))


def _fit(ws, maps):
    p = torch.from_numpy(np.stack(maps)).cuda()
    return ws.fit_best_aug_batch(p).cpu().numpy(), ws.fit_total_error(p).cpu().numpy()


def test_fit_equals_the_reference(sv, ws):
    maps = [m for _, m in SC.label_cases(256)]
    assert len(maps) == 15
    aug, total = _fit(ws, maps)                         # all 256-pixel cases in one batched call
    assert np.array_equal(aug, sv["fit256_aug"]), (aug.tolist(), sv["fit256_aug"].tolist())
    assert np.array_equal(total, sv["fit256_total"])
    aug, total = _fit(ws, maps[::-1])                   # rows must not depend on their neighbours
    assert np.array_equal(aug[::-1], sv["fit256_aug"]) and np.array_equal(total[::-1], sv["fit256_total"])
    for S in (512, 128):
        aug, total = _fit(ws, [m for _, m in SC.label_cases(S)])
        assert np.array_equal(aug, sv[f"fit{S}_aug"]), (S, aug.tolist())
        assert np.array_equal(total, sv[f"fit{S}_total"]), S
    assert ws.fit_best_aug(maps[1]) == (0, 127, 127, True)          # the reference's single-map form and types


def test_fit_in_chunks_equals_one_pass(sv, ws, monkeypatch):
    """A workspace that holds 2 of 5 images walks the batch in three chunks; same results."""
    from wmar_amd.watermarking import synchronization as sync
    maps = [m for _, m in SC.label_cases(256)][2:7]
    monkeypatch.setattr(sync, "WORKSPACE_CAP", 2 * 256 * 256 * 32 + 8192)
    aug, total = _fit(ws, maps)
    assert np.array_equal(aug, sv["fit256_aug"][2:7]) and np.array_equal(total, sv["fit256_total"][2:7])


def test_rotated_maps_equal_the_reference(sv, ws):
    cases = dict(SC.label_cases(256))
    p = torch.from_numpy(np.stack([cases[n] for n in SC.ROT_CASES])).cuda()
    for k, angle in enumerate(SC.ROT_ANGLES):
        got = ws.rotated_labels(p, angle).cpu().numpy()
        for n, name in enumerate(SC.ROT_CASES):
            bad = int((got[n] != sv[f"rot_{name}"][k]).sum())
            assert bad == 0, f"{name} at {angle} degrees: {bad} pixels differ"


def test_positions_and_sizes_equal_the_reference(sv, ws):
    p = torch.from_numpy(np.stack([SC.preds(*c) for c in SC.PRED_CASES[:3]])).cuda()
    pos, sizes = ws.positions_from_preds(p)
    for k in range(3):
        assert np.array_equal(pos[k].cpu().numpy(), sv[f"pred{k}_pos"]), k
        assert np.array_equal(sizes[k].cpu().numpy(), sv[f"pred{k}_sizes"]), k
    for (y, x), v in SC.PLANTED:                        # fp32 sigmoid(5e-8) is 0.5: not kept; sigmoid(2e-7) is above
        assert int(pos[0, y, x]) == (0 if v == 2e-7 else -1), (y, x, v)
    aug, _ = ws.estimate_augmentation_with_wam(torch.empty(3, 3, 256, 256, device="cuda"), p)
    assert np.array_equal(aug.cpu().numpy(), np.stack([sv[f"pred{k}_aug"] for k in range(3)]))
    seed, S, angle, fails = SC.PRED_CASES[3]            # 128 pixels, fails the confidence gate: the dummy estimate
    p = torch.from_numpy(SC.preds(seed, S, angle, fails))[None].cuda()
    aug, (pos, sizes) = ws.estimate_augmentation_with_wam(torch.empty(1, 3, S, S, device="cuda"), p)
    assert np.array_equal(pos[0].cpu().numpy(), sv["pred3_pos"]) and np.array_equal(sizes[0].cpu().numpy(), sv["pred3_sizes"])
    assert aug[0].tolist() == sv["pred3_aug"].tolist() == [0, 64, 64, 0]


def test_remove_sync_end_to_end(sv, ws):
    from wmar_amd.augmentations.geometric import HorizontalFlip, Rotate, resize_bilinear
    imgs = torch.from_numpy(SC.e2e_images()).cuda()
    calls = ws.wam.detect_calls
    out, info, (pos, sizes) = ws.remove_sync(imgs, return_info=True)
    assert ws.wam.detect_calls == calls + 1                                   # one detect over the batch
    assert np.array_equal(pos.cpu().numpy(), SC.e2e_positions())
    want = sv["e2e_aug"]
    assert [[a[0], a[1], a[2], int(a[3])] for a in info] == want.tolist() == [[0, 127, 127, 0], [0, 127, 127, 1], [-10, 127, 127, 0],
                                                                              [0, 181, 183, 0]]
    x = ws.normalize(imgs)
    pad_i, pad_j = 2 * int(want[3][1]) - 256, 2 * int(want[3][2]) - 256
    expect = [x[0:1], HorizontalFlip()(x[1:2]), Rotate()(x[2:3], int(want[2][0])),
              resize_bilinear(torch.nn.functional.pad(x[3:4], (0, pad_j, 0, pad_i)), (256, 256))]
    for n in range(4):
        assert torch.equal(out[n:n + 1], ws.unnormalize(expect[n])), SC.E2E[n]
    # the flip brings the layout back exactly: the reverted image fits to "nothing to do"
    assert ws.remove_sync(out[1:2], return_info=True)[1] == [(0, 127, 127, False)]
    with pytest.raises(ValueError, match="square"):
        ws.remove_sync(torch.zeros(1, 3, 64, 32, device="cuda"))


def _harness_model():
    from wmar_amd.models.taming_wrapper import TamingARMMWrapper
    from wmar_amd.utils import synth
    gcfg, vcfg = synth.GPTConfig(**synth.HARNESS_GPT), synth.VQConfig(**synth.HARNESS_VQ)
    return TamingARMMWrapper(None, gpt_cfg=gcfg, vq_cfg=vcfg, gpt_state=synth.synth_gpt_state(gcfg, seed=21, logit_scale=40.0),
                             vq_state=synth.synth_vq_state(vcfg, seed=21), max_batch=4)


def test_harness_fills_the_fourth_slot(ws, tmp_path):
    from wmar_amd import harness
    from wmar_amd.augmentations.geometric import HorizontalFlip
    from wmar_amd.watermarking.synchronization import SyncManager
    m = _harness_model()
    codes = torch.from_numpy(np.random.RandomState(5).randint(0, 16384, size=(3, 64))).cuda()
    flip = HorizontalFlip()
    ev = {"metric_names": ["l0"], "augmentations": [("flip-h", flip, [0, 1])], "max_roundtrips": 1, "orig_only": False}

    # without a manager: the launches of the parent commit's code path, restated here, bit for bit
    log = {"batch": [1, 1, 9]}
    harness.fill_batch_log(log, "k", m, codes, ev, sync_manager=None)
    imgs = m.codes_to_images(codes)
    rt_codes = m.images_to_codes(imgs)
    assert np.array_equal(log["k"]["roundtrips"][0][2], imgs.cpu().numpy()) and log["k"]["roundtrips"][0][3] is None
    assert np.array_equal(log["k"]["roundtrips"][1][1], rt_codes.cpu().numpy())
    assert np.array_equal(log["k"]["roundtrips"][1][2], m.codes_to_images(rt_codes).cpu().numpy())
    flipped = (flip(imgs / 2.0 + 0.5).clamp(0, 1) * 2.0 - 1.0)
    assert np.array_equal(log["k"]["flip-h"][1][2], flipped.cpu().numpy())
    assert np.array_equal(log["k"]["flip-h"][1][1], m.images_to_codes(flipped).cpu().numpy())
    assert all(t[3] is None for k in ("roundtrips", "flip-h") for t in log["k"][k])

    # with one: the signal is added after the first decode, removed in front of every re-encode
    mgr = SyncManager(None, "cuda", sync=ws)
    slog = {"batch": [1, 1, 9]}
    harness.fill_batch_log(slog, "k", m, codes, ev, sync_manager=mgr)
    synced = ws.add_sync(imgs)
    assert np.array_equal(slog["k"]["roundtrips"][0][2], synced.cpu().numpy()) and slog["k"]["roundtrips"][0][3] is None
    assert not torch.equal(synced, imgs)
    for name in ("roundtrips", "flip-h"):
        for param, c, im, nosync in slog["k"][name][(1 if name == "roundtrips" else 0):]:
            assert nosync is not None and nosync.shape == im.shape, (name, param)
            assert np.array_equal(c, m.images_to_codes(torch.from_numpy(nosync).cuda()).cpu().numpy()), (name, param)
    assert np.array_equal(slog["k"]["roundtrips"][1][3], ws.remove_sync(synced).cpu().numpy())
    harness.compute_metrics_and_save_from_batch_log(slog, str(tmp_path), None, ev, cond_indices=[1, 2, 1])
    files = sorted(f for _, _, fs in os.walk(tmp_path) for f in fs)
    assert sum(f.endswith("_nosync.png") for f in files) == 3 * 3 and "0001_k_flip-h_1_nosync.png" in files
