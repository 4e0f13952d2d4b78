"""CPU-side checks of the synchronisation layer: flags, ABI bookkeeping, manager dispatch, the grid masks and SyncSeal's plumbing."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests.conftest import REPO

SYNC_SYMBOLS = ["wmar_sync_positions", "wmar_sync_workspace_bytes", "wmar_sync_fit", "wmar_sync_rotate_labels"]


def _args(*argv):
    import detect
    import generate
    return generate.get_parser().parse_args(list(argv)), detect.get_parser().parse_args(list(argv))


def test_parsers_accept_sync_flags():
    import generate
    g, d = _args("--sync", "true", "--sync_factory", "pkg.mod:make", "--syncpath", "checkpoints/wam_mit.pth")
    for a in (g, d):
        assert a.sync is True and a.sync_factory == "pkg.mod:make" and a.syncpath == "checkpoints/wam_mit.pth"
        generate.check_wm_args(a)
    g, _ = _args()
    assert g.sync is False and g.sync_factory is None
    generate.check_wm_args(g)
    for bad in (["--sync_factory", "pkg.mod:make"], ["--sync", "true", "--sync_factory", "nocolon"], ["--sync", "true"]):
        with pytest.raises(ValueError, match="sync"):
            generate.check_wm_args(generate.get_parser().parse_args(bad))


def test_sync_factory_builds_the_manager(tmp_path, monkeypatch):
    from wmar_amd import cli
    from wmar_amd.watermarking.synchronization import SyncManager, WamSync
    (tmp_path / "my_sync_factory.py").write_text(
        "from tests.sync_standins import ColourWam\n"
        "class M:\n    def add_sync(self, x, return_masks=False):\n        return x + 1\n"
        "    def remove_sync(self, x, return_info=False):\n        return x - 1\n"
        "def wam(args, device):\n    return ColourWam(device)\n"
        "def manager(args, device):\n    return M()\n"
        "def junk(args, device):\n    return object()\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    g, _ = _args("--sync", "true", "--sync_factory", "my_sync_factory:wam")
    m = cli.build_sync_manager(g, "cpu")
    assert isinstance(m, SyncManager) and isinstance(m.sync, WamSync) and type(m.sync.wam).__name__ == "ColourWam"
    g, _ = _args("--sync", "true", "--sync_factory", "my_sync_factory:manager")
    m = cli.build_sync_manager(g, "cpu")
    assert torch.equal(m.remove_sync(m.add_sync(torch.zeros(2))), torch.zeros(2)) and set(m.last_seconds) == {"add_sync", "remove_sync"}
    g, _ = _args("--sync", "true", "--sync_factory", "my_sync_factory:junk")
    with pytest.raises(TypeError, match="embed / detect"):
        cli.build_sync_manager(g, "cpu")
    assert cli.build_sync_manager(_args()[0], "cpu") is None


def test_sync_symbols_declared_listed_and_exported():
    from wmar_amd import _lib
    header = open(os.path.join(REPO, "include", "wmar_hip.h")).read()
    L = _lib.load()
    for s in SYNC_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _lib.SYMBOLS and hasattr(L, s), s
    assert L.wmar_sync_workspace_bytes(1, 256) >= 256 * 256 * 4 * 8 + 41 * 20
    assert L.wmar_sync_workspace_bytes(64, 256) - L.wmar_sync_workspace_bytes(63, 256) in range(2 << 20, (2 << 20) + 1280)
    assert L.wmar_sync_workspace_bytes(0, 256) == 0
    from wmar_amd import build
    assert ("sync.hip", ["-ffp-contract=off"]) in build.SOURCES


def test_fit_refuses_bad_arguments_before_any_launch():
    from wmar_amd import _lib
    L = _lib.load()
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data
    assert L.wmar_sync_fit(p, 1, 1024, p, None, p, 1 << 40, None) != 0 and b"4..512" in L.wmar_last_error()
    assert L.wmar_sync_fit(p, 1, 256, p, None, p, 4096, None) != 0 and b"workspace" in L.wmar_last_error()
    assert L.wmar_sync_rotate_labels(p, 1, 256, 0, p, None, 0, None) != 0
    from wmar_amd.watermarking.synchronization import WamSync
    ws = WamSync(None, "cpu", wam=object())
    with pytest.raises(RuntimeError, match="no host fallback"):
        ws.fit_best_aug(np.zeros((256, 256), dtype=np.int8))
    with pytest.raises(ValueError, match="square"):
        ws.fit_best_aug_batch(np.zeros((1, 8, 16), dtype=np.int8))
    with pytest.raises(RuntimeError, match="no host fallback"):
        ws.positions_from_preds(torch.zeros(1, 33, 8, 8))


def test_manager_dispatches_on_the_file_name(monkeypatch):
    from wmar_amd.watermarking import synchronization as S
    made = []
    monkeypatch.setattr(S, "WamSync", lambda path, device: made.append(("wam", path)) or "W")
    monkeypatch.setattr(S, "SyncSeal", lambda path, device: made.append(("seal", path)) or "S")
    assert S.SyncManager("checkpoints/wam_mit.pth", "cpu").sync == "W"
    assert S.SyncManager("checkpoints/syncmodel.jit.pt", "cpu").sync == "S"
    assert made == [("wam", "checkpoints/wam_mit.pth"), ("seal", "checkpoints/syncmodel.jit.pt")]
    with pytest.raises(NotImplementedError, match="Unknown wam model other.pth"):
        S.SyncManager("other.pth", "cpu")
    assert S.SyncManager("other.pth", "cpu", sync="ready").sync == "ready"


def test_missing_wam_checkout_says_where_it_looked(monkeypatch):
    from wmar_amd.watermarking.synchronization import WamSync
    monkeypatch.setitem(sys.modules, "deps", None)          # whatever the checkout has: the import fails here
    with pytest.raises(ImportError) as e:
        WamSync("checkpoints/wam_mit.pth", "cpu")
    msg = str(e.value)
    assert "deps.watermark_anything.utils.inference_utils" in msg and "load_model_from_checkpoint" in msg
    assert os.getcwd() in msg and "wam=" in msg


def test_grid_masks_and_normalisation_equal_the_reference():
    from wmar_amd.watermarking.synchronization import WamSync
    sv = np.load(os.path.join(REPO, "tests", "golden", "sync_vectors.npz"))
    ws = WamSync(None, "cpu", wam=object())
    for S in (256, 512):
        m = ws.create_grid_mask(torch.zeros(3, S, S), 4)
        assert m.shape == (4, 1, S, S) and np.array_equal(m[:, 0].numpy().astype(np.uint8), sv[f"grid{S}"]), S
    x = torch.rand(2, 3, 8, 8) * 2 - 1
    n = ws.normalize(x)
    assert torch.allclose(n[:, 1], ((x[:, 1] + 1) / 2 - 0.456) / 0.224, atol=1e-6)
    assert torch.allclose(ws.unnormalize(n), x, atol=1e-6) and float(ws.unnormalize(n * 10).abs().max()) <= 1.0


def test_syncseal_round_trips_through_torchscript(tmp_path):
    from tests.sync_standins import TinySeal
    from wmar_amd.watermarking.synchronization import SyncManager
    path = str(tmp_path / "syncmodel.jit.pt")
    torch.jit.script(TinySeal()).save(path)
    m = SyncManager(path, "cpu")
    x = torch.rand(2, 3, 16, 16) * 2 - 1
    y = m.add_sync(x)
    assert torch.allclose(y, (((x + 1) / 2) * 0.5 + 0.125) * 2 - 1, atol=1e-6)
    assert torch.allclose(m.remove_sync(y), x, atol=1e-6)
    with pytest.raises(AssertionError):
        m.add_sync(x, return_masks=True)
