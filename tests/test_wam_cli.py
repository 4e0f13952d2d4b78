"""CPU: ``--sync_embedder`` at the parsers, its routing in ``build_sync_manager``, and the ``embedder=`` argument of ``WamSync``."""
import os
import sys
import types

import pytest
import torch


def _args(*argv):
    import detect
    import generate
    return generate.get_parser().parse_args(list(argv)), detect.get_parser().parse_args(list(argv))


def test_sync_embedder_defaults_to_torch_and_native_needs_a_wam_checkpoint():
    import generate
    for a in _args():
        assert a.sync_embedder == "torch"
        generate.check_wm_args(a)
    for a in _args("--sync", "true", "--syncpath", "checkpoints/wam_mit.pth", "--sync_embedder", "native"):
        assert a.sync_embedder == "native"
        generate.check_wm_args(a)
    for a in _args("--sync", "true", "--syncpath", "checkpoints/syncmodel.jit.pt", "--sync_embedder", "native"):
        with pytest.raises(ValueError, match="SyncSeal has no native embedder"):
            generate.check_wm_args(a)
    with pytest.raises(ValueError, match="only read with --sync true"):
        generate.check_wm_args(_args("--sync_embedder", "native", "--syncpath", "checkpoints/wam_mit.pth")[0])
    with pytest.raises(SystemExit):
        _args("--sync_embedder", "triton")


def test_native_with_a_syncseal_path_stops_at_the_parser(monkeypatch, capsys):
    import generate
    monkeypatch.setattr(sys, "argv", ["generate.py", "--outdir", "unused", "--model", "taming", "--sync", "true", "--syncpath",
                                      "checkpoints/syncmodel.jit.pt", "--sync_embedder", "native"])
    with pytest.raises(SystemExit) as e:
        generate.main()
    assert e.value.code == 2 and "SyncSeal has no native embedder" in capsys.readouterr().err
    assert not os.path.exists("unused")


def test_build_sync_manager_routes_native(tmp_path, monkeypatch):
    from wmar_amd import cli
    from wmar_amd.watermarking import synchronization as S
    made = []

    class Spy:
        def __init__(self, syncpath, device, wam=None, embedder=None):
            made.append((syncpath, device, wam, embedder))

        def add_sync(self, imgs, return_masks=False):
            return imgs

        def remove_sync(self, imgs, return_info=False):
            return imgs

    monkeypatch.setattr(S, "WamSync", Spy)
    g, _ = _args("--sync", "true", "--syncpath", "checkpoints/wam_mit.pth", "--sync_embedder", "native")
    m = cli.build_sync_manager(g, "cpu")
    assert isinstance(m, S.SyncManager) and isinstance(m.sync, Spy)
    assert made == [("checkpoints/wam_mit.pth", "cpu", None, "native")]
    # with a factory that returns a WAM-like object: the same, with wam= that object
    (tmp_path / "my_wam_factory.py").write_text(
        "class W:\n    def embed(self, imgs, msg):\n        raise AssertionError('the native embedder embeds')\n"
        "    def detect(self, imgs):\n        return {}\n"
        "def wam(args, device):\n    return W()\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    del made[:]
    g, _ = _args("--sync", "true", "--syncpath", "checkpoints/wam_mit.pth", "--sync_embedder", "native", "--sync_factory", "my_wam_factory:wam")
    m = cli.build_sync_manager(g, "cpu")
    assert len(made) == 1 and type(made[0][2]).__name__ == "W" and made[0][3] == "native"
    # and without the flag the two-argument call of before
    del made[:]
    monkeypatch.setattr(S, "WamSync", lambda path, device: made.append((path, device)) or "W")
    g, _ = _args("--sync", "true", "--syncpath", "checkpoints/wam_mit.pth")
    assert cli.build_sync_manager(g, "cpu").sync == "W" and made == [("checkpoints/wam_mit.pth", "cpu")]


class FakeEmbedder:
    cfg = types.SimpleNamespace(resolution=16)
    device = "cpu"

    def __init__(self):
        self.calls = []

    def add_sync(self, imgs, msgs, masks):
        self.calls.append((tuple(imgs.shape), tuple(msgs.shape), tuple(masks.shape)))
        return imgs * 0.5


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the PyTorch network was touched ({name})")


def test_embedder_takes_add_sync_and_the_network_is_not_touched():
    from wmar_amd.watermarking.synchronization import WamSync
    fake = FakeEmbedder()
    ws = WamSync(None, "cpu", wam=Untouchable(), embedder=fake)
    x = torch.rand(2, 3, 16, 16) * 2 - 1
    out, masks = ws.add_sync(x, return_masks=True)
    assert torch.equal(out, x * 0.5) and masks.shape == (4, 1, 16, 16)
    assert fake.calls == [((2, 3, 16, 16), (4, 32), (4, 1, 16, 16))]
    ws = WamSync(None, "cpu", wam=object(), embedder=fake)
    assert torch.equal(ws.add_sync(x), x * 0.5) and len(fake.calls) == 2


def test_other_sizes_keep_the_torch_path_and_a_missing_checkout_raises_there(monkeypatch):
    from wmar_amd.watermarking.synchronization import WamSync
    from tests.sync_standins import ColourWam
    fake = FakeEmbedder()
    ws = WamSync(None, "cpu", wam=ColourWam("cpu"), embedder=fake)
    out = ws.add_sync(torch.zeros(1, 3, 32, 32))           # not the embedder's 16 x 16: today's loop over wam.embed
    assert out.shape == (1, 3, 32, 32) and fake.calls == []
    monkeypatch.setitem(sys.modules, "deps", None)
    ws = WamSync("checkpoints/wam_mit.pth", "cpu", embedder=fake)      # no ImportError at construction ...
    assert ws.add_sync(torch.zeros(1, 3, 16, 16)).shape == (1, 3, 16, 16)
    with pytest.raises(ImportError, match="load_model_from_checkpoint"):      # ... but where the network is first needed
        ws.remove_sync(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ImportError, match="load_model_from_checkpoint"):
        ws.add_sync(torch.zeros(1, 3, 32, 32))


def test_without_embedder_nothing_changes(monkeypatch):
    from wmar_amd.watermarking.synchronization import WamSync
    monkeypatch.setitem(sys.modules, "deps", None)
    with pytest.raises(ImportError, match="load_model_from_checkpoint"):
        WamSync("checkpoints/wam_mit.pth", "cpu")
    w = object()
    assert WamSync(None, "cpu", wam=w).wam is w
    with pytest.raises(ValueError, match="native"):
        WamSync(None, "cpu", wam=w, embedder="torch")


def test_embedder_refuses_what_is_not_its_size_on_the_host():
    from wmar_amd.utils import synth
    from wmar_amd.watermarking.wam_embedder import WamEmbedder
    e = WamEmbedder.__new__(WamEmbedder)            # argument checks run before anything touches the device
    e.cfg, e.device = synth.WAM_RELEASED, "cpu"
    with pytest.raises(ValueError, match="256 x 256"):
        e.embed(torch.zeros(1, 3, 128, 128), torch.zeros(1, 32))
    with pytest.raises(ValueError, match="256 x 256"):
        e.add_sync(torch.zeros(1, 3, 128, 128), torch.zeros(4, 32), torch.zeros(4, 256, 256))
    with pytest.raises(ValueError, match="GPU"):
        e.embed(torch.zeros(1, 3, 256, 256), torch.zeros(1, 32))
