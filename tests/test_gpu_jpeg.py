"""The device JPEG round trip (wmar_jpeg, wmar_amd/csrc/jpeg.hip) on the MI355X against the host path it replaces (PIL's encoder +
decoder, valuemetric.jpeg_compress) and against the committed PIL fixture: bit for bit in the harness's fused form, in the module
form (3-D / 4-D, straight-through or not, the straight-through gradient), fallbacks for shapes the kernel does not cover, argument
checks of the C ABI, the harness's sweep with PIL unavailable, determinism."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from wmar_amd import _lib  # noqa: E402
from wmar_amd.augmentations import AugmentationManager  # noqa: E402
from wmar_amd.augmentations import device_ops as D  # noqa: E402
from wmar_amd.augmentations import valuemetric  # noqa: E402
from wmar_amd.augmentations.valuemetric import JPEG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_QUALITIES = [100, 95, 85, 75, 65, 55, 45, 35, 25, 15, 5]


def _decoder_batch(B, H, W, seed):
    """[-1, 1] images as the decoder hands them over: smooth content plus noise, saturated pixels (exactly -1 / +1) and values whose
    [0, 1] form times 255 lands just below an integer"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    base = torch.stack([xx, yy, xx * yy]).unsqueeze(0) * torch.rand(B, 3, 1, 1, generator=g)
    v = (base + 0.3 * torch.randn(B, 3, H, W, generator=g)).clamp(-1.2, 1.2).clamp(-1, 1)
    k = torch.randint(1, 255, (B, 3, H, W), generator=g).float()
    below = torch.nextafter(k / 255, torch.zeros(())) * 2 - 1                   # (v / 2 + 0.5) * 255 just under k
    m = torch.rand(B, 3, H, W, generator=g)
    v = torch.where(m < 0.1, below, v)
    v = torch.where((m > 0.95) & (m < 0.975), torch.ones(()), v)
    return torch.where(m >= 0.975, -torch.ones(()), v)


def _host_fused(imgs, q):
    return JPEG()(imgs.cpu() / 2.0 + 0.5, q).clamp(0, 1) * 2.0 - 1.0


@pytest.mark.parametrize("hw", [(256, 256), (512, 512), (48, 80)])
def test_fused_form_equals_the_host_path(hw):
    imgs = _decoder_batch(4, *hw, seed=hw[0] + hw[1])
    dev = imgs.cuda()
    for q in TABLE_QUALITIES:
        got = D.fused("jpeg", dev, q)
        assert got is not None and got.is_cuda and got.shape == dev.shape, q
        ref = _host_fused(imgs, q)
        assert torch.equal(got.cpu(), ref), (hw, q, int((got.cpu() != ref).sum()))


def test_fixture():
    v = np.load(os.path.join(HERE, "golden", "jpeg_vectors.npz"))
    for key in sorted(k[len("qualities_"):] for k in v.files if k.startswith("qualities_")):
        u = torch.from_numpy(v[f"{key}_in"].astype(np.float32))
        x = ((u + 0.5) / 255).cuda()                                            # truncates back to u on entry
        for q in v[f"qualities_{key}"]:
            got = D.jpeg(x, int(q), passthrough=False).cpu().mul(255).round().to(torch.uint8).numpy()
            assert np.array_equal(got, v[f"{key}_q{int(q)}"]), (key, int(q))


@pytest.mark.parametrize("passthrough", [True, False])
def test_module_form_3d_and_4d(passthrough):
    g = torch.Generator().manual_seed(11)
    x4 = torch.rand(3, 3, 64, 96, generator=g) * 1.1 - 0.05
    x3 = torch.rand(3, 32, 32, generator=g)
    T = JPEG(passthrough=passthrough)
    for q in (5, 50, 90):
        for x in (x4, x3):
            got = T(x.cuda(), q)
            assert got.is_cuda and torch.equal(got.cpu(), T(x, q)), (passthrough, q, x.dim())


def test_module_form_straight_through_gradient():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 48, 64, generator=g)
    xd = x.cuda().requires_grad_(True)
    xh = x.clone().requires_grad_(True)
    yd, yh = JPEG()(xd, 35), JPEG()(xh, 35)
    assert yd.requires_grad and yd.is_cuda
    assert torch.equal(yd.detach().cpu(), yh.detach())
    w = torch.randn(x.shape, generator=g)
    (yd * w.cuda()).sum().backward()
    (yh * w).sum().backward()
    assert torch.equal(xd.grad.cpu(), xh.grad) and torch.equal(xh.grad, w)       # identity, as on the host path


def test_fallbacks_and_errors():
    x40 = torch.rand(2, 3, 40, 40)
    assert D.fused("jpeg", x40.cuda() * 2 - 1, 50) is None
    assert torch.equal(JPEG()(x40.cuda(), 50).cpu(), JPEG()(x40, 50))
    x1 = torch.rand(2, 1, 32, 32)
    assert D.fused("jpeg", x1.cuda() * 2 - 1, 50) is None
    with pytest.raises(TypeError):                                             # PIL has no 1-channel HxWx1 form: same on both paths
        JPEG()(x1, 50)
    with pytest.raises(TypeError):
        JPEG()(x1.cuda(), 50)

    L = _lib.load()
    x = torch.rand(1, 3, 32, 32, device="cuda")
    out = torch.empty_like(x)
    ws = torch.empty(L.wmar_jpeg_workspace_bytes(1, 32, 32), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 32 * 32 * 3 // 2
    st = _lib.stream_ptr()

    def call(inp, o, nbytes, H=32, W=32, q=50):
        return L.wmar_jpeg(inp.data_ptr(), o.data_ptr(), ws.data_ptr(), nbytes, 1, H, W, q, 0, 1, st)

    assert call(x, out, ws.numel()) == 0
    torch.cuda.synchronize()
    for rc in (call(x, out, ws.numel(), H=40), call(x, out, ws.numel(), q=0), call(x, out, ws.numel(), q=101),
               call(x, x, ws.numel()), call(x, out, ws.numel() - 1)):
        assert rc == -1
        with pytest.raises(_lib.WmarError):
            _lib.check(rc)


def test_harness_sweep_runs_without_pil(monkeypatch):
    """the default table's jpeg entry runs on the device in fill_batch_log: with the host JPEG made unusable the sweep completes,
    and its records equal those of an unfused run that goes through PIL"""
    from wmar_amd import harness

    class M:
        def codes_to_images(self, codes):
            return (codes.float().view(-1, 1, 8, 8).repeat(1, 3, 4, 4) / 32.0 - 1.0).cuda() * torch.tensor([1.0, 0.8, 0.6], device="cuda").view(1, 3, 1, 1)
        def images_to_codes(self, imgs): return ((imgs[:, 0, ::4, ::4] + 1.0) * 32.0).round().long().view(imgs.shape[0], -1)

    codes = torch.randint(0, 64, (3, 64), generator=torch.Generator().manual_seed(1)).cuda()
    table = [a for a in AugmentationManager(False, False, True).augs if a[0] == "jpeg"]
    ref = {}
    monkeypatch.setenv("WMAR_AUG_TORCH", "1")                                   # the reference run: the module's host path (PIL)
    harness.fill_batch_log(ref, "m", M(), codes, {"metric_names": [], "augmentations": table, "max_roundtrips": 0, "orig_only": False,
                                                 "fuse_augmentations": False})
    monkeypatch.delenv("WMAR_AUG_TORCH")

    def no_pil(*a, **k):
        raise RuntimeError("host JPEG called")

    monkeypatch.setattr(valuemetric, "jpeg_compress", no_pil)
    got = {}
    harness.fill_batch_log(got, "m", M(), codes, {"metric_names": [], "augmentations": table, "max_roundtrips": 0, "orig_only": False})
    assert [r[0] for r in got["m"]["jpeg"]] == TABLE_QUALITIES
    for a, b in zip(got["m"]["jpeg"], ref["m"]["jpeg"]):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), a[0]


def test_determinism():
    x = _decoder_batch(8, 256, 256, seed=9).cuda()
    a, b = D.fused("jpeg", x, 45), D.fused("jpeg", x, 45)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
