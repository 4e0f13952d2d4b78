"""CPU: the torch restatement of the WAM extractor (tests/wam_extractor_reference.py) against what the reference's own modules
computed (tests/golden/wam_extractor_*.npz, written by tests/golden/make_wam_extractor_vectors.py), the configuration read back from
a state dict, and ``--sync_extractor`` at the parsers."""
import os

import numpy as np
import pytest
import torch

import detect
import generate
from tests import wam_extractor_cases as XC
from tests import wam_extractor_reference as XR
from wmar_amd.utils import synth
from wmar_amd.watermarking.wam_extractor import config_from_state

# float64 rounding over 12 layers of O(1) values
TOL = 1e-10


@pytest.fixture(scope="module")
def fx():
    return XC.load()


def _run64(cfg, seed, B):
    st = XR.to_dtype(synth.synth_wamx_state(cfg, seed), torch.float64)
    x = torch.from_numpy(XC.images_norm(seed, B, cfg.img_size)).double()
    stages = {}
    with torch.no_grad():
        preds = XR.forward(st, cfg, x, stages)
    return preds.numpy(), {k: v.numpy() for k, v in stages.items()}


def _check_preds(tag, preds, fx, R):
    sub = XC.pred_subset(R)
    d = np.abs(preds[:, :, sub, :][:, :, :, sub] - fx[f"{tag}_preds64_sub"]).max()
    assert d <= TOL, d
    assert np.array_equal(np.packbits(preds > 0), fx[f"{tag}_signs"])
    err = fx[f"{tag}_preds_err"]
    near = (np.abs(preds) < XC.MARGIN_MULT * err[0]).any(axis=1)
    assert np.array_equal(np.packbits(near), fx[f"{tag}_near"])
    assert float(fx[f"{tag}_near_share"].max()) <= XC.NEAR_CAP


def test_restatement_equals_the_reference_small(fx):
    cfg = synth.WAMX_SMALL
    preds, st = _run64(cfg, XC.SMALL_SEED, XC.SMALL_B)
    for i in range(cfg.depth + 1):
        assert np.abs(st[f"tokens{i}"] - fx[f"s_tokens{i}"]).max() <= TOL, i
    assert np.abs(st["neck"] - fx["s_neck"]).max() <= TOL
    assert np.abs(st["up0"] - fx["s_up0"]).max() <= TOL
    assert np.abs(st["up1"][:1] - fx["s_up1_img0"]).max() <= TOL
    assert np.abs(st["up2"][:1] - fx["s_up2_img0"]).max() <= TOL
    _check_preds("s", preds, fx, cfg.img_size)


def test_restatement_equals_the_reference_released(fx):
    cfg = synth.WAMX_RELEASED
    preds, _ = _run64(cfg, XC.RELEASED_SEED, XC.RELEASED_B)
    _check_preds("r", preds, fx, cfg.img_size)


def test_upsample_written_out_is_torch_upsample():
    x = torch.randn(2, 3, 5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for f in (2, 4):
        ref = torch.nn.Upsample(scale_factor=f, mode="bilinear", align_corners=False)(x)
        assert float((XR.upsample_bilinear(x, f) - ref).abs().max()) <= 1e-14


def test_library_form_of_the_restatement_gives_the_same_logits():
    """forward(library=True) is what scripts/perf_sync.py times on the GPU: the same network with torch's interpolation kernel."""
    cfg = synth.WAMX_SMALL
    st = XR.to_dtype(synth.synth_wamx_state(cfg, XC.SMALL_SEED), torch.float64)
    x = torch.from_numpy(XC.images_norm(XC.SMALL_SEED, 1, cfg.img_size)).double()
    with torch.no_grad():
        assert float((XR.forward(st, cfg, x, library=True) - XR.forward(st, cfg, x)).abs().max()) <= TOL


@pytest.mark.parametrize("name", ["WAMX_SMALL", "WAMX_RELEASED"])
def test_config_from_state_round_trip(name):
    cfg = getattr(synth, name)
    shapes = synth.wamx_shapes(cfg)
    state = {k: torch.empty(v, device="meta") for k, v in shapes.items()}
    assert config_from_state(state) == cfg
    if name == "WAMX_SMALL":
        real = synth.synth_wamx_state(cfg, 5)
        assert config_from_state(real) == cfg and {k: tuple(v.shape) for k, v in real.items()} == shapes
    assert synth.WamExtractorConfig() == synth.WAMX_RELEASED and synth.WAMX_RELEASED.nbits == 32


def test_synth_state_distributions():
    st = synth.synth_wamx_state(synth.WAMX_SMALL, 5)
    e = "image_encoder."
    assert abs(float(st[e + "blocks.1.attn.rel_pos_h"].std()) - 0.2) < 0.03
    assert abs(float(st[e + "pos_embed"].std()) - 0.02) < 0.002
    for k in (e + "neck.1", e + "neck.3", "pixel_decoder.output_upscaling.0.upsample_block.3", e + "blocks.0.norm1"):
        assert abs(float(st[k + ".weight"].mean()) - 1.0) < 0.05 and abs(float(st[k + ".weight"].std()) - 0.1) < 0.04, k
        assert abs(float(st[k + ".bias"].std()) - 0.1) < 0.04, k
    w = st[e + "blocks.0.mlp.lin2.weight"]
    assert float(w.abs().max()) <= (3.0 / w.shape[1]) ** 0.5


def test_sync_extractor_at_the_parsers():
    base = ["--outdir", "x", "--conditioning", "1", "--model", "taming", "--images", "x"]
    for p in (generate.get_parser(), detect.get_parser()):
        a, _ = p.parse_known_args(base)
        assert a.sync_extractor == "torch"
        a, _ = p.parse_known_args(base + ["--sync", "true", "--syncpath", "checkpoints/wam_mit.pth", "--sync_extractor", "native"])
        assert a.sync_extractor == "native"
        generate.check_wm_args(a)
        with pytest.raises(SystemExit):
            p.parse_known_args(base + ["--sync_extractor", "triton"])
    a, _ = generate.get_parser().parse_known_args(base + ["--sync", "true", "--syncpath", "checkpoints/syncmodel.jit.pt", "--sync_extractor", "native"])
    with pytest.raises(ValueError, match="native extractor"):
        generate.check_wm_args(a)
    a, _ = generate.get_parser().parse_known_args(base + ["--syncpath", "checkpoints/wam_mit.pth", "--sync_extractor", "native"])
    with pytest.raises(ValueError, match="--sync true"):
        generate.check_wm_args(a)


def test_sync_extractor_is_routed_to_wamsync(monkeypatch):
    from wmar_amd import cli
    from wmar_amd.watermarking import synchronization as S
    seen = {}

    class FakeSync:
        def __init__(self, syncpath, device, **kw):
            seen.update(kw, syncpath=syncpath)

        add_sync = remove_sync = None

    monkeypatch.setattr(S, "WamSync", FakeSync)
    base = ["--outdir", "x", "--conditioning", "1", "--model", "taming", "--sync", "true", "--syncpath", "checkpoints/wam_mit.pth"]
    a, _ = generate.get_parser().parse_known_args(base + ["--sync_embedder", "native", "--sync_extractor", "native"])
    cli.build_sync_manager(a, "cpu")
    assert seen == {"embedder": "native", "extractor": "native", "syncpath": "checkpoints/wam_mit.pth"}
    seen.clear()
    a, _ = generate.get_parser().parse_known_args(base + ["--sync_extractor", "native"])
    cli.build_sync_manager(a, "cpu")
    assert seen == {"extractor": "native", "syncpath": "checkpoints/wam_mit.pth"}


def test_fixture_files_are_under_one_mib(fx):
    for name, keys in XC.FILES.items():
        assert os.path.getsize(os.path.join(XC.GOLDEN, name)) < (1 << 20), name
        assert all(k in fx for k in keys)
