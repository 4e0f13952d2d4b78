"""GPU: the WAM embedder on the device (wmar_wam_embed / wmar_wam_add_sync and the three probes) against what the reference's own
modules computed in float64 (tests/golden/wam_vectors*.npz) and against the float64 restatement (tests/wam_reference.py).

Gates, none of them measured on the code under test: for preds_w, imgs_w and add_sync the device error against the reference's
float64 run must stay within 4 x (rms) and 8 x (max) of the error of the reference's OWN float32 run against that float64 run, as
the fixture records it (``*_err``).  The measured ratios are printed on lines starting WAMEMBED.  Pixels whose float64 la (the
5 x 5 luminance stencil / 32) lies within 1e-3 of the switch at 127 are left out of the JND and image comparisons -- the two branches
differ by about 3 there -- and at most 1 pixel in 10 000 of an image may be.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import wam_cases as WC
from tests import wam_reference as WR
from wmar_amd.utils import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
EPS = 2.0 ** -24                                   # half an ulp of 1 in float32
RMS_GATE, MAX_GATE = 4.0, 8.0


@functools.lru_cache(maxsize=None)
def gold(name):
    return dict(np.load(os.path.join(GOLD, name)))


@functools.lru_cache(maxsize=None)
def engine(which, max_batch):
    from wmar_amd.watermarking.wam_embedder import WamEmbedder
    cfg, seed = (synth.WAM_SMALL, WC.SMALL_SEED) if which == "small" else (synth.WAM_RELEASED, WC.RELEASED_SEED)
    return WamEmbedder(cfg, synth.synth_wam_state(cfg, seed), DEV, max_batch=max_batch)


@functools.lru_cache(maxsize=None)
def small_inputs():
    u = torch.from_numpy(WC.images01(WC.SMALL_SEED, WC.SMALL_B, 64))
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    x = (u - mean) / std                           # normalize_img in float32, as the reference's float32 run was fed
    keep = ~WR.la_excluded(WR.unnormalize(x.double()))          # [B, R, R]
    assert all(int((~k).sum()) <= WC.LA_CAP * 64 * 64 for k in keep)
    return {"x": x.to(DEV), "pm1": torch.from_numpy(WC.images_pm1(WC.SMALL_SEED, WC.SMALL_B, 64)).to(DEV),
            "msgs": torch.from_numpy(WC.messages(WC.SMALL_SEED, WC.SMALL_B)).to(DEV), "keep": keep.numpy(),
            "sync_msgs": torch.from_numpy(WC.SYNC_MSGS).to(DEV), "masks": WR.grid_masks(64).to(DEV)}


def gate(tag, got, want64, ref_err, keep=None):
    """rms <= 4 x, max <= 8 x the reference's own float32 error (max, rms) against the same float64 array"""
    d = np.abs(got.astype(np.float64) - want64)
    if keep is not None:
        d = d[np.broadcast_to(keep[:, None], d.shape)]
    mx, rms = float(d.max()), float(np.sqrt(np.mean(d * d)))
    print(f"WAMEMBED {tag}: max {mx:.3g} = {mx / ref_err[0]:.2f} x reference fp32 ({ref_err[0]:.3g}), "
          f"rms {rms:.3g} = {rms / ref_err[1]:.2f} x ({ref_err[1]:.3g})")
    assert rms <= RMS_GATE * ref_err[1], (tag, rms, ref_err[1])
    assert mx <= MAX_GATE * ref_err[0], (tag, mx, ref_err[0])


# ---------------------------------------------------------------------------------------------------------------- whole calls
@pytest.mark.parametrize("max_batch", [5, 1])
def test_small_embed_and_add_sync_against_float64(max_batch):
    I, g, gf, gr = small_inputs(), gold("wam_vectors.npz"), gold("wam_vectors_f32.npz"), gold("wam_vectors_released.npz")
    e = engine("small", max_batch)
    out = e.embed(I["x"], I["msgs"])
    assert out["msgs"] is I["msgs"] and out["preds_w"].shape == out["imgs_w"].shape == (3, 3, 64, 64)
    gate(f"small mb{max_batch} preds_w", out["preds_w"].cpu().numpy(), g["s_preds64"], gr["s_preds_err"])
    gate(f"small mb{max_batch} imgs_w", out["imgs_w"].cpu().numpy(), g["s_imgs_w64"], gr["s_imgs_w_err"], I["keep"])
    # 3 images x 4 messages = 12 decoder rows: chunks of 5, 5, 2 (or twelve of 1); images cross chunk boundaries
    sync = e.add_sync(I["pm1"], I["sync_msgs"], I["masks"])
    gate(f"small mb{max_batch} add_sync", sync.cpu().numpy(), gf["s_sync64"], gr["s_sync_err"], I["keep"])
    assert float(sync.min()) >= -1.0 and float(sync.max()) <= 1.0


def test_small_single_image():
    I, g, gr = small_inputs(), gold("wam_vectors.npz"), gold("wam_vectors_released.npz")
    out = engine("small", 5).embed(I["x"][1:2], I["msgs"][1:2])
    gate("small B1 preds_w", out["preds_w"].cpu().numpy(), g["s_preds64"][1:2], gr["s_preds_err"])
    gate("small B1 imgs_w", out["imgs_w"].cpu().numpy(), g["s_imgs_w64"][1:2], gr["s_imgs_w_err"], I["keep"][1:2])
    # a row does not depend on what else is in the batch
    full = engine("small", 5).embed(I["x"], I["msgs"])
    assert torch.equal(full["imgs_w"][1:2], out["imgs_w"]) and torch.equal(full["preds_w"][1:2], out["preds_w"])


def test_released_add_sync_against_float32_in_full_and_the_float64_subset():
    gr = gold("wam_vectors_released.npz")
    e = engine("released", 4)
    pm1 = torch.from_numpy(WC.images_pm1(WC.RELEASED_SEED, 1, 256)).to(DEV)
    keep = ~WR.la_excluded(WR.unnormalize(WR.normalize((pm1.cpu().double() + 1.0) / 2.0))).numpy()
    assert int((~keep).sum()) <= WC.LA_CAP * 256 * 256
    got = e.add_sync(pm1, torch.from_numpy(WC.SYNC_MSGS).to(DEV), WR.grid_masks(256).to(DEV)).cpu().numpy()
    gate("released add_sync (every 4th pixel)", got[:, :, ::4, ::4], gr["r_sync64_sub"], gr["r_sync_err"], keep[:, ::4, ::4])
    # against the reference's float32 run in full: both lie around the same float64 values, the reference within its recorded error
    # and the device within its gate, so they are at most (1 + 8) x max apart, and (1 + 4) x in rms
    d = np.abs(got.astype(np.float64) - gr["r_sync32"])[np.broadcast_to(keep[:, None], got.shape)]
    mx, rms = float(d.max()), float(np.sqrt(np.mean(d * d)))
    print(f"WAMEMBED released add_sync against reference fp32 in full: max {mx:.3g} ({mx / gr['r_sync_err'][0]:.2f} x), rms {rms:.3g} "
          f"({rms / gr['r_sync_err'][1]:.2f} x)")
    assert mx <= (1 + MAX_GATE) * gr["r_sync_err"][0] and rms <= (1 + RMS_GATE) * gr["r_sync_err"][1]
    # embed at the released shape, against the float64 subset
    x = ((torch.from_numpy(WC.images01(WC.RELEASED_SEED, 1, 256)) - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
         / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)).to(DEV)
    out = e.embed(x, torch.from_numpy(WC.messages(WC.RELEASED_SEED, 1)).to(DEV))
    gate("released preds_w (every 4th pixel)", out["preds_w"].cpu().numpy()[:, :, ::4, ::4], gr["r_preds64_sub"], gr["r_preds_err"])
    gate("released imgs_w (every 4th pixel)", out["imgs_w"].cpu().numpy()[:, :, ::4, ::4], gr["r_imgs_w64_sub"], gr["r_imgs_w_err"],
         keep[:, ::4, ::4])


def test_two_runs_are_bit_equal_with_and_without_a_chunk_boundary():
    I = small_inputs()
    for mb in (5, 16):                             # 12 rows: 5 + 5 + 2, and one chunk
        e = engine("small", mb)
        a = e.add_sync(I["pm1"], I["sync_msgs"], I["masks"])
        b = e.add_sync(I["pm1"], I["sync_msgs"], I["masks"])
        assert torch.equal(a, b), mb
        ea, eb = e.embed(I["x"], I["msgs"]), e.embed(I["x"], I["msgs"])
        assert torch.equal(ea["imgs_w"], eb["imgs_w"]) and torch.equal(ea["preds_w"], eb["preds_w"]), mb
    # and the chunking does not change a bit either
    assert torch.equal(engine("small", 5).add_sync(I["pm1"], I["sync_msgs"], I["masks"]),
                       engine("small", 16).add_sync(I["pm1"], I["sync_msgs"], I["masks"]))


# ---------------------------------------------------------------------------------------------------------------- the tail, unfused
# Both forms differ from the fused tail only by the rounding of the last transform: WamSync.unnormalize evaluates (x std + mean) 2 - 1
# where the kernel evaluates ((x - (-mean / std)) / (1 / std)) 2 - 1, as the reference does.  In [0, 1] units each form makes at most
# two roundings of half an ulp of 4 scaled by std <= 0.229 or half an ulp of 1, and carries constants rounded to float32: below
# 4 * 2^-24 each; times 2 for the map to [-1, 1], two forms: 16 * 2^-24 = 9.6e-7.
UNFUSED_BOUND = 16 * EPS


class _NativeWam:
    """A WAM-like object whose embed is the device embedder: what the existing WamSync.add_sync loop is run with."""

    def __init__(self, e):
        self.e = e

    def embed(self, imgs, msg):
        return self.e.embed(imgs, msg)


def test_fused_add_sync_equals_the_existing_loop_over_native_embed():
    from wmar_amd.watermarking.synchronization import WamSync
    I, e = small_inputs(), engine("small", 5)
    loop = WamSync(None, DEV, wam=_NativeWam(e)).add_sync(I["pm1"])          # normalise, 4 x embed, mask blend, unnormalise in torch
    fused = WamSync(None, DEV, wam=object(), embedder=e).add_sync(I["pm1"])    # one wmar_wam_add_sync
    d = float((loop - fused).abs().max())
    print(f"WAMEMBED fused add_sync against the torch loop over native embed: max {d:.3g} (bound {UNFUSED_BOUND:.3g})")
    assert d <= UNFUSED_BOUND


def test_fused_tail_equals_unnormalize_of_native_embed():
    from wmar_amd.watermarking.synchronization import WamSync
    I, e = small_inputs(), engine("small", 5)
    ws = WamSync(None, DEV, wam=object())
    ones = torch.ones(1, 64, 64, device=DEV)
    for k in (1, 2):
        msg = I["sync_msgs"][k:k + 1]
        want = ws.unnormalize(e.embed(ws.normalize(I["pm1"]), msg.expand(3, -1).contiguous())["imgs_w"])
        got = e.add_sync(I["pm1"], msg, ones)
        assert float((got - want).abs().max()) <= UNFUSED_BOUND, k


# ---------------------------------------------------------------------------------------------------------------- probes
def _lib():
    from wmar_amd import _lib
    return _lib, _lib.load()


@pytest.mark.parametrize("pattern", ["zeros", "ones", "alternating", "random"])
def test_latent_msg_probe(pattern):
    L_, L = _lib()
    nbits, z, S, B, K = 32, 4, 8, 3, 4
    rng = np.random.Generator(np.random.PCG64(5))
    lat = torch.from_numpy(rng.standard_normal((B, S, S, 8)).astype(np.float32)).to(DEV)
    lat[..., z:] = 7.0                             # what the padding channels of the encoder output hold must not leak
    E = synth.synth_wam_state(synth.WAM_SMALL, WC.SMALL_SEED)["msg_processor.msg_embeddings.weight"]
    msgs = {"zeros": np.zeros((K, nbits)), "ones": np.ones((K, nbits)), "alternating": np.tile([0, 1], (K, nbits // 2)),
            "random": rng.integers(0, 2, (K, nbits))}[pattern].astype(np.int32)
    msgs[1:] = rng.integers(0, 2, (K - 1, nbits))  # row 0 carries the pattern
    Cs = 72
    out = torch.full((B * K, S, S, Cs), -3.0, device=DEV)
    m = torch.from_numpy(msgs).to(DEV)
    Ed = E.to(DEV).contiguous()
    L_.check(L.wmar_wam_probe_latent_msg(lat.data_ptr(), B, S, z, nbits, Ed.data_ptr(), m.data_ptr(), K, B * K, K, K, out.data_ptr(),
                                         L_.stream_ptr(DEV)))
    out = out.cpu().numpy()
    E64 = E.double().numpy()
    for r in range(B * K):
        b, k = r // K, r % K
        assert np.array_equal(out[r, :, :, :z], lat[b, :, :, :z].cpu().numpy())
        rows = E64[2 * np.arange(nbits) + msgs[k]]
        want, bound = rows.sum(axis=0), nbits * EPS * np.abs(rows).sum(axis=0)
        assert np.all(np.abs(out[r, 0, 0, z:z + 2 * nbits] - want) <= bound)
        assert np.array_equal(out[r, :, :, z:z + 2 * nbits], np.broadcast_to(out[r, 0, 0, z:z + 2 * nbits], (S, S, 2 * nbits)))
        assert np.all(out[r, :, :, z + 2 * nbits:] == 0.0)
    # the embed form: row r takes image r and message r
    out2 = torch.empty(3, S, S, Cs, device=DEV)
    L_.check(L.wmar_wam_probe_latent_msg(lat.data_ptr(), B, S, z, nbits, Ed.data_ptr(), m.data_ptr(), K, 3, 1, 0, out2.data_ptr(),
                                         L_.stream_ptr(DEV)))
    for r in range(3):
        assert np.array_equal(out2[r].cpu().numpy(), out[r * K + r])


def _jnd_probe(u):
    L_, L = _lib()
    u = u.to(DEV).contiguous()
    heat = torch.empty(u.shape[0], u.shape[-1], u.shape[-1], device=DEV)
    L_.check(L.wmar_wam_probe_jnd(u.data_ptr(), u.shape[0], u.shape[-1], heat.data_ptr(), L_.stream_ptr(DEV)))
    return heat.cpu().numpy()


def _jnd_bound(u64):
    """Per pixel, in heat units.  In 255 units: the luminance of a pixel carries at most 5 half-ulps of 255 (three products, two sums);
    the 5 x 5 stencil adds 25 of them with weights summing to 32 and divides by 32, the Sobel stencils add 8 with weights summing to 8:
    la within 2e-4, the gradient within 2e-4 * 8.  d cm / d g <= 0.2 and powf is good to 4 ulp of a cm <= 40: 2e-5.  The two-branch
    curve has slope 17 / (254 sqrt(la / 127 + 1e-5)) below 127 (21 at la = 0, 0.07 at 127) and 3 / 128 above.  Sum: 5e-4 + 2e-4 slope."""
    la, _ = WR.luminance_average(u64)
    slope = torch.where(la <= 127.0, 17.0 / (254.0 * torch.sqrt(la / 127.0 + 1e-5)), torch.full_like(la, 3.0 / 128.0))
    return ((5e-4 + 2e-4 * slope) / 255.0)[:, 0].numpy()


def test_jnd_probe_on_constructed_images():
    cases = WC.jnd_cases(32)
    u = torch.from_numpy(np.stack(list(cases.values())))
    got, want = _jnd_probe(u), WR.jnd_heat(u.double())[:, 0].numpy()
    keep = ~WR.la_excluded(u.double()).numpy()
    assert keep.all()                              # the constructed levels stay 1 away from the switch
    for i, name in enumerate(cases):
        assert np.all(np.abs(got[i] - want[i]) <= _jnd_bound(u.double())[i]), name
    # exact values: flat 0 is la = 17 (1 - sqrt(1e-5)) everywhere, the border included
    assert np.allclose(got[0], 17.0 * (1.0 - np.sqrt(1e-5)) / 255.0, rtol=0, atol=4 * EPS)


@pytest.mark.parametrize("R", [64, 40, 256])
def test_jnd_probe_on_fixture_images(R):
    if R == 40:                                    # a size that is no multiple of the 32 x 32 tile: crops of the 64 x 64 images
        u = torch.from_numpy(np.ascontiguousarray(WC.images01(WC.SMALL_SEED, 3, 64)[:, :, 3:43, 5:45]))
    else:
        u = torch.from_numpy(WC.images01(WC.SMALL_SEED if R == 64 else WC.RELEASED_SEED, 3 if R == 64 else 1, R))
    got, want = _jnd_probe(u), WR.jnd_heat(u.double())[:, 0].numpy()
    keep = ~WR.la_excluded(u.double()).numpy()
    assert all(int((~k).sum()) <= WC.LA_CAP * R * R for k in keep)
    ok = np.abs(got - want) <= _jnd_bound(u.double())
    assert ok[keep].all(), float(np.abs(got - want)[keep].max())
    if R == 64:                                    # and the reference's own float64 heat map of these images
        x = (u - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        got = _jnd_probe(WR.unnormalize(x.double()).float())
        assert (np.abs(got - gold("wam_vectors.npz")["s_heat64"]) <= _jnd_bound(WR.unnormalize(x.double())) + 2 * EPS)[keep].all()


def test_tail_probe_against_the_restatement():
    L_, L = _lib()
    I = small_inputs()
    rng = np.random.Generator(np.random.PCG64(9))
    y = torch.from_numpy(rng.standard_normal((3, 64, 64, 8)).astype(np.float32) * 0.7)
    preds64 = torch.tanh(y[..., :3].double()).permute(0, 3, 1, 2)
    for att_name, att in (("none", 0), ("jnd_1_3", 1), ("jnd_1_3_blue", 2)):
        want = WR.blend(I["x"].cpu().double(), preds64, 2.0, 1.0, att_name).numpy()
        out, preds = torch.empty(3, 3, 64, 64, device=DEV), torch.empty(3, 3, 64, 64, device=DEV)
        L_.check(L.wmar_wam_probe_tail(y.to(DEV).data_ptr(), I["x"].data_ptr(), 1, 3, 64, None, 0, 2.0, 1.0, att, out.data_ptr(),
                                       preds.data_ptr(), L_.stream_ptr(DEV)))
        # |w| <= 5: tanh to 2 ulp, the blend and the two colour transforms a dozen roundings of half an ulp of 8; the heat map as bounded
        # above multiplies u_w - u = scaling_w d std (|.| <= 2 std) and the result is divided by std again: twice the heat bound
        tol = 12 * 8 * EPS + (2.0 * _jnd_bound(WR.unnormalize(I["x"].cpu().double()))[:, None] if att else 0.0)
        ok = (np.abs(out.cpu().numpy() - want) <= tol) | ~np.broadcast_to(I["keep"][:, None], want.shape)
        assert ok.all(), (att_name, float(np.abs(out.cpu().numpy() - want).max()))
        assert float((preds.cpu().double() - preds64).abs().max()) <= 4 * EPS


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_output_untouched():
    L_, L = _lib()
    e = engine("released", 4)
    sentinel = 123.25
    out = torch.full((1, 3, 256, 256), sentinel, device=DEV)
    msgs, masks = torch.from_numpy(WC.SYNC_MSGS).to(DEV), WR.grid_masks(256).to(DEV)
    good = torch.zeros(1, 3, 256, 256, device=DEV)
    with pytest.raises(ValueError, match="256 x 256"):                    # a 128 x 128 image into the 256 x 256 engine
        e.add_sync(torch.zeros(1, 3, 128, 128, device=DEV), msgs, masks[:, :, :128, :128], out=out)
    with pytest.raises(ValueError, match="0 or 1"):                       # a mask value of 2
        e.add_sync(good, msgs, masks * 2, out=out)
    with pytest.raises(ValueError, match="1..8"):                         # K = 9
        e.add_sync(good, msgs[:1].expand(9, -1).contiguous(), masks[:1].expand(9, -1, -1, -1).contiguous(), out=out)
    with pytest.raises(ValueError, match="256 x 256"):
        e.embed(torch.zeros(1, 3, 128, 128, device=DEV), msgs[:1])
    # and the C entry points themselves: WMAR_EINVAL, nothing launched
    small = torch.zeros(1, 3, 128, 128, device=DEV)
    m8 = masks.reshape(4, 256, 256).to(torch.uint8).contiguous()
    st = L_.stream_ptr(DEV)
    assert L.wmar_wam_add_sync(e._h, small.data_ptr(), 1, 128, msgs.data_ptr(), 4, m8.data_ptr(), out.data_ptr(), st) == -1
    assert b"128 x 128" in L.wmar_last_error() and b"256 x 256" in L.wmar_last_error()
    m9 = torch.zeros(9, 256, 256, dtype=torch.uint8, device=DEV)
    msgs9 = torch.zeros(9, 32, dtype=torch.int32, device=DEV)
    assert L.wmar_wam_add_sync(e._h, good.data_ptr(), 1, 256, msgs9.data_ptr(), 9, m9.data_ptr(), out.data_ptr(), st) == -1
    assert b"1..8" in L.wmar_last_error()
    assert L.wmar_wam_embed(e._h, small.data_ptr(), 1, 128, msgs.data_ptr(), out.data_ptr(), None, st) == -1
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


def test_create_refuses_with_a_text():
    from wmar_amd._lib import WmarError
    from wmar_amd.watermarking.wam_embedder import WamEmbedder
    import dataclasses
    state = synth.synth_wam_state(synth.WAM_SMALL, 0)
    for bad, text in ((dict(ch=48), "multiple of 32"), (dict(resolution=32), "multiple of 8"), (dict(nbits=65), "1..64")):
        with pytest.raises(WmarError, match=text):
            WamEmbedder(dataclasses.replace(synth.WAM_SMALL, **bad), state, DEV, max_batch=2)
    with pytest.raises(ValueError, match="attenuation"):
        WamEmbedder(dataclasses.replace(synth.WAM_SMALL, attenuation="jnd_3_3"), state, DEV, max_batch=2)


# ---------------------------------------------------------------------------------------------------------------- the CLI route
def test_sync_embedder_native_from_a_synthetic_checkpoint(tmp_path, monkeypatch):
    """--sync true --sync_embedder native: the embedder from the checkpoint's embedder.* tensors, the extractor from --sync_factory,
    and no WAM checkout on the path."""
    import importlib
    import generate
    from wmar_amd import cli
    state = synth.synth_wam_state(synth.WAM_RELEASED, WC.RELEASED_SEED)
    ckpt = {"embedder." + k: v for k, v in state.items()}
    ckpt["detector.pixel_decoder.bias"] = torch.zeros(3)          # the rest of a Wam state dict is ignored
    path = tmp_path / "wam_mit_synth.pth"
    torch.save(ckpt, path)
    (tmp_path / "wam_extractor_factory.py").write_text(
        "from tests.sync_standins import ColourWam\n"
        "def extractor(args, device):\n    return ColourWam(device)\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    with pytest.raises(ImportError):
        importlib.import_module("deps.watermark_anything.utils.inference_utils")
    args = generate.get_parser().parse_args(["--sync", "true", "--syncpath", str(path), "--sync_embedder", "native", "--sync_factory",
                                             "wam_extractor_factory:extractor"])
    generate.check_wm_args(args)
    mgr = cli.build_sync_manager(args, DEV)
    assert mgr.sync.embedder.cfg == synth.WAM_RELEASED and type(mgr.sync.wam).__name__ == "ColourWam"
    pm1 = torch.from_numpy(WC.images_pm1(WC.RELEASED_SEED, 1, 256)).to(DEV)
    out = mgr.add_sync(pm1)
    assert torch.equal(out, engine("released", 4).add_sync(pm1, torch.from_numpy(WC.SYNC_MSGS).to(DEV), WR.grid_masks(256).to(DEV)))
    assert mgr.remove_sync(out).shape == out.shape and set(mgr.last_seconds) == {"add_sync", "remove_sync"}
