"""MI355X: the BILINEAR ingest (``wmar_image_ingest_filtered``) against PIL byte for byte -- eight shapes, windows touching every
edge, both outputs, a mixed batch, the LANCZOS entry unchanged -- and ``precompute_codes.py`` end to end against the host path."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

from tests import bilinear_reference as BL

pytestmark = pytest.mark.gpu

LANCZOS, BILINEAR = 1, 2


def _device(pix, plans, T, filt):
    from wmar_amd.utils import ingest
    host, desc = ingest.pack(pix, T, plans)
    out, u8 = ingest.ingest_packed(host.cuda(), desc, T, return_u8=True, filter=filt)
    return out.cpu(), u8.cpu().numpy()


def _exit(u8):
    return (torch.from_numpy(u8).to(torch.float64) / 255.0 * 2 - 1).permute(2, 0, 1).to(torch.float32)


@pytest.mark.parametrize("wh,T", BL.SHAPES)
def test_bilinear_windows_equal_pil(wh, T):
    w, h = wh
    a = BL.image(w, h, 7 * w + h)
    new = BL.resize_plan(wh, T)
    ref = np.array(Image.fromarray(a).resize(new, Image.BILINEAR))
    wins = BL.windows(new, T)
    out, u8 = _device([a] * len(wins), [(new, xy) for xy in wins], T, BILINEAR)        # one batch: the same image at every window
    for i, (x0, y0) in enumerate(wins):
        want = ref[y0:y0 + T, x0:x0 + T]
        assert np.array_equal(u8[i], want), (wh, T, x0, y0)
        assert torch.equal(out[i], _exit(want)), (wh, T, x0, y0)


def test_a_mixed_batch_equals_the_per_image_results_and_lanczos_is_unchanged():
    from wmar_amd.utils import ingest
    T = 32
    shapes = [wh for wh, t in BL.SHAPES if t == T] + [(32, 32), (64, 32), (500, 375)]
    pix = [BL.image(w, h, 3 * w + h) for w, h in shapes]
    gen = torch.Generator().manual_seed(2)
    plans = []
    for w, h in shapes:
        new = ingest.resize_plan((w, h), T)
        plans.append((new, ingest.random_crop_origin(new, T, gen)))
    out, u8 = _device(pix, plans, T, BILINEAR)
    for i, (a, (new, (x0, y0))) in enumerate(zip(pix, plans)):
        one_out, one_u8 = _device([a], [plans[i]], T, BILINEAR)
        want = np.array(Image.fromarray(a).resize(new, Image.BILINEAR).crop((x0, y0, x0 + T, y0 + T)))
        assert np.array_equal(u8[i], want) and np.array_equal(one_u8[0], want), shapes[i]
        assert torch.equal(out[i], one_out[0]) and torch.equal(out[i], _exit(want)), shapes[i]
    # the existing entry and the filtered one with LANCZOS: the same bytes, and PIL's
    host, desc = ingest.pack(pix, T)
    dev = host.cuda()
    old, old_u8 = ingest.ingest_packed(dev, desc, T, return_u8=True)
    new_, new_u8 = ingest.ingest_packed(dev, desc, T, return_u8=True, filter=LANCZOS)
    from wmar_amd import _lib
    via = torch.empty_like(old)
    via_u8 = torch.empty_like(old_u8)
    _lib.check(_lib.load().wmar_image_ingest_filtered(dev.data_ptr(), dev.numel(), desc, len(pix), T, via.data_ptr(), via_u8.data_ptr(), LANCZOS,
                                                      _lib.stream_ptr(dev.device)))
    assert torch.equal(old, new_) and torch.equal(old_u8, new_u8) and torch.equal(old, via) and torch.equal(old_u8, via_u8)
    for i, a in enumerate(pix):
        nw, (x0, y0) = ingest.plan((a.shape[1], a.shape[0]), T)
        want = np.array(Image.fromarray(a).resize(nw, Image.LANCZOS).crop((x0, y0, x0 + T, y0 + T)))
        assert np.array_equal(old_u8[i].cpu().numpy(), want), shapes[i]
    with pytest.raises(_lib.WmarError, match="filter"):
        ingest.ingest_packed(dev, desc, T, filter=3)


def test_precompute_cli_equals_the_host_path_and_feeds_finetune(tmp_path, capsys):
    import finetune as ft_cli
    import precompute_codes as cli
    from wmar_amd.models.taming_wrapper import TamingARMMWrapper
    from wmar_amd.utils import ingest, synth
    T = 32
    rng = np.random.default_rng(4)
    src = tmp_path / "images"
    src.mkdir()
    rgb = Image.fromarray(rng.integers(0, 256, (53, 37, 3), dtype=np.uint8))
    Image.fromarray(rng.integers(0, 256, (40, 71, 4), dtype=np.uint8), "RGBA").save(src / "a_rgba.png")
    Image.fromarray(rng.integers(0, 256, (T, T, 3), dtype=np.uint8)).save(src / "b_exact.png")
    Image.fromarray(rng.integers(0, 256, (90, 33), dtype=np.uint8), "L").save(src / "c_grey.png")
    rgb.save(src / "d_rgb.png")
    rgb.resize((64, 48)).convert("P", palette=Image.ADAPTIVE, colors=17).save(src / "e_pal.png")
    (src / "f_bad.png").write_bytes(b"not an image")
    out = tmp_path / "out"
    argv = f"--model taming --synthetic --synthetic_config harness --images {src} --outdir {out} --seed 3 --batch_size 4 --save_images".split()
    assert cli.main(argv) == 1
    captured = capsys.readouterr()
    assert "f_bad.png" in captured.err and "5 images, 1 unreadable" in captured.out
    files = (out / "files.txt").read_text().splitlines()
    assert [f.rsplit("/", 1)[1] for f in files] == ["a_rgba.png", "b_exact.png", "c_grey.png", "d_rgb.png", "e_pal.png"]
    codes = np.load(out / "codes.npy")
    cfg = synth.VQConfig(**synth.HARNESS_VQ)
    assert codes.dtype == np.int64 and codes.shape == (5, cfg.codes_size ** 2)
    # the host path: PIL resize and crop with the same generator draws, then the same engine
    model = TamingARMMWrapper.synthetic(synth.GPTConfig(**synth.HARNESS_GPT), cfg, seed=0, max_batch=8)
    gen = torch.Generator().manual_seed(3)
    xs, crops = [], []
    for f in files:
        img = Image.open(f).convert("RGB")
        new = ingest.resize_plan(img.size, T)
        if new != img.size:
            img = img.resize(new, Image.BILINEAR)
        if img.size != (T, T):
            i = int(torch.randint(0, img.size[1] - T + 1, size=(1,), generator=gen))
            j = int(torch.randint(0, img.size[0] - T + 1, size=(1,), generator=gen))
            img = img.crop((j, i, j + T, i + T))
        crops.append(np.array(img))
        xs.append(_exit(crops[-1]))
    want = model.model.vq_engine.encode(torch.stack(xs).cuda()).cpu().numpy()
    assert np.array_equal(codes, want)
    for k, crop in enumerate(crops):
        assert np.array_equal(np.array(Image.open(out / "images" / f"{k:08d}.png")), crop), files[k]
    # and finetune.py takes the file
    ft_out = tmp_path / "ft"
    assert ft_cli.main(f"--model taming --synthetic --synthetic_config harness --datapath {out / 'codes.npy'} --val_percent 0.4 --nb_epochs 1 "
                       f"--augs none --batch_size_per_gpu 2 --outdir {ft_out}".split()) == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert sum("step" in l for l in lines) == 2 and sum(l.get("split") == "val" and "aug" in l and l["n"] == 2 for l in lines) == 2
    assert (ft_out / "encoder_ft_delta.pth").exists() and (ft_out / "decoder_ft_delta.pth").exists()
