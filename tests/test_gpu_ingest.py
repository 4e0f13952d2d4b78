"""Image ingest on the MI355X (wmar_image_ingest, wmar_amd/csrc/ingest.hip) against the PIL path it replaces
(ImageTokenizer._whiten_transparency + _vqgan_input_from): bit for bit on every shape and mode, batched, argument checks of the C ABI,
Chameleon prompts that contain images, detect.py end to end, determinism.  Exact everywhere: no tolerances."""
import base64
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from tests import ingest_cases as K  # noqa: E402
from wmar_amd import _lib  # noqa: E402
from wmar_amd.utils import synth  # noqa: E402
from wmar_amd.utils.ingest import ingest, pack, plan  # noqa: E402


def _rgba(w, h, seed, opaque=False):
    a = K.pattern("random", w, h, 4, seed)
    if opaque:
        a[:, :, 3] = 255
    else:
        a[::3, ::2, 3] = 0              # fully transparent, fully opaque and everything between
        a[1::3, 1::2, 3] = 255
    return Image.fromarray(a, "RGBA")


def _check(images, T, label):
    got, u8 = ingest(images, T, "cuda", return_u8=True)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(images), 3, T, T)
    got, u8 = got.cpu(), u8.cpu().numpy()
    for i, img in enumerate(images):
        ref_f, ref_u8 = K.pil_path(img, T)
        assert np.array_equal(u8[i], ref_u8), (label, i, int((u8[i] != ref_u8).sum()))
        assert torch.equal(got[i], ref_f), (label, i)
    return got


@pytest.mark.parametrize("T,wh", K.CASES, ids=[f"{T}-{w}x{h}" for T, (w, h) in K.CASES])
def test_every_shape_and_mode_equals_pil(T, wh):
    w, h = wh
    images = [Image.fromarray(K.pattern("random", w, h, 3, 1)), _rgba(w, h, 2), _rgba(w, h, 3, opaque=True)]
    if w * h <= 2048 * 2048:
        images += [Image.fromarray(K.pattern("checker", w, h)), Image.fromarray(K.pattern("binary", w, h))]
    _check(images, T, (T, wh))


def test_device_whitening_table_on_all_65536_pairs():
    """a 256 x 256 RGBA image holding every (alpha, colour) pair at its own size: no resampling, so out_u8 is the device's whitening"""
    a, c = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.ascontiguousarray(np.stack([c, c[:, ::-1], (c.astype(np.int32) * 7 % 256).astype(np.uint8), a], axis=2))
    alpha = rgba[:, :, 3] / 255.0
    expect = ((1 - alpha[:, :, np.newaxis]) * 255 + alpha[:, :, np.newaxis] * rgba[:, :, :3]).astype("uint8")
    got, u8 = ingest([Image.fromarray(rgba, "RGBA")], 256, "cuda", return_u8=True)
    assert np.array_equal(u8[0].cpu().numpy(), expect)
    assert torch.equal(got[0].cpu(), K.pil_path(Image.fromarray(rgba, "RGBA"), 256)[0])
    # the same pairs under a resize (whitening comes first, then the filter)
    _check([Image.fromarray(rgba, "RGBA")], 64, "pairs-64")


def _mixed_batch():
    sizes = [(64, 64), (65, 64), (1, 1), (300, 1), (97, 211), (640, 480), (64, 192), (2, 3), (1000, 30), (128, 128), (33, 77),
             (1920, 1080), (50, 50), (64, 65), (20, 2000), (255, 256), (1024, 1024), (3, 2)]
    rng = np.random.default_rng(4)
    out = []
    for i, (w, h) in enumerate(sizes):
        kind = i % 4
        if kind == 0:
            out.append(Image.fromarray(K.pattern("random", w, h, 3, i)))
        elif kind == 1:
            out.append(_rgba(w, h, i))
        elif kind == 2:
            out.append(_rgba(w, h, i, opaque=True))
        else:
            out.append(Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), "L"))
    return out


def test_one_batch_of_mixed_sizes_and_modes_equals_the_per_image_results():
    images = _mixed_batch()
    assert len(images) >= 16
    whole = _check(images, 64, "mixed")
    for i, img in enumerate(images):
        assert torch.equal(ingest([img], 64, "cuda").cpu()[0], whole[i]), i


def test_determinism():
    images = _mixed_batch()
    a, ua = ingest(images, 64, "cuda", return_u8=True)
    b, ub = ingest(images, 64, "cuda", return_u8=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ua, ub)


def test_bad_descriptors_are_rejected_before_any_launch():
    L = _lib.load()
    T = 16
    px = [K.pattern("random", 40, 30, 3, 1), K.pattern("random", 24, 50, 4, 2)]
    host, desc = pack(px, T)
    dev = host.cuda()
    out = torch.full((2, 3, T, T), 7.0, device="cuda")
    u8 = torch.full((2, T, T, 3), 9, dtype=torch.uint8, device="cuda")

    def call(d, nbytes=None, target=T, n=2, pixels=dev):
        return L.wmar_image_ingest(pixels.data_ptr(), dev.numel() if nbytes is None else nbytes, d, n, target, out.data_ptr(),
                                   u8.data_ptr(), _lib.stream_ptr())

    def variant(i, **kw):
        d = (_lib.ImageDesc * 2)()
        for j in range(2):
            d[j] = _lib.ImageDesc(*[getattr(desc[j], f) for f, _ in _lib.ImageDesc._fields_])
        for k, v in kw.items():
            setattr(d[i], k, v)
        return d

    bad = [call(variant(1, offset=dev.numel())),                               # offset past pixels_bytes
           call(variant(1, offset=dev.numel() - 10)),                          # the image's end past pixels_bytes
           call(desc, nbytes=desc[1].offset + 24 * 50 * 4 - 1),                # the buffer one byte short
           call(variant(0, channels=2)), call(variant(0, channels=5)),
           call(variant(0, crop_x0=desc[0].new_width - T + 1)),                # crop window outside the resized image
           call(variant(1, crop_y0=-1)), call(variant(1, new_width=T - 1)),
           call(variant(0, width=0)), call(variant(0, height=32769)), call(variant(0, offset=-4)),
           call(desc, target=0), call(desc, n=0)]
    torch.cuda.synchronize()
    for rc in bad:
        assert rc == -1, bad
    with pytest.raises(_lib.WmarError, match="image_ingest"):
        _lib.check(bad[0])
    assert bool((out == 7.0).all()) and bool((u8 == 9).all())                  # nothing was launched
    assert call(desc) == 0
    torch.cuda.synchronize()
    for i, p in enumerate(px):
        ref_f, ref_u8 = K.pil_path(Image.fromarray(p), T)
        assert torch.equal(out[i].cpu(), ref_f) and np.array_equal(u8[i].cpu().numpy(), ref_u8)


# ------------------------------------------------------------------ Chameleon prompts with images
@pytest.fixture(scope="module")
def cham():
    from tests.test_gpu_chameleon import _cfg
    from wmar_amd.models.chameleon_wrapper import ChameleonARMMWrapper
    cfg = _cfg(hd=64, dim=256, vocab=2048)
    vq_cfg = synth.VQConfig(ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(), resolution=16, z_channels=32, embed_dim=32,
                            n_embed=512)
    return ChameleonARMMWrapper(None, 0, cfg=cfg, state=synth.synth_chameleon_state(cfg, seed=8, logit_scale=6.0),
                                vocab_map=synth.synth_chameleon_vocab(2048, 512), vq_cfg=vq_cfg, vq_state=synth.synth_vq_state(vq_cfg, 1),
                                max_batch=3, max_prompt_len=96)


def test_chameleon_tokenize_image_and_prompts(cham, tmp_path):
    m = cham
    img = _rgba(57, 41, 6)                                                   # non-square, larger than image_size (16), RGBA
    x = K.pil_path(img, m.image_size)[0][None].cuda()
    expect = [m.vocab.begin_image] + m.translation.convert_img2bp2(m.vq_engine.encode(x))[0].tolist() + [m.vocab.end_image]
    assert len(expect) == m.n_image_tokens + 2
    assert m.tokenize_image(img) == expect
    p = tmp_path / "in.png"
    img.save(p)
    buf = io.BytesIO()
    img.save(buf, format="PNG")
    b64 = base64.b64encode(buf.getvalue()).decode()
    assert m.tokenize_b64img(b64) == expect
    text = m.vocab.text_tokens
    for value in (img, "file:" + str(p), "data:image/png;base64," + b64):
        ids = m.tokens_from_ui([{"type": "ids", "value": [text[3]]}, {"type": "image", "value": value},
                                {"type": "sentinel", "value": "<END-OF-TURN>"}])
        assert ids == [m.vocab.bos_id, text[3]] + expect + [m.vocab.eot_id], type(value)
    with pytest.raises(ValueError, match="Unknown image format."):
        m.tokens_from_ui([{"type": "image", "value": str(p)}])
    with pytest.raises(ValueError, match="Unknown image type."):
        m.tokens_from_ui([{"type": "image", "value": np.zeros((4, 4, 3), np.uint8)}])
    with pytest.raises(ValueError, match="Unknown input type."):
        m.tokens_from_ui([{"type": "audio", "value": 0}])
    # a prompt batch with several images: the same ids as one at a time
    other = Image.fromarray(K.pattern("random", 16, 40, 3, 9))
    rows = m.tokens_from_ui_batch([[{"type": "image", "value": img}], [{"type": "image", "value": other}, {"type": "image", "value": img}]])
    assert rows[0] == [m.vocab.bos_id] + expect and rows[1] == [m.vocab.bos_id] + m.tokenize_image(other) + expect
    # generation conditioned on the image: the image tokens reach the image-conditioned stream
    full = m.tokens_from_ui([{"type": "image", "value": img}, {"type": "ids", "value": [text[5], text[9]]},
                             {"type": "sentinel", "value": "<END-OF-TURN>"}])
    streams = m.split_inputs_for_cfg([full])
    assert streams[1] == [m.vocab.bos_id] + expect + [m.vocab.begin_image]
    torch.manual_seed(1)
    codes = m.sample([(0, [{"type": "image", "value": img}, {"type": "ids", "value": [text[5], text[9]]}])],
                     {"temperature": 0.9, "top_p": 0.8})
    assert m.is_codes_shaped(codes) and codes.shape[0] == 1 and set(codes.flatten().tolist()) <= set(m.vocab.image_tokens)
    torch.manual_seed(1)
    plain = m.sample([(0, [text[5], text[9]])], {"temperature": 0.9, "top_p": 0.8})
    assert not torch.equal(codes, plain)                                       # the image is part of the condition


def test_wrappers_expose_the_pil_entry(cham):
    img = _rgba(57, 41, 6)
    x = cham.images_from_pil([img, img])
    assert torch.equal(x[0].cpu(), K.pil_path(img, 16)[0]) and torch.equal(x[0], x[1])
    assert cham.codes_from_pil([img])[0].tolist() == cham.tokenize_image(img)[1:-1]


# ------------------------------------------------------------------ detect.py end to end
TAMING_FLAGS = ["--model", "taming", "--synthetic", "1", "--synthetic_config", "harness", "--wm_method", "gentime", "--wm_seed_strategy",
                "linear", "--wm_split_strategy", "stratifiedrand", "--wm_context_size", "1", "--wm_delta", "4.0", "--wm_gamma", "0.25",
                "--batch_size", "5"]


def _write_images(model, codes, d, tag):
    imgs = model.codes_to_images(codes).cpu()
    u8 = ((imgs.clamp(-1, 1) + 1) / 2 * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    for i in range(u8.shape[0]):
        im = Image.fromarray(u8[i])
        im.save(os.path.join(d, f"{tag}_{i}_native.png"))
        if i == 0:
            im.resize((384, 384), Image.BICUBIC).save(os.path.join(d, f"{tag}_{i}_384.png"))
            im.resize((200, 300), Image.BICUBIC).save(os.path.join(d, f"{tag}_{i}_200x300.png"))
            im.resize((1000, 640), Image.BILINEAR).save(os.path.join(d, f"{tag}_{i}_1000x640.png"))
            im.convert("RGBA").save(os.path.join(d, f"{tag}_{i}_rgba.png"))


def _expected(model, wm, files):
    T = model.image_size
    x = torch.stack([K.pil_path(Image.open(f), T)[0] for f in files]).cuda()
    return wm.detect(model.images_to_codes(x)).cpu().numpy()


def _run_detect(monkeypatch, argv):
    import detect
    monkeypatch.setattr("sys.argv", ["detect.py"] + argv)
    return detect.main()


def test_detect_end_to_end_taming(tmp_path, monkeypatch):
    import detect
    from wmar_amd import cli
    args, _ = detect.get_parser().parse_known_args(TAMING_FLAGS)
    model = cli.build_model(args, "cuda:0", args.seed)
    wm = cli.build_watermarker(args, model)
    model.set_watermarker(wm)
    d = tmp_path / "imgs"
    d.mkdir()
    torch.manual_seed(0)
    gen = {"temperature": 1.0, "top_k": 250, "top_p": 0.92}
    _write_images(model, model.sample([1, 9, 400], gen, apply_watermark=True), str(d), "wm")
    _write_images(model, model.sample([1, 9, 400], gen, apply_watermark=False), str(d), "clean")
    (d / "broken.png").write_bytes(b"this is not an image")
    whole = (d / "wm_0_native.png").read_bytes()
    (d / "truncated.png").write_bytes(whole[:len(whole) // 2])
    out = tmp_path / "res" / "detect.json"
    assert _run_detect(monkeypatch, TAMING_FLAGS + ["--images", str(d), "--out", str(out)]) == 1      # unreadable files: non-zero
    recs = json.load(open(out))
    names = sorted(os.listdir(d))
    assert [os.path.basename(r["file"]) for r in recs] == names and len(names) == 16
    bad = [r for r in recs if "error" in r]
    assert sorted(os.path.basename(r["file"]) for r in bad) == ["broken.png", "truncated.png"]
    assert all("pvalue" not in r for r in bad)
    good = [r for r in recs if "error" not in r]
    expect = _expected(model, wm, [r["file"] for r in good])
    got = np.array([r["pvalue"] for r in good], dtype=np.float64)
    assert np.array_equal(got, expect, equal_nan=True), (got, expect)
    for r in good:
        assert (r["width"], r["height"]) == Image.open(r["file"]).size and r["n_scored"] >= r["n_green"] >= 0
    # a list of files instead of a directory, all readable: exit status 0, same values
    files = [str(d / n) for n in names if n not in ("broken.png", "truncated.png")]
    out2 = tmp_path / "detect2.json"
    assert _run_detect(monkeypatch, TAMING_FLAGS + ["--images"] + files[::-1] + ["--out", str(out2), "--batch_size", "64"]) == 0
    recs2 = json.load(open(out2))
    assert [r["file"] for r in recs2] == files
    assert np.array_equal(np.array([r["pvalue"] for r in recs2]), expect, equal_nan=True)


def test_detect_end_to_end_rar_gumbel(tmp_path, monkeypatch):
    from tests.test_gpu_gumbel_ctx import SMALL, SMALL_VQ
    from wmar_amd import cli
    from wmar_amd.models.rar_wrapper import RarARMMWrapper
    from wmar_amd.watermarking.gumbel_watermark import GumbelWatermark
    model = RarARMMWrapper(None, rar_cfg=SMALL, vq_cfg=SMALL_VQ, rar_state=synth.synth_rar_state(SMALL, seed=1, logit_scale=6.0),
                           vq_state=synth.synth_maskgit_state(SMALL_VQ, seed=1), max_batch=4)
    monkeypatch.setattr(cli, "build_model", lambda args, device, seed: model)
    flags = ["--model", "rar", "--wm_method", "gumbel", "--wm_context_size", "1", "--wm_gumbel_seed", "7", "--batch_size", "3"]
    wm = GumbelWatermark(256, seed=7, ngram=1, device="cuda")
    model.set_watermarker(wm)
    d = tmp_path / "imgs"
    d.mkdir()
    torch.manual_seed(0)
    _write_images(model, model.sample([7, 8], apply_watermark=True), str(d), "wm")
    out = tmp_path / "detect.json"
    assert _run_detect(monkeypatch, flags + ["--images", str(d), "--out", str(out)]) == 0
    recs = json.load(open(out))
    assert [os.path.basename(r["file"]) for r in recs] == sorted(os.listdir(d)) and len(recs) == 6
    expect = _expected(model, wm, [r["file"] for r in recs])
    assert np.array_equal(np.array([r["pvalue"] for r in recs]), expect, equal_nan=True)
    assert all("n_scored" in r and "n_green" not in r for r in recs)
