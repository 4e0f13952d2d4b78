"""MI355X: tokenizer training at Chameleon's layout (five levels, two neighbouring levels of equal width, no level attention, a mid
attention) and the forward-only ("frozen") engine handles.

``chameleon_small`` is finetune.py's CHAMELEON_SMALL_VQ: the layout of synth.CHAMELEON_VQ at 128 x 128 with an 8 x 8 code grid.
Forwards: taped, no-grad and ``frozen=True`` are bit-equal to the inference engine.  Gradients: the gate of tests/test_gpu_vq_train.py
-- per tensor |got - g64|_inf / |g64|_inf <= 8 x the same figure of torch's fp32 CPU autograd of the same walkers, measured in the
same run; the ratios are printed on VQTRAIN lines (run with -s)."""
import functools

import pytest
import torch

from tests import vq_grad_reference as G

pytestmark = pytest.mark.gpu

GATE = 8.0


def _cfg():
    import finetune as cli
    from wmar_amd.utils import synth
    return synth.VQConfig(**cli.CHAMELEON_SMALL_VQ)


@functools.lru_cache(maxsize=None)
def _setup():
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = _cfg()
    sd = synth.synth_vq_state(cfg, 5, "cpu")
    state = {k: v.detach().to("cuda", torch.float32).contiguous() for k, v in sd.items()}
    return cfg, sd, state, TrainableTokenizer(cfg, state, max_batch=2)


def _inputs(cfg, half, B, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * half + B)
    S, R = cfg.codes_size, cfg.resolution
    if half == 0:
        return torch.rand(B, 3, R, R, generator=g) * 2 - 1, torch.randn(B, cfg.embed_dim, S, S, generator=g)
    return torch.randn(B, cfg.embed_dim, S, S, generator=g), torch.randn(B, 3, R, R, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(half, B):
    cfg, sd, _, _ = _setup()
    x, r = _inputs(cfg, half, B)
    return G.half_gradients(sd, cfg, half, x, r, torch.float64), G.half_gradients(sd, cfg, half, x, r, torch.float32)


def test_the_small_config_keeps_chameleons_layout():
    from wmar_amd.utils import synth
    cfg = _cfg()
    assert cfg.ch_mult == synth.CHAMELEON_VQ.ch_mult and cfg.num_res_blocks == synth.CHAMELEON_VQ.num_res_blocks
    assert tuple(cfg.attn_resolutions) == tuple(synth.CHAMELEON_VQ.attn_resolutions) == ()
    assert cfg.codes_size == 8 and cfg.resolution % 128 == 0


@pytest.mark.parametrize("B", [2, 1])
def test_forwards_are_bit_equal_to_the_inference_engine(B):
    from wmar_amd.models.engine import VQGANEngine
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    cfg, _, state, tok = _setup()
    eng = VQGANEngine(cfg, state, max_batch=2)
    frozen = TrainableTokenizer(cfg, {k: v.detach().clone() for k, v in state.items()}, max_batch=2, frozen=True)
    x, _ = _inputs(cfg, 0, B, seed=3)
    codes = torch.randint(0, cfg.n_embed, (B, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(B)).cuda()
    _, pre = eng.encode(x.cuda(), return_prequant=True)
    with torch.no_grad():
        mine_eval = tok.encode_prequant(x.cuda())
        img_eval = tok.decode(tok.embed(codes))
    mine = tok.encode_prequant(x.cuda())                      # the taped engine
    img = tok.decode(tok.embed(codes))
    mine_frozen = frozen.encode_prequant(x.cuda())            # grad mode on: a frozen tokenizer still returns no graph
    img_frozen = frozen.decode(frozen.embed(codes))
    assert mine.requires_grad and img.requires_grad
    assert not mine_eval.requires_grad and not mine_frozen.requires_grad and not img_frozen.requires_grad
    for m in (mine, mine_eval, mine_frozen):
        assert torch.equal(m.detach().permute(0, 2, 3, 1).reshape(-1, cfg.embed_dim), pre)
    want = eng.decode(codes)
    for i in (img, img_eval, img_frozen):
        assert torch.equal(i.detach().clamp(-1, 1), want)


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("half", [0, 1], ids=["encoder", "decoder"])
def test_gradients_against_float64_autograd(half, B):
    from wmar_amd.models.tokenizer_train import _half_of
    cfg, _, _, tok = _setup()
    (out64, gx64, g64), (out32, gx32, g32) = _reference(half, B)
    x, r = _inputs(cfg, half, B)
    for p in tok.parameters():
        p.grad = None
    xc = x.cuda().requires_grad_(True)
    out = tok.encode_prequant(xc) if half == 0 else tok.decode(xc)
    (out * r.cuda()).sum().backward()
    got = {k: p.grad.clone() for k, p in tok.named_parameters() if _half_of(k) == half}
    assert set(got) == set(g64)
    worst, bad = 0.0, []
    for k, a, e64, e32 in [("input", xc.grad, gx64, gx32)] + [(k, got[k], g64[k], g32[k]) for k in g64]:
        scale = e64.abs().max()
        e = float((a.detach().cpu().double() - e64).abs().max() / scale)
        b = float((e32.double() - e64).abs().max() / scale)
        print("VQTRAIN chameleon_small %s B=%d %s err=%.3g torch_fp32=%.3g ratio=%.3g" % (("enc", "dec")[half], B, k, e, b, e / b), flush=True)
        worst = max(worst, e / b)
        if not e <= GATE * b:
            bad.append((k, e, b))
    e_out = float((out.detach().cpu().double() - out64).abs().max() / out64.abs().max())
    print("VQTRAIN chameleon_small %s B=%d worst_ratio=%.3g forward_err=%.3g" % (("enc", "dec")[half], B, worst, e_out), flush=True)
    assert not bad, "beyond %g x torch fp32: %s" % (GATE, bad)


def _flavours():
    from wmar_amd.models.tokenizer_train import MaskgitTrainableTokenizer, TrainableTokenizer
    from wmar_amd.utils import synth
    vq = synth.VQConfig(**synth.HARNESS_VQ)
    mvq = synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16, num_embeddings=512)
    return {"taming": (TrainableTokenizer, vq, synth.synth_vq_state(vq, 7, "cpu"), vq.embed_dim),
            "maskgit": (MaskgitTrainableTokenizer, mvq, synth.synth_maskgit_state(mvq, 7, "cpu"), mvq.z_channels)}


@pytest.mark.parametrize("flavour", ["taming", "maskgit"])
def test_a_frozen_handle_refuses_the_backward_and_stays_usable(flavour):
    from wmar_amd import _lib
    cls, cfg, sd, E = _flavours()[flavour]
    state = {k: v.detach().to("cuda", torch.float32).contiguous() for k, v in sd.items()}
    assert not any(v.requires_grad for v in state.values())
    frozen = cls(cfg, state, max_batch=2, frozen=True)
    assert not any(v.requires_grad for v in state.values())             # frozen=True leaves requires_grad as it found it
    assert frozen._train is None and frozen._eval is not None
    taped = cls(cfg, {k: v.detach().clone() for k, v in state.items()}, max_batch=2)
    assert 0 < frozen.device_bytes < taped._train.device_bytes
    print("VQTRAIN %s device_bytes frozen=%d taped=%d" % (flavour, frozen.device_bytes, taped._train.device_bytes), flush=True)
    S, R = cfg.codes_size, cfg.resolution
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 3, R, R, generator=g) * 2 - 1).cuda()
    z = torch.randn(2, E, S, S, generator=g).cuda()
    pre, img = frozen.encode_prequant(x), frozen.decode(z)
    assert not pre.requires_grad and not img.requires_grad
    with torch.no_grad():
        assert torch.equal(pre, taped.encode_prequant(x)) and torch.equal(img, taped.decode(z))
    assert torch.equal(pre, taped.encode_prequant(x).detach()) and torch.equal(img, taped.decode(z).detach())
    eng = frozen._eval
    zr = torch.zeros(2, S, S, E, device="cuda")
    for name, gbuf in (("encode_backward", zr), ("decode_backward", torch.zeros_like(x))):
        with pytest.raises(_lib.WmarError, match="frozen"):
            eng.call(name, gbuf.data_ptr(), 2, None)
    key = next(k for k in state if k.startswith("encoder.") and k.endswith(".weight"))
    with pytest.raises(_lib.WmarError, match="frozen"):
        names = (_lib.C.c_char_p * 1)(key.encode())
        ptrs = (_lib.C.c_void_p * 1)(torch.zeros_like(state[key]).data_ptr())
        eng.call("get_grads", names, ptrs, 1, 0)
    assert torch.equal(frozen.encode_prequant(x), pre) and torch.equal(frozen.decode(z), img)       # still usable
    # a weight change reaches the frozen handle through set_weights, as it reaches the taped one
    with torch.no_grad():
        for k in state:
            if k.startswith(("encoder.", "decoder.")):
                state[k].mul_(1.01)
                taped.state[k].mul_(1.01)
    pre2, img2 = frozen.encode_prequant(x), frozen.decode(z)
    assert not torch.equal(pre2, pre) and not torch.equal(img2, img)
    assert torch.equal(pre2, taped.encode_prequant(x).detach()) and torch.equal(img2, taped.decode(z).detach())


def _small_wrapper(seed=0, max_batch=8):
    import finetune as cli
    from wmar_amd.models.chameleon_wrapper import ChameleonARMMWrapper
    c, v = cli.synthetic_chameleon_configs("chameleon_small")
    return ChameleonARMMWrapper.synthetic(c, v, seed=seed, max_batch=max_batch)


def test_the_chameleon_wrapper_trains_one_rcc_step():
    from wmar_amd import finetune as ft
    model = _small_wrapper()
    tokenizer = model.get_image_tokenizer()
    before = {k: v.detach().clone() for k, v in tokenizer.state_dict().items()}
    codes = torch.randint(0, model._vq_cfg.n_embed, (2, model.codes_size ** 2), generator=torch.Generator().manual_seed(3)).cuda()
    model.vq_engine                                           # a packed engine exists: training must drop it
    assert model._vq_engine is not None
    tok = model.trainable_tokenizer(max_batch=2)
    assert all(tok.state[k] is tokenizer.state_dict()[k] for k in before)
    params = list(tok.parameters(("encoder.", "decoder.")))
    opt = torch.optim.Adam(params, lr=1e-3)
    loss, res, log, _ = ft.rcc_loss(tok, codes, [], loss_weight=1.0, orig=None)
    loss.backward()
    assert ft.calculate_gradient_norm(tok, "encoder.") > 0 and ft.calculate_gradient_norm(tok, "decoder.") > 0
    opt.step()
    loss2, *_ = ft.rcc_loss(tok, codes, [], loss_weight=1.0, orig=None)
    assert model._vq_engine is None                           # on_change dropped the packed engine
    assert torch.isfinite(loss2) and float(loss2.detach()) != float(loss.detach())
    moved = [k for k, v in tokenizer.state_dict().items() if k.startswith(("encoder.", "decoder.")) and not torch.equal(v.detach(), before[k])]
    assert moved
    assert torch.equal(tokenizer.state_dict()["quantize.embedding.weight"].detach(), before["quantize.embedding.weight"])
    imgs = model.codes_to_images(model.translation.convert_img2bp2(codes).to(torch.int64))
    assert model.images_to_codes(imgs).shape == codes.shape


def test_finetune_cli_trains_chameleon_and_its_deltas_reproduce_the_trained_state(tmp_path, capsys):
    import finetune as cli
    import wmar_amd.finetune as ft
    from wmar_amd.utils.utils import update_weights
    out = tmp_path / "ft"
    trained = {}
    orig_save = ft.save_delta

    def spy(trained_state, original_state, path):
        trained[path] = {k: v.detach().clone() for k, v in trained_state.items()}
        return orig_save(trained_state, original_state, path)

    ft.save_delta = spy
    try:
        assert cli.main("--model chameleon7b --synthetic --synthetic_config chameleon_small --dataset_size 4 --batch_size_per_gpu 2 --nb_epochs 1 "
                        "--augs none --optimizer adam --lr 1e-4 --idempotence_loss_weight 1.0 --idempotence_loss_weight_factor 1.0 "
                        f"--synthetic_lpips --outdir {out} --seed 0".split()) == 0
    finally:
        ft.save_delta = orig_save
    lines = [__import__("json").loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert sum("step" in l for l in lines) == 2 and all("rec_loss_perceptual_component" in l for l in lines if "step" in l)
    enc, dec = out / "encoder_ft_delta.pth", out / "decoder_ft_delta.pth"
    assert enc.exists() and dec.exists()
    model = _small_wrapper(seed=0)
    zeros = torch.zeros(1, 3, 128, 128, device="cuda")
    before = model.images_to_codes(zeros)
    tokenizer = model.get_image_tokenizer()
    update_weights(tokenizer.encoder, str(enc), delta=True)
    update_weights(tokenizer.decoder, str(dec), delta=True)
    moved = 0.0
    for name, path in (("encoder", enc), ("decoder", dec)):
        for k, v in trained[str(path)].items():
            assert torch.allclose(getattr(tokenizer, name).state_dict()[k], v, rtol=0, atol=1e-6), (name, k)
        moved += sum(float(v.abs().max()) for v in torch.load(str(path)).values())
    assert moved > 0
    after = model.images_to_codes(zeros)
    assert after.shape == before.shape and set(after.flatten().tolist()) <= set(model.vocab.image_tokens)
