"""MI355X: the taped training engine (wmar_vq_train_*, wmar_amd/models/tokenizer_train.py) -- forwards bit-equal to the inference
engine, gradients against float64 CPU autograd of the restated network (tests/vq_grad_reference.py), tape and weight behaviour.

Gradient gate: per tensor, |got - g64|_inf / |g64|_inf <= 8 x the same figure of torch's fp32 CPU autograd of the same walkers,
measured in the same run (8 = twice the layer gate of tests/test_gpu_vq_grad_layers.py: the taped forward and the backward each
carry that slack).  The ratios are printed on lines starting with VQTRAIN (run with -s)."""
import functools

import pytest
import torch

from tests import vq_grad_reference as G

pytestmark = pytest.mark.gpu

GATE = 8.0


def _cfgs():
    from wmar_amd.utils import synth
    return {"harness": synth.VQConfig(**synth.HARNESS_VQ),
            "wide": synth.VQConfig(ch=64, ch_mult=(1, 2), num_res_blocks=2, attn_resolutions=(16,), resolution=32, z_channels=16, embed_dim=8,
                                   n_embed=512)}


@functools.lru_cache(maxsize=None)
def _setup(name):
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = _cfgs()[name]
    sd = synth.synth_vq_state(cfg, 5, "cpu")
    state = {k: v.detach().to("cuda", torch.float32).contiguous() for k, v in sd.items()}
    return cfg, sd, state, TrainableTokenizer(cfg, state, max_batch=2)


def _inputs(cfg, half, B, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * half + B)
    S, R = cfg.codes_size, cfg.resolution
    if half == 0:
        x = torch.rand(B, 3, R, R, generator=g) * 2 - 1
        r = torch.randn(B, cfg.embed_dim, S, S, generator=g)
    else:
        x = torch.randn(B, cfg.embed_dim, S, S, generator=g)
        r = torch.randn(B, 3, R, R, generator=g)
    return x, r


@functools.lru_cache(maxsize=None)
def _reference(name, half, B):
    cfg, sd, _, _ = _setup(name)
    x, r = _inputs(cfg, half, B)
    return G.half_gradients(sd, cfg, half, x, r, torch.float64), G.half_gradients(sd, cfg, half, x, r, torch.float32)


def _run(tok, half, x, r):
    x = x.cuda().requires_grad_(True)
    out = tok.encode_prequant(x) if half == 0 else tok.decode(x)
    (out * r.cuda()).sum().backward()
    return out.detach(), x.grad


def _clear(tok):
    for p in tok.parameters():
        p.grad = None


def _grads(tok, half):
    from wmar_amd.models.tokenizer_train import _half_of
    return {k: p.grad.clone() for k, p in tok.named_parameters() if _half_of(k) == half}


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("name", ["harness", "wide"])
def test_forwards_are_bit_equal_to_the_inference_engine(name, B):
    from wmar_amd.models.engine import VQGANEngine
    cfg, _, state, tok = _setup(name)
    eng = VQGANEngine(cfg, state, max_batch=2)
    x, _ = _inputs(cfg, 0, B, seed=3)
    codes = torch.randint(0, cfg.n_embed, (B, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(B)).cuda()
    _, pre = eng.encode(x.cuda(), return_prequant=True)
    with torch.no_grad():
        mine_eval = tok.encode_prequant(x.cuda())
        img_eval = tok.decode(tok.embed(codes))
    mine = tok.encode_prequant(x.cuda())                      # the taped engine
    img = tok.decode(tok.embed(codes))
    assert mine.requires_grad and img.requires_grad and not mine_eval.requires_grad
    for m in (mine, mine_eval):
        assert torch.equal(m.detach().permute(0, 2, 3, 1).reshape(-1, cfg.embed_dim), pre)
    want = eng.decode(codes)
    for i in (img, img_eval):
        assert torch.equal(i.detach().clamp(-1, 1), want)


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("half", [0, 1], ids=["encoder", "decoder"])
@pytest.mark.parametrize("name", ["harness", "wide"])
def test_gradients_against_float64_autograd(name, half, B):
    cfg, _, _, tok = _setup(name)
    (out64, gx64, g64), (out32, gx32, g32) = _reference(name, half, B)
    x, r = _inputs(cfg, half, B)
    _clear(tok)
    out, gx = _run(tok, half, x, r)
    got = _grads(tok, half)
    assert set(got) == set(g64)
    worst, bad = 0.0, []
    for k, a, e64, e32 in [("input", gx, gx64, gx32)] + [(k, got[k], g64[k], g32[k]) for k in g64]:
        scale = e64.abs().max()
        e = float((a.detach().cpu().double() - e64).abs().max() / scale)
        b = float((e32.double() - e64).abs().max() / scale)
        print("VQTRAIN %s %s B=%d %s err=%.3g torch_fp32=%.3g ratio=%.3g" % (name, ("enc", "dec")[half], B, k, e, b, e / b), flush=True)
        worst = max(worst, e / b)
        if not e <= GATE * b:
            bad.append((k, e, b))
    e_out = float((out.cpu().double() - out64).abs().max() / out64.abs().max())
    print("VQTRAIN %s %s B=%d worst_ratio=%.3g forward_err=%.3g" % (name, ("enc", "dec")[half], B, worst, e_out), flush=True)
    assert not bad, "beyond %g x torch fp32: %s" % (GATE, bad)


@pytest.mark.parametrize("half", [0, 1], ids=["encoder", "decoder"])
def test_backward_is_bit_reproducible_and_grad_accumulates(half):
    cfg, _, _, tok = _setup("harness")
    x, r = _inputs(cfg, half, 2)
    _clear(tok)
    _, gx1 = _run(tok, half, x, r)
    g1 = _grads(tok, half)
    _, gx2 = _run(tok, half, x, r)                            # .grad now holds both
    for k, v in _grads(tok, half).items():
        assert torch.equal(v, g1[k] + g1[k]), k
    _clear(tok)
    _, gx3 = _run(tok, half, x, r)
    assert torch.equal(gx1, gx2) and torch.equal(gx1, gx3)
    for k, v in _grads(tok, half).items():
        assert torch.equal(v, g1[k]), k


def test_a_tape_survives_the_other_half_and_no_grad_forwards():
    cfg, _, _, tok = _setup("harness")
    (xe, re_), (xd, rd) = _inputs(cfg, 0, 2), _inputs(cfg, 1, 2)
    _clear(tok)
    _run(tok, 0, xe, re_)
    _run(tok, 1, xd, rd)
    want = {**_grads(tok, 0), **_grads(tok, 1)}
    _clear(tok)
    a, b = xe.cuda().requires_grad_(True), xd.cuda().requires_grad_(True)
    oe = tok.encode_prequant(a)
    od = tok.decode(b)
    with torch.no_grad():                                      # neither touches a tape
        tok.encode_prequant(torch.zeros_like(a))
        tok.decode(torch.ones_like(b))
    (od * rd.cuda()).sum().backward()
    (oe * re_.cuda()).sum().backward()
    for k, p in tok.named_parameters():
        assert torch.equal(p.grad, want[k]), k


def test_a_backward_of_a_replaced_tape_raises():
    cfg, _, _, tok = _setup("harness")
    xe, re_ = _inputs(cfg, 0, 2)
    o1 = tok.encode_prequant(xe.cuda())
    tok.encode_prequant(xe.cuda() * 0.5)
    with pytest.raises(RuntimeError, match="last forward"):
        (o1 * re_.cuda()).sum().backward()
    with pytest.raises(ValueError, match="max_batch"):
        tok.encode_prequant(torch.zeros(3, 3, cfg.resolution, cfg.resolution, device="cuda"))


def test_in_place_weight_change_is_repacked_and_drops_the_inference_engine():
    from wmar_amd.models.engine import VQGANEngine
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = _cfgs()["harness"]
    state = {k: v.to("cuda", torch.float32).contiguous() for k, v in synth.synth_vq_state(cfg, 6, "cpu").items()}
    dropped = []
    tok = TrainableTokenizer(cfg, state, max_batch=2, on_change=lambda: dropped.append(1))
    x, r = _inputs(cfg, 0, 2)
    z, rz = _inputs(cfg, 1, 2)
    _run(tok, 0, x, r)
    _run(tok, 1, z, rz)
    opt = torch.optim.Adam(list(tok.parameters()), lr=1e-3, betas=(0.9, 0.999))
    opt.step()
    assert not dropped
    pre = tok.encode_prequant(x.cuda())
    img = tok.decode(z.cuda())
    assert dropped == [1]
    fresh = TrainableTokenizer(cfg, state, max_batch=2)
    with torch.no_grad():
        assert torch.equal(pre.detach(), fresh.encode_prequant(x.cuda())) and torch.equal(img.detach(), fresh.decode(z.cuda()))
    _, pre_inf = VQGANEngine(cfg, state, max_batch=2).encode(x.cuda(), return_prequant=True)
    assert torch.equal(pre.detach().permute(0, 2, 3, 1).reshape(-1, cfg.embed_dim), pre_inf)


def test_error_returns_leave_the_engine_usable():
    from wmar_amd import _lib
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    cfg = _cfgs()["harness"]
    state = {k: v.to("cuda", torch.float32).contiguous() for k, v in synth.synth_vq_state(cfg, 7, "cpu").items()}
    tok = TrainableTokenizer(cfg, state, max_batch=2)
    eng = tok._train
    S, R, E = cfg.codes_size, cfg.resolution, cfg.embed_dim
    x = torch.zeros(2, 3, R, R, device="cuda")
    z = torch.zeros(2, S, S, E, device="cuda")
    for name, g in (("encode_backward", z), ("decode_backward", x)):
        with pytest.raises(_lib.WmarError, match="no tape"):
            eng.call(name, g.data_ptr(), 2, None)
    eng.call("encode", x.data_ptr(), 2, z.data_ptr())
    eng.call("decode", z.data_ptr(), 2, x.data_ptr())
    with pytest.raises(_lib.WmarError, match="the tape holds 2"):
        eng.call("encode_backward", z.data_ptr(), 1, None)
    with pytest.raises(_lib.WmarError, match="null argument"):
        eng.call("decode_backward", None, 2, None)
    with pytest.raises(_lib.WmarError, match="no backward"):
        names = (_lib.C.c_char_p * 1)(b"quant_conv.weight")
        ptrs = (_lib.C.c_void_p * 1)(state["quant_conv.weight"].data_ptr())
        eng.call("get_grads", names, ptrs, 1, 0)
    names, ptrs, n = _lib.tensor_table(tok._tensors())
    eng.call("set_weights", names, ptrs, n)
    for name, g in (("encode_backward", z), ("decode_backward", x)):
        with pytest.raises(_lib.WmarError, match="no tape"):
            eng.call(name, g.data_ptr(), 2, None)
    xi, r = _inputs(cfg, 0, 2)
    _, gx = _run(tok, 0, xi, r)                                # still usable
    assert torch.isfinite(gx).all() and all(p.grad is not None for p in tok.parameters("encoder."))


@pytest.mark.parametrize("aug", ["none", "hflip"])
def test_rcc_chain_gradients_against_the_float64_chain(aug):
    """decode -> (flip) -> re-encode through ``rcc_loss``: every encoder and decoder weight gradient against the same loss on a float64
    stand-in tokenizer, gate as above.  The loss reads the re-encoded vectors before the quantizer, so the hard indices (reported
    in res_dict only) cannot move a gradient."""
    import random
    from wmar_amd import finetune as ft
    from wmar_amd.augmentations.geometric import HorizontalFlip
    cfg, sd, _, tok = _setup("harness")
    augs = [] if aug == "none" else [(HorizontalFlip, [None])]
    idx = torch.randint(0, cfg.n_embed, (2, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(11))
    refs = []
    for dtype in (torch.float64, torch.float32):
        t, o = G.TorchTokenizer(cfg, sd, dtype), G.TorchTokenizer(cfg, sd, dtype)
        random.seed(0)
        loss, _, _, was = ft.rcc_loss(t, idx, augs, p=1.0, loss_weight=2.0, orig=o)
        assert was == (aug != "none")
        loss.backward()
        refs.append((loss.detach(), {k: v.grad for k, v in t.named_parameters()}))
    _clear(tok)
    random.seed(0)
    loss, res, _, was = ft.rcc_loss(tok, idx.cuda(), augs, p=1.0, loss_weight=2.0, orig=tok)
    assert was == (aug != "none") and res["rec_z_indices"].shape == idx.shape
    loss.backward()
    assert abs(float(loss.detach()) - float(refs[0][0])) <= 1e-5 * abs(float(refs[0][0]))
    bad, worst = [], 0.0
    for k, p in tok.named_parameters():
        e64, e32 = refs[0][1][k], refs[1][1][k]
        scale = e64.abs().max()
        e, b = float((p.grad.cpu().double() - e64).abs().max() / scale), float((e32.double() - e64).abs().max() / scale)
        worst = max(worst, e / b)
        if not e <= GATE * b:
            bad.append((k, e, b))
    print("VQTRAIN rcc %s worst_ratio=%.3g" % (aug, worst), flush=True)
    assert not bad, "beyond %g x torch fp32: %s" % (GATE, bad)


def test_finetune_cli_writes_deltas_that_reproduce_the_trained_state(tmp_path):
    import finetune as cli
    from wmar_amd.models.taming_wrapper import TamingARMMWrapper
    from wmar_amd.utils import synth
    from wmar_amd.utils.utils import update_weights
    out = tmp_path / "ft"
    trained = {}
    import wmar_amd.finetune as ft
    orig_save = ft.save_delta

    def spy(trained_state, original_state, path):
        trained[path] = {k: v.detach().clone() for k, v in trained_state.items()}
        return orig_save(trained_state, original_state, path)

    ft.save_delta = spy
    try:
        assert cli.main("--model taming --synthetic --synthetic_config harness --dataset_size 4 --batch_size_per_gpu 2 --nb_epochs 1 --augs none "
                        "--optimizer adam --lr 1e-4 --idempotence_loss_weight 1.0 --idempotence_loss_weight_factor 1.0 "
                        f"--outdir {out} --seed 0".split()) == 0
    finally:
        ft.save_delta = orig_save
    enc, dec = out / "encoder_ft_delta.pth", out / "decoder_ft_delta.pth"
    assert enc.exists() and dec.exists()
    model = TamingARMMWrapper.synthetic(synth.GPTConfig(**synth.HARNESS_GPT), synth.VQConfig(**synth.HARNESS_VQ), seed=0, max_batch=8)
    before = model.images_to_codes(torch.zeros(1, 3, 32, 32, device="cuda"))
    tokenizer = model.get_image_tokenizer()
    update_weights(tokenizer.encoder, str(enc), delta=True)
    update_weights(tokenizer.decoder, str(dec), delta=True)
    moved = 0.0
    for name, path in (("encoder", enc), ("decoder", dec)):
        for k, v in trained[str(path)].items():
            cur = getattr(tokenizer, name).state_dict()[k]
            assert torch.allclose(cur, v, rtol=0, atol=1e-6), (name, k)
        moved += sum(float(v.abs().max()) for v in torch.load(str(path)).values())
    assert moved > 0
    after = model.images_to_codes(torch.zeros(1, 3, 32, 32, device="cuda"))
    assert after.shape == before.shape
