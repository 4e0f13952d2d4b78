"""MI355X: RAR's MaskGIT-VQGAN through the taped training engine (wmar_mvq_train_create, MaskgitTrainableTokenizer) -- forwards
bit-equal to the inference engine, gradients against float64 CPU autograd of the restated network (tests/mvq_grad_reference.py), the
three new backward kernels alone, tape and weight behaviour, the rcc_loss chain and the CLI.

Gradient gate, as tests/test_gpu_vq_train.py: per tensor, |got - g64|_inf / |g64|_inf <= 8 x the same figure of torch's fp32 CPU
autograd of the same walkers, measured in the same run.  The ratios are printed on lines starting with MVQTRAIN (run with -s).

The clamp of ``decode`` (clamp(v, 0, 1) * 2 - 1) has a gradient that jumps at v = 0 and v = 1: a pixel whose v sits on a bound can fall
on different sides in fp32 and in float64, which is no numerical error.  The decode-half test therefore zeroes the cotangent, for all
three runs, where the float64 v lies within 1e-3 of a bound (the fp32 forward error of v is about 4e-6), and asserts on the reference
alone that this removes at most 1 % of the pixels and that 20-80 % of them lie strictly inside (0, 1).  The rcc_loss chain cannot be
masked that way; its test asserts that no float64 v of its codes lies within 1e-4 of a bound."""
import functools

import pytest
import torch

from tests import mvq_grad_reference as M

pytestmark = pytest.mark.gpu

GATE = 8.0
STATE_SEED = 5


def _cfgs():
    from wmar_amd.utils import synth
    return {"small": synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16,
                                           num_embeddings=512),
            "wide": synth.MaskgitVQConfig(hidden_channels=64, channel_mult=(1, 1, 2), num_res_blocks=2, resolution=32, z_channels=32,
                                          num_embeddings=512)}


def _sd(cfg, seed):
    from wmar_amd.utils import synth
    return synth.synth_maskgit_state(cfg, seed, "cpu")


def _state(cfg, seed):
    sd = _sd(cfg, seed)
    return sd, {k: v.detach().to("cuda", torch.float32).contiguous() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _setup(name):
    from wmar_amd.models.tokenizer_train import MaskgitTrainableTokenizer
    cfg = _cfgs()[name]
    sd, state = _state(cfg, STATE_SEED)
    return cfg, sd, state, MaskgitTrainableTokenizer(cfg, state, max_batch=2)


@functools.lru_cache(maxsize=None)
def _inputs(name, half, B, seed=0):
    """(x, r, clamp shares): half 0 images in [-1, 1] and a cotangent of the code vectors; half 1 randn latents and an image cotangent
    zeroed where the float64 value in front of the clamp lies within 1e-3 of 0 or 1."""
    cfg = _cfgs()[name]
    g = torch.Generator().manual_seed(seed + 10 * half + B)
    S, R = cfg.codes_size, cfg.resolution
    if half == 0:
        return torch.rand(B, 3, R, R, generator=g) * 2 - 1, torch.randn(B, cfg.z_channels, S, S, generator=g), None
    x = torch.randn(B, cfg.z_channels, S, S, generator=g)
    r = torch.randn(B, 3, R, R, generator=g)
    with torch.no_grad():
        v = M.decode_preclamp({k: t.double() for k, t in _sd(cfg, STATE_SEED).items()}, cfg, x.double())
    near = ((v.abs() <= 1e-3) | ((v - 1).abs() <= 1e-3))
    inside = (v > 0) & (v < 1)
    r = torch.where(near, torch.zeros_like(r), r)
    return x, r, (float(near.double().mean()), float(inside.double().mean()))


@functools.lru_cache(maxsize=None)
def _reference(name, half, B):
    cfg, sd, _, _ = _setup(name)
    x, r, _ = _inputs(name, half, B)
    return M.half_gradients(sd, cfg, half, x, r, torch.float64), M.half_gradients(sd, cfg, half, x, r, torch.float32)


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
@pytest.mark.parametrize("name", ["small", "wide"])
def test_forwards_are_bit_equal_to_the_inference_engine(name, B):
    from wmar_amd.models.engine import MaskgitVQEngine
    cfg, _, state, tok = _setup(name)
    eng = MaskgitVQEngine(cfg, state, max_batch=2)
    x, _, _ = _inputs(name, 0, B, seed=3)
    codes = torch.randint(0, cfg.num_embeddings, (B, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(B)).cuda()
    _, pre = eng.encode(x.cuda(), return_prequant=True)
    with torch.no_grad():
        mine_eval = tok.encode_prequant(x.cuda())
        img_eval = tok.decode(tok.embed(codes))
    mine = tok.encode_prequant(x.cuda())                      # the taped engine
    img = tok.decode(tok.embed(codes))
    assert mine.requires_grad and img.requires_grad and not mine_eval.requires_grad
    assert {k.split(".")[0] for k, _ in tok.named_parameters()} == {"encoder", "decoder"}
    for m in (mine, mine_eval):
        assert torch.equal(m.detach().permute(0, 2, 3, 1).reshape(-1, cfg.z_channels), pre)
    want = eng.decode(codes)
    for i in (img, img_eval):
        assert torch.equal(i.detach(), want)
    assert float(want.min()) == -1.0 and float(want.max()) == 1.0          # the clamp works on both sides


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("half", [0, 1], ids=["encoder", "decoder"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_gradients_against_float64_autograd(name, half, B):
    cfg, _, _, tok = _setup(name)
    x, r, shares = _inputs(name, half, B)
    if half == 1:
        print("MVQTRAIN %s dec B=%d zeroed_share=%.4f inside_share=%.3f" % (name, B, shares[0], shares[1]), flush=True)
        assert shares[0] <= 0.01 and 0.2 <= shares[1] <= 0.8
    (out64, gx64, g64), (out32, gx32, g32) = _reference(name, half, B)
    _clear(tok)
    out, gx = _run(tok, half, x, r)
    got = _grads(tok, half)
    assert set(got) == set(g64)
    assert not any(k.endswith(("conv1.bias", "conv2.bias", "nin_shortcut.bias", "encoder.conv_in.bias")) for k in got)
    worst, bad = 0.0, []
    for k, a, e64, e32 in [("input", gx, gx64, gx32)] + [(k, got[k], g64[k], g32[k]) for k in g64]:
        scale = e64.abs().max()
        e = float((a.detach().cpu().double() - e64).abs().max() / scale)
        b = float((e32.double() - e64).abs().max() / scale)
        print("MVQTRAIN %s %s B=%d %s err=%.3g torch_fp32=%.3g ratio=%.3g" % (name, ("enc", "dec")[half], B, k, e, b, e / b), flush=True)
        worst = max(worst, e / b)
        if not e <= GATE * b:
            bad.append((k, e, b))
    e_out = float((out.cpu().double() - out64).abs().max() / out64.abs().max())
    print("MVQTRAIN %s %s B=%d worst_ratio=%.3g forward_err=%.3g" % (name, ("enc", "dec")[half], B, worst, e_out), flush=True)
    assert not bad, "beyond %g x torch fp32: %s" % (GATE, bad)


def _check_avgpool_backward(B, Ho, Wo, Cc):
    import torch.nn.functional as F
    from wmar_amd import _lib
    g = torch.Generator().manual_seed(0)
    gy = torch.randn(B, Ho, Wo, Cc, generator=g)               # NHWC
    x = torch.randn(B, Cc, 2 * Ho, 2 * Wo, generator=g).requires_grad_(True)
    (F.avg_pool2d(x, kernel_size=2, stride=2) * gy.permute(0, 3, 1, 2)).sum().backward()
    gyd = gy.cuda().contiguous()
    gx = torch.full((B, 2 * Ho, 2 * Wo, Cc), float("nan"), device="cuda")
    _lib.check(_lib.load().wmar_vq_probe_avgpool_backward(gyd.data_ptr(), B, Ho, Wo, Cc, gx.data_ptr(), _lib.stream_ptr(gx.device)))
    assert torch.equal(gx.cpu().permute(0, 3, 1, 2), x.grad)


def test_avgpool_backward_probe_is_bit_equal_to_torch():
    _check_avgpool_backward(2, 8, 8, 32)


def test_avgpool_backward_probe_non_square_with_nine_channel_quads():
    """Ho != Wo (the kernel divides a pixel index by 2 Wo and indexes the window with Wo) and C / 4 = 9, not a power of two."""
    _check_avgpool_backward(2, 8, 12, 36)


def test_image_edge_backward_probes_are_bit_equal_to_torch():
    from wmar_amd import _lib
    L = _lib.load()
    B, Cc, H, Cs = 2, 3, 16, 8
    g = torch.Generator().manual_seed(1)
    v = torch.rand(B, Cc, H, H, generator=g) * 2 - 0.5          # about half inside (0, 1)
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    special = [0.0, 1.0, -0.0, float(torch.nextafter(zero, -one)), float(torch.nextafter(one, 2 * one)), float(torch.nextafter(zero, one)),
               float(torch.nextafter(one, zero)), -1e-3, 1.001]
    v.view(-1)[:len(special)] = torch.tensor(special)
    v.view(-1)[-len(special):] = torch.tensor(special)
    gi = torch.randn(B, Cc, H, H, generator=g)
    vr = v.clone().requires_grad_(True)
    ((torch.clamp(vr, 0.0, 1.0) * 2.0 - 1.0) * gi).sum().backward()
    want = vr.grad
    assert float(want.view(-1)[0]) == 2 * float(gi.view(-1)[0]) and float(want.view(-1)[1]) == 2 * float(gi.view(-1)[1])      # on a bound: passes
    assert float(want.view(-1)[3]) == 0.0 and float(want.view(-1)[4]) == 0.0                                             # just outside
    pre = torch.full((B, H * H, Cs), 0.5)                       # padding channels hold in-range values: their gradient is still 0
    pre[:, :, :Cc] = v.view(B, Cc, H * H).permute(0, 2, 1)
    pre_d, gi_d = pre.cuda().contiguous(), gi.cuda().contiguous()
    out = torch.full((B, H * H, Cs), float("nan"), device="cuda")
    _lib.check(L.wmar_mvq_probe_image_backward(pre_d.data_ptr(), gi_d.data_ptr(), B, Cc, H * H, Cs, out.data_ptr(), _lib.stream_ptr(out.device)))
    out = out.cpu()
    assert torch.equal(out[:, :, :Cc].permute(0, 2, 1).reshape(B, Cc, H, H), want)
    assert torch.equal(out[:, :, Cc:], torch.zeros(B, H * H, Cs - Cc))
    # encode edge: (x + 1) / 2
    gn = torch.randn(B, H * H, Cs, generator=g)
    xr = torch.randn(B, Cc, H, H, generator=g).requires_grad_(True)
    (((xr + 1.0) / 2.0) * gn[:, :, :Cc].permute(0, 2, 1).reshape(B, Cc, H, H)).sum().backward()
    gn_d = gn.cuda().contiguous()
    gx = torch.full((B, Cc, H, H), float("nan"), device="cuda")
    _lib.check(L.wmar_mvq_probe_input_backward(gn_d.data_ptr(), B, Cc, H * H, Cs, gx.data_ptr(), _lib.stream_ptr(gx.device)))
    assert torch.equal(gx.cpu(), xr.grad)


@pytest.mark.parametrize("half", [0, 1], ids=["encoder", "decoder"])
def test_backward_is_bit_reproducible_and_grad_accumulates(half):
    cfg, _, _, tok = _setup("small")
    x, r, _ = _inputs("small", half, 2)
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
    cfg, _, _, tok = _setup("small")
    (xe, re_, _), (xd, rd, _) = _inputs("small", 0, 2), _inputs("small", 1, 2)
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
    cfg, _, _, tok = _setup("small")
    xe, re_, _ = _inputs("small", 0, 2)
    o1 = tok.encode_prequant(xe.cuda())
    tok.encode_prequant(xe.cuda() * 0.5)
    with pytest.raises(RuntimeError, match="last forward"):
        (o1 * re_.cuda()).sum().backward()
    with pytest.raises(ValueError, match="max_batch"):
        tok.encode_prequant(torch.zeros(3, 3, cfg.resolution, cfg.resolution, device="cuda"))


def test_in_place_weight_change_is_repacked_and_drops_the_inference_engine():
    from wmar_amd.models.engine import MaskgitVQEngine
    from wmar_amd.models.tokenizer_train import MaskgitTrainableTokenizer
    cfg = _cfgs()["small"]
    _, state = _state(cfg, 6)
    dropped = []
    tok = MaskgitTrainableTokenizer(cfg, state, max_batch=2, on_change=lambda: dropped.append(1))
    x, r, _ = _inputs("small", 0, 2)
    z, rz, _ = _inputs("small", 1, 2)
    _run(tok, 0, x, r)
    _run(tok, 1, z, rz)
    opt = torch.optim.Adam(list(tok.parameters()), lr=1e-3, betas=(0.9, 0.999))
    opt.step()
    assert not dropped
    pre = tok.encode_prequant(x.cuda())
    img = tok.decode(z.cuda())
    assert dropped == [1]
    fresh = MaskgitTrainableTokenizer(cfg, state, max_batch=2)
    with torch.no_grad():
        assert torch.equal(pre.detach(), fresh.encode_prequant(x.cuda())) and torch.equal(img.detach(), fresh.decode(z.cuda()))
    _, pre_inf = MaskgitVQEngine(cfg, state, max_batch=2).encode(x.cuda(), return_prequant=True)
    assert torch.equal(pre.detach().permute(0, 2, 3, 1).reshape(-1, cfg.z_channels), pre_inf)


def test_error_returns_leave_the_engine_usable():
    from wmar_amd import _lib
    from wmar_amd.models.tokenizer_train import MaskgitTrainableTokenizer
    cfg = _cfgs()["small"]
    _, state = _state(cfg, 7)
    tok = MaskgitTrainableTokenizer(cfg, state, max_batch=2)
    eng = tok._train
    S, R, E = cfg.codes_size, cfg.resolution, cfg.z_channels
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
    scratch = torch.zeros(64, device="cuda")
    with pytest.raises(_lib.WmarError, match="no backward"):
        names = (_lib.C.c_char_p * 1)(b"encoder.conv_in.weight")
        ptrs = (_lib.C.c_void_p * 1)(state["encoder.conv_in.weight"].data_ptr())
        eng.call("get_grads", names, ptrs, 1, 0)
    eng.call("encode_backward", z.data_ptr(), 2, None)
    for missing in (b"encoder.conv_in.bias", b"encoder.down.1.block.0.nin_shortcut.bias", b"encoder.mid.0.conv1.bias"):
        with pytest.raises(_lib.WmarError, match=missing.decode() + "' is not a trainable tensor"):
            eng.call("get_grads", (_lib.C.c_char_p * 1)(missing), (_lib.C.c_void_p * 1)(scratch.data_ptr()), 1, 0)
    eng.call("get_grads", (_lib.C.c_char_p * 1)(b"encoder.conv_out.bias"), (_lib.C.c_void_p * 1)(scratch.data_ptr()), 1, 0)      # this one exists
    names, ptrs, n = _lib.tensor_table(tok._tensors())
    eng.call("set_weights", names, ptrs, n)
    for name, g in (("encode_backward", z), ("decode_backward", x)):
        with pytest.raises(_lib.WmarError, match="no tape"):
            eng.call(name, g.data_ptr(), 2, None)
    xi, r, _ = _inputs("small", 0, 2)
    _, gx = _run(tok, 0, xi, r)                                # still usable
    assert torch.isfinite(gx).all() and all(p.grad is not None for p in tok.parameters("encoder."))


RCC_CODE_SEED = 15


@pytest.mark.parametrize("aug", ["none", "hflip"])
def test_rcc_chain_gradients_against_the_float64_chain(aug):
    """decode -> (flip) -> re-encode through ``rcc_loss``: every encoder and decoder weight gradient against the same loss on the
    float64 stand-in, gate as above, and the loss itself to 1e-5.  The clamp sits inside the chain: the codes are drawn (seed picked on
    the CPU) so that no float64 value in front of the clamp lies within 1e-4 of a bound."""
    import random
    from wmar_amd import finetune as ft
    from wmar_amd.augmentations.geometric import HorizontalFlip
    cfg, sd, _, tok = _setup("small")
    augs = [] if aug == "none" else [(HorizontalFlip, [None])]
    idx = torch.randint(0, cfg.num_embeddings, (2, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(RCC_CODE_SEED))
    refs = []
    for dtype in (torch.float64, torch.float32):
        t, o = M.TorchTokenizer(cfg, sd, dtype), M.TorchTokenizer(cfg, sd, dtype)
        if dtype == torch.float64:
            with torch.no_grad():
                v = M.decode_preclamp(t.state, cfg, t.embed(idx))
            assert float(torch.minimum(v.abs(), (v - 1).abs()).min()) > 1e-4
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
    print("MVQTRAIN rcc %s loss=%.9g ref=%.9g" % (aug, float(loss.detach()), float(refs[0][0])), flush=True)
    bad, worst = [], 0.0
    for k, p in tok.named_parameters():
        e64, e32 = refs[0][1][k], refs[1][1][k]
        scale = e64.abs().max()
        e, b = float((p.grad.cpu().double() - e64).abs().max() / scale), float((e32.double() - e64).abs().max() / scale)
        worst = max(worst, e / b)
        if not e <= GATE * b:
            bad.append((k, e, b))
    print("MVQTRAIN rcc %s worst_ratio=%.3g" % (aug, worst), flush=True)
    assert abs(float(loss.detach()) - float(refs[0][0])) <= 1e-5 * abs(float(refs[0][0]))
    assert not bad, "beyond %g x torch fp32: %s" % (GATE, bad)


def test_finetune_cli_writes_deltas_that_reproduce_the_trained_state(tmp_path):
    import finetune as cli
    import wmar_amd.finetune as ft
    from wmar_amd.models.rar_wrapper import RarARMMWrapper
    from wmar_amd.utils.utils import update_weights
    out = tmp_path / "ft"
    trained = {}
    orig_save = ft.save_delta

    def spy(trained_state, original_state, path):
        trained[path] = {k: v.detach().clone() for k, v in trained_state.items()}
        return orig_save(trained_state, original_state, path)

    ft.save_delta = spy
    try:
        assert cli.main("--model rar --synthetic --synthetic_config maskgit_small --dataset_size 4 --batch_size_per_gpu 2 --nb_epochs 1 --augs none "
                        "--optimizer adam --lr 1e-4 --idempotence_loss_weight 1.0 --idempotence_loss_weight_factor 1.0 "
                        f"--outdir {out} --seed 0".split()) == 0
    finally:
        ft.save_delta = orig_save
    enc, dec = out / "encoder_ft_delta.pth", out / "decoder_ft_delta.pth"
    assert enc.exists() and dec.exists()
    model = RarARMMWrapper.synthetic(*cli.synthetic_rar_configs("maskgit_small"), seed=0, max_batch=8)
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
