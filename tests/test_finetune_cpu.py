"""CPU: the fine-tuning CLI's parser and refusals, and ``rcc_loss`` / the training loop / the delta files driven by a pure-torch
stand-in tokenizer built from the walkers of tests/vq_grad_reference.py."""
import argparse
import math
import random

import pytest
import torch

import finetune as cli
from tests import vq_grad_reference as G
from wmar_amd import finetune as ft
from wmar_amd.utils import synth


TorchTokenizer = G.TorchTokenizer


@pytest.fixture(scope="module")
def small():
    cfg = synth.VQConfig(**dict(synth.HARNESS_VQ, n_embed=64))
    return cfg, synth.synth_vq_state(cfg, 2, "cpu")


def test_parser_takes_the_reference_flags_and_refuses_what_is_not_built():
    p = cli.build_parser()
    a = p.parse_args("--model taming --synthetic --synthetic_config harness --datapath c.pt --dataset_size 4 --mode newenc-dec --nb_epochs 2 "
                     "--augs all+geom --augs_schedule 1,1 --optimizer adam --lr 1e-4 --batch_size_per_gpu 2 --idempotence_loss_weight 2.0 "
                     "--idempotence_loss_weight_factor 0.5 --loss hard-to-soft-with-ae --outdir out --seed 3".split())
    cli.check_args(a)
    assert (a.nb_epochs, a.augs_schedule, a.lr, a.idempotence_loss_weight_factor, a.seed) == (2, "1,1", 1e-4, 0.5, 3)
    base = "--synthetic --outdir out "
    for extra, word in (("--model rar", "rar"), ("--model chameleon7b", "chameleon7b"), ("--local_rank 0", "DDP"), ("--tensorboard", "tensorboard"),
                        ("--validate", "validation"), ("--mode other", "mode"), ("--loss l2", "loss"), ("--optimizer sgd", "optimizer"),
                        ("--modelpath m", "exactly one")):
        with pytest.raises(SystemExit, match=word):
            cli.check_args(p.parse_args((base + extra).split()))
    with pytest.raises(SystemExit, match="datapath"):
        cli.check_args(p.parse_args("--modelpath m --outdir out".split()))


def test_idempotence_regions_match_a_direct_restatement():
    from wmar_amd.augmentations.geometric import HorizontalFlip, Rotate, UpperLeftCropWithPadBack
    for S in (8, 16, 32):
        z = torch.arange(S * S, dtype=torch.float32).view(1, 1, S, S)
        skip = S // 8
        r = ft.idempotence_region(S, (Rotate, 10))
        assert torch.equal(z[:, :, r, r], z[:, :, skip:-skip, skip:-skip])
        for prm in (0.5, 0.7, 0.95):
            cutoff = int(torch.floor(torch.tensor(S) * prm).int())
            r = ft.idempotence_region(S, (UpperLeftCropWithPadBack, prm))
            assert torch.equal(z[:, :, r, r], z[:, :, :cutoff, :cutoff])
        for applied in (None, (HorizontalFlip, None)):
            r = ft.idempotence_region(S, applied)
            assert torch.equal(z[:, :, r, r], z)


def test_rcc_loss_without_augmentation_is_the_written_out_loss(small):
    cfg, sd = small
    tok, orig = TorchTokenizer(cfg, sd), TorchTokenizer(cfg, sd)
    with torch.no_grad():
        for _, prm in tok.named_parameters("decoder."):
            prm.add_(0.01 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(prm.numel())))
    idx = torch.randint(0, cfg.n_embed, (2, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(0))
    loss, res, log, was = ft.rcc_loss(tok, idx, [], p=0.5, loss_weight=3.0, orig=orig)
    z_q = tok.embed(idx)
    xrec = tok.decode(z_q)
    want = (xrec - orig.decode(z_q)).abs().mean() + 3.0 * torch.mean((z_q - tok.encode_prequant(xrec)) ** 2)
    assert not was and torch.allclose(loss, want, rtol=1e-6, atol=0)
    assert set(res) == {"orig_z_q", "orig_z_indices", "rec_x", "rec_x_maybe_augmented", "rec_x_orig_decoder", "rec_z", "rec_z_q", "rec_z_indices"}
    assert res["rec_z_indices"].shape == idx.shape and log["loss_weight"] == 3.0 and math.isclose(log["loss"], float(want.detach()), rel_tol=1e-6)
    loss.backward()
    assert ft.calculate_gradient_norm(tok, "decoder.") > 0 and ft.calculate_gradient_norm(tok, "encoder.") > 0
    n = sum(p.numel() for p in tok.parameters("encoder."))
    assert math.isclose(ft.calculate_gradient_norm(tok, "encoder."), math.sqrt(sum(float(p.grad.norm()) ** 2 for p in tok.parameters("encoder.")) / n),
                        rel_tol=1e-9)
    custom, *_ = ft.rcc_loss(tok, idx, None, orig=orig, loss_weight=0.0, rec_loss=lambda a, b: ((a - b) ** 2).mean())
    assert torch.allclose(custom, ((xrec - orig.decode(z_q)) ** 2).mean(), rtol=1e-6, atol=0)


def test_training_loop_anneals_the_weight_and_the_deltas_round_trip(small, tmp_path):
    from wmar_amd.models.tokenizer_handles import ImageTokenizerHandle
    from wmar_amd.utils.utils import update_weights
    cfg, sd = small
    tok, orig = TorchTokenizer(cfg, sd), TorchTokenizer(cfg, sd)
    codes = torch.randint(0, cfg.n_embed, (4, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(1))
    args = argparse.Namespace(augs="none", augs_schedule=None, nb_epochs=2, lr=1e-3, idempotence_loss_weight=2.0, idempotence_loss_weight_factor=0.5,
                              batch_size_per_gpu=2, seed=0, max_steps=None)
    lines = []
    random.seed(0)
    assert cli.train(tok, orig, codes, args, log=lambda s: lines.append(__import__("json").loads(s))) == 4
    assert [l["loss_weight"] for l in lines] == [2.0, 2.0, 1.0, 1.0]
    assert [round(l["lr"], 9) for l in lines] == [1e-3, 1e-3, 9e-4, 9e-4]
    assert not tok.state["quant_conv.weight"].requires_grad and torch.equal(tok.state["quant_conv.weight"], sd["quant_conv.weight"])
    for name in ("encoder", "decoder"):
        n = len(name) + 1
        trained = {k[n:]: v for k, v in tok.state.items() if k.startswith(name + ".")}
        diff = ft.save_delta(trained, {k[n:]: v for k, v in sd.items() if k.startswith(name + ".")}, str(tmp_path / f"{name}_ft_delta.pth"))
        assert any(float(v.abs().max()) > 0 for v in diff.values())
    fresh = {k: v.clone() for k, v in sd.items()}
    handle = ImageTokenizerHandle(fresh, lambda: None)
    update_weights(handle.encoder, str(tmp_path / "encoder_ft_delta.pth"), delta=True)
    update_weights(handle.decoder, str(tmp_path / "decoder_ft_delta.pth"), delta=True)
    for k, v in tok.state.items():
        assert torch.allclose(fresh[k], v.detach(), rtol=0, atol=1e-6), k
