"""CPU: what RAR tokenizer fine-tuning adds without a GPU -- the C ABI entries (declared, listed, exported, null arguments refused),
the float64 walkers of tests/mvq_grad_reference.py pinned to the trusted ``oracle.rar_oracle`` forwards, the CLI's model / shape
binding, and ``rcc_loss`` / the training loop / the delta files over the pure-torch MaskGIT stand-in."""
import argparse
import ctypes as C
import json
import math
import os
import random
import re

import pytest
import torch

import finetune as cli
from tests import mvq_grad_reference as M
from tests.conftest import REPO
from wmar_amd import finetune as ft
from wmar_amd.utils import synth

ENTRIES = ["wmar_mvq_train_create", "wmar_vq_probe_avgpool_backward", "wmar_mvq_probe_image_backward", "wmar_mvq_probe_input_backward"]


def _small_cfg():
    return synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16, num_embeddings=512)


@pytest.fixture(scope="module")
def small():
    cfg = _small_cfg()
    return cfg, synth.synth_maskgit_state(cfg, 2, "cpu")


def test_new_symbols_are_declared_listed_and_exported():
    from wmar_amd import _lib
    L = _lib.load()
    header = open(os.path.join(REPO, "include", "wmar_hip.h")).read()
    declared = set(re.findall(r"\b(wmar_[a-z0-9_]+)\s*\(", header))
    for s in ENTRIES:
        assert s in declared and s in _lib.SYMBOLS and hasattr(L, s), s


def test_null_arguments_are_refused_with_a_message():
    from wmar_amd import _lib
    L = _lib.load()
    calls = [lambda: L.wmar_mvq_train_create(None, None, None, 0, None, None),
             lambda: L.wmar_vq_probe_avgpool_backward(None, 1, 8, 8, 32, None, None),
             lambda: L.wmar_mvq_probe_image_backward(None, None, 1, 3, 64, 8, None, None),
             lambda: L.wmar_mvq_probe_input_backward(None, 1, 3, 64, 8, None, None)]
    for call in calls:
        assert call() == -1                                   # WMAR_EINVAL
        assert b"null argument" in L.wmar_last_error()


def test_walker_forwards_equal_the_oracle_bit_for_bit(small):
    from oracle import rar_oracle
    cfg, sd = small
    S, z = cfg.codes_size, cfg.z_channels
    codes = torch.randint(0, cfg.num_embeddings, (2, S * S), generator=torch.Generator().manual_seed(0))
    x = torch.rand(2, 3, cfg.resolution, cfg.resolution, generator=torch.Generator().manual_seed(1)) * 2 - 1
    tok = M.TorchTokenizer(cfg, sd)
    with torch.no_grad():
        img = M.decode(sd, cfg, tok.embed(codes))
        pre = M.encoder_prequant(sd, cfg, x)
        assert torch.equal(img, M.decode_preclamp(sd, cfg, tok.embed(codes)).clamp(0, 1) * 2 - 1)
    assert torch.equal(img, rar_oracle.maskgit_decode(sd, cfg, codes))
    assert torch.equal(pre.permute(0, 2, 3, 1).reshape(-1, z), rar_oracle.maskgit_prequant(sd, cfg, x))
    assert float(img.min()) == -1.0 and float(img.max()) == 1.0          # the clamp is active on both sides
    _, idx = tok.quantize(pre)
    assert torch.equal(idx, rar_oracle.maskgit_encode(sd, cfg, x))
    # bias-free convs have no bias gradient: the key set of each half is the state's
    out, gx, g = M.half_gradients(sd, cfg, 0, x, torch.ones_like(pre), torch.float64)
    assert set(g) == {k for k in sd if k.startswith("encoder.")} and "encoder.conv_in.bias" not in g and gx.dtype == torch.float64
    out, gz, g = M.half_gradients(sd, cfg, 1, tok.embed(codes), torch.ones_like(img), torch.float64)
    assert set(g) == {k for k in sd if k.startswith("decoder.")} and "decoder.mid.0.conv1.bias" not in g


def test_parser_binds_synthetic_shapes_to_models():
    p = cli.build_parser()
    a = p.parse_args("--model rar --synthetic --synthetic_config maskgit_small --dataset_size 4 --batch_size_per_gpu 2 --nb_epochs 1 --augs none "
                     "--outdir out".split())
    cli.check_args(a)
    cli.check_args(p.parse_args("--model rar --synthetic --synthetic_config maskgit --outdir out".split()))
    cli.check_args(p.parse_args("--model rar --modelpath m --datapath c.pt --outdir out".split()))
    with pytest.raises(SystemExit, match="rar.*maskgit_small, maskgit"):
        cli.check_args(p.parse_args("--model rar --synthetic --outdir out".split()))
    with pytest.raises(SystemExit, match="rar"):
        cli.check_args(p.parse_args("--model rar --synthetic --synthetic_config taming --outdir out".split()))
    with pytest.raises(SystemExit, match="taming.*harness, taming"):
        cli.check_args(p.parse_args("--model taming --synthetic --synthetic_config maskgit_small --outdir out".split()))
    with pytest.raises(SystemExit, match="chameleon7b is not built"):
        cli.check_args(p.parse_args("--model chameleon7b --synthetic --outdir out".split()))
    assert p.get_default("synthetic_config") == "harness"
    r, v = cli.synthetic_rar_configs("maskgit_small")
    assert v == _small_cfg() and r.image_seq_len == v.codes_size ** 2 and r.codebook_size == v.num_embeddings
    assert cli.synthetic_rar_configs("maskgit")[1] == synth.MASKGIT_VQ


def test_rcc_loss_without_augmentation_is_the_loss_of_the_reference_forward(small):
    """titok.py:145-191 by hand: decode_like_taming with the trained and the original decoder, |.| mean between them, the encoder on
    (xrec + 1) / 2, the mean squared difference of the code vectors."""
    cfg, sd = small
    tok, orig = M.TorchTokenizer(cfg, sd, torch.float64), M.TorchTokenizer(cfg, sd, torch.float64)
    with torch.no_grad():
        for _, prm in tok.named_parameters("decoder."):
            prm.add_(0.01 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(prm.numel()), dtype=torch.float64))
    idx = torch.randint(0, cfg.num_embeddings, (2, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(0))
    loss, res, log, was = ft.rcc_loss(tok, idx, [], p=0.5, loss_weight=3.0, orig=orig)
    S = cfg.codes_size
    z_q = tok.state["quantize.embedding.weight"][idx].view(2, S, S, cfg.z_channels).permute(0, 3, 1, 2)
    xrec = torch.clamp(M.decode_preclamp(tok.state, cfg, z_q), 0.0, 1.0) * 2.0 - 1.0
    xorig = torch.clamp(M.decode_preclamp(orig.state, cfg, z_q), 0.0, 1.0) * 2.0 - 1.0
    zrec = M.encoder_prequant(tok.state, cfg, xrec)
    want = torch.mean(torch.abs(xorig - xrec)) + 3.0 * torch.mean((z_q - zrec) ** 2)
    assert not was and torch.allclose(loss, want, rtol=1e-12, atol=0)
    assert float(xrec.detach().min()) == -1.0 and float(xrec.detach().max()) == 1.0
    assert set(res) == {"orig_z_q", "orig_z_indices", "rec_x", "rec_x_maybe_augmented", "rec_x_orig_decoder", "rec_z", "rec_z_q", "rec_z_indices"}
    assert res["rec_z_indices"].shape == idx.shape and log["loss_weight"] == 3.0 and math.isclose(log["loss"], float(want.detach()), rel_tol=1e-12)
    loss.backward()
    assert ft.calculate_gradient_norm(tok, "decoder.") > 0 and ft.calculate_gradient_norm(tok, "encoder.") > 0
    assert {k.split(".")[0] for k, _ in tok.named_parameters()} == {"encoder", "decoder"}


def test_training_loop_over_the_stand_in_and_the_deltas_round_trip(small, tmp_path):
    from wmar_amd.models.tokenizer_handles import ImageTokenizerHandle
    from wmar_amd.utils.utils import update_weights
    cfg, sd = small
    tok, orig = M.TorchTokenizer(cfg, sd), M.TorchTokenizer(cfg, sd)
    codes = torch.randint(0, cfg.num_embeddings, (4, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(1))
    args = argparse.Namespace(augs="none", augs_schedule=None, nb_epochs=1, lr=1e-3, idempotence_loss_weight=2.0, idempotence_loss_weight_factor=0.5,
                              batch_size_per_gpu=2, seed=0, max_steps=None)
    lines = []
    random.seed(0)
    assert cli.train(tok, orig, codes, args, log=lambda s: lines.append(json.loads(s))) == 2
    assert [l["loss_weight"] for l in lines] == [2.0, 2.0] and all(l["enc_grad_L2"] > 0 and l["dec_grad_L2"] > 0 for l in lines)
    assert torch.equal(tok.state["quantize.embedding.weight"], sd["quantize.embedding.weight"])
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
