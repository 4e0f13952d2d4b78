"""CPU: the validation pass of the fine-tuning loop (``wmar_amd.finetune.validate``) against a written-out loop over the pure-torch
stand-in tokenizer of tests/vq_grad_reference.py; the ``--val_percent`` split and its refusals; ``weight_distance`` against the
formula; the RNG states validation must leave alone; the validation lines of ``finetune.train``."""
import argparse
import json
import random

import pytest
import torch

import finetune as cli
from tests import vq_grad_reference as G
from wmar_amd import finetune as ft
from wmar_amd.augmentations.geometric import HorizontalFlip, Identity, Rotate, UpperLeftCropWithPadBack
from wmar_amd.utils import synth

TorchTokenizer = G.TorchTokenizer
AUGS = [(HorizontalFlip, [0]), (Rotate, [-10, 10]), (UpperLeftCropWithPadBack, [0.5, 0.7])]


@pytest.fixture(scope="module")
def setup():
    cfg = synth.VQConfig(**dict(synth.HARNESS_VQ, n_embed=64))
    sd = synth.synth_vq_state(cfg, 2, "cpu")
    tok, orig = TorchTokenizer(cfg, sd), TorchTokenizer(cfg, sd)
    with torch.no_grad():
        for _, prm in tok.named_parameters(("encoder.", "decoder.")):
            prm.add_(0.01 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(prm.numel())))
    codes = torch.randint(0, cfg.n_embed, (5, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(0))
    return cfg, sd, tok, orig, codes


def test_validate_equals_the_written_out_loop(setup):
    cfg, sd, tok, orig, codes = setup
    recs = ft.validate(tok, orig, codes, AUGS, batch_size=2, loss_weight=3.0)
    assert len(recs) == 1 + sum(len(p) for _, p in AUGS)
    assert [(r["aug"], r["param"]) for r in recs] == [("Identity", 0), ("HorizontalFlip", 0), ("Rotate", -10), ("Rotate", 10),
                                                      ("UpperLeftCropWithPadBack", 0.5), ("UpperLeftCropWithPadBack", 0.7)]
    batches = [codes[0:2], codes[2:4], codes[4:5]]           # the last one is short
    for rec, (cls, param) in zip(recs, [(Identity, 0)] + [(c, p) for c, ps in AUGS for p in ps]):
        want = {"loss": 0.0, "idem_loss": 0.0, "rec_loss": 0.0, "l0": 0.0, "loss_weight": 0.0}
        for b in batches:
            with torch.no_grad():
                _, res, log, was = ft.rcc_loss(tok, b, [(cls, [param])], p=1.0, loss_weight=3.0, orig=orig)
            assert was == (cls is not Identity)
            log["l0"] = float((res["orig_z_indices"] != res["rec_z_indices"]).float().mean())
            for k in want:
                want[k] += log[k] * b.shape[0]
        assert rec["n"] == 5 and rec["loss_weight"] == 3.0
        assert "rec_loss_perceptual_component" not in rec
        for k in want:
            assert rec[k] == want[k] / 5, (rec["aug"], k)
    # Identity is the loss without any augmentation, and l0 the direct count
    total, changed = 0.0, 0
    for b in batches:
        with torch.no_grad():
            loss, res, _, _ = ft.rcc_loss(tok, b, [], p=0.5, loss_weight=3.0, orig=orig)
            z_q = tok.embed(b)
            _, idx = tok.quantize(tok.encode_prequant(tok.decode(z_q)))
        total += float(loss) * b.shape[0]
        changed += int((idx != b).sum())
    assert recs[0]["loss"] == total / 5
    assert abs(recs[0]["l0"] - changed / codes.numel()) < 1e-7
    assert 0 < changed                                        # the perturbed tokenizer does change codes: l0 measures something


def test_validate_logs_the_perceptual_component_of_a_rec_loss_that_has_one(setup):
    cfg, sd, tok, orig, codes = setup

    class Rec:
        perceptual_component = None

        def __call__(self, a, b):
            self.perceptual_component = ((a - b) ** 2).mean().detach()
            return (a - b).abs().mean() + self.perceptual_component

    recs = ft.validate(tok, orig, codes[:3], [], batch_size=2, loss_weight=1.0, rec_loss=Rec())
    assert len(recs) == 1 and recs[0]["rec_loss_perceptual_component"] > 0


def test_validate_leaves_every_rng_state_and_every_gradient_alone(setup):
    cfg, sd, tok, orig, codes = setup
    random.seed(7)
    torch.manual_seed(7)
    py, cpu = random.getstate(), torch.get_rng_state()
    grads = [p.grad for p in tok.parameters()]
    out = ft.validate(tok, orig, codes, AUGS, batch_size=2, loss_weight=1.0)
    assert random.getstate() == py and torch.equal(torch.get_rng_state(), cpu)
    assert all(p.grad is g for p, g in zip(tok.parameters(), grads))
    assert all(isinstance(v, (int, float, str)) for r in out for v in r.values())      # plain records: they go out as JSON
    json.dumps(out)


def test_split_arithmetic_and_refusals():
    assert cli.split_rows(8, 0.0) == (8, 0) and cli.split_rows(8, 0.25) == (6, 2) and cli.split_rows(100, 0.05) == (95, 5)
    assert cli.split_rows(10, 0.33) == (int(10 * (1 - 0.33)), 10 - int(10 * (1 - 0.33)))
    assert cli.split_rows(5, 0.4) == (3, 2) and cli.split_rows(4, 0.1) == (3, 1)
    for n, f in ((4, 1e-20), (1, 0.5), (3, 0.9)):             # int(n (1 - F)) == n or == 0: an empty half
        with pytest.raises(SystemExit, match="val_percent"):
            cli.split_rows(n, f)
    p = cli.build_parser()
    assert p.parse_args("--synthetic --outdir o".split()).val_percent == 0.0
    cli.check_args(p.parse_args("--synthetic --outdir o --val_percent 0.25".split()))
    for bad in ("1.0", "-0.1", "1.5"):
        with pytest.raises(SystemExit, match="val_percent"):
            cli.check_args(p.parse_args(f"--synthetic --outdir o --val_percent {bad}".split()))
    with pytest.raises(SystemExit, match="val_percent"):      # --validate stays refused and points here
        cli.check_args(p.parse_args("--synthetic --outdir o --validate".split()))
    # the Chameleon shapes are bound to their model
    cli.check_args(p.parse_args("--model chameleon7b --synthetic --synthetic_config chameleon_small --outdir o".split()))
    with pytest.raises(SystemExit, match="chameleon_small"):
        cli.check_args(p.parse_args("--model taming --synthetic --synthetic_config chameleon_small --outdir o".split()))


def test_weight_distance_is_the_mean_of_the_tensor_norms(setup):
    cfg, sd, tok, orig, codes = setup
    for prefix in ("encoder.", "decoder."):
        keys = [k for k in tok.state if k.startswith(prefix)]
        want = torch.mean(torch.stack([torch.norm(tok.state[k].detach() - sd[k]) for k in keys])).item()
        assert ft.weight_distance(tok.state, sd, prefix) == want and want > 0
        assert ft.weight_distance(sd, sd, prefix) == 0.0


def test_training_with_validation_logs_both_and_trains_the_same(setup):
    cfg, sd, _, _, codes = setup
    args = argparse.Namespace(augs="none", augs_schedule=None, nb_epochs=2, lr=1e-3, idempotence_loss_weight=2.0,
                              idempotence_loss_weight_factor=0.5, batch_size_per_gpu=2, seed=0, max_steps=None)
    runs = {}
    for name, val in (("plain", None), ("val", codes[3:])):
        tok, orig = TorchTokenizer(cfg, sd), TorchTokenizer(cfg, sd)
        lines = []
        random.seed(0)
        torch.manual_seed(0)
        assert cli.train(tok, orig, codes[:3], args, log=lambda s: lines.append(json.loads(s)), val_codes=val, original=sd) == 4
        runs[name] = (tok, lines)
    plain, val = runs["plain"][1], runs["val"][1]
    assert len(plain) == 4 and all("split" not in l for l in plain)
    assert [l for l in val if "split" not in l] == plain                      # training lines stay as they are
    v = [l for l in val if l.get("split") == "val"]
    assert [l["epoch"] for l in v] == [0, 0, 1, 1, 2, 2]                      # before each epoch and once after the last
    assert [l["loss_weight"] for l in v if "aug" in l] == [2.0, 1.0, 0.5]
    assert all(l["aug"] == "Identity" and l["n"] == 2 for l in v if "aug" in l)
    d = [l for l in v if "enc_l2" in l]
    assert d[0]["enc_l2"] == 0.0 and d[0]["dec_l2"] == 0.0 and d[2]["enc_l2"] > 0 and d[2]["dec_l2"] > 0
    assert val.index(v[0]) == 0 and val[-1] is v[-1]
    for k, t in runs["plain"][0].state.items():
        assert torch.equal(t, runs["val"][0].state[k]), k                       # validation does not move training
    # --max_steps ends training early: the final validation still runs
    tok, orig = TorchTokenizer(cfg, sd), TorchTokenizer(cfg, sd)
    lines = []
    args.max_steps = 1
    assert cli.train(tok, orig, codes[:3], args, log=lambda s: lines.append(json.loads(s)), val_codes=codes[3:], original=sd) == 1
    assert [l.get("epoch") for l in lines if l.get("split") == "val"] == [0, 0, 2, 2]
