"""MI355X: ``finetune.py --val_percent`` end to end -- the validation lines it emits, the first ``l0`` against a direct computation on
the wrapper's own engines, the weight distances, and that a run with a validation split writes the deltas of a run on the same training
rows without one, bit for bit."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

COMMON = ("--synthetic --augs all+geom --augs_schedule 0,1 --nb_epochs 1 --batch_size_per_gpu 2 --optimizer adam --lr 1e-4 "
          "--idempotence_loss_weight 1.0 --idempotence_loss_weight_factor 1.0 --seed 0")


def _run(capsys, argv):
    import finetune as cli
    assert cli.main(argv.split()) == 0
    return [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_taming_run_emits_two_validations_and_the_first_l0_is_the_direct_count(capsys, tmp_path):
    from wmar_amd.models.taming_wrapper import TamingARMMWrapper
    from wmar_amd.models.tokenizer_train import TrainableTokenizer
    from wmar_amd.utils import synth
    out = tmp_path / "val"
    lines = _run(capsys, f"--model taming --synthetic_config harness {COMMON} --dataset_size 8 --val_percent 0.25 --outdir {out}")
    val = [l for l in lines if l.get("split") == "val"]
    train = [l for l in lines if "step" in l]
    assert len(train) == 3                                     # 6 training rows in batches of 2
    for epoch in (0, 1):
        recs = [l for l in val if l["epoch"] == epoch and "aug" in l]
        dist = [l for l in val if l["epoch"] == epoch and "enc_l2" in l]
        assert len(recs) == 17 and len(dist) == 1, (epoch, len(recs), len(dist))
        assert recs[0]["aug"] == "Identity" and all(r["n"] == 2 for r in recs)
        assert all(0.0 <= r["l0"] <= 1.0 and r["loss"] == r["loss"] for r in recs)
        assert len({(r["aug"], r["param"]) for r in recs}) == 17
    assert len(val) == 36
    # the lines come in order: validation of epoch 0, the training steps, the final validation
    assert lines.index(val[17]) < lines.index(train[0]) and lines.index(train[-1]) < lines.index(val[18])
    first, last = [l for l in val if "enc_l2" in l]
    assert first["enc_l2"] == 0.0 and first["dec_l2"] == 0.0 and last["enc_l2"] > 0 and last["dec_l2"] > 0
    # l0 of Identity before the first step, directly: decode on a forward-only handle over the wrapper's weights, re-encode on its engine
    cfg = synth.VQConfig(**synth.HARNESS_VQ)
    model = TamingARMMWrapper.synthetic(synth.GPTConfig(**synth.HARNESS_GPT), cfg, seed=0, max_batch=8)
    codes = torch.randint(0, cfg.n_embed, (8, cfg.codes_size ** 2), generator=torch.Generator().manual_seed(0))[6:].cuda()
    tok = TrainableTokenizer(cfg, model.model.vq_state, max_batch=2, frozen=True)
    again = model.model.vq_engine.encode(tok.decode(tok.embed(codes)))
    l0 = float((again != codes).float().mean())
    ident = [l for l in val if l["epoch"] == 0 and l.get("aug") == "Identity"][0]
    assert ident["l0"] == l0
    # the same training rows without a validation split: the same deltas, bit for bit
    plain = tmp_path / "plain"
    lines2 = _run(capsys, f"--model taming --synthetic_config harness {COMMON} --dataset_size 6 --outdir {plain}")
    assert not [l for l in lines2 if l.get("split") == "val"]
    assert [l for l in lines2 if "step" in l] == train
    for name in ("encoder_ft_delta.pth", "decoder_ft_delta.pth"):
        a, b = torch.load(str(out / name)), torch.load(str(plain / name))
        assert set(a) == set(b) and any(float(v.abs().max()) > 0 for v in a.values())
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)


def test_rar_run_emits_the_validation_records(capsys, tmp_path):
    lines = _run(capsys, f"--model rar --synthetic_config maskgit_small {COMMON} --dataset_size 8 --val_percent 0.25 --outdir {tmp_path / 'rar'}")
    val = [l for l in lines if l.get("split") == "val"]
    assert len(val) == 36 and sum("aug" in l for l in val) == 34 and sum("enc_l2" in l for l in val) == 2
    assert [l["epoch"] for l in val] == [0] * 18 + [1] * 18
    assert all(l["n"] == 2 and 0.0 <= l["l0"] <= 1.0 for l in val if "aug" in l)
    assert len([l for l in lines if "step" in l]) == 3
