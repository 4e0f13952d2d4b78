"""Tokenizer fine-tuning (reverse-cycle-consistency) for ``--model taming``, ``--model chameleon7b`` and ``--model rar`` on one
MI355X: the reference's finetune.py flags, driving ``wmar_amd.finetune.rcc_loss`` over the native trainable tokenizer (the Taming
VQGAN, Chameleon's VQGAN -- the Taming network at its own layout -- or RAR's MaskGIT-VQGAN).  Writes ``encoder_ft_delta.pth`` and ``decoder_ft_delta.pth`` into ``--outdir`` in the form
``generate.py --encoder_ft_ckpt / --decoder_ft_ckpt`` accept.

    python finetune.py --model taming --synthetic --synthetic_config harness --nb_epochs 1 --augs none --optimizer adam --lr 1e-4 \
        --batch_size_per_gpu 2 --dataset_size 4 --idempotence_loss_weight 1.0 --idempotence_loss_weight_factor 1.0 --outdir out/
    python finetune.py --model rar --synthetic --synthetic_config maskgit_small --nb_epochs 1 --augs none --batch_size_per_gpu 2 \
        --dataset_size 4 --outdir out/
    python finetune.py --model chameleon7b --synthetic --synthetic_config chameleon_small --nb_epochs 1 --augs none --batch_size_per_gpu 2 \
        --dataset_size 4 --outdir out/

``--lpips_vgg PATH --lpips_lin PATH`` (torchvision's VGG16 state dict and the reference's ``vgg.pth``) add the reference's perceptual
term to the regulariser, ``|x_orig_dec - x_rec| + --perceptual_weight x LPIPS``, on the device (wmar_amd/lpips.py); ``--synthetic_lpips``
draws random LPIPS weights for a ``--synthetic`` run.  Without them the regulariser is the L1 half alone.  LPIPS runs at the
tokenizer's resolution, which must be a multiple of 128.

``--synthetic_config`` names are bound to models: ``harness`` / ``harness128`` / ``taming`` are Taming shapes, ``maskgit_small`` / ``maskgit`` are
MaskGIT shapes for ``--model rar``, ``chameleon_small`` / ``chameleon`` are Chameleon shapes (five levels, no level attention; 128 x 128
and the real 512 x 512); ``--model rar --modelpath DIR`` loads ``RarARMMWrapper(DIR)``, ``--model chameleon7b --modelpath DIR``
``ChameleonARMMWrapper(DIR)``.  The codes of ``--datapath`` are the tokenizer's own code ids ``0 .. n_embed - 1`` (for Chameleon: not
vocabulary ids); ``precompute_codes.py`` writes such a file from a directory of images.

``--val_percent F`` (0 <= F < 1, default 0: no validation; the reference hard-codes 0.05) keeps the last ``n - int(n * (1 - F))`` rows,
in file order after ``--dataset_size``, for validation (finetune.py:73-128, 388-391, 509-514): before every epoch and once after
training ends, the loss without gradients for "no augmentation" and for every (transform, parameter) of the epoch's curriculum, one
JSON line each with ``"split": "val"``, the share of codes that change (``l0``), and one line with the mean L2 distance of the
encoder's and the decoder's tensors from the originals (``enc_l2`` / ``dec_l2``).  Validation draws from no generator training sees:
the deltas are bit-identical to those of a run on the same training rows without it.

The original decoder of the regulariser and every no-grad forward run on forward-only engine handles (no tape, no gradient memory).

Not built here, each rejected with a message: multi-GPU training (DDP), tensorboard logging, and the reference's ``--validate``
switch (use ``--val_percent``)."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--model", type=str, default="taming", choices=["taming", "chameleon7b", "rar"])
    p.add_argument("--modelpath", type=str, help="taming: directory with configs/net2net.yaml and checkpoints/net2net.ckpt; "
                                                 "rar: directory with maskgit-vqgan-imagenet-f16-256.bin and rar_xl.bin")
    p.add_argument("--synthetic", action="store_true", help="random-init weights instead of --modelpath")
    p.add_argument("--synthetic_config", type=str, default="harness", choices=["harness", "harness128", "taming", "maskgit_small", "maskgit", "chameleon_small", "chameleon"])
    p.add_argument("--datapath", type=str, help="int64 [N, S*S] codes, .pt or .npy (with --synthetic: random codes when absent)")
    p.add_argument("--dataset_size", type=int, help="number of rows to use")
    p.add_argument("--mode", type=str, default="newenc-dec")
    p.add_argument("--nb_epochs", type=int, default=1)
    p.add_argument("--augs", type=str, default="none", choices=["none", "all+geom"])
    p.add_argument("--augs_schedule", type=str, default=None, help="epochs per augmentation stage, e.g. 1,1,4,4")
    p.add_argument("--optimizer", type=str, default="adam")
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--batch_size_per_gpu", type=int, default=4)
    p.add_argument("--idempotence_loss_weight", type=float, default=1.0)
    p.add_argument("--idempotence_loss_weight_factor", type=float, default=1.0)
    p.add_argument("--loss", type=str, default="hard-to-soft-with-ae")
    p.add_argument("--outdir", type=str, required=True)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--max_steps", type=int, default=None, help="stop after this many optimizer steps")
    p.add_argument("--local_rank", "--local-rank", type=int, default=-1)
    p.add_argument("--tensorboard", action="store_true")
    p.add_argument("--validate", action="store_true")
    p.add_argument("--val_percent", type=float, default=0.0, help="share of the rows (the last ones, in file order) kept for the validation "
                                                                  "pass; 0: no validation (the reference hard-codes 0.05)")
    p.add_argument("--lpips_vgg", type=str, help="torchvision's VGG16 state dict (features.N.weight / .bias): with --lpips_lin, adds the "
                                                 "reference's LPIPS term to the regulariser")
    p.add_argument("--lpips_lin", type=str, help="the reference's vgg.pth (the lin layers of LPIPS)")
    p.add_argument("--synthetic_lpips", action="store_true", help="with --synthetic: a random-init full-width LPIPS instead of the two files")
    p.add_argument("--perceptual_weight", type=float, default=1.0)
    return p


# the synthetic shapes each trainable model takes (harness128: the harness shape at 128 x 128, the smallest LPIPS takes)
SYNTHETIC_CONFIGS = {"taming": ("harness128", "harness", "taming"), "rar": ("maskgit_small", "maskgit"),
                     "chameleon7b": ("chameleon_small", "chameleon")}
# resolution of each synthetic shape
SYNTHETIC_RESOLUTION = {"harness": 32, "harness128": 128, "taming": 256, "maskgit_small": 32, "maskgit": 256, "chameleon_small": 128,
                        "chameleon": 512}
# chameleon_small keeps Chameleon's layout -- five levels, two neighbouring levels of equal width (a downsample behind blocks without a
# shortcut), no level attention, a mid attention (64 tokens) -- at 128 x 128, a resolution LPIPS takes, with an 8 x 8 code grid
CHAMELEON_SMALL_VQ = dict(ch=32, ch_mult=(1, 1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(), resolution=128, z_channels=32, embed_dim=32,
                          n_embed=512)


def wants_lpips(args) -> bool:
    return bool(args.lpips_vgg or args.lpips_lin or args.synthetic_lpips)


def check_args(args) -> None:
    """Everything this CLI does not implement is refused here, before any model is built."""
    if args.model not in SYNTHETIC_CONFIGS:
        raise SystemExit(f"finetune.py: --model {args.model} is not built")
    if args.synthetic and args.synthetic_config not in SYNTHETIC_CONFIGS[args.model]:
        raise SystemExit(f"finetune.py: --synthetic_config {args.synthetic_config} with --model {args.model} is not built: "
                         f"the shapes of that model are {', '.join(SYNTHETIC_CONFIGS[args.model])}")
    if args.local_rank != -1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("finetune.py: multi-GPU training (DDP) is not built: run one process on one GPU")
    if args.tensorboard:
        raise SystemExit("finetune.py: tensorboard logging is not built: the log lines go to stdout as JSON")
    if args.validate:
        raise SystemExit("finetune.py: --validate is not built: the validation pass runs with --val_percent F (the reference's share is 0.05)")
    if not 0.0 <= getattr(args, "val_percent", 0.0) < 1.0:
        raise SystemExit(f"finetune.py: --val_percent {args.val_percent} outside [0, 1)")
    if args.mode != "newenc-dec":
        raise SystemExit(f"finetune.py: --mode {args.mode} not supported (newenc-dec)")
    if args.loss != "hard-to-soft-with-ae":
        raise SystemExit(f"finetune.py: --loss {args.loss} not supported (hard-to-soft-with-ae)")
    if args.optimizer != "adam":
        raise SystemExit(f"finetune.py: --optimizer {args.optimizer} not supported (adam)")
    if bool(args.modelpath) == bool(args.synthetic):
        raise SystemExit("finetune.py: give exactly one of --modelpath and --synthetic")
    if not args.synthetic and not args.datapath:
        raise SystemExit("finetune.py: --datapath is required with --modelpath")
    if bool(args.lpips_vgg) != bool(args.lpips_lin):
        raise SystemExit("finetune.py: --lpips_vgg and --lpips_lin go together: LPIPS needs the VGG16 weights and the lin layers")
    if args.synthetic_lpips and not args.synthetic:
        raise SystemExit("finetune.py: --synthetic_lpips is valid only with --synthetic (random LPIPS weights mean nothing to a real model)")
    if args.synthetic_lpips and args.lpips_vgg:
        raise SystemExit("finetune.py: give either --synthetic_lpips or --lpips_vgg / --lpips_lin")
    if wants_lpips(args) and args.synthetic and SYNTHETIC_RESOLUTION[args.synthetic_config] % 128:
        raise SystemExit(f"finetune.py: LPIPS needs a resolution that is a multiple of 128, --synthetic_config {args.synthetic_config} has "
                         f"{SYNTHETIC_RESOLUTION[args.synthetic_config]}")


def load_codes(path: str):
    import numpy as np
    import torch
    codes = torch.from_numpy(np.load(path)) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    if codes.ndim != 2 or codes.dtype != torch.int64:
        raise SystemExit(f"finetune.py: {path} must hold an int64 [N, S*S] tensor, got {codes.dtype} {tuple(codes.shape)}")
    return codes


def split_rows(n: int, val_percent: float):
    """(n_train, n_val) of ``--val_percent``: the first ``int(n * (1 - F))`` rows train, the rest validate; an empty half is refused."""
    if not val_percent:
        return n, 0
    n_train = int(n * (1 - val_percent))
    if n_train < 1 or n_train >= n:
        raise SystemExit(f"finetune.py: --val_percent {val_percent} of {n} rows leaves {n_train} to train on and {n - n_train} to validate on: "
                         f"both halves need at least one row")
    return n_train, n - n_train


def run_validation(tok, orig, val_codes, entries, epoch, weight, args, original, log, rec_loss):
    """One validation pass (wmar_amd.finetune.validate) as JSON lines: a record per (transform, parameter), then the weight distances."""
    from wmar_amd.finetune import validate, weight_distance
    for rec in validate(tok, orig, val_codes, entries, args.batch_size_per_gpu, weight, rec_loss=rec_loss):
        log(json.dumps(dict(rec, split="val", epoch=epoch)))
    if original is not None:
        log(json.dumps({"split": "val", "epoch": epoch, "enc_l2": weight_distance(tok.state, original, "encoder."),
                        "dec_l2": weight_distance(tok.state, original, "decoder.")}))


def train(tok, orig, codes, args, log=print, rec_loss=None, val_codes=None, original=None):
    """Adam (0.9, 0.999) + StepLR(gamma 0.9 per epoch) over the encoder's and the decoder's weights; the idempotence weight is multiplied
    by its factor after every epoch.  ``rec_loss``: the regulariser of ``rcc_loss`` (None: L1 only).  ``val_codes``: rows for the
    validation pass, run before every epoch with that epoch's curriculum and the current idempotence weight, and once after training
    ends for any reason with ``epoch = nb_epochs`` and the last epoch's entries (finetune.py:388-391, 509-514); ``original``: the
    state the weight distances are taken from.  Returns the number of optimizer steps."""
    from wmar_amd.augmentations import finetune_schedule
    schedule = finetune_schedule(args.augs, args.augs_schedule, args.nb_epochs)
    steps, weight = _train(tok, orig, codes, args, log, rec_loss, val_codes, original, schedule)
    if val_codes is not None:
        run_validation(tok, orig, val_codes, schedule[args.nb_epochs - 1], args.nb_epochs, weight, args, original, log, rec_loss)
    return steps


def _train(tok, orig, codes, args, log, rec_loss, val_codes, original, schedule):
    """The loop of ``train``; returns (optimizer steps, the idempotence weight it ended with)."""
    import torch
    from wmar_amd.finetune import calculate_gradient_norm, rcc_loss
    for k, prm in tok.named_parameters():
        prm.requires_grad_(k.startswith(("encoder.", "decoder.")))          # the 1x1 quant convolutions stay as they are
    params = list(tok.parameters(("encoder.", "decoder.")))
    opt = torch.optim.Adam(params, lr=args.lr, betas=(0.9, 0.999))
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.9)
    weight, steps, bs = args.idempotence_loss_weight, 0, args.batch_size_per_gpu
    gen = torch.Generator().manual_seed(args.seed)
    for epoch in range(args.nb_epochs):
        if val_codes is not None:
            run_validation(tok, orig, val_codes, schedule[epoch], epoch, weight, args, original, log, rec_loss)
        order = torch.randperm(codes.shape[0], generator=gen)
        for b0 in range(0, codes.shape[0], bs):
            batch = codes[order[b0:b0 + bs]]
            loss, _, log_dict, was_aug = rcc_loss(tok, batch, schedule[epoch], p=0.5, loss_weight=weight, orig=orig, rec_loss=rec_loss)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            log_dict.update(epoch=epoch, step=steps, was_augmented=bool(was_aug), lr=sched.get_last_lr()[0],
                            enc_grad_L2=calculate_gradient_norm(tok, "encoder."), dec_grad_L2=calculate_gradient_norm(tok, "decoder."))
            opt.step()
            steps += 1
            log(json.dumps(log_dict))
            if args.max_steps is not None and steps >= args.max_steps:
                return steps, weight
        sched.step()
        weight *= args.idempotence_loss_weight_factor
    return steps, weight


def synthetic_rar_configs(name: str):
    """(RARConfig, MaskgitVQConfig) of a ``--synthetic_config`` of ``--model rar``.  The transformer is not trained: a small one whose
    sequence is the tokenizer's code grid."""
    from wmar_amd.utils import synth
    v = (synth.MaskgitVQConfig(hidden_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, resolution=32, z_channels=16, num_embeddings=512)
         if name == "maskgit_small" else synth.MASKGIT_VQ)
    r = synth.RARConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, image_seq_len=v.codes_size ** 2,
                        codebook_size=v.num_embeddings)
    return r, v


def synthetic_chameleon_configs(name: str):
    """(ChameleonConfig, VQConfig) of a ``--synthetic_config`` of ``--model chameleon7b``.  The transformer is not trained: a small one
    whose vocabulary holds the tokenizer's codes."""
    from wmar_amd.utils import synth
    v = synth.VQConfig(**CHAMELEON_SMALL_VQ) if name == "chameleon_small" else synth.CHAMELEON_VQ
    c = synth.ChameleonConfig(dim=256, n_layers=2, n_heads=4, n_kv_heads=4, vocab_size=max(1024, 2 * v.n_embed), multiple_of=64,
                              qk_normalization=True)
    return c, v


def load_model(args):
    """The wrapper of ``--model``, its tokenizer config, the codebook size and the class of its trainable tokenizer."""
    from wmar_amd.models import tokenizer_train as tt
    from wmar_amd.utils import synth
    mb = max(8, args.batch_size_per_gpu)
    if args.model == "rar":
        from wmar_amd.models.rar_wrapper import RarARMMWrapper
        if args.synthetic:
            r, v = synthetic_rar_configs(args.synthetic_config)
            model = RarARMMWrapper.synthetic(r, v, seed=args.seed, max_batch=mb)
        else:
            model = RarARMMWrapper(args.modelpath, max_batch=mb)
        return model, model._vq_cfg, model._vq_cfg.num_embeddings, tt.MaskgitTrainableTokenizer
    if args.model == "chameleon7b":
        from wmar_amd.models.chameleon_wrapper import ChameleonARMMWrapper
        if args.synthetic:
            c, v = synthetic_chameleon_configs(args.synthetic_config)
            model = ChameleonARMMWrapper.synthetic(c, v, seed=args.seed, max_batch=mb)
        else:
            model = ChameleonARMMWrapper(args.modelpath, max_batch=mb)
        return model, model._vq_cfg, model._vq_cfg.n_embed, tt.TrainableTokenizer
    from wmar_amd.models.taming_wrapper import TamingARMMWrapper
    if args.synthetic:
        if args.synthetic_config == "harness":
            g, v = synth.GPTConfig(**synth.HARNESS_GPT), synth.VQConfig(**synth.HARNESS_VQ)
        elif args.synthetic_config == "harness128":     # 32 x 32 codes: the transformer (not trained) gets a sequence that long
            g = synth.GPTConfig(**dict(synth.HARNESS_GPT, block_size=1024))
            v = synth.VQConfig(**dict(synth.HARNESS_VQ, resolution=SYNTHETIC_RESOLUTION["harness128"]))
        else:
            g, v = synth.TAMING_GPT, synth.TAMING_VQ
        model = TamingARMMWrapper.synthetic(g, v, seed=args.seed, max_batch=mb)
    else:
        model = TamingARMMWrapper(args.modelpath, max_batch=mb)
    return model, model.model.vq_cfg, model.model.vq_cfg.n_embed, tt.TrainableTokenizer


def load_lpips(args, resolution: int, device):
    """The LPIPS engine the flags ask for, at the tokenizer's resolution; None without any of them."""
    if not wants_lpips(args):
        return None
    from wmar_amd.lpips import LPIPS
    if resolution % 128:
        raise SystemExit(f"finetune.py: LPIPS needs a resolution that is a multiple of 128, the tokenizer has {resolution}")
    if args.synthetic_lpips:
        from wmar_amd.utils import synth
        return LPIPS(synth.synth_lpips_state(seed=args.seed), resolution=resolution, max_batch=args.batch_size_per_gpu, device=device)
    return LPIPS.from_files(args.lpips_vgg, args.lpips_lin, resolution=resolution, max_batch=args.batch_size_per_gpu, device=device)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    check_args(args)
    import torch
    from wmar_amd.finetune import save_delta
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    model, vcfg, n_codes, tok_class = load_model(args)
    if args.datapath:
        codes = load_codes(args.datapath)
    else:
        codes = torch.randint(0, n_codes, (args.dataset_size or 4 * args.batch_size_per_gpu, vcfg.codes_size ** 2),
                              generator=torch.Generator().manual_seed(args.seed))
    if args.dataset_size:
        codes = codes[:args.dataset_size]
    if codes.shape[1] != vcfg.codes_size ** 2:
        raise SystemExit(f"finetune.py: codes have {codes.shape[1]} columns, the tokenizer has {vcfg.codes_size ** 2}")
    n_train, n_val = split_rows(codes.shape[0], args.val_percent)
    codes = codes.to(model.model.device)
    codes, val_codes = codes[:n_train], (codes[n_train:] if n_val else None)
    tokenizer = model.get_image_tokenizer()
    original = {k: v.detach().clone() for k, v in tokenizer.state_dict().items()}
    # the original decoder: forward only, on a handle without tape or gradient memory
    orig = tok_class(vcfg, {k: v.clone() for k, v in original.items()}, max_batch=args.batch_size_per_gpu, device=model.model.device, frozen=True)
    tok = model.trainable_tokenizer(max_batch=args.batch_size_per_gpu)
    lpips = load_lpips(args, vcfg.resolution, model.model.device)
    rec_loss = None
    if lpips is not None:
        from wmar_amd.finetune import reference_rec_loss
        rec_loss = reference_rec_loss(lpips, args.perceptual_weight)
    steps = train(tok, orig, codes, args, rec_loss=rec_loss, val_codes=val_codes, original=original)
    os.makedirs(args.outdir, exist_ok=True)
    for name in ("encoder", "decoder"):
        handle = getattr(tokenizer, name)
        n = len(name) + 1
        save_delta(handle.state_dict(), {k[n:]: v for k, v in original.items() if k.startswith(name + ".")},
                   os.path.join(args.outdir, f"{name}_ft_delta.pth"))
    summary = {"steps": steps, "outdir": args.outdir, "device_bytes": tok.device_bytes}
    if lpips is not None:
        summary["lpips_device_bytes"] = lpips.device_bytes
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
