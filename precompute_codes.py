"""Images -> the codes ``finetune.py --datapath`` takes: what the reference's precompute_imagenet_codes.py does to every file -- PIL
open, ``Resize(size)`` with BILINEAR, ``RandomCrop(size)``, ``2x - 1``, the tokenizer's encoder -- with the resize, the crop and the
normalisation on the GPU (``wmar_image_ingest_filtered``, bit for bit what Pillow and torchvision return) in one call per batch.

    python precompute_codes.py --model {taming,chameleon7b,rar} (--modelpath DIR | --synthetic [--synthetic_config NAME])
        --images DIR | FILE ... --outdir OUT [--seed 1] [--batch_size 16] [--save_images]

Files are taken in sorted order.  The host opens each with ``Image.open(f).convert("RGB")`` (no alpha whitening: that belongs to
Chameleon's prompt path).  ``size`` is the tokenizer's resolution: the short side is resized to it, the long side to
``int(size * long / short)`` (torchvision's ``Resize(int)``), a side that does not change is not filtered; the crop origin is drawn per
image, in file order, top then left, from one ``torch.Generator().manual_seed(seed)``, and not at all for an image that is already
``size x size`` (``RandomCrop.get_params``).  The codes are the tokenizer's own -- ``0 .. n_embed - 1``, for Chameleon not vocabulary
ids and without the 8-bit round trip of its ``images_to_codes``.

Writes ``OUT/codes.npy`` (int64 [N, S*S]), ``OUT/files.txt`` (the files behind the rows, one per line) and, with ``--save_images``, the
cropped 8-bit images as ``OUT/images/<row>.png``.  A file PIL cannot open is reported and skipped, and the exit status is 1.  The
reference script's ImageNet label handling and its file-count assertion are not carried over.
"""
from __future__ import annotations

import argparse
import os
import sys

import finetune as ft_cli


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--model", type=str, default="taming", choices=["taming", "chameleon7b", "rar"])
    p.add_argument("--modelpath", type=str, help="the model directory, as finetune.py --modelpath")
    p.add_argument("--synthetic", action="store_true", help="random-init weights instead of --modelpath")
    p.add_argument("--synthetic_config", type=str, default="harness", choices=sorted(ft_cli.SYNTHETIC_RESOLUTION))
    p.add_argument("--images", type=str, nargs="+", required=True, help="a directory of image files, or a list of image files")
    p.add_argument("--outdir", type=str, required=True)
    p.add_argument("--seed", type=int, default=1, help="seed of the crop origins")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--save_images", action="store_true", help="also write the cropped 8-bit images as PNG")
    return p


def check_args(args) -> None:
    if bool(args.modelpath) == bool(args.synthetic):
        raise SystemExit("precompute_codes.py: give exactly one of --modelpath and --synthetic")
    if args.synthetic and args.synthetic_config not in ft_cli.SYNTHETIC_CONFIGS[args.model]:
        raise SystemExit(f"precompute_codes.py: --synthetic_config {args.synthetic_config} with --model {args.model} is not built: "
                         f"the shapes of that model are {', '.join(ft_cli.SYNTHETIC_CONFIGS[args.model])}")
    if args.batch_size < 1:
        raise SystemExit("precompute_codes.py: --batch_size must be positive")


def list_images(images):
    """The files of ``--images`` in sorted order: the entries of one directory (not recursive), or the files as given."""
    if len(images) == 1 and os.path.isdir(images[0]):
        d = images[0]
        return sorted(os.path.join(d, f) for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)))
    return sorted(images)


def vq_engine_of(model):
    """The wrapper's packed tokenizer engine (the Taming wrapper keeps it one level down)."""
    return model.vq_engine if hasattr(type(model), "vq_engine") else model.model.vq_engine


def run(engine, size: int, files, seed: int, batch_size: int, device, save_dir=None):
    """(codes int64 [N, S*S] on the host, the files behind its rows, [(file, error)] of the files PIL could not open)."""
    import numpy as np
    import torch
    from PIL import Image
    from wmar_amd import _lib
    from wmar_amd.utils import ingest
    gen = torch.Generator().manual_seed(seed)
    done, bad, rows = [], [], []
    for b0 in range(0, len(files), batch_size):
        pix, plans = [], []
        for f in files[b0:b0 + batch_size]:
            try:
                with Image.open(f) as im:
                    px = np.asarray(im.convert("RGB"))      # decodes the file: a truncated one fails here
            except Exception as e:      # PIL raises OSError / SyntaxError / ValueError subclasses for files it cannot read
                bad.append((f, f"{type(e).__name__}: {e}"))
                print(f"precompute_codes.py: cannot read {f}: {type(e).__name__}: {e}", file=sys.stderr)
                continue
            if max(px.shape[:2]) > ingest.MAX_SIDE:
                bad.append((f, f"{px.shape[1]} x {px.shape[0]} image (sides up to {ingest.MAX_SIDE})"))
                print(f"precompute_codes.py: cannot take {f}: {bad[-1][1]}", file=sys.stderr)
                continue
            new = ingest.resize_plan((px.shape[1], px.shape[0]), size)
            plans.append((new, ingest.random_crop_origin(new, size, gen)))
            pix.append(np.ascontiguousarray(px))
            done.append(f)
        if not pix:
            continue
        host, desc = ingest.pack(pix, size, plans)
        x, u8 = ingest.ingest_packed(host.to(device, non_blocking=True), desc, size, return_u8=True, filter=_lib.RESAMPLE_BILINEAR)
        rows.append(engine.encode(x).cpu())
        if save_dir is not None:
            for k, img in enumerate(u8.cpu().numpy()):
                Image.fromarray(img, "RGB").save(os.path.join(save_dir, f"{len(done) - len(pix) + k:08d}.png"))
    S = engine.cfg.codes_size
    codes = torch.cat(rows) if rows else torch.empty(0, S * S, dtype=torch.int64)
    return codes, done, bad


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    check_args(args)
    import numpy as np
    model, vcfg, _, _ = ft_cli.load_model(argparse.Namespace(model=args.model, modelpath=args.modelpath, synthetic=args.synthetic,
                                                             synthetic_config=args.synthetic_config, seed=0, batch_size_per_gpu=args.batch_size))
    os.makedirs(args.outdir, exist_ok=True)
    save_dir = os.path.join(args.outdir, "images") if args.save_images else None
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
    codes, done, bad = run(vq_engine_of(model), vcfg.resolution, list_images(args.images), args.seed, args.batch_size, model.model.device, save_dir)
    np.save(os.path.join(args.outdir, "codes.npy"), codes.numpy())
    with open(os.path.join(args.outdir, "files.txt"), "w") as fh:
        fh.writelines(f + "\n" for f in done)
    print(f"{len(done)} images, {len(bad)} unreadable -> {os.path.join(args.outdir, 'codes.npy')}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
