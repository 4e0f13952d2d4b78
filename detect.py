"""Is this image watermarked?  Reads image files of any size and mode, brings them to the model's resolution on the GPU exactly as the
reference's PIL path does (wmar_amd.utils.ingest), encodes them and runs the watermark detector.

Takes the model and watermark flags of ``generate.py`` (the key must be the one the images were generated with) plus

    --images DIR | FILE [FILE ...]   --batch_size N   --out results.json

(``--sync true --syncpath ... | --sync_factory ...`` removes the synchronisation layer's geometric attack estimate first, as
``generate.py`` does in front of every re-encode.)

and writes one JSON list in sorted file order: ``file``, ``width``, ``height``, ``pvalue`` and the detector's counts
(``n_scored``, and ``n_green`` for the greenlist watermark; none for a ``--wm_method custom`` watermarker that only offers the
reference's ``detect``); a file PIL cannot open gets ``error`` instead, the rest are processed and the exit status is 1.
"""
import json
import os
import sys

import generate


def get_parser():
    parser = generate.get_parser()
    parser.add_argument("--images", type=str, nargs="+", help="a directory of image files, or a list of image files")
    parser.add_argument("--out", type=str, help="where to write the JSON list of results")
    return parser


def list_images(images):
    """The files of ``--images`` in sorted order: the entries of one directory (not recursive), or the files as given."""
    if len(images) == 1 and os.path.isdir(images[0]):
        d = images[0]
        return sorted(os.path.join(d, f) for f in os.listdir(d) if os.path.isfile(os.path.join(d, f)))
    return sorted(images)


def detect_codes(watermarker, codes):
    """pvalue (float64 [n]) and whatever counts the watermarker exposes, as lists per image."""
    if not hasattr(watermarker, "detect_counts"):   # a reference-style watermarker: detect(codes) -> float64 [B], no counts
        import torch
        return torch.as_tensor(watermarker.detect(codes)).reshape(-1).cpu().tolist(), {}
    res = watermarker.detect_counts(codes)          # (pvalue, n_scored[, n_green])
    counts = dict(zip(("n_scored", "n_green"), (t.cpu().tolist() for t in res[1:])))
    return res[0].cpu().tolist(), counts


def run(model, watermarker, files, batch_size, sync_manager=None):
    """One record per file, in the order given.  Batches are formed by count, whatever the images' sizes.  With a `sync_manager`
    (--sync) the synchronisation signal is read and the estimated flip / rotation / crop reverted before the images are encoded."""
    from wmar_amd.utils.ingest import open_image, pixels_of
    records = []
    for b0 in range(0, len(files), batch_size):
        batch, pix = [], []
        for f in files[b0:b0 + batch_size]:
            rec = {"file": f}
            try:
                img = open_image(f)
                rec["width"], rec["height"] = img.size
                pix.append(pixels_of(img))          # decodes the file: a truncated one fails here
                batch.append(rec)
            except Exception as e:      # PIL raises OSError / SyntaxError / ValueError subclasses for files it cannot read
                rec["error"] = f"{type(e).__name__}: {e}"
            records.append(rec)
        if not batch:
            continue
        if sync_manager is None:
            codes = model.codes_from_pil(pix)
        else:
            codes = model.images_to_codes(sync_manager.remove_sync(model.images_from_pil(pix)))
        pvals, counts = detect_codes(watermarker, codes)
        for i, rec in enumerate(batch):
            rec["pvalue"] = pvals[i]
            for k, v in counts.items():
                rec[k] = v[i]
    return records


def main():
    sys.path.append(os.getcwd())
    parser = get_parser()
    args, _ = parser.parse_known_args()
    try:
        generate.check_wm_args(args)
    except ValueError as e:
        parser.error(str(e))
    if not args.images:
        parser.error("--images is required")
    if not args.out:
        parser.error("--out is required")
    if args.wm_method in (None, "none"):
        parser.error("--wm_method: a watermark to look for is required (gentime | gumbel | custom)")
    assert args.model in ("taming", "rar", "chameleon7b"), f"Model {args.model} not supported"

    import torch

    from wmar_amd import cli
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    model = cli.build_model(args, f"cuda:{local_rank}", args.seed)
    watermarker = cli.build_watermarker(args, model)
    files = list_images(args.images)
    records = run(model, watermarker, files, max(1, args.batch_size), sync_manager=cli.build_sync_manager(args, f"cuda:{local_rank}"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
    bad = sum("error" in r for r in records)
    print(f"{len(records) - bad} images, {bad} unreadable -> {args.out}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
