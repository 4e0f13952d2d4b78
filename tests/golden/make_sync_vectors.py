"""Generate tests/golden/sync_vectors.npz: what the REFERENCE's synchronisation layer (wmar/watermarking/synchronization.py)
returns for the inputs of tests/sync_cases.py.

Usage (build machine with scipy; the GPU box never runs this):
    python tests/golden/make_sync_vectors.py --ref /path/to/wmar

The reference module is loaded from its checkout (never copied) under stand-in modules for torchvision, loguru and
deps.watermark_anything, none of which the recorded methods call; a WamSync is made with ``__new__`` (no WAM checkpoint) and
``fit_best_aug`` / ``rotate_wm`` / ``find_cut`` / ``estimate_augmentation_with_wam`` / ``create_grid_mask`` are called on it.
Everything written is data, outputs only:

  fit<S>_aug      int32 [n, 4]      (rotation, cut_i, cut_j, flipped) per label case of size S, in sync_cases.label_cases order
  fit<S>_total    float64 [n, 41]   errori + errorj per angle
  rot_<case>      uint8 [5, S, S]   rotate_wm at sync_cases.ROT_ANGLES for sync_cases.ROT_CASES
  pred<k>_pos     int8 [S, S], pred<k>_sizes int32 [4], pred<k>_aug int32 [4]      per sync_cases.PRED_CASES entry
  e2e_aug         int32 [4, 4]      the fit of sync_cases.e2e_positions (the remove_sync end-to-end test)
  grid<S>         uint8 [4, S, S]   create_grid_mask at 256 and 512
  min_margin      float64           smallest |interpolated value - 0.5| over every case, label and angle

and tests/golden/sync_edge_vectors.npz for the edge inputs of sync_cases (ragged and odd sizes, every find_cut branch, ties, counts on
the threshold, wide angles, planted prediction pixels; `--only base|edge` writes one file, `--jobs N` spreads the edge fits):

  efit<S>_aug     int32 [n, 4], efit<S>_total float64 [n, 41]      per sync_cases.edge_label_cases(S) entry
  efit<S>_cuts    int32 [n, 41, 3]  (cut_i, cut_j, flipped_j) find_cut returned at every angle
  erot_<case>     uint8 [angles, S, S]   rotate_wm of sync_cases.edge_rot_cases() at each case's angles
  epos<S>_pos     int8 [3, S, S], epos<S>_sizes int32 [3, 4]       per sync_cases.edge_pred_cases() batch, image by image
  e2e512_aug      int32 [4, 4]      the fit of sync_cases.e2e_positions(512)
  min_margin      float64           as above, over every fitted case (41 angles) and every rotated map (its recorded angles)

The GPU tests demand exact equality, so no thresholded pixel may sit on a knife edge: the fp64 values scipy interpolates are
evaluated for every (case, label, angle) and none may lie within 1e-10 of the 0.5 threshold (a 16-tap fp64 sum of values <= 289
carries ~5e-13 of rounding).  A case that violates the margin needs another seed in sync_cases; it is never dropped.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
MARGIN = 1e-10


def load_reference(ref):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Logger:
        def __getattr__(self, n):
            return lambda *a, **k: None

    mod("loguru", logger=_Logger())
    tvf = mod("torchvision.transforms.functional")
    mod("torchvision.transforms", functional=tvf)
    mod("torchvision")
    saved = {k: v for k, v in sys.modules.items() if k == "deps" or k.startswith("deps.")}
    mod("deps").__path__ = []
    for name in ("deps.watermark_anything", "deps.watermark_anything.augmentation", "deps.watermark_anything.utils"):
        mod(name).__path__ = []
    mod("deps.watermark_anything.augmentation.geometric", HorizontalFlip=None, Rotate=None)
    mod("deps.watermark_anything.utils.inference_utils", load_model_from_checkpoint=None, normalize_img=None, unnormalize_img=None)
    spec = importlib.util.spec_from_file_location("ref_synchronization", os.path.join(ref, "wmar", "watermarking", "synchronization.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for k in [k for k in sys.modules if k == "deps" or k.startswith("deps.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    return m


def margin_of(positions, angles=range(-20, 21)):
    """Smallest distance of an interpolated fp64 value from the threshold, over the four labels and 41 angles."""
    from scipy import ndimage
    worst = np.inf
    for k in range(4):
        mask = (positions == k) * 255.0
        for angle in angles:
            worst = min(worst, float(np.abs(ndimage.rotate(mask, angle, reshape=False) - 0.5).min()))
    return worst


WS = None           # the reference's WamSync, set by main() before any worker process is forked


def fit_with_cuts(positions):
    """fit_best_aug, with errori + errorj and (cut_i, cut_j, flipped_j) of every angle taken from the calls it makes itself."""
    ws = WS
    totals, cuts, pending = [], [], []
    orig = ws.find_cut

    def spy(cumsums, pairs, dim, SZ):
        r = orig(cumsums, pairs, dim, SZ)
        pending.append(r)
        if len(pending) == 2:
            totals.append(float(pending[0][0] + pending[1][0]))
            cuts.append([int(pending[0][1]), int(pending[1][1]), int(bool(pending[1][2]))])
            pending.clear()
        return r

    ws.find_cut = spy
    try:
        aug = ws.fit_best_aug(positions.astype(np.int64))
    finally:
        del ws.find_cut
    assert len(totals) == 41
    return [int(aug[0]), int(aug[1]), int(aug[2]), int(bool(aug[3]))], totals, cuts


def edge_fit_job(job):
    name, pos = job
    m = margin_of(pos)
    assert m > MARGIN, f"{name}: an interpolated value lies {m:.3g} from the threshold; choose another seed"
    return (name, m) + fit_with_cuts(pos)


def edge_rot_job(job):
    name, pos, angles = job
    m = margin_of(pos, angles)
    assert m > MARGIN, f"{name}: an interpolated value lies {m:.3g} from the threshold; choose another seed"
    wm = np.zeros(pos.shape, dtype=np.int64)
    for k in range(4):
        wm[pos == k] = k + 1
    return name, m, np.stack([WS.rotate_wm(wm, a) for a in angles]).astype(np.uint8)


def write_edge(SC, torch, jobs):
    import multiprocessing
    pool = multiprocessing.get_context("fork").Pool(jobs)
    out, worst = {}, np.inf
    fits = [(f"{name}@{S}", pos) for S in SC.EDGE_FIT_SIZES for name, pos in SC.edge_label_cases(S)]
    fits += [(f"e2e512 {name}", pos) for name, pos in zip(SC.E2E, SC.e2e_positions(512))]
    res = {}
    for name, m, aug, tot, cuts in pool.imap(edge_fit_job, fits):
        print(f"{name}: {aug}  margin {m:.3g}", flush=True)
        worst = min(worst, m)
        res[name] = (aug, tot, cuts)
    for S in SC.EDGE_FIT_SIZES:
        rows = [res[f"{name}@{S}"] for name, _ in SC.edge_label_cases(S)]
        out[f"efit{S}_aug"] = np.array([r[0] for r in rows], dtype=np.int32)
        out[f"efit{S}_total"] = np.array([r[1] for r in rows], dtype=np.float64)
        out[f"efit{S}_cuts"] = np.array([r[2] for r in rows], dtype=np.int32)
    out["e2e512_aug"] = np.array([res[f"e2e512 {name}"][0] for name in SC.E2E], dtype=np.int32)
    for name, m, maps in pool.imap(edge_rot_job, SC.edge_rot_cases()):
        print(f"rot {name}: margin {m:.3g}", flush=True)
        worst = min(worst, m)
        out[f"erot_{name}"] = maps
    pool.close()
    for S, batch in SC.edge_pred_cases():
        pos = []
        for k in range(batch.shape[0]):
            _, (_, p, _) = WS.estimate_augmentation_with_wam(torch.zeros(1, 3, S, S), WS.wm_msgs, torch.from_numpy(batch[k])[None], 1,
                                                             500, idx=k)
            pos.append(np.asarray(p).astype(np.int8))
        out[f"epos{S}_pos"] = np.stack(pos)
        out[f"epos{S}_sizes"] = np.array([[(p == c).sum() for c in range(4)] for p in pos], dtype=np.int32)
        print(f"positions@{S}: sizes {out[f'epos{S}_sizes'].tolist()}", flush=True)
    out["min_margin"] = np.array(worst)
    path = os.path.join(HERE, "sync_edge_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; smallest margin", worst)


def main():
    global WS
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (facebookresearch/wmar)")
    ap.add_argument("--only", choices=("base", "edge"), help="write sync_vectors.npz or sync_edge_vectors.npz alone")
    ap.add_argument("--jobs", type=int, default=1, help="worker processes of the edge fits")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from tests import sync_cases as SC
    ref = load_reference(args.ref)
    ws = WS = ref.WamSync.__new__(ref.WamSync)
    ws.nb_msgs = 4
    ws.device = "cpu"
    ws.wm_msgs = torch.from_numpy(SC.MSGS)
    if args.only != "base":
        write_edge(SC, torch, args.jobs)
    if args.only != "edge":
        write_base(ws, SC, torch)


def write_base(ws, SC, torch):
    def fit_with_totals(positions):
        return fit_with_cuts(positions)[:2]

    out, worst = {}, np.inf
    for S in (256, 512, 128):
        augs, totals = [], []
        for name, pos in SC.label_cases(S):
            m = margin_of(pos)
            assert m > MARGIN, f"{name}@{S}: an interpolated value lies {m:.3g} from the threshold; choose another seed"
            worst = min(worst, m)
            aug, tot = fit_with_totals(pos)
            print(f"{name}@{S}: {aug}  margin {m:.3g}", flush=True)
            augs.append(aug)
            totals.append(tot)
            if S == 256 and name in SC.ROT_CASES:
                wm = np.zeros((S, S), dtype=np.int64)
                for k in range(4):
                    wm[pos == k] = k + 1
                out[f"rot_{name}"] = np.stack([ws.rotate_wm(wm, a) for a in SC.ROT_ANGLES]).astype(np.uint8)
        out[f"fit{S}_aug"] = np.array(augs, dtype=np.int32)
        out[f"fit{S}_total"] = np.array(totals, dtype=np.float64)

    for k, (seed, S, angle, fails) in enumerate(SC.PRED_CASES):
        p = torch.from_numpy(SC.preds(seed, S, angle, fails))[None]
        aug, (_, pos, _) = ws.estimate_augmentation_with_wam(torch.zeros(1, 3, S, S), ws.wm_msgs, p, 1, 500, idx=k)
        pos = np.asarray(pos).astype(np.int8)
        sizes = np.array([(pos == c).sum() for c in range(4)], dtype=np.int32)
        m = margin_of(pos)
        assert m > MARGIN, f"pred{k}: margin {m:.3g}"
        worst = min(worst, m)
        print(f"pred{k}: sizes {sizes.tolist()} aug {aug}", flush=True)
        out[f"pred{k}_pos"], out[f"pred{k}_sizes"] = pos, sizes
        out[f"pred{k}_aug"] = np.array([int(aug[0]), int(aug[1]), int(aug[2]), int(bool(aug[3]))], dtype=np.int32)

    e2e = []
    for name, pos in zip(SC.E2E, SC.e2e_positions()):
        m = margin_of(pos)
        assert m > MARGIN, f"e2e {name}: margin {m:.3g}"
        worst = min(worst, m)
        e2e.append(fit_with_totals(pos)[0])
        print(f"e2e {name}: {e2e[-1]}", flush=True)
    out["e2e_aug"] = np.array(e2e, dtype=np.int32)
    for S in (256, 512):
        out[f"grid{S}"] = ws.create_grid_mask(torch.zeros(3, S, S), 4)[:, 0].numpy().astype(np.uint8)
    out["min_margin"] = np.array(worst)
    path = os.path.join(HERE, "sync_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; smallest margin", worst)


if __name__ == "__main__":
    main()
