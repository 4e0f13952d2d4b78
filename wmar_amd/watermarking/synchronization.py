"""The synchronisation layer of the reference (``wmar/watermarking/synchronization.py``): ``WamSync``, ``SyncSeal`` and
``SyncManager`` with the reference's public surface, for the MI355X build.

The neural half (the WAM embedder / extractor, the SyncSeal TorchScript) is ordinary PyTorch and is NOT part of this package: it is
bound from the user's own checkout or handed in as an object -- except the WAM networks at their own image size, which
``WamSync(..., embedder=..., extractor=...)`` runs on the device from the checkpoint's ``embedder.*`` / ``detector.*`` tensors
(wam_embedder.py, wmar_amd/csrc/wam.h: ``wmar_wam_add_sync``; wam_extractor.py, wmar_amd/csrc/wam_extractor.h:
``wmar_wamx_detect``).  What the reference computes on the host per image -- the message
label of every pixel, and ``fit_best_aug``: four label masks rotated by 41 angles with ``scipy.ndimage.rotate``, thresholded, counted
and searched for the best cut and flip (2.3 s per 256 x 256 image) -- runs here as kernels over the whole batch
(wmar_amd/csrc/sync.hip: ``wmar_sync_positions``, ``wmar_sync_fit``, ``wmar_sync_rotate_labels``), and ``remove_sync`` copies one
``[B, 4]`` table to the host per batch.  There is no host fallback: the fit needs tensors on the GPU.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from ..augmentations.geometric import HorizontalFlip, Rotate, resize_bilinear

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
N_ANGLES = 41                       # fit_best_aug tries -20 .. 20 degrees
WORKSPACE_CAP = 256 << 20           # spline coefficients are 32 bytes per pixel: larger batches are walked in chunks inside the call

WAM_IMPORT = "deps.watermark_anything.utils.inference_utils"


def _load_wam(syncpath, device):
    """The WAM network from the user's reference checkout (its ``deps/watermark_anything``)."""
    try:
        import importlib
        load_model_from_checkpoint = importlib.import_module(WAM_IMPORT).load_model_from_checkpoint
    except ImportError as e:
        raise ImportError(
            f"WamSync needs the WAM network, which this package does not ship: `from {WAM_IMPORT} import "
            f"load_model_from_checkpoint` failed ({e}); looked on sys.path, working directory {os.getcwd()}. "
            "Run from a checkout of the reference with deps/watermark_anything in place, or pass wam=<object with "
            "embed(imgs, msg) -> {'imgs_w'} and detect(imgs) -> {'preds'}>.") from e
    json_path = os.path.join("deps", "watermark_anything", "params.json")
    return load_model_from_checkpoint(json_path, os.path.join(syncpath)).to(device).eval()


def _square(t, what):
    if t.shape[-1] != t.shape[-2]:
        raise ValueError(f"{what}: {t.shape[-2]} x {t.shape[-1]} -- the synchronisation layer assumes square images throughout")
    return int(t.shape[-1])


def _workspace(L, B, S, device):
    full = int(L.wmar_sync_workspace_bytes(B, S))
    least = int(L.wmar_sync_workspace_bytes(B, S)) - (B - 1) * S * S * 32
    return torch.empty(max(least, min(full, WORKSPACE_CAP)), dtype=torch.uint8, device=device)


def _positions_arg(positions, device):
    p = torch.as_tensor(positions)
    if p.dim() == 2:
        p = p.unsqueeze(0)
    if p.dim() != 3:
        raise ValueError(f"label maps must be [B, S, S] or [S, S], got {tuple(p.shape)}")
    _square(p, "label map")
    p = p.to(device=device, dtype=torch.int8).contiguous()
    if not p.is_cuda:
        raise RuntimeError("the geometry fit runs on the GPU (wmar_sync_fit); there is no host fallback")
    return p


class WamSync:
    def __init__(self, syncpath, device, wam=None, embedder=None, extractor=None):
        """``embedder``: a ``WamEmbedder`` (wam_embedder.py), or "native" to build one from ``syncpath``.  With one, ``add_sync`` on
        images of its resolution is one device call and the PyTorch network is only loaded at the first ``remove_sync`` (or the
        first ``add_sync`` of another image size).  ``extractor``: a ``WamExtractor`` (wam_extractor.py), or "native": the detect of
        ``remove_sync`` on images of its size is one device call as well; with both, nothing is imported from a checkout unless
        an image of another size arrives."""
        self.device = device
        self.syncpath = syncpath
        if isinstance(embedder, str):
            if embedder != "native":
                raise ValueError(f"embedder {embedder!r}: a WamEmbedder or 'native'")
            from .wam_embedder import WamEmbedder
            embedder = WamEmbedder.from_checkpoint(syncpath, device)
        if isinstance(extractor, str):
            if extractor != "native":
                raise ValueError(f"extractor {extractor!r}: a WamExtractor or 'native'")
            from .wam_extractor import WamExtractor
            extractor = WamExtractor.from_checkpoint(syncpath, device)
        self.embedder = embedder
        self.extractor = extractor
        self._wam = wam
        if wam is None and embedder is None and extractor is None:
            self._wam = _load_wam(syncpath, device)
        self.epsilon = 1
        self.min_samples = 500
        self.wm_msgs = torch.tensor([[0] * 32, [0] * 16 + [1] * 16, [1] * 16 + [0] * 16, [1] * 32]).to(device)
        self.nb_msgs = 4
        self._mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=device).view(1, 3, 1, 1)
        self._std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=device).view(1, 3, 1, 1)
        self._flip, self._rotate = HorizontalFlip(), Rotate()

    @property
    def wam(self):
        """The PyTorch network (embed / detect): handed in, loaded at construction, or -- with a native embedder or extractor --
        loaded from the user's checkout when it is first needed."""
        if self._wam is None:
            self._wam = _load_wam(self.syncpath, self.device)
        return self._wam

    @wam.setter
    def wam(self, value):
        self._wam = value

    # transfer to WAM space, [-1, 1] -> [0, 1] + normalized
    def normalize(self, imgs):
        return ((imgs + 1.0) / 2.0 - self._mean.to(imgs.device)) / self._std.to(imgs.device)

    # transfer from WAM space, [0, 1] + normalized -> [-1, 1]
    def unnormalize(self, imgs):
        imgs = (imgs * self._std.to(imgs.device) + self._mean.to(imgs.device)) * 2.0 - 1.0
        return imgs.clamp(-1, 1)

    def create_grid_mask(self, img_pt, num_masks):
        """[num_masks, 1, H, W]: message k in the k-th square of the 2 x 2 grid, a cross of 19 (37 beyond 256) pixels left free."""
        H, W = img_pt.shape[-2], img_pt.shape[-1]
        masks = torch.zeros((num_masks, 1, H, W))
        n = int(np.sqrt(self.nb_msgs))
        q = W // n
        for i in range(n):
            for j in range(n):
                masks[i * n + j, 0, i * q:(i + 1) * q, j * q:(j + 1) * q] = 1
        mid = W // 2
        leeway = 18 if W == 256 else 36
        a, b = mid - leeway // 2, mid + leeway // 2 + 1
        masks[:, :, :, a:b] = 0
        masks[:, :, a:b, :] = 0
        return masks.to(img_pt.device)

    # ---- the device half -----------------------------------------------------------------------------------------------------
    def positions_from_preds(self, preds):
        """preds fp32 [B, 33, S, S] on the GPU -> (positions int8 [B, S, S] in {-1, 0..3}, sizes int32 [B, 4]); one launch."""
        if preds.dim() != 4 or preds.shape[1] != 33:
            raise ValueError(f"WAM predictions must be [B, 33, S, S], got {tuple(preds.shape)}")
        S = _square(preds, "WAM predictions")
        if not preds.is_cuda:
            raise RuntimeError("positions_from_preds runs on the GPU (wmar_sync_positions); there is no host fallback")
        preds = preds.to(torch.float32).contiguous()
        B = preds.shape[0]
        positions = torch.empty(B, S, S, dtype=torch.int8, device=preds.device)
        sizes = torch.empty(B, 4, dtype=torch.int32, device=preds.device)
        L = _lib.load()
        with torch.cuda.device(preds.device):
            _lib.check(L.wmar_sync_positions(preds.data_ptr(), B, S, positions.data_ptr(), sizes.data_ptr(), _lib.stream_ptr(preds.device)))
        return positions, sizes

    def _fit(self, positions, want_total):
        p = _positions_arg(positions, self.device)
        B, S = p.shape[0], p.shape[-1]
        aug = torch.empty(B, 4, dtype=torch.int32, device=p.device)
        total = torch.empty(B, N_ANGLES, dtype=torch.float64, device=p.device) if want_total else None
        L = _lib.load()
        ws = _workspace(L, B, S, p.device)
        with torch.cuda.device(p.device):
            _lib.check(L.wmar_sync_fit(p.data_ptr(), B, S, aug.data_ptr(), total.data_ptr() if want_total else None, ws.data_ptr(),
                                       ws.numel(), _lib.stream_ptr(p.device)))
        return aug, total

    def fit_best_aug_batch(self, positions):
        """int32 [B, 4] = (rotation, cut_i, cut_j, flipped) per label map, on the device."""
        return self._fit(positions, False)[0]

    def fit_total_error(self, positions):
        """float64 [B, 41]: errori + errorj of every angle -20 .. 20."""
        return self._fit(positions, True)[1]

    def rotated_labels(self, positions, angle):
        """uint8 [B, S, S]: the reference's ``rotate_wm(wm, angle)`` (labels 1..4, 0 = background) of every map."""
        p = _positions_arg(positions, self.device)
        B, S = p.shape[0], p.shape[-1]
        out = torch.empty(B, S, S, dtype=torch.uint8, device=p.device)
        L = _lib.load()
        ws = _workspace(L, B, S, p.device)
        with torch.cuda.device(p.device):
            _lib.check(L.wmar_sync_rotate_labels(p.data_ptr(), B, S, int(angle), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _lib.stream_ptr(p.device)))
        return out

    def fit_best_aug(self, positions):
        """One label map [S, S] -> (rotation, cut_i, cut_j, flipped), as the reference returns it."""
        r, ci, cj, fl = self.fit_best_aug_batch(positions)[0].tolist()
        return (r, ci, cj, bool(fl))

    def estimate_augmentation_with_wam(self, imgs, preds):
        """Batched form of the reference's method: imgs [B, 3, H, H] (only their size is read), preds [B, 33, h, h] ->
        (aug int32 [B, 4] on the device, (positions, sizes)).  Images that fail the confidence gate get (0, H // 2, H // 2, 0)."""
        H = _square(imgs, "image")
        if preds.shape[-1] != H or preds.shape[-2] != H:
            # the reference resizes the mask probabilities and the bit logits separately; the mask is only compared with 0.5
            mask = F.interpolate(torch.sigmoid(preds[:, :1]), size=(H, H), mode="bilinear", align_corners=False)
            bits = F.interpolate(preds[:, 1:], size=(H, H), mode="bilinear", align_corners=False)
            preds = torch.cat([torch.logit(mask), bits], dim=1)
        positions, sizes = self.positions_from_preds(preds)
        aug = self.fit_best_aug_batch(positions)
        thresh = round((H * H) * (0.7 if H == 256 else 0.75))
        dummy = torch.tensor([0, H // 2, H // 2, 0], dtype=torch.int32, device=aug.device)
        aug = torch.where((sizes.sum(dim=1) < thresh)[:, None], dummy[None], aug)
        return aug, (positions, sizes)

    def revert_augmentation(self, imgs, aug_info):
        """The reference's revert for ONE estimate applied to every image of `imgs` [b, 3, H, H] (WAM-normalised pixels)."""
        H = _square(imgs, "image")
        angle, cuti, cutj, is_flipped = aug_info
        if is_flipped:
            return self._flip(imgs)
        if abs(angle) >= 3:
            return self._rotate(imgs, angle)
        pad_thresh = 10 if H == 256 else 25
        pad_i = 2 * cuti - H
        pad_i = 0 if pad_i < pad_thresh else pad_i
        pad_j = max(0, 2 * cutj - H)
        pad_j = 0 if pad_j < pad_thresh else pad_j
        if pad_i == 0 and pad_j == 0:
            return imgs                              # a resize to the size the image already has
        return resize_bilinear(F.pad(imgs, (0, pad_j, 0, pad_i)), (H, H))

    def revert_batch(self, imgs, aug):
        """Per-image revert with the images grouped by what is done to them: one launch for the flipped ones, one per distinct angle,
        one pad + resize per distinct padding.  aug: [B, 4] on the host."""
        groups = {}
        for i, a in enumerate(aug):
            a = tuple(int(v) for v in a)
            H = imgs.shape[-1]
            pad_thresh = 10 if H == 256 else 25
            if a[3]:
                key = ("flip",)
            elif abs(a[0]) >= 3:
                key = ("rot", a[0])
            else:
                pad = [0 if p < pad_thresh else p for p in (2 * a[1] - H, max(0, 2 * a[2] - H))]
                key = ("crop", pad[0], pad[1])
            groups.setdefault(key, (a, []))[1].append(i)
        if len(groups) == 1:
            (a, _), = groups.values()
            return self.revert_augmentation(imgs, (a[0], a[1], a[2], bool(a[3])))
        out = torch.empty_like(imgs)
        for a, idx in groups.values():
            idx = torch.tensor(idx, device=imgs.device)
            out[idx] = self.revert_augmentation(imgs[idx], (a[0], a[1], a[2], bool(a[3])))
        return out

    # imgs: [b, 3, 256, 256] in [-1, 1] -> return same
    @torch.no_grad()
    def add_sync(self, imgs, return_masks=False):
        orig_device = imgs.device
        emb = self.embedder
        if emb is not None and imgs.dim() == 4 and imgs.shape[-1] == emb.cfg.resolution and imgs.shape[-2] == emb.cfg.resolution:
            # the whole method as one call: normalise, 1 encoder + K decoder passes, blend, unnormalise (wmar_wam_add_sync)
            dev = getattr(emb, "device", self.device)
            x = imgs.to(dev)
            masks = self.create_grid_mask(x[-1], num_masks=len(self.wm_msgs))
            ret = emb.add_sync(x, self.wm_msgs.to(dev), masks).to(orig_device)
            return (ret, masks) if return_masks else ret
        imgs = self.normalize(imgs.to(self.device))
        masks = self.create_grid_mask(imgs[-1], num_masks=len(self.wm_msgs))
        multi = imgs.clone()
        for k in range(len(self.wm_msgs)):
            msg = self.wm_msgs[k].unsqueeze(0).expand(imgs.shape[0], -1)
            multi = self.wam.embed(imgs, msg)["imgs_w"] * masks[k] + multi * (1 - masks[k])
        ret = self.unnormalize(multi).to(orig_device)
        return (ret, masks) if return_masks else ret

    # imgs: [b, 3, 256, 256] in [-1, 1] -> return same
    @torch.no_grad()
    def remove_sync(self, imgs, return_info=False):
        """One WAM detect over the batch, one positions launch, one batched fit, one [B, 4] copy to the host, then the revert."""
        orig_device = imgs.device
        imgs = self.normalize(imgs.to(self.device))
        _square(imgs, "image")
        ext = self.extractor
        if ext is not None and imgs.shape[-1] == ext.cfg.img_size:
            preds = ext.detect(imgs.to(getattr(ext, "device", self.device)))["preds"].to(imgs.device)      # wmar_wamx_detect
        else:
            preds = self.wam.detect(imgs)["preds"]      # [B, 33, h, h]
        aug, wam_info = self.estimate_augmentation_with_wam(imgs, preds)
        aug_host = aug.cpu().tolist()
        reverted = self.unnormalize(self.revert_batch(imgs, aug_host)).to(orig_device)
        if return_info:
            return reverted, [(a[0], a[1], a[2], bool(a[3])) for a in aug_host], wam_info
        return reverted


class SyncSeal:
    def __init__(self, syncpath, device, model=None):
        self.model = model if model is not None else torch.jit.load(syncpath, map_location=device).eval()
        self.device = device

    # transfer to SYNC space, [-1, 1] -> [0, 1]
    def normalize(self, imgs):
        return (imgs + 1.0) / 2.0

    # transfer from SYNC space, [0, 1]-> [-1, 1]
    def unnormalize(self, imgs):
        return (imgs * 2.0 - 1.0).clamp(-1, 1)

    def add_sync(self, imgs, return_masks=False):
        assert not return_masks, "return_masks not supported for SyncSeal"
        orig_device = imgs.device
        with torch.no_grad():
            imgs_w = self.model.embed(self.normalize(imgs).to(self.device))["imgs_w"]
        return self.unnormalize(imgs_w).to(orig_device)

    def remove_sync(self, imgs, return_info=False):
        assert not return_info, "return_info not supported for SyncSeal"
        orig_device = imgs.device
        orig_size = imgs.shape[-2], imgs.shape[-1]
        imgs = self.normalize(imgs).to(self.device)
        with torch.no_grad():
            pred_pts = self.model.detect(imgs)["preds_pts"]        # Bx8 normalized [-1,1]
            unwarped = self.model.unwarp(imgs, pred_pts, orig_size)
        return self.unnormalize(unwarped).to(orig_device)


class SyncManager:
    """Dispatch on the checkpoint's file name as the reference does; ``sync`` injects a ready WamSync / SyncSeal-like object."""

    def __init__(self, syncpath, device, sync=None):
        if sync is not None:
            self.sync = sync
        elif "wam_mit" in str(syncpath):
            self.sync = WamSync(syncpath, device)
        elif "syncmodel.jit.pt" in str(syncpath):
            self.sync = SyncSeal(syncpath, device)
        else:
            raise NotImplementedError(f"Unknown wam model {syncpath}")
        self.last_seconds = {}

    # imgs: [b, 3, 256, 256] in [-1, 1] -> return same
    def add_sync(self, imgs, return_masks=False):
        t = time.time()
        ret = self.sync.add_sync(imgs, return_masks)
        self.last_seconds["add_sync"] = time.time() - t
        return ret

    # imgs: [b, 3, 256, 256] in [-1, 1] -> return same
    def remove_sync(self, imgs, return_info=False):
        t = time.time()
        ret = self.sync.remove_sync(imgs, return_info)
        self.last_seconds["remove_sync"] = time.time() - t
        return ret
