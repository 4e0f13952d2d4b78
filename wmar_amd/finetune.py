"""Reverse-cycle-consistency (RCC) fine-tuning of an image tokenizer: the loss of ``VQModel.forward``
(deps/taming/models/vqgan.py:93-169) and of RAR's ``PretrainedTokenizer.forward`` (deps/rar/modeling/titok.py:125-208) for the
precomputed-codes input -- the two are the same computation over ``decode`` / ``encode_prequant`` -- and the helpers of the
reference's finetune.py (``compute_and_save_delta``, ``calculate_gradient_norm``, wmar/utils/utils.py:189-227).

``tok`` is anything with ``embed(indices)``, ``decode(z_q)``, ``encode_prequant(images)``, ``quantize(z)`` and
``named_parameters(prefix)`` -- on the MI355X a ``TrainableTokenizer`` or a ``MaskgitTrainableTokenizer``
(wmar_amd/models/tokenizer_train.py).  For RAR ``decode`` is ``decode_like_taming`` (clamped, [-1, 1]) and ``encode_prequant`` takes
[-1, 1] images (titok.py:91-123), so the loss below needs no RAR branch."""
from __future__ import annotations

import math
import random
from typing import Callable, Dict, List, Optional

import torch

from .utils.utils import apply_random_augmentation


def idempotence_region(S: int, applied):
    """The slice of the S x S code grid the idempotence loss is taken over (vqgan.py:141-150; titok.py:180-189 has the same three
    cases): the inner 6/8 for ``Rotate``, the
    upper-left ``floor(S * param)`` for ``UpperLeftCropWithPadBack``, everything otherwise.  ``applied`` = (module class, parameter) or None."""
    from .augmentations.geometric import Rotate, UpperLeftCropWithPadBack
    if applied is not None and applied[0] is Rotate:
        skip = S // 8
        return slice(skip, S - skip)
    if applied is not None and applied[0] is UpperLeftCropWithPadBack:
        return slice(0, int(math.floor(S * applied[1])))
    return slice(0, S)


def rcc_loss(tok, z_indices: torch.Tensor, augmentations, p: float = 0.5, loss_weight: float = 1.0, orig=None,
             rec_loss: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None):
    """decode -> ``apply_random_augmentation`` -> re-encode -> quantize, loss ``hard-to-soft-with-ae``: the regulariser
    ``rec_loss(xrec, orig.decode(z_q))`` plus ``loss_weight`` x the mean squared difference between the original (hard) code vectors
    and the re-encoded (soft) ones over ``idempotence_region``.  ``orig``: a frozen tokenizer holding the original decoder (the
    reference's ``orig_decoder``); None drops the regulariser.  ``rec_loss`` defaults to the mean absolute difference, the L1 half of
    the reference's regulariser; ``reference_rec_loss(LPIPS(...))`` is the whole of it (L1 + LPIPS on the device, wmar_amd/lpips.py).
    A ``rec_loss`` that leaves a ``perceptual_component`` attribute behind gets it logged as ``rec_loss_perceptual_component``.
    Returns the reference's ``(loss, res_dict, log_dict, was_augmented)``."""
    z_q = tok.embed(z_indices)
    xrec = tok.decode(z_q)
    log_dict: Dict[str, float] = {}
    xrec_orig = None
    reg = xrec.new_zeros(())
    if orig is not None:
        with torch.no_grad():
            xrec_orig = orig.decode(z_q)
        reg = rec_loss(xrec, xrec_orig) if rec_loss is not None else (xrec - xrec_orig).abs().mean()
        log_dict["rec_loss"] = float(reg.detach())
        if rec_loss is not None and getattr(rec_loss, "perceptual_component", None) is not None:
            log_dict["rec_loss_perceptual_component"] = float(rec_loss.perceptual_component)
    applied = None
    xaug = xrec
    if augmentations is not None and len(augmentations) > 0:
        xaug, applied = apply_random_augmentation(xrec, augmentations, p=p)
    was_augmented = applied is not None
    zrec = tok.encode_prequant(xaug)
    zrec_q, zrec_indices = tok.quantize(zrec.detach())
    assert zrec.shape == z_q.shape, f"zrec shape {tuple(zrec.shape)} != zq shape {tuple(z_q.shape)}"
    r = idempotence_region(z_q.shape[2], applied)
    idem = torch.mean((z_q[:, :, r, r] - zrec[:, :, r, r]) ** 2)
    loss = reg + loss_weight * idem
    log_dict["idem_loss"] = float(idem.detach())
    log_dict["loss"] = float(loss.detach())
    log_dict["loss_weight"] = loss_weight
    res_dict = {"orig_z_q": z_q, "orig_z_indices": z_indices, "rec_x": xrec, "rec_x_maybe_augmented": xaug, "rec_x_orig_decoder": xrec_orig,
                "rec_z": zrec, "rec_z_q": zrec_q, "rec_z_indices": zrec_indices}
    return loss, res_dict, log_dict, was_augmented


class _rng_kept:
    """Saves the state of Python's ``random``, of torch's CPU generator and of the current device's generator, and puts all three back
    on exit: what runs inside draws (``apply_random_augmentation`` does, even at p = 1) without moving anything outside."""

    def __enter__(self):
        self._py, self._cpu = random.getstate(), torch.get_rng_state()
        self._dev = torch.cuda.get_rng_state() if torch.cuda.is_available() and torch.cuda.is_initialized() else None
        return self

    def __exit__(self, *exc):
        random.setstate(self._py)
        torch.set_rng_state(self._cpu)
        if self._dev is not None:
            torch.cuda.set_rng_state(self._dev)
        return False


def validate(tok, orig, codes: torch.Tensor, augmentations, batch_size: int, loss_weight: float,
             rec_loss: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None) -> List[dict]:
    """The reference's validation pass (finetune.py:73-128) over ``codes`` [N, S*S]: for ``[(Identity, [0])] + augmentations`` and every
    parameter of every entry, ``rcc_loss(tok, batch, [(cls, [param])], p=1.0, ...)`` under ``torch.no_grad()`` on batches of
    ``batch_size`` (the last may be short), with ``l0 = mean(orig_z_indices != rec_z_indices)`` added; every logged value is averaged
    over rows, weighted by the batch size (:86-99).  One record per (transform, parameter): ``aug`` (class name), ``param``, ``n`` and
    the averages.  Nothing is trained and no tape is touched: the forwards run on the tokenizer's no-grad engine.  The states of Python's
    ``random`` and of torch's CPU and current-device generators are the same after the call as before it, so a run that validates
    trains exactly as one that does not."""
    from .augmentations.geometric import Identity
    records = []
    with _rng_kept(), torch.no_grad():
        for cls, params in [(Identity, [0])] + list(augmentations or []):
            for param in params:
                sums: Dict[str, float] = {}
                n = 0
                for b0 in range(0, codes.shape[0], batch_size):
                    batch = codes[b0:b0 + batch_size]
                    _, res, log, _ = rcc_loss(tok, batch, [(cls, [param])], p=1.0, loss_weight=loss_weight, orig=orig, rec_loss=rec_loss)
                    log["l0"] = float((res["orig_z_indices"] != res["rec_z_indices"]).float().mean())
                    for k, v in log.items():
                        sums[k] = sums.get(k, 0.0) + v * batch.shape[0]
                    n += batch.shape[0]
                rec = {"aug": cls.__name__, "param": param, "n": n}
                rec.update({k: v / n for k, v in sums.items()})
                records.append(rec)
    return records


def weight_distance(state: Dict[str, torch.Tensor], original_state: Dict[str, torch.Tensor], prefix: str) -> float:
    """The mean over the tensors under ``prefix`` of ``||a - b||_2`` between ``state`` and ``original_state`` (``get_decoder_dist`` /
    ``get_encoder_dist``, wmar/utils/utils.py:180-186)."""
    dists = [torch.norm(v.detach() - original_state[k].detach().to(v.device)) for k, v in state.items() if k.startswith(prefix)]
    return float(torch.mean(torch.stack(dists))) if dists else 0.0


class reference_rec_loss:
    """The reference's regulariser ``torch.mean(|x_orig_dec - x_rec| + perceptual_weight * LPIPS(x_orig_dec, x_rec))``
    (deps/taming/modules/losses/vqperceptual.py:83-92 with the GAN off; deps/rar/modeling/titok.py:113-115) as a ``rec_loss`` of
    ``rcc_loss``: ``(xrec, xrec_orig) -> mean|xrec - xrec_orig| + perceptual_weight * mean_b lpips(xrec, xrec_orig)``.  The mean of the
    broadcast sum is the sum of the two means.  LPIPS is symmetric in its arguments (every term is ``(n0 - n1)^2``), so handing it
    ``xrec`` first changes no bit of the value and puts the gradient where the reference has it, on ``xrec``.  ``perceptual_component``
    holds the last call's ``mean_b LPIPS`` (the reference logs it as ``vqgan_rec_loss_perceptual_component``)."""

    def __init__(self, lpips, perceptual_weight: float = 1.0):
        self.lpips, self.perceptual_weight = lpips, float(perceptual_weight)
        self.perceptual_component: Optional[torch.Tensor] = None

    def __call__(self, xrec: torch.Tensor, xrec_orig: torch.Tensor) -> torch.Tensor:
        p = self.lpips(xrec, xrec_orig).mean()
        self.perceptual_component = p.detach()
        return (xrec - xrec_orig).abs().mean() + self.perceptual_weight * p


def save_delta(trained_state: Dict[str, torch.Tensor], original_state: Dict[str, torch.Tensor], path: str) -> Dict[str, torch.Tensor]:
    """Writes ``{key: trained - original}`` (CPU tensors) for the keys both states hold: what ``update_weights(module, path, delta=True)``
    adds back (``compute_and_save_delta``, wmar/utils/utils.py:215-227).  Keys are relative to the module the delta is for."""
    diff = {}
    for k, v in trained_state.items():
        if k in original_state:
            diff[k] = v.detach().cpu() - original_state[k].detach().cpu()
        else:
            print(f"Diffing Warning: Key {k} not found in original state dict")
    torch.save(diff, path)
    return diff


def calculate_gradient_norm(tok, prefix: str) -> float:
    """sqrt(sum |grad|^2 / parameter count) over the parameters under ``prefix`` (wmar/utils/utils.py:189-213); a parameter without a
    gradient counts with norm 0."""
    total, count = 0.0, 0
    for _, prm in tok.named_parameters(prefix):
        if prm.grad is not None:
            total += float(torch.norm(prm.grad)) ** 2
        count += prm.numel()
    return math.sqrt(total / count) if count else 0.0
