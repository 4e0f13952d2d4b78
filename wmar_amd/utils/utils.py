"""Mirror of the pieces of ``wmar.utils.utils`` the generation harness and a fine-tuning loop use
(wmar/utils/utils.py:25-80): the random training augmentation, uint8 conversion and delta-checkpoint patching."""
from __future__ import annotations

import random
from typing import Union

import numpy as np
import torch
from PIL import Image


def apply_random_augmentation(x, augmentations, p=0.5):
    """One training-time augmentation of a [-1, 1] batch, behaving as the function of this name in wmar/utils/utils.py.

    `augmentations` lists ``(module class, candidate parameters)`` pairs.  The host RNG is consulted in a fixed order -- a uniform
    draw compared with `p`, then the pair, then the parameter -- and never more often than needed, so a seeded run picks what the
    reference picks.  Returns ``(x, None)`` when nothing is applied (empty list, the draw is not below `p`, or the pair is
    ``Identity``), else ``(augmented, (cls, parameter))``.  The modules work in [0, 1], so the batch is mapped there and back; the
    gradient reaches `x` through the transform (on the MI355X through ``wmar_augment_backward``), except for ``JPEG``, whose
    result only replaces the value of `x`: its gradient is the identity."""
    from ..augmentations.geometric import Identity
    from ..augmentations.valuemetric import JPEG
    untouched = (x, None)
    if not augmentations or random.random() >= p:
        return untouched
    module_cls, candidates = random.choice(augmentations)
    if module_cls is Identity:
        return untouched
    chosen = random.choice(candidates)
    augmented = 2.0 * module_cls()(0.5 * x + 0.5, chosen) - 1.0
    if module_cls is JPEG:
        augmented = x + (augmented - x).detach()
    return augmented, (module_cls, chosen)


def simple_rescale(x):
    return (x + 1.0) / 2.0


# Rescale to [0, 1], clip (!), transpose, rescale to [0, 255], convert to uint8 -> PIL image
def chw_to_pillow(x: Union[torch.Tensor, np.ndarray]) -> Image.Image:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = (255 * simple_rescale(x.transpose(1, 2, 0))).clip(0, 255)
    x = np.round(x).astype(np.uint8)  # round-half-even, like the reference
    return Image.fromarray(x)


def tolerant_torch_load(path):
    """``torch.load(path, map_location="cpu", weights_only=False)`` of the reference, without its installed packages: Lightning
    checkpoints pickle objects of pytorch_lightning / omegaconf; only ``state_dict`` matters, so unknown classes are replaced
    by inert stand-ins while unpickling."""
    import pickle
    from types import SimpleNamespace
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        pass

    class _Stub:
        def __init__(self, *a, **k):
            pass

        def __setstate__(self, s):
            pass

    class _Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            try:
                return super().find_class(module, name)
            except Exception:
                return _Stub

    pm = SimpleNamespace(Unpickler=_Unpickler, load=lambda f, **k: _Unpickler(f, **k).load(), __name__="tolerant_pickle")
    return torch.load(path, map_location="cpu", weights_only=False, pickle_module=pm)


def update_weights(model, ckpt_path, delta=True, *legacy):  # Deltas!
    """wmar/utils/utils.py:47-66, same signature and semantics: ``model`` is anything with ``state_dict()`` and
    ``load_state_dict(sd, strict=False)`` -- the handles ``get_image_tokenizer().encoder`` / ``.decoder`` return
    (generate.py:327-332) or a torch module.  ``delta=True`` ADDS the checkpoint's tensors to the current ones key by key
    (keys the model lacks are carried along and then ignored by the non-strict load, as in the reference).

    Earlier rounds' form ``update_weights(wrapper, "encoder" | "decoder", ckpt_path[, delta])`` is still accepted."""
    if isinstance(ckpt_path, str) and ckpt_path in ("encoder", "decoder") and hasattr(model, "get_image_tokenizer"):
        which, ckpt_path = ckpt_path, delta
        delta = legacy[0] if legacy else True
        model = getattr(model.get_image_tokenizer(), which)
    state_dict = tolerant_torch_load(ckpt_path)
    if "state_dict" in state_dict:
        state_dict = state_dict["state_dict"]

    if delta:
        state_dict_to_apply = dict(model.state_dict())
        for key in state_dict:
            if key in state_dict_to_apply:
                cur = state_dict_to_apply[key]
                state_dict_to_apply[key] = cur + state_dict[key].to(cur.device)
            else:
                state_dict_to_apply[key] = state_dict[key]
    else:
        state_dict_to_apply = state_dict

    return model.load_state_dict(state_dict_to_apply, strict=False)
