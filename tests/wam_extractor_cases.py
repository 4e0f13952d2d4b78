"""Inputs the WAM extractor tests and tests/golden/make_wam_extractor_vectors.py share.  numpy only; nothing here is stored in the
fixture."""
import os

import numpy as np

from tests import wam_cases as WC

SMALL_SEED, RELEASED_SEED = 21, 22        # synth_wamx_state seeds of the two recorded networks
SMALL_B, RELEASED_B = 3, 1
MARGIN_MULT = 8                           # a pixel is "near" when some channel has |preds64| < MARGIN_MULT * preds_err[0] ...
NEAR_CAP = 0.01                           # ... at most this share of any image

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(1, 3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(1, 3, 1, 1)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# fixture files (each below 1 MiB) and the arrays they hold
FILES = {
    "wam_extractor_tokens.npz": ["s_tokens0", "s_tokens1", "s_tokens2", "s_tokens3", "s_tokens4"],
    "wam_extractor_stages.npz": ["s_neck", "s_up0"],
    "wam_extractor_up1.npz": ["s_up1_img0", "r_signs"],      # r_signs rides here: next to r_preds64_sub it would pass the limit
    "wam_extractor_up2.npz": ["s_up2_img0"],
    "wam_extractor_small.npz": ["s_preds64_sub", "s_signs", "s_near", "s_preds_err", "s_near_share"],
    "wam_extractor_released.npz": ["r_preds64_sub", "r_near", "r_preds_err", "r_near_share"],
}


def images_norm(seed, B, R):
    """float32 [B, 3, R, R]: wam_cases.images01 normalised in float32, what ``detect`` is handed."""
    return ((WC.images01(seed, B, R) - MEAN) / STD).astype(np.float32)


def pred_subset(R):
    """Every 5th row / column and the last one: 5 is coprime to the 16-fold upsampling, so every interpolation phase and both
    reflected borders occur."""
    return sorted(set(range(0, R, 5)) | {R - 1})


def load():
    """All fixture arrays in one dict."""
    out = {}
    for name in FILES:
        with np.load(os.path.join(GOLDEN, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out
