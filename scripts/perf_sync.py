"""Dev tool: the synchronisation layer's device half (csrc/sync.hip).  Times, as the median of 20 event-bracketed calls after 3
warm-ups: wmar_sync_fit for B = 64 at 256^2 and B = 16 at 512^2 (label maps of tests/sync_cases.py, tiled), and a whole
WamSync.remove_sync of 64 images with the colour-coded stand-in WAM of tests/sync_standins.py (no network: normalise, positions, fit,
the [B, 4] copy, revert), and the WAM extractor at the released shape with synthetic weights: WamExtractor.detect (wmar_wamx_detect)
of 64 images at 256^2 against the float32 torch restatement of the same network (tests/wam_extractor_reference.py) on the same GPU,
and a remove_sync of the 64 images through it.  Then the host path (tests/sync_reference.py = the reference's scipy arithmetic) per image, if scipy is here.
usage: perf_sync.py [--quick]   (--quick: 3 timed calls, no host path -- for a rocprofv3 --kernel-trace --stats run)"""
import os, sys, time
import numpy as np
import torch
ROOT = os.environ.get("WMAR_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sync_cases as SC
from tests.sync_standins import ColourWam
from wmar_amd.watermarking.synchronization import WamSync

QUICK = "--quick" in sys.argv
REPS, WARM = (3, 1) if QUICK else (20, 3)
ws = WamSync(None, "cuda", wam=ColourWam("cuda"))


def median_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def tiled(S, B):
    maps = [m for _, m in SC.label_cases(S)]
    return torch.from_numpy(np.stack([maps[i % len(maps)] for i in range(B)])).cuda()


for S, B in ((256, 64), (512, 16)):
    p = tiled(S, B)
    ms = median_ms(lambda: ws.fit_best_aug_batch(p))
    print(f"wmar_sync_fit B={B} S={S}: {ms:.3f} ms per call, {ms / B * 1e3:.1f} us per image", flush=True)
imgs = torch.from_numpy(np.concatenate([SC.e2e_images()] * 16)).cuda()
ms = median_ms(lambda: ws.remove_sync(imgs))
print(f"remove_sync B=64 S=256 (stand-in WAM): {ms:.3f} ms per call (sanity bound: 125 ms, the batch's VQGAN decode + re-encode)", flush=True)
# ---- the extractor: native against the float32 torch restatement, released shape, 34 GMAC per image
from tests import wam_extractor_cases as XC
from tests import wam_extractor_reference as XR
from wmar_amd.utils import synth
from wmar_amd.watermarking.wam_extractor import WamExtractor
xcfg = synth.WAMX_RELEASED
xstate = synth.synth_wamx_state(xcfg, XC.RELEASED_SEED)
ext = WamExtractor(xcfg, xstate, "cuda", max_batch=64)
xs = XR.to_dtype(xstate, torch.float32, "cuda")
xin = torch.from_numpy(np.concatenate([XC.images_norm(XC.RELEASED_SEED, 4, 256)] * 16)).cuda()
with torch.no_grad():
    d = float((ext.detect(xin[:4])["preds"] - XR.forward(xs, xcfg, xin[:4], library=True)).abs().max())
    ms_n = median_ms(lambda: ext.detect(xin))
    ms_t = median_ms(lambda: XR.forward(xs, xcfg, xin, library=True))
gmac = 34.0 * 64
print(f"extractor detect B=64 S=256: native {ms_n:.2f} ms ({gmac * 2 / ms_n:.1f} TFLOP/s of 34 GMAC per image), float32 torch restatement "
      f"{ms_t:.2f} ms ({gmac * 2 / ms_t:.1f} TFLOP/s); max |native - torch| on 4 images {d:.3g}; engine {ext.device_bytes / 2 ** 20:.0f} MiB", flush=True)
wsx = WamSync(None, "cuda", wam=object(), extractor=ext)
ms = median_ms(lambda: wsx.remove_sync(imgs))
print(f"remove_sync B=64 S=256 (native extractor, synthetic weights): {ms:.3f} ms per call", flush=True)
if not QUICK:
    try:
        from tests import sync_reference as SR
        cases = dict(SC.label_cases(256))
        t0 = time.perf_counter(); SR.fit(cases["rot+7"]); t1 = time.perf_counter()
        SR.fit(dict(SC.label_cases(512))["rot-13"]); t2 = time.perf_counter()
        print(f"host fit (scipy, this box): {t1 - t0:.2f} s per 256^2 image, {t2 - t1:.2f} s per 512^2 image")
    except ImportError as e:
        print(f"host fit: scipy is not on this box ({e})")
