"""Dev tool: the WAM embedder on the device (csrc/wam.h).  Times WamEmbedder.add_sync (4 messages, the reference's grid masks) at the
released shape, 256 x 256, for batches of 16 and 64 images with max_batch = 64 decoder rows, as the median of 10 event-bracketed calls
after 2 warm-ups, and the three kernels of its own alone (probes wait for the stream: wall clock of the call).
usage: perf_wam.py [--quick]   (--quick: 2 timed calls)"""
import os, sys, time
import numpy as np
import torch
ROOT = os.environ.get("WMAR_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import wam_cases as WC
from wmar_amd import _lib
from wmar_amd.utils import synth
from wmar_amd.watermarking.synchronization import WamSync
from wmar_amd.watermarking.wam_embedder import WamEmbedder

QUICK = "--quick" in sys.argv
REPS, WARM = (2, 1) if QUICK else (10, 2)
cfg = synth.WAM_RELEASED
emb = WamEmbedder(cfg, synth.synth_wam_state(cfg, WC.RELEASED_SEED), "cuda", max_batch=64)
ws = WamSync(None, "cuda", wam=object(), embedder=emb)
print(f"embedder at {cfg.resolution}^2, max_batch 64 decoder rows: {emb.device_bytes / 2 ** 20:.0f} MiB on the device", flush=True)


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


for B in (16, 64):
    imgs = torch.from_numpy(np.concatenate([WC.images_pm1(WC.RELEASED_SEED, 4, 256)] * (B // 4))).cuda()
    ms = median_ms(lambda: ws.add_sync(imgs))
    print(f"add_sync B={B} S=256 (1 encoder pass + 4 decoder rows per image): {ms:.2f} ms per call, {ms / B:.3f} ms per image", flush=True)

L = _lib.load()
u = torch.from_numpy(WC.images01(WC.RELEASED_SEED, 4, 256)).cuda().repeat(16, 1, 1, 1).contiguous()
heat = torch.empty(64, 256, 256, device="cuda")
torch.cuda.synchronize()
for _ in range(3):
    t0 = time.perf_counter()
    _lib.check(L.wmar_wam_probe_jnd(u.data_ptr(), 64, 256, heat.data_ptr(), _lib.stream_ptr("cuda")))
    dt = time.perf_counter() - t0
print(f"k_wam_jnd B=64 S=256: {dt * 1e3:.3f} ms per call including launch and wait ({64 * 256 * 256 * 16 / dt / 1e9:.0f} GB/s of 16 B per pixel)")
