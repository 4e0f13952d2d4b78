"""Dev tool: the device JPEG round trip (wmar_jpeg, csrc/jpeg.hip) in the harness's fused form on a [B, 3, R, R] batch, per quality
of the AugmentationManager table: microseconds per call (device events), bytes moved against the HBM floor of reading the batch once
and writing it once, and PIL's time for the same batch on the host.  usage: perf_jpeg.py [batch=64] [res=256]"""
import os, sys, time
import torch
ROOT = os.environ.get("WMAR_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wmar_amd.augmentations import device_ops as D
from wmar_amd.augmentations.valuemetric import JPEG

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
R = int(sys.argv[2]) if len(sys.argv) > 2 else 256
QS = [100, 95, 85, 75, 65, 55, 45, 35, 25, 15, 5]
px = B * R * R
floor_b = px * 3 * 4 * 2                              # fp32 in + out
moved_b = px * (3 * 4 + 1.5) + px * (1.5 + 3 * 4 + 3 * 4)   # k_jpeg_code: in + samples; k_jpeg_out: samples + in + out
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.rand(B, 3, R, R, device="cuda", generator=g) * 2 - 1
for q in QS:
    D.fused("jpeg", x, q)
torch.cuda.synchronize()
reps = 50
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
tot = 0.0
for q in QS:
    e0.record()
    for _ in range(reps):
        D.fused("jpeg", x, q)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    tot += us
    print(f"q={q:3d}: {us:8.1f} us per call ({px / us / 1e3:.2f} Gpx/s; {moved_b / us / 1e6:.2f} TB/s of {moved_b / 1e6:.0f} MB moved; "
          f"floor {floor_b / 1e6:.0f} MB)")
print(f"batch {B} x {R}^2, 11 qualities: {tot:.0f} us on the device")
xc = (x[:8].cpu() / 2 + 0.5)
t0 = time.perf_counter()
JPEG()(xc, 75)
dt = time.perf_counter() - t0
print(f"host PIL path: {dt / 8 * 1e3:.2f} ms per {R}^2 image per quality ({dt / 8 * B * 11:.2f} s for the batch's 11 qualities)")
