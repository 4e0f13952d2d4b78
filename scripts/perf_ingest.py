"""Timing of the image ingest on one GPU: 64 images each at 4000x3000, 1920x1080 and 1024x1024 to targets 512
and 256.

    python scripts/perf_ingest.py [--runs 5] [--batch 64] [--log profiles/ingest_perf.log]

Per (size, target), from uint8 arrays already decoded on the host (both paths start there):
  pack       host clock around pack(): one thread copies every image into a pinned buffer and builds the descriptors; `first` is the
             very first call for this size (the pinned allocation included), `warm` the median of the later ones
  upload     HIP events around the host-to-device copy of the packed pixels
  ingest     HIP events around wmar_image_ingest (host table construction, two launches, the wait)
  e2e        host clock around ingest(arrays, T, "cuda") as a user calls it (pack + upload + device call), ending in a synchronise
and, as the baseline a user has without the device path, PIL's resize(LANCZOS) + crop on this machine's host from PIL images: one
thread, and a 16-thread pool.  Bytes read per image = the input region the crop window touches; the HBM fraction uses 8 TB/s."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def pil_one(img, T):
    from wmar_amd.utils.ingest import plan
    new, (x0, y0) = plan(img.size, T)
    return img.resize(new, Image.LANCZOS).crop((x0, y0, x0 + T, y0 + T))


def bytes_touched(w, h, T):
    """Input bytes the crop window's taps touch (RGB), from the library's own tables."""
    import ctypes as C
    from wmar_amd import _lib
    from wmar_amd.utils.ingest import plan
    (nw, nh), (x0, y0) = plan((w, h), T)
    span = []
    for a, b, o in ((w, nw, x0), (h, nh, y0)):
        if a == b:
            span.append(T)
            continue
        xmin, cnt, k = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T * 4096, np.int32)
        ks = C.c_int32(0)
        _lib.check(_lib.load().wmar_resample_coeffs(a, b, o, T, xmin.ctypes.data, cnt.ctypes.data, k.ctypes.data, k.size, C.byref(ks)))
        span.append(int(xmin[-1] + cnt[-1] - xmin[0]))
    return span[0] * span[1] * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    from wmar_amd.utils.ingest import ingest_packed, pack
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}; PIL {Image.__version__}; batch {args.batch}; runs {args.runs} (medians); ms per batch")
    say("size        target  pil_1t/img  pil_1t   pil_16t  pack_first  pack_warm  upload  ingest  pack+up+ing  e2e     "
        "e2e/pil_16t  MB_read/img  GB/s_ingest  HBM_frac")
    from wmar_amd.utils.ingest import ingest
    rng = np.random.default_rng(0)
    for (w, h) in ((4000, 3000), (1920, 1080), (1024, 1024)):
        arrs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(args.batch)]
        imgs = [Image.fromarray(a) for a in arrs]
        for T in (512, 256):
            t0 = time.perf_counter()
            host, desc = pack(arrs, T)
            pack_first = (time.perf_counter() - t0) * 1e3
            dev = host.cuda()
            ingest_packed(dev, desc, T)                       # warm-up: code objects, the library's scratch
            torch.cuda.synchronize()
            pk, up, ing, e2e = [], [], [], []
            for _ in range(args.runs):
                del host
                t0 = time.perf_counter()
                host, desc = pack(arrs, T)
                pk.append((time.perf_counter() - t0) * 1e3)
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                dev.copy_(host, non_blocking=True)
                e[1].record()
                out = ingest_packed(dev, desc, T)
                e[2].record()
                torch.cuda.synchronize()
                up.append(e[0].elapsed_time(e[1]))
                ing.append(e[1].elapsed_time(e[2]))
            del dev, host
            for _ in range(args.runs):
                t0 = time.perf_counter()
                out = ingest(arrs, T, "cuda")
                torch.cuda.synchronize()
                e2e.append((time.perf_counter() - t0) * 1e3)
            n1 = min(8, args.batch)
            t0 = time.perf_counter()
            ref = [pil_one(im, T) for im in imgs[:n1]]
            one = (time.perf_counter() - t0) * 1e3 / n1
            pool = []
            with ThreadPoolExecutor(max_workers=16) as ex:
                for _ in range(max(2, args.runs // 2)):
                    t0 = time.perf_counter()
                    list(ex.map(lambda im: pil_one(im, T), imgs))
                    pool.append((time.perf_counter() - t0) * 1e3)
            got = ((out[:n1].permute(0, 2, 3, 1).double() + 1) / 2 * 255).round().to(torch.uint8).cpu().numpy()
            assert all(np.array_equal(got[i], np.array(ref[i])) for i in range(n1)), "device result differs from PIL"
            med = statistics.median
            mk, mu, mi, me, mp = med(pk), med(up), med(ing), med(e2e), med(pool)
            rd = bytes_touched(w, h, T)
            bw = rd * args.batch / (mi * 1e-3)
            say(f"{w}x{h:<6} {T:<7} {one:<11.1f} {one * args.batch:<8.0f} {mp:<8.1f} {pack_first:<11.1f} {mk:<10.1f} {mu:<7.2f} {mi:<7.2f} "
                f"{mk + mu + mi:<12.1f} {me:<7.1f} {me / mp:<12.2f} {rd / 1e6:<12.2f} {bw / 1e9:<12.1f} {bw / HBM_BYTES_PER_S:.4f}")
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
