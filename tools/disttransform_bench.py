#!/usr/bin/env python
"""distanceTransform (opencv_amd.distanceTransform / distanceTransformBatch, csrc/disttransform.hip) on 3840 x 2160 CV_8UC1 masks resident in HBM: microseconds
per frame with HIP events on the launch stream, median of --repeats timed repeats after a warm-up.  Masks: `noise`, thresholded noise with a site density of
0.03, and `blobs`, a few large discs of non-zero pixels on a zero background (distances up to the disc radius); every frame of a batch has its own mask.  Rows:
DIST_L2 precise -> CV_32F, DIST_L1 -> CV_8U and DIST_C -> CV_32F in a batch on both masks, single calls of one frame rotating over the frames of the batch, and
the worst case of the outward row scan, one frame with a single site in a corner.  `bytes` is the algorithmic traffic -- every source byte read once, every
destination element written once -- and `vs_copy` that traffic per second over `copy_GBs`, mi355cv_copyProbe measured in the same process (bytes read + bytes
written per second); the scratch round trip of the column distances (2 bytes written and 2 read per pixel) counts against that fraction.  The time of each pass
comes from a traced run (rocprofv3 --kernel-trace --stats -- python tools/disttransform_bench.py --iters 3 --repeats 3), profiles/disttransform_kernel_stats.txt.
Prints one JSON object per row and appends them to --out (default profiles/disttransform_bench.jsonl)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opencv_amd as cv  # noqa: E402

W, H = 3840, 2160


def timeit(fn, iters, repeats, warm_ms=50.0):
    """median over `repeats` of the mean time of `iters` calls, us per call"""
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / iters)
    return statistics.median(out)


def noise(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand((n, H, W), device="cuda", generator=g) >= 0.03).to(torch.uint8) * 255).contiguous()


def blobs(n, seed):
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    out = torch.zeros((n, H, W), dtype=torch.uint8, device="cuda")
    for i in range(n):
        for _ in range(6):
            cy, cx, r = (float(torch.rand((), generator=g)) * H, float(torch.rand((), generator=g)) * W, 200.0 + 300.0 * float(torch.rand((), generator=g)))
            out[i] |= (((yy - cy) ** 2 + (xx - cx) ** 2) < r * r).to(torch.uint8) * 255
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16, help="frames per batch (a 4K frame is 8.3 MB in and 33 MB out as CV_32F)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disttransform_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = cv._lib.lib
    n = a.batch

    x = torch.empty((n, H, W, 4), dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    nb = x.numel()
    us = timeit(lambda: L.mi355cv_copyProbe(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nb), 1, 1), a.iters, a.repeats)
    copy_gbs = 2.0 * nb / us / 1e3
    del x, y
    torch.cuda.empty_cache()

    rows = []

    def row(name, us_frame, dst_esz, kernel):
        nbytes = H * W * (1 + dst_esz)
        gbs = nbytes / us_frame / 1e3
        rows.append({"row": name, "us_per_frame": round(us_frame, 2), "bytes": nbytes, "GBs": round(gbs, 1), "copy_GBs": round(copy_gbs, 1),
                     "vs_copy": round(gbs / copy_gbs, 3), "kernel": kernel})

    out32 = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    out8 = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    cases = (("L2 precise -> 32F", cv.DIST_L2, cv.DIST_MASK_PRECISE, cv.CV_32F, out32, 4), ("L1 -> 8U", cv.DIST_L1, cv.DIST_MASK_3, cv.CV_8U, out8, 1),
             ("C -> 32F", cv.DIST_C, cv.DIST_MASK_3, cv.CV_32F, out32, 4))
    for mname, make in (("noise 0.03", noise), ("blobs", blobs)):
        m = make(n, 1)
        for cname, dist, mask, dtype, dst, esz in cases:
            usb = timeit(lambda: cv.distanceTransformBatch(m, dist, mask, dstType=dtype, dst=dst), a.iters, a.repeats) / n
            row(f"distanceTransformBatch {cname} 4K x{n}, {mname}", usb, esz, L.mi355cv_lastKernel().decode())
        if mname == "noise 0.03":
            turn = [0]

            def one():
                i = turn[0] % n
                turn[0] += 1
                cv.distanceTransform(m[i], cv.DIST_L2, cv.DIST_MASK_PRECISE, dst=out32[i])
            us1 = timeit(one, a.iters * n, a.repeats)
            row(f"distanceTransform L2 precise -> 32F 4K single calls rotating over {n} frames in HBM, {mname}", us1, 4, L.mi355cv_lastKernel().decode())
        del m
    worst = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
    worst[0, 0] = 0
    usw = timeit(lambda: cv.distanceTransform(worst, cv.DIST_L2, cv.DIST_MASK_PRECISE, dst=out32[0]), a.iters, a.repeats)
    row("distanceTransform L2 precise -> 32F 4K single call, one site in a corner (worst case of the row scan)", usw, 4, L.mi355cv_lastKernel().decode())
    rows.append({"row": "yardsticks", "copyProbe_GBs": round(copy_gbs, 1), "batch": n, "iters": a.iters, "repeats": a.repeats})
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
