#!/usr/bin/env python
"""calcOpticalFlowFarneback (opencv_amd.calcOpticalFlowFarneback, csrc/farneback.hip) on 1920 x 1080 and 3840 x 2160 frames resident in HBM, flows left on the device.
Frames are windows of one smooth random texture that move by (2, -1) a frame.  Parameters (0.5, 3, 15, 3, 5, 1.2, 0) and the same with OPTFLOW_FARNEBACK_GAUSSIAN.
Microseconds from HIP events on the launch stream around a window of calls (asynchronous mode: the calls return after the enqueue), the median of --groups windows
with their minimum and maximum, next to the rate of mi355cv_copyProbe measured in the same process:
  call                the single call, per flow
  batch of 8          calcOpticalFlowFarnebackBatch on 8 frames, per flow (7 flows)
  k_fb_polyexp / k_fb_update_matrices / k_fb_update_flow   the stage entries at full resolution, one kernel each
alg_bytes: what the algorithm has to move.  Per pixel of a level: smoothing 1 + 4 (+ 4 + 4 per level pixel for the resize above level 0), expansion 4 + 20, update
matrices 20 + 20 + 8 + 20, update flow 20 + 8, the flow upscale 8 + 8; a call expands two frames, a batch one per flow.
There is no speed gate: the parent has no such path.  Prints one JSON object per row and appends them to --out (default profiles/farneback_bench.jsonl)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import opencv_amd as cv  # noqa: E402


def window_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def timeit(fn, groups, warm_ms=30.0):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        torch.cuda.synchronize()
    return [window_us(fn) for _ in range(groups)]


def sequence(n, h, w, g):
    pad = 2 * n + 16
    big = torch.rand((1, 1, h + 2 * pad, w + 2 * pad), device="cuda", generator=g)
    for _ in range(3):
        big = torch.nn.functional.avg_pool2d(big, 5, stride=1, padding=2)
    big = big[0, 0]
    big = ((big - big.min()) / (big.max() - big.min()) * 255).round().to(torch.uint8)
    return torch.stack([big[pad + i:pad + i + h, pad - 2 * i:pad - 2 * i + w] for i in range(n)]).contiguous()


def level_sizes(w, h, pyr, levels):
    out = []
    for k in range(levels):
        s = pyr ** k
        if k and (w * s < 32 or h * s < 32):
            break
        out.append((round(w * s), round(h * s)))
    return out


def alg_bytes(w, h, pyr, levels, iterations, frames_per_flow):
    sizes = level_sizes(w, h, pyr, levels)
    total = 0
    for k, (lw, lh) in enumerate(sizes):
        lp = lw * lh
        expand = w * h * 5 + (0 if k == 0 else w * h * 4 + lp * 4) + lp * 24
        upscale = lp * 8 + (sizes[k + 1][0] * sizes[k + 1][1] * 8 if k + 1 < len(sizes) else 0)      # the level flow written (zeros at the coarsest), the coarser one read
        total += frames_per_flow * expand + upscale + lp * 68 + iterations * lp * 28 + max(iterations - 1, 0) * lp * 68
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "farneback_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = cv._lib.lib

    x = torch.empty((16, 2160, 3840, 4), dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    nb = x.numel()
    us = statistics.median(timeit(lambda: L.mi355cv_copyProbe(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nb), 1, 1), a.groups))
    copy_gbs = 2.0 * nb / us / 1e3
    del x, y
    torch.cuda.empty_cache()

    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []

    def row(name, t, nbytes, **extra):
        med = statistics.median(t)
        gbs = nbytes / med / 1e3
        r = {"row": name, "us": round(med, 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1), "alg_bytes": int(nbytes), "GBs": round(gbs, 1),
             "frac_of_8TBs": round(gbs / 8000.0, 3), "copy_GBs": round(copy_gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 3), "kernel": L.mi355cv_lastKernel().decode()}
        r.update(extra)
        rows.append(r)
        print(json.dumps(r), flush=True)

    pyr, levels, winsize, iterations, poly_n, poly_sigma = 0.5, 3, 15, 3, 5, 1.2
    cv.set_async(True)
    try:
        for (w, h, tag) in ((1920, 1080, "1080p"), (3840, 2160, "4K")):
            frames = sequence(8, h, w, g)
            flow = torch.empty((h, w, 2), dtype=torch.float32, device="cuda")
            flows = torch.empty((7, h, w, 2), dtype=torch.float32, device="cuda")
            for flags, win in ((0, "box"), (256, "gauss")):
                args = (pyr, levels, winsize, iterations, poly_n, poly_sigma, flags)
                t1 = timeit(lambda: [cv.calcOpticalFlowFarneback(frames[i], frames[i + 1], flow, *args) for i in range(4)], a.groups)
                row("call %s %s" % (tag, win), [v / 4 for v in t1], alg_bytes(w, h, pyr, levels, iterations, 2))
                t8 = timeit(lambda: cv.calcOpticalFlowFarnebackBatch(frames, flows, *args), a.groups)
                row("batch of 8 %s %s, per flow" % (tag, win), [v / 7 for v in t8], alg_bytes(w, h, pyr, levels, iterations, 1),
                    speedup_over_call=round(statistics.median(t1) / 4 / (statistics.median(t8) / 7), 2))
            # the stages at full resolution
            img = frames[0].to(torch.float32)
            R0 = cv.farnebackPolyExp(img, poly_n, poly_sigma)
            R1 = cv.farnebackPolyExp(frames[1].to(torch.float32), poly_n, poly_sigma)
            cv.calcOpticalFlowFarneback(frames[0], frames[1], flow, *args)
            M = cv.farnebackUpdateMatrices(R0, R1, flow)
            M2 = torch.empty_like(M)
            px = w * h
            row("k_fb_polyexp %s n=5" % tag, [v / 4 for v in timeit(lambda: [cv.farnebackPolyExp(img, poly_n, poly_sigma, dst=R0) for _ in range(4)], a.groups)], px * 24)
            row("k_fb_update_matrices %s" % tag, [v / 4 for v in timeit(lambda: [cv.farnebackUpdateMatrices(R0, R1, flow, M=M2) for _ in range(4)], a.groups)], px * 68)
            f2 = torch.empty_like(flow)
            for flags, win in ((0, "box"), (256, "gauss")):
                row("k_fb_update_flow %s winsize 15 %s" % (tag, win), [v / 4 for v in timeit(lambda: [cv.farnebackUpdateFlow(M, winsize, flags, flow=f2) for _ in range(4)], a.groups)],
                    px * 28)
            row("k_fb_update_flow %s winsize 5 box" % tag, [v / 4 for v in timeit(lambda: [cv.farnebackUpdateFlow(M, 5, 0, flow=f2) for _ in range(4)], a.groups)], px * 28)
            torch.cuda.synchronize()
            del frames, flow, flows, img, R0, R1, M, M2, f2
            torch.cuda.empty_cache()
    finally:
        cv.set_async(False)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
