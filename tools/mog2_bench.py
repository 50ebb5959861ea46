#!/usr/bin/env python
"""BackgroundSubtractorMOG2 (opencv_amd.createBackgroundSubtractorMOG2, csrc/mog2.hip) on 3840 x 2160 frames resident in HBM, masks left on the device.
The sequence is synthetic: a static background of a few grey levels, +-2 of noise per frame and a 400 x 400 block that moves 16 pixels a frame, so that the mode
counts are what a fixed camera gives (1 - 3).  The model first sees --settle frames; then, per type, microseconds per frame from HIP events on the launch stream
around 16 frames' worth of calls (asynchronous mode: the calls return after the enqueue), the median of --groups such windows with their minimum and maximum:
  apply               16 single apply calls
  applyBatch T=4/16/64  4 / 1 / 1 calls (T = 64: 64 frames in the window)
  getBackgroundImage  one call
The apply and applyBatch T=16 windows ALTERNATE in one loop, so the two are compared within the same run and the same drift.  Three figures per row:
  alg_bytes_per_frame  what the algorithm has to move: cn * sizeof(T) + 1 bytes per pixel for frame and mask, plus the model each way divided by T, the model's
                       size taken from the ACTUAL modesUsed after the run (a pixel's planes below its count, and its count byte);
  frac_of_8TBs         those bytes per second over 8 TB/s;
  frac_of_copy         the same over the rate of mi355cv_copyProbe measured in this process (bytes read plus bytes written).
There is no speed gate: the parent has no such path.  Prints one JSON object per row and appends them to --out (default profiles/mog2_bench.jsonl)."""
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
WINDOW = 16


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


def sequence(n, cn, g):
    """n frames [n, H, W(, cn)] uint8 on the device"""
    shape = (H, W) if cn == 1 else (H, W, cn)
    levels = torch.tensor([30, 70, 110, 150, 200], device="cuda", dtype=torch.int16)
    base = levels[torch.randint(0, 5, shape, device="cuda", generator=g)]
    out = torch.empty((n,) + shape, dtype=torch.uint8, device="cuda")
    for t in range(n):
        f = base + torch.randint(-2, 3, shape, device="cuda", generator=g, dtype=torch.int16)
        x0, y0 = (100 + 16 * t) % (W - 400), (200 + 9 * t) % (H - 400)
        f[y0:y0 + 400, x0:x0 + 400] = 240 - (t % 3) * 5
        out[t] = f.clamp_(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=9)
    ap.add_argument("--settle", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mog2_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = cv._lib.lib

    x = torch.empty((16, H, W, 4), dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    nb = x.numel()
    us = statistics.median(timeit(lambda: L.mi355cv_copyProbe(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nb), 1, 1), a.groups))
    copy_gbs = 2.0 * nb / us / 1e3
    del x, y
    torch.cuda.empty_cache()

    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    cv.set_async(True)
    try:
        for cn in (1, 3):
            frames = sequence(64, cn, g)
            masks = torch.empty((64, H, W), dtype=torch.uint8, device="cuda")
            m = cv.createBackgroundSubtractorMOG2()
            for t in range(a.settle):
                m.apply(frames[t % 64], masks[0])
            torch.cuda.synchronize()
            pos = [0]

            def singles():
                for i in range(WINDOW):
                    m.apply(frames[(pos[0] + i) % 64], masks[i])
                pos[0] = (pos[0] + WINDOW) % 64

            def batch(T, n):
                def run():
                    for _ in range(n):
                        if pos[0] + T > 64:
                            pos[0] = 0
                        m.applyBatch(frames[pos[0]:pos[0] + T], masks[:T])
                        pos[0] = (pos[0] + T) % 64
                return run

            singles(); batch(16, 1)(); torch.cuda.synchronize()                # code objects loaded, both shapes warm
            t_single, t_b16 = [], []
            for _ in range(a.groups):                                           # alternating windows of the same 16 frames' worth
                t_single.append(window_us(singles) / WINDOW)
                t_b16.append(window_us(batch(16, 1)) / 16)
            t_b4 = [v / 16 for v in timeit(batch(4, 4), a.groups)]
            t_b64 = [v / 64 for v in timeit(batch(64, 1), a.groups)]
            bg = m.getBackgroundImage()
            t_bg = timeit(lambda: m.getBackgroundImage(dst=bg), a.groups)
            torch.cuda.synchronize()
            modes = m.getModel()[0]
            mean_modes = float(modes.float().mean())
            hist = torch.bincount(modes.reshape(-1).int(), minlength=6).tolist()
            model_bytes = (mean_modes * (2 + cn) * 4 + 1) * H * W               # one way
            io = (cn + 1) * H * W

            def row(name, t, nbytes, kernel, **extra):
                med = statistics.median(t)
                gbs = nbytes / med / 1e3
                r = {"row": "%s 4K CV_8UC%d" % (name, cn), "us_per_frame": round(med, 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
                     "alg_bytes_per_frame": int(nbytes), "GBs": round(gbs, 1), "frac_of_8TBs": round(gbs / 8000.0, 3), "copy_GBs": round(copy_gbs, 1),
                     "frac_of_copy": round(gbs / copy_gbs, 3), "mean_modesUsed": round(mean_modes, 3), "modesUsed_histogram": hist, "kernel": kernel}
                r.update(extra)
                rows.append(r)
                print(json.dumps(r), flush=True)

            singles()
            k1 = L.mi355cv_lastKernel().decode()
            row("apply, 16 single calls", t_single, io + 2 * model_bytes, k1, alternated_with="applyBatch T=16")
            for T, t in ((4, t_b4), (16, t_b16), (64, t_b64)):
                batch(T, 1)()
                row("applyBatch T=%d" % T, t, io + 2 * model_bytes / T, L.mi355cv_lastKernel().decode(),
                    **({"alternated_with": "apply", "speedup_over_apply": round(statistics.median(t_single) / statistics.median(t), 2)} if T == 16 else {}))
            m.getBackgroundImage(dst=bg)
            row("getBackgroundImage", t_bg, cn * H * W + model_bytes, L.mi355cv_lastKernel().decode())
            torch.cuda.synchronize()
            del m, frames, masks, bg, modes
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
