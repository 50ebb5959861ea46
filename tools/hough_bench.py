#!/usr/bin/env python
"""HoughLines (opencv_amd.HoughLinesBatch, csrc/hough.hip) on 3840 x 2160 CV_8UC1 edge maps resident in HBM: synthetic line scenes (bright lines at many slopes
and a few rectangles on a noisy ground) passed through opencv_amd.Canny, then the standard transform with rho = 1, theta = pi / 180.  Microseconds per frame,
HIP events on the launch stream around a whole batch call (its one host synchronisation included), the median of --groups timed calls after at least 30 ms of
warm-up.  Reported: the edge density, the per-frame time of the whole call, the per-frame time of compaction + vote alone (mi355cv_houghLinesAccum on one frame,
its device-to-device copy of the accumulator included), and mi355cv_copyProbe's rate from the same process.  There is no speed gate: the parent has no such path.

The per-kernel split needs a traced run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/hough_bench.py --batch 4 --groups 1 --out ''
and a second, untraced pass that reads the trace's kernel statistics (--kernel-stats DIR/.../*_kernel_stats.csv): it adds every k_hough_* kernel's and the sort's
share of the kernel time, and the compaction kernel's rate (source bytes read per second of k_hough_points) beside the copy rate.
Prints one JSON object per row and appends them to --out (default profiles/hough_bench.jsonl)."""
import argparse
import csv
import ctypes
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opencv_amd as cv  # noqa: E402

W, H = 3840, 2160


def timeit(fn, groups, warm_ms=30.0):
    """median over `groups` timed calls, us per call"""
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(groups):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return statistics.median(out)


def scene(seed):
    """one 4K frame: 24 lines at slopes between -2 and 2, four rectangles, uniform noise of +-6 grey levels"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.full((H, W), 40.0, device="cuda")
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    for i in range(24):
        ang = math.pi * (i + 0.37 * seed) / 24
        off = 200.0 + 140.0 * i
        d = (xx * math.cos(ang) + yy * math.sin(ang) - off).abs()
        img = torch.where(d < 2.0, torch.full_like(img, 220.0), img)
    for i in range(4):
        x0, y0 = 300 + 800 * i, 250 + 350 * i
        img[y0:y0 + 400, x0:x0 + 600] = 150.0
    img = img + torch.randint(-6, 7, (H, W), device="cuda", generator=g).float()
    return img.clamp(0, 255).to(torch.uint8)


def kernel_shares(path):
    """rocprofv3's kernel statistics -> {kernel name: total ns} for the kernels of a HoughLines call"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            calls = int(float(row.get("Calls") or 0))
            for key in ("k_hough_points", "k_hough_vote", "k_hough_maxima", "k_hough_emit", "rocprim", "radix", "onesweep"):
                if key in name:
                    k = key if key.startswith("k_hough") else "sort (rocPRIM)"
                    a = out.setdefault(k, [0.0, 0])
                    a[0] += ns
                    a[1] += calls
                    break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--threshold", type=int, default=300)
    ap.add_argument("--kernel-stats", default="", help="kernel statistics (csv) of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hough_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = cv._lib.lib
    n = a.batch

    x = torch.empty((16, H, W, 4), dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    nb = x.numel()
    us = timeit(lambda: L.mi355cv_copyProbe(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nb), 1, 1), a.groups)
    copy_gbs = 2.0 * nb / us / 1e3
    del x, y
    torch.cuda.empty_cache()

    edges = torch.stack([cv.Canny(scene(i), 60, 160) for i in range(n)])
    density = float((edges != 0).float().mean())
    theta = math.pi / 180
    counts, _ = cv.HoughLinesBatch(edges, 1, theta, a.threshold)
    kernel = L.mi355cv_lastKernel().decode()
    usf = timeit(lambda: cv.HoughLinesBatch(edges, 1, theta, a.threshold), a.groups) / n
    us_acc = timeit(lambda: cv.HoughLinesAccumulator(edges[0], 1, theta), a.groups)
    row = {"row": "HoughLinesBatch 4K x%d CV_8UC1, Canny edges of synthetic line scenes, rho 1, theta pi/180, threshold %d" % (n, a.threshold),
           "edge_density": round(density, 5), "edge_pixels_per_frame": int(density * H * W), "lines_per_frame": [min(counts), max(counts)],
           "us_per_frame": round(usf, 2), "us_points_and_vote_one_frame": round(us_acc, 2), "copy_GBs": round(copy_gbs, 1), "kernel": kernel,
           "host_baseline": "not measured: no reference build with HoughLines on this machine"}
    if a.kernel_stats:
        ks = kernel_shares(a.kernel_stats)
        total = sum(v[0] for v in ks.values()) or 1.0
        row["kernel_shares"] = {k: round(v[0] / total, 4) for k, v in sorted(ks.items())}
        if "k_hough_points" in ks and ks["k_hough_points"][1]:
            ns_call = ks["k_hough_points"][0] / ks["k_hough_points"][1]                 # one launch covers a whole batch of the traced run
            row["k_hough_points_ns_per_launch"] = round(ns_call, 1)
            row["note"] = "compaction rate = traced batch x %d bytes / k_hough_points_ns_per_launch, to be read beside copy_GBs" % (H * W)
    else:
        row["kernel_shares"] = "not measured in this run (see --kernel-stats)"
    print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
