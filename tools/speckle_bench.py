#!/usr/bin/env python
"""cv::filterSpeckles (opencv_amd.filterSpeckles, csrc/speckle.hip) on maps resident in HBM, filtered in place.
Microseconds per frame from HIP events on the launch stream around a window of calls, the median of --groups windows with their minimum and maximum; every shape is
warmed first.  The call works in place, so every timed call first restores its input from a pristine copy (one device-to-device copy of the map); that copy alone is
timed in windows of its own in the same rounds and reported next to the totals (`copy_us_per_frame`), and `net` = total - copy.  The tile path and the forced plain
kernels (mi355cv_filterSpecklesSetKernel -1 / 0) run in alternating rounds of one process and their images are compared at every timed size.
  rows      1080p and 4K CV_16S x a single map and a batch of 8 x four inputs: the map cv.StereoBM makes of a textured pair (the workload that matters), a constant
            map (one component), a checkerboard of singletons, a serpentine one pixel wide; one CV_8U 4K row
  figures   us per frame; `plain_over_fast` on the totals and on the net times; `copy_rate_share` = copy / net: the copy reads and writes the map once, which is the
            algorithmic traffic of the filter, so this is the fraction of the measured copy rate the filter reaches; `fast_wins`: the two ranges of windows do not overlap
The plain kernels walk long parent chains on large components and can take a second per 4K frame: a call that takes more than 100 ms is timed in two windows of one
call, and after --budget seconds the remaining plain arms are skipped and the rows say so.  Prints one JSON object per row and appends them to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opencv_amd as cv  # noqa: E402
from opencv_amd import _lib  # noqa: E402


def window_us(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / inner


def warm(fn, warm_ms, window_ms):
    """runs fn twice at least (once if a call takes more than 100 ms) and for warm_ms; the calls per timed window that fill window_ms, and one call's milliseconds"""
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        ms = (time.perf_counter() - t0) * 1e3
        if ms / n > 100.0 or (n >= 2 and ms >= warm_ms):
            break
    one = ms / n
    return int(min(200, max(1, window_ms / one))), one


def stats(us):
    return dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2)) if us else None


def stereo_maps(n, h, w, g):
    """the CV_16S maps StereoBM (64 disparities, blocks of 15) makes of smooth random frames and their copies shifted by 24 columns, with a band of a second disparity"""
    big = torch.rand((n, 1, h + 4, w + 40 + 4), device="cuda", generator=g)
    big = F.avg_pool2d(big, 5, stride=1) * 255
    left = big[:, 0, :, :w].to(torch.uint8).contiguous()
    right = big[:, 0, :, 24:24 + w].to(torch.uint8).contiguous()
    right[:, h // 3:h // 2] = big[:, 0, h // 3:h // 2, 37:37 + w].to(torch.uint8)
    return cv.StereoBM_create(64, 15).computeBatch(left, right)


def serpentine(n, h, w, dtype):
    img = torch.full((n, h, w), -16 if dtype == torch.int16 else 0, dtype=dtype, device="cuda")
    img[:, 0::2] = 320 if dtype == torch.int16 else 200
    ys = torch.arange(1, h - 1, 2, device="cuda")
    xs = torch.where((torch.arange(len(ys), device="cuda") % 2) == 0, w - 1, 0)
    img[:, ys, xs] = 320 if dtype == torch.int16 else 200
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--budget", type=float, default=420.0, help="seconds after which the remaining plain arms are skipped")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speckle_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    prop = torch.cuda.get_device_properties(0)
    dev = dict(device=prop.name, cus=prop.multi_processor_count)
    g = torch.Generator(device="cuda").manual_seed(1)
    t_start = time.perf_counter()
    setk = _lib.lib.mi355cv_filterSpecklesSetKernel
    sizes = (("1080p", 1080, 1920), ("4K", 2160, 3840)) if not a.small else (("small", 70, 600),)
    rows = [(name, h, w, nb, torch.int16, inp) for name, h, w in sizes for nb in (1, 8) for inp in ("stereobm", "constant", "checkerboard", "serpentine")]
    rows.append((sizes[-1][0], sizes[-1][1], sizes[-1][2], 1, torch.uint8, "stereobm>>4"))
    for name, h, w, nb, dtype, inp in rows:
        # (pristine maps, newVal, maxSpeckleSize, maxDiff)
        if inp == "stereobm":
            pristine, args = stereo_maps(nb, h, w, g), (-16, 200, 32)
        elif inp == "stereobm>>4":
            m = stereo_maps(nb, h, w, g)
            pristine, args = torch.where(m < 0, 0, (m >> 4) + 1).to(torch.uint8), (0, 200, 2)
        elif inp == "constant":
            pristine, args = torch.full((nb, h, w), 320, dtype=dtype, device="cuda"), (-16, 200, 16)
        elif inp == "checkerboard":
            yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
            pristine, args = (((yy + xx) & 1) * 100 + 100).to(dtype).expand(nb, h, w).contiguous(), (-16, 1, 0)
        else:
            pristine, args = serpentine(nb, h, w, dtype), (-16, 200, 0)
        work = torch.empty_like(pristine)
        restore = lambda: work.copy_(pristine)
        if nb == 1:
            fn = lambda: (restore(), cv.filterSpeckles(work[0], *args))
        else:
            fn = lambda: (restore(), cv.filterSpecklesBatch(work, *args))
        skip_plain = time.perf_counter() - t_start > a.budget
        inner, one_ms, outs, kernels, res = {}, {}, {}, {}, {-1: [], 0: [], "copy": []}
        for mode in ((-1,) if skip_plain else (-1, 0)):
            setk(mode)
            inner[mode], one_ms[mode] = warm(fn, 30.0 if mode < 0 else 0.0, 20.0)
            outs[mode] = work.clone()
            kernels[mode] = _lib.lib.mi355cv_lastKernel().decode()
        inner["copy"], _ = warm(restore, 5.0, 20.0)
        plain_windows = 0 if skip_plain else 2 if one_ms[0] > 100.0 else 3
        for rnd in range(a.groups):
            order = [-1, "copy", 0] if rnd % 2 == 0 else [0, "copy", -1]
            for mode in order:
                if mode == 0 and rnd >= plain_windows:
                    continue
                if mode != "copy":
                    setk(mode)
                res[mode].append(window_us(restore if mode == "copy" else fn, inner[mode]) / nb)
        setk(-1)
        fast, copy = statistics.median(res[-1]), statistics.median(res["copy"])
        plain = statistics.median(res[0]) if res[0] else None
        erased = int((outs[-1] != pristine).sum().item())
        row = dict(case=name, frames=nb, depth="16S" if dtype == torch.int16 else "8U", input=inp, newVal=args[0], maxSpeckleSize=args[1], maxDiff=args[2],
                   erased_pixels_per_frame=erased // nb, us_per_frame=stats(res[-1]), plain_us_per_frame=stats(res[0]), copy_us_per_frame=stats(res["copy"]),
                   net_us_per_frame=round(fast - copy, 2), plain_net_us_per_frame=round(plain - copy, 2) if plain else None,
                   plain_over_fast=round(plain / fast, 2) if plain else None, plain_over_fast_net=round((plain - copy) / (fast - copy), 2) if plain else None,
                   copy_rate_share=round(copy / (fast - copy), 4), fast_wins=bool(max(res[-1]) < min(res[0])) if res[0] else None,
                   images_equal=bool(torch.equal(outs[-1], outs[0])) if 0 in outs else None, plain_skipped="budget" if skip_plain else None,
                   calls_per_window=inner[-1], plain_calls_per_window=inner.get(0), plain_windows=len(res[0]), interleaved=True,
                   algorithmic_bytes_per_frame=2 * h * w * pristine.element_size(), kernel=kernels[-1], plain_kernel=kernels.get(0), **dev)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
