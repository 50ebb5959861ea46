#!/usr/bin/env python
"""calcHist / calcBackProject (opencv_amd.calcHistBatch / calcBackProjectBatch, csrc/calchist.hip) on a batch of 3840 x 2160 frames resident in HBM, results left on the
device (no read-back).  Microseconds per frame, HIP events on the launch stream around a whole batch call, the median of --groups timed calls after at least 30 ms
of warm-up.  Three numbers from the SAME run:
  frac_of_8TBs     bytes the call has to read (source, plus the mask when there is one; back-projection: plus the bytes it writes) per second, over 8 TB/s;
  frac_of_copy     the same bytes per second over the rate of mi355cv_copyProbe measured in this process.  The copy's rate counts the bytes it reads AND the bytes it
                   writes; a histogram only reads, so at equal memory traffic per second the ratio is 1 although it takes half a copy's time per source byte;
  torch_us         torch.bincount over the same CV_8UC1 frames, one frame at a time (it has no batched form), on int32 copies made BEFORE the timed region (bincount
                   takes no uint8), as an independent comparator and a check.
The CV_8UC1 256-bin row is repeated for four contents -- random, constant, a smooth horizontal ramp, a two-value checkerboard -- because the LDS atomics of
k_calchist_lds cost what the content makes them collide.
There is no speed gate: the parent has no such path.  Prints one JSON object per row and appends them to --out (default profiles/calchist_bench.jsonl)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--groups", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calchist_bench.jsonl"))
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

    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []

    def row(name, fn, nbytes, **extra):
        fn()
        kernel = L.mi355cv_lastKernel().decode()
        usf = timeit(fn, a.groups) / n
        gbs = nbytes / usf / 1e3
        r = {"row": name, "us_per_frame": round(usf, 2), "bytes_per_frame": nbytes, "GBs": round(gbs, 1), "frac_of_8TBs": round(gbs / 8000.0, 3),
             "copy_GBs": round(copy_gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 3), "kernel": kernel}
        r.update(extra)
        rows.append(r)
        print(json.dumps(r), flush=True)

    rand = torch.randint(0, 256, (n, H, W), device="cuda", generator=g, dtype=torch.uint8)
    const = torch.full((n, H, W), 200, device="cuda", dtype=torch.uint8)
    ramp = (torch.arange(W, device="cuda") * 256 // W).to(torch.uint8).expand(n, H, W).contiguous()
    mask = (torch.rand((n, H, W), device="cuda", generator=g) < 0.5).to(torch.uint8)
    one = [0], [256], [0, 256]
    yy, xx = torch.arange(H, device="cuda")[:, None], torch.arange(W, device="cuda")[None, :]
    checker = torch.where((yy + xx) % 2 == 0, 10, 240).to(torch.uint8).expand(n, H, W).contiguous()
    # the comparator doubles as a check of this run's results; its uint8 -> int32 conversion is not timed
    got = cv.calcHistBatch(rand, [0], None, [256], [0, 256], dtype=np.int32, device=True)
    as_int = [rand[f].reshape(-1).int() for f in range(n)]
    assert all(torch.equal(got[f].long(), torch.bincount(as_int[f], minlength=256)) for f in range(n))
    t_us = timeit(lambda: [torch.bincount(v, minlength=256) for v in as_int], a.groups) / n
    del as_int
    torch.cuda.empty_cache()
    for content, frames in (("random", rand), ("constant", const), ("horizontal ramp", ramp), ("two-value checkerboard", checker)):
        extra = {"torch_bincount_int32_us_per_frame": round(t_us, 2)} if content == "random" else {}
        row("calcHistBatch 4K x%d CV_8UC1 256 bins, %s content" % (n, content),
            lambda: cv.calcHistBatch(frames, one[0], None, one[1], one[2], dtype=np.int32, device=True), H * W, **extra)
    row("calcHistBatch 4K x%d CV_8UC1 256 bins, random content, masked (one CV_8UC1 mask per frame)" % n,
        lambda: cv.calcHistBatch(rand, one[0], mask, one[1], one[2], dtype=np.int32, device=True), 2 * H * W)
    del const, ramp, checker, mask
    torch.cuda.empty_cache()
    rgb = torch.randint(0, 256, (n, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
    for channels, hs, rg in (([0, 1], [30, 32], [0, 180, 0, 256]), ([0, 1, 2], [32, 32, 32], [0, 256] * 3), ([0, 1], [180, 256], [0, 180, 0, 256])):
        row("calcHistBatch 4K x%d CV_8UC3 channels %s at %s, random content" % (n, channels, " x ".join(map(str, hs))),
            lambda: cv.calcHistBatch(rgb, channels, None, hs, rg, dtype=np.float32, device=True), 3 * H * W)
    hist = cv.calcHistBatch(rgb[:1], [0, 1], None, [30, 32], [0, 180, 0, 256], device=True)[0]
    dst = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    row("calcBackProjectBatch 4K x%d CV_8UC3 through 30 x 32, one shared histogram (bytes: read + written)" % n,
        lambda: cv.calcBackProjectBatch(rgb, [0, 1], hist, [0, 180, 0, 256], 255.0 / float(hist.max()), dst=dst), 4 * H * W)
    del rgb, dst
    torch.cuda.empty_cache()
    f32 = torch.rand((n, H, W), device="cuda", generator=g)
    row("calcHistBatch 4K x%d CV_32FC1 256 bins over (0, 1), random content" % n, lambda: cv.calcHistBatch(f32, [0], None, [256], [0, 1], dtype=np.float32, device=True), 4 * H * W)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
