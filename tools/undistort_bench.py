#!/usr/bin/env python
"""The rectifying warp and cv::reprojectImageTo3D (opencv_amd.calib3d, csrc/undistort.hip) on frames resident in HBM, the result left on the device.
Microseconds per frame from HIP events on the launch stream around a window of calls of at least 20 ms, the median of --groups windows with their minimum and maximum;
every shape is warmed first and the arms of a row are timed in the same process in alternating rounds.
  rows      1080p and 4K x CV_8UC1, CV_8UC3 x a single frame and batches of 8 and 64 frames of one camera (4K CV_8UC3 x 64: 32, to stay inside a few GiB), CV_8UC4
            single and x 8; the lens
            k1 = -0.28, k2 = 0.09, p1 = 0.0012, p2 = -0.0007, k3 = -0.015 and a 0.02 rad rectifying rotation; INTER_LINEAR, BORDER_CONSTANT
  arms      `fused_us`     k_undist8_tile (mi355cv_undistortSetKernel 1): the rule evaluated per destination tile, no maps
            `composed_us`  what a user runs without it: the CV_16SC2 + CV_16UC1 maps built ONCE outside the timing (initUndistortRectifyMap), cv.remap per frame
            `grid_sample_us`  torch.nn.functional.grid_sample (bilinear, zeros) on a float copy, as the outside comparison only: float arithmetic, not expected to agree
            `library_composed_us`  single frames: mi355cv_undistortSetKernel 0, the maps built inside the call, then remap
            fused and composed must agree bit for bit before a time is written (`results_equal`)
  figures   `copy_us`: reading and writing the frame (2 bytes per pixel and channel) at the device-to-device copy rate of this run; `copy_share` = that / fused
  fpw A/B   batch of 64, 4K CV_8UC1: frames per workgroup 1 against the default (mi355cv_undistortSetFramesPerGroup)
  reproject 4K from CV_16S and CV_32F, with and without handleMissingValues, against the copy rate for its bytes (the disparity + 12 bytes per pixel)
No speed gate against the parent, which has no such path.  Prints one JSON object per row and appends them to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opencv_amd as cv  # noqa: E402
from opencv_amd import _lib  # noqa: E402

LENS = [-0.28, 0.09, 0.0012, -0.0007, -0.015]
CV_16SC2, CV_32FC1 = 11, 5


def window_us(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / inner


def warm(fn, warm_ms, window_ms):
    """runs fn twice at least and for warm_ms; the calls per timed window that fill window_ms"""
    t0 = time.perf_counter()
    n = 0
    while n < 2 or (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        torch.cuda.synchronize()
        n += 1
    one = (time.perf_counter() - t0) * 1e3 / n
    return int(min(200, max(1, -(-window_ms // one))))


def stats(us):
    return dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2)) if us else None


def copy_rate():
    """GB/s of a device-to-device copy of 1 GiB, read + write counted"""
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    fn = lambda: b.copy_(a)                                                              # noqa: E731
    inner = warm(fn, 20.0, 20.0)
    us = statistics.median(window_us(fn, inner) for _ in range(5))
    return 2 * (1 << 30) / (us * 1e-6) / 1e9


def camera(w, h):
    f = 0.8 * w
    K = np.array([[f, 0, w / 2 - 0.3], [0, f * 0.9975, h / 2 + 0.4], [0, 0, 1]], np.float64)
    a = 0.02
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)
    return K, R


def alternate(arms, groups):
    """arms: {name: (set, fn, inner, per)} -> {name: [us per frame]}"""
    res = {k: [] for k in arms}
    order = list(arms)
    for rnd in range(groups):
        for k in (order if rnd % 2 == 0 else order[::-1]):
            setup, fn, inner, per = arms[k]
            setup()
            res[k].append(window_us(fn, inner) / per)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    L = _lib.lib
    prop = torch.cuda.get_device_properties(0)
    dev = dict(device=prop.name, cus=prop.multi_processor_count)
    g = torch.Generator(device="cuda").manual_seed(1)
    gbs = copy_rate()
    sizes = (("1080p", 1080, 1920), ("4K", 2160, 3840)) if not a.small else (("small", 70, 250),)
    batches = (1, 8, 64) if not a.small else (1, 3)

    def emit(row):
        row.update(copy_gbs=round(gbs, 1), **dev)
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    def setk(mode, fpw=0):
        def go():
            L.mi355cv_undistortSetKernel(mode)
            L.mi355cv_undistortSetFramesPerGroup(fpw)
        return go

    for name, h, w in sizes:
        K, R = camera(w, h)
        m1, m2 = cv.initUndistortRectifyMap(K, LENS, R, None, (w, h), CV_16SC2, device="cuda")
        mx, my = cv.initUndistortRectifyMap(K, LENS, R, None, (w, h), CV_32FC1, device="cuda")
        grid = torch.stack([(mx + 0.5) * (2.0 / w) - 1, (my + 0.5) * (2.0 / h) - 1], dim=-1)[None]
        for cn in (1, 3, 4):
            for nb in (batches if cn != 4 else batches[:2]):
                if name == "4K" and cn == 3 and nb == 64:
                    nb = 32
                shape = (nb, h, w) + ((cn,) if cn > 1 else ())
                src = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
                dst, ref = torch.empty_like(src), torch.empty_like(src)
                if nb == 1:
                    fused = lambda: cv.undistortRectify(src[0], K, LENS, R, None, (w, h), dst=dst[0])                      # noqa: E731
                else:
                    fused = lambda: cv.undistortRectifyBatch(src, K, LENS, R, None, (w, h), dst=dst)                      # noqa: E731

                def composed():
                    for f in range(nb):
                        cv.remap(src[f], m1, m2, cv.INTER_LINEAR, cv.BORDER_CONSTANT, 0, dst=ref[f])
                setk(1)()
                fused()
                kernel = L.mi355cv_lastKernel().decode()
                composed()
                ckernel = L.mi355cv_lastKernel().decode()
                torch.cuda.synchronize()
                equal = bool(torch.equal(dst, ref))
                if not equal:
                    emit(dict(case=name, frames=nb, cn=cn, results_equal=False, kernel=kernel, composed_kernel=ckernel))
                    raise SystemExit("the arms disagree: no time is written")
                arms = {"fused": (setk(1), fused, warm(fused, 30.0, 20.0), nb), "composed": (setk(1), composed, warm(composed, 30.0, 20.0), nb)}
                if nb == batches[-1] and name == sizes[-1][0] and cn == 1:
                    arms["fused_fpw1"] = (setk(1, 1), fused, arms["fused"][2], nb)
                if nb == 1:                              # the library's own composed arm, which builds the maps inside the call: what the built-in rule's other branch costs
                    arms["library_composed"] = (setk(0), fused, arms["composed"][2], nb)
                res = alternate(arms, a.groups)
                setk(-1)()
                fused()
                torch.cuda.synchronize()
                rule_kernel = L.mi355cv_lastKernel().decode()
                gus = None
                if nb == 1:
                    x = (src[0] if cn > 1 else src[0][:, :, None]).permute(2, 0, 1)[None].float()
                    gfn = lambda: F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)       # noqa: E731
                    gus = stats([window_us(gfn, warm(gfn, 10.0, 20.0)) for _ in range(3)])
                    del x
                med = statistics.median(res["fused"])
                cus = 2.0 * h * w * cn / (gbs * 1e9) * 1e6
                emit(dict(case=name, frames=nb, cn=cn, op="undistortRectify", fused_us=stats(res["fused"]), composed_us=stats(res["composed"]),
                          fused_fpw1_us=stats(res.get("fused_fpw1")), library_composed_us=stats(res.get("library_composed")), composed_over_fused=round(statistics.median(res["composed"]) / med, 3), results_equal=equal,
                          grid_sample_us=gus, copy_us=round(cus, 2), copy_share=round(cus / med, 3), interleaved=True, kernel=kernel, composed_kernel=ckernel,
                          rule_kernel=rule_kernel))
                del src, dst, ref
        del m1, m2, mx, my, grid

    name, h, w = sizes[-1]
    Q = np.array([[1, 0, 0, -w / 2], [0, 1, 0, -h / 2], [0, 0, 0, 0.8 * w], [0, 0, 1 / 0.12, 0]], np.float64)
    for dt, esz in ((torch.int16, 2), (torch.float32, 4)):
        disp = torch.randint(16, 16 * 128, (h, w), device="cuda", generator=g).to(dt)
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        for hm in (False, True):
            fn = lambda: cv.reprojectImageTo3D(disp, Q, hm, dst=out)                                                      # noqa: E731
            inner = warm(fn, 30.0, 20.0)
            us = [window_us(fn, inner) for _ in range(a.groups)]
            cus = (esz + 12.0) * h * w / (gbs * 1e9) * 1e6
            emit(dict(case=name, op="reprojectImageTo3D", disparity=str(dt).replace("torch.", ""), handleMissingValues=hm, us=stats(us), copy_us=round(cus, 2),
                      copy_share=round(cus / statistics.median(us), 3), kernel=L.mi355cv_lastKernel().decode()))


if __name__ == "__main__":
    main()
