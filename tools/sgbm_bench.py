#!/usr/bin/env python
"""cv::StereoSGBM (opencv_amd.StereoSGBM, csrc/sgbm.hip) on frames resident in HBM, the CV_16S map left on the device.
Microseconds per frame from HIP events on the launch stream around a window of calls of at least 20 ms, the median of --groups windows with their minimum and maximum;
every shape is warmed first.  The two arms of the path aggregation are timed in the same process in alternating rounds (mi355cv_stereoSGBMSetKernel 1 / 0) and their
maps compared at the timed size.
  rows      1080p and 4K x numDisparities 64, 128 x blockSize 5 x MODE_SGBM, MODE_HH x a single pair and a batch of 8; one row with speckleWindowSize = 100;
            P1 = 8 w^2, P2 = 32 w^2, preFilterCap 31, uniquenessRatio 10, disp12MaxDiff 1
  figures   us per frame of the fast arm and of the forced plain arm, and three references:
            `traffic_bound_us`  the bytes of C and S the design as built moves per valid pixel and disparity -- C written once (2) and read by every direction (2 each),
                                S stored by the first direction (4), read and written by the others (8 each), read by the decision (4) -- over 8 TB/s
            `copy_us`           the same bytes at the device-to-device copy rate measured in this run (`copy_gbs`, read + write counted)
            `torch_one_direction_us`  one horizontal scan of the same recurrence written in torch (a loop over the columns, every step vectorised over rows and
                                disparities), single pairs only; the full aggregation is 5 or 8 of these
There is no speed gate against the parent, which has no such path.  Prints one JSON object per row and appends them to --out."""
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
    """runs fn twice at least and for warm_ms; the calls per timed window that fill window_ms"""
    t0 = time.perf_counter()
    n = 0
    while n < 2 or (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        torch.cuda.synchronize()
        n += 1
    one = (time.perf_counter() - t0) * 1e3 / n
    return int(min(100, max(1, -(-window_ms // one))))


def stats(us):
    return dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))


def frames(n, h, w, shift, g):
    """smooth random frames and their copies shifted by `shift` columns: N x H x W uint8 on the device"""
    big = torch.rand((n, 1, h + 4, w + shift + 4), device="cuda", generator=g)
    big = F.avg_pool2d(big, 5, stride=1) * 255
    return big[:, 0, :, shift:shift + w].to(torch.uint8).contiguous(), big[:, 0, :, :w].to(torch.uint8).contiguous()


def copy_rate():
    """GB/s of a device-to-device copy of 1 GiB, read + write counted"""
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    fn = lambda: b.copy_(a)
    inner = warm(fn, 20.0, 20.0)
    us = statistics.median(window_us(fn, inner) for _ in range(5))
    return 2 * (1 << 30) / (us * 1e-6) / 1e9


def torch_scan(C, P1, P2):
    """L_r for r = (0, 1) over C [H, W1, n] int32"""
    big = 1 << 28
    prev = C[:, 0]
    out = torch.empty_like(C)
    out[:, 0] = prev
    for x in range(1, C.shape[1]):
        M = prev.min(dim=1, keepdim=True).values
        dn = F.pad(prev[:, :-1], (1, 0), value=big) + P1
        up = F.pad(prev[:, 1:], (0, 1), value=big) + P1
        prev = C[:, x] + torch.minimum(torch.minimum(prev, M + P2), torch.minimum(dn, up)) - M
        out[:, x] = prev
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgbm_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    prop = torch.cuda.get_device_properties(0)
    dev = dict(device=prop.name, cus=prop.multi_processor_count)
    g = torch.Generator(device="cuda").manual_seed(1)
    gbs = copy_rate()
    sizes = (("1080p", 1080, 1920), ("4K", 2160, 3840)) if not a.small else (("small", 60, 260),)
    setk = _lib.lib.mi355cv_stereoSGBMSetKernel
    bs = 5
    rows = [(name, h, w, nb, n, mode, 0) for name, h, w in sizes for nb in (1, 8) for n in (64, 128) for mode in (cv.StereoSGBM_MODE_SGBM, cv.StereoSGBM_MODE_HH)]
    rows.append(sizes[0] + (1, 64, cv.StereoSGBM_MODE_SGBM, 100))
    made = {}
    for name, h, w, nb, n, mode, spw in rows:
        if (name, nb) not in made:
            made.clear()
            made[(name, nb)] = frames(nb, h, w, 24, g) + (torch.empty((nb, h, w), dtype=torch.int16, device="cuda"),)
        lefts, rights, disp = made[(name, nb)]
        sg = cv.StereoSGBM_create(0, n, bs, 8 * bs * bs, 32 * bs * bs, 1, 31, 10, spw, 2 if spw else 0, mode)
        fn = (lambda: sg.compute(lefts[0], rights[0], disp=disp[0])) if nb == 1 else (lambda: sg.computeBatch(lefts, rights, disp=disp))
        inner, maps, kernels, res = {}, {}, {}, {1: [], 0: []}
        for arm in (1, 0):
            setk(arm)
            inner[arm] = warm(fn, 30.0 if arm else 0.0, 20.0)
            maps[arm] = disp.clone()
            kernels[arm] = _lib.lib.mi355cv_lastKernel().decode()
        for rnd in range(a.groups):
            for arm in ((1, 0) if rnd % 2 == 0 else (0, 1)):
                if arm == 0 and rnd >= 3:                                                # the plain arm takes several times as long: three windows
                    continue
                setk(arm)
                res[arm].append(window_us(fn, inner[arm]) / nb)
        setk(-1)
        med = statistics.median(res[1])
        valid = h * (w - (n - 1))
        ndir = 8 if mode == cv.StereoSGBM_MODE_HH else 5
        nbytes = valid * n * (2 + 2 * ndir + 4 + 8 * (ndir - 1) + 4)
        tus = None
        if nb == 1 and not spw and mode == cv.StereoSGBM_MODE_SGBM:
            C = torch.randint(0, 2000, (h, w - (n - 1), n), dtype=torch.int32, device="cuda", generator=g)
            tfn = lambda: torch_scan(C, 8 * bs * bs, 32 * bs * bs)
            tfn()
            torch.cuda.synchronize()
            tus = round(window_us(tfn, 1), 1)
            del C
        row = dict(case=name, frames=nb, numDisparities=n, blockSize=bs, mode="HH" if mode == cv.StereoSGBM_MODE_HH else "SGBM", speckleWindowSize=spw,
                   us_per_frame=stats(res[1]), plain_us_per_frame=stats(res[0]), plain_over_fast=round(statistics.median(res[0]) / med, 2),
                   maps_equal=bool(torch.equal(maps[1], maps[0])), kept_share=round(float((maps[1] != -16).float().mean()), 3),
                   calls_per_window=inner[1], plain_calls_per_window=inner[0], interleaved=True,
                   traffic_bytes=nbytes, traffic_bound_us=round(nbytes / 8e12 * 1e6, 1), copy_gbs=round(gbs, 1), copy_us=round(nbytes / (gbs * 1e9) * 1e6, 1),
                   torch_one_direction_us=tus, kernel=kernels[1], plain_kernel=kernels[0], **dev)
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
