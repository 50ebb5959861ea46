#!/usr/bin/env python
"""cv::StereoBM (opencv_amd.StereoBM, csrc/stereobm.hip) on frames resident in HBM, the CV_16S map left on the device.
Microseconds per frame from HIP events on the launch stream around a window of calls, the median of --groups windows with their minimum and maximum; every shape is
warmed first.  The two cost kernels are timed in the same process in alternating rounds (mi355cv_stereoBMSetKernel -1 / 0) and their maps compared at the timed size.
  rows      1080p and 4K x numDisparities 64, 128 x blockSize 9, 15, 21 x a single frame and a batch of 8; the other parameters are the defaults
  figures   us per frame; `definition_ops_share`: the numDisparities x blockSize^2 byte differences per valid pixel that the DEFINITION asks for, per second, over the
            chip's integer vector rate (CUs x 64 lanes x clock from the device properties) -- the rolling kernel executes far fewer, so this is a speed-up over the plain
            form expressed in the chip's units, not a utilisation, and may exceed 1; `hbm_share`: the bytes the algorithm needs (two images in, one CV_16S map out: 4
            bytes per pixel) per second over 8 TB/s
  torch     the comparator in the same run on the same GPU: a cost volume of shifted absolute differences, avg_pool2d over the block, argmin (no prefilter, no
            rejects, no sub-pixel step: less work than ours)
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
    """runs fn for warm_ms at least; the calls per timed window that fill window_ms"""
    t0 = time.perf_counter()
    n = 0
    while n < 2 or (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        torch.cuda.synchronize()
        n += 1
    one = (time.perf_counter() - t0) * 1e3 / n
    return int(min(100, max(1, window_ms / one)))


def stats(us):
    return dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))


def frames(n, h, w, shift, g):
    """smooth random frames and their copies shifted by `shift` columns: N x H x W uint8 on the device"""
    big = torch.rand((n, 1, h + 4, w + shift + 4), device="cuda", generator=g)
    big = F.avg_pool2d(big, 5, stride=1) * 255
    return big[:, 0, :, :w].to(torch.uint8).contiguous(), big[:, 0, :, shift:shift + w].to(torch.uint8).contiguous()


def torch_bm(left, right, n, w):
    """N x H x W uint8 -> N x H x W int64 disparities"""
    l, r = left.float()[:, None], right.float()[:, None]
    W = l.shape[-1]
    vol = torch.full((n,) + tuple(l.shape), float("inf"), device=l.device)
    for d in range(n):
        vol[d, ..., d:] = F.avg_pool2d((l[..., d:] - r[..., :W - d]).abs(), w, stride=1, padding=w // 2, count_include_pad=True)
    return vol.argmin(dim=0)[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereobm_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    prop = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(prop, "clock_rate", 0)) * 1e3 or 2.4e9
    int_rate = prop.multi_processor_count * 64 * clock_hz
    dev = dict(device=prop.name, cus=prop.multi_processor_count, clock_mhz=clock_hz / 1e6)
    g = torch.Generator(device="cuda").manual_seed(1)
    sizes = (("1080p", 1080, 1920), ("4K", 2160, 3840)) if not a.small else (("small", 60, 200),)
    setk = _lib.lib.mi355cv_stereoBMSetKernel
    for name, h, w in sizes:
        for nb in (1, 8):
            lefts, rights = frames(nb, h, w, 24, g)
            disp = torch.empty((nb, h, w), dtype=torch.int16, device="cuda")
            for n in (64, 128):
                for bs in (9, 15, 21):
                    bm = cv.StereoBM_create(n, bs)
                    fn = (lambda: bm.compute(lefts[0], rights[0], disp=disp[0])) if nb == 1 else (lambda: bm.computeBatch(lefts, rights, disp=disp))
                    inner, maps, kernels, res = {}, {}, {}, {-1: [], 0: []}
                    for mode in (-1, 0):
                        setk(mode)
                        inner[mode] = warm(fn, 30.0 if mode < 0 else 0.0, 20.0)
                        maps[mode] = disp.clone()
                        kernels[mode] = _lib.lib.mi355cv_lastKernel().decode()
                    groups = a.groups
                    for rnd in range(groups):
                        for mode in ((-1, 0) if rnd % 2 == 0 else (0, -1)):
                            if mode == 0 and rnd >= 3:                                   # the generic kernel takes tens of milliseconds a frame: three windows
                                continue
                            setk(mode)
                            res[mode].append(window_us(fn, inner[mode]) / nb)
                    setk(-1)
                    med = statistics.median(res[-1])
                    valid = h * (w - (n - 1))
                    tus = []
                    if nb == 1 or n == 64:
                        tfn = lambda: torch_bm(lefts, rights, n, bs)
                        tin = warm(tfn, 0.0, 1.0)
                        tus = [window_us(tfn, tin) / nb for _ in range(3)]
                    row = dict(case=name, frames=nb, numDisparities=n, blockSize=bs, us_per_frame=stats(res[-1]), generic_us_per_frame=stats(res[0]),
                               generic_over_fast=round(statistics.median(res[0]) / med, 2), maps_equal=bool(torch.equal(maps[-1], maps[0])),
                               calls_per_window=inner[-1], generic_calls_per_window=inner[0], interleaved=True,
                               definition_ops_share=round(valid * n * bs * bs / (med * 1e-6) / int_rate, 3), hbm_share=round(h * w * 4 / (med * 1e-6) / 8e12, 4),
                               torch_us_per_frame=stats(tus) if tus else None, kernel=kernels[-1], generic_kernel=kernels[0], **dev)
                    print(json.dumps(row), flush=True)
                    with open(a.out, "a") as f:
                        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
