#!/usr/bin/env python
"""cv::fastNlMeansDenoising / fastNlMeansDenoisingColored (opencv_amd.photo, csrc/nlmeans.hip) on frames resident in HBM, the result left on the device.
Microseconds per frame from HIP events on the launch stream around a window of calls of at least 20 ms, the median of --groups windows with their minimum and maximum;
every shape is warmed first.  The two kernels are timed in the same process in alternating rounds (mi355cv_fastNlMeansSetKernel 1 / 0) and their results compared at
the timed size.
  rows      1080p and 4K x CV_8UC1, CV_8UC3 x h = 3, 10 at 7 / 21, single frames; Colored (h = hColor = 3) at both sizes; a batch of 8 frames of 1080p CV_8UC1
  figures   us per frame of the tile kernel and of the forced plain kernel, and three references:
            `vector_bound_us`  the lane operations the tile kernel's design needs -- per pixel and offset 3 cn for the squared differences, 2 for the ring of T rows,
                               T - 1 for the sum over lanes, 2 for the shift and the compare, 1 + cn where the weight is not zero (counted as always), with the walk's
                               (16 + T - 1) / 16 rows and 64 / (64 - (T - 1)) lanes -- over 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz; `vector_share` = that / measured
            `copy_us`          reading and writing the frame at the device-to-device copy rate measured in this run (`copy_gbs`, read + write counted)
            `torch_us`         the same rule composed in torch (the reflect-padded image, per offset the shifted squared differences, avg_pool2d with divisor 1 for
                               the patch sums -- exact in float32 below 2^24 --, a gather from the table), single frames, results compared as well
There is no speed gate against the parent, which has no such path.  Prints one JSON object per row and appends them to --out."""
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

VECTOR_LANE_OPS = 256 * 4 * 32 * 2.4e9


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
    return dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2)) if us else None


def frames(n, h, w, cn, g):
    """smooth frames with noise of sigma 8: N x H x W (x C) uint8 on the device"""
    big = torch.rand((n * cn, 1, h + 8, w + 8), device="cuda", generator=g)
    big = F.avg_pool2d(big, 9, stride=1) * 1500 - 620
    big = big + 8 * torch.randn(big.shape, device="cuda", generator=g)
    out = big.clamp(0, 255).to(torch.uint8).reshape(n, cn, h, w).permute(0, 2, 3, 1).contiguous()
    return out[..., 0].contiguous() if cn == 1 else out


def copy_rate():
    """GB/s of a device-to-device copy of 1 GiB, read + write counted"""
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    fn = lambda: b.copy_(a)
    inner = warm(fn, 20.0, 20.0)
    us = statistics.median(window_us(fn, inner) for _ in range(5))
    return 2 * (1 << 30) / (us * 1e-6) / 1e9


def torch_rule(img, table, shift, th, sh):
    """the rule on one frame [H, W] or [H, W, C], composed of torch operators"""
    a = (img if img.dim() == 3 else img[:, :, None]).permute(2, 0, 1).float()[None]
    H, W = a.shape[2:]
    b, T = th + sh, 2 * th + 1
    ext = F.pad(a, (b, b, b, b), mode="reflect")
    base = ext[:, :, sh:sh + H + 2 * th, sh:sh + W + 2 * th]
    wsum = torch.zeros((H, W), dtype=torch.int64, device=img.device)
    est = torch.zeros((a.shape[1], H, W), dtype=torch.int64, device=img.device)
    last = table.numel() - 1
    for dy in range(-sh, sh + 1):
        for dx in range(-sh, sh + 1):
            d = base - ext[:, :, sh + dy:sh + dy + H + 2 * th, sh + dx:sh + dx + W + 2 * th]
            D = F.avg_pool2d((d * d).sum(dim=1, keepdim=True), T, stride=1, divisor_override=1)[0, 0]
            w = table[(D.long() >> shift).clamp_(max=last)]
            wsum += w
            est += w[None] * ext[0, :, b + dy:b + dy + H, b + dx:b + dx + W].long()
    out = ((est + (wsum // 2)[None]) // wsum[None]).clamp_(max=255).to(torch.uint8).permute(1, 2, 0)
    return out[..., 0] if img.dim() == 2 else out


def design_lane_ops(cn, T):
    per_offset = 3 * cn + 2 + (T - 1) + 2 + 1 + cn
    return per_offset * (16 + T - 1) / 16 * 64 / (64 - (T - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlmeans_bench.jsonl"))
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    prop = torch.cuda.get_device_properties(0)
    dev = dict(device=prop.name, cus=prop.multi_processor_count)
    g = torch.Generator(device="cuda").manual_seed(1)
    gbs = copy_rate()
    sizes = (("1080p", 1080, 1920), ("4K", 2160, 3840)) if not a.small else (("small", 70, 250),)
    setk = _lib.lib.mi355cv_fastNlMeansSetKernel
    tws, sws = 7, 21
    th, sh, S = tws // 2, sws // 2, sws
    rows = [(name, h, w, 1, cn, hh, False) for name, h, w in sizes for cn in (1, 3) for hh in (3.0, 10.0)]
    rows += [(name, h, w, 1, 3, 3.0, True) for name, h, w in sizes]
    rows.append(sizes[0] + (8, 1, 3.0, False))
    made = {}
    for name, h, w, nb, cn, hh, colored in rows:
        if (name, nb, cn) not in made:
            made.clear()
            src = frames(nb, h, w, cn, g)
            made[(name, nb, cn)] = (src, torch.empty_like(src))
        src, dst = made[(name, nb, cn)]
        if colored:
            fn = lambda: cv.fastNlMeansDenoisingColored(src[0], hh, hh, tws, sws, dst=dst[0])
        elif nb == 1:
            fn = lambda: cv.fastNlMeansDenoising(src[0], hh, tws, sws, dst=dst[0])
        else:
            fn = lambda: cv.fastNlMeansDenoisingBatch(src, hh, tws, sws, dst=dst)
        inner, outs, kernels, res = {}, {}, {}, {1: [], 0: []}
        for arm in (1, 0):
            setk(arm)
            inner[arm] = warm(fn, 30.0 if arm else 0.0, 20.0)
            outs[arm] = dst.clone()
            kernels[arm] = _lib.lib.mi355cv_lastKernel().decode()
        for rnd in range(a.groups):
            for arm in ((1, 0) if rnd % 2 == 0 else (0, 1)):
                if arm == 0 and rnd >= 2:                                                # the plain kernel takes many times as long: two windows
                    continue
                setk(arm)
                res[arm].append(window_us(fn, inner[arm]) / nb)
        setk(-1)
        fn()
        torch.cuda.synchronize()
        rule_kernel = _lib.lib.mi355cv_lastKernel().decode()
        med = statistics.median(res[1])
        ops = h * w * S * S * (design_lane_ops(1, tws) + design_lane_ops(2, tws) if colored else design_lane_ops(cn, tws))
        nbytes = 2 * h * w * cn
        tus = teq = None
        if nb == 1 and not colored and not a.no_torch:
            table, shift, _, prefix = cv.fastNlMeansWeights(hh, cn, tws, sws)
            ttab = torch.from_numpy(table[:prefix + 1].astype(np.int64)).cuda()          # the prefix and one zero: indices past it are clamped onto the zero
            tfn = lambda: torch_rule(src[0], ttab, shift, th, sh)
            got = tfn()
            torch.cuda.synchronize()
            teq = bool(torch.equal(got, outs[1][0]))
            tus = round(window_us(tfn, 1), 1)
            del got
        row = dict(case=name, frames=nb, cn=cn, h=hh, colored=colored, templateWindowSize=tws, searchWindowSize=sws,
                   us_per_frame=stats(res[1]), plain_us_per_frame=stats(res[0]), plain_over_tile=round(statistics.median(res[0]) / med, 2),
                   results_equal=bool(torch.equal(outs[1], outs[0])), changed_share=round(float((outs[1] != src).float().mean()), 3),
                   calls_per_window=inner[1], plain_calls_per_window=inner[0], interleaved=True,
                   design_lane_ops=int(ops), vector_bound_us=round(ops / VECTOR_LANE_OPS * 1e6, 1), vector_share=round(ops / VECTOR_LANE_OPS * 1e6 / med, 3),
                   copy_gbs=round(gbs, 1), copy_us=round(nbytes / (gbs * 1e9) * 1e6, 2), torch_us=tus, torch_equal=teq,
                   kernel=kernels[1], plain_kernel=kernels[0], rule_kernel=rule_kernel, **dev)
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
