#!/usr/bin/env python
"""minMaxLoc (opencv_amd.minMaxLocBatch, csrc/minmax.hip) on a batch of 3840 x 2160 frames resident in HBM: CV_8UC1 and CV_32FC1, unmasked and with a CV_8UC1
mask of its own per frame, results left on the device (device=True: no read-back).  Microseconds per frame, HIP events on the launch stream around a whole batch
call, the median of --groups timed calls after at least 30 ms of warm-up.  Three numbers from the SAME run:
  frac_of_8TBs     bytes the call has to read (source, plus the mask when there is one) per second, over 8 TB/s;
  frac_of_copy     the same bytes per second over the rate of mi355cv_copyProbe measured in this process.  The copy's rate counts the bytes it reads AND the bytes it
                   writes; a reduction only reads, so at equal memory traffic per second the ratio is 1 although the reduction takes half a copy's time per
                   source byte;
  torch_us         torch.amin + amax + argmin + argmax over the same tensors (four reductions; no mask -- torch has no masked form, the masked rows repeat
                   the unmasked figure), as an independent comparator.  NaN-free data, so that both compute the same thing.
There is no speed gate: the parent has no such path.  Prints one JSON object per row and appends them to --out (default profiles/minmax_bench.jsonl)."""
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


def torch_four(frames):
    flat = frames.reshape(frames.shape[0], -1)
    return flat.amin(1), flat.amax(1), flat.argmin(1), flat.argmax(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--groups", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minmax_bench.jsonl"))
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
    mask = (torch.rand((n, H, W), device="cuda", generator=g) < 0.5).to(torch.uint8)
    rows = []
    for name, frames in (("CV_8UC1", torch.randint(0, 256, (n, H, W), device="cuda", generator=g, dtype=torch.uint8)),
                         ("CV_32FC1", torch.randn((n, H, W), device="cuda", generator=g))):
        esz = frames.element_size()
        t_us = timeit(lambda: torch_four(frames), a.groups) / n
        for m in (None, mask):
            vals, locs = cv.minMaxLocBatch(frames, m, device=True)
            kernel = L.mi355cv_lastKernel().decode()
            if m is None:                                                    # the comparator doubles as a check of this run's results
                lo, hi, alo, ahi = torch_four(frames)
                assert torch.equal(vals[:, 0], lo.double()) and torch.equal(vals[:, 1], hi.double())
                if frames.is_floating_point():                               # torch does not promise the first index on ties, which CV_8U is full of
                    assert torch.equal(locs[:, 1].long() * W + locs[:, 0], alo) and torch.equal(locs[:, 3].long() * W + locs[:, 2], ahi)
            usf = timeit(lambda: cv.minMaxLocBatch(frames, m, device=True), a.groups) / n
            nbytes = H * W * (esz + (1 if m is not None else 0))
            gbs = nbytes / usf / 1e3
            rows.append({"row": "minMaxLocBatch 4K x%d %s, %s, results on the device" % (n, name, "masked (one CV_8UC1 mask per frame)" if m is not None else "unmasked"),
                         "us_per_frame": round(usf, 2), "bytes_read_per_frame": nbytes, "read_GBs": round(gbs, 1), "frac_of_8TBs": round(gbs / 8000.0, 3),
                         "copy_GBs": round(copy_gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 3),
                         "torch_amin_amax_argmin_argmax_us_per_frame": round(t_us, 2), "kernel": kernel})
    for row in rows:
        print(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
