#!/usr/bin/env python
"""CLAHE (opencv_amd.createCLAHE, csrc/clahe.hip) on 4K frames: microseconds per frame for a single apply on a device tensor and for applyBatch of 64 frames,
CV_8UC1 and CV_16UC1, default parameters (clip 40, 8 x 8 tiles), with HIP events on the launch stream.  `frac` is the compulsory traffic -- one read and one
write of every pixel, 2 B/px for 8U and 4 B/px for 16U -- over 8 TB/s, divided into the measured time.  A host-memory apply (numpy in, numpy out: two PCIe
crossings) is timed too, for the library's host-cost class.  Prints one JSON object per row; --out FILE also writes them there."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opencv_amd as cv  # noqa: E402

HBM = 8000.0                      # GB/s
W4, H4 = 3840, 2160


def timeit(fn, n, warm_ms=50.0):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / n              # us per call


def frames(n, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == "8u":
        return torch.randint(0, 256, (n, H4, W4), dtype=torch.uint8, device="cuda", generator=g)
    # 12-bit data stored in 16 bits, the common case for 16U sensors
    return torch.randint(0, 4096, (n, H4, W4), dtype=torch.int16, device="cuda", generator=g).view(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    c = cv.createCLAHE(40.0, (8, 8))
    rows = []
    for dt, bpp in (("8u", 2), ("16u", 4)):
        x = frames(a.batch, dt, 1)
        y = torch.empty_like(x)
        one = x[0]
        one_out = y[0]
        us1 = timeit(lambda: c.apply(one, dst=one_out), a.iters * 5)
        kern = cv._lib.lib.mi355cv_lastKernel().decode()
        usb = timeit(lambda: c.applyBatch(x, dst=y), a.iters) / a.batch
        kernb = cv._lib.lib.mi355cv_lastKernel().decode()
        need = W4 * H4 * bpp / (HBM * 1e3)          # us at 8 TB/s
        rows.append({"row": f"clahe {dt} 4K apply (device tensor)", "us_per_frame": round(us1, 2), "frac_8TBs": round(need / us1, 3), "kernel": kern})
        rows.append({"row": f"clahe {dt} 4K applyBatch x{a.batch}", "us_per_frame": round(usb, 2), "frac_8TBs": round(need / usb, 3), "kernel": kernb})
        host = one.view(torch.int16).cpu().numpy().view(np.uint16) if dt == "16u" else one.cpu().numpy()
        t0 = time.perf_counter()
        n = 10
        for _ in range(n):
            c.apply(host)
        rows.append({"row": f"clahe {dt} 4K apply (numpy host image, staged)", "us_per_frame": round((time.perf_counter() - t0) * 1e6 / n, 1)})
        del x, y
        torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
