#!/usr/bin/env python
"""Bayer demosaicing (opencv_amd.demosaicing / demosaicingBatch, csrc/demosaic.hip) on 3840 x 2160 frames: microseconds per frame with HIP events on the launch
stream, for batches resident in HBM -- CV_8UC1 -> BGR, BGRA and gray on the rolling kernel with its default (transposed) stores and, set through
MI355CV_DEMOSAIC_STORE=lanes, with lane-contiguous stores; CV_8UC1 -> BGR on the generic kernel (a source view 4 bytes off the rolling kernel's alignment: same
frames, same traffic); CV_16UC1 -> BGR -- and for single device-resident calls that rotate over the frame pairs of the batch (so they too stream from HBM; what
they add is one launch per frame).  The batch is sized so that source + destination are several times the 256 MB Infinity Cache.  `bytes` is the compulsory
traffic of the 1 + dcn model -- every source element read once, dcn destination elements written -- and `frac_8TBs` that traffic over 8 TB/s divided into the
measured time.  The yardstick is measured in the same process and carried by every row: `copy_GBs`, mi355cv_copyProbe over a buffer of the BGR batch's
destination size (bytes read + bytes written per second); `vs_copy` is the row's rate over it.
Prints one JSON object per row and appends them to --out (default profiles/demosaic_bench.jsonl)."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import opencv_amd as cv  # noqa: E402

HBM = 8000.0                      # GB/s
W, H = 3840, 2160


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=48, help="frames of the CV_8UC1 batch (48: 0.4 GB in, 1.2 GB of BGR out); CV_16U uses half as many")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demosaic_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = cv._lib.lib
    n = a.batch
    g = torch.Generator(device="cuda").manual_seed(1)

    # yardstick of this run
    x = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    y = torch.empty_like(x)
    nb = x.numel()
    us = timeit(lambda: L.mi355cv_copyProbe(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nb), 1, 1), a.iters)
    copy_gbs = 2.0 * nb / us / 1e3
    del x, y
    torch.cuda.empty_cache()

    rows = []

    def row(name, us_frame, dcn, esz, kernel):
        nbytes = (1 + dcn) * W * H * esz
        gbs = nbytes / us_frame / 1e3
        rows.append({"row": name, "us_per_frame": round(us_frame, 2), "bytes": nbytes, "GBs": round(gbs, 1), "frac_8TBs": round(gbs / HBM, 3),
                     "copy_GBs": round(copy_gbs, 1), "vs_copy": round(gbs / copy_gbs, 3), "kernel": kernel})

    def out_of(frames, dcn):
        return torch.empty(tuple(frames.shape) + ((dcn,) if dcn > 1 else ()), dtype=frames.dtype, device="cuda")

    s = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=g)
    for dcn, code, what in ((3, cv.COLOR_BayerBG2BGR, "BGR"), (4, cv.COLOR_BayerBG2BGRA, "BGRA"), (1, cv.COLOR_BayerBG2GRAY, "GRAY")):
        o = out_of(s, dcn)
        for lay in (("transposed", "lanes") if dcn > 1 else ("",)):
            if lay == "lanes":
                os.environ["MI355CV_DEMOSAIC_STORE"] = "lanes"
            usb = timeit(lambda: cv.demosaicingBatch(s, code, dst=o), a.iters) / n
            os.environ.pop("MI355CV_DEMOSAIC_STORE", None)
            row(f"demosaicingBatch 8u -> {what} 4K x{n}" + (f", {lay} stores" if lay else ""), usb, dcn, 1, L.mi355cv_lastKernel().decode())
        if dcn == 3:
            pairs = [(s[i], o[i]) for i in range(n)]
            turn = [0]

            def one():
                src, dst = pairs[turn[0] % n]
                turn[0] += 1
                cv.demosaicing(src, code, dst=dst)
            us1 = timeit(one, a.iters * n)
            row(f"demosaicing 8u -> BGR 4K single calls rotating over {n} frame pairs in HBM", us1, 3, 1, L.mi355cv_lastKernel().decode())
            del pairs
            wide = torch.empty((n, H, W + 16), dtype=torch.uint8, device="cuda")
            off = wide[:, :, 4:4 + W]
            off.copy_(s)
            usg = timeit(lambda: cv.demosaicingBatch(off, code, dst=o), max(2, a.iters // 4)) / n
            row(f"demosaicingBatch 8u -> BGR 4K x{n}, generic kernel (source 4 bytes off alignment)", usg, 3, 1, L.mi355cv_lastKernel().decode())
            del wide, off
        del o
        torch.cuda.empty_cache()
    del s
    torch.cuda.empty_cache()
    n16 = max(1, n // 2)
    s16 = torch.randint(0, 65536, (n16, H, W), dtype=torch.int32, device="cuda", generator=g).to(torch.int16).view(torch.uint16)
    o16 = out_of(s16, 3)
    us16 = timeit(lambda: cv.demosaicingBatch(s16, cv.COLOR_BayerBG2BGR, dst=o16), max(2, a.iters // 4)) / n16
    row(f"demosaicingBatch 16u -> BGR 4K x{n16}", us16, 3, 2, L.mi355cv_lastKernel().decode())
    rows.append({"row": "yardstick", "copyProbe_GBs": round(copy_gbs, 1), "batch": n})
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
