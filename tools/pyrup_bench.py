#!/usr/bin/env python
"""pyrUp (opencv_amd.pyrUp / pyrUpBatch, csrc/pyrup.hip) 1920 x 1080 -> 3840 x 2160: microseconds per frame with HIP events on the launch stream, for batches
resident in HBM (CV_8UC1, CV_8UC3, CV_32FC1; enough frames that source + destination are several times the 256 MB Infinity Cache), for single
device-resident calls that rotate over the frame pairs of that batch (so they too stream from HBM; what they add is one launch per frame), and for the
CV_8UC1 batch on the generic kernel (a source view 4 bytes off the rolling kernel's alignment: same frames, same traffic).  `bytes` is the compulsory traffic of the 1 + 4 model -- every source element read once, four destination elements written -- and
`frac_8TBs` that traffic over 8 TB/s divided into the measured time.  Two yardsticks are measured in the same process and carried by every row:
`copy_GBs`, mi355cv_copyProbe over a buffer of the batch's destination size (bytes read + bytes written per second), and `pyrdown_GBs`, pyrDownBatch on
the same pair of sizes (3840 x 2160 -> 1920 x 1080, CV_8UC1, 4 + 1 bytes per destination pixel).  `vs_copy` and `vs_pyrdown` are the row's rate over them.
Prints one JSON object per row and appends them to --out (default profiles/pyrup_bench.jsonl)."""
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
W, H = 1920, 1080


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


def frames(n, kind, h, w, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "32fc1":
        return torch.rand((n, h, w), dtype=torch.float32, device="cuda", generator=g)
    shape = (n, h, w, 3) if kind == "8uc3" else (n, h, w)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128, help="frames of the CV_8UC1 batch; the other types use as many bytes")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyrup_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = cv._lib.lib

    # yardsticks of this run
    x = frames(a.batch, "8uc1", 2 * H, 2 * W, 1)
    y = torch.empty_like(x)
    nb = x.numel()
    us = timeit(lambda: L.mi355cv_copyProbe(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nb), 1, 1), a.iters)
    copy_gbs = 2.0 * nb / us / 1e3
    del y
    d = torch.empty((a.batch, H, W), dtype=torch.uint8, device="cuda")
    us = timeit(lambda: cv.pyrDownBatch(x, dst=d), a.iters)
    down_gbs = 5.0 * d.numel() / us / 1e3
    down_kernel = L.mi355cv_lastKernel().decode()
    del x, d
    torch.cuda.empty_cache()

    rows = []

    def row(name, us_frame, elems, esz, kernel):
        nbytes = 5 * elems * esz
        gbs = nbytes / us_frame / 1e3
        rows.append({"row": name, "us_per_frame": round(us_frame, 2), "bytes": nbytes, "GBs": round(gbs, 1), "frac_8TBs": round(gbs / HBM, 3),
                     "copy_GBs": round(copy_gbs, 1), "pyrdown_GBs": round(down_gbs, 1), "vs_copy": round(gbs / copy_gbs, 3), "vs_pyrdown": round(gbs / down_gbs, 3),
                     "kernel": kernel})

    for kind, cn, esz in (("8uc1", 1, 1), ("8uc3", 3, 1), ("32fc1", 1, 4)):
        n = max(1, a.batch // (cn * esz))
        s = frames(n, kind, H, W, 2)
        o = torch.empty((n, 2 * H, 2 * W) + tuple(s.shape[3:]), dtype=s.dtype, device="cuda")
        usb = timeit(lambda: cv.pyrUpBatch(s, dst=o), a.iters) / n
        row(f"pyrUpBatch {kind} 1080p->4K x{n}", usb, H * W * cn, esz, L.mi355cv_lastKernel().decode())
        if kind == "8uc1":
            pairs = [(s[i], o[i]) for i in range(n)]
            turn = [0]

            def one():
                src, dst = pairs[turn[0] % n]
                turn[0] += 1
                cv.pyrUp(src, dst=dst)
            us1 = timeit(one, a.iters * n)
            row(f"pyrUp 8uc1 1080p->4K single calls rotating over {n} frame pairs in HBM", us1, H * W, 1, L.mi355cv_lastKernel().decode())
            del pairs
            wide = torch.empty((n, H, W + 8), dtype=torch.uint8, device="cuda")
            off = wide[:, :, 4:4 + W]
            off.copy_(s)
            usg = timeit(lambda: cv.pyrUpBatch(off, dst=o), a.iters) / n
            row(f"pyrUpBatch 8uc1 1080p->4K x{n}, generic kernel (source 4 bytes off alignment)", usg, H * W, 1, L.mi355cv_lastKernel().decode())
            del wide, off
        del s, o
        torch.cuda.empty_cache()
    rows.append({"row": "yardsticks", "copyProbe_GBs": round(copy_gbs, 1), "pyrDownBatch_4K->1080p_8uc1_GBs": round(down_gbs, 1), "pyrdown_kernel": down_kernel,
                 "batch": a.batch})
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
