#!/usr/bin/env python
"""connectedComponents (opencv_amd.connectedComponentsBatch / connectedComponentsWithStatsBatch, csrc/ccl.hip) on 3840 x 2160 CV_8UC1 masks resident in HBM:
microseconds per frame, HIP events on the launch stream around a whole batch call (its one host synchronisation included), the median of four timed groups after
at least 30 ms of warm-up.  The batch is sized so that one pass moves at least 2 GiB of algorithmic bytes.  Inputs: `blobs`, thresholded blurred noise with a few
hundred components per frame (the workload the feature is for); `random 0.5`; `serpentine`, one component that crosses every seam (merge depth); `all foreground`
(every statistics update lands on one label); `checkerboard` at connectivity 4 (the most labels a frame can hold).  Rows: labels only and labels + stats, at
connectivity 4 and 8, CV_32S.  `bytes` is the algorithmic traffic -- 1 byte read and 4 written per pixel, plus the stats rows -- `of_8TBs` that traffic per second
over 8 TB/s, and `vs_copy` over `copy_GBs`, mi355cv_copyProbe measured in the same process.  The per-kernel split comes from a separate traced run
(rocprofv3 --kernel-trace --stats -- python tools/ccl_bench.py --batch 8 --groups 1).  A host baseline is recorded only where the reference build is present
(oracle/_ref); otherwise the record says so.  Prints one JSON object per row and appends them to --out (default profiles/ccl_bench.jsonl)."""
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


def blobs(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((n, 1, H, W), device="cuda", generator=g)
    for _ in range(3):
        x = torch.nn.functional.avg_pool2d(x, 31, stride=1, padding=15)
    return ((x[:, 0] > x.mean() + 0.8 * x.std()).to(torch.uint8) * 255).contiguous()


def random_half(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand((n, H, W), device="cuda", generator=g) < 0.5).to(torch.uint8) * 255).contiguous()


def serpentine(n, seed):
    a = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    a[0::2, :] = 255
    a[1::4, W - 1] = 255
    a[3::4, 0] = 255
    return a[None].repeat(n, 1, 1).contiguous()


def all_foreground(n, seed):
    return torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda")


def checkerboard(n, seed):
    yy = torch.arange(H, device="cuda")[:, None]
    xx = torch.arange(W, device="cuda")[None, :]
    return ((((yy + xx) & 1) == 0).to(torch.uint8) * 255)[None].repeat(n, 1, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=52, help="frames per batch: 52 4K frames are 2.0 GiB of source bytes read and CV_32S labels written")
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ccl_bench.jsonl"))
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

    have_ref = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libocvref.so"))
    rows = []
    labels = torch.empty((n, H, W), dtype=torch.int32, device="cuda")
    inputs = (("blobs", blobs, (4, 8)), ("random 0.5", random_half, (4, 8)), ("serpentine", serpentine, (4, 8)), ("all foreground", all_foreground, (4, 8)),
              ("checkerboard", checkerboard, (4,)))
    for name, make, conns in inputs:
        m = make(n, 1)
        for conn in conns:
            counts, _ = cv.connectedComponentsBatch(m, labels=labels, connectivity=conn)
            for stats in (False, True):
                if stats:
                    fn = lambda: cv.connectedComponentsWithStatsBatch(m, labels=labels, connectivity=conn)
                else:
                    fn = lambda: cv.connectedComponentsBatch(m, labels=labels, connectivity=conn)
                usf = timeit(fn, a.groups) / n
                nbytes = H * W * 5 + (max(counts) * 36 if stats else 0)
                gbs = nbytes / usf / 1e3
                rows.append({"row": "connectedComponents%sBatch 4K x%d CV_32S, connectivity %d, %s" % ("WithStats" if stats else "", n, conn, name),
                             "components_per_frame": [min(counts) - 1, max(counts) - 1], "us_per_frame": round(usf, 2), "bytes": nbytes, "GBs": round(gbs, 1),
                             "of_8TBs": round(gbs / 8000.0, 4), "copy_GBs": round(copy_gbs, 1), "vs_copy": round(gbs / copy_gbs, 4), "kernel": L.mi355cv_lastKernel().decode(),
                             "host_baseline": "not measured: the reference build (oracle/_ref) is %s" % ("present but has no labelling entry" if have_ref else "not present")})
        del m
    rows.append({"row": "yardsticks", "copyProbe_GBs": round(copy_gbs, 1), "batch": n, "groups": a.groups, "pass_GiB": round(n * H * W * 5 / 2 ** 30, 2)})
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
