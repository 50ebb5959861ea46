#!/usr/bin/env python
"""cv::BFMatcher (opencv_amd.BFMatcher, csrc/bfmatch.hip) on descriptors resident in HBM, matches left on the device.
Microseconds from HIP events on the launch stream around a window of calls (the calls return after the enqueue on torch's stream), the median of --groups windows with
their minimum and maximum.
  rows      32-byte rows (ORB): 500 x 500 with k = 1, k = 2 and crossCheck; 10 000 x 10 000; 100 000 x 100 000; a batch of 64 pairs of 2 000 x 2 000; one generic-path
            row (61 bytes, 10 000 x 10 000) and one CV_32F row of 128 elements (NORM_L2, 4 000 x 4 000)
  figures   us per call, pairs per second and, for the fast kernel, the share of the chip's vector rate that 2 x (dwords per row) lane operations per pair (one XOR,
            one popcount-accumulate) amount to: CUs x 128 lanes x clock from the device properties
  torch     the comparator in the same run on the same GPU: bits unpacked to float16, Hamming = |q| + |t| - 2 q.t through a matmul, topk; its indices are checked
            against ours wherever the k-th and (k+1)-th distances of a query differ (no tie at the list's edge, none inside it)
--ab: the A/B of the split of the train rows (mi355cv_bfSetSplitMode 0 / 1, interleaved rounds in one process) over nq in {64, 500, 4 000, 32 000} at nt = 10 000.
There is no speed gate: the parent has no such path.  Prints one JSON object per row and appends them to --out."""
import argparse
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
from opencv_amd import _lib  # noqa: E402


def window_us(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / inner


def timeit(fn, groups, warm_ms=30.0, window_ms=20.0):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max((time.perf_counter() - t0) * 1e3, 1e-3)
    n = 1
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        fn()
        n += 1
    torch.cuda.synchronize()
    one = min(one, (time.perf_counter() - t0) * 1e3 / n)
    inner = int(min(200, max(1, window_ms / one)))
    return [window_us(fn, inner) for _ in range(groups)], inner


def descriptors(n, nbytes, g):
    return torch.randint(0, 256, (n, nbytes), dtype=torch.uint8, device="cuda", generator=g)


def unpack(d):
    bits = ((d.to(torch.int16)[:, :, None] >> torch.arange(8, device=d.device, dtype=torch.int16)) & 1).reshape(d.shape[0], -1)
    return bits.to(torch.float16)


def torch_knn(q, t, k, chunk=8192):
    """Hamming k-nn through a matmul on the unpacked bits (exact: counts <= 512 in float16 products accumulated in float32), topk per chunk of queries"""
    tb = unpack(t)
    tn = tb.float().sum(1)
    idx, dist = [], []
    for i in range(0, q.shape[0], chunk):
        qb = unpack(q[i:i + chunk])
        d = qb.float().sum(1)[:, None] + tn[None, :] - 2 * (qb @ tb.T).float()
        v, j = torch.topk(d, min(k + 1, d.shape[1]), dim=1, largest=False, sorted=True)
        idx.append(j)
        dist.append(v)
    return torch.cat(dist), torch.cat(idx)


def agreement(ours, cnt, dist, idx, k):
    """rows whose first k + 1 reference distances are pairwise different: the indices must agree there"""
    m = cv.dmatch_records(ours) if hasattr(ours, "cpu") else ours
    if m.ndim == 1:
        m = m[:, None]
    d, j = dist.cpu().numpy(), idx.cpu().numpy()
    clear = (np.diff(d, axis=1) > 0).all(axis=1)
    same = (m["trainIdx"][:, :k] == j[:, :k]).all(axis=1) & (m["distance"][:, :k] == d[:, :k]).all(axis=1)
    return int(clear.sum()), int((clear & ~same).sum())


def row(out, **kw):
    print(json.dumps(kw), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(kw) + "\n")


def stats(us):
    return dict(us_median=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bfmatch_bench.jsonl"))
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "bfmatch_split_ab.jsonl"))
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    prop = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(prop, "clock_rate", 0)) * 1e3 or 2.4e9
    lane_rate = prop.multi_processor_count * 128 * clock_hz
    g = torch.Generator(device="cuda").manual_seed(1)
    scale = 50 if a.small else 1
    dev = dict(device=prop.name, cus=prop.multi_processor_count, clock_mhz=clock_hz / 1e6)

    if a.ab:
        nt = 10000 // scale
        t = descriptors(nt, 32, g)
        for nq in (64, 500, 4000, 32000):
            q = descriptors(max(nq // scale, 1), 32, g)
            for k in (1, 2):
                bf = cv.BFMatcher(cv.NORM_HAMMING)
                res = {0: [], 1: []}
                for rnd in range(a.groups):
                    for mode in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                        _lib.lib.mi355cv_bfSetSplitMode(mode)
                        us, inner = timeit(lambda: bf.knnMatch(q, t, k=k), 1, warm_ms=5.0, window_ms=10.0)
                        res[mode].append(us[0])
                _lib.lib.mi355cv_bfSetSplitMode(-1)
                bf.knnMatch(q, t, k=k)
                row(a.ab_out, shape="%dx%d" % (q.shape[0], nt), k=k, single_pass=stats(res[0]), split_merge=stats(res[1]), rounds=a.groups, interleaved=True,
                    rule_picks=_lib.lib.mi355cv_lastKernel().decode(), **dev)
        return

    def fast_row(name, nq, nt, k, cross=False, nbytes=32, compare=True):
        q, t = descriptors(nq, nbytes, g), descriptors(nt, nbytes, g)
        bf = cv.BFMatcher(cv.NORM_HAMMING, crossCheck=cross)
        fn = lambda: bf.knnMatch(q, t, k=k)
        us, inner = timeit(fn, a.groups)
        med = statistics.median(us)
        kernel = _lib.lib.mi355cv_lastKernel().decode()
        pairs = nq * nt * (2 if cross else 1)
        extra = {}
        if compare:
            _lib.lib.mi355cv_bfSetSplitMode(-1)
            ours, cnt = bf.knnMatch(q, t, k=k) if not cross else cv.BFMatcher(cv.NORM_HAMMING).knnMatch(q, t, k=k)
            tfn = lambda: torch_knn(q, t, k)
            tus, _ = timeit(tfn, max(3, a.groups // 3), warm_ms=5.0, window_ms=1.0)
            dist, idx = torch_knn(q, t, k)
            clear, bad = agreement(ours, cnt, dist, idx, k)
            extra = dict(torch_us_median=round(statistics.median(tus), 2), torch_rows_without_ties=clear, torch_rows_disagreeing=bad)
        row(a.out, case=name, shape="%dx%d" % (nq, nt), row_bytes=nbytes, k=k, crossCheck=cross, calls_per_window=inner, pairs_per_s=round(pairs / med * 1e6, 1),
            vector_rate_share=round(pairs * 2 * (nbytes // 4) / (med * 1e-6) / lane_rate, 4), kernel=kernel, **stats(us), **extra, **dev)

    fast_row("orb 500", 500 // scale, 500 // scale, 1)
    fast_row("orb 500", 500 // scale, 500 // scale, 2)
    fast_row("orb 500 crossCheck", 500 // scale, 500 // scale, 1, cross=True)
    fast_row("10k", 10000 // scale, 10000 // scale, 2)
    fast_row("100k", 100000 // scale, 100000 // scale, 2)

    nb, n = (64, 2000) if not a.small else (3, 40)
    qs, ts = [descriptors(n, 32, g) for _ in range(nb)], [descriptors(n, 32, g) for _ in range(nb)]
    bf = cv.BFMatcher(cv.NORM_HAMMING)
    us, inner = timeit(lambda: bf.knnMatchBatch(qs, ts, 2), a.groups)
    kernel = _lib.lib.mi355cv_lastKernel().decode()
    us1, inner1 = timeit(lambda: [bf.knnMatch(q, t, k=2) for q, t in zip(qs, ts)], a.groups)
    med = statistics.median(us)
    row(a.out, case="batch", shape="%d x %dx%d" % (nb, n, n), row_bytes=32, k=2, calls_per_window=inner, pairs_per_s=round(nb * n * n / med * 1e6, 1),
        vector_rate_share=round(nb * n * n * 16 / (med * 1e-6) / lane_rate, 4), kernel=kernel, single_calls=stats(us1), **stats(us), **dev)

    n = 10000 // scale
    q, t = descriptors(n, 61, g), descriptors(n, 61, g)
    us, inner = timeit(lambda: bf.knnMatch(q, t, k=2), a.groups)
    row(a.out, case="generic 61-byte rows", shape="%dx%d" % (n, n), row_bytes=61, k=2, calls_per_window=inner, pairs_per_s=round(n * n / statistics.median(us) * 1e6, 1),
        kernel=_lib.lib.mi355cv_lastKernel().decode(), **stats(us), **dev)

    n = 4000 // scale
    q, t = torch.randn((n, 128), device="cuda", generator=g), torch.randn((n, 128), device="cuda", generator=g)
    bl = cv.BFMatcher(cv.NORM_L2)
    us, inner = timeit(lambda: bl.knnMatch(q, t, k=2), a.groups)
    row(a.out, case="CV_32F 128 elements, NORM_L2", shape="%dx%d" % (n, n), row_bytes=512, k=2, calls_per_window=inner,
        pairs_per_s=round(n * n / statistics.median(us) * 1e6, 1), kernel=_lib.lib.mi355cv_lastKernel().decode(), **stats(us), **dev)


if __name__ == "__main__":
    main()
