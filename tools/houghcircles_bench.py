#!/usr/bin/env python
"""HoughCircles (opencv_amd.HoughCircles*, csrc/houghcircles.hip) on 1920 x 1080 and 3840 x 2160 CV_8UC1 frames resident in HBM: synthetic bright discs on a noisy
ground, dp = 1, param1 = 100, param2 = 30, minDist = 20, minRadius = 8, over a ladder of maxRadius (and 0, the default max(rows, cols)).  Microseconds per
call, HIP events on the launch stream around the whole call (its host synchronisations included), the median of --groups timed calls after at least 30 ms of warm-up.

Per row (one frame size, one maxRadius):
  edge_us            opencv_amd.Canny + the two opencv_amd.Sobel planes as separate calls (the stage the full call runs inside itself)
  accum_hbm_us       mi355cv_houghCirclesAccum under mi355cv_houghCirclesSetKernel(0): row counts, prefix, points, k_hc_vote and the copy of the accumulator
  accum_tile_us      the same under SetKernel(1), k_hc_vote_tile (not run when the reach is above --tile-reach cells: every tile would walk nearly every point)
  after_edges_us     mi355cv_houghCirclesGradient with the arm the library chooses: everything after the edge stage, its one synchronisation included
  rest_us            after_edges_us - the chosen arm's accum time: maxima, two sorts, k_hc_radius, k_hc_suppress, the counts' read-back
  full_us            mi355cv_houghCircles; batch8_us_per_frame: mi355cv_houghCirclesBatch over 8 frames, per frame
  furthest_stage     the stage with the lowest (bytes it must touch at least once) / time, as a fraction of mi355cv_copyProbe's rate measured in the same run
The arm crossing -- the largest reach (maxRadius / dp, in cells) at which the tile arm is still the faster one -- decides whether the library ever chooses it.
There is no speed gate: the parent has no such path.  Prints one JSON object per row and writes them to --out (default profiles/houghcircles_bench.jsonl)."""
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

CV_16S, BORDER_REPLICATE = 3, 1
DP, MIN_DIST, P1, P2, MIN_RADIUS = 1.0, 20.0, 100, 30, 8


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


def scene(w, h, seed):
    """discs of radius 10 .. 120 on a ground of 40 +- 6 grey levels, about one disc per 260 x 260 pixels"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.full((h, w), 40.0, device="cuda")
    yy = torch.arange(h, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(w, device="cuda", dtype=torch.float32)[None, :]
    cpu = torch.Generator().manual_seed(seed)
    for _ in range(max(4, (w * h) // (260 * 260))):
        cx, cy = float(torch.randint(0, w, (1,), generator=cpu)), float(torch.randint(0, h, (1,), generator=cpu))
        r = float(torch.randint(10, 121, (1,), generator=cpu))
        img = torch.where((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r, torch.full_like(img, 150.0 + float(torch.randint(0, 90, (1,), generator=cpu))), img)
    img = img + torch.randint(-6, 7, (h, w), device="cuda", generator=g).float()
    return img.clamp(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--radii", default="16,32,48,64,96,128,256,512,0")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--tile-reach", type=int, default=600, help="the tile arm is not timed above this reach (cells)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "houghcircles_bench.jsonl"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = cv._lib.lib
    setk = L.mi355cv_houghCirclesSetKernel
    rows = []

    x = torch.empty((16, 2160, 3840, 4), dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    nb = x.numel()
    us = timeit(lambda: L.mi355cv_copyProbe(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_size_t(nb), 1, 1), a.groups)
    copy_gbs = 2.0 * nb / us / 1e3
    del x, y
    torch.cuda.empty_cache()

    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        frames = torch.stack([scene(w, h, s) for s in range(a.batch)])
        img = frames[0]
        low, high = max(1, P1 // 2), P1

        def edge_stage():
            return cv.Canny(img, low, high), cv.Sobel(img, CV_16S, 1, 0, 3, borderType=BORDER_REPLICATE), cv.Sobel(img, CV_16S, 0, 1, 3, borderType=BORDER_REPLICATE)

        edges, dx, dy = edge_stage()
        edge_us = timeit(edge_stage, a.groups)
        points = int((edges != 0).sum())
        for max_radius in (int(v) for v in a.radii.split(",")):
            reach = max_radius if max_radius > 0 else max(w, h)
            row = {"row": "HoughCircles %dx%d CV_8UC1, discs on noise, dp 1, param1 %d, param2 %d, minDist %g, radius %d..%d" % (w, h, P1, P2, MIN_DIST, MIN_RADIUS, max_radius),
                   "reach_cells": reach, "edge_pixels": points, "edge_us": round(edge_us, 1), "copy_GBs": round(copy_gbs, 1)}
            accum = {}
            for arm, key in ((0, "accum_hbm_us"), (1, "accum_tile_us")):
                if arm == 1 and reach > a.tile_reach:
                    row[key] = "not run: reach above --tile-reach"
                    continue
                setk(arm)
                acc = cv.HoughCirclesAccumulator(edges, dx, dy, DP, MIN_RADIUS, max_radius)
                accum[arm] = acc if arm == 0 else accum[0]
                if arm == 1:
                    row["arms_identical"] = bool(torch.equal(acc, accum[0]))
                row[key] = round(timeit(lambda: cv.HoughCirclesAccumulator(edges, dx, dy, DP, MIN_RADIUS, max_radius), a.groups), 1)
            setk(-1)
            out = cv.HoughCirclesGradient(edges, dx, dy, DP, MIN_DIST, P2, MIN_RADIUS, max_radius)
            row["kernel"] = L.mi355cv_lastKernel().decode()
            row["circles"] = int(out.shape[0])
            chosen = "accum_tile_us" if row["kernel"].startswith("k_hc_vote_tile") else "accum_hbm_us"
            row["after_edges_us"] = round(timeit(lambda: cv.HoughCirclesGradient(edges, dx, dy, DP, MIN_DIST, P2, MIN_RADIUS, max_radius), a.groups), 1)
            row["rest_us"] = round(row["after_edges_us"] - row[chosen], 1) if isinstance(row[chosen], float) else None
            row["full_us"] = round(timeit(lambda: cv.HoughCircles(img, cv.HOUGH_GRADIENT, DP, MIN_DIST, P1, P2, MIN_RADIUS, max_radius), a.groups), 1)
            if max_radius in (64, 0):
                counts, _ = cv.HoughCirclesBatch(frames, cv.HOUGH_GRADIENT, DP, MIN_DIST, P1, P2, MIN_RADIUS, max_radius)
                row["batch%d_us_per_frame" % a.batch] = round(timeit(lambda: cv.HoughCirclesBatch(frames, cv.HOUGH_GRADIENT, DP, MIN_DIST, P1, P2, MIN_RADIUS, max_radius),
                                                                     a.groups) / a.batch, 1)
                row["batch_circles"] = [min(counts), max(counts)]
            # what each stage must touch at least once: the frame and its three planes for the edges; the three planes and the accumulator for the vote; the
            # accumulator and the candidate keys (written, sorted, read) for the rest
            cells = (h + 2) * (w + 2)
            need = {"edges": w * h * (1 + 2 + 2 + 1), "vote (" + chosen + ")": w * h * 5 + cells * 4, "rest": cells * 4 + 3 * 8 * (h * ((w + 1) // 2))}
            took = {"edges": edge_us, "vote (" + chosen + ")": row[chosen], "rest": row["rest_us"]}
            frac = {k: need[k] / (took[k] * 1e3) / copy_gbs for k in need if isinstance(took[k], float) and took[k] > 0}
            row["fraction_of_copy_rate"] = {k: round(v, 4) for k, v in frac.items()}
            row["furthest_stage"] = min(frac, key=frac.get) if frac else None
            rows.append(row)
            print(json.dumps(row), flush=True)
        both = [r for r in rows if r["row"].startswith("HoughCircles %dx%d" % (w, h)) and isinstance(r["accum_tile_us"], float)]
        wins = [r["reach_cells"] for r in both if r["accum_tile_us"] < r["accum_hbm_us"]]
        cross = {"row": "arm crossing %dx%d" % (w, h), "tile_faster_at_reach": wins, "largest_reach_tile_wins": max(wins) if wins else None,
                 "tile_over_hbm": {str(r["reach_cells"]): round(r["accum_tile_us"] / r["accum_hbm_us"], 3) for r in both}}
        rows.append(cross)
        print(json.dumps(cross), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:                                         # one run, one record: never stacked under an older build's rows
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
