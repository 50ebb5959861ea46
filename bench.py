#!/usr/bin/env python
"""bench.py -- headline metric of BASELINE.json: Mpix/s of cv::GaussianBlur 5x5 (sigma=0) on
3840x2160 CV_8U frames + achieved HBM GB/s against the MI355X roofline.

A "step" is one pass of the hot path over one batch: B device-resident 4K 8UC1 frames per GPU through
mi355cv_gaussianBlurBinomialBatch, issued as B / 512 consecutive launches over sub-batches of 512 frames (each with its own
event pair).  B is sized for the GPU's HBM (pick_batch: 9216 frames = 153 GB of source + destination on a 288 GB MI355X),
so a step is ~26 ms and 20 steps span > 0.5 s.  Frames are independent units, so N GPUs = N processes each owning its own
frames: weak scaling, no data-path collective; the only collective is the RCCL broadcast of the launch plan (filter size,
border rule, frames per launch -- rank 0 decides, every rank runs what it received) at plan time.
`python bench.py --gpus N` spawns the N ranks itself when no launcher did (torch.distributed.run) and refuses to run on
fewer than N GPUs.

A plain run does only what the headline needs: set up, warm up, time `--steps` steps, write the outputs (`--dump-outputs DIR`) and
print the line.  `roofline.achieved` / `frac` come from the events of the timed launches themselves.

`--full` adds everything else: the bit-exact parity gate before the timed region and, after it, the measured copy rate, the cfg4 / cfg5
legs on N > 1 GPUs, and on one GPU `roofline.traffic` (rank 0 re-runs one sub-batch of the same launch geometry under
`rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE`, separate passes, nothing else traced, together with a 16 B / lane copy of known
size that calibrates both counters on the GPU at hand), `cpu_baseline`, BASELINE configs 2-5 and the host-inclusive rows.

Prints ONE JSON line on rank 0 (contract in the task statement); under --full it includes `cpu_baseline` and the per-config summary.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W4K, H4K = 3840, 2160
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
ALGO_BYTES_PER_PIXEL = 2.0     # 1 B read + 1 B written per 8UC1 pixel


def host_cpu():
    """CPU model and last-level cache of the box ("core count and CPU model printed")"""
    model, llc = "unknown", None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip(); break
    except OSError:
        pass
    try:
        best = -1
        base = "/sys/devices/system/cpu/cpu0/cache"
        for d in os.listdir(base):
            lvl = int(open(os.path.join(base, d, "level")).read())
            if lvl > best and open(os.path.join(base, d, "type")).read().strip() != "Instruction":
                best, llc = lvl, f"L{lvl} {open(os.path.join(base, d, 'size')).read().strip()}"
    except (OSError, ValueError):
        pass
    if llc is None:                                             # containers often hide /sys/devices/system/cpu/*/cache: ask lscpu
        try:
            import subprocess
            for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
                if line.strip().startswith("L3 cache"):
                    llc = "L3 " + line.split(":", 1)[1].strip(); break
        except Exception:
            pass
    return model, llc


def cpu_baseline(budget_s=12.0):
    """Reference CPU path on this box's host cores, bounded sample (rank 0, N=1 only)."""
    cpu_model, cpu_llc = host_cpu()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc
    NF = 160                                              # 160 distinct frames: 1.33 GB in + 1.33 GB out per sweep, 5x the 512 MiB L3 of the
                                                          # EPYC 9575F boxes (r04's 32 frames = 530 MB partly sat in it: VERDICT r4)
    ref = orc.load_ref()
    if ref is not None:
        # inputs from cv::RNG(809564) of the reference itself (rng.fill UNIFORM [0,256)), one tall Mat viewed as NF frames
        frames = orc.ref_rng_fill((NF * H4K, W4K), np.uint8, 809564, 0, 256).reshape(NF, H4K, W4K)
    else:
        frames = np.random.default_rng(809564).integers(0, 256, (NF, H4K, W4K), dtype=np.uint8)
    frame = frames[0]
    if ref is not None:
        import ctypes
        cores = ref.ref_getNumberOfCPUs()
        ref.ref_setNumThreads(cores)
        dsts = np.empty_like(frames)
        def run(i):
            s, d = frames[i % NF], dsts[i % NF]
            rc = ref.ref_GaussianBlur(orc.P(s), orc.step(s), orc.P(d), orc.step(d), W4K, H4K, 0, 5, 5,
                                      ctypes.c_double(0), ctypes.c_double(0), 4)
            assert rc == 0
        for i in range(NF):
            run(i)                                        # warm-up (thread pool, page faults)
        n, t0 = 0, time.perf_counter()
        while True:
            run(n)
            n += 1
            dt = time.perf_counter() - t0
            if dt > budget_s or n >= 200000:
                break
        # SURVEY §8d also asks for the one-thread figure: 3 s of the same calls with cv::setNumThreads(1)
        ref.ref_setNumThreads(1)
        run(0)
        n1, t1 = 0, time.perf_counter()
        while time.perf_counter() - t1 < 3.0:
            run(n1); n1 += 1
        dt1 = time.perf_counter() - t1
        ref.ref_setNumThreads(cores)
        try:
            allowed = len(os.sched_getaffinity(0))
        except AttributeError:
            allowed = os.cpu_count()
        return {"value": round(n * W4K * H4K / dt / 1e6, 1), "unit": "Mpix/s", "cores": int(cores), "kind": "reference",
                "one_thread_Mpix_s": round(n1 * W4K * H4K / dt1 / 1e6, 1),
                "cpu_model": cpu_model, "cpu_llc": cpu_llc, "logical_cpus": os.cpu_count(), "cpus_allowed": allowed,
                "sample_short": f"{n} x cv::GaussianBlur 5x5 over {NF} distinct 4K 8UC1 frames ({2 * NF * W4K * H4K / 1e9:.2f} GB cycle > LLC {cpu_llc}), "
                                f"{cores} threads, {dt:.1f} s; 1 thread: {n1} calls {dt1:.1f} s; reference built by oracle/ref/Makefile",
                "sample": f"{n} x cv::GaussianBlur(5x5,sigma=0,REFLECT_101) cycling over {NF} distinct 3840x2160 CV_8UC1 frames, "
                          f"{cores} threads = cv::getNumberOfCPUs() of this process (the box shows {os.cpu_count()} logical CPUs, the container's cgroup / affinity "
                          f"limit leaves {cores}); one_thread_Mpix_s = {n1} of the same calls under cv::setNumThreads(1) in {dt1:.1f} s; "
                          f"(oracle/_ref build of the reference: SSE3 baseline, smooth dispatched to AVX2 -- the widest its CMake lists --, "
                          f"pthreads backend, no IPP / OpenCL), inputs from cv::RNG(809564), {dt:.1f} s"}
    crop = np.ascontiguousarray(frame[:540, :960])
    n, t0 = 0, time.perf_counter()
    while True:
        orc.orc_gaussianBlurBinomialU8(crop, 5, 4)
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s:
            break
    return {"value": round(n * crop.size / dt / 1e6, 1), "unit": "Mpix/s", "cores": 1, "kind": "port", "cpu_model": cpu_model, "cpu_llc": cpu_llc,
            "sample": f"{n} x oracle C restatement on a 960x540 crop, 1 thread, {dt:.1f} s"}


def other_configs(with_cpu=True):
    """BASELINE.json configs 2-5 on this GPU (tools/bench_configs.py: HIP-event times, algorithmic bytes / flops) with the
    reference's CPU path timed beside them on the host cores (rank 0, N=1 only; reported, never part of `value`)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_configs
    rows = bench_configs.run(quick=False)
    if not with_cpu:
        return rows
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc
    if orc.load_ref() is None:
        return rows
    rng = np.random.default_rng(809564)

    def t(fn, reps=2):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e3

    cpu = {}
    bgr = rng.integers(0, 256, (H4K, W4K, 3), dtype=np.uint8)
    gray = orc.ref_cvtColor(bgr, 6, 1)
    cpu["cfg2a"] = t(lambda: orc.ref_cvtColor(bgr, 6, 1))
    k = np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], np.float32)
    cpu["cfg2c"] = t(lambda: orc.ref_filter2D(gray, -1, k))
    f8k = rng.random((4320, 7680), dtype=np.float32)
    cpu["cfg3a"] = t(lambda: orc.ref_resize(f8k, (5120, 2880)))
    cpu["cfg3b"] = t(lambda: orc.ref_resize(f8k, (3840, 2160)))
    M = orc.ref_getRotationMatrix2D((7680 / 2.0, 4320 / 2.0), 7.0, 0.95)
    cpu["cfg3c"] = t(lambda: orc.ref_warpAffine(f8k, M, (7680, 4320), 1, 0, 0.0))
    hd = np.ascontiguousarray(gray[:1080, :1920])
    cpu["cfg4a"] = t(lambda: orc.ref_cornerHarris(hd, 2, 3, 0.04))

    def pyr():
        l = hd
        for _ in range(4):
            l = orc.ref_pyrDown(l)
    cpu["cfg4b"] = t(pyr)
    tpl = rng.integers(0, 256, (128, 128), dtype=np.uint8)
    cpu["cfg5"] = t(lambda: orc.ref_matchTemplate(gray, tpl, 3), reps=1)
    # the long separable kernels: cv::GaussianBlur sigma 3 / 5.5 / 21 on CV_8U (19 / 33 / 129 taps: sepmx.hip), sigma 16 / 3 on CV_32F with 97 / 19 taps (seplong.hip)
    cpu["gs3"] = t(lambda: orc.ref_GaussianBlur(gray, (19, 19), 3.0, 3.0, 4))
    cpu["gs3c3"] = t(lambda: orc.ref_GaussianBlur(bgr, (19, 19), 3.0, 3.0, 4))
    cpu["gs5"] = t(lambda: orc.ref_GaussianBlur(gray, (33, 33), 5.5, 5.5, 4))
    cpu["gs21"] = t(lambda: orc.ref_GaussianBlur(gray, (129, 129), 21.0, 21.0, 4), reps=1)
    cpu["gs15"] = t(lambda: orc.ref_GaussianBlur(gray, (9, 9), 1.5, 1.5, 4))
    f4k = np.ascontiguousarray(f8k[:H4K, :W4K])
    cpu["gs16"] = t(lambda: orc.ref_GaussianBlur(f4k, (97, 97), 16.0, 16.0, 4), reps=1)
    cpu["gs3f"] = t(lambda: orc.ref_GaussianBlur(f4k, (19, 19), 3.0, 3.0, 4))
    try:
        rows += next_rows(orc, t, gray, bgr, hd)
    except Exception as e:                                      # reported rows only: never lose the headline line over them
        rows.append({"config": "next rows", "error": repr(e)})
    for r in rows:
        key = r["config"].split()[0]
        if key in cpu:
            r["cpu_reference_ms_per_frame"] = round(cpu[key], 3)
            if "frames" in r and "ms" in r:
                r["gpu_ms_per_frame"] = round(r["ms"] / r["frames"], 4)
    return rows


def next_rows(orc, t, gray, bgr, hd):
    """SURVEY §8 "next" rows (f1 / f3 / f4) on one frame: end-to-end time per call through the Python mirror on device-resident data
    (includes ~14 us of host time per hook call) beside the reference's CPU path.  Kernel durations: profiles/r01g_f1_kernel_stats.csv."""
    import opencv_amd as cv

    def g(fn, reps=10):
        fn(); fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    dgray, dbgr, dhd = torch.from_numpy(gray).cuda(), torch.from_numpy(bgr).cuda(), torch.from_numpy(hd).cuda()
    nv = np.ascontiguousarray(np.concatenate([gray, gray[: H4K // 2]], axis=0))
    dnv = torch.from_numpy(nv).cuda()
    out = []

    def row(name, gpu_ms, cpu_ms):
        out.append({"config": name, "gpu_ms_per_call": round(gpu_ms, 4), "cpu_reference_ms_per_frame": round(cpu_ms, 3), "speedup": round(cpu_ms / gpu_ms, 1)})

    row("f1 Canny 3840x2160 8UC1 (50,150)", g(lambda: cv.Canny(dgray, 50, 150)), t(lambda: orc.ref_Canny(gray, 50, 150)))
    row("f1 medianBlur 5x5 3840x2160 8UC1", g(lambda: cv.medianBlur(dgray, 5)), t(lambda: orc.ref_medianBlur(gray, 5)))
    row("f1 equalizeHist 3840x2160", g(lambda: cv.equalizeHist(dgray)), t(lambda: orc.ref_equalizeHist(gray)))
    row("f1 threshold OTSU 3840x2160", g(lambda: cv.threshold(dgray, 0, 255, 8)), t(lambda: orc.ref_threshold(gray, 0, 255, 8)))
    row("f4 NV12->BGR 3840x2160", g(lambda: cv.cvtColor(dnv, 91)), t(lambda: orc.ref_cvtColorYUV(nv, 91)))
    row("f4 BGR->I420 3840x2160", g(lambda: cv.cvtColor(dbgr, 128)), t(lambda: orc.ref_cvtColorMisc(bgr, 128)))
    row("f2 resize LANCZOS4 4K->2880x1620 8UC1", g(lambda: cv.resize(dgray, (2880, 1620), interpolation=4), 5), t(lambda: orc.ref_resize(gray, (2880, 1620), interpolation=4)))
    # f3: sparse pyramidal LK, 1080p pair, 5000 points, 21x21 window, 4 levels
    rng = np.random.default_rng(7)
    smooth = orc.ref_GaussianBlur(orc.ref_GaussianBlur(hd, 5, 0, 0, 4), 5, 0, 0, 4)
    nxt = np.ascontiguousarray(np.roll(smooth, (2, 3), axis=(0, 1)))
    pts = (rng.random((5000, 2)) * [1900, 1060] + 10).astype(np.float32)
    dprev, dnext, dpts = torch.from_numpy(smooth).cuda(), torch.from_numpy(nxt).cuda(), torch.from_numpy(pts).cuda()
    row("f3 calcOpticalFlowPyrLK 1920x1080, 5000 pts, 21x21, maxLevel 3", g(lambda: cv.calcOpticalFlowPyrLK(dprev, dnext, dpts, None, (21, 21), 3), 5),
        t(lambda: orc.ref_calcOpticalFlowPyrLK(smooth, nxt, pts, (21, 21), 3)))
    # the tracking front end as one pipeline on a 1080p NV12 frame pair: decode -> gray -> Gaussian 5x5 -> goodFeaturesToTrack(1000) on the
    # previous frame -> pyramidal LK into the current one.  GPU: every image stays in HBM (only the corner list crosses PCIe, as in cv::).
    bgr0 = np.ascontiguousarray(np.stack([smooth, np.roll(smooth, 5, 1), np.roll(smooth, 9, 0)], axis=-1))
    bgr1 = np.ascontiguousarray(np.roll(bgr0, (2, 3), axis=(0, 1)))
    nv0, nv1 = orc.ref_cvtBGRtoTwoPlaneYUV(bgr0, 0, 1), orc.ref_cvtBGRtoTwoPlaneYUV(bgr1, 0, 1)
    dnv0, dnv1 = torch.from_numpy(nv0).cuda(), torch.from_numpy(nv1).cuda()
    ntracked = {}

    def pipe_gpu():
        g0 = cv.GaussianBlur(cv.cvtColor(cv.cvtColor(dnv0, 91), 6), (5, 5), 0)
        g1 = cv.GaussianBlur(cv.cvtColor(cv.cvtColor(dnv1, 91), 6), (5, 5), 0)
        c = cv.goodFeaturesToTrack(g0, 1000, 0.01, 10)
        _, st, _ = cv.calcOpticalFlowPyrLK(g0, g1, torch.from_numpy(c).cuda(), None, (21, 21), 3)
        ntracked["gpu"] = int(st.sum())

    def pipe_cpu():
        g0 = orc.ref_GaussianBlur(orc.ref_cvtColor(orc.ref_cvtColorYUV(nv0, 91), 6, 1), 5, 0, 0, 4)
        g1 = orc.ref_GaussianBlur(orc.ref_cvtColor(orc.ref_cvtColorYUV(nv1, 91), 6, 1), 5, 0, 0, 4)
        c = orc.ref_goodFeaturesToTrack(g0, 1000, 0.01, 10)
        _, st, _ = orc.ref_calcOpticalFlowPyrLK(g0, g1, c, (21, 21), 3)
        ntracked["cpu"] = int(st.sum())

    row("f3 pipeline 1920x1080: 2x(NV12->BGR->GRAY->Gaussian5x5), goodFeaturesToTrack(1000), calcOpticalFlowPyrLK", g(pipe_gpu, 5), t(pipe_cpu))
    out[-1]["tracked_gpu_cpu"] = [ntracked.get("gpu"), ntracked.get("cpu")]
    return out


def host_inclusive():
    """SURVEY §8d / BASELINE.md §4.4: H2D + D2H-inclusive throughput beside the kernel-only figure.  Frames and results live in page-locked HOST
    memory; the library's pipelined batch entry (rt.h runHostBatch: upload of chunk k+1 and download of chunk k-1 under the kernel of chunk k) is timed
    wall-clock around the whole call.  Reported, never `value`."""
    import opencv_amd as cv
    rows = []

    def wall(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    n = 64
    src = torch.randint(0, 256, (n, H4K, W4K), dtype=torch.uint8).pin_memory()
    dst = torch.empty_like(src).pin_memory()
    ms = wall(lambda: cv.GaussianBlurBatch(src, 5, dst=dst))
    rows.append({"config": "host-inclusive: GaussianBlur 5x5, 64 x 4K 8UC1 from / to page-locked host memory (pipelined H2D + kernel + D2H)", "frames": n, "ms": round(ms, 3),
                 "us_per_frame": round(ms / n * 1e3, 1), "Mpix_s": round(n * W4K * H4K / ms / 1e3, 1), "pcie_GBs_both_ways": round(2 * src.numel() / ms / 1e6, 1)})
    d = torch.empty((n, H4K, W4K), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms_up = wall(lambda: d.copy_(src, non_blocking=True))
    ms_dn = wall(lambda: dst.copy_(d, non_blocking=True))
    rows.append({"config": "host-inclusive: plain hipMemcpyAsync of the same 64 frames (the PCIe ceiling of this box)", "h2d_GBs": round(src.numel() / ms_up / 1e6, 1), "d2h_GBs": round(src.numel() / ms_dn / 1e6, 1)})
    del d
    try:
        bgr = torch.randint(0, 256, (24, H4K, W4K, 3), dtype=torch.uint8).pin_memory()
        gray = torch.empty((24, H4K, W4K), dtype=torch.uint8).pin_memory()
        ms = wall(lambda: cv.cvtColorBatch(bgr, cv.COLOR_BGR2GRAY, dst=gray))
        rows.append({"config": "host-inclusive: cvtColor BGR2GRAY, 24 x 4K 8UC3 from / to page-locked host memory", "frames": 24, "ms": round(ms, 3), "us_per_frame": round(ms / 24 * 1e3, 1),
                     "Mpix_s": round(24 * W4K * H4K / ms / 1e3, 1), "pcie_GBs_both_ways": round((bgr.numel() + gray.numel()) / ms / 1e6, 1)})
    except Exception as e:                                      # noqa: BLE001 -- reported rows only
        rows.append({"config": "host-inclusive cvtColor", "error": repr(e)[:200]})
    return rows


SUMMARY_KEYS = ("cfg2a", "cfg2c", "cfg2e", "cfg2d", "cfg3a", "cfg3b", "cfg3c", "cfg4a", "cfg4b", "cfg5", "cfg5f")


def compact_summary(rows):
    """BASELINE cfg1-cfg5 and the weakest rows as {key: [ms per frame, fraction of the bounding roofline]} -- printed LAST in the JSON line so that all of them
    survive a tail-only record of the output.  Fractions: of 8 TB/s for HBM rows, of the i8 (cfg5) / bf16 (cfg5f) dense MFMA peak."""
    out = {}
    short = {"a1 GaussianBlur 5x5 4K 8UC3 batch": "gauss_8uc3", "a1 GaussianBlur 5x5 1080p 8UC1 batch": "gauss_1080p", "a1 GaussianBlur 5x5 8K 8UC1 batch": "gauss_8k",
             "a8 warpAffine 4K 8UC1": "affine_8uc1", "a8 warpAffine 4K 8UC3": "affine_8uc3", "a9 warpPerspective 4K 8UC1": "persp_8uc1", "a9 warpPerspective 4K 8UC3": "persp_8uc3",
             "f1 integral 4K 8U -> 32S batch": "integral", "a7 resize 1080p 8UC3 -> 4K bilinear": "up2x_lin_8uc3", "a7 resize 1080p 8UC3 -> 4K INTER_CUBIC": "up2x_cubic_8uc3",
             "f2 warpAffine 4K 8UC1 rot 7deg INTER_CUBIC": "affine_cubic_8uc1", "f2 warpAffine 4K 8UC1 rot 7deg INTER_LANCZOS4": "affine_lanczos_8uc1",
             "a4 Sobel dx 3x3 4K 8U->16S batch": "sobel_16s", "gs3 GaussianBlur": "gauss_sigma3_8uc1", "gs3c3 GaussianBlur": "gauss_sigma3_8uc3", "gs21 GaussianBlur": "gauss_sigma21_8uc1",
             "gs16 GaussianBlur": "gauss_sigma16_32f", "a3 filter2D 5x5 4K 32FC1 batch": "filter5_32f", "a3t7 filter2D": "filter7_8uc1", "a3t11 filter2D": "filter11_8uc1", "host-inclusive: GaussianBlur": "host_gauss"}
    for r in rows if isinstance(rows, list) else []:
        c = r.get("config", "")
        key = c.split()[0] if c.split() and c.split()[0] in SUMMARY_KEYS else next((v for k, v in short.items() if c.startswith(k)), None)
        if key is None or "error" in r:
            continue
        fr = r.get("frames", 1) or 1
        ms = r.get("ms", r.get("ms_per_frame"))
        frac = r.get("frac", r.get("frac_of_i8_dense_peak" if key == "cfg5" else "frac_of_bf16_dense_peak"))
        if key == "host_gauss":
            out[key] = [r.get("us_per_frame"), r.get("Mpix_s"), r.get("pcie_GBs_both_ways")]
        elif ms is not None:
            out[key] = [round(ms / fr * 1e3, 2) if "ms" in r else round(ms * 1e3, 2), frac]
            if key.startswith("gauss_sigma") and "cpu_reference_ms_per_frame" in r:      # the long separable kernels: the reference's CPU time per frame beside them, in us
                out[key].append(round(r["cpu_reference_ms_per_frame"] * 1e3, 1))
            if "ms_per_frame_after_the_other_rows" in r:         # cfg5 (clock-bound): timed first and again last
                out[key] += [round(r["ms_per_frame_after_the_other_rows"] * 1e3, 2), r.get("frac_of_i8_dense_peak_after_the_other_rows")]
    return out

MAX_LINE = 4096                # the driver parses the LAST stdout line; r04's 20.5 KB line came back "parsed": null


def emit(res):
    """Full record -> bench_detail.json (beside this script, and gpurun_out/ when it exists) and stderr; stdout gets ONE compact line
    (< MAX_LINE bytes, asserted) holding only the contract keys + roofline + cpu_baseline + the per-config summary."""
    detail = json.dumps(res)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_detail.json"), "w") as f:
                    f.write(detail + "\n")
            except OSError:
                pass
    print(detail, file=sys.stderr, flush=True)
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "per_gpu_mpix_s", "timed_region_s")
    line = {k: res[k] for k in keep if k in res}
    cfg = dict(res.get("config", {}))
    line["config"] = cfg
    rf = res.get("roofline", {})
    line["roofline"] = {k: rf[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms",
                                           "algorithmic_bytes_per_launch", "launches_timed", "measured_copy_GBs") if k in rf}
    cb = res.get("cpu_baseline")
    if cb is not None:
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "one_thread_Mpix_s", "cpu_model", "sample") if k in cb}
        line["cpu_baseline"]["sample"] = str(cb.get("sample_short", cb.get("sample", "")))[:200]
    p = res.get("parity")
    if p is not None:
        line["parity"] = p if len(json.dumps(p)) < 300 else str(p)[:300]
    if "test_mode" in res:
        line["test_mode"] = res["test_mode"][:120]
    if "summary_us_per_frame_and_frac" in res:
        line["summary"] = res["summary_us_per_frame_and_frac"]
    elif isinstance(res.get("other_configs"), list):             # multi-GPU legs: keep name -> value pairs only
        line["summary"] = {str(r.get("config", "?")).split()[0] + "_frames_s": r.get("frames_s", r.get("error")) for r in res["other_configs"][:12]}
    line["detail"] = "bench_detail.json + stderr"
    out = json.dumps(line)
    if len(out) >= MAX_LINE:                                     # never lose the record to an oversize line: shed the optional parts, then assert
        for k in ("summary", "parity", "test_mode"):
            line.pop(k, None)
            out = json.dumps(line)
            if len(out) < MAX_LINE:
                break
    assert len(out) < MAX_LINE, len(out)
    print(out, flush=True)


def pick_batch(dev, requested):
    """4K frames per GPU per step.  The step is one pass of the hot path over one device-resident batch; the batch is sized for the GPU's
    HBM (source + destination = 55 % of the free memory, at most 9216 frames = 153 GB on a 288 GB MI355X) so that a step is ~26 ms, the
    working set is hundreds of times the 256 MB Infinity Cache, and 20 timed steps span > 0.5 s."""
    if requested > 0:
        return requested
    free, _total = torch.cuda.mem_get_info(dev)
    b = int(free * 0.55 / (2 * W4K * H4K)) // 128 * 128
    return max(128, min(9216, b))


def parity_gate(cv, frames, out, B):
    """bit-exact check of the batch result before anything is timed: three whole frames against the plain-C restatement of the reference
    (oracle/smooth.c), sixteen more against the single-frame hook (a different launch geometry of the same arithmetic)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc
    checked = []
    for f in sorted({0, B // 2, B - 1}):
        want = orc.orc_gaussianBlurBinomialU8(frames[f].cpu().numpy(), 5, 4)
        assert np.array_equal(out[f].cpu().numpy(), want), f"parity check failed: frame {f} differs from the oracle"
        checked.append(f)
    rng = np.random.default_rng(1)
    for f in rng.integers(0, B, 16).tolist():
        assert torch.equal(out[f], cv.GaussianBlur(frames[f], 5)), f"batch != single-frame path on frame {f}"
    return {"frames_vs_oracle": checked, "frames_vs_single_frame_hook": 16, "result": "bit-exact"}


DUMP_SAMPLE = 1 << 22          # pixels of the seeded sample over the whole batch (16 MB as float32)


def dump_outputs(d, out):
    """--dump-outputs DIR: what the timed path handed its caller in the last step -- the blurred batch `out` (B x 2160 x 3840 CV_8UC1, B x 8.3 MB:
    too large to write whole) -- as float32: the last frame whole (33 MB, every border) and a fixed sample of DUMP_SAMPLE pixels drawn over the
    whole batch with a seeded generator (the same pixels for the same arguments, so that two builds compare output for output)."""
    os.makedirs(d, exist_ok=True)
    torch.cuda.synchronize()
    np.save(os.path.join(d, "gauss5x5_last_frame.npy"), out[-1].cpu().numpy().astype(np.float32))
    idx = np.sort(np.random.default_rng(809564).integers(0, out.numel(), DUMP_SAMPLE))
    sample = out.reshape(-1)[torch.from_numpy(idx).to(out.device)]
    np.save(os.path.join(d, "gauss5x5_batch_sample.npy"), sample.cpu().numpy().astype(np.float32))


def copy_probe(views, reps=2):
    """the measured-copy denominator: a 16 B / lane device-to-device copy of the same sub-batches, launched and timed the same way"""
    import ctypes
    from opencv_amd import _lib
    from opencv_amd.core import bind_stream, Img
    bind_stream(Img(views[0][0][0]))
    calls = [(ctypes.c_void_p(f.data_ptr()), ctypes.c_void_p(o.data_ptr()), ctypes.c_size_t(f.numel())) for f, o in views]
    assert _lib.lib.mi355cv_copyProbe(calls[0][0], calls[0][1], calls[0][2], 1, 1) == 0      # one 16-byte chunk per lane: the fastest form measured (6.3-6.4 TB/s)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        for sp, dp, nb in calls:
            _lib.lib.mi355cv_copyProbe(sp, dp, nb, 1, 1)
    b.record(); torch.cuda.synchronize()
    return 2.0 * sum(f.numel() for f, _ in views) * reps / (a.elapsed_time(b) * 1e-3) / 1e9


def pmc_child(fpl):
    """the process rocprofv3 --pmc wraps (measure_traffic): two distinct sub-batches of the timed launch geometry through the headline kernel, and a
    16 B / lane copy of one sub-batch whose byte count is known exactly -- the calibration of FETCH_SIZE / WRITE_SIZE on this box"""
    import ctypes
    import opencv_amd as cv
    from opencv_amd import _lib
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda"); g.manual_seed(809564)
    frames = torch.empty((2 * fpl, H4K, W4K), dtype=torch.uint8, device="cuda")
    for lo in range(0, 2 * fpl, 256):
        frames[lo:lo + 256] = torch.randint(0, 256, (min(256, 2 * fpl - lo), H4K, W4K), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty_like(frames)
    cv.set_async(True)
    for rep in range(3):
        for lo in (0, fpl):
            cv.GaussianBlurBatch(frames[lo:lo + fpl], 5, dst=out[lo:lo + fpl])
    for rep in range(2):
        for lo in (0, fpl):
            assert _lib.lib.mi355cv_copyProbe(ctypes.c_void_p(frames[lo].data_ptr()), ctypes.c_void_p(out[lo].data_ptr()), ctypes.c_size_t(fpl * H4K * W4K), 1, 1) == 0
    torch.cuda.synchronize()
    print("PMC_CHILD_KERNEL " + _lib.lib.mi355cv_lastKernel().decode(), flush=True)
    return 0


def measure_traffic(fpl, kernel, timeout_s=240):
    """roofline.traffic, measured in this run: `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` as two separate passes (the two counters do not
    fit the TCC's slots together; nothing else is traced) over `bench.py --pmc-child`.  Both counters are in KiB.  MI355X_MICROARCH.md: on gfx950
    FETCH_SIZE reports half the bytes of a wide coalesced read and WRITE_SIZE is uncalibrated -- so both are calibrated here on a 16 B / lane copy of
    known size run in the same passes, and the calibrated figures are what `traffic` reports (raw values and factors are kept beside them)."""
    import csv
    import glob
    import shutil
    import statistics
    import subprocess
    import tempfile
    info = {"method": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate passes over `bench.py --pmc-child` in this run; KiB -> bytes; "
                      "calibrated on a 16 B/lane copy of known size in the same passes"}
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        info["error"] = "rocprofv3 not found"; return info
    if any(k.startswith(("ROCPROF", "ROCP_", "ROCPROFILER")) for k in os.environ):
        info["error"] = "this run is itself under rocprofv3: nested counter collection skipped"; return info
    copy_bytes = fpl * W4K * H4K
    raw = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="mi355cv_pmc_", dir="/tmp")
        env = dict(os.environ); env["TMPDIR"] = "/tmp"
        cmd = [exe, "--pmc", ctr, "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--pmc-child", "--frames-per-launch", str(fpl)]
        try:
            p = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout_s)
        except subprocess.TimeoutExpired:
            info["error"] = f"{ctr} pass timed out"; shutil.rmtree(d, ignore_errors=True); return info
        child_kernel = [l for l in p.stdout.splitlines() if l.startswith("PMC_CHILD_KERNEL ")]
        vals = {"gauss": [], "copy": []}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f, newline="")):
                if r.get("Counter_Name") != ctr:
                    continue
                if "k_binomial_roll2" in r["Kernel_Name"]:
                    vals["gauss"].append(float(r["Counter_Value"]))
                elif "k_copy16" in r["Kernel_Name"]:
                    vals["copy"].append(float(r["Counter_Value"]))
        shutil.rmtree(d, ignore_errors=True)
        if p.returncode != 0 or not vals["gauss"] or not vals["copy"] or not child_kernel:
            info["error"] = f"{ctr} pass: rc {p.returncode}, {len(vals['gauss'])} kernel rows; tail: {p.stdout[-300:]}"; return info
        if child_kernel[0][len("PMC_CHILD_KERNEL "):].split(" grid=")[0] != kernel.split(" grid=")[0]:
            info["error"] = "the profiled pass launched another kernel instance than the timed region"; return info
        raw[ctr] = (statistics.median(vals["gauss"]) * 1024, statistics.median(vals["copy"]) * 1024, len(vals["gauss"]))
    fcal = copy_bytes / raw["FETCH_SIZE"][1]
    wcal = copy_bytes / raw["WRITE_SIZE"][1]
    fetch, write = raw["FETCH_SIZE"][0] * fcal, raw["WRITE_SIZE"][0] * wcal
    info.update({"frames_per_launch": fpl, "dispatches_sampled": raw["FETCH_SIZE"][2],
                 "fetch_raw_bytes": int(raw["FETCH_SIZE"][0]), "write_raw_bytes": int(raw["WRITE_SIZE"][0]),
                 "fetch_calibration": round(fcal, 4), "write_calibration": round(wcal, 4),
                 "fetch_bytes_per_launch": int(fetch), "write_bytes_per_launch": int(write), "hbm_bytes_per_launch": int(fetch + write),
                 "algorithmic_bytes_per_launch": int(2 * copy_bytes), "traffic_over_algorithmic": round((fetch + write) / (2 * copy_bytes), 4)})
    return info


def multi_gpu_legs(cv, dist, dev, rank, world):
    """BASELINE configs 4 and 5 under N > 1: frames sharded by index, shared parameters broadcast from rank 0 over RCCL, no
    data-path collective.  cfg4: 256 x 1080p frames -> cornerHarris + buildPyramid(4); cfg5: batched matchTemplate, one template."""
    from opencv_amd import shard
    rows = []

    def timed(fn, n, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t[0]) / n

    g = torch.Generator(device=dev); g.manual_seed(809564 + rank)
    lo, hi = shard.frame_range(256, rank, world)
    fr = torch.randint(0, 256, (hi - lo, 1080, 1920), dtype=torch.uint8, device=dev, generator=g)
    resp = torch.empty((hi - lo, 1080, 1920), dtype=torch.float32, device=dev)
    params = shard.broadcast_params(np.array([2, 3, 0.04]), 0, dev)              # blockSize, ksize, k: plan-time broadcast
    bs, ks, kk = int(params[0]), int(params[1]), float(params[2])
    cv.set_async(True)
    s = timed(lambda: (cv.cornerHarrisBatch(fr, bs, ks, kk, dst=resp), cv.buildPyramidBatch(fr, 4)), 10)
    rows.append({"config": f"cfg4 cornerHarris(2,3,0.04) + buildPyramid(4), 256 x 1080p 8UC1 sharded {hi - lo} frames / GPU", "n_gpus": world,
                 "ms_per_pass": round(s * 1e3, 4), "frames_s": round(256 / s, 1)})
    del fr, resp
    B5 = 8
    img = torch.randint(0, 256, (B5, H4K, W4K), dtype=torch.uint8, device=dev, generator=g)
    tpl = torch.randint(0, 256, (128, 128), dtype=torch.uint8, device=dev, generator=g)
    dist.broadcast(tpl, src=0)                                                   # the one shared template (16 KB) over RCCL
    res = torch.empty((B5, H4K - 127, W4K - 127), dtype=torch.float32, device=dev)
    s = timed(lambda: cv.matchTemplateBatch(img, tpl, cv.TM_CCORR_NORMED, result=res), 3, 1)
    rows.append({"config": f"cfg5 matchTemplate TM_CCORR_NORMED 4K x 128x128 8UC1, {B5} frames / GPU, template broadcast", "n_gpus": world,
                 "ms_per_pass": round(s * 1e3, 3), "frames_s": round(world * B5 / s, 2)})
    cv.set_async(False)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("MI355CV_BENCH_BATCH", "0")),
                    help="4K frames per GPU per step; 0 = sized for the GPU's HBM (see pick_batch)")
    ap.add_argument("--frames-per-launch", type=int, default=int(os.environ.get("MI355CV_BENCH_FPL", "512")),
                    help="a step (one pass over the resident batch) is issued as consecutive launches over sub-batches of this many frames")
    ap.add_argument("--full", action="store_true",
                    help="also the parity gate, the measured copy rate, roofline.traffic, cpu_baseline, BASELINE configs 2-5, the host-inclusive rows "
                         "and (N > 1) the cfg4 / cfg5 legs; a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float32; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline and the CPU times beside other_configs")
    ap.add_argument("--no-pmc", action="store_true", help="with --full: skip the in-run rocprofv3 --pmc passes that measure roofline.traffic")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-other-configs", action="store_true", help="with --full: skip BASELINE configs 2-5 (reported under other_configs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # test hook, never a reportable number: MI355CV_BENCH_SHARED_GPU=1 lets the N ranks share GPU 0 over gloo, so that the N > 1 code path
    # (spawn, sharding, broadcasts, max-over-ranks timing, the cfg4 / cfg5 legs) can be exercised on a one-GPU box; the line says so
    shared = os.environ.get("MI355CV_BENCH_SHARED_GPU") == "1"
    if args.pmc_child:
        return pmc_child(args.frames_per_launch)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        from opencv_amd import shard                       # no launcher: become the launcher (N ranks, one per GPU, RCCL); loud when < N GPUs
        sys.exit(shard.spawn_ranks(args.gpus, __file__, sys.argv[1:], need_gpus=not shared))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)")
    if shared:
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        sys.exit(f"bench.py: rank {rank} has no GPU (local_rank {local_rank}, {torch.cuda.device_count()} visible)")
    dist = None
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if shared:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        assert dist.get_world_size() == args.gpus

    import opencv_amd as cv
    from opencv_amd import _lib

    # plan time: rank 0 owns the launch plan -- filter size, border rule, frames per launch -- and broadcasts it (RCCL over xGMI, a few bytes,
    # once); every rank runs what it RECEIVED, so a rank that missed the broadcast would launch a different (and refused: ksize 0) filter
    plan = torch.tensor([5, cv.BORDER_REFLECT_101, args.frames_per_launch] if rank == 0 else [0, 0, 0], dtype=torch.int32, device=dev)
    if dist is not None:
        dist.broadcast(plan, src=0)
    KS, BORDER, FPL_PLAN = (int(v) for v in plan.cpu().tolist())

    B = pick_batch(dev, args.batch)
    if dist is not None:                                    # every rank runs the same per-GPU batch (weak scaling)
        tb = torch.tensor([B], dtype=torch.int64, device=dev)
        dist.all_reduce(tb, op=dist.ReduceOp.MIN)
        B = int(tb[0])
    # A step = ONE pass of the hot path over the whole resident batch, issued as B / FPL consecutive launches over sub-batches of FPL frames:
    # the same 9216 frames ran 4-6 % slower as a single 1.66 M-workgroup launch than as 18 launches of 512 frames (tools/split_probe.py,
    # profiles/r02_split_probe.txt) -- the library's batch entry splits a large batch the same way on its own; here the sub-batches are
    # explicit so that every kernel launch gets its own pair of events.
    FPL = max(1, min(FPL_PLAN, B))
    B = B // FPL * FPL
    g = torch.Generator(device=dev)
    g.manual_seed(809564 + rank)
    frames = torch.empty((B, H4K, W4K), dtype=torch.uint8, device=dev)
    for lo in range(0, B, 256):                             # filled in slabs: the generator's scratch stays small next to a 76 GB batch
        frames[lo:lo + 256] = torch.randint(0, 256, (min(256, B - lo), H4K, W4K), dtype=torch.uint8, device=dev, generator=g)
    out = torch.empty_like(frames)

    # parity gate before timing (rank 0: against the CPU checker; every rank: the call must succeed)
    cv.GaussianBlurBatch(frames, KS, BORDER, dst=out)
    torch.cuda.synchronize()
    kernel = _lib.lib.mi355cv_lastKernel().decode()
    parity = parity_gate(cv, frames, out, B) if rank == 0 and args.full else None

    views = [(frames[lo:lo + FPL], out[lo:lo + FPL]) for lo in range(0, B, FPL)]
    nl = len(views)
    cv.set_async(True)
    cv.GaussianBlurBatch(views[0][0], KS, BORDER, dst=views[0][1])
    kernel = _lib.lib.mi355cv_lastKernel().decode()        # the instance and geometry of the timed launches
    for _ in range(args.warmup):
        for f, o in views:
            cv.GaussianBlurBatch(f, KS, BORDER, dst=o)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps * nl + 1)]
    t0 = time.perf_counter()
    k = 0
    for s in range(args.steps):
        for f, o in views:
            ev[k].record(); k += 1             # launches are bound to torch's current stream (core.bind_stream)
            cv.GaussianBlurBatch(f, KS, BORDER, dst=o)
    ev[k].record()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    cv.set_async(False)
    per_launch = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps * nl)])      # launch to launch: gaps included
    per_step = per_launch.reshape(args.steps, nl).sum(axis=1)
    kern_ms = float(per_launch.mean())
    if dist is not None:
        t = torch.tensor([elapsed, kern_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, kern_ms = float(t[0]), float(t[1])
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, out)            # before copy_probe, which overwrites `out`
    copy_gbs = copy_probe(views) if rank == 0 and args.full else None

    legs = None
    if world > 1 and args.full and not args.no_other_configs:
        del frames, out, views
        torch.cuda.empty_cache()
        try:
            legs = multi_gpu_legs(cv, dist, dev, rank, world)
        except Exception as e:
            legs = [{"config": "multi-GPU legs", "error": repr(e)}]

    if rank == 0:
        pix_per_step = B * W4K * H4K
        value = world * pix_per_step * args.steps / elapsed / 1e6
        algo = ALGO_BYTES_PER_PIXEL * FPL * W4K * H4K        # per kernel launch
        achieved = algo / (kern_ms * 1e-3) / 1e9
        q = max(1, args.steps // 4)
        # HBM bytes per launch from the PMC counters, measured in THIS run on THIS box (measure_traffic below)
        traffic_info = None
        if world == 1 and args.full and not args.no_pmc:
            del frames, out, views
            frames = out = views = None
            torch.cuda.empty_cache()
            traffic_info = measure_traffic(FPL, kernel)
        traffic = traffic_info.get("hbm_bytes_per_launch") if traffic_info else None
        res = {
            "metric": "Mpix/s per GPU (4K CV_8U Gaussian5x5) + achieved HBM GB/s vs roofline, 1/2/4/8 GPUs",
            "value": round(value, 1), "unit": "Mpix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": "cv::GaussianBlur 5x5 sigma=0 BORDER_REFLECT_101 on 3840x2160 CV_8UC1, "
                                   f"{B} device-resident frames per GPU per step ({2 * B * W4K * H4K / 1e9:.1f} GB of HBM: one pass = {nl} launches of {FPL} frames)",
                       "frames_per_gpu": B, "frames_per_launch": FPL, "launches_per_step": nl, "sharding": f"frames x{world}, no data-path collective", "ranks": world,
                       "collective": ("gloo (test mode)" if shared else "RCCL") + " broadcast of the launch plan (ksize, border, frames per launch) from rank 0 at plan time" if world > 1 else "none (1 GPU)"},
            "per_gpu_mpix_s": round(value / world, 1),
            "timed_region_s": round(elapsed, 4),
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_detail": traffic_info,
                         "kernel": kernel, "avg_launch_ms": round(kern_ms, 4),
                         "algorithmic_bytes_per_launch": int(algo),
                         "launches_timed": int(per_launch.size),
                         "launch_ms": {"median": round(float(np.median(per_launch)), 4), "p10": round(float(np.percentile(per_launch, 10)), 4),
                                       "p90": round(float(np.percentile(per_launch, 90)), 4), "min": round(float(per_launch.min()), 4),
                                       "max": round(float(per_launch.max()), 4)},
                         "step_ms": {"median": round(float(np.median(per_step)), 4), "min": round(float(per_step.min()), 4), "max": round(float(per_step.max()), 4),
                                     "first_quarter_mean": round(float(per_step[:q].mean()), 4),
                                     "rest_mean": round(float(per_step[q:].mean()), 4) if args.steps > q else None}},
        }
        if copy_gbs is not None:
            res["roofline"].update({"measured_copy_GBs": round(copy_gbs, 1), "frac_of_measured_copy": round(achieved / copy_gbs, 4)})
        if parity is not None:
            res["parity"] = parity
        if shared:
            res["test_mode"] = f"{world} ranks SHARE ONE GPU over gloo (MI355CV_BENCH_SHARED_GPU=1): a code-path test, not a measurement"
        if legs is not None:
            res["other_configs"] = legs
        if world == 1 and args.full and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline()
        if world == 1 and args.full and not args.no_other_configs:
            frames = out = views = None
            torch.cuda.empty_cache()
            try:
                res["other_configs"] = other_configs(with_cpu=not args.no_cpu_baseline)
            except Exception as e:                           # never let the secondary numbers take the headline down
                res["other_configs"] = {"error": repr(e)}
            try:
                hrows = host_inclusive()
            except Exception as e:
                hrows = [{"config": "host-inclusive rows", "error": repr(e)[:300]}]
            if isinstance(res["other_configs"], list):
                res["other_configs"] += hrows
            else:
                res["host_inclusive"] = hrows
            # last key of the line: [us per frame, fraction of the bounding roofline] per BASELINE config / weak row; host_gauss = [us per frame, Mpix/s, PCIe GB/s]
            res["summary_us_per_frame_and_frac"] = compact_summary(res["other_configs"] if isinstance(res["other_configs"], list) else hrows)
            res["summary_us_per_frame_and_frac"]["headline"] = [round(elapsed / args.steps / B * 1e6, 3), round(achieved / HBM_PEAK_GBS, 4)]
        emit(res)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
