"""Every batch entry where it cuts a long batch, and past 65535 frames.

A batch entry cuts a long batch somewhere: at a grid dimension (65535), at a scratch budget, at a tuned launch length, at the 16-frame chunks of the host pipeline.
The other suites run batches of 3 .. 70 frames, which stay inside one launch / group / chunk; what happens BETWEEN two of them -- the first-frame offsets of the
pointers, the scratch slab the next group reuses, the counters of a chunk, the idle waves behind a partial launch -- is checked here.  Every case asserts from
mi355cv_lastKernel that its cut was crossed (batchcuts.cut_of), so a case that stays inside one group fails instead of passing silently, and compares bit for bit
against the restatement / oracle of the operation.  The long batches are `periodic` (251 distinct frames repeated) or `all4x4` (every binary 4 x 4 image), see
tests/batchcuts.py; their references are held against the per-image restatements in tests/test_batch_cuts_cpu.py.

The last test sweeps the remaining batch entries at 65537 frames.  A grid dimension holds 65535, so such a batch is either served -- every frame equals its oracle
frame -- or declined with a reason that names the bound and the destination left alone (include/mi355cv.h, "Frame counts").  A failed launch or a destination
that was silently not written is neither."""
import functools
import os

import numpy as np
import pytest
import torch

import batchcuts as B
import ccl_restate as C
import clahe_restate as CL
import demosaic_restate as DM
import disttransform_restate as D
import hough_restate as H
import mog2_restate as M
import pyrup_restate as PU
import viewcheck as V

pytestmark = pytest.mark.gpu

N_BIG = 65541                                  # 65535 + 6: the second launch / group holds a few frames, and 65536 (the 4 x 4 images start again) lies inside it
N_SWEEP = 65537
FILL = 0xA5                                    # what a destination holds before the call


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    return opencv_amd


def dev(a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:                  # (a shared reference array: torch wants a writable one to wrap)
        a = a.copy()
    if a.dtype == np.uint16:                   # moved as int16 bits, viewed back
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def host(t):
    if isinstance(t, np.ndarray):
        return t
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def pinned(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).pin_memory().view(torch.uint16)
    return torch.from_numpy(a).pin_memory()


def prefilled(shape, dtype):
    """a device tensor whose every byte is FILL"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(FILL)
    return t


def untouched(t):
    return bool((t.view(torch.uint8) == FILL).all())


def note(cv):
    return cv._lib.lib.mi355cv_lastKernel().decode()


def crossed(cv, nframes):
    """the kernel note of the call just made, which must prove more than one launch / group"""
    k = note(cv)
    ok, text = B.cut_of(k, nframes)
    assert ok, "the batch of %d frames stayed inside one launch / group: %s" % (nframes, k)
    return k


def first_wrong(got, want):
    bad = (got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1)
    return int(np.flatnonzero(bad)[0]) if bad.any() else None


# ---------------------------------------------------------------------------------------------------------------- the Gaussian's launch split (smooth.hip launchRoll2)
# gauss_seg = 5: (W, H, cn) -> work items per frame = strips of 64 chunks x segments of 5 rows
GAUSS = [(64, 33, 1, 7), (1040, 33, 1, 14), (1040, 83, 1, 34), (64, 33, 3, 7)]          # one strip / a second strip with one lane / 17 segments: the XCD regrouping / 3 channels


@pytest.mark.parametrize("w,h,cn,per_frame", GAUSS)
def test_gaussian_launch_split(cv, orc, w, h, cn, per_frame):
    """gauss_launch_waves cuts a batch into launches of ceil(waves / per_frame) frames: 5 frames as 1+1+1+1+1, 2+2+1, 3+2 and one launch; the last launch is partial
    and (per_frame * nf + 3) / 4 workgroups leave idle waves behind the kernel's frame guard.  This is the path of the benchmark (18 launches of 512 frames)."""
    L = cv._lib.lib
    default_waves = int(os.environ.get("MI355CV_GAUSS_LAUNCH_WAVES", "393216"))
    rng = np.random.default_rng(w * 100 + h + cn)
    a = rng.integers(0, 256, (5, h, w, cn) if cn > 1 else (5, h, w), dtype=np.uint8)
    d = dev(a)
    out = torch.empty_like(d)
    try:
        assert L.mi355cv_setParam(b"gauss_seg", 5) == 0
        for ksize in (3, 5):
            for border in (0, 1, 2, 4):
                want = np.stack([orc.orc_gaussianBlurBinomialU8(f, ksize, border) for f in a])
                for variant in (6, 3):
                    assert L.mi355cv_setParam(b"gauss_variant", variant) == 0
                    for waves, launches, chunk in [(per_frame, 5, 1), (per_frame + 1, 3, 2), (2 * per_frame + 1, 2, 3), (0, 1, 5)]:
                        assert L.mi355cv_setParam(b"gauss_launch_waves", waves) == 0
                        out.fill_(FILL)
                        cv.GaussianBlurBatch(d, ksize, border, dst=out)
                        k = note(cv)
                        what = (ksize, border, variant, waves, k)
                        assert k.startswith("k_binomial_roll2<%d,%d," % (ksize, cn)) and " seg=5 rows" in k, what
                        assert "%d launch(es) of <= %d frames" % (launches, chunk) in k and B.cut_of(k, 5)[0] == (launches > 1), what
                        got = host(out)
                        assert np.array_equal(got, want), what + (first_wrong(got, want),)
    finally:
        L.mi355cv_setParam(b"gauss_seg", 0)
        L.mi355cv_setParam(b"gauss_variant", 0)
        L.mi355cv_setParam(b"gauss_launch_waves", default_waves)


# ---------------------------------------------------------------------------------------------------------------- every binary 4 x 4 image: CCL and distanceTransform
@functools.lru_cache(maxsize=None)
def frames4x4():
    f = B.all4x4(N_BIG)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def dev4x4():
    return dev(frames4x4())


@pytest.mark.parametrize("connectivity,ccltype,order", [(4, C.CCL_DEFAULT, C.PIXEL), (8, C.CCL_WU, C.PIXEL), (8, C.CCL_DEFAULT, C.BLOCK)])
def test_ccl_groups(cv, connectivity, ccltype, order):
    """ccl.hip runCCL: groups of min(nframes, 65535, 256 MiB / scratch per frame); the scratch P / B / K is cleared again per group, the counts land at hostN + f0"""
    assert C.order_of(connectivity, ccltype) == order
    want_n, want = B.label4x4(frames4x4(), connectivity, order)
    n0 = cv.call_count("connectedComponentsBatch")
    counts, labels = cv.connectedComponentsBatch(dev4x4(), connectivity=connectivity, ltype=cv.CV_32S, ccltype=ccltype)
    k = crossed(cv, N_BIG)
    assert cv.call_count("connectedComponentsBatch") == n0 + 1 and k.startswith("k_ccl_strip<%s,%d," % (order, connectivity)), k
    counts, labels = np.asarray(counts, np.int32), host(labels)
    assert labels.dtype == np.int32 and np.array_equal(counts, want_n), (k, first_wrong(counts[:, None], want_n[:, None]))
    assert np.array_equal(labels, want), (k, first_wrong(labels, want))


def test_ccl_16u_and_stats_decline_past_65535_frames(cv):
    """CV_16U labels are written after every frame is counted, so they are one group: past 65535 frames the call is declined with the bound in the reason and the
    label buffer left alone; the statistics of such a batch are declined the same way"""
    lab = prefilled((N_BIG, 4, 4), torch.int16).view(torch.uint16)
    with pytest.raises(NotImplementedError, match="65535"):
        cv.connectedComponentsBatch(dev4x4(), labels=lab, ltype=cv.CV_16U)
    assert untouched(lab)
    with pytest.raises(NotImplementedError, match="65535"):
        cv.connectedComponentsWithStatsBatch(dev4x4())
    # ... and one frame fewer than the bound allows is served (the bound is the reason, not the size of the batch)
    counts, lab = cv.connectedComponentsBatch(dev4x4()[:65535], ltype=cv.CV_16U)
    want_n, want = B.label4x4(frames4x4()[:65535], 8, C.BLOCK)
    assert np.array_equal(np.asarray(counts, np.int32), want_n) and np.array_equal(host(lab), want.astype(np.uint16))


@pytest.mark.parametrize("metric,dtype", [(D.DIST_L2, np.float32), (D.DIST_L1, np.float32), (D.DIST_C, np.float32), (D.DIST_L1, np.uint8)])
def test_distance_transform_groups(cv, metric, dtype):
    """disttransform.hip launchDist: groups of min(nframes, 65535, 128 MiB / scratch per frame).  Frame 65535, exactly on the cut, is the all-ones image, which has
    no site: it gets the library's no-site value and its neighbours 65534 and 65536 are what they are on their own"""
    want = B.dist4x4(frames4x4(), metric, dtype)
    n0 = cv.call_count("distanceTransformBatch")
    got = cv.distanceTransformBatch(dev4x4(), metric, cv.DIST_MASK_PRECISE, dstType=cv.CV_8U if dtype == np.uint8 else cv.CV_32F)
    k = crossed(cv, N_BIG)
    assert cv.call_count("distanceTransformBatch") == n0 + 1 and k.startswith("k_dist_row<"), k
    got = host(got)
    assert got.dtype == dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (k, first_wrong(got.view(np.uint8), want.view(np.uint8)))
    none = D.NO_SITE_8U if dtype == np.uint8 else D.NO_SITE_32F
    assert (got[65535] == none).all() and (got[65536] == 0).all() and np.array_equal(got[65534], want[65534]) and got[65534].max() < none


# ---------------------------------------------------------------------------------------------------------------- CLAHE: groups by scratch (clahe.hip claheFrames)
def clahe_group(dtype, w, h, tiles, n):
    """G of claheFrames for frames whose size the grid divides: min(nframes, 256 MiB / (histogram slab + LUTs of a frame), 65535) with one slice per tile"""
    hist, e = (65536, 2) if dtype == np.uint16 else (256, 1)
    nT = tiles[0] * tiles[1]
    slab = nT * hist * (2 if dtype == np.uint16 else 4)
    return max(1, min(n, (256 << 20) // (slab + nT * hist * e), 65535))


# CV_16U on the default 8 x 8 grid: 16 MiB a frame, G = 16.  CV_8U needs many tiles to reach the budget with few frames: 64 x 64 tiles of 2 x 2 pixels are 5 MiB a
# frame, G = 51 (the restatement costs as much per tile as the library's scratch does, so fewer frames of more tiles are no cheaper to check)
@pytest.mark.parametrize("dtype,w,h,tiles,n", [(np.uint16, 48, 64, (8, 8), 19), (np.uint8, 128, 128, (64, 64), 54)])
def test_clahe_groups(cv, dtype, w, h, tiles, n):
    G = clahe_group(dtype, w, h, tiles, n)
    assert 1 < G < n and n % G not in (0, 1), G                    # a partial last group of several frames
    rng = np.random.default_rng(n)
    frames = rng.integers(0, 65536 if dtype == np.uint16 else 256, (n, h, w)).astype(dtype)          # all distinct
    want = np.stack([CL.clahe(f, 2.0, tiles) for f in frames])
    n0 = cv.call_count("claheBatch")
    got = cv.createCLAHE(2.0, tiles).applyBatch(dev(frames))
    k = crossed(cv, n)
    assert cv.call_count("claheBatch") == n0 + 1 and "k_clahe_interp" in k and "frames=%d/launch" % G in k, k
    got = host(got)
    assert np.array_equal(got, want), (k, first_wrong(got, want))


# ---------------------------------------------------------------------------------------------------------------- Hough: groups by scratch (hough.hip runHough)
def hough_group(w, h, rho, theta, n):
    pad = lambda b: (b + 255) & ~255                                                            # noqa: E731
    numangle, numrho = H.geometry(w, h, rho, theta)
    cells, cap = (numangle + 2) * (numrho + 2), numangle * ((numrho + 1) // 2)
    return numrho, min(n, max(1, (1 << 30) // (pad(w * h * 4) + pad(cells * 4) + 2 * pad(cap * 8))))


@pytest.mark.parametrize("side,rho,theta", [("lds", 0.016, H.PI / 720), ("hbm", 0.01, H.PI / 450)])
def test_hough_groups(cv, side, rho, theta):
    """an accumulator of more than 1 GiB / 8 / 12 cells leaves room for 7 frames in the scratch: 9 frames are a group of 7 and one of 2, the counters of the second
    at ctr + 2 * 7.  The frames differ in their number of edge points, so a counter read at the wrong frame changes the votes.  One geometry whose rows of bins are
    voted in LDS, one whose rows are voted in HBM."""
    n, thr, cap = 9, 10, 512
    numrho, G = hough_group(64, 64, rho, theta, n)
    assert 1 < G < n and (numrho + 2 <= H.LDS_BINS) == (side == "lds"), (numrho, G)
    frames = np.stack([H.drawn_lines(64, 64) for _ in range(n)])
    for i in range(n):
        frames[i, 64 - 5 * i:] = 0
    assert len({int((f != 0).sum()) for f in frames}) == n
    want = [H.hough(f, rho, theta, thr)[1] for f in frames]
    n0 = cv.call_count("houghLinesBatch")
    counts, lines = cv.HoughLinesBatch(dev(frames), rho, theta, thr, maxLines=cap)
    k = crossed(cv, n)
    assert cv.call_count("houghLinesBatch") == n0 + 1 and k.startswith("k_hough_vote<%s>" % side) and "in groups of %d" % G in k, k
    lines = host(lines)
    assert len({len(w_) for w_ in want}) > 1 and all(0 < len(w_) <= cap for w_ in want)
    for i in range(n):
        assert counts[i] == len(want[i]) and H.same_bits(lines[i, :counts[i]], want[i][:, :2]), (i, counts[i], len(want[i]), k)


# ---------------------------------------------------------------------------------------------------------------- demosaic and pyrUp: f0 += 65535, y0 += 4 * 65535
def base_frames(dtype, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536 if dtype == np.uint16 else 256, (B.P, h, w)).astype(dtype)


def check_periodic(got, want_P, k):
    ok, frame = B.same_periodic(host(got), want_P)
    assert ok, ("first wrong frame", frame, k)


# the per-pixel kernels take the frame from blockIdx.z and cut at 65535 ("2 launch(es)"); the rolling kernels have a 1-D grid and no cut: they must still find frame
# 65535 and beyond (a work-item index that is divided back into strip, segment and frame), and their note says how many frames the one launch had
@pytest.mark.parametrize("dtype,w,h,kernel,proof", [(np.uint8, 5, 3, "k_demosaic<depth 0,3>", "2 launch(es)"), (np.uint16, 16, 3, "k_demosaic<depth 2,3>", "2 launch(es)"),
                                                    (np.uint8, 16, 4, "k_demosaic_roll<3,", "%d frame(s)" % N_BIG)])
def test_demosaic_past_65535_frames(cv, dtype, w, h, kernel, proof):
    base = base_frames(dtype, h, w, 46)
    want = np.stack([DM.demosaic(f, "BG", 3) for f in base])
    got = cv.demosaicingBatch(dev(B.periodic(base, N_BIG)), cv.COLOR_BayerBG2BGR)
    k = note(cv)
    assert k.startswith(kernel) and proof in k and (B.cut_of(k, N_BIG)[0] or "roll" in kernel), k
    check_periodic(got, want, k)


@pytest.mark.parametrize("dtype,w,h,kernel,proof", [(np.uint8, 5, 2, "k_pyrup<depth 0>", "2 launch(es)"), (np.uint16, 16, 2, "k_pyrup<depth 2>", "2 launch(es)"),
                                                    (np.uint8, 8, 2, "k_pyrup_roll<4>", "%d frame(s)" % N_BIG)])
def test_pyrup_past_65535_frames(cv, dtype, w, h, kernel, proof):
    base = base_frames(dtype, h, w, 47)
    want = np.stack([PU.pyrUp(f) for f in base])
    got = cv.pyrUpBatch(dev(B.periodic(base, N_BIG)))
    k = note(cv)
    assert k.startswith(kernel) and proof in k and (B.cut_of(k, N_BIG)[0] or "roll" in kernel), k
    check_periodic(got, want, k)


@pytest.mark.parametrize("dtype,w,h", [(np.uint8, 3, 262147), (np.int16, 1, 262141)])
def test_pyrup_taller_than_one_launch(cv, dtype, w, h):
    """grid.y holds 65535 workgroups of 4 source rows: a taller image takes a second launch that starts at source row 262140"""
    rng = np.random.default_rng(h)
    src = rng.integers(-32768 if dtype == np.int16 else 0, 32768 if dtype == np.int16 else 256, (h, w)).astype(dtype)
    got = cv.pyrUp(dev(src))
    k = crossed(cv, 1)
    assert k.startswith("k_pyrup<depth %d>" % (3 if dtype == np.int16 else 0)) and "2 launch(es)" in k, k
    got, want = host(got), PU.pyrUp(src)
    assert got.dtype == want.dtype and np.array_equal(got, want), (k, first_wrong(got, want))


# ---------------------------------------------------------------------------------------------------------------- the host pipeline: three chunks (runtime.hip hostBatchPipeline)
N_HOST = 37                                    # 16 + 16 + 5: the third chunk reuses buffer set 0, the last one is partial


def staged(cv):
    return cv._lib.lib.mi355cv_stagedBytes()


def host_case(cv, frames, call, want):
    src = pinned(frames)
    s0 = staged(cv)
    got = call(src)
    moved = staged(cv) - s0
    out = got[-1] if isinstance(got, tuple) else got
    assert not out.is_cuda and moved == src.numel() * src.element_size() + out.numel() * out.element_size(), moved      # every byte crossed PCIe once each way
    g = host(out)
    assert g.dtype == want.dtype and np.array_equal(g.view(np.uint8), want.view(np.uint8)), first_wrong(g.view(np.uint8), want.view(np.uint8))
    return got


def test_host_pipeline_demosaic_pyrup_clahe_distance(cv):
    """37 small distinct frames in page-locked memory through the entries whose host batches the other suites run as one chunk"""
    rng = np.random.default_rng(37)
    f = rng.integers(0, 256, (N_HOST, 6, 16), dtype=np.uint8)
    host_case(cv, f, lambda s: cv.demosaicingBatch(s, cv.COLOR_BayerBG2BGR), np.stack([DM.demosaic(x, "BG", 3) for x in f]))
    f16 = rng.integers(0, 65536, (N_HOST, 5, 7)).astype(np.uint16)
    host_case(cv, f16, lambda s: cv.demosaicingBatch(s, cv.COLOR_BayerBG2BGR), np.stack([DM.demosaic(x, "BG", 3) for x in f16]))
    f = rng.integers(0, 256, (N_HOST, 4, 8), dtype=np.uint8)
    host_case(cv, f, cv.pyrUpBatch, np.stack([PU.pyrUp(x) for x in f]))
    f = rng.integers(0, 256, (N_HOST, 16, 24), dtype=np.uint8)
    host_case(cv, f, cv.createCLAHE(2.0, (3, 2)).applyBatch, np.stack([CL.clahe(x, 2.0, (3, 2)) for x in f]))
    f = (rng.random((N_HOST, 8, 12)) < 0.8).astype(np.uint8) * 255
    host_case(cv, f, lambda s: cv.distanceTransformBatch(s, cv.DIST_L2, cv.DIST_MASK_PRECISE), np.stack([D.distanceTransform(x, D.DIST_L2) for x in f]))


def test_host_pipeline_ccl_counts_follow_the_chunks(cv):
    """the component count differs from frame to frame and the chunks write theirs at nlabels + done"""
    rng = np.random.default_rng(38)
    f = np.stack([C.random_frame(rng, 8, 12, 0.1 + 0.02 * i) for i in range(N_HOST)])
    ref = [C.label(x, 8, C.BLOCK) for x in f]
    want_n = [r[0] for r in ref]
    assert len(set(want_n[:16])) > 3 and len(set(want_n[16:32])) > 3 and want_n[:5] != want_n[32:]
    counts, _ = host_case(cv, f, cv.connectedComponentsBatch, np.stack([r[1] for r in ref]))
    assert list(counts) == want_n


def test_host_pipeline_mog2_model_follows_the_chunks(cv):
    """37 frames of a camera through MOG2's applyBatch from page-locked memory: the model stays in HBM from chunk to chunk, and the masks and the final model are
    the restatement's"""
    frames, _ = M.sequence(5, 12, 1, np.uint8, seed=39, nframes=N_HOST)
    ref = M.Mog2("vec", history=8)
    want = np.stack(ref.applyBatch(frames, 0.1))
    m = cv.createBackgroundSubtractorMOG2(8, 16, True)
    host_case(cv, np.stack(frames), lambda s: m.applyBatch(s, learningRate=0.1), want)
    for name, g, w_ in zip(("modesUsed", "gmm", "mean"), m.getModel(), ref.export()):
        V.check_result("model " + name, host(g), w_)
    V.check_result("background", host(m.getBackgroundImage()), ref.getBackgroundImage())


# ---------------------------------------------------------------------------------------------------------------- 65537 frames through the remaining batch entries
_K3 = [0.25, 0.5, 0.25]
_SHARPEN = np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], np.float32)
_P = np.array([[1.05, 0.04, -1.0], [0.03, 0.95, 0.5], [1e-3, -1e-3, 1.0]])


def _affine(cv):
    return cv.getRotationMatrix2D((8.0, 2.0), 9.0, 0.9)


def _templ():
    return dev(np.random.default_rng(3).integers(0, 256, (2, 5), dtype=np.uint8))


def _gauss_q(orc, a, sigma):
    k = [int(v) for v in orc.orc_getGaussianKernelQ(5, sigma)]
    return orc.orc_sepSmoothFixedU8(a, k, k, 4)


# name -> (channels, (w, h), the single-image answer(s) for one frame: f(cv, orc, device frame, numpy frame) -> tensor / array or a tuple of them,
#          the batch call f(cv, frames, tuple of destinations))
SWEEP = {
    "thresholdBatch": (1, (16, 4), lambda cv, o, x, a: cv.threshold(x, 100.7, 200, 0)[1], lambda cv, f, d: cv.thresholdBatch(f, 100.7, 200, 0, dst=d[0])),
    "cvtColorBatch BGR2GRAY": (3, (16, 4), lambda cv, o, x, a: cv.cvtColor(x, cv.COLOR_BGR2GRAY), lambda cv, f, d: cv.cvtColorBatch(f, cv.COLOR_BGR2GRAY, dst=d[0])),
    "resizeBatch nearest": (1, (16, 4), lambda cv, o, x, a: cv.resize(x, (8, 2), interpolation=0), lambda cv, f, d: cv.resizeBatch(f, (8, 2), interpolation=0, dst=d[0])),
    "resizeBatch linear": (1, (16, 4), lambda cv, o, x, a: cv.resize(x, (11, 3), interpolation=1), lambda cv, f, d: cv.resizeBatch(f, (11, 3), interpolation=1, dst=d[0])),
    "resizeBatch area 2x2": (1, (16, 4), lambda cv, o, x, a: cv.resize(x, (8, 2), interpolation=3), lambda cv, f, d: cv.resizeBatch(f, (8, 2), interpolation=3, dst=d[0])),
    "warpAffineBatch": (1, (16, 4), lambda cv, o, x, a: cv.warpAffine(x, _affine(cv), (16, 4), 1, 0, 7.0),
                        lambda cv, f, d: cv.warpAffineBatch(f, _affine(cv), (16, 4), 1, 0, 7.0, dst=d[0])),
    "warpPerspectiveBatch": (1, (16, 4), lambda cv, o, x, a: cv.warpPerspective(x, _P, (16, 4), 1 | cv.WARP_INVERSE_MAP, 0, 3.0),
                             lambda cv, f, d: cv.warpPerspectiveBatch(f, _P, (16, 4), 1 | cv.WARP_INVERSE_MAP, 0, 3.0, dst=d[0])),
    "pyrDownBatch": (1, (16, 4), lambda cv, o, x, a: cv.pyrDown(x), lambda cv, f, d: cv.pyrDownBatch(f, dst=d[0])),
    "buildPyramidBatch maxlevel 2": (1, (16, 4), lambda cv, o, x, a: tuple(cv.buildPyramid(x, 2)[1:]), lambda cv, f, d: cv.buildPyramidBatch(f, 2, dst=[f] + list(d))),
    "buildPyramidBatch maxlevel 4": (1, (16, 16), lambda cv, o, x, a: tuple(cv.buildPyramid(x, 4)[1:]), lambda cv, f, d: cv.buildPyramidBatch(f, 4, dst=[f] + list(d))),
    "cornerHarrisBatch": (1, (16, 4), lambda cv, o, x, a: cv.cornerHarris(x, 2, 3, 0.04), lambda cv, f, d: cv.cornerHarrisBatch(f, 2, 3, 0.04, dst=d[0])),
    "integralBatch": (1, (16, 4), lambda cv, o, x, a: cv.integral(x, sqsum=True), lambda cv, f, d: cv.integralBatch(f, sqsum=True, dst=(d[0], d[1]))),
    "SobelBatch": (1, (16, 4), lambda cv, o, x, a: cv.Sobel(x, cv.CV_16S, 1, 0, 3), lambda cv, f, d: cv.SobelBatch(f, cv.CV_16S, 1, 0, 3, dst=d[0])),
    "boxFilterBatch": (1, (16, 4), lambda cv, o, x, a: cv.boxFilter(x, -1, (3, 3)), lambda cv, f, d: cv.boxFilterBatch(f, -1, (3, 3), dst=d[0])),
    "sepFilter2DBatch": (1, (16, 4), lambda cv, o, x, a: cv.sepFilter2D(x, cv.CV_32F, _K3, _K3, delta=0.5),
                         lambda cv, f, d: cv.sepFilter2DBatch(f, cv.CV_32F, _K3, _K3, delta=0.5, dst=d[0])),
    "filter2DBatch": (1, (16, 4), lambda cv, o, x, a: cv.filter2D(x, -1, _SHARPEN), lambda cv, f, d: cv.filter2DBatch(f, -1, _SHARPEN, dst=d[0])),
    "cvtColorFilter2DBatch": (3, (16, 4), lambda cv, o, x, a: cv.filter2D(cv.cvtColor(x, cv.COLOR_BGR2GRAY), -1, _SHARPEN),
                              lambda cv, f, d: cv.cvtColorFilter2DBatch(f, cv.COLOR_BGR2GRAY, _SHARPEN, dst=d[0])),
    "matchTemplateBatch": (1, (16, 4), lambda cv, o, x, a: cv.matchTemplate(x, _templ(), cv.TM_CCORR_NORMED),
                           lambda cv, f, d: cv.matchTemplateBatch(f, _templ(), cv.TM_CCORR_NORMED, result=d[0])),
    "GaussianBlurBatch BORDER_WRAP": (1, (16, 4), lambda cv, o, x, a: o.orc_gaussianBlurBinomialU8(a, 5, 3), lambda cv, f, d: cv.GaussianBlurBatch(f, 5, cv.BORDER_WRAP, dst=d[0])),
    "GaussianBlurBatch sigma 1.3": (1, (16, 4), lambda cv, o, x, a: _gauss_q(o, a, 1.3), lambda cv, f, d: cv.GaussianBlurBatch(f, 5, dst=d[0], sigmaX=1.3)),
}
# What each entry does with 65537 frames, from its launch code (written down before the first run; the file and line that decides it is in the commit message): all
# of them serve the batch -- by slicing it at 65535 frames (rt.h sliceFrames), by a 1-D grid, or frame by frame.  An entry that declines instead must say so here.
DECLINES = set()
# entries whose note must show the second launch
PROOF = {"GaussianBlurBatch BORDER_WRAP": "k_binomial_roll<5,1>"}


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_65537_frames(cv, orc, name):
    cn, (w, h), single, batch = SWEEP[name]
    rng = np.random.default_rng(len(name) * 131 + w)
    base = rng.integers(0, 256, (B.P, h, w, cn) if cn > 1 else (B.P, h, w), dtype=np.uint8)
    base_dev = dev(base)
    ans = [single(cv, orc, base_dev[i], base[i]) for i in range(B.P)]
    ans = [a if isinstance(a, tuple) else (a,) for a in ans]
    want = [np.stack([host(a[o]) for a in ans]) for o in range(len(ans[0]))]                 # per output: [P, ...]
    frames = dev(B.periodic(base, N_SWEEP))
    # destinations of N + 1 frames, every byte FILL; the call gets the first N, the last one is a guard
    torch_of = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32,
                np.dtype(np.float64): torch.float64}
    whole = [prefilled((N_SWEEP + 1,) + w_.shape[1:], torch_of[w_.dtype]) for w_ in want]
    dst = tuple(t[:N_SWEEP] for t in whole)
    try:
        batch(cv, frames, dst)
    except NotImplementedError as e:                                                        # outcome (b): declined, for the frame count, nothing written
        assert "65535" in str(e) or "MAX_GRID_FRAMES" in str(e), str(e)
        assert all(untouched(t) for t in whole), "declined, but the destination changed"
        assert name in DECLINES, "declined (%s), where the launch code reads as serving the batch" % e
        return
    k = note(cv)
    assert name not in DECLINES, k
    for o, (t, w_) in enumerate(zip(whole, want)):                                         # outcome (a): every frame is its oracle frame
        assert untouched(t[N_SWEEP:]), (name, "output %d: written past the last frame" % o)
        ok, frame = B.same_periodic(host(t[:N_SWEEP]), w_)
        assert ok, (name, "output %d: first wrong frame" % o, frame, k)
    if name in PROOF:
        assert k.startswith(PROOF[name]) and B.cut_of(k, N_SWEEP)[0], k
