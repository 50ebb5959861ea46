"""HoughCircles without a GPU: the two restatements (tests/houghcircles_restate.py) against known answers and against each other, the lines of
opencv_amd/csrc/houghcircles_math.h compiled for the host (tests/hostemu/houghcircles_emu.cpp) against them, the rule's sanity on drawn discs through the project's
own Canny / Sobel oracle, and the argument refusals of the mi355cv_houghCircles* entries that come before any device is touched."""
import ctypes
import functools
import os

import numpy as np
import pytest

import emubuild
import houghcircles_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_IMPLEMENTED = 0, 1
F = np.float32
GRID = [(dp, radii) for dp in R.DPS for radii in R.RADII]
MIN_DISTS = (1.0, 7.5, 1000.0)                 # every centre apart; a few pixels; beyond every frame here


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


def one_pixel(h, w, x, y, vx, vy):
    e, dx, dy = np.zeros((h, w), np.uint8), np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    e[y, x], dx[y, x], dy[y, x] = 255, vx, vy
    return e, dx, dy


@functools.lru_cache(maxsize=None)
def small_frames():
    rng = np.random.default_rng(1)
    discs = R.simple_gradients(R.discs_on_noise(26, 34, ((9, 10, 6), (24, 15, 5)), seed=3))
    out = {"random 17 x 23": R.random_planes(rng, 17, 23, 0.3), "discs 26 x 34": discs, "uniform 8 x 8": R.uniform_planes(8, 8, 3, 4), "1 x 1": R.uniform_planes(1, 1, -7, 0),
           "empty": R.empty_planes(5, 6), "1 x 19": R.random_planes(rng, 1, 19, 0.6), "19 x 1": R.random_planes(rng, 19, 1, 0.6)}
    for planes in out.values():
        for a in planes:
            a.setflags(write=False)
    return out


# ---- known answers
@pytest.mark.parametrize("vec", [False, True])
def test_horizontal_gradient_votes_along_its_row(vec):
    h, w, x, y = 9, 21, 6, 4
    for vx in (5, -300):
        acc, circles = R.hough_circles(*one_pixel(h, w, x, y, vx, 0), 1.0, 5.0, 100, 1, 2, 9, vec=vec)
        want = np.zeros((h + 2, w + 2), np.int32)
        for r in range(2, 10):
            for c in (x + r, x - r):
                if 0 <= c < w:                                              # clipped at the accumulator: x - 7 .. x - 9 are outside it
                    want[y, c] += 1
        assert np.array_equal(acc, want) and want.sum() == 8 + 5
        assert len(circles) == 0                                            # no cell above accT = 1 ... the top vote is 1


@pytest.mark.parametrize("vec", [False, True])
def test_gradient_3_4_steps_614_819(vec):
    e, dx, dy = one_pixel(30, 30, 10, 10, 3, 4)
    acc, _ = R.hough_circles(e, dx, dy, 1.0, 5.0, 100, 1, 5, 5, vec=vec)        # maxRadius 5 <= minRadius 5 -> 7
    want = np.zeros((32, 32), np.int32)
    for r in (5, 6, 7):
        for sg in (1, -1):
            want[(10 * 1024 + sg * r * 819) >> 10, (10 * 1024 + sg * r * 614) >> 10] += 1
    assert np.array_equal(acc, want) and acc.sum() == 6
    assert R.cv_round(F(3) * F(1024) / F(5)) == 614 and R.cv_round(F(4) * F(1024) / F(5)) == 819


@pytest.mark.parametrize("vec", [False, True])
def test_row_0_and_column_0_vote_but_are_never_centres(vec):
    h, w = 6, 12
    e, dx, dy = np.zeros((h, w), np.uint8), np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    e[0, :] = 255
    dx[0, :] = 9                                                            # every pixel of row 0 votes along row 0
    e[:, 0] = 255
    dy[1:, 0] = 9                                                           # and column 0 along column 0
    acc, circles = R.hough_circles(e, dx, dy, 1.0, 1.0, 100, 1, 1, 3, vec=vec)
    assert acc[0, :w].min() >= 2 and acc[1:h, 0].min() >= 2 and not acc[1:, 1:].any()
    assert len(circles) == 0                                                # the only cells with votes are in row 0 and column 0
    p = R.prepare(w, h, 1.0, 1.0, 100, 1, 1, 3)
    assert len(R.centres_vec(acc, p, 1)) == 0 and len(R.centres_loops(acc, p, 1)) == 0


def test_prepared_arguments():
    p = R.prepare(67, 45, 0.5, 3, 100.5, 99.5, -4, 0)
    assert (p.dp, p.idp, p.canny, p.acc_t, p.min_radius, p.max_radius, p.centers_only) == (1, 1, 100, 100, 0, 67, False)      # halves go to even
    assert (p.arows, p.acols, p.astep, p.n_bins) == (45, 67, 69, 670)
    p = R.prepare(67, 45, 1.5, 3, 100, 100, 10, 10)
    assert (p.max_radius, p.centers_only, p.n_bins) == (12, False, R.cv_round(F(2) / F(1.5) * F(10)))
    assert (p.arows, p.acols) == (int(np.ceil(F(45) * (F(1) / F(1.5)))), int(np.ceil(F(67) * (F(1) / F(1.5)))))
    p = R.prepare(67, 45, 3, 3, 100, 100, 3, -1)
    assert (p.max_radius, p.centers_only, p.arows, p.acols) == (67, True, 15, 23)
    assert R.canny_thresholds(100) == (50, 100) and R.canny_thresholds(1) == (1, 1) and R.canny_thresholds(2.5) == (1, 2)


# ---- the two restatements agree
@pytest.mark.parametrize("dp,radii", GRID)
def test_restatements_agree(dp, radii):
    for name, (e, dx, dy) in small_frames().items():
        h, w = e.shape
        p = R.prepare(w, h, dp, 1.0, 100, 100, *radii)
        acc_l, nz = R.accum_loops(e, dx, dy, p)
        acc_v, pts = R.accum_vec(e, dx, dy, p)
        assert acc_l.shape == acc_v.shape == (p.arows + 2, p.acols + 2) and np.array_equal(acc_l, acc_v), name
        assert [tuple(q) for q in zip(*pts)] == nz, name                    # the point list, row by row
        top = int(acc_l.max())
        for acc_t in (0, top // 2, top):
            assert list(R.centres_vec(acc_v, p, acc_t)) == R.centres_loops(acc_l, p, acc_t), (name, acc_t)
            for b in (R.centres_loops(acc_l, p, acc_t)[:6] if p.n_bins >= 1 else ()):
                cx, cy = (F(b % p.astep) + F(0.5)) * p.dp, (F(b // p.astep) + F(0.5)) * p.dp
                bl, bv = R.bins_loops(cx, cy, nz, p), R.bins_vec(cx, cy, pts, p)
                assert np.array_equal(bl, bv), (name, acc_t, b)
                rl, rv = R.scan_loops(bl, p), R.scan_vec(bv, p)
                assert rl[1] == rv[1] and R.same_bits(rl[0], rv[0]), (name, acc_t, b)
            if p.n_bins < 1 and not p.centers_only:
                continue                                                    # the library refuses these arguments
            cand_l, cand_v = R.candidates_loops(acc_l, nz, p, acc_t), R.candidates_vec(acc_v, pts, p, acc_t)
            for md in MIN_DISTS:
                p.min_dist = F(md)
                cl, cvv = R.suppress_loops(cand_l, p, None), R.suppress_vec(cand_v, p)
                assert R.same_bits(cl, cvv), (name, acc_t, md)
                assert acc_t < top or len(cl) == 0
                assert np.all(cl[:-1, 3] >= cl[1:, 3])                      # votes descending
                if md == 1000.0:
                    assert len(cl) <= 1
                cap = R.suppress_vec(cand_v, p, 2)
                assert R.same_bits(cap, cvv[:2]) and R.same_bits(R.suppress_loops(cand_l, p, 2), cap)


def test_scan_forms_agree_on_random_bins_and_a_window_that_ends_at_bin_0():
    rng = np.random.default_rng(7)
    p = R.prepare(64, 64, 1.0, 1.0, 100, 100, 3, 40)
    for trial in range(200):
        n = int(rng.integers(1, 400))
        p.n_bins = n
        bins = ((rng.random(n) < rng.choice([0.02, 0.2, 0.9])) * rng.integers(1, 9, n)).astype(np.int32)
        a, b = R.scan_loops(bins, p), R.scan_vec(bins, p)
        assert a[1] == b[1] and R.same_bits(a[0], b[0]), trial
    p.n_bins = 30
    bins = np.zeros(30, np.int32)
    bins[4], bins[0] = 3, 5                                                 # the window of bin 4 runs through bin 0 and stops at j = -1
    r, m = R.scan_loops(bins, p)
    assert m == 8 and r == F(4 - 1) / F(2) / F(10) * F(1) + F(3) and (r, m) == R.scan_vec(bins, p)
    bins[:] = 0
    bins[0] = 9                                                             # bin 0 alone never opens a window
    assert R.scan_loops(bins, p) == (0, 0) == R.scan_vec(bins, p)


# ---- houghcircles_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("houghcircles_emu.cpp", "libhoughcircles_emu.so", ["-ffp-contract=off"])
    i32, dbl, vp, sz = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    lib.emu_hc_prepare.argtypes = [i32, i32, dbl, dbl, dbl, dbl, i32, i32, vp]
    lib.emu_hc_make_ray.argtypes = [i32, i32, i32, i32, ctypes.c_float, vp]
    lib.emu_hc_accum.argtypes = [vp, sz, vp, vp, sz, i32, i32, dbl, i32, i32, vp, vp]
    lib.emu_hc_circles.argtypes = [vp, vp, i32, i32, i32, dbl, dbl, dbl, dbl, i32, i32, i32, i32, i32, vp]
    return lib


def emu_prepare(emu, w, h, dp, md, p1, p2, r0, r1):
    out = np.full(8, -9, np.int32)
    return emu.emu_hc_prepare(w, h, dp, md, p1, p2, r0, r1, P(out)), out.tolist()


def emu_run(emu, planes, dp, md, radii, acc_t, cn=4, cap=None):
    e, dx, dy = (np.ascontiguousarray(a) for a in planes)
    h, w = e.shape
    p = R.prepare(w, h, dp, md, 100, max(acc_t, 1), *radii)
    acc = np.full((p.arows + 2, p.astep), -7, np.int32)
    pts = np.zeros(w * h, np.uint32)
    n = emu.emu_hc_accum(P(e), e.strides[0], P(dx), P(dy), dx.strides[0] // 2, w, h, dp, radii[0], radii[1], P(acc), P(pts))
    cap = cap if cap is not None else max(1, p.arows * ((p.acols + 1) // 2))
    out = np.full((cap, cn), -7.0, F)
    k = emu.emu_hc_circles(P(acc), P(pts), n, w, h, dp, md, 100.0, float(max(acc_t, 1)), radii[0], radii[1], acc_t, cn, cap, P(out))
    return acc, n, k, out


def test_emulated_constants_and_rays(emu):
    want = [R.MAX_DIM, R.MAX_ACCUM, R.MAX_RADIUS, R.MAX_CIRCLES, R.LDS_BINS, R.TILE, R.STEP_BLOCK, R.SHIFT, R.ONE, R.BINS_PER_DR, R.HOUGH_GRADIENT,
            R.HOUGH_GRADIENT_ALT]
    assert [emu.emu_hc_limit(i) for i in range(len(want))] == want and emu.emu_hc_limit(len(want)) == -1
    out = np.zeros(4, np.int32)
    assert emu.emu_hc_make_ray(10, 20, 3, 4, 1.0, P(out)) == 1 and out.tolist() == [10240, 20480, 614, 819]
    assert emu.emu_hc_make_ray(10, 20, 0, 0, 1.0, P(out)) == 0
    assert emu.emu_hc_make_ray(7, 9, -32768, -32768, 1.0, P(out)) == 1 and out.tolist() == [7168, 9216, -724, -724]       # the squares' sum is 2^31: no int overflow
    rng = np.random.default_rng(4)
    for _ in range(300):
        x, y = (int(v) for v in rng.integers(0, 4000, 2))
        vx, vy = (int(v) for v in rng.integers(-1020, 1021, 2))
        idp = F(1) / F(rng.choice([1.0, 1.5, 2.0, 3.0]))
        if vx == 0 and vy == 0:
            continue
        mag = np.sqrt(F(vx * vx + vy * vy))
        want = [R.cv_round(F(x) * idp * F(1024)), R.cv_round(F(y) * idp * F(1024)), R.cv_round(F(vx) * idp * F(1024) / mag), R.cv_round(F(vy) * idp * F(1024) / mag)]
        assert emu.emu_hc_make_ray(x, y, vx, vy, idp, P(out)) == 1 and out.tolist() == want


def test_emulated_prepare_and_its_refusals(emu):
    for w, h in ((1, 1), (67, 45), (200, 150), (3840, 2160)):
        for dp, radii in GRID:
            p = R.prepare(w, h, dp, 2.0, 100.5, 30.5, *radii)
            want = [p.arows, p.acols, p.n_bins, p.min_radius, p.max_radius, int(p.centers_only), p.canny, p.acc_t]
            rc, got = emu_prepare(emu, w, h, dp, 2.0, 100.5, 30.5, *radii)
            if p.n_bins < 1:
                assert rc == 4, (w, h, dp, radii)                           # minRadius beyond the tiny frame's default maxRadius
            else:
                assert (rc, got) == (0, want), (w, h, dp, radii)
    nan = float("nan")
    for bad in ((0.0, 1.0, 100.0, 100.0), (-1.0, 1.0, 100.0, 100.0), (nan, 1.0, 100.0, 100.0), (1.0, 0.0, 100.0, 100.0), (1.0, -2.0, 100.0, 100.0), (1.0, nan, 100.0, 100.0),
                (1.0, 1.0, 0.0, 100.0), (1.0, 1.0, 0.5, 100.0), (1.0, 1.0, nan, 100.0), (1.0, 1.0, 100.0, 0.0), (1.0, 1.0, 100.0, 0.4), (1.0, 1.0, 100.0, -3.0),
                (1.0, 1.0, 100.0, nan), (1.0, 1e-60, 100.0, 100.0), (1.0, 1.0, 1e300, 100.0)):
        assert emu_prepare(emu, 67, 45, *bad, 0, 0)[0] == 1, bad
    assert emu_prepare(emu, 67, 45, 1.0, 1.0, 0.51, 1.5, 0, 0) == (0, [45, 67, 670, 0, 67, 0, 1, 2])      # cvRound(0.51) = 1, cvRound(1.5) = 2
    assert emu_prepare(emu, R.MAX_DIM, R.MAX_DIM, 1.0, 1.0, 100.0, 100.0, 0, 0)[0] == 2                  # 16386^2 cells
    assert emu_prepare(emu, R.MAX_DIM, R.MAX_DIM, 2.01, 1.0, 100.0, 100.0, 0, 0)[0] == 0
    assert emu_prepare(emu, 67, 45, 1.0, 1.0, 100.0, 100.0, 0, R.MAX_RADIUS + 1)[0] == 3 and emu_prepare(emu, 67, 45, 1.0, 1.0, 100.0, 100.0, 0, R.MAX_RADIUS)[0] == 0
    assert emu_prepare(emu, 67, 45, 1.0, 1.0, 100.0, 100.0, R.MAX_RADIUS - 1, 5)[0] == 3                 # minRadius + 2
    assert emu_prepare(emu, 67, 45, 1.0, 1.0, 100.0, 100.0, 68, 0)[0] == 4 and emu_prepare(emu, 67, 45, 1e6, 1.0, 100.0, 100.0, 0, 0)[0] == 4


@pytest.mark.parametrize("dp,radii", GRID)
def test_emulated_kernels_match_the_restatement(emu, dp, radii):
    rng = np.random.default_rng(2)
    frames = dict(small_frames())
    frames["random 45 x 67"] = R.random_planes(rng, 45, 67, 0.1)
    frames["uniform 16 x 16"] = R.uniform_planes(16, 16, -5, 5)             # long runs of tied votes through both orders
    for name, planes in frames.items():
        h, w = planes[0].shape
        if R.prepare(w, h, dp, 1.0, 100, 100, *radii).n_bins < 1:
            continue                                                        # refused, see test_emulated_prepare_and_its_refusals
        want_acc, _ = R.hough_circles(*planes, dp, 1.0, 100, 1, *radii)
        top = int(want_acc.max())
        pts = R.points_vec(*planes)
        for acc_t in (0, top // 2, top):
            p = R.prepare(w, h, dp, 1.0, 100, 1, *radii)
            cands = R.candidates_vec(want_acc, (pts[0], pts[1]), p, acc_t)
            for md in MIN_DISTS:
                acc, n, k, out = emu_run(emu, planes, dp, md, radii, acc_t)
                p.min_dist = F(md)
                want = R.suppress_vec(cands, p)
                assert np.array_equal(acc, want_acc) and n == len(pts[0]), (name, acc_t, md)
                assert k == len(want) and R.same_bits(out[:k], want), (name, acc_t, md, k, len(want))
                assert np.all(out[k:] == -7.0)


def test_emulated_three_floats_and_a_short_list(emu):
    planes = small_frames()["discs 26 x 34"]
    want = R.hough_circles(*planes, 1.0, 2.0, 100, 4, 0, 0)[1]
    assert len(want) > 3
    _, _, k, out = emu_run(emu, planes, 1.0, 2.0, (0, 0), 4, cn=3, cap=3)
    assert k == 3 and R.same_bits(out, want[:3, :3])
    assert R.same_bits(R.hough_circles(*planes, 1.0, 2.0, 100, 4, 0, 0, max_circles=3)[1], want[:3])


# ---- sanity of the rule on drawn discs, through the project's own Canny / Sobel oracle
DISCS = ((40, 40, 20), (90, 50, 12), (70, 75, 9))
DISC_MARGIN = 1.0 + 1.0                         # dp + 1 px


def test_drawn_discs_are_found(orc):
    """the restatement, never a kernel, on the oracle's Canny / Sobel planes of three drawn discs: all three found, each within dp + 1 px of the truth in centre and
    radius (what the restatement gives: 0.5, 1.5 and 0.6 px).  param2 = 12: the accumulator's top vote on this frame is 22, the smallest disc's centre has fewer"""
    img = R.discs_on_noise(96, 128, DISCS, seed=11)
    low, high = R.canny_thresholds(100)
    edges = orc.orc_Canny(img, low, high, 3, False)
    dx, dy = orc.orc_Sobel(img, 3, 1, 0, 3, border=1), orc.orc_Sobel(img, 3, 0, 1, 3, border=1)
    assert dx.dtype == np.int16 and edges.any()
    for vec in (True, False):
        _, circles = R.hough_circles(edges, dx, dy, 1.0, 20.0, 100, 12, 5, 40, vec=vec)
        print("circles", circles.tolist())
        assert len(circles) == 3
        for (cx, cy, r) in DISCS:
            d = np.abs(circles[:, :3] - np.array([cx, cy, r], F)).max(axis=1)
            print("disc", (cx, cy, r), "nearest", float(d.min()))
            assert d.min() <= DISC_MARGIN, (cx, cy, r, circles.tolist())


# ---- the C ABI's refusals that need no device
ENTRIES = ("mi355cv_houghCircles", "mi355cv_houghCirclesBatch", "mi355cv_houghCirclesGradient", "mi355cv_houghCirclesAccum", "mi355cv_houghCirclesSetKernel")
COUNTERS = (b"houghCircles", b"houghCirclesBatch", b"houghCirclesGradient", b"houghCirclesAccum")


def test_header_symbols_are_bound():
    from opencv_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mi355cv.h")).read()
    for name in ENTRIES:
        assert name + "(" in txt and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert "cv::HoughLinesP and cv::HoughLinesPointSet have no entry" in txt and "cv::HoughCircles and" not in txt


def test_bounds_are_exposed_and_pinned():
    from opencv_amd import _lib
    for key, value in R.LIMITS.items():
        assert _lib.limit(key) == value, key
    assert R.MAX_DIM <= 65535 and R.MAX_DIM * R.MAX_DIM <= 1 << 28
    assert R.MAX_DIM * 1024 + R.MAX_RADIUS * 1025 < 1 << 31                 # x0 + r * sx, |sx| <= idp * ONE + 0.5
    assert R.LDS_BINS * 4 <= 160 << 10 and R.TILE * R.TILE * 4 <= 64 << 10


def test_set_kernel_takes_the_three_modes():
    from opencv_amd import _lib
    Lb = _lib.lib
    assert Lb.mi355cv_houghCirclesSetKernel(2) == -1 and Lb.mi355cv_houghCirclesSetKernel(-2) == -1
    assert Lb.mi355cv_houghCirclesSetKernel(0) == 0 and Lb.mi355cv_houghCirclesSetKernel(1) == 0 and Lb.mi355cv_houghCirclesSetKernel(-1) == 0


def test_entries_decline_bad_arguments_before_a_device_is_touched():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.ones((16, 16), np.uint8)
    g = np.ones((16, 16), np.int16)
    circles = np.full((8, 4), 7.0, F)
    acc = np.full((18, 18), 7, np.int32)
    nc = (ctypes.c_int * 2)(-5, -5)
    ar, ac = ctypes.c_int(-5), ctypes.c_int(-5)
    n0 = sum(L.mi355cv_callCount(n) for n in COUNTERS)
    big = _lib.limit("houghcircles_max_dim") + 1
    ptr = lambda v: P(v) if v is not None else None

    def one(src=a, step=16, w=16, h=16, dst=circles, cn=3, cap=8, method=R.HOUGH_GRADIENT, dp=1.0, md=2.0, p1=100.0, p2=10.0, r0=0, r1=0, n=nc, **_):
        return L.mi355cv_houghCircles(ptr(src), step, w, h, ptr(dst), cn, cap, method, dp, md, p1, p2, r0, r1, n)

    def batch(src=a, step=16, w=16, h=16, dst=circles, cn=3, cap=4, method=R.HOUGH_GRADIENT, dp=1.0, md=2.0, p1=100.0, p2=10.0, r0=0, r1=0, n=nc, nf=2, sf=128, lf=48, **_):
        return L.mi355cv_houghCirclesBatch(ptr(src), step, sf, w, h, ptr(dst), cn, cap, lf, nf, method, dp, md, p1, p2, r0, r1, n)

    def grad(src=a, step=16, w=16, h=16, dst=circles, cn=3, cap=8, method=R.HOUGH_GRADIENT, dp=1.0, md=2.0, p1=100.0, p2=10.0, r0=0, r1=0, n=nc, gx=g, gy=g, gstep=32, **_):
        return L.mi355cv_houghCirclesGradient(ptr(src), step, ptr(gx), ptr(gy), gstep, w, h, ptr(dst), cn, cap, method, dp, md, p1, p2, r0, r1, n)

    def accum(src=a, step=16, w=16, h=16, dst=acc, dp=1.0, r0=0, r1=0, gx=g, gy=g, gstep=32, astep=18 * 4, pa=ctypes.byref(ar), pc=ctypes.byref(ac), **_):
        return L.mi355cv_houghCirclesAccum(ptr(src), step, ptr(gx), ptr(gy), gstep, w, h, dp, r0, r1, ptr(dst), astep, pa, pc)

    reason = lambda: L.mi355cv_lastError().decode()
    nan = float("nan")
    for f in (one, batch, grad, accum):
        assert f(dp=0.0) == NOT_IMPLEMENTED and f(dp=-1.0) == NOT_IMPLEMENTED and f(dp=nan) == NOT_IMPLEMENTED and "dp" in reason()
        assert f(src=None) == NOT_IMPLEMENTED
        assert f(w=0) == NOT_IMPLEMENTED and f(h=-2) == NOT_IMPLEMENTED and f(w=big) == NOT_IMPLEMENTED and f(h=big) == NOT_IMPLEMENTED and "HOUGHCIRCLES_MAX_DIM" in reason()
        assert f(w=big - 1, h=big - 1, step=big - 1, gstep=2 * big) == NOT_IMPLEMENTED and "HOUGHCIRCLES_MAX_ACCUM" in reason()
        assert f(r1=_lib.limit("houghcircles_max_radius") + 1) == NOT_IMPLEMENTED and "HOUGHCIRCLES_MAX_RADIUS" in reason()
        assert f(r0=17) == NOT_IMPLEMENTED and "nBins" in reason()
        assert f(step=15) == NOT_IMPLEMENTED and "step" in reason()
    for f in (one, batch, grad):
        assert f(method=R.HOUGH_GRADIENT_ALT) == NOT_IMPLEMENTED and "HOUGH_GRADIENT_ALT" in reason()
        assert f(method=0) == NOT_IMPLEMENTED and f(method=9) == NOT_IMPLEMENTED and "HOUGH_GRADIENT" in reason()
        assert f(md=0.0) == NOT_IMPLEMENTED and f(md=-1.0) == NOT_IMPLEMENTED and f(md=nan) == NOT_IMPLEMENTED and "minDist" in reason()
        assert f(p1=0.0) == NOT_IMPLEMENTED and f(p1=0.5) == NOT_IMPLEMENTED and f(p1=nan) == NOT_IMPLEMENTED and f(p1=-4.0) == NOT_IMPLEMENTED and "param1" in reason()
        assert f(p2=0.0) == NOT_IMPLEMENTED and f(p2=0.5) == NOT_IMPLEMENTED and f(p2=nan) == NOT_IMPLEMENTED and f(p2=-4.0) == NOT_IMPLEMENTED and "param2" in reason()
        assert f(dst=None) == NOT_IMPLEMENTED and "circles" in reason()
        assert f(n=None) == NOT_IMPLEMENTED and "ncircles" in reason()
        for cn in (0, 2, 5):
            assert f(cn=cn) == NOT_IMPLEMENTED and "circles_cn" in reason()
        assert f(cap=0) == NOT_IMPLEMENTED and f(cap=-1) == NOT_IMPLEMENTED and f(cap=_lib.limit("houghcircles_max_circles") + 1) == NOT_IMPLEMENTED
        assert "HOUGHCIRCLES_MAX_CIRCLES" in reason()
    for f in (grad, accum):
        assert f(gx=None) == NOT_IMPLEMENTED and f(gy=None) == NOT_IMPLEMENTED and "dx" in reason()
        assert f(gstep=30) == NOT_IMPLEMENTED and f(gstep=33) == NOT_IMPLEMENTED and "grad_step" in reason()
    assert batch(nf=0) == NOT_IMPLEMENTED and "nframes" in reason()
    assert batch(nf=65536, sf=256, lf=48) == NOT_IMPLEMENTED and "65535" in reason()
    assert batch(lf=8) == NOT_IMPLEMENTED and batch(lf=49) == NOT_IMPLEMENTED and "circles_frame_stride" in reason()
    assert batch(sf=100) == NOT_IMPLEMENTED and "src_frame_stride" in reason()
    assert accum(astep=17 * 4) == NOT_IMPLEMENTED and accum(astep=18 * 4 + 2) == NOT_IMPLEMENTED and "accum_step" in reason()
    assert accum(pa=None) == NOT_IMPLEMENTED and accum(pc=None) == NOT_IMPLEMENTED and "arows" in reason()
    assert sum(L.mi355cv_callCount(n) for n in COUNTERS) == n0
    assert np.all(circles == 7.0) and np.all(acc == 7) and list(nc) == [-5, -5] and (ar.value, ac.value) == (-5, -5)
    # the geometry alone needs no device either
    assert accum(dst=None) == OK and (ar.value, ac.value) == (16, 16)
    assert accum(dst=None, dp=3.0, w=67, h=45, step=67, gstep=134) == OK and (ar.value, ac.value) == (15, 23)
    assert accum(dst=None, dp=0.25) == OK and (ar.value, ac.value) == (16, 16)                             # dp below 1 is 1


def test_python_api_refuses_bad_arguments():
    import opencv_amd as cv
    for name in ("HoughCircles", "HoughCirclesBatch", "HoughCirclesGradient", "HoughCirclesAccumulator"):
        assert name in cv.imgproc.__all__ and hasattr(cv, name), name
    assert (cv.HOUGH_GRADIENT, cv.HOUGH_GRADIENT_ALT) == (R.HOUGH_GRADIENT, R.HOUGH_GRADIENT_ALT)
    a = np.zeros((8, 8), np.uint8)
    g = np.zeros((8, 8), np.int16)
    n0 = cv._lib.decline_count()
    for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8), np.uint16), np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 1), np.uint8), np.zeros((8, 8), np.int8)):
        with pytest.raises(ValueError):
            cv.HoughCircles(bad, cv.HOUGH_GRADIENT, 1, 5)
        with pytest.raises(ValueError):
            cv.HoughCirclesGradient(bad, g, g, 1, 5)
        with pytest.raises(ValueError):
            cv.HoughCirclesAccumulator(bad, g, g, 1)
    for kw in (dict(dp=0), dict(dp=-1), dict(dp=float("nan")), dict(minDist=0), dict(minDist=-2), dict(param1=0), dict(param1=-1), dict(param2=0), dict(param2=float("nan")),
               dict(maxCircles=0), dict(method=7)):
        args = dict(method=cv.HOUGH_GRADIENT, dp=1, minDist=5)
        args.update(kw)
        with pytest.raises(ValueError):
            cv.HoughCircles(a, **args)
    for gx, gy in ((np.zeros((8, 8), np.int32), g), (g, np.zeros((8, 9), np.int16)), (np.zeros((8, 8, 2), np.int16), g)):
        with pytest.raises(ValueError):
            cv.HoughCirclesGradient(a, gx, gy, 1, 5)
        with pytest.raises(ValueError):
            cv.HoughCirclesAccumulator(a, gx, gy, 1)
    with pytest.raises(ValueError):
        cv.HoughCirclesGradient(a, g, g, 1, 5, param2=0)
    with pytest.raises(ValueError):
        cv.HoughCirclesAccumulator(a, g, g, 0)
    with pytest.raises(ValueError):
        cv.HoughCirclesBatch(a, cv.HOUGH_GRADIENT, 1, 5)
    assert cv._lib.decline_count() == n0                                    # nothing reached the library
    with pytest.raises(NotImplementedError, match="HOUGH_GRADIENT_ALT"):
        cv.HoughCircles(a, cv.HOUGH_GRADIENT_ALT, 1.5, 5, 300, 0.9)
