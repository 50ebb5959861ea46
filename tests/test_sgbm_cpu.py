"""cv::StereoSGBM without a GPU: the two forms of the restatement (tests/sgbm_restate.py) against each other bit for bit, answers worked out by hand, the lines of
opencv_amd/csrc/sgbm_math.h compiled for the host (tests/hostemu/sgbm_emu.cpp) against the restatement stage by stage, the refusals of the mi355cv_stereoSGBM* entries
that come before any device is touched, the limits, the arithmetic of the 16-bit cost bound and the layout of mi355cv_StereoSGBMParams.  The last tests: the smooth
shifted pairs of the GPU suite on the restatement itself, and StereoBM's surface as it was."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import emubuild
import sgbm_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, mode, shift)
GRID = [(6, 30, 0, 16, 3, 8, 32, 1, 31, 10, R.MODE_SGBM, 3), (5, 29, 4, 16, 5, 0, 0, 0, 0, 0, R.MODE_HH, 9), (7, 44, -8, 32, 1, 5, 5, 2, 63, 40, R.MODE_HH4, -2),
        (4, 26, -21, 16, 3, 10, 3000, -1, 15, 10, R.MODE_HH, -12), (1, 24, 0, 16, 3, 8, 32, 1, 31, 15, R.MODE_SGBM, 15), (5, 16, 0, 16, 5, 8, 32, 1, 31, 0, R.MODE_HH, 0),
        (9, 23, 2, 16, 9, 3, 90, 1, 20, 5, R.MODE_SGBM, 4)]


def params(case):
    H, W, m, n, w, P1, P2, lr, cap, uniq, mode, s = case
    return R.Params(m, n, w, P1, P2, lr, cap, uniq, 0, 0, mode)


def pairs(case, seed):
    H, W, s = case[0], case[1], case[-1]
    rng = np.random.default_rng(seed)
    return R.random_pair(rng, H, W), R.smooth_pair(rng, H, W, s), R.constant_pair(H, W)


@pytest.mark.parametrize("case", GRID)
def test_the_two_forms_of_the_restatement_agree(case):
    p = params(case)
    W = case[1]
    for L, Rr in pairs(case, 11):
        for ft in (15, 31, 63):
            assert np.array_equal(R.prefilter_loops(L, ft), R.prefilter_np(L, ft))
        pa, pb = R.pixel_cost_loops(L, Rr, p), R.pixel_cost_np(L, Rr, p)
        assert np.array_equal(pa, pb)
        Ca, Cb = R.block_cost_loops(pa, p.w), R.block_cost_np(pb, p.w)
        assert np.array_equal(Ca, Cb) and (Cb.size == 0 or Cb.max() <= R.cost_bound(p) - p.P2)
        for ry, rx in R.DIRECTIONS[R.MODE_HH]:
            La, Lb = R.path_loops(Ca, ry, rx, p.P1, p.P2), R.path_np(Cb, ry, rx, p.P1, p.P2)
            assert np.array_equal(La, Lb), (ry, rx)
            assert Lb.size == 0 or (0 <= Lb.min() and Lb.max() <= R.cost_bound(p)), "the bound under which every L_r fits 16 bits"
        Sa, Sb = R.aggregate_loops(Ca, p), R.aggregate_np(Cb, p)
        assert np.array_equal(Sa, Sb)
        da, db = R.decide_loops(Sa, p), R.decide_np(Sb, p)
        for a, b in zip(da, db):
            assert np.array_equal(a, b)
        for lr in (-1, 0, 1, 3):
            q = p._replace(disp12MaxDiff=lr)
            assert np.array_equal(R.left_right_loops(*da, W, q), R.left_right_np(*db, W, q)), lr
        assert np.array_equal(R.compute_loops(L, Rr, p), R.compute_np(L, Rr, p))


def test_a_row_without_penalties_is_the_cost_times_the_directions():
    """1 x 20, n = 16, w = 1, P1 = P2 = 0: the minimum of the recurrence is M + P2 = M, so L_r = C + M - M = C on every path and S = |R| C"""
    rng = np.random.default_rng(3)
    L, Rr = R.random_pair(rng, 1, 20)
    for mode, nr in ((R.MODE_SGBM, 5), (R.MODE_HH, 8), (R.MODE_HH4, 4)):
        p = R.Params(0, 16, 1, 0, 0, mode=mode)
        st = {}
        R.compute_np(L, Rr, p, st)
        assert st["C"].shape == (1, 5, 16) and np.array_equal(st["pc"], st["C"])              # xlo = 15: five valid columns; w = 1: the block is the pixel
        assert np.array_equal(st["S"], nr * st["C"].astype(np.int64))
        assert np.array_equal(R.aggregate_loops(st["C"], p), st["S"])
    # one cost by hand.  Left pixel X = 17 against right pixel 17 - 3: both planes
    Lr, Rw = L[0].astype(int), Rr[0].astype(int)

    def bt(a, x):
        am, ap = (a[x] + a[max(x - 1, 0)]) >> 1, (a[x] + a[min(x + 1, 19)]) >> 1
        return a[x], min(am, ap, a[x]), max(am, ap, a[x])
    u, lol, hil = bt(Lr, 17)
    v, lor, hir = bt(Rw, 14)
    raw = min(max(0, u - hir, lor - u), max(0, v - hil, lol - v)) >> 2
    gl = [15] + [min(max(4 * (Lr[x + 1] - Lr[x - 1]), -15), 15) + 15 for x in range(1, 19)] + [15]     # H = 1: the row is its own neighbours, 2 g + g + g
    gr = [15] + [min(max(4 * (Rw[x + 1] - Rw[x - 1]), -15), 15) + 15 for x in range(1, 19)] + [15]
    u, lol, hil = bt(gl, 17)
    v, lor, hir = bt(gr, 14)
    assert st["pc"][0, 2, 3] == raw + min(max(0, u - hir, lor - u), max(0, v - hil, lol - v))


def test_each_term_of_the_recurrence_wins_once():
    """a path of two pixels, n = 4, P1 = 2, P2 = 7.  L(p0) = C(p0) = (9, 0, 5, 30), M = 0.  At p1: k = 0: min(9, 0 + 2, -, 0 + 7) = 2, the k + 1 term; k = 1: min(0, 9 + 2,
    5 + 2, 7) = 0, the term of k itself; k = 2: min(5, 0 + 2, 30 + 2, 7) = 2, the k - 1 term; k = 3: min(30, 5 + 2, -, 7) = 7: with P1 = 2 the k - 1 term ties M + P2, so
    P2 = 6 makes M + P2 the only winner"""
    C = np.array([[[9, 0, 5, 30], [100, 200, 300, 400]]], np.int32)
    for f in (R.path_loops, R.path_np):
        assert f(C, 0, 1, 2, 7)[0, 1].tolist() == [102, 200, 302, 407]
        assert f(C, 0, 1, 2, 6)[0, 1].tolist() == [102, 200, 302, 406]
        assert f(C, 0, 1, 2, 7)[0, 0].tolist() == [9, 0, 5, 30]                                # no predecessor: L = C
        assert f(C, 0, -1, 0, 0)[0, 0].tolist() == [9, 0, 5, 30]                               # P1 = P2 = 0 as given: + M - M
        assert f(C, 1, 0, 2, 7)[0].tolist() == C[0].tolist()                                   # a single row: every pixel starts a vertical path
    # M is subtracted: predecessor (9, 4, 5, 30), M = 4
    C[0, 0, 1] = 4
    for f in (R.path_loops, R.path_np):
        assert f(C, 0, 1, 2, 7)[0, 1].tolist() == [100 + 6 - 4, 200 + 4 - 4, 300 + 5 - 4, 400 + 7 - 4]


def test_the_sub_pixel_quotient_is_c_division():
    """S = (.., 40, 10, 21, ..) at best = 5: den = 40 + 21 - 20 = 41; numerator (40 - 21) * 16 + 41 = 345, 345 / 82 = 4.  Mirrored, (21, 10, 40): (21 - 40) * 16 + 41 = -263,
    -263 / 82 = -3.2: toward zero -3 (floor would give -4): d = 5 * 16 - 3 = 77"""
    S = np.full((1, 1, 16), 1000, np.int64)
    S[0, 0, 4:7] = 40, 10, 21
    p = R.Params(0, 16, 3)
    for f in (R.decide_loops, R.decide_np):
        assert f(S, p)[0][0, 0] == 84
        assert f(S[:, :, ::-1].copy(), p)[0][0, 0] == 10 * 16 - 3                              # reversed: best = 10 between 21 and 40, the -263 / 82 = -3 of below
    S[0, 0, 4:7] = 21, 10, 40
    for f in (R.decide_loops, R.decide_np):
        assert f(S, p)[0][0, 0] == 77
        assert f(S, p._replace(minDisparity=-3))[0][0, 0] == 77 - 48
    assert R.cdiv(-263, 82) == -3 and -263 // 82 == -4
    # the ends of the range take no sub-pixel step; a flat minimum has den = max(0, 1) = 1 and numerator 1: 1 / 2 = 0
    S[0, 0] = 1000; S[0, 0, 0] = 5
    assert R.decide_np(S, p)[0][0, 0] == 0 and R.decide_loops(S, p)[0][0, 0] == 0
    S[0, 0] = 7
    assert R.decide_np(S, p)[0][0, 0] == 0                                                     # all equal: the smallest k
    # uniqueness 10: S_k * 90 < ms * 100 with ms = 90: S_k = 99 rejects (8910 < 9000), 100 does not; next to the winner nothing rejects
    for v, k, keep in ((99, 9, False), (100, 9, True), (99, 6, True), (99, 4, True), (99, 7, False)):
        S[0, 0] = 1000; S[0, 0, 5] = 90; S[0, 0, k] = v
        q = p._replace(uniquenessRatio=10)
        assert R.decide_np(S, q)[3][0, 0] == keep == R.decide_loops(S, q)[3][0, 0], (v, k)


def test_a_left_right_tie_goes_to_the_larger_x():
    """W = 24, m = -4, n = 16: valid columns 11 .. 19.  X = 14 with disparity 1 and X = 17 with disparity 4 both vote for column 13 with the same S: the larger x wins,
    d2[13] = 4, and X = 14 looks at column 14 - 1 = 13 and sees |4 - 1| = 3 > q = 1"""
    p = R.Params(-4, 16, 3, disp12MaxDiff=1)
    W = 24
    xlo, xhi = R.valid_columns(W, p)
    assert (xlo, xhi) == (11, 20)
    W1 = xhi - xlo
    kept = np.zeros((1, W1), bool)
    best, ms = np.zeros((1, W1), np.int32), np.zeros((1, W1), np.int64)
    d = np.full((1, W1), p.filtered, np.int32)
    # X = 14 with disparity 1 (best = 5) and X = 17 with disparity 4 (best = 8) vote for column 13
    for x, b in ((3, 5), (6, 8)):
        kept[0, x], best[0, x], ms[0, x], d[0, x] = True, b, 50, (b + p.m) * 16
    for f in (R.left_right_loops, R.left_right_np):
        out = f(d, best, ms, kept, W, p)
        assert out[0, 6] == 64 and out[0, 3] == p.filtered, "the larger x wins the tie; the loser sees |4 - 1| = 3 > 1"
        ms2 = ms.copy(); ms2[0, 3] = 49
        out = f(d, best, ms2, kept, W, p)
        assert out[0, 3] == 16 and out[0, 6] == p.filtered, "a smaller S beats the larger x"
        out = f(d, best, ms, kept, W, p._replace(disp12MaxDiff=3))
        assert out[0, 3] == 16 and out[0, 6] == 64, "|4 - 1| = 3 > 3 is false"
        for lr in (0, -1):                                                                      # q = 1 whenever disp12MaxDiff <= 0: the check is always made
            assert f(d, best, ms, kept, W, p._replace(disp12MaxDiff=lr))[0, 3] == p.filtered


def test_the_smooth_pairs_meet_the_conditions_of_the_gpu_test_on_the_cpu():
    """the test of tests/test_sgbm_gpu.py that does not rest on the restatement, run on the restatement itself"""
    for mode in (R.MODE_SGBM, R.MODE_HH, R.MODE_HH4):
        for m, s in ((0, 5), (0, 15), (4, 9), (-8, -3), (-20, -12)):
            L, Rr = R.smooth_pair(np.random.default_rng(100 + s), 40, 96, s)
            p = R.Params(m, 16, 5, 200, 800, 1, 63, 10, mode=mode)
            R.check_shift_recovered(R.compute_np(L, Rr, p), p, s)


@functools.lru_cache(maxsize=1)
def emu():
    lib = emubuild.load("sgbm_emu.cpp", "libsgbm_emu.so")
    i32, vp = ctypes.c_int, ctypes.c_void_p
    lib.emu_sgbm_geom.argtypes = [i32, i32, i32, vp]
    lib.emu_sgbm_bound.argtypes, lib.emu_sgbm_bound.restype = [i32, i32, i32], ctypes.c_longlong
    lib.emu_sgbm_frame_scratch.argtypes, lib.emu_sgbm_frame_scratch.restype = [i32] * 4, ctypes.c_ulonglong
    lib.emu_sgbm_prefilter.argtypes = [vp, i32, i32, i32, vp]
    lib.emu_sgbm_pixel_cost.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.emu_sgbm_block_cost.argtypes = [vp, i32, i32, i32, i32, vp]
    lib.emu_sgbm_aggregate.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.emu_sgbm_decide.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    lib.emu_sgbm_leftright.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp]
    return lib


@pytest.mark.parametrize("case", GRID)
def test_sgbm_math_on_the_host_matches_the_restatement(case):
    E = emu()
    H, W, m, n, w, P1, P2, lr, cap, uniq, mode, s = case
    p = params(case)
    g = np.zeros(5, np.int32)
    E.emu_sgbm_geom(W, m, n, g.ctypes.data)
    xlo, xhi = R.valid_columns(W, p)
    assert (g[0], g[1], g[2], g[3], g[4]) == (xlo, xhi, xhi - xlo, p.Dmax, p.filtered) and E.emu_sgbm_ft(cap) == p.ft
    W1 = max(xhi - xlo, 0)
    for L, Rr in pairs(case, 12):
        GL, GR = np.empty_like(L), np.empty_like(Rr)
        for ft in (15, 63, p.ft):
            E.emu_sgbm_prefilter(L.ctypes.data, W, H, ft, GL.ctypes.data)
            assert np.array_equal(GL, R.prefilter_np(L, ft)), ft
        E.emu_sgbm_prefilter(Rr.ctypes.data, W, H, p.ft, GR.ctypes.data)
        if W1 == 0:
            continue
        st = {}
        R.compute_np(L, Rr, p, st)
        pc = np.zeros((H, W1, n), np.int32)
        E.emu_sgbm_pixel_cost(GL.ctypes.data, GR.ctypes.data, L.ctypes.data, Rr.ctypes.data, W, H, m, n, pc.ctypes.data)
        assert np.array_equal(pc, st["pc"])
        C = np.zeros_like(pc)
        E.emu_sgbm_block_cost(pc.ctypes.data, W1, H, n, w, C.ctypes.data)
        assert np.array_equal(C, st["C"])
        for md in (R.MODE_SGBM, R.MODE_HH, R.MODE_HH4):
            S, visits = np.zeros_like(C), np.zeros((len(R.DIRECTIONS[md]), H, W1), np.int32)
            E.emu_sgbm_aggregate(C.ctypes.data, W1, H, n, P1, P2, md, S.ctypes.data, visits.ctypes.data)
            assert (visits == 1).all(), "every pixel lies on exactly one path of a direction"
            assert np.array_equal(S, R.aggregate_np(C, p._replace(mode=md))), md
        S = np.ascontiguousarray(st["S"].astype(np.int32))
        d, win = np.zeros((H, W1), np.int32), np.zeros((H, W1), np.uint32)
        E.emu_sgbm_decide(S.ctypes.data, W1, H, m, n, uniq, d.ctypes.data, win.ctypes.data)
        assert np.array_equal(d, st["d"])
        assert np.array_equal(win != 0xffffffff, st["kept"])
        k = st["kept"]
        assert np.array_equal((win >> 8)[k], st["ms"][k]) and np.array_equal((win & 255)[k], st["best"][k])
        for mx in (-1, 0, 1, 3):
            want = R.left_right_np(st["d"], st["best"], st["ms"], st["kept"], W, p._replace(disp12MaxDiff=mx))
            for stride in (1, 5, 7):
                if np.gcd(stride, W1) != 1:
                    continue
                out = np.zeros((H, W1), np.int32)
                E.emu_sgbm_leftright(d.ctypes.data, win.ctypes.data, W, H, m, n, mx, stride, out.ctypes.data)
                assert np.array_equal(out, want), (mx, stride)
    assert E.emu_sgbm_disparity16(5, 10, 21, 40, 16, 0) == 77 and E.emu_sgbm_disparity16(5, 10, 40, 21, 16, 0) == 84


LIMITS = {"sgbm_max_dim": 16384, "sgbm_max_disparities": 256, "sgbm_max_cost": 32767, "sgbm_max_scratch_mib": 16384, "sgbm_tile_cols": 64, "sgbm_strip_rows": 32,
          "sgbm_chunk": 16, "sgbm_path_block": 16}


def test_limits_are_pinned():
    """how far StereoSGBM was built; tests/test_sgbm_gpu.py derives its shapes from mi355cv_limit"""
    from opencv_amd import _lib
    E = emu()
    for i, (k, v) in enumerate(LIMITS.items()):
        assert _lib.limit(k) == v == E.emu_sgbm_limit(i), k
    # 4K at 256 disparities is served: 3840 - 255 valid columns
    need = E.emu_sgbm_frame_scratch(3840, 2160, 3840 - 255, 256)
    assert 3585 * 2160 * 256 * 6 <= need <= LIMITS["sgbm_max_scratch_mib"] << 20
    assert need < 12 << 30


def test_the_sixteen_bit_bound():
    """w^2 (2 ft + 63) + P2 <= 32767 with ft = max(preFilterCap, 15) | 1.  ft = 15: 93 per pixel, w = 17 gives 26 877 (+ P2 up to 5890), w = 19 gives 33 573: declined.
    ft = 63: 189 per pixel, w = 13 gives 31 941, w = 15 gives 42 525"""
    E = emu()
    assert [E.emu_sgbm_ft(c) for c in (0, 14, 15, 16, 31, 62, 63, 64)] == [15, 15, 15, 17, 31, 63, 63, 65]
    assert E.emu_sgbm_bound(17, 15, 0) == 26877 and E.emu_sgbm_bound(19, 15, 0) == 33573 and E.emu_sgbm_bound(13, 63, 0) == 31941 and E.emu_sgbm_bound(15, 63, 0) == 42525
    assert E.emu_sgbm_bound(5, 63, 800) == 25 * 189 + 800 == R.cost_bound(R.Params(0, 16, 5, 200, 800, preFilterCap=63))
    assert E.emu_sgbm_bound(181, 65535, 2 ** 31 - 1) == 181 * 181 * (2 * 65535 + 63) + 2 ** 31 - 1      # no overflow on the way


def test_refusals_before_a_device_is_touched():
    import opencv_amd as cv
    from opencv_amd import _lib
    from opencv_amd.calib3d import StereoSGBMParams
    Lb, NI, top = _lib.lib, _lib.NOT_IMPLEMENTED, _lib.limit
    reason = lambda: Lb.mi355cv_lastError().decode()
    img = np.zeros((64, 96), np.uint8)
    out = np.full((64, 96), 1234, np.int16)

    def call(W=96, H=64, depth=3, lstep=96, rstep=96, dstep=192, batch=None, **kw):
        P = StereoSGBMParams()
        Lb.mi355cv_stereoSGBMDefaults(ctypes.byref(P))
        for k, v in kw.items():
            setattr(P, k, v)
        if batch is not None:
            return Lb.mi355cv_stereoSGBMBatch(img.ctypes.data, lstep, 64 * 96, img.ctypes.data, rstep, 64 * 96, out.ctypes.data, dstep, 64 * 192, batch, W, H, depth, ctypes.byref(P))
        return Lb.mi355cv_stereoSGBM(img.ctypes.data, lstep, img.ctypes.data, rstep, out.ctypes.data, dstep, W, H, depth, ctypes.byref(P))

    cases = [
        (dict(mode=cv.StereoSGBM_MODE_SGBM_3WAY), "MODE_SGBM_3WAY is not served"), (dict(mode=4), "none of MODE_SGBM"), (dict(mode=-1), "none of MODE_SGBM"),
        (dict(depth=2), "neither CV_16SC1 nor CV_32FC1"), (dict(depth=4), "neither CV_16SC1 nor CV_32FC1"),
        (dict(numDisparities=24), "n % 16 != 0"), (dict(numDisparities=0), "n < 16"), (dict(numDisparities=-16), "n < 16"),
        (dict(numDisparities=top("sgbm_max_disparities") + 16), "SGBM_MAX_DISPARITIES"),
        (dict(blockSize=4), "w % 2 == 0"), (dict(blockSize=0), "w < 1"), (dict(blockSize=-3), "w < 1"),
        (dict(preFilterCap=-1), "preFilterCap < 0"),
        (dict(P1=-1), "P1 < 0"), (dict(P1=9, P2=8), "P2 < p->P1"),
        (dict(uniquenessRatio=-1), "uniquenessRatio < 0"), (dict(uniquenessRatio=101), "uniquenessRatio > 100"),
        (dict(speckleWindowSize=-1), "speckleWindowSize < 0"), (dict(speckleRange=-1), "speckleRange < 0"),
        (dict(blockSize=19), "SGBM_MAX_COST"), (dict(blockSize=17, P2=5891), "SGBM_MAX_COST"), (dict(blockSize=15, preFilterCap=63), "SGBM_MAX_COST"),
        (dict(blockSize=3, P2=32767), "SGBM_MAX_COST"), (dict(blockSize=3, preFilterCap=2 ** 31 - 1), "SGBM_MAX_COST"), (dict(blockSize=46341), "SGBM_MAX_COST"),
        (dict(W=top("sgbm_max_dim") + 1, lstep=1 << 15, rstep=1 << 15, dstep=1 << 16), "SGBM_MAX_DIM"), (dict(H=top("sgbm_max_dim") + 1), "SGBM_MAX_DIM"),
        (dict(minDisparity=-2048), "range of a CV_16S map"), (dict(minDisparity=2040), "range of a CV_16S map"),
        (dict(lstep=95), "lstep < (size_t)W"), (dict(rstep=95), "rstep < (size_t)W"), (dict(dstep=190), "dstep < (size_t)W * esz"),
        (dict(depth=5, dstep=192), "dstep < (size_t)W * esz"), (dict(dstep=193), "off their element's boundary"),
        (dict(batch=0), "nframes < 1"), (dict(batch=-3), "nframes < 1"), (dict(batch=2, lstep=95), "left_step < (size_t)width"),
    ]
    for kw, why in cases:
        assert call(**kw) == NI, kw
        assert why in reason(), (kw, reason())
    assert (out == 1234).all()
    # the scratch bound, lowered: one 64 x 96 frame at n = 16 takes 81 valid columns x 64 x 16 x 6 bytes and more
    assert Lb.mi355cv_stereoSGBMSetScratchLimit(81 * 64 * 16 * 6) == 0
    try:
        assert call() == NI and "SGBM_MAX_SCRATCH_BYTES" in reason()
    finally:
        Lb.mi355cv_stereoSGBMSetScratchLimit(0)
    assert (out == 1234).all()
    assert Lb.mi355cv_stereoSGBMSetKernel(2) == -1 and Lb.mi355cv_stereoSGBMSetKernel(-2) == -1
    assert Lb.mi355cv_stereoSGBMSetKernel(0) == 0 and Lb.mi355cv_stereoSGBMSetKernel(1) == 0 and Lb.mi355cv_stereoSGBMSetKernel(-1) == 0
    # the Python mirror: the reference's defaults, getters and setters, and its own argument errors
    sg = cv.StereoSGBM_create()
    get = lambda o: (o.getMinDisparity(), o.getNumDisparities(), o.getBlockSize(), o.getP1(), o.getP2(), o.getDisp12MaxDiff(), o.getPreFilterCap(), o.getUniquenessRatio(),
                     o.getSpeckleWindowSize(), o.getSpeckleRange(), o.getMode())
    assert get(sg) == (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, cv.StereoSGBM_MODE_SGBM)
    sg = cv.StereoSGBM_create(-4, 32, 5, 8, 32, 2, 31, 10, 100, 2, cv.StereoSGBM_MODE_HH)
    assert get(sg) == (-4, 32, 5, 8, 32, 2, 31, 10, 100, 2, 1)
    sg.setMinDisparity(3); sg.setNumDisparities(48); sg.setBlockSize(7); sg.setP1(1); sg.setP2(2); sg.setDisp12MaxDiff(-1); sg.setPreFilterCap(9); sg.setUniquenessRatio(5)
    sg.setSpeckleWindowSize(0); sg.setSpeckleRange(1); sg.setMode(cv.StereoSGBM_MODE_HH4)
    assert get(sg) == (3, 48, 7, 1, 2, -1, 9, 5, 0, 1, 3)
    assert (cv.StereoSGBM_MODE_SGBM, cv.StereoSGBM_MODE_HH, cv.StereoSGBM_MODE_SGBM_3WAY, cv.StereoSGBM_MODE_HH4) == (0, 1, 2, 3)
    assert (cv.StereoSGBM.MODE_SGBM, cv.StereoSGBM.MODE_HH, cv.StereoSGBM.MODE_SGBM_3WAY, cv.StereoSGBM.MODE_HH4) == (0, 1, 2, 3)
    assert not hasattr(sg, "getTextureThreshold") and not hasattr(sg, "getROI1") and sg.getDefaultName() == "StereoMatcher.SGBM"
    with pytest.raises(NotImplementedError, match="inputs must be CV_8UC1"):
        sg.compute(np.zeros((64, 96), np.uint16), np.zeros((64, 96), np.uint16))
    with pytest.raises(NotImplementedError, match="inputs must be CV_8UC1"):
        sg.compute(np.zeros((64, 96, 3), np.uint8), np.zeros((64, 96, 3), np.uint8))
    with pytest.raises(NotImplementedError, match="neither CV_16SC1 nor CV_32FC1"):
        sg.compute(img, img, disp=np.zeros((64, 96), np.int32))
    with pytest.raises(ValueError, match="same size"):
        sg.compute(img, img[:, :90])
    with pytest.raises(ValueError, match="shape of the inputs"):
        sg.compute(img, img, disp=np.zeros((64, 90), np.int16))
    # the decline ledger counts the mirror's refusals and the library's under the entry
    n0, b0 = _lib.decline_count("stereoSGBM"), _lib.decline_count("stereoSGBMBatch")
    with pytest.raises(NotImplementedError, match="MODE_SGBM_3WAY"):
        cv.StereoSGBM_create(mode=cv.StereoSGBM_MODE_SGBM_3WAY).compute(img, img)
    with pytest.raises(NotImplementedError, match="inputs must be CV_8UC1"):
        sg.compute(img.astype(np.float32), img.astype(np.float32))
    with pytest.raises(NotImplementedError, match="P2 < p->P1"):
        cv.StereoSGBM_create(P1=5, P2=4).computeBatch(np.stack([img, img]), np.stack([img, img]))
    assert (_lib.decline_count("stereoSGBM"), _lib.decline_count("stereoSGBMBatch")) == (n0 + 2, b0 + 1)


def test_params_layout(tmp_path):
    """mi355cv_StereoSGBMParams as a C compiler lays it out from include/mi355cv.h against the ctypes mirror"""
    from opencv_amd.calib3d import StereoSGBMParams
    names = [f for f, _ in StereoSGBMParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355cv.h"\nint main(void) { printf("%zu", sizeof(mi355cv_StereoSGBMParams));\n'
                   + "".join('printf(" %%zu", offsetof(mi355cv_StereoSGBMParams, %s));\n' % n for n in names) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(StereoSGBMParams)] + [getattr(StereoSGBMParams, n).offset for n in names]
    assert got[0] == 11 * 4 and names == ["minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap", "uniquenessRatio", "speckleWindowSize",
                                          "speckleRange", "mode"]


def test_stereobm_is_as_it_was():
    """the matcher base the two mirrors now share changes nothing StereoBM shows: its entries, its accessors, its ROI methods, and speckleWindowSize > 0 still declined"""
    import opencv_amd as cv
    from opencv_amd import _lib
    bm = cv.StereoBM_create(16, 9)
    assert (bm._single, bm._batch, bm.getDefaultName()) == ("stereoBM", "stereoBMBatch", "StereoMatcher.BM")
    assert (bm.getTextureThreshold(), bm.getPreFilterType(), bm.getROI1()) == (10, cv.PREFILTER_XSOBEL, (0, 0, 0, 0)) and not hasattr(bm, "getP1")
    bm.setSpeckleWindowSize(5)
    img = np.zeros((64, 96), np.uint8)
    with pytest.raises(NotImplementedError, match="stereoBM"):
        bm.compute(img, img)
    assert "cv::filterSpeckles is not served" in _lib.lib.mi355cv_lastError().decode()
