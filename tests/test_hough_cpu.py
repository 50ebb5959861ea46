"""HoughLines without a GPU: the two restatements (tests/hough_restate.py) against known answers and against each other, the lines of
opencv_amd/csrc/hough_math.h compiled for the host (tests/hostemu/hough_emu.cpp) against them, the geometry's edge cases, and the argument refusals of the three
mi355cv_houghLines* entries that come before any device is touched."""
import ctypes
import math
import os

import numpy as np
import pytest

import emubuild
import hough_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_IMPLEMENTED = 0, 1
F = np.float32
PI = math.pi
GRID = [(rho, theta, win) for rho in R.RHOS for theta in R.THETAS for win in R.WINDOWS]


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- known answers
@pytest.mark.parametrize("vec", [False, True])
def test_one_pixel_votes_once_in_every_angle_row(vec):
    a = np.zeros((7, 9), np.uint8)
    a[3, 5] = 9
    acc, lines = R.hough(a, 1.0, PI / 180, 0, vec=vec)
    assert acc.shape == (182, 2 * 16 + 1 + 2) and acc.dtype == np.int32
    assert np.all(acc[1:-1].sum(axis=1) == 1) and not acc[0].any() and not acc[-1].any() and acc.max() == 1
    acc, lines = R.hough(a, 1.0, PI / 180, 0, min_theta=0.0, max_theta=PI / 360, vec=vec)
    assert acc.shape[0] == 3 and lines.tolist() == [[5.0, 0.0, 1.0]]        # one angle: the pixel's column


@pytest.mark.parametrize("vec", [False, True])
def test_full_column_and_full_row(vec):
    h, w, c = 12, 17, 5
    a = np.zeros((h, w), np.uint8)
    a[:, c] = 255
    _, lines = R.hough(a, 1.0, PI / 180, h - 1, vec=vec)
    assert lines[0].tolist() == [float(c), 0.0, float(h)]
    h, w = 12, 120                                                          # wide enough for the angles beside n = 90 to spread the row over several bins
    a = np.zeros((h, w), np.uint8)
    a[c, :] = 255
    acc, lines = R.hough(a, 1.0, PI / 180, w - 1, vec=vec)
    numrho = acc.shape[1] - 2
    assert acc[91, c + (numrho - 1) // 2 + 1] == w and len(lines) == 1
    assert lines[0, 0] == c and lines[0, 2] == w
    # theta is emitted as (float)min_theta + n * theta_f (step 8).  The table's own angle for n = 90 is the float SUM of 90 steps, which is not the same number:
    # each of its additions rounds by at most half an ulp of a value below 2 (2 ** -24), so the two are within 90 * 2 ** -24 of each other
    t = F(0)
    for _ in range(90):
        t = F(t + F(PI / 180))
    assert lines[0, 1] == F(0) + F(90) * F(PI / 180) and abs(float(lines[0, 1]) - float(t)) <= 90 * 2.0 ** -24
    assert acc[91].max() == w > acc[90].max() and w > acc[92].max()       # the table's angle for n = 90 is the one that keeps the whole row in one bin


# ---- the two restatements agree
def small_frames():
    rng = np.random.default_rng(1)
    return {"random 9 x 13": R.random_frame(rng, 9, 13, 0.3), "all 6 x 6": np.full((6, 6), 3, np.uint8), "1 x 1": np.ones((1, 1), np.uint8),
            "lines 12 x 15": R.drawn_lines(12, 15), "empty": np.zeros((4, 5), np.uint8)}


@pytest.mark.parametrize("rho,theta,win", GRID)
def test_restatements_agree_on_accumulator_and_lines(rho, theta, win):
    for name, a in small_frames().items():
        acc_l, acc_v = R.accum_loops(a, rho, theta, *win), R.accum_vec(a, rho, theta, *win)
        assert acc_l.shape == acc_v.shape and np.array_equal(acc_l, acc_v), name
        for thr in (0, int(acc_l.max()) // 2, int(acc_l.max())):
            ll, lv = R.lines_loops(acc_l, rho, theta, thr, win[0]), R.lines_vec(acc_v, rho, theta, thr, win[0])
            assert R.same_bits(ll, lv), (name, thr)
            assert thr < acc_l.max() or len(ll) == 0
            v = ll[:, 2]
            assert np.all(v[:-1] >= v[1:])                                  # votes descending


def test_tables_agree():
    for rho, theta, win in GRID:
        na, _ = R.geometry(45, 67, rho, theta, *win)
        sl, cl = R.table_loops(na, rho, theta, win[0])
        sv, cv_ = R.table_vec(na, rho, theta, win[0])
        assert R.same_bits(np.array(sl, F), sv) and R.same_bits(np.array(cl, F), cv_)


# ---- geometry
def test_geometry_edge_cases():
    # rho = 2: (2 (w + h) + 1) / 2 is an exact .5 and goes to the even neighbour
    assert R.geometry(45, 67, 2.0, PI / 180)[1] == 112                      # 225 / 2 = 112.5 -> 112
    assert R.geometry(46, 67, 2.0, PI / 180)[1] == 114                      # 227 / 2 = 113.5 -> 114
    assert R.geometry(45, 67, 1.0, PI / 180) == (180, 225)                  # [0, pi]: 181 angles, the last one dropped
    assert R.geometry(45, 67, 1.0, PI / 180, 0.0, PI / 2)[0] == 91          # [0, pi / 2]: kept
    assert R.geometry(45, 67, 1.0, PI / 7)[0] == 7 and R.geometry(45, 67, 1.0, PI / 90)[0] == 90
    assert R.geometry(45, 67, 0.5, PI / 180)[1] == 450 and R.geometry(45, 67, 3.0, PI / 180)[1] == 75
    assert R.geometry(1, 1, 1000.0, 1.0) == (3, 0) and R.half_of(0) == 0    # no distance bin at all


# ---- hough_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("hough_emu.cpp", "libhough_emu.so", ["-ffp-contract=off"])
    i32, dbl, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    lib.emu_hough_geometry.argtypes = [i32, i32, dbl, dbl, dbl, dbl, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.emu_hough_table.argtypes = [i32, i32, dbl, dbl, dbl, dbl, vp, vp]
    lib.emu_hough_accum.argtypes = [vp, ctypes.c_size_t, i32, i32, dbl, dbl, dbl, dbl, vp]
    lib.emu_hough_lines.argtypes = [vp, i32, i32, dbl, dbl, dbl, dbl, i32, i32, i32, vp]
    lib.emu_hough_cv_round.argtypes = [ctypes.c_float]
    lib.emu_hough_sort_key.argtypes = [i32, i32]
    lib.emu_hough_sort_key.restype = ctypes.c_uint64
    return lib


def emu_geometry(emu, w, h, rho, theta, lo=0.0, hi=PI):
    na, nr = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = emu.emu_hough_geometry(w, h, rho, theta, lo, hi, ctypes.byref(na), ctypes.byref(nr))
    return rc, na.value, nr.value


def test_emulated_constants_rounding_and_key(emu):
    assert (emu.emu_hough_max_dim(), emu.emu_hough_max_accum()) == (R.MAX_DIM, R.MAX_ACCUM)
    assert (emu.emu_hough_vote_chunk(), emu.emu_hough_vote_split(), emu.emu_hough_lds_bins()) == (R.VOTE_CHUNK, R.VOTE_SPLIT, R.LDS_BINS)
    for v, want in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (112.5, 112), (113.5, 114), (0.49999997, 0), (-2.5000002, -3)):
        assert emu.emu_hough_cv_round(v) == want == R.cv_round(v)
    keys = [emu.emu_hough_sort_key(v, b) for v, b in ((9, 7), (9, 8), (8, 1), (1, 0), (1, 1 << 25))]
    assert keys == sorted(keys) and keys[0] == ((~9 & 0xFFFFFFFF) << 32 | 7)


def test_emulated_geometry_and_its_refusals(emu):
    for w, h in ((1, 1), (45, 67), (46, 67), (512, 512), (3840, 2160)):
        for rho, theta, win in GRID:
            assert emu_geometry(emu, w, h, rho, theta, *win) == (0,) + R.geometry(w, h, rho, theta, *win)
    assert emu_geometry(emu, 1, 1, 1000.0, 1.0) == (0, 3, 0)
    for bad in ((0.0, 1.0, 0.0, PI), (-1.0, 1.0, 0.0, PI), (1.0, 0.0, 0.0, PI), (1.0, -0.1, 0.0, PI), (1.0, 1.0, -0.1, PI), (1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 2.0, 1.0),
                (1.0, 1.0, 0.0, PI + 1e-9), (float("nan"), 1.0, 0.0, PI), (1.0, float("nan"), 0.0, PI), (1e-60, 1.0, 0.0, PI)):
        assert emu_geometry(emu, 45, 67, *bad)[0] == 1, bad
    assert emu_geometry(emu, 45, 67, 1e-6, 1.0)[0] == 2 and emu_geometry(emu, 45, 67, 1.0, 1e-9)[0] == 2      # an accumulator past the bound
    assert emu_geometry(emu, 3840, 2160, 0.25, PI / 720)[0] == 0                                             # the header's example is inside it


def emu_hough(emu, a, rho, theta, thr, win, cn=3, max_lines=None):
    a = np.ascontiguousarray(a)
    h, w = a.shape
    na, nr = R.geometry(w, h, rho, theta, *win)
    acc = np.full((na + 2, nr + 2), -7, np.int32)
    assert emu.emu_hough_accum(P(a), a.strides[0], w, h, rho, theta, win[0], win[1], P(acc)) == int((a != 0).sum())
    cap = max_lines if max_lines is not None else max(1, na * ((nr + 1) // 2))
    lines = np.full((cap, cn), -7.0, F)
    n = emu.emu_hough_lines(P(acc), w, h, rho, theta, win[0], win[1], thr, cn, cap, P(lines))
    return acc, n, lines


@pytest.mark.parametrize("rho,theta,win", GRID)
def test_emulated_kernels_match_the_restatement(emu, rho, theta, win):
    rng = np.random.default_rng(2)
    frames = list(small_frames().values()) + [R.random_frame(rng, 45, 67, 0.1), R.drawn_lines(37, 64), np.full((16, 16), 1, np.uint8), R.random_frame(rng, 1, 37, 0.5),
                                              R.random_frame(rng, 37, 1, 0.5)]
    for a in frames:
        want_acc, want = R.hough(a, rho, theta, 0, *win)
        top = int(want_acc.max())
        for thr in (0, top // 2, top):
            acc, n, lines = emu_hough(emu, a, rho, theta, thr, win)
            want = R.lines_vec(want_acc, rho, theta, thr, win[0])
            assert np.array_equal(acc, want_acc) and n == len(want) and R.same_bits(lines[:n], want), (a.shape, thr)
            assert np.all(lines[n:] == -7.0)


def test_emulated_table_matches(emu):
    for rho, theta, win in GRID:
        na, _ = R.geometry(45, 67, rho, theta, *win)
        s, c = np.zeros(na, F), np.zeros(na, F)
        assert emu.emu_hough_table(45, 67, rho, theta, win[0], win[1], P(s), P(c)) == na
        sv, cv_ = R.table_vec(na, rho, theta, win[0])
        assert R.same_bits(s, sv) and R.same_bits(c, cv_)


def test_emulated_two_floats_and_a_short_list(emu):
    a = R.drawn_lines(37, 64)
    want = R.hough(a, 1.0, PI / 180, 5)[1]
    assert len(want) > 4
    acc, n, lines = emu_hough(emu, a, 1.0, PI / 180, 5, (0.0, PI), cn=2, max_lines=4)
    assert n == len(want) and R.same_bits(lines, want[:4, :2])


def test_votes_that_leave_their_row_follow_the_flat_index(emu):
    """rho far above the frame: numrho is 0 or 1 and a vote can land in the padding column or in a neighbouring row, as the reference's flat index would"""
    rng = np.random.default_rng(3)
    a = R.random_frame(rng, 9, 13, 0.5)
    for rho in (30.0, 45.0, 100.0, 1000.0):
        for theta in (PI / 7, PI / 90):
            acc_l, acc_v = R.accum_loops(a, rho, theta), R.accum_vec(a, rho, theta)
            acc, n, lines = emu_hough(emu, a, rho, theta, 0, (0.0, PI))
            assert np.array_equal(acc_l, acc_v) and np.array_equal(acc, acc_v)
            assert n == len(R.lines_vec(acc_v, rho, theta, 0))


# ---- the C ABI's refusals that need no device
ENTRIES = ("mi355cv_houghLines", "mi355cv_houghLinesBatch", "mi355cv_houghLinesAccum")
COUNTERS = (b"houghLines", b"houghLinesBatch", b"houghLinesAccum")


def test_header_symbols_are_bound():
    from opencv_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mi355cv.h")).read()
    for name in ENTRIES:
        assert name + "(" in txt and name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_bounds_are_exposed_and_pinned():
    from opencv_amd import _lib
    assert _lib.limit(R.MAX_DIM_KEY) == 16384 == R.MAX_DIM and _lib.limit(R.MAX_DIM_KEY) <= 65535
    assert _lib.limit(R.MAX_ACCUM_KEY) == 1 << 26 == R.MAX_ACCUM
    assert R.MAX_DIM * R.MAX_DIM <= 1 << 28 and 2 * (2 * R.MAX_DIM) + 1 < 1 << 24     # counts in 32 bits, float(2 (w + h) + 1) exact
    assert R.LDS_BINS * 4 <= 64 << 10


def test_entries_decline_bad_arguments_before_a_device_is_touched():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.ones((16, 16), np.uint8)
    lines = np.full((8, 3), 7.0, F)
    acc = np.full((182, 67), 7, np.int32)
    nl = (ctypes.c_int * 2)(-5, -5)
    na, nr = ctypes.c_int(-5), ctypes.c_int(-5)
    n0 = sum(L.mi355cv_callCount(n) for n in COUNTERS)
    big = _lib.limit(R.MAX_DIM_KEY) + 1

    def one(src=a, w=16, h=16, dst=lines, cn=2, cap=8, rho=1.0, theta=PI / 180, thr=1, srn=0.0, stn=0.0, lo=0.0, hi=PI, n=nl):
        return L.mi355cv_houghLines(P(src) if src is not None else None, 16, w, h, P(dst) if dst is not None else None, cn, cap, rho, theta, thr, srn, stn, lo, hi, n)

    def batch(src=a, w=16, h=16, dst=lines, cn=2, cap=4, rho=1.0, theta=PI / 180, thr=1, srn=0.0, stn=0.0, lo=0.0, hi=PI, n=nl, nf=2, lf=48):
        return L.mi355cv_houghLinesBatch(P(src) if src is not None else None, 16, 128, w, h, P(dst) if dst is not None else None, cn, cap, lf, nf, rho, theta, thr, srn, stn,
                                         lo, hi, n)

    def accum(src=a, w=16, h=16, dst=acc, rho=1.0, theta=PI / 180, lo=0.0, hi=PI, step=67 * 4, pa=ctypes.byref(na), pr=ctypes.byref(nr), **_):
        return L.mi355cv_houghLinesAccum(P(src) if src is not None else None, 16, w, h, rho, theta, lo, hi, P(dst) if dst is not None else None, step, pa, pr)

    reason = lambda: L.mi355cv_lastError().decode()
    for f in (one, batch, accum):
        assert f(rho=0.0) == NOT_IMPLEMENTED and "rho" in reason()
        assert f(rho=-1.0) == NOT_IMPLEMENTED and f(theta=0.0) == NOT_IMPLEMENTED and f(theta=-0.5) == NOT_IMPLEMENTED and "theta" in reason()
        assert f(lo=-0.1) == NOT_IMPLEMENTED and f(hi=PI + 1e-6) == NOT_IMPLEMENTED and f(lo=1.0, hi=1.0) == NOT_IMPLEMENTED and f(lo=2.0, hi=1.0) == NOT_IMPLEMENTED
        assert "min_theta" in reason()
        assert f(src=None) == NOT_IMPLEMENTED and "src" in reason()
        assert f(w=0) == NOT_IMPLEMENTED and f(h=-2) == NOT_IMPLEMENTED and f(w=big) == NOT_IMPLEMENTED and f(h=big) == NOT_IMPLEMENTED and "HOUGH_MAX_DIM" in reason()
        assert f(rho=1e-6) == NOT_IMPLEMENTED and "HOUGH_MAX_ACCUM" in reason()
        assert f(theta=1e-9) == NOT_IMPLEMENTED and "HOUGH_MAX_ACCUM" in reason()
    for f in (one, batch):
        assert f(srn=1.0) == NOT_IMPLEMENTED and "srn" in reason()
        assert f(stn=2.0) == NOT_IMPLEMENTED and "multi-scale" in reason()
        assert f(dst=None) == NOT_IMPLEMENTED and "lines" in reason()
        assert f(n=None) == NOT_IMPLEMENTED and "nlines" in reason()
        for cn in (0, 1, 4):
            assert f(cn=cn) == NOT_IMPLEMENTED and "lines_cn" in reason()
        assert f(cap=0) == NOT_IMPLEMENTED and f(cap=-1) == NOT_IMPLEMENTED and "max_lines" in reason()
    assert batch(nf=0) == NOT_IMPLEMENTED and "nframes" in reason()
    assert batch(lf=8) == NOT_IMPLEMENTED and batch(lf=49) == NOT_IMPLEMENTED and "lines_frame_stride" in reason()
    assert accum(step=66 * 4) == NOT_IMPLEMENTED and accum(step=67 * 4 + 2) == NOT_IMPLEMENTED and "accum_step" in reason()
    assert accum(pa=None) == NOT_IMPLEMENTED and accum(pr=None) == NOT_IMPLEMENTED and "numangle" in reason()
    assert sum(L.mi355cv_callCount(n) for n in COUNTERS) == n0
    assert np.all(lines == 7.0) and np.all(acc == 7) and list(nl) == [-5, -5] and (na.value, nr.value) == (-5, -5)
    # the geometry alone needs no device either
    assert accum(dst=None) == OK and (na.value, nr.value) == (180, 65)
    assert accum(dst=None, lo=0.0, hi=PI / 2, rho=2.0) == OK and (na.value, nr.value) == (91, 32)           # 65 / 2 = 32.5 -> 32


def test_python_api_refuses_bad_arguments():
    import opencv_amd as cv
    for name in ("HoughLines", "HoughLinesWithAccumulator", "HoughLinesBatch", "HoughLinesAccumulator"):
        assert name in cv.imgproc.__all__ and hasattr(cv, name), name
    a = np.zeros((8, 8), np.uint8)
    n0 = cv._lib.decline_count()
    for fn in (cv.HoughLines, cv.HoughLinesWithAccumulator):
        for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8), np.uint16), np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 1), np.uint8), np.zeros((8, 8), np.int8)):
            with pytest.raises(ValueError):
                fn(bad, 1, PI / 180, 10)
        for kw in (dict(rho=0), dict(rho=-1), dict(theta=0), dict(theta=float("nan")), dict(min_theta=-0.1), dict(max_theta=4.0), dict(min_theta=1.0, max_theta=1.0),
                   dict(srn=-1), dict(stn=-1), dict(maxLines=0)):
            args = dict(rho=1, theta=PI / 180, threshold=10)
            args.update(kw)
            with pytest.raises(ValueError):
                fn(a, **args)
    with pytest.raises(ValueError):
        cv.HoughLinesBatch(a, 1, PI / 180, 10)
    with pytest.raises(ValueError):
        cv.HoughLinesAccumulator(a, 0, PI / 180)
    assert cv._lib.decline_count() == n0                                    # nothing reached the library
    with pytest.raises(NotImplementedError, match="multi-scale"):
        cv.HoughLines(a, 1, PI / 180, 10, srn=2)
