"""distanceTransform without a GPU: the restatement (tests/disttransform_restate.py) against scipy and against known answers, the lines of
opencv_amd/csrc/disttransform_math.h compiled for the host (tests/hostemu/disttransform_emu.cpp) against that restatement, and the argument refusals of
mi355cv_distanceTransform / mi355cv_distanceTransformBatch that come before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

import disttransform_restate as R
import emubuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_IMPLEMENTED = 1
CV_8U, CV_8S, CV_16U, CV_32F, CV_64F = 0, 1, 2, 5, 6
METRICS = (R.DIST_L1, R.DIST_L2, R.DIST_C)


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


def random_mask(rng, h, w, density):
    return np.where(rng.random((h, w)) < density, 0, rng.integers(1, 256, (h, w))).astype(np.uint8)


# ---- the restatement itself
def test_known_answers():
    a = np.full((5, 5), 255, np.uint8)
    a[2, 2] = 0
    d1 = [[4, 3, 2, 3, 4], [3, 2, 1, 2, 3], [2, 1, 0, 1, 2], [3, 2, 1, 2, 3], [4, 3, 2, 3, 4]]
    dc = [[2, 2, 2, 2, 2], [2, 1, 1, 1, 2], [2, 1, 0, 1, 2], [2, 1, 1, 1, 2], [2, 2, 2, 2, 2]]
    d2 = [[8, 5, 4, 5, 8], [5, 2, 1, 2, 5], [4, 1, 0, 1, 4], [5, 2, 1, 2, 5], [8, 5, 4, 5, 8]]
    assert np.array_equal(R.distanceTransform(a, R.DIST_L1), np.array(d1, np.float32))
    assert np.array_equal(R.distanceTransform(a, R.DIST_C), np.array(dc, np.float32))
    assert np.array_equal(R.distanceTransform(a, R.DIST_L2), np.sqrt(np.array(d2, np.float64)).astype(np.float32))
    assert R.distanceTransform(a, R.DIST_L2)[0, 0] == np.float32(2.8284271)
    assert np.array_equal(R.distanceTransform(a, R.DIST_L1, np.uint8), np.array(d1, np.uint8))


def test_long_row_roots_in_double():
    """1 x 5000 with the site at x = 0: d2 = x^2 passes 2^24 at x = 4096, where the cast to float would round before the root"""
    a = np.full((1, 5000), 1, np.uint8)
    a[0, 0] = 0
    got = R.distanceTransform(a, R.DIST_L2)
    assert got.dtype == np.float32 and np.array_equal(got[0], np.arange(5000, dtype=np.float32))
    d2 = np.arange(5000, dtype=np.int64) ** 2
    assert int(d2[-1]) > 1 << 24
    assert np.array_equal(R.integer(a, R.DIST_L2)[0], d2)
    # an exact integer above 2^24 that is no float: the root of the rounded value differs from the rounded root of the exact one somewhere in this range
    v = np.arange((1 << 24), (1 << 24) + 200000, dtype=np.int64)
    assert (np.sqrt(v.astype(np.float32)) != np.sqrt(v.astype(np.float64)).astype(np.float32)).any()


def test_l1_into_8u_saturates():
    a = np.full((1, 300), 7, np.uint8)
    a[0, 0] = 0
    got = R.distanceTransform(a, R.DIST_L1, np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got[0], np.minimum(np.arange(300), 255))
    assert np.array_equal(R.distanceTransform(a, R.DIST_L1)[0], np.arange(300, dtype=np.float32))


def test_frame_without_a_site():
    a = np.full((3, 4), 9, np.uint8)
    for m in METRICS:
        got = R.distanceTransform(a, m)
        assert got.dtype == np.float32 and np.all(got == np.float32(31622776.0))
    assert np.all(R.distanceTransform(a, R.DIST_L1, np.uint8) == 255)
    assert np.float32(31622776.0) == np.sqrt(np.float32(1e15))
    assert R.brute(a, R.DIST_L2) is None and R.separable(a, R.DIST_L2) is None


def test_the_two_searches_agree():
    rng = np.random.default_rng(1)
    for h, w, dens in ((1, 1, 1.0), (1, 9, 0.3), (9, 1, 0.3), (13, 17, 0.5), (13, 17, 0.03), (40, 31, 0.01), (31, 40, 0.2)):
        a = random_mask(rng, h, w, dens)
        a[rng.integers(h), rng.integers(w)] = 0
        for m in METRICS:
            assert np.array_equal(R.brute(a, m), R.separable(a, m)), (h, w, dens, m)


def test_restatement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    shapes = [(1, 1), (1, 2), (2, 1), (1, 37), (37, 1), (5, 7), (16, 16), (33, 65), (64, 130), (100, 100), (300, 300)]
    for i, (h, w) in enumerate(shapes):
        a = random_mask(rng, h, w, (0.5, 0.05, 0.005)[i % 3])
        a[rng.integers(h), rng.integers(w)] = 0                                            # scipy has no rule for a mask without a site
        assert np.array_equal(R.distanceTransform(a, R.DIST_L2), ndi.distance_transform_edt(a).astype(np.float32)), (h, w)
        assert np.array_equal(R.integer(a, R.DIST_L1), ndi.distance_transform_cdt(a, "taxicab")), (h, w)
        assert np.array_equal(R.integer(a, R.DIST_C), ndi.distance_transform_cdt(a, "chessboard")), (h, w)


# ---- disttransform_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("disttransform_emu.cpp", "libdisttransform_emu.so", ["-ffp-contract=off"])
    lib.emu_disttransform.restype = ctypes.c_int
    lib.emu_disttransform.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.emu_dist_columns.restype = ctypes.c_int
    lib.emu_dist_columns.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.emu_dist_root.restype = None
    lib.emu_dist_root.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.emu_dist_cap.restype = ctypes.c_uint
    return lib


def _emu(emu, a, metric, dt=np.float32):
    h, w = a.shape
    got = np.empty((h, w), dt)
    assert emu.emu_disttransform(P(a), a.strides[0], P(got), got.strides[0], w, h, metric, CV_8U if dt == np.uint8 else CV_32F) == 0
    return got


def _check(emu, a):
    for m in METRICS:
        assert np.array_equal(_emu(emu, a, m), R.distanceTransform(a, m)), (a.shape, m)
    assert np.array_equal(_emu(emu, a, R.DIST_L1, np.uint8), R.distanceTransform(a, R.DIST_L1, np.uint8)), a.shape


def test_lines_are_the_restatement_on_random_masks(emu):
    rng = np.random.default_rng(3)
    # heights around one and two column segments of 64 rows, widths of every parity
    for h, w in ((1, 1), (1, 2), (2, 1), (1, 65), (65, 1), (7, 5), (63, 9), (64, 9), (65, 9), (127, 6), (128, 6), (129, 6), (37, 130), (200, 33)):
        for dens in (0.5, 0.03, 0.001):
            a = random_mask(rng, h, w, dens)
            _check(emu, a)                                                                # (a sparse one may hold no site at all: the sentinel)
            a[rng.integers(h), rng.integers(w)] = 0
            _check(emu, a)


def test_lines_on_the_patterns(emu):
    h, w = 70, 90
    for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):                        # the full scan radius
        a = np.full((h, w), 200, np.uint8)
        a[cy, cx] = 0
        _check(emu, a)
    _check(emu, np.zeros((h, w), np.uint8))                                               # every pixel a site
    _check(emu, np.full((h, w), 1, np.uint8))                                             # none
    a = np.full((h, w), 1, np.uint8); a[:, 17] = 0; _check(emu, a)                        # one column
    a = np.full((h, w), 1, np.uint8); a[66, :] = 0; _check(emu, a)                        # one row
    a = np.full((h, w), 1, np.uint8); a[3, 5] = 0; a[68, 80] = 0; _check(emu, a)


def test_capped_columns(emu):
    """columns without a site in a frame that has some: their column distance is CAP, above every real one, and the row pass still finds the true minimum"""
    rng = np.random.default_rng(4)
    h, w = 130, 40
    a = random_mask(rng, h, w, 0.05)
    a[:, 5:19] = 3
    a[:, 33] = 9
    a[64, 0] = 0
    g = np.empty((h, w), np.uint16)
    assert emu.emu_dist_columns(P(a), a.strides[0], P(g), w, h) == 0
    cap = emu.emu_dist_cap()
    assert cap == 32768 and cap > 2 * (R.MAX_DIM - 1) and cap * cap + (R.MAX_DIM - 1) ** 2 < 1 << 31 and 2 * (R.MAX_DIM - 1) ** 2 < cap * cap
    want = R.column_distance(a)
    assert np.all(g[:, 5:19] == cap) and np.all(g[:, 33] == cap)
    assert np.array_equal(np.where(g == cap, -1, g.astype(np.int64)), np.where(want >= (1 << 30), -1, want))
    _check(emu, a)


def test_root_is_the_correctly_rounded_one(emu):
    """root(d2) against np.sqrt(float64(d2)).astype(float32): every integer below 2^24 (the sqrtf branch), and the double branch from 2^24 up to the largest
    squared distance served"""
    def root(v):
        v = np.ascontiguousarray(v, np.uint32)
        out = np.empty(v.shape, np.float32)
        emu.emu_dist_root(P(v), P(out), v.size)
        return out
    v = np.arange(1 << 24, dtype=np.uint32)
    assert np.array_equal(root(v), np.sqrt(v.astype(np.float64)).astype(np.float32))
    rng = np.random.default_rng(5)
    top = 2 * (R.MAX_DIM - 1) ** 2
    v = np.concatenate([np.arange(1 << 24, (1 << 24) + 300000), rng.integers(1 << 24, top, 300000), [top, top - 1, 4999 ** 2, 16383 ** 2]]).astype(np.uint32)
    assert np.array_equal(root(v), np.sqrt(v.astype(np.float64)).astype(np.float32))


def test_long_lines(emu):
    for shape, at in (((1, 5000), (0, 0)), ((5000, 1), (4999, 0)), ((1, 5000), (0, 4999))):
        a = np.full(shape, 1, np.uint8)
        a[at] = 0
        _check(emu, a)
    a = np.full((1, 300), 7, np.uint8)
    a[0, 0] = 0
    assert np.array_equal(_emu(emu, a, R.DIST_L1, np.uint8)[0], np.minimum(np.arange(300), 255))


def test_emu_refuses_what_is_not_served(emu):
    a = np.zeros((4, 4), np.float32)
    assert emu.emu_disttransform(P(a), 16, P(a), 16, 4, 4, R.DIST_L2, CV_8U) == -1
    assert emu.emu_disttransform(P(a), 16, P(a), 16, 4, 4, 4, CV_32F) == -1
    assert emu.emu_disttransform(P(a), 16, P(a), 16, R.MAX_DIM + 1, 1, R.DIST_L2, CV_32F) == -1
    assert emu.emu_dist_seg() == 64 and emu.emu_dist_max_dim() == R.MAX_DIM


# ---- the C ABI's refusals that need no device
def test_header_symbols_are_bound():
    from opencv_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mi355cv.h")).read()
    for name in ("mi355cv_distanceTransform", "mi355cv_distanceTransformBatch"):
        assert name + "(" in txt and name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_width_bound_is_exposed_and_pinned():
    from opencv_amd import _lib
    assert _lib.limit(R.LIMIT_KEY) == 16384 == R.MAX_DIM
    # squared distances are 32-bit in the kernels: the largest one served stays below 2^30
    assert 2 * (_lib.limit(R.LIMIT_KEY) - 1) ** 2 < 1 << 30


def test_entry_declines_bad_arguments():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.zeros((16, 16), np.uint8)
    d = np.full((16, 16), 7, np.float32)
    d8 = np.full((16, 16), 7, np.uint8)
    names = (b"distanceTransform", b"distanceTransformBatch")
    n0 = sum(L.mi355cv_callCount(n) for n in names)
    one = lambda dist, mask, depth, dst=d, w=16, h=16: L.mi355cv_distanceTransform(P(a), 16, w, h, P(dst), dst.strides[0], dist, mask, depth)
    batch = lambda dist, mask, depth, nf=1, w=16, h=16: L.mi355cv_distanceTransformBatch(P(a), 16, 256, w, h, P(d), 64, 1024, nf, dist, mask, depth)
    reason = lambda: L.mi355cv_lastError().decode()
    for f in (one, batch):
        assert f(R.DIST_L2, 3, CV_32F) == NOT_IMPLEMENTED and "DIST_MASK_PRECISE" in reason()      # the chamfer approximations
        assert f(R.DIST_L2, 5, CV_32F) == NOT_IMPLEMENTED
        assert f(R.DIST_L2, 0, CV_8U) == NOT_IMPLEMENTED and "CV_8U output without DIST_L1" in reason()
        assert f(R.DIST_C, 3, CV_8U) == NOT_IMPLEMENTED
        assert f(R.DIST_L1, 3, CV_16U) == NOT_IMPLEMENTED and "dstDepth" in reason()
        assert f(R.DIST_L1, 3, CV_64F) == NOT_IMPLEMENTED
        assert f(R.DIST_L1, 3, CV_8S) == NOT_IMPLEMENTED
        for dist in (-1, 0, 4, 5, 6, 7):                                                             # DIST_USER, DIST_L12, DIST_FAIR, DIST_WELSCH, DIST_HUBER
            assert f(dist, 3, CV_32F) == NOT_IMPLEMENTED and "distanceType" in reason()
        assert f(R.DIST_L1, 7, CV_32F) == NOT_IMPLEMENTED and "maskSize" in reason()
        assert f(R.DIST_L2, 0, CV_32F, w=R.MAX_DIM + 1) == NOT_IMPLEMENTED and "DISTTRANSFORM_MAX_DIM" in reason()
        assert f(R.DIST_L2, 0, CV_32F, h=R.MAX_DIM + 1) == NOT_IMPLEMENTED
        assert f(R.DIST_L2, 0, CV_32F, w=0) == NOT_IMPLEMENTED
        assert f(R.DIST_L2, 0, CV_32F, h=-3) == NOT_IMPLEMENTED
    assert one(R.DIST_L1, 3, CV_8U, dst=d8, w=R.MAX_DIM + 1) == NOT_IMPLEMENTED
    assert batch(R.DIST_L2, 0, CV_32F, nf=0) == NOT_IMPLEMENTED and "nframes" in reason()
    assert L.mi355cv_distanceTransform(None, 16, 16, 16, P(d), 64, R.DIST_L2, 0, CV_32F) == NOT_IMPLEMENTED
    assert L.mi355cv_distanceTransform(P(a), 16, 16, 16, None, 64, R.DIST_L2, 0, CV_32F) == NOT_IMPLEMENTED
    assert L.mi355cv_distanceTransformBatch(None, 16, 256, 16, 16, P(d), 64, 1024, 1, R.DIST_L2, 0, CV_32F) == NOT_IMPLEMENTED
    assert sum(L.mi355cv_callCount(n) for n in names) == n0
    assert np.all(d == 7) and np.all(d8 == 7)
    assert not hasattr(L, "mi355cv_distanceTransformWithLabels")                                     # the labelled variant has no entry point


def test_python_api_refuses_what_the_reference_asserts_on():
    import opencv_amd as cv
    for name in ("distanceTransform", "distanceTransformBatch", "DIST_L1", "DIST_L2", "DIST_C", "DIST_MASK_3", "DIST_MASK_5", "DIST_MASK_PRECISE"):
        assert name in cv.imgproc.__all__ and hasattr(cv, name), name
    assert (cv.DIST_L1, cv.DIST_L2, cv.DIST_C, cv.DIST_MASK_3, cv.DIST_MASK_5, cv.DIST_MASK_PRECISE) == (1, 2, 3, 3, 5, 0)
    a = np.zeros((8, 8), np.uint8)
    for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8), np.uint16), np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.int8)):
        with pytest.raises(ValueError):
            cv.distanceTransform(bad, cv.DIST_L2, cv.DIST_MASK_PRECISE)
    with pytest.raises(ValueError):
        cv.distanceTransform(a, cv.DIST_L2, cv.DIST_MASK_PRECISE, dstType=cv.CV_8U)
    with pytest.raises(ValueError):
        cv.distanceTransform(a, cv.DIST_C, cv.DIST_MASK_3, dstType=cv.CV_8U)
    with pytest.raises(ValueError):
        cv.distanceTransform(a, cv.DIST_L1, cv.DIST_MASK_3, dstType=cv.CV_16U)
    with pytest.raises(ValueError):
        cv.distanceTransform(a, cv.DIST_L1, cv.DIST_MASK_3, dst=np.zeros((8, 9), np.float32))
    with pytest.raises(ValueError):
        cv.distanceTransformBatch(a, cv.DIST_L1, cv.DIST_MASK_3)
