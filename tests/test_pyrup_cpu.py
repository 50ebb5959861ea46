"""pyrUp without a GPU: the known answers of the restatement (tests/pyrup_restate.py), the lines of opencv_amd/csrc/pyrup_math.h compiled for the host
(tests/hostemu/pyrup_emu.cpp) against that restatement, and the argument refusals of mi355cv_pyrup / mi355cv_pyrupBatch that come before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

import emubuild
import orc
import pyrup_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_IMPLEMENTED = 1
DEPTH = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 2, np.dtype(np.int16): 3, np.dtype(np.float32): 5}


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- the restatement itself
def test_known_answers():
    for dt in (np.uint8, np.uint16, np.int16, np.float32):
        assert np.all(R.pyrUp(np.full((3, 4), 77, dt)) == 77)                    # a constant image stays constant
    a = np.zeros((5, 5), np.uint8)
    a[2, 2] = 255
    got = R.pyrUp(a)
    want = np.zeros((10, 10), np.uint8)
    want[2:7, 2:7] = [[4, 16, 24, 16, 4], [16, 64, 96, 64, 16], [24, 96, 143, 96, 24], [16, 64, 96, 64, 16], [4, 16, 24, 16, 4]]
    assert np.array_equal(got, want)
    assert np.array_equal(R.pyrUp(np.array([[10]], np.uint8)), np.full((2, 2), 10))
    assert np.array_equal(R.pyrUp(np.array([[0, 255]], np.uint8)), [[64, 128, 223, 255]] * 2)
    assert np.array_equal(R.pyrUp(np.array([[-32768, 32767, -1]], np.int16)), [[-16384, 0, 20479, 16383, 4095, -1]] * 2)
    assert R.pyrUp(np.zeros((3, 5, 3), np.uint16)).shape == (6, 10, 3)


# ---- pyrup_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("pyrup_emu.cpp", "libpyrup_emu.so", ["-ffp-contract=off"])
    lib.emu_pyrup.restype = ctypes.c_int
    lib.emu_pyrup.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.emu_pyrup_packed.restype = ctypes.c_int
    lib.emu_pyrup_packed.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
    return lib


SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (17, 9), (33, 4)]                # (w, h)


def data(rng, dt, shape, kind="full"):
    if dt == np.float32:
        return (rng.random(shape) if kind == "unit" else rng.uniform(-1000, 1000, shape)).astype(np.float32)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, shape).astype(dt)


def _emu(emu, src):
    h, w = src.shape[:2]
    cn = 1 if src.ndim == 2 else src.shape[2]
    got = np.empty((2 * h, 2 * w) + src.shape[2:], src.dtype)
    assert emu.emu_pyrup(P(src), src.strides[0], P(got), got.strides[0], w, h, DEPTH[src.dtype], cn) == 0
    return got


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.int16])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_integer_lines_are_the_restatement(emu, dt, cn):
    rng = np.random.default_rng(cn)
    for w, h in SIZES:
        src = data(rng, dt, (h, w) if cn == 1 else (h, w, cn))
        assert np.array_equal(_emu(emu, src), R.pyrUp(src)), (w, h)
        hi = np.full_like(src, np.iinfo(dt).max)
        lo = np.full_like(src, np.iinfo(dt).min)
        assert np.array_equal(_emu(emu, hi), hi.repeat(2, 0).repeat(2, 1)) and np.array_equal(_emu(emu, lo), lo.repeat(2, 0).repeat(2, 1))


@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("kind", ["unit", "pm1000"])
def test_float_lines_against_the_restatement(emu, cn, kind):
    rng = np.random.default_rng(10 + cn)
    for w, h in SIZES:
        src = data(rng, np.float32, (h, w) if cn == 1 else (h, w, cn), kind)
        assert orc.rel_err(_emu(emu, src), R.pyrUp(src)) <= 1e-6, (w, h)


def test_known_answers_of_the_lines(emu):
    """the answers of test_known_answers, on pyrup_math.h itself: the scalar lines (k_pyrup) and, for CV_8UC1, the packed ones (k_pyrup_roll)"""
    def packed(src):
        h, w = src.shape
        got = np.empty((2 * h, 2 * w), np.uint8)
        assert emu.emu_pyrup_packed(P(src), src.strides[0], P(got), got.strides[0], w, h) == 0
        return got
    a = np.zeros((5, 5), np.uint8)
    a[2, 2] = 255
    want = np.zeros((10, 10), np.uint8)
    want[2:7, 2:7] = [[4, 16, 24, 16, 4], [16, 64, 96, 64, 16], [24, 96, 143, 96, 24], [16, 64, 96, 64, 16], [4, 16, 24, 16, 4]]
    for f in (lambda x: _emu(emu, x), packed):
        assert np.all(f(np.full((3, 4), 77, np.uint8)) == 77)
        assert np.array_equal(f(a), want)
        assert np.array_equal(f(np.array([[10]], np.uint8)), np.full((2, 2), 10))
        assert np.array_equal(f(np.array([[0, 255]], np.uint8)), [[64, 128, 223, 255]] * 2)
    for dt in (np.uint16, np.int16, np.float32):
        assert np.all(_emu(emu, np.full((3, 4), 77, dt)) == 77)
    assert np.array_equal(_emu(emu, np.array([[-32768, 32767, -1]], np.int16)), [[-16384, 0, 20479, 16383, 4095, -1]] * 2)


def test_packed_lines_are_the_restatement(emu):
    """the 2 x u16 sums of k_pyrup_roll: random data, all-255 and a 0 / 255 checkerboard (the inputs that would carry between the halves)"""
    rng = np.random.default_rng(3)
    for w, h in SIZES + [(16, 7), (40, 3)]:
        yy, xx = np.mgrid[0:h, 0:w]
        for src in (data(rng, np.uint8, (h, w)), np.full((h, w), 255, np.uint8), (((xx + yy) & 1) * 255).astype(np.uint8), ((xx & 1) * 255).astype(np.uint8)):
            got = np.empty((2 * h, 2 * w), np.uint8)
            assert emu.emu_pyrup_packed(P(src), src.strides[0], P(got), got.strides[0], w, h) == 0
            assert np.array_equal(got, R.pyrUp(src)), (w, h)


def test_emu_refuses_other_depths(emu):
    a = np.zeros((4, 4), np.float64)
    assert emu.emu_pyrup(P(a), 32, P(a), 32, 2, 2, 6, 1) == -1
    assert emu.emu_pyrup(P(a), 32, P(a), 32, 2, 2, 0, 5) == -1


# ---- the C ABI's refusals that need no device
def test_entry_declines_bad_arguments():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.zeros((16, 16), np.uint8)
    d = np.zeros((40, 40), np.uint8)
    f = np.zeros((16, 16), np.float64)
    g = np.zeros((32, 32), np.float64)
    n0 = L.mi355cv_callCount(b"pyrup") + L.mi355cv_callCount(b"pyrupBatch")
    assert L.mi355cv_pyrup(P(f), 128, 16, 16, P(g), 256, 32, 32, 6, 1, 4) == NOT_IMPLEMENTED                  # CV_64F
    assert "depth" in L.mi355cv_lastError().decode()
    assert L.mi355cv_pyrup(P(a), 16, 16, 16, P(d), 40, 32, 32, 1, 1, 4) == NOT_IMPLEMENTED                    # CV_8S
    assert L.mi355cv_pyrup(P(a), 80, 16, 16, P(d), 160, 32, 32, 0, 5, 4) == NOT_IMPLEMENTED                   # cn 5
    assert L.mi355cv_pyrup(P(a), 16, 16, 16, P(d), 40, 33, 32, 0, 1, 4) == NOT_IMPLEMENTED                    # dst 2w + 1
    assert "dw != 2 * sw" in L.mi355cv_lastError().decode()
    assert L.mi355cv_pyrup(P(a), 16, 16, 16, P(d), 40, 32, 31, 0, 1, 4) == NOT_IMPLEMENTED                    # dst 2h - 1
    assert L.mi355cv_pyrup(P(a), 16, 16, 16, P(d), 40, 32, 32, 0, 1, 1) == NOT_IMPLEMENTED                    # BORDER_REPLICATE
    assert "border" in L.mi355cv_lastError().decode()
    assert L.mi355cv_pyrup(P(a), 16, 16, 16, P(d), 40, 32, 32, 0, 1, 0) == NOT_IMPLEMENTED                    # BORDER_CONSTANT
    assert L.mi355cv_pyrup(None, 16, 16, 16, P(d), 40, 32, 32, 0, 1, 4) == NOT_IMPLEMENTED                    # null pointers
    assert L.mi355cv_pyrup(P(a), 16, 16, 16, None, 40, 32, 32, 0, 1, 4) == NOT_IMPLEMENTED
    assert L.mi355cv_pyrup(P(a), 16, 0, 16, P(d), 40, 0, 32, 0, 1, 4) == NOT_IMPLEMENTED                      # empty image
    assert L.mi355cv_pyrup(P(a), 16, 16, -1, P(d), 40, 32, -2, 0, 1, 4) == NOT_IMPLEMENTED
    assert L.mi355cv_pyrupBatch(P(a), 16, 256, 16, 16, P(d), 40, 1600, 32, 32, 0, 0, 1, 4) == NOT_IMPLEMENTED   # no frames
    assert "nframes" in L.mi355cv_lastError().decode()
    assert L.mi355cv_pyrupBatch(P(f), 128, 2048, 16, 16, P(g), 256, 8192, 32, 32, 1, 6, 1, 4) == NOT_IMPLEMENTED  # CV_64F
    assert L.mi355cv_pyrupBatch(P(a), 16, 256, 16, 16, P(d), 40, 1600, 33, 32, 1, 0, 1, 4) == NOT_IMPLEMENTED   # dst 2w + 1
    assert L.mi355cv_pyrupBatch(P(a), 16, 256, 16, 16, P(d), 40, 1600, 32, 32, 1, 0, 1, 1) == NOT_IMPLEMENTED   # BORDER_REPLICATE
    assert L.mi355cv_pyrupBatch(None, 16, 256, 16, 16, P(d), 40, 1600, 32, 32, 1, 0, 1, 4) == NOT_IMPLEMENTED
    assert L.mi355cv_callCount(b"pyrup") + L.mi355cv_callCount(b"pyrupBatch") == n0
    assert np.all(d == 0)


def test_python_api_refuses_what_the_reference_asserts_on():
    import opencv_amd as cv
    a = np.zeros((8, 8), np.uint8)
    assert "pyrUp" in cv.imgproc.__all__ and "pyrUpBatch" in cv.imgproc.__all__
    with pytest.raises(ValueError):
        cv.pyrUp(a, borderType=cv.BORDER_REPLICATE)
    with pytest.raises(ValueError):
        cv.pyrUp(a, borderType=cv.BORDER_DEFAULT | cv.BORDER_ISOLATED)
    with pytest.raises(ValueError):
        cv.pyrUpBatch(a)
