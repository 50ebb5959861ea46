"""CLAHE without a GPU: the two known answers of the restatement (tests/clahe_restate.py), the lines of opencv_amd/csrc/clahe_math.h compiled for the host
(tests/hostemu/clahe_emu.cpp) against that restatement, and the argument refusals of mi355cv_clahe / mi355cv_claheBatch that come before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

import clahe_restate as R
import emubuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_IMPLEMENTED = 1


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- the restatement itself
def test_known_answers():
    img = np.full((64, 64), 100, np.uint8)
    # A = 64, clip = 10, clipped = 54, residual step 4: LUT[100] = 25 + 11 = 36, 36 * 255 / 64 rounds to 143
    assert np.all(R.clahe(img) == 143)
    assert np.all(R.clahe(img, clipLimit=0.0) == 255)
    assert R.clip_limit(40.0, 64, 256) == 10 and R.clip_limit(0.0, 64, 256) == 0 and R.clip_limit(0.001, 64, 256) == 1


def test_padding_rule():
    assert R.plan(64, 64, (8, 8)) == (8, 8, 64, 64)
    assert R.plan(64, 61, (8, 8)) == (9, 8, 64, 61)                   # a divisible width still gains a whole tilesX columns
    assert R.plan(5, 8, (8, 1)) == (1, 9, 5, 8)                       # ... and a divisible height a whole tilesY rows
    assert R.plan(64, 61, (8, 8), margins=(3, 100)) == (9, 8, 67, 64)  # parent pixels first, at most the padding
    assert list(R.reflect101(np.arange(10), 4)) == [0, 1, 2, 3, 2, 1, 0, 1, 2, 3]
    assert list(R.reflect101(np.arange(3), 1)) == [0, 0, 0]


# ---- clahe_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("clahe_emu.cpp", "libclahe_emu.so", ["-ffp-contract=off"])
    lib.emu_clahe_lut.restype = None
    lib.emu_clahe_lut.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    lib.emu_clahe.restype = ctypes.c_int
    lib.emu_clahe.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    return lib


def _emu_lut(emu, hist, clip, scale, maxv):
    h = np.ascontiguousarray(hist, np.int32)
    out = np.empty(h.shape[0], np.int32)
    emu.emu_clahe_lut(P(h), h.shape[0], clip, float(scale), maxv, P(out))
    return out


@pytest.mark.parametrize("histSize", [256, 65536])
def test_lut_lines_against_the_restatement(emu, histSize):
    rng = np.random.default_rng(histSize)
    maxv = histSize - 1
    cases = []
    for area in (64, 480 * 270, 1000, 65535, 7):
        for kind in ("uniform", "narrow", "spike"):
            if kind == "uniform":
                px = rng.integers(0, histSize, area)
            elif kind == "narrow":                                        # 12-bit data in 16 bits / a dim 8-bit image
                px = rng.integers(0, max(2, histSize // 16), area) + histSize // 4
            else:
                px = np.where(rng.random(area) < 0.9, histSize // 3, rng.integers(0, histSize, area))
            h = np.bincount(px, minlength=histSize)
            for clipLimit in (0.0, 2.0, 40.0, 1e6, 0.5):
                cases.append((h, R.clip_limit(clipLimit, area, histSize), np.float32(maxv) / np.float32(area)))
    # residual cases: residual > histSize / 2 (step 1), residual = 1, a residual that divides histSize unevenly
    for clipped in (histSize - 1, histSize // 2 + 1, 1, 3, histSize + 5):
        h = np.zeros(histSize, np.int64)
        h[7] = 10 + clipped
        h[histSize - 1] = 4
        cases.append((h, 10, np.float32(maxv) / np.float32(h.sum())))
    for h, clip, scale in cases:
        got = _emu_lut(emu, h, clip, scale, maxv)
        want = R.lut_from_hist(h[None, :], clip, scale, maxv)[0]
        assert np.array_equal(got, want), (histSize, clip, int(h.sum()))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_whole_clahe_lines_against_the_restatement(emu, dtype):
    rng = np.random.default_rng(7)
    hi = 256 if dtype == np.uint8 else 65536
    for (w, h, tiles, clip) in [(64, 64, (8, 8), 40.0), (61, 37, (8, 8), 2.0), (64, 61, (8, 8), 40.0), (5, 9, (8, 8), 40.0), (40, 30, (3, 5), 0.0),
                                (33, 47, (1, 1), 1e6), (100, 80, (16, 16), 4.0)]:
        for data in ("full", "12bit"):
            top = hi if data == "full" else min(hi, 4096)
            src = rng.integers(0, top, (h, w)).astype(dtype)
            got = np.empty_like(src)
            assert emu.emu_clahe(P(src), src.strides[0], P(got), got.strides[0], w, h, 0 if dtype == np.uint8 else 2, 0, 0, clip, *tiles) == 0
            assert np.array_equal(got, R.clahe(src, clip, tiles)), (w, h, tiles, clip, data)
    # a submatrix whose padding comes from the parent's pixels
    parent = rng.integers(0, hi, (90, 120)).astype(dtype)
    x0, y0, w, h = 10, 20, 61, 45
    roi = parent[y0:y0 + h, x0:x0 + w]
    got = np.empty((h, w), dtype)
    mr, mb = parent.shape[1] - x0 - w, parent.shape[0] - y0 - h
    assert emu.emu_clahe(P(roi), roi.strides[0], P(got), got.strides[0], w, h, 0 if dtype == np.uint8 else 2, mr, mb, 40.0, 8, 8) == 0
    want = R.clahe(roi, 40.0, (8, 8), parent=parent, origin=(x0, y0))
    assert np.array_equal(got, want)
    assert not np.array_equal(want, R.clahe(np.ascontiguousarray(roi), 40.0, (8, 8)))       # the margins matter here


def test_emu_refuses_what_the_reference_cannot_run(emu):
    a = np.zeros((8, 8), np.uint8)
    for depth, tx, ty in [(1, 8, 8), (0, 0, 8), (0, 8, -1)]:
        assert emu.emu_clahe(P(a), 8, P(a), 8, 8, 8, depth, 0, 0, 40.0, tx, ty) == -1


# ---- the C ABI's refusals that need no device
def test_entry_declines_bad_arguments():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.zeros((16, 16), np.uint8)
    f = np.zeros((16, 16), np.float32)
    assert L.mi355cv_clahe(P(f), 64, P(f), 64, 16, 16, 5, 0, 0, 40.0, 8, 8) == NOT_IMPLEMENTED               # CV_32F
    assert "depth" in L.mi355cv_lastError().decode()
    assert L.mi355cv_clahe(P(a), 16, P(a), 16, 16, 16, 1, 0, 0, 40.0, 8, 8) == NOT_IMPLEMENTED               # CV_8S
    assert L.mi355cv_clahe(P(a), 16, P(a), 16, 16, 16, 0, 0, 0, 40.0, 0, 8) == NOT_IMPLEMENTED               # tiles <= 0
    assert L.mi355cv_clahe(P(a), 16, P(a), 16, 16, 16, 0, 0, 0, 40.0, 8, -2) == NOT_IMPLEMENTED
    assert "tilesX <= 0" in L.mi355cv_lastError().decode()
    assert L.mi355cv_clahe(None, 16, P(a), 16, 16, 16, 0, 0, 0, 40.0, 8, 8) == NOT_IMPLEMENTED               # null pointers
    assert L.mi355cv_clahe(P(a), 16, None, 16, 16, 16, 0, 0, 0, 40.0, 8, 8) == NOT_IMPLEMENTED
    assert L.mi355cv_clahe(P(a), 16, P(a), 16, 0, 16, 0, 0, 0, 40.0, 8, 8) == NOT_IMPLEMENTED                # empty image
    assert L.mi355cv_clahe(P(a), 16, P(a), 16, 16, 16, 0, -1, 0, 40.0, 8, 8) == NOT_IMPLEMENTED              # negative margin
    assert L.mi355cv_claheBatch(P(a), 16, 256, P(a), 16, 256, 1, 16, 16, 2, 40.0, 0, 8) == NOT_IMPLEMENTED
    assert L.mi355cv_claheBatch(P(a), 16, 256, P(a), 16, 256, 0, 16, 16, 0, 40.0, 8, 8) == NOT_IMPLEMENTED   # no frames


def test_python_api_refuses_what_the_reference_asserts_on():
    import opencv_amd as cv
    c = cv.createCLAHE()
    assert c.getClipLimit() == 40.0 and c.getTilesGridSize() == (8, 8)
    c.setClipLimit(2.5); c.setTilesGridSize((3, 5))
    assert c.getClipLimit() == 2.5 and c.getTilesGridSize() == (3, 5)
    c.collectGarbage()
    with pytest.raises(ValueError):
        c.apply(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        c.apply(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        cv.createCLAHE(40.0, (0, 8))
    with pytest.raises(ValueError):
        c.setTilesGridSize((8, -1))
