"""Bayer demosaicing without a GPU: the known answers of the restatement (tests/demosaic_restate.py), the lines of opencv_amd/csrc/demosaic_math.h compiled for
the host (tests/hostemu/demosaic_emu.cpp, scalar and packed) against that restatement, the argument refusals of mi355cv_demosaic / mi355cv_demosaicBatch that
come before any device is touched, and the constants of the Python surface."""
import ctypes
import os

import numpy as np
import pytest

import demosaic_restate as R
import emubuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_IMPLEMENTED = 1
DEPTH = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 2}


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- the restatement itself
def test_known_answers():
    R.known_answers(R.demosaic)


def test_pattern_is_relative_to_the_origin():
    """a view one row / one column into a mosaic is the mosaic of the neighbouring pattern"""
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, (9, 10), dtype=np.uint8)
    # interior pixels only: the border copy belongs to the image handed in
    assert np.array_equal(R.demosaic(x, "BG", 3)[2:-1, 1:-1], R.demosaic(x[1:], "GR", 3)[1:-1, 1:-1])
    assert np.array_equal(R.demosaic(x, "BG", 3)[1:-1, 2:-1], R.demosaic(x[:, 1:], "GB", 3)[1:-1, 1:-1])
    assert np.array_equal(R.demosaic(x, "BG", 1)[2:-1, 2:-1], R.demosaic(x[1:, 1:], "RG", 1)[1:-1, 1:-1])


# ---- demosaic_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("demosaic_emu.cpp", "libdemosaic_emu.so", ["-ffp-contract=off"])
    lib.emu_demosaic.restype = ctypes.c_int
    lib.emu_demosaic.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_int] * 5
    lib.emu_demosaic_packed.restype = ctypes.c_int
    lib.emu_demosaic_packed.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_int] * 4
    lib.emu_demosaic_gray_weights.argtypes = [ctypes.c_void_p]
    return lib


def _pattern(name, rgb):
    return R.PATTERNS.index(R.RGB_OF[name] if rgb else name)


def _scalar(emu):
    def f(src, name, dcn, rgb=False):
        h, w = src.shape
        got = np.empty((h, w) if dcn == 1 else (h, w, dcn), src.dtype)
        assert emu.emu_demosaic(P(src), src.strides[0], P(got), got.strides[0], w, h, DEPTH[src.dtype], dcn, _pattern(name, rgb)) == 0
        return got
    return f


def _packed(emu):
    def f(src, name, dcn, rgb=False):
        if src.dtype != np.uint8:
            return _scalar(emu)(src, name, dcn, rgb)
        h, w = src.shape
        got = np.empty((h, w) if dcn == 1 else (h, w, dcn), np.uint8)
        assert emu.emu_demosaic_packed(P(src), src.strides[0], P(got), got.strides[0], w, h, dcn, _pattern(name, rgb)) == 0
        return got
    return f


def inputs(rng, dt, h, w):
    """random data, the depth's maximum, and the 0 / max checkerboards x&1, y&1, (x+y)&1: the inputs that carry between packed halves"""
    top = np.iinfo(dt).max
    yy, xx = np.mgrid[0:h, 0:w]
    yield rng.integers(0, top + 1, (h, w)).astype(dt)
    yield np.full((h, w), top, dt)
    for m in (xx & 1, yy & 1, (xx + yy) & 1):
        yield (m * top).astype(dt)


SIZES = [(3, 3), (4, 3), (3, 4), (5, 5), (8, 4), (17, 6), (19, 9)]              # (w, h)


def test_known_answers_of_the_lines(emu):
    R.known_answers(_scalar(emu))
    R.known_answers(_packed(emu))
    k = (ctypes.c_uint * 3)()
    emu.emu_demosaic_gray_weights(k)
    assert list(k) == [1868, 9617, 4899] and sum(k) == 1 << 14


@pytest.mark.parametrize("dt", [np.uint8, np.uint16])
@pytest.mark.parametrize("dcn", [1, 3, 4])
def test_scalar_lines_are_the_restatement(emu, dt, dcn):
    rng = np.random.default_rng(dcn)
    f = _scalar(emu)
    for w, h in SIZES:
        for src in inputs(rng, dt, h, w):
            for p in R.PATTERNS:
                assert np.array_equal(f(src, p, dcn), R.demosaic(src, p, dcn)), (w, h, p)


@pytest.mark.parametrize("dcn", [1, 3, 4])
def test_packed_lines_are_the_restatement(emu, dcn):
    rng = np.random.default_rng(10 + dcn)
    f = _packed(emu)
    for w, h in SIZES + [(16, 5), (33, 4)]:
        for src in inputs(rng, np.uint8, h, w):
            for p in R.PATTERNS:
                assert np.array_equal(f(src, p, dcn), R.demosaic(src, p, dcn)), (w, h, p)


def test_emu_refuses_what_the_library_declines(emu):
    a = np.zeros((8, 8), np.uint8)
    d = np.zeros((8, 8, 4), np.uint8)
    assert emu.emu_demosaic(P(a), 8, P(d), 32, 2, 8, 0, 3, 0) == -1
    assert emu.emu_demosaic(P(a), 8, P(d), 32, 8, 2, 0, 3, 0) == -1
    assert emu.emu_demosaic(P(a), 8, P(d), 32, 8, 8, 1, 3, 0) == -1
    assert emu.emu_demosaic(P(a), 8, P(d), 32, 8, 8, 0, 2, 0) == -1
    assert emu.emu_demosaic(P(a), 8, P(d), 32, 8, 8, 0, 3, 4) == -1


# ---- the C ABI's refusals that need no device
def test_entry_declines_bad_arguments():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.zeros((16, 16), np.uint8)
    d = np.zeros((16, 16, 4), np.uint8)
    f = np.zeros((16, 16), np.float32)
    big = L.mi355cv_limit(b"demosaic_max_dim")
    assert big == 16384
    n0 = L.mi355cv_callCount(b"demosaic") + L.mi355cv_callCount(b"demosaicBatch")
    one = L.mi355cv_demosaic
    assert one(P(a), 16, P(d), 64, 2, 16, 0, 3, 0) == NOT_IMPLEMENTED                       # w < 3
    assert "w < 3 || h < 3" in L.mi355cv_lastError().decode()
    assert one(P(a), 16, P(d), 64, 16, 2, 0, 3, 0) == NOT_IMPLEMENTED                       # h < 3
    assert one(P(a), 16, P(d), 64, 0, 16, 0, 3, 0) == NOT_IMPLEMENTED                       # empty image
    assert one(P(a), 16, P(d), 64, 16, -1, 0, 3, 0) == NOT_IMPLEMENTED
    for depth in (1, 3, 4, 5, 6):                                                           # CV_8S, CV_16S, CV_32S, CV_32F, CV_64F
        assert one(P(f), 64, P(d), 64, 4, 4, depth, 3, 0) == NOT_IMPLEMENTED
        assert "depth" in L.mi355cv_lastError().decode()
    for dcn in (0, 2, 5, -1):
        assert one(P(a), 16, P(d), 64, 16, 16, 0, dcn, 0) == NOT_IMPLEMENTED
        assert "dcn" in L.mi355cv_lastError().decode()
    for pattern in (-1, 4):
        assert one(P(a), 16, P(d), 64, 16, 16, 0, 3, pattern) == NOT_IMPLEMENTED
    assert one(None, 16, P(d), 64, 16, 16, 0, 3, 0) == NOT_IMPLEMENTED                      # null pointers
    assert one(P(a), 16, None, 64, 16, 16, 0, 3, 0) == NOT_IMPLEMENTED
    assert one(P(a), 16, P(d), 64, big + 1, 16, 0, 1, 0) == NOT_IMPLEMENTED                 # above the limit
    assert one(P(a), 16, P(d), 64, 16, big + 1, 0, 1, 0) == NOT_IMPLEMENTED
    assert one(P(a), 15, P(d), 64, 16, 16, 0, 3, 0) == NOT_IMPLEMENTED                      # a pitch below the row
    assert one(P(a), 16, P(d), 47, 16, 16, 0, 3, 0) == NOT_IMPLEMENTED
    assert one(P(a), 17, P(d), 64, 8, 16, 2, 3, 0) == NOT_IMPLEMENTED                       # CV_16U with an odd pitch
    bat = L.mi355cv_demosaicBatch
    assert bat(P(a), 16, 256, P(d), 64, 1024, 16, 16, 0, 0, 3, 0) == NOT_IMPLEMENTED        # no frames
    assert "nframes" in L.mi355cv_lastError().decode()
    assert bat(P(a), 16, 256, P(d), 64, 1024, 16, 16, -2, 0, 3, 0) == NOT_IMPLEMENTED
    assert bat(P(a), 16, 256, P(d), 64, 1024, 2, 16, 1, 0, 3, 0) == NOT_IMPLEMENTED         # w < 3
    assert bat(P(f), 64, 1024, P(d), 64, 1024, 4, 4, 1, 5, 3, 0) == NOT_IMPLEMENTED         # CV_32F
    assert bat(P(a), 16, 256, P(d), 64, 1024, 16, 16, 1, 0, 2, 0) == NOT_IMPLEMENTED        # dcn 2
    assert bat(None, 16, 256, P(d), 64, 1024, 16, 16, 1, 0, 3, 0) == NOT_IMPLEMENTED
    assert bat(P(a), 16, 256, None, 64, 1024, 16, 16, 1, 0, 3, 0) == NOT_IMPLEMENTED
    assert L.mi355cv_callCount(b"demosaic") + L.mi355cv_callCount(b"demosaicBatch") == n0
    assert not d.any()


# ---- the Python surface
FAMILIES = {"BGR": R.CODES_BGR, "GRAY": R.CODES_GRAY, "BGRA": R.CODES_BGRA}
SENSOR = {"RGGB": "BG", "GRBG": "GB", "BGGR": "RG", "GBRG": "GR"}


def test_constants_and_all():
    import opencv_amd as cv
    names = cv.imgproc.__all__
    assert "demosaicing" in names and "demosaicingBatch" in names
    for fam, codes in FAMILIES.items():
        for p, code in zip(R.PATTERNS, codes):
            n = f"COLOR_Bayer{p}2{fam}"
            assert n in names and getattr(cv, n) == code, n
    assert (cv.COLOR_BayerBG2BGR, cv.COLOR_BayerGB2BGR, cv.COLOR_BayerRG2BGR, cv.COLOR_BayerGR2BGR) == (46, 47, 48, 49)
    assert (cv.COLOR_BayerBG2GRAY, cv.COLOR_BayerGR2GRAY, cv.COLOR_BayerBG2BGRA, cv.COLOR_BayerGR2BGRA) == (86, 89, 139, 142)


def test_alias_identities_of_the_code_table():
    import opencv_amd as cv
    names = cv.imgproc.__all__
    assert (cv.COLOR_BayerBG2RGB, cv.COLOR_BayerGB2RGB, cv.COLOR_BayerRG2RGB, cv.COLOR_BayerGR2RGB) == (48, 49, 46, 47)
    for p in R.PATTERNS:                                                        # ...2RGB(A) = the ...2BGR(A) code with the B and R patterns exchanged
        assert getattr(cv, f"COLOR_Bayer{p}2RGB") == getattr(cv, f"COLOR_Bayer{R.RGB_OF[p]}2BGR")
        assert getattr(cv, f"COLOR_Bayer{p}2RGBA") == getattr(cv, f"COLOR_Bayer{R.RGB_OF[p]}2BGRA")
        assert f"COLOR_Bayer{p}2RGB" in names and f"COLOR_Bayer{p}2RGBA" in names
    for sensor, p in SENSOR.items():                                            # the sensor-order names of 4.x, all families
        for fam in ("BGR", "RGB", "GRAY", "BGRA", "RGBA"):
            n = f"COLOR_Bayer{sensor}2{fam}"
            assert n in names and getattr(cv, n) == getattr(cv, f"COLOR_Bayer{p}2{fam}"), n


def test_python_api_refuses_before_the_library():
    import opencv_amd as cv
    a = np.zeros((8, 8), np.uint8)
    n0 = cv.call_count("demosaic")
    for code in R.CODES_VNG + R.CODES_EA:                                       # not built: they keep raising
        with pytest.raises(NotImplementedError):
            cv.demosaicing(a, code)
        with pytest.raises(NotImplementedError):
            cv.cvtColor(a, code)
    with pytest.raises(ValueError):
        cv.demosaicing(a, cv.COLOR_BGR2GRAY)                                    # no Bayer code
    with pytest.raises(ValueError):
        cv.demosaicing(np.zeros((8, 8, 3), np.uint8), cv.COLOR_BayerBG2BGR)     # not single-channel
    with pytest.raises(ValueError):
        cv.cvtColor(np.zeros((8, 8, 2), np.uint8), cv.COLOR_BayerBG2GRAY)
    with pytest.raises(ValueError):
        cv.demosaicing(a, cv.COLOR_BayerBG2BGR, dstCn=2)
    with pytest.raises(ValueError):
        cv.demosaicing(a, cv.COLOR_BayerBG2BGR, dst=np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(NotImplementedError):
        cv.demosaicing(np.zeros((2, 8), np.uint8), cv.COLOR_BayerBG2BGR)       # declined by the library: h < 3
    with pytest.raises(NotImplementedError):
        cv.demosaicing(np.zeros((8, 8), np.float32), cv.COLOR_BayerBG2BGR)
    with pytest.raises(ValueError):
        cv.demosaicingBatch(a, cv.COLOR_BayerBG2BGR)
    assert cv.call_count("demosaic") == n0
