"""minMaxLoc without a GPU: the two restatements (tests/minmax_restate.py) against known answers and against each other, the lines of
opencv_amd/csrc/minmax_math.h compiled for the host (tests/hostemu/minmax_emu.cpp) against them, and the refusals of the two mi355cv_minMaxLoc* entries that
come before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

import emubuild
import minmax_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_IMPLEMENTED = 0, 1
NAN, INF = float("nan"), float("inf")
BOTH = [R.minmax_loops, R.minmax_vec]


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- known answers
@pytest.mark.parametrize("fn", BOTH)
def test_known_answers(fn):
    for dt in R.DTYPES:
        assert fn(np.full((3, 4), 7, dt)) == (7.0, 7.0, (0, 0), (0, 0))                          # a constant image: both at the first pixel
    for dt in (np.float32, np.float64):
        got = fn(np.array([[0.0, -0.0]], dt))
        assert got[0] == 0.0 and got[2] == (0, 0) and got[3] == (0, 0)                           # +0 == -0: the earlier wins, for min and for max
        got = fn(np.array([[-0.0, 0.0]], dt))
        assert got[1] == 0.0 and got[3] == (0, 0) and got[2] == (0, 0)
        assert fn(np.array([[NAN, 2.0, 1.0], [3.0, NAN, 1.0]], dt)) == (1.0, 3.0, (2, 0), (0, 1))   # NaN at the first pixel is skipped
        assert fn(np.full((2, 3), NAN, dt)) == R.EMPTY
        assert fn(np.full((2, 3), NAN, dt), np.ones((2, 3), np.uint8)) == R.EMPTY
        assert fn(np.array([[1.0, -INF, INF], [INF, -INF, 0.0]], dt)) == (-INF, INF, (1, 0), (2, 0))
        assert fn(np.array([[NAN, INF]], dt)) == (INF, INF, (1, 0), (1, 0))
    a = np.arange(12, dtype=np.int16).reshape(3, 4)
    assert fn(a, np.zeros((3, 4), np.uint8)) == R.EMPTY                                          # an all-zero mask
    m = np.zeros((3, 4), np.uint8)
    m[1, 2] = 1
    m[2, 1] = 255
    assert fn(a, m) == (6.0, 9.0, (2, 1), (1, 2))
    m = np.array([[1, 0, 1]], np.uint8)
    assert fn(np.array([[NAN, 5.0, NAN]], np.float32), m) == R.EMPTY                             # mask and NaN together leave nothing


@pytest.mark.parametrize("fn", BOTH)
def test_type_extremes_of_every_integer_depth(fn):
    for dt in (np.uint8, np.int8, np.uint16, np.int16, np.int32):
        ii = np.iinfo(dt)
        a = np.array([[0, ii.max, ii.min], [ii.min, ii.max, 1]], dt)
        first_min = (2, 0) if ii.min < 0 else (0, 0)
        assert fn(a) == (float(ii.min), float(ii.max), first_min, (1, 0))
        assert fn(np.full((2, 2), ii.max, dt)) == (float(ii.max), float(ii.max), (0, 0), (0, 0))
        assert fn(np.full((2, 2), ii.min, dt)) == (float(ii.min), float(ii.min), (0, 0), (0, 0))


# ---- the two restatements agree
def small_frames():
    """(name, frame, mask): few levels, so that ties are the rule"""
    rng = np.random.default_rng(11)
    out = []
    for dt in R.DTYPES:
        for (h, w) in ((1, 1), (1, 9), (7, 1), (5, 6), (9, 13)):
            for levels in (3, 4, 5):
                a = R.random_frame(rng, h, w, dt, levels=levels, nan=0.2 if levels == 4 else 0.0, special=levels == 5)
                for mk in ("none", "random", "zero"):
                    m = None if mk == "none" else (rng.random((h, w)) < 0.4).astype(np.uint8) * 3 if mk == "random" else np.zeros((h, w), np.uint8)
                    out.append(("%s %dx%d L%d %s" % (np.dtype(dt).name, h, w, levels, mk), a, m))
    return out


def test_restatements_agree_on_small_frames_full_of_ties():
    ties = 0
    for name, a, m in small_frames():
        l, v = R.minmax_loops(a, m), R.minmax_vec(a, m)
        assert R.same(l, v), (name, l, v)
        if l != R.EMPTY:
            sel = np.ones(a.shape, bool) if m is None else m != 0
            ties += int((a[sel].astype(np.float64) == l[0]).sum() > 1)
    assert ties > 100                                                                            # the tie-break was exercised, not avoided


# ---- minmax_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("minmax_emu.cpp", "libminmax_emu.so", ["-ffp-contract=off"])
    i32, u32, u64, vp = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.emu_minmax_keys.argtypes = [i32, vp, i32, vp, vp]
    lib.emu_minmax_values.argtypes = [i32, vp, i32, vp]
    lib.emu_minmax_combine.argtypes = [i32, u64, u32, u64, u32, ctypes.POINTER(u64), ctypes.POINTER(u32)]
    lib.emu_minmax_reduce.argtypes = [i32, vp, ctypes.c_size_t, i32, i32, vp, ctypes.c_size_t, i32, vp, vp]
    lib.emu_minmax_none.restype = u32
    return lib


def sorted_samples(dt):
    """strictly ascending values of the depth: the extremes, and for floats denormals, one zero, +-inf, for 32-bit depths the values around the sign boundary"""
    dt = np.dtype(dt)
    if dt.kind == "f":
        fi = np.finfo(dt)
        pos = [fi.smallest_subnormal, fi.smallest_subnormal * 2, fi.tiny / 2, fi.tiny, fi.tiny * 2, 1e-5, 0.5, 1.0, np.nextafter(dt.type(1), dt.type(2)), 2.0, 1e5,
               fi.max / 2, fi.max, np.inf]
        vals = [-v for v in reversed(pos)] + [0.0] + pos
    else:
        ii = np.iinfo(dt)
        vals = sorted({ii.min, ii.min + 1, ii.min + 2, -2, -1, 0, 1, 2, 127, 128, ii.max // 2, ii.max // 2 + 1, ii.max - 1, ii.max} & set(range(ii.min, ii.max + 1))
                      if ii.bits <= 16 else {ii.min, ii.min + 1, -2, -1, 0, 1, 2, 0x7FFFFFFE, ii.max, -0x7FFFFFFF, 65535, 65536, -65536})
    a = np.array(vals, dt)
    assert np.all(a[:-1] < a[1:])
    return a


def keys_of(emu, a):
    keys, valid = np.zeros(a.size, np.uint64), np.zeros(a.size, np.uint8)
    a = np.ascontiguousarray(a)
    assert emu.emu_minmax_keys(R.DEPTHS[a.dtype], P(a), a.size, P(keys), P(valid)) == 0
    return keys, valid


@pytest.mark.parametrize("dt", R.DTYPES)
def test_key_is_strictly_monotone_and_decode_inverts_it(emu, dt):
    a = sorted_samples(dt)
    keys, valid = keys_of(emu, a)
    assert valid.all() and np.all(keys[:-1] < keys[1:]), np.dtype(dt).name
    assert keys.max() < (1 << 32) or np.dtype(dt) == np.float64
    back = np.zeros(a.size, np.float64)
    assert emu.emu_minmax_values(R.DEPTHS[np.dtype(dt)], P(keys), a.size, P(back)) == 0
    assert np.array_equal(back, a.astype(np.float64))
    rng = np.random.default_rng(5)                                                               # and on random full-range values: order and round trip
    r = R.random_frame(rng, 40, 50, dt, special=True).ravel()
    keys, valid = keys_of(emu, r)
    assert valid.all()
    o = np.argsort(r, kind="stable")
    d = r[o].astype(np.float64)
    k = keys[o]
    assert np.all((d[:-1] < d[1:]) == (k[:-1] < k[1:])) and np.all((d[:-1] == d[1:]) == (k[:-1] == k[1:]))
    back = np.zeros(r.size, np.float64)
    emu.emu_minmax_values(R.DEPTHS[np.dtype(dt)], P(keys), r.size, P(back))
    assert np.array_equal(back, r.astype(np.float64))


def test_float_zeros_share_a_key_and_nan_has_none(emu):
    for dt, nans in ((np.float32, np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)),
                     (np.float64, np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF], np.uint64))):
        keys, valid = keys_of(emu, np.array([0.0, -0.0, np.inf, -np.inf], dt))
        assert valid.all() and keys[0] == keys[1] and keys[3] < keys[0] < keys[2]
        _, valid = keys_of(emu, nans.view(dt))
        assert not valid.any()
        # the identity of the combine, all ones, is no candidate's key: as a minimum it would be a NaN pattern, as a maximum (complemented) too
        top = np.array([np.inf], dt)
        assert keys_of(emu, top)[0][0] < (1 << (32 if dt == np.float32 else 64)) - 1


def test_combine_keeps_the_smallest_index_on_ties(emu):
    none = emu.emu_minmax_none()
    assert none == 0xFFFFFFFF

    def comb(wide, a, b):
        ko, io = ctypes.c_uint64(), ctypes.c_uint32()
        emu.emu_minmax_combine(wide, a[0], a[1], b[0], b[1], ctypes.byref(ko), ctypes.byref(io))
        return ko.value, io.value

    for wide, ones in ((0, 0xFFFFFFFF), (1, 0xFFFFFFFFFFFFFFFF)):
        ident = (ones, none)
        for a, b, want in (((5, 9), (5, 3), (5, 3)), ((5, 3), (5, 9), (5, 3)), ((4, 9), (5, 3), (4, 9)), ((5, 3), (4, 9), (4, 9)), ((5, 3), (5, 3), (5, 3)),
                           ((ones, 7), ident, (ones, 7)), (ident, (ones, 7), (ones, 7)), (ident, ident, ident), ((0, 0), ident, (0, 0)),
                           ((ones, 7), (ones, 2), (ones, 2))):
            assert comb(wide, a, b) == want, (wide, a, b)
    # the same pairs as a maximum: the key complemented, the index not -- equal values still keep the smaller index
    v, w = 0x12345678, 0x12345679
    assert comb(0, (~v & 0xFFFFFFFF, 9), (~v & 0xFFFFFFFF, 3)) == (~v & 0xFFFFFFFF, 3) and comb(0, (~v & 0xFFFFFFFF, 1), (~w & 0xFFFFFFFF, 8)) == (~w & 0xFFFFFFFF, 8)
    # 64-bit keys that differ only in the low word, below float precision
    assert comb(1, ((7 << 32) | 2, 1), ((7 << 32) | 1, 8)) == ((7 << 32) | 1, 8)


def emu_reduce(emu, a, m, order):
    a = np.ascontiguousarray(a)
    vals, locs = np.full(2, -7.0), np.full(4, -7, np.int32)
    m = None if m is None else np.ascontiguousarray(m)
    assert emu.emu_minmax_reduce(R.DEPTHS[a.dtype], P(a), a.strides[0], a.shape[1], a.shape[0], P(m) if m is not None else None, m.strides[0] if m is not None else 0,
                                 order, P(vals), P(locs)) == 0
    return vals[0], vals[1], (locs[0], locs[1]), (locs[2], locs[3])


def test_emulated_reduction_matches_in_every_association_order(emu):
    assert emu.emu_minmax_orders() == 5 and emu.emu_minmax_max_dim() == R.MAX_DIM
    frames = small_frames()
    rng = np.random.default_rng(12)
    for dt in R.DTYPES:                                                                          # more than 64 lanes' worth of pixels, full range, with the extremes
        frames.append((np.dtype(dt).name + " 23x31", R.random_frame(rng, 23, 31, dt, nan=0.3), None))
        frames.append((np.dtype(dt).name + " 23x31 constant", np.full((23, 31), 3, dt), None))
    for name, a, m in frames:
        want = R.minmax_vec(a, m)
        for order in range(5):
            got = emu_reduce(emu, a, m, order)
            assert R.same(got, want), (name, order, got, want)


# ---- the C ABI's refusals that need no device
ENTRIES = ("mi355cv_minMaxLoc", "mi355cv_minMaxLocBatch")
COUNTERS = (b"minMaxLoc", b"minMaxLocBatch")


def test_header_symbols_are_bound():
    from opencv_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mi355cv.h")).read()
    for name in ENTRIES:
        assert name + "(" in txt and name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_bound_is_exposed_and_pinned():
    from opencv_amd import _lib
    assert _lib.limit(R.MAX_DIM_KEY) == 16384 == R.MAX_DIM
    assert R.MAX_DIM * R.MAX_DIM <= 1 << 28


def test_entries_decline_bad_arguments_before_a_device_is_touched():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.ones((16, 16), np.float64)
    m = np.ones((16, 16), np.uint8)
    vals, locs = np.full(4, 7.0), np.full(8, 7, np.int32)
    n0 = sum(L.mi355cv_callCount(n) for n in COUNTERS)
    big = _lib.limit(R.MAX_DIM_KEY) + 1
    vp = lambda x: P(x) if x is not None else None

    def one(src=a, step=128, w=16, h=16, depth=6, mask=None, mstep=16, v=vals, l=locs, off=0, **_):
        return L.mi355cv_minMaxLoc(ctypes.c_void_p(src.ctypes.data + off) if src is not None else None, step, w, h, depth, vp(mask), mstep, vp(v), vp(l))

    def batch(src=a, step=128, w=16, h=8, depth=6, mask=None, mstep=16, v=vals, l=locs, nf=2, sf=1024, mf=0, off=0):
        return L.mi355cv_minMaxLocBatch(ctypes.c_void_p(src.ctypes.data + off) if src is not None else None, step, sf, w, h, depth, vp(mask), mstep, mf, nf, vp(v), vp(l))

    reason = lambda: L.mi355cv_lastError().decode()
    for f in (one, batch):
        assert f(src=None) == NOT_IMPLEMENTED and "src" in reason()
        assert f(v=None) == NOT_IMPLEMENTED and "vals" in reason()
        assert f(l=None) == NOT_IMPLEMENTED and "locs" in reason()
        for depth in (-1, 7, 8, 100):
            assert f(depth=depth) == NOT_IMPLEMENTED and "depth" in reason()
        assert f(w=0) == NOT_IMPLEMENTED and f(h=0) == NOT_IMPLEMENTED and f(w=-3) == NOT_IMPLEMENTED and f(h=-3) == NOT_IMPLEMENTED
        assert f(w=big, step=big * 8) == NOT_IMPLEMENTED and f(h=big) == NOT_IMPLEMENTED and "MINMAX_MAX_DIM" in reason()
        assert f(step=127) == NOT_IMPLEMENTED and f(step=120) == NOT_IMPLEMENTED and "smaller than a row" in reason()      # a pitch smaller than the row
        assert f(mask=m, mstep=15) == NOT_IMPLEMENTED and "smaller than a row" in reason()
        assert f(step=132) == NOT_IMPLEMENTED and "multiple of the element size" in reason()                                 # 132 % 8 != 0
        assert f(depth=3, step=33) == NOT_IMPLEMENTED and f(depth=5, step=66) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
        assert f(depth=5, off=2) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
    assert batch(nf=0) == NOT_IMPLEMENTED and batch(nf=-1) == NOT_IMPLEMENTED and batch(nf=65536) == NOT_IMPLEMENTED and "nframes" in reason()
    assert batch(sf=1028) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
    assert sum(L.mi355cv_callCount(n) for n in COUNTERS) == n0
    assert np.all(vals == 7.0) and np.all(locs == 7)


def test_python_api_refuses_bad_arguments():
    import opencv_amd as cv
    for name in ("minMaxLoc", "minMaxLocBatch"):
        assert name in cv.imgproc.__all__ and hasattr(cv, name), name
    a = np.zeros((8, 8), np.uint8)
    n0 = cv._lib.decline_count()
    with pytest.raises(ValueError):
        cv.minMaxLoc(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        cv.minMaxLoc(np.zeros((8, 8, 1), np.uint8))
    for bad in (np.zeros((8, 7), np.uint8), np.zeros((8, 8), np.int8), np.zeros((8, 8), np.float32)):
        with pytest.raises(ValueError):
            cv.minMaxLoc(a, bad)
    with pytest.raises(ValueError):
        cv.minMaxLocBatch(a)
    assert cv._lib.decline_count() == n0                                    # nothing reached the library
