"""calcHist / calcBackProject without a GPU: the two restatements (tests/calchist_restate.py) against known answers, against each other and against
numpy.histogramdd where both definitions coincide; the lines of opencv_amd/csrc/calchist_math.h compiled for the host (tests/hostemu/calchist_emu.cpp) against them;
and the refusals of the four mi355cv_calcHist* / mi355cv_calcBackProject* entries that come before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

import calchist_restate as R
import emubuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_IMPLEMENTED = 0, 1
BOTH_HIST = [R.calchist_loops, R.calchist_vec]
BOTH_BP = [R.backproject_loops, R.backproject_vec]

# the (n, lo, hi) of tests/test_calchist_gpu.py
BIN_PARAMS = [(n, lo, hi) for n in (1, 2, 7, 180, 256) for (lo, hi) in ((0, 256), (0, 180), (10.5, 200.25), (-5, 300))]
BIN_PARAMS_16U = [(1000, 0, 65536), (65536, 0, 65536), (256, 0, 65536), (7, 100.5, 40000.25)]
NONUNIFORM_8U = np.array([3, 10, 11, 50.5, 128, 200, 250], np.float32)            # 6 bins; starts above 0, ends below 255
NONUNIFORM_16U = np.array([100, 101, 1000.5, 30000, 65000], np.float32)            # 4 bins


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- known answers
@pytest.mark.parametrize("fn", BOTH_HIST)
def test_known_answers(fn):
    a = np.array([[0, 1, 2, 3], [127, 128, 254, 255]], np.uint8)
    assert np.array_equal(fn(a, [0], None, [2], [0, 256]), np.array([5, 3], np.float32))
    assert np.array_equal(fn(a, [0], None, [256], [0, 256], hist_depth=R.CV_32S), np.bincount(a.ravel(), minlength=256).astype(np.int32))
    assert np.array_equal(fn(a, [0], None, [2], [1, 255]), np.array([4, 2], np.float32))                    # 0 and 255 lie outside [1, 255)
    m = np.array([[1, 0, 0, 9], [0, 0, 0, 255]], np.uint8)
    assert np.array_equal(fn(a, [0], m, [2], [0, 256]), np.array([2, 1], np.float32))
    assert np.array_equal(fn(a, [0], np.zeros((2, 4), np.uint8), [3], [0, 256]), np.zeros(3, np.float32))
    assert np.array_equal(fn(a, [0], None, [1], [0, 256]), np.array([8], np.float32))
    # two dimensions over two channels, any order, a repeated channel
    c = np.zeros((1, 3, 3), np.uint8)
    c[0, :, 0] = [0, 100, 200]
    c[0, :, 2] = [255, 0, 128]
    want = np.zeros((2, 2), np.int32)
    want[0, 1] += 1; want[0, 0] += 1; want[1, 1] += 1                                                      # (ch0, ch2) = (0,255), (100,0), (200,128)
    assert np.array_equal(fn(c, [0, 2], None, [2, 2], [0, 256, 0, 256], hist_depth=R.CV_32S), want)
    assert np.array_equal(fn(c, [2, 0], None, [2, 2], [0, 256, 0, 256], hist_depth=R.CV_32S), want.T)
    assert np.array_equal(fn(c, [0, 0], None, [2, 2], [0, 256, 0, 256], hist_depth=R.CV_32S), np.array([[2, 0], [0, 1]], np.int32))
    # non-uniform
    assert np.array_equal(fn(a, [0], None, [2], [1, 3, 255], uniform=False, hist_depth=R.CV_32S), np.array([2, 4], np.int32))
    # CV_32F: NaN, infinities and the upper end are not counted; -0 is 0
    f = np.array([[np.nan, np.inf, -np.inf, -0.0, 0.0, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(0))]], np.float32)
    assert np.array_equal(fn(f, [0], None, [2], [0, 1], hist_depth=R.CV_32S), np.array([2, 2], np.int32))
    # accumulate: 2.5 -> 2, 3.5 -> 4 (ties to even), int32 as it is
    assert np.array_equal(fn(a, [0], None, [2], [0, 256], start=np.array([2.5, 3.5], np.float32)), np.array([7, 7], np.float32))
    assert np.array_equal(fn(a, [0], None, [2], [0, 256], hist_depth=R.CV_32S, start=np.array([10, -1], np.int32)), np.array([15, 2], np.int32))


@pytest.mark.parametrize("fn", BOTH_BP)
def test_back_projection_known_answers(fn):
    a = np.array([[0, 1, 127, 128, 255]], np.uint8)
    h = np.array([10, 3], np.float32)
    assert np.array_equal(fn(a, [0], h, [0, 256], 1.0), np.array([[10, 10, 10, 3, 3]], np.uint8))
    assert np.array_equal(fn(a, [0], h, [0, 256], 0.25), np.array([[2, 2, 2, 1, 1]], np.uint8))           # 2.5 -> 2 (tie to even), 0.75 -> 1
    assert np.array_equal(fn(a, [0], np.array([14, 6], np.float32), [0, 256], 0.25), np.array([[4, 4, 4, 2, 2]], np.uint8))      # 3.5 -> 4, 1.5 -> 2
    assert np.array_equal(fn(a, [0], h, [0, 256], 100.0), np.array([[255, 255, 255, 255, 255]], np.uint8))
    assert np.array_equal(fn(a, [0], h, [0, 256], -1.0), np.zeros((1, 5), np.uint8))
    assert np.array_equal(fn(a, [0], h, [1, 255], 1.0), np.array([[0, 10, 10, 3, 0]], np.uint8))          # outside the range: 0
    s = np.array([[0, 40000, 65535]], np.uint16)
    assert np.array_equal(fn(s, [0], h, [0, 65536], 7000.0), np.array([[65535, 21000, 21000]], np.uint16))
    f = np.array([[0.25, 0.75, np.nan, 2.0]], np.float32)
    assert np.array_equal(fn(f, [0], h, [0, 1], 0.1), np.array([[np.float32(10 * 0.1), np.float32(np.float64(np.float32(3)) * 0.1), 0, 0]], np.float32))


def small_cases():
    rng = np.random.default_rng(7)
    out = []
    for dt in (np.uint8, np.uint16):
        top = np.iinfo(dt).max
        for (h, w) in ((1, 1), (3, 7), (9, 13)):
            for cn in (1, 3):
                img = rng.integers(0, top + 1, (h, w, cn)).astype(dt)
                img.ravel()[:2] = [0, top][:img.size]
                m = (rng.random((h, w)) < 0.6).astype(np.uint8) * 5
                out.append((img, [0], None, [7], [10.5, top * 0.8]))
                out.append((img, [cn - 1], m, [1], [0, top + 1]))
                if cn == 3:
                    out.append((img, [2, 0], m, [5, 3], [0, top + 1, -5, top * 1.2]))
                    out.append((img, [0, 1, 2], None, [2, 3, 4], [0, top + 1] * 3))
                    out.append((img, [1, 1], None, [4, 4], [0, top + 1, 0, top / 2]))
    f = (rng.random((9, 13, 2)) * 3 - 1).astype(np.float32)
    f[0, 0] = [np.nan, 0.5]; f[0, 1] = [np.inf, -np.inf]; f[1, 1] = [-0.0, 1.0]
    out.append((f, [0], None, [64], [0, 1]))
    out.append((f, [1, 0], (rng.random((9, 13)) < 0.7).astype(np.uint8), [5, 4], [0, 1, -0.5, 1.5]))
    return out


def test_restatements_agree_on_small_frames():
    for img, ch, m, hs, rg in small_cases():
        for depth in (R.CV_32S, R.CV_32F):
            l, v = R.calchist_loops(img, ch, m, hs, rg, hist_depth=depth), R.calchist_vec(img, ch, m, hs, rg, hist_depth=depth)
            assert l.dtype == v.dtype and np.array_equal(l, v), (img.dtype, ch, hs, rg)
        start = (np.random.default_rng(1).random(hs) * 9).astype(np.float32)
        start.ravel()[0] = 2.5
        assert np.array_equal(R.calchist_loops(img, ch, m, hs, rg, start=start), R.calchist_vec(img, ch, m, hs, rg, start=start))
        hist = R.calchist_vec(img, ch, m, hs, rg)
        for scale in (1.0, 0.37, 300.0):
            l, v = R.backproject_loops(img, ch, hist, rg, scale), R.backproject_vec(img, ch, hist, rg, scale)
            assert l.dtype == v.dtype == img.dtype and np.array_equal(l, v, equal_nan=True), (img.dtype, ch, hs, rg, scale)
    for img, bounds in ((np.arange(256, dtype=np.uint8).reshape(16, 16), NONUNIFORM_8U), (np.arange(0, 65536, 7, dtype=np.uint16).reshape(-1, 3), NONUNIFORM_16U)):
        n = len(bounds) - 1
        l, v = R.calchist_loops(img, [0], None, [n], bounds, uniform=False), R.calchist_vec(img, [0], None, [n], bounds, uniform=False)
        assert np.array_equal(l, v) and 0 < l.sum() < img.size


def test_restatement_equals_histogramdd_where_the_definitions_coincide():
    """integer data, power-of-two bin widths, hi above every value: a and b are exact and floor((v - lo) / width) is the bin under either definition"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (31, 45, 3)).astype(np.uint8)
    for hs in ([256], [64], [8, 32], [4, 16, 2]):
        ch = list(range(len(hs)))
        rg = [0, 256] * len(hs)
        want, _ = np.histogramdd(img.reshape(-1, 3)[:, :len(hs)].astype(np.float64), bins=hs, range=[(0, 256)] * len(hs))
        for fn in BOTH_HIST:
            assert np.array_equal(fn(img, ch, None, hs, rg, hist_depth=R.CV_32S), want.astype(np.int32)), hs
    s = rng.integers(0, 65536, (20, 33)).astype(np.uint16)
    want, _ = np.histogramdd(s.reshape(-1, 1).astype(np.float64), bins=[1024], range=[(0, 65536)])
    for fn in BOTH_HIST:
        assert np.array_equal(fn(s, [0], None, [1024], [0, 65536], hist_depth=R.CV_32S), want.astype(np.int32))


# ---- calchist_math.h on the host
@pytest.fixture(scope="module")
def emu():
    # -ffp-contract=fast, and -mfma where this CPU has it, on purpose: the header itself must make contraction impossible
    try:
        fma = ["-mfma"] if " fma " in open("/proc/cpuinfo").read() else []
    except OSError:
        fma = []
    lib = emubuild.load("calchist_emu.cpp", "libcalchist_emu.so", ["-ffp-contract=fast"] + fma)
    i32, vp, f32, dbl = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_double
    lib.emu_calchist_table.argtypes = [i32, i32, i32, vp, i32, vp]
    lib.emu_calchist_bins_f32.argtypes = [vp, i32, i32, f32, f32, vp]
    lib.emu_calchist_coef.argtypes = [i32, f32, f32, vp]
    lib.emu_calchist_bin_nonuniform.argtypes = [f32, vp, i32]
    lib.emu_calchist_backproject.argtypes = [i32, vp, i32, dbl, vp]
    lib.emu_calchist_count_of_float.argtypes = [vp, i32, vp]
    lib.emu_calchist_float_of_count.argtypes = [vp, i32, vp]
    return lib


def emu_table(emu, levels, n, ranges, uniform, mult=1):
    tab = np.zeros(levels, np.int32)
    r = np.ascontiguousarray(ranges, np.float32)
    emu.emu_calchist_table(levels, n, 1 if uniform else 0, P(r), mult, P(tab))
    return tab


def test_constants_are_the_restatements(emu):
    assert emu.emu_calchist_max_dim() == R.MAX_DIM and emu.emu_calchist_max_bins() == R.MAX_BINS and emu.emu_calchist_max_bins_per_dim() == R.MAX_BINS_PER_DIM
    skip = emu.emu_calchist_skip()
    assert 3 * skip > -2 ** 31 and skip + 2 * R.MAX_BINS < 0


def test_tables_of_every_bin_parameter_of_the_gpu_file(emu):
    skip = emu.emu_calchist_skip()
    for levels, params in ((256, BIN_PARAMS), (65536, BIN_PARAMS_16U + [(n, lo, hi) for (n, lo, hi) in BIN_PARAMS if n in (7, 256)])):
        for n, lo, hi in params:
            want = R.table(levels, n, [lo, hi], True)
            got = emu_table(emu, levels, n, [lo, hi], True, mult=3)
            assert np.array_equal(got, np.where(want < 0, skip, want * 3)), (levels, n, lo, hi)
            # ... and the loops agree with the vectorised table at every value that can differ: the ends of the range and of each bin
            probe = sorted({0, levels - 1, int(max(0, np.floor(lo))), int(min(levels - 1, np.ceil(hi)))} | {int(v) for v in np.linspace(0, levels - 1, 50)})
            for v in probe:
                k = R.bin_loops(v, "i", n, [np.float32(lo), np.float32(hi)], True)
                assert (k if k is not None else -1) == want[v], (levels, n, lo, hi, v)
    for levels, bounds in ((256, NONUNIFORM_8U), (65536, NONUNIFORM_16U)):
        n = len(bounds) - 1
        want = R.table(levels, n, bounds, False)
        assert np.array_equal(emu_table(emu, levels, n, bounds, False), np.where(want < 0, skip, want))
        assert want[0] == -1 and want[levels - 1] == -1 and set(want.tolist()) == set(range(-1, n))
        for v in (0, int(bounds[0]) - 1, int(bounds[0]), int(bounds[1]), int(bounds[-1]) - 1, int(bounds[-1]), levels - 1):
            k = R.bin_loops(v, "i", n, bounds, False)
            assert (k if k is not None else -1) == want[v] == emu.emu_calchist_bin_nonuniform(float(v), P(bounds), n), v


def emu_bins_f32(emu, vals, n, lo, hi):
    v = np.ascontiguousarray(vals, np.float32)
    out = np.zeros(v.size, np.int32)
    emu.emu_calchist_bins_f32(P(v), v.size, n, lo, hi, P(out))
    return out


def test_float_rule_on_special_values(emu):
    for n, lo, hi in ((64, 0, 1), (7, -1.5, 2.25), (256, 0, 256)):
        vals = np.array(R.f32_special_values(lo, hi), np.float32)
        got = emu_bins_f32(emu, vals, n, lo, hi)
        want = R.bins_vec(vals.reshape(1, -1), n, [lo, hi], True).ravel()
        loops = [R.bin_loops(float(v), "f", n, [np.float32(lo), np.float32(hi)], True) for v in vals]
        assert np.array_equal(got, want) and [(-1 if k is None else k) for k in loops] == want.tolist(), (n, lo, hi, got, want)
        assert got[0] == got[1] == got[2] == -1                              # NaN, +inf, -inf
        assert got[6] == -1 and got[7] == n - 1 and got[8] == -1             # hi is outside, the float below hi is the last bin, the float below lo is outside
        assert got[5] == 0                                                   # lo itself is the first bin
        if lo == 0:
            assert got[3] == got[4] == 0                                     # -0 and +0
    ab = np.zeros(2)
    emu.emu_calchist_coef(64, 0, 1, P(ab))
    assert tuple(ab) == R.coef(64, 0, 1) == (64.0, -0.0)


def fma_values():
    """(n, lo, hi, [(v, bin, fused bin)]) over ranges whose a and b are not exact"""
    out = []
    for n, lo, hi in R.FMA_RANGES:
        out.append((n, lo, hi, R.fma_sensitive(n, lo, hi, R.fma_candidates(n, lo, hi))))
    return out


def test_a_fused_multiply_add_would_be_another_function(emu):
    found = 0
    for n, lo, hi, sens in fma_values():
        cand = np.array(R.fma_candidates(n, lo, hi), np.float32)
        got = emu_bins_f32(emu, cand, n, lo, hi)
        assert np.array_equal(got, R.bins_vec(cand.reshape(1, -1), n, [lo, hi], True).ravel()), (n, lo, hi)
        for v, two, fused in sens:
            assert two != fused and emu_bins_f32(emu, [v], n, lo, hi)[0] == two == R.bin_loops(float(v), "f", n, [np.float32(lo), np.float32(hi)], True)
        found += len(sens)
    assert found >= 1                                                        # the set does hold values on which the two functions differ


def test_back_projection_rounding_and_saturation(emu):
    h = np.array([0, 1, 2.5, 3.5, 0.5, 1.5, 254.5, 255.5, 255, 256, 1e9, -1, -0.5, 65534.5, 65535.5, 70000, 3e38], np.float32)
    for depth, dt in ((0, np.uint8), (2, np.uint16)):
        for scale in (1.0, 0.37, 0.5, 2.0, -3.0, 1e-3):
            out = np.zeros(h.size, np.uint32)
            emu.emu_calchist_backproject(depth, P(h), h.size, scale, P(out))
            want = [R.round_half_even_sat(float(v) * scale, 0, int(np.iinfo(dt).max)) for v in h]
            assert out.tolist() == want, (depth, scale)
            vec = R.backproject_vec(np.arange(h.size, dtype=dt).reshape(1, -1), [0], h, [0, h.size], scale)
            assert vec.ravel().tolist() == want
    out = np.zeros(h.size, np.uint32)
    emu.emu_calchist_backproject(0, P(h), h.size, 1.0, P(out))
    assert out.tolist()[:10] == [0, 1, 2, 4, 0, 2, 254, 255, 255, 255]       # ties to even, the upper saturation
    assert out[11] == 0 and out[12] == 0 and out[10] == 255                  # the lower saturation
    for scale in (1.0, 0.37, 1e-40, 1e10):
        emu.emu_calchist_backproject(5, P(h), h.size, scale, P(out))
        with np.errstate(over="ignore"):
            want = (h.astype(np.float64) * scale).astype(np.float32)
        assert np.array_equal(out.view(np.float32), want)


def test_accumulate_conversions(emu):
    f = np.array([2.5, 3.5, -2.5, -3.5, 0.5, 1.5, 0.49999997, 7, -0.0, 3e9, -3e9, 2147483520.0, np.inf, -np.inf, 16777217.0], np.float32)
    out = np.zeros(f.size, np.int32)
    emu.emu_calchist_count_of_float(P(f), f.size, P(out))
    assert out.tolist()[:8] == [2, 4, -2, -4, 0, 2, 0, 7]
    assert out.tolist() == [R.round_half_even_sat(float(v), -2 ** 31, 2 ** 31 - 1) for v in f] == R.start_counts(f).tolist()
    assert out[9] == 2 ** 31 - 1 and out[10] == -2 ** 31 and out[12] == 2 ** 31 - 1 and out[13] == -2 ** 31
    c = np.array([0, 1, -1, 16777216, 16777217, 16777218, 16777219, 16785409, 2 ** 31 - 1, -2 ** 31], np.int32)
    back = np.zeros(c.size, np.float32)
    emu.emu_calchist_float_of_count(P(c), c.size, P(back))
    assert np.array_equal(back, c.astype(np.float32)) and np.array_equal(back, R.finish(c, R.CV_32F))
    assert back[4] == 16777216.0 and back[6] == 16777220.0 and back[7] == np.float32(16785409) == 16785408.0      # ties to even


# ---- the C ABI's refusals that need no device
ENTRIES = ("mi355cv_calcHist", "mi355cv_calcHistBatch", "mi355cv_calcBackProject", "mi355cv_calcBackProjectBatch")
COUNTERS = (b"calcHist", b"calcHistBatch", b"calcBackProject", b"calcBackProjectBatch")


def test_header_symbols_are_bound():
    from opencv_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mi355cv.h")).read()
    for name in ENTRIES:
        assert name + "(" in txt and name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_bounds_are_exposed_and_pinned():
    from opencv_amd import _lib
    assert _lib.limit(R.MAX_DIM_KEY) == 16384 == R.MAX_DIM
    assert _lib.limit(R.MAX_BINS_KEY) == 1048576 == R.MAX_BINS
    assert R.MAX_DIM * R.MAX_DIM <= 1 << 28 and R.MAX_BINS_PER_DIM == 65536


def test_entries_decline_bad_arguments_before_a_device_is_touched():
    """every decline that needs no device.  The two that classify pointers -- a histogram or destination that overlaps the source or the mask in HBM, and arguments on
    different devices -- come after the device is set: the overlaps are held in tests/test_calchist_gpu.py, the second needs two GPUs and is not tested."""
    from opencv_amd import _lib
    L = _lib.lib
    img = np.ones((16, 16, 4), np.float32)                                   # 16 x 16 of 4 channels, 256 bytes a row; read as CV_8U / CV_16U too
    msk = np.ones((16, 16), np.uint8)
    hist = np.full(4096, 7.0, np.float32)
    dst = np.full((16, 64), 7, np.uint8)
    n0 = sum(L.mi355cv_callCount(n) for n in COUNTERS)
    big = _lib.limit(R.MAX_DIM_KEY) + 1
    iarr = lambda v: (ctypes.c_int * len(v))(*v)
    farr = lambda v: (ctypes.c_float * len(v))(*v)
    vp = lambda x: P(x) if x is not None else None
    NOARG = object()

    def args(kw):
        a = dict(src=img, step=256, w=16, h=16, depth=0, cn=4, ch=[0, 1], hs=[8, 8], rg=[0, 256, 0, 256], uni=1, mask=None, mstep=16, hist=hist, hd=5, acc=0, nf=2, sf=2048,
                 mf=0, off=0, dst=dst, dstep=64, df=512, hf=0, scale=1.0)
        a.update(kw)
        a["dims"] = kw.get("dims", len(a["ch"]) if a["ch"] is not None else 1)
        a["srcp"] = ctypes.c_void_p(a["src"].ctypes.data + a["off"]) if a["src"] is not None else None
        for k in ("ch", "hs"):
            a[k] = iarr(a[k]) if a[k] is not None else None
        a["rg"] = farr(a["rg"]) if a["rg"] is not None else None
        return a

    def hist1(**kw):
        a = args(kw)
        return L.mi355cv_calcHist(a["srcp"], a["step"], a["w"], a["h"], a["depth"], a["cn"], a["ch"], a["dims"], a["hs"], a["rg"], a["uni"], vp(a["mask"]), a["mstep"],
                                  vp(a["hist"]), a["hd"], a["acc"])

    def histb(**kw):
        a = args(dict(h=8, **kw) if "h" not in kw else kw)
        return L.mi355cv_calcHistBatch(a["srcp"], a["step"], a["sf"], a["w"], a["h"], a["depth"], a["cn"], a["nf"], a["ch"], a["dims"], a["hs"], a["rg"], a["uni"], vp(a["mask"]),
                                       a["mstep"], a["mf"], vp(a["hist"]), a["hd"], a["acc"])

    def bp1(**kw):
        a = args(kw)
        return L.mi355cv_calcBackProject(a["srcp"], a["step"], a["w"], a["h"], a["depth"], a["cn"], a["ch"], a["dims"], a["hs"], a["rg"], a["uni"], vp(a["hist"]), a["scale"],
                                         vp(a["dst"]), a["dstep"])

    def bpb(**kw):
        a = args(dict(h=8, **kw) if "h" not in kw else kw)
        return L.mi355cv_calcBackProjectBatch(a["srcp"], a["step"], a["sf"], a["w"], a["h"], a["depth"], a["cn"], a["nf"], a["ch"], a["dims"], a["hs"], a["rg"], a["uni"],
                                              vp(a["hist"]), a["hf"], a["scale"], vp(a["dst"]), a["dstep"], a["df"])

    reason = lambda: L.mi355cv_lastError().decode()
    inf, nan = float("inf"), float("nan")
    for f in (hist1, histb, bp1, bpb):
        for name in ("src", "ch", "hs", "rg", "hist"):                       # null pointers
            assert f(**{name: None}) == NOT_IMPLEMENTED and ("!" + {"ch": "channels", "hs": "histSize", "rg": "ranges"}.get(name, name)) in reason(), (f.__name__, name, reason())
        for depth in (-1, 1, 3, 4, 6, 7):                                    # other depths
            assert f(depth=depth) == NOT_IMPLEMENTED and "depth is not CV_8U, CV_16U or CV_32F" in reason()
        for cn in (0, 5, -1):
            assert f(cn=cn) == NOT_IMPLEMENTED and "cn < 1 || cn > 4" in reason()
        for dims in (0, 4, -1):
            assert f(dims=dims) == NOT_IMPLEMENTED and "dims < 1 || dims > " in reason()
        for ch in ([0, 4], [-1, 0], [4, 4]):
            assert f(ch=ch) == NOT_IMPLEMENTED and "channel index" in reason()
        assert f(ch=[1, 1], cn=1) == NOT_IMPLEMENTED and "channel index" in reason()
        for hs in ([0, 8], [8, -1], [65537, 1]):                             # n_d < 1, n_d above its bound
            assert f(hs=hs) == NOT_IMPLEMENTED and "histSize is below 1 or above 65536" in reason()
        assert f(hs=[1024, 1025]) == NOT_IMPLEMENTED and "CALCHIST_MAX_BINS" in reason()          # the product just above the bound
        assert f(ch=[0, 1, 2], hs=[128, 128, 65], rg=[0, 256] * 3) == NOT_IMPLEMENTED and "CALCHIST_MAX_BINS" in reason()
        for rg in ([0, 0, 0, 256], [0, 256, 5, 4]):
            assert f(rg=rg) == NOT_IMPLEMENTED and "hi <= lo" in reason()
        for rg in ([0, inf, 0, 256], [-inf, 256, 0, 256], [0, 256, nan, 256]):
            assert f(rg=rg) == NOT_IMPLEMENTED and "not finite" in reason()
        assert f(uni=0, ch=[0], hs=[3], rg=[0, 5, 5, 9]) == NOT_IMPLEMENTED and "strictly ascending" in reason()
        assert f(uni=0, ch=[0], hs=[3], rg=[0, 5, 4, 9]) == NOT_IMPLEMENTED and "strictly ascending" in reason()
        assert f(uni=0, ch=[0], hs=[3], rg=[0, 5, 6, nan]) == NOT_IMPLEMENTED and "not finite" in reason()
        assert f(uni=0, depth=5, ch=[0], hs=[3], rg=[0, 5, 6, 9]) == NOT_IMPLEMENTED and "non-uniform ranges on CV_32F" in reason()
        assert f(w=0) == NOT_IMPLEMENTED and f(h=0) == NOT_IMPLEMENTED and f(w=-3) == NOT_IMPLEMENTED and f(h=-3) == NOT_IMPLEMENTED
        assert f(w=big, cn=1, ch=[0, 0], step=big) == NOT_IMPLEMENTED and f(h=big) == NOT_IMPLEMENTED and "CALCHIST_MAX_DIM" in reason()
        assert f(step=63) == NOT_IMPLEMENTED and "src_step is smaller than a row" in reason()       # 16 x 4 channels = 64 bytes
        assert f(depth=2, step=127) == NOT_IMPLEMENTED and "src_step is smaller than a row" in reason()
        assert f(depth=2, step=129) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
        assert f(depth=5, step=258) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
        assert f(depth=5, off=2) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
    for f in (hist1, histb):
        for hd in (0, 2, 3, 6, -1):
            assert f(hd=hd) == NOT_IMPLEMENTED and "hist_depth is neither CV_32S nor CV_32F" in reason()
        assert f(mask=msk, mstep=15) == NOT_IMPLEMENTED and "mask_step is smaller than a row" in reason()
    for f in (bp1, bpb):
        assert f(dst=None) == NOT_IMPLEMENTED and "!dst" in reason()
        assert f(dstep=15) == NOT_IMPLEMENTED and "dst_step is smaller than a row" in reason()
        assert f(depth=2, dstep=33) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
    for f in (histb, bpb):
        for nf in (0, -1, 65536):
            assert f(nf=nf) == NOT_IMPLEMENTED and "nframes" in reason()
        assert f(depth=2, sf=2049) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
    assert bpb(depth=5, df=514) == NOT_IMPLEMENTED and "multiple of the element size" in reason()
    assert sum(L.mi355cv_callCount(n) for n in COUNTERS) == n0
    assert np.all(hist == 7.0) and np.all(dst == 7)                          # nothing was written


def test_python_api_refuses_bad_arguments():
    import opencv_amd as cv
    for name in ("calcHist", "calcHistBatch", "calcBackProject", "calcBackProjectBatch"):
        assert name in cv.imgproc.__all__ and hasattr(cv, name), name
    a = np.zeros((8, 8, 3), np.uint8)
    h = np.zeros((4, 4), np.float32)
    n0 = cv._lib.decline_count()
    with pytest.raises(NotImplementedError):
        cv.calcHist([a, a], [0], None, [8], [0, 256])                        # several images in one call
    with pytest.raises(NotImplementedError):
        cv.calcBackProject([a, a], [0, 1], h, [0, 256, 0, 256], 1.0)
    with pytest.raises(ValueError):
        cv.calcHist(a, [0], None, [8], [0, 256])                             # not a list
    with pytest.raises(ValueError):
        cv.calcHist([a], [0, 1], None, [8], [0, 256])                        # one histSize for two channels
    with pytest.raises(ValueError):
        cv.calcHist([a], [0], None, [8], [0, 256, 0, 256])                   # too many range values
    with pytest.raises(ValueError):
        cv.calcHist([a], [0], None, [3], [0, 1, 2], uniform=False)           # n + 1 boundaries wanted
    with pytest.raises(ValueError):
        cv.calcHist([a], [0], np.zeros((8, 7), np.uint8), [8], [0, 256])     # the mask's size
    with pytest.raises(ValueError):
        cv.calcHist([a], [0], None, [8], [0, 256], dtype=np.float64)
    with pytest.raises(ValueError):
        cv.calcHist([a], [0], None, [8], [0, 256], accumulate=True)          # nothing to accumulate into
    with pytest.raises(ValueError):
        cv.calcHist([a], [0], None, [8], [0, 256], hist=np.zeros(9, np.float32))
    with pytest.raises(ValueError):
        cv.calcBackProject([a], [0], h, [0, 256], 1.0)                       # a 2-D histogram for one channel
    with pytest.raises(ValueError):
        cv.calcBackProject([a], [0, 1], h.astype(np.float64), [0, 256, 0, 256], 1.0)
    with pytest.raises(ValueError):
        cv.calcHistBatch(a[0], [0], None, [8], [0, 256])
    assert cv._lib.decline_count() == n0                                    # nothing reached the library
