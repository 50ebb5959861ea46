"""connectedComponents without a GPU: the restatement (tests/ccl_restate.py) against known answers and scipy.ndimage, the lines of opencv_amd/csrc/ccl_math.h
compiled for the host (tests/hostemu/ccl_emu.cpp) against that restatement, and the argument refusals of the four mi355cv_connectedComponents* entries that come
before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

import ccl_restate as R
import emubuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_IMPLEMENTED = 1
CV_8U, CV_8S, CV_16U, CV_16S, CV_32S, CV_32F, CV_64F = range(7)
DENSITIES = (0.1, 0.41, 0.59, 0.9)                  # 0.41 and 0.59: near the 8- and 4-connected percolation thresholds
U64 = (1 << 64) - 1


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- the restatement itself
def test_known_answers_the_two_orders_differ():
    a = np.array([[0, 0, 0, 1], [1, 0, 0, 0]], np.uint8)
    n, lab = R.label(a, 8, R.BLOCK)
    assert n == 3 and np.array_equal(lab, [[0, 0, 0, 2], [1, 0, 0, 0]])           # numbered left to right: block 0 holds (1, 0)
    n, lab = R.label(a, 8, R.PIXEL)
    assert n == 3 and np.array_equal(lab, [[0, 0, 0, 1], [2, 0, 0, 0]])           # numbered by first raster pixel


def test_known_answers_diagonal_pair_and_ring():
    d = np.array([[1, 0], [0, 1]], np.uint8)
    assert R.label(d, 8)[0] == 2 and np.array_equal(R.label(d, 8)[1], [[1, 0], [0, 1]])
    assert R.label(d, 4)[0] == 3 and np.array_equal(R.label(d, 4)[1], [[1, 0], [0, 2]])
    ring = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], np.uint8)
    for c in (4, 8):
        n, lab = R.label(ring, c)
        assert n == 2 and np.array_equal(lab, ring)
        st, ce = R.stats(lab, n)
        assert np.array_equal(st, [[1, 1, 1, 1, 1], [0, 0, 3, 3, 8]]) and np.array_equal(ce, [[1.0, 1.0], [1.0, 1.0]])


def test_empty_background_rule():
    n, lab = R.label(np.full((3, 4), 9, np.uint8), 8)
    assert n == 2 and np.all(lab == 1)
    st, ce = R.stats(lab, n)
    assert np.array_equal(st, [[0, 0, 0, 0, 0], [0, 0, 4, 3, 12]]) and np.all(np.isnan(ce[0])) and np.array_equal(ce[1], [1.5, 1.0])
    n, lab = R.label(np.zeros((3, 4), np.uint8), 4)
    assert n == 1 and not lab.any()


def test_patterns_are_what_they_claim():
    assert R.label(R.serpentine(33, 40), 4)[0] == 2 and R.label(R.comb(20, 41), 4)[0] == 2 and R.label(R.spiral(31, 45), 4)[0] == 2
    assert R.label(R.rings(20, 30), 8)[0] == 1 + 5
    assert R.label(R.checkerboard(7, 9), 8)[0] == 2 and R.label(R.checkerboard(7, 9), 4)[0] == 1 + (7 * 9 + 1) // 2
    d = R.diagonals(40, 300)
    assert R.label(d, 4)[0] > R.label(d, 8)[0]
    for flip in (0, 1):
        s = R.seam_pairs(40, 300, flip)
        assert R.label(s, 8)[0] - 1 == (R.label(s, 4)[0] - 1) // 2 > 0
    o = R.orders_differ(16, 64)
    assert (R.label(o, 8, R.PIXEL)[1] != R.label(o, 8, R.BLOCK)[1]).sum() == (o != 0).sum()


SHAPES = [(1, 1), (1, 2), (2, 1), (1, 37), (37, 1), (2, 2), (5, 7), (16, 16), (33, 65), (64, 130), (100, 100), (257, 300)]


def test_restatement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    structure = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: np.ones((3, 3), int)}
    for i, (h, w) in enumerate(SHAPES):
        for dens in DENSITIES:
            a = R.random_frame(rng, h, w, dens)
            for c in (4, 8):
                want, k = ndi.label(a, structure[c])
                n, lab = R.label(a, c, R.PIXEL)
                assert n == k + 1 and lab.dtype == np.int32 and np.array_equal(lab, want), (h, w, dens, c)
                st, ce = R.stats(lab, n)
                objs = ndi.find_objects(lab)
                com = ndi.center_of_mass(np.ones_like(lab), lab, range(1, n)) if n > 1 else []
                for j in range(1, n):
                    ys, xs = objs[j - 1]
                    assert tuple(st[j]) == (xs.start, ys.start, xs.stop - xs.start, ys.stop - ys.start, int((lab == j).sum()))
                    assert abs(ce[j, 0] - com[j - 1][1]) < 1e-9 and abs(ce[j, 1] - com[j - 1][0]) < 1e-9
                assert st[0, 4] == int((lab == 0).sum()) and st[:, 4].sum() == h * w


def test_block_order_is_the_permutation_by_block_key():
    rng = np.random.default_rng(3)
    for h, w in ((2, 4), (7, 9), (33, 65), (64, 130)):
        for dens in DENSITIES + (0.03,):
            a = R.random_frame(rng, h, w, dens)
            n, pix = R.label(a, 8, R.PIXEL)
            nb, blk = R.label(a, 8, R.BLOCK)
            assert n == nb and np.array_equal(pix == 0, blk == 0)
            yy, xx = np.mgrid[0:h, 0:w]
            key = (yy >> 1) * ((w + 1) >> 1) + (xx >> 1)
            kmin = np.array([key[pix == j].min() for j in range(1, n)], np.int64)
            assert len(set(kmin.tolist())) == n - 1                                       # a block meets one component at most
            perm = np.zeros(n, np.int32)
            perm[1 + np.argsort(kmin)] = np.arange(1, n)
            assert np.array_equal(perm[pix], blk), (h, w, dens)


# ---- ccl_math.h on the host
@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("ccl_emu.cpp", "libccl_emu.so", ["-ffp-contract=off"])
    u64, i32 = ctypes.c_uint64, ctypes.c_int
    lib.emu_ccl.restype = i32
    lib.emu_ccl.argtypes = [ctypes.c_void_p, ctypes.c_size_t, i32, i32, i32, i32, ctypes.c_void_p]
    lib.emu_ccl_stats.restype = i32
    lib.emu_ccl_stats.argtypes = [ctypes.c_void_p, i32, i32, i32, ctypes.c_void_p, ctypes.c_void_p]
    for name, args, res in (("run_start", [u64, i32], i32), ("run_end", [u64, i32], i32), ("tile_run_start", [ctypes.c_void_p, i32, i32], i32),
                            ("row_word", [u64, u64, u64, u64, i32], u64), ("link8", [u64, u64, i32, i32], u64), ("link_direct", [u64, u64, i32, i32], u64),
                            ("link_left", [u64, u64, i32, i32], u64), ("link_right", [u64, u64, i32, i32], u64), ("run_sum_x", [ctypes.c_uint32, ctypes.c_uint32], u64),
                            ("block_key", [i32, i32, i32], ctypes.c_uint32), ("order_of", [i32, i32], i32)):
        f = getattr(lib, "emu_ccl_" + name)
        f.argtypes, f.restype = args, res
    return lib


def bits(v):
    return [(v >> i) & 1 for i in range(64)]


def words(rng):
    edge = [U64, 0, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0xFFFF000000000000, 1 << 63, 1, 0x7FFFFFFFFFFFFFFF, U64 - 1, 0xF00000000000000F]
    return edge + [int(x) for x in rng.integers(0, 1 << 63, 30, dtype=np.uint64) * 2 + rng.integers(0, 2, 30, dtype=np.uint64)] + \
        [int(x) for x in (rng.integers(0, 1 << 63, 10, dtype=np.uint64) | rng.integers(0, 1 << 63, 10, dtype=np.uint64)) << np.uint64(1)]


def test_run_start_and_end_for_every_lane(emu):
    rng = np.random.default_rng(4)
    for m in words(rng):
        b = bits(m)
        for lane in range(64):
            if not b[lane]:
                continue
            s = lane
            while s > 0 and b[s - 1]:
                s -= 1
            e = lane
            while e < 64 and b[e]:
                e += 1
            assert emu.emu_ccl_run_start(m, lane) == s and emu.emu_ccl_run_end(m, lane) == e, (hex(m), lane)


def test_run_start_across_the_words_of_a_tile(emu):
    rng = np.random.default_rng(5)
    for _ in range(40):
        row = (rng.random(256) < rng.choice([0.5, 0.9, 0.99, 1.0])).astype(np.uint8)
        W = np.array([sum(int(row[64 * j + i]) << i for i in range(64)) for j in range(4)], np.uint64)
        for c in np.flatnonzero(row):
            s = int(c)
            while s > 0 and row[s - 1]:
                s -= 1
            assert emu.emu_ccl_tile_run_start(P(W), int(c) >> 6, int(c) & 63) == s


def test_row_word_interleaves_the_byte_ballots(emu):
    rng = np.random.default_rng(6)
    for _ in range(20):
        row = (rng.random(256) < 0.5).astype(np.uint8)
        b = [sum(int(row[4 * l + k]) << l for l in range(64)) for k in range(4)]
        for j in range(4):
            assert emu.emu_ccl_row_word(b[0], b[1], b[2], b[3], j) == sum(int(row[64 * j + i]) << i for i in range(64))


def test_links_with_their_carries(emu):
    """the 8-connected link word, and the cut into direct / left / right pairs: together they name every touching (run, run above) pair and nothing else"""
    rng = np.random.default_rng(7)
    ws = words(rng)
    for i in range(len(ws)):
        W, U = ws[i], ws[(i * 7 + 3) % len(ws)]
        for Wl, Ul, Wr, Ur in ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0)):
            w, u = [Wl] + bits(W) + [Wr], [Ul] + bits(U) + [Ur]                           # index c + 1 = column c
            want8 = sum((w[c + 1] & (u[c] | u[c + 1] | u[c + 2])) << c for c in range(64))
            assert emu.emu_ccl_link8(W, U, Ul, Ur) == want8
            d, l, r = emu.emu_ccl_link_direct(W, U, Wl, Ul), emu.emu_ccl_link_left(W, U, Wl, Ul), emu.emu_ccl_link_right(W, U, Wr, Ur)
            assert (d | l | r) & ~want8 == 0 and d & ~(W & U) == 0 and l & r & U == 0
            both = [w[c] & u[c] for c in range(66)]
            assert d == sum((both[c + 1] & (1 - both[c])) << c for c in range(64))          # the first bit of every run of W & U, runs coming in from the left word cut
            for c in range(64):
                if not w[c + 1] or u[c + 1]:
                    continue
                # above c is empty: the diagonal neighbours are pairs of their own unless the pixel beside c has them right above it
                assert ((l >> c) & 1) == (1 if u[c] and not w[c] else 0)
                assert ((r >> c) & 1) == (1 if u[c + 2] and not w[c + 2] else 0)


def test_closed_forms(emu):
    rng = np.random.default_rng(8)
    for x, n in [(0, 1), (0, 64), (16383, 1), (16320, 64), (5, 0)] + [(int(a), int(b)) for a, b in zip(rng.integers(0, 16384, 50), rng.integers(1, 65, 50))]:
        assert emu.emu_ccl_run_sum_x(x, n) == sum(range(x, x + n))
    for x, y, w in ((0, 0, 1), (3, 2, 5), (16383, 16383, 16384), (7, 9, 8), (6, 1, 7)):
        assert emu.emu_ccl_block_key(x, y, w) == (y >> 1) * ((w + 1) >> 1) + (x >> 1)
    for c in (4, 8):
        for t in range(-3, 8):
            want = -1 if t < -1 or t > 5 else (0 if R.order_of(c, t) == R.PIXEL else 1)
            assert emu.emu_ccl_order_of(c, t) == want
    assert emu.emu_ccl_tile_w() == R.TILE_W and emu.emu_ccl_strip_h() == R.STRIP_H and emu.emu_ccl_max_dim() == R.MAX_DIM


def _emu_label(emu, a, connectivity, ccltype):
    h, w = a.shape
    lab = np.full((h, w), -7, np.int32)
    n = emu.emu_ccl(P(a), a.strides[0], w, h, connectivity, ccltype, P(lab))
    return n, lab


def _check(emu, a, what=""):
    a = np.ascontiguousarray(a)
    for c, t in ((4, R.CCL_DEFAULT), (8, R.CCL_SAUF), (8, R.CCL_DEFAULT)):
        n, lab = _emu_label(emu, a, c, t)
        wn, want = R.label(a, c, R.order_of(c, t))
        assert n == wn and np.array_equal(lab, want), (what, a.shape, c, t)
        st = np.full((n, 5), -7, np.int32)
        ce = np.full((n, 2), -7.0, np.float64)
        assert emu.emu_ccl_stats(P(lab), a.shape[1], a.shape[0], n, P(st), P(ce)) == 0
        assert R.same_stats(st, ce, *R.stats(want, wn)), (what, a.shape, c, t)


T, S = R.TILE_W, R.STRIP_H


@pytest.mark.parametrize("h,w", [(S - 1, T - 1), (S, T), (S + 1, T + 1), (2 * S + 1, 2 * T + 1), (37, 70)])
def test_emulated_kernels_on_the_pattern_list(emu, h, w):
    for name, a in R.patterns(h, w).items():
        _check(emu, a, name)


def test_emulated_kernels_on_lines_and_small_frames(emu):
    rng = np.random.default_rng(9)
    _check(emu, np.ones((1, 1), np.uint8)); _check(emu, np.zeros((1, 1), np.uint8))
    for n in (2, 63, 64, 65, 255, 256, 257):
        for dens in (0.5, 0.9):
            _check(emu, R.random_frame(rng, 1, n, dens)); _check(emu, R.random_frame(rng, n, 1, dens))
        _check(emu, np.ones((1, n), np.uint8)); _check(emu, np.ones((n, 1), np.uint8))
    for h, w in SHAPES:
        for dens in DENSITIES:
            _check(emu, R.random_frame(rng, h, w, dens))


def test_emulated_stats_skip_values_that_are_no_label(emu):
    lab = np.array([[0, 1, 1, 9], [2, 2, -1, 1]], np.int32)
    st = np.zeros((3, 5), np.int32); ce = np.zeros((3, 2), np.float64)
    assert emu.emu_ccl_stats(P(lab), 4, 2, 3, P(st), P(ce)) == 0
    assert R.same_stats(st, ce, *R.stats(lab, 3)) and st[:, 4].tolist() == [1, 3, 2]


# ---- the C ABI's refusals that need no device
ENTRIES = ("mi355cv_connectedComponents", "mi355cv_connectedComponentsBatch", "mi355cv_connectedComponentsStats", "mi355cv_connectedComponentsStatsBatch")
COUNTERS = (b"connectedComponents", b"connectedComponentsBatch", b"connectedComponentsStats", b"connectedComponentsStatsBatch")


def test_header_symbols_are_bound():
    from opencv_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mi355cv.h")).read()
    for name in ENTRIES:
        assert name + "(" in txt and name in _lib.SIGNATURES and hasattr(_lib.lib, name)


def test_bound_is_exposed_and_pinned():
    from opencv_amd import _lib
    top = _lib.limit(R.LIMIT_KEY)
    assert top == 16384 == R.MAX_DIM
    assert top * top <= 1 << 28 and top * top * (top - 1) < 1 << 53                       # pixel indices and areas in 32 bits, coordinate sums exact in a double


def test_label_entries_decline_bad_arguments():
    from opencv_amd import _lib
    L = _lib.lib
    a = np.ones((16, 16), np.uint8)
    d = np.full((16, 16), 7, np.int32)
    d16 = np.full((16, 16), 7, np.uint16)
    nl = (ctypes.c_int * 4)(-5, -5, -5, -5)
    n0 = sum(L.mi355cv_callCount(n) for n in COUNTERS)

    def one(conn=8, ltype=CV_32S, ccl=-1, dst=d, w=16, h=16, src=a, n=nl):
        return L.mi355cv_connectedComponents(P(src) if src is not None else None, 16, w, h, P(dst) if dst is not None else None, 64, conn, ltype, ccl, n)

    def batch(conn=8, ltype=CV_32S, ccl=-1, dst=d, w=16, h=16, src=a, n=nl, nf=1):
        return L.mi355cv_connectedComponentsBatch(P(src) if src is not None else None, 16, 256, w, h, P(dst) if dst is not None else None, 64, 1024, nf, conn, ltype, ccl, n)

    reason = lambda: L.mi355cv_lastError().decode()
    for f in (one, batch):
        for conn in (0, 1, 6, 16, -4):
            assert f(conn=conn) == NOT_IMPLEMENTED and "connectivity" in reason()
        for lt in (CV_8U, CV_8S, CV_16S, CV_32F, CV_64F, 7, -1):
            assert f(ltype=lt) == NOT_IMPLEMENTED and "ltype" in reason()
        for t in (-2, 6, 100):
            assert f(ccl=t) == NOT_IMPLEMENTED and "ccltype" in reason()
        assert f(w=R.MAX_DIM + 1) == NOT_IMPLEMENTED and "CCL_MAX_DIM" in reason()
        assert f(h=R.MAX_DIM + 1) == NOT_IMPLEMENTED and "CCL_MAX_DIM" in reason()
        assert f(w=0) == NOT_IMPLEMENTED and f(h=-3) == NOT_IMPLEMENTED
        assert f(src=None) == NOT_IMPLEMENTED and "src" in reason()
        assert f(dst=None) == NOT_IMPLEMENTED and "labels" in reason()
        assert f(n=None) == NOT_IMPLEMENTED and "nlabels" in reason()
        assert f(ltype=CV_16U, dst=d16, conn=5) == NOT_IMPLEMENTED
    assert batch(nf=0) == NOT_IMPLEMENTED and "nframes" in reason()
    assert batch(nf=-1) == NOT_IMPLEMENTED
    assert sum(L.mi355cv_callCount(n) for n in COUNTERS) == n0
    assert np.all(d == 7) and np.all(d16 == 7) and list(nl) == [-5] * 4


def test_stats_entries_decline_bad_arguments():
    from opencv_amd import _lib
    L = _lib.lib
    lab = np.zeros((16, 16), np.int32)
    st = np.full((4, 5), 7, np.int32)
    ce = np.full((4, 2), 7.0, np.float64)
    nl = (ctypes.c_int * 2)(3, 4)
    n0 = sum(L.mi355cv_callCount(n) for n in COUNTERS)

    def one(ltype=CV_32S, n=4, w=16, h=16, labels=lab, stats=st):
        return L.mi355cv_connectedComponentsStats(P(labels) if labels is not None else None, 64, w, h, ltype, n, P(stats) if stats is not None else None, 20, P(ce), 16)

    def batch(ltype=CV_32S, n=nl, mx=4, w=16, h=16, labels=lab, stats=st, nf=1):
        return L.mi355cv_connectedComponentsStatsBatch(P(labels) if labels is not None else None, 64, 1024, w, h, ltype, nf, n, mx,
                                                      P(stats) if stats is not None else None, 20, 80, P(ce), 16, 32)

    reason = lambda: L.mi355cv_lastError().decode()
    for f in (one, batch):
        for lt in (CV_8U, CV_16S, CV_32F, CV_64F):
            assert f(ltype=lt) == NOT_IMPLEMENTED and "ltype" in reason()
        assert f(w=R.MAX_DIM + 1) == NOT_IMPLEMENTED and "CCL_MAX_DIM" in reason()
        assert f(h=0) == NOT_IMPLEMENTED
        assert f(labels=None) == NOT_IMPLEMENTED and "labels" in reason()
        assert f(stats=None) == NOT_IMPLEMENTED and "stats" in reason()
    assert one(n=0) == NOT_IMPLEMENTED and "nlabels" in reason()
    assert one(n=-2) == NOT_IMPLEMENTED
    assert batch(nf=0) == NOT_IMPLEMENTED and "nframes" in reason()
    assert batch(n=None) == NOT_IMPLEMENTED and "nlabels" in reason()
    assert batch(nf=2, mx=3) == NOT_IMPLEMENTED and "max_labels" in reason()               # nlabels[1] = 4 > max_labels
    assert batch(mx=0) == NOT_IMPLEMENTED and "max_labels" in reason()
    assert sum(L.mi355cv_callCount(n) for n in COUNTERS) == n0
    assert np.all(st == 7) and np.all(ce == 7.0)


def test_python_api_refuses_what_the_reference_asserts_on():
    import opencv_amd as cv
    names = ("connectedComponents", "connectedComponentsWithStats", "connectedComponentsBatch", "connectedComponentsWithStatsBatch", "CC_STAT_LEFT", "CC_STAT_TOP",
             "CC_STAT_WIDTH", "CC_STAT_HEIGHT", "CC_STAT_AREA", "CC_STAT_MAX", "CCL_DEFAULT", "CCL_WU", "CCL_GRANA", "CCL_BOLELLI", "CCL_SAUF", "CCL_BBDT", "CCL_SPAGHETTI")
    for name in names:
        assert name in cv.imgproc.__all__ and hasattr(cv, name), name
    assert (cv.CC_STAT_LEFT, cv.CC_STAT_TOP, cv.CC_STAT_WIDTH, cv.CC_STAT_HEIGHT, cv.CC_STAT_AREA, cv.CC_STAT_MAX) == (0, 1, 2, 3, 4, 5)
    assert (cv.CCL_DEFAULT, cv.CCL_WU, cv.CCL_GRANA, cv.CCL_BOLELLI, cv.CCL_SAUF, cv.CCL_BBDT, cv.CCL_SPAGHETTI) == (-1, 0, 1, 2, 3, 4, 5)
    a = np.zeros((8, 8), np.uint8)
    for fn in (cv.connectedComponents, cv.connectedComponentsWithStats):
        for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8), np.uint16), np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 1), np.uint8), np.zeros((8, 8), np.int8)):
            with pytest.raises(ValueError):
                fn(bad)
        for conn in (0, 6, 16):
            with pytest.raises(ValueError):
                fn(a, connectivity=conn)
        for lt in (cv.CV_8U, cv.CV_16S, cv.CV_32F):
            with pytest.raises(ValueError):
                fn(a, ltype=lt)
        with pytest.raises(ValueError):
            fn(a, labels=np.zeros((8, 9), np.int32))
        with pytest.raises(ValueError):
            fn(a, labels=np.zeros((8, 8), np.uint16))                                      # ltype is CV_32S
    with pytest.raises(ValueError):
        cv.connectedComponentsBatch(a)
    with pytest.raises(ValueError):
        cv.connectedComponentsWithStatsBatch(a)
