"""cv::BFMatcher without a GPU: the two forms of the restatement (tests/bfmatch_restate.py) against each other bit for bit, hand-computed known answers, the lines of
opencv_amd/csrc/bfmatch_math.h compiled for the host (tests/hostemu/bfmatch_emu.cpp) against the restatement -- distances, keys, insertion --, the refusals of the
mi355cv_bf* entries that come before any device is touched, the limits and the layout of mi355cv_DMatch."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import bfmatch_restate as R
import emubuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS_8U = (R.NORM_HAMMING, R.NORM_HAMMING2)
NORMS_32F = (R.NORM_L1, R.NORM_L2, R.NORM_L2SQR)


def same(a, b):
    """record planes / lists equal bit for bit (the float field as its bit pattern)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _sets(norm, rng, nq=9, nts=(7, 5), length=6):
    if norm in NORMS_8U:
        return R.tie_heavy(rng, nq, length), [R.tie_heavy(rng, n, length) for n in nts]
    Q, Ts = R.tie_heavy_float(rng, nq, length), [R.tie_heavy_float(rng, n, length) for n in nts]
    Ts[0][1, 2] = np.nan                                                              # a row no query is a candidate of
    return Q, Ts


@pytest.mark.parametrize("norm", NORMS_8U + NORMS_32F)
def test_the_two_forms_of_the_restatement_agree(norm):
    rng = np.random.default_rng(norm)
    Q, Ts = _sets(norm, rng)
    for q in range(len(Q)):
        for t in range(len(Ts[0])):
            a, b = R.distance_loops(Q[q], Ts[0][t], norm), R.distances_np(Q[q:q + 1], Ts[0][t:t + 1], norm)[0, 0]
            assert a.tobytes() == b.tobytes(), (q, t, a, b)
    masks = [rng.integers(0, 2, (len(Q), len(Ts[0])), dtype=np.uint8) * 255, None]
    masks[0][3] = 0
    for ms in (None, masks):
        for k in (1, 3, 20):
            (a, ca), (b, cb) = R.knn_loops(Q, Ts, ms, norm, k), R.knn_np(Q, Ts, ms, norm, k)
            assert same(a, b) and np.array_equal(ca, cb), (k, ms is not None)
        dist = np.unique(R.distances_np(Q, Ts[1], norm))
        for md in (0.0, float(dist[len(dist) // 2]), -1.0):
            la, lb = R.radius_loops(Q, Ts, ms, norm, md), R.radius_np(Q, Ts, ms, norm, md)
            assert len(la) == len(lb) and all(same(x, y) for x, y in zip(la, lb)), md
    (a, ca), (b, cb) = R.cross_loops(Q, Ts[0], norm), R.cross_np(Q, Ts[0], norm)
    assert same(a, b) and np.array_equal(ca, cb)
    assert 0 < ca.sum() <= min(len(Q), len(Ts[0]))


def test_known_answers():
    # both Hamming norms on two-byte rows: q ^ t = {1100 0011, 0000 0110}: 6 bits set; non-zero 2-bit groups: 2 + 2
    q, t = np.array([[0xC3, 0x06]], np.uint8), np.array([[0, 0]], np.uint8)
    for f in (lambda n: R.distance_loops(q[0], t[0], n), lambda n: R.distances_np(q, t, n)[0, 0]):
        assert f(R.NORM_HAMMING) == 6 and f(R.NORM_HAMMING2) == 4
    # L1: 2^24 + 1 + 1 in THIS order stays 2^24 (each 1 is half an ulp and the tie goes to even); any other order gives 2^24 + 2
    q, z = np.array([[2.0 ** 24, 1, 1]], np.float32), np.zeros((1, 3), np.float32)
    assert R.distances_np(q, z, R.NORM_L1)[0, 0] == np.float32(2.0 ** 24) == R.distance_loops(q[0], z[0], R.NORM_L1)
    assert R.distances_np(q[:, ::-1], z, R.NORM_L1)[0, 0] == np.float32(2.0 ** 24 + 2)
    # L2SQR: the same with squares; and a product that must be rounded before it is added: x = {2^-12, 1 + 2^-12}: fl(x1^2) = 1 + 2^-11 (the 2^-24 is a tie, to even),
    # 2^-24 + that is a tie again, to even: 1 + 2^-11.  A fused multiply-add would give 1 + 2^-11 + 2^-23.
    q = np.array([[4096, 1, 1]], np.float32)
    assert R.distances_np(q, z, R.NORM_L2SQR)[0, 0] == np.float32(2.0 ** 24) and R.distances_np(q, z, R.NORM_L2)[0, 0] == np.float32(4096)
    q = np.array([[2.0 ** -12, 1 + 2.0 ** -12]], np.float32)
    for d in (R.distances_np(q, z[:, :2], R.NORM_L2SQR)[0, 0], R.distance_loops(q[0], z[0, :2], R.NORM_L2SQR)):
        assert d == np.float32(1 + 2.0 ** -11) and d != np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    # a three-way tie resolved by (imgIdx, trainIdx): distances to q = 0 are {1, 2} in image 0 and {1, 1} in image 1
    q, trains = np.array([[0]], np.uint8), [np.array([[1], [3]], np.uint8), np.array([[2], [4]], np.uint8)]
    for f in (R.knn_loops, R.knn_np):
        out, cnt = f(q, trains, None, R.NORM_HAMMING, 5)
        assert cnt[0] == 4
        assert [(m["imgIdx"], m["trainIdx"], m["distance"]) for m in out[0, :4]] == [(0, 0, 1.0), (1, 0, 1.0), (1, 1, 1.0), (0, 1, 2.0)]
        assert out[0, 4] == R.PAD
    # crossCheck: q0's best train row t0 prefers q1 (distance 0), so only (q1, t0) survives
    Q, T = np.array([[0], [1]], np.uint8), np.array([[1], [7]], np.uint8)
    for f in (R.cross_loops, R.cross_np):
        out, cnt = f(Q, T, R.NORM_HAMMING)
        assert cnt.tolist() == [0, 1] and out[0, 0] == R.PAD and out[1, 0] == np.array((1, 0, 0, 0.0), R.DMATCH)


@functools.lru_cache(maxsize=1)
def emu():
    # the library's own flag: every product and sum is rounded on its own
    lib = emubuild.load("bfmatch_emu.cpp", "libbfmatch_emu.so", ["-ffp-contract=off"])
    i32, u32, vp, u64, f32 = ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_float
    lib.emu_bf_distance.argtypes, lib.emu_bf_distance.restype = [i32, i32, vp, vp, i32], f32
    lib.emu_bf_hamming_words.argtypes, lib.emu_bf_hamming_words.restype = [i32, vp, vp, i32], u32
    lib.emu_bf_key_float.argtypes, lib.emu_bf_key_float.restype = [f32, u32], u64
    lib.emu_bf_key_int.argtypes, lib.emu_bf_key_int.restype = [u32, u32], u64
    lib.emu_bf_key_distance.argtypes, lib.emu_bf_key_distance.restype = [u64, i32], f32
    lib.emu_bf_no_key.restype = u64
    lib.emu_bf_knn.argtypes = [i32, i32, vp, i32, vp, i32, i32, i32, i32, vp]
    return lib


@pytest.mark.parametrize("norm", NORMS_8U + NORMS_32F)
def test_bfmatch_math_on_the_host_matches_the_restatement(norm):
    E = emu()
    rng = np.random.default_rng(100 + norm)
    is_float = int(norm in NORMS_32F)
    for length in ((1, 2, 31, 32, 33, 64) if not is_float else (1, 4, 33)):
        if is_float:
            Q, T = R.tie_heavy_float(rng, 11, length), R.tie_heavy_float(rng, 13, length)
            Q[0] = rng.standard_normal(length).astype(np.float32) * 1e3                   # rows whose sums round
            T[1] = rng.standard_normal(length).astype(np.float32) * 1e-3
            T[2, 0] = np.nan
            T[3, 0] = np.inf
        else:
            Q, T = R.tie_heavy(rng, 11, length), R.tie_heavy(rng, 13, length)
            Q[0] = rng.integers(0, 256, length)
        D = R.distances_np(Q, T, norm)
        for q in range(len(Q)):
            for t in range(len(T)):
                got = np.float32(E.emu_bf_distance(is_float, norm, Q[q].ctypes.data, T[t].ctypes.data, length))
                assert got.tobytes() == D[q, t].tobytes(), (length, q, t, got, D[q, t])
        if not is_float and length % 4 == 0:
            for q in range(len(Q)):
                for t in range(len(T)):
                    assert E.emu_bf_hamming_words(int(norm == R.NORM_HAMMING2), Q[q].ctypes.data, T[t].ctypes.data, length // 4) == int(D[q, t])
        # insertion: the k smallest keys, whatever the order the rows arrive in
        for k in (1, 2, 4, 8):
            want, cnt = R.knn_np(Q, [T], None, norm, k)
            for stride in (1, 5, 12):
                keys = np.zeros((len(Q), k), np.uint64)
                assert E.emu_bf_knn(is_float, norm, Q.ctypes.data, len(Q), T.ctypes.data, len(T), length, k, stride, keys.ctypes.data) == 0
                for q in range(len(Q)):
                    for j in range(k):
                        if j >= cnt[q]:
                            assert int(keys[q, j]) == E.emu_bf_no_key()
                            continue
                        assert int(keys[q, j]) & 0xffffffff == want["trainIdx"][q, j]
                        assert np.float32(E.emu_bf_key_distance(int(keys[q, j]), is_float)).tobytes() == want["distance"][q, j].tobytes()


def test_keys_order_like_the_rule():
    E = emu()
    d = np.array([0.0, 1e-45, 1e-38, 0.5, 1.0, np.nextafter(np.float32(1), np.float32(2)), 3e38, np.inf], np.float32)
    keys = [E.emu_bf_key_float(float(v), r) for v in d for r in (0, 1, 0xfffffffe)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert E.emu_bf_key_float(float("nan"), 3) == E.emu_bf_no_key() and max(keys) < E.emu_bf_no_key()
    ik = [E.emu_bf_key_int(v, r) for v in (0, 1, 2, 16384) for r in (0, 7, 0xfffffffe)]
    assert ik == sorted(ik) and E.emu_bf_key_distance(E.emu_bf_key_int(16384, 5), 0) == 16384.0


LIMITS = {"bfmatch_max_rows": 1 << 24, "bfmatch_max_k": 8, "bfmatch_max_row_bytes": 2048, "bfmatch_max_images": 64, "bfmatch_max_radius_row": 4096,
          "bfmatch_tile_rows": 256, "bfmatch_split_rows": 512}


def test_limits_are_pinned():
    """how far the matcher was built; tests/test_bfmatch_gpu.py derives every refusal it asserts from mi355cv_limit and runs parity at k = bfmatch_max_k, across
    bfmatch_tile_rows and bfmatch_split_rows.  The issue's floors: k >= 8, rows of >= 2048 bytes, radius lists of >= 4096."""
    from opencv_amd import _lib
    E = emu()
    for i, (k, v) in enumerate(LIMITS.items()):
        assert _lib.limit(k) == v == E.emu_bf_limit(i), k
    assert LIMITS["bfmatch_max_k"] >= 8 and LIMITS["bfmatch_max_row_bytes"] >= 2048 and LIMITS["bfmatch_max_radius_row"] >= 4096
    assert LIMITS["bfmatch_split_rows"] % LIMITS["bfmatch_tile_rows"] == 0


def test_refusals_before_a_device_is_touched():
    from opencv_amd import _lib
    L = _lib.lib
    NI = _lib.NOT_IMPLEMENTED
    q8, t8 = np.zeros((4, 32), np.uint8), np.zeros((5, 32), np.uint8)
    qf, tf = np.zeros((4, 8), np.float32), np.zeros((5, 8), np.float32)
    out, cnt = np.zeros((4, 8), R.DMATCH), np.zeros(4, np.int32)
    reason = lambda: L.mi355cv_lastError().decode()

    def knn(q=q8, t=t8, nq=4, nt=(5,), length=32, typ=0, norm=6, k=1, cross=0, masks=None, nimg=1, qstep=None, tstep=None):
        n = len(nt)
        tp = (ctypes.c_void_p * n)(*[t.ctypes.data] * n)
        ts = (ctypes.c_size_t * n)(*[t.strides[0] if tstep is None else tstep] * n)
        tr = (ctypes.c_int * n)(*nt)
        mp = ms = None
        if masks is not None:
            mp = (ctypes.c_void_p * n)(*[m.ctypes.data if m is not None else None for m in masks])
            ms = (ctypes.c_size_t * n)(*[m.strides[0] if m is not None else 0 for m in masks])
        return L.mi355cv_bfKnnMatch(q.ctypes.data, q.strides[0] if qstep is None else qstep, nq, length, typ, tp, ts, tr, mp, ms, nimg, norm, k, cross, out.ctypes.data, cnt.ctypes.data)

    top = _lib.limit
    cases = [
        (dict(q=qf, t=tf, length=8, typ=5, norm=6), "CV_32F descriptors are served with NORM_L1"),
        (dict(norm=4), "CV_8U descriptors are served with NORM_HAMMING"),
        (dict(typ=2), "neither CV_8UC1 nor CV_32FC1"),
        (dict(k=top("bfmatch_max_k") + 1), "BFMATCH_MAX_K"), (dict(k=0), "k < 1"),
        (dict(length=top("bfmatch_max_row_bytes") + 1, qstep=4096, tstep=4096), "BFMATCH_MAX_ROW_BYTES"),
        (dict(q=qf, t=tf, typ=5, norm=4, length=top("bfmatch_max_row_bytes") // 4 + 1, qstep=4096, tstep=4096), "BFMATCH_MAX_ROW_BYTES"),
        (dict(length=0), "len < 1"),
        (dict(nq=top("bfmatch_max_rows") + 1), "BFMATCH_MAX_ROWS"),
        (dict(nt=(top("bfmatch_max_rows"), 1), nimg=2), "BFMATCH_MAX_ROWS"),
        (dict(nt=(1,) * (top("bfmatch_max_images") + 1), nimg=top("bfmatch_max_images") + 1), "BFMATCH_MAX_IMAGES"),
        (dict(qstep=31), "a step below the row"), (dict(tstep=31), "a step below the row"),
        (dict(q=qf, t=tf, length=8, typ=5, norm=4, qstep=34), "off a 4-byte boundary"),
        (dict(cross=1, masks=[np.ones((4, 5), np.uint8)]), "crossCheck together with a mask"),
        (dict(cross=1, nt=(2, 3), nimg=2), "crossCheck with more than one train matrix"),
        (dict(masks=[np.ones((4, 4), np.uint8)]), "mask: a step below nt bytes"),
    ]
    for kw, why in cases:
        assert knn(**kw) == NI, kw
        assert why in reason(), (kw, reason())
    assert knn(cross=1, k=2) == -1 and "crossCheck is defined for k = 1 only" in reason()
    # radiusMatch answers -1 for what it does not serve, with the same reasons
    tp, ts, tr = (ctypes.c_void_p * 1)(t8.ctypes.data), (ctypes.c_size_t * 1)(32), (ctypes.c_int * 1)(5)
    assert L.mi355cv_bfRadiusMatch(q8.ctypes.data, 32, 4, 32, 0, tp, ts, tr, None, None, 1, 4, 1.0, out.ctypes.data, 32, cnt.ctypes.data) == -1 and "NORM_HAMMING" in reason()
    assert L.mi355cv_bfRadiusMatch(q8.ctypes.data, 32, 4, 32, 0, tp, ts, tr, None, None, 1, 6, 1.0, out.ctypes.data, -1, cnt.ctypes.data) == -1 and "capacity < 0" in reason()
    assert L.mi355cv_bfRadiusMatch(q8.ctypes.data, 32, 0, 32, 0, tp, ts, tr, None, None, 1, 6, 1.0, out.ctypes.data, 32, cnt.ctypes.data) == 0        # no query: no match, no device
    # the Python mirror's own argument errors
    import opencv_amd as cv
    with pytest.raises(ValueError, match="crossCheck is defined for k = 1 only"):
        cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True).knnMatch(q8, t8, k=2)
    with pytest.raises(ValueError, match="share type and length"):
        cv.BFMatcher(cv.NORM_HAMMING).match(q8, tf)
    with pytest.raises(ValueError, match="no train descriptors"):
        cv.BFMatcher(cv.NORM_HAMMING).match(q8)
    with pytest.raises(NotImplementedError, match="crossCheck with radiusMatch"):
        cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True).radiusMatch(q8, t8, 3)
    m = cv.BFMatcher_create(cv.NORM_HAMMING)
    assert m.empty()
    m.add([t8, t8]); m.add(t8)
    assert not m.empty() and len(m.getTrainDescriptors()) == 3
    m.clear()
    assert m.empty()


def test_dmatch_layout(tmp_path):
    """mi355cv_DMatch as a C compiler lays it out from include/mi355cv.h against DMATCH_DTYPE of the Python mirror (and the restatement's): cv::DMatch, 16 bytes"""
    from opencv_amd import features2d as f2d
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355cv.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mi355cv_DMatch), offsetof(mi355cv_DMatch, queryIdx), offsetof(mi355cv_DMatch, trainIdx),\n'
                   '  offsetof(mi355cv_DMatch, imgIdx), offsetof(mi355cv_DMatch, distance)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = f2d.DMATCH_DTYPE
    assert got == [D.itemsize] + [D.fields[n][1] for n in ("queryIdx", "trainIdx", "imgIdx", "distance")] == [16, 0, 4, 8, 12]
    assert D == R.DMATCH and D.fields["distance"][0] == np.float32
    assert (f2d.NORM_L1, f2d.NORM_L2, f2d.NORM_L2SQR, f2d.NORM_HAMMING, f2d.NORM_HAMMING2) == (2, 4, 5, 6, 7)
