"""HoughLines on the MI355X (opencv_amd.HoughLines* -> mi355cv_houghLines*, opencv_amd/csrc/hough.hip) against the restatement (tests/hough_restate.py): the whole
accumulator through mi355cv_houghLinesAccum, the count and the line list, all bit for bit -- there is no tolerance anywhere in this file.  Every call asserts
that its call counter moved and that mi355cv_lastKernel names the vote kernel.  The reference for a (frame, parameters) pair is computed once and shared."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import hough_restate as R

pytestmark = pytest.mark.gpu

PI = math.pi
F = np.float32
VOTE_CHUNK = R.VOTE_CHUNK                      # points a workgroup of k_hough_vote walks at a time: a frame with more points has several workgroups per angle row
assert VOTE_CHUNK == 4096
DEG = PI / 180
FULL = (0.0, PI)


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return opencv_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def last_kernel(cv):
    return cv._lib.lib.mi355cv_lastKernel().decode()


@functools.lru_cache(maxsize=None)
def frame(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    make = {
        "1x1": lambda: np.full((1, 1), 7, np.uint8),
        "1x37": lambda: R.random_frame(rng, 37, 1, 0.6),                    # width 1, height 37
        "37x1": lambda: R.random_frame(rng, 1, 37, 0.6),
        "45x67": lambda: R.random_frame(rng, 67, 45, 0.1),                  # width 45: no multiple of 4
        "64x130": lambda: R.random_frame(rng, 130, 64, 0.1),
        "64x130 1%": lambda: R.random_frame(rng, 130, 64, 0.01),
        "64x130 50%": lambda: R.random_frame(rng, 130, 64, 0.5),
        "64x130 lines": lambda: R.drawn_lines(130, 64),
        "64x130 empty": lambda: np.zeros((130, 64), np.uint8),
        "16x16 all": lambda: np.full((16, 16), 255, np.uint8),
        "256x256 50%": lambda: R.random_frame(rng, 256, 256, 0.5),
        "300x200 lines": lambda: R.drawn_lines(200, 300),
    }[name]
    a = make()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_acc(name, rho, theta, win):
    acc = R.accum_vec(frame(name), rho, theta, *win)
    acc.setflags(write=False)
    return acc


@functools.lru_cache(maxsize=None)
def want_lines(name, rho, theta, win, thr):
    out = R.lines_vec(want_acc(name, rho, theta, win), rho, theta, thr, win[0])
    out.setflags(write=False)
    return out


def thresholds(name, rho, theta, win):
    top = int(want_acc(name, rho, theta, win).max())
    return (0, top // 2, top)                  # every positive maximum; a mid threshold; above every vote but the largest -> no line


def check(cv, name, rho=1.0, theta=DEG, win=FULL, thrs=None, src=None, cns=(3,)):
    """accumulator, count and line list of one frame under one parameter set"""
    a = frame(name)
    d = src if src is not None else dev(a)
    n0 = cv.call_count("houghLinesAccum")
    acc = cv.HoughLinesAccumulator(d, rho, theta, *win)
    assert cv.call_count("houghLinesAccum") == n0 + 1 and last_kernel(cv).startswith("k_hough_vote<"), last_kernel(cv)
    acc = acc.cpu().numpy() if isinstance(acc, torch.Tensor) else acc
    wacc = want_acc(name, rho, theta, win)
    assert acc.dtype == np.int32 and acc.shape == wacc.shape and np.array_equal(acc, wacc), (name, rho, theta, win)
    for thr in (thrs if thrs is not None else thresholds(name, rho, theta, win)):
        want = want_lines(name, rho, theta, win, thr)
        for cn in cns:
            n0 = cv.call_count("houghLines")
            fn = cv.HoughLinesWithAccumulator if cn == 3 else cv.HoughLines
            got = fn(d, rho, theta, thr, min_theta=win[0], max_theta=win[1])
            assert cv.call_count("houghLines") > n0 and last_kernel(cv).startswith("k_hough_vote<"), last_kernel(cv)
            assert isinstance(got, torch.Tensor) == isinstance(d, torch.Tensor) and (not isinstance(d, torch.Tensor) or got.is_cuda == d.is_cuda)
            got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
            assert got.dtype == F and got.shape == (len(want), cn) and R.same_bits(got, want[:, :cn]), (name, rho, theta, win, thr, cn)
    return wacc


@pytest.mark.parametrize("name", ["1x1", "1x37", "37x1", "64x130", "64x130 1%", "64x130 50%", "64x130 lines", "300x200 lines"])
def test_shapes_and_frames(cv, name):
    check(cv, name, cns=(2, 3))


def test_empty_frame_gives_no_line(cv):
    wacc = check(cv, "64x130 empty", thrs=(0, -1))
    assert not wacc.any()
    assert cv.HoughLines(dev(frame("64x130 empty")), 1, DEG, 0).shape == (0, 2)


def test_all_nonzero_16x16(cv):
    """the most contention on a bin, and plateaus of equal votes on both sides of the predicate"""
    for theta in (DEG, PI / 90):
        wacc = check(cv, "16x16 all", theta=theta, cns=(2, 3))
        inner = wacc[1:-1, 1:-1]
        assert (inner[:, :-1] == inner[:, 1:])[inner[:, 1:] > 0].any() and (inner[:-1] == inner[1:])[inner[1:] > 0].any()
    v = want_lines("16x16 all", 1.0, DEG, FULL, 0)[:, 2]
    assert len(v) > 50 and (v[:-1] == v[1:]).sum() > 20                     # long runs of tied votes go through the sort


def test_padded_pitch_and_sub_view(cv):
    a = frame("45x67")
    h, w = a.shape
    assert w % 4 != 0
    parent = torch.full((h, 80), 255, dtype=torch.uint8, device="cuda")     # a padded pitch: the bytes behind a row are non-zero and must not vote
    parent[:, :w] = dev(a)
    check(cv, "45x67", src=parent[:, :w], cns=(2, 3))
    big = torch.full((h + 5, w + 30), 255, dtype=torch.uint8, device="cuda")
    big[2:2 + h, 7:7 + w] = dev(a)                                          # an odd byte offset: the rows are not dword-aligned
    check(cv, "45x67", src=big[2:2 + h, 7:7 + w])


def test_several_workgroups_merge_into_one_angle_row(cv):
    a = frame("256x256 50%")
    assert (a != 0).sum() > 4 * VOTE_CHUNK
    top = int(want_acc("256x256 50%", 1.0, DEG, FULL).max())
    check(cv, "256x256 50%", thrs=(top * 3 // 4,))
    assert "k_hough_vote<lds> grid=16x180x1" in last_kernel(cv), last_kernel(cv)


@pytest.mark.parametrize("rho", R.RHOS)
@pytest.mark.parametrize("theta", R.THETAS)
def test_parameter_grid(cv, rho, theta):
    for win in R.WINDOWS:
        check(cv, "45x67", rho, theta, win)
    check(cv, "64x130 lines", rho, theta, FULL, cns=(2,))


def test_geometry_edge_cases_on_the_device(cv):
    assert cv.HoughLinesAccumulator(dev(frame("45x67")), 2.0, DEG).shape == (182, 114)                  # 225 / 2 = 112.5 -> 112 bins (half to even), 180 angles
    assert cv.HoughLinesAccumulator(dev(frame("45x67")), 1.0, DEG, 0.0, PI / 2).shape == (93, 227)      # [0, pi / 2] keeps its last angle


def test_rows_too_long_for_lds_vote_in_hbm(cv):
    rho = 0.02
    assert R.geometry(64, 130, rho, PI / 7)[1] + 2 > R.LDS_BINS
    check(cv, "64x130 lines", rho, PI / 7, thrs=(2, 40))
    assert last_kernel(cv).startswith("k_hough_vote<hbm>"), last_kernel(cv)
    check(cv, "64x130", 0.024, PI / 7, thrs=(1,))                           # 16210 bins: the longest rows still voted in LDS are around here
    assert last_kernel(cv).startswith("k_hough_vote<lds>"), last_kernel(cv)


def c_hough(cv, src, lines, cn, cap, thr, rho=1.0, theta=DEG, srn=0.0, stn=0.0, win=FULL):
    n = ctypes.c_int(-3)
    cv.core.bind_stream(cv.core.Img(src))
    rc = cv._lib.lib.mi355cv_houghLines(ctypes.c_void_p(src.data_ptr()), src.stride(0), src.shape[1], src.shape[0], ctypes.c_void_p(lines.data_ptr()), cn, cap, rho, theta, thr,
                                        srn, stn, win[0], win[1], ctypes.byref(n))
    torch.cuda.synchronize()
    return rc, n.value


@pytest.mark.parametrize("cn", [2, 3])
def test_max_lines_below_the_count(cv, cn):
    name = "64x130 lines"
    want = want_lines(name, 1.0, DEG, FULL, 20)
    cap = 5
    assert len(want) > cap + 3
    lines = torch.full((cap + 3, cn), -7.0, dtype=torch.float32, device="cuda")
    n0 = cv.call_count("houghLines")
    rc, n = c_hough(cv, dev(frame(name)), lines, cn, cap, 20)
    assert rc == 0 and cv.call_count("houghLines") == n0 + 1
    got = lines.cpu().numpy()
    assert n == len(want) and R.same_bits(got[:cap], want[:cap, :cn]) and np.all(got[cap:] == -7.0)      # the top rows, the total, the rows behind intact
    # capacity above the count: rows past the count are never written
    want = want_lines(name, 1.0, DEG, FULL, 60)
    assert 0 < len(want) < 40
    lines = torch.full((40, cn), -7.0, dtype=torch.float32, device="cuda")
    rc, n = c_hough(cv, dev(frame(name)), lines, cn, 40, 60)
    got = lines.cpu().numpy()
    assert rc == 0 and n == len(want) and R.same_bits(got[:n], want[:, :cn]) and np.all(got[n:] == -7.0)
    # the Python call with maxLines keeps the strongest; without it a second call fetches what the first capacity could not hold
    got = (cv.HoughLinesWithAccumulator if cn == 3 else cv.HoughLines)(dev(frame(name)), 1, DEG, 20, maxLines=cap)
    assert R.same_bits(got.cpu().numpy(), want_lines(name, 1.0, DEG, FULL, 20)[:cap, :cn])


def test_second_call_when_the_first_capacity_is_too_small(cv, monkeypatch):
    monkeypatch.setattr(cv.imgproc, "_HOUGH_MAX_LINES", 4)
    want = want_lines("64x130 lines", 1.0, DEG, FULL, 20)
    n0 = cv.call_count("houghLines")
    got = cv.HoughLinesWithAccumulator(dev(frame("64x130 lines")), 1, DEG, 20)
    assert cv.call_count("houghLines") == n0 + 2 and R.same_bits(got.cpu().numpy(), want)


BATCH = ("64x130", "64x130 lines", "64x130 empty", "64x130 50%", "64x130 1%")


@pytest.mark.parametrize("cn", [2, 3])
def test_batch_equals_the_single_calls(cv, cn):
    frames = np.stack([frame(n) for n in BATCH])
    thr, cap = 12, 512
    n0 = cv.call_count("houghLinesBatch")
    counts, lines = cv.HoughLinesBatch(dev(frames), 1, DEG, thr, maxLines=cap, withAccumulator=cn == 3)
    assert cv.call_count("houghLinesBatch") == n0 + 1 and last_kernel(cv).startswith("k_hough_vote<lds>") and "5 frame(s)" in last_kernel(cv), last_kernel(cv)
    lines = lines.cpu().numpy()
    assert lines.shape == (len(BATCH), cap, cn) and counts[2] == 0 and any(c > cap for c in counts) and any(0 < c < cap for c in counts)
    for i, name in enumerate(BATCH):
        want = want_lines(name, 1.0, DEG, FULL, thr)
        single = (cv.HoughLinesWithAccumulator if cn == 3 else cv.HoughLines)(dev(frames[i]), 1, DEG, thr).cpu().numpy()
        k = min(len(want), cap)
        assert counts[i] == len(want) == len(single) and R.same_bits(single, want[:, :cn]) and R.same_bits(lines[i, :k], want[:k, :cn]), name


def test_batch_leaves_rows_past_the_counts_alone(cv):
    frames = dev(np.stack([frame(n) for n in BATCH]))
    cap, thr = 512, 12
    lines = torch.full((len(BATCH), cap + 2, 3), -7.0, dtype=torch.float32, device="cuda")
    counts = (ctypes.c_int * len(BATCH))()
    cv.core.bind_stream(cv.core.Img(frames[0]))
    rc = cv._lib.lib.mi355cv_houghLinesBatch(ctypes.c_void_p(frames.data_ptr()), frames.stride(1), frames.stride(0), 64, 130, ctypes.c_void_p(lines.data_ptr()), 3, cap,
                                             (cap + 2) * 12, len(BATCH), 1.0, DEG, thr, 0.0, 0.0, 0.0, PI, counts)
    torch.cuda.synchronize()
    assert rc == 0
    got = lines.cpu().numpy()
    for i, name in enumerate(BATCH):
        want = want_lines(name, 1.0, DEG, FULL, thr)
        k = min(len(want), cap)
        assert counts[i] == len(want) and R.same_bits(got[i, :k], want[:k]) and np.all(got[i, k:] == -7.0), name


def test_host_resident_frame_and_batch(cv):
    check(cv, "64x130 lines", src=np.array(frame("64x130 lines")), thrs=(20,), cns=(2, 3))
    # a short capacity on the host: only the written rows come back
    a = np.array(frame("64x130 lines"))
    lines = np.full((8, 3), -7.0, F)
    n = ctypes.c_int(0)
    rc = cv._lib.lib.mi355cv_houghLines(ctypes.c_void_p(a.ctypes.data), a.strides[0], 64, 130, ctypes.c_void_p(lines.ctypes.data), 3, 5, 1.0, DEG, 20, 0.0, 0.0, 0.0, PI,
                                        ctypes.byref(n))
    want = want_lines("64x130 lines", 1.0, DEG, FULL, 20)
    assert rc == 0 and n.value == len(want) and R.same_bits(lines[:5], want[:5]) and np.all(lines[5:] == -7.0)
    frames = torch.from_numpy(np.stack([frame(n) for n in BATCH])).pin_memory()
    n0 = cv.call_count("houghLinesBatch")
    counts, out = cv.HoughLinesBatch(frames, 1, DEG, 12, maxLines=64, withAccumulator=True)
    assert cv.call_count("houghLinesBatch") == n0 + 1 and not out.is_cuda
    for i, name in enumerate(BATCH):
        want = want_lines(name, 1.0, DEG, FULL, 12)
        k = min(len(want), 64)
        assert counts[i] == len(want) and R.same_bits(out[i, :k].numpy(), want[:k]), name


def test_canny_into_hough_on_the_device(cv):
    rng = np.random.default_rng(5)
    img = np.full((200, 300), 40, np.uint8)
    img[R.drawn_lines(200, 300) != 0] = 220
    img[60:140, 100:220] = 150
    img = (img.astype(np.int32) + rng.integers(-6, 7, img.shape)).clip(0, 255).astype(np.uint8)
    edges = cv.Canny(dev(img), 60, 160)
    lines = cv.HoughLinesWithAccumulator(edges, 1, DEG, 40)                 # the edge map never leaves HBM
    assert lines.is_cuda and last_kernel(cv).startswith("k_hough_vote<lds>")
    e = edges.cpu().numpy()
    assert 0 < (e != 0).sum() < e.size // 4
    acc, want = R.hough(e, 1.0, DEG, 40)
    assert len(want) > 3 and R.same_bits(lines.cpu().numpy(), want)
    assert np.array_equal(cv.HoughLinesAccumulator(edges, 1, DEG).cpu().numpy(), acc)


def test_declines_leave_the_destinations_alone(cv):
    a = dev(frame("16x16 all"))
    lines = torch.full((8, 3), -7.0, dtype=torch.float32, device="cuda")
    calls = cv.call_count("houghLines")
    L = cv._lib.lib
    for kw in (dict(srn=1.0), dict(stn=1.0), dict(rho=0.0), dict(theta=-1.0), dict(win=(0.0, 4.0)), dict(win=(1.0, 0.5)), dict(rho=1e-6)):
        rc, n = c_hough(cv, a, lines, 3, 8, 1, **kw)
        assert rc == 1 and n == -3, kw
    for cn, cap in ((1, 8), (4, 8), (3, 0)):
        assert c_hough(cv, a, lines, cn, cap, 1) == (1, -3)
    with pytest.raises(NotImplementedError, match="multi-scale"):
        cv.HoughLines(a, 1, DEG, 1, srn=2)
    top = cv.limit(R.MAX_DIM_KEY)
    with pytest.raises(NotImplementedError, match="HOUGH_MAX_DIM"):
        cv.HoughLines(torch.zeros((2, top + 1), dtype=torch.uint8, device="cuda"), 1, DEG, 1)
    with pytest.raises(NotImplementedError, match="HOUGH_MAX_ACCUM"):
        cv.HoughLines(a, 1e-6, DEG, 1)
    # lines that overlap the source in HBM
    buf = torch.full((1024,), 1, dtype=torch.uint8, device="cuda")
    before = buf.clone()
    rc, n = c_hough(cv, buf[:256].view(16, 16), buf.view(torch.float32)[:24].view(8, 3), 3, 8, 1)
    assert rc == 1 and n == -3 and "overlap" in L.mi355cv_lastError().decode()
    # an accumulator that overlaps it
    na, nr = ctypes.c_int(-3), ctypes.c_int(-3)
    big = torch.full((182 * 67 * 4,), 1, dtype=torch.uint8, device="cuda")
    keep = big.clone()
    rc = L.mi355cv_houghLinesAccum(ctypes.c_void_p(big.data_ptr() + 64), 16, 16, 16, 1.0, DEG, 0.0, PI, ctypes.c_void_p(big.data_ptr()), 67 * 4, ctypes.byref(na), ctypes.byref(nr))
    torch.cuda.synchronize()
    assert rc == 1 and (na.value, nr.value) == (-3, -3) and torch.equal(big, keep)
    assert torch.equal(buf, before) and bool((lines == -7.0).all()) and cv.call_count("houghLines") == calls
