"""HoughCircles on the MI355X (opencv_amd.HoughCircles* -> mi355cv_houghCircles*, opencv_amd/csrc/houghcircles.hip) against the restatement
(tests/houghcircles_restate.py): the whole accumulator through mi355cv_houghCirclesAccum under both vote kernels, the count and the circle list, all bit for bit --
there is no tolerance anywhere in this file.  Every call asserts that its call counter moved and that mi355cv_lastKernel names the expected vote kernel.  The
reference for a (frame, parameters) pair is computed once and shared.  The library refuses cvRound(param2) < 1, so the lowest threshold here is 1."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import houghcircles_restate as R

pytestmark = pytest.mark.gpu

F = np.float32
CV_16S, BORDER_REPLICATE = 3, 1
ARMS = {0: "k_hc_vote,", 1: "k_hc_vote_tile,"}               # the note starts with the vote kernel's name and a comma
OK, NOT_IMPLEMENTED = 0, 1
assert (R.TILE, R.LDS_BINS) == (64, 40960)      # the shapes below are chosen around these two


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    yield opencv_amd
    opencv_amd._lib.lib.mi355cv_houghCirclesSetKernel(-1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def last_kernel(cv):
    return cv._lib.lib.mi355cv_lastKernel().decode()


def set_arm(cv, arm):
    assert cv._lib.lib.mi355cv_houghCirclesSetKernel(arm) == 0


def auto_arm(p):
    return 0                                    # the tile kernel won at no reach: it runs behind the switch only


DISCS_150 = ((40, 50, 22), (100, 60, 30), (75, 140, 45), (120, 170, 12), (20, 180, 9))


@functools.lru_cache(maxsize=None)
def planes(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    make = {
        "1x1": lambda: R.uniform_planes(1, 1, -7, 2),
        "1x37": lambda: R.random_planes(rng, 37, 1, 0.6),                   # width 1, height 37
        "37x1": lambda: R.random_planes(rng, 1, 37, 0.6),
        "45x67": lambda: R.random_planes(rng, 67, 45, 0.1),                 # width 45: no multiple of 4
        "64x130": lambda: R.random_planes(rng, 130, 64, 0.1),
        "64x130 1%": lambda: R.random_planes(rng, 130, 64, 0.01),
        "64x130 50%": lambda: R.random_planes(rng, 130, 64, 0.5),
        "64x130 empty": lambda: R.empty_planes(130, 64),
        "16x16 all": lambda: R.uniform_planes(16, 16, -5, 5),
        "150x200 discs": lambda: R.simple_gradients(R.discs_on_noise(200, 150, DISCS_150, seed=5)),
    }[name]
    out = make()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dev_planes(name):
    return tuple(dev(a) for a in planes(name))


def prepared(name, dp, radii, md=1.0, acc_t=1):
    h, w = planes(name)[0].shape
    return R.prepare(w, h, dp, md, 100, acc_t, *radii)


@functools.lru_cache(maxsize=None)
def want_acc(name, dp, radii):
    acc, pts = R.accum_vec(*planes(name), prepared(name, dp, radii))
    acc.setflags(write=False)
    return acc, pts


@functools.lru_cache(maxsize=None)
def want_candidates(name, dp, radii, acc_t):
    acc, pts = want_acc(name, dp, radii)
    return tuple(R.candidates_vec(acc, pts, prepared(name, dp, radii), acc_t))


def want_circles(name, dp, radii, acc_t, md, cap=None):
    out = R.suppress_vec(list(want_candidates(name, dp, radii, acc_t)), prepared(name, dp, radii, md), cap)
    return out


def thresholds(name, dp, radii):
    top = int(want_acc(name, dp, radii)[0].max())
    return (1, max(1, top // 2), max(1, top))


def check_acc(cv, name, dp=1.0, radii=(0, 0), arms=(0, 1), src=None):
    """the accumulator of one frame under both vote kernels"""
    e, dx, dy = src if src is not None else dev_planes(name)
    wacc = want_acc(name, dp, radii)[0]
    for arm in arms:
        set_arm(cv, arm)
        n0 = cv.call_count("houghCirclesAccum")
        acc = cv.HoughCirclesAccumulator(e, dx, dy, dp, *radii)
        kernel = ARMS[arm if arm >= 0 else auto_arm(prepared(name, dp, radii))]
        assert cv.call_count("houghCirclesAccum") == n0 + 1 and last_kernel(cv).startswith(kernel), last_kernel(cv)
        assert isinstance(acc, torch.Tensor) == isinstance(e, torch.Tensor)
        acc = host(acc)
        assert acc.dtype == np.int32 and acc.shape == wacc.shape and np.array_equal(acc, wacc), (name, dp, radii, arm, int((acc != wacc).sum()))
    set_arm(cv, -1)
    return wacc


def check_circles(cv, name, dp=1.0, radii=(0, 0), mds=(1.0, 7.5), acc_ts=None, cns=(4,), arm=-1, src=None, radius_kernel=None):
    e, dx, dy = src if src is not None else dev_planes(name)
    p = prepared(name, dp, radii)
    set_arm(cv, arm)
    kernel = ARMS[arm if arm >= 0 else auto_arm(p)]
    for acc_t in (acc_ts if acc_ts is not None else thresholds(name, dp, radii)):
        for md in mds:
            want = want_circles(name, dp, radii, acc_t, md)
            for cn in cns:
                n0 = cv.call_count("houghCirclesGradient")
                got = cv.HoughCirclesGradient(e, dx, dy, dp, md, acc_t, *radii, withVotes=cn == 4)
                assert cv.call_count("houghCirclesGradient") > n0 and last_kernel(cv).startswith(kernel), last_kernel(cv)
                if radius_kernel is not None:
                    assert "k_hc_radius<%s>" % radius_kernel in last_kernel(cv), last_kernel(cv)
                assert isinstance(got, torch.Tensor) == isinstance(e, torch.Tensor) and (not isinstance(e, torch.Tensor) or got.is_cuda == e.is_cuda)
                got = host(got)
                assert got.dtype == F and got.shape == (len(want), cn) and R.same_bits(got, want[:, :cn]), (name, dp, radii, acc_t, md, cn, got[:4], want[:4])
    set_arm(cv, -1)


@pytest.mark.parametrize("name", ["1x1", "1x37", "37x1", "45x67", "64x130", "64x130 1%", "64x130 50%"])
def test_shapes_and_densities(cv, name):
    check_acc(cv, name)
    check_circles(cv, name, cns=(3, 4))


def test_empty_frame_gives_no_circle(cv):
    assert not check_acc(cv, "64x130 empty").any()
    check_circles(cv, "64x130 empty", acc_ts=(1,))
    assert cv.HoughCirclesGradient(*dev_planes("64x130 empty"), 1, 5, 1).shape == (0, 3)


def test_all_edges_with_one_gradient_16x16(cv):
    """the most contention on a cell, plateaus of equal votes on both sides of the predicate, long runs of tied votes through both sorts"""
    for dp in (1.0, 2.0):
        wacc = check_acc(cv, "16x16 all", dp=dp)
        inner = wacc[:-2, :-2]
        assert (inner[:, :-1] == inner[:, 1:])[inner[:, 1:] > 0].any() and (inner[:-1] == inner[1:])[inner[1:] > 0].any()
        check_circles(cv, "16x16 all", dp=dp, mds=(1.0, 3.0), cns=(3, 4))
    cands = want_candidates("16x16 all", 1.0, (0, 0), 1)
    votes = [c[3] for c in cands]
    assert len(votes) > len(set(votes))                                     # tied circles: the cell index decides


def test_discs_across_tiles(cv):
    """an accumulator of 3 x 4 tiles, rays that cross the seams, and a maxRadius larger than a tile; both kernels, forced and chosen"""
    name = "150x200 discs"
    for radii in ((5, 40), (0, 0), (10, 100)):
        check_acc(cv, name, radii=radii, arms=(0, 1, -1))
    check_acc(cv, name, dp=2.0, radii=(5, 40), arms=(0, 1, -1))
    for arm in (0, 1):
        check_circles(cv, name, radii=(5, 60), mds=(20.0,), acc_ts=(12,), arm=arm, cns=(3, 4), radius_kernel="lds")
    found = want_circles(name, 1.0, (5, 60), 12, 20.0)
    assert len(found) >= 4                                                  # the drawn discs, for what the crude edge map is worth


@pytest.mark.parametrize("dp", R.DPS)
@pytest.mark.parametrize("radii", R.RADII)
def test_parameter_grid_45x67(cv, dp, radii):
    check_acc(cv, "45x67", dp=dp, radii=radii)
    check_circles(cv, "45x67", dp=dp, radii=radii, mds=(1.0, 7.5, 1000.0), radius_kernel="none" if radii[1] < 0 else "lds")


def test_radius_bins_on_both_sides_of_the_lds_budget(cv):
    top = cv._lib.limit("houghcircles_lds_bins")
    for max_radius, kernel in ((top // 10, "lds"), (top // 10 + 1, "hbm"), (top // 10 + 62, "hbm")):
        p = prepared("45x67", 1.0, (0, max_radius))
        assert (p.n_bins <= top) == (kernel == "lds") and abs(p.n_bins - top) <= 620
        check_acc(cv, "45x67", radii=(0, max_radius))
        check_circles(cv, "45x67", radii=(0, max_radius), acc_ts=(1, 3), mds=(1.0,), radius_kernel=kernel)


# ---- the C ABI directly: capacities, rows behind the count
def raw_gradient(cv, src, out, cn, cap, dp, md, acc_t, radii, n):
    e, dx, dy = src
    L = cv._lib.lib
    return L.mi355cv_houghCirclesGradient(e.data_ptr(), e.stride(0), dx.data_ptr(), dy.data_ptr(), dx.stride(0) * 2, e.shape[1], e.shape[0], out.data_ptr(), cn, cap,
                                          R.HOUGH_GRADIENT, dp, md, 100.0, float(acc_t), radii[0], radii[1], n)


def test_max_circles_below_the_count(cv, monkeypatch):
    name, dp, radii, acc_t, md = "64x130", 1.0, (0, 0), 1, 3.0
    want = want_circles(name, dp, radii, acc_t, md)
    assert len(want) > 12
    for cap in (1, 5, len(want) - 1, len(want), len(want) + 3):
        for cn in (3, 4):
            out = torch.full((cap + 2, cn), -7.0, device="cuda")
            n = ctypes.c_int(-1)
            n0 = cv.call_count("houghCirclesGradient")
            assert raw_gradient(cv, dev_planes(name), out, cn, cap, dp, md, acc_t, radii, ctypes.byref(n)) == OK and cv.call_count("houghCirclesGradient") == n0 + 1
            k = min(cap, len(want))
            assert n.value == k and R.same_bits(out[:k].cpu().numpy(), want_circles(name, dp, radii, acc_t, md, cap)[:, :cn]) and R.same_bits(out[:k].cpu().numpy(), want[:k, :cn])
            assert bool((out[k:] == -7.0).all())                            # rows past the count are never written
        got = cv.HoughCirclesGradient(*dev_planes(name), dp, md, acc_t, *radii, maxCircles=cap, withVotes=True)
        assert R.same_bits(host(got), want[:cap])
    # without maxCircles the Python call doubles its capacity until the count stays below it
    monkeypatch.setattr(cv.imgproc, "_HOUGH_MAX_CIRCLES", 2)
    n0 = cv.call_count("houghCirclesGradient")
    got = cv.HoughCirclesGradient(*dev_planes(name), dp, md, acc_t, *radii, withVotes=True)
    calls, cap = 1, 2
    while cap <= len(want):
        calls, cap = calls + 1, cap * 2
    assert R.same_bits(host(got), want) and cv.call_count("houghCirclesGradient") == n0 + calls and calls >= 4


# ---- the full call: the edge stage inside
@functools.lru_cache(maxsize=None)
def image(name):
    img = {"96x128": lambda: R.discs_on_noise(128, 96, ((30, 40, 18), (65, 90, 24), (70, 30, 10)), seed=2),
           "96x128 b": lambda: R.discs_on_noise(128, 96, ((50, 64, 35), (20, 110, 9)), seed=3, noise=40),
           "96x128 flat": lambda: np.full((128, 96), 90, np.uint8)}[name]()
    img.setflags(write=False)
    return img


FULL = dict(dp=1.0, md=15.0, p1=120, p2=10, radii=(5, 50))


@functools.lru_cache(maxsize=None)
def stage_planes(name, p1):
    """the project's own Canny and Sobel, pinned against the oracle elsewhere (tests/test_canny_gpu.py, the filter tests)"""
    import opencv_amd as cv
    d = dev(image(name))
    low, high = R.canny_thresholds(p1)
    return cv.Canny(d, low, high, 3, False), cv.Sobel(d, CV_16S, 1, 0, 3, borderType=BORDER_REPLICATE), cv.Sobel(d, CV_16S, 0, 1, 3, borderType=BORDER_REPLICATE)


@functools.lru_cache(maxsize=None)
def want_full(name, dp, md, p1, p2, radii, cap=None):
    e, dx, dy = (host(a) for a in stage_planes(name, p1))
    out = R.hough_circles(e, dx, dy, dp, md, p1, p2, *radii, max_circles=cap)[1]
    out.setflags(write=False)
    return out


def test_full_call_equals_its_stages(cv):
    for name in ("96x128", "96x128 b", "96x128 flat"):
        for kw in (FULL, dict(FULL, dp=2.0), dict(FULL, radii=(0, 0)), dict(FULL, radii=(4, -1), p2=6), dict(FULL, p1=301, p2=8)):
            want = want_full(name, kw["dp"], kw["md"], kw["p1"], kw["p2"], kw["radii"])
            for cn in (3, 4):
                n0 = cv.call_count("houghCircles")
                got = cv.HoughCircles(dev(image(name)), cv.HOUGH_GRADIENT, kw["dp"], kw["md"], kw["p1"], kw["p2"], *kw["radii"], withVotes=cn == 4)
                assert cv.call_count("houghCircles") == n0 + 1 and last_kernel(cv).startswith("k_hc_vote"), last_kernel(cv)
                assert got.is_cuda and R.same_bits(host(got), want[:, :cn]), (name, kw, cn)
            # the internal edge stage is the stage entries' one: the transform from Canny / Sobel planes gives the same list
            e, dx, dy = stage_planes(name, kw["p1"])
            via = cv.HoughCirclesGradient(e, dx, dy, kw["dp"], kw["md"], kw["p2"], *kw["radii"], withVotes=True)
            assert via.is_cuda and R.same_bits(host(via), want), (name, kw)
    assert len(want_full("96x128", 1.0, 15.0, 120, 10, (5, 50))) >= 3 and len(want_full("96x128 flat", 1.0, 15.0, 120, 10, (5, 50))) == 0


def test_canny_to_circles_stays_in_hbm(cv):
    d = dev(image("96x128"))
    edges = cv.Canny(d, 60, 120)
    dx, dy = cv.Sobel(d, CV_16S, 1, 0, 3, borderType=BORDER_REPLICATE), cv.Sobel(d, CV_16S, 0, 1, 3, borderType=BORDER_REPLICATE)
    out = cv.HoughCirclesGradient(edges, dx, dy, 1.0, 15.0, 10, 5, 50, withVotes=True)
    acc = cv.HoughCirclesAccumulator(edges, dx, dy, 1.0, 5, 50)
    assert edges.is_cuda and out.is_cuda and acc.is_cuda and R.same_bits(host(out), want_full("96x128", 1.0, 15.0, 120, 10, (5, 50)))


def test_batch_equals_single_calls(cv):
    names = ("96x128", "96x128 flat", "96x128 b", "96x128")
    frames = torch.stack([dev(image(n)) for n in names])
    cap, kw = 4, FULL
    wants = [want_full(n, kw["dp"], kw["md"], kw["p1"], kw["p2"], kw["radii"]) for n in names]
    assert len(wants[1]) == 0 and any(len(w) > cap for w in wants) and any(0 < len(w) < cap for w in wants)
    L = cv._lib.lib
    for cn in (3, 4):
        out = torch.full((len(names), cap + 1, cn), -7.0, device="cuda")
        counts = (ctypes.c_int * len(names))(*([-1] * len(names)))
        n0 = cv.call_count("houghCirclesBatch")
        rc = L.mi355cv_houghCirclesBatch(frames.data_ptr(), frames.stride(1), frames.stride(0), 96, 128, out.data_ptr(), cn, cap, out.stride(0) * 4, len(names), R.HOUGH_GRADIENT,
                                         kw["dp"], kw["md"], float(kw["p1"]), float(kw["p2"]), kw["radii"][0], kw["radii"][1], counts)
        assert rc == OK and cv.call_count("houghCirclesBatch") == n0 + 1 and last_kernel(cv).startswith("k_hc_vote") and "%d frame(s)" % len(names) in last_kernel(cv)
        o = out.cpu().numpy()
        for f, w in enumerate(wants):
            k = min(cap, len(w))
            assert counts[f] == k and R.same_bits(o[f, :k], w[:k, :cn]), (f, cn)
            assert np.all(o[f, k:] == -7.0)                                 # rows past the counts, the empty frame's all
    counts, circles = cv.HoughCirclesBatch(frames, cv.HOUGH_GRADIENT, kw["dp"], kw["md"], kw["p1"], kw["p2"], *kw["radii"], maxCircles=64, withVotes=True)
    assert circles.is_cuda and circles.shape == (len(names), 64, 4)
    for f, w in enumerate(wants):
        single = cv.HoughCircles(frames[f], cv.HOUGH_GRADIENT, kw["dp"], kw["md"], kw["p1"], kw["p2"], *kw["radii"], withVotes=True)
        assert counts[f] == len(w) == len(single) and R.same_bits(host(circles[f, :counts[f]]), w) and R.same_bits(host(single), w)


def test_host_resident_frame_and_batch(cv):
    kw = FULL
    names = ("96x128", "96x128 flat", "96x128 b")
    for n in names:
        got = cv.HoughCircles(np.array(image(n)), cv.HOUGH_GRADIENT, kw["dp"], kw["md"], kw["p1"], kw["p2"], *kw["radii"], withVotes=True)
        assert isinstance(got, np.ndarray) and R.same_bits(got, want_full(n, kw["dp"], kw["md"], kw["p1"], kw["p2"], kw["radii"]))
    frames = torch.from_numpy(np.stack([image(n) for n in names]))
    out_before = cv.call_count("houghCirclesBatch")
    counts, circles = cv.HoughCirclesBatch(frames, cv.HOUGH_GRADIENT, kw["dp"], kw["md"], kw["p1"], kw["p2"], *kw["radii"], maxCircles=3, withVotes=True)
    assert cv.call_count("houghCirclesBatch") == out_before + 1 and not circles.is_cuda
    for f, n in enumerate(names):
        w = want_full(n, kw["dp"], kw["md"], kw["p1"], kw["p2"], kw["radii"])
        assert counts[f] == min(3, len(w)) and R.same_bits(circles[f, :counts[f]].numpy(), w[:3])
    e, dx, dy = planes("45x67")
    got = cv.HoughCirclesGradient(np.array(e), np.array(dx), np.array(dy), 1.0, 3.0, 2, withVotes=True)
    assert isinstance(got, np.ndarray) and R.same_bits(got, want_circles("45x67", 1.0, (0, 0), 2, 3.0))
    acc = cv.HoughCirclesAccumulator(np.array(e), np.array(dx), np.array(dy), 1.0)
    assert isinstance(acc, np.ndarray) and np.array_equal(acc, want_acc("45x67", 1.0, (0, 0))[0])


def test_padded_pitch_and_odd_offsets(cv):
    """rows with non-zero bytes behind them, views that start at an odd byte (the edge map, the image) or an odd short (the gradients)"""
    e, dx, dy = planes("45x67")
    h, w = e.shape
    be = torch.full((h + 6, w + 20), 0xAB, dtype=torch.uint8, device="cuda")
    bx = torch.full((h + 6, w + 20), 0x1234, dtype=torch.int16, device="cuda")
    by = torch.full((h + 6, w + 20), -0x1234, dtype=torch.int16, device="cuda")
    be[2:2 + h, 5:5 + w], bx[2:2 + h, 7:7 + w], by[4:4 + h, 7:7 + w] = dev(e), dev(dx), dev(dy)
    src = (be[2:2 + h, 5:5 + w], bx[2:2 + h, 7:7 + w], by[4:4 + h, 7:7 + w])
    assert src[0].data_ptr() % 2 == 1 and src[1].data_ptr() % 4 == 2
    check_acc(cv, "45x67", src=src)
    check_circles(cv, "45x67", src=src, acc_ts=(1, 3), mds=(3.0,))
    img = image("96x128")
    big = torch.full((128 + 4, 96 + 31), 0xCD, dtype=torch.uint8, device="cuda")
    big[2:130, 3:99] = dev(img)
    kw = FULL
    got = cv.HoughCircles(big[2:130, 3:99], cv.HOUGH_GRADIENT, kw["dp"], kw["md"], kw["p1"], kw["p2"], *kw["radii"], withVotes=True)
    assert big[2:130, 3:99].data_ptr() % 2 == 1 and R.same_bits(host(got), want_full("96x128", kw["dp"], kw["md"], kw["p1"], kw["p2"], kw["radii"]))
    assert int((big == 0xCD).sum()) == big.numel() - 128 * 96


def test_overlap_on_the_device_is_declined_and_touches_nothing(cv):
    L = cv._lib.lib
    buf = torch.zeros(128 * 96 + 4096, dtype=torch.uint8, device="cuda")
    buf[:128 * 96] = dev(image("96x128")).reshape(-1)
    before = buf.clone()
    n = ctypes.c_int(-5)
    n0 = cv.call_count("houghCircles") + cv.call_count("houghCirclesGradient") + cv.call_count("houghCirclesAccum")
    for off in (0, 128 * 96 - 16):                                          # circles over the first rows, and straddling the last one
        rc = L.mi355cv_houghCircles(buf.data_ptr(), 96, 96, 128, buf.data_ptr() + off, 4, 8, R.HOUGH_GRADIENT, 1.0, 15.0, 120.0, 10.0, 5, 50, ctypes.byref(n))
        assert rc == NOT_IMPLEMENTED and "overlap" in L.mi355cv_lastError().decode()
    e, dx, dy = dev_planes("45x67")
    keep = dx.clone()
    rc = L.mi355cv_houghCirclesGradient(e.data_ptr(), 45, dx.data_ptr(), dy.data_ptr(), 90, 45, 67, dx.data_ptr() + 8, 3, 8, R.HOUGH_GRADIENT, 1.0, 3.0, 100.0, 2.0, 0, 0,
                                        ctypes.byref(n))
    assert rc == NOT_IMPLEMENTED and "overlap" in L.mi355cv_lastError().decode()
    ar, ac = ctypes.c_int(-5), ctypes.c_int(-5)
    rc = L.mi355cv_houghCirclesAccum(e.data_ptr(), 45, dx.data_ptr(), dy.data_ptr(), 90, 45, 67, 1.0, 0, 0, dy.data_ptr(), 47 * 4, ctypes.byref(ar), ctypes.byref(ac))
    assert rc == NOT_IMPLEMENTED and "overlap" in L.mi355cv_lastError().decode()
    assert n.value == -5 and (ar.value, ac.value) == (-5, -5) and torch.equal(buf, before) and torch.equal(dx, keep) and torch.equal(dy, dev(planes("45x67")[2]))
    assert cv.call_count("houghCircles") + cv.call_count("houghCirclesGradient") + cv.call_count("houghCirclesAccum") == n0
