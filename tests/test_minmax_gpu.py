"""minMaxLoc on the MI355X (opencv_amd.minMaxLoc / minMaxLocBatch -> mi355cv_minMaxLoc*, opencv_amd/csrc/minmax.hip) against the restatement
(tests/minmax_restate.py), bit for bit -- there is no tolerance anywhere in this file (a returned zero is compared with ==, its sign is unspecified).  Every call
asserts that its call counter moved and that mi355cv_lastKernel names the minmax kernels.

The kernel's unit of work is a 16-byte chunk; a workgroup takes 256 of them per grid pass and a frame gets ceil(chunks / 1024) workgroups.  300 x 200 is therefore
4 workgroups of about 4 passes on CV_8U and 30 workgroups on CV_64F, 1030 x 517 is 34 workgroups on CV_8U; 45 x 67 is one workgroup of two passes."""
import numpy as np
import pytest
import torch

import minmax_restate as R

pytestmark = pytest.mark.gpu


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


def one(cv, t, mask=None):
    """one call on a device tensor (possibly a view); counter and kernel name asserted"""
    n0 = cv.call_count("minMaxLoc")
    got = cv.minMaxLoc(t, mask)
    assert cv.call_count("minMaxLoc") == n0 + 1 and last_kernel(cv).startswith("k_minmax_partial<"), last_kernel(cv)
    assert ("nomask" in last_kernel(cv)) == (mask is None)
    return got


def batch(cv, t, mask=None, device=False):
    n0 = cv.call_count("minMaxLocBatch")
    vals, locs = cv.minMaxLocBatch(t, mask, device=device)
    assert cv.call_count("minMaxLocBatch") == n0 + 1 and last_kernel(cv).startswith("k_minmax_partial<"), last_kernel(cv)
    assert vals.dtype == torch.float64 and locs.dtype == torch.int32 and vals.is_cuda == device and locs.is_cuda == device
    assert tuple(vals.shape) == (t.shape[0], 2) and tuple(locs.shape) == (t.shape[0], 4)
    return vals, locs


def rows(vals, locs):
    v, l = vals.cpu().numpy(), locs.cpu().numpy()
    return [(float(v[i, 0]), float(v[i, 1]), (int(l[i, 0]), int(l[i, 1])), (int(l[i, 2]), int(l[i, 3]))) for i in range(len(v))]


def check(cv, a, m=None):
    want = R.minmax_vec(a, m)
    got = one(cv, dev(a), dev(m) if m is not None else None)
    assert R.same(got, want), (a.dtype, a.shape, got, want)
    return want


# ---- geometry
@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (67, 45), (200, 300), (517, 1030)])
def test_geometry(cv, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for dt in (np.uint8, np.float32) if shape[0] * shape[1] > 100000 else R.DTYPES:
        a = R.random_frame(rng, shape[0], shape[1], dt, levels=5, special=False)
        check(cv, a)
        check(cv, a, (rng.random(shape) < 0.5).astype(np.uint8))


@pytest.mark.parametrize("dt", R.DTYPES)
def test_roi_at_an_odd_origin_and_padding_more_extreme_than_any_pixel(cv, dt):
    """a view that starts at an odd column and row of a larger parent whose every other byte holds the type's extremes, in both directions: any read outside the
    rows of the view changes the answer"""
    rng = np.random.default_rng(3)
    dtn = np.dtype(dt)
    lo, hi = (-np.inf, np.inf) if dtn.kind == "f" else (np.iinfo(dtn).min, np.iinfo(dtn).max)
    for (h, w, y0, x0, ph, pw) in ((67, 45, 3, 5, 75, 61), (20, 130, 1, 1, 23, 135), (9, 16, 1, 3, 12, 21)):
        parent = np.where(rng.random((ph, pw)) < 0.5, lo, hi).astype(dt)
        inner = R.random_frame(rng, h, w, dt, levels=4, special=False)
        if dtn.kind != "f":
            inner = np.clip(inner, lo + 1, hi - 1).astype(dt) if lo < 0 else np.clip(inner, 1, hi - 1).astype(dt)
        parent[y0:y0 + h, x0:x0 + w] = inner
        want = R.minmax_vec(inner)
        assert want[0] > lo and want[1] < hi
        view = dev(parent)[y0:y0 + h, x0:x0 + w]
        assert not view.is_contiguous() and (dtn.itemsize > 1 or view.data_ptr() % 16 != 0)
        assert R.same(one(cv, view), want)
        pm = np.full((ph + 2, pw + 7), 255, np.uint8)                         # a mask with its own pitch, taken from a ROI of an all-selecting parent
        m = (rng.random((h, w)) < 0.5).astype(np.uint8)
        pm[2:2 + h, 7:7 + w] = m
        assert R.same(one(cv, view, dev(pm)[2:2 + h, 7:7 + w]), R.minmax_vec(inner, m))


# ---- ties across the machine
def test_constant_frames(cv):
    for dt in R.DTYPES:
        for shape in ((67, 45), (200, 300)):
            assert check(cv, np.full(shape, 3, dt))[2:] == ((0, 0), (0, 0))


@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float32, np.float64])
def test_the_earlier_of_two_equal_extremes_wins_for_min_and_for_max(cv, dt):
    h, w = 200, 300
    rng = np.random.default_rng(8)
    base = (rng.integers(0, 4, (h, w)) + 10).astype(dt)
    n = h * w
    pairs = [(5, 40), (5, 70), (5, 3 * w + 129), (7, 13 * w + 7), (7, 150 * w + 299), (0, n - 1), (n - 2, n - 1), (w - 1, w), (31, 32)]
    for first, second in pairs:                # same wave, neighbouring waves, different workgroups, first / last pixel, across a row end, across a chunk end
        for val, slot in ((100, 3), (1, 2)):   # a maximum above every pixel, a minimum below
            a = base.copy()
            a.ravel()[[first, second]] = val
            want = check(cv, a)
            assert want[slot] == (first % w, first // w)
    a = base.copy()                            # the extremes at the last pixel only
    a[-1, -1] = 100
    assert check(cv, a)[3] == (w - 1, h - 1)
    a[-1, -1] = 1
    assert check(cv, a)[2] == (w - 1, h - 1)


# ---- depths
@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("shape", [(67, 45), (200, 300)])
def test_depths(cv, dt, shape):
    rng = np.random.default_rng(21)
    h, w = shape
    check(cv, R.random_frame(rng, h, w, dt, levels=4))                       # few levels and the type's extremes (floats: +-inf, denormals, +-0)
    check(cv, R.random_frame(rng, h, w, dt))                                 # the full range
    check(cv, R.random_frame(rng, h, w, dt, special=False))
    if np.dtype(dt).kind == "f":
        a = R.random_frame(rng, h, w, dt, nan=0.1)
        a[0, 0] = np.nan
        check(cv, a)
        a = R.random_frame(rng, h, w, dt, levels=5, nan=0.9)                 # NaN the majority
        a[0, 0] = np.nan
        check(cv, a)
        assert check(cv, np.full(shape, np.nan, dt)) == R.EMPTY
        z = np.zeros(shape, dt)
        z[h // 2, w // 3] = -0.0
        z[0, 1] = -0.0
        assert check(cv, z)[2:] == ((0, 0), (0, 0))
        z = -z
        assert check(cv, z)[2:] == ((0, 0), (0, 0))
        fi = np.finfo(dt)
        d = np.zeros(shape, dt)                                              # denormals around zero decide both ends
        d[h - 1, w - 1] = fi.smallest_subnormal
        d[h - 2, 0] = -fi.smallest_subnormal
        assert check(cv, d)[2:] == ((0, h - 2), (w - 1, h - 1))
    if np.dtype(dt) == np.float64:
        a = np.full(shape, 1.0)                                              # values that differ only below float precision
        a[h // 2, 7] = 1.0 + 2.0 ** -40
        a[h // 3, 9] = 1.0 - 2.0 ** -41
        a[h - 1, 1] = 1.0 + 2.0 ** -40
        want = check(cv, a)
        assert want[2] == (9, h // 3) and want[3] == (7, h // 2) and np.float32(want[0]) == np.float32(want[1])
    if np.dtype(dt) == np.int32:
        for v in (np.iinfo(np.int32).max, np.iinfo(np.int32).min):           # the key of these is the identity's in one direction: still candidates
            assert check(cv, np.full(shape, v, dt)) == (float(v), float(v), (0, 0), (0, 0))


# ---- mask
@pytest.mark.parametrize("dt", [np.uint8, np.int32, np.float32, np.float64])
def test_masks(cv, dt):
    rng = np.random.default_rng(33)
    for (h, w) in ((67, 45), (200, 300)):
        a = R.random_frame(rng, h, w, dt, levels=5)
        assert check(cv, a, np.zeros((h, w), np.uint8)) == R.EMPTY
        m = np.zeros((h, w), np.uint8)
        m[h - 3, w - 2] = 7
        assert check(cv, a, m)[2:] == ((w - 2, h - 3), (w - 2, h - 3))
        full = R.minmax_vec(a)
        m = np.ones((h, w), np.uint8)                                        # a mask that excludes the true extremes
        m[a.astype(np.float64) == full[0]] = 0
        m[a.astype(np.float64) == full[1]] = 0
        want = check(cv, a, m)
        assert want[0] > full[0] and want[1] < full[1]
        check(cv, a, (rng.random((h, w)) < 0.02).astype(np.uint8) * 255)
        if np.dtype(dt).kind == "f":
            b = a.copy()
            m = (rng.random((h, w)) < 0.3).astype(np.uint8)
            b[m != 0] = np.nan                                               # every selected pixel is NaN
            assert check(cv, b, m) == R.EMPTY


# ---- batch
@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float32, np.float64])
@pytest.mark.parametrize("nb", [3, 5])
def test_batch(cv, dt, nb):
    rng = np.random.default_rng(nb)
    h, w = 67, 45
    ph, pw = h + 5, w + 11
    dtn = np.dtype(dt)
    lo, hi = (-np.inf, np.inf) if dtn.kind == "f" else (np.iinfo(dtn).min, np.iinfo(dtn).max)
    parent = np.where(rng.random((nb, ph, pw)) < 0.5, lo, hi).astype(dt)      # pitch and inter-frame padding more extreme than any pixel
    frames = np.stack([(rng.integers(0, 5, (h, w)) + 10 * (f + 1)).astype(dt) for f in range(nb)])
    for f in range(nb):                                                      # different extremes per frame
        frames[f].ravel()[rng.choice(h * w, 2, replace=False)] = [10 * (f + 1) - 1 - f, 10 * (f + 1) + 5 + f]
    if dtn.kind == "f":
        frames[1] = np.nan                                                   # one all-NaN frame
    parent[:, 3:3 + h, 5:5 + w] = frames
    t = dev(parent)[:, 3:3 + h, 5:5 + w]                                      # a strided view, served without a copy
    assert not t.is_contiguous()
    want = [R.minmax_vec(frames[f]) for f in range(nb)]
    got = rows(*batch(cv, t))
    assert all(R.same(g, w_) for g, w_ in zip(got, want)), (got, want)
    assert got == [one(cv, t[f]) for f in range(nb)]                          # the batch equals the per-frame calls
    if dtn.kind == "f":
        assert got[1] == R.EMPTY
    dv, dl = batch(cv, t, device=True)                                       # device results equal the host-result call
    assert rows(dv, dl) == got
    assert rows(*batch(cv, t)) == got                                        # two runs are identical
    # a shared mask, and per-frame masks of which one selects nothing
    shared = (rng.random((h, w)) < 0.5).astype(np.uint8)
    want = [R.minmax_vec(frames[f], shared) for f in range(nb)]
    got = rows(*batch(cv, t, dev(shared)))
    assert all(R.same(g, w_) for g, w_ in zip(got, want)), (got, want)
    per = (rng.random((nb, h, w)) < 0.5).astype(np.uint8) * 9
    per[nb - 1] = 0
    pm = np.full((nb, h + 2, w + 3), 255, np.uint8)
    pm[:, 1:1 + h, 2:2 + w] = per
    want = [R.minmax_vec(frames[f], per[f]) for f in range(nb)]
    assert want[nb - 1] == R.EMPTY and want[0] != R.EMPTY
    got = rows(*batch(cv, t, dev(pm)[:, 1:1 + h, 2:2 + w], device=True))
    assert all(R.same(g, w_) for g, w_ in zip(got, want)), (got, want)
    assert got == [one(cv, t[f], dev(per[f])) for f in range(nb)]


def test_batch_of_larger_frames_with_several_workgroups_each(cv):
    rng = np.random.default_rng(77)
    frames = np.stack([R.random_frame(rng, 200, 300, np.float32, levels=5, nan=0.05) for _ in range(3)])
    got = rows(*batch(cv, dev(frames), device=True))
    assert all(R.same(g, R.minmax_vec(f)) for g, f in zip(got, frames))


# ---- pipeline
def test_match_template_then_min_max_without_leaving_the_device(cv):
    rng = np.random.default_rng(5)
    templ = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    places = [(7, 11), (60, 3), (33, 64)]                                    # (x, y)
    frames = rng.integers(100, 140, (3, 80, 96), dtype=np.uint8)
    for f, (x, y) in enumerate(places):
        frames[f, y:y + 16, x:x + 16] = templ
    d, t = dev(frames), dev(templ)
    for method in (cv.TM_SQDIFF, cv.TM_CCORR_NORMED, cv.TM_CCOEFF, cv.TM_CCOEFF_NORMED):
        res = cv.matchTemplateBatch(d, t, method)
        assert res.is_cuda and tuple(res.shape) == (3, 65, 81)
        vals, locs = batch(cv, res, device=True)
        assert vals.is_cuda and locs.is_cuda
        got = rows(vals, locs)
        host = res.cpu().numpy()
        for f, place in enumerate(places):
            assert R.same(got[f], R.minmax_vec(host[f])), (method, f)
            assert (got[f][2] if method == cv.TM_SQDIFF else got[f][3]) == place, (method, f, got[f])
