"""distanceTransform on the MI355X (opencv_amd.distanceTransform / distanceTransformBatch -> mi355cv_distanceTransform / mi355cv_distanceTransformBatch,
opencv_amd/csrc/disttransform.hip) against the numpy restatement (tests/disttransform_restate.py), bit for bit in every case.  Every call asserts that its call
counter moved and that mi355cv_lastKernel names the row kernel of the metric and output type asked for.  The column pass cuts columns into segments of 64 rows;
the row pass runs a workgroup of 256 threads per row with the row in LDS."""
import numpy as np
import pytest
import torch

import disttransform_restate as R

pytestmark = pytest.mark.gpu

SEG, SPAN = 64, 256
L1, L2, C = R.DIST_L1, R.DIST_L2, R.DIST_C
KERNEL = {(L2, np.float32): "k_dist_row<L2,32F>", (L1, np.float32): "k_dist_row<L1,32F>", (C, np.float32): "k_dist_row<C,32F>", (L1, np.uint8): "k_dist_row<L1,8U>"}
COMBOS = [(L2, 0, np.float32), (L1, 3, np.float32), (C, 3, np.float32), (L1, 3, np.uint8)]


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


def cvtype(cv, dt):
    return cv.CV_8U if dt == np.uint8 else cv.CV_32F


def run(cv, src, metric, mask, dt=np.float32, **kw):
    n0 = cv.call_count("distanceTransform")
    got = cv.distanceTransform(src, metric, mask, dstType=cvtype(cv, dt), **kw)
    assert cv.call_count("distanceTransform") == n0 + 1, "the GPU path did not run"
    assert last_kernel(cv).startswith(KERNEL[(metric, dt)]), last_kernel(cv)
    return got


def check_all(cv, a):
    """all four served outputs of one mask against the restatement"""
    d = dev(a)
    for metric, mask, dt in COMBOS:
        got = run(cv, d, metric, mask, dt).cpu().numpy()
        want = R.distanceTransform(a, metric, dt)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want), (a.shape, metric, dt)


def random_mask(rng, h, w, density):
    return np.where(rng.random((h, w)) < density, 0, rng.integers(1, 256, (h, w))).astype(np.uint8)


def test_one_pixel(cv):
    check_all(cv, np.zeros((1, 1), np.uint8))
    check_all(cv, np.full((1, 1), 5, np.uint8))                                           # no site: 31622776.0f / 255
    assert run(cv, dev(np.full((1, 1), 5, np.uint8)), L2, 0).item() == 31622776.0


@pytest.mark.parametrize("n", [2, 63, 64, 65, 257])
def test_single_rows_and_columns(cv, n):
    rng = np.random.default_rng(n)
    for shape in ((1, n), (n, 1)):
        a = random_mask(rng, shape[0], shape[1], 0.1)
        a[0, 0] = 0
        check_all(cv, a)
        a = np.full(shape, 1, np.uint8)
        a[-1, -1] = 0
        check_all(cv, a)


@pytest.mark.parametrize("h", [SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1])
def test_heights_around_the_column_segments(cv, h):
    rng = np.random.default_rng(h)
    a = random_mask(rng, h, 9, 0.02)                                                      # sparse: the carries cross segments
    a[rng.integers(h), 4] = 0
    check_all(cv, a)
    a = np.full((h, 70), 1, np.uint8)
    a[0, 3] = 0; a[h - 1, 66] = 0; a[min(h - 1, SEG), 30] = 0                              # sites at the first row, the last row and the first row of segment 1
    check_all(cv, a)
    a = np.full((h, 5), 1, np.uint8)
    a[h - 1, :] = 0                                                                       # every distance carried up from the last segment
    check_all(cv, a)


@pytest.mark.parametrize("w", [SPAN - 1, SPAN, SPAN + 1, 2 * SPAN - 1, 2 * SPAN, 2 * SPAN + 1])
def test_widths_around_the_workgroup_span(cv, w):
    rng = np.random.default_rng(w)
    check_all(cv, random_mask(rng, 5, w, 0.02))
    a = np.full((3, w), 1, np.uint8)
    a[1, w - 1] = 0
    check_all(cv, a)


def test_largest_width_and_height(cv):
    top = cv.limit(R.LIMIT_KEY)
    assert top == R.MAX_DIM
    rng = np.random.default_rng(7)
    a = np.full((2, top), 1, np.uint8)
    a[rng.integers(0, 2, 24), rng.integers(0, top, 24)] = 0
    a[0, 0] = 0; a[1, top - 1] = 0
    check_all(cv, a)
    check_all(cv, np.ascontiguousarray(a.T))                                              # the largest height: 256 column segments
    b = np.full((1, top), 1, np.uint8)
    b[0, 0] = 0                                                                           # the longest scan and the largest squared distance of a row
    check_all(cv, b)
    for shape in ((2, top + 1), (top + 1, 2)):                                            # one past the bound is refused
        n0 = cv._lib.decline_count("distanceTransform")
        with pytest.raises(NotImplementedError):
            cv.distanceTransform(dev(np.zeros(shape, np.uint8)), L2, 0)
        assert cv._lib.decline_count("distanceTransform") == n0 + 1


PATTERN_SHAPES = [(37, 130), (64, 257)]


def patterns(h, w):
    rng = np.random.default_rng(h * w)
    out = {}
    for dens in (0.5, 0.03, 0.001):
        a = random_mask(rng, h, w, dens)
        a[rng.integers(h), rng.integers(w)] = 0
        out["random %g" % dens] = a
    for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):                        # the full scan radius
        a = np.full((h, w), 200, np.uint8)
        a[cy, cx] = 0
        out["corner %d %d" % (cy, cx)] = a
    out["all sites"] = np.zeros((h, w), np.uint8)
    a = np.full((h, w), 1, np.uint8); a[:, w // 3] = 0; out["one column"] = a
    a = np.full((h, w), 1, np.uint8); a[h // 3, :] = 0; out["one row"] = a
    a = random_mask(rng, h, w, 0.05); a[:, 5:40] = 3; a[:, w - 1] = 9; a[h // 2, 0] = 0; out["columns without a site"] = a
    return out


@pytest.mark.parametrize("h,w", PATTERN_SHAPES)
def test_site_patterns(cv, h, w):
    for name, a in patterns(h, w).items():
        check_all(cv, a)


def test_long_lines_root_in_double(cv):
    """one site at the end of 5000 pixels: squared distances above 2^24, where float would round before the root, and the longest scans"""
    for shape, at in (((1, 5000), (0, 0)), ((5000, 1), (4999, 0)), ((1, 5000), (0, 4999))):
        a = np.full(shape, 1, np.uint8)
        a[at] = 0
        got = run(cv, dev(a), L2, 0).cpu().numpy()
        assert np.array_equal(got, R.distanceTransform(a, L2))
        assert np.array_equal(np.sort(got.reshape(-1)), np.arange(5000, dtype=np.float32))
    a = np.full((4200, 64), 1, np.uint8)                                                   # roots of non-squares above 2^24: the rows from 4096 on
    a[0, 0] = 0
    got = run(cv, dev(a), L2, 0)[4096:].cpu().numpy()
    yy, xx = np.mgrid[4096:4200, 0:64].astype(np.int64)
    d2 = yy * yy + xx * xx
    assert d2.min() >= 1 << 24 and np.array_equal(got, np.sqrt(d2.astype(np.float64)).astype(np.float32))
    assert (got != np.sqrt(d2.astype(np.float32))).any()                                  # the float root of the rounded integer is another number somewhere here


def test_l1_into_8u(cv):
    a = np.full((1, 300), 7, np.uint8)
    a[0, 0] = 0
    got = run(cv, dev(a), L1, 3, np.uint8).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got[0], np.minimum(np.arange(300), 255))
    rng = np.random.default_rng(11)
    b = random_mask(rng, 45, 77, 0.01)
    b[44, 76] = 0
    assert np.array_equal(run(cv, dev(b), L1, 5, np.uint8).cpu().numpy(), R.distanceTransform(b, L1, np.uint8))


def test_mask_size_does_not_matter_for_l1_and_c(cv):
    rng = np.random.default_rng(12)
    a = random_mask(rng, 33, 70, 0.02)
    a[5, 5] = 0
    d = dev(a)
    for metric in (L1, C):
        want = R.distanceTransform(a, metric)
        for mask in (cv.DIST_MASK_3, cv.DIST_MASK_5, cv.DIST_MASK_PRECISE):
            assert np.array_equal(run(cv, d, metric, mask).cpu().numpy(), want), (metric, mask)


@pytest.mark.parametrize("metric,mask,dt", COMBOS)
def test_views_and_dst(cv, metric, mask, dt):
    """source and destination as views of wider tensors; the destination's parent is filled with a sentinel that must survive"""
    rng = np.random.default_rng(13)
    h, w = 70, 131
    sparent = random_mask(rng, h + 4, 200, 0.03)
    sparent[2 + 10, 7 + 20] = 0
    sentinel = rng.integers(1, 200, (h + 5, 150)).astype(dt)
    sp, dp = dev(sparent), dev(sentinel)
    sview, dview = sp[2:2 + h, 7:7 + w], dp[3:3 + h, 11:11 + w]
    out = run(cv, sview, metric, mask, dt, dst=dview)
    assert out is dview
    got = dp.cpu().numpy()
    assert np.array_equal(got[3:3 + h, 11:11 + w], R.distanceTransform(sparent[2:2 + h, 7:7 + w], metric, dt))
    keep = np.ones(sentinel.shape, bool)
    keep[3:3 + h, 11:11 + w] = False
    assert np.array_equal(got[keep], sentinel[keep])                                      # nothing outside the view written


def test_host_resident_image_is_staged(cv):
    rng = np.random.default_rng(14)
    a = random_mask(rng, 66, 90, 0.02)
    a[1, 1] = 0
    for metric, mask, dt in COMBOS:
        got = run(cv, a, metric, mask, dt)
        assert isinstance(got, np.ndarray) and got.dtype == dt
        assert np.array_equal(got, R.distanceTransform(a, metric, dt))


def batch_frames():
    rng = np.random.default_rng(15)
    h, w = 67, 140
    a = random_mask(rng, h, w, 0.03); a[0, 0] = 0
    b = np.full((h, w), 9, np.uint8)                                                      # no site
    c = np.full((h, w), 1, np.uint8); c[h - 1, w - 1] = 0
    return np.stack([a, b, c])


@pytest.mark.parametrize("metric,mask,dt", COMBOS)
def test_batch_with_a_frame_without_a_site(cv, metric, mask, dt):
    frames = batch_frames()
    n0 = cv.call_count("distanceTransformBatch")
    out = cv.distanceTransformBatch(dev(frames), metric, mask, dstType=cvtype(cv, dt))
    assert cv.call_count("distanceTransformBatch") == n0 + 1 and last_kernel(cv).startswith(KERNEL[(metric, dt)]), last_kernel(cv)
    got = out.cpu().numpy()
    assert got.shape == frames.shape and got.dtype == dt
    for i in range(3):
        assert np.array_equal(got[i], R.distanceTransform(frames[i], metric, dt)), i
    assert np.all(got[1] == (255 if dt == np.uint8 else np.float32(31622776.0)))


def test_host_resident_batch_goes_through_the_pipeline(cv):
    frames = batch_frames()
    n0 = cv.call_count("distanceTransformBatch")
    out = cv.distanceTransformBatch(torch.from_numpy(frames).pin_memory(), L2, 0)
    assert cv.call_count("distanceTransformBatch") > n0 and not out.is_cuda
    assert last_kernel(cv).startswith(KERNEL[(L2, np.float32)]), last_kernel(cv)
    for i in range(3):
        assert np.array_equal(out[i].numpy(), R.distanceTransform(frames[i], L2)), i


def test_declines_leave_the_destination_alone(cv):
    a = dev(np.zeros((16, 16), np.uint8))
    dst = torch.full((16, 16), 7.0, device="cuda")
    dst8 = torch.full((16, 16), 7, dtype=torch.uint8, device="cuda")
    calls = cv.call_count("distanceTransform")

    def declined(fn, entry="distanceTransform"):
        n0 = cv._lib.decline_count(entry)
        with pytest.raises(NotImplementedError):
            fn()
        assert cv._lib.decline_count(entry) == n0 + 1

    declined(lambda: cv.distanceTransform(a, L2, cv.DIST_MASK_3, dst=dst))                # the chamfer approximations
    declined(lambda: cv.distanceTransform(a, L2, cv.DIST_MASK_5, dst=dst))
    declined(lambda: cv.distanceTransform(a, 4, cv.DIST_MASK_3, dst=dst))                 # DIST_L12
    declined(lambda: cv.distanceTransform(a, L1, 7, dst=dst))
    declined(lambda: cv.distanceTransformBatch(a[None], L2, cv.DIST_MASK_3, dst=dst[None]), "distanceTransformBatch")
    with pytest.raises(ValueError):
        cv.distanceTransform(a, L2, 0, dstType=cv.CV_8U, dst=dst8)                        # the reference asserts
    # source and destination that overlap in HBM
    buf = torch.zeros(16 * 16 * 4, dtype=torch.uint8, device="cuda")
    before = buf.clone()
    declined(lambda: cv.distanceTransform(buf[:256].view(16, 16), L2, 0, dst=buf.view(torch.float32).view(16, 16)))
    declined(lambda: cv.distanceTransform(buf[:256].view(16, 16), L1, 3, dstType=cv.CV_8U, dst=buf[:256].view(16, 16)))
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert torch.all(dst == 7.0) and torch.all(dst8 == 7) and cv.call_count("distanceTransform") == calls
