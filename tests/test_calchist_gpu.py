"""calcHist / calcBackProject on the MI355X (opencv_amd.calcHist* / calcBackProject* -> mi355cv_calcHist*, mi355cv_calcBackProject*, opencv_amd/csrc/calchist.hip)
against the restatement (tests/calchist_restate.py), bit for bit -- there is no tolerance anywhere in this file.  Every call asserts that its call counter moved
and that mi355cv_lastKernel names the calchist kernels.

k_calchist_lds reads a row in units of 16 bytes (48 for three channels) between a scalar head and tail, 1024 units to a workgroup: 45 x 67 is one workgroup, 300 x 200
CV_8UC1 four, 1030 x 517 some 34; CV_8UC3 at 300 x 200 has 20 units a row.  k_calchist_generic and k_backproject walk 2048 pixels / 1024 dwords of output a workgroup."""
import ctypes

import numpy as np
import pytest
import torch

import calchist_restate as R
import viewcheck as V

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32


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


def depth_of(dtype):
    return R.CV_32S if np.dtype(dtype) == np.int32 else R.CV_32F


def hist_one(cv, t, channels, mask, hs, rg, uniform=True, dtype=F32, hist=None, accumulate=False, kernel="k_calchist_"):
    """one call on a device tensor (possibly a view); counter and kernel name asserted; the histogram comes back as numpy"""
    n0 = cv.call_count("calcHist")
    got = cv.calcHist([t], channels, mask, hs, rg, hist=hist, accumulate=accumulate, uniform=uniform, dtype=dtype)
    assert cv.call_count("calcHist") == n0 + 1 and last_kernel(cv).startswith(kernel), last_kernel(cv)
    assert ("nomask" in last_kernel(cv)) == (mask is None)
    assert got.is_cuda and tuple(got.shape) == tuple(hs)
    return got.cpu().numpy()


def check(cv, a, channels, m, hs, rg, uniform=True, kernel="k_calchist_", dtypes=(I32, F32)):
    for dt in dtypes:
        want = R.calchist_vec(a, channels, m, hs, rg, uniform, depth_of(dt))
        got = hist_one(cv, dev(a), channels, dev(m) if m is not None else None, hs, rg, uniform, dt, kernel=kernel)
        assert got.dtype == want.dtype and np.array_equal(got, want), (a.dtype, a.shape, channels, hs, rg, np.argwhere(got != want)[:4])
    return want


def random_image(rng, h, w, cn, dt):
    if np.dtype(dt) == np.float32:
        return (rng.random((h, w, cn)) * 3 - 1).astype(np.float32).reshape((h, w, cn) if cn > 1 else (h, w))
    top = int(np.iinfo(dt).max)
    a = rng.integers(0, top + 1, (h, w, cn)).astype(dt)
    a.ravel()[:2] = [0, top][:a.size]
    return a.reshape((h, w, cn) if cn > 1 else (h, w))


def full_range(dt):
    return [0, 1] if np.dtype(dt) == np.float32 else [0, int(np.iinfo(dt).max) + 1]


# ---- geometry
@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (67, 45), (200, 300), (517, 1030)])
def test_geometry(cv, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    h, w = shape
    a = random_image(rng, h, w, 1, np.uint8)
    check(cv, a, [0], None, [256], [0, 256], kernel="k_calchist_lds<1ch")
    check(cv, a, [0], (rng.random(shape) < 0.5).astype(np.uint8) * 7, [256], [0, 256], kernel="k_calchist_lds<1ch")
    if h * w <= 45 * 67 or h * w >= 200 * 300:                               # the three smallest and the two largest: the other depths, and the other channel counts
        for dt in (np.uint16, np.float32):
            b = random_image(rng, h, w, 1, dt)
            check(cv, b, [0], None, [256], full_range(dt), kernel="k_calchist_generic<")
            check(cv, b, [0], (rng.random(shape) < 0.5).astype(np.uint8), [256], full_range(dt), kernel="k_calchist_generic<", dtypes=(I32,))
        for cn in (2, 3, 4):
            c = random_image(rng, h, w, cn, np.uint8)
            check(cv, c, [cn - 1], None, [256], [0, 256], kernel="k_calchist_lds<%dch" % cn, dtypes=(I32,))
            check(cv, c, [0], (rng.random(shape) < 0.5).astype(np.uint8), [256], [0, 256], kernel="k_calchist_lds<%dch" % cn, dtypes=(I32,))


@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_roi_at_an_odd_origin_of_a_parent_that_only_a_sentinel_bin_can_receive(cv, cn):
    """the ROI's pixels lie in [0, 200); every other byte of the parent is 255 and bin 255 of a 256-bin histogram is the only one that can take it: any read outside
    the rows of the view shows there.  The mask comes from a ROI with its own pitch, inside a parent that selects everything."""
    rng = np.random.default_rng(3 + cn)
    for (h, w, y0, x0, ph, pw) in ((67, 45, 3, 5, 75, 61), (20, 130, 1, 1, 23, 135), (9, 16, 1, 3, 12, 21), (5, 3, 1, 1, 7, 6)):
        parent = np.full((ph, pw, cn), 255, np.uint8)
        inner = rng.integers(0, 200, (h, w, cn)).astype(np.uint8)
        parent[y0:y0 + h, x0:x0 + w] = inner
        p = dev(parent if cn > 1 else parent[:, :, 0])
        view = p[y0:y0 + h, x0:x0 + w]
        assert not view.is_contiguous()
        inner_ = inner if cn > 1 else inner[:, :, 0]
        for ch in range(cn):
            want = R.calchist_vec(inner_, [ch], None, [256], [0, 256], hist_depth=R.CV_32S)
            got = hist_one(cv, view, [ch], None, [256], [0, 256], dtype=I32, kernel="k_calchist_lds<%dch" % cn)
            assert got[255] == 0 and np.array_equal(got, want)
        pm = np.full((ph + 2, pw + 7), 255, np.uint8)
        m = (rng.random((h, w)) < 0.5).astype(np.uint8)
        pm[2:2 + h, 7:7 + w] = m
        got = hist_one(cv, view, [0], dev(pm)[2:2 + h, 7:7 + w], [256], [0, 256], dtype=I32)
        assert got[255] == 0 and np.array_equal(got, R.calchist_vec(inner_, [0], m, [256], [0, 256], hist_depth=R.CV_32S))
    if cn in (2, 4):                                                         # a base no pixel of which ever meets a 16-byte boundary: the byte-by-byte rows
        flat = torch.full((40 * 50 * cn + 64,), 255, dtype=torch.uint8, device="cuda")
        inner = rng.integers(0, 200, (40, 50, cn)).astype(np.uint8)
        odd = flat[1:1 + 40 * 50 * cn].view(40, 50, cn)
        odd.copy_(dev(inner))
        assert odd.data_ptr() % 2 == 1
        got = hist_one(cv, odd, [1], None, [256], [0, 256], dtype=I32)
        assert np.array_equal(got, R.calchist_vec(inner, [1], None, [256], [0, 256], hist_depth=R.CV_32S))


# ---- contention
def test_constant_and_checkerboard_frames(cv):
    for cn in (1, 3):
        a = np.full((200, 300, cn), 77, np.uint8)
        want = check(cv, a, [0], None, [256], [0, 256])
        assert want[77] == 60000 and want.sum() == 60000
        yy, xx = np.indices((200, 300))
        b = np.where((yy + xx) % 2 == 0, 10, 240).astype(np.uint8)
        b = np.repeat(b[:, :, None], cn, axis=2)
        want = check(cv, b, [cn - 1], None, [256], [0, 256])
        assert want[10] == want[240] == 30000
    for dt in (np.uint16, np.float32):                                       # the wave-uniform path of the atomics kernel
        check(cv, np.full((200, 300), 0.5 if dt == np.float32 else 30000, dt), [0], None, [256], full_range(dt), kernel="k_calchist_generic<")
    big = np.full((200, 300, 3), 9, np.uint8)                                # ... and of a CV_8U histogram too large for LDS
    check(cv, big, [0, 1, 2], None, [64, 64, 64], [0, 256] * 3, dtypes=(I32,))


def test_one_large_constant_frame_counts_past_2_to_24(cv):
    """4097 x 4097 = 16785409 pixels in one bin: exact as CV_32S; as CV_32F the tie between 16785408 and 16785410 goes to the even mantissa"""
    t = torch.full((4097, 4097), 200, dtype=torch.uint8, device="cuda")
    got = hist_one(cv, t, [0], None, [256], [0, 256], dtype=I32, kernel="k_calchist_lds<1ch")
    assert got[200] == 16785409 and got.sum() == 16785409
    got = hist_one(cv, t, [0], None, [256], [0, 256], dtype=F32, kernel="k_calchist_lds<1ch")
    assert got.dtype == np.float32 and got[200] == np.float32(16785409) == 16785408.0 and np.count_nonzero(got) == 1


# ---- bin parameters
@pytest.fixture(scope="module")
def frame8():
    rng = np.random.default_rng(17)
    return random_image(rng, 67, 45, 1, np.uint8), random_image(rng, 200, 300, 1, np.uint8)


@pytest.mark.parametrize("n", [1, 2, 7, 180, 256])
def test_bin_parameters(cv, frame8, n):
    for (lo, hi) in ((0, 256), (0, 180), (10.5, 200.25), (-5, 300)):
        for a in frame8:
            check(cv, a, [0], None, [n], [lo, hi], dtypes=(I32,))


# ---- CV_16U
def test_16u(cv):
    rng = np.random.default_rng(19)
    a = random_image(rng, 200, 300, 1, np.uint16)
    check(cv, a, [0], None, [1000], [0, 65536], kernel="k_calchist_generic<16u")
    want = check(cv, a, [0], None, [65536], [0, 65536], kernel="k_calchist_generic<16u")                    # the per-dimension bound
    assert np.array_equal(want, np.bincount(a.ravel(), minlength=65536).astype(np.float32))
    check(cv, a, [0], None, [7], [100.5, 40000.25], kernel="k_calchist_generic<16u", dtypes=(I32,))
    c = random_image(rng, 67, 45, 3, np.uint16)
    check(cv, c, [2, 0], None, [16, 8], [0, 65536, 1000, 50000], kernel="k_calchist_generic<16u", dtypes=(I32,))
    n0 = cv._lib.decline_count("calcHist")
    with pytest.raises(NotImplementedError):
        cv.calcHist([dev(a)], [0], None, [R.MAX_BINS_PER_DIM + 1], [0, 65536])
    assert cv._lib.decline_count("calcHist") == n0 + 1


# ---- several dimensions
@pytest.fixture(scope="module")
def frames_color():
    rng = np.random.default_rng(23)
    return {3: random_image(rng, 200, 300, 3, np.uint8), 4: random_image(rng, 67, 45, 4, np.uint8)}


@pytest.mark.parametrize("case", [((0, 1), (30, 32), "lds"), ((2, 0), (7, 5), "lds"), ((0, 1), (180, 256), "generic"), ((0, 1, 2), (8, 8, 8), "lds"),
                                  ((0, 1, 2), (32, 32, 32), "lds"), ((0, 1, 2), (64, 64, 64), "generic"), ((1, 1), (16, 16), "lds"), ((2, 1, 2), (4, 9, 5), "lds")],
                         ids=lambda c: "ch%s-%s" % ("".join(map(str, c[0])), "x".join(map(str, c[1]))))
def test_several_dimensions(cv, frames_color, case):
    channels, hs, kernel = case
    rgs = {1: [0, 256], 2: [0, 256, 0, 256], 3: [0, 256, 10.5, 200.25, -5, 300]}[len(hs)] if hs != (30, 32) else [0, 180, 0, 256]
    for cn, a in frames_color.items():
        check(cv, a, list(channels), None, list(hs), rgs, kernel="k_calchist_" + kernel, dtypes=(I32,) if cn == 4 else (I32, F32))
        if hs == (32, 32, 32):                                               # 3 KiB of tables and one copy of 32769 words: the dynamic LDS above 64 KiB
            assert last_kernel(cv).startswith("k_calchist_lds<%dch" % cn) and "copies=1 " in last_kernel(cv) and "lds=134148" in last_kernel(cv), last_kernel(cv)
    m = (np.random.default_rng(29).random((200, 300)) < 0.3).astype(np.uint8)
    check(cv, frames_color[3], list(channels), m, list(hs), rgs, kernel="k_calchist_" + kernel, dtypes=(I32,))


def test_product_of_sizes_just_above_the_bound_is_declined(cv, frames_color):
    assert cv.limit(R.MAX_BINS_KEY) == R.MAX_BINS == 1024 * 1024
    t = dev(frames_color[3])
    n0 = cv._lib.decline_count("calcHist")
    side, whole = R.MAX_BINS // 1024, full_range(np.uint8)                     # the refusals are derived from the bound, not written as numbers
    with pytest.raises(NotImplementedError):
        cv.calcHist([t], [0, 1], None, [side, side + 1], whole * 2)
    with pytest.raises(NotImplementedError):
        cv.calcHist([t], [0, 1, 2], None, [128, 128, R.MAX_BINS // (128 * 128) + 1], whole * 3)
    assert cv._lib.decline_count("calcHist") == n0 + 2
    got = hist_one(cv, t, [0, 1], None, [1024, 1024], [0, 256, 0, 256], dtype=I32, kernel="k_calchist_generic<8u")      # AT the bound
    assert np.array_equal(got, R.calchist_vec(frames_color[3], [0, 1], None, [1024, 1024], [0, 256, 0, 256], hist_depth=R.CV_32S))


# ---- overlap in HBM
def declined_for_overlap(cv, entry, call, *buffers):
    """`call` is refused for an overlap: NotImplementedError, the reason, a moved decline counter, no call counted, every byte of `buffers` as it was"""
    before = [b.clone() for b in buffers]
    d0, c0 = cv._lib.decline_count(entry), cv.call_count(entry)
    with pytest.raises(NotImplementedError, match="overlap"):
        call()
    torch.cuda.synchronize()
    assert "overlap" in cv._lib.lib.mi355cv_lastError().decode()
    assert cv._lib.decline_count(entry) == d0 + 1 and cv.call_count(entry) == c0
    assert all(torch.equal(b, k) for b, k in zip(buffers, before))


def test_a_histogram_or_destination_that_overlaps_an_input_in_hbm_is_declined(cv):
    """every overlap the entries refuse that one GPU can show: a histogram inside the source, a histogram inside the mask (each at its first and at its last bytes, so
    that both ends of the span arithmetic are held), a destination that is the source, a destination inside the histogram.  "Arguments on different devices" needs a
    second GPU and is not tested here."""
    h, w = 64, 64
    rng = np.random.default_rng(83)
    buf = dev(rng.integers(0, 256, h * w + 1024, dtype=np.uint8))             # the source's 4096 bytes, then 1024 bytes of its own
    src = buf[:h * w].view(h, w)
    other = dev(rng.integers(1, 256, h * w + 1024, dtype=np.uint8))
    mask = other[:h * w].view(h, w)
    one = ([0], None, [256], [0, 256])
    for first in (0, (h * w - 4) // 4):                                      # cells that begin on the span's first bytes, and on its last four
        hist = buf.view(torch.int32)[first:first + 256]
        declined_for_overlap(cv, "calcHist", lambda: cv.calcHist([src], *one, hist=hist), buf)
        declined_for_overlap(cv, "calcHist", lambda: cv.calcHist([src], *one, hist=hist.view(torch.float32), accumulate=True), buf)
        hist = other.view(torch.int32)[first:first + 256]
        declined_for_overlap(cv, "calcHist", lambda: cv.calcHist([src], [0], mask, [256], [0, 256], hist=hist), buf, other)
    # ... and the cells just past the source are served
    clear = buf.view(torch.int32)[h * w // 4:]
    got = hist_one(cv, src, *one, hist=clear, kernel="k_calchist_lds<1ch")
    assert np.array_equal(got, R.calchist_vec(src.cpu().numpy(), *one, hist_depth=R.CV_32S))
    # the batch entry: the last frame's last row ends on the histogram's first cell
    frames = buf[:h * w].view(4, h // 4, w)
    before = buf.clone()
    lib = cv._lib.lib
    ch, hs, rg = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(256), (ctypes.c_float * 2)(0, 256)
    rc = lib.mi355cv_calcHistBatch(ctypes.c_void_p(frames.data_ptr()), w, (h // 4) * w, w, h // 4, 0, 1, 4, ch, 1, hs, rg, 1, None, 0, 0,
                                   ctypes.c_void_p(buf.data_ptr() + h * w - 4), R.CV_32S, 0)
    torch.cuda.synchronize()
    assert rc == 1 and "overlap" in lib.mi355cv_lastError().decode() and torch.equal(buf, before)

    # back-projection: dst is the source; dst ends on the histogram's first cell; dst begins on its last
    hb = dev(rng.random(h * w, dtype=np.float32) * 300)
    raw = hb.view(torch.uint8)
    hist = hb[1024:1280]                                                     # bytes 4096 ... 5120 of hb
    declined_for_overlap(cv, "calcBackProject", lambda: cv.calcBackProject([src], [0], hist, [0, 256], 1.0, dst=src), buf, hb)
    for first in (4, 5120 - 4):
        dst = raw[first:first + h * w].view(h, w)
        declined_for_overlap(cv, "calcBackProject", lambda: cv.calcBackProject([src], [0], hist, [0, 256], 1.0, dst=dst), buf, hb)
    keep = hist.clone()
    want = R.backproject_vec(src.cpu().numpy(), [0], keep.cpu().numpy(), [0, 256], 1.0)
    for first in (0, 5120):                                                  # ... and a destination that ends where the cells begin, or begins where they end, is served
        got = project(cv, src, [0], hist, [0, 256], 1.0, dst=raw[first:first + h * w].view(h, w))
        assert torch.equal(hist, keep) and np.array_equal(got.cpu().numpy(), want)
    frames3 = dev(rng.integers(0, 256, (3, 16, 16), dtype=np.uint8))
    declined_for_overlap(cv, "calcBackProjectBatch", lambda: cv.calcBackProjectBatch(frames3, [0], hist, [0, 256], 1.0, dst=frames3), frames3)


# ---- non-uniform
def test_non_uniform_ranges(cv, frames_color):
    rng = np.random.default_rng(31)
    b8 = np.array([3, 10, 11, 50.5, 128, 200, 250], np.float32)              # the first boundary above 0, the last below 255
    a = random_image(rng, 200, 300, 1, np.uint8)
    want = check(cv, a, [0], None, [6], b8, uniform=False, kernel="k_calchist_lds<")
    assert want.sum() < a.size
    check(cv, frames_color[3], [2, 0], None, [6, 3], [b8, [0, 1, 100.5, 256]], uniform=False, kernel="k_calchist_lds<")
    b16 = np.array([100, 101, 1000.5, 30000, 65000], np.float32)
    s = random_image(rng, 200, 300, 1, np.uint16)
    s[0, :40] = np.array([99, 100, 101, 1000, 1001, 29999, 30000, 64999, 65000, 65535] * 4, np.uint16)
    want = check(cv, s, [0], None, [4], b16, uniform=False, kernel="k_calchist_generic<16u")
    assert want.sum() < s.size
    with pytest.raises(NotImplementedError):
        cv.calcHist([dev(a.astype(np.float32))], [0], None, [6], b8, uniform=False)


# ---- CV_32F
def test_32f_with_special_and_fma_sensitive_values(cv):
    rng = np.random.default_rng(37)
    a = (rng.random((200, 300)) * 3 - 1).astype(np.float32)                  # uniform(-1, 2)
    special = R.f32_special_values(0, 1)
    a.ravel()[1000:1000 + len(special)] = special
    check(cv, a, [0], None, [64], [0, 1], kernel="k_calchist_generic<32f")
    found = 0
    for n, lo, hi in R.FMA_RANGES:
        cand = np.array(R.fma_candidates(n, lo, hi), np.float32)
        sens = R.fma_sensitive(n, lo, hi, cand)
        found += len(sens)
        sens = sens[:4]
        b = (rng.random((67, 45)) * (hi - lo) * 1.5 + lo - 0.25 * (hi - lo)).astype(np.float32)
        b.ravel()[:min(cand.size, 2000)] = cand[:2000]
        b.ravel()[2000:2000 + len(sens)] = [v for v, _, _ in sens]
        b.ravel()[2500:2500 + len(special)] = R.f32_special_values(lo, hi)
        want = check(cv, b, [0], None, [n], [lo, hi], kernel="k_calchist_generic<32f", dtypes=(I32,))
        for v, two, fused in sens:                                           # a frame of that value alone: all of it in the two-rounding bin
            got = hist_one(cv, dev(np.full((3, 5), v, np.float32)), [0], None, [n], [lo, hi], dtype=I32)
            assert got[two] == 15 and got[fused] == 0
        assert want.sum() > 0
    assert found >= 1
    c = np.stack([a, a[::-1], -a], axis=2)                                   # three channels, two dimensions
    check(cv, c, [2, 0], None, [5, 9], [-1, 0.5, 0, 1], kernel="k_calchist_generic<32f", dtypes=(I32,))


# ---- accumulate
@pytest.mark.parametrize("dt", [I32, F32])
def test_accumulate(cv, frame8, dt):
    a = frame8[1]
    t = dev(a)
    once = hist_one(cv, t, [0], None, [32], [0, 256], dtype=dt)
    h = cv.calcHist([t], [0], None, [32], [0, 256], dtype=dt)
    got = hist_one(cv, t, [0], None, [32], [0, 256], hist=h, accumulate=True)
    assert got.dtype == np.dtype(dt) and np.array_equal(got, 2 * once)
    start = (np.random.default_rng(41).random(32) * 1000).astype(np.float32) if dt == F32 else np.random.default_rng(41).integers(-50, 1000, 32).astype(np.int32)
    if dt == F32:
        start[:4] = [2.5, 3.5, 0.49999997, 1e6 + 0.5]                        # non-integers, ties to even
    got = hist_one(cv, t, [0], None, [32], [0, 256], hist=dev(start), accumulate=True)
    assert np.array_equal(got, R.calchist_vec(a, [0], None, [32], [0, 256], hist_depth=depth_of(dt), start=start))
    s16 = random_image(np.random.default_rng(43), 67, 45, 1, np.uint16)      # the atomics kernel, and a host-resident histogram
    hh = start.copy()
    n0 = cv.call_count("calcHist")
    out = cv.calcHist([s16], [0], None, [32], [0, 65536], hist=hh, accumulate=True)
    assert cv.call_count("calcHist") == n0 + 1 and out is hh
    assert np.array_equal(hh, R.calchist_vec(s16, [0], None, [32], [0, 65536], hist_depth=depth_of(dt), start=start))


# ---- batch
def batch(cv, t, channels, mask, hs, rg, dtype=F32, device=False, uniform=True):
    n0 = cv.call_count("calcHistBatch")
    got = cv.calcHistBatch(t, channels, mask, hs, rg, uniform=uniform, dtype=dtype, device=device)
    assert cv.call_count("calcHistBatch") == n0 + 1 and last_kernel(cv).startswith("k_calchist_"), last_kernel(cv)
    assert got.is_cuda == device and tuple(got.shape) == (t.shape[0],) + tuple(hs) and got.dtype == (torch.float32 if dtype == F32 else torch.int32)
    return got


@pytest.mark.parametrize("kind", ["8uc1", "8uc3", "16uc1", "32fc1"])
def test_batch(cv, kind):
    rng = np.random.default_rng(47)
    dt, cn = {"8uc1": (np.uint8, 1), "8uc3": (np.uint8, 3), "16uc1": (np.uint16, 1), "32fc1": (np.float32, 1)}[kind]
    nb, h, w = 5, 67, 45
    parent = np.stack([random_image(rng, h + 3, w + 5 + 6, cn, dt) for _ in range(nb)])
    t = dev(parent)[:, 3:, 5:5 + w]                                          # frames[:, 3:, 5:]-style view: base, pitch and frame stride all ragged
    assert not t.is_contiguous()
    frames = parent[:, 3:, 5:5 + w]
    channels, hs, rg = ([0], [64], full_range(dt)) if cn == 1 else ([2, 0], [30, 32], [0, 180, 0, 256])
    want = [R.calchist_vec(frames[f], channels, None, hs, rg, hist_depth=R.CV_32S) for f in range(nb)]
    got = batch(cv, t, channels, None, hs, rg, dtype=I32).numpy()
    assert all(np.array_equal(got[f], want[f]) for f in range(nb))
    assert np.array_equal(got, np.stack([hist_one(cv, t[f], channels, None, hs, rg, dtype=I32) for f in range(nb)]))       # the batch equals the per-frame calls
    d = batch(cv, t, channels, None, hs, rg, dtype=F32, device=True)         # stays in HBM
    assert np.array_equal(d.cpu().numpy(), got.astype(np.float32))
    shared = (rng.random((h, w)) < 0.5).astype(np.uint8)
    got = batch(cv, t, channels, dev(shared), hs, rg, dtype=I32).numpy()
    assert all(np.array_equal(got[f], R.calchist_vec(frames[f], channels, shared, hs, rg, hist_depth=R.CV_32S)) for f in range(nb))
    per = (rng.random((nb, h, w)) < 0.5).astype(np.uint8) * 9
    per[nb - 1] = 0                                                          # an all-zero mask: an all-zero histogram
    pm = np.full((nb, h + 2, w + 3), 255, np.uint8)
    pm[:, 1:1 + h, 2:2 + w] = per
    got = batch(cv, t, channels, dev(pm)[:, 1:1 + h, 2:2 + w], hs, rg, dtype=I32, device=True).cpu().numpy()
    assert all(np.array_equal(got[f], R.calchist_vec(frames[f], channels, per[f], hs, rg, hist_depth=R.CV_32S)) for f in range(nb))
    assert not got[nb - 1].any() and got[0].any()


def test_host_resident_batch_under_the_suites_host_policy(cv):
    rng = np.random.default_rng(53)
    frames = np.stack([random_image(rng, 67, 45, 3, np.uint8) for _ in range(3)])
    mask = (rng.random((3, 67, 45)) < 0.5).astype(np.uint8)
    t = torch.from_numpy(frames)
    s0 = cv._lib.lib.mi355cv_stagedBytes()
    got = batch(cv, t, [0, 1], torch.from_numpy(mask), [30, 32], [0, 180, 0, 256], dtype=F32).numpy()
    assert cv._lib.lib.mi355cv_stagedBytes() > s0
    assert all(np.array_equal(got[f], R.calchist_vec(frames[f], [0, 1], mask[f], [30, 32], [0, 180, 0, 256])) for f in range(3))
    one = cv.calcHist([frames[1]], [0, 1], mask[1], [30, 32], [0, 180, 0, 256])                           # numpy in, numpy out
    assert isinstance(one, np.ndarray) and np.array_equal(one, got[1])


# ---- back-projection
def project(cv, t, channels, hist, rg, scale, uniform=True, dst=None):
    n0 = cv.call_count("calcBackProject")
    got = cv.calcBackProject([t], channels, hist, rg, scale, uniform=uniform, dst=dst)
    assert cv.call_count("calcBackProject") == n0 + 1 and last_kernel(cv).startswith("k_backproject<"), last_kernel(cv)
    return got


def check_project(cv, a, channels, hist, rg, scale, uniform=True, mode=None):
    want = R.backproject_vec(a, channels, hist, rg, scale, uniform)
    for hh in (hist, dev(hist)):                                             # the histogram on the host (it is uploaded), and in HBM
        got = project(cv, dev(a), channels, hh, rg, scale, uniform)
        assert got.is_cuda and got.dtype == dev(a).dtype and tuple(got.shape) == a.shape[:2]
        ok, idx, detail = V.exact(got.cpu().numpy(), want)
        assert ok, (a.dtype, channels, hist.shape, scale, idx, detail)
        assert mode is None or ("mode=" + mode) in last_kernel(cv), last_kernel(cv)
    return want


def scales_for(hist):
    return (1.0, 0.37, 255.0 / float(hist.max()))


def test_back_projection_8u(cv, frames_color):
    rng = np.random.default_rng(59)
    a = random_image(rng, 200, 300, 1, np.uint8)
    for n, rg in ((256, [0, 256]), (180, [10.5, 200.25]), (7, [-5, 300])):
        hist = R.calchist_vec(a, [0], None, [n], rg)
        hist[0] += 0.5                                                       # a non-integer: the rounding matters at scale 1 too
        for scale in scales_for(hist):
            want = check_project(cv, a, [0], hist, rg, scale, mode="lut256")
        if rg[0] > 0:
            assert (want[a < rg[0]] == 0).all() and (want[a >= rg[1]] == 0).all() and want.any()          # out-of-range pixels give 0
    hist = R.calchist_vec(a, [0], None, [256], [0, 256])
    want = check_project(cv, a, [0], hist, [0, 256], 1.05)                   # a scale that saturates the fuller bins (234 pixels a bin on average)
    assert (want == 255).sum() > 1000 and (want < 255).sum() > 1000
    assert (check_project(cv, a, [0], hist, [0, 256], 3.0) == 255).all()
    assert not check_project(cv, a, [0], hist, [0, 256], -1.0).any()
    c = frames_color[3]
    for channels, hs, rg in (([0, 1], [30, 32], [0, 180, 0, 256]), ([0, 1, 2], [8, 8, 8], [0, 256, 10.5, 200.25, -5, 300]), ([2, 2], [16, 4], [0, 256, 0, 128])):
        hist = R.calchist_vec(c, channels, None, hs, rg)
        for scale in scales_for(hist):
            check_project(cv, c, channels, hist, rg, scale, mode="lds")
    hist = R.calchist_vec(c, [0, 1], None, [180, 256], [0, 180, 0, 256])     # too many cells for LDS: gathered
    check_project(cv, c, [0, 1], hist, [0, 180, 0, 256], 7.5, mode="gather")
    b8 = np.array([3, 10, 11, 50.5, 128, 200, 250], np.float32)
    check_project(cv, a, [0], np.array([1, 20, 300, 4.5, 5.5, 60], np.float32), b8, 0.5, uniform=False, mode="lut256")


def test_back_projection_16u_and_32f(cv):
    rng = np.random.default_rng(61)
    s = random_image(rng, 200, 300, 1, np.uint16)
    hist = R.calchist_vec(s, [0], None, [1000], [0, 65536])
    for scale in scales_for(hist) + (900.0,):                                # 900: saturates CV_16U
        want = check_project(cv, s, [0], hist, [0, 65536], scale, mode="lds")
    assert (want == 65535).any()
    check_project(cv, s, [0], R.calchist_vec(s, [0], None, [65536], [0, 65536]), [0, 65536], 1000.0, mode="gather")
    want = check_project(cv, s, [0], np.array([5, 6, 7.5, 8], np.float32), np.array([100, 101, 1000.5, 30000, 65000], np.float32), 1.0, uniform=False)
    assert (want[s >= 65000] == 0).all() and (want[s < 100] == 0).all()
    c = random_image(rng, 67, 45, 3, np.uint16)
    check_project(cv, c, [2, 0], R.calchist_vec(c, [2, 0], None, [16, 8], [0, 65536, 1000, 50000]), [0, 65536, 1000, 50000], 0.37)
    a = (rng.random((200, 300)) * 3 - 1).astype(np.float32)
    special = R.f32_special_values(0, 1)
    a.ravel()[1000:1000 + len(special)] = special
    hist = R.calchist_vec(a, [0], None, [64], [0, 1])
    for scale in scales_for(hist) + (1e38,):                                 # 1e38: the float overflows to inf, as (float)p does
        want = check_project(cv, a, [0], hist, [0, 1], scale, mode="lds")
    assert np.isinf(want).any() and (want[~((a >= 0) & (a < 1))] == 0).all()
    f3 = np.stack([a, a[::-1], -a], axis=2)
    check_project(cv, f3, [2, 0], R.calchist_vec(f3, [2, 0], None, [5, 9], [-1, 0.5, 0, 1]), [-1, 0.5, 0, 1], 0.37)


def test_back_projection_batch_with_shared_and_per_frame_histograms(cv):
    rng = np.random.default_rng(67)
    nb, h, w = 4, 67, 45
    parent = np.stack([random_image(rng, h + 3, w + 11, 3, np.uint8) for _ in range(nb)])
    t = dev(parent)[:, 3:, 5:5 + w]
    frames = parent[:, 3:, 5:5 + w]
    channels, hs, rg = [0, 1], [30, 32], [0, 180, 0, 256]
    hists = np.stack([R.calchist_vec(frames[f], channels, None, hs, rg) for f in range(nb)])
    for hist, per in ((hists[1], False), (hists, True)):
        for hh in (hist, dev(hist)):
            n0 = cv.call_count("calcBackProjectBatch")
            got = cv.calcBackProjectBatch(t, channels, hh, rg, 0.37)
            assert cv.call_count("calcBackProjectBatch") == n0 + 1 and last_kernel(cv).startswith("k_backproject<8u"), last_kernel(cv)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (nb, h, w)
            got = got.cpu().numpy()
            for f in range(nb):
                assert np.array_equal(got[f], R.backproject_vec(frames[f], channels, hists[f] if per else hist, rg, 0.37)), (per, f)
    host = cv.calcBackProjectBatch(torch.from_numpy(np.ascontiguousarray(frames)), channels, hists, rg, 0.37)             # a host-resident batch
    assert not host.is_cuda and np.array_equal(host.numpy(), got)


class Device:
    @staticmethod
    def put(a):
        return torch.from_numpy(a).cuda()

    @staticmethod
    def get(a):
        return a.cpu().numpy()


@pytest.mark.parametrize("layout", ["B", "C", "E", "F"])
@pytest.mark.parametrize("kind", ["8uc1", "8uc3", "16uc1", "32fc1"])
def test_back_projection_into_a_guarded_pitched_roi(cv, kind, layout):
    dt, cn = {"8uc1": (np.uint8, 1), "8uc3": (np.uint8, 3), "16uc1": (np.uint16, 1), "32fc1": (np.float32, 1)}[kind]
    h, w = 37, 45
    img = V.content(dt, (h, w, cn) if cn > 1 else (h, w), 71, lo=0 if dt == np.float32 else None, hi=1 if dt == np.float32 else None)
    channels, hs, rg = ([0], [64], full_range(dt)) if cn == 1 else ([2, 0], [30, 32], [0, 180, 0, 256])
    hist = R.calchist_vec(img, channels, None, hs, rg) + np.float32(0.5)
    want = R.backproject_vec(img, channels, hist, rg, 2.25)
    assert want.any()
    name, _ = V.run(lambda s, d: project(cv, s, channels, hist, rg, 2.25, dst=d), layout, img, want, what="calcBackProject " + kind, device=Device,
                    kernel_name=lambda: last_kernel(cv))
    assert name.startswith("k_backproject<")


# ---- pipeline
def test_hue_saturation_histogram_and_back_projection_without_leaving_the_device(cv):
    rng = np.random.default_rng(73)
    bgr = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    bgr[50:120, 80:200] = (rng.integers(0, 40, (70, 120, 3)) + np.array([20, 180, 200])).astype(np.uint8)               # a region of one colour
    mask = np.zeros((200, 300), np.uint8)
    mask[50:120, 80:200] = 255
    hsv = cv.cvtColor(dev(bgr), cv.COLOR_BGR2HSV)
    assert hsv.is_cuda
    hsv_host = hsv.cpu().numpy()
    channels, hs, rg = [0, 1], [30, 32], [0, 180, 0, 256]
    hist = batch(cv, hsv[None], channels, dev(mask), hs, rg, dtype=F32, device=True)
    want_hist = R.calchist_vec(hsv_host, channels, mask, hs, rg)
    assert np.array_equal(hist[0].cpu().numpy(), want_hist) and want_hist.sum() == 70 * 120
    scale = 255.0 / float(want_hist.max())
    bp = project(cv, hsv, channels, hist[0], rg, scale)
    assert bp.is_cuda
    want = R.backproject_vec(hsv_host, channels, hist[0].cpu().numpy(), rg, scale)
    assert np.array_equal(bp.cpu().numpy(), want)
    assert want[50:120, 80:200].mean() > 4 * want[130:, :].mean()            # the region lights up
