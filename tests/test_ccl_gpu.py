"""connectedComponents on the MI355X (opencv_amd.connectedComponents* -> mi355cv_connectedComponents*, opencv_amd/csrc/ccl.hip) against the numpy restatement
(tests/ccl_restate.py): labels and N bit for bit, stats and centroids bit for bit (NaN rows with equal_nan).  Every call asserts that its call counter moved and
that mi355cv_lastKernel names the labelling kernel with the order, the connectivity and the label type asked for.  k_ccl_strip works on tiles of T = 256 columns
x S = 16 rows, a wave each; the shapes sit around those two numbers."""
import ctypes

import numpy as np
import pytest
import torch

import ccl_restate as R

pytestmark = pytest.mark.gpu

T, S = R.TILE_W, R.STRIP_H
assert (T, S) == (256, 16)
# (connectivity, ccltype): pixel order at 4, pixel order at 8, block order at 8
MODES = [(4, R.CCL_DEFAULT), (8, R.CCL_SAUF), (8, R.CCL_DEFAULT)]


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return opencv_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def full16(shape, v):
    """a CV_16U tensor filled with v (filled as int16: the 16-bit unsigned type has few operators)"""
    return torch.full(shape, v, dtype=torch.int16, device="cuda").view(torch.uint16)


def last_kernel(cv):
    return cv._lib.lib.mi355cv_lastKernel().decode()


def lt_of(cv, dt):
    return cv.CV_16U if dt == np.uint16 else cv.CV_32S


def kernel_name(conn, ccl, dt):
    return "k_ccl_strip<%s,%d,%s>" % (R.order_of(conn, ccl), conn, "16U" if dt == np.uint16 else "32S")


def run(cv, src, conn, ccl, dt=np.int32, **kw):
    """connectedComponentsWithStats with the bookkeeping asserted -> numpy (n, labels, stats, centroids)"""
    n0, s0 = cv.call_count("connectedComponents"), cv.call_count("connectedComponentsStats")
    n, lab, st, ce = cv.connectedComponentsWithStats(src, connectivity=conn, ltype=lt_of(cv, dt), ccltype=ccl, **kw)
    assert cv.call_count("connectedComponents") == n0 + 1 and cv.call_count("connectedComponentsStats") == s0 + 1, "the GPU path did not run"
    assert last_kernel(cv).startswith("k_ccl_stats<%s>" % ("16U" if dt == np.uint16 else "32S")), last_kernel(cv)
    tonp = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return n, tonp(lab), tonp(st), tonp(ce)


def labels_only(cv, src, conn, ccl, dt=np.int32, **kw):
    n0 = cv.call_count("connectedComponents")
    n, lab = cv.connectedComponents(src, connectivity=conn, ltype=lt_of(cv, dt), ccltype=ccl, **kw)
    assert cv.call_count("connectedComponents") == n0 + 1, "the GPU path did not run"
    assert last_kernel(cv).startswith(kernel_name(conn, ccl, dt)), last_kernel(cv)
    return n, lab


def check(cv, a, modes=MODES, dts=(np.int32,), what=""):
    d = dev(a)
    for conn, ccl in modes:
        wn, want = R.label(a, conn, R.order_of(conn, ccl))
        wst, wce = R.stats(want, wn)
        for dt in dts:
            n, lab = labels_only(cv, d, conn, ccl, dt)
            lab = lab.cpu().numpy()
            assert n == wn and lab.dtype == dt and np.array_equal(lab, want), (what, a.shape, conn, ccl, dt)
            n, lab, st, ce = run(cv, d, conn, ccl, dt)
            assert n == wn and np.array_equal(lab, want) and R.same_stats(st, ce, wst, wce), (what, a.shape, conn, ccl, dt)


def test_one_pixel(cv):
    check(cv, np.ones((1, 1), np.uint8), dts=(np.int32, np.uint16))                       # the empty-background rule at its smallest: N = 2, row 0 zeros and NaN
    check(cv, np.zeros((1, 1), np.uint8), dts=(np.int32, np.uint16))
    n, lab, st, ce = run(cv, dev(np.ones((1, 1), np.uint8)), 8, R.CCL_DEFAULT)
    assert n == 2 and st.tolist() == [[0, 0, 0, 0, 0], [0, 0, 1, 1, 1]] and np.isnan(ce[0]).all() and ce[1].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257])
def test_single_rows_and_columns(cv, n):
    rng = np.random.default_rng(n)
    for shape in ((1, n), (n, 1)):
        check(cv, R.random_frame(rng, shape[0], shape[1], 0.6))
        check(cv, np.ones(shape, np.uint8), modes=MODES[1:])
        a = np.ones(shape, np.uint8); a.flat[n // 2] = 0
        check(cv, a, modes=MODES[:2], dts=(np.uint16,))


PATTERN_SHAPES = [(S - 1, T - 1), (S, T), (S + 1, T + 1), (2 * S + 1, 2 * T + 1), (S + 1, 2 * T + 1), (2 * S + 1, T - 1)]


@pytest.mark.parametrize("h,w", PATTERN_SHAPES)
def test_patterns_around_tile_and_strip(cv, h, w):
    """random frames at the four densities, serpentine, comb, spiral, rings, diagonals, pairs at the word and tile seams, checkerboard, the frame on which the two
    orders differ, all foreground (N = 2, row 0 zeros with a NaN centroid), all background (N = 1)"""
    for name, a in R.patterns(h, w).items():
        check(cv, a, what=name)
    n, lab, st, ce = run(cv, dev(np.full((h, w), 3, np.uint8)), 8, R.CCL_DEFAULT)
    assert n == 2 and st[0].tolist() == [0] * 5 and np.isnan(ce[0]).all() and st[1].tolist() == [0, 0, w, h, w * h]
    n, lab, st, ce = run(cv, dev(np.zeros((h, w), np.uint8)), 4, R.CCL_DEFAULT)
    assert n == 1 and st.tolist() == [[0, 0, w, h, w * h]]
    cb = R.checkerboard(h, w)
    assert labels_only(cv, dev(cb), 8, R.CCL_DEFAULT)[0] == 2 and labels_only(cv, dev(cb), 4, R.CCL_DEFAULT)[0] == 1 + (h * w + 1) // 2


def test_labels_into_16u(cv):
    for name, a in R.patterns(2 * S + 1, T + 1, seed=1).items():
        check(cv, a, dts=(np.uint16,), what=name)


def test_every_ccltype_picks_its_order(cv):
    a = R.orders_differ(2 * S + 2, T + 9)
    d = dev(a)
    for conn in (4, 8):
        for ccl in (-1, 0, 1, 2, 3, 4, 5):
            n, lab = labels_only(cv, d, conn, ccl)
            wn, want = R.label(a, conn, R.order_of(conn, ccl))
            assert n == wn and np.array_equal(lab.cpu().numpy(), want), (conn, ccl)
    pix, blk = R.label(a, 8, R.PIXEL)[1], R.label(a, 8, R.BLOCK)[1]
    assert (pix != blk).sum() == (a != 0).sum() > 100                                     # the two orders differ at every foreground pixel of this frame


def test_16u_at_its_bound(cv):
    """511 x 511 with isolated pixels at even (x, y): 65536 components, one too many for CV_16U -- declined, destination intact; one pixel fewer is served and its
    highest label is 65535"""
    a = np.zeros((511, 511), np.uint8)
    a[0::2, 0::2] = 255
    assert (a != 0).sum() == 65536
    d = dev(a)
    dst = full16((511, 511), 77)
    calls, n0 = cv.call_count("connectedComponents"), cv._lib.decline_count("connectedComponents")
    with pytest.raises(NotImplementedError, match="65535"):
        cv.connectedComponents(d, labels=dst, connectivity=8, ltype=cv.CV_16U)
    torch.cuda.synchronize()
    assert cv._lib.decline_count("connectedComponents") == n0 + 1 and cv.call_count("connectedComponents") == calls
    assert bool((dst.cpu().view(torch.int16) == 77).all())
    n, lab = labels_only(cv, d, 8, R.CCL_DEFAULT)                                         # CV_32S holds them
    assert n == 65537 and int(lab.max()) == 65536
    a[510, 510] = 0
    wn, want = R.label(a, 8, R.BLOCK)
    n, lab = labels_only(cv, dev(a), 8, R.CCL_DEFAULT, np.uint16, labels=dst)
    got = lab.cpu().numpy()
    assert lab is dst and n == wn == 65536 and got.dtype == np.uint16 and int(got.max()) == 65535 and np.array_equal(got, want)


@pytest.mark.parametrize("conn,ccl", MODES)
def test_views_and_strides(cv, conn, ccl):
    """source and labels as interior views of wider tensors, stats and centroids with a row stride wider than the row; the sentinels around every destination survive"""
    rng = np.random.default_rng(13)
    h, w = 2 * S + 3, T + 37
    sparent = R.random_frame(rng, h + 4, w + 70, 0.45)
    a = np.ascontiguousarray(sparent[2:2 + h, 7:7 + w])                                    # an odd byte offset: the rows are not dword-aligned
    wn, want = R.label(a, conn, R.order_of(conn, ccl))
    wst, wce = R.stats(want, wn)
    sp = dev(sparent)
    for dt, tdt in ((np.int32, torch.int32), (np.uint16, torch.uint16)):
        lparent = full16((h + 5, w + 30), 77) if dt == np.uint16 else torch.full((h + 5, w + 30), 77, dtype=tdt, device="cuda")
        stp = torch.full((wn + 2, 8), -9, dtype=torch.int32, device="cuda")
        cep = torch.full((wn + 2, 5), -9.0, dtype=torch.float64, device="cuda")
        lview, stv, cev = lparent[3:3 + h, 11:11 + w], stp[1:1 + wn, 2:7], cep[1:1 + wn, 1:3]
        n, lab, st, ce = run(cv, sp[2:2 + h, 7:7 + w], conn, ccl, dt, labels=lview, stats=stv, centroids=cev)
        assert n == wn and np.array_equal(lab, want) and R.same_stats(st, ce, wst, wce)
        got = lparent.cpu().view(torch.int16 if dt == np.uint16 else torch.int32).numpy()
        keep = np.ones(got.shape, bool); keep[3:3 + h, 11:11 + w] = False
        assert np.all(got[keep] == 77) and np.array_equal(got[3:3 + h, 11:11 + w].astype(np.int64) & 0xFFFFFFFF, want)
        gs, gc = stp.cpu().numpy(), cep.cpu().numpy()
        ks = np.ones(gs.shape, bool); ks[1:1 + wn, 2:7] = False
        kc = np.ones(gc.shape, bool); kc[1:1 + wn, 1:3] = False
        assert np.all(gs[ks] == -9) and np.all(gc[kc] == -9.0)


def test_largest_dimension(cv):
    top = cv.limit(R.LIMIT_KEY)
    assert top == R.MAX_DIM
    rng = np.random.default_rng(7)
    a = R.random_frame(rng, 2, top, 0.5)
    a[:, -3:] = 1
    check(cv, a, modes=MODES[1:])
    check(cv, np.ascontiguousarray(a.T), modes=MODES[:2])                                  # the largest height: 1024 strips
    for shape in ((2, top + 1), (top + 1, 2)):                                             # one past the bound is refused
        n0 = cv._lib.decline_count("connectedComponents")
        with pytest.raises(NotImplementedError):
            cv.connectedComponents(dev(np.zeros(shape, np.uint8)))
        assert cv._lib.decline_count("connectedComponents") == n0 + 1


def test_host_resident_image_is_staged(cv):
    rng = np.random.default_rng(14)
    a = R.random_frame(rng, 2 * S + 5, T + 70, 0.5)
    for conn, ccl in MODES:
        for dt in (np.int32, np.uint16):
            n, lab, st, ce = run(cv, a, conn, ccl, dt)
            assert all(isinstance(t, np.ndarray) for t in (lab, st, ce)) and lab.dtype == dt
            wn, want = R.label(a, conn, R.order_of(conn, ccl))
            assert n == wn and np.array_equal(lab, want) and R.same_stats(st, ce, *R.stats(want, wn))


def batch_frames():
    rng = np.random.default_rng(15)
    h, w = 2 * S + 3, T + 44
    return np.stack([R.random_frame(rng, h, w, 0.45), np.zeros((h, w), np.uint8), np.full((h, w), 200, np.uint8)])


@pytest.mark.parametrize("conn,ccl", MODES)
@pytest.mark.parametrize("dt", [np.int32, np.uint16])
def test_batch_many_none_and_all_foreground(cv, conn, ccl, dt):
    frames = batch_frames()
    n0, s0 = cv.call_count("connectedComponentsBatch"), cv.call_count("connectedComponentsStatsBatch")
    counts, lab, st, ce = cv.connectedComponentsWithStatsBatch(dev(frames), connectivity=conn, ltype=lt_of(cv, dt), ccltype=ccl)
    assert cv.call_count("connectedComponentsBatch") == n0 + 1 and cv.call_count("connectedComponentsStatsBatch") == s0 + 1
    assert last_kernel(cv).startswith("k_ccl_stats<"), last_kernel(cv)
    lab, st, ce = lab.cpu().numpy(), st.cpu().numpy(), ce.cpu().numpy()
    mx = max(counts)
    assert lab.dtype == dt and st.shape == (3, mx, 5) and ce.shape == (3, mx, 2) and counts[1] == 1 and counts[2] == 2 and counts[0] == mx > 2
    for i in range(3):
        wn, want = R.label(frames[i], conn, R.order_of(conn, ccl))
        assert counts[i] == wn and np.array_equal(lab[i], want), i
        assert R.same_stats(st[i, :wn], ce[i, :wn], *R.stats(want, wn)), i
        assert not st[i, wn:].any() and not ce[i, wn:].any()                               # zero-filled above the frame's N
    c2, l2 = cv.connectedComponentsBatch(dev(frames), connectivity=conn, ltype=lt_of(cv, dt), ccltype=ccl)
    assert last_kernel(cv).startswith(kernel_name(conn, ccl, dt)), last_kernel(cv)
    assert c2 == counts and np.array_equal(l2.cpu().numpy(), lab)


def test_host_resident_batch(cv):
    frames = batch_frames()
    pinned = torch.from_numpy(frames).pin_memory()
    n0 = cv.call_count("connectedComponentsBatch")
    counts, lab = cv.connectedComponentsBatch(pinned, connectivity=8)
    assert cv.call_count("connectedComponentsBatch") > n0 and not lab.is_cuda
    assert last_kernel(cv).startswith(kernel_name(8, R.CCL_DEFAULT, np.int32)), last_kernel(cv)
    for i in range(3):
        wn, want = R.label(frames[i], 8, R.BLOCK)
        assert counts[i] == wn and np.array_equal(lab[i].numpy(), want), i
    # the statistics of a host-resident batch are declined
    L = cv._lib.lib
    mx = max(counts)
    st = torch.full((3, mx, 5), 7, dtype=torch.int32).pin_memory()
    ce = torch.full((3, mx, 2), 7.0, dtype=torch.float64).pin_memory()
    arr = (ctypes.c_int * 3)(*counts)
    s0 = cv.call_count("connectedComponentsStatsBatch")
    rc = L.mi355cv_connectedComponentsStatsBatch(ctypes.c_void_p(lab.data_ptr()), lab.stride(1) * 4, lab.stride(0) * 4, lab.shape[2], lab.shape[1], cv.CV_32S, 3, arr, mx,
                                                ctypes.c_void_p(st.data_ptr()), 20, mx * 20, ctypes.c_void_p(ce.data_ptr()), 16, mx * 16)
    assert rc == 1 and "device-resident" in L.mi355cv_lastError().decode() and cv.call_count("connectedComponentsStatsBatch") == s0
    assert bool((st == 7).all()) and bool((ce == 7.0).all())
    with pytest.raises(NotImplementedError):
        cv.connectedComponentsWithStatsBatch(pinned)


def test_stats_skip_values_that_are_no_label(cv):
    """a hand-made label image holding a value >= nlabels: ignored, the other rows right, nothing written past row nlabels - 1"""
    rng = np.random.default_rng(16)
    h, w = S + 3, T + 5
    lab = rng.integers(0, 6, (h, w)).astype(np.int32)
    lab[3, 5:90] = 1000000; lab[7, 0] = 6; lab[h - 1, w - 1] = 2 ** 31 - 1; lab[0, 64] = -1
    L = cv._lib.lib
    for dt, tdt, lt in ((np.int32, torch.int32, cv.CV_32S), (np.uint16, torch.uint16, cv.CV_16U)):
        src = lab.astype(dt)
        d = dev(src)
        st = torch.full((9, 5), -9, dtype=torch.int32, device="cuda")
        ce = torch.full((9, 2), -9.0, dtype=torch.float64, device="cuda")
        s0 = cv.call_count("connectedComponentsStats")
        cv.core.bind_stream(cv.core.Img(d))
        rc = L.mi355cv_connectedComponentsStats(ctypes.c_void_p(d.data_ptr()), w * src.itemsize, w, h, lt, 6, ctypes.c_void_p(st.data_ptr()), 20, ctypes.c_void_p(ce.data_ptr()), 16)
        torch.cuda.synchronize()
        assert rc == 0 and cv.call_count("connectedComponentsStats") == s0 + 1
        gs, gc = st.cpu().numpy(), ce.cpu().numpy()
        assert R.same_stats(gs[:6], gc[:6], *R.stats(src.astype(np.int64), 6))
        assert np.all(gs[6:] == -9) and np.all(gc[6:] == -9.0)
        # centroids may be null
        st2 = torch.full((6, 5), -9, dtype=torch.int32, device="cuda")
        assert L.mi355cv_connectedComponentsStats(ctypes.c_void_p(d.data_ptr()), w * src.itemsize, w, h, lt, 6, ctypes.c_void_p(st2.data_ptr()), 20, None, 0) == 0
        torch.cuda.synchronize()
        assert np.array_equal(st2.cpu().numpy(), gs[:6])


def test_declines_leave_the_destinations_alone(cv):
    a = dev(np.ones((16, 16), np.uint8))
    dst = torch.full((16, 16), 7, dtype=torch.int32, device="cuda")
    calls = cv.call_count("connectedComponents")

    def declined(fn, entry="connectedComponents"):
        n0 = cv._lib.decline_count(entry)
        with pytest.raises(NotImplementedError):
            fn()
        assert cv._lib.decline_count(entry) == n0 + 1

    declined(lambda: cv.connectedComponents(a, labels=dst, ccltype=6))
    declined(lambda: cv.connectedComponents(a, labels=dst, ccltype=-2))
    declined(lambda: cv.connectedComponentsBatch(a[None], labels=dst[None], ccltype=9), "connectedComponentsBatch")
    # source and labels that overlap in HBM
    buf = torch.ones(16 * 16 * 4, dtype=torch.uint8, device="cuda")
    before = buf.clone()
    declined(lambda: cv.connectedComponents(buf[:256].view(16, 16), labels=buf.view(torch.int32).view(16, 16)))
    declined(lambda: cv.connectedComponents(buf[256:512].view(16, 16), labels=buf[:512].view(torch.uint16).view(16, 16), ltype=cv.CV_16U))
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    assert bool((dst == 7).all()) and cv.call_count("connectedComponents") == calls
