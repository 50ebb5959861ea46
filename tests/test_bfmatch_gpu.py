"""cv::BFMatcher on the GPU (opencv_amd/csrc/bfmatch.hip) against tests/bfmatch_restate.py bit for bit -- indices, counts and distances -- across the tile and the split of
the fast Hamming kernel, the generic kernel's row lengths and layouts, masks, collections, the float norms, crossCheck, radiusMatch and the batch entries; every refusal is
derived from mi355cv_limit and checks the recorded reason.  The last test does not rest on the restatement: ORB on two shifted crops, matched on the device."""
import ctypes

import numpy as np
import pytest
import torch

import bfmatch_restate as R
import opencv_amd as cv
from opencv_amd import _lib

pytestmark = pytest.mark.gpu
L = _lib.lib
TILE, SPLIT = _lib.limit("bfmatch_tile_rows"), _lib.limit("bfmatch_split_rows")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def last_kernel():
    return L.mi355cv_lastKernel().decode()


def reason():
    return L.mi355cv_lastError().decode()


def lists_of(res):
    """what BFMatcher returned, as a list of record arrays per query: numpy results are that already; device results are (plane, counts), whose padding is checked here"""
    if not isinstance(res, tuple):
        return res
    out, cnt = cv.dmatch_records(res[0]), res[1].cpu().numpy()
    if out.ndim == 1:
        out = out[:, None]
    for i, c in enumerate(cnt):
        assert (out[i, c:] == R.PAD).all(), (i, c, out[i])
    return [out[i, :c] for i, c in enumerate(cnt)]


def want_lists(plane_cnt):
    out, cnt = plane_cnt
    return [out[i, :c] for i, c in enumerate(cnt)]


def check(got, want, what=""):
    got = lists_of(got)
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, i, g, w)


@pytest.mark.parametrize("nbytes,k", [(32, 1), (32, 2), (64, 1), (64, 2)])
def test_fast_hamming_kernel_across_tile_and_split(nbytes, k):
    """lane counts around a wavefront and a workgroup x train rows around the LDS tile (T) and around a part of the split train set (S): nq <= 257 cannot fill the chip,
    so from S + 1 rows on k_bf_merge joins more than one partial list"""
    rng = np.random.default_rng(nbytes + k)
    Q, T = R.tie_heavy(rng, 257, nbytes), R.tie_heavy(rng, 2 * SPLIT + 3, nbytes)
    dQ, dT = dev(Q), dev(T)
    bf = cv.BFMatcher(cv.NORM_HAMMING)
    for nt in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, SPLIT - 1, SPLIT + 1, 2 * SPLIT + 3):
        full = R.knn_np(Q, [T[:nt]], None, R.NORM_HAMMING, k)
        for nq in (1, 63, 64, 65, 257):
            check(bf.knnMatch(dQ[:nq], dT[:nt], k=k), want_lists((full[0][:nq], full[1][:nq])), (nq, nt))
            lk = last_kernel()
            assert "k_bf_hamming<%d,%d>" % (nbytes // 4, k) in lk, lk
            parts = int(lk.split("grid=")[1].split(" ")[0].split("x")[1])
            assert parts == -(-nt // SPLIT), (nt, lk)


def test_list_edges_and_ties():
    rng = np.random.default_rng(3)
    kmax = _lib.limit("bfmatch_max_k")
    Q, T = R.tie_heavy(rng, 70, 32), R.tie_heavy(rng, SPLIT + 40, 32)
    bf = cv.BFMatcher(cv.NORM_HAMMING)
    for k in (3, 4, 5, kmax):
        check(bf.knnMatch(dev(Q), dev(T), k=k), want_lists(R.knn_np(Q, [T], None, R.NORM_HAMMING, k)), k)
    for nt in (3, kmax - 1):                                                           # k > nt: shorter lists
        got = lists_of(bf.knnMatch(dev(Q), dev(T[:nt]), k=kmax))
        check(got, want_lists(R.knn_np(Q, [T[:nt]], None, R.NORM_HAMMING, kmax)))
        assert all(len(g) == nt for g in got)
    # one row repeated: every distance of a query ties, the order is the train index alone -- across tiles and parts
    same = np.repeat(T[:1], 2 * SPLIT + 5, axis=0)
    got = lists_of(bf.knnMatch(dev(Q), dev(same), k=kmax))
    check(got, want_lists(R.knn_np(Q, [same], None, R.NORM_HAMMING, kmax)))
    assert all(g["trainIdx"].tolist() == list(range(kmax)) for g in got)
    with pytest.raises(NotImplementedError, match="BFMATCH_MAX_K"):
        bf.knnMatch(dev(Q), dev(T), k=kmax + 1)


@pytest.mark.parametrize("norm", [cv.NORM_HAMMING, cv.NORM_HAMMING2])
def test_row_lengths_steps_and_misaligned_bases(norm):
    rng = np.random.default_rng(norm)
    bf = cv.BFMatcher(norm)
    for nbytes in (1, 31, 32, 33, 61, 64, 65):
        Q, T = R.tie_heavy(rng, 67, nbytes), R.tie_heavy(rng, TILE + 9, nbytes)
        want = want_lists(R.knn_np(Q, [T], None, norm, 3))
        check(bf.knnMatch(dev(Q), dev(T), k=3), want, nbytes)
        fast = norm == cv.NORM_HAMMING and nbytes in (32, 64)
        assert ("k_bf_hamming" if fast else "k_bf_generic") in last_kernel(), (nbytes, last_kernel())
        check(bf.knnMatch(Q, T, k=3), want, nbytes)                                    # numpy: staged through HBM
        # row step > row size: views of wider matrices (step 4-aligned for the 32 / 64-byte rows: still the fast kernel)
        wq, wt = np.zeros((67, nbytes + 12), np.uint8), np.zeros((TILE + 9, nbytes + 20), np.uint8)
        wq[:, 4:4 + nbytes], wt[:, 8:8 + nbytes] = Q, T
        dq, dt = dev(wq), dev(wt)
        check(bf.knnMatch(dq[:, 4:4 + nbytes], dt[:, 8:8 + nbytes], k=3), want, nbytes)
        assert ("k_bf_hamming" if fast else "k_bf_generic") in last_kernel()
        check(bf.knnMatch(wq[:, 4:4 + nbytes], wt[:, 8:8 + nbytes], k=3), want, nbytes)
        # the base address off by one byte: the generic kernel, and still right
        check(bf.knnMatch(dq[:, 5:5 + nbytes], dt[:, 8:8 + nbytes], k=3), want_lists(R.knn_np(wq[:, 5:5 + nbytes], [T], None, norm, 3)), nbytes)
        assert "k_bf_generic" in last_kernel(), (nbytes, last_kernel())
        flat = dev(np.concatenate([[0], T.ravel()]).astype(np.uint8))
        check(bf.knnMatch(dev(Q), flat[1:].view(TILE + 9, nbytes), k=3), want, nbytes)
        assert "k_bf_generic" in last_kernel(), (nbytes, last_kernel())


def test_guarded_outputs():
    """the bytes around the match plane and the counts stay as they were (device buffers, both kernels' paths)"""
    rng = np.random.default_rng(5)
    for nbytes, nq, nt, k in ((32, 65, TILE + 1, 2), (33, 65, 40, 3), (32, 5, 2, 4)):
        Q, T = R.tie_heavy(rng, nq, nbytes), R.tie_heavy(rng, nt, nbytes)
        dq, dt = dev(Q), dev(T)
        G = 64
        out = torch.full((G + nq * k * 4 + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        cnt = torch.full((G + nq + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        tp, ts, tr = (ctypes.c_void_p * 1)(dt.data_ptr()), (ctypes.c_size_t * 1)(nbytes), (ctypes.c_int * 1)(nt)
        L.mi355cv_resetStream()
        assert L.mi355cv_bfKnnMatch(dq.data_ptr(), nbytes, nq, nbytes, 0, tp, ts, tr, None, None, 1, 6, k, 0, out.data_ptr() + 4 * G, cnt.data_ptr() + 4 * G) == 0, reason()
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
        for g in (o[:G], o[-G:], c[:G], c[-G:]):
            assert (g == 0x5A5A5A5A).all()
        want, wc = R.knn_np(Q, [T], None, R.NORM_HAMMING, k)
        assert o[G:-G].tobytes() == want.tobytes() and np.array_equal(c[G:-G], wc)


def test_masks_collections_and_compact_result():
    rng = np.random.default_rng(6)
    Q = R.tie_heavy(rng, 40, 32)
    trains = [R.tie_heavy(rng, n, 32) for n in (30, 1, 50)]
    trains[2][:10] = trains[0][:10]                                                    # rows duplicated across images
    trains[1][0] = trains[0][3]
    masks = [rng.integers(0, 2, (40, len(t)), dtype=np.uint8) for t in trains]
    masks[0][7] = 0; masks[1][7] = 0; masks[2][7] = 0                                  # query 7 has no candidate at all
    masks[0][:, 4] = 0                                                                 # an all-zero column
    masks[0][9] = 0; masks[1][9] = 0; masks[2][9] = 0; masks[2][9, 17] = 200           # one single non-zero
    for norm in (cv.NORM_HAMMING, cv.NORM_HAMMING2):
        bf = cv.BFMatcher(norm)
        bf.add(trains)
        for ms in (None, masks, [masks[0], None, masks[2]]):
            want = R.knn_np(Q, trains, ms, norm, 4)
            check(bf.knnMatch(Q, k=4, masks=ms), want_lists(want), "numpy")
            dms = None if ms is None else [None if m is None else dev(m) for m in ms]
            d = cv.BFMatcher(norm)
            d.add([dev(t) for t in trains])
            check(d.knnMatch(dev(Q), 4, masks=dms), want_lists(want), "device")
            assert "k_bf_generic" in last_kernel()
        want = R.knn_np(Q, trains, masks, norm, 4)
        assert want[1][7] == 0 and want[1][9] == 1 and want[0]["imgIdx"][9, 0] == 2 and want[0]["trainIdx"][9, 0] == 17
        full, compact = bf.knnMatch(Q, k=4, masks=masks), bf.knnMatch(Q, k=4, masks=masks, compactResult=True)
        assert len(full) == 40 and len(full[7]) == 0 and len(compact) == int((want[1] > 0).sum()) < 40
        check(compact, [w for w in want_lists(want) if len(w)])
        m = bf.match(Q, masks=masks)                                                   # knnMatch(1) flattened: query 7 does not appear
        w1 = R.knn_np(Q, trains, masks, norm, 1)
        assert m.tobytes() == w1[0][w1[1] > 0, 0].tobytes() and 7 not in m["queryIdx"]
        # one train matrix with a mask, with a pitched mask view
        wide = np.zeros((40, 64), np.uint8); wide[:, 3:33] = masks[0]
        check(bf.knnMatch(Q, trains[0], k=2, mask=wide[:, 3:33]), want_lists(R.knn_np(Q, [trains[0]], [masks[0]], norm, 2)))
        check(bf.knnMatch(dev(Q), dev(trains[0]), k=2, mask=dev(wide)[:, 3:33]), want_lists(R.knn_np(Q, [trains[0]], [masks[0]], norm, 2)))


@pytest.mark.parametrize("norm", [cv.NORM_L1, cv.NORM_L2, cv.NORM_L2SQR])
def test_float_norms(norm):
    rng = np.random.default_rng(norm)
    bf = cv.BFMatcher(norm)
    for length in (1, 4, 128, 130):
        Q, T = R.tie_heavy_float(rng, 66, length), R.tie_heavy_float(rng, SPLIT + 7, length)
        Q[1] = rng.standard_normal(length).astype(np.float32) * 100                   # sums that round at every step
        T[2] = rng.standard_normal(length).astype(np.float32) * 100
        T[5, 0] = np.nan                                                               # a row that is nobody's candidate
        if length >= 4:
            # squared distances 2^24 and 2^24 + 2 from query 0, both with the root 4096: NORM_L2 ties where NORM_L2SQR does not
            Q[0] = 0
            T[9] = 0; T[9, 2] = 4096
            T[8] = 0; T[8, 0] = 1; T[8, 1] = 1; T[8, 2] = 4096
            d2, d = R.distances_np(Q[:1], T[8:10], R.NORM_L2SQR)[0], R.distances_np(Q[:1], T[8:10], R.NORM_L2)[0]
            assert d2[0] == 2.0 ** 24 + 2 and d2[1] == 2.0 ** 24 and d[0] == d[1] == 4096
        want = R.knn_np(Q, [T], None, norm, 3)
        assert not (want[0]["trainIdx"] == 5).any()
        check(bf.knnMatch(dev(Q), dev(T), k=3), want_lists(want), length)
        assert "k_bf_generic" in last_kernel()
        check(bf.knnMatch(Q, T, k=3), want_lists(want), length)
        far = R.knn_np(Q[:1], [T[8:10]], None, norm, 2) if length >= 4 else None
        if far is not None:
            check(bf.knnMatch(dev(Q[:1]), dev(T[8:10]), k=2), want_lists(far), length)
            assert far[0]["trainIdx"][0].tolist() == ([0, 1] if norm == cv.NORM_L2 else [1, 0])
    c = cv.BFMatcher(norm, crossCheck=True)
    Q, T = R.tie_heavy_float(rng, 50, 4), R.tie_heavy_float(rng, 60, 4)
    check(c.knnMatch(dev(Q), dev(T), k=1), want_lists(R.cross_np(Q, T, norm)))


def test_cross_check():
    rng = np.random.default_rng(8)
    for nbytes in (32, 64, 33):
        Q, T = R.tie_heavy(rng, 300, nbytes), R.tie_heavy(rng, SPLIT + 70, nbytes)
        T[:20] = Q[:20]; T[40:50] = Q[5]; Q[100:110] = T[30]                           # duplicates on both sides
        want = R.cross_np(Q, T, R.NORM_HAMMING)
        assert 0 < want[1].sum() < len(Q)
        bf = cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True)
        check(bf.knnMatch(dev(Q), dev(T), k=1), want_lists(want), nbytes)
        m = bf.match(Q, T)
        assert m.tobytes() == want[0][want[1] > 0, 0].tobytes()
        dm, dc = bf.match(dev(Q), dev(T))
        assert cv.dmatch_records(dm)[dc.cpu().numpy() > 0].tobytes() == m.tobytes()


def test_radius_match():
    rng = np.random.default_rng(9)
    top = _lib.limit("bfmatch_max_radius_row")
    for norm, Q, trains in ((cv.NORM_HAMMING, R.tie_heavy(rng, 70, 32), [R.tie_heavy(rng, 90, 32), R.tie_heavy(rng, 33, 32)]),
                            (cv.NORM_L2, R.tie_heavy_float(rng, 70, 5), [R.tie_heavy_float(rng, 90, 5)])):
        D = R.distances_np(Q, trains[0], norm)
        bf = cv.BFMatcher(norm)
        bf.add(trains)
        db = cv.BFMatcher(norm)
        db.add([dev(t) for t in trains])
        for md in (float(np.sort(D.ravel())[D.size // 3]), 0.0, -1.0, float(D.max())):   # an occurring distance; zero; below every distance; everything of image 0
            want = R.radius_np(Q, trains, None, norm, md)
            check(bf.radiusMatch(Q, md), want, md)
            flat, cnt = db.radiusMatch(dev(Q), maxDistance=md)
            assert np.array_equal(cnt.cpu().numpy(), [len(w) for w in want])
            assert cv.dmatch_records(flat).tobytes() == (np.concatenate(want).tobytes() if len(flat) else b"")
        assert sum(len(w) for w in R.radius_np(Q, trains, None, norm, float(D.max()))) > max(4 * len(Q), 1024)      # the Python mirror's first capacity was too small
        mask = rng.integers(0, 2, (70, 90), dtype=np.uint8)
        md = float(np.median(D))
        check(cv.BFMatcher(norm).radiusMatch(Q, trains[0], md, mask=mask), R.radius_np(Q, trains[:1], [mask], norm, md))
        full = cv.BFMatcher(norm).radiusMatch(Q, trains[0], 0.0)
        assert len(cv.BFMatcher(norm).radiusMatch(Q, trains[0], 0.0, compactResult=True)) == sum(1 for f in full if len(f)) < len(full) or all(len(f) for f in full)
    # the capacity retry of the C entry: the total is returned, the first `cap` records are written, the rest of the buffer is not touched
    Q, T = R.tie_heavy(rng, 20, 32), R.tie_heavy(rng, 50, 32)
    want = np.concatenate(R.radius_np(Q, [T], None, R.NORM_HAMMING, 300.0))
    assert len(want) == 1000
    tp, ts, tr = (ctypes.c_void_p * 1)(T.ctypes.data), (ctypes.c_size_t * 1)(32), (ctypes.c_int * 1)(50)
    out, cnt = np.full(1100, R.PAD, R.DMATCH), np.zeros(20, np.int32)
    L.mi355cv_resetStream()
    assert L.mi355cv_bfRadiusMatch(Q.ctypes.data, 32, 20, 32, 0, tp, ts, tr, None, None, 1, 6, 300.0, out.ctypes.data, 130, cnt.ctypes.data) == 1000
    assert out[:130].tobytes() == want[:130].tobytes() and (out[130:] == R.PAD).all() and (cnt == 50).all()
    assert L.mi355cv_bfRadiusMatch(Q.ctypes.data, 32, 20, 32, 0, tp, ts, tr, None, None, 1, 6, 300.0, out.ctypes.data, 1100, cnt.ctypes.data) == 1000
    assert out[:1000].tobytes() == want.tobytes() and (out[1000:] == R.PAD).all()
    # a query's list AT the bound is sorted in LDS; one row more and the call is declined
    row = R.tie_heavy(rng, 1, 32)
    T = np.repeat(row, top + 1, axis=0)
    got = cv.BFMatcher(cv.NORM_HAMMING).radiusMatch(dev(row), dev(T[:top]), 0.0)
    assert got[1].cpu().tolist() == [top] and cv.dmatch_records(got[0])["trainIdx"].tolist() == list(range(top))
    Tm = T[:top].copy(); Tm[1::2, 0] ^= 1                                               # odd rows at distance 1: the sort has work to do
    got = cv.BFMatcher(cv.NORM_HAMMING).radiusMatch(row, Tm, 1.0)
    check(got, R.radius_np(row, [Tm], None, R.NORM_HAMMING, 1.0))
    with pytest.raises(NotImplementedError, match="BFMATCH_MAX_RADIUS_ROW"):
        cv.BFMatcher(cv.NORM_HAMMING).radiusMatch(dev(row), dev(T), 0.0)


def test_batches_equal_single_calls():
    rng = np.random.default_rng(10)
    for nbytes, norm in ((32, cv.NORM_HAMMING), (64, cv.NORM_HAMMING), (33, cv.NORM_HAMMING2)):
        sizes = [(70, SPLIT + 5), (0, 40), (300, 0), (257, TILE + 1)]
        Qs = [R.tie_heavy(rng, nq, nbytes) for nq, _ in sizes]
        Ts = [R.tie_heavy(rng, nt, nbytes) for _, nt in sizes]
        for cross in (False, True):
            bf = cv.BFMatcher(norm, crossCheck=cross)
            for k in ((1,) if cross else (1, 3)):
                want = [want_lists(R.cross_np(q, t, norm) if cross else R.knn_np(q, [t], None, norm, k)) for q, t in zip(Qs, Ts)]
                got_d = bf.knnMatchBatch([dev(q) for q in Qs], [dev(t) for t in Ts], k)
                lk = last_kernel()
                assert ("k_bf_hamming" if nbytes != 33 else "k_bf_generic") in lk and "x%d x256" % len(sizes) in lk, lk      # one launch sequence: the pairs are the grid's z
                for b in range(len(sizes)):                                            # (reading the device results also ends the device call: the host call below
                    check(got_d[b], want[b], (nbytes, cross, k, b))                    # runs on the library's own stream, which nothing orders against torch's)
                got_h = bf.knnMatchBatch(Qs, Ts, k)
                for b in range(len(sizes)):
                    check(got_h[b], want[b], (nbytes, cross, k, b))
                    if sizes[b][0] and sizes[b][1]:
                        check(bf.knnMatch(dev(Qs[b]), dev(Ts[b]), k=k), want[b])
                    assert all(len(w) == 0 for w in want[b]) or (sizes[b][0] and sizes[b][1])
        flat = cv.BFMatcher(norm).matchBatch(Qs, Ts)
        for b, (q, t) in enumerate(zip(Qs, Ts)):
            w = R.knn_np(q, [t], None, norm, 1)
            assert flat[b].tobytes() == w[0][w[1] > 0, 0].tobytes()
        # empty sides through the single entries
        assert cv.BFMatcher(norm).knnMatch(Qs[1], Ts[1], k=2) == [] and all(len(m) == 0 for m in cv.BFMatcher(norm).knnMatch(Qs[2], Ts[2], k=2))


def test_device_and_host_placements_agree():
    rng = np.random.default_rng(11)
    Q, T = R.tie_heavy(rng, 130, 32), R.tie_heavy(rng, 2 * SPLIT + 1, 32)
    bf = cv.BFMatcher(cv.NORM_HAMMING)
    staged0 = int(L.mi355cv_stagedBytes())
    d = bf.knnMatch(dev(Q), dev(T), k=2)
    assert int(L.mi355cv_stagedBytes()) == staged0                                     # device in, device out: nothing crossed PCIe through the stager
    assert d[0].is_cuda and d[1].is_cuda and d[0].shape == (130, 2, 4) and d[0].dtype == torch.int32
    want = want_lists(R.knn_np(Q, [T], None, R.NORM_HAMMING, 2))
    check(d, want)
    h = bf.knnMatch(Q, T, k=2)
    assert int(L.mi355cv_stagedBytes()) > staged0
    mixed = bf.knnMatch(Q, dev(T), k=2)
    check(h, want); check(mixed, want)


def test_declines_and_errors():
    rng = np.random.default_rng(12)
    q8, t8 = dev(R.tie_heavy(rng, 10, 32)), dev(R.tie_heavy(rng, 12, 32))
    qf, tf = dev(R.tie_heavy_float(rng, 10, 8)), dev(R.tie_heavy_float(rng, 12, 8))
    n0 = _lib.decline_count("bfKnnMatch")
    cases = [
        (lambda: cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True).match(q8, t8, mask=torch.ones((10, 12), dtype=torch.uint8, device="cuda")), "crossCheck together with a mask"),
        (lambda: cv.BFMatcher(cv.NORM_HAMMING).match(qf, tf), "CV_32F descriptors are served with NORM_L1"),
        (lambda: cv.BFMatcher(cv.NORM_HAMMING2).match(qf, tf), "CV_32F descriptors are served with NORM_L1"),
        (lambda: cv.BFMatcher(cv.NORM_L2).match(q8, t8), "CV_8U descriptors are served with NORM_HAMMING"),
        (lambda: cv.BFMatcher().match(q8, t8), "CV_8U descriptors are served with NORM_HAMMING"),
        (lambda: cv.BFMatcher(cv.NORM_L1).match(dev(np.zeros((4, 8), np.int16)), dev(np.zeros((4, 8), np.int16))), "neither CV_8UC1 nor CV_32FC1"),
        (lambda: cv.BFMatcher(cv.NORM_HAMMING).knnMatch(q8, t8, k=_lib.limit("bfmatch_max_k") + 1), "BFMATCH_MAX_K"),
        (lambda: cv.BFMatcher(cv.NORM_HAMMING).match(torch.zeros((2, _lib.limit("bfmatch_max_row_bytes") + 1), dtype=torch.uint8, device="cuda"),
                                                     torch.zeros((2, _lib.limit("bfmatch_max_row_bytes") + 1), dtype=torch.uint8, device="cuda")), "BFMATCH_MAX_ROW_BYTES"),
        (lambda: cv.BFMatcher(cv.NORM_L2).match(torch.zeros((2, _lib.limit("bfmatch_max_row_bytes") // 4 + 1), device="cuda"),
                                                torch.zeros((2, _lib.limit("bfmatch_max_row_bytes") // 4 + 1), device="cuda")), "BFMATCH_MAX_ROW_BYTES"),
        (lambda: cv.BFMatcher(cv.NORM_HAMMING).match(torch.zeros((_lib.limit("bfmatch_max_rows") + 1, 1), dtype=torch.uint8, device="cuda"), t8[:, :1]), "BFMATCH_MAX_ROWS"),
        (lambda: cv.BFMatcher(cv.NORM_HAMMING).match(q8[:, :1], torch.zeros((_lib.limit("bfmatch_max_rows") + 1, 1), dtype=torch.uint8, device="cuda")), "BFMATCH_MAX_ROWS"),
    ]
    two = cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True)
    two.add([t8, t8])
    cases.append((lambda: two.match(q8), "crossCheck with more than one train matrix"))
    many = cv.BFMatcher(cv.NORM_HAMMING)
    many.add([t8] * (_lib.limit("bfmatch_max_images") + 1))
    cases.append((lambda: many.match(q8), "BFMATCH_MAX_IMAGES"))
    for call, why in cases:
        with pytest.raises(NotImplementedError, match=why):
            call()
        assert why in reason()
    assert _lib.decline_count("bfKnnMatch") == n0 + len(cases)
    with pytest.raises(ValueError, match="k = 1"):
        cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True).knnMatch(q8, t8, k=2)
    with pytest.raises(NotImplementedError, match="crossCheck with radiusMatch"):
        cv.BFMatcher(cv.NORM_HAMMING, crossCheck=True).radiusMatch(q8, t8, 3.0)
    # parity AT the bounds: the longest row, the largest collection
    top = _lib.limit("bfmatch_max_row_bytes")
    Q, T = R.tie_heavy(rng, 5, top), R.tie_heavy(rng, 9, top)
    check(cv.BFMatcher(cv.NORM_HAMMING).knnMatch(dev(Q), dev(T), k=2), want_lists(R.knn_np(Q, [T], None, R.NORM_HAMMING, 2)))
    Qf, Tf = R.tie_heavy_float(rng, 5, top // 4), R.tie_heavy_float(rng, 9, top // 4)
    check(cv.BFMatcher(cv.NORM_L2).knnMatch(dev(Qf), dev(Tf), k=2), want_lists(R.knn_np(Qf, [Tf], None, R.NORM_L2, 2)))
    trains = [R.tie_heavy(rng, 1 + i % 3, 32) for i in range(_lib.limit("bfmatch_max_images"))]
    full = cv.BFMatcher(cv.NORM_HAMMING)
    full.add([dev(t) for t in trains])
    check(full.knnMatch(q8, 3), want_lists(R.knn_np(q8.cpu().numpy(), trains, None, R.NORM_HAMMING, 3)))


def test_orb_to_matcher_end_to_end():
    """does not rest on the restatement: two 256 x 256 crops of one random-texture image, offset by a known (dx, dy); ORB(nlevels = 1) on each, crossCheck matching on
    the device; the most frequent keypoint displacement over the matches is exactly (dx, dy) and at least one match has distance 0"""
    rng = np.random.default_rng(13)
    big = np.kron(rng.integers(0, 256, (64, 64)).astype(np.uint8), np.ones((6, 6), np.uint8))
    big = np.clip(big.astype(np.int32) + rng.integers(-6, 7, big.shape), 0, 255).astype(np.uint8)
    dx, dy = 11, 7
    a, b = np.ascontiguousarray(big[40:296, 50:306]), np.ascontiguousarray(big[40 + dy:296 + dy, 50 + dx:306 + dx])
    orb = cv.ORB(nfeatures=500, nlevels=1)
    ka, da = orb.detectAndCompute(dev(a))
    kb, db = orb.detectAndCompute(dev(b))
    assert len(ka) > 50 and len(kb) > 50 and da.shape[1] == 32
    m, c = cv.BFMatcher(orb.defaultNorm(), crossCheck=True).match(dev(da), dev(db))
    assert m.is_cuda and "k_bf_hamming<8,1>" in last_kernel()
    m = cv.dmatch_records(m)[c.cpu().numpy() > 0]
    assert len(m) > 20
    disp = np.stack([ka["x"][m["queryIdx"]] - kb["x"][m["trainIdx"]], ka["y"][m["queryIdx"]] - kb["y"][m["trainIdx"]]], axis=1)
    vals, counts = np.unique(disp, axis=0, return_counts=True)
    assert tuple(vals[np.argmax(counts)]) == (dx, dy), (vals[np.argmax(counts)], counts.max(), len(m))
    assert (m["distance"] == 0).any()
