"""cv::StereoSGBM on the GPU (opencv_amd/csrc/sgbm.hip) against tests/sgbm_restate.py bit for bit, under both arms of the path aggregation (the fast kernel and the
forced plain one): every lane packing of the fast kernel, a single valid column, a single row, widths and heights around the cost kernel's tile and strip and around the
fast kernel's block of steps, block sizes, minimum disparities, the three modes, penalties, uniqueness, the left-right check, the speckle filter, CV_32F maps, pitched
misaligned views with guarded destinations, batches (chunked by a lowered scratch bound too), numpy and device inputs.  The last test does not rest on the
restatement: a smooth image and its shifted copy."""
import contextlib

import numpy as np
import pytest
import torch

import sgbm_restate as R
import speckle_restate as SP
import viewcheck as vc
import opencv_amd as cv
from opencv_amd import _lib
from viewtable import Device

pytestmark = pytest.mark.gpu
Lb = _lib.lib
TILE, STRIP, PBLOCK, NMAX = (_lib.limit("sgbm_" + k) for k in ("tile_cols", "strip_rows", "path_block", "max_disparities"))
MODES = (R.MODE_SGBM, R.MODE_HH, R.MODE_HH4)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def last_kernel():
    return Lb.mi355cv_lastKernel().decode()


def matcher(p):
    return cv.StereoSGBM_create(*p)


def same(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])


@contextlib.contextmanager
def forced(arm):
    assert Lb.mi355cv_stereoSGBMSetKernel(arm) == 0
    try:
        yield
    finally:
        Lb.mi355cv_stereoSGBMSetKernel(-1)


@contextlib.contextmanager
def scratch_limit(nbytes):
    assert Lb.mi355cv_stereoSGBMSetScratchLimit(nbytes) == 0
    try:
        yield
    finally:
        Lb.mi355cv_stereoSGBMSetScratchLimit(0)


def expected(L, Rr, p):
    want = R.compute_np(L, Rr, p)
    if p.speckleWindowSize > 0:
        want = SP.filter_np(want, *R.speckle_args(p))
    return want


def both_arms(p, L, Rr, what=""):
    """device compute under the built-in rule, with the plain kernel forced and with the fast one forced: all equal the restatement; returns the map"""
    want = expected(L, Rr, p)
    sg, dL, dR = matcher(p), dev(L), dev(Rr)
    xlo, xhi = R.valid_columns(L.shape[1], p)
    for arm, name in ((-1, "k_sgbm_path_fast"), (0, "k_sgbm_path_plain"), (1, "k_sgbm_path_fast")):
        with forced(arm):
            same(sg.compute(dL, dR), want, (what, arm))
            served = last_kernel()
            assert ("k_sgbm_fill" if xhi <= xlo else name) in served, (what, arm, served)
    return want


def inputs(seed, H, W, s=3):
    """random bytes, a constant image, a smoothed shifted pair"""
    rng = np.random.default_rng(seed)
    return R.random_pair(rng, H, W), R.constant_pair(H, W), R.smooth_pair(rng, H, W, s)


@pytest.mark.parametrize("n", [16, 32, 48, 64, 96, 128, 192, NMAX])
def test_disparities(n):
    """16 / 32: several paths per wave; 64: a value per lane; 128 / 256: two and four values per lane; 48, 96, 192: lanes of the wave beyond the range"""
    H, W = 12, n - 1 + 1 + 21
    for i, (L, Rr) in enumerate(inputs(n, H, W)):
        want = both_arms(R.Params(0, n, 3, 8, 32, 1, 31, 0), L, Rr, (n, i))
        assert (want[:, n - 1:] != -16).any()
    with pytest.raises(NotImplementedError, match="SGBM_MAX_DISPARITIES"):
        cv.StereoSGBM_create(0, NMAX + 16, 3).compute(dev(L), dev(Rr))


def test_a_single_valid_column_a_single_row_and_none():
    rng = np.random.default_rng(1)
    for n in (16, 64, NMAX):
        for mode in MODES:
            L, Rr = R.random_pair(rng, 9, n)                                                    # W = Dmax + 1: W1 = 1
            both_arms(R.Params(0, n, 3, 8, 32, 1, 31, 10, mode=mode), L, Rr, ("W1 = 1", n, mode))
            L, Rr = R.random_pair(rng, 1, n + 30)                                               # H = 1
            both_arms(R.Params(0, n, 5, 8, 32, 1, 31, 10, mode=mode), L, Rr, ("H = 1", n, mode))
        L, Rr = R.random_pair(rng, 1, n)
        both_arms(R.Params(0, n, 1, 8, 32, 1, 31, 10), L, Rr, ("1 x 1", n))
    L, Rr = R.random_pair(rng, 6, 40)
    for m in (40, -60, 25):                                                                     # no valid column: the whole map is FILTERED
        p = R.Params(m, 16, 3)
        assert (both_arms(p, L, Rr, ("empty", m)) == p.filtered).all()
        assert "no valid column" in last_kernel()


@pytest.mark.parametrize("w", [3, 5])
def test_tile_and_strip_edges(w):
    """valid widths around the pixels a workgroup of the cost kernel produces and around two of them, heights around its strip of rows"""
    n, tw = 16, TILE - (w - 1)
    rng = np.random.default_rng(w)
    for W1 in (tw - 1, tw, tw + 1, 2 * tw, 2 * tw + 1):
        for H in (STRIP - 1, STRIP, STRIP + 1):
            L, Rr = R.random_pair(rng, H, W1 + n - 1)
            both_arms(R.Params(0, n, w, 8, 32, 1, 31, 10, mode=R.MODE_HH), L, Rr, (W1, H))
            assert "k_sgbm_cost grid=%dx%dx1 " % (-(-W1 // tw), -(-H // STRIP)) in last_kernel(), last_kernel()


@pytest.mark.parametrize("n", [16, 64, 128, NMAX])
def test_path_block_edges(n):
    """path lengths around the block of steps whose loads the fast kernel has in flight (16 up to 64 disparities, 8 up to 128, 4 above), and around two blocks"""
    blk = PBLOCK if n <= 64 else PBLOCK // 2 if n <= 128 else PBLOCK // 4
    rng = np.random.default_rng(n)
    for length in (blk - 1, blk, blk + 1, 2 * blk - 1, 2 * blk, 2 * blk + 1):
        L, Rr = R.random_pair(rng, length, length + n - 1)                                      # W1 = H = length: rows, columns and the main diagonals have it
        both_arms(R.Params(0, n, 3, 8, 32, 1, 31, 10, mode=R.MODE_HH), L, Rr, (n, length))
        L, Rr = R.random_pair(rng, length, 3 * blk + n + 2)
        both_arms(R.Params(0, n, 3, 8, 32, 1, 31, 10, mode=R.MODE_HH), L, Rr, (n, length, "wide"))


@pytest.mark.parametrize("w", [1, 3, 5, 9])
def test_block_sizes(w):
    for i, (L, Rr) in enumerate(inputs(w, 14, 50)):
        for cap in (0, 63):
            both_arms(R.Params(0, 16, w, 8, 32, 1, cap, 10), L, Rr, (w, i, cap))
    with pytest.raises(NotImplementedError, match="SGBM_MAX_COST"):
        cv.StereoSGBM_create(0, 16, 19).compute(dev(L), dev(Rr))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", [0, 4, -8, -20])
def test_min_disparities_and_modes(m, mode):
    for i, (L, Rr) in enumerate(inputs(100 + m, 13, 61, s=m + 6)):
        want = both_arms(R.Params(m, 16, 3, 8, 32, 1, 31, 10, mode=mode), L, Rr, (m, mode, i))
        if i == 2:
            assert (want != (m - 1) * 16).any()


def test_penalties():
    """P1 = P2 = 0 as given, and P2 so large that M + P2 never wins: then its value does not matter, which the restatement shows before the device is asked"""
    (L, Rr), _, (Ls, Rs) = inputs(7, 12, 48)
    for mode in MODES:
        both_arms(R.Params(0, 16, 3, 0, 0, 1, 31, 10, mode=mode), L, Rr, ("zero", mode))
        both_arms(R.Params(-3, 32, 3, 0, 0, 1, 31, 0, mode=mode), Ls, Rs, ("zero, smooth", mode))
        for a, b in ((L, Rr), (Ls, Rs)):
            big, bigger = R.Params(0, 16, 3, 5, 20000, 1, 31, 10, mode=mode), R.Params(0, 16, 3, 5, 30000, 1, 31, 10, mode=mode)
            sa, sb = {}, {}
            R.compute_np(a, b, big, sa); R.compute_np(a, b, bigger, sb)
            assert np.array_equal(sa["S"], sb["S"])
            both_arms(big, a, b, ("large P2", mode))
        both_arms(R.Params(0, 16, 3, 7, 7, 1, 31, 10, mode=mode), L, Rr, ("P1 = P2", mode))
    with pytest.raises(NotImplementedError, match="P2 < p->P1"):
        cv.StereoSGBM_create(0, 16, 3, 9, 8).compute(dev(L), dev(Rr))


@pytest.mark.parametrize("uniq", [0, 10])
@pytest.mark.parametrize("lr", [-1, 0, 2])
def test_uniqueness_and_the_left_right_check(uniq, lr):
    for i, (L, Rr) in enumerate(inputs(uniq + lr + 5, 14, 70, s=5)):
        p = R.Params(-4, 32, 3, 8, 32, lr, 31, uniq)
        st = {}
        R.compute_np(L, Rr, p, st)
        want = both_arms(p, L, Rr, (uniq, lr, i))
        if i == 0:                                                                              # from the restatement alone: the inputs reach both rejects
            xlo, xhi = R.valid_columns(70, p)
            assert (uniq == 0) == st["kept"].all()
            assert (st["kept"] & (want[:, xlo:xhi] == p.filtered)).any(), "the left-right check rejects something"


@pytest.mark.parametrize("spw", [0, 20])
def test_speckles(spw):
    """the served filterSpeckles on the CV_16S map, against the restatement followed by tests/speckle_restate.py"""
    for i, (L, Rr) in enumerate(inputs(spw, 20, 300 if spw else 80, s=4)):                      # 300: past one tile of the speckle kernel
        p = R.Params(0, 16, 3, 8, 32, 1, 31, 5, spw, 2)
        raw = R.compute_np(L, Rr, p)
        want = both_arms(p, L, Rr, (spw, i))
        if spw and i == 0:
            assert (raw != want).any() and (want != p.filtered).any(), "the filter erases something and keeps something"
            assert "mi355cv_filterSpecklesBatch" in last_kernel()
        same(matcher(p).compute(dev(L), dev(Rr), disptype=cv.CV_32F), R.to_float(want), (spw, i, "32F"))


def test_float_maps():
    for i, (L, Rr) in enumerate(inputs(3, 11, 47)):
        for m in (0, -8):
            p = R.Params(m, 16, 3, 8, 32, 1, 31, 10)
            want = R.compute_np(L, Rr, p)
            for arm in (-1, 0):
                with forced(arm):
                    f = matcher(p).compute(dev(L), dev(Rr), disptype=cv.CV_32F)
                    assert f.dtype == torch.float32
                    same(f, R.to_float(want), (i, m, arm))
            assert np.array_equal(f.cpu().numpy() * 16, want.astype(np.float32))


@pytest.mark.parametrize("device", [Device, vc.Host], ids=["device", "host"])
@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_pitched_views_at_misaligned_origins(layout, device):
    """both inputs and the map as views of wider parents at the layout's offsets and pitches; the map's parent is guarded, the inputs' parents are hostile"""
    rng = np.random.default_rng(5)
    H, W = 21, 83
    L, Rr = R.random_pair(rng, H, W)
    for p, depth in ((R.Params(-12, 16, 5, 8, 32, 1, 31, 10, mode=R.MODE_HH), cv.CV_16S), (R.Params(0, 32, 3, 8, 32, 1, 31, 0, 20, 2), cv.CV_16S),
                     (R.Params(3, 64, 3, 4, 40, 2, 0, 5), cv.CV_32F)):
        want = expected(L, Rr, p)
        want = want if depth == cv.CV_16S else R.to_float(want)
        for arm in (-1, 0):
            with forced(arm):
                def call(lv, dv, rv):
                    assert matcher(p).compute(lv, rv, disp=dv) is dv
                name, _ = vc.run(call, layout, L, want, what="%s %s arm %d" % (layout, p, arm), device=device, kernel_name=last_kernel, inputs=(Rr,))
                assert ("k_sgbm_path_fast" if arm else "k_sgbm_path_plain") in name, name


@pytest.mark.parametrize("nframes", [1, 3, 17])
def test_batches_equal_single_calls(nframes):
    rng = np.random.default_rng(nframes)
    H, W = 13, 70
    pairs = [R.smooth_pair(rng, H, W, 2 + f % 4) if f % 2 else R.random_pair(rng, H, W) for f in range(nframes)]
    for p in (R.Params(-3, 16, 3, 8, 32, 1, 31, 10, mode=R.MODE_HH), R.Params(0, 32, 5, 8, 32, 1, 31, 10, 20, 2)):
        sg = matcher(p)
        want = np.stack([expected(a, b, p) for a, b in pairs])
        for torch_side in (True, False):
            # frames one row down, three columns in, inside parents that are taller and wider: non-trivial steps and frame strides larger than the frame
            Lp, Rp = np.zeros((nframes, H + 3, W + 9), np.uint8), np.zeros((nframes, H + 2, W + 4), np.uint8)
            Dp = np.full((nframes, H + 2, W + 6), -777, np.int16)
            for f, (a, b) in enumerate(pairs):
                Lp[f, 1:H + 1, 3:3 + W], Rp[f, 1:H + 1, 3:3 + W] = a, b
            if torch_side:
                Lp, Rp, Dp = dev(Lp), dev(Rp), dev(Dp)
            lv, rv, dv = Lp[:, 1:H + 1, 3:3 + W], Rp[:, 1:H + 1, 3:3 + W], Dp[:, 1:H + 1, 3:3 + W]
            out = sg.computeBatch(lv, rv, disp=dv)
            assert out is dv
            same(dv, want, torch_side)
            assert "k_sgbm_path_fast" in last_kernel() and "x%d " % nframes in last_kernel() and "%d frame(s) per chunk" % nframes in last_kernel(), last_kernel()
            with forced(0):
                same(sg.computeBatch(lv, rv), want, ("forced plain", torch_side))
                assert "k_sgbm_path_plain" in last_kernel(), last_kernel()
            d = Dp.cpu().numpy() if torch_side else Dp
            g = np.ones(d.shape, bool)
            g[:, 1:H + 1, 3:3 + W] = False
            assert (d[g] == -777).all()
            for f in (0, nframes - 1):
                same(sg.compute(lv[f], rv[f]), want[f], f)
            same(sg.computeBatch(lv, rv, disptype=cv.CV_32F), R.to_float(want))
            same(sg.computeBatch([lv[f] for f in range(nframes)], [rv[f] for f in range(nframes)]), want)
            # a scratch bound that holds two frames: the batch runs in chunks of two, with identical maps; one that holds none declines
            per = (W - max(p.Dmax, 0) + min(p.m, 0)) * H * p.n * 6 + W * H * 16 + 32 * H + 4096
            with scratch_limit(2 * per + per // 2):
                same(sg.computeBatch(lv, rv), want, ("chunks of two", torch_side))
                assert "%d frame(s) per chunk" % min(2, nframes) in last_kernel(), last_kernel()
            with scratch_limit(per - 1):
                with pytest.raises(NotImplementedError, match="SGBM_MAX_SCRATCH_BYTES"):
                    sg.computeBatch(lv, rv)


def test_numpy_in_numpy_out_and_device_refusals():
    (L, Rr), _, _ = inputs(9, 12, 50)
    p = R.Params(0, 16, 3, 8, 32, 1, 31, 10)
    want = R.compute_np(L, Rr, p)
    got = matcher(p).compute(L, Rr)
    assert isinstance(got, np.ndarray)
    same(got, want)
    gf = matcher(p).compute(L, Rr, disptype=cv.CV_32F)
    assert isinstance(gf, np.ndarray)
    same(gf, R.to_float(want))
    got = matcher(p).compute(dev(L), dev(Rr))
    assert isinstance(got, torch.Tensor) and got.is_cuda
    # a disparity map inside an input's buffer
    H, W = 20, 64
    buf = torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")
    other = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    disp = buf.view(torch.int16)[:, :W]
    for a, b in ((buf[:, :W], other), (other, buf[:, :W])):
        with pytest.raises(NotImplementedError, match="overlaps an input"):
            cv.StereoSGBM_create(0, 16, 3).compute(a, b, disp=disp)
    assert (buf == 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,s", [(0, 5), (0, 15), (4, 9), (-8, -3), (-20, -12)])
def test_a_known_shift_is_recovered(m, s, mode):
    """does not rest on the restatement: a 3 x 3-box-smoothed random 40 x 96 image and its copy shifted by s; n = 16, w = 5, P1 = 200, P2 = 800, preFilterCap = 63,
    uniquenessRatio = 10, disp12MaxDiff = 1"""
    L, Rr = R.smooth_pair(np.random.default_rng(100 + s), 40, 96, s)
    p = R.Params(m, 16, 5, 200, 800, 1, 63, 10, mode=mode)
    for arm in (-1, 0):
        with forced(arm):
            d = matcher(p).compute(dev(L), dev(Rr)).cpu().numpy()
        assert d.dtype == np.int16
        R.check_shift_recovered(d, p, s)
    f = matcher(p).compute(dev(L), dev(Rr), disptype=cv.CV_32F).cpu().numpy()
    assert f.dtype == np.float32 and np.array_equal(f * 16, d.astype(np.float32))
