"""cv::StereoBM on the GPU (opencv_amd/csrc/stereobm.hip) against tests/stereobm_restate.py bit for bit: across the column tile, the lanes and the row strip of the fast
kernel, the disparity chunks, the block sizes on either side of the generic kernel's threshold, pitched views at misaligned origins with guarded destinations, numpy and
device inputs, CV_16S and CV_32F maps, batches; the forced generic kernel equals the fast one on every fast-path case; mi355cv_lastKernel says which kernel served.  The
last test does not rest on the restatement: a smooth image and its shifted copy."""
import contextlib

import numpy as np
import pytest
import torch

import stereobm_restate as R
import opencv_amd as cv
from opencv_amd import _lib

pytestmark = pytest.mark.gpu
Lb = _lib.lib
CHUNK, TILE, STRIP, GTILE = (_lib.limit("stereobm_" + k) for k in ("chunk", "tile_cols", "strip_rows", "generic_tile_cols"))
ROLL_MAX, BLOCK_MAX, NMAX = _lib.limit("stereobm_roll_max_block"), _lib.limit("stereobm_max_block"), _lib.limit("stereobm_max_disparities")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def last_kernel():
    return Lb.mi355cv_lastKernel().decode()


def matcher(p):
    bm = cv.StereoBM_create(p.n, p.w)
    bm.setMinDisparity(p.m); bm.setPreFilterCap(p.c); bm.setTextureThreshold(p.tex); bm.setUniquenessRatio(p.uniq); bm.setDisp12MaxDiff(p.lr)
    return bm


def params(m=0, n=16, w=9, tex=10, uniq=15, lr=-1, c=31):
    return R.Params(minDisparity=m, numDisparities=n, blockSize=w, preFilterCap=c, textureThreshold=tex, uniquenessRatio=uniq, disp12MaxDiff=lr)


def same(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])


@contextlib.contextmanager
def forced_generic():
    assert Lb.mi355cv_stereoBMSetKernel(0) == 0
    try:
        yield
    finally:
        Lb.mi355cv_stereoBMSetKernel(-1)


def both_kernels(p, L, Rr, what=""):
    """device compute under the built-in rule and with the generic kernel forced: both equal the restatement; returns the map and what the rule launched"""
    want = R.compute_np(L, Rr, p)
    bm, dL, dR = matcher(p), dev(L), dev(Rr)
    xlo, xhi, _, _ = R.valid_columns(L.shape[1], p)
    same(bm.compute(dL, dR), want, what)
    name = "k_sbm_fill" if xhi <= xlo else "k_sbm_cost_roll" if p.w <= ROLL_MAX else "k_sbm_cost_generic"
    served = last_kernel()
    assert name in served, (what, served)
    if name == "k_sbm_cost_roll":
        with forced_generic():
            same(bm.compute(dL, dR), want, ("forced generic", what))
            assert "k_sbm_cost_generic" in last_kernel(), last_kernel()
    return want, served


@pytest.mark.parametrize("w", [5, 9])
def test_tile_and_lane_edges(w):
    """widths around a wavefront of window columns and around the pixels a workgroup produces, heights around the window and past one strip of rows"""
    n, tw = 16, TILE - (w - 1)
    rng = np.random.default_rng(w)
    for W in (n + w, 63 + n, 64 + n, 65 + n, n - 1 + tw - 1, n - 1 + tw, n - 1 + tw + 1, n - 1 + 2 * tw + 3):
        for H in (w, w + 1, 2 * w + 3, STRIP, STRIP + 3):
            L, Rr = R.tie_heavy(rng, H, W, 4, 3)
            _, served = both_kernels(params(n=n, w=w, lr=1), L, Rr, (W, H))
            assert "grid=%dx%dx1 " % (-(-(W - (n - 1)) // tw), -(-H // STRIP)) in served, (W, H, served)


@pytest.mark.parametrize("n", [16, 32, 48, 64, NMAX])
def test_disparities(n):
    """one chunk, several, the limit (a workgroup of 1024 lanes); minimum disparities of either sign, a range wholly left of the image, an empty valid range"""
    rng = np.random.default_rng(n)
    H, W = 11, n + 45
    L, Rr = R.tie_heavy(rng, H, W, 3, 5)
    for m in (0, 4, -8, -(n + 5), W):
        p = params(m=m, n=n, w=5, lr=2 if m == 4 else -1)
        want, served = both_kernels(p, L, Rr, (n, m))
        if m == W:
            assert (want == p.filtered).all() and "no valid column" in served
        elif m in (0, 4, -8):                                                           # the true shift, 5, is inside the range
            assert (want != p.filtered).any(), (n, m)
    with pytest.raises(NotImplementedError, match="STEREOBM_MAX_DISPARITIES"):
        cv.StereoBM_create(NMAX + 16, 5).compute(dev(L), dev(Rr))


@pytest.mark.parametrize("w", [5, 9, ROLL_MAX, ROLL_MAX + 2, BLOCK_MAX])
def test_block_sizes(w):
    """ROLL_MAX + 2 is the first size on the generic kernel, BLOCK_MAX the last one served"""
    rng = np.random.default_rng(w)
    n = 16
    for H, W in ((w, n + w), (w + 4, n + w + GTILE + 5)):
        L, Rr = R.smooth_pair(rng, H, W, 4)
        _, served = both_kernels(params(n=n, w=w, tex=0, lr=1), L, Rr, (w, H, W))
        assert ("k_sbm_cost_roll" if w <= ROLL_MAX else "k_sbm_cost_generic") in served
    if w == BLOCK_MAX:
        L, Rr = R.smooth_pair(rng, w + 2, w + 20, 4)
        with pytest.raises(NotImplementedError, match="STEREOBM_MAX_BLOCK"):
            cv.StereoBM_create(16, w + 2).compute(dev(L), dev(Rr))
        p = params(n=NMAX, w=w, m=-NMAX // 2)                                       # the generic kernel's largest tiles: both limits at once
        L, Rr = R.smooth_pair(rng, w, NMAX + 44, 4)
        both_kernels(p, L, Rr, "both limits")


def guarded(a, off, torch_side, guard):
    """a copy of `a` as a view at column `off`, one row down, of a wider and taller array filled with `guard`: (parent, view)"""
    H, W = a.shape
    parent = np.full((H + 2, W + off + 5), guard, a.dtype)
    parent[1:H + 1, off:off + W] = a
    if torch_side:
        parent = torch.from_numpy(parent).cuda()
    return parent, parent[1:H + 1, off:off + W]


def guards_intact(parent, H, W, off, guard):
    p = parent.cpu().numpy() if isinstance(parent, torch.Tensor) else parent
    m = np.ones(p.shape, bool)
    m[1:H + 1, off:off + W] = False
    return (p[m] == guard).all()


@pytest.mark.parametrize("torch_side", [True, False])
@pytest.mark.parametrize("depth", [cv.CV_16S, cv.CV_32F])
def test_pitched_views_at_misaligned_origins(torch_side, depth):
    rng = np.random.default_rng(5)
    H, W = 24, 90
    L, Rr = R.tie_heavy(rng, H, W, 4, 3)
    for p in (params(m=-12, n=16, w=5, lr=1), params(m=0, n=32, w=ROLL_MAX + 2, tex=0)):
        want = R.compute_np(L, Rr, p)
        want = want if depth == cv.CV_16S else R.to_float(want)
        for offs in ((0, 0, 0), (3, 7, 1), (16, 1, 3)):
            (_, lv), (_, rv) = guarded(L, offs[0], torch_side, 0), guarded(Rr, offs[1], torch_side, 0)
            guard = -999 if depth == cv.CV_16S else np.float32(-999.5)
            dp, dv = guarded(np.zeros((H, W), want.dtype), offs[2], torch_side, guard)
            out = matcher(p).compute(lv, rv, disp=dv)
            assert out is dv
            same(dv, want, (p.w, offs))
            assert guards_intact(dp, H, W, offs[2], guard), offs
            assert ("k_sbm_cost_roll" if p.w <= ROLL_MAX else "k_sbm_cost_generic") in last_kernel()
            with forced_generic():
                same(matcher(p).compute(lv, rv, disptype=depth), want, ("forced generic", p.w, offs))
                assert "k_sbm_cost_generic" in last_kernel()
        got = matcher(p).compute(lv, rv, disptype=depth)                              # allocated: the kind of the input
        assert isinstance(got, torch.Tensor) == torch_side
        same(got, want)


@pytest.mark.parametrize("nframes", [1, 3, 17])
def test_batches_equal_single_calls(nframes):
    rng = np.random.default_rng(nframes)
    H, W = 13, 70
    pairs = [R.tie_heavy(rng, H, W, 3, 2 + f % 4) for f in range(nframes)]
    p = params(m=-3, n=16, w=7, lr=1)
    bm = matcher(p)
    want = np.stack([R.compute_np(a, b, p) for a, b in pairs])
    for torch_side in (True, False):
        # frames one row down, three columns in, inside parents that are taller and wider: non-trivial steps and frame strides
        Lp, Rp = np.zeros((nframes, H + 3, W + 9), np.uint8), np.zeros((nframes, H + 2, W + 4), np.uint8)
        Dp = np.full((nframes, H + 2, W + 6), -777, np.int16)
        for f, (a, b) in enumerate(pairs):
            Lp[f, 1:H + 1, 3:3 + W], Rp[f, 1:H + 1, 3:3 + W] = a, b
        if torch_side:
            Lp, Rp, Dp = dev(Lp), dev(Rp), dev(Dp)
        lv, rv, dv = Lp[:, 1:H + 1, 3:3 + W], Rp[:, 1:H + 1, 3:3 + W], Dp[:, 1:H + 1, 3:3 + W]
        out = bm.computeBatch(lv, rv, disp=dv)
        assert out is dv
        same(dv, want, torch_side)
        assert "k_sbm_cost_roll grid=" in last_kernel() and "x%d " % nframes in last_kernel(), last_kernel()
        with forced_generic():
            same(bm.computeBatch(lv, rv), want, ("forced generic", torch_side))
            assert "k_sbm_cost_generic grid=" in last_kernel() and "x%d " % nframes in last_kernel(), last_kernel()
        d = Dp.cpu().numpy() if torch_side else Dp
        m = np.ones(d.shape, bool)
        m[:, 1:H + 1, 3:3 + W] = False
        assert (d[m] == -777).all()
        for f in (0, nframes - 1):
            same(bm.compute(lv[f], rv[f]), want[f], f)
        same(bm.computeBatch(lv, rv, disptype=cv.CV_32F), R.to_float(want))
        same(bm.computeBatch([lv[f] for f in range(nframes)], [rv[f] for f in range(nframes)]), want)


def test_every_outcome_of_the_decision_and_the_left_right_check():
    L, Rr = R.tie_heavy(np.random.default_rng(5), 24, 90, 4, 3)
    p = params(m=-12, n=16, w=5, tex=10, uniq=15, lr=1)
    before, after, out, tied, dd0 = R.outcomes_np(L, Rr, p)
    # from the restatement alone: the inputs reach every branch
    assert (out == R.TEXTURE_REJECT).any() and (out == R.UNIQUENESS_REJECT).any() and tied.any() and dd0.any()
    assert ((before != p.filtered) & (after == p.filtered)).any()
    same(matcher(p).compute(dev(L), dev(Rr)), after)
    both_kernels(p, L, Rr)
    q = params(m=-12, n=16, w=5, tex=10, uniq=15, lr=-1)
    same(matcher(q).compute(dev(L), dev(Rr)), before)
    for tex, uniq in ((0, 0), (0, 15), (10, 0), (5000, 15), (10, 400)):
        both_kernels(params(m=-12, n=16, w=5, tex=tex, uniq=uniq, lr=0), L, Rr, (tex, uniq))


def test_prefilter_stage_and_device_refusals():
    rng = np.random.default_rng(9)
    for H, W in ((1, 40), (2, 3), (7, 16), (9, 75), (5, 1040)):
        img = rng.integers(0, 256, (H, W)).astype(np.uint8)
        for c in (1, 31, 63):
            want = R.prefilter_np(img, c)
            same(cv.stereoPrefilterXSobel(dev(img), c), want, (H, W, c))
            same(cv.stereoPrefilterXSobel(img, c), want, (H, W, c))
            sp, sv = guarded(img, 5, True, 0)
            dp, dv = guarded(np.zeros_like(img), 2, True, 201)
            cv.stereoPrefilterXSobel(sv, c, dst=dv)
            same(dv, want)
            assert guards_intact(dp, H, W, 2, 201)
    # a disparity map inside an input's buffer
    H, W = 20, 64
    buf = torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")
    other = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    disp = buf.view(torch.int16)[:, :W]
    for a, b in ((buf[:, :W], other), (other, buf[:, :W])):
        with pytest.raises(NotImplementedError, match="overlaps an input"):
            cv.StereoBM_create(16, 5).compute(a, b, disp=disp)
    with pytest.raises(NotImplementedError, match="w > std::min"):
        cv.StereoBM_create(16, 21).compute(other, other)


@pytest.mark.parametrize("m,s", [(0, 5), (0, 15), (4, 9), (-8, -3), (-20, -12)])
def test_a_known_shift_is_recovered(m, s):
    """does not rest on the restatement: a 3 x 3-box-smoothed random 40 x 96 image and its copy shifted by s, defaults except n = 16, w = 9"""
    L, Rr = R.smooth_pair(np.random.default_rng(100 + s), 40, 96, s)
    bm = cv.StereoBM_create(16, 9)
    bm.setMinDisparity(m)
    d = bm.compute(dev(L), dev(Rr)).cpu().numpy()
    assert d.dtype == np.int16 and "k_sbm_cost_roll" in last_kernel()
    R.check_shift_recovered(d, R.Params(minDisparity=m, numDisparities=16, blockSize=9), s)
    f = bm.compute(dev(L), dev(Rr), disptype=cv.CV_32F).cpu().numpy()
    assert f.dtype == np.float32 and np.array_equal(f * 16, d.astype(np.float32))
