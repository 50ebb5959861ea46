"""cv::StereoBM without a GPU: the two forms of the restatement (tests/stereobm_restate.py) against each other bit for bit, known answers worked out by hand, the lines
of opencv_amd/csrc/stereobm_math.h compiled for the host (tests/hostemu/stereobm_emu.cpp) against the restatement stage by stage, the refusals of the mi355cv_stereo*
entries that come before any device is touched, the limits and the layout of mi355cv_StereoBMParams."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import emubuild
import stereobm_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, minDisparity, numDisparities, blockSize, textureThreshold, uniquenessRatio, disp12MaxDiff, shift)
GRID = [(9, 30, 0, 16, 5, 10, 15, -1, 3), (7, 29, 4, 16, 7, 0, 0, 1, 9), (8, 40, -8, 32, 5, 3, 40, 0, -2), (6, 26, -21, 16, 5, 5, 10, 2, -12),
        (5, 24, 0, 16, 5, 10, 15, 1, 15), (1 + 4, 21, 10, 16, 5, 10, 15, -1, 12)]


def params(m, n, w, tex, uniq, lr, c=31):
    return R.Params(minDisparity=m, numDisparities=n, blockSize=w, preFilterCap=c, textureThreshold=tex, uniquenessRatio=uniq, disp12MaxDiff=lr)


@pytest.mark.parametrize("case", GRID)
def test_the_two_forms_of_the_restatement_agree(case):
    H, W, m, n, w, tex, uniq, lr, s = case
    rng = np.random.default_rng(abs(hash(case)) % 1000)
    p = params(m, n, w, tex, uniq, lr)
    for L, Rr in (R.tie_heavy(rng, H, W, 3, s), R.smooth_pair(rng, H, W, s)):
        for c in (1, 31, 63):
            assert np.array_equal(R.prefilter_loops(L, c), R.prefilter_np(L, c))
        PL, PR = R.prefilter_np(L, p.c), R.prefilter_np(Rr, p.c)
        (Sa, Ta), (Sb, Tb) = R.volumes_loops(PL, PR, p), R.volumes_np(PL, PR, p)
        assert np.array_equal(Sa, Sb) and np.array_equal(Ta, Tb)
        da, db = R.decision_loops(Sa, Ta, p), R.decision_np(Sb, Tb, p)
        for a, b in zip(da, db):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        for mx in (lr, 0, 3):
            q = params(m, n, w, tex, uniq, mx)
            assert np.array_equal(R.leftright_loops(da[0], da[1], q), R.leftright_np(da[0], da[1], q))
        assert np.array_equal(R.compute_loops(L, Rr, p), R.compute_np(L, Rr, p))
    one = np.full((1, 12), 7, np.uint8)
    one[0, 5:] = 90
    assert np.array_equal(R.prefilter_loops(one, 31), R.prefilter_np(one, 31))                # H == 1: the row is its own neighbour


def test_known_answers():
    flat = np.full((30, 100), 77, np.uint8)
    d = R.compute_np(flat, flat, R.Params())
    assert d.dtype == np.int16 and (d == -16).all()                                           # prefiltered: cap everywhere, T = 0 < 10
    # no texture test, no uniqueness test: all SADs are 0, the tie goes to i = 0 (D = Dmax), p = nn = SAD_1 = 0, dd = 0, q = 0: (Dmax * 256 + 15) >> 4 = 16 Dmax
    small = np.full((8, 40), 5, np.uint8)
    for m in (0, 4, -3):
        p = params(m, 16, 5, 0, 0, -1)
        for f in (R.compute_np, R.compute_loops):
            d = f(small, small, p)
            xlo, xhi, _, _ = R.valid_columns(40, p)
            assert (d[:, xlo:xhi] == p.Dmax * 16).all() and (d[:, :xlo] == p.filtered).all() and (d[:, xhi:] == p.filtered).all()
    # sub-pixel with a negative quotient: ms = 0 at i = 5 (D = 10 of Dmax = 15), p = SAD_6 = 13, nn = SAD_4 = 51: dd = 13 + 51 - 0 + 38 = 102,
    # (13 - 51) * 256 / 102 = -95.37: toward zero -95 (floor would give -96); (2560 - 95 + 15) >> 4 = 2480 >> 4 = 155 exactly (floor: 2479 >> 4 = 154; without + 15: 154)
    p = params(0, 16, 5, 10, 15, -1)
    sad = np.full(16, 1000, np.int64)
    sad[4], sad[5], sad[6] = 51, 0, 13
    assert R.decide_pixel(sad, 500, p)[:3] == (155, 0, R.KEPT)
    S, T = np.zeros((1, 20, 16), np.int64), np.zeros((1, 20), np.int64)
    S[0, 17], T[0, 17] = sad, 500
    assert R.decision_np(S, T, p)[0][0, 17] == 155
    assert R.decide_pixel(sad, 9, p)[0] == -16 and R.decide_pixel(sad, 10, p)[0] == 155       # T < textureThreshold is strict
    # thresh: 107 + 107 * 15 / 100 = 107 + 16 = 123 (integer division); a SAD of 123 outside [mi - 1, mi + 1] rejects, 124 does not, 123 next to the winner does not
    for v, i, want in ((123, 9, R.UNIQUENESS_REJECT), (124, 9, R.KEPT), (123, 6, R.KEPT), (123, 4, R.KEPT), (123, 7, R.UNIQUENESS_REJECT)):
        sad = np.full(16, 1000, np.int64)
        sad[5], sad[i] = 107, v
        assert R.decide_pixel(sad, 500, p)[2] == want, (v, i)
        S[0, 17] = sad
        assert R.decision_np(S, T, p)[2][0, 17] == want
    # left-right: x = 3 (d = 16) and x = 4 (d = 32) both vote for column 2.  Equal costs: x = 3 wins, d2[2] = 16, so x = 4 sees |16 - 32| = 16 > 0 and goes;
    # a smaller cost at x = 4 turns it round
    p0 = params(0, 16, 5, 10, 15, 0)
    d = np.full((1, 8), -16, np.int16)
    d[0, 3], d[0, 4] = 16, 32
    cost = np.zeros((1, 8), np.int64)
    cost[0, 3] = cost[0, 4] = 5
    for f in (R.leftright_loops, R.leftright_np):
        assert f(d, cost, p0)[0].tolist() == [-16, -16, -16, 16, -16, -16, -16, -16]
        c2 = cost.copy(); c2[0, 4] = 4
        assert f(d, c2, p0)[0].tolist() == [-16, -16, -16, -16, 32, -16, -16, -16]
        assert f(d, cost, params(0, 16, 5, 10, 15, 1))[0].tolist() == d[0].tolist()           # |16 - 32| = 16 > 16 is false
        assert f(d, cost, params(0, 16, 5, 10, 15, -1))[0].tolist() == d[0].tolist()


def test_the_smooth_pairs_meet_the_conditions_of_the_gpu_test_on_the_cpu():
    """the test of tests/test_stereobm_gpu.py that does not rest on the restatement, run on the restatement itself"""
    for m, s in ((0, 5), (0, 15), (4, 9), (-8, -3), (-20, -12)):
        L, Rr = R.smooth_pair(np.random.default_rng(100 + s), 40, 96, s)
        p = R.Params(minDisparity=m, numDisparities=16, blockSize=9)
        R.check_shift_recovered(R.compute_np(L, Rr, p), p, s)


@functools.lru_cache(maxsize=1)
def emu():
    lib = emubuild.load("stereobm_emu.cpp", "libstereobm_emu.so")
    i32, vp = ctypes.c_int, ctypes.c_void_p
    lib.emu_sbm_geom.argtypes = [i32, i32, i32, vp]
    lib.emu_sbm_prefilter.argtypes = [vp, i32, i32, i32, vp]
    lib.emu_sbm_volumes.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.emu_sbm_decide.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.emu_sbm_leftright.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.emu_sbm_subpixel.argtypes = [i32] * 5
    return lib


@pytest.mark.parametrize("case", GRID)
def test_stereobm_math_on_the_host_matches_the_restatement(case):
    E = emu()
    H, W, m, n, w, tex, uniq, lr, s = case
    rng = np.random.default_rng(7 + abs(hash(case)) % 1000)
    p = params(m, n, w, tex, uniq, lr)
    g = np.zeros(6, np.int32)
    E.emu_sbm_geom(W, m, n, g.ctypes.data)
    assert tuple(g[:4]) == R.valid_columns(W, p) and (g[4], g[5]) == (p.Dmax, p.filtered)
    for L, Rr in (R.tie_heavy(rng, H, W, 3, s), R.smooth_pair(rng, H, W, s)):
        L, Rr = np.ascontiguousarray(L), np.ascontiguousarray(Rr)
        PL, PR = np.empty_like(L), np.empty_like(Rr)
        for c in (1, 63, p.c):
            E.emu_sbm_prefilter(L.ctypes.data, W, H, c, PL.ctypes.data)
            assert np.array_equal(PL, R.prefilter_np(L, c)), c
        E.emu_sbm_prefilter(Rr.ctypes.data, W, H, p.c, PR.ctypes.data)
        S, T = R.volumes_np(PL, PR, p)
        sad, tt = np.zeros((H, W, n), np.int32), np.zeros((H, W), np.int32)
        E.emu_sbm_volumes(PL.ctypes.data, PR.ctypes.data, W, H, m, n, w, p.c, sad.ctypes.data, tt.ctypes.data)
        assert np.array_equal(sad, S) and np.array_equal(tt, T)
        want = R.decision_np(S, T, p)
        for chunked in (0, 1):
            d, win = np.zeros((H, W), np.int16), np.zeros((H, W), np.int32)
            E.emu_sbm_decide(sad.ctypes.data, tt.ctypes.data, W, H, m, n, tex, uniq, chunked, d.ctypes.data, win.ctypes.data)
            assert np.array_equal(d, want[0]), chunked
            kept = want[2] == R.KEPT
            assert np.array_equal(win[kept], want[1][kept]), chunked
        cost = np.ascontiguousarray(want[1].astype(np.int32))
        for mx in (0, 1, 3):
            q = params(m, n, w, tex, uniq, mx)
            for stride in (1, 5, 7):
                if np.gcd(stride, W) != 1:
                    continue
                out = np.zeros((H, W), np.int16)
                E.emu_sbm_leftright(want[0].ctypes.data, cost.ctypes.data, W, H, m, n, mx, stride, out.ctypes.data)
                assert np.array_equal(out, R.leftright_np(want[0], want[1], q)), (mx, stride)
    assert E.emu_sbm_subpixel(0, 13, 51, 15, 5) == 155


LIMITS = {"stereobm_max_dim": 16384, "stereobm_max_disparities": 256, "stereobm_max_block": 51, "stereobm_roll_max_block": 21, "stereobm_chunk": 16,
          "stereobm_tile_cols": 64, "stereobm_strip_rows": 32, "stereobm_generic_tile_cols": 32}


def test_limits_are_pinned():
    """how far StereoBM was built; tests/test_stereobm_gpu.py derives its shapes and every refusal it asserts from mi355cv_limit.  The issue's floors: 256 disparities, blocks of 51"""
    from opencv_amd import _lib
    E = emu()
    for i, (k, v) in enumerate(LIMITS.items()):
        assert _lib.limit(k) == v == E.emu_sbm_limit(i), k
    assert LIMITS["stereobm_max_disparities"] >= 256 and LIMITS["stereobm_max_block"] >= 51 and LIMITS["stereobm_max_dim"] == 16384


def test_refusals_before_a_device_is_touched():
    import opencv_amd as cv
    from opencv_amd import _lib
    from opencv_amd.calib3d import StereoBMParams
    Lb, NI, top = _lib.lib, _lib.NOT_IMPLEMENTED, _lib.limit
    reason = lambda: Lb.mi355cv_lastError().decode()
    img = np.zeros((64, 96), np.uint8)
    out = np.full((64, 96), 1234, np.int16)

    def call(W=96, H=64, depth=3, lstep=96, rstep=96, dstep=192, batch=None, **kw):
        P = StereoBMParams()
        Lb.mi355cv_stereoBMDefaults(ctypes.byref(P))
        P.numDisparities, P.blockSize = 16, 9
        for k, v in kw.items():
            setattr(P, k, (ctypes.c_int * 4)(*v) if k.startswith("roi") else v)
        if batch is not None:
            return Lb.mi355cv_stereoBMBatch(img.ctypes.data, lstep, 64 * 96, img.ctypes.data, rstep, 64 * 96, out.ctypes.data, dstep, 64 * 192, batch, W, H, depth, ctypes.byref(P))
        return Lb.mi355cv_stereoBM(img.ctypes.data, lstep, img.ctypes.data, rstep, out.ctypes.data, dstep, W, H, depth, ctypes.byref(P))

    cases = [
        (dict(preFilterType=cv.PREFILTER_NORMALIZED_RESPONSE), "PREFILTER_NORMALIZED_RESPONSE is not served"),
        (dict(speckleWindowSize=1), "cv::filterSpeckles is not served"),
        (dict(roi1=(0, 0, 96, 64)), "ROI-based validity is not served"), (dict(roi2=(1, 1, 9, 9)), "ROI-based validity is not served"),
        (dict(depth=2), "neither CV_16SC1 nor CV_32FC1"), (dict(depth=4), "neither CV_16SC1 nor CV_32FC1"),
        (dict(numDisparities=24), "n % 16 != 0"), (dict(numDisparities=top("stereobm_max_disparities") + 16), "STEREOBM_MAX_DISPARITIES"),
        (dict(blockSize=8), "w % 2 == 0"), (dict(blockSize=3), "w < 5"), (dict(blockSize=top("stereobm_max_block") + 2, W=96, H=64), "STEREOBM_MAX_BLOCK"),
        (dict(blockSize=21, H=19), "std::min(width, height)"),
        (dict(preFilterCap=0), "preFilterCap < 1"), (dict(preFilterCap=64), "preFilterCap > 63"),
        (dict(textureThreshold=-1), "textureThreshold < 0"), (dict(uniquenessRatio=-1), "uniquenessRatio < 0"),
        (dict(W=top("stereobm_max_dim") + 1, lstep=1 << 15, rstep=1 << 15, dstep=1 << 16), "STEREOBM_MAX_DIM"),
        (dict(H=top("stereobm_max_dim") + 1), "STEREOBM_MAX_DIM"),
        (dict(minDisparity=-2048), "range of a CV_16S map"), (dict(minDisparity=2040), "range of a CV_16S map"),
        (dict(lstep=95), "lstep < (size_t)W"), (dict(rstep=95), "rstep < (size_t)W"), (dict(dstep=190), "dstep < (size_t)W * esz"),
        (dict(depth=5, dstep=192), "dstep < (size_t)W * esz"), (dict(dstep=193), "off their element's boundary"),
        (dict(batch=0), "nframes < 1"), (dict(batch=-3), "nframes < 1"), (dict(batch=2, lstep=95), "left_step < (size_t)width"),
    ]
    for kw, why in cases:
        assert call(**kw) == NI, kw
        assert why in reason(), (kw, reason())
    assert (out == 1234).all()
    assert Lb.mi355cv_stereoPrefilterXSobel(img.ctypes.data, 96, out.ctypes.data, 96, 96, 64, 0) == NI and "cap < 1" in reason()
    assert Lb.mi355cv_stereoPrefilterXSobel(img.ctypes.data, 95, out.ctypes.data, 96, 96, 64, 31) == NI and "src_step < (size_t)width" in reason()
    assert Lb.mi355cv_stereoBMSetKernel(1) == -1 and Lb.mi355cv_stereoBMSetKernel(0) == 0 and Lb.mi355cv_stereoBMSetKernel(-1) == 0
    # the Python mirror: the reference's getters and setters, and its own argument errors
    bm = cv.StereoBM_create()                                                                 # numDisparities = 0 is kept as given; compute takes it for 64
    assert (bm.getNumDisparities(), bm.getBlockSize(), bm.getMinDisparity(), bm.getPreFilterType(), bm.getPreFilterSize(), bm.getPreFilterCap(), bm.getTextureThreshold(),
            bm.getUniquenessRatio(), bm.getSpeckleWindowSize(), bm.getSpeckleRange(), bm.getDisp12MaxDiff()) == (0, 21, 0, cv.PREFILTER_XSOBEL, 9, 31, 10, 15, 0, 0, -1)
    bm = cv.StereoBM_create(32, 9)
    bm.setMinDisparity(-4); bm.setDisp12MaxDiff(2); bm.setUniquenessRatio(0)
    assert (bm.getNumDisparities(), bm.getBlockSize(), bm.getMinDisparity(), bm.getDisp12MaxDiff(), bm.getUniquenessRatio()) == (32, 9, -4, 2, 0)
    assert (cv.StereoBM_DISP_SHIFT, cv.StereoBM_DISP_SCALE, cv.PREFILTER_NORMALIZED_RESPONSE, cv.PREFILTER_XSOBEL) == (4, 16, 0, 1)
    with pytest.raises(NotImplementedError, match="inputs must be CV_8UC1"):
        bm.compute(np.zeros((64, 96), np.uint16), np.zeros((64, 96), np.uint16))
    with pytest.raises(NotImplementedError, match="neither CV_16SC1 nor CV_32FC1"):
        bm.compute(img, img, disp=np.zeros((64, 96), np.int32))
    with pytest.raises(ValueError, match="same size"):
        bm.compute(img, img[:, :90])
    with pytest.raises(ValueError, match="shape of the inputs"):
        bm.compute(img, img, disp=np.zeros((64, 90), np.int16))


def test_params_layout(tmp_path):
    """mi355cv_StereoBMParams as a C compiler lays it out from include/mi355cv.h against the ctypes mirror"""
    from opencv_amd.calib3d import StereoBMParams
    names = [f for f, _ in StereoBMParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355cv.h"\nint main(void) { printf("%zu", sizeof(mi355cv_StereoBMParams));\n'
                   + "".join('printf(" %%zu", offsetof(mi355cv_StereoBMParams, %s));\n' % n for n in names) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(StereoBMParams)] + [getattr(StereoBMParams, n).offset for n in names]
    assert got[0] == 19 * 4 and names[:3] == ["minDisparity", "numDisparities", "blockSize"]
