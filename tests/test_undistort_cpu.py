"""cv::initUndistortRectifyMap / undistort / reprojectImageTo3D without a GPU: the two forms of the restatement (tests/undistort_restate.py) against each other;
opencv_amd/csrc/undistort_math.h compiled for the host with -ffp-contract=off (tests/hostemu/undistort_emu.cpp) against the restatement stage by stage -- ir, (u, v) as
64-bit patterns, the three map forms, the tile's box, whole small images as k_undist8_tile orders the work, the frame walk of a batch included; identity, shift and
the non-finite pixel verified in numpy; the closed form against the reference's accumulating form; hand-worked answers; the pinned limits; every refusal before a
device is touched; the Python mirror's argument errors and ledger counts."""
import ctypes

import numpy as np
import pytest

import emubuild
import undistort_restate as R

K = np.array(R.K_TEST, np.float64)
ROT = np.array(R.rot_y(0.02), np.float64)
CASES = {
    "lens": dict(K=K, dist=R.LENS, R=ROT, newK=None),
    "barrel": dict(K=K, dist=[-0.6, 0, 0, 0], R=None, newK=None),
    "quarter": dict(K=K, dist=R.LENS, R=None, newK=[[K[0, 0] / 4, 0, K[0, 2]], [0, K[1, 1] / 4, K[1, 2]], [0, 0, 1]]),
    "rational": dict(K=K, dist=[-0.2, 0.05, 0.001, -0.002, 0.01, 0.02, -0.01, 0.003, 0.004, -0.003, 0.002, 0.001], R=ROT, newK=None),
    "plain": dict(K=K, dist=None, R=None, newK=None),
}


@pytest.fixture(scope="module")
def emu():
    E = emubuild.load("undistort_emu.cpp", "libundistort_emu.so", flags=("-ffp-contract=off",))
    E.emu_und_sat.argtypes = [ctypes.c_double]
    E.emu_und_reproject.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    return E


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _cam_args(cam):
    """(ir, k12, cam4) as arrays the emulation takes; keep the tuple alive while the pointers are in use"""
    return np.array(cam["ir"], np.float64), np.array(cam["k"], np.float64), np.array([cam["fx"], cam["fy"], cam["u0"], cam["v0"]], np.float64)


def _cval(value, cn):
    v = (list(np.atleast_1d(np.asarray(value, np.float64)).ravel()) + [0.0] * 4)[:4]                     # a number is cv::Scalar(v) = (v, 0, 0, 0)
    return sum(int(np.clip(np.rint(np.float32(v[k])), 0, 255)) << (8 * k) for k in range(4))


def _emu_tile(emu, case, src, dsize, border=0, value=0, nframes=1, fpw=8, lds=24 << 10, dwords=1, boxes=None):
    cam = R.camera(**CASES[case])
    args = _cam_args(cam)
    frames = src if nframes > 1 else src[None]
    frames = np.ascontiguousarray(frames)
    sh, sw = frames.shape[1:3]
    cn = 1 if frames.ndim == 3 else frames.shape[3]
    out = np.full((frames.shape[0], dsize[1], dsize[0]) + ((cn,) if cn > 1 else ()), 77, np.uint8)
    emu.emu_und_tile(*[_ptr(a) for a in args], _ptr(frames), sw, sh, cn, _ptr(out), dsize[0], dsize[1], frames.shape[0], fpw, lds, border, _cval(value, cn), dwords,
                     None if boxes is None else _ptr(boxes))
    return out if nframes > 1 else out[0]


def _image(seed, h, w, cn):
    return np.random.default_rng(seed).integers(0, 256, (h, w) + ((cn,) if cn > 1 else ()), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_forms_of_the_map_rule_agree(case):
    cam = R.camera(**CASES[case])
    ua, va = R.map_uv(cam, 37, 9)
    ub, vb = R.map_uv_loops(cam, 37, 9)
    assert R.same_floats(ua, ub) and R.same_floats(va, vb)
    for t in (R.CV_32FC1, R.CV_32FC2, R.CV_16SC2):
        a, b = R.init_maps(size=(37, 9), m1type=t, **CASES[case]), R.init_maps(size=(37, 9), m1type=t, loops=True, **CASES[case])
        assert all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_two_forms_of_the_reprojection_agree():
    rng = np.random.default_rng(5)
    Q = [[1, 0, 0, -19.5], [0, 1, 0, -7.25], [0, 0, 0, 533.25], [0, 0, 1 / 0.12, 0.3]]
    for dt in (np.uint8, np.int16, np.int32, np.float32):
        d = rng.integers(0, 90, (7, 13)).astype(dt)
        d[2, 3] = d[4, 11] = d.min()
        for hm in (False, True):
            assert R.same_floats(R.reproject(d, Q, hm), R.reproject_loops(d, Q, hm)), (dt, hm)


# ---------------------------------------------------------------------------------------------------------------- verified here in numpy
def test_identity_map_up_to_640x480():
    m1, m2 = R.init_maps(K, None, None, K, (640, 480), R.CV_16SC2)
    jj, ii = np.meshgrid(np.arange(640), np.arange(480))
    assert np.array_equal(m1[..., 0], jj) and np.array_equal(m1[..., 1], ii) and not m2.any()
    src = _image(1, 48, 64, 3)
    assert np.array_equal(R.undistort_rectify(src, K, None), src)


def test_shift_map_and_image():
    newK = K.copy()
    newK[0, 2] += 3
    newK[1, 2] -= 2
    m1, m2 = R.init_maps(K, None, None, newK, (160, 120), R.CV_16SC2)
    jj, ii = np.meshgrid(np.arange(160), np.arange(120))
    assert np.array_equal(m1[..., 0], jj - 3) and np.array_equal(m1[..., 1], ii + 2) and not m2.any()
    src = _image(2, 120, 160, 1)
    got = R.undistort_rectify(src, K, None, newK=newK, value=37)
    want = np.full_like(src, 37)
    want[:118, 3:] = src[2:, :157]
    assert np.array_equal(got, want)


def test_non_finite_pixel_is_pinned():
    """newK = I, R = [[1,0,0],[0,1,0],[0.125,0,-1]] is its own inverse; _w = j / 8 - 1 is exactly 0 in column 8: those pixels take INT_MIN, entry (0, 0), fraction 0.
    Elsewhere x = j / (j / 8 - 1), y = i / (j / 8 - 1) with u = x, v = y (K = I): column 0 maps to (0, -i), column 16 to (16, i), column 12 to (24, 2 i)."""
    Rm = [[1, 0, 0], [0, 1, 0], [0.125, 0, -1]]
    ir = R.inverse(np.eye(3), Rm)
    assert [abs(t) for t in ir] == [1, 0, 0, 0, 1, 0, 0.125, 0, 1] and ir[0] == 1 and ir[4] == 1 and ir[6] == 0.125 and ir[8] == -1
    m1, m2 = R.init_maps(np.eye(3), None, Rm, np.eye(3), (16, 3), R.CV_16SC2)
    assert m1[:, 8].tolist() == [[0, 0]] * 3 and m2[:, 8].tolist() == [0, 0, 0]
    assert m1[:, 0].tolist() == [[0, 0], [0, -1], [0, -2]] and m1[:, 12].tolist() == [[24, 0], [24, 2], [24, 4]] and not m2[:, [0, 12]].any()
    # column 4: w = -2, x = -8, y = -2 i; column 9: _w = 1/8, x = 72, y = 8 i; column 10: _w = 1/4, x = 40, y = 4 i
    want = np.array([[[int(np.rint(32 * j / (j / 8 - 1))) >> 5, int(np.rint(32 * i / (j / 8 - 1))) >> 5] if j != 8 else [0, 0] for j in range(16)] for i in range(3)])
    assert np.array_equal(m1, want)
    assert m1[1].tolist() == [[0, -1], [-2, -2], [-3, -2], [-5, -2], [-8, -2], [-14, -3], [-24, -4], [-56, -8], [0, 0], [72, 8], [40, 4], [29, 2], [24, 2], [20, 1], [18, 1],
                              [17, 1]]
    u, v = R.map_uv(R.camera(np.eye(3), None, Rm, np.eye(3)), 16, 3)
    assert not np.isfinite(u[:, 8]).any() and np.isnan(v[0, 8]) and R.sat_int(np.array([np.nan, np.inf, -np.inf, 2.5, 3.5, -2.5, 1e12, -1e12])).tolist() == \
        [R.INT_MIN, R.INT_MIN, R.INT_MIN, 2, 4, -2, R.INT_MAX, R.INT_MIN]


def test_closed_form_against_the_accumulating_form():
    """every CV_16SC2 entry of the bench's lens at 640 x 480 either agrees with the reference's accumulating form or differs by one unit of 1/32 px in one coordinate;
    the count is measured (printed) and quoted in DESIGN 6.21"""
    cam = R.camera(K, R.LENS, ROT, None)
    a = np.stack(R.fixed(*R.map_uv(cam, 640, 480)), -1)
    b = np.stack(R.fixed(*R.accumulated_uv(cam, 640, 480)), -1)
    diff = np.abs(a - b)
    print("closed form vs accumulating form: %d of %d entries differ" % (int((diff.sum(-1) > 0).sum()), diff.shape[0] * diff.shape[1]))
    assert (diff.sum(-1) <= 1).all()


def test_one_pixel_by_hand():
    """K = [[128, 0, 64], [0, 128, 32], [0, 0, 1]], k1 = 0.25, everything else absent.  det = 16384, ir = [1/128, 0, -1/2, 0, 1/128, -1/4, 0, 0, 1], all exact.
    Pixel (j, i) = (192, 32): _x = 1.5 - 0.5 = 1, _y = 0.25 - 0.25 = 0, _w = 1; r2 = 1, kr = 1.25, xd = 1.25, yd = 0; u = 128 * 1.25 + 64 = 224, v = 32.
    Pixel (160, 32): x = 0.75, r2 = 0.5625, kr = 1.140625, xd = 0.85546875, u = 109.5 + 64 = 173.5: entry (173, 32), fraction word 16."""
    Kh = [[128, 0, 64], [0, 128, 32], [0, 0, 1]]
    cam = R.camera(Kh, [0.25, 0, 0, 0])
    assert [abs(t) for t in cam["ir"]] == [1 / 128, 0, 0.5, 0, 1 / 128, 0.25, 0, 0, 1]
    for f in (R.map_uv, R.map_uv_loops):
        u, v = f(cam, 193, 33)
        assert (u[32, 192], v[32, 192], u[32, 160], v[32, 160]) == (224.0, 32.0, 173.5, 32.0)
    m1, m2 = R.init_maps(Kh, [0.25, 0, 0, 0], None, None, (193, 33), R.CV_16SC2)
    assert m1[32, 192].tolist() == [224, 32] and m2[32, 192] == 0 and m1[32, 160].tolist() == [173, 32] and m2[32, 160] == 16


def test_reprojection_by_hand():
    """Q = [[1,0,0,-64],[0,1,0,-32],[0,0,0,256],[0,0,0.25,0]]: the point of (x, y, d) is (4 (x - 64) / d, 4 (y - 32) / d, 1024 / d), exact for d a power of two.
    d = 0: h_3 = 0, iw = inf; x = 64 gives 0 * inf = NaN in the first coordinate."""
    Q = [[1, 0, 0, -64], [0, 1, 0, -32], [0, 0, 0, 256], [0, 0, 0.25, 0]]
    d = np.full((34, 66), 8, np.int16)
    d[33, 65], d[0, 0], d[32, 64], d[10, 64] = 2, 16, 4, 0
    d[5, 5] = d[6, 7] = d[33, 0] = 1                                                   # the minimum of the non-zero part; with the 0 the minimum is 0, once
    p = R.reproject(d, Q)
    assert p[33, 65].tolist() == [2.0, 2.0, 512.0] and p[0, 0].tolist() == [-16.0, -8.0, 64.0] and p[32, 64].tolist() == [0.0, 0.0, 256.0]
    assert np.isnan(p[10, 64, 0]) and p[10, 64, 1] == -np.inf and p[10, 64, 2] == np.inf and np.isnan(p).sum() == 1
    d2 = np.where(d == 0, 8, d).astype(np.int16)                                        # now the minimum 1 occurs three times
    m = R.reproject(d2, Q, True)
    assert (m[..., 2] == 10000).sum() == 3 and m[5, 5].tolist() == [-236.0, -108.0, 10000.0] and m[6, 7, 2] == 10000 and m[33, 0, 2] == 10000
    assert R.same_floats(m[..., :2], R.reproject(d2, Q)[..., :2])
    assert R.same_floats(R.reproject_loops(d, Q, True), R.reproject(d, Q, True)) and (R.reproject(d, Q, True)[..., 2] == 10000).sum() == 1


# ---------------------------------------------------------------------------------------------------------------- undistort_math.h on the host, stage by stage
def test_emu_inverse_and_sat(emu):
    rng = np.random.default_rng(9)
    mats = [(K, np.eye(3)), (K, ROT), (np.eye(3), [[1, 0, 0], [0, 1, 0], [0.125, 0, -1]]), (CASES["quarter"]["newK"], ROT)]
    mats += [(K + rng.normal(0, 1, (3, 3)), rng.normal(0, 1, (3, 3))) for _ in range(20)]
    for nK, Rm in mats:
        nK, Rm = np.ascontiguousarray(nK, np.float64), np.ascontiguousarray(Rm, np.float64)
        got = np.zeros(9)
        assert emu.emu_und_inverse(_ptr(nK), _ptr(Rm), _ptr(got)) == 1
        assert R.same_floats(got, np.array(R.inverse(nK, Rm)))
    for nK in (np.zeros((3, 3)), np.full((3, 3), np.inf), np.diag([1.0, np.nan, 1.0]), np.ones((3, 3))):
        assert emu.emu_und_inverse(_ptr(np.ascontiguousarray(nK)), _ptr(np.eye(3)), _ptr(np.zeros(9))) == 0 and R.inverse(nK, np.eye(3)) is None
    vals = [np.nan, np.inf, -np.inf, 0.5, 1.5, 2.5, -0.5, -1.5, 2147483646.5, 2147483647.0, 3e9, -2147483648.0, -2147483648.5, -3e9, 1e300, 12345.49999]
    assert [emu.emu_und_sat(v) for v in vals] == R.sat_int(np.array(vals)).tolist()


@pytest.mark.parametrize("case", sorted(CASES))
def test_emu_uv_and_the_three_map_forms(emu, case):
    cam = R.camera(**CASES[case])
    args = _cam_args(cam)
    w, h = 131, 33
    u, v = np.zeros((h, w)), np.zeros((h, w))
    emu.emu_und_uv(*[_ptr(a) for a in args], w, h, _ptr(u), _ptr(v))
    wu, wv = R.map_uv(cam, w, h)
    assert R.same_floats(u, wu) and R.same_floats(v, wv)
    for form, t in enumerate((R.CV_32FC1, R.CV_32FC2, R.CV_16SC2)):
        w1, w2 = R.init_maps(size=(w, h), m1type=t, **CASES[case])
        g1 = np.zeros_like(w1)
        g2 = np.zeros_like(w2) if w2 is not None else np.zeros(1)
        emu.emu_und_maps(*[_ptr(a) for a in args], w, h, form, _ptr(g1), _ptr(g2))
        assert (R.same_floats(g1, w1) if t != R.CV_16SC2 else np.array_equal(g1, w1)) and (w2 is None or (R.same_floats(g2, w2) if t == R.CV_32FC1 else np.array_equal(g2, w2)))


def test_emu_non_finite_map(emu):
    cam = R.camera(np.eye(3), None, [[1, 0, 0], [0, 1, 0], [0.125, 0, -1]], np.eye(3))
    args = _cam_args(cam)
    g1, g2 = np.full((3, 16, 2), 9, np.int16), np.full((3, 16), 9, np.uint16)
    emu.emu_und_maps(*[_ptr(a) for a in args], 16, 3, 2, _ptr(g1), _ptr(g2))
    w1, w2 = R.fixed_maps(*R.map_uv(cam, 16, 3))
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2) and g1[:, 8].tolist() == [[0, 0]] * 3


@pytest.mark.parametrize("case,cn,dsize,ssize", [("lens", 1, (129, 33), (129, 33)), ("lens", 3, (257, 65), (300, 80)), ("barrel", 1, (257, 65), (257, 65)),
                                                 ("barrel", 4, (129, 33), (140, 40)), ("quarter", 1, (257, 65), (257, 65)), ("quarter", 3, (129, 33), (129, 33)),
                                                 ("rational", 4, (257, 65), (257, 65)), ("plain", 1, (5, 3), (2, 2)), ("plain", 3, (1, 1), (1, 1))])
def test_emu_of_the_tile_kernel(emu, case, cn, dsize, ssize):
    """whole images as k_undist8_tile orders the work, and the box of every tile against the extremes of the restatement's map"""
    src = _image(sum(dsize) + cn, ssize[1], ssize[0], cn)
    th = 32 if cn == 1 else 16
    gx, gy = -(-dsize[0] // 128), -(-dsize[1] // th)
    m1, _ = R.init_maps(size=dsize, m1type=R.CV_16SC2, **CASES[case])
    for border, value in ((R.BORDER_CONSTANT, (37, 99, 250.6, 3)), (R.BORDER_REPLICATE, 0), (R.BORDER_REFLECT_101, 0), (R.BORDER_REFLECT, 0), (R.BORDER_WRAP, 0)):
        want = R.undistort_rectify(src, dsize=dsize, border=border, value=value, **CASES[case])
        boxes = np.zeros((gy * gx, 6), np.int32)
        assert np.array_equal(_emu_tile(emu, case, src, dsize, border, value, boxes=boxes), want), (border, "staged")
        for ty in range(gy):
            for tx in range(gx):
                t = m1[ty * th:(ty + 1) * th, tx * 128:(tx + 1) * 128]
                assert boxes[ty * gx + tx, :4].tolist() == [t[..., 0].min(), t[..., 0].max(), t[..., 1].min(), t[..., 1].max()]
        assert np.array_equal(_emu_tile(emu, case, src, dsize, border, value, lds=96), want), (border, "allotment of 96 bytes: every box overflows")
        assert np.array_equal(_emu_tile(emu, case, src, dsize, border, value, dwords=0), want), (border, "no dword path")


def test_emu_some_box_is_staged_and_some_overflows(emu):
    boxes = np.zeros((3 * 3, 6), np.int32)
    src = _image(3, 80, 300, 1)                                                         # larger than the destination: the last tile row, one row high, has a footprint too
    _emu_tile(emu, "lens", src, (257, 65), boxes=boxes)
    assert (boxes[:, 4] > 0).all()                                                      # every tile of the bench's lens stages a box at the default allotment
    _emu_tile(emu, "lens", src, (257, 65), lds=2048, boxes=boxes)
    assert (boxes[:, 4] > 0).any() and ((boxes[:, 4] == 0) & (boxes[:, 5] == 0)).any()  # 2 KiB: the ragged edge tiles fit, the full ones overflow
    _emu_tile(emu, "quarter", src, (257, 65), boxes=boxes)
    assert (boxes[:, 5] == -1).any()                                                    # a quarter of the focal length: whole tiles fall outside the source


@pytest.mark.parametrize("cn,nframes,fpw", [(1, 3, 2), (3, 5, 4), (4, 2, 1), (1, 9, 8)])
def test_emu_frame_walk(emu, cn, nframes, fpw):
    frames = np.stack([_image(40 + f, 33, 129, cn) for f in range(nframes)])
    got = _emu_tile(emu, "lens", frames, (129, 33), R.BORDER_CONSTANT, 5, nframes=nframes, fpw=fpw)
    for f in range(nframes):
        assert np.array_equal(got[f], R.undistort_rectify(frames[f], dsize=(129, 33), value=5, **CASES["lens"])), f


def test_emu_reprojection(emu):
    rng = np.random.default_rng(8)
    Q = np.array([[1, 0, 0, -64], [0, 1, 0, -32], [0, 0, 0, 256], [0, 0, 0.25, 0.001]], np.float64)
    for depth, dt in ((0, np.uint8), (3, np.int16), (4, np.int32), (5, np.float32)):
        d = rng.integers(0, 100, (9, 21)).astype(dt)
        if dt == np.float32:
            d[3, 3] = np.nan
        for hm in (0, 1):
            out = np.zeros((9, 21, 3), np.float32)
            emu.emu_und_reproject(_ptr(d), depth, 21, 9, _ptr(Q), hm, R.frame_min(d), _ptr(out))
            assert R.same_floats(out, R.reproject(d, Q, bool(hm))), (dt, hm)


# ---------------------------------------------------------------------------------------------------------------- the library, no device
def test_limits_are_pinned():
    from opencv_amd import _lib
    keys = ("undist_max_dim", "undist_max_src_dim", "undist_tile_cols", "undist_tile_rows", "undist_lds_kib", "undist_max_lds_kib", "undist_frames_per_group",
            "undist_max_frames_per_group", "reproject_max_dim")
    assert {k: _lib.limit(k) for k in keys} == dict(zip(keys, (16384, 32767, 128, 32, 24, 48, 8, 64, 16384)))
    # a destination column and a source coordinate in 1/32 px are exact in an int and a double; six workgroups of the default allotment fit the LDS of a CU
    assert 16384 * 32 < 2 ** 31 and 6 * (24 * 1024 + 64) <= 160 * 1024 and 48 * 1024 + 64 <= 64 * 1024 and _lib.limit("reproject_max_dim") == _lib.limit("minmax_max_dim") \
        if _has_limit(_lib, "minmax_max_dim") else True


def _has_limit(_lib, key):
    try:
        _lib.limit(key)
        return True
    except KeyError:
        return False


def test_refusals_before_a_device_is_touched():
    import opencv_amd as cv
    from opencv_amd import _lib
    Lb, NI, top = _lib.lib, _lib.NOT_IMPLEMENTED, _lib.limit
    reason = lambda: Lb.mi355cv_lastError().decode()                                                      # noqa: E731
    W, H = 96, 64
    buf = np.zeros((4 * H, 16 * W), np.uint8)
    out = np.full((4 * H, 16 * W), 123, np.uint8)
    Kc = np.ascontiguousarray(K)
    d14 = np.zeros(14)
    tau = d14.copy()
    tau[13] = 1e-3
    bv = (ctypes.c_double * 4)(0, 0, 0, 0)
    Q = np.eye(4)
    P = lambda a: None if a is None else _ptr(a)                                                          # noqa: E731

    def rect(src_type=0, sstep=16 * W, sw=W, sh=H, dstep=16 * W, dw=W, dh=H, Kp=Kc, dist=None, ndist=0, Rp=None, newK=None, interp=1, border=0, batch=None, sframe=H * 16 * W,
             dframe=H * 16 * W, src=None, dst=None):
        s, d = buf.ctypes.data if src is None else src, out.ctypes.data if dst is None else dst
        if batch is not None:
            return Lb.mi355cv_undistortRectifyBatch(src_type, s, sstep, sframe, sw, sh, d, dstep, dframe, dw, dh, batch, P(Kp), P(dist), ndist, P(Rp), P(newK), interp, border, bv)
        return Lb.mi355cv_undistortRectify(src_type, s, sstep, sw, sh, d, dstep, dw, dh, P(Kp), P(dist), ndist, P(Rp), P(newK), interp, border, bv)

    def maps(w=W, h=H, m1type=R.CV_16SC2, s1=16 * W, s2=16 * W, m2=True, **kw):
        return Lb.mi355cv_initUndistortRectifyMap(P(kw.get("Kp", Kc)), P(kw.get("dist")), kw.get("ndist", 0), None, P(kw.get("newK")), w, h, m1type, out.ctypes.data, s1,
                                                  out.ctypes.data + 2 * H * 16 * W if m2 else None, s2)

    def repro(w=W, h=H, t=3, sstep=16 * W, dstep=16 * W, ddepth=-1, batch=None, sframe=H * 16 * W, dframe=H * 16 * W, src=None, dst=None, Qp=Q):
        s, d = buf.ctypes.data if src is None else src, out.ctypes.data if dst is None else dst
        if batch is not None:
            return Lb.mi355cv_reprojectImageTo3DBatch(s, sstep, sframe, t, d, dstep, dframe, w, h, batch, P(Qp), 0, ddepth)
        return Lb.mi355cv_reprojectImageTo3D(s, sstep, t, d, dstep, w, h, P(Qp), 0, ddepth)

    big = top("undist_max_dim") + 1
    sing = np.ascontiguousarray(np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]))
    infk = np.ascontiguousarray(np.array([[np.inf, 0, 0], [0, 1.0, 0], [0, 0, 1]]))
    cases = [
        (rect, dict(Kp=None), "!K"), (rect, dict(ndist=3, dist=d14), "ndist is none of"), (rect, dict(ndist=6, dist=d14), "ndist is none of"), (rect, dict(ndist=-1), "ndist is none of"),
        (rect, dict(ndist=5), "ndist > 0 && !dist"), (rect, dict(ndist=14, dist=tau), "tauX / tauY"), (rect, dict(newK=sing), "singular"), (rect, dict(Kp=np.zeros((3, 3))), "singular"),
        (rect, dict(newK=infk), "singular"), (rect, dict(Rp=np.zeros((3, 3))), "singular"),
        (rect, dict(dw=0), "width < 1"), (rect, dict(dh=-3), "height < 1"), (rect, dict(dw=big, dstep=1 << 16), "UNDIST_MAX_DIM"), (rect, dict(dh=big), "UNDIST_MAX_DIM"),
        (rect, dict(sw=0), "sw < 1"), (rect, dict(sw=top("undist_max_src_dim") + 1, sstep=1 << 16), "UNDIST_MAX_SRC_DIM"), (rect, dict(sh=40000), "UNDIST_MAX_SRC_DIM"),
        (rect, dict(src_type=7), "depth < 0 || depth > 6"), (rect, dict(border=6), "border < 0"),
        (rect, dict(sstep=W - 1), "sstep < srow"), (rect, dict(dstep=W - 1), "dstep < drow"), (rect, dict(src_type=16, sstep=3 * W - 1), "sstep < srow"),
        (rect, dict(dst=buf.ctypes.data), "src and dst overlap"), (rect, dict(dst=buf.ctypes.data + 5 * 16 * W + 7), "src and dst overlap"),
        (rect, dict(batch=0), "nframes < 1"), (rect, dict(batch=-2), "nframes < 1"), (rect, dict(batch=2, sframe=H * 16 * W - 16 * W), "sframe <"), (rect, dict(batch=2, dframe=W), "dframe <"),
        (rect, dict(batch=2, ndist=7, dist=d14), "ndist is none of"), (rect, dict(batch=2, dst=buf.ctypes.data + H * 16 * W), "src and dst overlap"),
        (maps, dict(m1type=0), "m1type is none of"), (maps, dict(m1type=R.CV_16UC1), "m1type is none of"), (maps, dict(m1type=3), "m1type is none of"),
        (maps, dict(w=0), "width < 1"), (maps, dict(h=big), "UNDIST_MAX_DIM"), (maps, dict(s1=4 * W - 1), "map1_step < r1"), (maps, dict(s2=2 * W - 2), "map2_step < r2"),
        (maps, dict(m2=False), "!map2"), (maps, dict(ndist=2, dist=d14), "ndist is none of"), (maps, dict(ndist=14, dist=tau), "tauX / tauY"), (maps, dict(newK=sing), "singular"),
        (maps, dict(m1type=R.CV_32FC2, s1=8 * W - 4), "map1_step < r1"),
        (repro, dict(t=2), "the disparity is none of"), (repro, dict(t=6), "the disparity is none of"), (repro, dict(t=1), "the disparity is none of"), (repro, dict(t=3 + 8), "the disparity is none of"),
        (repro, dict(ddepth=3), "CV_16SC3 / CV_32SC3"), (repro, dict(ddepth=4), "CV_16SC3 / CV_32SC3"), (repro, dict(ddepth=0), "ddepth != -1"), (repro, dict(Qp=None), "!Q"),
        (repro, dict(w=0), "w < 1"), (repro, dict(h=top("reproject_max_dim") + 1), "REPROJECT_MAX_DIM"), (repro, dict(sstep=2 * W - 2), "sstep < srow"), (repro, dict(dstep=12 * W - 4), "dstep < drow"),
        (repro, dict(sstep=2 * W + 1), "no multiple of its element size"), (repro, dict(dst=buf.ctypes.data + 64), "src and dst overlap"),
        (repro, dict(batch=0), "nframes < 1"), (repro, dict(batch=2, sframe=2 * W), "sframe <"), (repro, dict(batch=2, dframe=12 * W), "dframe <"),
    ]
    for fn, kw, why in cases:
        assert fn(**kw) == NI, kw
        assert why in reason(), (kw, reason())
    assert (out == 123).all() and (buf == 0).all()
    assert [Lb.mi355cv_undistortSetKernel(m) for m in (-2, 2, 0, 1, -1)] == [-1, -1, 0, 0, 0]
    assert [Lb.mi355cv_undistortSetLds(b) for b in (-1, (top("undist_max_lds_kib") << 10) + 1, 96, 0)] == [-1, -1, 0, 0]
    assert [Lb.mi355cv_undistortSetFramesPerGroup(n) for n in (-1, top("undist_max_frames_per_group") + 1, 2, 0)] == [-1, -1, 0, 0]

    # the Python mirror: its own argument errors, and the ledger counts its refusals and the library's under the entry
    img = np.zeros((H, W), np.uint8)
    with pytest.raises(ValueError, match="cameraMatrix must be 3 x 3"):
        cv.undistort(img, np.eye(4), None)
    with pytest.raises(ValueError, match="newCameraMatrix must be 3 x 3 or 3 x 4"):
        cv.undistort(img, K, None, newCameraMatrix=np.eye(2))
    with pytest.raises(ValueError, match="size = "):
        cv.initUndistortRectifyMap(K, None, None, K, 7, R.CV_16SC2)
    with pytest.raises(ValueError, match="dsize and the type of the source"):
        cv.undistort(img, K, None, dst=np.zeros((H, W - 1), np.uint8))
    with pytest.raises(ValueError, match="a stack"):
        cv.undistortBatch(img, K, None)
    with pytest.raises(ValueError, match="Q must be 4 x 4"):
        cv.reprojectImageTo3D(img, np.eye(3))
    with pytest.raises(ValueError, match="disparity must be H x W"):
        cv.reprojectImageTo3D(np.zeros((2, H, W), np.uint8), np.eye(4))
    with pytest.raises(ValueError, match="H x W x 3 float32"):
        cv.reprojectImageTo3D(img, np.eye(4), dst=np.zeros((H, W, 3), np.float64))
    names = ("initUndistortRectifyMap", "undistortRectify", "undistortRectifyBatch", "reprojectImageTo3D", "reprojectImageTo3DBatch")
    n0 = [_lib.decline_count(n) for n in names]
    keep = np.full((H, W), 9, np.uint8)
    with pytest.raises(NotImplementedError, match="m1type is none of"):
        cv.initUndistortRectifyMap(K, None, None, K, (W, H), 0)
    with pytest.raises(NotImplementedError, match="ndist is none of"):
        cv.initUndistortRectifyMap(K, [0.1, 0.2, 0.3], None, K, (W, H), R.CV_16SC2)
    with pytest.raises(NotImplementedError, match="tauX / tauY"):
        cv.undistort(img, K, tau, dst=keep)
    with pytest.raises(NotImplementedError, match="singular"):
        cv.undistortRectify(img, K, None, np.zeros((3, 3)), dst=keep)
    with pytest.raises(NotImplementedError, match="src and dst overlap"):
        cv.undistort(img, K, None, dst=img)
    with pytest.raises(NotImplementedError, match="UNDIST_MAX_DIM"):
        cv.undistortRectifyBatch(np.stack([img, img]), K, None, dsize=(big, 1))
    with pytest.raises(NotImplementedError, match="the disparity is none of"):
        cv.reprojectImageTo3D(img.astype(np.uint16), np.eye(4))
    with pytest.raises(NotImplementedError, match="CV_16SC3 / CV_32SC3"):
        cv.reprojectImageTo3D(img, np.eye(4), ddepth=cv.CV_16S)
    with pytest.raises(NotImplementedError, match="the disparity is none of"):
        cv.reprojectImageTo3DBatch(np.zeros((2, H, W), np.float64), np.eye(4))
    assert [_lib.decline_count(n) - a for n, a in zip(names, n0)] == [2, 3, 1, 2, 1]
    assert (keep == 9).all()
