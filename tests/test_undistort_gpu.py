"""cv::initUndistortRectifyMap, cv::undistort, the rectifying warp and cv::reprojectImageTo3D on the GPU against tests/undistort_restate.py, all by exact equality:
the three map forms at every width and height around the launch and tile edges and on misaligned pitched views with guarded destinations; the master equality
undistortRectify == remap(initUndistortRectifyMap(CV_16SC2)) under each arm of mi355cv_undistortSetKernel with the kernel that ran asserted, the composed arm in turn
against the restatement's own bilinear; the classes only the composed arm serves; batches (frame counts around the frames per workgroup, cut batches, host-resident
frames, numpy and device inputs); identity and shift; reprojectImageTo3D on the four depths, with the per-frame minimum, and fed from StereoBM without leaving HBM."""
import numpy as np
import pytest
import torch

import undistort_restate as R
import viewcheck as vc
import opencv_amd as cv
from opencv_amd import _lib
from viewtable import Device

pytestmark = pytest.mark.gpu
Lb = _lib.lib
K = np.array(R.K_TEST, np.float64)
ROT = np.array(R.rot_y(0.02), np.float64)
CASES = {
    "lens": dict(K=K, dist=R.LENS, R=ROT, newK=None),
    "barrel": dict(K=K, dist=[-0.6, 0, 0, 0], R=None, newK=None),
    "quarter": dict(K=K, dist=R.LENS, R=None, newK=[[K[0, 0] / 4, 0, K[0, 2]], [0, K[1, 1] / 4, K[1, 2]], [0, 0, 1]]),
}
BORDERS = [(cv.BORDER_CONSTANT, (37, 99, 250.6, 3)), (cv.BORDER_REPLICATE, 0), (cv.BORDER_REFLECT_101, 0)]
FPW = _lib.limit("undist_frames_per_group")


def last_kernel():
    return Lb.mi355cv_lastKernel().decode()


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    Lb.mi355cv_undistortSetKernel(-1)
    Lb.mi355cv_undistortSetLds(0)
    Lb.mi355cv_undistortSetFramesPerGroup(0)


def _image(seed, h, w, cn, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    shape = (h, w) + ((cn,) if cn > 1 else ())
    if dtype == np.float32:
        return rng.normal(0, 50, shape).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def _call(case, src, dsize=None, border=cv.BORDER_CONSTANT, value=0, interp=cv.INTER_LINEAR, **kw):
    c = CASES[case]
    return cv.undistortRectify(src, c["K"], c["dist"], c["R"], c["newK"], dsize, interp, border, value, **kw)


def _maps(case, dsize, device="cuda"):
    c = CASES[case]
    return cv.initUndistortRectifyMap(c["K"], c["dist"], c["R"], c["newK"], dsize, R.CV_16SC2, device=device)


def _same_map(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return R.same_floats(got, want) if want.dtype == np.float32 else np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- the maps
@pytest.mark.parametrize("m1type", [R.CV_32FC1, R.CV_32FC2, R.CV_16SC2])
def test_maps_at_every_edge_size(m1type):
    c = CASES["lens"]
    for w in (1, 3, 4, 5, 127, 128, 129, 131):
        for h in (1, 15, 16, 17, 31, 32, 33):
            want = R.init_maps(c["K"], c["dist"], c["R"], c["newK"], (w, h), m1type)
            got = cv.initUndistortRectifyMap(c["K"], c["dist"], c["R"], c["newK"], (w, h), m1type, device="cuda")
            assert "k_undist_map" in last_kernel()
            assert _same_map(got[0], want[0]) and (want[1] is None and got[1] is None or _same_map(got[1], want[1])), (w, h)
    got = cv.initUndistortRectifyMap(c["K"], c["dist"], c["R"], c["newK"], (131, 33), m1type)               # numpy maps: staged
    want = R.init_maps(c["K"], c["dist"], c["R"], c["newK"], (131, 33), m1type)
    assert isinstance(got[0], np.ndarray) and _same_map(got[0], want[0]) and (want[1] is None or _same_map(got[1], want[1]))


@pytest.mark.parametrize("layout", vc.LAYOUTS)
@pytest.mark.parametrize("m1type", [R.CV_32FC1, R.CV_32FC2, R.CV_16SC2])
def test_maps_on_views_with_guarded_destinations(layout, m1type):
    c = CASES["lens"]
    w, h = 131, 33
    want = [m for m in R.init_maps(c["K"], c["dist"], c["R"], c["newK"], (w, h), m1type) if m is not None]

    def call(_src, dst):
        d = dst if isinstance(dst, tuple) else (dst, None)
        cv.initUndistortRectifyMap(c["K"], c["dist"], c["R"], c["newK"], (w, h), m1type, map1=d[0], map2=d[1])
    try:
        vc.run(call, layout, np.zeros((2, 2), np.uint8), want if len(want) > 1 else want[0], "initUndistortRectifyMap %d layout %s" % (m1type, layout), device=Device)
    except vc.Unreachable as e:
        pytest.skip(str(e))


def test_non_finite_map_entries():
    Rm = [[1, 0, 0], [0, 1, 0], [0.125, 0, -1]]
    m1, m2 = cv.initUndistortRectifyMap(np.eye(3), None, Rm, np.eye(3), (16, 3), R.CV_16SC2, device="cuda")
    w1, w2 = R.init_maps(np.eye(3), None, Rm, np.eye(3), (16, 3), R.CV_16SC2)
    assert np.array_equal(m1.cpu().numpy(), w1) and np.array_equal(m2.cpu().numpy(), w2) and m1[:, 8].cpu().tolist() == [[0, 0]] * 3 and not m2.cpu().numpy()[:, 8].any()
    for t in (R.CV_32FC1, R.CV_32FC2):
        got = cv.initUndistortRectifyMap(np.eye(3), None, Rm, np.eye(3), (16, 3), t, device="cuda")
        want = R.init_maps(np.eye(3), None, Rm, np.eye(3), (16, 3), t)
        assert _same_map(got[0], want[0]) and (want[1] is None or _same_map(got[1], want[1]))


# ---------------------------------------------------------------------------------------------------------------- the master equality
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("case", sorted(CASES))
def test_master_equality_under_each_arm(case, cn):
    for dsize, ssize in (((129, 33), (129, 33)), ((257, 65), (300, 80))):
        src_np = _image(cn + dsize[0], ssize[1], ssize[0], cn)
        src = torch.from_numpy(src_np).cuda()
        m1, m2 = _maps(case, dsize)
        for border, value in BORDERS:
            want = cv.remap(src, m1, m2, cv.INTER_LINEAR, border, value)
            # the chain does not rest on remap alone: the restatement's own bilinear on the restatement's maps
            assert np.array_equal(want.cpu().numpy(), R.undistort_rectify(src_np, dsize=dsize, border=border, value=value, **CASES[case])), (dsize, border)
            for mode, lds, name in ((-1, 0, None), (0, 0, "k_undist_map"), (1, 0, "k_undist8_tile<%d>" % cn), (1, 1024, "k_undist8_tile<%d>" % cn)):
                Lb.mi355cv_undistortSetKernel(mode)
                Lb.mi355cv_undistortSetLds(lds)
                got = _call(case, src, dsize, border, value)
                if name:
                    assert name in last_kernel(), (mode, last_kernel())
                assert torch.equal(got, want), (dsize, border, mode, lds, last_kernel())


def test_built_in_rule():
    """the tile kernel serves every batch and single frames of 3 and 4 channels, a single one-channel frame goes to the composed arm"""
    c = CASES["lens"]
    for cn in (1, 3, 4):
        frames = torch.from_numpy(np.stack([_image(f, 33, 129, cn) for f in range(2)])).cuda()
        _call("lens", frames[0])
        assert ("composed" if cn == 1 else "k_undist8_tile<%d>" % cn) in last_kernel(), last_kernel()
        cv.undistortRectifyBatch(frames, c["K"], c["dist"], c["R"], c["newK"])
        assert "k_undist8_tile<%d>" % cn in last_kernel(), last_kernel()


def test_tile_kernel_on_a_misaligned_view_takes_the_byte_path():
    parent = torch.from_numpy(_image(3, 90, 333, 1)).cuda()
    src = parent[5:85, 3:303]
    m1, m2 = _maps("lens", (257, 65))
    want = cv.remap(src.contiguous(), m1, m2, cv.INTER_LINEAR, cv.BORDER_CONSTANT, 9)
    Lb.mi355cv_undistortSetKernel(1)
    dparent = torch.full((70, 301), 200, dtype=torch.uint8, device="cuda")
    got = _call("lens", src, (257, 65), cv.BORDER_CONSTANT, 9, dst=dparent[2:67, 1:258])
    assert "k_undist8_tile<1>" in last_kernel() and "dwords=0" in last_kernel()
    assert torch.equal(got, want) and int((dparent != 200).sum()) == int((want != 200).sum())


@pytest.mark.parametrize("dtype,cn,interp", [(np.uint16, 1, cv.INTER_LINEAR), (np.float32, 1, cv.INTER_LINEAR), (np.uint8, 1, cv.INTER_NEAREST), (np.uint8, 1, cv.INTER_CUBIC)])
def test_composed_only_classes(dtype, cn, interp):
    src = torch.from_numpy(_image(11, 80, 150, cn, dtype)).cuda()
    m1, m2 = _maps("lens", (129, 33))
    Lb.mi355cv_undistortSetKernel(1)
    got = _call("lens", src, (129, 33), cv.BORDER_REFLECT_101, 0, interp)
    assert "composed" in last_kernel()
    assert torch.equal(got, cv.remap(src, m1, m2, interp, cv.BORDER_REFLECT_101, 0))


# ---------------------------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("cn", [1, 3])
def test_batches_equal_single_calls(cn):
    c = CASES["lens"]
    for n in (1, 2, FPW + 1):
        frames = torch.from_numpy(np.stack([_image(50 + f, 40, 140, cn) for f in range(n)])).cuda()
        singles = torch.stack([_call("lens", frames[f], (129, 33), cv.BORDER_CONSTANT, 5) for f in range(n)])
        for mode, fpw, lds in ((-1, 0, 0), (1, 0, 0), (1, 2, 0), (1, 1, 512), (0, 0, 0)):
            Lb.mi355cv_undistortSetKernel(mode)
            Lb.mi355cv_undistortSetFramesPerGroup(fpw)
            Lb.mi355cv_undistortSetLds(lds)
            got = cv.undistortRectifyBatch(frames, c["K"], c["dist"], c["R"], c["newK"], (129, 33), cv.INTER_LINEAR, cv.BORDER_CONSTANT, 5)
            assert mode == -1 or ("k_undist8_tile<%d>" % cn if mode else "composed") in last_kernel(), last_kernel()
            assert torch.equal(got, singles), (n, mode, fpw, lds)
        Lb.mi355cv_undistortSetKernel(-1)
        Lb.mi355cv_undistortSetFramesPerGroup(0)
        Lb.mi355cv_undistortSetLds(0)
        host = cv.undistortRectifyBatch(frames.cpu().numpy(), c["K"], c["dist"], c["R"], c["newK"], (129, 33), cv.INTER_LINEAR, cv.BORDER_CONSTANT, 5)     # the shared pipeline
        assert isinstance(host, np.ndarray) and np.array_equal(host, singles.cpu().numpy())
    one = cv.undistortBatch(frames, c["K"], c["dist"])
    assert torch.equal(one[1], cv.undistort(frames[1], c["K"], c["dist"])) and np.array_equal(cv.undistort(frames[1].cpu().numpy(), c["K"], c["dist"]), one[1].cpu().numpy())


def test_undistort_identity_and_shift():
    src_np = _image(2, 120, 160, 3)
    src = torch.from_numpy(src_np).cuda()
    for mode in (0, 1):
        Lb.mi355cv_undistortSetKernel(mode)
        assert torch.equal(cv.undistort(src, K, None), src)
        newK = K.copy()
        newK[0, 2] += 3
        newK[1, 2] -= 2
        got = cv.undistort(src, K, None, newCameraMatrix=newK).cpu().numpy()
        want = np.zeros_like(src_np)
        want[:118, 3:] = src_np[2:, :157]
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- reprojectImageTo3D
Q = np.array([[1, 0, 0, -64], [0, 1, 0, -32], [0, 0, 0, 256], [0, 0, 0.25, 0]], np.float64)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.float32])
def test_reproject_depths_and_widths(dtype):
    rng = np.random.default_rng(4)
    for w in (1, 3, 4, 5, 255, 256, 257):
        d = rng.integers(0, 100, (9, w)).astype(dtype)
        for hm in (False, True):
            got = cv.reprojectImageTo3D(torch.from_numpy(d).cuda(), Q, hm)
            assert "k_reproject3d" in last_kernel()
            assert R.same_floats(got.cpu().numpy(), R.reproject(d, Q, hm)), (w, hm)
    assert R.same_floats(cv.reprojectImageTo3D(d, Q, True), R.reproject(d, Q, True))                       # numpy: staged
    parent = torch.full((12, 300 * 3), 7.0, device="cuda")
    out = torch.as_strided(parent, (9, 257, 3), (900, 3, 1), 903)
    cv.reprojectImageTo3D(torch.from_numpy(d).cuda(), Q, False, dst=out)                                  # a pitched, 4-byte aligned destination: the scalar stores
    assert "vec=0" in last_kernel() and R.same_floats(out.cpu().numpy(), R.reproject(d, Q)) and float(parent[0].min()) == 7.0 and float(parent[10:].min()) == 7.0


def test_reproject_batch_with_per_frame_minimum():
    rng = np.random.default_rng(6)
    d = rng.integers(10, 90, (3, 17, 70)).astype(np.int16)
    for f, m in enumerate((3, 7, 5)):                                                   # minima differ, each occurs several times
        d[f, 2, 3] = d[f, 9, 60] = d[f, 16, 69] = m
    got = cv.reprojectImageTo3DBatch(torch.from_numpy(d).cuda(), Q, True).cpu().numpy()
    for f in range(3):
        assert R.same_floats(got[f], R.reproject(d[f], Q, True)) and (got[f, ..., 2] == 10000).sum() == 3
    assert R.same_floats(cv.reprojectImageTo3DBatch(d, Q, True), got)                                      # host-resident frames through the shared pipeline
    f32 = d.astype(np.float32)
    f32[1, 0, 0] = np.nan
    got = cv.reprojectImageTo3DBatch(torch.from_numpy(f32).cuda(), Q, True).cpu().numpy()
    assert all(R.same_floats(got[f], R.reproject(f32[f], Q, True)) for f in range(3))


def test_reproject_straight_from_stereobm():
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (64, 160 + 8), dtype=np.uint8)
    left, right = torch.from_numpy(np.ascontiguousarray(base[:, 8:])).cuda(), torch.from_numpy(np.ascontiguousarray(base[:, :160])).cuda()
    disp = cv.StereoBM_create(16, 9).compute(left, right, disptype=cv.CV_32F)
    assert disp.is_cuda and disp.dtype == torch.float32
    Qs = np.array([[1, 0, 0, -80], [0, 1, 0, -32], [0, 0, 0, 533.25], [0, 0, 1 / 0.12, 0]], np.float64)
    pts = cv.reprojectImageTo3D(disp, Qs, True)
    assert pts.is_cuda and R.same_floats(pts.cpu().numpy(), R.reproject(disp.cpu().numpy(), Qs, True))
