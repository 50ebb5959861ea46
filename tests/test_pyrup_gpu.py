"""pyrUp on the MI355X (opencv_amd.pyrUp / pyrUpBatch -> mi355cv_pyrup / mi355cv_pyrupBatch, opencv_amd/csrc/pyrup.hip) against the numpy restatement
(tests/pyrup_restate.py): integers bit for bit, CV_32F within orc.rel_err <= 1e-6 (the bar float pyrDown is held to).  Every call asserts that its call counter
moved and that mi355cv_lastKernel names the kernel expected for the shape: k_pyrup_roll for CV_8UC1 with a width divisible by 8 and aligned rows, k_pyrup else."""
import numpy as np
import pytest
import torch

import orc
import pyrup_restate as R

pytestmark = pytest.mark.gpu

ROLL, GENERIC = "k_pyrup_roll<", "k_pyrup<"


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return opencv_amd


def to_torch(a):
    if a.dtype == np.uint16:                              # moved as int16 bits, viewed back as uint16
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.uint16)
    return torch.from_numpy(np.ascontiguousarray(a))


def to_dev(a):
    return to_torch(a).cuda()


def to_host(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def last_kernel(cv):
    return cv._lib.lib.mi355cv_lastKernel().decode()


def run(cv, src, kernel, **kw):
    n0 = cv.call_count("pyrup")
    got = cv.pyrUp(src, **kw)
    assert cv.call_count("pyrup") == n0 + 1, "the GPU path did not run"
    assert last_kernel(cv).startswith(kernel), last_kernel(cv)
    return got


def data(rng, dt, shape, kind="full"):
    if dt == np.float32:
        return (rng.random(shape) if kind == "unit" else rng.uniform(-1000, 1000, shape)).astype(np.float32)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, shape).astype(dt)


def check(got, src):
    want = R.pyrUp(src)
    assert got.shape == want.shape and got.dtype == want.dtype
    if src.dtype == np.float32:
        assert orc.rel_err(got, want) <= 1e-6
    else:
        assert np.array_equal(got, want)


# ---- the rolling kernel: widths 8 / 16 / 24 (the smallest it takes), 1032 = two full waves of 8-byte chunks plus one lane; one step either side of
# the width rule goes to the generic kernel.  Heights 1, 2, 3, 7 and 37: a single call runs segments of 4 source rows, so 7 spans two (the second one
# ragged) and 37 ten.
@pytest.mark.parametrize("w,kernel", [(8, ROLL), (16, ROLL), (24, ROLL), (1032, ROLL), (7, GENERIC), (9, GENERIC), (15, GENERIC), (17, GENERIC), (1031, GENERIC),
                                      (1033, GENERIC), (1036, GENERIC)])
def test_8uc1_widths_and_heights(cv, w, kernel):
    rng = np.random.default_rng(w)
    for h in (1, 2, 3, 7, 37):
        yy, xx = np.mgrid[0:h, 0:w]
        # all-255 and the 0 / 255 checkerboards are the inputs that would expose a carry between the packed 16-bit halves
        for src in (data(rng, np.uint8, (h, w)), np.full((h, w), 255, np.uint8), (((xx + yy) & 1) * 255).astype(np.uint8), ((xx & 1) * 255).astype(np.uint8)):
            got = to_host(run(cv, to_dev(src), kernel))
            assert np.array_equal(got, R.pyrUp(src)), (w, h)


def test_known_answers_on_the_device(cv):
    a = np.zeros((5, 5), np.uint8)
    a[2, 2] = 255
    got = to_host(run(cv, to_dev(a), GENERIC))
    assert got[4, 2:7].tolist() == [24, 96, 143, 96, 24] and got[2, 2:7].tolist() == [4, 16, 24, 16, 4] and int(got.sum()) == int(R.pyrUp(a).sum())
    assert to_host(run(cv, to_dev(np.array([[0, 255]], np.uint8)), GENERIC)).tolist() == [[64, 128, 223, 255]] * 2
    assert to_host(run(cv, to_dev(np.array([[-32768, 32767, -1]], np.int16)), GENERIC)).tolist() == [[-16384, 0, 20479, 16383, 4095, -1]] * 2
    assert np.all(to_host(run(cv, to_dev(np.full((9, 16), 201, np.uint8)), ROLL)) == 201)


# ---- more source rows than one launch of the generic kernel covers (grid.y holds 65535 blocks of 4 rows): it takes two; the rolling kernel's segments
# are spread over grid.x.  Structured rows, so that a row written from the wrong source row shows.
@pytest.mark.parametrize("w,kernel", [(3, GENERIC), (8, ROLL)])
def test_taller_than_one_grid(cv, w, kernel):
    h = 4 * 65535 + 3
    src = ((np.arange(h)[:, None] * 7 + np.arange(w)[None, :] * 31) % 251).astype(np.uint8)
    assert np.array_equal(to_host(run(cv, to_dev(src), kernel)), R.pyrUp(src))


# ---- the generic kernel
SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (5, 3), (31, 7), (65, 49)]               # (w, h)


@pytest.mark.parametrize("dt,kind", [(np.uint8, "full"), (np.uint16, "full"), (np.int16, "full"), (np.float32, "unit"), (np.float32, "pm1000")])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_generic_kernel(cv, dt, kind, cn):
    rng = np.random.default_rng(cn * 7 + np.dtype(dt).itemsize)
    for w, h in SIZES:
        src = data(rng, dt, (h, w) if cn == 1 else (h, w, cn), kind)
        check(to_host(run(cv, to_dev(src), GENERIC)), src)
    if dt != np.float32:                                                          # the extremes of the type stay what they are
        for v in (np.iinfo(dt).min, np.iinfo(dt).max):
            src = np.full((5, 9) if cn == 1 else (5, 9, cn), v, dt)
            assert np.all(to_host(run(cv, to_dev(src), GENERIC)) == v)


# ---- views into wider parents; the destination's parent is filled with a sentinel that must survive
@pytest.mark.parametrize("dt,cn,w,h,spitch,dpitch,sx,dx,kernel", [
    (np.uint8, 1, 40, 11, 64, 160, 8, 16, ROLL),            # aligned views: the rolling kernel
    (np.uint8, 1, 40, 11, 64, 100, 8, 16, GENERIC),         # a destination pitch that is no multiple of 16
    (np.uint8, 1, 40, 11, 64, 160, 3, 16, GENERIC),         # a source that does not start on 8 bytes
    (np.uint8, 1, 37, 11, 61, 99, 5, 7, GENERIC),
    (np.int16, 3, 21, 6, 30, 70, 2, 5, GENERIC),
    (np.float32, 1, 33, 9, 50, 90, 1, 3, GENERIC),
])
def test_views_and_pitches(cv, dt, cn, w, h, spitch, dpitch, sx, dx, kernel):
    rng = np.random.default_rng(w + dpitch)
    tail = () if cn == 1 else (cn,)
    sparent = data(rng, dt, (h + 4, spitch) + tail, "pm1000")
    sentinel = data(rng, dt, (2 * h + 5, dpitch) + tail, "pm1000")
    sp, dp = to_dev(sparent), to_dev(sentinel)
    sview, dview = sp[2:2 + h, sx:sx + w], dp[3:3 + 2 * h, dx:dx + 2 * w]
    out = run(cv, sview, kernel, dst=dview)
    assert out is dview
    got = to_host(dp)
    src = sparent[2:2 + h, sx:sx + w]
    check(np.ascontiguousarray(got[3:3 + 2 * h, dx:dx + 2 * w]), src)
    mask = np.ones(sentinel.shape[:2], bool)
    mask[3:3 + 2 * h, dx:dx + 2 * w] = False
    assert np.array_equal(got[mask], sentinel[mask])                             # nothing outside the view written


# ---- batches: one launch, equal frame by frame to the single call
@pytest.mark.parametrize("dt,cn,w,h,kernel", [(np.uint8, 1, 48, 9, ROLL), (np.uint8, 1, 1032, 6, ROLL), (np.uint8, 3, 31, 7, GENERIC), (np.float32, 1, 31, 7, GENERIC),
                                              (np.uint16, 4, 10, 5, GENERIC)])
def test_batch_equals_per_frame(cv, dt, cn, w, h, kernel):
    rng = np.random.default_rng(w * h)
    frames = np.stack([data(rng, dt, (h, w) if cn == 1 else (h, w, cn), "pm1000") for _ in range(5)])      # random: the frames differ at their edges
    dev = to_dev(frames)
    n0 = cv.call_count("pyrupBatch")
    out = cv.pyrUpBatch(dev)
    assert cv.call_count("pyrupBatch") == n0 + 1 and last_kernel(cv).startswith(kernel), last_kernel(cv)
    assert tuple(out.shape) == (5, 2 * h, 2 * w) + frames.shape[3:]
    for i in range(5):
        single = to_host(run(cv, dev[i], kernel))
        assert np.array_equal(to_host(out[i]), single), i
        check(single, frames[i])


def test_host_resident_batch_goes_through_the_pipeline(cv):
    rng = np.random.default_rng(21)
    frames = data(rng, np.uint8, (5, 36, 64))
    n0 = cv.call_count("pyrupBatch")
    out = cv.pyrUpBatch(torch.from_numpy(frames).pin_memory())
    assert cv.call_count("pyrupBatch") > n0 and not out.is_cuda
    assert last_kernel(cv).startswith(ROLL), last_kernel(cv)                      # 64 wide, staged into aligned device buffers
    for i in range(5):
        assert np.array_equal(out[i].numpy(), R.pyrUp(frames[i])), i


def test_numpy_host_input_is_staged(cv):
    rng = np.random.default_rng(22)
    for dt, shape in ((np.uint8, (48, 64)), (np.int16, (19, 23, 3)), (np.float32, (19, 23))):
        src = data(rng, dt, shape, "unit")
        got = run(cv, src, "k_pyrup")
        assert isinstance(got, np.ndarray)
        check(got, src)


def test_round_trip_with_pyrdown(cv):
    rng = np.random.default_rng(23)
    x = data(rng, np.uint8, (48, 64))
    down = cv.pyrDown(to_dev(x))
    assert np.array_equal(to_host(down), orc.orc_pyrDown(x))
    up = run(cv, down, ROLL)
    assert np.array_equal(to_host(up), R.pyrUp(orc.orc_pyrDown(x)))


def test_python_refusals(cv):
    d = to_dev(np.zeros((8, 16), np.uint8))
    with pytest.raises(ValueError):
        cv.pyrUp(d, borderType=cv.BORDER_REPLICATE)
    n0 = cv.call_count("pyrup")
    with pytest.raises(NotImplementedError):
        cv.pyrUp(d, dstsize=(33, 16))
    assert cv.call_count("pyrup") == n0
    assert to_host(run(cv, d, ROLL, dstsize=(32, 16))).shape == (16, 32) and to_host(run(cv, d, ROLL, dstsize=(0, 0))).shape == (16, 32)
