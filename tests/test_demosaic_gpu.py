"""Bayer demosaicing on the MI355X (opencv_amd.demosaicing / demosaicingBatch / the Bayer codes of cvtColor -> mi355cv_demosaic / mi355cv_demosaicBatch,
opencv_amd/csrc/demosaic.hip) against the numpy restatement (tests/demosaic_restate.py), bit for bit.  Every call asserts that its call counter moved and that
mi355cv_lastKernel names the kernel expected for the shape: k_demosaic_roll for CV_8UC1 with at least 16 columns and a source whose base, pitch and frame stride
are multiples of 16 bytes (a last chunk of 1 .. 3 columns that opens a new strip of 64 chunks excepted), k_demosaic for everything else."""
import numpy as np
import pytest
import torch

import demosaic_restate as R

pytestmark = pytest.mark.gpu

ROLL, GENERIC = "k_demosaic_roll<", "k_demosaic<"
SEG = 7                                                     # rows per segment of the rolling kernel in a single call on a small image
CODE = {1: R.CODES_GRAY, 3: R.CODES_BGR, 4: R.CODES_BGRA}   # dcn -> the codes of BG, GB, RG, GR


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


def run(cv, src, code, kernel, **kw):
    n0 = cv.call_count("demosaic")
    got = cv.demosaicing(src, code, **kw)
    assert cv.call_count("demosaic") == n0 + 1, "the GPU path did not run"
    assert last_kernel(cv).startswith(kernel), last_kernel(cv)
    return got


def inputs(rng, dt, h, w):
    """random data, the depth's maximum, and the 0 / max checkerboards x&1, y&1, (x+y)&1: the inputs that would carry between packed halves"""
    top = np.iinfo(dt).max
    yy, xx = np.mgrid[0:h, 0:w]
    return [rng.integers(0, top + 1, (h, w)).astype(dt), np.full((h, w), top, dt)] + [(m * top).astype(dt) for m in (xx & 1, yy & 1, (xx + yy) & 1)]


def pitched(a, pitch):
    """`a` on the device as a view into rows of `pitch` elements (a 16-byte aligned base: the allocator's)"""
    h, w = a.shape
    parent = np.zeros((h, pitch), a.dtype)
    parent[:, :w] = a
    return to_dev(parent)[:, :w]


def cross_of_cases(cv, w, heights, pitch, kernel, seed):
    rng = np.random.default_rng(seed)
    for h in heights:
        for src in inputs(rng, np.uint8, h, w):
            dev = pitched(src, pitch) if pitch else to_dev(src)
            for dcn in (1, 3, 4):
                for p, name in enumerate(R.PATTERNS):
                    got = to_host(run(cv, dev, CODE[dcn][p], kernel))
                    assert np.array_equal(got, R.demosaic(src, name, dcn)), (w, h, dcn, name)


# ---- the rolling kernel, the full cross of widths x heights x patterns x dcn x input kinds.  Widths, each with a source pitch that is a multiple of 16 bytes:
# 16, 32, 48 the smallest; 17, 31, 33 a ragged last chunk; 1024 one full wave of chunks, 1040 one lane more (the wave-edge side load); 1039 and 1041 ragged on
# either side of it.  Heights: 3, 4, 5, then one below, at, one above and twice the rows of a segment, and one more (SEG is odd, so the second segment starts on an
# odd row and the pattern phase has to follow the absolute row; 2 * SEG + 1 leaves row h-1 alone in a third segment).
HEIGHTS = (3, 4, 5, SEG - 1, SEG, SEG + 1, 2 * SEG, 2 * SEG + 1)


@pytest.mark.parametrize("w", [16, 32, 48, 17, 31, 33, 1024, 1040, 1039, 1041])
def test_rolling_kernel(cv, w):
    cross_of_cases(cv, w, HEIGHTS, (w + 15) // 16 * 16, ROLL, w)


# ---- the other side of the width / alignment rule: below 16 columns; a pitch that is no multiple of 16 (the contiguous image of an odd width); 1025 columns,
# where the one-column last chunk would open the second strip
@pytest.mark.parametrize("w,pitch", [(15, 16), (3, 16), (17, 0), (31, 0), (1039, 0), (1025, 1040)])
def test_generic_kernel_next_to_the_rule(cv, w, pitch):
    cross_of_cases(cv, w, (3, 9), pitch, GENERIC, w)


def test_segment_length_is_what_the_heights_assume(cv):
    run(cv, to_dev(np.zeros((2 * SEG, 16), np.uint8)), cv.COLOR_BayerBG2BGR, ROLL)
    assert f"seg={SEG} rows x 2," in last_kernel(cv), last_kernel(cv)


# ---- CV_16U: the generic kernel
@pytest.mark.parametrize("w,h", [(3, 3), (5, 7), (37, 70)])
def test_16u(cv, w, h):
    rng = np.random.default_rng(w * h)
    for src in (rng.integers(0, 65536, (h, w)).astype(np.uint16), np.full((h, w), 65535, np.uint16)):
        dev = to_dev(src)
        for dcn in (1, 3, 4):
            for p, name in enumerate(R.PATTERNS):
                got = to_host(run(cv, dev, CODE[dcn][p], GENERIC))
                assert got.dtype == np.uint16 and np.array_equal(got, R.demosaic(src, name, dcn)), (w, h, dcn, name)


def test_known_answers_on_the_device(cv):
    def on_device(src, name, dcn, rgb=False):                                   # these images are narrower than 16 columns: the generic kernel
        p = R.PATTERNS.index(R.RGB_OF[name] if rgb else name)
        return to_host(run(cv, to_dev(src), CODE[dcn][p], GENERIC))
    R.known_answers(on_device)
    # the same answers through the rolling kernel: the 5 x 5 spike inside a 5 x 16 image of zeros (columns 0 .. 3 of the answer do not see the added columns)
    a = np.zeros((5, 16), np.uint8)
    a[2, 2] = 255
    got = to_host(run(cv, to_dev(a), cv.COLOR_BayerBG2BGR, ROLL))
    assert not got[..., 0].any() and not got[..., 1].any()
    assert got[:, :4, 2].tolist() == [[64, 64, 128, 64], [64, 64, 128, 64], [128, 128, 255, 128], [64, 64, 128, 64], [64, 64, 128, 64]] and not got[:, 4:, 2].any()
    for code, (centre, edge, corner) in ((cv.COLOR_BayerBG2GRAY, (76, 38, 19)), (cv.COLOR_BayerRG2GRAY, (29, 15, 7)), (cv.COLOR_BayerGB2GRAY, (150, 37, 0)),
                                         (cv.COLOR_BayerGR2GRAY, (150, 37, 0))):
        got = to_host(run(cv, to_dev(a), code, ROLL))
        assert np.array_equal(got[:, :4], R.cross(centre, edge, corner)[:, :4]) and not got[:, 4:].any()
    yy, xx = np.mgrid[0:4, 0:16]
    cb = (((xx + yy) & 1) * 255).astype(np.uint8)
    for p, bgr, gray in ((0, (0, 255, 0), 150), (2, (0, 255, 0), 150), (1, (255, 0, 255), 105), (3, (255, 0, 255), 105)):
        got = to_host(run(cv, to_dev(cb), R.CODES_BGR[p], ROLL))
        assert tuple(got[1, 1]) == bgr and tuple(got[1, 2]) == bgr
        got = to_host(run(cv, to_dev(cb), R.CODES_GRAY[p], ROLL))
        assert got[1, 1] == gray and got[1, 2] == gray
    m = np.full((4, 32), 255, np.uint8)
    for p in range(4):
        for dcn in (1, 3, 4):
            assert np.all(to_host(run(cv, to_dev(m), CODE[dcn][p], ROLL)) == 255)


# ---- views: the pattern is relative to the view; the destination's padding must survive
@pytest.mark.parametrize("w,h,pitch,x0,y0,kernel", [
    (48, 9, 64, 0, 1, ROLL),               # a view starting one row down: the pitch keeps it aligned, the phase is the view's
    (48, 9, 64, 16, 3, ROLL),
    (48, 9, 64, 1, 0, GENERIC),            # starting at an odd column: no longer aligned
    (48, 9, 64, 5, 1, GENERIC),
    (33, 8, 50, 16, 1, GENERIC),           # aligned start, but a pitch that is no multiple of 16
])
def test_source_views(cv, w, h, pitch, x0, y0, kernel):
    rng = np.random.default_rng(w + x0 + 7 * y0)
    parent = rng.integers(0, 256, (h + 4, pitch), dtype=np.uint8)
    dev = to_dev(parent)
    view = dev[y0:y0 + h, x0:x0 + w]
    src = parent[y0:y0 + h, x0:x0 + w]
    for dcn in (1, 3, 4):
        for p, name in enumerate(R.PATTERNS):
            assert np.array_equal(to_host(run(cv, view, CODE[dcn][p], kernel)), R.demosaic(src, name, dcn)), (dcn, name)


@pytest.mark.parametrize("dt,w,h,kernel", [(np.uint8, 48, 9, ROLL), (np.uint8, 33, 9, ROLL), (np.uint8, 21, 6, GENERIC), (np.uint16, 21, 6, GENERIC)])
def test_destination_with_padded_rows(cv, dt, w, h, kernel):
    rng = np.random.default_rng(w)
    top = np.iinfo(dt).max
    src = rng.integers(0, top + 1, (h, w)).astype(dt)
    dev = pitched(src, 48) if kernel == ROLL else to_dev(src)
    for dcn in (1, 3, 4):
        shape = (h + 2, w + 5) if dcn == 1 else (h + 2, w + 5, dcn)
        sentinel = rng.integers(0, top + 1, shape).astype(dt)
        dp = to_dev(sentinel)
        dview = dp[1:1 + h, 3:3 + w]
        out = run(cv, dev, CODE[dcn][2], kernel, dst=dview)
        assert out is dview
        got = to_host(dp)
        assert np.array_equal(got[1:1 + h, 3:3 + w], R.demosaic(src, "RG", dcn))
        mask = np.ones(sentinel.shape[:2], bool)
        mask[1:1 + h, 3:3 + w] = False
        assert np.array_equal(got[mask], sentinel[mask])                         # nothing outside the view written


# ---- batches: one launch, equal frame by frame to the single call
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("dt,w,h,kernel", [(np.uint8, 48, 2 * SEG + 1, ROLL), (np.uint8, 1041, 5, ROLL), (np.uint8, 21, 7, GENERIC), (np.uint16, 21, 7, GENERIC)])
def test_batch_equals_per_frame(cv, n, dt, w, h, kernel):
    rng = np.random.default_rng(w * h + n)
    top = np.iinfo(dt).max
    pitch = (w + 15) // 16 * 16 if kernel == ROLL else w + 3
    frames = rng.integers(0, top + 1, (n, h, w)).astype(dt)                     # random: the frames differ at their edges
    # source and destination frames further apart than a frame is long; the gaps must survive
    sparent = np.zeros((n, h + 2, pitch), dt)
    sparent[:, :h, :w] = frames
    sview = to_dev(sparent)[:, :h, :w]
    for dcn in (1, 3, 4):
        tail = () if dcn == 1 else (dcn,)
        sentinel = rng.integers(0, top + 1, (n, h + 3, w + 2) + tail).astype(dt)
        dparent = to_dev(sentinel)
        dview = dparent[:, :h, :w]
        n0 = cv.call_count("demosaicBatch")
        out = cv.demosaicingBatch(sview, CODE[dcn][1], dst=dview)
        assert out is dview and cv.call_count("demosaicBatch") == n0 + 1 and last_kernel(cv).startswith(kernel), last_kernel(cv)
        got = to_host(dparent)
        for i in range(n):
            single = to_host(run(cv, sview[i], CODE[dcn][1], kernel))
            assert np.array_equal(got[i, :h, :w], single), (dcn, i)
            assert np.array_equal(single, R.demosaic(frames[i], "GB", dcn)), (dcn, i)
        mask = np.ones(sentinel.shape[:3], bool)
        mask[:, :h, :w] = False
        assert np.array_equal(got[mask], sentinel[mask])
    if kernel == ROLL:                                                          # a fresh destination, through cvtColorBatch
        n0 = cv.call_count("demosaicBatch")
        out = cv.cvtColorBatch(sview, cv.COLOR_BayerGR2RGB)
        assert cv.call_count("demosaicBatch") == n0 + 1 and tuple(out.shape) == (n, h, w, 3)
        for i in range(n):
            assert np.array_equal(to_host(out[i]), R.demosaic(frames[i], "GR", 3, rgb=True)), i


def test_host_resident_inputs_are_staged(cv):
    rng = np.random.default_rng(31)
    src = rng.integers(0, 256, (12, 64), dtype=np.uint8)
    got = run(cv, src, cv.COLOR_BayerBG2BGR, ROLL)                              # staged into aligned device buffers
    assert isinstance(got, np.ndarray) and np.array_equal(got, R.demosaic(src, "BG", 3))
    frames = rng.integers(0, 256, (5, 12, 64), dtype=np.uint8)
    n0 = cv.call_count("demosaicBatch")
    out = cv.demosaicingBatch(torch.from_numpy(frames).pin_memory(), cv.COLOR_BayerRG2GRAY)
    assert cv.call_count("demosaicBatch") > n0 and not out.is_cuda
    for i in range(5):
        assert np.array_equal(out[i].numpy(), R.demosaic(frames[i], "RG", 1)), i


# ---- the Python surface
def test_python_surface(cv):
    rng = np.random.default_rng(41)
    src = rng.integers(0, 256, (10, 32), dtype=np.uint8)
    dev = to_dev(src)
    n0 = cv.call_count("demosaic")
    a = to_host(cv.cvtColor(dev, cv.COLOR_BayerRG2RGB))
    b = to_host(cv.demosaicing(dev, cv.COLOR_BayerBG2BGR))
    assert cv.call_count("demosaic") == n0 + 2
    assert np.array_equal(a, b) and np.array_equal(a, R.demosaic(src, "RG", 3, rgb=True))
    for p, name in enumerate(R.PATTERNS):
        rgb = to_host(run(cv, dev, getattr(cv, f"COLOR_Bayer{name}2RGB"), ROLL))
        assert np.array_equal(rgb, R.demosaic(src, name, 3, rgb=True)), name
        rgba = to_host(run(cv, dev, getattr(cv, f"COLOR_Bayer{name}2RGBA"), ROLL))
        assert np.array_equal(rgba, R.demosaic(src, name, 4, rgb=True)), name
        four = to_host(run(cv, dev, R.CODES_BGR[p], ROLL, dstCn=4))             # dstCn = 4 on a ...2BGR code
        assert four.shape == (10, 32, 4) and np.array_equal(four, R.demosaic(src, name, 4)), name
        three = to_host(cv.cvtColor(dev, R.CODES_BGRA[p], dstCn=3))
        assert np.array_equal(three, R.demosaic(src, name, 3)), name
        gray = to_host(cv.cvtColor(dev, R.CODES_GRAY[p], dstCn=3))              # gray stays one channel
        assert gray.shape == (10, 32) and np.array_equal(gray, R.demosaic(src, name, 1)), name
    n0 = cv.call_count("demosaic")
    for code in R.CODES_VNG + R.CODES_EA:
        with pytest.raises(NotImplementedError):
            cv.demosaicing(dev, code)
        with pytest.raises(NotImplementedError):
            cv.cvtColor(dev, code)
    with pytest.raises(NotImplementedError):                                    # source and destination overlapping in HBM
        buf = torch.zeros((10, 32 * 4), dtype=torch.uint8, device="cuda")
        cv.demosaicing(buf[:, :32], cv.COLOR_BayerBG2GRAY, dst=buf[:, 16:48])
    assert cv.call_count("demosaic") == n0
