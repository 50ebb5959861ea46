"""cv::filterSpeckles without a GPU: the three forms of the restatement (tests/speckle_restate.py) against each other bit for bit, answers worked out by hand or known by
construction, the lines of opencv_amd/csrc/speckle_math.h compiled for the host with both kernel sequences emulated around them (tests/hostemu/speckle_emu.cpp) against
the restatement, the refusals of the mi355cv_filterSpeckles* entries that come before any device is touched, the limits and the Python surface."""
import ctypes
import functools
import os

import numpy as np
import pytest

import emubuild
import speckle_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = (R.filter_scan, R.filter_graph, R.filter_np)
SHAPES = [(1, 1), (1, 7), (1, 13), (6, 1), (13, 1), (2, 2), (3, 5), (5, 4), (7, 7), (9, 12), (12, 9), (13, 13)]


def random_cases(seed, shapes=SHAPES, per_shape=4):
    """(image, newVal, maxSpeckleSize, maxDiff): both depths, few-level values so that chains of links occur, newVal among the values, sizes 0 .. 11, maxDiff 0 .. 3"""
    rng = np.random.default_rng(seed)
    for H, W in shapes:
        for dtype in (np.uint8, np.int16):
            for _ in range(per_shape):
                img, nv = R.few_levels(rng, H, W, dtype)
                yield img, nv, int(rng.integers(0, 12)), int(rng.integers(0, 4))


def test_the_three_forms_of_the_restatement_agree():
    changed = total = 0
    for img, nv, S, md in random_cases(1):
        outs = [f(img, nv, S, md) for f in FORMS]
        for o in outs[1:]:
            assert o.dtype == img.dtype and np.array_equal(o, outs[0]), (img.shape, img.dtype, nv, S, md)
        total += 1
        changed += int(not np.array_equal(outs[0], img))
    assert total >= 90 and changed >= total // 2, (total, changed)           # the cases do exercise the erase
    # no links at all, nothing erased, and a size that takes everything
    img, nv = R.few_levels(np.random.default_rng(2), 9, 11, np.int16)
    for f in FORMS:
        assert np.array_equal(f(img, nv, 0, 3), img) and np.array_equal(f(img, nv, -5, 3), img)
        assert (f(img, nv, 1, -1) == nv).all()                              # maxDiff < 0: every live pixel is a component of one
        assert (f(img, nv, img.size, 1 << 20) == nv).all()


def test_links_are_not_transitive_in_the_values():
    row = np.array([[0, 1, 2, 9, 4, 3]], np.uint8)                            # 0-1-2 is one component with maxDiff = 1 although |0 - 2| = 2; 4-3 another
    for f in FORMS:
        assert f(row, 200, 2, 1).tolist() == [[0, 1, 2, 200, 200, 200]]
        assert f(row, 200, 3, 1).tolist() == [[200] * 6]
        assert f(row, 200, 1, 0).tolist() == [[200] * 6]


def test_planted_blobs():
    img, want, changed = R.planted()
    assert img.shape == (48, 160) and changed == 35 and int((img != want).sum()) == 35
    for f in (R.filter_graph, R.filter_np):
        assert np.array_equal(f(img, -16, R.PLANTED_S, 16), want)
    from opencv_amd import _lib
    img, want, changed = R.planted_seams(_lib.limit("speckle_tile_cols"), _lib.limit("speckle_tile_rows"))
    assert changed == 35 and int((img != want).sum()) == 35
    assert np.array_equal(R.filter_graph(img, -16, R.PLANTED_S, 16), want)


def test_ramp():
    img = R.ramp()
    gone = np.full_like(img, -16)
    for md, S, want in ((16, 639, img), (16, 640, gone), (15, 3, img), (15, 4, gone)):
        for f in (R.filter_graph, R.filter_np):
            assert np.array_equal(f(img, -16, S, md), want), (md, S)


def test_extremes_of_the_depths():
    pair = np.array([[-32768, 32767]], np.int16)
    for f in FORMS:
        assert f(pair, 0, 1, 65534).tolist() == [[0, 0]]                      # no link: two components of one
        assert f(pair, 0, 1, 65535).tolist() == [[-32768, 32767]]             # a link: one component of two
        assert f(pair, 0, 2, 65535).tolist() == [[0, 0]]
        assert f(pair, -32768, 1, 65535).tolist() == [[-32768, -32768]]       # newVal at the depth's end: only the other pixel is live
    b = np.array([[0, 255, 255], [0, 0, 255], [7, 0, 0]], np.uint8)
    for f in FORMS:
        assert f(b, 0, 1, 0).tolist() == [[0, 255, 255], [0, 0, 255], [0, 0, 0]]           # newVal 0: the zeros are not live, the 7 goes
        assert f(b, 255, 1, 0).tolist() == [[0, 255, 255], [0, 0, 255], [255, 0, 0]]       # newVal 255: the zeros are a component of five
        assert f(b, 255, 5, 0).tolist() == [[255] * 3] * 3


def test_serpentine_and_spiral_are_one_component():
    for H, W in ((5, 9), (6, 9), (9, 5), (12, 17)):
        for img, n in (R.serpentine(H, W, np.int16, 40, -1), R.serpentine(H, W, np.int16, 40, -1, transpose=True), R.spiral(H, W, np.uint8, 9, 200)):
            fg, bg = int(img[0, 0]), int(img.max() if img.dtype == np.uint8 else img.min())
            assert n == int((img == fg).sum()) and n > max(H, W)
            assert np.array_equal(R.filter_graph(img, bg, n - 1, 0), img)
            assert (R.filter_graph(img, bg, n, 0) == bg).all()


@functools.lru_cache(maxsize=1)
def emu():
    lib = emubuild.load("speckle_emu.cpp", "libspeckle_emu.so")
    i32, vp = ctypes.c_int, ctypes.c_void_p
    lib.emu_spk_filter.argtypes = [vp, ctypes.c_size_t, i32, i32, i32, i32, i32, i32, i32, i32]
    lib.emu_spk_filter.restype = None
    lib.emu_spk_runlen.argtypes = [ctypes.c_ulonglong, i32]
    return lib


def emu_filter(img, nv, S, md, fast, stride=1):
    """the emulated kernel sequence on a pitched copy inside a guarded buffer"""
    E = emu()
    H, W = img.shape
    guard = 77 if img.dtype == np.uint8 else -7777
    buf = np.full((H + 2, W + 5), guard, img.dtype)
    buf[1:H + 1, 3:W + 3] = img
    view = buf[1:H + 1, 3:W + 3]
    E.emu_spk_filter(view.ctypes.data, view.strides[0], W, H, int(img.dtype == np.int16), nv, S, md, fast, stride)
    out = view.copy()
    buf[1:H + 1, 3:W + 3] = guard
    assert (buf == guard).all(), "bytes outside the view were written"
    return out


def test_speckle_math_on_the_host_matches_the_restatement():
    TW, TH = emu().emu_spk_limit(1), emu().emu_spk_limit(2)
    cases = list(random_cases(3, per_shape=2))
    rng = np.random.default_rng(4)
    for H, W in ((TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 3), (TH - 1, TW - 1), (TH, TW), (1, 2 * TW + 3), (2 * TH + 3, 1)):
        for dtype in (np.uint8, np.int16):
            img, nv = R.few_levels(rng, H, W, dtype)
            cases.append((img, nv, int(rng.integers(0, 12)), int(rng.integers(0, 4))))
    H, W = 2 * TH + 3, 2 * TW + 3                                            # paths through every emulated tile, each crossing the seams
    for img, n in (R.serpentine(H, W, np.int16, 40, -1), R.serpentine(H, W, np.int16, 40, -1, transpose=True), R.spiral(H, W, np.int16, 40, -1),
                   R.serpentine(H, W, np.uint8, 9, 200), R.spiral(H, W, np.uint8, 9, 200)):
        bg = int(img[1, 1])
        cases += [(img, bg, n - 1, 0), (img, bg, n, 0)]
        live_bg = img.copy()
        live_bg[img == bg] = 100                                              # the gaps live too but far in value: held apart by the predicate alone
        cases.append((live_bg, bg, n - 1, 5))
    img, want, _ = R.planted_seams(TW, TH)
    cases.append((img, -16, R.PLANTED_S, 16))
    cases.append((np.array([[-32768, 32767]], np.int16), 0, 1, 65534))
    cases.append((np.array([[-32768, 32767]], np.int16), 0, 1, 65535))
    cases.append((R.checkerboard(TH + 2, TW + 2, np.uint8, 3, 4), 0, 1, 0))
    changed = 0
    for img, nv, S, md in cases:
        want = R.filter_graph(img, nv, S, md)
        changed += int(not np.array_equal(want, img))
        for fast in (0, 1):
            for stride in (1, 7):
                got = emu_filter(img, nv, S, md, fast, stride)
                bad = np.argwhere(got != want)
                assert not len(bad), (img.shape, img.dtype, nv, S, md, fast, stride, len(bad), bad[:4].tolist())
    assert changed >= len(cases) // 3
    assert np.array_equal(emu_filter(R.planted_seams(TW, TH)[0], -16, R.PLANTED_S, 16, 1), R.planted_seams(TW, TH)[1])
    E = emu()
    assert E.emu_spk_linked(-32768, 32767, 65534) == 0 and E.emu_spk_linked(-32768, 32767, 65535) == 1 and E.emu_spk_linked(5, 5, -1) == 0
    assert E.emu_spk_linked(0, 2, 1) == 0 and E.emu_spk_linked(2, 1, 1) == 1
    assert [E.emu_spk_fits(v, 0) for v in (-1, 0, 255, 256)] == [0, 1, 1, 0] and [E.emu_spk_fits(v, 1) for v in (-32769, -32768, 32767, 32768)] == [0, 1, 1, 0]
    assert E.emu_spk_runlen(0, 0) == 1 and E.emu_spk_runlen(0xfffffffffffffffe, 0) == 64 and E.emu_spk_runlen(0b0110, 0) == 3 and E.emu_spk_runlen(1 << 63, 62) == 2
    assert E.emu_spk_runlen(0, 63) == 1 and E.emu_spk_runlen(0b0110, 3) == 1


LIMITS = {"speckle_max_dim": 16384, "speckle_tile_cols": 256, "speckle_tile_rows": 16}


def test_limits_are_pinned():
    """how far filterSpeckles was built; tests/test_speckle_gpu.py derives its shapes from mi355cv_limit"""
    from opencv_amd import _lib
    E = emu()
    for i, (k, v) in enumerate(LIMITS.items()):
        assert _lib.limit(k) == v == E.emu_spk_limit(i), k


def test_refusals_before_a_device_is_touched():
    from opencv_amd import _lib
    Lb, NI, top = _lib.lib, _lib.NOT_IMPLEMENTED, _lib.limit
    reason = lambda: Lb.mi355cv_lastError().decode()
    H, W = 24, 40
    buf = np.full((3, H, W), 1234, np.int16)
    big = top("speckle_max_dim") + 1

    def call(ptr=buf.ctypes.data, step=2 * W, W=W, H=H, depth=3, newVal=-16, batch=None, fstride=2 * W * H):
        if batch is not None:
            return Lb.mi355cv_filterSpecklesBatch(ptr, step, fstride, batch, W, H, depth, newVal, 10, 16)
        return Lb.mi355cv_filterSpeckles(ptr, step, W, H, depth, newVal, 10, 16)

    cases = [
        (dict(depth=2), "neither CV_8UC1 nor CV_16SC1"), (dict(depth=1), "neither CV_8UC1 nor CV_16SC1"), (dict(depth=5), "neither CV_8UC1 nor CV_16SC1"),
        (dict(ptr=None), "!img"), (dict(ptr=None, batch=2), "!img"),
        (dict(batch=0), "nframes < 1"), (dict(batch=-3), "nframes < 1"),
        (dict(W=0), "W < 1"), (dict(H=0), "H < 1"), (dict(W=-4), "W < 1"),
        (dict(W=big, step=2 * big), "SPECKLE_MAX_DIM"), (dict(H=big), "SPECKLE_MAX_DIM"),
        (dict(step=2 * W - 2), "step < rowBytes"), (dict(depth=0, step=W - 1), "step < rowBytes"),
        (dict(step=2 * W + 1), "off their element's boundary"), (dict(ptr=buf.ctypes.data + 1), "off their element's boundary"),
        (dict(batch=2, fstride=2 * W * H + 1), "off their element's boundary"),
        (dict(newVal=32768), "outside the range of the image's depth"), (dict(newVal=-32769), "outside the range of the image's depth"),
        (dict(depth=0, step=W, newVal=256), "outside the range of the image's depth"), (dict(depth=0, step=W, newVal=-1), "outside the range of the image's depth"),
        (dict(batch=2, fstride=2 * W * H - 2), "frames of the batch overlap"), (dict(batch=3, fstride=0), "frames of the batch overlap"),
        (dict(batch=2, step=4 * W, fstride=4 * W * (H - 1)), "frames of the batch overlap"),
    ]
    for kw, why in cases:
        assert call(**kw) == NI, kw
        assert why in reason(), (kw, reason())
    assert (buf == 1234).all()
    # the ledger is kept by the layer above the C ABI: the Python mirror counts a decline of the entry under its name, with the entry's reason
    import opencv_amd as cv
    n0, b0, all0 = _lib.decline_count("filterSpeckles"), _lib.decline_count("filterSpecklesBatch"), _lib.decline_count()
    with pytest.raises(NotImplementedError, match="outside the range of the image's depth"):
        cv.filterSpeckles(buf[0], 32768, 10, 16)
    with pytest.raises(NotImplementedError, match="frames of the batch overlap"):
        cv.filterSpecklesBatch(np.broadcast_to(buf[0], (3, H, W)), -16, 10, 16)
    assert (_lib.decline_count("filterSpeckles"), _lib.decline_count("filterSpecklesBatch"), _lib.decline_count()) == (n0 + 1, b0 + 1, all0 + 2)
    assert (buf == 1234).all()
    assert Lb.mi355cv_filterSpecklesSetKernel(1) == -1 and Lb.mi355cv_filterSpecklesSetKernel(-2) == -1
    assert Lb.mi355cv_filterSpecklesSetKernel(0) == 0 and Lb.mi355cv_filterSpecklesSetKernel(-1) == 0


def test_python_surface():
    import opencv_amd as cv
    from opencv_amd import _lib
    for name in ("filterSpeckles", "filterSpecklesBatch"):
        assert name in cv.calib3d.__all__ and hasattr(cv, name), name
    txt = open(os.path.join(ROOT, "include", "mi355cv.h")).read()
    for name in ("mi355cv_filterSpeckles", "mi355cv_filterSpecklesBatch", "mi355cv_filterSpecklesSetKernel"):
        assert name + "(" in txt and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    img = np.zeros((8, 12), np.int16)
    n0 = _lib.decline_count("filterSpeckles")
    for bad in (np.zeros((8, 12), np.uint16), np.zeros((8, 12), np.float32), np.zeros((8, 12), np.int32)):
        with pytest.raises(NotImplementedError, match="neither CV_8UC1 nor CV_16SC1"):
            cv.filterSpeckles(bad, 0, 4, 1)
    with pytest.raises(NotImplementedError, match="neither CV_8UC1 nor CV_16SC1"):
        cv.filterSpecklesBatch(np.zeros((2, 8, 12), np.float32), 0, 4, 1)
    assert _lib.decline_count("filterSpeckles") == n0 + 3
    with pytest.raises(NotImplementedError, match="outside the range"):
        cv.filterSpeckles(img, 40000, 4, 1, buf=np.zeros(4, np.uint8))        # buf is accepted; the decline is the C entry's
    assert _lib.decline_count("filterSpeckles") == n0 + 4
    assert (img == 0).all()
    for bad in (np.zeros((2, 8, 12), np.int16), np.zeros(12, np.int16), [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="H x W"):
            cv.filterSpeckles(bad, 0, 4, 1)
    for bad in (img, np.zeros((0, 8, 12), np.int16)):
        with pytest.raises(ValueError, match="N x H x W"):
            cv.filterSpecklesBatch(bad, 0, 4, 1)
    with pytest.raises(ValueError, match="finite numbers"):
        cv.filterSpeckles(img, float("nan"), 4, 1)
    with pytest.raises(ValueError, match="dense"):
        cv.filterSpeckles(np.zeros((8, 24), np.int16)[:, ::2], 0, 4, 1)
