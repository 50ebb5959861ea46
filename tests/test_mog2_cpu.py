"""BackgroundSubtractorMOG2 without a GPU: hand-computed known answers for the two restatements (tests/mog2_restate.py), the two against each other on sequences
that take every branch of the update (the loops version counts them), the lines of opencv_amd/csrc/mog2_math.h compiled for the host (tests/hostemu/mog2_emu.cpp)
against them bit for bit, the refusals of the mi355cv_mog2* entries that come before any device is touched, and the two limits."""
import ctypes
import functools
import os

import numpy as np
import pytest

import emubuild
import mog2_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_IMPLEMENTED = 0, 1
F = np.float32
IMPLS = ["loops", "vec"]
# (h, w, cn, dtype, nmixtures): at most 17 x 23, both channel counts, both input types
SEQS = [(5, 7, 1, np.uint8, 5), (4, 5, 3, np.uint8, 5), (3, 5, 1, np.float32, 5), (3, 4, 3, np.float32, 5), (6, 5, 1, np.uint8, 3), (4, 3, 3, np.uint8, 1),
        (3, 3, 1, np.float32, 1), (2, 5, 3, np.float32, 3)]
HISTORY = 6


def P(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- known answers
@pytest.mark.parametrize("impl", IMPLS)
def test_known_answers_on_one_pixel(impl):
    px = np.array([[100]], np.uint8)
    # first frame: one mode of weight 1 and variance varInit, foreground: 255.  With detectShadows the stated algorithm tests the pixel against the UPDATED model, whose
    # only mode is the pixel itself (a = 1, distance 0): 127.  DESIGN 6.14 records the doubt about the issue's "mask 255", which holds as stated without shadows.
    assert R.Mog2(impl, detectShadows=False).apply(px)[0, 0] == 255
    m = R.Mog2(impl)
    assert m.apply(px)[0, 0] == 127
    modes, gmm, mean = m.export()
    assert modes[0, 0] == 1 and gmm[0, 0, 0, 0] == F(1) and gmm[0, 0, 0, 1] == F(15) and mean[0, 0, 0, 0] == F(100)
    assert not gmm[0, 0, 1:].any() and not mean[0, 0, 1:].any()
    assert m.apply(px)[0, 0] == 0                                         # the same value again: background
    # alphaT = 1/4: w = 0.75 * 1 - 0.25 * 0.05 + 0.25 = 0.9875, normalised to 1; k = 0.25 / 0.9875; variance 15 - k * 15
    modes, gmm, mean = m.export()
    w = F(0.75) * F(1) + -(F(0.25) * F(0.05)) + F(0.25)
    k = F(0.25) / w
    assert modes[0, 0] == 1 and gmm[0, 0, 0, 0] == w * (F(1) / w) and gmm[0, 0, 0, 1] == F(15) + k * (F(0) - F(15)) and mean[0, 0, 0, 0] == F(100)
    before = m.export()
    assert m.apply(px, 0)[0, 0] == 0                                      # learningRate 0: the model stays bit-identical
    assert R.same_model(before, m.export()) and m.nframes == 3
    assert m.apply(np.array([[30]], np.uint8), 1)[0, 0] == 127             # learningRate 1 re-initialises (a first frame again)
    modes, gmm, mean = m.export()
    assert m.nframes == 1 and modes[0, 0] == 1 and gmm[0, 0, 0, 0] == F(1) and gmm[0, 0, 0, 1] == F(15) and mean[0, 0, 0, 0] == F(30)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("shadows,want", [(True, 127), (False, 255)])
def test_half_bright_pixel_over_an_established_mode(impl, shadows, want):
    m = R.Mog2(impl, detectShadows=shadows)
    row = np.array([[200, 100, 60]], np.uint8)                            # 1 x 3
    for _ in range(6):
        m.apply(row)
    got = m.apply(np.array([[100, 100, 200]], np.uint8))
    # 200 -> 100: a = 0.5 >= tau, on the line through the mean: shadow.  100 -> 100: background.  60 -> 200: brighter, never a shadow
    assert got.tolist() == [[want, 0, 255]]
    assert m.getBackgroundImage().tolist() == [[200, 100, 60]]


@pytest.mark.parametrize("impl", IMPLS)
def test_background_of_a_pixel_without_modes_is_zero(impl):
    m = R.Mog2(impl)
    m.apply(np.array([[9.5, 3.0]], np.float32))
    m.modes[0, 1] = 0
    assert m.getBackgroundImage().tolist() == [[9.5, 0.0]]


# ---- the two restatements agree, and the sequences take every branch
@functools.lru_cache(maxsize=None)
def run_sequence(impl, h, w, cn, dtype, nmix, shadows=True):
    frames, rates = R.sequence(h, w, cn, dtype, seed=h * 100 + w)
    m = R.Mog2(impl, history=HISTORY, nmixtures=nmix, detectShadows=shadows)
    masks, models, bgs = [], [], []
    for f, r in zip(frames, rates):
        masks.append(m.apply(f, r))
        models.append(m.export())
        bgs.append(m.getBackgroundImage())
    return frames, rates, masks, models, bgs, dict(m.cnt)


@pytest.mark.parametrize("case", SEQS, ids=lambda c: "%dx%dx%d-%s-m%d" % (c[0], c[1], c[2], np.dtype(c[3]).name, c[4]))
def test_restatements_agree_bit_for_bit(case):
    _, _, ml, gl, bl, _ = run_sequence("loops", *case)
    _, _, mv, gv, bv, _ = run_sequence("vec", *case)
    assert 12 <= len(ml) <= 24
    for t in range(len(ml)):
        assert np.array_equal(ml[t], mv[t]), t
        assert R.same_model(gl[t], gv[t]), t
        assert bl[t].dtype == bv[t].dtype and bl[t].tobytes() == bv[t].tobytes(), t


def test_sequences_take_every_branch():
    total = dict.fromkeys(R.COUNTERS, 0)
    for case in SEQS:
        if case[4] != 5:
            continue
        cnt = run_sequence("loops", *case)[5]
        for k in R.COUNTERS:
            total[k] += cnt[k]
    assert all(v > 0 for v in total.values()), total
    # ... and the first CV_8UC1 sequence alone takes them all
    cnt = run_sequence("loops", *SEQS[0])[5]
    assert all(cnt[k] > 0 for k in R.COUNTERS), cnt


def test_batch_rule_reinitialises_once():
    frames, _ = R.sequence(3, 4, 1, np.uint8, seed=5, nframes=12)
    a, b = R.Mog2("vec", history=HISTORY), R.Mog2("vec", history=HISTORY)
    a.apply(frames[0]); b.apply(frames[0])
    ma = a.applyBatch(frames[1:6], 1.5)
    assert a.nframes == 5
    mb = [b.apply(frames[1], 1.5)] + [b.apply(f, 1.5, _may_reinit=False) for f in frames[2:6]]
    assert all(np.array_equal(x, y) for x, y in zip(ma, mb)) and R.same_model(a.export(), b.export())


# ---- mog2_math.h compiled for the host
def emu():
    # the library's own flag: every product and sum is rounded on its own
    lib = emubuild.load("mog2_emu.cpp", "libmog2_emu.so", ["-ffp-contract=off"])
    i32, vp, f32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    lib.emu_mog2_apply.argtypes = [i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, i32, f32, vp]
    lib.emu_mog2_background.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    lib.emu_mog2_round8.argtypes = [f32]
    lib.emu_mog2_round8.restype = ctypes.c_uint
    return lib


def params_array(p):
    return np.array([p["varThreshold"], p["backgroundRatio"], p["varThresholdGen"], p["varInit"], p["varMin"], p["varMax"], p["complexityReductionThreshold"],
                     p["shadowThreshold"]], np.float32)


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("case", SEQS, ids=lambda c: "%dx%dx%d-%s-m%d" % (c[0], c[1], c[2], np.dtype(c[3]).name, c[4]))
def test_mog2_math_h_on_the_host_equals_the_restatement(case, shadows):
    lib = emu()
    h, w, cn, dtype, nmix = case
    frames, rates, masks, models, bgs, _ = run_sequence("vec", *case, shadows)
    par = params_array(dict(R.DEFAULTS))
    npix = h * w
    modes = np.zeros(npix, np.uint8)
    gmm = np.zeros((npix, nmix, 2), np.float32)
    mean = np.zeros((npix, nmix, cn), np.float32)
    nf = 0
    for t, (f, r) in enumerate(zip(frames, rates)):
        nf += 1
        alphaT = F(r if (r >= 0 and nf > 1) else 1.0 / min(2 * nf, HISTORY))
        fr = np.ascontiguousarray(f)
        mask = np.full(npix, 7, np.uint8)
        lib.emu_mog2_apply(cn, int(dtype == np.float32), P(fr), npix, nmix, P(modes), P(gmm), P(mean), P(par), int(shadows), 127, alphaT, P(mask))
        assert np.array_equal(mask.reshape(h, w), masks[t]), t
        got = (modes.reshape(h, w), gmm.reshape(h, w, nmix, 2), mean.reshape(h, w, nmix, cn))
        assert R.same_model(got, models[t]), t
        bg = np.zeros((npix, cn), np.float32)
        lib.emu_mog2_background(cn, npix, nmix, P(modes), P(gmm), P(mean), P(par), P(bg))
        if dtype == np.uint8:
            bg = np.array([lib.emu_mog2_round8(float(v)) for v in bg.ravel()], np.uint8)
        assert bg.reshape(bgs[t].shape).tobytes() == bgs[t].tobytes(), t


def test_round8_is_nearest_even_and_saturates():
    lib = emu()
    assert [lib.emu_mog2_round8(v) for v in (0.5, 1.5, 2.5, 254.5, 255.5, 300.0, -3.0, 126.49)] == [0, 2, 2, 254, 255, 255, 0, 126]


# ---- limits and the refusals that need no device
def test_limits():
    from opencv_amd import _lib
    lib = emu()
    assert _lib.limit("mog2_max_dim") == 16384 == lib.emu_mog2_max_dim()
    assert _lib.limit("mog2_max_mixtures") == 5 == lib.emu_mog2_max_mixtures()


def reason():
    from opencv_amd import _lib
    return _lib.lib.mi355cv_lastError().decode()


def test_declines_before_any_device():
    from opencv_amd import _lib
    L = _lib.lib
    big = _lib.limit("mog2_max_dim") + 1
    h = ctypes.c_void_p()
    assert L.mi355cv_mog2Create(ctypes.byref(h), 0, 16.0, 1) == NOT_IMPLEMENTED and "history < 1" in reason()
    assert L.mi355cv_mog2Create(ctypes.byref(h), 8, 16.0, 1) == OK and h.value
    try:
        v = ctypes.c_double()
        for name, want in (("history", 8), ("nmixtures", 5), ("varThreshold", 16), ("backgroundRatio", float(F(0.9))), ("varThresholdGen", 9), ("varInit", 15),
                           ("varMin", 4), ("varMax", 75), ("complexityReductionThreshold", float(F(0.05))), ("detectShadows", 1), ("shadowValue", 127),
                           ("shadowThreshold", 0.5)):
            assert L.mi355cv_mog2GetParam(h, name.encode(), ctypes.byref(v)) == OK and v.value == want, name
        assert L.mi355cv_mog2SetParam(h, b"varMax", 60.0) == OK and L.mi355cv_mog2GetParam(h, b"varMax", ctypes.byref(v)) == OK and v.value == 60.0
        for bad in (0, 6):
            assert L.mi355cv_mog2SetParam(h, b"nmixtures", float(bad)) == NOT_IMPLEMENTED and "MOG2_MAX_MIXTURES" in reason()
        assert L.mi355cv_mog2SetParam(h, b"history", 0.0) == NOT_IMPLEMENTED
        assert L.mi355cv_mog2GetParam(h, b"nmixtures", ctypes.byref(v)) == OK and v.value == 5
        assert L.mi355cv_mog2SetParam(h, b"noSuchName", 1.0) == NOT_IMPLEMENTED and L.mi355cv_mog2GetParam(h, b"noSuchName", ctypes.byref(v)) == NOT_IMPLEMENTED
        img = np.zeros((4, 8, 4), np.uint8)
        mask = np.zeros((4, 8), np.uint8)
        for typ in (1, 2, 8, 24, 6, 13):                                   # CV_8S, CV_16U, CV_8UC2, CV_8UC4, CV_64F, CV_32FC2
            assert L.mi355cv_mog2Apply(h, P(img), 32, P(mask), 8, 8, 4, typ, -1.0) == NOT_IMPLEMENTED and "typeServed" in reason(), typ
        assert L.mi355cv_mog2Apply(h, P(img), 1 << 20, P(mask), 1 << 20, big, 4, 0, -1.0) == NOT_IMPLEMENTED and "MOG2_MAX_DIM" in reason()
        assert L.mi355cv_mog2Apply(h, P(img), 8, P(mask), 8, 8, big, 0, -1.0) == NOT_IMPLEMENTED and "MOG2_MAX_DIM" in reason()
        assert L.mi355cv_mog2Apply(h, P(img), 8, P(mask), 8, 0, 4, 0, -1.0) == NOT_IMPLEMENTED
        assert L.mi355cv_mog2Apply(h, P(img), 7, P(mask), 8, 8, 4, 0, -1.0) == NOT_IMPLEMENTED and "sstep < rowb" in reason()
        assert L.mi355cv_mog2Apply(h, None, 8, P(mask), 8, 8, 4, 0, -1.0) == NOT_IMPLEMENTED
        assert L.mi355cv_mog2ApplyBatch(h, P(img), 8, 32, P(mask), 8, 32, 0, 8, 4, 0, -1.0) == NOT_IMPLEMENTED
        assert L.mi355cv_mog2ApplyBatch(h, P(img), 8, 16, P(mask), 8, 32, 2, 8, 2, 0, -1.0) == NOT_IMPLEMENTED          # frames that overlap
        # no model yet
        assert L.mi355cv_mog2GetBackgroundImage(h, P(mask), 8, 8, 4, 0) == NOT_IMPLEMENTED and "nframes == 0" in reason()
        gm = np.zeros(8 * 4 * 5 * 2, np.float32)
        assert L.mi355cv_mog2GetModel(h, P(mask), P(gm), P(gm)) == NOT_IMPLEMENTED and "nframes == 0" in reason()
        assert L.mi355cv_mog2Apply(None, P(img), 8, P(mask), 8, 8, 4, 0, -1.0) == NOT_IMPLEMENTED
    finally:
        assert L.mi355cv_mog2Free(h) == OK
    assert L.mi355cv_mog2Free(None) == OK
