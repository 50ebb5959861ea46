"""BackgroundSubtractorMOG2 on the GPU against the restatement (tests/mog2_restate.py, the vectorised form; tests/test_mog2_cpu.py holds it against the loops form and
checks that the sequences take every branch), all bit for bit: masks per frame, the exported model and the background image after the last frame."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mog2_restate as R
import viewcheck as V

pytestmark = pytest.mark.gpu

HISTORY = 6
TYPES = [(np.uint8, 1), (np.uint8, 3), (np.float32, 1), (np.float32, 3)]
TYPE_IDS = ["8UC1", "8UC3", "32FC1", "32FC3"]


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    return opencv_amd


def last_kernel():
    from opencv_amd import _lib
    return _lib.lib.mi355cv_lastKernel().decode()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@functools.lru_cache(maxsize=None)
def reference(h, w, cn, dtype, nmix, shadows, nframes=22, history=HISTORY):
    """(frames, rates, masks, final export, final background) of the restatement; computed once, never modified"""
    frames, rates = R.sequence(h, w, cn, dtype, seed=h * 100 + w, nframes=nframes)
    m = R.Mog2("vec", history=history, nmixtures=nmix, detectShadows=shadows)
    masks = [m.apply(f, r) for f, r in zip(frames, rates)]
    return frames, rates, masks, m.export(), m.getBackgroundImage()


def make(cv, nmix=5, shadows=True, history=HISTORY):
    m = cv.createBackgroundSubtractorMOG2(history, 16, shadows)
    if nmix != 5:
        m.setNMixtures(nmix)
    return m


def check_model(m, export, background, what=""):
    got = tuple(host(a) for a in m.getModel())
    for name, g, w_ in zip(("modesUsed", "gmm", "mean"), got, export):
        V.check_result("%s %s" % (what, name), g, w_)
    V.check_result(what + " background", host(m.getBackgroundImage()), background)


# ---- the four types x nmixtures x shadows
@pytest.mark.parametrize("shadows", [True, False], ids=["shadows", "noshadows"])
@pytest.mark.parametrize("nmix", [1, 3, 5])
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_types_mixtures_shadows(cv, typ, nmix, shadows):
    dtype, cn = typ
    h, w = 7, 20                                                            # CV_8UC1: rows on dwords, a width of whole quads -> the quad kernel
    frames, rates, masks, export, background = reference(h, w, cn, dtype, nmix, shadows)
    m = make(cv, nmix, shadows)
    for t, (f, r) in enumerate(zip(frames, rates)):
        got = host(m.apply(dev(f), learningRate=r))
        V.check_result("frame %d" % t, got, masks[t])
    assert ("quad" in last_kernel()) == (dtype == np.uint8 and cn == 1), last_kernel()
    check_model(m, export, background)


# ---- widths around the vector path's edges
@pytest.mark.parametrize("h", [1, 2, 7])
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_widths(cv, typ, h):
    dtype, cn = typ
    for w in ((1, 3, 4, 5, 15, 16, 17, 67) if (dtype == np.uint8 and cn == 1) else (1, 5, 21)):
        frames, rates, masks, export, background = reference(h, w, cn, dtype, 5, True, nframes=12)
        m = make(cv)
        for t, (f, r) in enumerate(zip(frames, rates)):
            V.check_result("w=%d frame %d" % (w, t), host(m.apply(dev(f), learningRate=r)), masks[t])
        check_model(m, export, background, "w=%d" % w)


# ---- applyBatch against single calls
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("T", [1, 2, 13])
def test_batch_equals_single_calls(cv, typ, T):
    dtype, cn = typ
    h, w = 5, 12
    frames, _ = R.sequence(h, w, cn, dtype, seed=3, nframes=16)
    # automatic rates across the 2 * nframes < history knee (history = 8): 1/2, 1/4, 1/6, 1/8, 1/8 ...; the batch follows two single calls
    single, batch = make(cv, history=8), make(cv, history=8)
    want = []
    for f in frames[:2 + T]:
        want.append(host(single.apply(dev(f))))
    for f in frames[:2]:
        batch.apply(dev(f))
    got = host(batch.applyBatch(dev(np.stack(frames[2:2 + T]))))
    for t in range(T):
        V.check_result("batch frame %d" % t, got[t], want[2 + t])
    for a, b in zip(single.getModel(), batch.getModel()):
        V.check_result("model", host(b), host(a))
    # ... and against the restatement, first call included (T frames from an empty model)
    ref = R.Mog2("vec", history=8)
    want = ref.applyBatch(frames[:T])
    fresh = make(cv, history=8)
    got = host(fresh.applyBatch(dev(np.stack(frames[:T]))))
    for t in range(T):
        V.check_result("fresh batch frame %d" % t, got[t], want[t])
    check_model(fresh, ref.export(), ref.getBackgroundImage(), "fresh batch")


def test_batch_with_rate_one_reinitialises_once(cv):
    frames, _ = R.sequence(5, 12, 1, np.uint8, seed=4, nframes=8)
    ref, m = R.Mog2("vec", history=8), make(cv, history=8)
    for f in frames[:3]:
        ref.apply(f)
        m.apply(dev(f))
    want = ref.applyBatch(frames[3:8], 1.0)
    got = host(m.applyBatch(dev(np.stack(frames[3:8])), learningRate=1.0))
    assert ref.nframes == 5
    for t in range(5):
        V.check_result("frame %d" % t, got[t], want[t])
    check_model(m, ref.export(), ref.getBackgroundImage())
    # the next automatic rate is that of a sixth frame
    V.check_result("after", host(m.apply(dev(frames[0]))), ref.apply(frames[0]))


def test_batch_longer_than_one_launch(cv):
    """more than 64 frames take several launches; the model carries over"""
    frames, _ = R.sequence(3, 8, 1, np.uint8, seed=6, nframes=22)
    seq = [frames[i % 22] for i in range(70)]
    ref, m = R.Mog2("vec", history=8), make(cv, history=8)
    want = ref.applyBatch(seq, 0.05)
    got = host(m.applyBatch(dev(np.stack(seq)), learningRate=0.05))
    for t in range(70):
        V.check_result("frame %d" % t, got[t], want[t])
    check_model(m, ref.export(), ref.getBackgroundImage())


# ---- misaligned, pitched ROI views with guarded destinations
class Device:
    @staticmethod
    def put(a):
        return torch.from_numpy(a).cuda()

    @staticmethod
    def get(a):
        return a.cpu().numpy()


def reachable_views(h, w):
    """(type, layout) pairs the pixel sizes allow (a 12-byte pixel has no base of 4 modulo 16, for instance)"""
    out, ids = [], []
    for typ, tid in zip(TYPES, TYPE_IDS):
        for layout in V.LAYOUTS:
            try:
                V.plan(layout, typ[0], typ[1], w, h, np.uint8, 1)
            except V.Unreachable:
                continue
            out.append((typ, layout))
            ids.append(tid + "-" + layout)
    return out, ids


VIEW_CASES, VIEW_IDS = reachable_views(6, 20)


@pytest.mark.parametrize("typ,layout", VIEW_CASES, ids=VIEW_IDS)
def test_views(cv, typ, layout):
    dtype, cn = typ
    h, w = 6, 20
    frames, rates, masks, _, _ = reference(h, w, cn, dtype, 5, True, nframes=12)
    m = make(cv)
    for t in range(11):
        m.apply(dev(frames[t]), learningRate=rates[t])
    name, _ = V.run(lambda s, d: m.apply(s, d, learningRate=rates[11]), layout, frames[11], masks[11], what="apply " + layout, device=Device, kernel_name=last_kernel)
    if dtype == np.uint8 and cn == 1:
        assert ("quad" in name) == (layout in ("A", "E", "F")), (layout, name)      # every row of both views on a dword


@pytest.mark.parametrize("form", V.BATCH_FORMS)
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_batch_views(cv, typ, form):
    dtype, cn = typ
    h, w = 6, 20
    frames, _ = R.sequence(h, w, cn, dtype, seed=8, nframes=12)
    ref = R.Mog2("vec", history=8)
    want = np.stack(ref.applyBatch(frames, 0.1))
    m = make(cv, history=8)

    def call(s, d):
        assert (s.stride(0) * s.element_size()) % 16 != 0 and d.stride(0) % 16 != 0      # frame strides that are no multiple of 16
        return m.applyBatch(s, d, learningRate=0.1)
    V.run_batch(call, form, np.stack(frames), want, what="applyBatch", device=Device)
    check_model(m, ref.export(), ref.getBackgroundImage(), form)


# ---- re-initialisation, independence
def test_geometry_change_and_set_nmixtures_reinitialise(cv):
    f1, r1 = R.sequence(4, 8, 1, np.uint8, seed=1, nframes=6)
    f2, _ = R.sequence(5, 8, 1, np.uint8, seed=2, nframes=6)
    ref, m = R.Mog2("vec", history=8), make(cv, history=8)
    for f in f1:
        V.check_result("first", host(m.apply(dev(f))), ref.apply(f))
    for f in f2:                                                            # another height: both start over
        V.check_result("second", host(m.apply(dev(f))), ref.apply(f))
    assert ref.nframes == 6
    check_model(m, ref.export(), ref.getBackgroundImage())
    ref.set("nmixtures", 3)
    m.setNMixtures(3)
    for f in f2[:3]:
        V.check_result("third", host(m.apply(dev(f))), ref.apply(f))
    assert ref.nframes == 3 and m.getNMixtures() == 3
    check_model(m, ref.export(), ref.getBackgroundImage())
    f3, _ = R.sequence(5, 8, 1, np.float32, seed=2, nframes=3)               # another type
    for f in f3:
        V.check_result("fourth", host(m.apply(dev(f))), ref.apply(f))
    assert ref.nframes == 3
    check_model(m, ref.export(), ref.getBackgroundImage())


def test_two_subtractors_do_not_share_state(cv):
    fa, _ = R.sequence(4, 8, 1, np.uint8, seed=1, nframes=8)
    fb, _ = R.sequence(4, 8, 1, np.uint8, seed=9, nframes=8)
    ra, rb, a, b = R.Mog2("vec"), R.Mog2("vec"), make(cv, history=500), make(cv, history=500)
    for x, y in zip(fa, fb):
        V.check_result("a", host(a.apply(dev(x))), ra.apply(x))
        V.check_result("b", host(b.apply(dev(y))), rb.apply(y))
    check_model(a, ra.export(), ra.getBackgroundImage())
    check_model(b, rb.export(), rb.getBackgroundImage())


# ---- the refusals that touch the device
def test_declines_on_the_device(cv):
    from opencv_amd import _lib
    m = make(cv)
    with pytest.raises(NotImplementedError):                                # no model yet
        m.getBackgroundImage()
    out = torch.zeros((4, 8), dtype=torch.uint8, device="cuda")
    rc = _lib.lib.mi355cv_mog2GetBackgroundImage(m._h, ctypes.c_void_p(out.data_ptr()), 8, 8, 4, 0)
    assert rc == 1 and "nframes == 0" in _lib.lib.mi355cv_lastError().decode()
    frames, _ = R.sequence(4, 8, 1, np.uint8, seed=1, nframes=3)
    ref = R.Mog2("vec", history=HISTORY)
    V.check_result("first", host(m.apply(dev(frames[0]))), ref.apply(frames[0]))
    x = dev(frames[1])
    keep = x.clone()
    with pytest.raises(NotImplementedError, match="overlapOnDevice"):       # the mask is the source
        m.apply(x, x)
    assert torch.equal(x, keep)
    both = torch.zeros((6, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError, match="overlapOnDevice"):       # ... or shares rows with it
        m.apply(both[0:4], both[2:6])
    with pytest.raises(NotImplementedError):                                # a geometry other than the model's
        m.getBackgroundImage(dst=torch.zeros((5, 8), dtype=torch.uint8, device="cuda"))
    # the declined calls left the model alone
    V.check_result("second", host(m.apply(x)), ref.apply(frames[1]))
    check_model(m, ref.export(), ref.getBackgroundImage())


# ---- host frames
@pytest.mark.parametrize("typ", TYPES, ids=TYPE_IDS)
def test_host_frames_equal_device_frames(cv, typ):
    dtype, cn = typ
    h, w = 7, 21
    frames, rates, masks, export, background = reference(h, w, cn, dtype, 5, True, nframes=12)
    m = make(cv)
    for t in range(6):
        got = m.apply(frames[t], learningRate=rates[t])
        assert isinstance(got, np.ndarray)
        V.check_result("host frame %d" % t, got, masks[t])
    ref = R.Mog2("vec", history=HISTORY)
    for t in range(6):
        ref.apply(frames[t], rates[t])
    want = ref.applyBatch(frames[6:12], 0.1)
    got = m.applyBatch(np.stack(frames[6:12]), learningRate=0.1)            # the host-batch pipeline; the model stays on the device
    for t in range(6):
        V.check_result("host batch frame %d" % t, got[t], want[t])
    got = m.getModel()
    assert all(isinstance(a, np.ndarray) for a in got)
    check_model(m, ref.export(), ref.getBackgroundImage(), "host")
