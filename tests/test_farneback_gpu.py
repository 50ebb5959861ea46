"""calcOpticalFlowFarneback on the GPU against the restatement (tests/farneback_restate.py, the vectorised form; tests/test_farneback_cpu.py holds it against the loops
form, known answers and a known translation), all bit for bit: the three stage entries at their edges, the whole call, the batch against single calls."""
import functools

import numpy as np
import pytest
import torch

import farneback_restate as R
import viewcheck as V

pytestmark = pytest.mark.gpu

F = np.float32
GAUSS, INITIAL = R.OPTFLOW_FARNEBACK_GAUSSIAN, R.OPTFLOW_USE_INITIAL_FLOW
WINDOWS = [0, GAUSS]
WINDOW_IDS = ["box", "gauss"]


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    return opencv_amd


def last_kernel():
    from opencv_amd import _lib
    return _lib.lib.mi355cv_lastKernel().decode()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                             # (a copy: the cached inputs are read-only)


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def texture(h, w, seed=0):
    return frozen(R.texture_pair(h, w, (0, 0), seed=seed)[0])


@functools.lru_cache(maxsize=None)
def sequence(h, w, n, seed=0):
    """n frames: windows of one texture that move by (1, -1) and a little more each frame"""
    big = texture(h + 2 * n + 2, w + 2 * n + 2, seed)
    return tuple(frozen(big[n + 1 - i:n + 1 - i + h, 2 + i + i // 2:2 + i + i // 2 + w].copy()) for i in range(n))


@functools.lru_cache(maxsize=None)
def image(h, w, seed=0):
    return frozen((np.random.default_rng(seed + 1000 * h + w).random((h, w), dtype=F) * 255).astype(F))


@functools.lru_cache(maxsize=None)
def expansion(h, w, seed=0):
    """a pair of five-channel fields with the magnitudes of real expansions; computed once, never modified"""
    return frozen(R.poly_exp_vec(image(h, w, seed), 5, 1.1)), frozen(R.poly_exp_vec(image(h, w, seed + 1), 5, 1.1))


@functools.lru_cache(maxsize=None)
def reference(h, w, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags, seed=0):
    a, b = sequence(h, w, 2, seed)
    return frozen(R.calc(a, b, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags))


# ---- polyExp
@pytest.mark.parametrize("sigma", [0.0, 1.1, 1.5])
@pytest.mark.parametrize("n", [1, 5, 7])
def test_polyexp_edges(cv, n, sigma):
    for h in (1, 2, n + 1, 17):
        for w in (1, 2, n, n + 1, 63, 64, 65, 67):                         # the tile is 64 x 16: one tile, its edge, two tiles; images narrower than the halo
            src = image(h, w)
            got = host(cv.farnebackPolyExp(dev(src), n, sigma))
            V.check_result("polyExp %dx%d n=%d" % (h, w, n), got, R.poly_exp_vec(src, n, sigma))
    assert "k_fb_polyexp" in last_kernel()


# ---- updateMatrices
def flows_for(h, w):
    """three flow fields; the restatement confirms below that each takes both branches of the inside test"""
    yy, xx = np.mgrid[0:h, 0:w].astype(F)
    rng = np.random.default_rng(h * 100 + w)
    out = np.stack([np.where(xx < w / 2, -xx - 1.5, w - xx + 0.5), np.where(yy < h / 2, -yy - 0.25, h - yy + 2.0)], axis=2).astype(F)        # outside on every side ...
    out[1::2, 1::2] = (rng.random(out[1::2, 1::2].shape, dtype=F) - 0.5).astype(F)                                                    # ... next to pixels that stay inside
    integer = np.rint(rng.random((h, w, 2)) * 6 - 3).astype(F)                                                                        # exactly on integer positions
    last = np.zeros((h, w, 2), F)                                                                                                     # exactly on the last row and column
    last[::2, :, 0] = (w - 1 - xx)[::2]
    last[:, ::2, 1] = (h - 1 - yy)[:, ::2]
    return {"outside": out, "integer": integer, "last": last}


@pytest.mark.parametrize("size", [(4, 4), (9, 11), (12, 70)], ids=["4x4", "9x11", "12x70"])    # 4 x 4, 9 x 11: the border bands of opposite edges overlap
def test_update_matrices(cv, size):
    h, w = size
    R0, R1 = expansion(h, w)
    for name, flow in flows_for(h, w).items():
        ins = R.inside_mask(flow)
        assert ins.any() and not ins.all(), name
        if name == "outside":
            fx, fy = np.arange(w)[None, :] + flow[..., 0], np.arange(h)[:, None] + flow[..., 1]
            assert (fx < 0).any() and (fx >= w).any() and (fy < 0).any() and (fy >= h).any()
        if name == "last":
            assert (np.arange(w)[None, :] + flow[..., 0] == w - 1).any() and (np.arange(h)[:, None] + flow[..., 1] == h - 1).any()
        got = host(cv.farnebackUpdateMatrices(dev(R0), dev(R1), dev(flow)))
        V.check_result("updateMatrices %dx%d %s" % (h, w, name), got, R.update_matrices_vec(R0, R1, flow))
    assert "k_fb_update_matrices" in last_kernel()


# ---- updateFlow
@pytest.mark.parametrize("flags", WINDOWS, ids=WINDOW_IDS)
@pytest.mark.parametrize("winsize", [1, 2, 3, 15, 25])
def test_update_flow(cv, winsize, flags):
    for h, w in ((7, 9), (17, 31), (16, 32), (15, 33), (5, 65)):           # the tile is 32 x 16; 7 x 9 is smaller than the windows of 15 and 25
        R0, R1 = expansion(h, w)
        M = R.update_matrices_vec(R0, R1, flows_for(h, w)["integer"])
        want = R.update_flow_vec(M, winsize, bool(flags))
        got = host(cv.farnebackUpdateFlow(dev(M), winsize, flags))          # the last iteration: no matrix update
        V.check_result("updateFlow %dx%d" % (h, w), got, want)
        assert "k_fb_update_flow" in last_kernel() and "k_fb_update_matrices" not in last_kernel()
        got, nxt = cv.farnebackUpdateFlow(dev(M), winsize, flags, R0=dev(R0), R1=dev(R1))     # a middle one
        V.check_result("updateFlow %dx%d" % (h, w), host(got), want)
        V.check_result("updateFlow %dx%d next M" % (h, w), host(nxt), R.update_matrices_vec(R0, R1, want))
        assert "k_fb_update_matrices" in last_kernel()


# ---- the whole call
SIZES = [(7, 9, 0.5, 1), (33, 37, 0.5, 1), (64, 80, 0.5, 2), (131, 150, 0.5, 3), (50, 60, 0.8, 3)]
SIZE_IDS = ["7x9", "33x37", "64x80-2levels", "131x150-3levels", "50x60-scale0.8-3levels"]


@pytest.mark.parametrize("flags", WINDOWS, ids=WINDOW_IDS)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_end_to_end(cv, size, flags):
    h, w, pyr, levels = size
    assert len(R.level_plan(w, h, pyr, levels)) == levels
    a, b = (dev(f) for f in sequence(h, w, 2))
    for iterations, poly_n, sigma, winsize in ((0, 5, 1.1, 15), (1, 5, 1.2, 15), (3, 5, 1.1, 9), (0, 7, 1.5, 5), (1, 7, 1.5, 15), (3, 7, 1.5, 4)):
        got = host(cv.calcOpticalFlowFarneback(a, b, None, pyr, levels, winsize, iterations, poly_n, sigma, flags))
        V.check_result("%dx%d it=%d n=%d win=%d" % (h, w, iterations, poly_n, winsize), got, reference(h, w, pyr, levels, winsize, iterations, poly_n, sigma, flags))
        assert ("k_fb_update_flow<%s>" % ("gauss" if flags else "box") in last_kernel()) == (iterations > 0), last_kernel()
        assert "k_fb_polyexp n=%d" % poly_n in last_kernel()


@pytest.mark.parametrize("flags", WINDOWS, ids=WINDOW_IDS)
def test_initial_flow_at_one_level(cv, flags):
    h, w = 33, 37
    a, b = sequence(h, w, 2)
    init = (np.random.default_rng(4).random((h, w, 2), dtype=F) * 2 - 1).astype(F)
    want = R.calc(a, b, init, 0.5, 1, 9, 2, 5, 1.1, flags | INITIAL)
    assert want.tobytes() != reference(h, w, 0.5, 1, 9, 2, 5, 1.1, flags).tobytes()
    flow = dev(init)
    assert cv.calcOpticalFlowFarneback(dev(a), dev(b), flow, 0.5, 1, 9, 2, 5, 1.1, flags | INITIAL) is flow
    V.check_result("initial flow, device", host(flow), want)
    flow = init.copy()
    cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 3, 9, 2, 5, 1.1, flags | INITIAL)            # levels = 3 on 33 x 37 is still one effective level
    V.check_result("initial flow, host", flow, want)


class Device:
    @staticmethod
    def put(a):
        return torch.from_numpy(a).cuda()

    @staticmethod
    def get(a):
        return a.cpu().numpy()


@pytest.mark.parametrize("layout", ["A", "B", "F"])
@pytest.mark.parametrize("size", [(33, 37, 0.5, 1), (64, 80, 0.5, 2)], ids=["33x37", "64x80-2levels"])
def test_views(cv, size, layout):
    """the first frame a pitched ROI view inside a hostile parent, the flow a view of a guarded parent"""
    h, w, pyr, levels = size
    a, b = (V.tame(f) for f in sequence(h, w, 2))                           # (the depth's extremes are the hostile surroundings)
    want = R.calc(a, b, None, pyr, levels, 9, 3, 5, 1.1, 0)
    nxt, prv = dev(b), dev(a)
    V.run(lambda s, d: cv.calcOpticalFlowFarneback(s, nxt, d, pyr, levels, 9, 3, 5, 1.1, 0), layout, a, want, what="farneback " + layout, device=Device)
    # ... and the second frame
    V.run(lambda s, d: cv.calcOpticalFlowFarneback(prv, s, d, pyr, levels, 9, 3, 5, 1.1, 0), layout, b, want, what="farneback next " + layout, device=Device)


@pytest.mark.parametrize("size", SIZES[:3], ids=SIZE_IDS[:3])
def test_host_arrays(cv, size):
    h, w, pyr, levels = size
    a, b = sequence(h, w, 2)
    for flags in WINDOWS:
        got = cv.calcOpticalFlowFarneback(a, b, None, pyr, levels, 9, 3, 5, 1.1, flags)
        assert isinstance(got, np.ndarray)
        V.check_result("host %dx%d" % (h, w), got, reference(h, w, pyr, levels, 9, 3, 5, 1.1, flags))


# ---- batch
@pytest.mark.parametrize("flags", WINDOWS, ids=WINDOW_IDS)
def test_batch_equals_single_calls(cv, flags):
    h, w, n = 64, 80, 5
    frames = sequence(h, w, n)
    args = (0.5, 2, 9, 2, 5, 1.1, flags)
    single = [host(cv.calcOpticalFlowFarneback(dev(frames[i]), dev(frames[i + 1]), None, *args)) for i in range(n - 1)]
    for i in range(n - 1):
        V.check_result("single %d" % i, single[i], R.calc(frames[i], frames[i + 1], None, *args))
    got = host(cv.calcOpticalFlowFarnebackBatch(dev(np.stack(frames)), None, *args))
    assert got.shape == (n - 1, h, w, 2) and "%d flow(s)" % (n - 1) in last_kernel() and "k_fb_update_flow" in last_kernel()
    for i in range(n - 1):
        V.check_result("device batch flow %d" % i, got[i], single[i])
    got = cv.calcOpticalFlowFarnebackBatch(np.stack(frames), None, *args)
    assert isinstance(got, np.ndarray)
    for i in range(n - 1):
        V.check_result("host batch flow %d" % i, got[i], single[i])


@pytest.mark.parametrize("form", V.BATCH_FORMS)
def test_batch_views(cv, form):
    h, w, n = 33, 37, 3
    frames = [V.tame(f) for f in sequence(h, w, n)]
    args = (0.5, 1, 9, 2, 5, 1.1, 0)
    want = np.stack([R.calc(frames[i], frames[i + 1], None, *args) for i in range(n - 1)])
    # run_batch pairs frame i with result i: the flows' parent gets n frames, the last one stays guard
    src = np.stack(frames)
    sg = V.batch_geometry(form, np.uint8, 1, w, h, 2)
    dg = V.batch_geometry(form, F, 2, w, h, 3)
    sp0 = np.stack([V.hostile(np.uint8, sg.parent_shape())] * (n + 2))
    sp0[1:n + 1, sg.y0:sg.y0 + h, sg.x0:sg.x0 + w] = src
    dp0 = V.sentinel(F, (n + 1,) + dg.parent_shape())
    sp, dp = Device.put(sp0.copy()), Device.put(dp0.copy())
    cv.calcOpticalFlowFarnebackBatch(sp[1:n + 1, sg.y0:sg.y0 + h, sg.x0:sg.x0 + w], dp[1:n, dg.y0:dg.y0 + h, dg.x0:dg.x0 + w], *args)
    after = Device.get(dp)
    V.check_guard("batch " + form, dp0, after, dg, frames=(1, n - 1))
    V.check_guard("batch " + form + " source", sp0, Device.get(sp), sg, frames=(1, n), whole=True)
    for i in range(n - 1):
        V.check_result("batch %s flow %d" % (form, i), after[1 + i, dg.y0:dg.y0 + h, dg.x0:dg.x0 + w], want[i])


# ---- the refusals, counted
def test_declines_are_counted(cv):
    from opencv_amd import _lib
    h, w = 64, 80
    a, b = (dev(f) for f in sequence(h, w, 2))
    flow = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    keep = flow.clone()
    entry = "calcOpticalFlowFarneback"
    n0 = _lib.decline_count(entry)
    cases = [
        (lambda: cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 2, 15, 3, 5, 1.2, INITIAL), "OPTFLOW_USE_INITIAL_FLOW"),          # two effective levels
        (lambda: cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 1, 0, 3, 5, 1.2, 0), "winsize < 1"),
        (lambda: cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 1, _lib.limit("farneback_max_winsize") + 1, 3, 5, 1.2, 0), "FARNEBACK_MAX_WINSIZE"),
        (lambda: cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 1, 15, 3, 0, 1.2, 0), "polyN < 1"),
        (lambda: cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 1, 15, 3, _lib.limit("farneback_max_poly_n") + 1, 1.2, 0), "FARNEBACK_MAX_POLY_N"),
        (lambda: cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 1, 15, -1, 5, 1.2, 0), "iterations < 0"),
        (lambda: cv.calcOpticalFlowFarneback(a, b, flow, 0.5, 1, 15, 3, 5, 1.2, 1), "flags"),
        (lambda: cv.calcOpticalFlowFarneback(a.to(torch.float32), b.to(torch.float32), flow, 0.5, 1, 15, 3, 5, 1.2, 0), "CV_8UC1"),
        (lambda: cv.calcOpticalFlowFarneback(torch.stack([a, a, a], 2), torch.stack([b, b, b], 2), flow, 0.5, 1, 15, 3, 5, 1.2, 0), "CV_8UC1"),
    ]
    wide = torch.zeros((1, _lib.limit("farneback_max_dim") + 1), dtype=torch.uint8, device="cuda")
    cases.append((lambda: cv.calcOpticalFlowFarneback(wide, wide, None, 0.5, 1, 15, 3, 5, 1.2, 0), "FARNEBACK_MAX_DIM"))
    # in place / overlapping in HBM: the flow over the first frame's bytes, and over the second's
    raw = torch.zeros((h * w * 8 + 64,), dtype=torch.uint8, device="cuda")
    over = raw[:h * w * 8].view(torch.float32).view(h, w, 2)
    inside = raw[64:64 + h * w].view(h, w)
    cases.append((lambda: cv.calcOpticalFlowFarneback(inside, b, over, 0.5, 1, 15, 3, 5, 1.2, 0), "overlapOnDevice"))
    cases.append((lambda: cv.calcOpticalFlowFarneback(a, inside, over, 0.5, 1, 15, 3, 5, 1.2, 0), "overlapOnDevice"))
    for i, (call, why) in enumerate(cases):
        with pytest.raises(NotImplementedError, match=why):
            call()
        assert _lib.decline_count(entry) == n0 + i + 1, why
    assert torch.equal(flow, keep)
    # a level whose Gaussian would need more taps than the limit (scale 1/128: sigma 63.5, 317 taps); the frames are never touched
    tall = torch.zeros((4224, 8192), dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError, match="FARNEBACK_MAX_SMOOTH_TAPS"):
        cv.calcOpticalFlowFarneback(tall, tall, None, 0.5, 8, 15, 3, 5, 1.2, 0)
    nb = _lib.decline_count("calcOpticalFlowFarnebackBatch")
    frames = dev(np.stack(sequence(h, w, 3)))
    with pytest.raises(NotImplementedError, match="USE_INITIAL_FLOW"):
        cv.calcOpticalFlowFarnebackBatch(frames, None, 0.5, 1, 15, 3, 5, 1.2, INITIAL)
    flows = torch.zeros((2, h, w, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(NotImplementedError, match="flow_frame_stride"):     # the two flows are one buffer
        cv.calcOpticalFlowFarnebackBatch(frames, flows[:1].expand(2, h, w, 2), 0.5, 1, 15, 3, 5, 1.2, 0)
    assert _lib.decline_count("calcOpticalFlowFarnebackBatch") == nb + 2
    # the stages refuse their output over an input
    R0 = dev(expansion(8, 8)[0])
    ns = _lib.decline_count("farnebackUpdateMatrices")
    with pytest.raises(NotImplementedError, match="overlapOnDevice"):
        cv.farnebackUpdateMatrices(R0, R0, torch.zeros((8, 8, 2), dtype=torch.float32, device="cuda"), M=R0)
    assert _lib.decline_count("farnebackUpdateMatrices") == ns + 1
    # ... and the served call still works afterwards
    V.check_result("after the declines", host(cv.calcOpticalFlowFarneback(a, b, None, 0.5, 2, 9, 3, 5, 1.1, 0)), reference(h, w, 0.5, 2, 9, 3, 5, 1.1, 0))
