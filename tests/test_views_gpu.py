"""The older hooks on misaligned, pitched ROI views with a guarded destination (tests/viewcheck.py): what a cv::Mat submatrix hands a hook.  Their own GPU suites feed
fresh tensors (base aligned to hundreds of bytes, pitch == row bytes, nothing behind a row but the next row), so the pointer half of every alignment predicate, every store
past a row end and the batch entries' column offsets are invisible there.  Here every op of the table runs on the six layouts of viewcheck.LAYOUTS; the result equals the
oracle's for the contiguous copy of the view under the comparison the op's own suite uses (the line it is copied from is cited), no byte of the destination's parent
outside the view changes, and the source's parent does not change.  Calls are made without roi=, so a view is the image it shows (BORDER_ISOLATED semantics) and the
oracle of the copy is the answer for every border mode.  Layout A is the control: where the op's own suite asserts a kernel name, A asserts the same.  The kernel each
(op, layout) ran is collected and printed once at the end of the module (from the fixture's teardown, which pytest captures: run with -s to see the table)."""
import functools

import numpy as np
import pytest
import torch

import orc as O
import viewcheck as vc
from test_oracle_canny import scene
from test_oracle_smooth import V_U8
from viewtable import Device, Op, img, last_kernel, mark, marked, print_kernel_table, rel, short

pytestmark = pytest.mark.gpu

U8, U16, S16, F32, F64 = np.uint8, np.uint16, np.int16, np.float32, np.float64
SHAPES = [(w, h) for w in (13, 64, 1043) for h in (1, 37)]          # < 16 bytes a row / whole vectors, one partial wave / a second strip with a ragged last chunk; one row / segments with a tail
HEAVY = [(13, 19), (64, 19), (131, 19)]                             # bilateral, Canny, median 9, Gaussian-C adaptive threshold
EVEN = [(w, h) for w in (16, 64, 1042) for h in (2, 36)]            # 4:2:0 / 4:2:2 need even sizes
KERNELS = {}                                                        # (op, layout) -> set of kernel names


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    yield opencv_amd
    print_kernel_table(KERNELS, vc.LAYOUTS + ("inplace",) + vc.BATCH_FORMS)


OPS = []


def op(*a, shapes=SHAPES, **kw):
    OPS.append(Op(*a, shapes=shapes, **kw))


# ---------------------------------------------------------------------------------------------------------------- threshold (tests/test_thresh_gpu.py:30: bit for bit)
for _dt, _cn, _t in [(U8, 1, 100.0), (U8, 3, 100.0), (S16, 1, 1000.0), (F32, 1, 0.5), (F64, 1, 0.5)]:
    for _type in (0, 3):
        op("threshold %s C%d type %d" % (np.dtype(_dt).name, _cn, _type), lambda w, h, dt=_dt, cn=_cn: img(dt, cn, w, h, 1),
           lambda a, t=_t, ty=_type: O.orc_threshold(a, t, 200.0, ty)[1], lambda cv, s, d, t=_t, ty=_type: cv.threshold(s, t, 200.0, ty, dst=d))
op("threshold OTSU uint8 C1", lambda w, h: img(U8, 1, w, h, 2), lambda a: O.orc_thresholdOtsu(a, 200.4, 0)[1],                    # tests/test_colormisc_gpu.py:123
   lambda cv, s, d: cv.threshold(s, 0, 200.4, 0 | cv.THRESH_OTSU, dst=d), extra=lambda rv, a: rv[0] == O.orc_thresholdOtsu(a, 200.4, 0)[0])
op("adaptiveThreshold MEAN_C 5", lambda w, h: img(U8, 1, w, h, 3), lambda a: O.orc_adaptiveThreshold(a, 255.0, 0, 5, 2.0),        # tests/test_thresh_gpu.py:56
   lambda cv, s, d: cv.adaptiveThreshold(s, 255.0, cv.ADAPTIVE_THRESH_MEAN_C, 0, 5, 2.0, dst=d))
op("adaptiveThreshold GAUSSIAN_C 7", lambda w, h: img(U8, 1, w, h, 4), lambda a: O.orc_adaptiveThreshold(a, 255.0, 0, 7, -3.5, method=1),   # :70
   lambda cv, s, d: cv.adaptiveThreshold(s, 255.0, cv.ADAPTIVE_THRESH_GAUSSIAN_C, 0, 7, -3.5, dst=d), shapes=HEAVY)

# ---------------------------------------------------------------------------------------------------------------- medianBlur (tests/test_median_gpu.py:25-28, :59-60, :74-75)
for _k in (3, 5):
    for _cn in (1, 3, 4):
        op("medianBlur uint8 C%d k%d" % (_cn, _k), lambda w, h, cn=_cn: img(U8, cn, w, h, 5), lambda a, k=_k: O.orc_medianBlur(a, k),
           lambda cv, s, d, k=_k: cv.medianBlur(s, k, dst=d), kernel=lambda w, h, k=_k, cn=_cn: ("k_median_roll<%d,%d," % (k, cn)) if w >= 64 else None)
op("medianBlur uint8 C1 k9", lambda w, h: img(U8, 1, w, h, 6), lambda a: O.orc_medianBlur(a, 9), lambda cv, s, d: cv.medianBlur(s, 9, dst=d), shapes=HEAVY,
   kernel=lambda w, h: "k_median_bits_u8")
op("medianBlur uint16 C1 k3", lambda w, h: img(U16, 1, w, h, 7), lambda a: O.orc_medianBlur(a, 3), lambda cv, s, d: cv.medianBlur(s, 3, dst=d),
   kernel=lambda w, h: "k_median_typed")
op("medianBlur float32 C3 k3", lambda w, h: img(F32, 3, w, h, 8), lambda a: O.orc_medianBlur(a, 3), lambda cv, s, d: cv.medianBlur(s, 3, dst=d),
   kernel=lambda w, h: "k_median_typed")

# ---------------------------------------------------------------------------------------------------------------- Canny (tests/test_canny_gpu.py:28)
for _cn in (1, 3):
    for _l2 in (False, True):
        op("Canny C%d %s" % (_cn, "L2" if _l2 else "L1"), lambda w, h, cn=_cn: vc.tame(scene(h, w, cn, w + cn)), lambda a, l2=_l2: O.orc_Canny(a, 50, 150, 3, l2),
           lambda cv, s, d, l2=_l2: cv.Canny(s, 50, 150, 3, l2, dst=d), shapes=HEAVY)

# ---------------------------------------------------------------------------------------------------------------- equalizeHist (tests/test_colormisc_gpu.py:101)
op("equalizeHist", lambda w, h: img(U8, 1, w, h, 9, lo=100, hi=140), O.orc_equalizeHist, lambda cv, s, d: cv.equalizeHist(s, dst=d))

# ---------------------------------------------------------------------------------------------------------------- bilateralFilter (tests/test_bilateral_gpu.py:29, :48-49)
for _b in (4, 0):
    for _cn in (1, 3):
        op("bilateralFilter uint8 C%d border %d" % (_cn, _b), lambda w, h, cn=_cn: img(U8, cn, w, h, 10), lambda a, b=_b: O.orc_bilateralFilter(a, 5, 25.0, 3.0, b),
           lambda cv, s, d, b=_b: cv.bilateralFilter(s, 5, 25.0, 3.0, b, dst=d), shapes=HEAVY)
    op("bilateralFilter float32 C1 border %d" % _b, lambda w, h: img(F32, 1, w, h, 11), lambda a, b=_b: O.orc_bilateralFilter(a, 5, 0.3, 2.0, b),
       lambda cv, s, d, b=_b: cv.bilateralFilter(s, 5, 0.3, 2.0, b, dst=d), shapes=HEAVY, compare=rel(1e-6, 3e-6), kernel=lambda w, h: "k_bilateral_f32")

# ---------------------------------------------------------------------------------------------------------------- moments: source layouts (tests/test_bilateral_gpu.py:112, :127)
_MK = ("m00", "m10", "m01", "m20", "m11", "m02", "m30", "m21", "m12", "m03")
for _dt in (U8, S16, F32, F64):
    op("moments %s" % np.dtype(_dt).name, lambda w, h, dt=_dt: img(dt, 1, w, h, 12), lambda a: None, lambda cv, s, d: cv.moments(s),
       extra=lambda rv, a: [rv[k] for k in _MK] == O.orc_moments(a).tolist())


# ---------------------------------------------------------------------------------------------------------------- integral: source layouts (tests/test_templmatch_gpu.py:193)
def _integral_ok(rv, a):
    s, q, _ = O.orc_integral(a, 4, 6, True)
    return rv[0].dtype == torch.int32 and np.array_equal(rv[0].cpu().numpy(), s) and np.array_equal(rv[1].cpu().numpy(), q)


op("integral uint8 -> 32S + 64F sqsum", lambda w, h: img(U8, 1, w, h, 13), lambda a: None, lambda cv, s, d: cv.integral(s, sqsum=True), extra=_integral_ok)

# ---------------------------------------------------------------------------------------------------------------- cvtColor, RGB / gray (tests/test_filters_gpu.py:315: bit for bit, CV_32F 1e-6)
for _name, _code, _dt, _scn in [("BGR2GRAY", 6, U8, 3), ("GRAY2BGR", 8, U8, 1), ("BGR2RGB", 4, U8, 3), ("BGR2BGRA", 0, U8, 3), ("BGRA2BGR", 1, U8, 4), ("BGR2GRAY", 6, U16, 3),
                                ("BGR2GRAY", 6, F32, 3)]:
    op("cvtColor %s %s" % (_name, np.dtype(_dt).name), lambda w, h, dt=_dt, cn=_scn: img(dt, cn, w, h, 14), lambda a, c=_code: O.orc_cvtColor(a, c),
       lambda cv, s, d, c=_code: cv.cvtColor(s, c, dst=d), compare=rel(1e-6) if _dt == F32 else vc.exact)

# ---------------------------------------------------------------------------------------------------------------- cvtColor, colour families (tests/test_yuv_gpu.py:25-28, test_colormisc_gpu.py:77, :147-148)
for _name, _code in [("BGR2YCrCb", 36), ("BGR2YUV", 82), ("YCrCb2BGR", 38), ("YUV2BGR", 84), ("BGR2HSV", 40)]:
    op("cvtColor %s" % _name, lambda w, h: img(U8, 3, w, h, 15), lambda a, c=_code: O.orc_cvtColorYUV(a, c), lambda cv, s, d, c=_code: cv.cvtColor(s, c, dst=d))
op("cvtColor HSV2BGR", lambda w, h: img(U8, 3, w, h, 16), lambda a: O.orc_cvtHSVtoBGR(a, 54, 3, 8), lambda cv, s, d: cv.cvtColor(s, 54, dst=d))
for _name, _code in [("BGR2HLS", 52), ("HLS2BGR", 60)]:
    op("cvtColor %s" % _name, lambda w, h: img(U8, 3, w, h, 17), lambda a, c=_code: O.orc_cvtColorHxx(a, c, 3), lambda cv, s, d, c=_code: cv.cvtColor(s, c, dst=d),
       kernel=lambda w, h: "HLS 8U")

# ---------------------------------------------------------------------------------------------------------------- cvtColor, YUV planes: the planes are rows of one view (tests/test_yuv_gpu.py:41, test_colormisc_gpu.py:33, :88)
for _name, _code in [("NV12 -> BGR", 91), ("I420 -> BGR", 101)]:
    op("cvtColor %s" % _name, lambda w, h: img(U8, 1, w, h * 3 // 2, 18), lambda a, c=_code: O.orc_cvtColorYUV(a, c), lambda cv, s, d, c=_code: cv.cvtColor(s, c, dst=d),
       shapes=EVEN)
op("cvtColor YUY2 -> BGR", lambda w, h: img(U8, 2, w, h, 19), lambda a: O.orc_cvtColorMisc(a, 116), lambda cv, s, d: cv.cvtColor(s, 116, dst=d), shapes=EVEN)
op("cvtColorBGR2NV (NV12)", lambda w, h: img(U8, 3, w, h, 20), lambda a: O.orc_cvtBGRtoTwoPlaneYUV(a, False, 1), lambda cv, s, d: cv.cvtColorBGR2NV(s, dst=d), shapes=EVEN)

# ---------------------------------------------------------------------------------------------------------------- pyrDown (tests/test_corner_gpu.py:89), resize (tests/test_warp_gpu.py:33-40, :59, :81)
for _dt, _cn in [(U8, 1), (U8, 3), (F32, 1)]:
    op("pyrDown %s C%d" % (np.dtype(_dt).name, _cn), lambda w, h, dt=_dt, cn=_cn: img(dt, cn, w, h, 21), O.orc_pyrDown, lambda cv, s, d: cv.pyrDown(s, dst=d),
       compare=rel(1e-6) if _dt == F32 else vc.exact)
_small = lambda w, h: (max(1, w * 2 // 3), max(1, h * 2 // 3) if h > 1 else 1)                                             # noqa: E731
for _name, _interp in [("linear", 1), ("nearest", 0)]:
    op("resize %s uint8 C3 -> 2/3" % _name, lambda w, h: img(U8, 3, w, h, 22), lambda a, i=_interp: O.orc_resize(a, _small(a.shape[1], a.shape[0]), interpolation=i),
       lambda cv, s, d, i=_interp: cv.resize(s, (d.shape[1], d.shape[0]), interpolation=i, dst=d))
op("resize area uint8 C3 x 1/2", lambda w, h: img(U8, 3, w, h, 23), lambda a: O.orc_resize(a, (a.shape[1] // 2, a.shape[0] // 2), interpolation=3),
   lambda cv, s, d: cv.resize(s, (d.shape[1], d.shape[0]), interpolation=3, dst=d), shapes=EVEN)

# ---------------------------------------------------------------------------------------------------------------- corners (tests/test_corner_gpu.py:41, :45: rel_err <= 1e-4)
op("cornerHarris uint8", lambda w, h: img(U8, 1, w, h, 24), lambda a: O.orc_cornerHarris(a, 2, 3, 0.04, 4), lambda cv, s, d: cv.cornerHarris(s, 2, 3, 0.04, dst=d),
   compare=rel(1e-4))
op("cornerMinEigenVal uint8", lambda w, h: img(U8, 1, w, h, 25), lambda a: O.orc_cornerMinEigenVal(a, 2, 3, 4), lambda cv, s, d: cv.cornerMinEigenVal(s, 2, 3, dst=d),
   compare=rel(1e-4))

# ---------------------------------------------------------------------------------------------------------------- FAST_dense (tests/test_fast_gpu.py:36), ScharrDeriv, copyMakeBorder (tests/test_lk_gpu.py:30, :41)
op("FAST_dense", lambda w, h: img(U8, 1, w, h, 26), lambda a: O.orc_FAST_dense(a, 2), lambda cv, s, d: cv.FAST_dense(s, dst=d))
op("ScharrDeriv uint8 C1", lambda w, h: img(U8, 1, w, h, 27), O.orc_ScharrDeriv, lambda cv, s, d: cv.ScharrDeriv(s, dst=d))
op("copyMakeBorder uint8 C1 reflect101", lambda w, h: img(U8, 1, w, h, 28),                                  # (one row: BORDER_REFLECT_101 of a length-1 axis repeats the row)
   lambda a: np.pad(np.pad(a, ((0, 0), (9, 4)), mode="reflect"), ((5, 7), (0, 0)), mode="reflect" if a.shape[0] > 1 else "edge"),
   lambda cv, s, d: cv.copyMakeBorder(s, 5, 7, 9, 4, 4, dst=d))

# ---------------------------------------------------------------------------------------------------------------- erode 3x3 (tests/test_morph_gpu.py), GaussianBlur 5x5 (tests/test_gaussian_gpu.py:56-58)
op("erode 3x3 uint8 C1", lambda w, h: img(U8, 1, w, h, 29), lambda a: O.orc_morph(0, a), lambda cv, s, d: cv.erode(s, dst=d))
for _cn in (1, 3):
    op("GaussianBlur 5x5 uint8 C%d" % _cn, lambda w, h, cn=_cn: img(U8, cn, w, h, 30),
       lambda a: O.orc_sepSmoothFixedU8(a, V_U8[5], V_U8[5 if a.shape[0] > 1 else 1], 4), lambda cv, s, d: cv.GaussianBlur(s, (5, 5), 0, dst=d),
       # tests/test_gauss_ring_gpu.py:85: the headline kernel wherever W * cn % 16 == 0 (64 and 192; not 13, 1043) -- with more than one row: cv::GaussianBlur makes
       # the kernel 5 x 1 for a one-row image (smooth.dispatch.cpp:623-630), which is not the binomial 5 x 5 hook's case
       kernel=lambda w, h: "k_binomial_roll2<5," if w == 64 and h > 1 else None)

BY_NAME = {o.name: o for o in OPS}
assert len(BY_NAME) == len(OPS)


@functools.lru_cache(maxsize=None)
def reference(name, w, h):
    """the source image and the oracle's answer, computed once per (op, shape) and shared by the six layouts (never written to)"""
    o = BY_NAME[name]
    image = np.ascontiguousarray(o.source(w, h))
    want = o.oracle(image)
    image.setflags(write=False)
    if want is not None:
        want = np.ascontiguousarray(want)
        want.setflags(write=False)
    return image, want


def pixels_known(*arrays):
    for a in arrays:
        if a is not None:
            assert (a.dtype.type, a.shape[2] if a.ndim == 3 else 1) in vc.PIXELS_USED, "add %s C%d to viewcheck.PIXELS_USED" % (a.dtype, a.shape[2] if a.ndim == 3 else 1)


@pytest.mark.parametrize("layout", vc.LAYOUTS)
@pytest.mark.parametrize("name", [o.name for o in OPS])
def test_views(cv, name, layout):
    o = BY_NAME[name]
    for (w, h) in o.shapes:
        image, want = reference(name, w, h)
        pixels_known(image, want)
        what = "%s layout %s %dx%d" % (name, layout, w, h)
        try:
            kern, rv = vc.run(marked(cv, o.call), layout, image, want, what=what, compare=o.compare, device=Device, kernel_name=last_kernel)
        except vc.Unreachable as e:
            if layout != "F":                                                   # only F's residues can be out of a pixel size's reach (8-byte pixels: no base of 4)
                raise
            pytest.skip("layout %s: %s" % (layout, e))
        KERNELS.setdefault((name, layout), set()).add(short(kern))
        if o.extra is not None:
            assert o.extra(rv, image), (what, rv)
        if layout == "A" and o.kernel is not None and o.kernel(w, h) is not None:
            assert o.kernel(w, h) in kern, (what, kern)                         # the control must not miss the fast path through its shape


# ---------------------------------------------------------------------------------------------------------------- in place on a layout-B view
# threshold (tests/test_thresh_gpu.py:36), adaptiveThreshold (:60), GaussianBlur (tests/test_gaussian_gpu.py:157: the wrapper clones the source, smooth.dispatch.cpp:685)
INPLACE = ["threshold uint8 C1 type 3", "adaptiveThreshold MEAN_C 5", "GaussianBlur 5x5 uint8 C1", "GaussianBlur 5x5 uint8 C3"]


@pytest.mark.parametrize("name", INPLACE)
def test_in_place_on_a_view(cv, name):
    o = BY_NAME[name]
    for (w, h) in o.shapes:
        image, want = reference(name, w, h)
        kern, _ = vc.run_inplace(marked(cv, o.call), image, want, what="%s %dx%d" % (name, w, h), compare=o.compare, device=Device, kernel_name=last_kernel)
        KERNELS.setdefault((name, "inplace"), set()).add(short(kern))


def test_cvtcolor_in_place_on_a_device_view_is_declined(cv):
    """cvtColor BGR2RGB with dst = src on a device image is declined (tests/test_colormisc_gpu.py:188-190 pins that for a fresh tensor): the same on a layout-B view,
    and neither the view nor its parent changes"""
    image, _ = reference("cvtColor BGR2RGB uint8", 64, 37)
    g, _ = vc.plan("B", image.dtype, 3, 64, 37)
    before = vc.source_parent(g, image)
    parent = Device.put(before.copy())
    v = g.view(parent)
    with pytest.raises(NotImplementedError):
        cv.cvtColor(v, cv.COLOR_BGR2RGB, dst=v)
    vc.check_guard("cvtColor BGR2RGB declined in place", before, Device.get(parent), g, whole=True)


# ---------------------------------------------------------------------------------------------------------------- batch entries, N = 3, frames as views of a guarded parent
BSHAPES = [(13, 5), (64, 37), (1043, 19)]
_K3 = [0.25, 0.5, 0.25]
# name -> (dtype, cn, batch call(cv, frames, dst), the single-image call on one contiguous frame (pinned to the oracle by test_views / the op's own suite))
BATCH = {
    "thresholdBatch": (U8, 1, lambda cv, f, d: cv.thresholdBatch(f, 100.7, 200, 0, dst=d), lambda cv, x: cv.threshold(x, 100.7, 200, 0)[1]),           # tests/test_batch_gpu.py:42
    "thresholdBatch C3": (U8, 3, lambda cv, f, d: cv.thresholdBatch(f, 90, 0, 2, dst=d), lambda cv, x: cv.threshold(x, 90, 0, 2)[1]),                   # :43
    "cvtColorBatch BGR2GRAY": (U8, 3, lambda cv, f, d: cv.cvtColorBatch(f, cv.COLOR_BGR2GRAY, dst=d), lambda cv, x: cv.cvtColor(x, cv.COLOR_BGR2GRAY)),
    "GaussianBlurBatch 3": (U8, 1, lambda cv, f, d: cv.GaussianBlurBatch(f, 3, dst=d), lambda cv, x: cv.GaussianBlur(x, (3, 3), 0)),
    "GaussianBlurBatch 5": (U8, 1, lambda cv, f, d: cv.GaussianBlurBatch(f, 5, dst=d), lambda cv, x: cv.GaussianBlur(x, (5, 5), 0)),
    "GaussianBlurBatch 5 C3": (U8, 3, lambda cv, f, d: cv.GaussianBlurBatch(f, 5, dst=d), lambda cv, x: cv.GaussianBlur(x, (5, 5), 0)),
    "SobelBatch 16S": (U8, 1, lambda cv, f, d: cv.SobelBatch(f, cv.CV_16S, 1, 0, 3, dst=d), lambda cv, x: cv.Sobel(x, cv.CV_16S, 1, 0, 3)),             # :33
    "boxFilterBatch 5x5": (U8, 1, lambda cv, f, d: cv.boxFilterBatch(f, -1, (5, 5), dst=d), lambda cv, x: cv.boxFilter(x, -1, (5, 5))),                 # :36
    "sepFilter2DBatch 32F": (U8, 1, lambda cv, f, d: cv.sepFilter2DBatch(f, cv.CV_32F, _K3, _K3, delta=0.5, dst=d),
                             lambda cv, x: cv.sepFilter2D(x, cv.CV_32F, _K3, _K3, delta=0.5)),                                                            # :41
    "pyrDownBatch": (U8, 1, lambda cv, f, d: cv.pyrDownBatch(f, dst=d), lambda cv, x: cv.pyrDown(x)),
}


@functools.lru_cache(maxsize=None)
def batch_reference(name, w, h):
    import opencv_amd as cv
    dt, cn, _, single = BATCH[name]
    frames = np.stack([img(dt, cn, w, h, 40 + f) for f in range(3)])
    want = np.stack([single(cv, torch.from_numpy(f).cuda()).cpu().numpy() for f in frames])
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, want


@pytest.mark.parametrize("form", vc.BATCH_FORMS)
@pytest.mark.parametrize("name", sorted(BATCH))
def test_batch_views(cv, name, form):
    """parent[:, 2:2+h, 3:3+w] (base, pitch and frame stride ragged) and parent[:, :, 3:3+w] (full height: frame stride == step * h, the tall-image merge with a step
    wider than the row), dst the matching guarded view: every frame equals the single-image call on the contiguous frame, the guards survive"""
    for (w, h) in BSHAPES:
        frames, want = batch_reference(name, w, h)
        kern, _ = vc.run_batch(marked(cv, BATCH[name][2]), form, frames, want, what="%s %dx%d" % (name, w, h), device=Device, kernel_name=last_kernel)
        KERNELS.setdefault((name, form), set()).add(short(kern))


@pytest.mark.parametrize("form", vc.BATCH_FORMS)
def test_integral_batch_views(cv, form):
    """integralBatch with a guarded dst pair: frames [3, h, w] -> sums [3, h + 1, w + 1] int32 and squared sums float64, each a view of its own guarded parent"""
    for (w, h) in BSHAPES:
        frames = np.stack([img(U8, 1, w, h, 50 + f) for f in range(3)])
        sg = vc.batch_geometry(form, U8, 1, w, h, 2)
        ag = vc.batch_geometry(form, np.int32, 1, w + 1, h + 1, 2)
        qg = vc.batch_geometry(form, F64, 1, w + 1, h + 1, 2)
        sp0 = np.stack([vc.hostile(U8, sg.parent_shape())] * 5)
        sp0[1:4, sg.y0:sg.y0 + h, sg.x0:sg.x0 + w] = frames
        ap0, qp0 = vc.sentinel(np.int32, (5,) + ag.parent_shape()), vc.sentinel(F64, (5,) + qg.parent_shape(), seed=7)
        sp, ap, qp = Device.put(sp0.copy()), Device.put(ap0.copy()), Device.put(qp0.copy())
        view = lambda p, g: p[1:4, g.y0:g.y0 + g.h, g.x0:g.x0 + g.w]                                                                                  # noqa: E731
        mark(cv)
        cv.integralBatch(view(sp, sg), sqsum=True, dst=(view(ap, ag), view(qp, qg)))
        KERNELS.setdefault(("integralBatch", form), set()).add(short(last_kernel()))
        a1, q1 = Device.get(ap), Device.get(qp)
        what = "integralBatch %s %dx%d" % (form, w, h)
        vc.check_guard(what + " sum", ap0, a1, ag, frames=(1, 3))
        vc.check_guard(what + " sqsum", qp0, q1, qg, frames=(1, 3))
        vc.check_guard(what + " source", sp0, Device.get(sp), sg, frames=(1, 3), whole=True)
        for f in range(3):
            s, q, _ = O.orc_integral(frames[f], 4, 6, True)
            vc.check_result(what + " sum frame %d" % f, view(a1, ag)[f], s)
            vc.check_result(what + " sqsum frame %d" % f, view(q1, qg)[f], q)
