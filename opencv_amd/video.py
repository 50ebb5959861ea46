"""Host-side mirror of the reference's sparse pyramidal Lucas-Kanade tracker (modules/video/src/lkpyramid.cpp).

The control flow is the reference's -- buildOpticalFlowPyramid (:747-843), the level loop of SparsePyrLKOpticalFlowImpl::calc (:1259-1425)
and the per-level point scaling of LKTrackerInvoker (:215-231); the work is done by the hooks the video module calls itself:
cv_hal_pyrdown, cv_hal_ScharrDeriv and cv_hal_LKOpticalFlowLevel (modules/video/src/hal_replacement.hpp), plus mi355cv_copyMakeBorder for
the padding.  With CUDA(ROCm) tensors nothing leaves HBM between the two input frames and the three result vectors.
"""
import ctypes

import numpy as np

from . import _lib
from .core import Img, bind_stream, torch, CV_8U, CV_32F, BORDER_CONSTANT, BORDER_REFLECT_101, BORDER_ISOLATED
from .imgproc import pyrDown

__all__ = ["ScharrDeriv", "copyMakeBorder", "buildOpticalFlowPyramid", "LKOpticalFlowLevel", "calcOpticalFlowPyrLK", "calcOpticalFlowPyrLK_hooks",
           "createBackgroundSubtractorMOG2", "BackgroundSubtractorMOG2", "OPTFLOW_USE_INITIAL_FLOW", "OPTFLOW_LK_GET_MIN_EIGENVALS", "TERM_COUNT", "TERM_EPS",
           "calcOpticalFlowFarneback", "calcOpticalFlowFarnebackBatch", "farnebackPolyExp", "farnebackUpdateMatrices", "farnebackUpdateFlow",
           "OPTFLOW_FARNEBACK_GAUSSIAN"]

L = _lib.lib
OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS = 4, 8
OPTFLOW_FARNEBACK_GAUSSIAN = 256
TERM_COUNT, TERM_EPS = 1, 2


def _vp(p):
    return ctypes.c_void_p(p)


def _is_dev(a):
    return torch is not None and isinstance(a, torch.Tensor) and a.is_cuda


def _empty(ref, shape, dtype_np):
    if torch is not None and isinstance(ref, torch.Tensor):
        return torch.empty(shape, dtype={np.uint8: torch.uint8, np.int16: torch.int16, np.float32: torch.float32}[dtype_np], device=ref.device)
    return np.empty(shape, dtype_np)


def _zeros(ref, shape, dtype_np):
    out = _empty(ref, shape, dtype_np)
    out[...] = 0
    return out


def ScharrDeriv(src, dst=None):
    """calcScharrDeriv (lkpyramid.cpp:59-71) through cv_hal_ScharrDeriv: CV_8U, cn channels -> CV_16S, 2*cn channels, (dI/dx, dI/dy) interleaved."""
    s = Img(src)
    if s.depth != CV_8U:
        raise ValueError("ScharrDeriv: CV_8U only")                                            # CV_Assert(depth == CV_8U), :64
    out = dst if dst is not None else _empty(src, (s.h, s.w, 2 * s.cn), np.int16)
    d = Img(out)
    bind_stream(s, d)
    _lib.check(L.mi355cv_ScharrDeriv(_vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h, s.cn), "ScharrDeriv")
    return out


def copyMakeBorder(src, top, bottom, left, right, borderType, dst=None):
    """cv::copyMakeBorder (core/src/copy.cpp:1183) for device-resident images, BORDER_CONSTANT value 0.  `dst` may be the array `src` is the
    interior of (then only the frame is written, as buildOpticalFlowPyramid does)."""
    s = Img(src)
    shape = (s.h + top + bottom, s.w + left + right) + ((s.cn,) if getattr(src, "ndim", 2) == 3 else ())
    out = dst if dst is not None else torch.empty(shape, dtype=src.dtype, device=src.device)
    d = Img(out)
    bind_stream(s, d)
    _lib.check(L.mi355cv_copyMakeBorder(_vp(s.ptr), s.step, s.w, s.h, _vp(d.ptr), d.step, top, bottom, left, right, s.cn * s.esz, int(borderType)),
               "copyMakeBorder")
    return out


def _padded_level(img, winW, winH):
    """a fresh array with a (winH, winW) frame around room for `img`; returns (whole, interior view)"""
    s = Img(img)
    shape = (s.h + 2 * winH, s.w + 2 * winW) + ((s.cn,) if getattr(img, "ndim", 2) == 3 else ())
    whole = _empty(img, shape, np.uint8)
    return whole, whole[winH:winH + s.h, winW:winW + s.w]


def _frame(whole, interior, winW, winH, borderType):
    if _is_dev(whole):
        copyMakeBorder(interior, winH, winH, winW, winW, borderType | BORDER_ISOLATED, dst=whole)
    else:                                                                                      # host arrays: the CPU's job (the hook declines host pointers)
        pad = ((winH, winH), (winW, winW)) + (((0, 0),) if interior.ndim == 3 else ())
        src = interior.numpy() if torch is not None and isinstance(interior, torch.Tensor) else interior
        whole[...] = torch.from_numpy(np.pad(src, pad, mode="reflect")) if torch is not None and isinstance(whole, torch.Tensor) else np.pad(src, pad, mode="reflect")


def buildOpticalFlowPyramid(img, winSize, maxLevel):
    """cv::buildOpticalFlowPyramid (lkpyramid.cpp:747-843) with withDerivatives = false, pyrBorder = BORDER_REFLECT_101: the list of
    level images, each one the interior view of an array padded by winSize on every side.  Stops early like the reference (:836-840)."""
    winW, winH = winSize
    if Img(img).depth != CV_8U or winW <= 2 or winH <= 2:
        raise ValueError("buildOpticalFlowPyramid: CV_8U image, winSize > 2")                  # CV_Assert, :753
    levels = []
    for level in range(maxLevel + 1):
        if level == 0:
            whole, inner = _padded_level(img, winW, winH)
            inner[...] = img
        else:
            prev = levels[-1]
            ph, pw = int(prev.shape[0]), int(prev.shape[1])
            sz = ((pw + 1) // 2, (ph + 1) // 2)
            shape = (sz[1] + 2 * winH, sz[0] + 2 * winW) + ((int(prev.shape[2]),) if prev.ndim == 3 else ())
            whole = _empty(prev, shape, np.uint8)
            inner = whole[winH:winH + sz[1], winW:winW + sz[0]]
            pyrDown(prev, sz, dst=inner)
        _frame(whole, inner, winW, winH, BORDER_REFLECT_101)
        levels.append(inner)
        h, w = int(inner.shape[0]), int(inner.shape[1])
        if (w + 1) // 2 <= winW or (h + 1) // 2 <= winH:
            break
    return levels


def LKOpticalFlowLevel(prevImg, prevDeriv, nextImg, prevPts, nextPts, status, err, winSize, maxCount, epsilon2, getMinEig, minEigThreshold):
    """cv_hal_LKOpticalFlowLevel: one pyramid level, in place on nextPts / status / err (status None above level 0).  The three images must be
    interior views of arrays padded by winSize."""
    I, D, J = Img(prevImg), Img(prevDeriv), Img(nextImg)
    n = int(prevPts.shape[0])
    bind_stream(I, J)
    ptr = lambda a: _vp(a.data_ptr() if torch is not None and isinstance(a, torch.Tensor) else a.ctypes.data) if a is not None else None
    rc = L.mi355cv_LKOpticalFlowLevel(_vp(I.ptr), I.step, _vp(D.ptr), D.step, _vp(J.ptr), J.step, I.w, I.h, I.cn, ptr(prevPts), ptr(nextPts), n,
                                      ptr(status), ptr(err), int(winSize[0]), int(winSize[1]), int(maxCount), float(epsilon2), bool(getMinEig),
                                      float(minEigThreshold))
    _lib.check(rc, "LKOpticalFlowLevel")


def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts=None, winSize=(21, 21), maxLevel=3, criteria=(TERM_COUNT | TERM_EPS, 30, 0.01), flags=0,
                         minEigThreshold=1e-4):
    """cv::calcOpticalFlowPyrLK (lkpyramid.cpp:1432; SparsePyrLKOpticalFlowImpl::calc :1259) through the one-call entry point (pyramids,
    derivatives and every level on the device).  prevPts: n x 2 float32 (same kind as the images).  Returns (nextPts n x 2 float32,
    status n uint8, err n float32).  The same computation assembled from the video module's hooks: calcOpticalFlowPyrLK_hooks."""
    winW, winH = int(winSize[0]), int(winSize[1])
    if maxLevel < 0 or winW <= 2 or winH <= 2:
        raise ValueError("calcOpticalFlowPyrLK: maxLevel >= 0 and winSize > 2")                # CV_Assert, :1277
    n = int(prevPts.shape[0])
    dev = _is_dev(prevImg)
    pts = prevPts.reshape(n, 2)
    if dev:
        pts = pts.to(device=prevImg.device, dtype=torch.float32).contiguous()
    else:
        pts = np.ascontiguousarray(np.asarray(pts), np.float32)
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        if nextPts is None or int(nextPts.shape[0]) != n:
            raise ValueError("calcOpticalFlowPyrLK: OPTFLOW_USE_INITIAL_FLOW needs nextPts of the same length")      # :1297
        out = nextPts.reshape(n, 2).to(device=prevImg.device, dtype=torch.float32).clone() if dev else np.array(np.asarray(nextPts).reshape(n, 2), np.float32)
    else:
        out = None
    if n == 0:
        return _empty(pts, (0, 2), np.float32), _empty(pts, (0,), np.uint8), _empty(pts, (0,), np.float32)
    status = _empty(pts, (n,), np.uint8)
    err = _empty(pts, (n,), np.float32)
    if out is None:
        out = _empty(pts, (n, 2), np.float32)
    I, J = Img(prevImg), Img(nextImg)
    if (I.w, I.h, I.cn, I.depth) != (J.w, J.h, J.cn, J.depth) or I.depth != CV_8U:
        raise ValueError("calcOpticalFlowPyrLK: two CV_8U images of the same size and type")   # CV_Assert, :1416-1417, :753
    bind_stream(I, J)
    ptr = lambda a: _vp(a.data_ptr() if torch is not None and isinstance(a, torch.Tensor) else a.ctypes.data)
    ctype, maxCount, eps = criteria
    rc = L.mi355cv_calcOpticalFlowPyrLK(_vp(I.ptr), I.step, _vp(J.ptr), J.step, I.w, I.h, I.cn, ptr(pts), ptr(out), n, ptr(status), ptr(err), winW, winH,
                                        int(maxLevel), int(ctype), int(maxCount), float(eps), int(flags), float(minEigThreshold))
    _lib.check(rc, "calcOpticalFlowPyrLK")
    return out, status, err


def calcOpticalFlowPyrLK_hooks(prevImg, nextImg, prevPts, nextPts=None, winSize=(21, 21), maxLevel=3, criteria=(TERM_COUNT | TERM_EPS, 30, 0.01), flags=0,
                         minEigThreshold=1e-4):
    """The level loop of SparsePyrLKOpticalFlowImpl::calc (lkpyramid.cpp:1397-1424) written out over the hooks the video module calls
    itself -- cv_hal_pyrdown, cv_hal_ScharrDeriv, cv_hal_LKOpticalFlowLevel -- with the per-level point scaling of LKTrackerInvoker
    (:215-231) done here.  Same arguments and results as calcOpticalFlowPyrLK."""
    winW, winH = int(winSize[0]), int(winSize[1])
    if maxLevel < 0 or winW <= 2 or winH <= 2:
        raise ValueError("calcOpticalFlowPyrLK_hooks: maxLevel >= 0 and winSize > 2")                # CV_Assert, :1277
    n = int(prevPts.shape[0])
    dev = _is_dev(prevImg)
    pts = prevPts.reshape(n, 2)
    if dev:
        pts = pts.to(device=prevImg.device, dtype=torch.float32).contiguous()
    else:
        pts = np.ascontiguousarray(np.asarray(pts), np.float32)
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        if nextPts is None or int(nextPts.shape[0]) != n:
            raise ValueError("calcOpticalFlowPyrLK_hooks: OPTFLOW_USE_INITIAL_FLOW needs nextPts of the same length")      # :1297
        out = nextPts.reshape(n, 2).to(device=prevImg.device, dtype=torch.float32).clone() if dev else np.array(np.asarray(nextPts).reshape(n, 2), np.float32)
    else:
        out = None
    if n == 0:
        return _empty(pts, (0, 2), np.float32), _empty(pts, (0,), np.uint8), _empty(pts, (0,), np.float32)
    status = _empty(pts, (n,), np.uint8)
    status[...] = 1
    err = _zeros(pts, (n,), np.float32)
    ctype, maxCount, eps = criteria
    maxCount = 30 if (ctype & TERM_COUNT) == 0 else min(max(int(maxCount), 0), 100)            # :1386-1395
    eps = 0.01 if (ctype & TERM_EPS) == 0 else min(max(float(eps), 0.0), 10.0)
    eps *= eps
    prevPyr = buildOpticalFlowPyramid(prevImg, (winW, winH), maxLevel)
    nextPyr = buildOpticalFlowPyramid(nextImg, (winW, winH), maxLevel)
    maxLevel = min(len(prevPyr), len(nextPyr)) - 1
    for level in range(maxLevel, -1, -1):
        I, J = prevPyr[level], nextPyr[level]
        h, w = int(I.shape[0]), int(I.shape[1])
        cn = int(I.shape[2]) if I.ndim == 3 else 1
        dwhole = _zeros(I, (h + 2 * winH, w + 2 * winW, 2 * cn), np.int16)                     # BORDER_CONSTANT frame of the derivative image (:1409)
        dI = dwhole[winH:winH + h, winW:winW + w]
        ScharrDeriv(I, dst=dI)
        scale = 1.0 / (1 << level)
        prevScaled = pts * scale if dev else pts * np.float32(scale)
        if level == maxLevel:
            out = (out * scale if dev else out * np.float32(scale)) if flags & OPTFLOW_USE_INITIAL_FLOW else (prevScaled.clone() if dev else prevScaled.copy())
        else:
            out = out * 2.0 if dev else out * np.float32(2)
        out = out.contiguous() if dev else np.ascontiguousarray(out, np.float32)
        LKOpticalFlowLevel(I, dI, J, prevScaled.contiguous() if dev else np.ascontiguousarray(prevScaled), out, status if level == 0 else None, err,
                           (winW, winH), maxCount, eps, bool(flags & OPTFLOW_LK_GET_MIN_EIGENVALS), minEigThreshold)
    return out, status, err


class BackgroundSubtractorMOG2:
    """cv::BackgroundSubtractorMOG2 (modules/video; no HAL hook) through the mi355cv_mog2* entries: the handle owns the per-pixel mixture model in HBM, frames are
    CV_8UC1 / CV_8UC3 / CV_32FC1 / CV_32FC3 torch device tensors or numpy arrays, masks CV_8UC1 of the same kind.  Create it with createBackgroundSubtractorMOG2."""
    _PARAMS = {"History": "history", "NMixtures": "nmixtures", "BackgroundRatio": "backgroundRatio", "VarThreshold": "varThreshold", "VarThresholdGen": "varThresholdGen",
               "VarInit": "varInit", "VarMin": "varMin", "VarMax": "varMax", "ComplexityReductionThreshold": "complexityReductionThreshold",
               "DetectShadows": "detectShadows", "ShadowValue": "shadowValue", "ShadowThreshold": "shadowThreshold"}
    _INT = {"history": int, "nmixtures": int, "shadowValue": int, "detectShadows": bool}

    def __init__(self, history=500, varThreshold=16, detectShadows=True):
        self._h = None
        h = ctypes.c_void_p()
        _lib.check(L.mi355cv_mog2Create(ctypes.byref(h), int(history), float(varThreshold), 1 if detectShadows else 0), "mog2Create")
        self._h = h
        self._last = None                                                                     # (array of the last frame's kind, h, w, cn, depth, the model's nmixtures)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and L is not None:
            L.mi355cv_mog2Free(h)

    def _get(self, name):
        v = ctypes.c_double()
        _lib.check(L.mi355cv_mog2GetParam(self._h, name.encode(), ctypes.byref(v)), "mog2GetParam")
        return self._INT.get(name, float)(v.value)

    def _set(self, name, v):
        _lib.check(L.mi355cv_mog2SetParam(self._h, name.encode(), float(v)), "mog2SetParam")

    def __getattr__(self, attr):                                                              # getHistory ... setShadowThreshold, the reference's names
        name = self._PARAMS.get(attr[3:]) if attr[:3] in ("get", "set") else None
        if name is None:
            raise AttributeError(attr)
        return (lambda: self._get(name)) if attr[:3] == "get" else (lambda v: self._set(name, v))

    @staticmethod
    def _frame(s):
        if s.depth not in (CV_8U, CV_32F) or s.cn not in (1, 3):
            raise ValueError("BackgroundSubtractorMOG2: CV_8UC1, CV_8UC3, CV_32FC1 or CV_32FC3 frames")

    def apply(self, image, fgmask=None, learningRate=-1):
        """one frame into the model; returns the CV_8UC1 mask (0 background, shadowValue, 255 foreground)"""
        s = Img(image)
        self._frame(s)
        out = fgmask if fgmask is not None else _empty(image, (s.h, s.w), np.uint8)
        d = Img(out)
        if (d.h, d.w, d.cn, d.depth) != (s.h, s.w, 1, CV_8U):
            raise ValueError("BackgroundSubtractorMOG2.apply: fgmask must be CV_8UC1 of the frame's size")
        bind_stream(s, d)
        _lib.check(L.mi355cv_mog2Apply(self._h, _vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h, s.type, float(learningRate)), "mog2Apply")
        self._last = (image, s.h, s.w, s.cn, s.depth, self._get("nmixtures"))
        return out

    def applyBatch(self, frames, fgmask=None, learningRate=-1):
        """T consecutive frames of the camera in time order, stacked as T x H x W (one channel) or T x H x W x C, in one launch per 64 frames: the model crosses HBM
        once.  learningRate < 0 gives every frame its own automatic rate; learningRate >= 1 re-initialises before the first frame only.  Returns T x H x W masks."""
        if isinstance(frames, (list, tuple)):
            frames = torch.stack(list(frames)) if _is_dev(frames[0]) else np.stack([np.asarray(f) for f in frames])
        if frames.ndim not in (3, 4) or int(frames.shape[0]) < 1:
            raise ValueError("BackgroundSubtractorMOG2.applyBatch: frames stacked as T x H x W or T x H x W x C")
        n = int(frames.shape[0])
        s = Img(frames[0])
        self._frame(s)
        out = fgmask if fgmask is not None else _empty(frames, (n, s.h, s.w), np.uint8)
        if out.ndim != 3 or int(out.shape[0]) != n:
            raise ValueError("BackgroundSubtractorMOG2.applyBatch: fgmask must be T x H x W, CV_8U")
        d = Img(out[0])
        if (d.h, d.w, d.cn, d.depth) != (s.h, s.w, 1, CV_8U):
            raise ValueError("BackgroundSubtractorMOG2.applyBatch: fgmask must be T x H x W, CV_8U")
        fstride = lambda a, esz: int(a.stride(0)) * esz if torch is not None and isinstance(a, torch.Tensor) else int(a.strides[0])
        bind_stream(s, d)
        _lib.check(L.mi355cv_mog2ApplyBatch(self._h, _vp(s.ptr), s.step, fstride(frames, s.esz), _vp(d.ptr), d.step, fstride(out, 1), n, s.w, s.h, s.type,
                                            float(learningRate)), "mog2ApplyBatch")
        self._last = (frames, s.h, s.w, s.cn, s.depth, self._get("nmixtures"))
        return out

    def _need_model(self, what):
        if self._last is None:
            raise NotImplementedError("BackgroundSubtractorMOG2.%s: no frame has been applied yet" % what)
        return self._last

    def getBackgroundImage(self, dst=None):
        ref, h, w, cn, depth, _ = self._need_model("getBackgroundImage")
        out = dst if dst is not None else _empty(ref, (h, w) if cn == 1 else (h, w, cn), np.uint8 if depth == CV_8U else np.float32)
        d = Img(out)
        bind_stream(d)
        _lib.check(L.mi355cv_mog2GetBackgroundImage(self._h, _vp(d.ptr), d.step, d.w, d.h, d.type), "mog2GetBackgroundImage")
        return out

    def getModel(self):
        """the model in the reference's order, of the last frame's kind: (modesUsed h x w uint8, gmm h x w x nmixtures x 2 = {weight, variance},
        mean h x w x nmixtures x cn); slots at and above a pixel's count are zero.  Enough to checkpoint a camera."""
        ref, h, w, cn, _, m = self._need_model("getModel")
        modes, gmm, mean = _empty(ref, (h, w), np.uint8), _empty(ref, (h, w, m, 2), np.float32), _empty(ref, (h, w, m, cn), np.float32)
        ptr = lambda a: _vp(a.data_ptr() if torch is not None and isinstance(a, torch.Tensor) else a.ctypes.data)
        bind_stream(Img(modes))
        _lib.check(L.mi355cv_mog2GetModel(self._h, ptr(modes), ptr(gmm), ptr(mean)), "mog2GetModel")
        return modes, gmm, mean


def createBackgroundSubtractorMOG2(history=500, varThreshold=16, detectShadows=True):
    """cv::createBackgroundSubtractorMOG2"""
    return BackgroundSubtractorMOG2(history, varThreshold, detectShadows)


# ---- cv::calcOpticalFlowFarneback (modules/video/src/optflowgf.cpp; no HAL hook): mi355cv_calcOpticalFlowFarneback* and its stages
def _decline(entry, why):
    """a refusal the C ABI cannot see (it takes no type argument): counted in the decline ledger like the library's own"""
    L.mi355cv_noteDecline(entry.encode())
    raise NotImplementedError("mi355cv_%s: NOT_IMPLEMENTED for these arguments (%s); no CPU fallback in opencv_amd" % (entry, why))


def _f32(a, cn, entry, what):
    i = Img(a)
    if i.depth != CV_32F or i.cn != cn:
        _decline(entry, "%s must be CV_32FC%d" % (what, cn))
    return i


def calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
    """cv::calcOpticalFlowFarneback: dense flow between two CV_8UC1 frames, H x W x 2 float32 of the frames' kind (torch device tensors stay in HBM, numpy arrays are
    staged).  `flow` may be None (allocated) unless flags has OPTFLOW_USE_INITIAL_FLOW, which is served for one effective pyramid level only."""
    entry = "calcOpticalFlowFarneback"
    p, n = Img(prev), Img(next)
    if (p.depth, p.cn) != (CV_8U, 1) or (n.depth, n.cn) != (CV_8U, 1):
        _decline(entry, "frames must be CV_8UC1")
    if (p.w, p.h) != (n.w, n.h):
        raise ValueError("calcOpticalFlowFarneback: two frames of the same size")
    if flow is None:
        if flags & OPTFLOW_USE_INITIAL_FLOW:
            raise ValueError("calcOpticalFlowFarneback: OPTFLOW_USE_INITIAL_FLOW needs a flow")
        flow = _empty(prev, (p.h, p.w, 2), np.float32)
    f = _f32(flow, 2, entry, "flow")
    if (f.w, f.h) != (p.w, p.h):
        raise ValueError("calcOpticalFlowFarneback: flow must be H x W x 2 of the frames' size")
    bind_stream(p, n, f)
    _lib.check(L.mi355cv_calcOpticalFlowFarneback(_vp(p.ptr), p.step, _vp(n.ptr), n.step, _vp(f.ptr), f.step, p.w, p.h, float(pyr_scale), int(levels), int(winsize),
                                                  int(iterations), int(poly_n), float(poly_sigma), int(flags)), entry)
    return flow


def calcOpticalFlowFarnebackBatch(frames, flows, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags):
    """T consecutive CV_8UC1 frames stacked as T x H x W -> T - 1 flows (T - 1) x H x W x 2, flow i from frame i to frame i + 1, each bit for bit the single call's;
    every shared frame's level images and polynomial expansions are computed once."""
    entry = "calcOpticalFlowFarnebackBatch"
    if isinstance(frames, (list, tuple)):
        frames = torch.stack(list(frames)) if _is_dev(frames[0]) else np.stack([np.asarray(f) for f in frames])
    if frames.ndim != 3 or int(frames.shape[0]) < 2:
        raise ValueError("calcOpticalFlowFarnebackBatch: at least two frames stacked as T x H x W")
    t = int(frames.shape[0])
    s = Img(frames[0])
    if (s.depth, s.cn) != (CV_8U, 1):
        _decline(entry, "frames must be CV_8UC1")
    if flows is None:
        flows = _empty(frames, (t - 1, s.h, s.w, 2), np.float32)
    if flows.ndim != 4 or int(flows.shape[0]) != t - 1:
        raise ValueError("calcOpticalFlowFarnebackBatch: flows must be (T - 1) x H x W x 2")
    d = _f32(flows[0], 2, entry, "flows")
    if (d.w, d.h) != (s.w, s.h):
        raise ValueError("calcOpticalFlowFarnebackBatch: flows must be (T - 1) x H x W x 2")
    fstride = lambda a, esz: int(a.stride(0)) * esz if torch is not None and isinstance(a, torch.Tensor) else int(a.strides[0])
    bind_stream(s, d)
    _lib.check(L.mi355cv_calcOpticalFlowFarnebackBatch(_vp(s.ptr), s.step, fstride(frames, 1), t, _vp(d.ptr), d.step, fstride(flows, 4), s.w, s.h, float(pyr_scale), int(levels),
                                                       int(winsize), int(iterations), int(poly_n), float(poly_sigma), int(flags)), entry)
    return flows


def farnebackPolyExp(src, poly_n, poly_sigma, dst=None):
    """the polynomial expansion of a CV_32FC1 image: H x W x 5 float32 (y-linear, x-linear, yy, xx, xy)"""
    s = _f32(src, 1, "farnebackPolyExp", "src")
    out = dst if dst is not None else _empty(src, (s.h, s.w, 5), np.float32)
    d = _f32(out, 5, "farnebackPolyExp", "dst")
    bind_stream(s, d)
    _lib.check(L.mi355cv_farnebackPolyExp(_vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h, int(poly_n), float(poly_sigma)), "farnebackPolyExp")
    return out


def farnebackUpdateMatrices(R0, R1, flow, M=None):
    """M (G11, G12, G22, h1, h2; H x W x 5) from the two expansions and the flow"""
    e = "farnebackUpdateMatrices"
    a, b, f = _f32(R0, 5, e, "R0"), _f32(R1, 5, e, "R1"), _f32(flow, 2, e, "flow")
    out = M if M is not None else _empty(R0, (a.h, a.w, 5), np.float32)
    m = _f32(out, 5, e, "M")
    if len({(i.w, i.h) for i in (a, b, f, m)}) != 1:
        raise ValueError("farnebackUpdateMatrices: R0, R1, flow and M of one size")
    bind_stream(a, b, f, m)
    _lib.check(L.mi355cv_farnebackUpdateMatrices(_vp(a.ptr), a.step, _vp(b.ptr), b.step, _vp(f.ptr), f.step, _vp(m.ptr), m.step, a.w, a.h), e)
    return out


def farnebackUpdateFlow(M, winsize, flags=0, flow=None, R0=None, R1=None, M_next=None):
    """one iteration: the flow (H x W x 2) from the window sums of M.  With R0 and R1 the update matrix of the new flow is computed too, as every iteration but the
    last does: returns (flow, M_next) then, else the flow."""
    e = "farnebackUpdateFlow"
    m = _f32(M, 5, e, "M")
    out = flow if flow is not None else _empty(M, (m.h, m.w, 2), np.float32)
    f = _f32(out, 2, e, "flow")
    update = R0 is not None or R1 is not None
    if update:
        a, b = _f32(R0, 5, e, "R0"), _f32(R1, 5, e, "R1")
        nxt = M_next if M_next is not None else _empty(M, (m.h, m.w, 5), np.float32)
        n = _f32(nxt, 5, e, "M_next")
        bind_stream(m, f, a, b, n)
        rc = L.mi355cv_farnebackUpdateFlow(_vp(m.ptr), m.step, _vp(f.ptr), f.step, _vp(a.ptr), a.step, _vp(b.ptr), b.step, _vp(n.ptr), n.step, m.w, m.h, int(winsize), int(flags))
    else:
        bind_stream(m, f)
        rc = L.mi355cv_farnebackUpdateFlow(_vp(m.ptr), m.step, _vp(f.ptr), f.step, None, 0, None, 0, None, 0, m.w, m.h, int(winsize), int(flags))
    _lib.check(rc, e)
    return (out, nxt) if update else out
