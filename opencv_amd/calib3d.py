"""Host-side mirror of cv::StereoBM (modules/calib3d; the reference has no HAL hook for it): the parameters with the reference's getters and setters, compute on one
rectified pair and computeBatch on N x H x W stacks.  The maps are made by mi355cv_stereoBM / mi355cv_stereoBMBatch (opencv_amd/csrc/stereobm.hip); torch device
tensors stay in HBM, numpy arrays are staged, the result has the kind of the input.  The definition served is the project's restatement.
cv::filterSpeckles (mi355cv_filterSpeckles / mi355cv_filterSpecklesBatch, opencv_amd/csrc/speckle.hip) works in place on the map where it lives.
cv::StereoSGBM (mi355cv_stereoSGBM / mi355cv_stereoSGBMBatch, opencv_amd/csrc/sgbm.hip) has the same surface: MODE_SGBM, MODE_HH and MODE_HH4.
The two ends of that pipeline (opencv_amd/csrc/undistort.hip): initUndistortRectifyMap, undistort / undistortRectify (+ Batch) in front of the matchers,
reprojectImageTo3D (+ Batch) behind them.  Out of scope: stereoRectify, getOptimalNewCameraMatrix, undistortPoints, the fisheye model."""
import ctypes

import numpy as np

from . import _lib
from .core import Img, bind_stream, torch, CV_8U, CV_16S, CV_32S, CV_32F, CV_MAKETYPE, INTER_LINEAR, BORDER_CONSTANT, empty_like_kind

__all__ = ["StereoBM", "StereoBM_create", "stereoPrefilterXSobel", "filterSpeckles", "filterSpecklesBatch", "PREFILTER_NORMALIZED_RESPONSE", "PREFILTER_XSOBEL", "StereoBM_PREFILTER_NORMALIZED_RESPONSE",
           "StereoBM_PREFILTER_XSOBEL", "StereoBM_DISP_SHIFT", "StereoBM_DISP_SCALE", "StereoSGBM", "StereoSGBM_create", "StereoSGBM_MODE_SGBM", "StereoSGBM_MODE_HH",
           "StereoSGBM_MODE_SGBM_3WAY", "StereoSGBM_MODE_HH4", "initUndistortRectifyMap", "undistort", "undistortBatch", "undistortRectify", "undistortRectifyBatch",
           "reprojectImageTo3D", "reprojectImageTo3DBatch"]

L = _lib.lib
PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1
StereoBM_PREFILTER_NORMALIZED_RESPONSE, StereoBM_PREFILTER_XSOBEL = 0, 1
StereoBM_DISP_SHIFT = 4
StereoBM_DISP_SCALE = 1 << StereoBM_DISP_SHIFT

_FIELDS = ("minDisparity", "numDisparities", "blockSize", "preFilterType", "preFilterSize", "preFilterCap", "textureThreshold", "uniquenessRatio", "speckleWindowSize",
           "speckleRange", "disp12MaxDiff")


class StereoBMParams(ctypes.Structure):
    """mi355cv_StereoBMParams"""
    _fields_ = [(f, ctypes.c_int) for f in _FIELDS] + [("roi1", ctypes.c_int * 4), ("roi2", ctypes.c_int * 4)]


def _vp(p):
    return ctypes.c_void_p(p)


def _decline(entry, why):
    """a refusal the C ABI cannot see (it takes no type argument for the inputs): counted in the decline ledger like the library's own"""
    L.mi355cv_noteDecline(entry.encode())
    raise NotImplementedError("mi355cv_%s: NOT_IMPLEMENTED for these arguments (%s); no CPU fallback in opencv_amd" % (entry, why))


def _empty(ref, shape, depth):
    if torch is not None and isinstance(ref, torch.Tensor):
        return torch.empty(shape, dtype=torch.int16 if depth == CV_16S else torch.float32, device=ref.device)
    return np.empty(shape, np.int16 if depth == CV_16S else np.float32)


def _frame_stride(a):
    return int(a.stride(0)) * a.element_size() if torch is not None and isinstance(a, torch.Tensor) else int(a.strides[0])


class _StereoMatcher:
    """what StereoBM and StereoSGBM share: the destination, compute on one pair, computeBatch on stacks.  A subclass names its two entries."""
    _single = _batch = None

    def _disp(self, ref, shape, disp, disptype, entry):
        if disp is None:
            if disptype not in (CV_16S, CV_32F):
                _decline(entry, "the disparity map is neither CV_16SC1 nor CV_32FC1")
            disp = _empty(ref, shape, disptype)
        if tuple(int(v) for v in disp.shape) != tuple(shape):
            raise ValueError("%s: disp must have the shape of the inputs" % entry)
        return disp

    def compute(self, left, right, disp=None, disptype=CV_16S):
        entry = self._single
        a, b = Img(left), Img(right)
        if (a.depth, a.cn) != (CV_8U, 1) or (b.depth, b.cn) != (CV_8U, 1):
            _decline(entry, "inputs must be CV_8UC1")
        if (a.w, a.h) != (b.w, b.h):
            raise ValueError("%s: two images of the same size" % entry)
        disp = self._disp(left, (a.h, a.w), disp, disptype, entry)
        d = Img(disp)
        if d.cn != 1 or d.depth not in (CV_16S, CV_32F):
            _decline(entry, "the disparity map is neither CV_16SC1 nor CV_32FC1")
        bind_stream(a, b, d)
        _lib.check(getattr(L, "mi355cv_" + entry)(_vp(a.ptr), a.step, _vp(b.ptr), b.step, _vp(d.ptr), d.step, a.w, a.h, d.depth, ctypes.byref(self._p)), entry)
        return disp

    def computeBatch(self, lefts, rights, disp=None, disptype=CV_16S):
        """N pairs stacked as N x H x W -> N x H x W maps, each bit for bit the single call's, in one sequence of launches"""
        entry = self._batch
        stack = lambda v: (torch.stack(list(v)) if torch is not None and isinstance(v[0], torch.Tensor) else np.stack([np.asarray(f) for f in v])) if isinstance(v, (list, tuple)) else v
        lefts, rights = stack(lefts), stack(rights)
        if lefts.ndim != 3 or tuple(lefts.shape) != tuple(rights.shape) or int(lefts.shape[0]) < 1:
            raise ValueError("%s: two stacks N x H x W of the same shape" % entry)
        n = int(lefts.shape[0])
        a, b = Img(lefts[0]), Img(rights[0])
        if (a.depth, a.cn) != (CV_8U, 1) or (b.depth, b.cn) != (CV_8U, 1):
            _decline(entry, "inputs must be CV_8UC1")
        disp = self._disp(lefts, (n, a.h, a.w), disp, disptype, entry)
        d = Img(disp[0])
        if d.depth not in (CV_16S, CV_32F):
            _decline(entry, "the disparity map is neither CV_16SC1 nor CV_32FC1")
        bind_stream(a, b, d)
        _lib.check(getattr(L, "mi355cv_" + entry)(_vp(a.ptr), a.step, _frame_stride(lefts), _vp(b.ptr), b.step, _frame_stride(rights), _vp(d.ptr), d.step, _frame_stride(disp), n,
                                                a.w, a.h, d.depth, ctypes.byref(self._p)), entry)
        return disp


class StereoBM(_StereoMatcher):
    """cv::StereoBM.  compute(left, right) -> the CV_16S map of disparities x 16 (pass disp= a float32 array / tensor, or disptype=CV_32F, for the CV_32F map of
    disparities); a pixel without a disparity holds (minDisparity - 1) * 16, respectively minDisparity - 1."""
    PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1
    DISP_SHIFT, DISP_SCALE = StereoBM_DISP_SHIFT, StereoBM_DISP_SCALE
    _single, _batch = "stereoBM", "stereoBMBatch"

    def __init__(self, numDisparities=0, blockSize=21):
        self._p = StereoBMParams()
        L.mi355cv_stereoBMDefaults(ctypes.byref(self._p))
        self._p.numDisparities = int(numDisparities)
        self._p.blockSize = int(blockSize)

    def getROI1(self): return tuple(self._p.roi1)
    def getROI2(self): return tuple(self._p.roi2)
    def setROI1(self, roi): self._p.roi1 = (ctypes.c_int * 4)(*[int(v) for v in roi])
    def setROI2(self, roi): self._p.roi2 = (ctypes.c_int * 4)(*[int(v) for v in roi])
    def getDefaultName(self): return "StereoMatcher.BM"


def _accessors(cls, name):
    cap = name[0].upper() + name[1:]
    setattr(cls, "get" + cap, lambda self: int(getattr(self._p, name)))
    setattr(cls, "set" + cap, lambda self, v: setattr(self._p, name, int(v)))


for _f in _FIELDS:
    _accessors(StereoBM, _f)


_SGBM_FIELDS = ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap", "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode")
StereoSGBM_MODE_SGBM, StereoSGBM_MODE_HH, StereoSGBM_MODE_SGBM_3WAY, StereoSGBM_MODE_HH4 = 0, 1, 2, 3


class StereoSGBMParams(ctypes.Structure):
    """mi355cv_StereoSGBMParams"""
    _fields_ = [(f, ctypes.c_int) for f in _SGBM_FIELDS]


class StereoSGBM(_StereoMatcher):
    """cv::StereoSGBM.  compute / computeBatch as StereoBM's: the CV_16S map of disparities x 16 or (disptype=CV_32F) the CV_32F map; a pixel without a disparity
    holds (minDisparity - 1) * 16, respectively minDisparity - 1.  speckleWindowSize > 0 is served: the map goes through filterSpeckles on the device."""
    MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3
    _single, _batch = "stereoSGBM", "stereoSGBMBatch"

    def __init__(self, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0, speckleWindowSize=0, speckleRange=0,
                 mode=StereoSGBM_MODE_SGBM):
        self._p = StereoSGBMParams()
        L.mi355cv_stereoSGBMDefaults(ctypes.byref(self._p))
        for f, v in zip(_SGBM_FIELDS, (minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange, mode)):
            setattr(self._p, f, int(v))

    def getDefaultName(self): return "StereoMatcher.SGBM"


for _f in _SGBM_FIELDS:
    _accessors(StereoSGBM, _f)


def StereoSGBM_create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0, speckleWindowSize=0, speckleRange=0,
                      mode=StereoSGBM_MODE_SGBM):
    """cv::StereoSGBM::create"""
    return StereoSGBM(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange, mode)


def StereoBM_create(numDisparities=0, blockSize=21):
    """cv::StereoBM::create"""
    return StereoBM(numDisparities, blockSize)


def stereoPrefilterXSobel(src, cap, dst=None):
    """the XSOBEL prefilter of StereoBM on one CV_8UC1 image (the stage entry)"""
    s = Img(src)
    if (s.depth, s.cn) != (CV_8U, 1):
        _decline("stereoPrefilterXSobel", "src must be CV_8UC1")
    if dst is None:
        dst = torch.empty((s.h, s.w), dtype=torch.uint8, device=src.device) if torch is not None and isinstance(src, torch.Tensor) else np.empty((s.h, s.w), np.uint8)
    d = Img(dst)
    if (d.depth, d.cn, d.w, d.h) != (CV_8U, 1, s.w, s.h):
        raise ValueError("stereoPrefilterXSobel: dst must be CV_8UC1 of the size of src")
    bind_stream(s, d)
    _lib.check(L.mi355cv_stereoPrefilterXSobel(_vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h, int(cap)), "stereoPrefilterXSobel")
    return dst


def _speckle_args(entry, newVal, maxSpeckleSize, maxDiff):
    # the reference takes newVal and maxDiff as double and truncates them to int
    try:
        return int(newVal), int(maxSpeckleSize), int(maxDiff)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: newVal, maxSpeckleSize and maxDiff must be finite numbers" % entry)


def _clamp_int(v):
    return max(-2 ** 31, min(2 ** 31 - 1, v))


def filterSpeckles(img, newVal, maxSpeckleSize, maxDiff, buf=None):
    """cv::filterSpeckles on one CV_8UC1 or CV_16SC1 map, IN PLACE: every connected component (4-neighbours with |a - b| <= maxDiff among the pixels != newVal) of at
    most maxSpeckleSize pixels becomes newVal.  Returns img: a device tensor stays in HBM, a numpy array is staged and written back into the same array.  buf is the
    reference's scratch argument: accepted and ignored."""
    entry = "filterSpeckles"
    if getattr(img, "ndim", 0) != 2:
        raise ValueError("filterSpeckles: img must be H x W")
    a = Img(img)
    newVal, maxSpeckleSize, maxDiff = _speckle_args(entry, newVal, maxSpeckleSize, maxDiff)
    if a.cn != 1 or a.depth not in (CV_8U, CV_16S):
        _decline(entry, "the image is neither CV_8UC1 nor CV_16SC1")
    bind_stream(a)
    _lib.check(L.mi355cv_filterSpeckles(_vp(a.ptr), a.step, a.w, a.h, a.depth, _clamp_int(newVal), _clamp_int(maxSpeckleSize), _clamp_int(maxDiff)), entry)
    return img


def filterSpecklesBatch(imgs, newVal, maxSpeckleSize, maxDiff, buf=None):
    """N maps stacked as N x H x W, each filtered in place bit for bit as the single call does, in one sequence of launches; the frame stride may exceed the frame"""
    entry = "filterSpecklesBatch"
    if getattr(imgs, "ndim", 0) != 3 or int(imgs.shape[0]) < 1:
        raise ValueError("filterSpecklesBatch: a stack N x H x W")
    a = Img(imgs[0])
    newVal, maxSpeckleSize, maxDiff = _speckle_args(entry, newVal, maxSpeckleSize, maxDiff)
    if a.cn != 1 or a.depth not in (CV_8U, CV_16S):
        _decline(entry, "the image is neither CV_8UC1 nor CV_16SC1")
    bind_stream(a)
    _lib.check(L.mi355cv_filterSpecklesBatch(_vp(a.ptr), a.step, _frame_stride(imgs), int(imgs.shape[0]), a.w, a.h, a.depth, _clamp_int(newVal), _clamp_int(maxSpeckleSize),
                                             _clamp_int(maxDiff)), entry)
    return imgs


# ---------------------------------------------------------------------------------------------------------------- rectification and reprojection
CV_32FC1, CV_32FC2, CV_16SC2 = CV_MAKETYPE(CV_32F, 1), CV_MAKETYPE(CV_32F, 2), CV_MAKETYPE(CV_16S, 2)


def _host(a):
    return a.detach().cpu().numpy() if torch is not None and isinstance(a, torch.Tensor) else np.asarray(a)


class _Camera:
    """K, distCoeffs, R, newCameraMatrix as the C ABI takes them: contiguous doubles, None -> NULL.  A 3 x 4 P gives its left 3 x 3."""

    def __init__(self, entry, K, dist, R=None, newK=None):
        def mat(m, name, cols=(3,)):
            if m is None:
                return None
            m = np.array(_host(m), np.float64)
            if m.ndim != 2 or m.shape[0] != 3 or m.shape[1] not in cols:
                raise ValueError("%s: %s must be 3 x %s" % (entry, name, " or 3 x ".join(str(c) for c in cols)))
            return np.ascontiguousarray(m[:, :3])
        self.K = mat(K, "cameraMatrix")
        if self.K is None:
            raise ValueError("%s: cameraMatrix is required" % entry)
        self.R, self.newK = mat(R, "R"), mat(newK, "newCameraMatrix", (3, 4))
        self.dist = np.zeros(0) if dist is None else np.ascontiguousarray(np.array(_host(dist), np.float64).ravel())

    def args(self):
        p = lambda m: None if m is None or m.size == 0 else _vp(m.ctypes.data)         # noqa: E731
        return p(self.K), p(self.dist), int(self.dist.size), p(self.R), p(self.newK)


def _size(entry, size):
    try:
        w, h = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("%s: size = (width, height)" % entry)
    return w, h


def _device_like(ref):
    return ref.device if torch is not None and isinstance(ref, torch.Tensor) else None


def initUndistortRectifyMap(cameraMatrix, distCoeffs, R, newCameraMatrix, size, m1type=CV_32FC1, map1=None, map2=None, device=None):
    """cv::initUndistortRectifyMap -> (map1, map2).  m1type CV_32FC1: two float maps; CV_32FC2: one, map2 is None; CV_16SC2: the fixed-point pair of cv::convertMaps.
    The maps are numpy arrays unless device= names a torch device (or map1 / map2 are given): they are made where they will be used."""
    entry = "initUndistortRectifyMap"
    cam = _Camera(entry, cameraMatrix, distCoeffs, R, newCameraMatrix)
    w, h = _size(entry, size)
    if m1type not in (CV_32FC1, CV_32FC2, CV_16SC2):
        _decline(entry, "m1type is none of CV_32FC1, CV_32FC2, CV_16SC2")
    shapes = {CV_32FC1: (((h, w), np.float32), ((h, w), np.float32)), CV_32FC2: (((h, w, 2), np.float32), None), CV_16SC2: (((h, w, 2), np.int16), ((h, w), np.uint16))}[m1type]

    def make(given, spec):
        if spec is None:
            return None
        shape, dt = spec
        if given is not None:
            if tuple(given.shape) != shape:
                raise ValueError("%s: a map of the wrong shape" % entry)
            return given
        if w < 1 or h < 1:
            return np.empty((0, 0), dt)
        if device is not None:
            return torch.empty(shape, dtype={np.float32: torch.float32, np.int16: torch.int16, np.uint16: torch.uint16}[dt], device=device)
        return np.empty(shape, dt)
    m1, m2 = make(map1, shapes[0]), make(map2, shapes[1])
    a = Img(m1) if m1.size else None
    b = Img(m2) if m2 is not None and m2.size else None
    bind_stream(a, b)
    _lib.check(L.mi355cv_initUndistortRectifyMap(*cam.args(), w, h, int(m1type), _vp(a.ptr if a else None), a.step if a else 0, _vp(b.ptr if b else None), b.step if b else 0), entry)
    return m1, m2


def _border_value(v):
    v = np.atleast_1d(np.asarray(v, np.float64)).ravel()
    return (ctypes.c_double * 4)(*(list(v) + [0.0] * 4)[:4]) if v.size > 1 else (ctypes.c_double * 4)(float(v[0]), 0.0, 0.0, 0.0)


def undistortRectify(src, cameraMatrix, distCoeffs, R=None, newCameraMatrix=None, dsize=None, interpolation=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0, dst=None):
    """the rectifying warp in one call: cv::remap(src, *cv::initUndistortRectifyMap(..., dsize, CV_16SC2), interpolation, borderMode, borderValue), bit for bit, without
    the maps where the tile kernel serves (CV_8U, 1 / 3 / 4 channels, INTER_LINEAR).  dsize = (width, height), None: the source's size."""
    entry = "undistortRectify"
    cam = _Camera(entry, cameraMatrix, distCoeffs, R, newCameraMatrix)
    s = Img(src)
    w, h = (s.w, s.h) if dsize is None else _size(entry, dsize)
    out = dst if dst is not None else empty_like_kind(src, max(h, 0), max(w, 0), s.cn, s.depth)
    d = Img(out)
    if (d.h, d.w, d.cn, d.depth) != (max(h, 0), max(w, 0), s.cn, s.depth):
        raise ValueError(entry + ": dst must have dsize and the type of the source")
    bind_stream(s, d)
    _lib.check(L.mi355cv_undistortRectify(s.type, _vp(s.ptr), s.step, s.w, s.h, _vp(d.ptr), d.step, w, h, *cam.args(), int(interpolation), int(borderMode),
                                          _border_value(borderValue)), entry)
    return out


def undistortRectifyBatch(frames, cameraMatrix, distCoeffs, R=None, newCameraMatrix=None, dsize=None, interpolation=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0,
                          dst=None):
    """N frames of one camera, N x H x W (x C): every frame bit for bit the single call's; the rule is evaluated once per destination tile for a group of frames"""
    entry = "undistortRectifyBatch"
    cam = _Camera(entry, cameraMatrix, distCoeffs, R, newCameraMatrix)
    frames = _stack(frames, entry)
    s = Img(frames[0])
    w, h = (s.w, s.h) if dsize is None else _size(entry, dsize)
    n = int(frames.shape[0])
    shape = (n, max(h, 0), max(w, 0)) + ((s.cn,) if frames.ndim == 4 else ())
    if dst is None:
        dst = torch.empty(shape, dtype=frames.dtype, device=frames.device) if torch is not None and isinstance(frames, torch.Tensor) else np.empty(shape, frames.dtype)
    if tuple(dst.shape) != shape or dst.dtype != frames.dtype or type(dst) is not type(frames):
        raise ValueError(entry + ": dst must be N x dsize of the kind and type of the frames")
    d = Img(dst[0])
    bind_stream(s, d)
    _lib.check(L.mi355cv_undistortRectifyBatch(s.type, _vp(s.ptr), s.step, _frame_stride(frames), s.w, s.h, _vp(d.ptr), d.step, _frame_stride(dst), w, h, n, *cam.args(),
                                               int(interpolation), int(borderMode), _border_value(borderValue)), entry)
    return dst


def _stack(frames, entry):
    if isinstance(frames, (list, tuple)):
        if not frames:
            raise ValueError("%s: an empty stack" % entry)
        frames = torch.stack(list(frames)) if torch is not None and isinstance(frames[0], torch.Tensor) else np.stack([np.asarray(f) for f in frames])
    elif not (torch is not None and isinstance(frames, torch.Tensor)):
        frames = np.asarray(frames)
    if frames.ndim not in (3, 4) or int(frames.shape[0]) < 1:
        raise ValueError("%s: a stack N x H x W or N x H x W x C" % entry)
    return frames


def undistort(src, cameraMatrix, distCoeffs, dst=None, newCameraMatrix=None):
    """cv::undistort: the rectifying warp with R absent, the source's size, INTER_LINEAR, BORDER_CONSTANT and border value 0"""
    return undistortRectify(src, cameraMatrix, distCoeffs, None, newCameraMatrix, None, INTER_LINEAR, BORDER_CONSTANT, 0, dst)


def undistortBatch(frames, cameraMatrix, distCoeffs, dst=None, newCameraMatrix=None):
    """cv::undistort over a stack N x H x W (x C) of one camera"""
    return undistortRectifyBatch(frames, cameraMatrix, distCoeffs, None, newCameraMatrix, None, INTER_LINEAR, BORDER_CONSTANT, 0, dst)


def _q16(entry, Q):
    Q = np.array(_host(Q), np.float64)
    if Q.shape != (4, 4):
        raise ValueError("%s: Q must be 4 x 4" % entry)
    return np.ascontiguousarray(Q)


def _points_like(ref, shape):
    if torch is not None and isinstance(ref, torch.Tensor):
        return torch.empty(shape, dtype=torch.float32, device=ref.device)
    return np.empty(shape, np.float32)


def _reproject_types(entry, a, ddepth):
    if a.cn != 1 or a.depth not in (CV_8U, CV_16S, CV_32S, CV_32F):
        _decline(entry, "the disparity is none of CV_8UC1, CV_16SC1, CV_32SC1, CV_32FC1")
    if ddepth not in (-1, CV_16S, CV_32S, CV_32F):
        raise ValueError("%s: ddepth is -1, CV_16S, CV_32S or CV_32F" % entry)
    if ddepth in (CV_16S, CV_32S):
        _decline(entry, "CV_16SC3 / CV_32SC3 output is not served")


def reprojectImageTo3D(disparity, Q, handleMissingValues=False, ddepth=-1, dst=None):
    """cv::reprojectImageTo3D: H x W disparity (CV_8U, CV_16S, CV_32S, CV_32F) -> H x W x 3 float32 points; a device tensor (the output of StereoBM / StereoSGBM
    compute) never leaves HBM.  handleMissingValues: the pixels at the frame's minimum get z = 10000."""
    entry = "reprojectImageTo3D"
    Q = _q16(entry, Q)
    if getattr(disparity, "ndim", 0) != 2:
        raise ValueError(entry + ": disparity must be H x W")
    a = Img(disparity)
    _reproject_types(entry, a, ddepth)
    out = dst if dst is not None else _points_like(disparity, (a.h, a.w, 3))
    d = Img(out)
    if (d.h, d.w, d.cn, d.depth) != (a.h, a.w, 3, CV_32F):
        raise ValueError(entry + ": dst must be H x W x 3 float32")
    bind_stream(a, d)
    _lib.check(L.mi355cv_reprojectImageTo3D(_vp(a.ptr), a.step, a.type, _vp(d.ptr), d.step, a.w, a.h, _vp(Q.ctypes.data), 1 if handleMissingValues else 0, int(ddepth)), entry)
    return out


def reprojectImageTo3DBatch(disparities, Q, handleMissingValues=False, ddepth=-1, dst=None):
    """N x H x W disparities -> N x H x W x 3 points, each frame bit for bit the single call's (handleMissingValues: every frame against its own minimum)"""
    entry = "reprojectImageTo3DBatch"
    Q = _q16(entry, Q)
    disparities = _stack(disparities, entry)
    if disparities.ndim != 3:
        raise ValueError(entry + ": a stack N x H x W")
    a = Img(disparities[0])
    _reproject_types(entry, a, ddepth)
    n = int(disparities.shape[0])
    out = dst if dst is not None else _points_like(disparities, (n, a.h, a.w, 3))
    if tuple(out.shape) != (n, a.h, a.w, 3) or type(out) is not type(disparities):
        raise ValueError(entry + ": dst must be N x H x W x 3 float32 of the kind of the disparities")
    d = Img(out[0])
    if d.depth != CV_32F:
        raise ValueError(entry + ": dst must be N x H x W x 3 float32 of the kind of the disparities")
    bind_stream(a, d)
    _lib.check(L.mi355cv_reprojectImageTo3DBatch(_vp(a.ptr), a.step, _frame_stride(disparities), a.type, _vp(d.ptr), d.step, _frame_stride(out), a.w, a.h, n,
                                                 _vp(Q.ctypes.data), 1 if handleMissingValues else 0, int(ddepth)), entry)
    return out
