"""Host-side mirror of cv::StereoBM (modules/calib3d; the reference has no HAL hook for it): the parameters with the reference's getters and setters, compute on one
rectified pair and computeBatch on N x H x W stacks.  The maps are made by mi355cv_stereoBM / mi355cv_stereoBMBatch (opencv_amd/csrc/stereobm.hip); torch device
tensors stay in HBM, numpy arrays are staged, the result has the kind of the input.  The definition served is the project's restatement.
cv::filterSpeckles (mi355cv_filterSpeckles / mi355cv_filterSpecklesBatch, opencv_amd/csrc/speckle.hip) works in place on the map where it lives.
cv::StereoSGBM (mi355cv_stereoSGBM / mi355cv_stereoSGBMBatch, opencv_amd/csrc/sgbm.hip) has the same surface: MODE_SGBM, MODE_HH and MODE_HH4."""
import ctypes

import numpy as np

from . import _lib
from .core import Img, bind_stream, torch, CV_8U, CV_16S, CV_32F

__all__ = ["StereoBM", "StereoBM_create", "stereoPrefilterXSobel", "filterSpeckles", "filterSpecklesBatch", "PREFILTER_NORMALIZED_RESPONSE", "PREFILTER_XSOBEL", "StereoBM_PREFILTER_NORMALIZED_RESPONSE",
           "StereoBM_PREFILTER_XSOBEL", "StereoBM_DISP_SHIFT", "StereoBM_DISP_SCALE", "StereoSGBM", "StereoSGBM_create", "StereoSGBM_MODE_SGBM", "StereoSGBM_MODE_HH",
           "StereoSGBM_MODE_SGBM_3WAY", "StereoSGBM_MODE_HH4"]

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
