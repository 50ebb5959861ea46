"""cv::fastNlMeansDenoising / cv::fastNlMeansDenoisingColored (photo.hpp; fast_nlmeans_denoising_invoker.hpp) on CV_8U -> mi355cv_fastNlMeansDenoising / ...Batch /
...Colored / ...ColoredBatch (opencv_amd/csrc/nlmeans.hip).  Images and stacks are numpy arrays or tensors (device-resident or host); the result has the
kind of the input.  No pixels are computed here; what the library does not serve raises NotImplementedError and is counted in the decline ledger under the entry's name."""
import ctypes

import numpy as np

from . import _lib
from .core import Img, empty_like_kind, bind_stream, torch
from .features2d import NORM_L2

__all__ = ["fastNlMeansDenoising", "fastNlMeansDenoisingBatch", "fastNlMeansDenoisingColored", "fastNlMeansDenoisingColoredBatch", "fastNlMeansDenoisingMulti",
           "fastNlMeansDenoisingColoredMulti", "fastNlMeansWeights"]

L = _lib.lib


def _vp(p):
    return ctypes.c_void_p(p)


def _decline(entry, why):
    """a refusal the C ABI has no entry for: counted in the decline ledger like the library's own"""
    L.mi355cv_noteDecline(entry.encode())
    raise NotImplementedError("mi355cv_%s: NOT_IMPLEMENTED for these arguments (%s); no CPU fallback in opencv_amd" % (entry, why))


def _h_vector(h):
    v = np.atleast_1d(np.asarray(h, dtype=np.float32)).ravel()
    if v.size < 1:
        raise ValueError("h: a number or a vector of numbers")
    return np.ascontiguousarray(v)


def _windows(templateWindowSize, searchWindowSize):
    t, s = int(templateWindowSize), int(searchWindowSize)
    if t < 1 or s < 1:
        raise ValueError("templateWindowSize and searchWindowSize must be positive")            # CV_Assert(template_window_size > 0 && search_window_size > 0)
    return t, s


def _frame_stride(a):
    return int(a.stride(0)) * a.element_size() if torch is not None and isinstance(a, torch.Tensor) else int(a.strides[0])


def _stack(frames, entry):
    """a stack N x H x W (x C): a tensor, a numpy array, or a list of either"""
    if isinstance(frames, (list, tuple)):
        if not frames:
            raise ValueError("%s: an empty stack" % entry)
        frames = torch.stack(list(frames)) if torch is not None and isinstance(frames[0], torch.Tensor) else np.stack([np.asarray(f) for f in frames])
    elif not (torch is not None and isinstance(frames, torch.Tensor)):
        frames = np.asarray(frames)
    if frames.ndim not in (3, 4) or int(frames.shape[0]) < 1:
        raise ValueError("%s: a stack N x H x W or N x H x W x C" % entry)
    return frames


def _dst_like(ref, dst, entry):
    if dst is None:
        return torch.empty_like(ref, memory_format=torch.contiguous_format) if torch is not None and isinstance(ref, torch.Tensor) else np.empty(ref.shape, ref.dtype)
    if tuple(dst.shape) != tuple(ref.shape) or dst.dtype != ref.dtype or type(dst) is not type(ref):
        raise ValueError("%s: dst must have the kind, shape and type of the source" % entry)
    return dst


def fastNlMeansDenoising(src, h=3.0, templateWindowSize=7, searchWindowSize=21, dst=None):
    """cv::fastNlMeansDenoising(src, dst, h, templateWindowSize, searchWindowSize) on CV_8U with 1 .. 4 channels.  h: a number (a vector of one number counts as it; a
    per-channel vector and CV_16U are declined by the library; the NORM_L1 overload of the reference is not mirrored).  Even window sizes count as the next odd value."""
    entry = "fastNlMeansDenoising"
    t, sw = _windows(templateWindowSize, searchWindowSize)
    hv = _h_vector(h)
    s = Img(src)
    out = dst if dst is not None else empty_like_kind(src, s.h, s.w, s.cn, s.depth)
    d = Img(out)
    if (d.h, d.w, d.cn, d.depth) != (s.h, s.w, s.cn, s.depth):
        raise ValueError(entry + ": dst must have the size and type of the source")
    bind_stream(s, d)
    _lib.check(L.mi355cv_fastNlMeansDenoising(_vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h, s.depth, s.cn, _vp(hv.ctypes.data), int(hv.size), t, sw, NORM_L2), entry)
    return out


def fastNlMeansDenoisingBatch(frames, h=3.0, templateWindowSize=7, searchWindowSize=21, dst=None):
    """cv::fastNlMeansDenoising over a stack N x H x W (x C): every frame bit for bit the single call's.  Device-resident stacks run with the frame in the grid,
    host-resident ones (numpy, CPU tensors) cross PCIe in chunks through the library's pipeline."""
    entry = "fastNlMeansDenoisingBatch"
    t, sw = _windows(templateWindowSize, searchWindowSize)
    hv = _h_vector(h)
    frames = _stack(frames, entry)
    out = _dst_like(frames, dst, entry)
    s, d = Img(frames[0]), Img(out[0])
    bind_stream(s, d)
    _lib.check(L.mi355cv_fastNlMeansDenoisingBatch(_vp(s.ptr), s.step, _frame_stride(frames), _vp(d.ptr), d.step, _frame_stride(out), int(frames.shape[0]), s.w, s.h, s.depth,
                                                   s.cn, _vp(hv.ctypes.data), int(hv.size), t, sw, NORM_L2), entry)
    return out


def fastNlMeansDenoisingColored(src, h=3.0, hColor=3.0, templateWindowSize=7, searchWindowSize=21, dst=None):
    """cv::fastNlMeansDenoisingColored on CV_8UC3: COLOR_LBGR2Lab, the rule on L with h and on a, b together with hColor, COLOR_Lab2LBGR.  CV_8UC4 is declined."""
    entry = "fastNlMeansDenoisingColored"
    t, sw = _windows(templateWindowSize, searchWindowSize)
    s = Img(src)
    out = dst if dst is not None else empty_like_kind(src, s.h, s.w, s.cn, s.depth)
    d = Img(out)
    if (d.h, d.w, d.cn, d.depth) != (s.h, s.w, s.cn, s.depth):
        raise ValueError(entry + ": dst must have the size and type of the source")
    bind_stream(s, d)
    _lib.check(L.mi355cv_fastNlMeansDenoisingColored(_vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h, s.depth, s.cn, float(h), float(hColor), t, sw), entry)
    return out


def fastNlMeansDenoisingColoredBatch(frames, h=3.0, hColor=3.0, templateWindowSize=7, searchWindowSize=21, dst=None):
    """cv::fastNlMeansDenoisingColored over a stack N x H x W x 3"""
    entry = "fastNlMeansDenoisingColoredBatch"
    t, sw = _windows(templateWindowSize, searchWindowSize)
    frames = _stack(frames, entry)
    out = _dst_like(frames, dst, entry)
    s, d = Img(frames[0]), Img(out[0])
    bind_stream(s, d)
    _lib.check(L.mi355cv_fastNlMeansDenoisingColoredBatch(_vp(s.ptr), s.step, _frame_stride(frames), _vp(d.ptr), d.step, _frame_stride(out), int(frames.shape[0]), s.w, s.h,
                                                          s.depth, s.cn, float(h), float(hColor), t, sw), entry)
    return out


def fastNlMeansDenoisingMulti(srcImgs, imgToDenoiseIndex, temporalWindowSize, h=3.0, templateWindowSize=7, searchWindowSize=21, dst=None):
    """cv::fastNlMeansDenoisingMulti: not built"""
    _decline("fastNlMeansDenoisingMulti", "the temporal variants are not built; fastNlMeansDenoisingBatch denoises every frame on its own")


def fastNlMeansDenoisingColoredMulti(srcImgs, imgToDenoiseIndex, temporalWindowSize, h=3.0, hColor=3.0, templateWindowSize=7, searchWindowSize=21, dst=None):
    """cv::fastNlMeansDenoisingColoredMulti: not built"""
    _decline("fastNlMeansDenoisingColoredMulti", "the temporal variants are not built; fastNlMeansDenoisingColoredBatch denoises every frame on its own")


def fastNlMeansWeights(h, cn=1, templateWindowSize=7, searchWindowSize=21):
    """the integer weight table of the rule, built on the host by the library (mi355cv_fastNlMeansWeights; touches no device)
    -> (table int32 [len], shift, mult, prefix): table[D >> shift] is the weight of patch distance D, table[0] = mult, the first `prefix` entries are non-zero"""
    t, sw = _windows(templateWindowSize, searchWindowSize)
    info = (ctypes.c_int * 4)()
    _lib.check(L.mi355cv_fastNlMeansWeights(float(h), int(cn), t, sw, None, 0, info), "fastNlMeansWeights")
    table = np.zeros(info[0], np.int32)
    _lib.check(L.mi355cv_fastNlMeansWeights(float(h), int(cn), t, sw, _vp(table.ctypes.data), int(table.size), info), "fastNlMeansWeights")
    return table, int(info[1]), int(info[2]), int(info[3])
