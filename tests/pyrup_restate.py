"""cv::pyrUp restated in numpy (imgproc/src/pyramids.cpp, pyrUp_<CastOp>), the reference of tests/test_pyrup_cpu.py and tests/test_pyrup_gpu.py.

Destination 2w x 2h, BORDER_DEFAULT only.  Per axis, for a source line s[0..n-1] with s[-1] := s[min(1, n-1)] and s[n] := s[n-1]:
    even output 2i   : s[i-1] + s[i]*6 + s[i+1]
    odd  output 2i+1 : (s[i] + s[i+1])*4
rows first, then columns, in the wide type; cast (v + 32) >> 6 for CV_8U / CV_16U / CV_16S (arithmetic shift), v / 64 for CV_32F.  Channels are
independent.  Integers are evaluated in int64 (exact), CV_32F in float64."""
import numpy as np


def _axis(a, axis):
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    lo = np.concatenate([a[min(1, n - 1):min(1, n - 1) + 1], a[:-1]])     # s[i-1]
    hi = np.concatenate([a[1:], a[n - 1:]])                               # s[i+1]
    out = np.empty((2 * n,) + a.shape[1:], a.dtype)
    out[0::2] = lo + a * 6 + hi
    out[1::2] = (a + hi) * 4
    return np.moveaxis(out, 0, axis)


def pyrUp(src):
    """src: [H,W] or [H,W,C] of uint8 / uint16 / int16 / float32 -> [2H,2W(,C)] of the same type"""
    flt = src.dtype == np.float32
    v = _axis(_axis(src.astype(np.float64 if flt else np.int64), 1), 0)
    return (v / 64.0).astype(np.float32) if flt else ((v + 32) >> 6).astype(src.dtype)
