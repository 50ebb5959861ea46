"""The distance transform the library serves (mi355cv_distanceTransform; include/mi355cv.h), restated in numpy: the reference of tests/test_disttransform_cpu.py
and tests/test_disttransform_gpu.py.

Input CV_8UC1 [H, W].  A pixel is a site iff it is 0; pixels outside the image are not sites.  For an output pixel (y, x) the minimum over all sites (sy, sx) of
    DIST_L2 (precise)   (y - sy)^2 + (x - sx)^2   as an exact integer, then np.sqrt(np.float64(d2)).astype(np.float32)
    DIST_L1             |y - sy| + |x - sx|         as float32, or as uint8 saturated at 255
    DIST_C              max(|y - sy|, |x - sx|)     as float32
all in int64.  A frame without any site: every pixel NO_SITE_32F (float32) / NO_SITE_8U (uint8) -- the library's own rule, not the reference's.

`brute` takes the minimum over the list of sites directly.  `separable` takes it one axis at a time -- first over the sites of each column, then over the columns --
which is the same minimum (each metric is monotone in |dy| for a fixed dx), still by exhaustive search and still exact, and costs H*H*W + H*W*W instead of
(H*W)^2.  `integer` uses whichever is cheaper for the mask at hand; tests/test_disttransform_cpu.py holds the two against each other and against scipy."""
import numpy as np

DIST_L1, DIST_L2, DIST_C = 1, 2, 3
NO_SITE_32F = np.float32(31622776.0)          # sqrtf(1e15f)
NO_SITE_8U = 255
MAX_DIM = 16384                               # mi355cv_limit("disttransform_max_dim")
LIMIT_KEY = "disttransform_max_dim"
_FAR = np.int64(1) << 30                      # above every coordinate difference; its square fits int64
_CHUNK = 1 << 22                              # elements of a temporary


def _combine(metric, dy, dx):
    if metric == DIST_L2:
        return dy * dy + dx * dx
    if metric == DIST_L1:
        return dy + dx
    if metric == DIST_C:
        return np.maximum(dy, dx)
    raise ValueError("metric")


def brute(mask, metric):
    """int64 [H, W]: the minimum over the list of sites; None if the mask has no site"""
    mask = np.asarray(mask)
    h, w = mask.shape
    sy, sx = [v.astype(np.int64) for v in np.nonzero(mask == 0)]
    if sy.size == 0:
        return None
    yy, xx = [v.reshape(-1).astype(np.int64) for v in np.mgrid[0:h, 0:w]]
    out = np.empty(h * w, np.int64)
    step = max(1, _CHUNK // sy.size)
    for i in range(0, h * w, step):
        dy = np.abs(yy[i:i + step, None] - sy[None, :])
        dx = np.abs(xx[i:i + step, None] - sx[None, :])
        out[i:i + step] = _combine(metric, dy, dx).min(axis=1)
    return out.reshape(h, w)


def column_distance(mask):
    """int64 [H, W]: |y - sy| to the nearest site of the pixel's own column, _FAR where the column has none"""
    mask = np.asarray(mask)
    h, w = mask.shape
    rows = np.arange(h, dtype=np.int64)
    g = np.empty((h, w), np.int64)
    step = max(1, _CHUNK // (h * h))
    for x in range(0, w, step):
        site = mask[:, x:x + step] == 0                                                   # [sy, x]
        d = np.where(site[None, :, :], np.abs(rows[:, None, None] - rows[None, :, None]), _FAR)   # [y, sy, x]
        g[:, x:x + step] = d.min(axis=1)
    return g


def separable(mask, metric):
    """the same minimum, one axis at a time; None if the mask has no site"""
    mask = np.asarray(mask)
    if not (mask == 0).any():
        return None
    h, w = mask.shape
    g = column_distance(mask)
    cols = np.arange(w, dtype=np.int64)
    dx = np.abs(cols[:, None] - cols[None, :])                                            # [q, x]
    out = np.empty((h, w), np.int64)
    step = max(1, _CHUNK // (w * w))
    for y in range(0, h, step):
        out[y:y + step] = _combine(metric, g[y:y + step, None, :], dx[None, :, :]).min(axis=2)
    return out


def integer(mask, metric):
    mask = np.asarray(mask)
    h, w = mask.shape
    nsites = int((mask == 0).sum())
    return brute(mask, metric) if nsites * h * w <= h * w * (h + w) else separable(mask, metric)


def distanceTransform(mask, distanceType, dstType=np.float32):
    """the served result: float32, or uint8 (DIST_L1 only)"""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2
    dstType = np.dtype(dstType)
    assert dstType == np.float32 or (dstType == np.uint8 and distanceType == DIST_L1)
    d = integer(mask, distanceType)
    if d is None:
        return np.full(mask.shape, NO_SITE_8U if dstType == np.uint8 else NO_SITE_32F, dstType)
    if dstType == np.uint8:
        return np.minimum(d, 255).astype(np.uint8)
    if distanceType == DIST_L2:
        return np.sqrt(d.astype(np.float64)).astype(np.float32)
    return d.astype(np.float32)
