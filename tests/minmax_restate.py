"""cv::minMaxLoc restated twice, independently: plain Python loops (minmax_loops) and a vectorised numpy form (minmax_vec).  This file is the contract of
mi355cv_minMaxLoc* (include/mi355cv.h); the reference's sources were not available, so the treatment of NaN, of infinities and of the empty candidate set is
this restatement's.

  source       one channel of CV_8U, CV_8S, CV_16U, CV_16S, CV_32S, CV_32F or CV_64F
  mask         optional, CV_8UC1 of the same size; non-zero selects a pixel
  candidates   the selected pixels whose value is not NaN
  minVal       the least candidate value; minLoc the first pixel in raster order (y, then x) that holds it
  maxVal       the greatest candidate value; maxLoc the FIRST pixel in raster order that holds it
  values       returned as double, exactly (double)element; -0.0 == +0.0, so the earlier of the two wins a tie and the sign of a returned zero is unspecified
               (compare with ==); +-inf are ordinary values
  empty set    (mask all zero, every pixel NaN, or both) -> (0.0, 0.0, (-1, -1), (-1, -1))

Both return (minVal, maxVal, (minX, minY), (maxX, maxY)) with Python floats and ints."""
import math

import numpy as np

MAX_DIM_KEY = "minmax_max_dim"
MAX_DIM = 16384
DEPTHS = {np.dtype(np.uint8): 0, np.dtype(np.int8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3, np.dtype(np.int32): 4, np.dtype(np.float32): 5,
          np.dtype(np.float64): 6}
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.int32, np.float32, np.float64]
EMPTY = (0.0, 0.0, (-1, -1), (-1, -1))


def minmax_loops(a, mask=None):
    h, w = a.shape
    best_min = best_max = None                 # (value, x, y)
    for y in range(h):
        for x in range(w):
            if mask is not None and mask[y, x] == 0:
                continue
            v = float(a[y, x])                 # exact for every depth: 32-bit integers and floats fit a double
            if math.isnan(v):
                continue
            if best_min is None or v < best_min[0]:
                best_min = (v, x, y)
            if best_max is None or v > best_max[0]:
                best_max = (v, x, y)
    if best_min is None:
        return EMPTY
    return best_min[0], best_max[0], (best_min[1], best_min[2]), (best_max[1], best_max[2])


def minmax_vec(a, mask=None):
    h, w = a.shape
    d = a.astype(np.float64)
    out = np.isnan(d)
    if mask is not None:
        out = out | (np.asarray(mask) == 0)
    if out.all():
        return EMPTY
    lo = np.nanmin(np.where(out, np.nan, d))
    hi = np.nanmax(np.where(out, np.nan, d))
    flat = np.where(out, np.nan, d).ravel()
    first_lo = int(np.flatnonzero(flat == lo)[0])          # explicit first-index search; NaN == x is False, -0.0 == 0.0 is True
    first_hi = int(np.flatnonzero(flat == hi)[0])
    return float(lo), float(hi), (first_lo % w, first_lo // w), (first_hi % w, first_hi // w)


def same(got, want):
    """bit for bit up to the sign of a zero: values with ==, locations exactly"""
    return (float(got[0]) == float(want[0]) and float(got[1]) == float(want[1]) and tuple(int(v) for v in got[2]) == tuple(want[2])
            and tuple(int(v) for v in got[3]) == tuple(want[3]))


def type_extremes(dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        fi = np.finfo(dt)
        return [fi.min, fi.max, -np.inf, np.inf, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal, 0.0, -0.0]
    ii = np.iinfo(dt)
    return [ii.min, ii.max, 0, ii.min + 1, ii.max - 1]


def random_frame(rng, h, w, dtype, levels=None, nan=0.0, special=True):
    """levels: draw from that many distinct values (ties are the rule); None: the full range.  nan: the share of NaN pixels (floats).  special: plant the type's
    extremes (floats: +-inf, denormals, +-0 too) at random pixels"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        if levels:
            pool = rng.standard_normal(levels).astype(dt)
            a = pool[rng.integers(0, levels, (h, w))]
        else:
            bits = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
            if dt == np.float64:
                a = (rng.standard_normal((h, w)) * 10.0 ** rng.integers(-300, 300, (h, w)).astype(np.float64)).astype(np.float64)
            else:
                a = bits.view(np.float32).copy()
                a[np.isnan(a)] = 1.5
    else:
        ii = np.iinfo(dt)
        if levels:
            pool = rng.integers(ii.min, int(ii.max) + 1, levels, dtype=np.int64)
            a = pool[rng.integers(0, levels, (h, w))].astype(dt)
        else:
            a = rng.integers(ii.min, int(ii.max) + 1, (h, w), dtype=np.int64).astype(dt)
    a = np.ascontiguousarray(a)
    if special and h * w >= 16:
        ext = type_extremes(dt)
        at = rng.choice(h * w, len(ext), replace=False)
        a.ravel()[at] = np.array(ext, dt)
    if nan > 0 and dt.kind == "f":
        a[rng.random((h, w)) < nan] = np.nan
    return a
