"""cv::calcHist and cv::calcBackProject restated twice, independently: plain Python loops (*_loops) and a vectorised numpy form (*_vec).  This file is the contract
of mi355cv_calcHist* and mi355cv_calcBackProject* (include/mi355cv.h); the reference's sources were not available, so the definition below is this restatement's.

  image        one interleaved image of cn = 1 .. 4 channels, CV_8U, CV_16U or CV_32F; dims in {1, 2, 3}; channels[d] in [0, cn), repeats and any order allowed;
               histSize[d] = n_d >= 1; mask optional, CV_8UC1, non-zero selects
  uniform      (lo_d, hi_d) as float32, lo < hi, finite.  In IEEE double a = n / ((double)hi - (double)lo), b = -a * lo; t = v * a + b with the product and the sum
               rounded SEPARATELY (a fused multiply-add is a different function).  CV_8U / CV_16U: v is counted iff lo <= v < hi, bin = min(max(floor(t), 0), n - 1).
               CV_32F: v is counted iff 0 <= t < n (NaN, +-inf and everything else that fails the comparison is not counted), bin = floor(t)
  non-uniform  n_d + 1 strictly ascending finite float32 boundaries r: the bin is the k with r[k] <= v < r[k + 1], outside [r[0], r[n]) not counted; CV_8U and
               CV_16U only
  counting     a pixel is counted iff the mask selects it and every dimension counts it; it adds 1 to the dense row-major cell [b0][b1][b2]; counts are exact
               32-bit integers, returned as CV_32S (int32) or CV_32F ((float)count, round to nearest even)
  accumulate   the starting count of a cell is the incoming value: CV_32S as it is, CV_32F through cvRound (ties to even) saturated to int32
  back-project the same bin rule, no mask; hist dense CV_32F of shape histSize; a pixel some dimension does not count gets 0, otherwise p = (double)hist[bin] * scale:
               CV_8U / CV_16U cvRound(p) (ties to even) saturated to the type, CV_32F (float)p

Python floats are IEEE doubles and every operation below is one rounding, so `v * a + b` written in Python IS the two-rounding form."""
import math

import numpy as np

MAX_DIM_KEY = "calchist_max_dim"
MAX_BINS_KEY = "calchist_max_bins"
MAX_DIM = 16384
MAX_BINS = 1 << 20
MAX_BINS_PER_DIM = 65536
DEPTHS = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 2, np.dtype(np.float32): 5}
CV_32S, CV_32F = 4, 5


def _split_ranges(hist_size, ranges, uniform):
    """ranges: flat floats (2 per dimension, or n_d + 1 per dimension), or one sequence per dimension -> a list of float32 arrays"""
    flat = np.concatenate([np.asarray(r, np.float32).ravel() for r in ranges]) if len(ranges) and np.ndim(ranges[0]) else np.asarray(ranges, np.float32).ravel()
    out, o = [], 0
    for n in hist_size:
        k = 2 if uniform else n + 1
        out.append(flat[o:o + k])
        o += k
    assert o == flat.size, "ranges do not match histSize"
    return out


def flat_ranges(hist_size, ranges, uniform):
    return np.concatenate(_split_ranges(hist_size, ranges, uniform)).astype(np.float32)


def coef(n, lo, hi):
    a = float(n) / (float(np.float32(hi)) - float(np.float32(lo)))
    return a, -a * float(np.float32(lo))


# ---- the loops
def bin_loops(v, kind, n, r, uniform):
    """the bin of one value (a Python int for 8- and 16-bit images, a float for CV_32F), None: not counted"""
    if uniform:
        lo, hi = float(r[0]), float(r[1])
        a, b = coef(n, lo, hi)
        if kind == "f":
            t = float(v) * a + b
            if not (0.0 <= t < n):
                return None
            return int(math.floor(t))
        if not (lo <= v < hi):
            return None
        t = float(v) * a + b
        return min(max(int(math.floor(t)), 0), n - 1)
    for k in range(n):
        if float(r[k]) <= v < float(r[k + 1]):
            return k
    return None


def round_half_even_sat(p, lo, hi):
    """cvRound (ties to even) of a double, saturated to [lo, hi]"""
    if p != p:
        return 0
    if p <= lo - 1:
        return lo
    if p >= hi + 1:
        return hi
    f = math.floor(p)
    d = p - f                                  # exact: |p| < 2^32
    r = f + 1 if d > 0.5 or (d == 0.5 and f % 2 == 1) else f
    return int(min(max(r, lo), hi))


def start_counts(hist):
    """accumulate: the incoming cells as counts"""
    hist = np.asarray(hist)
    if hist.dtype == np.int32:
        return hist.astype(np.int64)
    assert hist.dtype == np.float32
    out = np.zeros(hist.shape, np.int64)
    flat = out.reshape(-1)
    for i, v in enumerate(hist.reshape(-1)):
        flat[i] = round_half_even_sat(float(v), -2 ** 31, 2 ** 31 - 1)
    return out


def finish(counts, hist_depth):
    counts = np.asarray(counts, np.int64)
    assert counts.min(initial=0) >= -2 ** 31 and counts.max(initial=0) <= 2 ** 31 - 1
    return counts.astype(np.int32) if hist_depth == CV_32S else counts.astype(np.int32).astype(np.float32)       # int32 -> float32 rounds to nearest even


def _channels_view(img):
    return img[:, :, None] if img.ndim == 2 else img


def calchist_loops(img, channels, mask, hist_size, ranges, uniform=True, hist_depth=CV_32F, start=None):
    img = _channels_view(np.asarray(img))
    kind = "f" if img.dtype == np.float32 else "i"
    rs = _split_ranges(hist_size, ranges, uniform)
    counts = np.zeros(tuple(hist_size), np.int64) if start is None else start_counts(start).reshape(tuple(hist_size)).copy()
    h, w = img.shape[:2]
    for y in range(h):
        for x in range(w):
            if mask is not None and mask[y, x] == 0:
                continue
            cell = []
            for d, c in enumerate(channels):
                v = float(img[y, x, c]) if kind == "f" else int(img[y, x, c])
                k = bin_loops(v, kind, hist_size[d], rs[d], uniform)
                if k is None:
                    break
                cell.append(k)
            else:
                counts[tuple(cell)] += 1
    return finish(counts, hist_depth)


def backproject_loops(img, channels, hist, ranges, scale, uniform=True):
    img = _channels_view(np.asarray(img))
    hist = np.asarray(hist, np.float32)
    hist_size = hist.shape
    kind = "f" if img.dtype == np.float32 else "i"
    rs = _split_ranges(hist_size, ranges, uniform)
    h, w = img.shape[:2]
    out = np.zeros((h, w), img.dtype)
    for y in range(h):
        for x in range(w):
            cell = []
            for d, c in enumerate(channels):
                v = float(img[y, x, c]) if kind == "f" else int(img[y, x, c])
                k = bin_loops(v, kind, hist_size[d], rs[d], uniform)
                if k is None:
                    break
                cell.append(k)
            else:
                p = float(hist[tuple(cell)]) * float(scale)
                if kind == "f":
                    out[y, x] = np.float32(p)
                else:
                    out[y, x] = round_half_even_sat(p, 0, int(np.iinfo(img.dtype).max))
    return out


# ---- the vectorised form, written on its own
def table(levels, n, r, uniform):
    """per value 0 .. levels - 1 of an 8- or 16-bit depth: the bin, or -1"""
    v = np.arange(levels, dtype=np.float64)
    r = np.asarray(r, np.float32).astype(np.float64)
    if uniform:
        a = np.float64(n) / (r[1] - r[0])
        b = -a * r[0]
        t = np.floor(v * a + b)                # numpy: a product array, then a sum array -- two roundings
        k = np.clip(t, 0, n - 1).astype(np.int64)
        return np.where((v >= r[0]) & (v < r[1]), k, -1)
    k = np.searchsorted(r, v, side="right") - 1          # the last boundary <= v
    return np.where((k >= 0) & (k < n), k, -1).astype(np.int64)


def bins_vec(plane, n, r, uniform):
    """the bin of every element of one channel plane, -1: not counted"""
    if plane.dtype == np.float32:
        assert uniform
        r = np.asarray(r, np.float32).astype(np.float64)
        a = np.float64(n) / (r[1] - r[0])
        b = -a * r[0]
        with np.errstate(invalid="ignore", over="ignore"):
            prod = plane.astype(np.float64) * a
            t = prod + b
            ok = (t >= 0) & (t < n)             # NaN compares false
            return np.where(ok, np.floor(np.where(ok, t, 0.0)), -1).astype(np.int64)
    return table(256 if plane.dtype == np.uint8 else 65536, n, r, uniform)[plane]


def _cells_vec(img, channels, hist_size, ranges, uniform):
    img = _channels_view(np.asarray(img))
    rs = _split_ranges(hist_size, ranges, uniform)
    cell = np.zeros(img.shape[:2], np.int64)
    ok = np.ones(img.shape[:2], bool)
    for d, c in enumerate(channels):
        k = bins_vec(img[:, :, c], hist_size[d], rs[d], uniform)
        ok &= k >= 0
        cell = cell * hist_size[d] + np.maximum(k, 0)
    return cell, ok


def calchist_vec(img, channels, mask, hist_size, ranges, uniform=True, hist_depth=CV_32F, start=None):
    cell, ok = _cells_vec(img, channels, hist_size, ranges, uniform)
    if mask is not None:
        ok = ok & (np.asarray(mask) != 0)
    total = int(np.prod(hist_size))
    counts = np.bincount(cell[ok], minlength=total).astype(np.int64)
    if start is not None:
        s = np.asarray(start).reshape(-1)
        counts += s.astype(np.int64) if s.dtype == np.int32 else np.clip(np.rint(s.astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)   # rint: ties to even
    return finish(counts.reshape(tuple(hist_size)), hist_depth)


def backproject_vec(img, channels, hist, ranges, scale, uniform=True):
    hist = np.asarray(hist, np.float32)
    cell, ok = _cells_vec(img, channels, hist.shape, ranges, uniform)
    p = hist.reshape(-1).astype(np.float64)[cell] * np.float64(scale)
    dt = np.asarray(img).dtype
    if dt == np.float32:
        with np.errstate(over="ignore"):
            return np.where(ok, p.astype(np.float32), np.float32(0))
    top = np.iinfo(dt).max
    return np.where(ok, np.clip(np.rint(p), 0, top), 0).astype(dt)


# ---- values for which a fused multiply-add gives another bin
def fma_sensitive(n, lo, hi, candidates):
    """those float32 candidates v whose bin under t = fl(fl(v * a) + b) differs from the bin under the single rounding fl(v * a + b), decided in exact rational
    arithmetic; returns [(v, bin_two_roundings, bin_fused)]"""
    from fractions import Fraction
    a, b = coef(n, lo, hi)
    out = []
    for v in candidates:
        v = float(np.float32(v))
        two = v * a + b
        exact = Fraction(v) * Fraction(a) + Fraction(b)
        fused = float(exact)                   # Fraction -> float rounds to nearest even: the fused result
        if math.floor(two) != math.floor(fused) and 0.0 <= two < n and 0.0 <= fused < n:
            out.append((np.float32(v), int(math.floor(two)), int(math.floor(fused))))
    return out


def fma_candidates(n, lo, hi):
    """float32 values just around the points where t crosses an integer: where the two forms can differ"""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    c = []
    for k in range(1, n):
        x = np.float32(lo + (hi - lo) * k / n)
        for _ in range(3):
            x = np.nextafter(x, np.float32(-np.inf))
        for _ in range(7):
            c.append(np.float32(x))
            x = np.nextafter(x, np.float32(np.inf))
    return c


# uniform CV_32F ranges whose a and b are not exact; the last three hold a float32 (0.22) whose t lies within half an ulp below an integer: fused, it is that integer
FMA_RANGES = ((64, 0.1, 0.9), (180, 0.3, 179.7), (7, -1.5, 2.25), (100, 0.1, 0.7), (50, 0.1, 0.7), (200, 0.1, 0.7))
F32_SPECIALS = [np.nan, np.inf, -np.inf, -0.0, 0.0]


def f32_special_values(lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    return [np.float32(v) for v in F32_SPECIALS] + [lo, hi, np.nextafter(hi, np.float32(-np.inf)), np.nextafter(lo, np.float32(-np.inf))]
