"""cv::fastNlMeansDenoising on CV_8U, restated (TEST INFRASTRUCTURE, never imported by opencv_amd).

This is the PROJECT'S STATEMENT OF THE RULE, written out from the reference's fast_nlmeans_denoising_invoker.hpp and its DistSquared policy; there is no copy of the
reference's sources to hold it against here, so the GPU (opencv_amd/csrc/nlmeans.hip) is held to THIS text, bit for bit, and DESIGN 6.20 says so.

Inputs: a CV_8U image [H, W] or [H, W, cn], cn in 1 .. 4, float h, templateWindowSize tws, searchWindowSize sws.

Geometry.  th = tws // 2, sh = sws // 2; the sizes in use are T = 2 th + 1 and S = 2 sh + 1 (an even argument counts as the next odd value); the border is b = th + sh
and a pixel outside the image comes from BORDER_REFLECT_101 through the reference's borderInterpolate loop (reflect101 below, written out: no np.pad), a dimension of
length 1 mapping everything to index 0.  Images narrower or shorter than b are legal.

Weight table (double precision, once per call).  mult = INT_MAX // (S S 255); shift = the smallest p with (1 << p) >= T T; k = (1 << shift) / (T T);
len = int(255 255 cn / k + 1); for a in [0, len): d = a k, w = exp(-d / (h h cn)) with h h cn evaluated in float32 and the division and exp in double, a NaN counting as
1.0; weight = cvRound(mult w) (ties to even), 0 when below 0.001 mult.  The table is non-increasing, table[0] = mult, its non-zero entries are a prefix.

Per pixel (y, x), over every offset (dy, dx) in [-sh, sh]^2: D = the sum over the T x T patch and the channels of (ext(y+ty, x+tx, c) - ext(y+dy+ty, x+dx+tx, c))^2,
w = table[D >> shift], weights_sum += w, est[c] += w ext(y+dy, x+dx, c).  Result: uint32(est[c] + weights_sum // 2) // weights_sum, saturated to 8 bits; the addition
is unsigned (a constant image of 255 at 7 / 21: est = 2 147 440 680 fits an int32, est + weights_sum // 2 = 2 151 651 348 does not).  weights_sum >= mult > 0.

Two forms: denoise_loops (the sentences above, one pixel and one offset at a time) and denoise (numpy: one offset at a time over the whole image, the patch sums from a
summed-area table).  Sums of exact integers do not depend on their order, so the two, and any kernel, must agree bit for bit.

Colored (denoise_colored): cvtColor(COLOR_LBGR2Lab), the rule on channel 0 with h and cn = 1, the rule on channels 1 - 2 together with hColor and cn = 2,
cvtColor(COLOR_Lab2LBGR); the two conversions are passed in (the project's own, which its own suite pins)."""
import math

import numpy as np

INT_MAX = 2 ** 31 - 1


def reflect101(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT_101)"""
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def geometry(tws, sws, cn):
    th, sh = tws // 2, sws // 2
    T, S = 2 * th + 1, 2 * sh + 1
    shift = 0
    while (1 << shift) < T * T:
        shift += 1
    k = float(1 << shift) / float(T * T)
    return dict(th=th, sh=sh, T=T, S=S, b=th + sh, shift=shift, mult=min(INT_MAX // (S * S * 255), INT_MAX), k=k, len=int(255.0 * 255.0 * cn / k + 1.0))


def _hh(h, cn):
    return float(np.float32(np.float32(h) * np.float32(h)) * np.float32(cn))        # h * h * cn in float


def weight_table_loops(h, cn, tws, sws):
    """-> (table int64 [len], geometry, prefix): one entry at a time, math.exp"""
    g = geometry(tws, sws, cn)
    hh = _hh(h, cn)
    table = np.zeros(g["len"], np.int64)
    for a in range(g["len"]):
        d = a * g["k"]
        if hh == 0.0:
            w = float("nan") if d == 0.0 else 0.0                                     # -0 / 0 is NaN, -d / 0 is -inf and exp(-inf) = 0
        else:
            x = -d / hh
            w = 0.0 if x < -745.2 else math.exp(x)                                    # below the smallest subnormal's logarithm exp is 0 (math.exp never raises there, the guard only says so)
        if w != w:
            w = 1.0
        weight = int(round(g["mult"] * w))                                            # Python's round: to nearest, ties to even, as cvRound
        if weight < 0.001 * g["mult"]:
            weight = 0
        table[a] = weight
    return table, g, int(np.count_nonzero(table))


def weight_table(h, cn, tws, sws):
    """the same table in numpy"""
    g = geometry(tws, sws, cn)
    hh = np.float64(_hh(h, cn))
    d = np.arange(g["len"], dtype=np.float64) * g["k"]
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        w = np.exp(-d / hh)
    w[np.isnan(w)] = 1.0
    table = np.rint(g["mult"] * w).astype(np.int64)
    table[table < 0.001 * g["mult"]] = 0
    return table, g, int(np.count_nonzero(table))


def _planes(src):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    a = src if src.ndim == 3 else src[:, :, None]
    assert 1 <= a.shape[2] <= 4
    return a


def _finish(est, wsum):
    v = ((est + wsum // 2) & 0xFFFFFFFF) // wsum                                      # the unsigned 32-bit sum
    return min(int(v), 255)


def denoise_loops(src, h, tws=7, sws=21):
    """the rule, one pixel and one offset at a time (small images only)"""
    a = _planes(src)
    H, W, cn = a.shape
    table, g, _ = weight_table(h, cn, tws, sws)
    th, sh, shift = g["th"], g["sh"], g["shift"]

    def ext(y, x, c):
        return int(a[reflect101(y, H), reflect101(x, W), c])

    out = np.zeros_like(a)
    for y in range(H):
        for x in range(W):
            wsum, est = 0, [0] * cn
            for dy in range(-sh, sh + 1):
                for dx in range(-sh, sh + 1):
                    D = 0
                    for ty in range(-th, th + 1):
                        for tx in range(-th, th + 1):
                            for c in range(cn):
                                D += (ext(y + ty, x + tx, c) - ext(y + dy + ty, x + dx + tx, c)) ** 2
                    w = int(table[D >> shift])
                    wsum += w
                    for c in range(cn):
                        est[c] += w * ext(y + dy, x + dx, c)
            for c in range(cn):
                out[y, x, c] = _finish(est[c], wsum)
    return out.reshape(np.asarray(src).shape)


def denoise(src, h, tws=7, sws=21):
    """the rule in numpy: the extended image by the index rule, then per offset the squared differences over the whole extended image, their T x T sums from a
    summed-area table, one table gather"""
    a = _planes(src)
    H, W, cn = a.shape
    table, g, _ = weight_table(h, cn, tws, sws)
    th, sh, b, shift, T = g["th"], g["sh"], g["b"], g["shift"], g["T"]
    iy = np.array([reflect101(p, H) for p in range(-b, H + b)])
    ix = np.array([reflect101(p, W) for p in range(-b, W + b)])
    ext = a[iy][:, ix].astype(np.int64)                                               # ext[b + y, b + x] is pixel (y, x)
    Hc, Wc = H + 2 * th, W + 2 * th                                                   # the rows and columns a patch of an image pixel can touch
    base = ext[sh:sh + Hc, sh:sh + Wc]
    wsum = np.zeros((H, W), np.int64)
    est = np.zeros((H, W, cn), np.int64)
    for dy in range(-sh, sh + 1):
        for dx in range(-sh, sh + 1):
            other = ext[sh + dy:sh + dy + Hc, sh + dx:sh + dx + Wc]
            d2 = ((base - other) ** 2).sum(axis=2)
            sat = np.zeros((Hc + 1, Wc + 1), np.int64)
            sat[1:, 1:] = d2.cumsum(axis=0).cumsum(axis=1)
            D = sat[T:, T:] - sat[:-T, T:] - sat[T:, :-T] + sat[:-T, :-T]             # [H, W]: the patch centred on (y, x)
            w = table[D >> shift]
            wsum += w
            est += w[:, :, None] * ext[b + dy:b + dy + H, b + dx:b + dx + W]
    assert wsum.min() >= g["mult"] > 0 and est.max() <= INT_MAX
    v = ((est + (wsum // 2)[:, :, None]) & 0xFFFFFFFF) // wsum[:, :, None]
    return np.minimum(v, 255).astype(np.uint8).reshape(np.asarray(src).shape)


def denoise_colored(src, h, hColor, tws, sws, to_lab, from_lab):
    """to_lab: CV_8UC3 -> Lab by COLOR_LBGR2Lab, from_lab: Lab -> CV_8UC3 by COLOR_Lab2LBGR"""
    src = np.asarray(src)
    assert src.ndim == 3 and src.shape[2] == 3
    lab = np.ascontiguousarray(to_lab(src))
    out = np.empty_like(lab)
    out[:, :, 0] = denoise(lab[:, :, 0], h, tws, sws)
    out[:, :, 1:3] = denoise(lab[:, :, 1:3], hColor, tws, sws)
    return from_lab(out)


# ---- the noise test's image (tests/test_nlmeans_cpu.py, tests/test_nlmeans_gpu.py): 24 x 40, round(128 + 60 sin(x / 9) + 40 cos(y / 7)) plus Gaussian noise
NOISE_SEEDS = {10: 1, 20: 2}           # sigma -> the seed fixed for it


def noise_case(sigma):
    """-> (clean float64 [24, 40], noisy uint8 [24, 40])"""
    y, x = np.mgrid[0:24, 0:40]
    clean = np.rint(128 + 60 * np.sin(x / 9.0) + 40 * np.cos(y / 7.0))
    noise = np.random.default_rng(NOISE_SEEDS[sigma]).normal(0.0, sigma, clean.shape)
    return clean, np.clip(np.rint(clean + noise), 0, 255).astype(np.uint8)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
