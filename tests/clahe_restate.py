"""A numpy restatement of cv::CLAHE::apply (imgproc/src/clahe.cpp: CLAHE_Impl::apply, CLAHE_CalcLut_Body, CLAHE_Interpolation_Body; the ROI rule of
copyMakeBorder, core/src/copy.cpp).  Written from the rules, independent of the library and of opencv_amd/csrc: the tests compare the GPU path and the
host build of clahe_math.h against it bit for bit.  All per-pixel arithmetic is float32, each operation rounded on its own."""
import numpy as np

INT_MIN = -(1 << 31)


def reflect101(idx, n):
    """borderInterpolate(i, n, BORDER_REFLECT_101) for i >= 0"""
    idx = np.asarray(idx, np.int64)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    m = idx % period
    return np.where(m < n, m, period - m)


def clip_limit(clipLimit, area, histSize):
    """static_cast<int>(clipLimit * area / histSize), at least 1; 0 (no clipping) unless clipLimit > 0.  Past INT_MAX the x86-64 conversion gives INT_MIN."""
    if not clipLimit > 0.0:
        return 0
    d = clipLimit * area / histSize
    c = int(d) if d < 2147483648.0 else INT_MIN
    return max(c, 1)


def clip_hist(hist, clip):
    """hist [nT, histSize] -> clipped and redistributed (a copy)"""
    h = np.array(hist, dtype=np.int64, copy=True)
    if clip <= 0:
        return h
    histSize = h.shape[1]
    clipped = np.maximum(h - clip, 0).sum(axis=1)
    np.minimum(h, clip, out=h)
    batch = clipped // histSize
    residual = clipped - batch * histSize
    h += batch[:, None]
    for k in np.nonzero(residual)[0]:
        r = int(residual[k])
        step = max(histSize // r, 1)
        i = np.arange(0, histSize, step)[:r]
        h[k, i] += 1
    return h


def lut_from_hist(hist, clip, lut_scale, maxv):
    """saturate_cast<T>((float)sum * lutScale) over the running sum of the clipped histogram"""
    h = clip_hist(hist, clip)
    cs = np.cumsum(h, axis=1)
    assert cs.max() < (1 << 31)
    v = np.rint(cs.astype(np.float32) * np.float32(lut_scale))
    return np.clip(v, 0, maxv).astype(np.int64)


def plan(w, h, tiles, margins=(0, 0)):
    """(tw, th, readW, readH): tile size of the LUT source and the real pixels it is cut from (the image plus the parent margins copyMakeBorder takes in)"""
    tx, ty = tiles
    if w % tx == 0 and h % ty == 0:
        return w // tx, h // ty, w, h
    padR, padB = tx - w % tx, ty - h % ty                     # both sides as soon as one is not divisible
    return (w + padR) // tx, (h + padB) // ty, w + min(margins[0], padR), h + min(margins[1], padB)


def clahe(src, clipLimit=40.0, tiles=(8, 8), parent=None, origin=(0, 0)):
    """CLAHE of `src` (2-D uint8 or uint16).  parent / origin: src is parent[oy:oy + h, ox:ox + w], whose pixels right of / below it feed the padding."""
    src = np.asarray(src)
    assert src.ndim == 2 and src.dtype in (np.uint8, np.uint16)
    histSize = 256 if src.dtype == np.uint8 else 65536
    maxv = histSize - 1
    H, W = src.shape
    tx, ty = tiles
    if parent is None:
        parent, origin = src, (0, 0)
    ox, oy = origin
    margins = (parent.shape[1] - ox - W, parent.shape[0] - oy - H)
    tw, th, readW, readH = plan(W, H, tiles, margins)
    real = parent[oy:oy + readH, ox:ox + readW]
    ext = real[reflect101(np.arange(th * ty), readH)][:, reflect101(np.arange(tw * tx), readW)]
    area = tw * th
    # histograms of all tiles at once: tile k = ty * tilesX + tx
    nT = tx * ty
    tiles_px = ext.reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(nT, area).astype(np.int64)
    hist = np.bincount((tiles_px + np.arange(nT, dtype=np.int64)[:, None] * histSize).ravel(), minlength=nT * histSize).reshape(nT, histSize)
    lut_scale = np.float32(histSize - 1) / np.float32(area)
    lut = lut_from_hist(hist, clip_limit(clipLimit, area, histSize), lut_scale, maxv).reshape(ty, tx, histSize).astype(np.float32)

    def axis(n, t, tiles_n):
        inv = np.float32(1.0) / np.float32(t)
        f = np.arange(n).astype(np.float32) * inv - np.float32(0.5)
        t1 = np.floor(f).astype(np.int64)
        a = f - t1.astype(np.float32)
        a1 = np.float32(1.0) - a
        t2 = np.minimum(t1 + 1, tiles_n - 1)
        t1 = np.maximum(t1, 0)
        return t1, t2, a, a1

    tx1, tx2, xa, xa1 = axis(W, tw, tx)
    ty1, ty2, ya, ya1 = axis(H, th, ty)
    v = src.astype(np.int64)
    Y1, Y2 = ty1[:, None], ty2[:, None]
    X1, X2 = tx1[None, :], tx2[None, :]
    top = lut[Y1, X1, v] * xa1[None, :] + lut[Y1, X2, v] * xa[None, :]
    bot = lut[Y2, X1, v] * xa1[None, :] + lut[Y2, X2, v] * xa[None, :]
    res = top * ya1[:, None] + bot * ya[:, None]
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, maxv).astype(src.dtype)
