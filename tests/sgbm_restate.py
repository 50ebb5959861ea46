"""cv::StereoSGBM as this project serves it, restated twice (TEST INFRASTRUCTURE, never imported by opencv_amd): once in plain loops (`*_loops`), the
normative text, and once in numpy (`*_np`), vectorised over the disparity index k and over the pixels orthogonal to a scan, which is what the GPU tests hold the device
maps against.  tests/test_sgbm_cpu.py holds the two against each other, stage by stage.  All arithmetic is exact integers.

  prefilter     G = clip(2 g(y) + g(y-) + g(y+), -ft, ft) + ft, g(r) = I[r][x+1] - I[r][x-1], rows REPLICATED, the two border columns ft; ft = max(preFilterCap, 15) | 1
  valid columns xlo = max(Dmax, 0) <= X < xhi = min(W, W + m), W1 = xhi - xlo; everything outside is FILTERED = (m - 1) * 16
  pixel cost    Birchfield-Tomasi on the planes (G, shift 0) and (raw I, shift 2)
  block cost    the w x w sum, rows clamped to the image, columns clamped to the VALID range
  paths         L_r(p, k) = C(p, k) + min(L_r(p-r, k), L_r(p-r, k-1) + P1, L_r(p-r, k+1) + P1, M + P2) - M, M = min_k L_r(p-r, k); L_r = C where p - r is outside
  decision      the smallest k with the smallest S, the uniqueness reject, the sub-pixel quotient with C division
  left-right    always; one vote per kept pixel into x2 = X - (best + m), the smallest S wins, ties to the larger x
"""
import collections

import numpy as np

MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3
# a direction (ry, rx) is the step from the predecessor to the pixel
DIRECTIONS = {
    MODE_HH: ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)),
    MODE_SGBM: ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1)),
    MODE_HH4: ((0, 1), (0, -1), (1, 0), (-1, 0)),
}

_P = collections.namedtuple("Params", "minDisparity numDisparities blockSize P1 P2 disp12MaxDiff preFilterCap uniquenessRatio speckleWindowSize speckleRange mode")


class Params(_P):
    __slots__ = ()

    def __new__(cls, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0, speckleWindowSize=0, speckleRange=0,
                mode=MODE_SGBM):
        return super().__new__(cls, minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange, mode)

    m = property(lambda s: s.minDisparity)
    n = property(lambda s: s.numDisparities)
    w = property(lambda s: s.blockSize)
    Dmax = property(lambda s: s.minDisparity + s.numDisparities - 1)
    ft = property(lambda s: max(s.preFilterCap, 15) | 1)
    filtered = property(lambda s: (s.minDisparity - 1) * 16)
    q = property(lambda s: s.disp12MaxDiff if s.disp12MaxDiff > 0 else 1)


def valid_columns(W, p):
    """(xlo, xhi)"""
    return max(p.Dmax, 0), min(W, W + p.m)


def cost_bound(p):
    """the largest value a C or an L_r can take: served iff <= 32767"""
    return p.w * p.w * (2 * p.ft + 63) + p.P2


def cdiv(a, b):
    """C division, b > 0: toward zero"""
    return -((-a) // b) if a < 0 else a // b


# ------------------------------------------------------------------------------------------------------------------------------------ plain loops
def prefilter_loops(I, ft):
    H, W = I.shape
    G = np.full((H, W), ft, np.int32)
    for y in range(H):
        ym, yp = max(y - 1, 0), min(y + 1, H - 1)
        for x in range(1, W - 1):
            g = lambda r: int(I[r][x + 1]) - int(I[r][x - 1])
            G[y][x] = min(max(2 * g(y) + g(ym) + g(yp), -ft), ft) + ft
    return G


def _bt_loops(row, x):
    W = len(row)
    a = int(row[x])
    am, ap = (a + int(row[max(x - 1, 0)])) >> 1, (a + int(row[min(x + 1, W - 1)])) >> 1
    return a, min(am, ap, a), max(am, ap, a)


def pixel_cost_loops(L, Rr, p):
    """pc[y][x][k], x counted from xlo"""
    H, W = L.shape
    xlo, xhi = valid_columns(W, p)
    W1 = max(xhi - xlo, 0)
    pc = np.zeros((H, W1, p.n), np.int32)
    planes = ((prefilter_loops(L, p.ft), prefilter_loops(Rr, p.ft), 0), (L, Rr, 2))
    for y in range(H):
        for x in range(W1):
            X = xlo + x
            for k in range(p.n):
                D = k + p.m
                s = 0
                for AL, AR, shift in planes:
                    u, loL, hiL = _bt_loops(AL[y], X)
                    v, loR, hiR = _bt_loops(AR[y], X - D)
                    c0 = max(0, u - hiR, loR - u)
                    c1 = max(0, v - hiL, loL - v)
                    s += min(c0, c1) >> shift
                pc[y][x][k] = s
    return pc


def block_cost_loops(pc, w):
    H, W1, n = pc.shape
    h = w // 2
    C = np.zeros_like(pc)
    for y in range(H):
        for x in range(W1):
            for k in range(n):
                s = 0
                for dy in range(-h, h + 1):
                    for dx in range(-h, h + 1):
                        s += int(pc[min(max(y + dy, 0), H - 1)][min(max(x + dx, 0), W1 - 1)][k])
                C[y][x][k] = s
    return C


def path_loops(C, ry, rx, P1, P2):
    H, W1, n = C.shape
    Lr = np.zeros((H, W1, n), np.int64)
    ys = range(H) if ry >= 0 else range(H - 1, -1, -1)
    xs = range(W1) if rx >= 0 else range(W1 - 1, -1, -1)
    for y in ys:
        for x in xs:
            py, px = y - ry, x - rx
            if py < 0 or py >= H or px < 0 or px >= W1:
                Lr[y][x] = C[y][x]
                continue
            prev = Lr[py][px]
            M = int(prev.min())
            for k in range(n):
                t = [int(prev[k]), M + P2]
                if k > 0:
                    t.append(int(prev[k - 1]) + P1)
                if k < n - 1:
                    t.append(int(prev[k + 1]) + P1)
                Lr[y][x][k] = int(C[y][x][k]) + min(t) - M
    return Lr


def aggregate_loops(C, p):
    S = np.zeros(C.shape, np.int64)
    for ry, rx in DIRECTIONS[p.mode]:
        S += path_loops(C, ry, rx, p.P1, p.P2)
    return S


def decide_loops(S, p):
    """(d, best, ms, kept) per valid pixel; d is the CV_16S value or FILTERED"""
    H, W1, n = S.shape
    d = np.full((H, W1), p.filtered, np.int32)
    best, ms, kept = np.zeros((H, W1), np.int32), np.zeros((H, W1), np.int64), np.zeros((H, W1), bool)
    for y in range(H):
        for x in range(W1):
            s = [int(v) for v in S[y][x]]
            b = min(range(n), key=lambda k: (s[k], k))
            best[y][x], ms[y][x] = b, s[b]
            if p.uniquenessRatio > 0 and any(abs(k - b) > 1 and s[k] * (100 - p.uniquenessRatio) < s[b] * 100 for k in range(n)):
                continue
            v = b * 16
            if 0 < b < n - 1:
                den = max(s[b - 1] + s[b + 1] - 2 * s[b], 1)
                v += cdiv((s[b - 1] - s[b + 1]) * 16 + den, 2 * den)
            d[y][x], kept[y][x] = v + 16 * p.m, True
    return d, best, ms, kept


def left_right_loops(d, best, ms, kept, W, p):
    """the valid columns' map after the left-right check"""
    H, W1 = d.shape
    xlo, _ = valid_columns(W, p)
    out = d.copy()
    for y in range(H):
        d2, win = [p.m - 1] * W, [None] * W
        for x in range(W1):
            if not kept[y][x]:
                continue
            X = xlo + x
            x2 = X - (int(best[y][x]) + p.m)
            if 0 <= x2 < W and (win[x2] is None or (int(ms[y][x]), -X) < win[x2]):
                win[x2], d2[x2] = (int(ms[y][x]), -X), int(best[y][x]) + p.m
        for x in range(W1):
            if not kept[y][x]:
                continue
            X, d1 = xlo + x, int(d[y][x])
            fails = 0
            for dk in (d1 >> 4, (d1 + 15) >> 4):
                xk = X - dk
                fails += 0 <= xk < W and d2[xk] >= p.m and abs(d2[xk] - dk) > p.q
            if fails == 2:
                out[y][x] = p.filtered
    return out


# ------------------------------------------------------------------------------------------------------------------------------------ numpy
def prefilter_np(I, ft):
    I = I.astype(np.int32)
    H, W = I.shape
    G = np.full((H, W), ft, np.int32)
    if W > 2:
        g = I[:, 2:] - I[:, :-2]
        gp = np.pad(g, ((1, 1), (0, 0)), mode="edge")
        G[:, 1:W - 1] = np.clip(2 * g + gp[:-2] + gp[2:], -ft, ft) + ft
    return G


def _bt_np(A):
    A = A.astype(np.int32)
    Ap = np.pad(A, ((0, 0), (1, 1)), mode="edge")
    am, ap = (A + Ap[:, :-2]) >> 1, (A + Ap[:, 2:]) >> 1
    return A, np.minimum(np.minimum(am, ap), A), np.maximum(np.maximum(am, ap), A)


def pixel_cost_np(L, Rr, p):
    H, W = L.shape
    xlo, xhi = valid_columns(W, p)
    W1 = max(xhi - xlo, 0)
    pc = np.zeros((H, W1, p.n), np.int32)
    if W1 == 0:
        return pc
    X = np.arange(xlo, xhi)
    for AL, AR, shift in ((prefilter_np(L, p.ft), prefilter_np(Rr, p.ft), 0), (L, Rr, 2)):
        u, loL, hiL = (a[:, X] for a in _bt_np(AL))
        v_, loR_, hiR_ = _bt_np(AR)
        for k in range(p.n):
            XR = X - (k + p.m)
            v, loR, hiR = v_[:, XR], loR_[:, XR], hiR_[:, XR]
            c0 = np.maximum(0, np.maximum(u - hiR, loR - u))
            c1 = np.maximum(0, np.maximum(v - hiL, loL - v))
            pc[:, :, k] += np.minimum(c0, c1) >> shift
    return pc


def block_cost_np(pc, w):
    H, W1, n = pc.shape
    if W1 == 0:
        return pc.copy()
    h = w // 2
    P = np.pad(pc, ((h, h), (h, h), (0, 0)), mode="edge")
    C = np.zeros_like(pc)
    for dy in range(w):
        for dx in range(w):
            C += P[dy:dy + H, dx:dx + W1]
    return C


def _step_np(c, prev, P1, P2):
    """c, prev: ... x n"""
    M = prev.min(axis=-1, keepdims=True)
    big = np.iinfo(np.int64).max // 4
    pad = np.full(prev.shape[:-1] + (1,), big, np.int64)
    dn = np.concatenate([pad, prev[..., :-1]], axis=-1) + P1
    up = np.concatenate([prev[..., 1:], pad], axis=-1) + P1
    return c + np.minimum(np.minimum(prev, M + P2), np.minimum(dn, up)) - M


def path_np(C, ry, rx, P1, P2):
    H, W1, n = C.shape
    C = C.astype(np.int64)
    Lr = C.copy()
    if ry == 0:
        xs = range(1, W1) if rx > 0 else range(W1 - 2, -1, -1)
        for x in xs:
            Lr[:, x] = _step_np(C[:, x], Lr[:, x - rx], P1, P2)
        return Lr
    ys = range(1, H) if ry > 0 else range(H - 2, -1, -1)
    x = np.arange(W1)
    ok = (x - rx >= 0) & (x - rx < W1)
    for y in ys:
        Lr[y, x[ok]] = _step_np(C[y, x[ok]], Lr[y - ry, x[ok] - rx], P1, P2)
    return Lr


def aggregate_np(C, p):
    S = np.zeros(C.shape, np.int64)
    for ry, rx in DIRECTIONS[p.mode]:
        S += path_np(C, ry, rx, p.P1, p.P2)
    return S


def decide_np(S, p):
    H, W1, n = S.shape
    S = S.astype(np.int64)
    if W1 == 0:
        z = np.zeros((H, 0), np.int32)
        return z, z, z.astype(np.int64), z.astype(bool)
    best = S.argmin(axis=-1).astype(np.int32)                       # the first of the smallest
    ms = np.take_along_axis(S, best[..., None].astype(np.int64), -1)[..., 0]
    kept = np.ones((H, W1), bool)
    if p.uniquenessRatio > 0:
        k = np.arange(n)
        far = np.abs(k[None, None, :] - best[..., None]) > 1
        kept = ~(far & (S * (100 - p.uniquenessRatio) < ms[..., None] * 100)).any(axis=-1)
    bi = np.clip(best, 1, n - 2) if n > 2 else best
    sm = np.take_along_axis(S, (bi - 1)[..., None].astype(np.int64), -1)[..., 0]
    sp = np.take_along_axis(S, (bi + 1)[..., None].astype(np.int64), -1)[..., 0]
    den = np.maximum(sm + sp - 2 * ms, 1)
    num = (sm - sp) * 16 + den
    quo = np.where(num < 0, -((-num) // (2 * den)), num // (2 * den))
    inner = (best > 0) & (best < n - 1)
    d = best.astype(np.int64) * 16 + np.where(inner, quo, 0) + 16 * p.m
    return np.where(kept, d, p.filtered).astype(np.int32), best, ms, kept


def left_right_np(d, best, ms, kept, W, p):
    H, W1 = d.shape
    xlo, _ = valid_columns(W, p)
    out = d.copy()
    if W1 == 0:
        return out
    X = xlo + np.arange(W1)
    NONE = np.iinfo(np.int64).max
    for y in range(H):
        k = kept[y]
        x2 = X - (best[y] + p.m)
        k = k & (x2 >= 0) & (x2 < W)
        # (ms, W - 1 - X, best): the smallest wins
        key = (ms[y].astype(np.int64) << 32) | ((W - 1 - X).astype(np.int64) << 16) | best[y].astype(np.int64)
        keys = np.full(W, NONE, np.int64)
        np.minimum.at(keys, x2[k], key[k])
        d2 = np.where(keys == NONE, p.m - 1, (keys & 0xffff) + p.m)
        d1 = d[y].astype(np.int64)
        fails = np.zeros(W1, np.int32)
        for dk in (d1 >> 4, (d1 + 15) >> 4):
            xk = X - dk
            inside = (xk >= 0) & (xk < W)
            e = d2[np.clip(xk, 0, W - 1)]
            fails += inside & (e >= p.m) & (np.abs(e - dk) > p.q)
        out[y][kept[y] & (fails == 2)] = p.filtered
    return out


def _assemble(valid, H, W, p):
    xlo, xhi = valid_columns(W, p)
    out = np.full((H, W), p.filtered, np.int16)
    if xhi > xlo:
        out[:, xlo:xhi] = valid
    return out


def compute_np(L, Rr, p, stages=None):
    """the CV_16S map before the speckle filter (the GPU tests apply tests/speckle_restate.py after it)"""
    H, W = L.shape
    pc = pixel_cost_np(L, Rr, p)
    C = block_cost_np(pc, p.w)
    S = aggregate_np(C, p)
    d, best, ms, kept = decide_np(S, p)
    out = left_right_np(d, best, ms, kept, W, p)
    if stages is not None:
        stages.update(pc=pc, C=C, S=S, d=d, best=best, ms=ms, kept=kept)
    return _assemble(out, H, W, p)


def compute_loops(L, Rr, p):
    H, W = L.shape
    S = aggregate_loops(block_cost_loops(pixel_cost_loops(L, Rr, p), p.w), p)
    d, best, ms, kept = decide_loops(S, p)
    return _assemble(left_right_loops(d, best, ms, kept, W, p), H, W, p)


def speckle_args(p):
    """(newVal, maxSpeckleSize, maxDiff) of the filterSpeckles call that follows when speckleWindowSize > 0"""
    return p.filtered, p.speckleWindowSize, 16 * p.speckleRange


def to_float(d16):
    return d16.astype(np.float32) * np.float32(0.0625)


# ------------------------------------------------------------------------------------------------------------------------------------ inputs
def random_pair(rng, H, W):
    return rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)


def constant_pair(H, W, v=77):
    return np.full((H, W), v, np.uint8), np.full((H, W), v, np.uint8)


def smooth_pair(rng, H, W, s):
    """a 3 x 3-box-smoothed random image and its copy shifted by s: left[x] = right[x - s]"""
    pad = abs(s) + 2
    base = rng.integers(0, 256, (H + 2, W + 2 * pad + 2)).astype(np.int32)
    sm = sum(base[dy:dy + H, dx:dx + W + 2 * pad] for dy in range(3) for dx in range(3)) // 9
    sm = sm.astype(np.uint8)
    right = sm[:, pad:pad + W]
    left = sm[:, pad - s:pad - s + W]
    return np.ascontiguousarray(left), np.ascontiguousarray(right)


def check_shift_recovered(d, p, s):
    """the conditions of the test that does not rest on the restatement; fixed"""
    H, W = d.shape
    xlo, xhi = valid_columns(W, p)
    h = p.w // 2
    outside = np.ones((H, W), bool)
    outside[:, xlo:xhi] = False
    assert (d[outside] == p.filtered).all()
    inner = d[h + 1:H - h - 1, xlo + h + 1:xhi - h - 1].astype(np.int32)
    assert inner.size > 0
    assert (inner != p.filtered).all(), int((inner == p.filtered).sum())
    assert np.abs(inner - 16 * s).max() <= 8, int(np.abs(inner - 16 * s).max())
    valid = d[:, xlo:xhi]
    assert (valid == p.filtered).mean() <= 0.02, float((valid == p.filtered).mean())
