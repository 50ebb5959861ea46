"""cv::calcOpticalFlowFarneback (modules/video/src/optflowgf.cpp) as this project restates it: the DEFINITION the host-compiled farneback_math.h and the kernels of
farneback.hip are held against bit for bit (test infrastructure, like mog2_restate.py).  Two forms of every stage, plain loops ("loops") and vectorised numpy ("vec").

All image arithmetic is float32 with one rounding per operation and every sum in a fixed order (taps in ascending index, polynomial sums centre first then k = 1 .. n);
taps and the four inverse-moment constants are prepared in float64 (math.exp, the C library's) and rounded to float32 once.  `T=np.float64` evaluates the same
restatement with float64 image arithmetic (same float32-rounded taps): the yardstick for what float32 accumulators cost.

Stages: level_plan, gaussian_taps, smooth, resize_linear, poly_setup, poly_exp, update_matrices, win_setup, update_flow, calc (the whole call)."""
import math

import numpy as np

F = np.float32
OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_FARNEBACK_GAUSSIAN = 256
FLT_EPSILON = 1.1920928955078125e-7
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
MIN_SIZE = 32
_SMALL = {1: (1.0,), 3: (0.25, 0.5, 0.25), 5: (0.0625, 0.25, 0.375, 0.25, 0.0625), 7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125)}


def cv_round(v):
    return int(np.rint(np.float64(v)))                                   # half to even


def reflect101(p, n):
    if 0 <= p < n:
        return p
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


# ---------------------------------------------------------------- host-side preparation (float64, rounded once)
def gaussian_taps(n, sigma):
    """getGaussianKernel's rule: fixed tables for sigma <= 0 and odd n <= 7; else exp(-x^2 / 2 sigma^2) normalised, sigma <= 0 meaning 0.3 ((n - 1) / 2 - 1) + 0.8"""
    if sigma <= 0 and n % 2 == 1 and n <= 7:
        return np.array(_SMALL[n], F)
    sg = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2 = -0.5 / (sg * sg)
    e = [math.exp(scale2 * (i - (n - 1) * 0.5) * (i - (n - 1) * 0.5)) for i in range(n)]
    s = 0.0
    for v in e:
        s += v
    inv = 1.0 / s
    return np.array([v * inv for v in e], F)


def poly_setup(n, sigma):
    """(g, xg, xxg) for k = 0 .. n as float32 arrays and (ig11, ig03, ig33, ig55) as float32"""
    if sigma < FLT_EPSILON:
        sigma = n * 0.3
    g = [F(math.exp(-x * x / (2 * sigma * sigma))) for x in range(-n, n + 1)]
    s = 0.0
    for v in g:
        s += float(v)
    s = 1.0 / s
    g = [F(float(v) * s) for v in g]
    gk = np.array([g[k + n] for k in range(n + 1)], F)
    xg = np.array([F(k * float(g[k + n])) for k in range(n + 1)], F)
    xxg = np.array([F(k * k * float(g[k + n])) for k in range(n + 1)], F)
    a = b = c = d = 0.0
    for y in range(-n, n + 1):
        for x in range(-n, n + 1):
            gg = float(g[y + n]) * float(g[x + n])
            a += gg
            b += gg * (x * x)
            c += gg * (x * x * x * x)
            d += gg * (x * x * y * y)
    D = a * (c + d) - 2 * b * b
    ig = (F(1.0 / b), F(-b / D), F((a * c - b * b) / ((c - d) * D)), F(1.0 / d))
    return gk, xg, xxg, ig


def moment_matrix(n, sigma):
    """the 6 x 6 matrix of g (x) g over (1, x, y, x^2, y^2, xy) in float64, for checking poly_setup's closed-form inverse against a general one"""
    if sigma < FLT_EPSILON:
        sigma = n * 0.3
    gk = poly_setup(n, sigma)[0].astype(np.float64)
    g = lambda k: gk[abs(k)]
    G = np.zeros((6, 6))
    for y in range(-n, n + 1):
        for x in range(-n, n + 1):
            b = np.array([1, x, y, x * x, y * y, x * y], np.float64)
            G += g(y) * g(x) * np.outer(b, b)
    return G


def win_setup(winsize, gaussian):
    """(taps of the 2 m + 1 window, the factor applied to the five sums)"""
    m = winsize // 2
    if gaussian:
        return gaussian_taps(2 * m + 1, 0.3 * m), F(1)
    return np.ones(2 * m + 1, F), F(1.0 / ((2 * m + 1) * (2 * m + 1)))


def level_plan(w, h, pyr_scale, levels):
    """[(scale, level width, level height, ksize, sigma)] for k = 0 .. count - 1"""
    out = []
    for k in range(levels):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        if k > 0 and (w * scale < MIN_SIZE or h * scale < MIN_SIZE):
            break
        sigma = (1.0 / scale - 1) * 0.5
        out.append((scale, cv_round(w * scale), cv_round(h * scale), max(cv_round(sigma * 5) | 1, 3), sigma))
    return out


def resize_coords(dst, src):
    """per destination index: (i0, i1, fraction as float32)"""
    scale = src / dst
    i0, i1, fr = np.zeros(dst, np.int64), np.zeros(dst, np.int64), np.zeros(dst, F)
    for d in range(dst):
        c = F((d + 0.5) * scale - 0.5)
        fl = F(np.floor(c))
        s, f = int(fl), F(c - fl)
        if s < 0:
            s, f = 0, F(0)
        if s >= src - 1:
            s, f = src - 1, F(0)
        i0[d], i1[d], fr[d] = s, min(s + 1, src - 1), f
    return i0, i1, fr


# ---------------------------------------------------------------- vectorised form
def smooth_vec(img, taps, T=F):
    """separable Gaussian, BORDER_REFLECT_101: horizontal pass then vertical, taps in ascending index"""
    src = np.asarray(img).astype(T)
    h, w = src.shape
    n, r = len(taps), len(taps) // 2
    t = taps.astype(T)
    acc = None
    for k in range(n):
        idx = [reflect101(x + k - r, w) for x in range(w)]
        term = t[k] * src[:, idx]
        acc = term if acc is None else acc + term
    tmp, acc = acc, None
    for k in range(n):
        idx = [reflect101(y + k - r, h) for y in range(h)]
        term = t[k] * tmp[idx, :]
        acc = term if acc is None else acc + term
    return acc


def resize_vec(src, dw, dh, factor=None, T=F):
    """bilinear resize of [h, w] or [h, w, c]: horizontal pass s0 (1 - f) + s1 f, then vertical; factor: each result times it in float64, rounded once"""
    src = np.asarray(src, T)
    h, w = src.shape[:2]
    x0, x1, fx = resize_coords(dw, w)
    y0, y1, fy = resize_coords(dh, h)
    fx, fy = fx.astype(T), fy.astype(T)
    fxb, fyb = (fx[None, :, None], fy[:, None, None]) if src.ndim == 3 else (fx[None, :], fy[:, None])
    one = T(1)
    t = src[:, x0] * (one - fxb) + src[:, x1] * fxb
    out = t[y0] * (one - fyb) + t[y1] * fyb
    if factor is not None:
        out = (out.astype(np.float64) * np.float64(factor)).astype(T)
    return out


def poly_exp_vec(src, n, sigma, T=F):
    src = np.asarray(src, T)
    h, w = src.shape
    g, xg, xxg, ig = (a.astype(T) if isinstance(a, np.ndarray) else tuple(T(v) for v in a) for a in poly_setup(n, sigma))
    ys, xs = np.arange(h), np.arange(w)
    v0, v1, v2 = src * g[0], np.zeros((h, w), T), np.zeros((h, w), T)
    for k in range(1, n + 1):
        up, dn = src[np.clip(ys - k, 0, h - 1)], src[np.clip(ys + k, 0, h - 1)]
        p = up + dn
        v0 = v0 + g[k] * p
        v1 = v1 + xg[k] * (dn - up)
        v2 = v2 + xxg[k] * p
    b1, b3, b5 = v0 * g[0], v1 * g[0], v2 * g[0]
    b2, b4, b6 = np.zeros((h, w), T), np.zeros((h, w), T), np.zeros((h, w), T)
    for k in range(1, n + 1):
        il, ir = np.clip(xs - k, 0, w - 1), np.clip(xs + k, 0, w - 1)
        tg = v0[:, ir] + v0[:, il]
        b1 = b1 + tg * g[k]
        b4 = b4 + tg * xxg[k]
        b2 = b2 + (v0[:, ir] - v0[:, il]) * xg[k]
        b3 = b3 + (v1[:, ir] + v1[:, il]) * g[k]
        b6 = b6 + (v1[:, ir] - v1[:, il]) * xg[k]
        b5 = b5 + (v2[:, ir] + v2[:, il]) * g[k]
    ig11, ig03, ig33, ig55 = ig
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55], axis=2)


def border_weights(n, T=F):
    out = np.ones(n, T)
    for p in range(n):
        a = T(BORDER[p]) if p < 5 else T(1)
        b = T(BORDER[n - p - 1]) if p >= n - 5 else T(1)
        out[p] = a * b
    return out


def inside_mask(flow, T=F):
    """which pixels sample R1 (True) and which take the outside branch, for tests that must take both"""
    flow = np.asarray(flow, T)
    h, w = flow.shape[:2]
    fx = np.arange(w, dtype=T)[None, :] + flow[..., 0]
    fy = np.arange(h, dtype=T)[:, None] + flow[..., 1]
    x1, y1 = np.floor(fx), np.floor(fy)
    return (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)


def update_matrices_vec(R0, R1, flow, T=F):
    R0, R1, flow = np.asarray(R0, T), np.asarray(R1, T), np.asarray(flow, T)
    h, w = flow.shape[:2]
    dx, dy = flow[..., 0], flow[..., 1]
    fx = np.arange(w, dtype=T)[None, :] + dx
    fy = np.arange(h, dtype=T)[:, None] + dy
    x1f, y1f = np.floor(fx), np.floor(fy)
    ins = (x1f >= 0) & (x1f < w - 1) & (y1f >= 0) & (y1f < h - 1)
    x1 = np.where(ins, x1f, 0).astype(np.int64)
    y1 = np.where(ins, y1f, 0).astype(np.int64)
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)
    ax, ay = np.where(ins, fx - x1f, 0).astype(T), np.where(ins, fy - y1f, 0).astype(T)
    one = T(1)
    a00, a01, a10, a11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
    with np.errstate(invalid="ignore"):
        s = [a00 * R1[y1, x1, c] + a01 * R1[y1, x2, c] + a10 * R1[y2, x1, c] + a11 * R1[y2, x2, c] for c in range(5)]
    zero = np.zeros((h, w), T)
    r2, r3 = np.where(ins, s[0], zero), np.where(ins, s[1], zero)
    r4 = np.where(ins, (R0[..., 2] + s[2]) * T(0.5), R0[..., 2])
    r5 = np.where(ins, (R0[..., 3] + s[3]) * T(0.5), R0[..., 3])
    r6 = np.where(ins, (R0[..., 4] + s[4]) * T(0.25), R0[..., 4] * T(0.5))
    r2 = (R0[..., 0] - r2) * T(0.5)
    r3 = (R0[..., 1] - r3) * T(0.5)
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    sc = border_weights(w, T)[None, :] * border_weights(h, T)[:, None]
    r2, r3, r4, r5, r6 = r2 * sc, r3 * sc, r4 * sc, r5 * sc, r6 * sc
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], axis=2).astype(T)


def update_flow_vec(M, winsize, gaussian, T=F):
    M = np.asarray(M, T)
    h, w = M.shape[:2]
    taps, scale = win_setup(winsize, gaussian)
    taps, scale = taps.astype(T), T(scale)
    m = winsize // 2
    ys, xs = np.arange(h), np.arange(w)
    acc = None
    for i in range(2 * m + 1):
        term = taps[i] * M[np.clip(ys + i - m, 0, h - 1)]
        acc = term if acc is None else acc + term
    vs, acc = acc, None
    for i in range(2 * m + 1):
        term = taps[i] * vs[:, np.clip(xs + i - m, 0, w - 1)]
        acc = term if acc is None else acc + term
    g11, g12, g22, h1, h2 = (acc[..., c] * scale for c in range(5))
    idet = T(1) / (g11 * g22 - g12 * g12 + T(F(1e-3)))
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], axis=2)


# ---------------------------------------------------------------- plain loops (float32 only)
def smooth_loops(img, taps):
    src = np.asarray(img)
    h, w = src.shape
    n, r = len(taps), len(taps) // 2
    tmp, out = np.zeros((h, w), F), np.zeros((h, w), F)
    for y in range(h):
        for x in range(w):
            s = taps[0] * F(src[y, reflect101(x - r, w)])
            for k in range(1, n):
                s = F(s + taps[k] * F(src[y, reflect101(x + k - r, w)]))
            tmp[y, x] = s
    for y in range(h):
        for x in range(w):
            s = taps[0] * tmp[reflect101(y - r, h), x]
            for k in range(1, n):
                s = F(s + taps[k] * tmp[reflect101(y + k - r, h), x])
            out[y, x] = s
    return out


def resize_loops(src, dw, dh, factor=None):
    src = np.asarray(src, F)
    h, w = src.shape[:2]
    s3 = src.reshape(h, w, -1)
    cn = s3.shape[2]
    x0, x1, fx = resize_coords(dw, w)
    y0, y1, fy = resize_coords(dh, h)
    out = np.zeros((dh, dw, cn), F)
    one = F(1)
    for y in range(dh):
        for x in range(dw):
            for c in range(cn):
                top = s3[y0[y], x0[x], c] * (one - fx[x]) + s3[y0[y], x1[x], c] * fx[x]
                bot = s3[y1[y], x0[x], c] * (one - fx[x]) + s3[y1[y], x1[x], c] * fx[x]
                v = F(top * (one - fy[y]) + bot * fy[y])
                if factor is not None:
                    v = F(np.float64(v) * np.float64(factor))
                out[y, x, c] = v
    return out.reshape((dh, dw) + src.shape[2:])


def poly_exp_loops(src, n, sigma):
    src = np.asarray(src, F)
    h, w = src.shape
    g, xg, xxg, (ig11, ig03, ig33, ig55) = poly_setup(n, sigma)
    v = np.zeros((h, w, 3), F)
    for y in range(h):
        for x in range(w):
            t0, t1, t2 = src[y, x] * g[0], F(0), F(0)
            for k in range(1, n + 1):
                up, dn = src[max(y - k, 0), x], src[min(y + k, h - 1), x]
                p = F(up + dn)
                t0 = F(t0 + g[k] * p)
                t1 = F(t1 + xg[k] * F(dn - up))
                t2 = F(t2 + xxg[k] * p)
            v[y, x] = (t0, t1, t2)
    out = np.zeros((h, w, 5), F)
    for y in range(h):
        for x in range(w):
            b1, b2, b3, b4, b5, b6 = v[y, x, 0] * g[0], F(0), v[y, x, 1] * g[0], F(0), v[y, x, 2] * g[0], F(0)
            for k in range(1, n + 1):
                L, R = v[y, max(x - k, 0)], v[y, min(x + k, w - 1)]
                tg = F(R[0] + L[0])
                b1 = F(b1 + tg * g[k])
                b4 = F(b4 + tg * xxg[k])
                b2 = F(b2 + F(R[0] - L[0]) * xg[k])
                b3 = F(b3 + F(R[1] + L[1]) * g[k])
                b6 = F(b6 + F(R[1] - L[1]) * xg[k])
                b5 = F(b5 + F(R[2] + L[2]) * g[k])
            out[y, x] = (b3 * ig11, b2 * ig11, F(b1 * ig03) + F(b5 * ig33), F(b1 * ig03) + F(b4 * ig33), b6 * ig55)
    return out


def update_matrices_loops(R0, R1, flow):
    R0, R1, flow = np.asarray(R0, F), np.asarray(R1, F), np.asarray(flow, F)
    h, w = flow.shape[:2]
    M = np.zeros((h, w, 5), F)
    bw, bh = border_weights(w), border_weights(h)
    one = F(1)
    for y in range(h):
        for x in range(w):
            dx, dy = flow[y, x]
            fx, fy = F(F(x) + dx), F(F(y) + dy)
            x1f, y1f = F(np.floor(fx)), F(np.floor(fy))
            r0 = R0[y, x]
            if 0 <= x1f < w - 1 and 0 <= y1f < h - 1:
                ax, ay = F(fx - x1f), F(fy - y1f)
                a00, a01, a10, a11 = F(one - ax) * F(one - ay), ax * F(one - ay), F(one - ax) * ay, ax * ay
                p, q = R1[int(y1f), int(x1f):int(x1f) + 2], R1[int(y1f) + 1, int(x1f):int(x1f) + 2]
                s = [F(F(F(a00 * p[0, c]) + F(a01 * p[1, c])) + F(a10 * q[0, c])) + F(a11 * q[1, c]) for c in range(5)]
                r2, r3 = F(s[0]), F(s[1])
                r4 = F(r0[2] + s[2]) * F(0.5)
                r5 = F(r0[3] + s[3]) * F(0.5)
                r6 = F(r0[4] + s[4]) * F(0.25)
            else:
                r2, r3, r4, r5, r6 = F(0), F(0), r0[2], r0[3], r0[4] * F(0.5)
            r2 = F(r0[0] - r2) * F(0.5)
            r3 = F(r0[1] - r3) * F(0.5)
            r2 = F(r2 + F(F(r4 * dy) + F(r6 * dx)))
            r3 = F(r3 + F(F(r6 * dy) + F(r5 * dx)))
            sc = F(bw[x] * bh[y])
            r2, r3, r4, r5, r6 = r2 * sc, r3 * sc, r4 * sc, r5 * sc, r6 * sc
            M[y, x] = (F(r4 * r4) + F(r6 * r6), F(r4 + r5) * r6, F(r5 * r5) + F(r6 * r6), F(r4 * r2) + F(r6 * r3), F(r6 * r2) + F(r5 * r3))
    return M


def update_flow_loops(M, winsize, gaussian):
    M = np.asarray(M, F)
    h, w = M.shape[:2]
    taps, scale = win_setup(winsize, gaussian)
    m = winsize // 2
    vs = np.zeros((h, w, 5), F)
    for y in range(h):
        for x in range(w):
            for c in range(5):
                s = taps[0] * M[max(y - m, 0), x, c]
                for i in range(1, 2 * m + 1):
                    s = F(s + taps[i] * M[min(max(y + i - m, 0), h - 1), x, c])
                vs[y, x, c] = s
    flow = np.zeros((h, w, 2), F)
    for y in range(h):
        for x in range(w):
            hs = []
            for c in range(5):
                s = taps[0] * vs[y, max(x - m, 0), c]
                for i in range(1, 2 * m + 1):
                    s = F(s + taps[i] * vs[y, min(max(x + i - m, 0), w - 1), c])
                hs.append(F(s * scale))
            g11, g12, g22, h1, h2 = hs
            idet = F(1) / F(F(F(g11 * g22) - F(g12 * g12)) + F(1e-3))
            flow[y, x] = (F(F(g11 * h2) - F(g12 * h1)) * idet, F(F(g22 * h1) - F(g12 * h2)) * idet)
    return flow


# ---------------------------------------------------------------- the whole call
STAGES = {"vec": (smooth_vec, resize_vec, poly_exp_vec, update_matrices_vec, update_flow_vec),
          "loops": (smooth_loops, resize_loops, poly_exp_loops, update_matrices_loops, update_flow_loops)}


def level_image(img, level, impl="vec", T=F):
    """the float image of one pyramid level: Gaussian of the level's ksize on the full frame, then the bilinear resize to the level's size"""
    smooth, resize = STAGES[impl][:2]
    _, lw, lh, ksize, sigma = level
    kw = {} if impl == "loops" else {"T": T}
    return resize(smooth(img, gaussian_taps(ksize, sigma), **kw), lw, lh, **kw)


def calc(prev, nxt, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags, impl="vec", T=F):
    """returns the flow [h, w, 2]; `flow` is read only with OPTFLOW_USE_INITIAL_FLOW, which is served for one effective level only (ValueError otherwise)"""
    prev, nxt = np.asarray(prev), np.asarray(nxt)
    assert prev.dtype == np.uint8 and prev.ndim == 2 and prev.shape == nxt.shape and nxt.dtype == np.uint8
    assert levels >= 1 and winsize >= 1 and poly_n >= 1 and iterations >= 0 and 0 < pyr_scale < 1 and not flags & ~(OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_FARNEBACK_GAUSSIAN)
    h, w = prev.shape
    plan = level_plan(w, h, pyr_scale, levels)
    if flags & OPTFLOW_USE_INITIAL_FLOW and len(plan) > 1:
        raise ValueError("OPTFLOW_USE_INITIAL_FLOW with %d levels" % len(plan))
    _, resize, poly_exp, update_matrices, update_flow = STAGES[impl]
    kw = {} if impl == "loops" else {"T": T}
    gaussian = bool(flags & OPTFLOW_FARNEBACK_GAUSSIAN)
    cur = None
    for k in range(len(plan) - 1, -1, -1):
        _, lw, lh, _, _ = plan[k]
        if cur is None:
            cur = np.array(flow, T).reshape(h, w, 2) if flags & OPTFLOW_USE_INITIAL_FLOW else np.zeros((lh, lw, 2), T)
        else:
            cur = resize(cur, lw, lh, factor=1.0 / pyr_scale, **kw)
        R0 = poly_exp(level_image(prev, plan[k], impl, T), poly_n, poly_sigma, **kw)
        R1 = poly_exp(level_image(nxt, plan[k], impl, T), poly_n, poly_sigma, **kw)
        M = update_matrices(R0, R1, cur, **kw)
        for i in range(iterations):
            cur = update_flow(M, winsize, gaussian, **kw)
            if i < iterations - 1:
                M = update_matrices(R0, R1, cur, **kw)
    return cur


def texture_pair(h, w, shift, seed=0):
    """two 8-bit frames cropped from one smooth random texture (uniform noise under a 9-tap, sigma 2 Gaussian, stretched to 0 .. 255); the second is the first
    moved by shift = (sx, sy): next(x + sx, y + sy) = prev(x, y), so the true flow is (sx, sy) everywhere"""
    sx, sy = shift
    pad = 8 + max(abs(sx), abs(sy))
    rng = np.random.default_rng(seed)
    big = rng.random((h + 2 * pad, w + 2 * pad))
    t = gaussian_taps(9, 2.0).astype(np.float64)
    big = np.apply_along_axis(lambda r: np.convolve(r, t, mode="same"), 1, big)
    big = np.apply_along_axis(lambda c: np.convolve(c, t, mode="same"), 0, big)
    big = big[4:-4, 4:-4]
    big = np.rint((big - big.min()) / (big.max() - big.min()) * 255).astype(np.uint8)
    p = pad - 4
    return big[p:p + h, p:p + w].copy(), big[p - sy:p - sy + h, p - sx:p - sx + w].copy()
