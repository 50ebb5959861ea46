"""The circle transform (cv::HoughCircles with HOUGH_GRADIENT, HoughCirclesGradient in imgproc/src/hough.cpp, as recalled: the reference and cv2 were not
available) restated twice.  The GPU tests and the host build of opencv_amd/csrc/houghcircles_math.h are held against these, and the two against each other.

  *_loops   the steps as plain loops over np.float32 scalars: the ray with its `break`, the radius histogram point by point, the scan one bin per step
  *_vec     written on its own with numpy arrays: every step of every ray at once under the inside mask (np.logical_and.accumulate along the ray is the `break`:
            it needs no assumption about where a ray starts), np.bincount for votes and bins, the scan jumping between the non-zero bins with searchsorted

"float" is IEEE binary32, every operation rounded on its own (numpy never fuses); np.sqrt and / are correctly rounded; cvRound is round-half-to-even (np.rint).
Inputs are an edge map (uint8, non-zero = edge) and the two CV_16S gradient planes; what makes them is not this file's business."""
from types import SimpleNamespace

import numpy as np

F = np.float32
SHIFT, ONE, BINS_PER_DR = 10, 1024, 10
EPS = F(1.1920929e-07)
HOUGH_GRADIENT, HOUGH_GRADIENT_ALT = 3, 4
MAX_DIM, MAX_ACCUM, MAX_RADIUS, MAX_CIRCLES = 16384, 1 << 26, 32768, 65536          # opencv_amd/csrc/houghcircles_math.h
LDS_BINS, TILE, STEP_BLOCK = 40960, 64, 16
LIMITS = {"houghcircles_max_dim": MAX_DIM, "houghcircles_max_accum": MAX_ACCUM, "houghcircles_max_radius": MAX_RADIUS, "houghcircles_max_circles": MAX_CIRCLES,
          "houghcircles_lds_bins": LDS_BINS, "houghcircles_tile": TILE}


def cv_round(v):
    return int(np.rint(F(v)))


def prepare(w, h, dp, min_dist, param1, param2, min_radius, max_radius):
    """the arguments as the public function prepares them.  param1 / param2 are taken as they come (0 included): refusing them is the library's business"""
    p = SimpleNamespace(w=w, h=h)
    p.dp = max(F(dp), F(1))
    p.idp = F(1) / p.dp
    p.canny, p.acc_t = int(np.rint(param1)), int(np.rint(param2))
    p.min_dist = F(min_dist)
    p.min_radius = max(0, int(min_radius))
    p.centers_only = max_radius < 0
    if max_radius <= 0:
        max_radius = max(w, h)
    elif max_radius <= p.min_radius:
        max_radius = p.min_radius + 2
    p.max_radius = int(max_radius)
    p.acols, p.arows = int(np.ceil(F(w) * p.idp)), int(np.ceil(F(h) * p.idp))
    p.astep = p.acols + 2
    p.n_bins = cv_round(F(p.max_radius - p.min_radius) / p.dp * F(BINS_PER_DR))
    return p


def canny_thresholds(param1):
    """(low, high) of the edge stage"""
    c = int(np.rint(param1))
    return max(1, c // 2), c


# ---- plain loops
def accum_loops(edges, dx, dy, p):
    """-> (accumulator int32 [arows + 2, acols + 2], nz: the list of (x, y) of the pixels that voted, row by row)"""
    acc = np.zeros((p.arows + 2) * p.astep, np.int32)
    nz = []
    for y in range(p.h):
        for x in range(p.w):
            vx, vy = int(dx[y, x]), int(dy[y, x])
            if not edges[y, x] or (vx == 0 and vy == 0):
                continue
            mag = np.sqrt(F(vx * vx + vy * vy))
            if mag < F(1):
                continue
            sx = cv_round(F(vx) * p.idp * F(ONE) / mag)
            sy = cv_round(F(vy) * p.idp * F(ONE) / mag)
            x0 = cv_round(F(x) * p.idp * F(ONE))
            y0 = cv_round(F(y) * p.idp * F(ONE))
            for _ in range(2):
                x1, y1 = x0 + p.min_radius * sx, y0 + p.min_radius * sy
                for _r in range(p.min_radius, p.max_radius + 1):
                    x2, y2 = x1 >> SHIFT, y1 >> SHIFT
                    if not (0 <= x2 < p.acols and 0 <= y2 < p.arows):
                        break
                    acc[y2 * p.astep + x2] += 1
                    x1 += sx
                    y1 += sy
                sx, sy = -sx, -sy
            nz.append((x, y))
    return acc.reshape(p.arows + 2, p.astep), nz


def centres_loops(acc, p, acc_t):
    """-> the cells b of the centres, ordered by (votes descending, b ascending)"""
    a = acc.reshape(-1)
    s = p.astep
    out = []
    for y in range(1, p.arows + 1):
        for x in range(1, p.acols + 1):
            b = y * s + x
            if a[b] > acc_t and a[b] > a[b - 1] and a[b] >= a[b + 1] and a[b] > a[b - s] and a[b] >= a[b + s]:
                out.append(b)
    out.sort(key=lambda b: (-int(a[b]), b))
    return out


def bins_loops(cx, cy, nz, p):
    bins = np.zeros(max(p.n_bins, 0), np.int32)
    min_r2, max_r2 = F(p.min_radius * p.min_radius), F(p.max_radius * p.max_radius)
    for (px, py) in nz:
        ex, ey = cx - F(px), cy - F(py)
        r2 = ex * ex + ey * ey
        if min_r2 <= r2 <= max_r2:
            r = np.sqrt(r2)
            b = cv_round((r - F(p.min_radius)) / p.dp * F(BINS_PER_DR))
            bins[min(max(b, 0), p.n_bins - 1)] += 1
    return bins


def scan_loops(bins, p):
    """-> (rBest float32, maxCount)"""
    n = len(bins)
    max_count, r_best = 0, F(0)
    j = n - 1
    while j > 0:
        if bins[j]:
            upbin, cur = j, 0
            while j > upbin - BINS_PER_DR and j >= 0:
                cur += int(bins[j])
                j -= 1
            r_cur = F(upbin + j) / F(2) / F(BINS_PER_DR) * p.dp + F(p.min_radius)
            if F(cur) * r_best >= F(max_count) * r_cur or (r_best < EPS and cur >= max_count):
                r_best, max_count = r_cur, cur
        j -= 1
    return r_best, max_count


def suppress_loops(cands, p, max_circles):
    """cands: (x, y, r, votes, b) -> float32 [n, 4]"""
    cands = sorted(cands, key=lambda c: (-c[3], c[4]))
    md2 = p.min_dist * p.min_dist
    kept = []
    for c in cands:
        ok = True
        for k in kept:
            ddx, ddy = k[0] - c[0], k[1] - c[1]
            if ddx * ddx + ddy * ddy < md2:
                ok = False
                break
        if ok:
            kept.append(c)
            if max_circles is not None and len(kept) == max_circles:
                break
    return np.array([[c[0], c[1], c[2], F(c[3])] for c in kept], F).reshape(-1, 4)


def candidates_loops(acc, nz, p, acc_t=None):
    """-> [(x, y, r, votes, b)] of every circle before the suppression, in the centres' order"""
    acc_t = p.acc_t if acc_t is None else acc_t
    a = acc.reshape(-1)
    cands = []
    for b in centres_loops(acc, p, acc_t):
        cx, cy = (F(b % p.astep) + F(0.5)) * p.dp, (F(b // p.astep) + F(0.5)) * p.dp
        if p.centers_only:
            cands.append((cx, cy, F(0), int(a[b]), b))
            continue
        bins = bins_loops(cx, cy, nz, p)
        if not bins.any():
            continue
        r_best, max_count = scan_loops(bins, p)
        if max_count > acc_t:
            cands.append((cx, cy, r_best, max_count, b))
    return cands


def circles_loops(acc, nz, p, acc_t=None, max_circles=None):
    return suppress_loops(candidates_loops(acc, nz, p, acc_t), p, max_circles)


# ---- numpy, written on its own
def points_vec(edges, dx, dy):
    vx, vy = dx.astype(np.int64), dy.astype(np.int64)
    m = (edges != 0) & ((vx != 0) | (vy != 0))
    mag = np.sqrt((vx * vx + vy * vy).astype(F))
    assert mag.dtype == F
    m &= mag >= F(1)
    ys, xs = np.nonzero(m)                                                   # row by row
    return xs, ys, vx[ys, xs], vy[ys, xs], mag[ys, xs]


def accum_vec(edges, dx, dy, p):
    xs, ys, vx, vy, mag = points_vec(edges, dx, dy)
    acc = np.zeros((p.arows + 2) * p.astep, np.int64)
    if len(xs):
        k = F(ONE)
        sx = np.rint(vx.astype(F) * p.idp * k / mag).astype(np.int64)
        sy = np.rint(vy.astype(F) * p.idp * k / mag).astype(np.int64)
        x0 = np.rint(xs.astype(F) * p.idp * k).astype(np.int64)
        y0 = np.rint(ys.astype(F) * p.idp * k).astype(np.int64)
        r = np.arange(p.min_radius, p.max_radius + 1, dtype=np.int64)[None, :]
        for sg in (1, -1):
            x2 = (x0[:, None] + r * (sg * sx)[:, None]) >> SHIFT
            y2 = (y0[:, None] + r * (sg * sy)[:, None]) >> SHIFT
            ok = (x2 >= 0) & (x2 < p.acols) & (y2 >= 0) & (y2 < p.arows)
            ok = np.logical_and.accumulate(ok, axis=1)                       # the ray ends at its first miss
            acc += np.bincount((y2 * p.astep + x2)[ok], minlength=acc.size)
    return acc.astype(np.int32).reshape(p.arows + 2, p.astep), (xs, ys)


def centres_vec(acc, p, acc_t):
    c = acc[1:p.arows + 1, 1:p.acols + 1]
    is_max = (c > acc_t) & (c > acc[1:p.arows + 1, 0:p.acols]) & (c >= acc[1:p.arows + 1, 2:p.acols + 2]) & (c > acc[0:p.arows, 1:p.acols + 1]) & \
             (c >= acc[2:p.arows + 2, 1:p.acols + 1])
    y, x = np.nonzero(is_max)
    b = (y + 1) * p.astep + x + 1
    votes = c[y, x].astype(np.int64)
    return b[np.lexsort((b, -votes))]


def bins_vec(cx, cy, pts, p):
    xs, ys = pts
    ex, ey = cx - xs.astype(F), cy - ys.astype(F)
    r2 = ex * ex + ey * ey
    assert r2.dtype == F
    m = (r2 >= F(p.min_radius * p.min_radius)) & (r2 <= F(p.max_radius * p.max_radius))
    q = np.rint((np.sqrt(r2[m]) - F(p.min_radius)) / p.dp * F(BINS_PER_DR)).astype(np.int64)
    return np.bincount(np.clip(q, 0, p.n_bins - 1), minlength=p.n_bins).astype(np.int32)


def scan_vec(bins, p):
    nzb = np.nonzero(bins)[0]
    nzb = nzb[nzb > 0]                                                       # bin 0 never opens a window
    csum = np.concatenate(([0], np.cumsum(bins, dtype=np.int64)))
    max_count, r_best = 0, F(0)
    j = len(bins) - 1
    while j > 0:
        k = np.searchsorted(nzb, j, side="right")                            # the non-zero bins <= j
        if k == 0:
            break
        upbin = int(nzb[k - 1])
        j = max(upbin - BINS_PER_DR, -1)
        cur = int(csum[upbin + 1] - csum[j + 1])
        r_cur = F(upbin + j) / F(2) / F(BINS_PER_DR) * p.dp + F(p.min_radius)
        if F(cur) * r_best >= F(max_count) * r_cur or (r_best < EPS and cur >= max_count):
            r_best, max_count = r_cur, cur
        j -= 1
    return r_best, max_count


def candidates_vec(acc, pts, p, acc_t=None):
    acc_t = p.acc_t if acc_t is None else acc_t
    a = acc.reshape(-1)
    bs = centres_vec(acc, p, acc_t)
    cx = (((bs % p.astep).astype(F) + F(0.5)) * p.dp).astype(F)
    cy = (((bs // p.astep).astype(F) + F(0.5)) * p.dp).astype(F)
    if p.centers_only:
        return [(cx[i], cy[i], F(0), int(a[b]), int(b)) for i, b in enumerate(bs)]
    rows = []
    for i, b in enumerate(bs):
        r_best, max_count = scan_vec(bins_vec(cx[i], cy[i], pts, p), p)
        if max_count > acc_t and max_count > 0:
            rows.append((cx[i], cy[i], r_best, max_count, int(b)))
    return rows


def suppress_vec(rows, p, max_circles=None):
    if not rows:
        return np.zeros((0, 4), F)
    x, y, r, v, b = (np.array(c) for c in zip(*rows))
    order = np.lexsort((b, -v.astype(np.int64)))
    x, y, r, v = x[order].astype(F), y[order].astype(F), r[order].astype(F), v[order]
    md2 = p.min_dist * p.min_dist
    kept = []
    for i in range(len(x)):
        if kept:
            ddx, ddy = x[kept] - x[i], y[kept] - y[i]
            if np.any(ddx * ddx + ddy * ddy < md2):
                continue
        kept.append(i)
        if max_circles is not None and len(kept) == max_circles:
            break
    return np.stack([x[kept], y[kept], r[kept], v[kept].astype(F)], axis=1).astype(F)


def circles_vec(acc, pts, p, acc_t=None, max_circles=None):
    return suppress_vec(candidates_vec(acc, pts, p, acc_t), p, max_circles)


def hough_circles(edges, dx, dy, dp, min_dist, param1=100, param2=100, min_radius=0, max_radius=0, max_circles=None, vec=True, acc_t=None):
    """-> (accumulator, circles float32 [n, 4] of (x, y, r, votes))"""
    h, w = edges.shape
    p = prepare(w, h, dp, min_dist, param1, param2, min_radius, max_radius)
    if vec:
        acc, pts = accum_vec(edges, dx, dy, p)
        return acc, circles_vec(acc, pts, p, acc_t, max_circles)
    acc, nz = accum_loops(edges, dx, dy, p)
    return acc, circles_loops(acc, nz, p, acc_t, max_circles)


def same_bits(a, b):
    """two float32 arrays, bit for bit"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- frames
def discs_on_noise(h, w, discs, seed=0, noise=12):
    """bright discs (cx, cy, r) on a dim noisy ground, uint8"""
    rng = np.random.default_rng(seed)
    img = rng.integers(20, 20 + noise, (h, w)).astype(np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    for i, (cx, cy, r) in enumerate(discs):
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 170 + 20 * (i % 4)
    return img.astype(np.uint8)


def simple_gradients(img):
    """a 3 x 3 Sobel pair with replicated borders (int16) and a crude edge map, |gx| + |gy| above 200: stand-ins where the project's own Canny is not at hand"""
    a = np.pad(img.astype(np.int32), 1, mode="edge")
    gx = (a[:-2, 2:] + 2 * a[1:-1, 2:] + a[2:, 2:]) - (a[:-2, :-2] + 2 * a[1:-1, :-2] + a[2:, :-2])
    gy = (a[2:, :-2] + 2 * a[2:, 1:-1] + a[2:, 2:]) - (a[:-2, :-2] + 2 * a[:-2, 1:-1] + a[:-2, 2:])
    edges = ((np.abs(gx) + np.abs(gy)) > 200).astype(np.uint8) * 255
    return edges, gx.astype(np.int16), gy.astype(np.int16)


def random_planes(rng, h, w, density, zero_gradients=0.05):
    """a random edge map with random gradients, some of them (0, 0): such an edge pixel does not vote and is no point"""
    edges = ((rng.random((h, w)) < density) * rng.integers(1, 256, (h, w))).astype(np.uint8)
    dx = rng.integers(-1020, 1021, (h, w)).astype(np.int16)
    dy = rng.integers(-1020, 1021, (h, w)).astype(np.int16)
    z = rng.random((h, w)) < zero_gradients
    dx[z] = 0
    dy[z] = 0
    return edges, dx, dy


def uniform_planes(h, w, vx, vy):
    """every pixel an edge, one gradient everywhere"""
    return np.full((h, w), 255, np.uint8), np.full((h, w), vx, np.int16), np.full((h, w), vy, np.int16)


def empty_planes(h, w):
    return np.zeros((h, w), np.uint8), np.full((h, w), 5, np.int16), np.full((h, w), -3, np.int16)


DPS = (0.5, 1.0, 1.5, 2.0, 3.0)
RADII = ((0, 0), (5, 30), (10, 10), (3, -1))
