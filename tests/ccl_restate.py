"""A plain numpy / Python restatement of cv::connectedComponents and cv::connectedComponentsWithStats as include/mi355cv.h states them: a run-based two-pass
union-find, components numbered by sorting them on the key of the order asked for.  The GPU tests and the host build of ccl_math.h are held against it; the
CPU tests hold it against scipy.ndimage."""
import numpy as np

MAX_DIM = 16384
LIMIT_KEY = "ccl_max_dim"
TILE_W, STRIP_H = 256, 16                        # the tile of k_ccl_strip (opencv_amd/csrc/ccl_math.h)
PIXEL, BLOCK = "pixel", "block"
CCL_DEFAULT, CCL_WU, CCL_GRANA, CCL_BOLELLI, CCL_SAUF, CCL_BBDT, CCL_SPAGHETTI = -1, 0, 1, 2, 3, 4, 5


def order_of(connectivity, ccltype):
    """the numbering the library states for a (connectivity, ccltype) pair"""
    if connectivity == 4 or ccltype in (CCL_WU, CCL_SAUF):
        return PIXEL
    return BLOCK


def _runs(row):
    d = np.diff(np.concatenate(([0], (row != 0).astype(np.int8), [0])))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)          # starts, ends (exclusive)


def label(a, connectivity=8, order=PIXEL):
    """-> (n, labels int32): labels 0 .. n - 1, 0 the background; components numbered 1, 2, ... by their smallest pixel key y * w + x (PIXEL) or by their
    smallest block key (y >> 1) * ceil(w / 2) + (x >> 1) (BLOCK)"""
    a = np.asarray(a)
    assert a.ndim == 2 and connectivity in (4, 8) and order in (PIXEL, BLOCK)
    h, w = a.shape
    bw = (w + 1) >> 1
    slack = 1 if connectivity == 8 else 0
    parent, ry, rs, re = [], [], [], []

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    prev = (0, 0)                                                    # [first, last) run ids of the row above
    for y in range(h):
        s, e = _runs(a[y])
        first = len(parent)
        for xs, xe in zip(s.tolist(), e.tolist()):
            parent.append(len(parent)); ry.append(y); rs.append(xs); re.append(xe)
        p, c = prev[0], first
        while p < prev[1] and c < len(parent):
            if rs[p] < re[c] + slack and rs[c] < re[p] + slack:      # the runs touch
                u, v = find(p), find(c)
                if u != v:
                    parent[max(u, v)] = min(u, v)
            if re[p] < re[c]:
                p += 1
            else:
                c += 1
        prev = (first, len(parent))
    nr = len(parent)
    roots = np.array([find(i) for i in range(nr)], np.int64)
    ry, rs, re = np.array(ry, np.int64), np.array(rs, np.int64), np.array(re, np.int64)
    pkey = ry * w + rs
    key = pkey if order == PIXEL else (ry >> 1) * bw + (rs >> 1)
    big = np.iinfo(np.int64).max
    kmin = np.full(nr, big, np.int64)
    pmin = np.full(nr, big, np.int64)
    np.minimum.at(kmin, roots, key)
    np.minimum.at(pmin, roots, pkey)
    comps = np.flatnonzero(kmin != big)
    comps = comps[np.lexsort((pmin[comps], kmin[comps]))]
    lab_of = np.zeros(nr, np.int32)
    lab_of[comps] = np.arange(1, len(comps) + 1, dtype=np.int32)
    out = np.zeros((h, w), np.int32)
    rl = lab_of[roots]
    for i in range(nr):
        out[ry[i], rs[i]:re[i]] = rl[i]
    return len(comps) + 1, out


def stats(labels, n):
    """-> (stats int32 [n, 5]: left, top, width, height, area; centroids float64 [n, 2]).  A value >= n in the image is skipped.  A label without a pixel (label 0
    of a frame without background) has the five stats 0 and the centroid (nan, nan)."""
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    yy, xx = np.mgrid[0:h, 0:w]
    ok = (lab >= 0) & (lab < n)
    l, x, y = lab[ok], xx[ok].astype(np.int64), yy[ok].astype(np.int64)
    area = np.zeros(n, np.int64); sx = np.zeros(n, np.int64); sy = np.zeros(n, np.int64)
    np.add.at(area, l, 1); np.add.at(sx, l, x); np.add.at(sy, l, y)
    x0 = np.full(n, w, np.int64); y0 = np.full(n, h, np.int64); x1 = np.full(n, -1, np.int64); y1 = np.full(n, -1, np.int64)
    np.minimum.at(x0, l, x); np.minimum.at(y0, l, y); np.maximum.at(x1, l, x); np.maximum.at(y1, l, y)
    st = np.zeros((n, 5), np.int32)
    ce = np.full((n, 2), np.nan, np.float64)
    has = area > 0
    st[has] = np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1, area], 1)[has].astype(np.int32)
    ce[has, 0] = sx[has].astype(np.float64) / area[has].astype(np.float64)
    ce[has, 1] = sy[has].astype(np.float64) / area[has].astype(np.float64)
    return st, ce


def same_stats(got_stats, got_cent, want_stats, want_cent):
    """bit for bit: the ints equal, the doubles equal as bits except that a NaN matches a NaN"""
    gs, gc, ws, wc = np.asarray(got_stats), np.asarray(got_cent), np.asarray(want_stats), np.asarray(want_cent)
    if gs.dtype != np.int32 or gc.dtype != np.float64 or gs.shape != ws.shape or gc.shape != wc.shape or not np.array_equal(gs, ws):
        return False
    nan = np.isnan(wc)
    return np.array_equal(np.isnan(gc), nan) and np.array_equal(gc[~nan].view(np.uint64), wc[~nan].view(np.uint64))


# ---- the pattern list shared by the CPU emulation and the GPU tests
def random_frame(rng, h, w, density):
    return np.where(rng.random((h, w)) < density, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)


def serpentine(h, w):
    """a one-pixel-wide path: every other row full, joined alternately at the right and the left end -- one component"""
    a = np.zeros((h, w), np.uint8)
    a[0::2, :] = 255
    for i, y in enumerate(range(1, h, 2)):
        a[y, w - 1 if i % 2 == 0 else 0] = 255
    return a


def comb(h, w):
    """teeth in every other column that join only in the last row"""
    a = np.zeros((h, w), np.uint8)
    a[:, 0::2] = 1
    a[h - 1, :] = 1
    return a


def spiral(h, w):
    """a one-pixel-wide path that winds inwards with one pixel of background between its turns: one component"""
    a = np.zeros((h, w), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 7
    turns = 0
    while turns < 2:
        ny, nx, my, mx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < h and 0 <= nx < w and a[ny, nx] == 0 and not (0 <= my < h and 0 <= mx < w and a[my, mx])
        if free:
            y, x, turns = ny, nx, 0
            a[y, x] = 7
        else:
            dy, dx = dx, -dy
            turns += 1
    return a


def rings(h, w):
    """concentric rectangles two pixels apart: nested components, background enclosed by foreground"""
    a = np.zeros((h, w), np.uint8)
    for k in range(0, min(h, w) // 2, 2):
        a[k, k:w - k] = 9; a[h - 1 - k, k:w - k] = 9; a[k:h - k, k] = 9; a[k:h - k, w - 1 - k] = 9
    return a


def diagonals(h, w):
    """lines in both directions, three columns apart: connectivity 8 joins each line, 4 leaves single pixels; they cross every word and tile seam"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx + yy) % 7 == 0) | ((xx - yy) % 11 == 0), 200, 0).astype(np.uint8)


def seam_pairs(h, w, flip=0):
    """diagonal pixel pairs exactly at the 64-column word seams and the tile seams, the direction alternating from row pair to row pair (flip: the other way
    round, so that the pair across a strip seam is seen in both directions)"""
    a = np.zeros((h, w), np.uint8)
    for i, y in enumerate(range(0, h - 1, 3)):
        for s in range(64, w, 64):
            if (i + flip) % 2 == 0:
                a[y, s - 1] = 1; a[y + 1, s] = 1                     # down-right across the seam
            else:
                a[y, s] = 1; a[y + 1, s - 1] = 1                     # down-left across the seam
    return a


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) == 0).astype(np.uint8) * 255


def orders_differ(h, w):
    """in every block row an isolated pixel in the odd row to the left of an isolated pixel in the even row: the two orders number them the other way round"""
    a = np.zeros((h, w), np.uint8)
    for y in range(0, h - 1, 4):
        for x in range(0, w - 5, 8):
            a[y + 1, x] = 1
            a[y, x + 4] = 1
    return a


def patterns(h, w, seed=0):
    rng = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    out = {"random %g" % d: random_frame(rng, h, w, d) for d in (0.1, 0.41, 0.59, 0.9)}
    out["serpentine"] = serpentine(h, w)
    out["comb"] = comb(h, w)
    out["spiral"] = spiral(h, w)
    out["rings"] = rings(h, w)
    out["diagonals"] = diagonals(h, w)
    out["seam pairs"] = seam_pairs(h, w)
    out["seam pairs, flipped"] = seam_pairs(h, w, 1)
    out["checkerboard"] = checkerboard(h, w)
    out["orders differ"] = orders_differ(h, w)
    out["all foreground"] = np.full((h, w), 3, np.uint8)
    out["all background"] = np.zeros((h, w), np.uint8)
    return out
