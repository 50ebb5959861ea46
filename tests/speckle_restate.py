"""cv::filterSpeckles as this project serves it, written three times: the reference's raster scan with flood fills that erases as it goes (filter_scan),
the graph form -- live pixels, links between 4-neighbours with |a - b| <= maxDiff, components by a loop union-find, sizes, erase (filter_graph) -- and a numpy form that
spreads the smallest pixel index over the two link planes until nothing changes (filter_np).  tests/test_speckle_cpu.py holds the three against each other; the GPU is
held against filter_graph.  Below them: the inputs the tests share, among them cases whose answer is known by construction."""
import numpy as np


def _check(img, newVal):
    assert img.ndim == 2 and img.dtype in (np.uint8, np.int16)
    info = np.iinfo(img.dtype)
    assert info.min <= int(newVal) <= info.max, "newVal outside the depth's range is declined, not served"


def filter_scan(img, newVal, maxSpeckleSize, maxDiff):
    """the reference's order of work: a raster scan; an unlabelled live pixel starts a flood fill over unlabelled live neighbours within maxDiff, the fill's pixel count
    decides whether the label is small; a pixel whose label is small is erased when the scan reaches it"""
    _check(img, newVal)
    out = img.copy()
    H, W = out.shape
    newVal, maxDiff = int(newVal), int(maxDiff)
    labels = np.zeros((H, W), np.int64)
    small = {}
    cur = 0
    for i in range(H):
        for j in range(W):
            if int(out[i, j]) == newVal:
                continue
            if labels[i, j]:
                if small[labels[i, j]]:
                    out[i, j] = newVal
                continue
            cur += 1
            labels[i, j] = cur
            stack, count = [(i, j)], 0
            while stack:
                y, x = stack.pop()
                count += 1
                v = int(out[y, x])
                for yy, xx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                    if 0 <= yy < H and 0 <= xx < W and not labels[yy, xx] and int(out[yy, xx]) != newVal and abs(v - int(out[yy, xx])) <= maxDiff:
                        labels[yy, xx] = cur
                        stack.append((yy, xx))
            small[cur] = count <= maxSpeckleSize
            if small[cur]:
                out[i, j] = newVal
    return out


def link_planes(img, newVal, maxDiff):
    """live, link-left (pixel linked to its left neighbour), link-up (to its upper neighbour); differences in Python / int64, so that CV_16S cannot wrap"""
    v = img.astype(np.int64)
    live = v != int(newVal)
    left = np.zeros_like(live)
    up = np.zeros_like(live)
    left[:, 1:] = live[:, 1:] & live[:, :-1] & (np.abs(v[:, 1:] - v[:, :-1]) <= int(maxDiff))
    up[1:, :] = live[1:, :] & live[:-1, :] & (np.abs(v[1:, :] - v[:-1, :]) <= int(maxDiff))
    return live, left, up


def components(img, newVal, maxDiff):
    """root[y, x] = the smallest linear index of the pixel's component (-1 where not live), by a loop union-find over the links"""
    live, left, up = link_planes(img, newVal, maxDiff)
    H, W = img.shape
    par = list(range(H * W))

    def find(a):
        r = a
        while par[r] != r:
            r = par[r]
        while par[a] != r:
            par[a], a = r, par[a]
        return r

    ys, xs = np.nonzero(left)
    pairs = [(y * W + x, y * W + x - 1) for y, x in zip(ys.tolist(), xs.tolist())]
    ys, xs = np.nonzero(up)
    pairs += [(y * W + x, (y - 1) * W + x) for y, x in zip(ys.tolist(), xs.tolist())]
    for a, b in pairs:
        a, b = find(a), find(b)
        if a != b:
            par[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(H * W)], np.int64).reshape(H, W)
    root[~live] = -1
    return root


def _erase(img, root, newVal, maxSpeckleSize):
    out = img.copy()
    live = root >= 0
    size = np.bincount(root[live], minlength=img.size)
    kill = np.zeros(img.shape, bool)
    kill[live] = size[root[live]] <= int(maxSpeckleSize)
    out[kill] = newVal
    return out


def filter_graph(img, newVal, maxSpeckleSize, maxDiff):
    _check(img, newVal)
    return _erase(img, components(img, newVal, maxDiff), newVal, maxSpeckleSize)


def filter_np(img, newVal, maxSpeckleSize, maxDiff):
    """every live pixel starts with its own index and takes the minimum over its links, again and again, until nothing changes"""
    _check(img, newVal)
    live, left, up = link_planes(img, newVal, maxDiff)
    H, W = img.shape
    big = H * W
    lab = np.where(live, np.arange(H * W, dtype=np.int64).reshape(H, W), big)
    while True:
        new = lab.copy()
        new[:, 1:] = np.where(left[:, 1:], np.minimum(new[:, 1:], lab[:, :-1]), new[:, 1:])
        new[:, :-1] = np.where(left[:, 1:], np.minimum(new[:, :-1], lab[:, 1:]), new[:, :-1])
        new[1:, :] = np.where(up[1:, :], np.minimum(new[1:, :], lab[:-1, :]), new[1:, :])
        new[:-1, :] = np.where(up[1:, :], np.minimum(new[:-1, :], lab[1:, :]), new[:-1, :])
        if np.array_equal(new, lab):
            break
        lab = new
    root = np.where(live, lab, -1)
    return _erase(img, root, newVal, maxSpeckleSize)


# ---------------------------------------------------------------------------------------------------------------- inputs
def few_levels(rng, H, W, dtype):
    """2 .. 6 levels times a step of 1 .. 3 around a base, so that chains of links occur; returns (image, a newVal among its values)"""
    levels, step = int(rng.integers(2, 7)), int(rng.integers(1, 4))
    base = int(rng.integers(0, 200)) if dtype == np.uint8 else int(rng.integers(-300, 300))
    img = (base + step * rng.integers(0, levels, (H, W))).astype(dtype)
    return img, int(img.flat[int(rng.integers(0, img.size))])


def checkerboard(H, W, dtype, a, b):
    y, x = np.mgrid[0:H, 0:W]
    return np.where((x + y) & 1, b, a).astype(dtype)


def serpentine(H, W, dtype, fg, bg, transpose=False):
    """a path one pixel wide: every other row in full, joined at alternating ends; returns (image, the number of path pixels)"""
    if transpose:
        img, n = serpentine(W, H, dtype, fg, bg)
        return np.ascontiguousarray(img.T), n
    img = np.full((H, W), bg, dtype)
    img[0::2, :] = fg
    for k, y in enumerate(range(1, H - 1, 2)):                                 # a joint only where a full row follows
        img[y, W - 1 if k % 2 == 0 else 0] = fg
    return img, int((img == fg).sum())


def spiral(H, W, dtype, fg, bg):
    """a path one pixel wide that winds inwards with one pixel between its turns; returns (image, the number of path pixels)"""
    on = np.zeros((H, W), bool)
    y = x = 0
    on[0, 0] = True
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    d = 0

    def free(yy, xx):
        return 0 <= yy < H and 0 <= xx < W and not on[yy, xx]

    def can(yy, xx, dy, dx):
        ny, nx = yy + dy, xx + dx
        if not free(ny, nx):
            return False
        # the cell after the next one and the next one's side neighbours must be free too, or the path would touch itself
        for ay, ax in ((ny + dy, nx + dx), (ny + dx, nx + dy), (ny - dx, nx - dy)):
            if 0 <= ay < H and 0 <= ax < W and on[ay, ax] and (ay, ax) != (yy, xx):
                return False
        return True

    while True:
        dy, dx = dirs[d]
        if can(y, x, dy, dx):
            y, x = y + dy, x + dx
            on[y, x] = True
            continue
        d = (d + 1) % 4
        dy, dx = dirs[d]
        if not can(y, x, dy, dx):
            break
    return np.where(on, fg, bg).astype(dtype), int(on.sum())


def blob(img, y, x, size, width, value):
    """`size` pixels of `value` filled row-major into rows `width` wide from (y, x)"""
    for k in range(size):
        img[y + k // width, x + k % width] = value


PLANTED_S = 12


def planted(H=48, W=160, places=None):
    """a CV_16S plane of 320 with blobs of 800; newVal = -16, maxDiff = 16, maxSpeckleSize = S = 12.  Returns (image, the expected image built by construction: the
    blobs of size <= S become -16, everything else is unchanged, the number of pixels that change)"""
    S = PLANTED_S
    if places is None:
        places = ((S - 1, 3, 5, 4), (S, 3, 62, 4), (S + 1, 14, 62, 4), (S + 2, 30, 126, 5), (S, 15, 30, 1), (S + 1, 30, 3, 13))
    img = np.full((H, W), 320, np.int16)
    want = img.copy()
    changed = 0
    for size, y, x, width in places:
        blob(img, y, x, size, width, 800)
        blob(want, y, x, size, width, -16 if size <= S else 800)
        changed += size if size <= S else 0
    return img, want, changed


def planted_seams(tw, th):
    """the same blobs placed so that those of S and S + 1 pixels straddle a vertical and a horizontal seam of tiles tw x th"""
    S = PLANTED_S
    places = ((S - 1, 3, 5, 4), (S, th - 1, tw - 2, 4), (S + 1, 2 * th - 2, tw - 2, 4), (S + 2, th - 1, 2 * tw - 2, 5), (S, th - 6, 30, 1), (S + 1, th + 4, tw - 6, 13))
    return planted(2 * th + 3, 2 * tw + 3, places)


def ramp(H=4, W=160):
    return np.tile((16 * np.arange(W)).astype(np.int16), (H, 1))
