"""Source views and guarded destination views for the hooks (test infrastructure, like refpatterns.py).

A large share of real cv::Mats are submatrices: the data pointer sits a few pixels into a parent row, the step is the parent's (wider than the row, rarely a
multiple of 16) and the bytes around the view belong to someone else.  This module builds such views for a given shape, dtype, channel count and LAYOUT, hands
them to an op, and checks three things: the result equals the oracle's for the contiguous copy of the view, no byte of the destination's parent outside the view
changed, and the source's parent did not change.

Layouts (source side, destination side).  Offsets are whole pixels, so every pointer stays element-aligned as a real ROI's is.  "base" is the byte offset of the
view from its allocation, "pitch" the parent's row bytes, both modulo 16:

  A  base 0, pitch 0                  | base 0, pitch 0                         control
  B  1 px in, ragged pitch            | another odd offset, another ragged pitch  everything misaligned (ROI of an odd-width parent)
  C  as A                             | as B                                    only the destination is misaligned
  D  as B                             | as A                                    only the source is misaligned
  E  base 0, pitch 4 or 8             | the same                                pointer aligned, step not: row 0 aligned, rows 1.. not
  F  base 4, pitch 0                  | base 8 or 12, pitch 0                   dword-aligned, not 16-byte aligned

"ragged" = not a multiple of 16, and not a multiple of 4 either where the pixel size allows it.  A layout a pixel size cannot give (no pixel offset has the
residue: 8-byte pixels have no base of 4) raises Unreachable with the reason.

Guards: ROWS_ABOVE / ROWS_BELOW parent rows around the view and at least TAIL_BYTES after the end of every view row, inside the allocation, so that a kernel that
overruns by a vector or a row fails an assertion instead of faulting.  The destination parent is filled with per-byte pseudo-random data from a fixed seed (a
constant would hide a stray 0 or 255); the source parent outside the view is hostile (NaN for float depths, the depth's extremes -- which `content` never
produces -- otherwise), so a kernel that reads the parent where the border rule applies changes its output.

Beyond one source and one destination, `run` takes further read-only inputs (maps), several guarded destinations from one call, and a destination that is an
input too; `run_batch` takes frames in the forms of BATCH_FORMS_ALL and in ALIGNED, the control of 'oddstride'.  tests/test_viewcheck_cpu.py holds a correct and a
deliberately wrong numpy stand-in against each of these.
"""
import numpy as np

LAYOUTS = ("A", "B", "C", "D", "E", "F")
_SIDES = {"A": ("a", "a"), "B": ("b", "b2"), "C": ("a", "b2"), "D": ("b", "a"), "E": ("e", "e"), "F": ("f", "f2")}
ROWS_ABOVE, ROWS_BELOW, TAIL_BYTES = 4, 2, 64      # 4 rows above: 4 * pitch is a multiple of 16 for every pitch that is a multiple of 4 (layout E's base 0)
SENTINEL_SEED = 0x5EED
# every (depth, channels) a source, a map or a destination of tests/test_views_gpu.py and tests/test_warp_views_gpu.py has; tests/test_viewcheck_cpu.py checks the
# layouts' residues for each.  (CV_32FC4 is not among them on purpose: its pixels have 16 bytes, so layout B cannot be built for it.)
PIXELS_USED = [(np.uint8, 1), (np.uint8, 2), (np.uint8, 3), (np.uint8, 4), (np.uint16, 1), (np.uint16, 3), (np.int16, 1), (np.int16, 2), (np.int32, 1),
               (np.float32, 1), (np.float32, 2), (np.float32, 3), (np.float64, 1)]


class Unreachable(Exception):
    """the layout cannot be built for this pixel size; str() is the reason"""


class GuardTouched(AssertionError):
    """a byte of a parent outside the view changed.  row / byte: position in the parent; rel_row / rel_byte: relative to the view's first row / to the first
    byte of the view's row; where: 'above', 'below', 'left', 'right' (of the view, on one of its rows), 'inside' (a source view that changed), 'gap' (the bytes
    between two frames of an 'oddstride' batch: row = the parent's row count, byte = the byte of the gap, frame = the frame the gap follows)"""

    def __init__(self, what, row, byte, rel_row, rel_byte, where, past_end, frame=None):
        self.row, self.byte, self.rel_row, self.rel_byte, self.where, self.past_end, self.frame = row, byte, rel_row, rel_byte, where, past_end, frame
        at = "" if frame is None else "frame %d, " % frame
        msg = "%s: guard touched at %sparent (row %d, byte %d) = view row %+d, byte %+d of the view row: %s the view" % (what, at, row, byte, rel_row, rel_byte, where)
        if where == "right":
            msg += ", %d byte(s) past the row end" % past_end
        super().__init__(msg)


class ResultMismatch(AssertionError):
    """the view's content is not the oracle's result; index: first differing element (row, column[, channel]) or None when the comparison is a norm"""

    def __init__(self, what, index, detail):
        self.index = index
        super().__init__("%s: result differs from the oracle%s%s" % (what, "" if index is None else " first at " + str(tuple(int(i) for i in index)), detail))


def pixel_bytes(dtype, cn):
    return np.dtype(dtype).itemsize * cn


def _first(rng_, ok):
    for v in rng_:
        if ok(v):
            return v
    return None


def side_plan(kind, px, w):
    """(x0, wp): the view's first column and the parent's width in pixels for one side of a layout ('a', 'b', 'b2', 'e', 'f', 'f2'), pixels of px bytes, w columns"""
    tail = -(-TAIL_BYTES // px)

    def width(x0, ok, start=0):
        need = max(x0 + w + tail, start)
        return _first(range(need, need + 64), lambda wp: ok(wp * px))

    if kind == "a":
        return 0, width(0, lambda p: p % 16 == 0)
    if kind in ("b", "b2"):
        if px % 16 == 0:
            raise Unreachable("pixels of %d bytes: every pitch and every pixel offset is a multiple of 16" % px)
        x0 = 1 if kind == "b" else 3

        def ragged(p, x=x0):
            base = ROWS_ABOVE * p + x * px
            return p % 16 != 0 and base % 16 != 0 and (px % 4 == 0 or (p % 4 != 0 and base % 4 != 0))
        if kind == "b":
            return x0, width(x0, ragged)
        _, wb = side_plan("b", px, w)                                  # "a different ragged pitch": another residue than side b's for the same row
        return x0, width(x0, lambda p: ragged(p) and p % 16 != (wb * px) % 16 if px % 8 else ragged(p), wb + 1)
    if kind == "e":
        for res in (4, 8):
            wp = width(0, lambda p, r=res: p % 16 == r)
            if wp is not None:
                return 0, wp
        raise Unreachable("pixels of %d bytes: no parent width gives a pitch of 4 or 8 modulo 16" % px)
    want = (4,) if kind == "f" else (12, 8)
    for res in want:
        x0 = _first(range(1, 17), lambda x, r=res: (x * px) % 16 == r)
        if x0 is not None:
            return x0, width(x0, lambda p: p % 16 == 0)
    raise Unreachable("pixels of %d bytes: no pixel offset gives a base of %s modulo 16" % (px, " or ".join(str(r) for r in want)))


class Geometry:
    """where a view of h x w pixels (px bytes each) sits in its parent"""

    def __init__(self, kind, dtype, cn, w, h, ndim):
        self.kind, self.dtype, self.cn, self.w, self.h, self.ndim = kind, np.dtype(dtype), cn, w, h, ndim
        self.px = pixel_bytes(dtype, cn)
        self.x0, self.wp = side_plan(kind, self.px, w)
        self.y0, self.hp = ROWS_ABOVE, ROWS_ABOVE + h + ROWS_BELOW
        self.pitch = self.wp * self.px
        self.base = self.y0 * self.pitch + self.x0 * self.px

    def parent_shape(self):
        return (self.hp, self.wp) + ((self.cn,) if self.ndim == 3 else ())

    def view(self, parent):
        return parent[self.y0:self.y0 + self.h, self.x0:self.x0 + self.w]


def plan(layout, src_dtype, src_cn, w, h, dst_dtype=None, dst_cn=None, dw=None, dh=None, src_ndim=None, dst_ndim=None):
    """(source Geometry, destination Geometry or None) of a layout; raises Unreachable where a side cannot be built"""
    ks, kd = _SIDES[layout]
    s = Geometry(ks, src_dtype, src_cn, w, h, src_ndim or (3 if src_cn > 1 else 2))
    if dst_dtype is None:
        return s, None
    d = Geometry(kd, dst_dtype, dst_cn, w if dw is None else dw, h if dh is None else dh, dst_ndim or (3 if dst_cn > 1 else 2))
    return s, d


_RANGE = {np.dtype(np.uint8): (8, 248), np.dtype(np.int8): (-100, 100), np.dtype(np.uint16): (256, 65000), np.dtype(np.int16): (-30000, 30000),
          np.dtype(np.int32): (-(1 << 30), 1 << 30)}


def content(dtype, shape, seed, lo=None, hi=None):
    """pseudo-random view content: integers inside the depth's range minus its ends (the hostile values), floats in [lo, hi) (default [-1, 2))"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        lo, hi = (-1.0 if lo is None else lo), (2.0 if hi is None else hi)
        return (rng.random(shape) * (hi - lo) + lo).astype(dtype)
    a, b = _RANGE[dtype]
    return rng.integers(a if lo is None else max(a, lo), b if hi is None else min(b, hi), shape).astype(dtype)


def tame(image):
    """an image of the caller's (a scene, a packed YUV frame) with the depth's extremes, which are the hostile values, clipped away"""
    image = np.asarray(image)
    if image.dtype.kind == "f":
        return image
    a, b = _RANGE[image.dtype]
    return np.clip(image, a, b - 1).astype(image.dtype)


def hostile(dtype, shape):
    """what surrounds a source view: NaN for floats; for integers the depth's two extremes in a checkerboard"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.full(shape, np.nan, dtype)
    info = np.iinfo(dtype)
    yy, xx = np.indices(shape[:2])
    board = np.where((yy + xx) % 2 == 0, info.max, info.min).astype(dtype)
    return board if len(shape) == 2 else np.repeat(board[:, :, None], shape[2], axis=2)


def sentinel(dtype, shape, seed=SENTINEL_SEED):
    """per-byte pseudo-random fill of a destination parent"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).view(dtype).reshape(shape).copy()


def source_parent(geom, image):
    parent = hostile(geom.dtype, geom.parent_shape())
    geom.view(parent)[...] = image
    return parent


def _rows_of_bytes(a, pitch):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, pitch)


def check_guard(what, before, after, geom, frames=None, whole=False):
    """`after` (the parent after the call) equals `before` (the sentinel / the hostile parent) in every byte outside the view; raises GuardTouched for the first
    byte that differs.  frames=(f0, n): the parents are [F, hp, wp(, cn)] and the views are geom's view of frames f0 .. f0 + n - 1.  whole: the view counts as
    guard too (a source must not change at all)"""
    expect = np.array(before, copy=True)
    if whole:
        pass
    elif frames is None:
        geom.view(expect)[...] = geom.view(after)
    else:
        f0, n = frames
        expect[f0:f0 + n, geom.y0:geom.y0 + geom.h, geom.x0:geom.x0 + geom.w] = after[f0:f0 + n, geom.y0:geom.y0 + geom.h, geom.x0:geom.x0 + geom.w]
    e, g = _rows_of_bytes(expect, geom.pitch), _rows_of_bytes(after, geom.pitch)
    bad = np.argwhere(e != g)
    if len(bad) == 0:
        return
    row, byte = (int(v) for v in bad[0])
    frame, prow = (None, row) if frames is None else (row // geom.hp, row % geom.hp)
    rel_row, rel_byte = prow - geom.y0, byte - geom.x0 * geom.px
    rowb = geom.w * geom.px
    if frames is not None and not (frames[0] <= frame < frames[0] + frames[1]):
        where = "above" if frame < frames[0] else "below"
    elif rel_row < 0:
        where = "above"
    elif rel_row >= geom.h:
        where = "below"
    elif 0 <= rel_byte < rowb:
        where = "inside"
    else:
        where = "left" if rel_byte < 0 else "right"
    raise GuardTouched(what, prow, byte, rel_row, rel_byte, where, rel_byte - rowb, None if frames is None else frame - frames[0])


def exact(got, want):
    """bit for bit: the two arrays hold the same bytes (so equal NaNs are equal, and -0.0 is not 0.0)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False, None, " (shape / dtype %s %s, expected %s %s)" % (got.shape, got.dtype, want.shape, want.dtype)
    isz = got.dtype.itemsize
    bad = np.argwhere((got.view(np.uint8).reshape(got.shape + (isz,)) != want.view(np.uint8).reshape(want.shape + (isz,))).any(axis=-1))
    if len(bad) == 0:
        return True, None, ""
    i = tuple(bad[0])
    return False, i, ": got %r, expected %r, %d element(s) differ" % (got[i], want[i], len(bad))


def check_result(what, got, want, compare=exact):
    ok, index, detail = compare(got, want)
    if not ok:
        raise ResultMismatch(what, index, detail)


class Host:
    """numpy stand-in for the device: parents live where they are made"""
    @staticmethod
    def put(a):
        return a

    @staticmethod
    def get(a):
        return np.asarray(a)


def _geometry_like(kind, dtype, shape):
    return Geometry(kind, dtype, shape[2] if len(shape) == 3 else 1, shape[1], shape[0], len(shape))


def run(call, layout, image, want, what="", compare=exact, device=Host, kernel_name=None, inputs=(), dst_like=None):
    """One op on one layout.  image: the source view's content, contiguous [h, w] or [h, w, cn]; want: the oracle's result for it (it fixes the destination's
    shape and dtype), or None for an op without an image output.  call(src_view, dst_view) runs the op into dst_view; without a destination it is
    call(src_view, None) and its return value is handed back.  device: put(ndarray) -> the array the op takes, get(array) -> ndarray.  kernel_name() is read
    right after the call.  Returns (kernel name or None, the op's return value).

    inputs: further read-only operands (the maps of remap and convertMaps).  Each is placed like the source side of the layout inside a hostile parent of its
    own, the views follow the destination -- call(src_view, dst_view, *input_views) -- and every parent is checked unchanged afterwards.

    want as a tuple or list of arrays: that many guarded destinations from one call (convertMaps); dst_view is then the tuple of their views, each in a parent
    of its own with its own sentinel, and compare may be a tuple as well.

    want as a callable, with dst_like = (dtype, shape): the destination is an input too (BORDER_TRANSPARENT keeps what the map does not reach).  The view starts
    with its parent's sentinel; want(prev) gets a copy of that content -- it is the oracle's dst= -- and returns the expected array."""
    image = np.ascontiguousarray(image)
    inputs = [np.ascontiguousarray(a) for a in inputs]
    ks, kd = _SIDES[layout]
    sg = _geometry_like(ks, image.dtype, image.shape)
    igs = [_geometry_like(ks, a.dtype, a.shape) for a in inputs]
    several = isinstance(want, (tuple, list))
    if want is None:
        wants = []
    elif callable(want):
        wants = [want]
    else:
        wants = [np.ascontiguousarray(w) for w in (want if several else [want])]
    dgs = [_geometry_like(kd, *(dst_like if callable(w) else (w.dtype, w.shape))) for w in wants]
    compares = list(compare) if isinstance(compare, (tuple, list)) else [compare] * len(wants)
    sp0 = source_parent(sg, image)
    sp = device.put(sp0.copy())
    ip0 = [source_parent(g, a) for g, a in zip(igs, inputs)]
    ip = [device.put(p.copy()) for p in ip0]
    dp0 = [sentinel(g.dtype, g.parent_shape(), SENTINEL_SEED + k) for k, g in enumerate(dgs)]
    dp = [device.put(p.copy()) for p in dp0]
    dviews = [g.view(p) for g, p in zip(dgs, dp)]
    rv = call(sg.view(sp), tuple(dviews) if several else dviews[0] if dviews else None, *[g.view(p) for g, p in zip(igs, ip)])
    name = kernel_name() if kernel_name else None
    after = [device.get(p) for p in dp]
    tag = lambda k: " dst %d" % k if several else ""                                 # noqa: E731
    for k, g in enumerate(dgs):
        check_guard(what + tag(k), dp0[k], after[k], g)
    check_guard(what + " source", sp0, device.get(sp), sg, whole=True)
    for k, g in enumerate(igs):
        check_guard(what + " input %d" % k, ip0[k], device.get(ip[k]), g, whole=True)
    for k, g in enumerate(dgs):
        expected = wants[k](np.array(g.view(dp0[k]), copy=True)) if callable(wants[k]) else wants[k]
        check_result(what + tag(k), g.view(after[k]), expected, compares[k])
    return name, rv


def run_inplace(call, image, want, what="", compare=exact, device=Host, kernel_name=None):
    """In place on a layout-B source view: call(view, view); the source's hostile parent doubles as the guard"""
    image = np.ascontiguousarray(image)
    h, w = image.shape[:2]
    cn = image.shape[2] if image.ndim == 3 else 1
    sg, _ = plan("B", image.dtype, cn, w, h, src_ndim=image.ndim)
    sp0 = source_parent(sg, image)
    sp = device.put(sp0.copy())
    v = sg.view(sp)
    rv = call(v, v)
    name = kernel_name() if kernel_name else None
    after = device.get(sp)
    check_guard(what + " in place", sp0, after, sg)
    check_result(what + " in place", sg.view(after), want, compare)
    return name, rv


BATCH_FORMS = ("roi", "columns")
ODDSTRIDE, ALIGNED = "oddstride", "aligned"
BATCH_FORMS_ALL = BATCH_FORMS + (ODDSTRIDE,)


def batch_geometry(form, dtype, cn, w, h, ndim):
    """frames as views of a parent [n + 2, hp, wp(, cn)] (a guard frame before and after): 'roi' = parent[1:-1, 2:2+h, 3:3+w], base, pitch and frame stride all
    ragged; 'columns' = parent[1:-1, :, 3:3+w], full height, so the frame stride is step * h (frames back to back are one tall image, with a step wider than the row).

    'aligned' = parent[1:-1, 2:2+h, 0:w] with a pitch that is a multiple of 16: pointer, step and frame stride all pass every alignment predicate.  It is the control
    of 'oddstride', which has the same frames, but in one flat allocation in which every frame's [hp, wp] block is followed by a gap of one element (g.gap bytes):
    the first frame and the step stay multiples of 16 and the frame stride hp * pitch + 1 (1-byte elements) / + 2 (2-byte elements) is the only thing that is no
    multiple of 4 -- what as_strided, or a header in front of every frame, gives.  That form is not built for wider elements: a frame stride has to be a multiple
    of the element size, so it would be a multiple of 4."""
    if form in (ODDSTRIDE, ALIGNED):
        g = Geometry("a", dtype, cn, w, h, ndim)                        # x0 = 0, pitch a multiple of 16 (the tail of the row above is the guard on the left)
    else:
        g = Geometry("b2", dtype, cn, w, h, ndim)                       # x0 = 3, ragged pitch
    if form == "columns":
        g.y0, g.hp = 0, h
    else:
        g.y0, g.hp = 2, h + 4
    g.gap = 0
    if form == ODDSTRIDE:
        if g.dtype.itemsize > 2:
            raise ValueError("the 'oddstride' form is built for 1- and 2-byte elements, not for %s" % g.dtype)
        g.gap = g.dtype.itemsize
    g.frame_stride = g.hp * g.pitch + g.gap
    g.base = g.y0 * g.pitch + g.x0 * g.px
    return g


def _strided(flat, dtype, shape, strides, offset):
    """a view of the flat typed 1-D array `flat` (numpy, or a tensor: anything else with as_strided(size, stride, storage_offset)); strides and offset in bytes"""
    if isinstance(flat, np.ndarray):
        return np.ndarray(shape, dtype, buffer=flat, offset=offset, strides=strides)
    isz = np.dtype(dtype).itemsize
    assert offset % isz == 0 and all(v % isz == 0 for v in strides)
    return flat.as_strided(tuple(shape), tuple(v // isz for v in strides), offset // isz)


def _odd_offset(g, k):
    """byte offset of block k of the flat allocation: the guard block (k = 0), the frames' blocks, each followed by its gap, the guard block behind them"""
    return k * g.hp * g.pitch + max(k - 1, 0) * g.gap


def _odd_flat(g, blocks):
    """blocks [n + 2, hp, wp(, cn)] -> the flat allocation (typed, 1-D); the gaps hold a sentinel of their own"""
    nb, body = blocks.shape[0], g.hp * g.pitch
    flat = np.random.default_rng(SENTINEL_SEED ^ 0xA5).integers(0, 256, _odd_offset(g, nb - 1) + body, dtype=np.uint8)
    rows = np.ascontiguousarray(blocks).reshape(nb, -1).view(np.uint8)
    for k in range(nb):
        flat[_odd_offset(g, k):_odd_offset(g, k) + body] = rows[k]
    return flat.view(g.dtype)


def _odd_split(g, flat, nb):
    """the flat allocation -> (blocks [n + 2, hp, wp(, cn)], gap bytes [n, g.gap]: the gap behind each frame)"""
    b, body = np.ascontiguousarray(flat).view(np.uint8), g.hp * g.pitch
    blocks = np.stack([b[_odd_offset(g, k):_odd_offset(g, k) + body] for k in range(nb)])
    gaps = np.stack([b[_odd_offset(g, k) + body:_odd_offset(g, k) + body + g.gap] for k in range(1, nb - 1)])
    return np.ascontiguousarray(blocks).view(g.dtype).reshape((nb,) + g.parent_shape()), gaps


def _odd_frames(g, flat, n):
    isz = g.dtype.itemsize
    shape = (n, g.h, g.w) + ((g.cn,) if g.ndim == 3 else ())
    strides = (g.frame_stride, g.pitch, g.px) + ((isz,) if g.ndim == 3 else ())
    return _strided(flat, g.dtype, shape, strides, _odd_offset(g, 1) + g.base)


def check_gaps(what, before, after, geom):
    """the gap bytes of an 'oddstride' allocation (before, after: [n, gap], the gap behind each frame) did not change"""
    bad = np.argwhere(before != after)
    if len(bad):
        block, byte = (int(v) for v in bad[0])
        raise GuardTouched(what, geom.hp, byte, geom.hp - geom.y0, byte - geom.x0 * geom.px, "gap", 0, block)


def run_batch(call, form, frames, want, what="", compare=exact, device=Host, kernel_name=None):
    """frames [n, h, w(, cn)] -> want [n, dh, dw(, dcn)] through call(src_views, dst_views), both views of guarded parents in the given form"""
    frames, want = np.ascontiguousarray(frames), np.ascontiguousarray(want)
    n, h, w = frames.shape[:3]
    sg = batch_geometry(form, frames.dtype, frames.shape[3] if frames.ndim == 4 else 1, w, h, frames.ndim - 1)
    dg = batch_geometry(form, want.dtype, want.shape[3] if want.ndim == 4 else 1, want.shape[2], want.shape[1], want.ndim - 1)
    sp0 = np.stack([hostile(sg.dtype, sg.parent_shape())] * (n + 2))
    sp0[1:n + 1, sg.y0:sg.y0 + h, sg.x0:sg.x0 + w] = frames
    dp0 = sentinel(dg.dtype, (n + 2,) + dg.parent_shape())
    if form == ODDSTRIDE:
        sf0, df0 = _odd_flat(sg, sp0), _odd_flat(dg, dp0)
        sf, df = device.put(sf0.copy()), device.put(df0.copy())
        rv = call(_odd_frames(sg, sf, n), _odd_frames(dg, df, n))
        name = kernel_name() if kernel_name else None
        after, dgaps = _odd_split(dg, device.get(df), n + 2)
        safter, sgaps = _odd_split(sg, device.get(sf), n + 2)
        check_guard(what + " " + form, dp0, after, dg, frames=(1, n))
        check_gaps(what + " " + form, _odd_split(dg, df0, n + 2)[1], dgaps, dg)
        check_guard(what + " " + form + " source", sp0, safter, sg, frames=(1, n), whole=True)
        check_gaps(what + " " + form + " source", _odd_split(sg, sf0, n + 2)[1], sgaps, sg)
    else:
        sp, dp = device.put(sp0.copy()), device.put(dp0.copy())
        rv = call(sp[1:n + 1, sg.y0:sg.y0 + h, sg.x0:sg.x0 + w], dp[1:n + 1, dg.y0:dg.y0 + dg.h, dg.x0:dg.x0 + dg.w])
        name = kernel_name() if kernel_name else None
        after = device.get(dp)
        check_guard(what + " " + form, dp0, after, dg, frames=(1, n))
        check_guard(what + " " + form + " source", sp0, device.get(sp), sg, frames=(1, n), whole=True)
    got = after[1:n + 1, dg.y0:dg.y0 + dg.h, dg.x0:dg.x0 + dg.w]
    for f in range(n):
        check_result("%s %s frame %d" % (what, form, f), got[f], want[f], compare)
    return name, rv
