"""resize, warpAffine, warpPerspective, remap, convertMaps and warpPolar on misaligned, pitched ROI views with guarded
destinations: tests/test_views_gpu.py's table for the geometric family.  tests/test_warp_gpu.py feeds fresh tensors (apart from two aligned windows), so the pointer
half of every alignment predicate in runWarp / runResize / warp8::plan / warp8::planResize, the four-pixels-per-lane dword stores next to bytes that belong to someone
else, map steps other than the row bytes and the batch entries' frame strides are invisible there.  Every row runs on the six layouts of viewcheck.LAYOUTS; source,
every map and every destination are views.  The result equals the oracle's (tests/orc.py, pinned to the reference by tests/test_oracle_warp.py) for the contiguous
copies under the comparison the op's own suite uses (the line it is taken from is cited at each section), no byte of a destination's parent outside the view changes,
and no source or map parent changes.  Around float views lies NaN, so a kernel that multiplies a neighbour of the ROI by a zero weight fails -- on purpose.

Layout A is the control: a row with kernel= asserts that at least one of its shapes reached the fast kernel the row is about.  A row may skip only on layout F and only
where an operand has 8-byte pixels (a CV_32FC2 map as an input: no pixel offset gives a base of 4 modulo 16).  The kernel each (row, layout) ran is printed at the end
of the module (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import orc as O
import viewcheck as vc
from viewtable import Device, img, last_kernel, marked, print_kernel_table, rel, short

pytestmark = pytest.mark.gpu

U8, U16, S16, F32 = np.uint8, np.uint16, np.int16, np.float32
SHAPES = [(13, 5), (64, 19), (131, 37)]         # under 16 bytes a row / exactly one 64-column tile, whole vectors / a third tile with a ragged last chunk, more rows than one tile of rows
EVEN = [(14, 6), (64, 20), (132, 38)]           # the 2 x 2 area mean: destinations of 7 (a lane's scalar tail only), 32 and 66 columns
KERNELS = {}                                    # (row, layout or batch form) -> set of kernel names
INVERSE, RELATIVE = 16, 32                      # WARP_INVERSE_MAP, WARP_RELATIVE_MAP
CONSTANT, REPLICATE, REFLECT, REFLECT_101, TRANSPARENT = 0, 1, 2, 4, 5
BVAL = (10, 200, 30, 77)
T16SC2, T32FC1, T32FC2 = 3 + 8, 5, 5 + 8        # CV_MAKETYPE
WARP8 = ("k_warp8_lean", "k_warp8_tile", "k_warp8_cubic", "k_resize8_lean")          # the kernels that read and store whole aligned dwords (warp8.h)


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    yield opencv_amd
    print_kernel_table(KERNELS, vc.LAYOUTS + vc.BATCH_FORMS + (vc.ALIGNED, vc.ODDSTRIDE))


def same_values(got, want):
    """np.array_equal, as the exact suites of resize assert it (tests/test_warp_gpu.py:102, :115, :129, :342, :358, :463): a NaN equals nothing"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False, None, " (shape / dtype %s %s, expected %s %s)" % (got.shape, got.dtype, want.shape, want.dtype)
    bad = np.argwhere(~(got == want))
    if len(bad) == 0:
        return True, None, ""
    i = tuple(bad[0])
    return False, i, ": got %r, expected %r, %d element(s) differ" % (got[i], want[i], len(bad))


def check_like(dtype):
    """tests/test_warp_gpu.py:33-40 (check): integers equal, CV_32F within 1e-6 of the norm"""
    return rel(1e-6) if np.dtype(dtype) == np.dtype(F32) else same_values


BITS = vc.exact                                 # tests/test_warp_gpu.py:43-49 (check_bits) and :466-470 (_bits): bit for bit, CV_32F included


def rot(w, h, angle=7.0, scale=0.95):
    """cv::getRotationMatrix2D about the centre, handed over as WARP_INVERSE_MAP"""
    cx, cy = float(np.float32(w / 2.0)), float(np.float32(h / 2.0))
    a = angle * np.pi / 180.0
    al, be = np.cos(a) * scale, np.sin(a) * scale
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]], np.float64)


S_MAT = np.array([[0.3, 0.1, -20.0], [-0.2, 0.4, 30.0]], np.float64)                                   # leaves the source on several sides
P_MAT = np.array([[1.05, 0.04, -6.0], [0.03, 0.95, 5.0], [1e-4, -1e-4, 1.0]], np.float64)              # tests/test_warp_gpu.py:166 (test_warp_tile_orders)
MATS = {"R": rot, "S": lambda w, h: S_MAT}


class Row:
    """one row of the table.  source(w, h) -> image; inputs(w, h) -> further read-only operands (maps); oracle(image, *inputs) -> expected array or tuple of arrays
    (one guarded destination each), with keeps=True oracle(image, *inputs, dst=previous content) and the destination is an input too; call(cv, src_view, dst_view or
    views, *input_views); kernel: a substring (or several: any of them) that mi355cv_lastKernel must hold on layout A for at least one shape"""

    def __init__(self, name, source, oracle, call, shapes=SHAPES, compare=vc.exact, kernel=None, inputs=None, keeps=False):
        self.name, self.source, self.oracle, self.call, self.shapes, self.compare, self.inputs, self.keeps = name, source, oracle, call, shapes, compare, inputs, keeps
        self.kernel = (kernel,) if isinstance(kernel, str) else kernel


ROWS = []


def row(*a, **kw):
    ROWS.append(Row(*a, **kw))


def tname(dt, cn):
    return "%s C%d" % (np.dtype(dt).name, cn)


# ---------------------------------------------------------------------------------------------------------------- resize
# linear / nearest: tests/test_warp_gpu.py:59-61 (check); area, cubic, Lanczos, the exact modes: :102, :115, :129, :342, :358, :463 (np.array_equal)
def up2(w, h):
    return 2 * w, 2 * h


def two3(w, h):
    return max(1, w * 2 // 3), max(1, h * 2 // 3)


def three2(w, h):
    return w * 3 // 2 + 1, h * 3 // 2 + 1


def half(w, h):
    return w // 2, h // 2


def resize_row(mode, interp, dt, cn, dsize, seed, shapes=SHAPES, compare=None, kernel=None):
    row("resize %s %s" % (mode, tname(dt, cn)), lambda w, h: img(dt, cn, w, h, seed), lambda a: O.orc_resize(a, dsize(a.shape[1], a.shape[0]), interpolation=interp),
        lambda cv, s, d: cv.resize(s, (d.shape[1], d.shape[0]), interpolation=interp, dst=d), shapes=shapes, compare=compare or check_like(dt), kernel=kernel)


resize_row("linear x 2", 1, U8, 1, up2, 101, kernel="k_resize8_lean")                 # (64, 19) -> (128, 38): sw * cn and dw * cn multiples of 4
resize_row("linear x 2", 1, U8, 3, up2, 102, kernel="k_resize8_lean")
resize_row("linear -> 2/3", 1, U8, 1, two3, 103)
resize_row("linear x 3/2", 1, U8, 4, three2, 104, kernel="k_resize_linC")
resize_row("linear x 3/2", 1, F32, 3, three2, 105, kernel="k_resize_linC")
resize_row("linear x 3/2", 1, F32, 1, three2, 106, kernel="k_resize_lin1")
resize_row("linear x 3/2", 1, U16, 1, three2, 107, kernel="k_resize grid")            # the generic kernel
resize_row("nearest -> 2/3", 0, F32, 1, two3, 108)
resize_row("cubic x 2", 2, U8, 1, up2, 109, compare=same_values, kernel="k_resize_tab8<4>")
resize_row("cubic x 2", 2, U8, 3, up2, 110, compare=same_values, kernel="k_resize_tab8<4>")
resize_row("cubic x 2", 2, F32, 1, up2, 111, compare=same_values)
resize_row("cubic x 2", 2, U16, 3, up2, 112, compare=same_values)
# Lanczos CV_8U: k_resize_tab8<8> is opt-in (MI355CV_RESIZE_TAB8=1, read once per process: resize.hip cubicLanczos, tab8); what serves it by default is the tiled kernel
resize_row("Lanczos x 2", 4, U8, 1, up2, 113, compare=same_values, kernel="k_resize_tiled<depth 0,8>")
resize_row("Lanczos x 2", 4, F32, 1, up2, 114, compare=same_values)
resize_row("LINEAR_EXACT x 3/2", 5, U8, 3, three2, 115, compare=same_values, kernel="k_resize_exact")
resize_row("LINEAR_EXACT x 3/2", 5, S16, 1, three2, 116, compare=same_values, kernel="k_resize_exact")
resize_row("NEAREST_EXACT x 3/2", 6, U8, 3, three2, 117, compare=same_values)
resize_row("area -> 2/3", 3, U8, 3, two3, 118, compare=same_values, kernel="k_resize_area")
resize_row("area -> 2/3", 3, F32, 1, two3, 119, compare=same_values, kernel="k_resize_area")
resize_row("area 2x2", 3, U8, 1, half, 120, shapes=EVEN, compare=same_values, kernel="k_area2x2_u8<1>")
resize_row("area 2x2", 3, U8, 4, half, 121, shapes=EVEN, compare=same_values, kernel="k_area2x2_u8<4>")
resize_row("area 2x2", 3, F32, 1, half, 122, shapes=EVEN, compare=same_values, kernel="k_area2x2_f32")


# ---------------------------------------------------------------------------------------------------------------- warpAffine
# nearest / linear: tests/test_warp_gpu.py:153 (check_bits); cubic / Lanczos: :487 (_bits); BORDER_TRANSPARENT linear: :210 (check), cubic: :487 (_bits)
def affine_row(mode, interp, dt, cn, border, mat, seed, compare=BITS, kernel=None, keeps=False):
    bname = {CONSTANT: "CONSTANT", REPLICATE: "REPLICATE", REFLECT_101: "REFLECT_101", TRANSPARENT: "TRANSPARENT"}[border]
    bval = BVAL if border == CONSTANT else 0.0

    def oracle(a, dst=None):
        h, w = a.shape[:2]
        return O.orc_warpAffine(a, MATS[mat](w, h), (w, h), interp, border, bval, dst=dst)
    row("warpAffine %s %s %s %s" % (mode, tname(dt, cn), bname, mat), lambda w, h: img(dt, cn, w, h, seed), oracle,
        lambda cv, s, d: cv.warpAffine(s, MATS[mat](s.shape[1], s.shape[0]), (d.shape[1], d.shape[0]), interp | INVERSE, border, bval, dst=d),
        compare=compare, kernel=kernel, keeps=keeps)


for _dt, _cn, _seed in [(U8, 1, 130), (U8, 3, 131)]:
    for _b in (CONSTANT, REPLICATE):
        for _m in ("R", "S"):
            affine_row("linear", 1, _dt, _cn, _b, _m, _seed, kernel=("k_warp8_lean<%d," % _cn, "k_warp8_tile<%d," % _cn))
for _dt, _cn, _seed, _k in [(U8, 4, 132, "k_warp_lin<depth 0,4,0>"), (U16, 1, 133, "k_warp grid"), (F32, 3, 134, "k_warp_lin<depth 5,3,0>")]:
    affine_row("linear", 1, _dt, _cn, CONSTANT, "R", _seed, kernel=_k)
    affine_row("linear", 1, _dt, _cn, REPLICATE, "S", _seed, kernel=_k)
affine_row("linear", 1, F32, 1, CONSTANT, "R", 135, kernel="k_warp32_strip")          # (64, 19): the strip kernel's floor is a (64, 16) destination
affine_row("linear", 1, F32, 1, CONSTANT, "S", 135, kernel="k_warp32_strip")
affine_row("linear", 1, F32, 1, REPLICATE, "R", 135, kernel="k_warp_lin<depth 5,1,0>")
affine_row("linear", 1, F32, 1, REPLICATE, "S", 135, kernel="k_warp32_tile")
affine_row("nearest", 0, U8, 1, REFLECT_101, "R", 136)
affine_row("cubic", 2, U8, 1, CONSTANT, "R", 137, kernel="k_warp8_cubic<1>")
affine_row("cubic", 2, U8, 3, REPLICATE, "R", 138, kernel="k_warp_taps_lds<4")
affine_row("cubic", 2, F32, 1, REFLECT_101, "R", 139, kernel="k_warp_taps_lds<4")
affine_row("cubic", 2, U8, 2, CONSTANT, "S", 140, kernel="k_warp_taps<4>")
affine_row("Lanczos", 4, U8, 1, REPLICATE, "R", 141, kernel="k_warp_taps_lds<8")
affine_row("Lanczos", 4, F32, 1, CONSTANT, "S", 142, kernel="k_warp_taps_lds<8")
affine_row("linear", 1, U8, 3, TRANSPARENT, "S", 143, compare=same_values, keeps=True)
affine_row("cubic", 2, F32, 1, TRANSPARENT, "S", 144, keeps=True)


# ---------------------------------------------------------------------------------------------------------------- warpPerspective
# linear: tests/test_warp_gpu.py:169 (check); cubic: :502 (_bits)
def persp_row(mode, interp, dt, cn, border, seed, compare):
    bval = 3.0 if border == CONSTANT else 0.0
    row("warpPerspective %s %s %s" % (mode, tname(dt, cn), "CONSTANT" if border == CONSTANT else "REPLICATE"), lambda w, h: img(dt, cn, w, h, seed),
        lambda a: O.orc_warpPerspective(a, P_MAT, (a.shape[1], a.shape[0]), interp, border, bval),
        lambda cv, s, d: cv.warpPerspective(s, P_MAT, (d.shape[1], d.shape[0]), interp | INVERSE, border, bval, dst=d), compare=compare)


for _dt, _cn, _seed in [(U8, 1, 150), (U8, 3, 151), (F32, 1, 152)]:
    for _b in (CONSTANT, REPLICATE):
        persp_row("linear", 1, _dt, _cn, _b, _seed, check_like(_dt))
persp_row("cubic", 2, U8, 1, CONSTANT, 153, BITS)


# ---------------------------------------------------------------------------------------------------------------- remap: source, maps and destination are all views
# linear / nearest: tests/test_warp_gpu.py:237, :318, :319, :445 (check); cubic: :527 (_bits).  Maps as in tests/test_warp_gpu.py:276 (_float_maps), of the
# destination's shape; the source is 3 columns and 2 rows larger, so no size can stand in for another
def source_shape(w, h):
    return w + 3, h + 2


@functools.lru_cache(maxsize=None)
def float_maps(w, h, seed=4):
    sw, sh = source_shape(w, h)
    rng = np.random.default_rng(seed * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    mapx = (xx * (sw / w) + rng.uniform(-3, 3, xx.shape)).astype(np.float32)
    mapy = (yy * (sh / h) - 1 + rng.uniform(-3, 3, yy.shape)).astype(np.float32)
    if h > 3 and w > 4:
        mapx[3, 4] = 17.515625; mapy[3, 4] = 8.984375                                                  # tests/test_warp_gpu.py:287: fractions that round up into the next pixel
    return mapx, mapy


@functools.lru_cache(maxsize=None)
def offset_maps(w, h):
    rng = np.random.default_rng(8000 + w)                                                              # tests/test_warp_gpu.py:437: offsets from the destination pixel
    return rng.uniform(-6, 6, (h, w)).astype(np.float32), rng.uniform(-6, 6, (h, w)).astype(np.float32)


def maps_pair(w, h):
    return list(float_maps(w, h))


def maps_relative(w, h):
    return list(offset_maps(w, h))


def maps_xy(w, h):
    return [np.ascontiguousarray(np.stack(float_maps(w, h), axis=-1))]


def maps_fixed(w, h):
    return list(O.orc_convertMaps(*float_maps(w, h), "16sc2", False))


def maps_nearest(w, h):
    return [O.orc_convertMaps(*float_maps(w, h), "16sc2", True)[0]]


def remap_row(maps_name, maps, interp, flags, border, dt, cn, seed, compare):
    bval = 9.0 if border == CONSTANT else 0.0
    bname = {CONSTANT: "CONSTANT", REPLICATE: "REPLICATE", REFLECT: "REFLECT", REFLECT_101: "REFLECT_101"}[border]

    def oracle(a, m1, m2=None):
        if m2 is not None and m1.dtype == np.float32:
            return O.orc_remap(a, m1, m2, interp | flags, border, bval)
        return O.orc_remapMaps(a, m1, m2, interp | flags, border, bval)
    row("remap %s %s %s %s" % (maps_name, {0: "nearest", 1: "linear", 2: "cubic"}[interp], bname, tname(dt, cn)), lambda w, h: img(dt, cn, *source_shape(w, h), seed),
        oracle, lambda cv, s, d, m1, m2=None: cv.remap(s, m1, m2, interp | flags, border, bval, dst=d), compare=compare, inputs=maps)


for _dt, _cn, _seed in [(U8, 3, 160), (F32, 1, 161)]:
    remap_row("32FC1 pair", maps_pair, 1, 0, CONSTANT, _dt, _cn, _seed, check_like(_dt))
    remap_row("32FC1 pair", maps_pair, 1, 0, REFLECT_101, _dt, _cn, _seed, check_like(_dt))
    remap_row("32FC1 pair", maps_pair, 2, 0, REFLECT_101, _dt, _cn, _seed, BITS)
    remap_row("32FC1 pair relative", maps_relative, 1, RELATIVE, REPLICATE, _dt, _cn, _seed, check_like(_dt))
    remap_row("32FC2", maps_xy, 1, 0, CONSTANT, _dt, _cn, _seed, check_like(_dt))
    remap_row("16SC2 + 16UC1", maps_fixed, 1, 0, REFLECT, _dt, _cn, _seed, check_like(_dt))
    remap_row("16SC2 alone", maps_nearest, 0, 0, REPLICATE, _dt, _cn, _seed, check_like(_dt))


# ---------------------------------------------------------------------------------------------------------------- convertMaps: map1 is the source, map2 an input, every
# destination guarded.  tests/test_warp_gpu.py:294, :301 (np.array_equal)
def convert_row(name, first, second, dstname, dsttype, nn=False):
    def outputs(m1, m2=None):
        return tuple(o for o in O.orc_convertMaps(m1, m2, dstname, nn) if o is not None)

    def call(cv, s, d, m2=None):
        return cv.convertMaps(s, m2, dsttype, nn, dst=d)
    row("convertMaps " + name, lambda w, h: first(w, h), outputs, call, compare=same_values, inputs=(lambda w, h: [second(w, h)]) if second else None)


convert_row("32FC1 pair -> 16SC2 + 16UC1", lambda w, h: float_maps(w, h)[0], lambda w, h: float_maps(w, h)[1], "16sc2", T16SC2)
convert_row("32FC2 -> 16SC2 + 16UC1", lambda w, h: maps_xy(w, h)[0], None, "16sc2", T16SC2)
convert_row("16SC2 + 16UC1 -> 32FC1 pair", lambda w, h: maps_fixed(w, h)[0], lambda w, h: maps_fixed(w, h)[1], "32fc1", T32FC1)
convert_row("16SC2 + 16UC1 -> 32FC2", lambda w, h: maps_fixed(w, h)[0], lambda w, h: maps_fixed(w, h)[1], "32fc2", T32FC2)
convert_row("32FC1 pair -> 16SC2 nearest", lambda w, h: float_maps(w, h)[0], lambda w, h: float_maps(w, h)[1], "16sc2", T16SC2, nn=True)


# ---------------------------------------------------------------------------------------------------------------- warpPolar
# tests/test_warp_gpu.py:330 (forward) and :373 (inverse): check
def polar_row(name, flags, dt, cn, seed):
    inverse = bool(flags & INVERSE)

    def geometry(sw, sh, dw, dh):
        w, h = (dw, dh) if inverse else (sw, sh)                                                       # the Cartesian side
        return (w / 2.0 + 0.5, h / 2.0 + 0.25), max(w, h) * 0.6

    def oracle(a):
        sh, sw = a.shape[:2]
        dw, dh = sw - 3, sh - 2
        return O.orc_warpPolar(a, (dw, dh), *geometry(sw, sh, dw, dh), flags)

    def call(cv, s, d):
        return cv.warpPolar(s, (d.shape[1], d.shape[0]), *geometry(s.shape[1], s.shape[0], d.shape[1], d.shape[0]), flags, dst=d)
    row("warpPolar %s %s" % (name, tname(dt, cn)), lambda w, h: img(dt, cn, *source_shape(w, h), seed), oracle, call, compare=check_like(dt))


for _dt, _cn, _seed in [(U8, 3, 170), (F32, 1, 171)]:
    polar_row("forward linear", 1 | 8, _dt, _cn, _seed)
    polar_row("forward semi-log", 1 | 256 | 8, _dt, _cn, _seed)
    polar_row("inverse", 1 | 16 | 8, _dt, _cn, _seed)

BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


@functools.lru_cache(maxsize=None)
def reference(name, w, h):
    """the source image, the maps and the oracle's answer, computed once per (row, shape) and shared by the six layouts (never written to).  A row whose destination
    is an input has no answer before the destination's content is known: its answer is None here"""
    r = BY_NAME[name]
    image = np.ascontiguousarray(r.source(w, h))
    inputs = [np.ascontiguousarray(m) for m in (r.inputs(w, h) if r.inputs else [])]
    want = None if r.keeps else r.oracle(image, *inputs)
    if want is not None:
        want = tuple(np.ascontiguousarray(x) for x in want) if isinstance(want, tuple) else np.ascontiguousarray(want)
    for a in [image] + inputs + list(want if isinstance(want, tuple) else [want] if want is not None else []):
        a.setflags(write=False)
        assert (a.dtype.type, a.shape[2] if a.ndim == 3 else 1) in vc.PIXELS_USED, "add %s C%d to viewcheck.PIXELS_USED" % (a.dtype, a.shape[2] if a.ndim == 3 else 1)
    return image, inputs, want


@pytest.mark.parametrize("layout", vc.LAYOUTS)
@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_warp_views(cv, name, layout):
    r = BY_NAME[name]
    reached = []
    for (w, h) in r.shapes:
        image, inputs, want = reference(name, w, h)
        what = "%s layout %s %dx%d" % (name, layout, w, h)
        kw = {}
        if r.keeps:
            want = lambda prev, image=image, inputs=inputs: r.oracle(image, *inputs, dst=prev)          # noqa: E731
            kw["dst_like"] = (image.dtype, image.shape)
        try:
            kern, _ = vc.run(marked(cv, r.call), layout, image, want, what=what, compare=r.compare, device=Device, kernel_name=last_kernel, inputs=inputs, **kw)
        except vc.Unreachable as e:
            # only F's residues can be out of a pixel size's reach, and only for 8-byte pixels (a CV_32FC2 map on the source side: no base of 4)
            assert layout == "F" and any(vc.pixel_bytes(a.dtype, a.shape[2] if a.ndim == 3 else 1) == 8 for a in [image] + inputs), (what, str(e))
            pytest.skip("layout %s: %s" % (layout, e))
        KERNELS.setdefault((name, layout), set()).add(short(kern))
        reached.append(((w, h), kern))
    if layout == "A" and r.kernel is not None:
        assert any(k in kern for _, kern in reached for k in r.kernel), (name, r.kernel, reached)        # the control must reach the kernel the row is about


# ---------------------------------------------------------------------------------------------------------------- batch entries, N = 3
# frames as views of a guarded parent in the forms of viewcheck.BATCH_FORMS_ALL; the expected frames come from the oracle, frame by frame.  'roi' and 'columns' are
# misaligned in pointer and step, so they run what a misaligned image runs.  'oddstride' has pointer and step aligned and only the frame stride off (1 or 2 modulo 4;
# built for 1- and 2-byte elements, so the CV_8U rows run it): the kernels of warp8.h read and store whole aligned dwords at addresses that include frame * stride,
# which their plans never see -- runWarp / runResize judge the strides -- and k_area2x2_u8 loads 8 bytes.  Each 'oddstride' case first runs its control,
# viewcheck.ALIGNED (the same frames without the gap), which must reach the row's fast kernel; the odd stride must then keep the batch off it
FAST = {
    "resizeBatch linear x 2 uint8 C1": ("k_resize8_lean<1,",),
    "resizeBatch area 2x2 uint8 C3": ("k_area2x2_u8<3>",),
    "warpAffineBatch linear uint8 C1": ("k_warp8_lean<1,", "k_warp8_tile<1,"),
    "warpAffineBatch linear uint8 C3": ("k_warp8_lean<3,", "k_warp8_tile<3,"),
    "warpAffineBatch cubic uint8 C1": ("k_warp8_cubic<1>",),
}
BATCH = {
    # name -> (dtype, cn, shapes, batch call(cv, frames, dst), oracle(frame), compare)
    "resizeBatch linear x 2 uint8 C1": (U8, 1, SHAPES, lambda cv, f, d: cv.resizeBatch(f, (d.shape[2], d.shape[1]), interpolation=1, dst=d),
                                        lambda a: O.orc_resize(a, up2(a.shape[1], a.shape[0]), interpolation=1), same_values),
    "resizeBatch area 2x2 uint8 C3": (U8, 3, EVEN, lambda cv, f, d: cv.resizeBatch(f, (d.shape[2], d.shape[1]), interpolation=3, dst=d),
                                      lambda a: O.orc_resize(a, half(a.shape[1], a.shape[0]), interpolation=3), same_values),
    "resizeBatch area 2x2 float32 C1": (F32, 1, EVEN, lambda cv, f, d: cv.resizeBatch(f, (d.shape[2], d.shape[1]), interpolation=3, dst=d),
                                        lambda a: O.orc_resize(a, half(a.shape[1], a.shape[0]), interpolation=3), same_values),
    "resizeBatch LINEAR_EXACT x 3/2 uint8 C1": (U8, 1, SHAPES, lambda cv, f, d: cv.resizeBatch(f, (d.shape[2], d.shape[1]), interpolation=5, dst=d),
                                                lambda a: O.orc_resize(a, three2(a.shape[1], a.shape[0]), interpolation=5), same_values),
    "warpAffineBatch linear uint8 C1": (U8, 1, SHAPES, lambda cv, f, d: cv.warpAffineBatch(f, rot(d.shape[2], d.shape[1]), (d.shape[2], d.shape[1]), 1 | INVERSE, CONSTANT, BVAL, dst=d),
                                        lambda a: O.orc_warpAffine(a, rot(a.shape[1], a.shape[0]), (a.shape[1], a.shape[0]), 1, CONSTANT, BVAL), BITS),
    "warpAffineBatch linear uint8 C3": (U8, 3, SHAPES, lambda cv, f, d: cv.warpAffineBatch(f, S_MAT, (d.shape[2], d.shape[1]), 1 | INVERSE, REPLICATE, 0.0, dst=d),
                                        lambda a: O.orc_warpAffine(a, S_MAT, (a.shape[1], a.shape[0]), 1, REPLICATE, 0.0), BITS),
    "warpAffineBatch linear float32 C1 CONSTANT": (F32, 1, SHAPES,
                                                   lambda cv, f, d: cv.warpAffineBatch(f, rot(d.shape[2], d.shape[1]), (d.shape[2], d.shape[1]), 1 | INVERSE, CONSTANT, BVAL, dst=d),
                                                   lambda a: O.orc_warpAffine(a, rot(a.shape[1], a.shape[0]), (a.shape[1], a.shape[0]), 1, CONSTANT, BVAL), BITS),
    "warpAffineBatch cubic uint8 C1": (U8, 1, SHAPES, lambda cv, f, d: cv.warpAffineBatch(f, rot(d.shape[2], d.shape[1]), (d.shape[2], d.shape[1]), 2 | INVERSE, CONSTANT, BVAL, dst=d),
                                       lambda a: O.orc_warpAffine(a, rot(a.shape[1], a.shape[0]), (a.shape[1], a.shape[0]), 2, CONSTANT, BVAL), BITS),
    "warpPerspectiveBatch linear uint8 C1": (U8, 1, SHAPES, lambda cv, f, d: cv.warpPerspectiveBatch(f, P_MAT, (d.shape[2], d.shape[1]), 1 | INVERSE, CONSTANT, 3.0, dst=d),
                                             lambda a: O.orc_warpPerspective(a, P_MAT, (a.shape[1], a.shape[0]), 1, CONSTANT, 3.0), same_values),
    "warpPerspectiveBatch linear float32 C1": (F32, 1, SHAPES, lambda cv, f, d: cv.warpPerspectiveBatch(f, P_MAT, (d.shape[2], d.shape[1]), 1 | INVERSE, REPLICATE, 0.0, dst=d),
                                               lambda a: O.orc_warpPerspective(a, P_MAT, (a.shape[1], a.shape[0]), 1, REPLICATE, 0.0), rel(1e-6)),
}
BATCH_CASES = [(name, form) for name in sorted(BATCH) for form in vc.BATCH_FORMS_ALL if form != vc.ODDSTRIDE or BATCH[name][0] == U8]


@functools.lru_cache(maxsize=None)
def batch_reference(name, w, h):
    dt, cn, _, _, oracle, _ = BATCH[name]
    frames = np.stack([img(dt, cn, w, h, 180 + f) for f in range(3)])
    want = np.stack([oracle(f) for f in frames])
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, want


@pytest.mark.parametrize("name,form", BATCH_CASES)
def test_warp_batch_views(cv, name, form):
    """every frame equals the oracle's result for the contiguous frame, the guards (the gaps between the frames of 'oddstride' included) survive, and an odd frame
    stride keeps the batch off the kernels of warp8.h"""
    _, _, shapes, call, _, compare = BATCH[name]
    reached = []
    for (w, h) in shapes:
        frames, want = batch_reference(name, w, h)
        for f in ((vc.ALIGNED, form) if form == vc.ODDSTRIDE else (form,)):
            kern, _ = vc.run_batch(marked(cv, call), f, frames, want, what="%s %dx%d" % (name, w, h), compare=compare, device=Device, kernel_name=last_kernel)
            KERNELS.setdefault((name, f), set()).add(short(kern))
            if f == vc.ALIGNED:
                reached.append(((w, h), kern))
            if f == vc.ODDSTRIDE:
                assert not any(k in kern for k in WARP8 + FAST.get(name, ())), (name, (w, h), kern)
    if form == vc.ODDSTRIDE and name in FAST:
        assert any(k in kern for _, kern in reached for k in FAST[name]), (name, FAST[name], reached)     # the control must reach the kernel the odd stride keeps away
