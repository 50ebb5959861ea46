"""k_warp32_strip (opencv_amd/csrc/warp.hip): the strip walk that serves every gentle CV_32FC1 bilinear warpAffine with BORDER_CONSTANT, and k_warp32_strip_rest, which
redoes the lanes it defers.  The kernel keeps the reference's order of float operations (remapBilinear), so every comparison here is BIT FOR BIT against the restatement
that tests/test_oracle_warp.py pins to the reference -- no tolerance anywhere; where the source holds NaN the NaN positions must agree (the payload of a NaN a blend
produces is the processor's) and every other pixel's bits.  After every call that must land on the strip kernel its name is asserted (mi355cv_lastKernel), so the file keeps
testing the kernel it is named after when the dispatch rule moves.

The dispatch rule (runWarp, M = the dst -> src matrix): bilinear, CV_32FC1, BORDER_CONSTANT, M4 > 0.25, sw % 4 == 0, sw >= 3, sh >= 2, dw >= 64, dh >= 16, all pointers /
steps / frame strides 16-byte aligned, |M3| 255 + 16 M4 + 4 <= 62, |M0 - M1 M3 / M4| 255 + 2 |M1 / M4| + 8 <= 288, |M1 / M4| < 0.5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP = "k_warp32_strip"


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    return opencv_amd


def dev(a):
    return torch.from_numpy(a).cuda()


def last():
    from opencv_amd import _lib
    return _lib.lib.mi355cv_lastKernel().decode()


def forget(cv):
    """mi355cv_lastKernel keeps the last name NOTED, and the plain bilinear kernels note none: put another kernel's name there before a call whose kernel is asserted"""
    cv.resize(torch.zeros((64, 64), dtype=torch.uint8, device="cuda"), (128, 128), interpolation=1)
    assert STRIP not in last() and last() != "", last()


def pitched(dw, dh, fill=None):
    """a dw x dh destination whose rows start at multiples of 16 bytes whatever dw is (a window of a tensor with a pitch of whole float4s): what the strip kernel takes"""
    canvas = torch.empty((dh, (dw + 3) // 4 * 4), dtype=torch.float32, device="cuda")
    if fill is not None:
        canvas.fill_(fill)
    return canvas[:, :dw]


def image(w, h, seed):
    """values in [0.5, 1.5): no pixel and no blend of pixels equals one of the border values used here"""
    return np.random.default_rng(seed).random((h, w), dtype=np.float32) + np.float32(0.5)


def rot(deg, cx, cy, shift=(0.0, 0.0), scale=1.0):
    """dst -> src: a rotation by `deg` about (cx, cy), then a shift of the source position"""
    a = np.deg2rad(deg)
    al, be = np.cos(a) * scale, np.sin(a) * scale
    return np.array([[al, be, (1 - al) * cx - be * cy + shift[0]], [-be, al, be * cx + (1 - al) * cy + shift[1]]], np.float64)


def bits(got, want, info=None):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, info
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (info, "NaN positions")
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    diff = (g.view(np.uint32) != w.view(np.uint32)) & ~nan
    if diff.any():
        ys, xs = np.nonzero(diff)
        raise AssertionError("%d pixels differ, first (x %d, y %d): got %r want %r; %r" % (diff.sum(), xs[0], ys[0], g[ys[0], xs[0]], w[ys[0], xs[0]], info))


def case(cv, orc, src, M, dsize, bval=0.0, strip=True, d_src=None):
    """warpAffine against the restatement; strip: True -- the strip kernel must have served it, False -- it must not, None -- whatever serves it"""
    want = orc.orc_warpAffine(src, M, dsize, 1, 0, bval)
    forget(cv)
    got = cv.warpAffine(dev(src) if d_src is None else d_src, M, dsize, 1 | cv.WARP_INVERSE_MAP, 0, bval, dst=pitched(dsize[0], dsize[1]))
    k = last()
    info = (M.tolist(), src.shape, dsize, bval, k)
    if strip is not None:
        assert (STRIP in k) == strip, info
    bits(got, want, info)
    return want


# ---- 1. the border value ------------------------------------------------------------------------------------------------------------------------------------------
BORDER_MAPS = [(rot(5.0, 128.0, 64.0, (-30.0, -25.0)), (330, 200)), (rot(-9.0, 128.0, 64.0, (-100.0, -40.0)), (521, 187)),
               (np.array([[1.0, 0.0, -17.3], [0.0, 1.0, -9.6]]), (300, 160))]


def straddling(want, cval):
    """(pixels, lanes): the 4-column lanes (columns 4 k .. 4 k + 3; strips start at multiples of 256) that hold both pixels equal to the border value and pixels that are
    not, and the border-valued pixels inside them -- the pixels a lane-granular border test gets wrong"""
    h, w = want.shape
    pad = (-w) % 4
    eq = want == np.float32(cval)
    e = np.pad(eq, ((0, 0), (0, pad)), constant_values=False).reshape(h, -1, 4)
    real = np.pad(np.ones_like(eq), ((0, 0), (0, pad)), constant_values=False).reshape(h, -1, 4)
    n_eq, n_real = e.sum(2), real.sum(2)
    mixed = (n_eq > 0) & (n_eq < n_real)
    return int(n_eq[mixed].sum()), int(mixed.sum())


@pytest.mark.parametrize("bval", [0.1, 123.456, -7.3, 0.0])
def test_border_value_is_stored_exactly(cv, orc, bval):
    """a pixel whose 2 x 2 footprint is wholly outside the source is the border value itself (remapBilinear), also where the other pixels of its lane are not: blended from
    border-filled taps, cval w0 + cval w1 + cval w2 + cval w3 is one or two ulp off for most weight pairs unless cval has few mantissa bits (0, 1, 255.5: the values
    that cannot see it).  Maps that leave the source on every side and at the corners."""
    src = image(256, 128, 11)
    for M, dsize in BORDER_MAPS:
        want = case(cv, orc, src, M, dsize, bval)
        pixels, lanes = straddling(want, bval)
        assert pixels >= 200, (pixels, lanes, dsize)
        for side in (want[0], want[-1], want[:, 0], want[:, -1]):                      # the source is left on all four sides
            assert np.all(side == np.float32(bval))


# ---- 2. both signs, the edge of acceptance ------------------------------------------------------------------------------------------------------------------------
def edge_maps():
    """(name, M, source size, dsize, strip kernel?)"""
    out = []
    for deg in (3, -3, 7, -7, 9, -9):                              # the row rule: 255 sin + 16 cos + 4 = 59.7 at 9 degrees, 64.0 at 10
        out.append(("rot%+d" % deg, rot(deg, 150.0, 100.0, (-22.0, -31.0)), (256, 160), (300, 200), True))
    for deg in (11, -11, 33):
        out.append(("rot%+d" % deg, rot(deg, 150.0, 100.0, (-22.0, -31.0)), (256, 160), (300, 200), False))
    A = lambda m0, m1, m2, m3, m4, m5: np.array([[m0, m1, m2], [m3, m4, m5]], np.float64)       # noqa: E731
    out += [("M4=3.5", A(1, 0, -13.25, 0, 3.5, -40.5), (256, 512), (300, 170), True),            # vertical minification: 16 * 3.5 + 4 = 60 rows
            ("M4=0.26", A(1, 0, -13.25, 0, 0.26, -4.4), (256, 64), (300, 280), True),
            ("g=1.09", A(1.09, 0, -20.5, 0, 1, -7.75), (320, 96), (300, 120), True),             # 1.09 * 255 + 8 = 286 columns of 288
            ("g=-1.09", A(-1.09, 0, 300.5, 0, 1, -7.75), (320, 96), (300, 120), True),
            ("g=0.3", A(0.3, 0, -9.5, 0, 1, -7.75), (64, 96), (300, 120), True),
            ("shear+0.49", A(1, 0.49, -60.25, 0, 1, -9.5), (256, 96), (330, 120), True),
            ("shear-0.49", A(1, -0.49, 10.25, 0, 1, -9.5), (256, 96), (330, 120), True),
            ("M1>0,M3>0", A(1, 0.12, -25.5, 0.13, 1, -40.25), (256, 128), (300, 160), True),      # (a rotation has M1 = -M3: these two do not)
            ("M1<0,M3<0", A(1, -0.12, 5.5, -0.13, 1, 20.25), (256, 128), (300, 160), True),
            ("M1>0,M3<0,M4=2", A(0.9, 0.3, -25.5, -0.1, 2.0, 10.25), (256, 320), (300, 160), True),
            ("M1<0,M3>0,M4=0.5", A(0.9, -0.2, 15.5, 0.15, 0.5, -30.25), (256, 128), (300, 160), True)]
    return out


@pytest.mark.parametrize("name,M,ssize,dsize,strip", edge_maps(), ids=[m[0] for m in edge_maps()])
def test_both_signs_and_the_edge_of_acceptance(cv, orc, name, M, ssize, dsize, strip):
    """rotations of both signs up to the last the ring holds (9 degrees) and the first it does not; anisotropic maps at the limits of every term of the rule; M1 and M3 of
    either sign -- with M3 < 0 the strip's last column reads the LOWEST source row (cYmin / cYmax swap)"""
    src = image(ssize[0], ssize[1], 21)
    case(cv, orc, src, M, dsize, 0.25, strip)


# ---- 3. geometry --------------------------------------------------------------------------------------------------------------------------------------------------
def test_destination_widths_and_heights(cv, orc):
    """ragged last lane and its scalar tail store, one to five strips; a partial last 8-row step, one, two and three segments of rows (pixels on both sides of every seam
    are in the comparison)"""
    src = image(256, 128, 31)
    for dw in (64, 67, 255, 256, 257, 600, 1030):
        case(cv, orc, src, rot(7.0, dw / 2.0, 12.0, (128.0 - dw / 2.0, 50.0)), (dw, 23), 0.1)
    src = image(256, 512, 32)
    for dh in (16, 17, 23, 280, 420, 700):
        case(cv, orc, src, rot(-7.0, 128.0, dh / 2.0, (0.0, 256.0 - dh / 2.0)), (257, dh), 0.1)
        if dh >= 280:
            k = last()
            assert "grid=2x%dx1 " % {280: 1, 420: 2, 700: 3}[dh] in k, k                # strips x segments x frames


def test_source_sizes(cv, orc):
    """sources from one 16-byte chunk per row to several pieces, one to three rows (everything else is border), much larger and much smaller than the destination"""
    for sw in (4, 8, 64, 256, 2048):
        for sh in (1, 2, 3, 128):
            src = image(sw, sh, 40 + sw + sh)
            M = rot(5.0, 100.0, 20.0, (min(sw, 200) / 2.0 - 100.0, min(sh, 40) / 2.0 - 20.0))
            # (one source row: no bilinear kernel takes it, the generic sampler serves it)
            case(cv, orc, src, M, (200, 40), 0.1, strip=True if sh >= 2 else None)
    big = image(2048, 128, 45)
    case(cv, orc, big, rot(-5.0, 32.0, 8.0, (1500.0, 60.0)), (64, 16), 0.1)            # a small window of a large source
    case(cv, orc, big, np.array([[1.0, 0.0, 1900.25], [0.0, 1.0, 100.5]]), (300, 64), 0.1)     # its bottom right corner
    small = image(8, 3, 46)
    case(cv, orc, small, rot(9.0, 300.0, 150.0, (-296.0, -148.5)), (600, 300), -7.3)   # the whole source inside one row piece, everything else border


# ---- 4. windows into larger buffers -------------------------------------------------------------------------------------------------------------------------------
def test_windows_into_larger_buffers(cv, orc):
    """the source is a window of a parent whose other pixels are NaN: a read across the window's rim surfaces in the result; the destination is a window of a tensor
    filled with a sentinel, which must be intact around it.  A source window at a column that is not a multiple of 4 is another kernel's: same bits."""
    rng = np.random.default_rng(51)
    parent = np.full((150, 288), np.nan, np.float32)
    y0, x0, h, w = 9, 12, 128, 256
    parent[y0:y0 + h, x0:x0 + w] = rng.random((h, w), dtype=np.float32) + np.float32(0.5)
    src = np.ascontiguousarray(parent[y0:y0 + h, x0:x0 + w])
    dparent = dev(parent)
    SENT = np.float32(-4242.5)
    for M, dsize in BORDER_MAPS[:2] + [(rot(7.0, 128.0, 64.0), (256, 128))]:
        want = orc.orc_warpAffine(src, M, dsize, 1, 0, 0.1)
        assert not np.isnan(want).any()
        forget(cv)
        got = cv.warpAffine(dparent[y0:y0 + h, x0:x0 + w], M, dsize, 1 | cv.WARP_INVERSE_MAP, 0, 0.1, dst=pitched(dsize[0], dsize[1]))
        assert STRIP in last(), last()
        bits(got, want, (dsize, last()))
        # destination window: column and pitch multiples of 4 floats
        dw, dh = dsize
        canvas = torch.full((dh + 11, (dw + 3) // 4 * 4 + 24), float(SENT), dtype=torch.float32, device="cuda")
        view = canvas[5:5 + dh, 8:8 + dw]
        forget(cv)
        cv.warpAffine(dparent[y0:y0 + h, x0:x0 + w], M, dsize, 1 | cv.WARP_INVERSE_MAP, 0, 0.1, dst=view)
        assert STRIP in last(), last()
        c = canvas.cpu().numpy()
        bits(c[5:5 + dh, 8:8 + dw], want, (dsize, "dst window", last()))
        c[5:5 + dh, 8:8 + dw] = SENT
        assert np.all(c == SENT), "pixels outside the destination window were written"
    # misaligned source window (x0 = 1)
    parent2 = np.full((150, 288), np.nan, np.float32)
    parent2[y0:y0 + h, 1:1 + w] = src
    M, dsize = BORDER_MAPS[0]
    forget(cv)
    got = cv.warpAffine(dev(parent2)[y0:y0 + h, 1:1 + w], M, dsize, 1 | cv.WARP_INVERSE_MAP, 0, 0.1, dst=pitched(dsize[0], dsize[1]))
    assert STRIP not in last(), last()
    bits(got, orc.orc_warpAffine(src, M, dsize, 1, 0, 0.1), last())


# ---- 5. batches ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_batches(cv, orc):
    """one launch over three different frames; frames that are windows of larger frames (frame stride != rows x pitch), NaN around them"""
    frames = np.stack([image(256, 128, 60 + i) for i in range(3)])
    M, dsize = BORDER_MAPS[1]
    def frames_out(dw, dh):
        return torch.empty((3, dh, (dw + 3) // 4 * 4), dtype=torch.float32, device="cuda")[:, :, :dw]
    forget(cv)
    out = cv.warpAffineBatch(dev(frames), M, dsize, 1 | cv.WARP_INVERSE_MAP, 0, 123.456, dst=frames_out(*dsize))
    assert STRIP in last(), last()
    for i in range(3):
        bits(out[i], orc.orc_warpAffine(frames[i], M, dsize, 1, 0, 123.456), (i, last()))
    big = np.full((3, 150, 288), np.nan, np.float32)
    big[:, 9:137, 12:268] = frames
    M, dsize = BORDER_MAPS[0]
    forget(cv)
    out = cv.warpAffineBatch(dev(big)[:, 9:137, 12:268], M, dsize, 1 | cv.WARP_INVERSE_MAP, 0, -7.3, dst=frames_out(*dsize))
    assert STRIP in last(), last()
    for i in range(3):
        bits(out[i], orc.orc_warpAffine(frames[i], M, dsize, 1, 0, -7.3), (i, "windows", last()))


# ---- 6. special values --------------------------------------------------------------------------------------------------------------------------------------------
def test_special_values(cv, orc):
    """+-Inf, NaN, denormals, -0.0 and the largest finite values scattered over the source, its first / last rows and columns among them.  A tap of weight 0 on an Inf is a
    NaN in the reference too: the NaN positions must agree, and the bits everywhere else (-0.0 and denormals included: nothing is flushed)."""
    rng = np.random.default_rng(71)
    src = image(256, 128, 70)
    specials = np.array([np.inf, -np.inf, np.nan, 1e-40, -1e-42, -0.0, 3.4e38, -3.4e38, 1.17549435e-38], np.float32)
    ys, xs = rng.integers(0, 128, 300), rng.integers(0, 256, 300)
    src[ys, xs] = specials[rng.integers(0, len(specials), 300)]
    for k, v in enumerate(specials):                                                 # ... and on the rim
        src[0, 10 + 9 * k] = v; src[127, 13 + 9 * k] = v; src[5 + 9 * k, 0] = v; src[7 + 9 * k, 255] = v
    src[0, 0] = np.inf; src[127, 255] = np.nan; src[0, 255] = -0.0; src[127, 0] = 1e-40
    nans = 0
    for M, dsize in BORDER_MAPS + [(np.array([[1.0, 0.0, -8.0], [0.0, 1.0, -6.0]]), (280, 144))]:      # (the last: whole-pixel shift, weights of exactly 0 on every second tap)
        want = case(cv, orc, src, M, dsize, 0.1)
        nans += int(np.isnan(want).sum())
    assert nans > 100, nans
    # a source of -0.0 and denormals only: the sign of zero and the denormal bits survive the blend
    tiny = np.where(rng.random((128, 256)) < 0.5, np.float32(-0.0), np.float32(1e-41)).astype(np.float32)
    want = case(cv, orc, tiny, BORDER_MAPS[2][0], BORDER_MAPS[2][1], -0.0)
    assert np.signbit(want).any() and (np.abs(want[want != 0]) < 1e-38).any()


# ---- 7. the deferred lanes ----------------------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import opencv_amd as cv
import orc
import test_warp32_strip_gpu as T
res = {}
for name, M, ssize, dsize, strip in T.edge_maps():
    if not strip:
        continue
    src = T.image(ssize[0], ssize[1], 21)
    dst = T.pitched(dsize[0], dsize[1], -4242.5)
    T.forget(cv)
    cv.warpAffine(T.dev(src), M, dsize, 1 | cv.WARP_INVERSE_MAP, 0, 0.25, dst=dst)
    on_strip = T.STRIP in T.last()
    left = int((dst == -4242.5).sum().item())
    exact = None
    if not left:
        try:
            T.bits(dst, orc.orc_warpAffine(src, M, dsize, 1, 0, 0.25)); exact = True
        except AssertionError as e:
            exact = str(e)[:300]
    res[name] = [left, on_strip, exact]
print("RESULT " + json.dumps(res))
"""


def _child(dbg):
    env = dict(os.environ, MI355CV_WARP32_DBG=str(dbg))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert all(v[1] for v in res.values()), res                                      # every one of the maps ran on the strip kernel
    return res


def test_deferred_lanes_take_the_second_kernel(cv, orc):
    """Lanes whose taps are not all in the ring (a row not resident, a column outside its row's piece) are left out by the walk, flagged per row piece and redone by
    k_warp32_strip_rest.  The switches of MI355CV_WARP32_DBG are read once per process, so each setting runs in a fresh child over the maps of edge_maps() that the strip
    kernel takes, into sentinel-filled destinations:
      8 (no flag is written: a deferred lane is never stored) -- NO map leaves a sentinel pixel.  Inside the dispatch rule nothing defers: its bounds (62 of the ring's
        64 rows, |g| 255 + 2 |h| + 8 of the piece's 288 columns) are the walk's own worst case plus slack, and a search over matrices on the rule's limits, replaying the
        lane test with the kernel's integer terms and piece origins on the CPU, found no lane that misses its piece either.  Asserted as such: if a change to the rule or
        to the walk makes lanes defer on ordinary maps (each costs a second pass), this says so.
      1 (no row pieces are requested after a segment's prologue: every lane below the prologue's rows misses its rows) -- the deferral path for real: with 1 | 8 sentinel
        pixels must survive in every map taller than the prologue, with 1 alone k_warp32_strip_rest redoes them and every map is complete and bit for bit."""
    quiet = _child(8)
    print("DBG=8, pixels never stored:", {k: v[0] for k, v in quiet.items()})
    assert all(v[0] == 0 and v[2] is True for v in quiet.values()), quiet
    lost = _child(9)
    print("DBG=9, pixels never stored:", {k: v[0] for k, v in lost.items()})
    assert all(v[0] > 0 for v in lost.values()), lost
    redone = _child(1)
    assert all(v[0] == 0 and v[2] is True for v in redone.values()), redone
