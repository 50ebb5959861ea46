"""Bilinear Bayer demosaicing (cv::demosaicing / the Bayer codes of cv::cvtColor: imgproc/src/demosaicing.cpp, Bayer2RGB_ / Bayer2Gray_) restated in numpy,
the reference of tests/test_demosaic_cpu.py and tests/test_demosaic_gpu.py.  Imports nothing from the product.

Pattern (named after the colours of row 1, columns 1 and 2), sites relative to the origin of the image handed in:
    BG: R G / G B      GB: G R / B G      RG: B G / G R      GR: G B / R G
Interior pixels (1 <= y <= h-2, 1 <= x <= w-2), c the centre, H = left + right, V = up + down, D = the four diagonals, exact integers:
    R / B site: own = c, green = (H + V + 2) >> 2, opposite = (D + 2) >> 2
    G site:     green = c, the colour of its row neighbours = (H + 1) >> 1, the colour of its column neighbours = (V + 1) >> 1
    gray, K_B = 1868, K_G = 9617, K_R = 4899:
    R / B site: (4 c K_own + D K_opposite + (H + V) K_G + 2^15) >> 16        G site: (H K_row + V K_column + 2 c K_G + 2^14) >> 15
Border, after the interior: rows 1 .. h-2: column 0 := column 1, column w-1 := column w-2; then row 0 := row 1, row h-1 := row h-2.
Channel order B, G, R (R, G, B with rgb=True); a fourth channel is the depth's maximum."""
import numpy as np

B, G, R = 0, 1, 2
PATTERNS = ("BG", "GB", "RG", "GR")                        # the C ABI's pattern numbers 0 .. 3
SITES = {"BG": ((R, G), (G, B)), "GB": ((G, R), (B, G)), "RG": ((B, G), (G, R)), "GR": ((G, B), (R, G))}
K = np.array([1868, 9617, 4899], np.int64)                 # indexed by colour

# the reference's conversion codes (imgproc.hpp): family -> (BG, GB, RG, GR)
CODES_BGR = (46, 47, 48, 49)
CODES_GRAY = (86, 87, 88, 89)
CODES_BGRA = (139, 140, 141, 142)
CODES_VNG = (62, 63, 64, 65)
CODES_EA = (135, 136, 137, 138)
RGB_OF = {"BG": "RG", "GB": "GR", "RG": "BG", "GR": "GB"}  # COLOR_Bayer<p>2RGB == COLOR_Bayer<RGB_OF[p]>2BGR


def demosaic(src, pattern, dcn, rgb=False):
    """src: [H,W] uint8 / uint16, H, W >= 3; pattern: one of PATTERNS; dcn 1 (gray), 3 or 4 -> [H,W] or [H,W,dcn] of the same type"""
    assert src.ndim == 2 and src.dtype in (np.uint8, np.uint16) and dcn in (1, 3, 4)
    h, w = src.shape
    assert h >= 3 and w >= 3
    a = src.astype(np.int64)
    c = a[1:-1, 1:-1]
    H = a[1:-1, :-2] + a[1:-1, 2:]
    V = a[:-2, 1:-1] + a[2:, 1:-1]
    D = a[:-2, :-2] + a[:-2, 2:] + a[2:, :-2] + a[2:, 2:]
    yy, xx = np.mgrid[1:h - 1, 1:w - 1]
    t = np.array(SITES[pattern])
    site, rowc, colc = t[yy & 1, xx & 1], t[yy & 1, (xx & 1) ^ 1], t[(yy & 1) ^ 1, xx & 1]
    green = site == G
    if dcn == 1:
        at_g = (H * K[np.where(green, rowc, 0)] + V * K[np.where(green, colc, 0)] + 2 * c * K[G] + (1 << 14)) >> 15
        own = np.where(green, R, site)
        at_rb = (4 * c * K[own] + D * K[2 - own] + (H + V) * K[G] + (1 << 15)) >> 16
        inner = np.where(green, at_g, at_rb)
    else:
        planes = []
        for col in ((R, G, B) if rgb else (B, G, R)):
            at_g = c if col == G else np.where(rowc == col, (H + 1) >> 1, (V + 1) >> 1)
            at_rb = (H + V + 2) >> 2 if col == G else np.where(site == col, c, (D + 2) >> 2)
            planes.append(np.where(green, at_g, at_rb))
        if dcn == 4:
            planes.append(np.full_like(c, np.iinfo(src.dtype).max))
        inner = np.stack(planes, axis=-1)
    out = np.zeros((h, w) + inner.shape[2:], np.int64)
    out[1:-1, 1:-1] = inner
    out[1:-1, 0] = out[1:-1, 1]
    out[1:-1, -1] = out[1:-1, -2]
    out[0] = out[1]
    out[-1] = out[-2]
    assert out.min() >= 0 and out.max() <= np.iinfo(src.dtype).max
    return out.astype(src.dtype)


# ---- known answers, computed by hand from the definition above; shared by the CPU and the GPU tests
def spike():
    a = np.zeros((5, 5), np.uint8)
    a[2, 2] = 255
    return a


def cross(centre, edge, corner):
    """the 5 x 5 answer to spike(): 3 x 3 interior, then the border copy"""
    inner = np.array([[corner, edge, corner], [edge, centre, edge], [corner, edge, corner]])
    return np.pad(inner, 1, mode="edge")


def checker():
    yy, xx = np.mgrid[0:4, 0:4]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


def wide():
    c = np.zeros((4, 4), np.uint16)
    c[1, 1] = c[1, 2] = 65535
    c[2, 1] = 1
    return c


def known_answers(f):
    """the answers the definition gives, computed by hand from it; f(src, pattern name, dcn, rgb=False) -> image"""
    a = spike()
    got = f(a, "BG", 3)
    assert not got[..., 0].any() and not got[..., 1].any()
    assert got[..., 2].tolist() == [[64, 64, 128, 64, 64], [64, 64, 128, 64, 64], [128, 128, 255, 128, 128], [64, 64, 128, 64, 64], [64, 64, 128, 64, 64]]
    assert np.array_equal(f(a, "BG", 1), cross(76, 38, 19))
    assert np.array_equal(f(a, "RG", 1), cross(29, 15, 7))
    assert np.array_equal(f(a, "GB", 1), cross(150, 37, 0)) and np.array_equal(f(a, "GR", 1), cross(150, 37, 0))
    cb = checker()
    for p, bgr, gray in (("BG", (0, 255, 0), 150), ("RG", (0, 255, 0), 150), ("GB", (255, 0, 255), 105), ("GR", (255, 0, 255), 105)):
        got = f(cb, p, 3)
        assert tuple(got[1, 1]) == bgr and tuple(got[1, 2]) == bgr, p
        g1 = f(cb, p, 1)
        assert g1[1, 1] == gray and g1[1, 2] == gray, p
    c = wide()
    assert f(c, "BG", 3)[1:3, 1:3].tolist() == [[[65535, 16384, 0], [32768, 65535, 0]], [[32768, 1, 0], [16384, 16384, 0]]]
    assert f(c, "BG", 1)[1:3, 1:3].tolist() == [[17089, 42203], [3737, 11485]]
    for dt in (np.uint8, np.uint16):                                         # the overflow check of the gray sum
        top = np.iinfo(dt).max
        m = np.full((4, 6), top, dt)
        for p in PATTERNS:
            assert np.all(f(m, p, 1) == top) and np.all(f(m, p, 3) == top) and np.all(f(m, p, 4) == top), (dt, p)
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (6, 7), dtype=np.uint8)
    for p in PATTERNS:
        assert np.array_equal(f(x, p, 3, rgb=True), f(x, RGB_OF[p], 3)), p
        assert np.array_equal(f(x, p, 4, rgb=True), f(x, RGB_OF[p], 4)), p
        assert np.array_equal(f(x, p, 3, rgb=True), f(x, p, 3)[..., ::-1]), p
        assert np.array_equal(f(x, p, 4)[..., :3], f(x, p, 3)) and np.all(f(x, p, 4)[..., 3] == 255), p
