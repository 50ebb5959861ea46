"""The host half of k_sepmx on the CPU (tests/hostemu/sepmx_emu.cpp over opencv_amd/csrc/sepmx_body.h): the plan, the border-folded Toeplitz operand tables with their
second product for weights beyond int8, the column matrix, the bias algebra and the finishes -- evaluated as plain integer matrix products over the SAME tables the product
uploads -- against the restatement of fixedSmoothInvoker / boxFilter that tests/test_oracle_smooth.py and test_oracle_filter.py pin to the reference.  Bit for bit; columns
outside the image hold garbage in the replay (their weight must be zero).  The matrix instruction's lane map itself is pinned by tests/test_sepmx_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

import emubuild
import orc as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    lib = emubuild.load("sepmx_emu.cpp", "libsepmx_emu.so", ["-ffp-contract=off"])
    lib.emu_sepmx.restype = ctypes.c_int
    return lib


def run(emu, view, parent_shape, off, border, kx, ax, ky, ay, box=(0, 0, 0, 0.0, 0.0), addr=0x7f0000000000):
    h, w = view.shape[:2]
    cn = 1 if view.ndim == 2 else view.shape[2]
    dst = np.full(view.shape, 0x5A, np.uint8)
    kx = np.ascontiguousarray(kx, np.uint16); ky = np.ascontiguousarray(ky, np.uint16)
    info = (ctypes.c_int * 6)()
    rc = emu.emu_sepmx(ctypes.c_void_p(view.ctypes.data), ctypes.c_size_t(view.strides[0]), o.P(dst), ctypes.c_size_t(dst.strides[0]), w, h, cn, parent_shape[1], parent_shape[0],
                       off[0], off[1], border, o.P(kx), len(kx), ax, o.P(ky), len(ky), ay, box[0], box[1], box[2], ctypes.c_float(box[3]), ctypes.c_double(box[4]),
                       ctypes.c_ulonglong(addr), info)
    return rc, dst, list(info)


def gauss(n, sigma):
    return [int(v) for v in o.orc_getGaussianKernelQ(n, sigma)]


@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_sepmx_host_half_gaussian(emu, cn):
    rng = np.random.default_rng(200 + cn)
    seen = set()
    for (w, h) in [(300, 40), (256 // cn, 33), (37, 5), (19, 70), (600 // cn, 9)]:
        src = rng.integers(0, 256, (h, w, cn) if cn > 1 else (h, w), dtype=np.uint8)
        for (kw, kh, sigma) in [(19, 19, 3.0), (7, 33, 2.5), (33, 9, 5.0), (65, 11, 11.0)]:
            if (kw - 1) * cn > 384:
                continue
            kx, ky = gauss(kw, sigma), gauss(kh, sigma)
            for border in (0, 1, 2, 3, 4):
                for addr in (0x7f0000000000, 0x7f0000000005):
                    rc, got, info = run(emu, src, src.shape[:2], (0, 0), border, kx, kw // 2, ky, kh // 2, addr=addr)
                    if rc == 2:
                        assert border == 3 or w < kw, (w, h, cn, kw, border)          # only BORDER_WRAP on wide rows / reflections in rows narrower than the kernel leave the window
                        continue
                    assert rc == 0, (rc, w, h, cn, kw, kh, border)
                    assert np.array_equal(got, o.orc_sepSmoothFixedU8(src, kx, ky, border)), (w, h, cn, kw, kh, border, info)
                    seen.add((info[0], info[1], info[4]))
    assert len(seen) >= 3, seen
    # what the matrix form must decline: a tap above 127, taps that sum beyond 256, rows of taps beyond thirteen K steps
    src = rng.integers(0, 256, (20, 64, cn) if cn > 1 else (20, 64), dtype=np.uint8)
    assert run(emu, src, src.shape[:2], (0, 0), 4, [0, 0, 256, 0, 0], 2, gauss(9, 1.5), 4)[0] == 1
    assert run(emu, src, src.shape[:2], (0, 0), 4, [100, 100, 100], 1, gauss(9, 1.5), 4)[0] == 1
    assert run(emu, src, src.shape[:2], (0, 0), 4, gauss(129, 21.0), 64, gauss(9, 1.5), 4)[0] == (0 if cn <= 3 else 1)      # 32 + 128 cn bytes of taps: 5 / 9 / 13 K steps, 17 for four channels


def test_sepmx_host_half_windows_and_box(emu):
    rng = np.random.default_rng(300)
    for cn in (1, 3):
        parent = rng.integers(0, 256, (60, 330, cn) if cn > 1 else (60, 330), dtype=np.uint8)
        kx, ky = gauss(19, 3.0), gauss(13, 2.0)
        for (x0, y0, w, h) in [(5, 4, 300, 40), (0, 0, 128, 60), (320, 10, 10, 40), (37, 11, 257, 33)]:
            margins = (x0, y0, 330 - x0 - w, 60 - y0 - h)
            roi = parent[y0:y0 + h, x0:x0 + w]
            for border in (0, 1, 2, 4):
                rc, got, info = run(emu, roi, parent.shape[:2], (x0, y0), border, kx, 9, ky, 6, addr=0x7f0000000000 + x0 * cn)
                assert rc == 0
                assert np.array_equal(got, o.orc_sepSmoothFixedU8(roi, kx, ky, border, margins)), (cn, x0, y0, w, h, border, info)
    # cv::boxFilter's three finishes with odd anchors
    src = rng.integers(0, 256, (50, 317), dtype=np.uint8)
    for (kw, kh, anchor, norm) in [(9, 9, (-1, -1), True), (15, 15, (-1, -1), True), (31, 17, (3, 16), True), (21, 5, (-1, -1), False), (129, 3, (-1, -1), True), (255, 41, (-1, -1), True), (9, 255, (-1, -1), True)]:
        ax = kw // 2 if anchor[0] < 0 else anchor[0]; ay = kh // 2 if anchor[1] < 0 else anchor[1]
        area = kw * kh
        if not norm:
            box = (3, 0, 0, 0.0, 0.0)
        elif area <= 256:
            d = int(np.rint(1.0 / (1.0 / area))); sf = float(1 << 23) / d; ds = int(np.floor(sf)); sf -= ds; dd = d // 2
            if sf < 0.5: dd += 1
            else: ds += 1
            box = (1, ds, dd, 0.0, 0.0)
        else:
            box = (2, 0, 0, float(np.float32(1.0 / area)), 1.0 / area)
        for border in (0, 1, 4):
            rc, got, info = run(emu, src, src.shape[:2], (0, 0), border, [1] * kw, ax, [1] * kh, ay, box=box)
            assert rc == 0
            assert np.array_equal(got, o.orc_boxFilter(src, -1, (kw, kh), anchor, norm, border)), (kw, kh, anchor, norm, border, info)


# ----------------------------------------------------------------------------- the unchecked loader's reach
def reach(emu, sstep, w, h, cn, full, off, kx, ax, ky, ay, addr, fast_rule=0, border=1):
    """(rc, dict) of emu_sepmx_inner_reach: the byte range, from the parent's first byte, of the chunks k_sepmx loads without a bounds test"""
    kx = np.ascontiguousarray(kx, np.uint16); ky = np.ascontiguousarray(ky, np.uint16)
    out = (ctypes.c_longlong * 9)()
    emu.emu_sepmx_inner_reach.restype = ctypes.c_int
    rc = emu.emu_sepmx_inner_reach(ctypes.c_size_t(sstep), w, h, cn, full[0], full[1], off[0], off[1], border, o.P(kx), len(kx), ax, o.P(ky), len(ky), ay,
                                   ctypes.c_ulonglong(addr), fast_rule, out)
    return rc, dict(zip(("min", "max", "span", "count", "fast", "ksx", "shift", "delta", "dma"), list(out)))


def inside(r):
    return r["count"] == 0 or (r["min"] >= 0 and r["max"] + 16 <= r["span"])


BASE = 0x7f0000000000
PITCHES = [512] + list(range(513, 640, 16)) + [527, 639, 640, 1024] + [528, 576, 624]      # (the last three: 16-byte aligned pitches inside the range, i.e. asynchronous staging)


def box_geometries(cn, kw):
    """(pitch, W, fullW, fullH, offX, offY, address, anchor.x, residue): cv::boxFilter rows with the window's anchor from its left end to its right end, widths that put the
    last strip's start 1 / 128 / 255 elements before the row's end (four channels: elements come in fours -- 4 / 128 / 252), row starts at 16 n and 16 n + 5, whole images
    and windows with columns of the parent to their left"""
    for ax in sorted({0, 1, kw // 2, kw - 2, kw - 1}):
        for pitch in PITCHES:
            for align in (0, 5):
                for off_x in (0, 7):
                    for res in ((1, 128, 255) if cn != 4 else (4, 128, 252)):
                        yield pitch, ax, align, off_x, res


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_sepmx_unchecked_loads_stay_inside_the_parent(emu, cn):
    """k_sepmx's `inner` loader (sepmx.hip request(): steps whose rows are all real rows of the parent other than its first and last) loads every chunk without a test.
    A chunk that leaves the parent's memory there is invisible in the output (its weights are zero), so the walk is replayed on the CPU with the kernel's own helpers
    (sepmx_body.h: innerStep, stripX0, chunkE0, pieceChunks) and every unchecked chunk must lie in [0, span).  Before plan() looked at the reach (g.fast = pitch >= 512
    alone), boxFilter with anchor.x near 0 and a window of thirteen K steps staged up to 639 bytes past a row's start: with a pitch of 512 .. 639 bytes the piece of row
    fullH - 2 ran past the end of the image.  The last loop shows that this replay sees exactly that under the old rule."""
    ky = [1] * 5                                                                  # anchor.y = 2: steps stage parent rows 32 t - 2 + offY .. + 31
    seen_fast, seen_slow, old_rule_out, walked = 0, 0, 0, 0
    for kw in (61, 62, 129, 243, 255):
        kx = [1] * kw
        for pitch, ax, align, off_x, res in box_geometries(cn, kw):
            addr = BASE + off_x * cn + align                                      # the ROI's first byte (the parent starts at BASE + align)
            rc, r0 = reach(emu, pitch, 8, 95, cn, (off_x + 8, 95), (off_x, 0), kx, ax, ky, 2, addr)
            if rc == 1:
                continue                                                          # (more K steps than the row pass has: plan() declines, another kernel's)
            # the widest ROI the pitch holds with (WE + shift) % 256 == res
            w = (pitch // cn) - off_x
            while w > 0 and (w * cn + r0["shift"]) % 256 != res:
                w -= 1
            if w <= 0:
                continue
            for off_y in (0, 3):
                full_h = 95 + off_y                                               # the third step's last row is the parent's row fullH - 2: the last row the shortcut may touch
                geo = (pitch, w, 95, cn, (off_x + w, full_h), (off_x, off_y), kx, ax, ky, 2, addr)
                rc, r = reach(emu, *geo)
                assert rc == 0
                assert r["shift"] == r0["shift"] and (w * cn + r["shift"]) % 256 == res
                walked += r["count"]
                seen_fast += r["fast"] != 0; seen_slow += r["fast"] == 0
                assert inside(r), (cn, kw, ax, pitch, align, off_x, off_y, w, r)
                rc, old = reach(emu, *geo, fast_rule=1)
                assert old["count"] > 0                                           # (every pitch here is >= 512 and the image is tall enough: the old rule always took the shortcut)
                old_rule_out += not inside(old)
    assert walked > 0 and seen_fast > 0, (walked, seen_fast, seen_slow)          # the shortcut is still taken where it fits ...
    print("cn", cn, "shortcut kept", seen_fast, "given up", seen_slow, "geometries the pitch rule let out of the parent", old_rule_out)
    assert seen_slow > 0 and old_rule_out > 0, (seen_slow, old_rule_out)          # ... is given up where it does not, and the replay sees the pitch rule's escapes


@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_sepmx_unchecked_loads_gaussian_control(emu, cn):
    """the centred windows of cv::GaussianBlur (the geometries of test_sepmx_host_half_gaussian, and taller / wider ones so that inner steps exist): the shortcut stays on
    wherever the pitch is 512 bytes or more, and stays inside"""
    walked = 0
    for (w, h) in [(300, 40), (256 // cn, 33), (37, 5), (19, 70), (600 // cn, 9), (600, 200), (512 // cn, 130), (1031, 97)]:
        for (kw, kh, sigma) in [(19, 19, 3.0), (7, 33, 2.5), (33, 9, 5.0), (65, 11, 11.0), (129, 15, 21.0)]:
            if (kw - 1) * cn > 384:
                continue
            kx, ky = gauss(kw, sigma), gauss(kh, sigma)
            for addr in (BASE, BASE + 5):
                for pitch in sorted({w * cn, (w * cn + 15) // 16 * 16, w * cn + 64}):
                    rc, r = reach(emu, pitch, w, h, cn, (w, h), (0, 0), kx, kw // 2, ky, kh // 2, addr, border=4)
                    assert rc == 0, (w, h, cn, kw, kh)
                    assert r["fast"] == (pitch >= 512), (w, h, cn, kw, pitch, r)
                    assert inside(r), (w, h, cn, kw, kh, pitch, r)
                    walked += r["count"]
    assert walked > 0
