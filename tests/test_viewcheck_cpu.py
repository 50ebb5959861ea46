"""The view harness (tests/viewcheck.py) checked without a GPU: numpy stand-ins for an op run through the same entry points tests/test_views_gpu.py uses.  A correct
stand-in passes on every layout; three wrong ones -- the three ways a kernel goes wrong on a cv::Mat ROI -- are each caught, with the right diagnosis; and the layouts
have the residues modulo 16 they promise for every pixel type the GPU tables use.  The second half does the same for what tests/test_warp_views_gpu.py needs:
further read-only inputs, a destination that is an input, two guarded destinations, and the 'oddstride' batch form with its control."""
import numpy as np
import pytest

import viewcheck as vc

TYPES = [(np.uint8, 1), (np.uint8, 3), (np.int16, 1), (np.float32, 1), (np.float64, 1)]
SHAPES = [(13, 1), (13, 5), (64, 3), (131, 4)]


def oracle(img):
    """a 1-2-1 row filter with a replicated border, in the image's own depth (integers wrap): an op with a border rule and a neighbourhood"""
    a = img if img.ndim == 3 else img[:, :, None]
    p = np.concatenate([a[:, :1], a, a[:, -1:]], axis=1)
    with np.errstate(over="ignore"):
        out = (p[:, :-2] + p[:, 1:-1] * a.dtype.type(2) + p[:, 2:]).astype(a.dtype)
    return out if img.ndim == 3 else out[:, :, 0]


def widened(v, left, right):
    """the view `v` of a parent, `left` / `right` pixels wider (what a kernel reaches through the same pointer and step)"""
    base = v
    while base.base is not None:
        base = base.base
    off = v.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    px = v.strides[1]
    shape = (v.shape[0], v.shape[1] + left + right) + v.shape[2:]
    return np.ndarray(shape, v.dtype, buffer=base.reshape(-1).view(np.uint8), offset=off - left * px, strides=v.strides)


def good(src, dst):
    dst[...] = oracle(np.ascontiguousarray(src))


def one_past_the_row_end(src, dst):
    """the last store of every row is one element too far"""
    out = oracle(np.ascontiguousarray(src))
    wide = widened(dst, 0, 1)
    wide[:, :-1] = out
    b = wide.view(np.uint8)                                          # (the stray element: its first byte flipped, whatever the sentinel holds)
    if wide.ndim == 3:
        b[:, -1, 0] ^= 0xFF
    else:
        b[:, -wide.itemsize] ^= 0xFF


def whole_vector_at_the_ragged_row_end(src, dst):
    """rows are stored in whole 16-byte vectors, the last one too although the row ends inside it"""
    out = np.ascontiguousarray(oracle(np.ascontiguousarray(src)))
    h = out.shape[0]
    rowb = out.size // h * out.itemsize
    padded = -(-rowb // 16) * 16
    rows = np.zeros((h, padded), np.uint8)
    rows[:, :rowb] = out.view(np.uint8).reshape(h, rowb)
    base = dst
    while base.base is not None:
        base = base.base
    off = dst.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    np.ndarray((h, padded), np.uint8, buffer=base.reshape(-1).view(np.uint8), offset=off, strides=(dst.strides[0], 1))[...] = rows


def reads_left_of_the_view(src, dst):
    """the left border pixel is read from memory instead of being replicated"""
    wide = widened(src, 1, 0)
    a = wide if wide.ndim == 3 else wide[:, :, None]
    p = np.concatenate([a, a[:, -1:]], axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        out = (p[:, :-2] + p[:, 1:-1] * a.dtype.type(2) + p[:, 2:]).astype(a.dtype)
    dst[...] = out if src.ndim == 3 else out[:, :, 0]


def image(dtype, cn, w, h):
    return vc.content(dtype, (h, w, cn) if cn > 1 else (h, w), seed=w * 7 + h)


def run(op, layout, dtype, cn, w, h):
    img = image(dtype, cn, w, h)
    return vc.run(op, layout, img, oracle(img), what="%s %s %dx%d" % (np.dtype(dtype).name, layout, w, h))


@pytest.mark.parametrize("dtype,cn", TYPES)
@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_correct_stand_in_passes(layout, dtype, cn):
    if layout == "F" and vc.pixel_bytes(dtype, cn) == 8:
        with pytest.raises(vc.Unreachable, match="no pixel offset gives a base of 4"):
            run(good, layout, dtype, cn, 13, 5)
        return
    for (w, h) in SHAPES:
        run(good, layout, dtype, cn, w, h)


@pytest.mark.parametrize("dtype,cn", TYPES)
@pytest.mark.parametrize("layout", ["A", "B", "C", "E"])
def test_store_one_element_past_the_row_end_is_caught(layout, dtype, cn):
    for (w, h) in SHAPES:
        with pytest.raises(vc.GuardTouched) as e:
            run(one_past_the_row_end, layout, dtype, cn, w, h)
        assert e.value.where == "right" and e.value.rel_row == 0 and e.value.past_end == 0, str(e.value)
        assert e.value.rel_byte == w * vc.pixel_bytes(dtype, cn) and "0 byte(s) past the row end" in str(e.value)


@pytest.mark.parametrize("dtype,cn", TYPES)
@pytest.mark.parametrize("layout", ["A", "B", "C", "E"])
def test_whole_vector_store_at_a_ragged_row_end_is_caught(layout, dtype, cn):
    for (w, h) in SHAPES:
        rowb = w * vc.pixel_bytes(dtype, cn)
        if rowb % 16 == 0:                                            # no ragged chunk: the stand-in is correct here, and must pass
            run(whole_vector_at_the_ragged_row_end, layout, dtype, cn, w, h)
            continue
        with pytest.raises(vc.GuardTouched) as e:
            run(whole_vector_at_the_ragged_row_end, layout, dtype, cn, w, h)
        assert e.value.where == "right" and e.value.rel_row == 0 and 0 <= e.value.past_end < 16 - rowb % 16, str(e.value)


@pytest.mark.parametrize("dtype,cn", TYPES)
@pytest.mark.parametrize("layout", ["A", "B", "D", "F"])
def test_reading_the_parent_instead_of_the_border_is_caught(layout, dtype, cn):
    if layout == "F" and vc.pixel_bytes(dtype, cn) == 8:
        with pytest.raises(vc.Unreachable):                           # CV_64FC1: no pixel offset gives a base of 4 modulo 16
            run(reads_left_of_the_view, layout, dtype, cn, 13, 5)
        return
    for (w, h) in SHAPES:
        with pytest.raises(vc.ResultMismatch) as e:
            run(reads_left_of_the_view, layout, dtype, cn, w, h)
        assert tuple(e.value.index[:2]) == (0, 0), str(e.value)       # the first wrong pixel is the first border pixel; no guard was touched


def test_in_place_and_batch_forms():
    img = image(np.uint8, 3, 64, 5)
    vc.run_inplace(lambda s, d: good(s.copy(), d), img, oracle(img))
    with pytest.raises(vc.GuardTouched) as e:
        vc.run_inplace(lambda s, d: one_past_the_row_end(s.copy(), d), img, oracle(img))
    assert e.value.where == "right"
    frames = np.stack([image(np.uint8, 1, 29, 6) + f for f in range(3)]).astype(np.uint8)
    want = np.stack([oracle(f) for f in frames])

    def each(op):
        def call(s, d):
            for f in range(len(s)):
                op(s[f], d[f])
        return call
    for form in vc.BATCH_FORMS:
        vc.run_batch(each(good), form, frames, want)
        with pytest.raises(vc.GuardTouched) as e:
            vc.run_batch(each(one_past_the_row_end), form, frames, want)
        assert e.value.where == "right" and e.value.frame == 0 and e.value.past_end == 0
        with pytest.raises(vc.ResultMismatch):
            vc.run_batch(each(reads_left_of_the_view), form, frames, want)
        g = vc.batch_geometry(form, np.uint8, 1, 29, 6, 2)
        assert g.x0 == 3 and g.pitch % 16 != 0 and g.pitch > 29
        assert (g.hp == 6 and g.y0 == 0) if form == "columns" else (g.y0 == 2 and g.hp == 10)    # 'columns': frame stride == step * height


def test_guards_are_as_wide_as_promised():
    for dtype, cn in vc.PIXELS_USED:
        for layout in vc.LAYOUTS:
            try:
                s, d = vc.plan(layout, dtype, cn, 13, 1, dtype, cn)
            except vc.Unreachable:
                continue
            for g in (s, d):
                assert g.y0 >= 2 and g.hp - g.y0 - g.h >= 2
                assert g.pitch - (g.x0 + g.w) * g.px >= 64


@pytest.mark.parametrize("dtype,cn", vc.PIXELS_USED)
def test_layout_residues(dtype, cn):
    """the residues modulo 16 each layout promises, measured on real views (pointer differences), for every pixel type of the GPU table"""
    px = vc.pixel_bytes(dtype, cn)
    for w in (13, 16, 64, 1042, 1043):
        for h in (1, 37):
            for layout in vc.LAYOUTS:
                try:
                    s, d = vc.plan(layout, dtype, cn, w, h, dtype, cn)
                except vc.Unreachable as e:
                    assert layout == "F" and px % 8 == 0 or px % 16 == 0, (layout, str(e))
                    continue
                res = []
                for g in (s, d):
                    parent = np.zeros(g.parent_shape(), dtype)
                    v = g.view(parent)
                    base = v.__array_interface__["data"][0] - parent.__array_interface__["data"][0]
                    assert base == g.base and parent.strides[0] == g.pitch and v.shape[:2] == (h, w)
                    res.append((base % 16, g.pitch % 16, base % 4, g.pitch % 4, g.x0))
                (sb, sp, sb4, sp4, sx), (db, dp, db4, dp4, dx) = res
                if layout == "A":
                    assert (sb, sp, db, dp) == (0, 0, 0, 0)
                if layout in "BD":
                    assert sx == 1 and sb != 0 and sp != 0 and (px % 4 == 0 or (sb4 != 0 and sp4 != 0))
                if layout in "BC":
                    assert dx == 3 and db != 0 and dp != 0 and (px % 4 == 0 or (db4 != 0 and dp4 != 0))
                if layout == "B":
                    assert s.wp != d.wp and (px % 8 == 0 or sp != dp)
                if layout == "C":
                    assert (sb, sp) == (0, 0)
                if layout == "D":
                    assert (db, dp) == (0, 0)
                if layout == "E":
                    assert sb == db == 0 and sp == dp and sp in (4, 8)
                if layout == "F":
                    assert (sb, sp, dp) == (4, 0, 0) and db in (8, 12)


# ---------------------------------------------------------------------------------------------------------------- what tests/test_warp_views_gpu.py adds to the harness
def _base_and_offset(v):
    base = v
    while base.base is not None:
        base = base.base
    return base, v.__array_interface__["data"][0] - base.__array_interface__["data"][0]


def shift_oracle(img, m):
    """an op with a map: out[y, x] = img[y, (x + m[y, x]) mod w]"""
    h, w = img.shape[:2]
    yy, xx = np.indices((h, w))
    return img[yy, (xx + m.astype(np.int64)) % w]


def shift_good(src, dst, m):
    dst[...] = shift_oracle(np.ascontiguousarray(src), np.ascontiguousarray(m))


def shift_reads_the_maps_parent(src, dst, m):
    """the map is read one pixel to the left: column 0 comes from the map's parent"""
    dst[...] = shift_oracle(np.ascontiguousarray(src), np.ascontiguousarray(widened(m, 1, 0)[:, :-1]))


def shift_writes_its_map(src, dst, m):
    shift_good(src, dst, m)
    m[0, 0] += 1


@pytest.mark.parametrize("dtype,cn", [(np.uint8, 3), (np.float32, 1)])
@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_further_read_only_inputs(layout, dtype, cn):
    """inputs=[...]: the map sits in a hostile parent like the source; a stand-in that reads that parent instead of the map is a wrong result at the first pixel,
    one that writes its map is a guard failure 'inside' input 0"""
    for (w, h) in SHAPES:
        img = image(dtype, cn, w, h)
        m = vc.content(np.int16, (h, w), seed=w + h, lo=0, hi=w + 5)
        what = "%s %s %dx%d" % (np.dtype(dtype).name, layout, w, h)
        vc.run(shift_good, layout, img, shift_oracle(img, m), what=what, inputs=[m])
        if layout in "BD":                                              # the map's left neighbour is its parent's pixel (layout A's view starts its parent's row)
            with pytest.raises(vc.ResultMismatch) as e:
                vc.run(shift_reads_the_maps_parent, layout, img, shift_oracle(img, m), what=what, inputs=[m])
            assert tuple(e.value.index[:2]) == (0, 0), str(e.value)
        with pytest.raises(vc.GuardTouched) as e:
            vc.run(shift_writes_its_map, layout, img, shift_oracle(img, m), what=what, inputs=[m])
        assert e.value.where == "inside" and (e.value.rel_row, e.value.rel_byte) == (0, 0) and "input 0" in str(e.value)


def _kept(h, w):
    yy, xx = np.indices((h, w))
    return (yy + 2 * xx) % 3 == 0                                       # the pixels the op does not reach


def keeping_oracle(img, prev):
    out = oracle(img)
    k = _kept(*img.shape[:2])
    out[k] = prev[k]
    return out


def keeping_good(src, dst):
    dst[...] = keeping_oracle(np.ascontiguousarray(src), np.ascontiguousarray(dst))


def keeping_overwrites_one(src, dst):
    """one pixel that should keep the destination's content is written"""
    out = keeping_oracle(np.ascontiguousarray(src), np.ascontiguousarray(dst))
    y, x = np.argwhere(_kept(*out.shape[:2]))[-1]
    out[y, x] = oracle(np.ascontiguousarray(src))[y, x] + out.dtype.type(1)
    dst[...] = out


@pytest.mark.parametrize("dtype,cn", [(np.uint8, 3), (np.float32, 1)])
@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_a_destination_that_is_an_input(layout, dtype, cn):
    """want as a callable: the expected result is computed from the sentinel the view starts with (NaNs and all: the comparison is bit for bit)"""
    for (w, h) in SHAPES:
        img = image(dtype, cn, w, h)
        like = (img.dtype, img.shape)
        seen = []

        def want(prev):
            seen.append(prev)
            return keeping_oracle(img, prev)
        vc.run(keeping_good, layout, img, want, dst_like=like)
        _, dg = vc.plan(layout, dtype, cn, w, h, dtype, cn)
        start = np.ascontiguousarray(dg.view(vc.sentinel(dtype, dg.parent_shape())))                    # what the view holds before the call
        assert np.array_equal(seen[0].view(np.uint8), start.view(np.uint8))
        with pytest.raises(vc.ResultMismatch) as e:
            vc.run(keeping_overwrites_one, layout, img, want, dst_like=like)
        assert tuple(e.value.index[:2]) == tuple(np.argwhere(_kept(h, w))[-1]), str(e.value)


def pair_oracle(img):
    return oracle(img), np.ascontiguousarray(img[::-1]).astype(np.int32 if img.dtype.kind != "f" else np.float64)


def pair_good(src, dsts):
    a, b = pair_oracle(np.ascontiguousarray(src))
    dsts[0][...] = a
    dsts[1][...] = b


def pair_second_one_past_the_row_end(src, dsts):
    a, _ = pair_oracle(np.ascontiguousarray(src))
    dsts[0][...] = a
    one_past_the_row_end_of(pair_oracle(np.ascontiguousarray(src))[1], dsts[1])


def one_past_the_row_end_of(out, dst):
    wide = widened(dst, 0, 1)
    wide[:, :-1] = out
    b = wide.view(np.uint8)
    if wide.ndim == 3:
        b[:, -1, 0] ^= 0xFF
    else:
        b[:, -wide.itemsize] ^= 0xFF


def pair_second_is_wrong(src, dsts):
    pair_good(src, dsts)
    dsts[1][-1, -1] += 1


@pytest.mark.parametrize("dtype,cn", [(np.uint8, 3), (np.int16, 1), (np.float32, 1)])
@pytest.mark.parametrize("layout", ["A", "B", "C", "E"])
def test_two_guarded_destinations(layout, dtype, cn):
    for (w, h) in SHAPES:
        img = image(dtype, cn, w, h)
        vc.run(pair_good, layout, img, pair_oracle(img))
        with pytest.raises(vc.GuardTouched) as e:
            vc.run(pair_second_one_past_the_row_end, layout, img, pair_oracle(img))
        assert e.value.where == "right" and e.value.rel_row == 0 and e.value.past_end == 0 and " dst 1:" in str(e.value), str(e.value)
        with pytest.raises(vc.ResultMismatch) as e:
            vc.run(pair_second_is_wrong, layout, img, pair_oracle(img))
        assert tuple(e.value.index[:2]) == (h - 1, w - 1) and " dst 1:" in str(e.value), str(e.value)


@pytest.mark.parametrize("dtype,cn", [(np.uint8, 1), (np.uint8, 3), (np.int16, 1), (np.uint16, 3)])
def test_oddstride_batch_form(dtype, cn):
    """frames behind a frame stride of hp * pitch + one element in one flat allocation.  Measured on the views: the first frame and the step are multiples of 16 and
    the frame stride is 1 or 2 modulo 4, so the stride is the only thing an alignment predicate can object to; 'aligned', its control, differs in the gap alone.  A
    correct stand-in passes, the wrong ones of the other forms are caught as there, and a store one element past a frame's last parent row lands in the gap and is
    caught as 'gap'"""
    def each(op):
        def call(s, d):
            for f in range(len(s)):
                op(s[f], d[f])
        return call
    isz = np.dtype(dtype).itemsize
    for (w, h) in [(13, 5), (29, 6), (64, 3), (131, 4)]:
        frames = np.stack([image(dtype, cn, w, h) + dtype(f) for f in range(3)])
        want = np.stack([oracle(f) for f in frames])
        g = vc.batch_geometry(vc.ODDSTRIDE, dtype, cn, w, h, 3 if cn > 1 else 2)
        c = vc.batch_geometry(vc.ALIGNED, dtype, cn, w, h, 3 if cn > 1 else 2)
        assert g.gap == isz and g.frame_stride == g.hp * g.pitch + isz and g.frame_stride % 4 == isz and (g.hp, g.y0, g.x0) == (h + 4, 2, 0)
        assert c.gap == 0 and c.frame_stride == c.hp * c.pitch and (c.hp, c.y0, c.x0, c.pitch) == (g.hp, g.y0, g.x0, g.pitch)
        seen = []

        def good_and_measured(s, d):
            for v in (s, d):
                ptr = v.__array_interface__["data"][0]
                seen.append((v.strides[0], v.strides[1] % 16, (ptr - _base_and_offset(v)[0].__array_interface__["data"][0]) % 16))
            each(good)(s, d)
        for form, stride in ((vc.ODDSTRIDE, g.frame_stride), (vc.ALIGNED, c.frame_stride)):
            del seen[:]
            vc.run_batch(good_and_measured, form, frames, want)
            assert seen == [(stride, 0, 0), (stride, 0, 0)], (form, seen)

        def into_the_gap(s, d, frame=1):
            each(good)(s, d)
            base, off = _base_and_offset(d)
            base.reshape(-1).view(np.uint8)[off - g.base + frame * g.frame_stride + g.hp * g.pitch] ^= 0xFF
        with pytest.raises(vc.GuardTouched) as e:
            vc.run_batch(into_the_gap, vc.ODDSTRIDE, frames, want)
        assert e.value.where == "gap" and e.value.frame == 1 and e.value.byte == 0 and e.value.row == g.hp, str(e.value)
        for form in (vc.ODDSTRIDE, vc.ALIGNED):
            with pytest.raises(vc.GuardTouched) as e:
                vc.run_batch(each(one_past_the_row_end), form, frames, want)
            assert e.value.where == "right" and e.value.frame == 0 and e.value.past_end == 0
        with pytest.raises(vc.ResultMismatch):
            vc.run_batch(each(reads_left_of_the_view), vc.ODDSTRIDE, frames, want)


def test_oddstride_is_not_built_for_four_byte_elements():
    with pytest.raises(ValueError, match="1- and 2-byte elements"):
        vc.batch_geometry(vc.ODDSTRIDE, np.float32, 1, 13, 5, 2)
    assert vc.BATCH_FORMS == ("roi", "columns") and vc.BATCH_FORMS_ALL == ("roi", "columns", "oddstride")
