"""cv::fastNlMeansDenoising / fastNlMeansDenoisingColored on the GPU (opencv_amd/csrc/nlmeans.hip) against tests/nlmeans_restate.py bit for bit, under the built-in
rule and with each kernel forced: images smaller than the border, widths and heights around the tile kernel's wave and workgroup edges, the window pairs, the strengths
(one whose table prefix exceeds the LDS bound and must be served by the plain kernel), 1 .. 4 channels, the contents, pitched misaligned views with guarded destinations,
batches (cut by a lowered chunk bound and by the host pipeline), numpy and device inputs, Colored against cvtColor -> restatement -> cvtColor.  The last test does not
rest on the restatement: a smooth image with Gaussian noise must come back closer to the clean one."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import nlmeans_restate as R
import viewcheck as vc
import opencv_amd as cv
from opencv_amd import _lib
from viewtable import Device

pytestmark = pytest.mark.gpu
Lb = _lib.lib
TILE_COLS, TILE_ROWS, TILE_MAX_T, LDS_TABLE, LDS_KIB = (_lib.limit("nlm_" + k) for k in ("tile_cols", "tile_rows", "tile_max_template", "lds_table", "tile_lds_kib"))
WAVE_ROWS = TILE_ROWS // 2
PLAIN, TILE = "k_nlm_plain", "k_nlm_tile"


def wave_cols(tws):
    """output columns of one wave of the tile kernel: its 64 lanes less the T - 1 a patch spans"""
    return TILE_COLS // 2 - 2 * (tws // 2)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def last_kernel():
    return Lb.mi355cv_lastKernel().decode()


def same(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), bad[:5].tolist(), [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])


@contextlib.contextmanager
def forced(arm):
    assert Lb.mi355cv_fastNlMeansSetKernel(arm) == 0
    try:
        yield
    finally:
        Lb.mi355cv_fastNlMeansSetKernel(-1)


@contextlib.contextmanager
def chunk(frames):
    assert Lb.mi355cv_fastNlMeansSetChunk(frames) == 0
    try:
        yield
    finally:
        Lb.mi355cv_fastNlMeansSetChunk(0)


def tile_serves(h, cn, tws, sws):
    """the library's rule for the tile kernel, from the limits it reports: T, the table's prefix, and the table (16-bit words where mult fits them, 32-bit
    otherwise, rounded up to 16 bytes) plus the tile within the LDS bound"""
    _, g, prefix = R.weight_table(h, cn, tws, sws)
    lds = (prefix * (4 if g["mult"] > 0xFFFF else 2) + 15) // 16 * 16 + (2 * wave_cols(tws) + 2 * g["b"]) * (TILE_ROWS + 2 * g["b"]) * cn
    return g["T"] <= TILE_MAX_T and prefix <= LDS_TABLE and lds <= LDS_KIB << 10


# ---- contents, [H, W] or [H, W, cn]
def shaped(H, W, cn):
    return (H, W) if cn == 1 else (H, W, cn)


def smooth_noisy(seed, H, W, cn=1, sigma=6.0):
    """a smooth image with noise: neighbouring patches are close, so most offsets of the window carry weight"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    planes = [128 + 50 * np.sin(x / (7.0 + c)) + 30 * np.cos(y / (5.0 + c)) for c in range(cn)]
    img = np.stack(planes, axis=2) + rng.normal(0.0, sigma, (H, W, cn))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(shaped(H, W, cn))


def random_bytes(seed, H, W, cn=1):
    return np.random.default_rng(seed).integers(0, 256, shaped(H, W, cn), dtype=np.uint8)


def checkerboard(H, W, cn=1, lo=100, hi=112):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(np.where((x + y) % 2 == 0, lo, hi).astype(np.uint8)[:, :, None], cn, axis=2).reshape(shaped(H, W, cn))


@functools.lru_cache(maxsize=None)
def _expected(key, h, tws, sws):
    return R.denoise(_IMAGES[key], h, tws, sws)


_IMAGES = {}


def expected(img, h, tws, sws):
    """the restatement's answer, computed once per (image, parameters)"""
    key = (img.shape, img.tobytes())
    _IMAGES.setdefault(key, img)
    return _expected(key, float(h), tws, sws)


def all_arms(img, h, tws=7, sws=21, what=""):
    """the device call under the built-in rule, with the plain kernel forced and with the tile kernel forced: all equal the restatement, each served by the
    kernel the rule names"""
    want = expected(img, h, tws, sws)
    d = dev(img)
    cn = 1 if img.ndim == 2 else img.shape[2]
    fast = tile_serves(h, cn, tws, sws)
    for arm, name in ((-1, TILE if fast else PLAIN), (0, PLAIN), (1, TILE if fast else PLAIN)):
        with forced(arm):
            n0 = cv.call_count("fastNlMeansDenoising")
            same(cv.fastNlMeansDenoising(d, h, tws, sws), want, (what, img.shape, h, tws, sws, arm))
            assert cv.call_count("fastNlMeansDenoising") == n0 + 1
            assert name in last_kernel(), (what, arm, last_kernel())
    return want


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 5)])
def test_images_smaller_than_the_border(shape):
    """7 / 21 has a border of 13: every index is reflected, several times over; a dimension of length 1 maps to index 0"""
    for cn in (1, 3):
        all_arms(smooth_noisy(1, *shape, cn), 10, what="small")
        all_arms(random_bytes(2, *shape, cn), 30, what="small random")


@pytest.mark.parametrize("tws,sws", [(7, 21), (3, 5)])
def test_widths_around_the_tile_edges(tws, sws):
    """one below, at and one above a wave's columns and a workgroup's, and two workgroups and one"""
    wc = wave_cols(tws)
    for w in (wc - 1, wc, wc + 1, 2 * wc - 1, 2 * wc, 2 * wc + 1, 4 * wc + 1):
        all_arms(smooth_noisy(w, 5, w), 10, tws, sws, what="width")


@pytest.mark.parametrize("tws,sws", [(7, 21), (3, 5)])
def test_heights_around_the_tile_edges(tws, sws):
    for h in (WAVE_ROWS - 1, WAVE_ROWS, WAVE_ROWS + 1, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1):
        all_arms(smooth_noisy(h, h, 7), 10, tws, sws, what="height")


def test_two_tiles_and_one_in_both_directions():
    all_arms(smooth_noisy(3, 2 * TILE_ROWS + 1, 4 * wave_cols(7) + 1), 10, what="2x2 tiles + 1")


@pytest.mark.parametrize("cn", [1, 2, 3, 4])
@pytest.mark.parametrize("tws,sws", [(1, 1), (1, 3), (3, 5), (7, 21), (9, 23), (6, 20)])
def test_window_pairs_and_channels(tws, sws, cn):
    """(6, 20) is served as (7, 21); S = 1 returns the input; T = 1 compares single pixels"""
    img = smooth_noisy(10 * tws + cn, 19, 70, cn)
    want = all_arms(img, 10, tws, sws, what="pair")
    if sws == 1:
        assert np.array_equal(want, img)
    if (tws, sws) == (6, 20):
        assert np.array_equal(want, expected(img, 10, 7, 21))


@pytest.mark.parametrize("h", [0, 0.5, 3, 10, 30])
def test_strengths(h):
    for cn in (1, 3):
        img = smooth_noisy(int(h * 2) + cn, 18, 61, cn)
        want = all_arms(img, h, what="h")
        if h == 0:
            assert np.array_equal(want, img)


def test_a_prefix_beyond_the_lds_table_goes_to_the_plain_kernel():
    _, _, prefix = R.weight_table(60, 3, 7, 21)
    assert prefix > LDS_TABLE and not tile_serves(60, 3, 7, 21)
    img = smooth_noisy(50, 9, 33, 3, sigma=20.0)
    all_arms(img, 60, what="long prefix")
    with forced(-1):
        cv.fastNlMeansDenoising(dev(img), 60)
        assert PLAIN in last_kernel(), last_kernel()


@pytest.mark.parametrize("h,cn,tws,sws", [(30, 3, 7, 21), (50, 3, 7, 21), (45, 4, 7, 21), (40, 2, 3, 5), (60, 1, 1, 11), (25, 3, 9, 13)])
def test_long_prefixes_in_lds(h, cn, tws, sws):
    """tables of tens of thousands of entries beside the tile: 16-bit words from S = 13 on (h = 50 on three channels at 7 / 21 asks for more than 64 KiB of LDS),
    32-bit words below, where mult does not fit 16 bits; weights close to mult and close to the cut at 0.001 mult are both read"""
    _, g, prefix = R.weight_table(h, cn, tws, sws)
    assert tile_serves(h, cn, tws, sws) and prefix > 4000 and (g["mult"] > 0xFFFF) == (sws < 13)
    img = smooth_noisy(h + cn, 21, 64, cn, sigma=25.0)
    all_arms(img, h, tws, sws, what="long prefix in LDS")


def test_contents():
    H, W = 17, 67
    for cn in (1, 3):
        for img in (random_bytes(4, H, W, cn), np.zeros(shaped(H, W, cn), np.uint8), np.full(shaped(H, W, cn), 255, np.uint8), checkerboard(H, W, cn),
                    smooth_noisy(5, H, W, cn)):
            want = all_arms(img, 10, what="content")
            if img.min() == img.max():
                assert np.array_equal(want, img)          # a constant image returns itself: 255 at 7 / 21 needs the unsigned sum


@pytest.mark.parametrize("device", [Device, vc.Host], ids=["device", "host"])
@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_pitched_views_at_misaligned_origins(layout, device):
    """source and destination as views of wider parents at the layout's offsets and pitches; the destination's parent is guarded, the source's is hostile"""
    for cn, tws, sws in ((1, 7, 21), (3, 3, 5)):
        img = vc.tame(smooth_noisy(7 + cn, 21, 83, cn))
        want = expected(img, 10, tws, sws)
        for arm in (-1, 0):
            with forced(arm):
                def call(sv, dv):
                    assert cv.fastNlMeansDenoising(sv, 10, tws, sws, dst=dv) is dv
                name, _ = vc.run(call, layout, img, want, what="%s cn %d arm %d" % (layout, cn, arm), device=device, kernel_name=last_kernel)
                assert (TILE if arm else PLAIN) in name, name


@pytest.mark.parametrize("nframes", [1, 3, 17])
def test_batches_equal_single_calls(nframes):
    """17 host-resident frames are cut by the host pipeline (16 frames a chunk), device-resident ones by the lowered chunk bound"""
    H, W = 13, 70
    for cn in (1, 3):
        frames = np.stack([smooth_noisy(100 + f, H, W, cn) if f % 2 else random_bytes(100 + f, H, W, cn) for f in range(nframes)])
        want = np.stack([expected(f, 10, 7, 21) for f in frames])
        for device in (Device, vc.Host):
            for form in vc.BATCH_FORMS:
                def call(sv, dv):
                    assert cv.fastNlMeansDenoisingBatch(sv, 10, dst=dv) is dv
                name, _ = vc.run_batch(call, form, frames, want, what="batch cn %d" % cn, device=device, kernel_name=last_kernel)
                assert TILE in name, name
        d = dev(frames)
        same(cv.fastNlMeansDenoisingBatch(d, 10), want, "device stack")
        assert "1 launch(es) of <= %d frames" % nframes in last_kernel(), last_kernel()
        with chunk(2):
            same(cv.fastNlMeansDenoisingBatch(d, 10), want, "chunks of two")
            assert "%d launch(es) of <= %d frames" % ((nframes + 1) // 2, min(2, nframes)) in last_kernel(), last_kernel()
        with forced(0):
            same(cv.fastNlMeansDenoisingBatch(d, 10), want, "forced plain")
            assert PLAIN in last_kernel(), last_kernel()
        got = cv.fastNlMeansDenoisingBatch(frames, 10)
        assert isinstance(got, np.ndarray)
        same(got, want, "numpy stack")
        same(cv.fastNlMeansDenoisingBatch([d[f] for f in range(nframes)], 10), want, "list of tensors")


def _to_lab(a):
    return cv.cvtColor(np.ascontiguousarray(a), cv.COLOR_LBGR2Lab)


def _from_lab(a):
    return cv.cvtColor(np.ascontiguousarray(a), cv.COLOR_Lab2LBGR)


def test_colored_is_lab_the_rule_twice_and_back():
    H, W = 20, 75
    imgs = [smooth_noisy(20 + f, H, W, 3, sigma=8.0) for f in range(3)]
    for h, hColor, tws, sws in ((10, 10, 7, 21), (3, 12, 3, 5)):
        want = [R.denoise_colored(a, h, hColor, tws, sws, _to_lab, _from_lab) for a in imgs]
        for arm in (-1, 0, 1):
            with forced(arm):
                same(cv.fastNlMeansDenoisingColored(dev(imgs[0]), h, hColor, tws, sws), want[0], ("colored", arm))
                assert "L by %s, ab by %s" % ((TILE, TILE) if arm else (PLAIN, PLAIN)) in last_kernel(), last_kernel()
        got = cv.fastNlMeansDenoisingColored(imgs[0], h, hColor, tws, sws)
        assert isinstance(got, np.ndarray)
        same(got, want[0], "colored numpy")
        same(cv.fastNlMeansDenoisingColoredBatch(dev(np.stack(imgs)), h, hColor, tws, sws), np.stack(want), "colored device stack")
        with chunk(2):
            same(cv.fastNlMeansDenoisingColoredBatch(dev(np.stack(imgs)), h, hColor, tws, sws), np.stack(want), "colored, groups of two")
            assert "in groups of 2" in last_kernel(), last_kernel()
        same(cv.fastNlMeansDenoisingColoredBatch(np.stack(imgs), h, hColor, tws, sws), np.stack(want), "colored numpy stack")


def test_numpy_in_numpy_out_and_device_refusals():
    img = smooth_noisy(9, 12, 50)
    got = cv.fastNlMeansDenoising(img, 10)
    assert isinstance(got, np.ndarray)
    same(got, expected(img, 10, 7, 21))
    got = cv.fastNlMeansDenoising(dev(img), 10)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    # src and dst in one device buffer, overlapping
    buf = torch.zeros((20, 96), dtype=torch.uint8, device="cuda")
    n0 = _lib.decline_count("fastNlMeansDenoising")
    for s, d in ((buf[:, :64], buf[:, 32:]), (buf[:, :64], buf[:, :64]), (buf[2:12, :64], buf[10:20, :64])):
        with pytest.raises(NotImplementedError, match="src and dst overlap"):
            cv.fastNlMeansDenoising(s, 10, dst=d)
    assert _lib.decline_count("fastNlMeansDenoising") == n0 + 3
    assert (buf == 0).all()
    with pytest.raises(NotImplementedError, match="CV_8UC4"):
        cv.fastNlMeansDenoisingColored(dev(smooth_noisy(1, 8, 8, 4)))


@pytest.mark.parametrize("sigma", [10, 20])
def test_noise_is_halved(sigma):
    """not against the restatement: 24 x 40, round(128 + 60 sin(x / 9) + 40 cos(y / 7)) plus Gaussian noise of sigma, denoised with h = sigma, must come back with
    an RMSE against the clean image of at most half the noisy image's (the restatement alone: 9.9 -> 3.05 and 20.2 -> 5.69, ratios 0.31 and 0.28; the CPU test
    holds it to 0.4 for these seeds)"""
    clean, noisy = R.noise_case(sigma)
    for arm in (-1, 0):
        with forced(arm):
            got = cv.fastNlMeansDenoising(dev(noisy), sigma).cpu().numpy()
        before, after = R.rmse(noisy, clean), R.rmse(got, clean)
        print("sigma %d arm %d: RMSE %.2f -> %.2f, ratio %.3f" % (sigma, arm, before, after, after / before))
        assert after <= 0.5 * before, (sigma, arm, before, after)
