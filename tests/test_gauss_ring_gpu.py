"""GPU parity for the rolling Gaussian kernel's row loop (k_binomial_roll2, smooth.hip) at the shapes where its structure can go wrong: the loop over
whole groups of KS rows, the peeled nrows % KS tail, the batched prologue and the ring -- with the ring kept in flight (gauss_variant 6) and with the
earlier loop (gauss_variant 3), bit for bit against the oracle.

Heights and segment lengths give tails of 0 .. 4 rows, segments shorter than the ring (seg 5 at KS 5 leaves last segments of 1 .. 4 rows), images shorter
than KS, segments walked upwards (every odd one), and the XCD regrouping of 16 or more segments (H = 83 at seg = 5: 17 segments).  Widths give one chunk,
one partial wave, and a second strip with a single active lane (1040 = 65 chunks at one channel)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BORDERS = [0, 1, 2, 4]                       # the four this kernel serves (BORDER_WRAP takes k_binomial_roll)
WIDTHS = [16, 64, 1040]
HEIGHTS = [1, 2, 3, 4, 5, 6, 9, 10, 11, 16, 17, 31, 33, 83]
SEGS = [0, 5, 7, 15, 16]
NFRAMES = 3

_src, _want = {}, {}


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    return opencv_amd


def _frames(w, h, cn):
    key = (w, h, cn)
    if key not in _src:
        rng = np.random.default_rng(1000 * w + 10 * h + cn)
        a = rng.integers(0, 256, (NFRAMES, h, w, cn) if cn > 1 else (NFRAMES, h, w), dtype=np.uint8)
        _src[key] = (a, torch.from_numpy(a).cuda())
    return _src[key]


def _reference(orc, w, h, cn, ksize, border):
    key = (w, h, cn, ksize, border)
    if key not in _want:
        a, _ = _frames(w, h, cn)
        _want[key] = np.stack([orc.orc_gaussianBlurBinomialU8(a[f], ksize, border) for f in range(NFRAMES)])
    return _want[key]


@pytest.mark.parametrize("variant", [6, 3])
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("ksize", [3, 5])
def test_batch_bit_exact_over_tails_segments_and_borders(cv, orc, ksize, cn, variant):
    from opencv_amd import _lib
    L = _lib.lib
    try:
        assert L.mi355cv_setParam(b"gauss_variant", variant) == 0
        for w in WIDTHS:
            for h in HEIGHTS:
                _, dev = _frames(w, h, cn)
                out = torch.empty_like(dev)
                for seg in SEGS:
                    assert L.mi355cv_setParam(b"gauss_seg", seg) == 0
                    for border in BORDERS:
                        out.zero_()
                        cv.GaussianBlurBatch(dev, ksize, border, dst=out)
                        got = out.cpu().numpy()
                        want = _reference(orc, w, h, cn, ksize, border)
                        assert np.array_equal(got, want), (ksize, cn, variant, w, h, seg, border)
                    k = L.mi355cv_lastKernel().decode()
                    assert k.startswith("k_binomial_roll2<%d,%d,true,false,4,true%s>" % (ksize, cn, ",true" if variant == 6 else "")), k
                    if seg:
                        assert " seg=%d rows" % min(seg, h) in k, k
    finally:
        L.mi355cv_setParam(b"gauss_seg", 0)
        L.mi355cv_setParam(b"gauss_variant", 0)


def test_single_frame_entry(cv, orc):
    """cv.GaussianBlur on one frame (the staging entry, default variant and segment length): a tail of 3 rows at the heuristic's segment length or not, the
    result is the oracle's"""
    from opencv_amd import _lib
    rng = np.random.default_rng(83)
    for (h, w, cn) in [(83, 1040, 1), (33, 64, 3), (4, 16, 1)]:
        src = rng.integers(0, 256, (h, w, cn) if cn > 1 else (h, w), dtype=np.uint8)
        for border in BORDERS:
            got = cv.GaussianBlur(torch.from_numpy(src).cuda(), (5, 5), 0, 0, border).cpu().numpy()
            assert "k_binomial_roll2<5," in _lib.lib.mi355cv_lastKernel().decode()
            assert np.array_equal(got, orc.orc_gaussianBlurBinomialU8(src, 5, border)), (h, w, cn, border)
