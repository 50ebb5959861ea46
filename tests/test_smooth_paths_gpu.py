"""One row per served path of the 8U Gaussian's path chain (smooth.hip, struct SmoothCall: binomialRoll, sepmxLong, seprollWhole, seprollWindow, sepmxShort, seplongQ88,
sepfixedGeneric) and of the two routes of the CV_16U sigma-0 case (runBinom16): the output is bit-equal to the oracle and mi355cv_lastKernel names the kernel the row
is about.  The batch entries walk the SAME chain, so a batch of 3 device-resident frames -- views with padding rows between them -- must give, frame for frame, what
the single-image call gives, under a note that names the same kernel.  (The matrices of sizes, borders and taps are test_gaussian_gpu.py / test_sepmx_gpu.py.)"""
import numpy as np
import pytest
import torch

from test_oracle_smooth16 import np_binom16

pytestmark = pytest.mark.gpu

N, H, W, W_RAGGED = 3, 40, 48, 50        # W: rows of whole 16-byte chunks; W_RAGGED: a ragged last chunk
PARENT, ROI = (60, 90, 3), (5, 4, 40, 30)  # a window (x0, y0, w, h) with real pixels on all four sides


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    return opencv_amd


def image(w, cn=1, dtype=np.uint8, h=H, seed=0):
    rng = np.random.default_rng(1000 * seed + 10 * w + cn)
    return rng.integers(0, np.iinfo(dtype).max + 1, (h, w, cn) if cn > 1 else (h, w)).astype(dtype)


def dev(a):
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def note(cv):
    return cv._lib.lib.mi355cv_lastKernel().decode()


def another_family_first(cv):
    """the note is the calling thread's last one: a call of another family first, so that a path that writes none cannot pass on a note left behind"""
    cv.medianBlur(dev(image(W)), 3)
    assert note(cv).startswith("k_median")


def taps(orc, n, sigma):
    return [int(v) for v in orc.orc_getGaussianKernelQ(n, sigma)]


def window(a):
    x0, y0, w, h = ROI
    return a[y0:y0 + h, x0:x0 + w]


MARGINS = (ROI[0], ROI[1], PARENT[1] - ROI[0] - ROI[2], PARENT[0] - ROI[1] - ROI[3])
SATURATING = [128, 128, 128]              # Q8.8 taps that sum to 384: no fixed-point path takes them

# (id, expected text, "starts" / "contains", source image, call on the device image, oracle on the host image)
ROWS = [
    ("roll2-5-c1", "k_binomial_roll2<5,1,true,false,4,true,true>", "starts", lambda: image(W),
     lambda cv, orc, d: cv.GaussianBlur(d, (5, 5), 0, borderType=4), lambda orc, a: orc.orc_gaussianBlurBinomialU8(a, 5, 4)),
    ("roll2-3-c2", "k_binomial_roll2<3,2,", "starts", lambda: image(W, 2),
     lambda cv, orc, d: cv.GaussianBlur(d, (3, 3), 0, borderType=1), lambda orc, a: orc.orc_gaussianBlurBinomialU8(a, 3, 1)),
    ("roll-wrap", "k_binomial_roll<5,1>", "starts", lambda: image(W),
     lambda cv, orc, d: cv.GaussianBlur(d, (5, 5), 0, borderType=3), lambda orc, a: orc.orc_gaussianBlurBinomialU8(a, 5, 3)),
    ("sepmx-long", "k_sepmx<", "starts", lambda: image(W_RAGGED),
     lambda cv, orc, d: cv.GaussianBlur(d, (11, 11), 2.0), lambda orc, a: orc.orc_sepSmoothFixedU8(a, taps(orc, 11, 2.0), taps(orc, 11, 2.0), 4)),
    ("sepmx-long-margins", "k_sepmx<", "starts", lambda: image(PARENT[1], PARENT[2], h=PARENT[0]),
     lambda cv, orc, d: cv.sepSmoothFixedU8(window(d), taps(orc, 11, 2.0), taps(orc, 11, 2.0), 4, margins=MARGINS),
     lambda orc, a: orc.orc_sepSmoothFixedU8(window(a), taps(orc, 11, 2.0), taps(orc, 11, 2.0), 4, MARGINS)),
    ("seproll-sigma", "k_sep_roll<FixedSmooth K=5", "starts", lambda: image(W, 3),
     lambda cv, orc, d: cv.GaussianBlur(d, (5, 5), 1.5), lambda orc, a: orc.orc_sepSmoothFixedU8(a, taps(orc, 5, 1.5), taps(orc, 5, 1.5), 4)),
    ("seproll-ragged", "k_sep_roll<FixedSmooth", "starts", lambda: image(W_RAGGED),          # not rollEligible: the ragged chunk
     lambda cv, orc, d: cv.GaussianBlur(d, (5, 5), 0), lambda orc, a: orc.orc_gaussianBlurBinomialU8(a, 5, 4)),
    ("seproll-window", "window of a larger image", "contains", lambda: image(PARENT[1], PARENT[2], h=PARENT[0]),
     lambda cv, orc, d: cv.sepSmoothFixedU8(window(d), taps(orc, 5, 0), taps(orc, 5, 0), 4, margins=MARGINS),
     lambda orc, a: orc.orc_sepSmoothFixedU8(window(a), taps(orc, 5, 0), taps(orc, 5, 0), 4, MARGINS)),
    ("sepmx-short", "k_sepmx<", "starts", lambda: image(W_RAGGED, 2),
     lambda cv, orc, d: cv.GaussianBlur(d, (5, 5), 1.5), lambda orc, a: orc.orc_sepSmoothFixedU8(a, taps(orc, 5, 1.5), taps(orc, 5, 1.5), 4)),
    ("seplong-q88", "k_seplong<3,", "starts", lambda: image(W_RAGGED, 2),                    # a centre tap above 127 is no int8 for k_sepmx, two channels are none of k_sep_roll's
     lambda cv, orc, d: cv.GaussianBlur(d, (7, 7), 0.5, borderType=4), lambda orc, a: orc.orc_sepSmoothFixedU8(a, taps(orc, 7, 0.5), taps(orc, 7, 0.5), 4)),
    ("generic-saturating", "k_sepfixed_generic", "starts", lambda: image(W_RAGGED),
     lambda cv, orc, d: cv.sepSmoothFixedU8(d, SATURATING, SATURATING, 4), lambda orc, a: orc.orc_sepSmoothFixedU8(a, SATURATING, SATURATING, 4)),
    ("binom16-roll", "k_sep_roll<Binom16", "starts", lambda: image(W, dtype=np.uint16),
     lambda cv, orc, d: cv.GaussianBlur(d, (5, 5), 0), lambda orc, a: np_binom16(a, 5, 4)),
    ("binom16-direct", "k_binom16_direct<7>", "starts", lambda: image(W, dtype=np.uint16),
     lambda cv, orc, d: cv.GaussianBlur(d, (7, 7), 0), lambda orc, a: np_binom16(a, 7, 4)),
]


@pytest.mark.parametrize("expected,how,source,call,oracle", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_each_path_serves_its_call(cv, orc, expected, how, source, call, oracle):
    src = source()
    another_family_first(cv)
    got = host(call(cv, orc, dev(src)))
    said = note(cv)
    want = oracle(orc, src)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    assert said.startswith(expected) if how == "starts" else expected in said, said


# (id, expected prefix, call on a batch or on one frame, oracle on one host frame)
BATCH_ROWS = [
    ("roll2-batch", "k_binomial_roll2<5,1,true,false,4,true,true>",
     lambda cv, b: cv.GaussianBlurBatch(b, 5), lambda cv, f: cv.GaussianBlur(f, (5, 5), 0), lambda orc, a: orc.orc_gaussianBlurBinomialU8(a, 5, 4)),
    ("seproll-batch", "k_sep_roll<FixedSmooth",
     lambda cv, b: cv.GaussianBlurBatch(b, (5, 5), sigmaX=1.5), lambda cv, f: cv.GaussianBlur(f, (5, 5), 1.5),
     lambda orc, a: orc.orc_sepSmoothFixedU8(a, taps(orc, 5, 1.5), taps(orc, 5, 1.5), 4)),
]


@pytest.mark.parametrize("expected,batch,single,oracle", [pytest.param(*r[1:], id=r[0]) for r in BATCH_ROWS])
def test_batch_walks_the_same_chain(cv, orc, expected, batch, single, oracle):
    padded = dev(np.stack([image(W, h=H + 3, seed=f + 1) for f in range(N)]))
    fr = padded[:, :H]                                                 # [N, H, W] as views of a tensor with 3 padding rows after every frame
    another_family_first(cv)
    got = batch(cv, fr)
    said_batch = note(cv)
    singles = [single(cv, f) for f in reversed(fr)][::-1]              # frame 0 last: its note is the one compared
    said_single = note(cv)
    for f in range(N):
        assert np.array_equal(host(got[f]), oracle(orc, host(fr[f]))), f
        assert torch.equal(got[f], singles[f]), f
    assert said_batch.startswith(expected), said_batch
    assert said_batch.split(" ")[0] == said_single.split(" ")[0], (said_batch, said_single)
