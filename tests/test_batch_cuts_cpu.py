"""The two vectorised references of tests/batchcuts.py over every binary 4 x 4 image (label4x4, dist4x4) against the per-image restatements the other suites use
(ccl_restate.label, disttransform_restate.distanceTransform), and the helpers themselves.  tests/test_batch_cuts_gpu.py compares 65541 frames of the library against
label4x4 / dist4x4 in one numpy comparison each; here a sample of those frames -- every 53rd and the ones around the 65535 / 65536 cut -- goes through the slow
restatement."""
import numpy as np
import pytest

import batchcuts as B
import ccl_restate as C
import disttransform_restate as D

N = 65541
SAMPLE = sorted(set(range(0, N, 53)) | set(range(65534, N)))


@pytest.fixture(scope="module")
def frames():
    f = B.all4x4(N)
    f.setflags(write=False)
    return f


def test_all4x4_is_every_binary_image_once_and_wraps(frames):
    assert frames.shape == (N, 4, 4) and frames.dtype == np.uint8 and set(np.unique(frames)) == {0, 255}
    code = ((frames.reshape(N, 16) != 0).astype(np.int64) << np.arange(16)).sum(axis=1)
    assert np.array_equal(code, np.arange(N) % 65536)
    assert not frames[0].any() and frames[65535].all() and not frames[65536].any() and frames[65537, 0, 0] == 255 and frames[65537].sum() == 255


def test_periodic_shows_a_wrong_frame():
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (B.P, 4, 16), dtype=np.uint8)
    fr = B.periodic(base, 65541)
    assert fr.shape == (65541, 4, 16) and np.array_equal(fr[B.P + 3], base[3]) and np.array_equal(fr[65535], base[65535 % B.P]) and 65535 % B.P == 24
    assert B.same_periodic(fr, base) == (True, None)
    restarted = fr.copy()
    restarted[65535:] = fr[:6]                                   # a second launch that starts again at frame 0
    assert B.same_periodic(restarted, base) == (False, 65535)
    skipped = fr.copy()
    skipped[70] = 0
    assert B.same_periodic(skipped, base) == (False, 70)


@pytest.mark.parametrize("connectivity,order", [(4, C.PIXEL), (8, C.PIXEL), (8, C.BLOCK)])
def test_label4x4_against_the_restatement(frames, connectivity, order):
    counts, labels = B.label4x4(frames, connectivity, order)
    assert counts.shape == (N,) and labels.shape == (N, 4, 4) and labels.dtype == np.int32
    wrong = []
    for i in SAMPLE:
        n, want = C.label(frames[i], connectivity, order)
        if n != counts[i] or not np.array_equal(want, labels[i]):
            wrong.append(i)
    assert not wrong, wrong[:10]
    assert counts[0] == 1 and counts[65535] == 2 and counts[65536] == 1


@pytest.mark.parametrize("metric,dtype", [(D.DIST_L2, np.float32), (D.DIST_L1, np.float32), (D.DIST_C, np.float32), (D.DIST_L1, np.uint8)])
def test_dist4x4_against_the_restatement(frames, metric, dtype):
    got = B.dist4x4(frames, metric, dtype)
    assert got.shape == (N, 4, 4) and got.dtype == dtype
    wrong = [i for i in SAMPLE if not np.array_equal(D.distanceTransform(frames[i], metric, dtype).view(np.uint8), got[i].view(np.uint8))]
    assert not wrong, wrong[:10]
    none = D.NO_SITE_8U if dtype == np.uint8 else D.NO_SITE_32F
    assert (got[65535] == none).all() and not got[65534].max() == none and (got[65536] == 0).all()


def test_cut_of_reads_the_three_wordings():
    assert B.cut_of("k_binomial_roll2<5,1,true,false,4,true,true> grid=9 x256 seg=5 rows alt=1, 3 launch(es) of <= 2 frames", 5)[0]
    assert not B.cut_of("k_binomial_roll2<5,1,true,false,4,true,true> grid=9 x256 seg=5 rows alt=1, 1 launch(es) of <= 5 frames", 5)[0]
    assert B.cut_of("k_ccl_strip<pixel,4,32S> grid=1x1x60000 x64 lds=1, seams, 65541 frame(s) in groups of 60000", 65541)[0]
    assert not B.cut_of("k_dist_row<L2,32F> grid=4x3 x256 lds=64, 3 frame(s) in groups of 3", 3)[0]
    assert B.cut_of("k_clahe_hist16 + k_clahe_lut16 + k_clahe_interp16 tiles=8x8 slices=1 frames=16/launch", 19)[0]
    assert B.cut_of("k_pyrup<depth 0> grid=1x1x65535 x256 cn=1, 2 launch(es)", 65541)[0] and not B.cut_of("k_pyrup<depth 0> grid=1x1x5 x256 cn=1, 1 launch(es)", 5)[0]
    assert not B.cut_of("k_median_roll<3,1,16>", 9)[0]
