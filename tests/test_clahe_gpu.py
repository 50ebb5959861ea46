"""CLAHE on the MI355X (opencv_amd.createCLAHE -> mi355cv_clahe / mi355cv_claheBatch, opencv_amd/csrc/clahe.hip) bit for bit against the numpy restatement
(tests/clahe_restate.py), with the call counters and mi355cv_lastKernel showing that the GPU kernels ran."""
import numpy as np
import pytest
import torch

import clahe_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return opencv_amd


def to_dev(a):
    if a.dtype == np.uint16:                              # moved as int16 bits, viewed back as uint16
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_host(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def last_kernel(cv):
    return cv._lib.lib.mi355cv_lastKernel().decode()


def image(rng, h, w, dtype, data="full"):
    hi = 256 if dtype == np.uint8 else (4096 if data == "12bit" else 65536)
    return rng.integers(0, hi, (h, w)).astype(dtype)


def run(cv, src, clip, tiles, **kw):
    n0 = cv.call_count("clahe")
    got = cv.createCLAHE(clip, tiles).apply(src, **kw)
    assert cv.call_count("clahe") == n0 + 1, "the GPU path did not run"
    assert "k_clahe_interp" in last_kernel(cv)
    return got


# sizes divisible and not (a divisible width with a non-divisible height among them), grids 1 x 1 .. 16 x 16 and one wider than the image
GEOMS = [((64, 64), (8, 8)), ((640, 480), (8, 8)), ((641, 479), (8, 8)), ((640, 477), (8, 8)), ((333, 200), (3, 5)), ((257, 129), (1, 1)),
         ((512, 384), (16, 16)), ((5, 40), (8, 8)), ((1000, 3), (7, 2))]


@pytest.mark.parametrize("dtype,data", [(np.uint8, "full"), (np.uint16, "full"), (np.uint16, "12bit")])
@pytest.mark.parametrize("geom", GEOMS, ids=[f"{w}x{h}-{tx}x{ty}" for (w, h), (tx, ty) in GEOMS])
def test_clahe_matches_restatement(cv, dtype, data, geom):
    (w, h), tiles = geom
    rng = np.random.default_rng(w * 31 + h)
    src = image(rng, h, w, dtype, data)
    d = to_dev(src)
    for clip in (40.0, 2.0, 0.0, 1e6):
        got = to_host(run(cv, d, clip, tiles))
        assert np.array_equal(got, R.clahe(src, clip, tiles)), (clip,)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_constant_image(cv, dtype):
    src = np.full((64, 64), 100, dtype)
    d = to_dev(src)
    got = to_host(run(cv, d, 40.0, (8, 8)))
    assert np.array_equal(got, R.clahe(src))
    if dtype == np.uint8:
        assert np.all(got == 143)                          # the known answers
        assert np.all(to_host(run(cv, d, 0.0, (8, 8))) == 255)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_submatrix_takes_padding_from_the_parent(cv, dtype):
    rng = np.random.default_rng(3)
    parent = image(rng, 300, 400, dtype)
    p = to_dev(parent)
    for (x0, y0, w, h) in [(3, 5, 201, 150), (16, 0, 384, 299), (0, 10, 397, 280), (7, 7, 393, 293)]:
        got = to_host(run(cv, p, 40.0, (8, 8), roi=(x0, y0, w, h)))
        want = R.clahe(parent[y0:y0 + h, x0:x0 + w], 40.0, (8, 8), parent=parent, origin=(x0, y0))
        assert np.array_equal(got, want), (x0, y0, w, h)
    # the same from host memory: the margins travel with the staged image
    got = run(cv, parent, 4.0, (3, 5), roi=(3, 5, 201, 150))
    assert np.array_equal(got, R.clahe(parent[5:155, 3:204], 4.0, (3, 5), parent=parent, origin=(3, 5)))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_in_place(cv, dtype):
    rng = np.random.default_rng(5)
    src = image(rng, 481, 643, dtype)
    d = to_dev(src)
    out = run(cv, d, 40.0, (8, 8), dst=d)
    assert out is d
    assert np.array_equal(to_host(d), R.clahe(src, 40.0, (8, 8)))
    # in place on a submatrix of a device parent
    parent = image(rng, 200, 300, dtype)
    p = to_dev(parent)
    view = p[20:170, 30:261]
    run(cv, p, 3.0, (4, 4), roi=(30, 20, 231, 150), dst=view)
    want = R.clahe(parent[20:170, 30:261], 3.0, (4, 4), parent=parent, origin=(30, 20))
    got = to_host(p)
    assert np.array_equal(got[20:170, 30:261], want)
    mask = np.ones(parent.shape, bool); mask[20:170, 30:261] = False
    assert np.array_equal(got[mask], parent[mask])          # nothing outside the ROI written


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_numpy_host_input(cv, dtype):
    rng = np.random.default_rng(9)
    src = image(rng, 360, 640, dtype)
    got = run(cv, src, 40.0, (8, 8))
    assert isinstance(got, np.ndarray) and got.dtype == dtype
    assert np.array_equal(got, R.clahe(src, 40.0, (8, 8)))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_batch_equals_per_frame(cv, dtype):
    rng = np.random.default_rng(11)
    frames = np.stack([image(rng, 270, 481, dtype, "12bit" if i % 2 else "full") for i in range(5)])
    c = cv.createCLAHE(2.0, (8, 8))
    dev = torch.stack([to_dev(f) for f in frames])
    n0 = cv.call_count("claheBatch")
    out = c.applyBatch(dev)
    assert cv.call_count("claheBatch") == n0 + 1 and "k_clahe_interp" in last_kernel(cv)
    for i in range(len(frames)):
        single = to_host(c.apply(dev[i]))
        assert np.array_equal(to_host(out[i]), single), i
        assert np.array_equal(single, R.clahe(frames[i], 2.0, (8, 8))), i
    # frames in host memory go through the pipelined host path
    host = torch.stack([torch.from_numpy(f.view(np.int16) if dtype == np.uint16 else f) for f in frames])
    if dtype == np.uint16:
        host = host.view(torch.uint16)
    hout = c.applyBatch(host.pin_memory())
    assert torch.equal(hout.cpu().view(torch.int16) if dtype == np.uint16 else hout.cpu(), out.cpu().view(torch.int16) if dtype == np.uint16 else out.cpu())


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_whole_4k_frame(cv, dtype):
    rng = np.random.default_rng(13)
    # a smooth scene plus noise: the tiles' histograms differ, some bins clip
    yy, xx = np.mgrid[0:2160, 0:3840]
    hi = 255 if dtype == np.uint8 else 4095
    base = (np.sin(xx / 300.0) * np.cos(yy / 200.0) * 0.4 + 0.5) * hi
    src = np.clip(base + rng.normal(0, hi * 0.03, base.shape), 0, hi).astype(dtype)
    d = to_dev(src)
    got = to_host(run(cv, d, 40.0, (8, 8)))
    assert np.array_equal(got, R.clahe(src, 40.0, (8, 8)))
    if dtype == np.uint16:
        full = image(rng, 2160, 3840, dtype)
        got = to_host(run(cv, to_dev(full), 2.0, (8, 8)))
        assert np.array_equal(got, R.clahe(full, 2.0, (8, 8)))
