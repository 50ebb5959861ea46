"""One row per served path of the three path chains of filter.hip / box.hip (sepServe, filterServe, boxServe): the single-image hook and the batch entry walk the
SAME chain, so a batch of 3 device-resident frames -- views with padding rows between them -- must give, frame for frame, what the hook gives, and
mi355cv_lastKernel must name the same kernel after both calls.  (What each kernel computes is pinned against the oracle in test_filters_gpu.py; which
geometries the batch entries cut differently in test_batch_gpu.py / test_batch_cuts_gpu.py.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W, W_RAGGED = 3, 40, 48, 50        # W: rows of whole 16-byte chunks; W_RAGGED: a ragged last chunk, and more than one 64-element block of the generic kernels with cn > 1


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    return opencv_amd


def frames(dtype, w, cn=1, seed=0):
    """[N, H, w(, cn)] as views of a tensor with 3 padding rows after every frame"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    shape = (N, H + 3, w) + ((cn,) if cn > 1 else ())
    if dtype == torch.float32:
        t = torch.rand(shape, dtype=torch.float32, device="cuda", generator=g) * 255 - 64
    elif dtype == torch.uint16:
        t = torch.randint(-32768, 32768, shape, dtype=torch.int16, device="cuda", generator=g).view(torch.uint16)
    else:
        t = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    return t[:, :H]


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def kernel_name(cv):
    note = cv._lib.lib.mi355cv_lastKernel().decode()
    return note.replace("(", " ").split(" ")[0]


K3 = [0.25, 0.5, 0.25]
K5F = [0.1, 0.5, 0.2, 0.05, 0.15]
K35 = list(np.hanning(37)[1:-1] / np.hanning(37)[1:-1].sum())
SHARPEN = np.array([[0, -1, 0], [-1, 5, -1], [0, -1, 0]], np.float32)
RNG = np.random.default_rng(7)
K7x7 = (RNG.uniform(-3, 10, (7, 7)) / 170).astype(np.float32)
K3x3F = (RNG.uniform(-3, 10, (3, 3)) / 31.5).astype(np.float32)
K2x3 = (RNG.uniform(-3, 10, (3, 2)) / 21).astype(np.float32)        # 2 wide, 3 high: fewer than 9 taps, what neither the rolling kernels nor the tile take

# (id, prefix of the kernel's name or None where the path writes no note, dtype, width, channels, single-image call, batch call)
ROWS = [
    # ---- sepServe
    ("sep-deriv16", "k_sep_roll<Deriv16", torch.uint8, W, 1,
     lambda cv, f: cv.Sobel(f, cv.CV_16S, 1, 0, 3), lambda cv, b: cv.SobelBatch(b, cv.CV_16S, 1, 0, 3)),
    ("sep-fix8u", "k_sep_roll<SepFix8U", torch.uint8, W, 1,
     lambda cv, f: cv.sepFilter2D(f, -1, K3, K3), lambda cv, b: cv.sepFilter2DBatch(b, -1, K3, K3)),
    ("sep-float", "k_sep_roll<SepF32", torch.uint8, W, 1,
     lambda cv, f: cv.sepFilter2D(f, cv.CV_32F, K5F, K5F), lambda cv, b: cv.sepFilter2DBatch(b, cv.CV_32F, K5F, K5F)),
    ("sep-f32", "k_sep_roll<SepF32F", torch.float32, W, 1,
     lambda cv, f: cv.sepFilter2D(f, -1, K5F, K5F), lambda cv, b: cv.sepFilter2DBatch(b, -1, K5F, K5F)),
    ("sep-f16", "k_sep_roll<SepF16<16U>", torch.uint16, W, 1,
     lambda cv, f: cv.sepFilter2D(f, -1, K3, K3), lambda cv, b: cv.sepFilter2DBatch(b, -1, K3, K3)),
    ("sep-ring-uncentred", "k_seplong<", torch.uint8, W_RAGGED, 1,
     lambda cv, f: cv.sepFilter2D(f, cv.CV_32F, K5F, K3, delta=0.5), lambda cv, b: cv.sepFilter2DBatch(b, cv.CV_32F, K5F, K3, delta=0.5)),
    ("sep-ring-big", "k_seplong<", torch.uint8, W_RAGGED, 1,
     lambda cv, f: cv.sepFilter2D(f, -1, K35, K35), lambda cv, b: cv.sepFilter2DBatch(b, -1, K35, K35)),
    ("sep-generic33", "k_sepfilter_generic<33>", torch.uint8, W_RAGGED, 5,
     lambda cv, f: cv.sepFilter2D(f, -1, K3, K3), lambda cv, b: cv.sepFilter2DBatch(b, -1, K3, K3)),
    ("sep-generic64", "k_sepfilter_generic64", torch.uint8, W_RAGGED, 1,
     lambda cv, f: cv.sepFilter2D(f, cv.CV_64F, K5F, K3), lambda cv, b: cv.sepFilter2DBatch(b, cv.CV_64F, K5F, K3)),
    # ---- filterServe
    ("filter-roll-f32", "k_filter2d_roll_f32<3>", torch.float32, W, 1,
     lambda cv, f: cv.filter2D(f, -1, K3x3F), lambda cv, b: cv.filter2DBatch(b, -1, K3x3F)),
    ("filter-tile", "k_filter2d_tile<", torch.uint8, W_RAGGED, 1,
     lambda cv, f: cv.filter2D(f, -1, K7x7), lambda cv, b: cv.filter2DBatch(b, -1, K7x7)),
    ("filter-generic", "k_filter2d_generic", torch.uint8, W_RAGGED, 1,
     lambda cv, f: cv.filter2D(f, -1, K2x3, delta=1.5), lambda cv, b: cv.filter2DBatch(b, -1, K2x3, delta=1.5)),
    ("filter-roll-8u", None, torch.uint8, W, 1,                          # k_filter2d_roll on CV_8U writes no note: values only
     lambda cv, f: cv.filter2D(f, -1, SHARPEN), lambda cv, b: cv.filter2DBatch(b, -1, SHARPEN)),
    # ---- boxServe
    ("box-roll", "k_sep_roll<BoxU8", torch.uint8, W, 1,
     lambda cv, f: cv.boxFilter(f, -1, (5, 5)), lambda cv, b: cv.boxFilterBatch(b, -1, (5, 5))),
    ("box-roll-f32", "k_sep_roll<BoxF32", torch.float32, W, 1,
     lambda cv, f: cv.boxFilter(f, -1, (5, 5)), lambda cv, b: cv.boxFilterBatch(b, -1, (5, 5))),
    ("box-sepmx", "k_sepmx<", torch.uint8, W_RAGGED, 1,
     lambda cv, f: cv.boxFilter(f, -1, (25, 25)), lambda cv, b: cv.boxFilterBatch(b, -1, (25, 25))),
    ("box-twopass", "k_box_rows", torch.uint16, W_RAGGED, 1,
     lambda cv, f: cv.boxFilter(f, -1, (21, 21)), lambda cv, b: cv.boxFilterBatch(b, -1, (21, 21))),
    ("box-generic", "k_box_generic", torch.uint16, W_RAGGED, 1,
     lambda cv, f: cv.boxFilter(f, -1, (3, 3)), lambda cv, b: cv.boxFilterBatch(b, -1, (3, 3))),
]


@pytest.mark.parametrize("prefix,dtype,w,cn,single,batch", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_batch_and_hook_share_the_chain(cv, prefix, dtype, w, cn, single, batch):
    fr = frames(dtype, w, cn, seed=w + cn)
    # the note is the calling thread's last one: a call of another family first, so that a path that writes none cannot pass on the note its twin left behind
    cv.medianBlur(frames(torch.uint8, W)[0], 3)
    assert kernel_name(cv).startswith("k_median")
    got = batch(cv, fr)
    name_batch = kernel_name(cv)
    singles = [single(cv, f) for f in reversed(fr)][::-1]               # frame 0 last: its note is the one compared
    name_single = kernel_name(cv)
    for f, one in enumerate(singles):
        assert got[f].shape == one.shape and got[f].dtype == one.dtype and torch.equal(bits(got[f]), bits(one)), f
    if prefix is not None:
        assert name_single.startswith(prefix), name_single
        assert name_batch == name_single, (name_batch, name_single)
