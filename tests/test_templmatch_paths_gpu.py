"""One row per served path of the matcher's path chain (templmatch.hip, struct MatchCall) and of cv::integral's three routes (integral.hip): the single-image hook and the
batch entry walk the SAME chain, so a batch of 3 device-resident frames -- views with padding rows between them -- must give, frame for frame and bit for bit, what the hook
gives (the frame index enters only the addressing, and no path accumulates with atomics), and mi355cv_lastKernel must name the same kernel after both calls.  (What each
kernel computes is pinned against the restatement in test_templmatch_gpu.py; this file pins WHICH path serves, from the smallest shapes that select it: the matrix-core
paths want >= 4096 results.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3
U8, F32 = torch.uint8, torch.float32
TM_SQDIFF, TM_CCORR, TM_CCORR_NORMED = 0, 2, 3


@pytest.fixture(scope="module")
def cv():
    import opencv_amd
    assert torch.cuda.is_available()
    return opencv_amd


def tensor(shape, dtype, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    if dtype == F32:
        return torch.rand(shape, dtype=F32, device="cuda", generator=g)
    return torch.randint(0, 256, shape, dtype=U8, device="cuda", generator=g)


def frames(dtype, w, h, cn, seed):
    """[N, h, w(, cn)] as views of a tensor with 3 padding rows after every frame"""
    return tensor((N, h + 3, w) + ((cn,) if cn > 1 else ()), dtype, seed)[:, :h]


def path_name(cv):
    """the note up to its launch geometry (which holds the frame count): kernel name with its template arguments, or the sentence of a path made of several kernels"""
    return cv._lib.lib.mi355cv_lastKernel().decode().split(" grid=")[0]


# (id, what the note begins with, dtype, channels, template (w, h), image (w, h), method)
MATCH_ROWS = [
    ("ring-sums-in-kernel", "k_ccorr_ring_i8<2,true>", U8, 1, (16, 66), (80, 129), TM_CCORR_NORMED),       # th >= 66 and rows of whole dwords: 65 x 64 results
    ("ring-separate-sums", "k_ccorr_ring_i8<2,false>", U8, 1, (8, 8), (71, 71), TM_CCORR_NORMED),          # 64 x 64 results
    ("mfma-narrow-image", "k_ccorr_mfma_i8<1>", U8, 1, (1, 1), (3, 1366), TM_CCORR_NORMED),                 # images narrower than 4 pixels: 3 x 1366 = 4098 results
    ("direct-integrals", "k_ccorr_direct", U8, 1, (8, 8), (70, 71), TM_CCORR_NORMED),                       # 63 x 64 = 4032 results: below the matrix paths
    ("direct-integrals-32fc3", "k_ccorr_direct", F32, 3, (8, 8), (70, 71), TM_CCORR_NORMED),
    ("direct-ccorr", "k_ccorr_direct", U8, 1, (8, 8), (70, 71), TM_CCORR),                                  # no integral images
    ("blocks-8u", "matchTemplate 129x4 as 2 blocks of <= 128 x 128", U8, 1, (129, 4), (192, 67), TM_CCORR_NORMED),   # blocks of 128 and 1 columns
    ("planes-8uc3", "matchTemplate 8x8 as 3 per-channel planes", U8, 3, (8, 8), (71, 71), TM_CCORR_NORMED),
    ("bf16-three-products", "k_ccorr_bf16<3> x3 ", F32, 1, (8, 8), (71, 71), TM_CCORR),
    ("bf16-four-products", "k_ccorr_bf16<3> x4 ", F32, 1, (8, 8), (71, 71), TM_SQDIFF),
    ("bf16-blocks", "k_ccorr_bf16<2> x3 (hi*hi + hi*mid + mid*hi) x 2 block(s)", F32, 1, (129, 4), (192, 67), TM_CCORR),
]


def other_family_first(cv):
    """the note is the calling thread's last one: a call of another family first, so that a path that writes none cannot pass on a note left behind"""
    cv.medianBlur(tensor((40, 48), U8, 1), 3)
    assert path_name(cv).startswith("k_median")


@pytest.mark.parametrize("prefix,dtype,cn,tsize,isize,method", [pytest.param(*r[1:], id=r[0]) for r in MATCH_ROWS])
def test_batch_and_hook_share_the_path(cv, prefix, dtype, cn, tsize, isize, method):
    (tw, th), (iw, ih) = tsize, isize
    fr = frames(dtype, iw, ih, cn, seed=iw + th)
    tpl = tensor((th, tw) + ((cn,) if cn > 1 else ()), dtype, seed=tw)
    other_family_first(cv)
    got = cv.matchTemplateBatch(fr, tpl, method)
    name_batch = path_name(cv)
    other_family_first(cv)
    singles = [cv.matchTemplate(f, tpl, method) for f in reversed(fr)][::-1]
    name_single = path_name(cv)
    for f, one in enumerate(singles):
        assert got[f].shape == one.shape == (ih - th + 1, iw - tw + 1) and torch.equal(got[f], one), f
    assert name_single.startswith(prefix), name_single
    assert name_batch == name_single, (name_batch, name_single)


def test_mask_on_byte_planes(cv):
    """CV_8U under a binary CV_8U mask, a method without a mean: three i8 correlations per channel (the hook has no batch twin)"""
    img, tpl = tensor((71, 71), U8, 5), tensor((8, 8), U8, 6)
    mask = (tensor((8, 8), U8, 7) > 127).to(U8)
    other_family_first(cv)
    got = cv.matchTemplate(img, tpl, TM_CCORR_NORMED, mask=mask)
    assert tuple(got.shape) == (64, 64) and bool(torch.isfinite(got).all())
    assert path_name(cv).startswith("matchTemplateMask on byte planes: 3 i8 correlation(s) per channel"), path_name(cv)


# (id, what the note begins with, dtype, channels, sdepth)
INTEGRAL_ROWS = [
    ("ordered", "k_iseq_rows", F32, 1, 5),                     # CV_32F -> CV_32F: the bits depend on the order of the additions
    ("tiled", "k_integral_tiles<int,false>", U8, 1, 4),        # CV_8UC1 -> CV_32S
    ("rows-and-columns", "k_integral_rows<int>", U8, 3, 4),    # CV_8UC3 -> CV_32S
]


@pytest.mark.parametrize("prefix,dtype,cn,sdepth", [pytest.param(*r[1:], id=r[0]) for r in INTEGRAL_ROWS])
def test_integral_routes(cv, prefix, dtype, cn, sdepth):
    fr = frames(dtype, 50, 40, cn, seed=cn)
    other_family_first(cv)
    singles = [cv.integral(f, sdepth=sdepth) for f in reversed(fr)][::-1]
    name_single = path_name(cv)
    for f, one in enumerate(singles):
        assert tuple(one.shape[:2]) == (41, 51) and int(one[0].abs().sum()) == 0 and int(one[:, 0].abs().sum()) == 0, f
    if prefix.startswith("k_integral_tiles"):                 # the one route with a batch entry
        other_family_first(cv)
        got = cv.integralBatch(fr)
        name_batch = path_name(cv)
        for f, one in enumerate(singles):
            assert torch.equal(got[f], one), f
        assert name_batch == name_single, (name_batch, name_single)
    assert name_single.startswith(prefix), name_single
