"""Host-side mirror of the reference's FAST corner detector (modules/features2d/src/fast.cpp), of cv::ORB (modules/features2d/src/orb.cpp;
SURVEY §8 f3 "features2d detectors") and of cv::BFMatcher (mi355cv_bf*).

cv::FAST -> the whole detector on the GPU in one call (mi355cv_FAST); FAST_dense / FAST_NMS are the two features2d HAL hooks
(modules/features2d/src/hal_replacement.hpp:75, :87) the reference's own hal_FAST (fast.cpp:438-493) is assembled from."""
import ctypes

import numpy as np

from . import _lib
from .core import Img, bind_stream, empty_like_kind, CV_8U

try:
    import torch
except Exception:                                        # numpy-only use
    torch = None

__all__ = ["FAST", "FAST_dense", "FAST_NMS", "FAST_hooks", "FAST_TYPE_5_8", "FAST_TYPE_7_12", "FAST_TYPE_9_16",
           "ORB", "ORB_create", "ORB_HARRIS_SCORE", "ORB_FAST_SCORE", "KEYPOINT_DTYPE",
           "BFMatcher", "BFMatcher_create", "DMATCH_DTYPE", "NORM_L1", "NORM_L2", "NORM_L2SQR", "NORM_HAMMING", "NORM_HAMMING2", "dmatch_records"]

L = _lib.lib
FAST_TYPE_5_8, FAST_TYPE_7_12, FAST_TYPE_9_16 = 0, 1, 2


def _vp(p):
    return ctypes.c_void_p(p)


def FAST(image, threshold, nonmaxSuppression=True, type=FAST_TYPE_9_16):
    """cv::FAST (fast.cpp:496): keypoints as an (n, 3) float32 array of (x, y, response) in the reference's order.  The other fields of
    cv::KeyPoint are constants there (size 7, angle -1, octave 0, class_id -1)."""
    s = Img(image)
    if s.depth != CV_8U or s.cn != 1:
        raise ValueError("FAST: CV_8UC1 image expected")
    bind_stream(s)
    cap = max(1 << 14, (s.w * s.h) >> 6)               # one keypoint per 64 pixels fits without a second call on ordinary frames
    while True:
        out = np.empty((cap, 3), np.float32)
        n = L.mi355cv_FAST(_vp(s.ptr), s.step, s.w, s.h, int(threshold), 1 if nonmaxSuppression else 0, int(type), out.ctypes.data, cap)
        if n == -1:
            raise NotImplementedError("mi355cv_FAST: NOT_IMPLEMENTED for these arguments (%s); no CPU fallback in opencv_amd" % L.mi355cv_lastError().decode())
        if n < 0:
            raise _lib.Mi355cvError("mi355cv_FAST failed: " + L.mi355cv_lastError().decode())
        if n <= cap:
            return out[:n].copy()
        cap = n


def FAST_dense(image, type=FAST_TYPE_9_16, dst=None):
    """cv_hal_FAST_dense: the score image (largest t + 1 for which the pixel is a corner at threshold t)"""
    s = Img(image)
    out = dst if dst is not None else empty_like_kind(image, s.h, s.w, 1, CV_8U)
    d = Img(out)
    bind_stream(s, d)
    _lib.check(L.mi355cv_FAST_dense(_vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h, int(type)), "FAST_dense")
    return out


def FAST_NMS(scores, dst=None):
    """cv_hal_FAST_NMS: 3x3 non-maximum suppression of a score image"""
    s = Img(scores)
    out = dst if dst is not None else empty_like_kind(scores, s.h, s.w, 1, CV_8U)
    d = Img(out)
    bind_stream(s, d)
    _lib.check(L.mi355cv_FAST_NMS(_vp(s.ptr), s.step, _vp(d.ptr), d.step, s.w, s.h), "FAST_NMS")
    return out


def FAST_hooks(image, threshold, nonmaxSuppression=True, type=FAST_TYPE_9_16):
    """cv::FAST the way the reference assembles it from the two hooks (hal_FAST, fast.cpp:438-493): dense scores, optional suppression, then the
    raster scan of the score image on the host"""
    if threshold > 20:
        raise NotImplementedError("hal_FAST serves thresholds <= 20 only (fast.cpp:440)")
    sc = FAST_dense(image, type)
    fin = FAST_NMS(sc) if nonmaxSuppression else sc
    a = fin.cpu().numpy() if hasattr(fin, "cpu") else np.asarray(fin)
    thr = 1 if (threshold == 0 and nonmaxSuppression) else threshold
    h, w = a.shape
    if h <= 6 or w <= 6:
        return np.zeros((0, 3), np.float32)
    inner = a[3:h - 3, 3:w - 3]
    ys, xs = np.nonzero(inner > thr)
    resp = (inner[ys, xs].astype(np.float32) - 1) if nonmaxSuppression else np.zeros(len(xs), np.float32)
    return np.stack([xs.astype(np.float32) + 3, ys.astype(np.float32) + 3, resp], axis=1)


# ---------------------------------------------------------------------------------------------------- cv::ORB (features2d.hpp:425-520, orb.cpp)
ORB_HARRIS_SCORE, ORB_FAST_SCORE = 0, 1
# cv::KeyPoint (core/types.hpp:777): pt.x, pt.y, size, angle, response, octave, class_id -- 28 bytes, the record mi355cv_KeyPoint declares
KEYPOINT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32),
                           ("octave", np.int32), ("class_id", np.int32)])


class _OrbParams(ctypes.Structure):
    _fields_ = [("nfeatures", ctypes.c_int), ("scaleFactor", ctypes.c_double), ("nlevels", ctypes.c_int), ("edgeThreshold", ctypes.c_int),
                ("firstLevel", ctypes.c_int), ("WTA_K", ctypes.c_int), ("scoreType", ctypes.c_int), ("patchSize", ctypes.c_int), ("fastThreshold", ctypes.c_int)]


class ORB:
    """cv::ORB (ORB_Impl, orb.cpp:655-760): the parameter set of ORB::create with its getters / setters, detect / compute / detectAndCompute.
    Keypoints are numpy records of KEYPOINT_DTYPE in the reference's order, descriptors an (n, 32) uint8 array (descriptorSize() = 32, CV_8U,
    NORM_HAMMING for WTA_K = 2, NORM_HAMMING2 otherwise).  The whole call runs on the GPU but for the two culls of the candidate lists."""

    kBytes = 32

    def __init__(self, nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=ORB_HARRIS_SCORE, patchSize=31, fastThreshold=20):
        if firstLevel < 0:
            raise ValueError("ORB: firstLevel >= 0 (orb.cpp:1261 CV_Assert)")
        self._p = dict(nfeatures=int(nfeatures), scaleFactor=float(np.float32(scaleFactor)), nlevels=int(nlevels), edgeThreshold=int(edgeThreshold), firstLevel=int(firstLevel),
                       WTA_K=int(WTA_K), scoreType=int(scoreType), patchSize=int(patchSize), fastThreshold=int(fastThreshold))

    # getters / setters under the reference's names (features2d.hpp:470-510)
    def descriptorSize(self): return self.kBytes
    def descriptorType(self): return CV_8U
    def defaultNorm(self): return 6 if self._p["WTA_K"] == 2 else 7                    # NORM_HAMMING / NORM_HAMMING2 (orb.cpp:700-709)
    def getDefaultName(self): return "Feature2D.ORB"

    def __getattr__(self, name):
        if name.startswith("get") and name[3:4].isupper():
            key = {"MaxFeatures": "nfeatures", "NLevels": "nlevels"}.get(name[3:], name[3].lower() + name[4:] if name[3:] != "WTA_K" else "WTA_K")
            if key in self._p:
                return lambda: self._p[key]
        if name.startswith("set") and name[3:4].isupper():
            key = {"MaxFeatures": "nfeatures", "NLevels": "nlevels"}.get(name[3:], name[3].lower() + name[4:] if name[3:] != "WTA_K" else "WTA_K")
            if key in self._p:
                def setter(v):
                    if key == "firstLevel" and v < 0:
                        raise ValueError("ORB: firstLevel >= 0")
                    self._p[key] = float(v) if key == "scaleFactor" else int(v)         # setScaleFactor(double) keeps the double; ORB::create rounds to float (orb.cpp:660, :1262)
                return setter
        raise AttributeError(name)

    def _gray(self, image):
        s = Img(image)
        if s.depth == CV_8U and s.cn in (3, 4):                                       # orb.cpp:1040-1041
            from .imgproc import cvtColor, COLOR_BGR2GRAY, COLOR_BGRA2GRAY
            image = cvtColor(image, COLOR_BGR2GRAY if s.cn == 3 else COLOR_BGRA2GRAY)
            s = Img(image)
        if s.depth != CV_8U or s.cn != 1:
            raise ValueError("ORB: CV_8UC1 (or 8-bit BGR / BGRA) image expected")
        return image, s

    def detectAndCompute(self, image, mask=None, keypoints=None, useProvidedKeypoints=False, descriptors=True):
        """ORB_Impl::detectAndCompute (orb.cpp:1012): -> (keypoints, descriptors or None)"""
        if self._p["patchSize"] < 2:
            raise ValueError("ORB: patchSize >= 2 (orb.cpp:1018 CV_Assert)")
        if (useProvidedKeypoints and not descriptors) or image is None or np.prod(np.shape(image)) == 0:      # orb.cpp:1023
            return (np.zeros(0, KEYPOINT_DTYPE) if keypoints is None else np.asarray(keypoints, KEYPOINT_DTYPE)), None
        image, s = self._gray(image)
        m = None
        if mask is not None:
            m = Img(mask)
            if m.depth != CV_8U or m.cn != 1 or (m.w, m.h) != (s.w, s.h):
                raise ValueError("ORB: the mask is a CV_8UC1 image of the image's size")
            if m.device != s.device:
                raise ValueError("ORB: image and mask live in the same kind of memory")
            bind_stream(s, m)
        else:
            bind_stream(s)
        prm = _OrbParams(**self._p)
        n_in = 0
        if useProvidedKeypoints:
            kin = np.ascontiguousarray(np.asarray(keypoints, KEYPOINT_DTYPE))
            n_in = len(kin)
        cap = max(n_in, self._p["nfeatures"] + 64, 1024)
        while True:
            kps = np.zeros(cap, KEYPOINT_DTYPE)
            if n_in:
                kps[:n_in] = kin
            desc = np.zeros((cap, 32), np.uint8) if descriptors else None
            n = L.mi355cv_ORB_detectAndCompute(_vp(s.ptr), s.step, s.w, s.h, _vp(m.ptr) if m is not None else None, m.step if m is not None else 0, ctypes.byref(prm),
                                                1 if useProvidedKeypoints else 0, kps.ctypes.data, n_in, cap, desc.ctypes.data if descriptors else None, 32)
            if n == -1:
                L.mi355cv_noteDecline(b"ORB_detectAndCompute")
                raise NotImplementedError("mi355cv_ORB_detectAndCompute: NOT_IMPLEMENTED for these arguments (%s); no CPU fallback in opencv_amd" % L.mi355cv_lastError().decode())
            if n < 0:
                raise _lib.Mi355cvError("mi355cv_ORB_detectAndCompute failed: " + L.mi355cv_lastError().decode())
            if n <= cap:
                return kps[:n].copy(), (desc[:n].copy() if descriptors else None)
            cap = n

    def detect(self, image, mask=None):
        """Feature2D::detect"""
        return self.detectAndCompute(image, mask, descriptors=False)[0]

    def compute(self, image, keypoints):
        """Feature2D::compute: keypoints too close to the border are dropped, the rest regrouped by octave; -> (keypoints, descriptors)"""
        return self.detectAndCompute(image, None, keypoints, useProvidedKeypoints=True)


def ORB_create(nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=ORB_HARRIS_SCORE, patchSize=31, fastThreshold=20):
    """cv::ORB::create (orb.cpp:1258-1265)"""
    return ORB(nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize, fastThreshold)


# ---------------------------------------------------------------------------------------------------- cv::BFMatcher (features2d.hpp, matchers.cpp)
NORM_L1, NORM_L2, NORM_L2SQR, NORM_HAMMING, NORM_HAMMING2 = 2, 4, 5, 6, 7           # core/base.hpp NormTypes
# cv::DMatch (core/types.hpp): queryIdx, trainIdx, imgIdx, distance -- 16 bytes, the record mi355cv_DMatch declares
DMATCH_DTYPE = np.dtype([("queryIdx", np.int32), ("trainIdx", np.int32), ("imgIdx", np.int32), ("distance", np.float32)])


def dmatch_records(t):
    """an (..., 4) int32 device tensor of matches (what BFMatcher returns for device-resident descriptors) as numpy records of DMATCH_DTYPE"""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(DMATCH_DTYPE).reshape(a.shape[:-1])


def _desc(a, what):
    if torch is not None and isinstance(a, torch.Tensor):
        if a.dim() == 2 and a.shape[0] == 0:
            a = a.new_empty((0, a.shape[1]))             # no row: whatever strides the empty view carries say nothing
    elif np.ndim(a) == 2 and np.shape(a)[0] == 0:
        s = Img(np.zeros((1, np.shape(a)[1]), np.asarray(a).dtype))      # (numpy reports no usable strides for an array without rows)
        s.h = 0
        return s
    s = Img(a)
    if s.cn != 1 or getattr(s.obj, "ndim", 2) != 2:
        raise ValueError("BFMatcher: %s descriptors are a 2-D one-channel matrix, one descriptor per row" % what)
    return s


class _PtrList:
    """the (pointer, step, rows) arrays of a list of matrices as the C ABI takes them"""

    def __init__(self, imgs):
        n = len(imgs)
        self.ptr = (ctypes.c_void_p * n)(*[(m.ptr or None) if m is not None else None for m in imgs])
        self.step = (ctypes.c_size_t * n)(*[m.step if m is not None else 0 for m in imgs])
        self.rows = (ctypes.c_int * n)(*[m.h if m is not None else 0 for m in imgs])


class BFMatcher:
    """cv::BFMatcher(normType, crossCheck): brute-force matching of descriptor rows on the GPU.  CV_8U rows with NORM_HAMMING / NORM_HAMMING2, CV_32F rows with NORM_L1 /
    NORM_L2 / NORM_L2SQR; anything else raises NotImplementedError.  Candidates of a query are ordered by (distance, imgIdx, trainIdx), so every result is fully
    determined.  Descriptors are numpy arrays or torch device tensors.  numpy queries give numpy records of DMATCH_DTYPE: match -> one array, knnMatch /
    radiusMatch -> a list of arrays, one per query.  Device queries give device tensors and nothing is downloaded: match / knnMatch -> (matches, counts), matches an
    (nq, 4) / (nq, k, 4) int32 tensor whose rows are DMatch records (dmatch_records() views them; the distance is the float32 in the fourth word) padded with
    trainIdx = -1, counts the (nq,) int32 number of valid entries; radiusMatch -> (matches (total, 4), counts (nq,)), the lists one after another."""

    def __init__(self, normType=NORM_L2, crossCheck=False):
        self.normType, self.crossCheck = int(normType), bool(crossCheck)
        self._train = []

    # DescriptorMatcher's collection
    def add(self, descriptors):
        self._train.extend(descriptors if isinstance(descriptors, (list, tuple)) else [descriptors])

    def clear(self): self._train = []
    def empty(self): return not self._train
    def getTrainDescriptors(self): return list(self._train)
    def isMaskSupported(self): return True
    def train(self): pass

    def _collection(self, train, mask, masks):
        if train is not None:
            trains, ms = [train], [mask]
        else:
            if not self._train:
                raise ValueError("BFMatcher: no train descriptors (pass a matrix or add() a collection)")
            trains = self._train
            ms = list(masks) if masks is not None else [None] * len(trains)
            if len(ms) != len(trains):
                raise ValueError("BFMatcher: one mask (or None) per train matrix")
        return trains, ms

    def _prepare(self, query, trains, ms):
        q = _desc(query, "query")
        ts = [_desc(t, "train") for t in trains]
        for t in ts:
            if t.depth != q.depth or (t.h and q.h and t.w != q.w):
                raise ValueError("BFMatcher: query and train descriptors share type and length")
        mi = []
        for t, m in zip(ts, ms):
            if m is None:
                mi.append(None)
                continue
            m = Img(m)
            if m.depth != CV_8U or m.cn != 1 or (m.h, m.w) != (q.h, t.h):
                raise ValueError("BFMatcher: a mask is a CV_8UC1 matrix of nq x nt")
            mi.append(m)
        bind_stream(q, *ts)
        length = q.w if q.h else (ts[0].w if ts else 0)
        return q, ts, mi, max(int(length), 1)

    @staticmethod
    def _alloc(q, shape):
        """matches (int32 words of DMatch records) and counts of the query's kind"""
        if q.device:
            return torch.empty(shape + (4,), dtype=torch.int32, device=q.obj.device), torch.empty(shape[:1], dtype=torch.int32, device=q.obj.device)
        return np.empty(shape, DMATCH_DTYPE), np.empty(shape[:1], np.int32)

    @staticmethod
    def _p(a):
        return _vp((a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) or None)

    def _knn(self, query, trains, ms, k):
        k = int(k)
        if k < 1:
            raise ValueError("BFMatcher: k >= 1")
        if self.crossCheck and k != 1:
            raise ValueError("BFMatcher: crossCheck is defined for k = 1 only")
        q, ts, mi, length = self._prepare(query, trains, ms)
        out, cnt = self._alloc(q, (q.h, k))
        T, M = _PtrList(ts), _PtrList(mi)
        _lib.check(L.mi355cv_bfKnnMatch(_vp(q.ptr or None), q.step, q.h, length, q.depth, T.ptr, T.step, T.rows, M.ptr if any(m is not None for m in mi) else None, M.step, len(ts),
                                        self.normType, k, 1 if self.crossCheck else 0, self._p(out), self._p(cnt)), "bfKnnMatch")
        return out, cnt

    @staticmethod
    def _lists(out, cnt, compact):
        return [out[i, :c].copy() for i, c in enumerate(cnt) if c or not compact]

    def knnMatch(self, queryDescriptors, trainDescriptors=None, k=1, mask=None, masks=None, compactResult=False):
        """DescriptorMatcher::knnMatch: the first min(k, eligible) candidates of every query in (distance, imgIdx, trainIdx) order.  knnMatch(query, train, k, mask) or, on
        the add()-ed collection, knnMatch(query, k=k, masks=[...]).  compactResult drops the empty lists (numpy results)."""
        if isinstance(trainDescriptors, (int, np.integer)):
            trainDescriptors, k = None, trainDescriptors
        trains, ms = self._collection(trainDescriptors, mask, masks)
        out, cnt = self._knn(queryDescriptors, trains, ms, k)
        return (out, cnt) if hasattr(out, "data_ptr") else self._lists(out, cnt, compactResult)

    def match(self, queryDescriptors, trainDescriptors=None, mask=None, masks=None):
        """DescriptorMatcher::match: knnMatch(1) flattened; queries without an eligible candidate do not appear (numpy results)"""
        trains, ms = self._collection(trainDescriptors, mask, masks)
        out, cnt = self._knn(queryDescriptors, trains, ms, 1)
        return (out[:, 0], cnt) if hasattr(out, "data_ptr") else out[cnt > 0, 0].copy()

    def radiusMatch(self, queryDescriptors, trainDescriptors=None, maxDistance=None, mask=None, masks=None, compactResult=False):
        """DescriptorMatcher::radiusMatch: every candidate with distance <= maxDistance, per query in (distance, imgIdx, trainIdx) order"""
        if maxDistance is None and isinstance(trainDescriptors, (int, float, np.integer, np.floating)):
            trainDescriptors, maxDistance = None, trainDescriptors
        if maxDistance is None:
            raise ValueError("BFMatcher: radiusMatch needs maxDistance")
        if self.crossCheck:
            raise NotImplementedError("BFMatcher: crossCheck with radiusMatch is not served; no CPU fallback in opencv_amd")
        trains, ms = self._collection(trainDescriptors, mask, masks)
        q, ts, mi, length = self._prepare(queryDescriptors, trains, ms)
        T, M = _PtrList(ts), _PtrList(mi)
        cap = max(4 * q.h, 1024)
        while True:
            out, _ = self._alloc(q, (cap,))
            cnt = self._alloc(q, (q.h,))[1]
            n = L.mi355cv_bfRadiusMatch(_vp(q.ptr or None), q.step, q.h, length, q.depth, T.ptr, T.step, T.rows, M.ptr if any(m is not None for m in mi) else None, M.step, len(ts),
                                        self.normType, float(maxDistance), self._p(out), cap, self._p(cnt))
            if n == -1:
                L.mi355cv_noteDecline(b"bfRadiusMatch")
                raise NotImplementedError("mi355cv_bfRadiusMatch: NOT_IMPLEMENTED for these arguments (%s); no CPU fallback in opencv_amd" % L.mi355cv_lastError().decode())
            if n < 0:
                raise _lib.Mi355cvError("mi355cv_bfRadiusMatch failed: " + L.mi355cv_lastError().decode())
            if n <= cap:
                break
            cap = n
        if hasattr(out, "data_ptr"):
            return out[:n], cnt
        ends = np.cumsum(cnt)
        return [out[e - c:e].copy() for c, e in zip(cnt, ends) if c or not compactResult]

    def knnMatchBatch(self, queries, trains, k=1, compactResult=False):
        """B independent (query_b, train_b) pairs with their own row counts in one sequence of launches (frame b against frame b + 1); exactly the results of B knnMatch calls"""
        k = int(k)
        if k < 1:
            raise ValueError("BFMatcher: k >= 1")
        if self.crossCheck and k != 1:
            raise ValueError("BFMatcher: crossCheck is defined for k = 1 only")
        if len(queries) != len(trains) or not len(queries):
            raise ValueError("BFMatcher: as many train matrices as queries, at least one")
        qs, ts = [_desc(a, "query") for a in queries], [_desc(a, "train") for a in trains]
        lengths = {m.w for m in qs + ts if m.h}
        if len(lengths) > 1 or len({m.depth for m in qs + ts}) != 1:
            raise ValueError("BFMatcher: all descriptors of a batch share type and length")
        bind_stream(*qs, *ts)
        res = [self._alloc(q, (q.h, k)) for q in qs]
        Q, T = _PtrList(qs), _PtrList(ts)
        n = len(qs)
        outs = (ctypes.c_void_p * n)(*[self._p(o).value for o, _ in res])
        cnts = (ctypes.c_void_p * n)(*[self._p(c).value for _, c in res])
        _lib.check(L.mi355cv_bfKnnMatchBatch(Q.ptr, Q.step, Q.rows, T.ptr, T.step, T.rows, n, max(int(next(iter(lengths), 1)), 1), qs[0].depth, self.normType, k,
                                             1 if self.crossCheck else 0, outs, cnts), "bfKnnMatchBatch")
        return [(o, c) if hasattr(o, "data_ptr") else self._lists(o, c, compactResult) for o, c in res]

    def matchBatch(self, queries, trains):
        """knnMatchBatch(1) flattened per pair"""
        k1 = self.knnMatchBatch(queries, trains, 1, compactResult=True)
        return [(r[0][:, 0], r[1]) if isinstance(r, tuple) else (np.concatenate(r) if r else np.zeros(0, DMATCH_DTYPE)) for r in k1]


def BFMatcher_create(normType=NORM_L2, crossCheck=False):
    """cv::BFMatcher::create"""
    return BFMatcher(normType, crossCheck)
