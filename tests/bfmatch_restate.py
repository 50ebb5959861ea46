"""cv::BFMatcher as this project serves it, restated twice: plain loops (`*_loops`, the definition read aloud) and vectorised numpy (`*_np`, fast enough
for the GPU suite's shapes).  tests/test_bfmatch_cpu.py holds the two against each other and against opencv_amd/csrc/bfmatch_math.h compiled for the host;
tests/test_bfmatch_gpu.py holds the kernels against `*_np`, bit for bit.

  distance   NORM_HAMMING (6): sum over bytes of popcount(q ^ t).  NORM_HAMMING2 (7): the non-zero 2-bit groups of q ^ t.  NORM_L1 (2): s = fl(s + fl(|fl(q - t)|)),
             NORM_L2SQR (5): x = fl(q - t), s = fl(s + fl(x * x)), elements ascending, every operation rounded to float32.  NORM_L2 (4): the correctly rounded float32
             square root of L2SQR.  Always reported as float32.
  eligible   the distance is not NaN and the pair's mask byte (if that train matrix has a mask) is non-zero.
  order      (distance, imgIdx, trainIdx) ascending; distances compare as float32.
  knnMatch   the first min(k, eligible) candidates per query.  crossCheck (k = 1, one train matrix, no mask): (q, s(q)) stays iff b(s(q)) = q, s(q) the train row with the
             smallest (distance, trainIdx), b(t) the query with the smallest (distance, queryIdx).
  radius     all eligible candidates with distance <= maxDistance, in the same order.
Results: a plane of DMATCH records (nq, k) padded with (-1, -1, -1, FLT_MAX) plus counts, as the C ABI writes them; radius: a list of record arrays per query."""
import numpy as np

NORM_L1, NORM_L2, NORM_L2SQR, NORM_HAMMING, NORM_HAMMING2 = 2, 4, 5, 6, 7
DMATCH = np.dtype([("queryIdx", np.int32), ("trainIdx", np.int32), ("imgIdx", np.int32), ("distance", np.float32)])
PAD = np.array((-1, -1, -1, np.finfo(np.float32).max), DMATCH)
_POP = np.array([bin(v).count("1") for v in range(256)], np.int64)
_POP2 = np.array([sum(1 for g in range(4) if (v >> (2 * g)) & 3) for v in range(256)], np.int64)


# ------------------------------------------------------------------------------------------------------------------------------------ loops
def distance_loops(q, t, norm):
    """one pair of rows -> np.float32"""
    if norm in (NORM_HAMMING, NORM_HAMMING2):
        s = 0
        for a, b in zip(q, t):
            x = int(a) ^ int(b)
            if norm == NORM_HAMMING:
                s += bin(x).count("1")
            else:
                s += sum(1 for g in range(4) if (x >> (2 * g)) & 3)
        return np.float32(s)
    s = np.float32(0)
    with np.errstate(all="ignore"):
        for a, b in zip(q, t):
            x = np.float32(a) - np.float32(b)
            s = np.float32(s + (np.abs(x) if norm == NORM_L1 else np.float32(x * x)))
        return np.float32(np.sqrt(s)) if norm == NORM_L2 else s


def _candidates_loops(Q, trains, masks, norm, qi):
    c = []
    for img, T in enumerate(trains):
        for ti in range(len(T)):
            if masks is not None and masks[img] is not None and not masks[img][qi, ti]:
                continue
            d = distance_loops(Q[qi], T[ti], norm)
            if d != d:
                continue
            c.append((float(d), img, ti))
    c.sort()
    return c


def _plane(lists, nq, k):
    out = np.full((nq, k), PAD, DMATCH)
    cnt = np.zeros(nq, np.int32)
    for qi, c in enumerate(lists):
        cnt[qi] = len(c)
        for j, (d, img, ti) in enumerate(c):
            out[qi, j] = (qi, ti, img, d)
    return out, cnt


def knn_loops(Q, trains, masks, norm, k):
    return _plane([_candidates_loops(Q, trains, masks, norm, qi)[:k] for qi in range(len(Q))], len(Q), k)


def radius_loops(Q, trains, masks, norm, max_distance):
    res = []
    for qi in range(len(Q)):
        c = [m for m in _candidates_loops(Q, trains, masks, norm, qi) if np.float32(m[0]) <= np.float32(max_distance)]
        res.append(np.array([(qi, ti, img, d) for d, img, ti in c], DMATCH))
    return res


def cross_loops(Q, T, norm):
    fwd = [_candidates_loops(Q, [T], None, norm, qi)[:1] for qi in range(len(Q))]
    rev = [_candidates_loops(T, [Q], None, norm, ti)[:1] for ti in range(len(T))]
    return _plane([f if f and rev[f[0][2]] and rev[f[0][2]][0][2] == qi else [] for qi, f in enumerate(fwd)], len(Q), 1)


# ------------------------------------------------------------------------------------------------------------------------------------ numpy
def distances_np(Q, T, norm):
    """(nq, nt) float32"""
    Q, T = np.asarray(Q), np.asarray(T)
    nq, nt, n = len(Q), len(T), (Q.shape[1] if len(Q) else (T.shape[1] if len(T) else 0))
    if norm in (NORM_HAMMING, NORM_HAMMING2):
        tab = _POP if norm == NORM_HAMMING else _POP2
        s = np.zeros((nq, nt), np.int64)
        for i in range(n):
            s += tab[Q[:, None, i] ^ T[None, :, i]]
        return s.astype(np.float32)
    s = np.zeros((nq, nt), np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            x = Q[:, None, i].astype(np.float32) - T[None, :, i].astype(np.float32)
            s = s + (np.abs(x) if norm == NORM_L1 else x * x)
            assert s.dtype == np.float32 and x.dtype == np.float32
        return np.sqrt(s) if norm == NORM_L2 else s


def _all_np(Q, trains, masks, norm):
    """distances (nq, NT) over the concatenated collection, eligibility, and the (imgIdx, trainIdx) of every global row"""
    D = np.concatenate([distances_np(Q, T, norm) for T in trains], axis=1) if trains else np.zeros((len(Q), 0), np.float32)
    E = ~np.isnan(D)
    col = 0
    for i, T in enumerate(trains):
        if masks is not None and masks[i] is not None:
            E[:, col:col + len(T)] &= np.asarray(masks[i]) != 0
        col += len(T)
    img = np.concatenate([np.full(len(T), i, np.int32) for i, T in enumerate(trains)]) if trains else np.zeros(0, np.int32)
    loc = np.concatenate([np.arange(len(T), dtype=np.int32) for T in trains]) if trains else np.zeros(0, np.int32)
    return D, E, img, loc


def _ordered(D, E, qi):
    """the eligible global rows of query qi in (distance, global row) order: a stable sort on the distance keeps the rows ascending inside a tie"""
    rows = np.nonzero(E[qi])[0]
    return rows[np.argsort(D[qi, rows], kind="stable")]


def knn_np(Q, trains, masks, norm, k):
    D, E, img, loc = _all_np(Q, trains, masks, norm)
    out = np.full((len(Q), k), PAD, DMATCH)
    cnt = np.zeros(len(Q), np.int32)
    for qi in range(len(Q)):
        r = _ordered(D, E, qi)[:k]
        cnt[qi] = len(r)
        out["queryIdx"][qi, :len(r)] = qi
        out["trainIdx"][qi, :len(r)] = loc[r]
        out["imgIdx"][qi, :len(r)] = img[r]
        out["distance"][qi, :len(r)] = D[qi, r]
    return out, cnt


def radius_np(Q, trains, masks, norm, max_distance):
    D, E, img, loc = _all_np(Q, trains, masks, norm)
    with np.errstate(invalid="ignore"):
        E = E & (D <= np.float32(max_distance))
    res = []
    for qi in range(len(Q)):
        r = _ordered(D, E, qi)
        m = np.zeros(len(r), DMATCH)
        m["queryIdx"], m["trainIdx"], m["imgIdx"], m["distance"] = qi, loc[r], img[r], D[qi, r]
        res.append(m)
    return res


def cross_np(Q, T, norm):
    fwd, fc = knn_np(Q, [T], None, norm, 1)
    rev, rc = knn_np(T, [Q], None, norm, 1)
    out = np.full((len(Q), 1), PAD, DMATCH)
    cnt = np.zeros(len(Q), np.int32)
    for qi in range(len(Q)):
        if fc[qi] and rc[fwd["trainIdx"][qi, 0]] and rev["trainIdx"][fwd["trainIdx"][qi, 0], 0] == qi:
            out[qi, 0] = fwd[qi, 0]
            cnt[qi] = 1
    return out, cnt


# ------------------------------------------------------------------------------------------------------------------------------------ data
def tie_heavy(rng, n, nbytes, pool=5, bits=3, dup=0.3):
    """n binary descriptors of nbytes drawn from a pool of `pool` rows, each with at most `bits` of the row's first bits flipped and a share `dup` of exact copies:
    equal distances are the rule, not the exception"""
    base = rng.integers(0, 256, (pool, nbytes), dtype=np.uint8)
    rows = base[rng.integers(0, pool, n)].copy()
    for i in range(n):
        if rng.random() < dup:
            continue
        for _ in range(int(rng.integers(0, bits + 1))):
            b = int(rng.integers(0, min(8 * nbytes, 16)))
            rows[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return rows


def tie_heavy_float(rng, n, length, pool=5, dup=0.3):
    """the float counterpart: small integers around a pool of rows, so sums are exact and distances tie"""
    base = rng.integers(-4, 5, (pool, length)).astype(np.float32)
    rows = base[rng.integers(0, pool, n)].copy()
    for i in range(n):
        if rng.random() >= dup:
            rows[i, int(rng.integers(0, length))] += np.float32(rng.integers(-2, 3))
    return rows
