// bfmatch.hip -- cv::BFMatcher on the GPU: knnMatch / match / crossCheck / radiusMatch over CV_8U (NORM_HAMMING, NORM_HAMMING2) and CV_32F (NORM_L1, NORM_L2, NORM_L2SQR)
// descriptors, one train matrix or a collection with masks, single pairs and batches.  The definition is the project's own restatement (tests/bfmatch_restate.py,
// DESIGN 6.16); the arithmetic that can be wrong is in bfmatch_math.h and is compiled for the host by tests/hostemu/bfmatch_emu.cpp.
//
//   k_bf_hamming<DW, K>   the hot path: NORM_HAMMING on rows of 32 / 64 bytes (DW = 8 / 16 dwords) whose pointers and steps are multiples of 4, one train matrix, no mask.
//                         A lane owns one query in DW VGPRs; the workgroup walks the train rows in tiles of TILE_ROWS staged once into LDS, every lane reading the same
//                         address (a broadcast); per pair and dword one XOR and one popcount-accumulate; the K best keys in registers with compile-time indices.
//   k_bf_generic<K>       everything else: rows of any length / step / alignment, NORM_HAMMING2, masks, collections, CV_32F.  The same split and the same lists.
//   k_bf_merge            the partial lists of a query (one per part of the train set) merged by key, then either the final keys (crossCheck) or the DMatch rows.
//   k_bf_intersect        crossCheck: (q, s(q)) survives iff the reverse direction's best of s(q) is q.
//   k_bf_radius<FILL>     radiusMatch: count pass and fill pass; k_bf_scan the exclusive scan between them; k_bf_radius_sort orders one query's keys in LDS and emits.
// A batch is one sequence of launches: the pair is the grid's z.  Keys (distance, global train row) are unique, so the result depends neither on the tile, nor on the
// split, nor on any atomic.
// Limits (mi355cv_limit): "bfmatch_max_rows" = 2^24, "bfmatch_max_k" = 8, "bfmatch_max_row_bytes" = 2048, "bfmatch_max_images" = 64, "bfmatch_max_radius_row" = 4096;
// the geometry the tests aim at: "bfmatch_tile_rows" = 256, "bfmatch_split_rows" = 512.
#include "rt.h"
#include "bfmatch_math.h"
#include <algorithm>
#include <atomic>
#include <float.h>
#include <vector>

namespace {
using namespace mi355;
using bfm::Key;
using bfm::KList;

static_assert(bfm::MAX_ROWS == lim::BFMATCH_MAX_ROWS && bfm::MAX_K == lim::BFMATCH_MAX_K && bfm::MAX_ROW_BYTES == lim::BFMATCH_MAX_ROW_BYTES &&
              bfm::MAX_IMAGES == lim::BFMATCH_MAX_IMAGES && bfm::MAX_RADIUS_ROW == lim::BFMATCH_MAX_RADIUS_ROW && bfm::TILE_ROWS == lim::BFMATCH_TILE_ROWS &&
              bfm::SPLIT_ROWS == lim::BFMATCH_SPLIT_ROWS, "mi355cv_limit(\"bfmatch_*\")");
static_assert(sizeof(mi355cv_DMatch) == 16, "cv::DMatch");
static_assert(bfm::SPLIT_ROWS % bfm::TILE_ROWS == 0 && bfm::MAX_RADIUS_ROW * sizeof(Key) <= 32768, "tiles per part; the LDS sort");

constexpr int QB = 256;                   // queries (lanes) per workgroup

// one train matrix of a pair: `base` is its first row among the rows of the collection concatenated in list order
struct Seg { const uchar* t; size_t tstep; const uchar* mask; size_t mstep; uint32_t base; int rows; };
// one (query, train collection) pair of a batch; qoff: queries of the pairs before it (the dense index of the scratch planes)
struct Pair { const uchar* q; size_t qstep; mi355cv_DMatch* out; int* cnt; unsigned long long qoff; int nq, segBegin, nseg; uint32_t nt; };

__device__ __forceinline__ int partsOf(uint32_t nt, int splitRows) { return nt ? (int)((nt + (uint32_t)splitRows - 1) / (uint32_t)splitRows) : 1; }

template <int K> __device__ __forceinline__ void storeList(const KList<K>& l, Key* partial, unsigned long long q, int nsplit, int part)
{
    Key* p = partial + ((size_t)q * nsplit + part) * K;
#pragma unroll
    for (int i = 0; i < K; i++) p[i] = l.v[i];
}

template <int DW, int K>
__global__ __launch_bounds__(QB) void k_bf_hamming(const Pair* __restrict__ pairs, const Seg* __restrict__ segs, int splitRows, int nsplit, Key* __restrict__ partial)
{
    __shared__ uint32_t tile[bfm::TILE_ROWS * DW];
    const Pair P = pairs[blockIdx.z];
    const uint32_t r0 = blockIdx.y * (uint32_t)splitRows;
    if ((int)(blockIdx.x * QB) >= P.nq || (r0 >= P.nt && blockIdx.y)) return;               // uniform over the workgroup
    const Seg S = segs[P.segBegin];
    const int q = blockIdx.x * QB + threadIdx.x;
    const bool live = q < P.nq;
    uint32_t qd[DW];
    {
        const uint32_t* qp = (const uint32_t*)(P.q + (size_t)(live ? q : P.nq - 1) * P.qstep);
#pragma unroll
        for (int c = 0; c < DW; c++) qd[c] = qp[c];
    }
    KList<K> best;
    bfm::clear(best);
    const uint32_t r1 = min(P.nt, r0 + (uint32_t)splitRows);
    for (uint32_t tb = r0; tb < r1; tb += bfm::TILE_ROWS) {
        const int n = (int)min((uint32_t)bfm::TILE_ROWS, r1 - tb);
        __syncthreads();
        for (int i = threadIdx.x; i < n * DW; i += QB)
            tile[i] = *(const uint32_t*)(S.t + (size_t)(tb + (uint32_t)(i / DW)) * S.tstep + (size_t)(i % DW) * 4);
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < n; r++) {
            uint32_t d = 0;
#pragma unroll
            for (int c = 0; c < DW; c++) d += bfm::popc32(qd[c] ^ tile[r * DW + c]);
            bfm::insert(best, bfm::keyOf(d, tb + (uint32_t)r));
        }
    }
    if (live) storeList(best, partial, P.qoff + q, nsplit, blockIdx.y);
}

__device__ __forceinline__ Key pairKey(const uchar* q, const uchar* t, int len, int norm, uint32_t row)
{
    if (norm >= bfm::NORM_HAMMING) return bfm::keyOf(bfm::hammingBytes(q, t, len, norm == bfm::NORM_HAMMING2), row);
    return bfm::keyOfFloat(bfm::floatDistance((const float*)q, (const float*)t, len, norm), row);
}

// the key of (q, global row r), NO_KEY when the mask excludes the pair; si walks the collection's matrices as r ascends
__device__ __forceinline__ Key collectionKey(const Pair& P, const Seg* __restrict__ segs, int& si, int q, const uchar* qrow, uint32_t r, int len, int norm)
{
    while (r >= segs[si].base + (uint32_t)segs[si].rows) si++;                               // r < P.nt: ends inside the pair's matrices
    const Seg& S = segs[si];
    const uint32_t local = r - S.base;
    if (S.mask && !S.mask[(size_t)q * S.mstep + local]) return bfm::NO_KEY;
    return pairKey(qrow, S.t + (size_t)local * S.tstep, len, norm, r);
}

template <int K>
__global__ __launch_bounds__(QB) void k_bf_generic(const Pair* __restrict__ pairs, const Seg* __restrict__ segs, int len, int norm, int splitRows, int nsplit,
                                                   Key* __restrict__ partial)
{
    const Pair P = pairs[blockIdx.z];
    const uint32_t r0 = blockIdx.y * (uint32_t)splitRows;
    const int q = blockIdx.x * QB + threadIdx.x;
    if (q >= P.nq || (r0 >= P.nt && blockIdx.y)) return;
    const uchar* qrow = P.q + (size_t)q * P.qstep;
    KList<K> best;
    bfm::clear(best);
    const uint32_t r1 = min(P.nt, r0 + (uint32_t)splitRows);
    int si = P.segBegin;
    for (uint32_t r = r0; r < r1; r++) bfm::insert(best, collectionKey(P, segs, si, q, qrow, r, len, norm));
    storeList(best, partial, P.qoff + q, nsplit, blockIdx.y);
}

__device__ __forceinline__ void storeMatch(mi355cv_DMatch* o, int queryIdx, int trainIdx, int imgIdx, float distance)
{
    o->queryIdx = queryIdx; o->trainIdx = trainIdx; o->imgIdx = imgIdx; o->distance = distance;
}

// key -> DMatch; NO_KEY -> the padding record (cv::DMatch's default: -1, -1, -1, FLT_MAX)
__device__ __forceinline__ bool emitMatch(mi355cv_DMatch* o, const Pair& P, const Seg* __restrict__ segs, int q, Key key, bool isFloat)
{
    if (key == bfm::NO_KEY) { storeMatch(o, -1, -1, -1, FLT_MAX); return false; }
    const uint32_t r = bfm::keyRow(key);
    int si = P.segBegin;
    while (r >= segs[si].base + (uint32_t)segs[si].rows) si++;
    storeMatch(o, q, (int)(r - segs[si].base), si - P.segBegin, bfm::keyDistance(key, isFloat));
    return true;
}

// KP: length of a partial list.  finalKeys != null: the k best keys of every query go there (k per query); otherwise the DMatch plane and the counts are written.
__global__ __launch_bounds__(QB) void k_bf_merge(const Pair* __restrict__ pairs, const Seg* __restrict__ segs, const Key* __restrict__ partial, int KP, int splitRows,
                                                 int nsplit, int k, int isFloat, Key* __restrict__ finalKeys)
{
    const Pair P = pairs[blockIdx.z];
    const int q = blockIdx.x * QB + threadIdx.x;
    if (q >= P.nq) return;
    KList<bfm::MAX_K> best;
    bfm::clear(best);
    const int parts = partsOf(P.nt, splitRows);
    const Key* p = partial + (size_t)(P.qoff + q) * nsplit * KP;
    for (int s = 0; s < parts; s++)
        for (int i = 0; i < KP; i++) {
            const Key key = p[(size_t)s * KP + i];
            if (key == bfm::NO_KEY) break;                                                   // a list is ascending: nothing follows
            bfm::insert(best, key);
        }
    if (finalKeys) {
#pragma unroll
        for (int i = 0; i < bfm::MAX_K; i++) if (i < k) finalKeys[(size_t)(P.qoff + q) * k + i] = best.v[i];
        return;
    }
    int n = 0;
#pragma unroll
    for (int i = 0; i < bfm::MAX_K; i++) if (i < k) n += emitMatch(P.out + (size_t)q * k + i, P, segs, q, best.v[i], isFloat != 0) ? 1 : 0;
    P.cnt[q] = n;
}

// rev: the best key of every train row over the queries (low word = query row), the pairs' train rows dense in batch order (toff[pair] rows before it)
__global__ __launch_bounds__(QB) void k_bf_intersect(const Pair* __restrict__ pairs, const Seg* __restrict__ segs, const Key* __restrict__ fwd, const Key* __restrict__ rev,
                                                     const unsigned long long* __restrict__ toff, int isFloat)
{
    const Pair P = pairs[blockIdx.z];
    const int q = blockIdx.x * QB + threadIdx.x;
    if (q >= P.nq) return;
    Key key = fwd[P.qoff + q];
    if (key != bfm::NO_KEY && bfm::keyRow(rev[toff[blockIdx.z] + bfm::keyRow(key)]) != (uint32_t)q) key = bfm::NO_KEY;
    P.cnt[q] = emitMatch(P.out + q, P, segs, q, key, isFloat != 0) ? 1 : 0;
}

// radiusMatch, one lane per query over the whole collection.  FILL = false: counts[q] = eligible pairs with distance <= maxDist; FILL = true: their keys, in row
// order, from keys[off[q]]
template <bool FILL>
__global__ __launch_bounds__(QB) void k_bf_radius(const Pair* __restrict__ pairs, const Seg* __restrict__ segs, int len, int norm, float maxDist, uint32_t* __restrict__ counts,
                                                  const uint32_t* __restrict__ off, Key* __restrict__ keys)
{
    const Pair P = pairs[0];
    const int q = blockIdx.x * QB + threadIdx.x;
    if (q >= P.nq) return;
    const uchar* qrow = P.q + (size_t)q * P.qstep;
    const bool isFloat = norm < bfm::NORM_HAMMING;
    int si = P.segBegin;
    uint32_t n = 0;
    Key* out = FILL ? keys + off[q] : nullptr;
    for (uint32_t r = 0; r < P.nt; r++) {
        const Key key = collectionKey(P, segs, si, q, qrow, r, len, norm);
        if (key == bfm::NO_KEY || !(bfm::keyDistance(key, isFloat) <= maxDist)) continue;
        if (FILL) out[n] = key;
        n++;
    }
    if (!FILL) counts[q] = n;
}

// exclusive scan of n counts by one workgroup of 1024; tot[0] = the sum (saturated at 2^32 - 1), tot[1] = the largest count
__global__ __launch_bounds__(1024) void k_bf_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ off, int n, uint32_t* __restrict__ tot)
{
    __shared__ unsigned long long sh[1024];
    __shared__ uint32_t shMax[1024];
    unsigned long long carry = 0;
    uint32_t mx = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const uint32_t c = i < n ? counts[i] : 0;
        mx = max(mx, c);
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const unsigned long long v = threadIdx.x >= (unsigned)d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += v;
            __syncthreads();
        }
        const unsigned long long incl = carry + sh[threadIdx.x];
        if (i < n) off[i] = (uint32_t)min(incl - c, 0xffffffffull);
        carry += sh[1023];
        __syncthreads();
    }
    shMax[threadIdx.x] = mx;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) shMax[threadIdx.x] = max(shMax[threadIdx.x], shMax[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { tot[0] = (uint32_t)min(carry, 0xffffffffull); tot[1] = shMax[0]; }
}

// one workgroup per query: its counts[q] <= MAX_RADIUS_ROW keys sorted ascending in LDS (bitonic over the next power of two, padded with NO_KEY), then the
// matches that fall below `cap` in the flat list written
__global__ __launch_bounds__(QB) void k_bf_radius_sort(const Pair* __restrict__ pairs, const Seg* __restrict__ segs, const uint32_t* __restrict__ counts,
                                                       const uint32_t* __restrict__ off, const Key* __restrict__ keys, int isFloat, mi355cv_DMatch* __restrict__ out, uint32_t cap)
{
    __shared__ Key sh[bfm::MAX_RADIUS_ROW];
    const Pair P = pairs[0];
    const int q = blockIdx.x;
    const uint32_t n = counts[q], o = off[q];
    if (n == 0 || o >= cap) return;
    uint32_t m = 1;
    while (m < n) m <<= 1;
    for (uint32_t i = threadIdx.x; i < m; i += QB) sh[i] = i < n ? keys[o + i] : bfm::NO_KEY;
    __syncthreads();
    for (uint32_t size = 2; size <= m; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = threadIdx.x; i < (m >> 1); i += QB) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = !(lo & size);
                const Key a = sh[lo], b = sh[hi];
                if ((b < a) == up) { sh[lo] = b; sh[hi] = a; }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < n && o + i < cap; i += QB) emitMatch(out + o + i, P, segs, q, sh[i], isFloat != 0);
}

// ------------------------------------------------------------------------------------------------------------------------------------ host side
std::atomic<int> g_splitMode{-1};        // mi355cv_bfSetSplitMode: -1 / 1 the rule below, 0 never split (the A/B's other arm)

struct HostPair {
    const void* q; size_t qstep; int nq, nimg;
    const void* const* t; const size_t* tstep; const int* nt; const void* const* masks; const size_t* mstep;
    mi355cv_DMatch* out; int* cnt;
};

inline int esz(int type) { return type == MI355CV_32F ? 4 : 1; }

// refusals that need no device: the (type, norm) pairs served, the limits, the geometry of every matrix
int checkArgs(const HostPair* hp, int npairs, int len, int type, int normType, bool needOut)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!hp || npairs < 1 || npairs > 65535);
    if (type != MI355CV_8U && type != MI355CV_32F) return MI355_DECLINED("descriptors are neither CV_8UC1 nor CV_32FC1");
    if (type == MI355CV_8U && normType != bfm::NORM_HAMMING && normType != bfm::NORM_HAMMING2) return MI355_DECLINED("CV_8U descriptors are served with NORM_HAMMING / NORM_HAMMING2 only");
    if (type == MI355CV_32F && normType != bfm::NORM_L1 && normType != bfm::NORM_L2 && normType != bfm::NORM_L2SQR) return MI355_DECLINED("CV_32F descriptors are served with NORM_L1 / NORM_L2 / NORM_L2SQR only");
    MI355_DECLINE_IF(len < 1 || (long long)len * esz(type) > lim::BFMATCH_MAX_ROW_BYTES);
    const size_t rowBytes = (size_t)len * esz(type), al = (size_t)esz(type) - 1;
    for (int b = 0; b < npairs; b++) {
        const HostPair& h = hp[b];
        MI355_DECLINE_IF(h.nq < 0 || h.nq > lim::BFMATCH_MAX_ROWS);
        MI355_DECLINE_IF(h.nimg < 1 || h.nimg > lim::BFMATCH_MAX_IMAGES);
        MI355_DECLINE_IF(!h.t || !h.tstep || !h.nt);
        if (h.nq && (!h.q || h.qstep < rowBytes || (((size_t)h.q | h.qstep) & al))) return MI355_DECLINED("query: null, a step below the row, or CV_32F rows off a 4-byte boundary");
        if (needOut && h.nq && (!h.out || !h.cnt || (((size_t)h.out | (size_t)h.cnt) & 3))) return MI355_DECLINED("matches / counts: null or off a 4-byte boundary");
        long long rows = 0;
        for (int i = 0; i < h.nimg; i++) {
            MI355_DECLINE_IF(h.nt[i] < 0);
            rows += h.nt[i];
            if (h.nt[i] && (!h.t[i] || h.tstep[i] < rowBytes || (((size_t)h.t[i] | h.tstep[i]) & al))) return MI355_DECLINED("train: null, a step below the row, or CV_32F rows off a 4-byte boundary");
            if (h.masks && h.masks[i] && h.nt[i] && h.nq && (!h.mstep || h.mstep[i] < (size_t)h.nt[i])) return MI355_DECLINED("mask: a step below nt bytes");
        }
        MI355_DECLINE_IF(rows > lim::BFMATCH_MAX_ROWS);
    }
    return MI355CV_OK;
}

struct Tables {
    std::vector<Pair> pairs; std::vector<Seg> segs;
    const Pair* dPairs = nullptr; const Seg* dSegs = nullptr;
    unsigned long long queries = 0; int maxNq = 0; uint32_t maxNt = 0; bool fast = false;
};

// rows of 32 / 64 bytes on dword boundaries, one train matrix, no mask, NORM_HAMMING: k_bf_hamming
void classify(Tables& T, int len, int type, int normType)
{
    T.fast = type == MI355CV_8U && normType == bfm::NORM_HAMMING && (len == 32 || len == 64);
    T.queries = 0; T.maxNq = 0; T.maxNt = 0;
    for (auto& P : T.pairs) {
        P.qoff = T.queries; T.queries += (unsigned long long)P.nq;
        T.maxNq = std::max(T.maxNq, P.nq); T.maxNt = std::max(T.maxNt, P.nt);
        if (P.nseg != 1 || (((size_t)P.q | P.qstep) & 3)) T.fast = false;
        for (int i = 0; i < P.nseg; i++) { const Seg& S = T.segs[P.segBegin + i]; if (S.mask || (((size_t)S.t | S.tstep) & 3)) T.fast = false; }
    }
}

bool upload(Stager& stg, Tables& T)
{
    T.dPairs = (const Pair*)stg.param(T.pairs.data(), T.pairs.size() * sizeof(Pair));
    T.dSegs = (const Seg*)stg.param(T.segs.data(), std::max<size_t>(1, T.segs.size()) * sizeof(Seg));
    return T.dPairs && T.dSegs;
}

// stages every matrix of the batch (host rows into HBM, device rows in place) and lays out the device tables
bool stage(Stager& stg, const HostPair* hp, int npairs, int len, int type, int k, bool withOut, Tables& T)
{
    const size_t rowBytes = (size_t)len * esz(type);
    T.segs.reserve(npairs);
    for (int b = 0; b < npairs; b++) {
        const HostPair& h = hp[b];
        Pair P{};
        P.nq = h.nq; P.segBegin = (int)T.segs.size(); P.nseg = h.nimg;
        if (h.nq) { P.q = stg.in((const uchar*)h.q, h.qstep, rowBytes, h.nq, &P.qstep); if (!P.q) return false; }
        uint32_t base = 0;
        for (int i = 0; i < h.nimg; i++) {
            Seg S{};
            S.base = base; S.rows = h.nt[i]; base += (uint32_t)h.nt[i];
            if (S.rows) { S.t = stg.in((const uchar*)h.t[i], h.tstep[i], rowBytes, S.rows, &S.tstep); if (!S.t) return false; }
            if (h.masks && h.masks[i] && S.rows && h.nq) { S.mask = stg.in((const uchar*)h.masks[i], h.mstep[i], (size_t)S.rows, h.nq, &S.mstep); if (!S.mask) return false; }
            T.segs.push_back(S);
        }
        P.nt = base;
        if (withOut && h.nq) {
            size_t ds;
            P.out = (mi355cv_DMatch*)stg.out((uchar*)h.out, (size_t)h.nq * k * sizeof(mi355cv_DMatch), (size_t)h.nq * k * sizeof(mi355cv_DMatch), 1, &ds);
            P.cnt = (int*)stg.out((uchar*)h.cnt, (size_t)h.nq * sizeof(int), (size_t)h.nq * sizeof(int), 1, &ds);
            if (!P.out || !P.cnt) return false;
        }
        T.pairs.push_back(P);
    }
    return true;
}

// The split rule (profiles/bfmatch_split_ab.jsonl).  A lane owns a query and walks its part of the train rows serially, about 60 ns a row, so the walk
// is what a call waits for: one pass over 10 000 rows took 603 - 611 us for 64 ... 32 000 queries, parts of SPLIT_ROWS with k_bf_merge behind them 47 ... 185 us.
// The single pass never won, so the train rows are always divided: parts of SPLIT_ROWS, at most MAX_SPLITS of them and at most PARTIAL_BYTES of partial lists
// (beyond either a part grows by whole multiples of SPLIT_ROWS).  mi355cv_bfSetSplitMode(0) keeps the single pass reachable for that A/B.
constexpr size_t PARTIAL_BYTES = size_t(256) << 20;
int splitRowsFor(const Tables& T, int KP)
{
    if (g_splitMode.load(std::memory_order_relaxed) == 0) return (int)std::max<uint32_t>(T.maxNt, 1);
    const uint32_t unit = (uint32_t)bfm::SPLIT_ROWS;
    const unsigned long long fit = PARTIAL_BYTES / (std::max<unsigned long long>(T.queries, 1) * KP * sizeof(Key));
    const uint32_t parts = (uint32_t)std::max<unsigned long long>(1, std::min<unsigned long long>(bfm::MAX_SPLITS, fit));
    return (int)(unit * std::max<uint32_t>(1, (T.maxNt + unit * parts - 1) / (unit * parts)));
}

template <int DW> void launchHamming(int KP, dim3 grid, hipStream_t st, const Tables& T, int splitRows, int nsplit, Key* partial)
{
    switch (KP) {
    case 1: hipLaunchKernelGGL((k_bf_hamming<DW, 1>), grid, dim3(QB), 0, st, T.dPairs, T.dSegs, splitRows, nsplit, partial); break;
    case 2: hipLaunchKernelGGL((k_bf_hamming<DW, 2>), grid, dim3(QB), 0, st, T.dPairs, T.dSegs, splitRows, nsplit, partial); break;
    case 4: hipLaunchKernelGGL((k_bf_hamming<DW, 4>), grid, dim3(QB), 0, st, T.dPairs, T.dSegs, splitRows, nsplit, partial); break;
    default: hipLaunchKernelGGL((k_bf_hamming<DW, 8>), grid, dim3(QB), 0, st, T.dPairs, T.dSegs, splitRows, nsplit, partial); break;
    }
}

void launchGeneric(int KP, dim3 grid, hipStream_t st, const Tables& T, int len, int norm, int splitRows, int nsplit, Key* partial)
{
    switch (KP) {
    case 1: hipLaunchKernelGGL(k_bf_generic<1>, grid, dim3(QB), 0, st, T.dPairs, T.dSegs, len, norm, splitRows, nsplit, partial); break;
    case 2: hipLaunchKernelGGL(k_bf_generic<2>, grid, dim3(QB), 0, st, T.dPairs, T.dSegs, len, norm, splitRows, nsplit, partial); break;
    case 4: hipLaunchKernelGGL(k_bf_generic<4>, grid, dim3(QB), 0, st, T.dPairs, T.dSegs, len, norm, splitRows, nsplit, partial); break;
    default: hipLaunchKernelGGL(k_bf_generic<8>, grid, dim3(QB), 0, st, T.dPairs, T.dSegs, len, norm, splitRows, nsplit, partial); break;
    }
}

// distance kernel + merge over the uploaded tables: the DMatch planes of the pairs (finalKeys == null) or the k best keys of every query
bool knnLaunch(Stager& stg, const Tables& T, int len, int type, int normType, int k, Key* finalKeys)
{
    if (!T.queries) return true;
    const int KP = k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8;
    const int splitRows = splitRowsFor(T, KP), nsplit = std::max(1, (int)((T.maxNt + (uint32_t)splitRows - 1) / (uint32_t)splitRows));
    Key* partial = (Key*)stg.scratch((size_t)T.queries * nsplit * KP * sizeof(Key));
    if (!partial) return false;
    hipStream_t st = stream();
    const dim3 grid(divUp(T.maxNq, QB), nsplit, (unsigned)T.pairs.size());
    if (T.fast) { if (len == 32) launchHamming<8>(KP, grid, st, T, splitRows, nsplit, partial); else launchHamming<16>(KP, grid, st, T, splitRows, nsplit, partial); }
    else launchGeneric(KP, grid, st, T, len, normType, splitRows, nsplit, partial);
    hipLaunchKernelGGL(k_bf_merge, dim3(grid.x, 1, grid.z), dim3(QB), 0, st, T.dPairs, T.dSegs, partial, KP, splitRows, nsplit, k, type == MI355CV_32F ? 1 : 0, finalKeys);
    if (T.fast) noteKernel("k_bf_hamming<%d,%d> grid=%ux%ux%u x%d lds=%d, %d row(s) per part, k_bf_merge", len / 4, KP, grid.x, grid.y, grid.z, QB, bfm::TILE_ROWS * len, splitRows);
    else noteKernel("k_bf_generic<%d> grid=%ux%ux%u x%d, norm %d, %d element(s) per row, %d row(s) per part, k_bf_merge", KP, grid.x, grid.y, grid.z, QB, normType, len, splitRows);
    return true;
}

int runKnn(const char* entry, const HostPair* hp, int npairs, int len, int type, int normType, int k, int crossCheck)
{
    if (const int rc = checkArgs(hp, npairs, len, type, normType, true)) return rc;
    MI355_DECLINE_IF(k < 1 || k > lim::BFMATCH_MAX_K);
    if (crossCheck) {
        if (k != 1) return setError(MI355CV_ERROR_UNKNOWN, "%s: crossCheck is defined for k = 1 only", entry);
        for (int b = 0; b < npairs; b++) {
            if (hp[b].nimg > 1) return MI355_DECLINED("crossCheck with more than one train matrix");
            if (hp[b].masks && hp[b].masks[0]) return MI355_DECLINED("crossCheck together with a mask");
        }
    }
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    for (int b = 0; b < npairs; b++)
        if (hp[b].nq && ptrKind(hp[b].q) == PTR_HOST) MI355_DECLINE_IF(hostImageTooSmall(hp[b].q, (size_t)hp[b].nq * len, minPixels(HOST_HEAVY)));
    Tables T;
    if (!stage(stg, hp, npairs, len, type, k, true, T)) return MI355_DECLINED("staging failed");
    classify(T, len, type, normType);
    if (!upload(stg, T)) return MI355_DECLINED("no scratch");
    const int isFloat = type == MI355CV_32F ? 1 : 0;
    if (!crossCheck) {
        if (!knnLaunch(stg, T, len, type, normType, k, nullptr)) return MI355_DECLINED("no scratch");
        return stg.finish(entry);
    }
    if (!T.queries) return stg.finish(entry);
    // the reverse direction: the train rows as queries, the queries as the one train matrix; its key's low word is the query row
    Tables R;
    std::vector<unsigned long long> toff(npairs);
    for (int b = 0; b < npairs; b++) {
        const Pair& P = T.pairs[b]; const Seg& S = T.segs[P.segBegin];
        Pair Q{}; Seg Z{};
        Q.q = S.t; Q.qstep = S.tstep; Q.nq = S.rows; Q.segBegin = b; Q.nseg = 1; Q.nt = (uint32_t)P.nq;
        Z.t = P.q; Z.tstep = P.qstep; Z.rows = P.nq;
        R.pairs.push_back(Q); R.segs.push_back(Z);
    }
    classify(R, len, type, normType);
    for (int b = 0; b < npairs; b++) toff[b] = R.pairs[b].qoff;
    const unsigned long long* dToff = (const unsigned long long*)stg.param(toff.data(), toff.size() * sizeof(unsigned long long));
    Key* fwd = (Key*)stg.scratch((size_t)T.queries * sizeof(Key));
    Key* rev = (Key*)stg.scratch((size_t)std::max<unsigned long long>(1, R.queries) * sizeof(Key));
    if (!upload(stg, R) || !dToff || !fwd || !rev) return MI355_DECLINED("no scratch");
    if (!knnLaunch(stg, R, len, type, normType, 1, rev) || !knnLaunch(stg, T, len, type, normType, 1, fwd)) return MI355_DECLINED("no scratch");
    hipLaunchKernelGGL(k_bf_intersect, dim3(divUp(T.maxNq, QB), 1, (unsigned)npairs), dim3(QB), 0, stream(), T.dPairs, T.dSegs, fwd, rev, dToff, isFloat);
    return stg.finish(entry);
}

// declines of mi355cv_bfRadiusMatch: the reason is recorded, the entry answers -1
#define BF_RADIUS_DECLINE_IF(...) do { if (__VA_ARGS__) { (void)MI355_DECLINED(#__VA_ARGS__); return -1; } } while (0)

} // namespace

extern "C" {

MI355CV_API int mi355cv_bfKnnMatch(const void* query, size_t query_step, int nq, int len, int type, const void* const* train, const size_t* train_step, const int* train_rows,
                                   const void* const* masks, const size_t* mask_step, int nimg, int normType, int k, int crossCheck, mi355cv_DMatch* matches, int* counts)
{
    mi355::EntryGuard entry_(__func__);
    const HostPair h{query, query_step, nq, nimg, train, train_step, train_rows, masks, mask_step, matches, counts};
    return runKnn("bfKnnMatch", &h, 1, len, type, normType, k, crossCheck);
}

MI355CV_API int mi355cv_bfKnnMatchBatch(const void* const* query, const size_t* query_step, const int* nq, const void* const* train, const size_t* train_step,
                                        const int* train_rows, int npairs, int len, int type, int normType, int k, int crossCheck, mi355cv_DMatch* const* matches,
                                        int* const* counts)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(npairs < 1 || npairs > 65535 || !query || !query_step || !nq || !train || !train_step || !train_rows || !matches || !counts);
    std::vector<HostPair> hp(npairs);
    for (int b = 0; b < npairs; b++) hp[b] = HostPair{query[b], query_step[b], nq[b], 1, train + b, train_step + b, train_rows + b, nullptr, nullptr, matches[b], counts[b]};
    return runKnn("bfKnnMatchBatch", hp.data(), npairs, len, type, normType, k, crossCheck);
}

MI355CV_API int mi355cv_bfRadiusMatch(const void* query, size_t query_step, int nq, int len, int type, const void* const* train, const size_t* train_step, const int* train_rows,
                                      const void* const* masks, const size_t* mask_step, int nimg, int normType, float maxDistance, mi355cv_DMatch* matches, int capacity,
                                      int* counts)
{
    mi355::EntryGuard entry_(__func__);
    const char* entry = "bfRadiusMatch";
    const HostPair h{query, query_step, nq, nimg, train, train_step, train_rows, masks, mask_step, matches, counts};
    if (checkArgs(&h, 1, len, type, normType, false)) return -1;
    BF_RADIUS_DECLINE_IF(capacity < 0 || (capacity > 0 && (!matches || ((size_t)matches & 3))) || (nq > 0 && (!counts || ((size_t)counts & 3))));
    if (nq == 0) return 0;
    Stager stg;
    BF_RADIUS_DECLINE_IF(!ensureDevice());
    if (ptrKind(query) == PTR_HOST) BF_RADIUS_DECLINE_IF(hostImageTooSmall(query, (size_t)nq * len, minPixels(HOST_HEAVY)));
    Tables T;
    if (!stage(stg, &h, 1, len, type, 1, false, T)) { (void)MI355_DECLINED("staging failed"); return -1; }
    classify(T, len, type, normType);
    size_t ds;
    uint32_t* dCounts = (uint32_t*)stg.out((uchar*)counts, (size_t)nq * sizeof(int), (size_t)nq * sizeof(int), 1, &ds);
    uint32_t* off = (uint32_t*)stg.scratch((size_t)nq * sizeof(uint32_t));
    uint32_t* dTot = (uint32_t*)stg.scratch(16);
    uint32_t* tot = (uint32_t*)stg.pinned(16);
    if (!upload(stg, T) || !dCounts || !off || !dTot || !tot) { (void)MI355_DECLINED("no scratch"); return -1; }
    hipStream_t st = stream();
    const dim3 grid(divUp(nq, QB));
    hipLaunchKernelGGL(k_bf_radius<false>, grid, dim3(QB), 0, st, T.dPairs, T.dSegs, len, normType, maxDistance, dCounts, (const uint32_t*)nullptr, (Key*)nullptr);
    hipLaunchKernelGGL(k_bf_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)dCounts, off, nq, dTot);
    // the call's one host synchronisation: the total and the longest list
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tot, dTot, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    const uint32_t total = tot[0], longest = tot[1];
    BF_RADIUS_DECLINE_IF(longest > (uint32_t)lim::BFMATCH_MAX_RADIUS_ROW);
    BF_RADIUS_DECLINE_IF(total > 0x7fffffffu);
    const uint32_t take = std::min<uint32_t>(total, (uint32_t)capacity);
    if (take) {
        Key* keys = (Key*)stg.scratch((size_t)total * sizeof(Key));
        mi355cv_DMatch* out = (mi355cv_DMatch*)stg.out((uchar*)matches, (size_t)take * sizeof(mi355cv_DMatch), (size_t)take * sizeof(mi355cv_DMatch), 1, &ds);
        if (!keys || !out) { (void)MI355_DECLINED("no scratch"); return -1; }
        hipLaunchKernelGGL(k_bf_radius<true>, grid, dim3(QB), 0, st, T.dPairs, T.dSegs, len, normType, maxDistance, (uint32_t*)nullptr, (const uint32_t*)off, keys);
        hipLaunchKernelGGL(k_bf_radius_sort, dim3(nq), dim3(QB), 0, st, T.dPairs, T.dSegs, (const uint32_t*)dCounts, (const uint32_t*)off, (const Key*)keys,
                           type == MI355CV_32F ? 1 : 0, out, take);
    }
    noteKernel("k_bf_radius grid=%u x%d, norm %d, %d element(s) per row, k_bf_scan + k_bf_radius<fill> + k_bf_radius_sort, %u match(es)", grid.x, QB, normType, len, total);
    return stg.finish(entry) == MI355CV_OK ? (int)total : -2;
}

MI355CV_API int mi355cv_bfSetSplitMode(int mode)
{
    if (mode < -1 || mode > 1) return MI355CV_ERROR_UNKNOWN;
    g_splitMode.store(mode, std::memory_order_relaxed);
    return MI355CV_OK;
}

} // extern "C"
