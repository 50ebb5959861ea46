// houghcircles.hip -- cv::HoughCircles, method HOUGH_GRADIENT (HoughCirclesGradient, imgproc/src/hough.cpp; the reference has no HAL hook for it) on CV_8UC1.
// Every line of arithmetic is in houghcircles_math.h.  Votes and radius histograms are integer counts and every float is computed per element, so every result is
// a pure function of the input whatever order the atomics land in.  The reference was not available to pin the semantics; they are restated in
// tests/houghcircles_restate.py (plain loops and an independent numpy form) and the kernels are held against that bit for bit.
//
//   edges            the two 3 x 3 Sobel planes (mi355cv_sobel, CV_16S, BORDER_REPLICATE) and stages 2-5 of mi355cv_canny (canny.h) with low = max(1, canny / 2),
//                    high = canny, L1 magnitude; dx, dy and edges stay in scratch.
//   k_hc_rowcount    a wave per row: the ballot compaction of hough_points.h over the pixels with edges != 0 and (vx, vy) != (0, 0) -- the pixels that vote; for the
//                    library's own edge stage every edge pixel is one (low >= 1 makes |vx| + |vy| > 1 on an edge), a caller's edge map need not be.
//   k_hc_rowscan     the exclusive prefix of the row counts, one workgroup per frame: rows[y] .. rows[y + 1] is row y's segment of the point list.
//   k_hc_points      a wave per row appends its points to its segment, in column order: no atomic, and the list itself is a pure function of the input.
//   k_hc_vote        lanes over (point, sign, block of STEP_BLOCK steps), integer atomicAdd into the accumulator in HBM; serves every parameter set.
//   k_hc_vote_tile   (mi355cv_houghCirclesSetKernel(1) only) a workgroup owns a TILE x TILE tile of the accumulator in LDS (16 KiB), walks the row segments within reach of the tile's footprint, votes the
//                    steps that land in its tile with LDS atomics and writes the tile with plain stores (every cell once: no memset).
//   k_hc_maxima      a thread per cell: the five-way predicate of hough_math.h; a wave appends its candidates behind one atomic add on the frame's counter.
//   sort             rocPRIM's radix sort (gftt_sort.hip) descending on the COMPLEMENT of (~votes << 32) | b, the unused tail being zeros.
//   k_hc_radius      a workgroup per centre: bins in LDS up to LDS_BINS = 40960 bins (160 KiB, the LDS of a CU: one workgroup of four waves a CU, one wave per SIMD;
//                    a histogram takes the bytes it needs, so up to 16384 bins two workgroups share a CU, up to 8192 four; the default maxRadius of a 4K frame has
//                    38400 bins and fits), longer histograms in a slab of HBM per workgroup with the same arithmetic.  The points of rows cy +- maxRadius
//                    stream in with 16-byte loads; wave 0 then walks the scan, skipping runs of empty bins 64 at a time with a ballot.  The circle's key goes back
//                    into the candidate list, its radius into the centre's own accumulator cell (the votes are in the key by then).
//   sort             again, on (~maxCount << 32) | b.
//   k_hc_suppress    one wave per frame walks the circles in order, the lanes test a candidate against the kept list (LDS, then the output rows), a ballot decides.
// Measurements, the arm crossing and the stage furthest from the copy rate: DESIGN 6.22 (tools/houghcircles_bench.py).
#include "rt.h"
#include "canny.h"
#include "hough_points.h"
#include "houghcircles_math.h"
#include <algorithm>
#include <atomic>
#include <cmath>

using namespace mi355;
namespace hc = houghcircles;

extern "C" MI355CV_API int mi355cv_sobel(const uchar* src_data, size_t src_step, uchar* dst_data, size_t dst_step, int width, int height,
        int src_depth, int dst_depth, int cn, int margin_left, int margin_top, int margin_right, int margin_bottom,
        int dx, int dy, int ksize, double scale, double delta, int border_type);

namespace mi355 {
size_t sortKeysDescTemp(unsigned n);                                                                             // gftt_sort.hip (rocPRIM)
bool sortKeysDesc(void* temp, size_t bytes, const unsigned long long* in, unsigned long long* out, unsigned n, hipStream_t st);
}

namespace {

using hc::Params;

std::atomic<int> g_arm{-1};                                                  // mi355cv_houghCirclesSetKernel: -1 the library chooses (k_hc_vote), 0 k_hc_vote, 1 k_hc_vote_tile
constexpr int KEEP_LDS = 4096;                                               // kept circles k_hc_suppress holds in LDS (32 KiB); later ones are read from the output rows
constexpr int CTR = 4;                                                       // counters per frame: [0] centres, [1] circles written

// the planes of nf frames: edges CV_8UC1, dx / dy CV_16S; steps and frame strides in BYTES
struct Planes { const uchar* edges; size_t estep, eframe; const uchar* dx; const uchar* dy; size_t gstep, gframe; };

__device__ __forceinline__ void gradAt(const Planes& pl, int f, int x, int y, int* vx, int* vy)
{
    const size_t off = (size_t)f * pl.gframe + (size_t)y * pl.gstep + (size_t)x * 2;
    *vx = *reinterpret_cast<const short*>(pl.dx + off);
    *vy = *reinterpret_cast<const short*>(pl.dy + off);
}

// the four edge bytes of columns x .. x + 3 with the ones that do not vote (gradient (0, 0)) cleared
__device__ __forceinline__ uint32_t votingPix4(const Planes& pl, int f, int x, int y, int w)
{
    uint32_t v = loadPix4(pl.edges + (size_t)f * pl.eframe + (size_t)y * pl.estep, x, w);
    if (!v) return 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if ((v >> (8 * k)) & 0xffu) {                                        // a non-zero byte lies inside the row
            int vx, vy;
            gradAt(pl, f, x + k, y, &vx, &vy);
            if (!(vx | vy)) v &= ~(0xffu << (8 * k));
        }
    return v;
}

// rows: h + 1 words per frame; here rows[y] = the number of voting pixels of row y
__global__ __launch_bounds__(256) void k_hc_rowcount(Planes pl, int w, int h, uint32_t* __restrict__ rows, size_t rframe)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    if (y >= h) return;                                                      // the whole wave
    uint32_t n = 0, pre;
    for (int x0 = 0; x0 < w; x0 += 256) n += ballotPoints4(votingPix4(pl, f, x0 + 4 * lane, y, w), lane, &pre);
    if (lane == 0) rows[(size_t)f * rframe + y] = n;
}

// in place: rows[y] = the points of the rows above y, rows[h] = all of them
__global__ __launch_bounds__(256) void k_hc_rowscan(uint32_t* __restrict__ rows, size_t rframe, int h)
{
    __shared__ uint32_t part[256];
    uint32_t* R = rows + (size_t)blockIdx.x * rframe;
    const int per = (h + 255) / 256, y0 = min(h, (int)threadIdx.x * per), y1 = min(h, y0 + per);
    uint32_t sum = 0;
    for (int y = y0; y < y1; y++) sum += R[y];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                                     // inclusive scan of the 256 partial sums
        const uint32_t add = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (int y = y0; y < y1; y++) { const uint32_t c = R[y]; R[y] = run; run += c; }
    if (threadIdx.x == 255) R[h] = part[255];
}

__global__ __launch_bounds__(256) void k_hc_points(Planes pl, int w, int h, const uint32_t* __restrict__ rows, size_t rframe, uint32_t* __restrict__ pts, size_t pframe)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
    if (y >= h) return;                                                      // the whole wave
    uint32_t base = rows[(size_t)f * rframe + y];
    uint32_t* P = pts + (size_t)f * pframe;
    for (int x0 = 0; x0 < w; x0 += 256) {
        const int x = x0 + 4 * lane;
        const uint32_t v = votingPix4(pl, f, x, y, w);
        uint32_t pre;
        const uint32_t total = ballotPoints4(v, lane, &pre);
        storePoints4(v, x, y, P + base + pre);                               // base + total <= rows[y + 1] <= w * h
        base += total;
    }
}

// items: (point, sign, block of STEP_BLOCK steps); neighbouring lanes hold the blocks of one ray, so a wave's atomics spread along rays of a few points
__global__ __launch_bounds__(256) void k_hc_vote(Planes pl, Params p, const uint32_t* __restrict__ rows, size_t rframe, const uint32_t* __restrict__ pts, size_t pframe,
                                                 int* __restrict__ acc, size_t aframe)
{
    const int f = blockIdx.y;
    const uint32_t np = rows[(size_t)f * rframe + p.h];
    const int nblk = (p.maxRadius - p.minRadius) / hc::STEP_BLOCK + 1;
    const uint64_t per = 2 * (uint64_t)nblk, items = np * per;
    const uint32_t* P = pts + (size_t)f * pframe;
    int* A = acc + (size_t)f * aframe;
    for (uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (uint64_t)gridDim.x * 256) {
        const uint32_t i = (uint32_t)(it / per), rem = (uint32_t)(it - i * per);
        const int sg = (rem & 1) ? -1 : 1, r0 = p.minRadius + (int)(rem >> 1) * hc::STEP_BLOCK;
        const uint32_t pt = P[i];
        const int x = hough::pointX(pt), y = hough::pointY(pt);
        int vx, vy;
        gradAt(pl, f, x, y, &vx, &vy);
        hc::Ray ray;
        if (!hc::makeRay(x, y, vx, vy, p.idp, &ray) || !hc::rayStarts(ray, sg, p.minRadius, p.acols, p.arows)) continue;
        const int r1 = min(r0 + hc::STEP_BLOCK, p.maxRadius + 1);
        for (int r = r0; r < r1; r++) {
            int x2, y2;
            hc::rayCell(ray, sg, r, &x2, &y2);
            if (!hc::inside(x2, y2, p.acols, p.arows)) break;                // monotone in r: every later step is outside too
            atomicAdd(A + (size_t)y2 * p.astep + x2, 1);
        }
    }
}

// reach: cells a ray can travel, rounded up with a margin (host side, tileReach); the tiles cover the whole (arows + 2) x (acols + 2) accumulator
__global__ __launch_bounds__(256) void k_hc_vote_tile(Planes pl, Params p, int reach, const uint32_t* __restrict__ rows, size_t rframe, const uint32_t* __restrict__ pts,
                                                      size_t pframe, int* __restrict__ acc, size_t aframe)
{
    __shared__ int tile[hc::TILE * hc::TILE];
    const int f = blockIdx.z, tx0 = blockIdx.x * hc::TILE, ty0 = blockIdx.y * hc::TILE;
    for (int i = threadIdx.x; i < hc::TILE * hc::TILE; i += 256) tile[i] = 0;
    __syncthreads();
    // the pixels whose rays can reach the tile: a superset is enough, every step is tested against the tile
    const int ylo = max(0, (int)floorf((float)(ty0 - reach) * p.dp) - 1), yhi = min(p.h - 1, (int)ceilf((float)(ty0 + hc::TILE + reach) * p.dp) + 1);
    const int xlo = (int)floorf((float)(tx0 - reach) * p.dp) - 1, xhi = (int)ceilf((float)(tx0 + hc::TILE + reach) * p.dp) + 1;
    if (ylo <= yhi && tx0 < p.acols && ty0 < p.arows) {
        const uint32_t* R = rows + (size_t)f * rframe;
        const uint32_t* P = pts + (size_t)f * pframe;
        const uint32_t begin = R[ylo], end = R[yhi + 1];
        for (uint64_t it = 2 * (uint64_t)begin + threadIdx.x; it < 2 * (uint64_t)end; it += 256) {
            const uint32_t pt = P[it >> 1];
            const int x = hough::pointX(pt), y = hough::pointY(pt), sg = (it & 1) ? -1 : 1;
            if (x < xlo || x > xhi) continue;
            int vx, vy;
            gradAt(pl, f, x, y, &vx, &vy);
            hc::Ray ray;
            if (!hc::makeRay(x, y, vx, vy, p.idp, &ray) || !hc::rayStarts(ray, sg, p.minRadius, p.acols, p.arows)) continue;
            for (int r = p.minRadius; r <= p.maxRadius; r++) {
                int x2, y2;
                hc::rayCell(ray, sg, r, &x2, &y2);
                if (!hc::inside(x2, y2, p.acols, p.arows)) break;
                const unsigned lx = (unsigned)(x2 - tx0), ly = (unsigned)(y2 - ty0);
                if (lx < (unsigned)hc::TILE && ly < (unsigned)hc::TILE) atomicAdd(&tile[ly * hc::TILE + lx], 1);
            }
        }
    }
    __syncthreads();
    int* A = acc + (size_t)f * aframe;
    for (int i = threadIdx.x; i < hc::TILE * hc::TILE; i += 256) {
        const int yy = ty0 + i / hc::TILE, xx = tx0 + i % hc::TILE;
        if (yy < p.arows + 2 && xx < p.astep) A[(size_t)yy * p.astep + xx] = tile[i];
    }
}

// cand: the COMPLEMENT of the sort key (the device sort is a descending one), zeros behind the candidates
__global__ __launch_bounds__(256) void k_hc_maxima(const int* __restrict__ acc, size_t aframe, Params p, unsigned long long* __restrict__ cand, size_t cframe,
                                                   uint32_t capacity, uint32_t* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63, x = blockIdx.x * 256 + threadIdx.x, f = blockIdx.z;
    const int* A = acc + (size_t)f * aframe;
    const int b = (blockIdx.y + 1) * p.astep + x + 1;
    const bool is = x < p.acols && hough::isMaximum(A, b, p.acols, p.accT);
    const uint64_t m = __ballot(is);
    if (!m) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(ctr + CTR * f, (uint32_t)__popcll(m));
    base = __shfl(base, 0, 64);
    if (!is) return;
    const uint32_t at = base + __popcll(m & ((uint64_t(1) << lane) - 1));
    if (at < capacity) cand[(size_t)f * cframe + at] = ~hough::sortKey(A[b], b);
}

template <bool LDS> __device__ __forceinline__ int binLoad(const int* b)
{
    if (LDS) return *b;
    return __hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the slab's adds were made in L2: do not read a line this CU still holds
}

// sorted: the centres in order (complement keys); cand[i] receives the circle's complement key, or 0 when the centre gives none; acc[b] its radius
template <bool LDS>
__global__ __launch_bounds__(256) void k_hc_radius(Params p, const uint32_t* __restrict__ rows, size_t rframe, const uint32_t* __restrict__ pts, size_t pframe,
                                                   const unsigned long long* __restrict__ sorted, unsigned long long* __restrict__ cand, size_t cframe, uint32_t capacity,
                                                   const uint32_t* __restrict__ ctr, int* __restrict__ acc, size_t aframe, int* __restrict__ slabs)
{
    extern __shared__ int lbins[];
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    int* bins = LDS ? lbins : slabs + ((size_t)f * gridDim.x + blockIdx.x) * (size_t)p.nBins;
    const uint32_t ncent = min(ctr[CTR * f], capacity);
    const uint32_t* R = rows + (size_t)f * rframe;
    const uint32_t* P = pts + (size_t)f * pframe;
    for (uint32_t i = blockIdx.x; i < ncent; i += gridDim.x) {
        for (int k = threadIdx.x; k < p.nBins; k += 256) bins[k] = 0;
        if (!LDS) __threadfence();                                          // the zeros reach L2 before any add does
        __syncthreads();
        const int b = hough::keyCell(~sorted[(size_t)f * cframe + i]);
        const float cx = hc::centreCoord(b % p.astep, p.dp), cy = hc::centreCoord(b / p.astep, p.dp);
        // rows that can hold a point within maxRadius of the centre (a superset: radiusBin tests every point)
        const float lo = floorf(cy - (float)p.maxRadius) - 1.f, hi = ceilf(cy + (float)p.maxRadius) + 1.f;
        const int ylo = lo < 0.f ? 0 : (int)lo, yhi = hi > (float)(p.h - 1) ? p.h - 1 : (int)hi;
        if (ylo <= yhi) {
            const uint32_t begin = R[ylo], end = R[yhi + 1];
            // 16-byte loads from the aligned word at or below begin; the list of a frame starts 256-byte aligned and is padded to a multiple of 256 bytes
            for (uint32_t q = (begin & ~3u) + 4 * threadIdx.x; q < end; q += 1024) {
                const uint4 v = *reinterpret_cast<const uint4*>(P + q);
                const uint32_t pv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (q + k < begin || q + k >= end) continue;
                    const int bin = hc::radiusBin(cx, cy, hough::pointX(pv[k]), hough::pointY(pv[k]), p);
                    if (bin >= 0) atomicAdd(bins + bin, 1);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                             // the scan, sequential by rule: wave 0 skips empty bins 64 at a time
            float rBest = 0.f;
            int maxCount = 0, j = p.nBins - 1;
            while (j > 0) {
                const int idx = j - lane;
                const uint64_t m = __ballot(idx > 0 && binLoad<LDS>(bins + idx) != 0);
                if (!m) { j -= 64; continue; }
                const int upbin = j - ctz64(m);
                const int k = upbin - lane;
                int cur = (lane < hc::BINS_PER_DR && k >= 0) ? binLoad<LDS>(bins + k) : 0;
#pragma unroll
                for (int d = 8; d; d >>= 1) cur += __shfl_xor(cur, d, 64);  // lanes 10 .. 15 hold 0: the sum of the window in lanes 0 .. 15
                cur = __shfl(cur, 0, 64);
                j = upbin - hc::BINS_PER_DR < -1 ? -1 : upbin - hc::BINS_PER_DR;
                hc::scanWindow(upbin, j, cur, p, &rBest, &maxCount);
                j--;                                                        // the outer loop's own step after a window
            }
            if (lane == 0) {
                cand[(size_t)f * cframe + i] = maxCount > p.accT ? ~hough::sortKey(maxCount, b) : 0ull;
                acc[(size_t)f * aframe + b] = __float_as_int(rBest);
            }
        }
        __syncthreads();
    }
}

// sorted: complement keys of the circles (or, centres only, of the centres) in order, zeros behind them.  One wave per frame.
__global__ __launch_bounds__(64) void k_hc_suppress(Params p, const unsigned long long* __restrict__ sorted, size_t cframe, uint32_t capacity, const int* __restrict__ acc,
                                                    size_t aframe, int cn, int maxCircles, float* circles, size_t oframe, uint32_t* __restrict__ ctr)
{
    __shared__ float kx[KEEP_LDS], ky[KEEP_LDS];
    const int f = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* S = sorted + (size_t)f * cframe;
    float* out = circles + (size_t)f * oframe;
    int nk = 0;
    bool done = false;
    for (uint32_t i0 = 0; i0 < capacity && !done; i0 += 64) {
        const unsigned long long mine = i0 + lane < capacity ? S[i0 + lane] : 0ull;
        for (int t = 0; t < 64; t++) {
            const unsigned long long c = __shfl(mine, t, 64);
            if (!c) { done = true; break; }                                 // behind the last circle
            const int b = hough::keyCell(~c);
            const float cx = hc::centreCoord(b % p.astep, p.dp), cy = hc::centreCoord(b / p.astep, p.dp);
            bool shadowed = false;
            for (int k0 = 0; k0 < nk && !shadowed; k0 += 64) {
                const int k = k0 + lane;
                bool close = false;
                if (k < nk) {
                    const float x = k < KEEP_LDS ? kx[k] : out[(size_t)k * cn], y = k < KEEP_LDS ? ky[k] : out[(size_t)k * cn + 1];
                    close = hc::tooClose(x, y, cx, cy, p.minDist2);
                }
                shadowed = __ballot(close) != 0;
            }
            if (shadowed) continue;
            if (lane == 0) {
                float* row = out + (size_t)nk * cn;
                row[0] = cx; row[1] = cy;
                row[2] = p.centersOnly ? 0.f : __int_as_float(acc[(size_t)f * aframe + b]);
                if (cn == 4) row[3] = (float)hough::keyVotes(~c);
                if (nk < KEEP_LDS) { kx[nk] = cx; ky[nk] = cy; }
            }
            __threadfence_block();                                          // lane 0's row before the other lanes read it back
            if (++nk == maxCircles) { done = true; break; }
        }
    }
    if (lane == 0) ctr[CTR * f + 1] = (uint32_t)nk;
}

// ---- host side
int tileReach(const Params& p)                                               // cells: r * |s| / ONE <= r * (idp + 0.5 / ONE), plus the rounding of the start
{
    return (int)std::ceil((double)p.maxRadius * p.idp + (double)p.maxRadius / (2.0 * hc::ONE)) + 2;
}
// The tile arm won at no reach: 1.146 x (reach 16 cells) to 10.761 x (512) the time of k_hc_vote at 4K, 1.167 x to 10.293 x at 1080p (profiles/houghcircles_bench.jsonl, rows
// "arm crossing"), so there is no bound below which the library chooses it; it stays behind the switch.  (It walks every ray whole, once per tile: DESIGN 6.22.)
bool tileArm() { return g_arm.load(std::memory_order_relaxed) == 1; }

// the refusals that need no device and depend on the geometry alone; 0 when served
int circleArgs(int w, int h, int method, double dp, double minDist, double param1, double param2, int minRadius, int maxRadius, Params* p)
{
    MI355_DECLINE_IF(disabled());
    if (method == hc::HOUGH_GRADIENT_ALT) return MI355_DECLINED("method is HOUGH_GRADIENT_ALT (only HOUGH_GRADIENT is served)");
    if (method != hc::HOUGH_GRADIENT) return MI355_DECLINED("method is not HOUGH_GRADIENT (HOUGH_GRADIENT_ALT, HOUGH_STANDARD, ... are not served)");
    MI355_DECLINE_IF(w <= 0 || h <= 0 || w > lim::HOUGHCIRCLES_MAX_DIM || h > lim::HOUGHCIRCLES_MAX_DIM);
    switch (hc::prepare(w, h, dp, minDist, param1, param2, minRadius, maxRadius, p)) {
    case 0: return 0;
    case 1: return MI355_DECLINED("dp, minDist, cvRound(param1) or cvRound(param2) is not positive (or is NaN, or beyond the float / int range)");
    case 2: return MI355_DECLINED("(arows + 2) * (acols + 2) > lim::HOUGHCIRCLES_MAX_ACCUM");
    case 3: return MI355_DECLINED("maxRadius > lim::HOUGHCIRCLES_MAX_RADIUS");
    default: return MI355_DECLINED("nBins < 1 (minRadius beyond the frame's default maxRadius)");
    }
}

struct Scr {
    uint32_t* rows; uint32_t* pts; int* acc; unsigned long long* cand; unsigned long long* sorted; void* temp; uint32_t* ctr; int* slabs;
    size_t rf, pf, af, cf, tempBytes;         // frame strides in elements
    uint32_t capacity;
    int group, radiusGrid;
};

size_t frameBytes(const Params& p, bool circles, uint32_t capacity)
{
    const size_t cells = (size_t)(p.arows + 2) * p.astep;
    return pad256(((size_t)p.h + 1) * 4) + pad256((size_t)p.w * p.h * 4) + pad256(cells * 4) + (circles ? 2 * pad256((size_t)capacity * 8) : 0);
}

// scratch for groups of frames and the zeroed counters of all frames; `extra` bytes per frame of a group are the caller's own (the edge stage's planes)
bool circleScratch(Stager& stg, const Params& p, int nframes, bool circles, size_t extra, Scr* s, uchar** extraAt)
{
    s->capacity = circles ? (uint32_t)hc::maxCentres(p.arows, p.acols) : 0;
    const size_t rB = pad256(((size_t)p.h + 1) * 4), pB = pad256((size_t)p.w * p.h * 4), aB = pad256((size_t)(p.arows + 2) * p.astep * 4), cB = pad256((size_t)s->capacity * 8);
    const size_t per = frameBytes(p, circles, s->capacity) + extra;
    s->group = (int)std::min<size_t>((size_t)nframes, std::max<size_t>(1, (size_t(1) << 30) / per));
    s->rf = rB / 4; s->pf = pB / 4; s->af = aB / 4; s->cf = cB / 8;
    s->tempBytes = s->capacity > 1 ? sortKeysDescTemp(s->capacity) : 0;
    if (s->capacity > 1 && !s->tempBytes) return false;
    // the radius stage: a workgroup walks centres blockIdx.x, + gridDim.x, ...; histograms beyond LDS_BINS take a slab each, 256 MiB of them at the most
    const bool slab = circles && !p.centersOnly && p.nBins > hc::LDS_BINS;
    s->radiusGrid = (int)std::min<size_t>(std::max<uint32_t>(1, s->capacity), slab ? std::max<size_t>(1, (size_t(256) << 20) / ((size_t)p.nBins * 4 * s->group)) : 2048);
    s->radiusGrid = std::min(s->radiusGrid, 2048);
    const size_t slabB = slab ? pad256((size_t)p.nBins * 4 * s->radiusGrid * s->group) : 0;
    uchar* at = (uchar*)stg.scratch(per * s->group + pad256(s->tempBytes) + pad256((size_t)nframes * CTR * 4) + slabB);
    if (!at) return false;
    s->rows = (uint32_t*)at; at += rB * s->group;
    s->pts = (uint32_t*)at; at += pB * s->group;
    s->acc = (int*)at; at += aB * s->group;
    s->cand = (unsigned long long*)at; at += cB * s->group;
    s->sorted = (unsigned long long*)at; at += cB * s->group;
    *extraAt = at; at += extra * s->group;
    s->temp = at; at += pad256(s->tempBytes);
    s->ctr = (uint32_t*)at; at += pad256((size_t)nframes * CTR * 4);
    s->slabs = (int*)at;
    return hipMemsetAsync(s->ctr, 0, (size_t)nframes * CTR * 4, stream()) == hipSuccess;
}

// the point list and the accumulator of nf frames
bool launchVotes(const Scr& s, const Params& p, const Planes& pl, int nf, hipStream_t st)
{
    hipLaunchKernelGGL(k_hc_rowcount, dim3(divUp(p.h, 4), nf), dim3(256), 0, st, pl, p.w, p.h, s.rows, s.rf);
    hipLaunchKernelGGL(k_hc_rowscan, dim3(nf), dim3(256), 0, st, s.rows, s.rf, p.h);
    hipLaunchKernelGGL(k_hc_points, dim3(divUp(p.h, 4), nf), dim3(256), 0, st, pl, p.w, p.h, s.rows, s.rf, s.pts, s.pf);
    if (tileArm()) {
        hipLaunchKernelGGL(k_hc_vote_tile, dim3(divUp(p.astep, hc::TILE), divUp(p.arows + 2, hc::TILE), nf), dim3(256), 0, st, pl, p, tileReach(p), s.rows, s.rf, s.pts, s.pf,
                           s.acc, s.af);
        return true;
    }
    if (hipMemsetAsync(s.acc, 0, s.af * 4 * nf, st) != hipSuccess) return false;
    const uint64_t items = (uint64_t)p.w * p.h * 2 * ((p.maxRadius - p.minRadius) / hc::STEP_BLOCK + 1);
    hipLaunchKernelGGL(k_hc_vote, dim3((unsigned)std::min<uint64_t>((items + 255) / 256, 8192), nf), dim3(256), 0, st, pl, p, s.rows, s.rf, s.pts, s.pf, s.acc, s.af);
    return true;
}

// centres, radii, order and suppression of nf frames into `out` (rows of cn floats, frames oframe floats apart); ctr: the first of their counters
bool launchCircles(const Scr& s, const Params& p, int nf, float* out, int cn, int maxCircles, size_t oframe, uint32_t* ctr, hipStream_t st)
{
    if (!s.capacity) return true;                                           // cannot happen (arows, acols >= 1), kept for the sort's sake
    if (hipMemsetAsync(s.cand, 0, s.cf * 8 * nf, st) != hipSuccess) return false;
    hipLaunchKernelGGL(k_hc_maxima, dim3(divUp(p.acols, 256), p.arows, nf), dim3(256), 0, st, s.acc, s.af, p, s.cand, s.cf, s.capacity, ctr);
    auto sortAll = [&]() {
        if (s.capacity < 2) return hipMemcpyAsync(s.sorted, s.cand, s.cf * 8 * nf, hipMemcpyDeviceToDevice, st) == hipSuccess;
        for (int f = 0; f < nf; f++)
            if (!sortKeysDesc(s.temp, s.tempBytes, s.cand + (size_t)f * s.cf, s.sorted + (size_t)f * s.cf, s.capacity, st)) return false;
        return true;
    };
    if (!sortAll()) return false;
    if (!p.centersOnly) {
        const dim3 grid(s.radiusGrid, nf);
        if (p.nBins <= hc::LDS_BINS) {
            static std::atomic<bool> attr[64];                              // more than 64 KiB of dynamic LDS has to be asked for, once per device
            const int dv = activeDevice() & 63;
            if (!attr[dv].load(std::memory_order_acquire)) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_hc_radius<true>), hipFuncAttributeMaxDynamicSharedMemorySize, hc::LDS_BINS * 4);
                attr[dv].store(true, std::memory_order_release);
            }
            hipLaunchKernelGGL(k_hc_radius<true>, grid, dim3(256), (size_t)p.nBins * 4, st, p, s.rows, s.rf, s.pts, s.pf, s.sorted, s.cand, s.cf, s.capacity, ctr, s.acc, s.af,
                               (int*)nullptr);
        } else
            hipLaunchKernelGGL(k_hc_radius<false>, grid, dim3(256), 0, st, p, s.rows, s.rf, s.pts, s.pf, s.sorted, s.cand, s.cf, s.capacity, ctr, s.acc, s.af, s.slabs);
        if (!sortAll()) return false;
    }
    hipLaunchKernelGGL(k_hc_suppress, dim3(nf), dim3(64), 0, st, p, s.sorted, s.cf, s.capacity, s.acc, s.af, cn, maxCircles, out, oframe, ctr);
    return true;
}

void noteVote(const Params& p, int nframes, int group)
{
    noteKernel("%s, %d frame(s) in groups of %d, acc=%dx%d r=%d..%d dp=%g, + k_hc_maxima + sort + k_hc_radius<%s> nBins=%d + sort + k_hc_suppress",
               tileArm() ? "k_hc_vote_tile" : "k_hc_vote", nframes, group, p.arows, p.acols, p.minRadius, p.maxRadius, (double)p.dp,
               p.centersOnly ? "none" : p.nBins <= hc::LDS_BINS ? "lds" : "hbm", p.nBins);
}

// the checks of the circle list that need no device
int listArgs(const float* circles, int cn, int maxCircles, size_t oframeBytes, int nframes, const int* ncircles)
{
    MI355_DECLINE_IF(!circles || !ncircles || nframes < 1);
    if (cn != 3 && cn != 4) return MI355_DECLINED("circles_cn is not 3 or 4");
    if (maxCircles < 1 || maxCircles > lim::HOUGHCIRCLES_MAX_CIRCLES) return MI355_DECLINED("max_circles < 1 || max_circles > lim::HOUGHCIRCLES_MAX_CIRCLES");
    if (nframes > 1 && (oframeBytes % 4 || oframeBytes < (size_t)cn * 4 * maxCircles)) return MI355_DECLINED("circles_frame_stride is no multiple of 4 or below max_circles rows");
    MI355_DECLINE_IF(nframes > 65535);
    return 0;
}

// counts to the host (the call's one synchronisation of its own), then the written rows of host-resident lists
int finishCircles(const char* entry, Stager& stg, const Scr& s, const Params& p, int nframes, bool host, float* circles, float* hcircles, size_t lrow, int maxCircles,
                  size_t oframeBytes, uint32_t* hostN, int* ncircles, hipStream_t st)
{
    if (hipMemcpyAsync(hostN, s.ctr, (size_t)nframes * CTR * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
    if (host) {
        const size_t hl = lrow * maxCircles;
        for (int f = 0; f < nframes; f++) {
            const size_t rows = hostN[CTR * f + 1];
            if (rows && hipMemcpyAsync((uchar*)circles + (size_t)f * oframeBytes, (uchar*)hcircles + (size_t)f * hl, rows * lrow, hipMemcpyDeviceToHost, st) != hipSuccess)
                return setError(MI355CV_ERROR_UNKNOWN, "%s: D2H failed: %s", entry, hipGetErrorString(hipGetLastError()));
            noteStagedBytes((long long)(rows * lrow));
        }
        if (hipStreamSynchronize(st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: D2H failed: %s", entry, hipGetErrorString(hipGetLastError()));
    }
    for (int f = 0; f < nframes; f++) ncircles[f] = (int)hostN[CTR * f + 1];
    noteVote(p, nframes, s.group);
    return stg.finish(entry);
}

int runCircles(const char* entry, const uchar* src, size_t sstep, size_t sframe, int w, int h, float* circles, int cn, int maxCircles, size_t oframeBytes, int nframes,
               int method, double dp, double minDist, double param1, double param2, int minRadius, int maxRadius, int* ncircles)
{
    Params p;
    MI355_DECLINE_IF(!src);
    if (const int rc = listArgs(circles, cn, maxCircles, oframeBytes, nframes, ncircles)) return rc;
    if (const int rc = circleArgs(w, h, method, dp, minDist, param1, param2, minRadius, maxRadius, &p)) return rc;
    if (sstep < (size_t)w || (nframes > 1 && sframe < (size_t)(h - 1) * sstep + w)) return MI355_DECLINED("src_step below the width or src_frame_stride below a frame");
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    const int skind = ptrKind(src), lkind = ptrKind(circles);
    if (skind == PTR_FOREIGN || lkind == PTR_FOREIGN || skind != lkind)
        return MI355_DECLINED("image and circles must both live on this thread's device or both on the host");
    const bool host = skind == PTR_HOST;
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_HEAVY)));
    const size_t lrow = (size_t)cn * 4, hl = lrow * maxCircles;
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + w, lspan = (size_t)(nframes - 1) * oframeBytes + hl;
    MI355_DECLINE_IF(overlapOnDevice(src, sspan, circles, lspan));

    // the edge stage's planes of a frame: dx, dy, edges, the hysteresis map and, for host-resident frames, the dense copy of the source
    const size_t gstep = pad256((size_t)w * 2), estep = pad256((size_t)w), hstep = pad256((size_t)w);
    const size_t gB = gstep * h, eB = estep * h, mB = pad256(cannyMapBytes(w, h)), hB = host ? hstep * h : 0;
    Scr s;
    uchar* planes;
    if (!circleScratch(stg, p, nframes, true, 2 * gB + eB + mB + hB, &s, &planes)) return MI355_DECLINED("no scratch");
    uchar* dxs = planes; uchar* dys = dxs + gB * s.group; uchar* eds = dys + gB * s.group; uchar* maps = eds + eB * s.group; uchar* hsrc = maps + mB * s.group;
    int* flag = (int*)stg.scratch(256);
    uint32_t* hostN = (uint32_t*)stg.pinned((size_t)nframes * CTR * 4);
    float* hcircles = host ? (float*)stg.scratch(hl * nframes) : nullptr;
    if (!flag || !hostN || (host && !hcircles)) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    const int low = std::max(1, p.canny / 2), high = p.canny;
    for (int f0 = 0; f0 < nframes; f0 += s.group) {
        const int nf = std::min(s.group, nframes - f0);
        for (int f = 0; f < nf; f++) {                                       // the hysteresis keeps its own host round-trips per frame
            const uchar* sp = src + (size_t)(f0 + f) * sframe;
            size_t ss = sstep;
            if (host) {
                uchar* d = hsrc + (size_t)f * hB;
                if (hipMemcpy2DAsync(d, hstep, sp, sstep, (size_t)w, h, hipMemcpyHostToDevice, st) != hipSuccess)
                    return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
                noteStagedBytes((long long)w * h);
                sp = d; ss = hstep;
            }
            uchar* dx = dxs + (size_t)f * gB; uchar* dy = dys + (size_t)f * gB;
            int rc = mi355cv_sobel(sp, ss, dx, gstep, w, h, MI355CV_8U, MI355CV_16S, 1, 0, 0, 0, 0, 1, 0, 3, 1.0, 0.0, B_REPLICATE);
            if (rc == MI355CV_OK) rc = mi355cv_sobel(sp, ss, dy, gstep, w, h, MI355CV_8U, MI355CV_16S, 1, 0, 0, 0, 0, 0, 1, 3, 1.0, 0.0, B_REPLICATE);
            if (rc != MI355CV_OK) return rc;
            if (!cannyFromGradients((const short*)dx, (const short*)dy, gstep, w, h, 1, 0, low, high, maps + (size_t)f * mB, flag, eds + (size_t)f * eB, estep, st))
                return setError(MI355CV_ERROR_UNKNOWN, "%s: the edge stage failed: %s", entry, hipGetErrorString(hipGetLastError()));
        }
        const Planes pl{eds, estep, eB, dxs, dys, gstep, gB};
        float* lp = host ? hcircles + (size_t)f0 * (hl / 4) : circles + (size_t)f0 * (oframeBytes / 4);
        if (!launchVotes(s, p, pl, nf, st) || !launchCircles(s, p, nf, lp, cn, maxCircles, host ? hl / 4 : oframeBytes / 4, s.ctr + CTR * (size_t)f0, st))
            return setError(MI355CV_ERROR_UNKNOWN, "%s: enqueue failed: %s", entry, hipGetErrorString(hipGetLastError()));
    }
    MI355_CHECK_LAUNCH(entry);
    return finishCircles(entry, stg, s, p, nframes, host, circles, hcircles, lrow, maxCircles, oframeBytes, hostN, ncircles, st);
}

// the planes of the two stage entries: all three on this thread's device, or all three on the host (then staged)
int stagePlanes(Stager& stg, const uchar* edges, size_t estep, const short* dx, const short* dy, size_t gstep, int w, int h, const void* dst, size_t dspan, bool* host, Planes* pl)
{
    const int ek = ptrKind(edges), xk = ptrKind(dx), yk = ptrKind(dy), dk = ptrKind(dst);
    if (ek == PTR_FOREIGN || xk == PTR_FOREIGN || yk == PTR_FOREIGN || dk == PTR_FOREIGN || ek != xk || ek != yk || ek != dk)
        return MI355_DECLINED("edges, dx, dy and the destination must all live on this thread's device or all on the host");
    *host = ek == PTR_HOST;
    MI355_DECLINE_IF(hostImageTooSmall(edges, (size_t)w * h, minPixels(HOST_HEAVY)));
    MI355_DECLINE_IF(overlapOnDevice(edges, span(estep, h, (size_t)w), dst, dspan) || overlapOnDevice(dx, span(gstep, h, (size_t)w * 2), dst, dspan) ||
                     overlapOnDevice(dy, span(gstep, h, (size_t)w * 2), dst, dspan));
    size_t es, xs, ys;
    pl->edges = stg.in(edges, estep, (size_t)w, h, &es);
    pl->dx = stg.in((const uchar*)dx, gstep, (size_t)w * 2, h, &xs);
    pl->dy = stg.in((const uchar*)dy, gstep, (size_t)w * 2, h, &ys);
    if (!pl->edges || !pl->dx || !pl->dy) return MI355_DECLINED("no scratch");
    if (xs != ys) return MI355_DECLINED("staged gradient planes of different pitch");
    pl->estep = es; pl->eframe = 0; pl->gstep = xs; pl->gframe = 0;
    return 0;
}

int planeArgs(const uchar* edges, size_t estep, const short* dx, const short* dy, size_t gstep, int w)
{
    MI355_DECLINE_IF(!edges || !dx || !dy);
    if (w > 0 && (estep < (size_t)w || gstep < (size_t)w * 2 || gstep % 2 || ((uintptr_t)dx | (uintptr_t)dy) % 2))
        return MI355_DECLINED("edges_step below the width, grad_step below the width in shorts or odd, or a gradient plane at an odd address");
    return 0;
}

} // namespace

static_assert(lim::HOUGHCIRCLES_MAX_DIM == hc::MAX_DIM && lim::HOUGHCIRCLES_MAX_ACCUM == hc::MAX_ACCUM && lim::HOUGHCIRCLES_MAX_RADIUS == hc::MAX_RADIUS &&
              lim::HOUGHCIRCLES_MAX_CIRCLES == hc::MAX_CIRCLES && lim::HOUGHCIRCLES_LDS_BINS == hc::LDS_BINS && lim::HOUGHCIRCLES_TILE == hc::TILE,
              "one bound");
static_assert(hc::MAX_DIM <= 65535, "packed points");
static_assert(hc::LDS_BINS * sizeof(int) <= 160 * 1024, "the bins of k_hc_radius<true> in LDS");

extern "C" {

MI355CV_API int mi355cv_houghCircles(const uchar* src_data, size_t src_step, int width, int height, float* circles, int circles_cn, int max_circles, int method, double dp,
                                     double minDist, double param1, double param2, int minRadius, int maxRadius, int* ncircles)
{
    mi355::EntryGuard entry_(__func__);
    return runCircles("houghCircles", src_data, src_step, 0, width, height, circles, circles_cn, max_circles, 0, 1, method, dp, minDist, param1, param2, minRadius, maxRadius,
                      ncircles);
}

MI355CV_API int mi355cv_houghCirclesBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, float* circles, int circles_cn,
                                          int max_circles, size_t circles_frame_stride, int nframes, int method, double dp, double minDist, double param1, double param2,
                                          int minRadius, int maxRadius, int* ncircles)
{
    mi355::EntryGuard entry_(__func__);
    return runCircles("houghCirclesBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, width, height, circles, circles_cn, max_circles,
                      nframes == 1 ? 0 : circles_frame_stride, nframes, method, dp, minDist, param1, param2, minRadius, maxRadius, ncircles);
}

MI355CV_API int mi355cv_houghCirclesGradient(const uchar* edges, size_t edges_step, const short* dx, const short* dy, size_t grad_step, int width, int height, float* circles,
                                             int circles_cn, int max_circles, int method, double dp, double minDist, double param1, double param2, int minRadius,
                                             int maxRadius, int* ncircles)
{
    mi355::EntryGuard entry_(__func__);
    const char* entry = "houghCirclesGradient";
    Params p;
    if (const int rc = planeArgs(edges, edges_step, dx, dy, grad_step, width)) return rc;
    if (const int rc = listArgs(circles, circles_cn, max_circles, 0, 1, ncircles)) return rc;
    if (const int rc = circleArgs(width, height, method, dp, minDist, param1, param2, minRadius, maxRadius, &p)) return rc;
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    const size_t lrow = (size_t)circles_cn * 4, hl = lrow * max_circles;
    bool host;
    Planes pl;
    if (const int rc = stagePlanes(stg, edges, edges_step, dx, dy, grad_step, width, height, circles, hl, &host, &pl)) return rc;
    Scr s;
    uchar* none;
    if (!circleScratch(stg, p, 1, true, 0, &s, &none)) return MI355_DECLINED("no scratch");
    uint32_t* hostN = (uint32_t*)stg.pinned(CTR * 4);
    float* hcircles = host ? (float*)stg.scratch(hl) : nullptr;
    if (!hostN || (host && !hcircles)) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    if (!launchVotes(s, p, pl, 1, st) || !launchCircles(s, p, 1, host ? hcircles : circles, circles_cn, max_circles, 0, s.ctr, st))
        return setError(MI355CV_ERROR_UNKNOWN, "%s: enqueue failed: %s", entry, hipGetErrorString(hipGetLastError()));
    MI355_CHECK_LAUNCH(entry);
    return finishCircles(entry, stg, s, p, 1, host, circles, hcircles, lrow, max_circles, 0, hostN, ncircles, st);
}

MI355CV_API int mi355cv_houghCirclesAccum(const uchar* edges, size_t edges_step, const short* dx, const short* dy, size_t grad_step, int width, int height, double dp,
                                          int minRadius, int maxRadius, int* accum, size_t accum_step, int* arows, int* acols)
{
    mi355::EntryGuard entry_(__func__);
    const char* entry = "houghCirclesAccum";
    Params p;
    MI355_DECLINE_IF(!arows || !acols);
    if (const int rc = planeArgs(edges, edges_step, dx, dy, grad_step, width)) return rc;
    if (const int rc = circleArgs(width, height, hc::HOUGH_GRADIENT, dp, 1.0, 1.0, 1.0, minRadius, maxRadius, &p)) return rc;
    if (!accum) { *arows = p.arows; *acols = p.acols; return MI355CV_OK; }  // the geometry alone: no device is touched
    const size_t rowBytes = (size_t)p.astep * 4;
    const int rows = p.arows + 2;
    if (accum_step < rowBytes || accum_step % 4) return MI355_DECLINED("accum_step is below (acols + 2) ints or no multiple of 4");
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    bool host;
    Planes pl;
    if (const int rc = stagePlanes(stg, edges, edges_step, dx, dy, grad_step, width, height, accum, span(accum_step, rows, rowBytes), &host, &pl)) return rc;
    Scr s;
    uchar* none;
    if (!circleScratch(stg, p, 1, false, 0, &s, &none)) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    if (!launchVotes(s, p, pl, 1, st)) return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed: %s", entry, hipGetErrorString(hipGetLastError()));
    MI355_CHECK_LAUNCH(entry);
    if (hipMemcpy2DAsync(accum, accum_step, s.acc, rowBytes, rowBytes, rows, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st) != hipSuccess)
        return setError(MI355CV_ERROR_UNKNOWN, "%s: copy failed: %s", entry, hipGetErrorString(hipGetLastError()));
    if (host) {
        noteStagedBytes((long long)(rowBytes * rows));
        if (hipStreamSynchronize(st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
    }
    *arows = p.arows; *acols = p.acols;
    noteKernel("%s, acc=%dx%d radius=%d..%d dp=%g, k_hc_rowcount + k_hc_rowscan + k_hc_points", tileArm() ? "k_hc_vote_tile" : "k_hc_vote", p.arows, p.acols, p.minRadius,
               p.maxRadius, (double)p.dp);
    return stg.finish(entry);
}

MI355CV_API int mi355cv_houghCirclesSetKernel(int mode)
{
    if (mode < -1 || mode > 1) return -1;
    g_arm.store(mode, std::memory_order_relaxed);
    return 0;
}

} // extern "C"
