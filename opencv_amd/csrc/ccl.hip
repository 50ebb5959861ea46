// ccl.hip -- cv::connectedComponents / cv::connectedComponentsWithStats (imgproc/src/connectedcomponents.cpp; the reference has no HAL hook for them) on
// CV_8UC1, 4- and 8-connected, labels CV_32S or CV_16U.  Every line of arithmetic is in ccl_math.h, and the find / unite loops are unionfind.h's (over its LDS
// and HBM memory policies); tests/hostemu/ccl_emu.cpp compiles both for the host.  A union-find over pixels whose root is the SMALLEST linear pixel index of the set
// (parents only ever decrease), so the root of a component is its first raster pixel whatever order the merges land in.
//
//   k_ccl_strip      a wave per tile of 256 columns x 16 rows.  A lane loads one dword (4 pixels), four 64-bit ballots become the four row words of the tile;
//                    runs and the links to the row above are bit scans of those words (no per-pixel work); the runs of the tile are merged in LDS (atomicMin
//                    on LDS), and every pixel's parent -- the first pixel of its component INSIDE the tile -- goes to the parent image P in HBM (BG for background).
//   k_ccl_vseam      a thread per (row, vertical tile seam), k_ccl_hseam a wave per (tile, strip seam): the pairs across the seams, united in HBM with
//                    atomicMin.  A find may read a parent another workgroup of the same kernel has just written: every such load is an agent-scope atomic load,
//                    and the union loop retries until its atomicMin returns the value it expected, so a stale read only costs another round.
//   k_ccl_flatten    every foreground pixel finds its root and stores it; the roots raise their flag in a bitmap over key space -- pixel order: the root's own
//                    index; block order: the smallest 2 x 2 block key of the component, an atomicMin per run of the root's block row into a table indexed by the
//                    root's block (a block meets one component at most), k_ccl_blockflags then raises the flags.
//   k_ccl_count / k_ccl_scan    an exclusive scan of the flags: per 64-bit word inside chunks of 256 words, then over the chunks by one workgroup per frame.
//                    The total is N - 1, the one value the host reads.
//   k_ccl_write      label = rank of the component's flag + 1, in the destination's type; only now is the destination touched.
//   k_ccl_stats*     runs of equal label per row (background runs included) add area, sums and bounds into a per-label accumulator, one update per run;
//                    k_ccl_stats_finish writes the five ints and the two doubles.
// Everything else is ordered by kernel boundaries; there is no grid-wide wait.
#include "rt.h"
#include "ccl_math.h"
#include "unionfind.h"
#include <algorithm>

using namespace mi355;

namespace {

using ccl::BG;
using ccl::STRIP_H;
using ccl::TILE_W;
using ccl::WORDS;
using uf::GlobalMem;
using uf::LdsMem;

// the scratch of a group of frames: parents, flag bitmap, the two levels of its scan, the block-key table, the totals
struct Scr {
    uint32_t* P; unsigned long long* B; uint32_t* wpre; uint32_t* chunk; uint32_t* K; uint32_t* total;
    size_t pf, bf, wf, cf, kf;             // frame strides in elements
    uint32_t nW, nchunk, npos;
};

// bytes x .. x + 3 of a row w wide as a dword, 0 for the ones past its end
__device__ __forceinline__ uint32_t loadPix4(const uchar* row, int x, int w)
{
    if (x + 4 <= w && ((uintptr_t)(row + x) & 3) == 0) return *reinterpret_cast<const uint32_t*>(row + x);
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) if (x + k < w) v |= (uint32_t)row[x + k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(64) void k_ccl_strip(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h, int conn8, uint32_t* __restrict__ P, size_t pframe)
{
    __shared__ uint32_t par[STRIP_H * TILE_W];
    __shared__ uint64_t wd[STRIP_H][WORDS];
    const int lane = threadIdx.x, x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * STRIP_H, rows = min(STRIP_H, h - y0);
    src += (size_t)blockIdx.z * sframe;
    P += (size_t)blockIdx.z * pframe;
    for (int r = 0; r < rows; r++) {
        const uint32_t v = loadPix4(src + (size_t)(y0 + r) * sstep, x0 + 4 * lane, w);
        const uint64_t b0 = __ballot(v & 0xffu), b1 = __ballot(v & 0xff00u), b2 = __ballot(v & 0xff0000u), b3 = __ballot(v & 0xff000000u);
        if (lane < WORDS) wd[r][lane] = ccl::rowWord(b0, b1, b2, b3, lane);
    }
    __syncthreads();
    for (int r = 0; r < rows; r++) {                                         // a node per run: its first pixel
        const uint64_t* W = wd[r];
        for (int j = 0; j < WORDS; j++)
            if ((W[j] >> lane) & 1) { const int c = 64 * j + lane; if (ccl::tileRunStart(W, j, lane) == c) par[r * TILE_W + c] = r * TILE_W + c; }
    }
    __syncthreads();
    LdsMem m{par};
    for (int r = 1; r < rows; r++) {                                         // the pairs (run, run of the row above) that touch
        const uint64_t* W = wd[r]; const uint64_t* U = wd[r - 1];
        for (int j = 0; j < WORDS; j++) {
            const uint64_t Wl = j ? W[j - 1] >> 63 : 0, Ul = j ? U[j - 1] >> 63 : 0, Wr = j + 1 < WORDS ? W[j + 1] & 1 : 0, Ur = j + 1 < WORDS ? U[j + 1] & 1 : 0;
            const uint64_t direct = ccl::linkDirect(W[j], U[j], Wl, Ul);
            const uint64_t left = conn8 ? ccl::linkLeft(W[j], U[j], Wl, Ul) : 0, right = conn8 ? ccl::linkRight(W[j], U[j], Wr, Ur) : 0;
            if (!(((direct | left | right) >> lane) & 1)) continue;
            const uint32_t a = r * TILE_W + ccl::tileRunStart(W, j, lane);
            if ((direct >> lane) & 1) uf::unite(m, a, (r - 1) * TILE_W + ccl::tileRunStart(U, j, lane));
            if ((left >> lane) & 1) { const int c = 64 * j + lane - 1; uf::unite(m, a, (r - 1) * TILE_W + ccl::tileRunStart(U, c >> 6, c & 63)); }
            if ((right >> lane) & 1) { const int c = 64 * j + lane + 1; uf::unite(m, a, (r - 1) * TILE_W + ccl::tileRunStart(U, c >> 6, c & 63)); }
        }
    }
    __syncthreads();
    for (int r = 0; r < rows; r++) {
        const uint64_t* W = wd[r];
        for (int j = 0; j < WORDS; j++) {
            const int x = x0 + 64 * j + lane;
            if (x >= w) continue;
            uint32_t p = BG;
            if ((W[j] >> lane) & 1) {
                const uint32_t root = uf::find(m, r * TILE_W + ccl::tileRunStart(W, j, lane));
                p = (uint32_t)(y0 + (int)(root / TILE_W)) * (uint32_t)w + (uint32_t)(x0 + (int)(root % TILE_W));
            }
            P[(size_t)(y0 + r) * w + x] = p;
        }
    }
}

// pixel (y, x - 1) against (y, x) and, 8-connected, the two diagonals above them, x a multiple of TILE_W
__global__ __launch_bounds__(64) void k_ccl_vseam(uint32_t* __restrict__ P, size_t pframe, int w, int h, int conn8)
{
    const int y = blockIdx.x * 64 + threadIdx.x, x = (blockIdx.y + 1) * TILE_W;
    if (y >= h) return;
    GlobalMem m{P + (size_t)blockIdx.z * pframe};
    const uint32_t b = (uint32_t)y * w + x, a = b - 1;
    const bool fa = m.load(a) != BG, fb = m.load(b) != BG;
    if (fa && fb) uf::unite(m, a, b);
    if (conn8 && y > 0) {
        if (fa && m.at(m.P + b - w) != BG) uf::unite(m, a, b - w);
        if (fb && m.at(m.P + a - w) != BG) uf::unite(m, b, a - w);
    }
}

// row y = first row of a strip against row y - 1, the carries taken from the neighbouring tiles
__global__ __launch_bounds__(64) void k_ccl_hseam(uint32_t* __restrict__ P, size_t pframe, int w, int conn8)
{
    const int lane = threadIdx.x, x0 = blockIdx.x * TILE_W, y = (blockIdx.y + 1) * STRIP_H;
    GlobalMem m{P + (size_t)blockIdx.z * pframe};
    const uint32_t* cur = m.P + (size_t)y * w; const uint32_t* up = cur - w;
    uint64_t W[WORDS + 2], U[WORDS + 2];                                     // [0] and [WORDS + 1]: the carries
    W[0] = x0 > 0 && m.at(cur + x0 - 1) != BG ? ~uint64_t(0) : 0; U[0] = x0 > 0 && m.at(up + x0 - 1) != BG ? ~uint64_t(0) : 0;
    W[WORDS + 1] = x0 + TILE_W < w && m.at(cur + x0 + TILE_W) != BG; U[WORDS + 1] = x0 + TILE_W < w && m.at(up + x0 + TILE_W) != BG;
#pragma unroll
    for (int j = 0; j < WORDS; j++) {
        const int x = x0 + 64 * j + lane;
        W[j + 1] = __ballot(x < w && m.at(cur + x) != BG);
        U[j + 1] = __ballot(x < w && m.at(up + x) != BG);
    }
#pragma unroll
    for (int j = 1; j <= WORDS; j++) {
        const uint64_t Wl = W[j - 1] >> 63, Ul = U[j - 1] >> 63, Wr = W[j + 1] & 1, Ur = U[j + 1] & 1;
        const uint64_t direct = ccl::linkDirect(W[j], U[j], Wl, Ul);
        const uint64_t left = conn8 ? ccl::linkLeft(W[j], U[j], Wl, Ul) : 0, right = conn8 ? ccl::linkRight(W[j], U[j], Wr, Ur) : 0;
        const uint32_t a = (uint32_t)y * w + x0 + 64 * (j - 1) + lane;
        if ((direct >> lane) & 1) uf::unite(m, a, a - w);
        if ((left >> lane) & 1) uf::unite(m, a, a - w - 1);
        if ((right >> lane) & 1) uf::unite(m, a, a - w + 1);
    }
}

// a wave per (row, tile): roots found and stored, flags raised
template <int ORDER>
__global__ __launch_bounds__(256) void k_ccl_flatten(Scr s, int w, int h)
{
    const int lane = threadIdx.x & 63, x0 = blockIdx.x * TILE_W, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    GlobalMem m{s.P + (size_t)blockIdx.z * s.pf};
#pragma unroll
    for (int j = 0; j < WORDS; j++) {
        const int x = x0 + 64 * j + lane;
        const uint32_t g = (uint32_t)y * w + x;
        const uint32_t p = x < w ? m.load(g) : BG;
        const bool fg = p != BG;
        uint32_t r = BG;
        if (fg) {
            r = uf::find(m, p);
            if (r != p) __hip_atomic_store(m.P + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (ORDER == ccl::ORDER_PIXEL) {
            const uint64_t m = __ballot(fg && r == g);
            if (m && lane == 0) {
                const uint32_t g0 = (uint32_t)y * w + x0 + 64 * j, sh = g0 & 63;
                unsigned long long* B = s.B + (size_t)blockIdx.z * s.bf + (g0 >> 6);
                atomicOr(B, (unsigned long long)(m << sh));
                if (sh && (m >> (64 - sh))) atomicOr(B + 1, (unsigned long long)(m >> (64 - sh)));
            }
        } else {
            // only the pixels in the block row of the root can hold the component's smallest block key, and of a run its first pixel does
            const uint64_t f = __ballot(fg);
            if (fg && r >= (uint32_t)(y & ~1) * w && (lane == 0 || !((f >> (lane - 1)) & 1))) {
                const int ry = r / (uint32_t)w, rx = r - ry * w;
                atomicMin(s.K + (size_t)blockIdx.z * s.kf + ccl::blockKey(rx, ry, w), ccl::blockKey(x, y, w));
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_ccl_blockflags(Scr s, uint32_t nblocks)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    const uint32_t k = s.K[(size_t)blockIdx.z * s.kf + b];
    if (k != BG) atomicOr(s.B + (size_t)blockIdx.z * s.bf + (k >> 6), 1ull << (k & 63));
}

__device__ __forceinline__ uint32_t waveInclusive(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}

// a workgroup per chunk of 256 bitmap words: the exclusive scan of their bit counts inside the chunk, and the chunk's total
__global__ __launch_bounds__(256) void k_ccl_count(Scr s)
{
    __shared__ uint32_t ws[4];
    const uint32_t i = blockIdx.x * ccl::CHUNK_WORDS + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t c = i < s.nW ? (uint32_t)ccl::popc64(s.B[(size_t)blockIdx.z * s.bf + i]) : 0;
    const uint32_t inc = waveInclusive(c, lane);
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    uint32_t off = 0;
    for (int k = 0; k < wv; k++) off += ws[k];
    if (i < s.nW) s.wpre[(size_t)blockIdx.z * s.wf + i] = off + inc - c;
    if (threadIdx.x == 255) s.chunk[(size_t)blockIdx.z * s.cf + blockIdx.x] = off + inc;
}

// one workgroup per frame: the chunk totals to their exclusive scan, in place; the grand total is the number of components
__global__ __launch_bounds__(1024) void k_ccl_scan(Scr s)
{
    __shared__ uint32_t ws[16];
    __shared__ uint32_t carry;
    uint32_t* c = s.chunk + (size_t)blockIdx.x * s.cf;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < s.nchunk; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < s.nchunk ? c[i] : 0;
        const uint32_t inc = waveInclusive(v, lane);
        if (lane == 63) ws[wv] = inc;
        __syncthreads();
        uint32_t off = carry, tot = 0;
        for (int k = 0; k < 16; k++) { if (k < wv) off += ws[k]; tot += ws[k]; }
        if (i < s.nchunk) c[i] = off + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) s.total[blockIdx.x] = carry;
}

template <typename T, int ORDER>
__global__ __launch_bounds__(256) void k_ccl_write(Scr s, int w, uchar* __restrict__ dst, size_t dstep, size_t dframe)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const size_t f = blockIdx.z;
    const uint32_t p = s.P[f * s.pf + (size_t)y * w + x];
    uint32_t lab = 0;
    if (p != BG) {
        uint32_t pos = p;
        if (ORDER == ccl::ORDER_BLOCK) { const int py = p / (uint32_t)w, px = p - py * w; pos = s.K[f * s.kf + ccl::blockKey(px, py, w)]; }
        if (pos < s.npos) lab = ccl::rank(s.chunk + f * s.cf, s.wpre + f * s.wf, reinterpret_cast<const uint64_t*>(s.B + f * s.bf), pos) + 1;
    }
    reinterpret_cast<T*>(dst + f * dframe + (size_t)y * dstep)[x] = (T)lab;
}

// ---- stats
__global__ __launch_bounds__(256) void k_ccl_stats_init(ccl::Acc* acc, int maxLabels)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < maxLabels) acc[(size_t)blockIdx.y * maxLabels + i] = ccl::accEmpty();
}

// a wave per (row, tile): the first pixel of every run of equal label inside a 64-column word makes the run's one update
template <typename T>
__global__ __launch_bounds__(256) void k_ccl_stats(const uchar* __restrict__ lab, size_t lstep, size_t lframe, int w, int h, const int* __restrict__ nlabels,
                                                   ccl::Acc* acc, int maxLabels)
{
    const int lane = threadIdx.x & 63, x0 = blockIdx.x * TILE_W, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    const T* row = reinterpret_cast<const T*>(lab + (size_t)blockIdx.z * lframe + (size_t)y * lstep);
    const uint32_t n = (uint32_t)nlabels[blockIdx.z];
    ccl::Acc* A = acc + (size_t)blockIdx.z * maxLabels;
#pragma unroll
    for (int j = 0; j < WORDS; j++) {
        const int x = x0 + 64 * j + lane;
        const bool valid = x < w;
        const uint32_t v = valid ? (uint32_t)row[x] : 0;
        const uint32_t left = __shfl_up(v, 1, 64);
        const uint64_t V = __ballot(valid), E = __ballot(valid && (lane == 0 || v != left));
        if (!(valid && ((E >> lane) & 1)) || v >= n) continue;                // a value that is no label of this frame is skipped, never indexed
        const uint64_t above = lane < 63 ? E >> (lane + 1) : 0;
        const uint32_t len = above ? (uint32_t)ccl::ctz64(above) + 1 : (uint32_t)(ccl::popc64(V) - lane);
        ccl::Acc* a = A + v;
        atomicAdd(&a->area, len);
        atomicAdd(&a->sx, (unsigned long long)ccl::runSumX((uint32_t)x, len));
        atomicAdd(&a->sy, (unsigned long long)y * len);
        atomicMin(&a->minx, x); atomicMax(&a->maxx, (int)(x + len - 1));
        atomicMin(&a->miny, y); atomicMax(&a->maxy, y);
    }
}

// rows from nlabels[frame] up to maxLabels are zero-filled (the batch entry; the single entry has maxLabels == nlabels)
__global__ __launch_bounds__(256) void k_ccl_stats_finish(const ccl::Acc* __restrict__ acc, const int* __restrict__ nlabels, int maxLabels,
                                                          uchar* __restrict__ stats, size_t sstep, size_t sframe, uchar* __restrict__ cent, size_t cstep, size_t cframe)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= maxLabels) return;
    const size_t f = blockIdx.y;
    int32_t* so = reinterpret_cast<int32_t*>(stats + f * sframe + (size_t)i * sstep);
    double* co = cent ? reinterpret_cast<double*>(cent + f * cframe + (size_t)i * cstep) : nullptr;
    if (i >= nlabels[f]) { so[0] = so[1] = so[2] = so[3] = so[4] = 0; if (co) co[0] = co[1] = 0.0; return; }
    ccl::accFinish(acc[f * maxLabels + i], so, co);
}

// ---- host side
struct Geom { uint32_t npos, nW, nchunk, nblocks; size_t pBytes, bBytes, wBytes, cBytes, kBytes, bytes; };
Geom geometry(int w, int h, int order)
{
    Geom q;
    q.nblocks = (uint32_t)((h + 1) >> 1) * (uint32_t)((w + 1) >> 1);
    q.npos = order == ccl::ORDER_BLOCK ? q.nblocks : (uint32_t)h * (uint32_t)w;
    q.nW = (q.npos + 63) >> 6;
    q.nchunk = (q.nW + ccl::CHUNK_WORDS - 1) / ccl::CHUNK_WORDS;
    q.pBytes = pad256((size_t)w * h * 4); q.bBytes = pad256((size_t)q.nW * 8); q.wBytes = pad256((size_t)q.nW * 4); q.cBytes = pad256((size_t)q.nchunk * 4);
    q.kBytes = order == ccl::ORDER_BLOCK ? pad256((size_t)q.nblocks * 4) : 0;
    q.bytes = q.pBytes + q.bBytes + q.wBytes + q.cBytes + q.kBytes;
    return q;
}

const char* typeName(int ltype) { return ltype == MI355CV_32S ? "32S" : "16U"; }

template <typename T>
void launchWrite(const Scr& s, int order, int w, int h, int nf, uchar* d, size_t dstep, size_t dframe, hipStream_t st)
{
    const dim3 grid(divUp(w, 256), h, nf);
    if (order == ccl::ORDER_BLOCK) hipLaunchKernelGGL((k_ccl_write<T, ccl::ORDER_BLOCK>), grid, dim3(256), 0, st, s, w, d, dstep, dframe);
    else hipLaunchKernelGGL((k_ccl_write<T, ccl::ORDER_PIXEL>), grid, dim3(256), 0, st, s, w, d, dstep, dframe);
}

// the refusals that need no device; 0 when the arguments are served
int cclArgs(const void* src, int w, int h, const void* labels, int nframes, int connectivity, int ltype, int ccltype, const int* nlabels)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!src || !labels || !nlabels || nframes < 1);
    if (connectivity != 4 && connectivity != 8) return MI355_DECLINED("connectivity is not 4 or 8");
    if (ltype != MI355CV_32S && ltype != MI355CV_16U) return MI355_DECLINED("ltype is not CV_32S or CV_16U");
    if (ccl::orderOf(connectivity, ccltype) < 0) return MI355_DECLINED("ccltype is not CCL_DEFAULT (-1) or one of 0 .. 5");
    // linear pixel indices and areas are 32-bit, coordinate sums stay below 2^53 (ccl_math.h)
    MI355_DECLINE_IF(w <= 0 || h <= 0 || w > lim::CCL_MAX_DIM || h > lim::CCL_MAX_DIM);
    return 0;
}

int runCCL(const char* entry, const uchar* src, size_t sstep, size_t sframe, int w, int h, uchar* labels, size_t lstep, size_t lframe, int nframes,
           int connectivity, int ltype, int ccltype, int* nlabels)
{
    if (const int rc = cclArgs(src, w, h, labels, nframes, connectivity, ltype, ccltype, nlabels)) return rc;
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_HEAVY)));
    const size_t e = depthBytes(ltype);
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + w, lspan = (size_t)(nframes - 1) * lframe + (size_t)(h - 1) * lstep + w * e;
    MI355_DECLINE_IF(overlapOnDevice(src, sspan, labels, lspan));
    size_t dss = sstep, dls = lstep;
    const uchar* ds = src; uchar* dl = labels;
    if (nframes == 1) {
        ds = stg.in(src, sstep, w, h, &dss);
        dl = stg.out(labels, lstep, w * e, h, &dls);
        MI355_DECLINE_IF(!ds || !dl);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(labels));

    const int order = ccl::orderOf(connectivity, ccltype), conn8 = connectivity == 8;
    const Geom q = geometry(w, h, order);
    // CV_16U: whether every frame's labels fit is known only after all frames are counted, and no destination may be written before: one group
    int group = (int)std::min<size_t>({(size_t)nframes, (size_t)65535, std::max<size_t>(1, (size_t(256) << 20) / q.bytes)});
    if (ltype == MI355CV_16U) { if (nframes > 65535) return MI355_DECLINED("nframes > 65535 with ltype CV_16U"); group = nframes; }
    uchar* scratch = (uchar*)stg.scratch(q.bytes * group + pad256((size_t)group * 4));
    uint32_t* hostN = (uint32_t*)stg.pinned((size_t)nframes * 4);
    if (!scratch || !hostN) return MI355_DECLINED("no scratch");
    Scr s;
    uchar* at = scratch;
    s.P = (uint32_t*)at; at += q.pBytes * group;
    s.B = (unsigned long long*)at; at += q.bBytes * group;
    s.wpre = (uint32_t*)at; at += q.wBytes * group;
    s.chunk = (uint32_t*)at; at += q.cBytes * group;
    s.K = (uint32_t*)at; at += q.kBytes * group;
    s.total = (uint32_t*)at;
    s.pf = q.pBytes / 4; s.bf = q.bBytes / 8; s.wf = q.wBytes / 4; s.cf = q.cBytes / 4; s.kf = q.kBytes / 4;
    s.nW = q.nW; s.nchunk = q.nchunk; s.npos = q.npos;
    hipStream_t st = stream();
    const int ntx = divUp(w, TILE_W), nstrips = divUp(h, STRIP_H);
    for (int f0 = 0; f0 < nframes; f0 += group) {
        const int nf = std::min(group, nframes - f0);
        const uchar* sp = ds + (size_t)f0 * sframe; uchar* lp = dl + (size_t)f0 * lframe;
        if (hipMemsetAsync(s.B, 0, q.bBytes * nf, st) != hipSuccess || (q.kBytes && hipMemsetAsync(s.K, 0xff, q.kBytes * nf, st) != hipSuccess))
            return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed: %s", entry, hipGetErrorString(hipGetLastError()));
        hipLaunchKernelGGL(k_ccl_strip, dim3(ntx, nstrips, nf), dim3(64), 0, st, sp, dss, sframe, w, h, conn8, s.P, s.pf);
        if (ntx > 1) hipLaunchKernelGGL(k_ccl_vseam, dim3(divUp(h, 64), ntx - 1, nf), dim3(64), 0, st, s.P, s.pf, w, h, conn8);
        if (nstrips > 1) hipLaunchKernelGGL(k_ccl_hseam, dim3(ntx, nstrips - 1, nf), dim3(64), 0, st, s.P, s.pf, w, conn8);
        if (order == ccl::ORDER_BLOCK) {
            hipLaunchKernelGGL(k_ccl_flatten<ccl::ORDER_BLOCK>, dim3(ntx, divUp(h, 4), nf), dim3(256), 0, st, s, w, h);
            hipLaunchKernelGGL(k_ccl_blockflags, dim3(divUp((int)q.nblocks, 256), 1, nf), dim3(256), 0, st, s, q.nblocks);
        } else hipLaunchKernelGGL(k_ccl_flatten<ccl::ORDER_PIXEL>, dim3(ntx, divUp(h, 4), nf), dim3(256), 0, st, s, w, h);
        hipLaunchKernelGGL(k_ccl_count, dim3(q.nchunk, 1, nf), dim3(256), 0, st, s);
        hipLaunchKernelGGL(k_ccl_scan, dim3(nf), dim3(1024), 0, st, s);
        if (ltype == MI355CV_32S) launchWrite<int32_t>(s, order, w, h, nf, lp, dls, lframe, st);
        if (hipMemcpyAsync(hostN + f0, s.total, (size_t)nf * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
            return setError(MI355CV_ERROR_UNKNOWN, "%s: D2H failed: %s", entry, hipGetErrorString(hipGetLastError()));
    }
    MI355_CHECK_LAUNCH(entry);
    if (hipStreamSynchronize(st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
    if (ltype == MI355CV_16U) {
        for (int f = 0; f < nframes; f++)
            if (hostN[f] > 65535) return MI355_DECLINED("ltype CV_16U and a frame has more than 65535 components (N - 1 > 65535)");
        launchWrite<unsigned short>(s, order, w, h, nframes, dl, dls, lframe, st);
    }
    for (int f = 0; f < nframes; f++) nlabels[f] = (int)hostN[f] + 1;
    noteKernel("k_ccl_strip<%s,%d,%s> grid=%dx%dx%d x64 lds=%zu, seams + k_ccl_flatten + scan + k_ccl_write, %d frame(s) in groups of %d",
               order == ccl::ORDER_BLOCK ? "block" : "pixel", connectivity, typeName(ltype), ntx, nstrips, std::min(group, nframes),
               sizeof(uint32_t) * STRIP_H * TILE_W + sizeof(uint64_t) * STRIP_H * WORDS, nframes, group);
    MI355_CHECK_LAUNCH(entry);
    return stg.finish(entry);
}

int statsArgs(const void* labels, int w, int h, int ltype, int nframes, const int* nlabels, int maxLabels, const void* stats)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!labels || !stats || !nlabels || nframes < 1);
    if (ltype != MI355CV_32S && ltype != MI355CV_16U) return MI355_DECLINED("ltype is not CV_32S or CV_16U");
    MI355_DECLINE_IF(w <= 0 || h <= 0 || w > lim::CCL_MAX_DIM || h > lim::CCL_MAX_DIM);
    MI355_DECLINE_IF(nframes > 65535);
    for (int f = 0; f < nframes; f++) if (nlabels[f] < 1) return MI355_DECLINED("nlabels < 1");
    for (int f = 0; f < nframes; f++) if (nlabels[f] > maxLabels) return MI355_DECLINED("nlabels > max_labels");
    return 0;
}

int runStats(const char* entry, const uchar* labels, size_t lstep, size_t lframe, int w, int h, int ltype, int nframes, const int* nlabels, int maxLabels,
             uchar* stats, size_t sstep, size_t sframe, uchar* cent, size_t cstep, size_t cframe, bool batch)
{
    if (const int rc = statsArgs(labels, w, h, ltype, nframes, nlabels, maxLabels, stats)) return rc;
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    if (batch && (!isDevicePtr(labels) || !isDevicePtr(stats) || (cent && !isDevicePtr(cent))))
        return MI355_DECLINED("labels, stats and centroids of a batch must be device-resident (host-resident frames are not served)");
    MI355_DECLINE_IF(hostImageTooSmall(labels, (size_t)w * h, minPixels(HOST_HEAVY)));
    const size_t e = depthBytes(ltype);
    const size_t lspan = (size_t)(nframes - 1) * lframe + (size_t)(h - 1) * lstep + w * e;
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(maxLabels - 1) * sstep + 20, cspan = (size_t)(nframes - 1) * cframe + (size_t)(maxLabels - 1) * cstep + 16;
    if (overlapOnDevice(labels, lspan, stats, sspan) || (cent && (overlapOnDevice(labels, lspan, cent, cspan) || overlapOnDevice(stats, sspan, cent, cspan))))
        return MI355_DECLINED("labels, stats and centroids overlap on the device");
    size_t dls = lstep, dss = sstep, dcs = cstep;
    const uchar* dl = labels; uchar* dst = stats; uchar* dc = cent;
    if (!batch) {
        // outputs live where the label image lives
        if (isDevicePtr(labels) != isDevicePtr(stats) || (cent && isDevicePtr(labels) != isDevicePtr(cent)))
            return MI355_DECLINED("stats and centroids must live where labels lives (all on the device or all on the host)");
        dl = stg.in(labels, lstep, w * e, h, &dls);
        dst = stg.out(stats, sstep, 20, maxLabels, &dss);
        if (cent) dc = stg.out(cent, cstep, 16, maxLabels, &dcs);
        MI355_DECLINE_IF(!dl || !dst || (cent && !dc));
    }
    ccl::Acc* acc = (ccl::Acc*)stg.scratch(sizeof(ccl::Acc) * (size_t)maxLabels * nframes);
    const int* dn = (const int*)stg.param(nlabels, (size_t)nframes * sizeof(int));
    if (!acc || !dn) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    const dim3 lgrid(divUp(maxLabels, 256), nframes);
    hipLaunchKernelGGL(k_ccl_stats_init, lgrid, dim3(256), 0, st, acc, maxLabels);
    const dim3 grid(divUp(w, TILE_W), divUp(h, 4), nframes);
    if (ltype == MI355CV_32S) hipLaunchKernelGGL(k_ccl_stats<int32_t>, grid, dim3(256), 0, st, dl, dls, lframe, w, h, dn, acc, maxLabels);
    else hipLaunchKernelGGL(k_ccl_stats<unsigned short>, grid, dim3(256), 0, st, dl, dls, lframe, w, h, dn, acc, maxLabels);
    hipLaunchKernelGGL(k_ccl_stats_finish, lgrid, dim3(256), 0, st, acc, dn, maxLabels, dst, dss, sframe, dc, dcs, cframe);
    noteKernel("k_ccl_stats<%s> grid=%dx%dx%d x256, k_ccl_stats_init + k_ccl_stats_finish grid=%dx%d x256, %d label row(s)", typeName(ltype), divUp(w, TILE_W), divUp(h, 4),
               nframes, divUp(maxLabels, 256), nframes, maxLabels);
    MI355_CHECK_LAUNCH(entry);
    return stg.finish(entry);
}

} // namespace

static_assert(lim::CCL_MAX_DIM == ccl::MAX_DIM, "one bound");
static_assert(sizeof(ccl::Acc) == 40, "accumulator layout");

extern "C" {

MI355CV_API int mi355cv_connectedComponents(const uchar* src_data, size_t src_step, int width, int height, uchar* labels_data, size_t labels_step,
                                            int connectivity, int ltype, int ccltype, int* nlabels)
{
    mi355::EntryGuard entry_(__func__);
    return runCCL("connectedComponents", src_data, src_step, 0, width, height, labels_data, labels_step, 0, 1, connectivity, ltype, ccltype, nlabels);
}

MI355CV_API int mi355cv_connectedComponentsBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height,
                                                 uchar* labels_data, size_t labels_step, size_t labels_frame_stride, int nframes,
                                                 int connectivity, int ltype, int ccltype, int* nlabels)
{
    mi355::EntryGuard entry_(__func__);
    if (const int rc = cclArgs(src_data, width, height, labels_data, nframes, connectivity, ltype, ccltype, nlabels)) return rc;
    if (hostBatchEligible(src_data, labels_data, nframes)) {        // frames in host memory
        const HostBatch hb = {src_data, src_step, src_frame_stride, (size_t)width, height, labels_data, labels_step, labels_frame_stride,
                              (size_t)width * depthBytes(ltype), height, nframes};
        int done = 0;                                               // the chunks come in frame order
        return runHostBatch("connectedComponentsBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            const int rc = mi355cv_connectedComponentsBatch(s, ss, sf, width, height, d, ds, df, nf, connectivity, ltype, ccltype, nlabels + done);
            done += nf;
            return rc; });
    }
    return runCCL("connectedComponentsBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, width, height, labels_data, labels_step,
                  nframes == 1 ? 0 : labels_frame_stride, nframes, connectivity, ltype, ccltype, nlabels);
}

MI355CV_API int mi355cv_connectedComponentsStats(const uchar* labels_data, size_t labels_step, int width, int height, int ltype, int nlabels,
                                                 int* stats, size_t stats_step, double* centroids, size_t centroids_step)
{
    mi355::EntryGuard entry_(__func__);
    return runStats("connectedComponentsStats", labels_data, labels_step, 0, width, height, ltype, 1, &nlabels, nlabels, (uchar*)stats, stats_step, 0,
                    (uchar*)centroids, centroids_step, 0, false);
}

MI355CV_API int mi355cv_connectedComponentsStatsBatch(const uchar* labels_data, size_t labels_step, size_t labels_frame_stride, int width, int height, int ltype,
                                                      int nframes, const int* nlabels, int max_labels, int* stats, size_t stats_step, size_t stats_frame_stride,
                                                      double* centroids, size_t centroids_step, size_t centroids_frame_stride)
{
    mi355::EntryGuard entry_(__func__);
    return runStats("connectedComponentsStatsBatch", labels_data, labels_step, labels_frame_stride, width, height, ltype, nframes, nlabels, max_labels,
                    (uchar*)stats, stats_step, stats_frame_stride, (uchar*)centroids, centroids_step, centroids_frame_stride, true);
}

} // extern "C"
