// clahe.hip -- cv::CLAHE::apply (imgproc/src/clahe.cpp; no HAL hook) on CV_8UC1 and CV_16UC1, single images and frame batches.
// Three launches in stream order per group of frames, the arithmetic in clahe_math.h:
//   k_clahe_hist8 / k_clahe_hist16   the tile histograms, each workgroup over one slice of one tile's rows, the padded rows / columns of the
//                                    LUT source read through BORDER_REFLECT_101 over the image plus its parent margins (no padded copy is made).
//                                    Each slice writes its partial histogram with plain stores to a slab of its own: no memset, no global atomics,
//                                    and the sums are the same whatever the order the workgroups run in.
//                                    8U: 256 bins, one LDS sub-histogram per wave.  16U: 65 536 bins as 16-bit counters in 128 KiB of LDS (two per
//                                    32-bit word), slices of at most 65 535 pixels so that no counter carries into its neighbour.
//   k_clahe_lut8 / k_clahe_lut16     one workgroup per (frame, tile): the slabs summed, clip and redistribution per bin in closed form, a block prefix scan,
//                                    the float scale and round-half-even -- integer sums are exact in any order, so this equals the reference's serial loop
//   k_clahe_interp8 / 16             per pixel, bilinear blend of four tile LUTs; 16-byte loads and stores per lane.  8U stages the LUT rows of the tile rows
//                                    a workgroup touches in LDS; 16U gathers from the LUTs in global memory (128 KiB per tile).
#include "rt.h"
#include "clahe_math.h"
#include <algorithm>

using namespace mi355;

namespace {

constexpr int HIST16_LDS = 65536 * 2;          // bytes of the 16-bit counters
constexpr int SLICE16_MAX = 65535;             // pixels per 16U slice: a 16-bit counter never overflows
constexpr int INTERP_ROWS = 4;                 // image rows per interpolation workgroup
constexpr size_t GROUP_SCRATCH = 256u << 20;   // slabs + LUTs of one group of frames

// inclusive prefix sum over a block of NT threads (NT a multiple of 64); *total receives the block's sum
template <int NT>
__device__ __forceinline__ int blockScan(int v, int* total)
{
    __shared__ int waveSum[NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) waveSum[w] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < NT / 64; i++) { const int s = waveSum[i]; before += i < w ? s : 0; all += s; }
    __syncthreads();                           // waveSum is reused by the next call
    *total = all;
    return v + before;
}

// rows of a tile slice spread over the block: `lanesPerRow` threads per row, `rowsPerPass` rows at a time
struct RowSplit { int lanesPerRow, rowsPerPass, rr, cc; };
__device__ __forceinline__ RowSplit rowSplit(int m, int nt)
{
    RowSplit s;
    s.lanesPerRow = m < nt ? m : nt;
    s.rowsPerPass = nt / s.lanesPerRow;
    s.rr = threadIdx.x / s.lanesPerRow;
    s.cc = threadIdx.x - s.rr * s.lanesPerRow;
    return s;
}

// histogram of one slice (blockIdx.x = tile * S + slice, blockIdx.y = frame of the group) into slab[frame][tile][slice][256]
__global__ __launch_bounds__(256) void k_clahe_hist8(const uchar* __restrict__ src, size_t sstep, size_t sframe, int tilesX, int tw, int th, int readW,
                                                     int readH, int S, int rowsPerSlice, unsigned* __restrict__ slab)
{
    __shared__ unsigned h[4][256];
    for (int i = threadIdx.x; i < 1024; i += 256) (&h[0][0])[i] = 0;
    __syncthreads();
    unsigned* mine = h[threadIdx.x >> 6];
    const int k = blockIdx.x / S, s = blockIdx.x - k * S;
    const int ty = k / tilesX, tx = k - ty * tilesX;
    const int x0 = tx * tw, xr = min(x0 + tw, readW);
    const int yb = ty * th + s * rowsPerSlice, nr = min(rowsPerSlice, th - s * rowsPerSlice);
    const uchar* base = src + (size_t)blockIdx.y * sframe;
    // real columns [x0, xr) as 16-byte vectors where every row of the tile starts on a 16-byte boundary; the rest (tail, padded columns) byte by byte
    const int nvec = (((uintptr_t)(base + x0) | sstep) & 15) == 0 && xr > x0 ? (xr - x0) >> 4 : 0;
    if (nvec > 0) {
        const RowSplit q = rowSplit(nvec, 256);
        if (q.rr < q.rowsPerPass)
            for (int r = q.rr; r < nr; r += q.rowsPerPass) {
                const uint4* row = (const uint4*)(base + (size_t)clahe::reflect101(yb + r, readH) * sstep + x0);
                for (int c = q.cc; c < nvec; c += q.lanesPerRow) {
                    const uint4 v = row[c];
                    const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        atomicAdd(&mine[w4[j] & 255], 1u); atomicAdd(&mine[(w4[j] >> 8) & 255], 1u);
                        atomicAdd(&mine[(w4[j] >> 16) & 255], 1u); atomicAdd(&mine[w4[j] >> 24], 1u);
                    }
                }
            }
    }
    const int xs = x0 + nvec * 16, m = x0 + tw - xs;
    if (m > 0) {
        const RowSplit q = rowSplit(m, 256);
        if (q.rr < q.rowsPerPass)
            for (int r = q.rr; r < nr; r += q.rowsPerPass) {
                const uchar* row = base + (size_t)clahe::reflect101(yb + r, readH) * sstep;
                for (int c = q.cc; c < m; c += q.lanesPerRow) atomicAdd(&mine[row[clahe::reflect101(xs + c, readW)]], 1u);
            }
    }
    __syncthreads();
    const int t = threadIdx.x;
    slab[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + t] = h[0][t] + h[1][t] + h[2][t] + h[3][t];
}

// 16U: the slice is rows [sy * rowsPerSlice, ...) x columns [sx * colsPerSlice, ...) of the tile, at most SLICE16_MAX pixels; slab entries are 16-bit
__global__ __launch_bounds__(1024) void k_clahe_hist16(const uchar* __restrict__ src, size_t sstep, size_t sframe, int tilesX, int tw, int th, int readW,
                                                       int readH, int S, int nsx, int rowsPerSlice, int colsPerSlice, unsigned short* __restrict__ slab)
{
    extern __shared__ __attribute__((aligned(16))) unsigned cnt[];       // bin 2j in the low half of word j, bin 2j + 1 in the high half
    uint4* c4 = reinterpret_cast<uint4*>(cnt);
    for (int i = threadIdx.x; i < HIST16_LDS / 16; i += 1024) c4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const int k = blockIdx.x / S, s = blockIdx.x - k * S;
    const int sy = s / nsx, sx = s - sy * nsx;
    const int ty = k / tilesX, tx = k - ty * tilesX;
    const int xb = tx * tw + sx * colsPerSlice, m = min(colsPerSlice, tw - sx * colsPerSlice);
    const int yb = ty * th + sy * rowsPerSlice, nr = min(rowsPerSlice, th - sy * rowsPerSlice);
    const uchar* base = src + (size_t)blockIdx.y * sframe;
    const RowSplit q = rowSplit(m, 1024);
    if (q.rr < q.rowsPerPass)
        for (int r = q.rr; r < nr; r += q.rowsPerPass) {
            const unsigned short* row = (const unsigned short*)(base + (size_t)clahe::reflect101(yb + r, readH) * sstep);
            for (int c = q.cc; c < m; c += q.lanesPerRow) {
                const unsigned v = row[clahe::reflect101(xb + c, readW)];
                atomicAdd(&cnt[v >> 1], 1u << ((v & 1) << 4));
            }
        }
    __syncthreads();
    uint4* out = reinterpret_cast<uint4*>(slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 65536);
    for (int i = threadIdx.x; i < HIST16_LDS / 16; i += 1024) out[i] = c4[i];
}

// one workgroup per (frame, tile) of the group, bin i on thread i
__global__ __launch_bounds__(256) void k_clahe_lut8(const unsigned* __restrict__ slab, int S, int clip, float lutScale, uchar* __restrict__ lut)
{
    const int i = threadIdx.x;
    const unsigned* p = slab + (size_t)blockIdx.x * S * 256 + i;
    int h = 0;
    for (int s = 0; s < S; s++) h += (int)p[(size_t)s * 256];
    if (clip > 0) {
        int clipped;
        (void)blockScan<256>(clahe::excess(h, clip), &clipped);
        h = clahe::binAfterClip(h, i, clip, clahe::redist(clipped, 256));
    }
    int total;
    const int sum = blockScan<256>(h, &total);
    lut[(size_t)blockIdx.x * 256 + i] = (uchar)clahe::lutEntry(sum, lutScale, 255);
}

// 16U: thread t owns bins [64 t, 64 t + 64)
__global__ __launch_bounds__(1024) void k_clahe_lut16(const unsigned short* __restrict__ slab, int S, int clip, float lutScale, unsigned short* __restrict__ lut)
{
    const int t = threadIdx.x, i0 = t * 64;
    int h[64];
#pragma unroll
    for (int j = 0; j < 64; j++) h[j] = 0;
    for (int s = 0; s < S; s++) {
        const uint4* p = reinterpret_cast<const uint4*>(slab + ((size_t)blockIdx.x * S + s) * 65536 + i0);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint4 v = p[q];
            const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++) { h[q * 8 + 2 * j] += (int)(w4[j] & 0xffff); h[q * 8 + 2 * j + 1] += (int)(w4[j] >> 16); }
        }
    }
    if (clip > 0) {
        int e = 0;
#pragma unroll
        for (int j = 0; j < 64; j++) e += clahe::excess(h[j], clip);
        int clipped;
        (void)blockScan<1024>(e, &clipped);
        const clahe::Redist r = clahe::redist(clipped, 65536);
#pragma unroll
        for (int j = 0; j < 64; j++) h[j] = clahe::binAfterClip(h[j], i0 + j, clip, r);
    }
    int local = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) local += h[j];
    int total;
    int sum = blockScan<1024>(local, &total) - local;
    uint4* out = reinterpret_cast<uint4*>(lut + (size_t)blockIdx.x * 65536 + i0);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        unsigned w4[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            sum += h[q * 8 + 2 * j];
            const unsigned lo = (unsigned)clahe::lutEntry(sum, lutScale, 65535);
            sum += h[q * 8 + 2 * j + 1];
            w4[j] = lo | (unsigned)clahe::lutEntry(sum, lutScale, 65535) << 16;
        }
        out[q] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    }
}

struct InterpArgs {
    int W, H, tilesX, tilesY;
    float invTw, invTh;
    int maxRows;     // LUT rows (tile rows) staged per workgroup (8U)
    int vec;         // every row of source and destination starts on a 16-byte boundary
};

// 8U: blockIdx.x = INTERP_ROWS image rows, blockIdx.y = frame of the group; lanes take 16-pixel chunks of those rows
template <bool STAGED>
__global__ __launch_bounds__(256) void k_clahe_interp8(const uchar* __restrict__ src, size_t sstep, size_t sframe, uchar* dst, size_t dstep, size_t dframe,
                                                       InterpArgs a, const uchar* __restrict__ lut)
{
    extern __shared__ __attribute__((aligned(16))) uchar slut[];
    const int y0 = blockIdx.x * INTERP_ROWS, y1 = min(y0 + INTERP_ROWS, a.H);
    const uchar* flut = lut + (size_t)blockIdx.y * a.tilesX * a.tilesY * 256;
    const uchar* L = flut;
    int tlo = 0;
    if constexpr (STAGED) {
        // the tile rows of [y0, y1): the tile indices grow with y, so rows y0 and y1 - 1 bound them
        tlo = clahe::axis(y0, a.invTh, a.tilesY).t1;
        const int nrows = min(clahe::axis(y1 - 1, a.invTh, a.tilesY).t2 - tlo + 1, a.maxRows);
        const uint4* g = reinterpret_cast<const uint4*>(flut + (size_t)tlo * a.tilesX * 256);
        uint4* l4 = reinterpret_cast<uint4*>(slut);
        for (int i = threadIdx.x; i < nrows * a.tilesX * 16; i += 256) l4[i] = g[i];
        __syncthreads();
        L = slut;
    }
    src += (size_t)blockIdx.y * sframe;
    dst += (size_t)blockIdx.y * dframe;
    const int nch = (a.W + 15) >> 4;
    for (int i = threadIdx.x; i < (y1 - y0) * nch; i += 256) {
        const int r = i / nch, x0 = (i - r * nch) * 16, y = y0 + r;
        const clahe::Axis ay = clahe::axis(y, a.invTh, a.tilesY);
        const uchar* L1 = L + (size_t)(ay.t1 - tlo) * a.tilesX * 256;
        const uchar* L2 = L + (size_t)(ay.t2 - tlo) * a.tilesX * 256;
        const uchar* s = src + (size_t)y * sstep + x0;
        uchar* d = dst + (size_t)y * dstep + x0;
        if (a.vec && x0 + 16 <= a.W) {
            const uint4 v = *reinterpret_cast<const uint4*>(s);
            const unsigned w4[4] = {v.x, v.y, v.z, v.w};
            unsigned o4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                unsigned o = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int px = (w4[j] >> (8 * b)) & 255;
                    const clahe::Axis ax = clahe::axis(x0 + 4 * j + b, a.invTw, a.tilesX);
                    const int t1 = ax.t1 * 256 + px, t2 = ax.t2 * 256 + px;
                    o |= (unsigned)clahe::blend(L1[t1], L1[t2], L2[t1], L2[t2], ax, ay, 255) << (8 * b);
                }
                o4[j] = o;
            }
            *reinterpret_cast<uint4*>(d) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        } else {
            for (int b = 0; b < 16 && x0 + b < a.W; b++) {
                const int px = s[b];
                const clahe::Axis ax = clahe::axis(x0 + b, a.invTw, a.tilesX);
                const int t1 = ax.t1 * 256 + px, t2 = ax.t2 * 256 + px;
                d[b] = (uchar)clahe::blend(L1[t1], L1[t2], L2[t1], L2[t2], ax, ay, 255);
            }
        }
    }
}

// 16U: 8-pixel chunks, the four LUT entries gathered from global memory
__global__ __launch_bounds__(256) void k_clahe_interp16(const uchar* __restrict__ src, size_t sstep, size_t sframe, uchar* dst, size_t dstep, size_t dframe,
                                                        InterpArgs a, const unsigned short* __restrict__ lut)
{
    const int y0 = blockIdx.x * INTERP_ROWS, y1 = min(y0 + INTERP_ROWS, a.H);
    const unsigned short* flut = lut + (size_t)blockIdx.y * a.tilesX * a.tilesY * 65536;
    src += (size_t)blockIdx.y * sframe;
    dst += (size_t)blockIdx.y * dframe;
    const int nch = (a.W + 7) >> 3;
    for (int i = threadIdx.x; i < (y1 - y0) * nch; i += 256) {
        const int r = i / nch, x0 = (i - r * nch) * 8, y = y0 + r;
        const clahe::Axis ay = clahe::axis(y, a.invTh, a.tilesY);
        const unsigned short* L1 = flut + (size_t)ay.t1 * a.tilesX * 65536;
        const unsigned short* L2 = flut + (size_t)ay.t2 * a.tilesX * 65536;
        const unsigned short* s = reinterpret_cast<const unsigned short*>(src + (size_t)y * sstep) + x0;
        unsigned short* d = reinterpret_cast<unsigned short*>(dst + (size_t)y * dstep) + x0;
        if (a.vec && x0 + 8 <= a.W) {
            const uint4 v = *reinterpret_cast<const uint4*>(s);
            const unsigned w4[4] = {v.x, v.y, v.z, v.w};
            unsigned o4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                unsigned o = 0;
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    const unsigned px = (w4[j] >> (16 * b)) & 0xffff;
                    const clahe::Axis ax = clahe::axis(x0 + 2 * j + b, a.invTw, a.tilesX);
                    const size_t t1 = (size_t)ax.t1 * 65536 + px, t2 = (size_t)ax.t2 * 65536 + px;
                    o |= (unsigned)clahe::blend(L1[t1], L1[t2], L2[t1], L2[t2], ax, ay, 65535) << (16 * b);
                }
                o4[j] = o;
            }
            *reinterpret_cast<uint4*>(d) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        } else {
            for (int b = 0; b < 8 && x0 + b < a.W; b++) {
                const unsigned px = s[b];
                const clahe::Axis ax = clahe::axis(x0 + b, a.invTw, a.tilesX);
                const size_t t1 = (size_t)ax.t1 * 65536 + px, t2 = (size_t)ax.t2 * 65536 + px;
                d[b] = (unsigned short)clahe::blend(L1[t1], L1[t2], L2[t1], L2[t2], ax, ay, 65535);
            }
        }
    }
}

// CLAHE of `nframes` device-resident frames of one geometry (frame strides in bytes), the source readable over p.readW x p.readH
int claheFrames(Stager& stg, const char* entry, const uchar* ds, size_t dss, size_t dsf, uchar* dd, size_t dds, size_t ddf, int nframes, int W, int H,
                int depth, const clahe::Plan& p)
{
    const bool u16 = depth == MI355CV_16U;
    const int histSize = u16 ? 65536 : 256, e = u16 ? 2 : 1;
    const long long nT = (long long)p.tilesX * p.tilesY;
    // slices per tile: 8U splits the rows until the histogram launch has ~2048 workgroups; 16U cuts slices of <= 65 535 pixels, more of them for a single frame
    int S, nsx = 1, rowsPerSlice, colsPerSlice = p.tw;
    if (!u16) {
        const long long want = std::max(1LL, std::min<long long>(p.th, (2048 + nT * nframes - 1) / (nT * nframes)));
        rowsPerSlice = divUp(p.th, (int)want);
        S = divUp(p.th, rowsPerSlice);
    } else {
        colsPerSlice = p.tw <= SLICE16_MAX ? p.tw : 32768;
        nsx = divUp(p.tw, colsPerSlice);
        rowsPerSlice = std::max(1, SLICE16_MAX / colsPerSlice);
        const long long want = std::min<long long>(p.th, (256 + nT * nsx * nframes - 1) / (nT * nsx * nframes));
        if (want > divUp(p.th, rowsPerSlice)) rowsPerSlice = divUp(p.th, (int)want);
        S = nsx * divUp(p.th, rowsPerSlice);
    }
    const size_t slabFrame = (size_t)nT * S * histSize * (u16 ? 2 : 4), lutFrame = (size_t)nT * histSize * e;
    if ((double)nT * S > 2e9) return declined(entry, __LINE__, "tiles x slices beyond one launch");
    const int G = (int)std::max<size_t>(1, std::min<size_t>({(size_t)nframes, GROUP_SCRATCH / (slabFrame + lutFrame), 65535}));
    uchar* slab = (uchar*)stg.scratch(slabFrame * G);
    uchar* lut = (uchar*)stg.scratch(lutFrame * G);
    if (!slab || !lut) return declined(entry, __LINE__, "!slab || !lut (scratch of frames x tilesX x tilesY x histSize)");

    hipStream_t st = stream();
    InterpArgs a;
    a.W = W; a.H = H; a.tilesX = p.tilesX; a.tilesY = p.tilesY;
    a.invTw = 1.0f / (float)p.tw; a.invTh = 1.0f / (float)p.th;
    a.maxRows = std::min(p.tilesY, (INTERP_ROWS - 1) / p.th + 4);
    a.vec = ((((uintptr_t)ds | dss | dsf | (uintptr_t)dd | dds | ddf) & 15) == 0) ? 1 : 0;
    const size_t stageBytes = (size_t)a.maxRows * p.tilesX * 256;
    const bool staged = !u16 && stageBytes <= 32 * 1024;
    if (u16) {
        static bool attrSet[16] = {};
        const int dv = activeDevice() & 15;
        if (!attrSet[dv]) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_clahe_hist16), hipFuncAttributeMaxDynamicSharedMemorySize, HIST16_LDS); attrSet[dv] = true; }
    }
    for (int f0 = 0; f0 < nframes; f0 += G) {
        const int g = std::min(G, nframes - f0);
        const uchar* s = ds + (size_t)f0 * dsf;
        uchar* d = dd + (size_t)f0 * ddf;
        const dim3 hgrid((unsigned)(nT * S), (unsigned)g);
        const dim3 igrid((unsigned)divUp(H, INTERP_ROWS), (unsigned)g);
        if (!u16) {
            hipLaunchKernelGGL(k_clahe_hist8, hgrid, dim3(256), 0, st, s, dss, dsf, p.tilesX, p.tw, p.th, p.readW, p.readH, S, rowsPerSlice, (unsigned*)slab);
            hipLaunchKernelGGL(k_clahe_lut8, dim3((unsigned)(nT * g)), dim3(256), 0, st, (const unsigned*)slab, S, p.clip, p.lutScale, lut);
            if (staged) hipLaunchKernelGGL(k_clahe_interp8<true>, igrid, dim3(256), stageBytes, st, s, dss, dsf, d, dds, ddf, a, lut);
            else        hipLaunchKernelGGL(k_clahe_interp8<false>, igrid, dim3(256), 0, st, s, dss, dsf, d, dds, ddf, a, lut);
        } else {
            hipLaunchKernelGGL(k_clahe_hist16, hgrid, dim3(1024), HIST16_LDS, st, s, dss, dsf, p.tilesX, p.tw, p.th, p.readW, p.readH, S, nsx, rowsPerSlice, colsPerSlice,
                               (unsigned short*)slab);
            hipLaunchKernelGGL(k_clahe_lut16, dim3((unsigned)(nT * g)), dim3(1024), 0, st, (const unsigned short*)slab, S, p.clip, p.lutScale, (unsigned short*)lut);
            hipLaunchKernelGGL(k_clahe_interp16, igrid, dim3(256), 0, st, s, dss, dsf, d, dds, ddf, a, (const unsigned short*)lut);
        }
        MI355_CHECK_LAUNCH(entry);
    }
    noteKernel("k_clahe_hist%d + k_clahe_lut%d + k_clahe_interp%d%s tiles=%dx%d slices=%d frames=%d/launch", u16 ? 16 : 8, u16 ? 16 : 8, u16 ? 16 : 8,
               u16 ? "" : staged ? "<staged>" : "<global>", p.tilesX, p.tilesY, S, G);
    return MI355CV_OK;
}

bool claheArgs(int width, int height, int depth, int margin_right, int margin_bottom, double clipLimit, int tilesX, int tilesY, clahe::Plan& p)
{
    if (depth != MI355CV_8U && depth != MI355CV_16U) return false;
    return clahe::plan(width, height, margin_right, margin_bottom, tilesX, tilesY, clipLimit, depth == MI355CV_8U ? 256 : 65536, p);
}

} // namespace

extern "C" {

// Host-resident images are staged (HOST_HEAVY): the reference's CPU path walks every pixel twice through scalar table lookups, and its 16-bit form builds a
// 65 536-entry LUT per tile.  The staged call costs 1.7 ms (8U) / 3.3 ms (16U) per 4K frame (tools/clahe_bench.py, profiles/clahe_bench.jsonl), PCIe included.
MI355CV_API int mi355cv_clahe(const uchar* src_data, size_t src_step, uchar* dst_data, size_t dst_step, int width, int height, int depth,
                              int margin_right, int margin_bottom, double clipLimit, int tilesX, int tilesY)
{
    mi355::EntryGuard entry_(__func__);
    clahe::Plan p;
    MI355_DECLINE_IF(disabled() || !src_data || !dst_data);
    MI355_DECLINE_IF(depth != MI355CV_8U && depth != MI355CV_16U);
    if (!claheArgs(width, height, depth, margin_right, margin_bottom, clipLimit, tilesX, tilesY, p))
        return MI355_DECLINED("width <= 0 || height <= 0 || tilesX <= 0 || tilesY <= 0 || margins < 0 || tile area beyond int");
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src_data, (size_t)width * height, minPixels(HOST_HEAVY)));
    const int e = depth == MI355CV_8U ? 1 : 2;
    size_t dss, dds;
    const uchar* ds = stg.in(src_data, src_step, (size_t)p.readW * e, p.readH, &dss);      // the parent margins the padding takes in travel with the image
    uchar* dd = stg.out(dst_data, dst_step, (size_t)width * e, height, &dds);
    MI355_DECLINE_IF(!ds || !dd);
    const int rc = claheFrames(stg, "mi355cv_clahe", ds, dss, 0, dd, dds, 0, 1, width, height, depth, p);
    if (rc != MI355CV_OK) return rc;
    return stg.finish("clahe");
}

// `nframes` whole frames of one geometry (no parent margins), strides in bytes, both ends in HBM or both in host memory
MI355CV_API int mi355cv_claheBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, uchar* dst_data, size_t dst_step, size_t dst_frame_stride,
                                   int nframes, int width, int height, int depth, double clipLimit, int tilesX, int tilesY)
{
    mi355::EntryGuard entry_(__func__);
    clahe::Plan p;
    MI355_DECLINE_IF(disabled() || !src_data || !dst_data || nframes < 1);
    if (!claheArgs(width, height, depth, 0, 0, clipLimit, tilesX, tilesY, p))
        return MI355_DECLINED("depth not 8U / 16U || width <= 0 || height <= 0 || tilesX <= 0 || tilesY <= 0 || tile area beyond int");
    const size_t rowBytes = (size_t)width * (depth == MI355CV_8U ? 1 : 2);
    if (hostBatchEligible(src_data, dst_data, nframes)) {                                       // frames in host memory: chunks through two sets of device buffers
        const HostBatch hb = {src_data, src_step, src_frame_stride, rowBytes, height, dst_data, dst_step, dst_frame_stride, rowBytes, height, nframes};
        return runHostBatch("claheBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_claheBatch(s, ss, sf, d, ds, df, nf, width, height, depth, clipLimit, tilesX, tilesY); });
    }
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    if (!ensureDevice() || !isDevicePtr(src_data) || !isDevicePtr(dst_data)) return setError(MI355CV_NOT_IMPLEMENTED, "claheBatch: device-resident frames only");
    const int rc = claheFrames(stg, "mi355cv_claheBatch", src_data, src_step, src_frame_stride, dst_data, dst_step, dst_frame_stride, nframes, width, height, depth, p);
    if (rc != MI355CV_OK) return rc;
    return stg.finish("claheBatch");
}

} // extern "C"
