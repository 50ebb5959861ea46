// calchist.hip -- cv::calcHist and cv::calcBackProject: one interleaved image of 1-4 channels (CV_8U, CV_16U, CV_32F), a dense histogram of 1-3 dimensions over any
// of its channels, uniform or (8- and 16-bit) non-uniform ranges, an optional CV_8UC1 mask; single frames and batches (mi355cv_calcHist, ...Batch,
// mi355cv_calcBackProject, ...Batch).  The bin rule, the tables, the roundings are in calchist_math.h, which the CPU suite compiles for the host.  The reference
// was not available: the definition is this project's restatement, tests/calchist_restate.py, and the kernels are held against it bit for bit.
//
// The counts are exact int32 and are counted IN PLACE in the destination's own 4-byte cells:
//   k_calchist_convert<toInt>     accumulate into a CV_32F histogram: float -> int32 in place before the count (without accumulate the cells are cleared),
//   k_calchist_lds / _generic     the count,
//   k_calchist_convert<toFloat>   int32 -> float in place for a CV_32F histogram.
// Integer atomic adds commute, so every result is independent of scheduling.  A fixed number of launches whatever the number of frames.
//
//   k_calchist_lds<CN, masked>   CV_8U whenever tables and cells fit the workgroup's LDS.  grid (P, frames).  A row is cut at its own 16-byte boundaries into a
//                    scalar head, whole units (16 bytes; 48 bytes = 16 pixels for three channels: the least run in which pixels and 16-byte lines meet again) read
//                    with dwordx4 loads, and a scalar tail; nothing outside [row, row + width * cn) is read.  A row whose address admits no pixel on a 16-byte
//                    boundary (an odd base with two channels) is read byte by byte.  Per dimension a 256-entry LDS table gives the pre-multiplied cell offset or
//                    calchist::SKIP; the sum of a pixel's entries is its cell, negative = not counted.  Counts go by ds_add into `copies` private histograms, the
//                    copy chosen BY LANE (lane % copies) with an odd stride between copies: the 64 lanes of a wave that meet one cell (a flat image) then hit
//                    `copies` different banks instead of one address.  A lane also keeps (cell, run length) of its latest pixels in registers and adds the run
//                    only when the cell changes, so a flat or slowly varying image costs one atomic per run instead of one per pixel.  The copies are summed at
//                    the end and added to the frame's cells with one global atomic per non-empty cell.
//   k_calchist_generic<depth, masked>   everything else: CV_16U (a 65536-entry table per dimension in HBM / L2), CV_32F (the bin computed with __dmul_rn /
//                    __dadd_rn) and CV_8U histograms too large for LDS.  One pixel per lane and pass, a vector atomic add on the int32 cell.  A wave whose active
//                    lanes all hold the SAME cell (a flat image) sends one add of the lane count instead of 64 adds to one address.
//   k_backproject<depth>   per frame: 8-bit tables in LDS; when the histogram fits (<= 8192 cells) every workgroup first turns it into OUTPUT values
//                    (hist * scale, rounded, saturated) in LDS, and for one CV_8U dimension folds table and outputs into one 256-entry table indexed by the pixel;
//                    larger histograms are gathered from L2 and converted per pixel.  A lane produces 4 bytes of destination, stored as one dword where the lane's
//                    pixels lie inside the row (the groups are cut at the destination row's own 4-byte boundaries).
#include "rt.h"
#include "calchist_math.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mi355;

namespace {

using calchist::SKIP;

struct Bins {                                    // by value to the kernels
    int dims, cn;
    int sh[3];                                   // 8 * channel: the byte of a packed CV_8U pixel
    int ch[3], n[3], mult[3];
    double a[3], b[3];                           // CV_32F: t = v * a + b
};

template <bool TO_INT> __global__ __launch_bounds__(256) void k_calchist_convert(int32_t* __restrict__ cells, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if (TO_INT) cells[i] = calchist::countOfFloat(__int_as_float(cells[i]));
        else cells[i] = __float_as_int(calchist::floatOfCount(cells[i]));
    }
}

template <int CN> struct Unit {                  // what a lane reads at once
    static constexpr int PX = CN == 1 ? 16 : CN == 2 ? 8 : CN == 3 ? 16 : 4;
    static constexpr int BYTES = PX * CN;
};

// pixels before the first one that starts on a 16-byte boundary, -1 if no pixel of the row ever does
template <int CN> __device__ __forceinline__ int headPixels(const uchar* rp)
{
    const int m = (int)((16 - ((uintptr_t)rp & 15)) & 15);
    if (CN == 1) return m;
    if (CN == 3) return (11 * m) & 15;           // 3 * 11 = 33 = 1 (mod 16)
    if (CN == 2) return (m & 1) ? -1 : m >> 1;
    return (m & 3) ? -1 : m >> 2;
}

template <int CN> __device__ __forceinline__ uint32_t packPixel(const uchar* p)
{
    uint32_t v = p[0];
    if (CN > 1) v |= (uint32_t)p[1] << 8;
    if (CN > 2) v |= (uint32_t)p[2] << 16;
    if (CN > 3) v |= (uint32_t)p[3] << 24;
    return v;
}

// pixel p of a unit held as little-endian words; p is a constant after unrolling, so every index and shift below is one too
template <int CN> __device__ __forceinline__ uint32_t pixelOfWords(const uint32_t* wd, int p)
{
    const int i = p * CN, q = i >> 2, s = 8 * (i & 3);
    uint32_t v = wd[q] >> s;
    if ((i & 3) + CN > 4) v |= wd[q + 1] << (32 - s);
    return CN == 4 ? v : v & ((1u << (8 * CN)) - 1u);
}

__device__ __forceinline__ int cellOf8(uint32_t pix, const int32_t* T, const Bins& B)
{
    int off = T[(pix >> B.sh[0]) & 255u];
    if (B.dims > 1) off += T[256 + ((pix >> B.sh[1]) & 255u)];
    if (B.dims > 2) off += T[512 + ((pix >> B.sh[2]) & 255u)];
    return off;
}

template <int CN, bool MASKED>
__global__ __launch_bounds__(256) void k_calchist_lds(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h, const uchar* __restrict__ mask,
                                                      size_t mstep, size_t mframe, const int32_t* __restrict__ tabs, Bins B, int cells, int copies, int cstride,
                                                      uint32_t nI, int32_t* __restrict__ hist)
{
    constexpr int PX = Unit<CN>::PX, UB = Unit<CN>::BYTES;
    extern __shared__ int32_t lds[];
    int32_t* T = lds;                                                        // [3][256]
    uint32_t* C = reinterpret_cast<uint32_t*>(lds + 768);                    // [copies][cstride]
    for (int i = threadIdx.x; i < 768; i += 256) T[i] = i < B.dims * 256 ? tabs[i] : 0;
    for (int i = threadIdx.x; i < copies * cstride; i += 256) C[i] = 0;
    __syncthreads();
    uint32_t* mine = C + (threadIdx.x & (copies - 1)) * cstride;            // the private copy BY LANE: 64 lanes that meet one cell hit `copies` addresses
    const uchar* S = src + (size_t)blockIdx.y * sframe;
    const uchar* M = MASKED ? mask + (size_t)blockIdx.y * mframe : nullptr;
    const uint32_t TT = gridDim.x * 256u, items = (uint32_t)h * nI;          // items <= 16384 * 4098
    uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t row = t / nI, j = t - row * nI;
    const uint32_t dr = TT / nI, dj = TT - dr * nI;
    int prev = -1;                                                           // the lane's open run: cell and length
    uint32_t run = 0;
    auto count = [&](int off) {
        if (off < 0) return;
        if (off == prev) { run++; return; }
        if (prev >= 0) atomicAdd(&mine[prev], run);
        prev = off; run = 1;
    };
    for (; t < items; t += TT) {
        const uchar* rp = S + (size_t)row * sstep;
        const uchar* mp = MASKED ? M + (size_t)row * mstep : nullptr;
        const int k = headPixels<CN>(rp);
        const bool aligned = k >= 0;
        const int k0 = aligned ? min(k, w) : 0;
        const int nunits = (w - k0) / PX;
        if (j >= 1 && (int)j <= nunits) {
            const int x0 = k0 + ((int)j - 1) * PX;
            uint32_t wd[UB / 4];
            if (aligned) {
#pragma unroll
                for (int q = 0; q < UB / 16; q++) {
                    const uint4 v = *reinterpret_cast<const uint4*>(rp + (size_t)x0 * CN + 16 * q);
                    wd[4 * q] = v.x; wd[4 * q + 1] = v.y; wd[4 * q + 2] = v.z; wd[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < UB / 4; q++) wd[q] = packPixel<4>(rp + (size_t)x0 * CN + 4 * q);
            }
            uchar m[PX];
            if (MASKED) __builtin_memcpy(m, mp + x0, PX);
#pragma unroll
            for (int p = 0; p < PX; p++) {
                const int off = cellOf8(pixelOfWords<CN>(wd, p), T, B);
                count(MASKED && !m[p] ? -1 : off);
            }
        } else if (j == 0 || j == nI - 1) {                                  // the head, or the tail
            const int xa = j == 0 ? 0 : k0 + nunits * PX, xb = j == 0 ? k0 : w;
            for (int x = xa; x < xb; x++) {
                if (MASKED && !mp[x]) continue;
                count(cellOf8(packPixel<CN>(rp + (size_t)x * CN), T, B));
            }
        }
        row += dr; j += dj;
        if (j >= nI) { j -= nI; row++; }
    }
    if (prev >= 0) atomicAdd(&mine[prev], run);
    __syncthreads();
    int32_t* H = hist + (size_t)blockIdx.y * cells;
    for (int i = threadIdx.x; i < cells; i += 256) {
        uint32_t s = 0;
        for (int c = 0; c < copies; c++) s += C[c * cstride + i];
        if (s) atomicAdd(&H[i], (int32_t)s);
    }
}

// the cell of the pixel at p (its first channel), negative: not counted
template <int DEPTH> __device__ __forceinline__ int cellOfPixel(const uchar* p, const int32_t* __restrict__ tabs, const Bins& B)
{
    int off = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        if (d >= B.dims) break;
        if (DEPTH == 0) off += tabs[d * 256 + p[B.ch[d]]];
        else if (DEPTH == 2) off += tabs[d * 65536 + reinterpret_cast<const uint16_t*>(p)[B.ch[d]]];
        else {
            calchist::Uniform u;
            u.a = B.a[d]; u.b = B.b[d];
            const int bin = calchist::binUniformF32(reinterpret_cast<const float*>(p)[B.ch[d]], B.n[d], u);
            off += bin < 0 ? SKIP : bin * B.mult[d];
        }
    }
    return off;
}

template <int DEPTH, bool MASKED>
__global__ __launch_bounds__(256) void k_calchist_generic(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h, const uchar* __restrict__ mask,
                                                          size_t mstep, size_t mframe, const int32_t* __restrict__ tabs, Bins B, int cells, int32_t* __restrict__ hist)
{
    constexpr int ESZ = DEPTH == 0 ? 1 : DEPTH == 2 ? 2 : 4;
    const uchar* S = src + (size_t)blockIdx.y * sframe;
    const uchar* M = MASKED ? mask + (size_t)blockIdx.y * mframe : nullptr;
    int32_t* H = hist + (size_t)blockIdx.y * cells;
    const uint32_t total = (uint32_t)h * (uint32_t)w, TT = gridDim.x * 256u, lane = threadIdx.x & 63u;
    for (uint32_t t0 = blockIdx.x * 256u + (threadIdx.x & ~63u); t0 < total; t0 += TT) {     // t0 is uniform in the wave: every lane makes every pass
        const uint32_t t = t0 + lane;
        int off = -1;
        if (t < total) {
            const uint32_t y = t / (uint32_t)w, x = t - y * (uint32_t)w;
            if (!MASKED || M[(size_t)y * mstep + x]) off = cellOfPixel<DEPTH>(S + (size_t)y * sstep + (size_t)x * B.cn * ESZ, tabs, B);
        }
        const bool act = off >= 0;
        const unsigned long long am = __ballot(act);
        if (!am) continue;
        const int leader = __ffsll((long long)am) - 1;
        const int first = __shfl(off, leader, 64);
        if (__all(!act || off == first)) {
            if ((int)lane == leader) atomicAdd(&H[first], (int32_t)__popcll(am));
        } else if (act) atomicAdd(&H[off], 1);
    }
}

template <int DEPTH> struct Out;
template <> struct Out<0> { typedef uint8_t T; static __device__ __forceinline__ uint32_t of(float hv, double s) { return calchist::backProjectInt(hv, s, 255u); } };
template <> struct Out<2> { typedef uint16_t T; static __device__ __forceinline__ uint32_t of(float hv, double s) { return calchist::backProjectInt(hv, s, 65535u); } };
template <> struct Out<5> { typedef uint32_t T; static __device__ __forceinline__ uint32_t of(float hv, double s) { return __float_as_uint(calchist::backProjectF32(hv, s)); } };

// mode 0: the histogram is gathered from memory; 1: its output values are in LDS; 2: (CV_8U, one dimension) one 256-entry table indexed by the pixel
template <int DEPTH>
__global__ __launch_bounds__(256) void k_backproject(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h, const int32_t* __restrict__ tabs, Bins B,
                                                     int cells, const float* __restrict__ hist, size_t hframe, double scale, int mode, uchar* __restrict__ dst,
                                                     size_t dstep, size_t dframe, uint32_t ng)
{
    typedef typename Out<DEPTH>::T OT;
    constexpr int ESZ = (int)sizeof(OT), G = 4 / ESZ;
    extern __shared__ int32_t lds[];
    int32_t* T = lds;                                                        // CV_8U: [3][256]
    uint32_t* O = reinterpret_cast<uint32_t*>(lds + (DEPTH == 0 ? 768 : 0)); // mode 1, 2: [cells] output values
    uint32_t* L = O + cells;                                                 // mode 2: [256]
    const float* Hf = hist + (size_t)blockIdx.y * hframe;
    if (DEPTH == 0) for (int i = threadIdx.x; i < 768; i += 256) T[i] = i < B.dims * 256 ? tabs[i] : 0;
    if (mode) for (int i = threadIdx.x; i < cells; i += 256) O[i] = Out<DEPTH>::of(Hf[i], scale);
    if (DEPTH == 0 || mode) __syncthreads();
    if (mode == 2) {
        const int o = T[threadIdx.x];
        L[threadIdx.x] = o < 0 ? 0u : O[o];
        __syncthreads();
    }
    const uchar* S = src + (size_t)blockIdx.y * sframe;
    uchar* D = dst + (size_t)blockIdx.y * dframe;
    const uint32_t TT = gridDim.x * 256u, items = (uint32_t)h * ng;
    for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < items; t += TT) {
        const uint32_t row = t / ng, g = t - row * ng;
        const uchar* rp = S + (size_t)row * sstep;
        uchar* dp = D + (size_t)row * dstep;
        const int shift = (int)((uintptr_t)dp & 3) / ESZ;                    // the group that holds the row's first pixel starts `shift` elements before it
        const int x0 = (int)g * G - shift;
        uint32_t v[G];
#pragma unroll
        for (int k = 0; k < G; k++) {
            const int x = x0 + k;
            v[k] = 0;
            if (x < 0 || x >= w) continue;
            const uchar* p = rp + (size_t)x * B.cn * ESZ;
            if (mode == 2) { v[k] = L[p[B.ch[0]]]; continue; }
            int off;
            if (DEPTH == 0) {
                off = T[p[B.ch[0]]];
                if (B.dims > 1) off += T[256 + p[B.ch[1]]];
                if (B.dims > 2) off += T[512 + p[B.ch[2]]];
            } else off = cellOfPixel<DEPTH>(p, tabs, B);
            if (off >= 0) v[k] = mode ? O[off] : Out<DEPTH>::of(Hf[off], scale);
        }
        if (x0 >= 0 && x0 + G <= w) {
            uint32_t word = v[0];
            if (G == 2) word |= v[1] << 16;
            if (G == 4) word |= (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            *reinterpret_cast<uint32_t*>(dp + (size_t)x0 * ESZ) = word;
        } else {
#pragma unroll
            for (int k = 0; k < G; k++) if (x0 + k >= 0 && x0 + k < w) reinterpret_cast<OT*>(dp)[x0 + k] = (OT)v[k];
        }
    }
}

// ---- host side
const char* depthName(int depth) { return depth == 0 ? "8u" : depth == 2 ? "16u" : "32f"; }
constexpr int LDS_SHARED_BLOCKS = 40 * 1024;     // up to here four workgroups share a CU's 160 KiB: private copies are added while they fit
constexpr int LDS_MAX_COPIES = 8;                // private copies of k_calchist_lds, chosen by lane (DESIGN 6.13 has the measurements behind the number)
constexpr int BP_LDS_CELLS = 8192;               // k_backproject keeps the output values of this many cells in LDS

// the most LDS a workgroup may ask for on the active device
int ldsLimit()
{
    static std::atomic<int> cached[64];          // several host threads drive several GPUs: each slot is written with the one value its device reports
    const int dev = activeDevice() & 63;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (!v) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, activeDevice()) != hipSuccess || v < 65536) { (void)hipGetLastError(); v = 65536; }
        cached[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

struct Binning {
    Bins B;
    int cells = 1, levels = 0;
    const std::vector<int32_t>* tabs = nullptr;  // CV_8U: [3][256] (unused dimensions zero), CV_16U: [dims][65536]; buildTables() sets it
};

// everything about (depth, cn, channels, dims, histSize, ranges, uniform) and the image geometry that is refused; fills bn but for the tables, which cost up to
// 3 x 65536 evaluations of the bin rule and are built (buildTables) only once nothing can decline the call any more.  No device is touched.
int checkArgs(const void* src, size_t sstep, size_t sframe, int w, int h, int depth, int cn, int nframes, const int* channels, int dims, const int* histSize,
              const float* ranges, int uniform, Binning& bn)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!src || !channels || !histSize || !ranges);
    if (depth != 0 && depth != 2 && depth != 5) return MI355_DECLINED("depth is not CV_8U, CV_16U or CV_32F");
    MI355_DECLINE_IF(cn < 1 || cn > 4);
    MI355_DECLINE_IF(dims < 1 || dims > calchist::MAX_DIMS);
    long long cells = 1;
    size_t nr = 0;
    for (int d = 0; d < dims; d++) {
        if (channels[d] < 0 || channels[d] >= cn) return MI355_DECLINED("a channel index is outside [0, cn)");
        if (histSize[d] < 1 || histSize[d] > calchist::MAX_BINS_PER_DIM) return MI355_DECLINED("a histSize is below 1 or above 65536");
        cells *= histSize[d];
        if (cells > lim::CALCHIST_MAX_BINS) return MI355_DECLINED("the product of histSize is above CALCHIST_MAX_BINS");
        nr += uniform ? 2 : (size_t)histSize[d] + 1;
    }
    if (!uniform && depth == 5) return MI355_DECLINED("non-uniform ranges on CV_32F");
    for (size_t i = 0; i < nr; i++) if (!std::isfinite(ranges[i])) return MI355_DECLINED("a range value is not finite");
    for (int d = 0, o = 0; d < dims; o += uniform ? 2 : histSize[d] + 1, d++)
        for (int i = 0; i < (uniform ? 1 : histSize[d]); i++)
            if (!(ranges[o + i] < ranges[o + i + 1])) return MI355_DECLINED(uniform ? "hi <= lo" : "the boundaries are not strictly ascending");
    MI355_DECLINE_IF(w <= 0 || h <= 0 || w > lim::CALCHIST_MAX_DIM || h > lim::CALCHIST_MAX_DIM);
    if (nframes < 1 || nframes > calchist::MAX_FRAMES) return MI355_DECLINED("nframes < 1 || nframes > 65535");
    const size_t esz = (size_t)depthBytes(depth);
    if (sstep < (size_t)w * cn * esz) return MI355_DECLINED("src_step is smaller than a row");
    if (sstep % esz || sframe % esz || (uintptr_t)src % esz) return MI355_DECLINED("src, src_step or src_frame_stride is no multiple of the element size");

    Bins& B = bn.B;
    memset(&B, 0, sizeof B);
    B.dims = dims; B.cn = cn;
    bn.cells = (int)cells;
    bn.levels = depth == 0 ? 256 : depth == 2 ? 65536 : 0;
    int mult = (int)cells;
    for (int d = 0, o = 0; d < dims; o += uniform ? 2 : histSize[d] + 1, d++) {
        mult /= histSize[d];
        B.ch[d] = channels[d]; B.sh[d] = 8 * channels[d]; B.n[d] = histSize[d]; B.mult[d] = mult;
        if (!bn.levels) { const calchist::Uniform u = calchist::uniformCoef(histSize[d], ranges[o], ranges[o + 1]); B.a[d] = u.a; B.b[d] = u.b; }
    }
    return MI355CV_OK;
}

// the CV_8U / CV_16U tables of a call that checkArgs has passed.  CV_16U evaluates the bin rule dims x 65536 times in double: the calling thread keeps its latest
// tables and rebuilds them only when (depth, histSize, ranges, uniform) change, as they do not from frame to frame.  (Their upload, 256 KiB a dimension, is per call.)
void buildTables(Binning& bn, int depth, int dims, const int* histSize, const float* ranges, int uniform)
{
    if (!bn.levels) return;
    thread_local std::vector<float> key;
    thread_local std::vector<int32_t> tabs;
    std::vector<float> k;
    k.push_back((float)depth); k.push_back((float)uniform);
    for (int d = 0, o = 0; d < dims; o += uniform ? 2 : histSize[d] + 1, d++) {
        k.push_back((float)histSize[d]);
        k.insert(k.end(), ranges + o, ranges + o + (uniform ? 2 : histSize[d] + 1));
    }
    if (k != key) {                              // (finite values only: checkArgs has refused the rest, so equal keys are equal bit for bit but for -0 == 0, which bin alike)
        key.clear();
        tabs.assign(depth == 0 ? 768 : (size_t)dims * 65536, 0);
        for (int d = 0, o = 0; d < dims; o += uniform ? 2 : histSize[d] + 1, d++)
            calchist::buildTable(bn.levels, histSize[d], uniform != 0, ranges + o, bn.B.mult[d], tabs.data() + (size_t)d * bn.levels);
        key.swap(k);
    }
    bn.tabs = &tabs;
}

// host-resident frames into dense device rows of pitch dstep
bool upload(const uchar* p, size_t step, size_t frame, size_t rowBytes, int h, int nf, uchar* dev, size_t dstep, hipStream_t st)
{
    for (int f = 0; f < nf; f++)
        if (hipMemcpy2DAsync(dev + (size_t)f * dstep * h, dstep, p + (size_t)f * frame, step, rowBytes, h, hipMemcpyHostToDevice, st) != hipSuccess) return false;
    noteStagedBytes((long long)rowBytes * h * nf);
    return true;
}

struct Count {
    const uchar* src; size_t sstep, sframe; int w, h;
    const uchar* mask; size_t mstep, mframe;
    const int32_t* tabs; int32_t* hist; int nf;
};

template <int CN> void launchLds(const Count& a, const Binning& bn, int copies, int cstride, int P, hipStream_t st)
{
    const uint32_t nI = (uint32_t)(a.w / Unit<CN>::PX + 2);
    const size_t lds = (size_t)(768 + copies * cstride) * 4;
    const dim3 grid(P, a.nf);
    if (a.mask) {
        if (lds > 65536) (void)hipFuncSetAttribute((const void*)k_calchist_lds<CN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_calchist_lds<CN, true>), grid, dim3(256), lds, st, a.src, a.sstep, a.sframe, a.w, a.h, a.mask, a.mstep, a.mframe, a.tabs, bn.B, bn.cells,
                           copies, cstride, nI, a.hist);
    } else {
        if (lds > 65536) (void)hipFuncSetAttribute((const void*)k_calchist_lds<CN, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_calchist_lds<CN, false>), grid, dim3(256), lds, st, a.src, a.sstep, a.sframe, a.w, a.h, (const uchar*)nullptr, (size_t)0, (size_t)0, a.tabs,
                           bn.B, bn.cells, copies, cstride, nI, a.hist);
    }
}

template <int D> void launchGeneric(const Count& a, const Binning& bn, int P, hipStream_t st)
{
    const dim3 grid(P, a.nf);
    if (a.mask) hipLaunchKernelGGL((k_calchist_generic<D, true>), grid, dim3(256), 0, st, a.src, a.sstep, a.sframe, a.w, a.h, a.mask, a.mstep, a.mframe, a.tabs, bn.B, bn.cells, a.hist);
    else hipLaunchKernelGGL((k_calchist_generic<D, false>), grid, dim3(256), 0, st, a.src, a.sstep, a.sframe, a.w, a.h, (const uchar*)nullptr, (size_t)0, (size_t)0, a.tabs, bn.B,
                            bn.cells, a.hist);
}

int runCalcHist(const char* entry, const uchar* src, size_t sstep, size_t sframe, int w, int h, int depth, int cn, int nframes, const int* channels, int dims,
                const int* histSize, const float* ranges, int uniform, const uchar* mask, size_t mstep, size_t mframe, void* hist, int hist_depth, int accumulate)
{
    Binning bn;
    if (const int rc = checkArgs(src, sstep, sframe, w, h, depth, cn, nframes, channels, dims, histSize, ranges, uniform, bn)) return rc;
    MI355_DECLINE_IF(!hist);
    if (hist_depth != 4 && hist_depth != 5) return MI355_DECLINED("hist_depth is neither CV_32S nor CV_32F");
    if (mask && mstep < (size_t)w) return MI355_DECLINED("mask_step is smaller than a row");
    if ((uintptr_t)hist % 4) return MI355_DECLINED("hist is not aligned to its 4-byte cells");
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    const int skind = ptrKind(src), mkind = mask ? ptrKind(mask) : skind, hkind = ptrKind(hist);
    if (skind == PTR_FOREIGN || mkind == PTR_FOREIGN || hkind == PTR_FOREIGN) return MI355_DECLINED("an argument lives on another device");
    if (skind != mkind) return MI355_DECLINED("src and mask must both live on this thread's device or both on the host");
    const bool shost = skind == PTR_HOST, rhost = hkind == PTR_HOST;
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_CHEAP)));
    const size_t esz = (size_t)depthBytes(depth), rowBytes = (size_t)w * cn * esz;
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + rowBytes, mspan = (size_t)(nframes - 1) * mframe + (size_t)(h - 1) * mstep + w;
    const size_t hbytes = (size_t)nframes * bn.cells * 4;
    if (overlapOnDevice(src, sspan, hist, hbytes) || (mask && overlapOnDevice(mask, mspan, hist, hbytes))) return MI355_DECLINED("the histogram overlaps the source or the mask in HBM");

    // the kernel: CV_8U whose tables, cells (at an odd stride) fit the workgroup's LDS -> k_calchist_lds, with as many private copies as keep four workgroups on a CU
    const int cstride = bn.cells | 1;
    bool useLds = depth == 0 && (size_t)(768 + cstride) * 4 <= (size_t)ldsLimit();
    int copies = 1;
    while (useLds && copies < LDS_MAX_COPIES && (size_t)(768 + 2 * copies * cstride) * 4 <= (size_t)LDS_SHARED_BLOCKS) copies *= 2;

    hipStream_t st = stream();
    int32_t* dH = rhost ? (int32_t*)stg.scratch(hbytes) : (int32_t*)hist;
    char* landing = rhost ? (char*)stg.pinned(hbytes) : nullptr;
    buildTables(bn, depth, dims, histSize, ranges, uniform);
    const int32_t* dtabs = bn.levels ? (const int32_t*)stg.param(bn.tabs->data(), bn.tabs->size() * 4) : nullptr;
    if (!dH || (rhost && !landing) || (bn.levels && !dtabs)) return MI355_DECLINED("no scratch");
    // host-resident frames: dense copies of a group of at most 1 GiB of them; a mask shared by all frames goes up once
    const bool sharedMask = mask && (nframes == 1 || mframe == 0);
    const size_t hstep = pad256(rowBytes), hmstep = pad256((size_t)w);
    const size_t perFrame = hstep * h + (mask && !sharedMask ? hmstep * h : 0);
    const int group = shost ? (int)std::min<size_t>((size_t)nframes, std::max<size_t>(1, (size_t(1) << 30) / perFrame)) : nframes;
    uchar* hsrc = shost ? (uchar*)stg.scratch(hstep * h * group) : nullptr;
    uchar* hmask = shost && mask ? (uchar*)stg.scratch(hmstep * h * (sharedMask ? 1 : group)) : nullptr;
    if (shost && (!hsrc || (mask && !hmask))) return MI355_DECLINED("no scratch");

    // the starting counts
    const size_t ncell = (size_t)nframes * bn.cells;
    const int cgrid = (int)std::min<size_t>((ncell + 255) / 256, 2048);
    if (!accumulate) {
        if (hipMemsetAsync(dH, 0, hbytes, st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed: %s", entry, hipGetErrorString(hipGetLastError()));
    } else {
        if (rhost) {
            memcpy(landing, hist, hbytes);
            if (hipMemcpyAsync(dH, landing, hbytes, hipMemcpyHostToDevice, st) != hipSuccess)
                return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
            noteStagedBytes((long long)hbytes);
        }
        if (hist_depth == 5) hipLaunchKernelGGL((k_calchist_convert<true>), dim3(cgrid), dim3(256), 0, st, dH, ncell);
    }
    if (shost && sharedMask && !upload(mask, mstep, 0, (size_t)w, h, 1, hmask, hmstep, st))
        return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));

    Count a;
    a.w = w; a.h = h; a.tabs = dtabs;
    int P = 1;
    for (int f0 = 0; f0 < nframes; f0 += group) {
        a.nf = std::min(group, nframes - f0);
        a.src = src + (size_t)f0 * sframe; a.sstep = sstep; a.sframe = sframe;
        a.mask = mask ? mask + (size_t)f0 * mframe : nullptr; a.mstep = mstep; a.mframe = sharedMask ? 0 : mframe;
        if (shost) {
            if (!upload(a.src, sstep, sframe, rowBytes, h, a.nf, hsrc, hstep, st) || (mask && !sharedMask && !upload(a.mask, mstep, mframe, (size_t)w, h, a.nf, hmask, hmstep, st)))
                return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
            a.src = hsrc; a.sstep = hstep; a.sframe = hstep * h;
            if (mask) { a.mask = hmask; a.mstep = hmstep; a.mframe = sharedMask ? 0 : hmstep * h; }
        }
        a.hist = dH + (size_t)f0 * bn.cells;
        if (useLds) {
            // a workgroup pays for clearing and merging its copies: fewer, longer workgroups for a large histogram
            const size_t items = (size_t)h * (w / (cn == 1 || cn == 3 ? 16 : cn == 2 ? 8 : 4) + 2);
            const size_t most = std::max<size_t>(1, (size_t)(bn.cells <= 2048 ? 2048 : 512) / a.nf);
            P = (int)std::max<size_t>(1, std::min((items + 1023) / 1024, most));
            switch (cn) {
            case 1: launchLds<1>(a, bn, copies, cstride, P, st); break;
            case 2: launchLds<2>(a, bn, copies, cstride, P, st); break;
            case 3: launchLds<3>(a, bn, copies, cstride, P, st); break;
            default: launchLds<4>(a, bn, copies, cstride, P, st); break;
            }
        } else {
            const size_t px = (size_t)w * h;
            P = (int)std::max<size_t>(1, std::min((px + 2047) / 2048, std::max<size_t>(1, (size_t)4096 / a.nf)));
            if (depth == 0) launchGeneric<0>(a, bn, P, st);
            else if (depth == 2) launchGeneric<2>(a, bn, P, st);
            else launchGeneric<5>(a, bn, P, st);
        }
    }
    if (hist_depth == 5) hipLaunchKernelGGL((k_calchist_convert<false>), dim3(cgrid), dim3(256), 0, st, dH, ncell);
    MI355_CHECK_LAUNCH(entry);
    if (rhost) {                                                             // the call's one read-back
        if (hipMemcpyAsync(landing, dH, hbytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
        memcpy(hist, landing, hbytes);
        noteStagedBytes((long long)hbytes);
    }
    if (useLds) noteKernel("k_calchist_lds<%dch,%s> grid=%dx%d x256 copies=%d by lane, runs combined cells=%d lds=%zu, %d frame(s)", cn, mask ? "mask" : "nomask", P,
                           std::min(group, nframes), copies, bn.cells, (size_t)(768 + copies * cstride) * 4, nframes);
    else noteKernel("k_calchist_generic<%s,%s> grid=%dx%d x256 cells=%d, %d frame(s)", depthName(depth), mask ? "mask" : "nomask", P, std::min(group, nframes), bn.cells, nframes);
    return stg.finish(entry);
}

struct Project {
    const uchar* src; size_t sstep, sframe; int w, h;
    const int32_t* tabs; const float* hist; size_t hframe; double scale; int mode;
    uchar* dst; size_t dstep, dframe; int nf, P; uint32_t ng; size_t lds;
};

template <int D> void launchProject(const Project& a, const Binning& bn, hipStream_t st)
{
    hipLaunchKernelGGL((k_backproject<D>), dim3(a.P, a.nf), dim3(256), a.lds, st, a.src, a.sstep, a.sframe, a.w, a.h, a.tabs, bn.B, bn.cells, a.hist, a.hframe, a.scale, a.mode,
                       a.dst, a.dstep, a.dframe, a.ng);
}

int runBackProject(const char* entry, const uchar* src, size_t sstep, size_t sframe, int w, int h, int depth, int cn, int nframes, const int* channels, int dims,
                   const int* histSize, const float* ranges, int uniform, const float* hist, size_t hframe, double scale, uchar* dst, size_t dstep, size_t dframe)
{
    Binning bn;
    if (const int rc = checkArgs(src, sstep, sframe, w, h, depth, cn, nframes, channels, dims, histSize, ranges, uniform, bn)) return rc;
    MI355_DECLINE_IF(!hist || !dst);
    const size_t esz = (size_t)depthBytes(depth), rowBytes = (size_t)w * cn * esz, drow = (size_t)w * esz;
    if (dstep < drow) return MI355_DECLINED("dst_step is smaller than a row");
    if (dstep % esz || dframe % esz || (uintptr_t)dst % esz) return MI355_DECLINED("dst, dst_step or dst_frame_stride is no multiple of the element size");
    if ((uintptr_t)hist % 4 || hframe % 4) return MI355_DECLINED("hist or hist_frame_stride is not aligned to its 4-byte cells");
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    const int skind = ptrKind(src), dkind = ptrKind(dst), hkind = ptrKind(hist);
    if (skind == PTR_FOREIGN || dkind == PTR_FOREIGN || hkind == PTR_FOREIGN) return MI355_DECLINED("an argument lives on another device");
    if (skind != dkind) return MI355_DECLINED("src and dst must both live on this thread's device or both on the host");
    const bool shost = skind == PTR_HOST;
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_CHEAP)));
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + rowBytes, dspan = (size_t)(nframes - 1) * dframe + (size_t)(h - 1) * dstep + drow;
    const size_t hspan = (size_t)(nframes - 1) * hframe + (size_t)bn.cells * 4;
    if (overlapOnDevice(src, sspan, dst, dspan) || overlapOnDevice(hist, hspan, dst, dspan)) return MI355_DECLINED("the destination overlaps the source or the histogram in HBM");

    hipStream_t st = stream();
    Project a;
    a.w = w; a.h = h; a.scale = scale;
    buildTables(bn, depth, dims, histSize, ranges, uniform);
    a.tabs = bn.levels ? (const int32_t*)stg.param(bn.tabs->data(), bn.tabs->size() * 4) : nullptr;
    if (bn.levels && !a.tabs) return MI355_DECLINED("no scratch");
    // the histogram(s): a host-resident one goes up densely
    const float* dhist = hist;
    size_t dhframe = hframe / 4;
    if (hkind == PTR_HOST) {
        const int nh = hframe ? nframes : 1;
        float* up = (float*)stg.scratch((size_t)nh * bn.cells * 4);
        if (!up) return MI355_DECLINED("no scratch");
        for (int f = 0; f < nh; f++)
            if (hipMemcpyAsync(up + (size_t)f * bn.cells, (const char*)hist + (size_t)f * hframe, (size_t)bn.cells * 4, hipMemcpyHostToDevice, st) != hipSuccess)
                return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
        noteStagedBytes((long long)nh * bn.cells * 4);
        dhist = up; dhframe = hframe ? (size_t)bn.cells : 0;
    }
    a.mode = bn.cells > BP_LDS_CELLS ? 0 : depth == 0 && dims == 1 ? 2 : 1;
    a.lds = ((depth == 0 ? 768 : 0) + (a.mode ? (size_t)bn.cells : 0) + (a.mode == 2 ? 256 : 0)) * 4;
    const int G = 4 / (int)esz;
    a.ng = (uint32_t)(w / G + 2);
    const size_t hdstep = pad256(drow), hstep = pad256(rowBytes);
    const int group = shost ? (int)std::min<size_t>((size_t)nframes, std::max<size_t>(1, (size_t(1) << 30) / ((hstep + hdstep) * h))) : nframes;
    uchar* hsrc = shost ? (uchar*)stg.scratch(hstep * h * group) : nullptr;
    uchar* hdst = shost ? (uchar*)stg.scratch(hdstep * h * group) : nullptr;
    if (shost && (!hsrc || !hdst)) return MI355_DECLINED("no scratch");
    for (int f0 = 0; f0 < nframes; f0 += group) {
        a.nf = std::min(group, nframes - f0);
        a.src = src + (size_t)f0 * sframe; a.sstep = sstep; a.sframe = sframe;
        a.dst = dst + (size_t)f0 * dframe; a.dstep = dstep; a.dframe = dframe;
        if (shost) {
            if (!upload(a.src, sstep, sframe, rowBytes, h, a.nf, hsrc, hstep, st)) return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
            a.src = hsrc; a.sstep = hstep; a.sframe = hstep * h;
            a.dst = hdst; a.dstep = hdstep; a.dframe = hdstep * h;
        }
        a.hist = dhist + (size_t)f0 * dhframe; a.hframe = dhframe;
        const size_t items = (size_t)h * a.ng;
        a.P = (int)std::max<size_t>(1, std::min((items + 1023) / 1024, std::max<size_t>(1, (size_t)4096 / a.nf)));
        if (depth == 0) launchProject<0>(a, bn, st);
        else if (depth == 2) launchProject<2>(a, bn, st);
        else launchProject<5>(a, bn, st);
        if (shost) {
            for (int f = 0; f < a.nf; f++)
                if (hipMemcpy2DAsync(dst + (size_t)(f0 + f) * dframe, dstep, hdst + (size_t)f * hdstep * h, hdstep, drow, h, hipMemcpyDeviceToHost, st) != hipSuccess)
                    return setError(MI355CV_ERROR_UNKNOWN, "%s: D2H failed: %s", entry, hipGetErrorString(hipGetLastError()));
            noteStagedBytes((long long)drow * h * a.nf);
        }
    }
    MI355_CHECK_LAUNCH(entry);
    if (shost && hipStreamSynchronize(st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
    noteKernel("k_backproject<%s> grid=%dx%d x256 mode=%s cells=%d lds=%zu, %d frame(s)", depthName(depth), a.P, std::min(group, nframes),
               a.mode == 2 ? "lut256" : a.mode ? "lds" : "gather", bn.cells, a.lds, nframes);
    return stg.finish(entry);
}

} // namespace

static_assert(lim::CALCHIST_MAX_DIM == calchist::MAX_DIM && lim::CALCHIST_MAX_BINS == calchist::MAX_BINS, "one bound");
static_assert((long long)calchist::MAX_DIM * calchist::MAX_DIM <= (1ll << 28), "a frame's pixels, and so any count of one call, stay below 2^28");
static_assert((long long)calchist::MAX_DIM * (calchist::MAX_DIM / 4 + 2) + 2048 * 256 < (1ll << 32), "the kernels count items in 32 bits");
static_assert(3ll * calchist::SKIP > INT32_MIN && calchist::SKIP + 2ll * calchist::MAX_BINS < 0, "a sum of table entries with one SKIP stays negative");

extern "C" {

MI355CV_API int mi355cv_calcHist(const uchar* src_data, size_t src_step, int width, int height, int depth, int cn, const int* channels, int dims, const int* histSize,
                                 const float* ranges, int uniform, const uchar* mask_data, size_t mask_step, void* hist, int hist_depth, int accumulate)
{
    mi355::EntryGuard entry_(__func__);
    return runCalcHist("calcHist", src_data, src_step, 0, width, height, depth, cn, 1, channels, dims, histSize, ranges, uniform, mask_data, mask_step, 0, hist, hist_depth,
                       accumulate);
}

MI355CV_API int mi355cv_calcHistBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, int depth, int cn, int nframes,
                                      const int* channels, int dims, const int* histSize, const float* ranges, int uniform, const uchar* mask_data, size_t mask_step,
                                      size_t mask_frame_stride, void* hist, int hist_depth, int accumulate)
{
    mi355::EntryGuard entry_(__func__);
    return runCalcHist("calcHistBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, width, height, depth, cn, nframes, channels, dims, histSize, ranges, uniform,
                       mask_data, mask_step, nframes == 1 ? 0 : mask_frame_stride, hist, hist_depth, accumulate);
}

MI355CV_API int mi355cv_calcBackProject(const uchar* src_data, size_t src_step, int width, int height, int depth, int cn, const int* channels, int dims,
                                        const int* histSize, const float* ranges, int uniform, const float* hist, double scale, uchar* dst_data, size_t dst_step)
{
    mi355::EntryGuard entry_(__func__);
    return runBackProject("calcBackProject", src_data, src_step, 0, width, height, depth, cn, 1, channels, dims, histSize, ranges, uniform, hist, 0, scale, dst_data, dst_step,
                          0);
}

MI355CV_API int mi355cv_calcBackProjectBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, int depth, int cn, int nframes,
                                             const int* channels, int dims, const int* histSize, const float* ranges, int uniform, const float* hist,
                                             size_t hist_frame_stride, double scale, uchar* dst_data, size_t dst_step, size_t dst_frame_stride)
{
    mi355::EntryGuard entry_(__func__);
    return runBackProject("calcBackProjectBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, width, height, depth, cn, nframes, channels, dims, histSize, ranges,
                          uniform, hist, nframes == 1 ? 0 : hist_frame_stride, scale, dst_data, dst_step, nframes == 1 ? 0 : dst_frame_stride);
}

} // extern "C"
