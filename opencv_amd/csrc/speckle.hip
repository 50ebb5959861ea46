// speckle.hip -- cv::filterSpeckles (calib3d, stereosgbm.cpp; the reference has no HAL hook for it) on one channel of CV_8U or CV_16S, in place, single maps and
// batches.  The definition is the project's own restatement (tests/speckle_restate.py): the connected components of the graph whose nodes are the pixels
// != newVal and whose edges join 4-neighbours with |a - b| <= maxDiff; every pixel of a component of at most maxSpeckleSize pixels becomes newVal.  The pieces that
// can be wrong are in speckle_math.h, compiled for the host by tests/hostemu/speckle_emu.cpp.  A union-find over pixels in scratch (unionfind.h) whose root is the
// smallest linear pixel index (parents only decrease), a 32-bit size at the root.
//
//   plain path   k_spk_init    a parent per pixel, its own index or DEAD; the size counters zeroed (scratch is reused between calls)
//                k_spk_link    a thread per pixel: the links to the left and the upper neighbour, united in HBM with atomicMin.  A find may read a parent another
//                              workgroup of the same kernel has just written: every such load is an agent-scope atomic load and the union loop retries until its
//                              atomicMin returns the value it expected (the discipline of k_ccl_vseam / k_ccl_hseam)
//                k_spk_count   every live pixel finds its root, stores it and adds 1 to the root's size
//   fast path    k_spk_tile    a wave per tile of 256 columns x 16 rows.  A lane loads 4 pixels (one 4- or 8-byte load where the address allows, element by element
//                              otherwise); twelve ballots per row become three bit planes: live, link-left, link-up.  Runs are bit scans of the link-left words,
//                              the runs of the tile are merged through the link-up bits in LDS, and every pixel's parent -- the first pixel of its component INSIDE
//                              the tile -- goes to HBM with a zeroed counter
//                k_spk_vseam / k_spk_hseam   the pairs across the tile seams, united in HBM as k_spk_link does
//                k_spk_count_runs   a wave per (row, 256 columns): roots found and stored, one atomicAdd of the run length per run of equal root
//   both         k_spk_erase   only now is the image written: a live pixel whose root's size <= maxSpeckleSize becomes newVal.  A kernel boundary separates the
//                              last count from the first erase, so every size is final.
// The image depends on component sizes only, never on label values or on the order the unions and adds land in: the atomics cannot make it differ from run to run.
// A batch is one sequence of launches: the frame is the grid's z.
#include "rt.h"
#include "speckle_math.h"
#include <atomic>
#include <vector>

namespace {
using namespace mi355;
using spk::DEAD;
using spk::STRIP_H;
using spk::TILE_W;
using spk::WORDS;
using uf::GlobalMem;
using uf::LdsMem;

static_assert(spk::MAX_DIM == lim::SPECKLE_MAX_DIM && TILE_W == lim::SPECKLE_TILE_COLS && STRIP_H == lim::SPECKLE_TILE_ROWS, "mi355cv_limit(\"speckle_*\")");
static_assert((long long)spk::MAX_DIM * spk::MAX_DIM <= (1ll << 28), "a pixel index and a size in 32 bits, below DEAD");

// one frame of a call: where it is read and where it is written -- the same rows for a device-resident map, two staged buffers for a host-resident one
struct Frame { const uchar* src; size_t sstep; uchar* dst; size_t dstep; };
// the scratch of a call: parents and sizes, `frame` elements apart per frame
struct Scr { uint32_t* P; uint32_t* C; size_t frame; };
struct Rule { int newVal, maxDiff, maxSize; };

template <typename T> __device__ __forceinline__ const T* rowOf(const Frame& F, int y) { return reinterpret_cast<const T*>(F.src + (size_t)y * F.sstep); }

// ------------------------------------------------------------------------------------------------------------------------------------ plain path
template <typename T>
__global__ __launch_bounds__(256) void k_spk_init(const Frame* __restrict__ frames, int w, int h, Rule R, Scr s)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const Frame F = frames[blockIdx.z];
    const uint32_t g = (uint32_t)y * w + x;
    const size_t at = (size_t)blockIdx.z * s.frame + g;
    s.P[at] = spk::live(rowOf<T>(F, y)[x], R.newVal) ? g : DEAD;
    s.C[at] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void k_spk_link(const Frame* __restrict__ frames, int w, int h, Rule R, Scr s)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const Frame F = frames[blockIdx.z];
    const T* row = rowOf<T>(F, y);
    const int v = row[x];
    if (!spk::live(v, R.newVal)) return;
    GlobalMem m{s.P + (size_t)blockIdx.z * s.frame};
    const uint32_t g = (uint32_t)y * w + x;
    if (x > 0) { const int a = row[x - 1]; if (spk::live(a, R.newVal) && spk::linked(v, a, R.maxDiff)) spk::unite(m, g, g - 1); }
    if (y > 0) { const int a = rowOf<T>(F, y - 1)[x]; if (spk::live(a, R.newVal) && spk::linked(v, a, R.maxDiff)) spk::unite(m, g, g - w); }
}

__global__ __launch_bounds__(256) void k_spk_count(int w, int h, Scr s)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    GlobalMem m{s.P + (size_t)blockIdx.z * s.frame};
    const uint32_t g = (uint32_t)y * w + x;
    const uint32_t p = m.load(g);
    if (p == DEAD) return;
    const uint32_t r = spk::find(m, p);
    if (r != p) __hip_atomic_store(m.P + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(s.C + (size_t)blockIdx.z * s.frame + r, 1u);
}

// ------------------------------------------------------------------------------------------------------------------------------------ fast path
// pixels x .. x + 3 of a row w wide; ok: bit k = pixel x + k exists
template <typename T> __device__ __forceinline__ int load4(const T* row, int x, int w, int* v);
template <> __device__ __forceinline__ int load4<uchar>(const uchar* row, int x, int w, int* v)
{
    if (x + 4 <= w && ((uintptr_t)(row + x) & 3) == 0) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(row + x);
        v[0] = q & 0xff; v[1] = (q >> 8) & 0xff; v[2] = (q >> 16) & 0xff; v[3] = q >> 24;
        return 15;
    }
    int ok = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = 0; if (x + k < w) { v[k] = row[x + k]; ok |= 1 << k; } }
    return ok;
}
template <> __device__ __forceinline__ int load4<short>(const short* row, int x, int w, int* v)
{
    if (x + 4 <= w && ((uintptr_t)(row + x) & 7) == 0) {
        const uint2 q = *reinterpret_cast<const uint2*>(row + x);
        v[0] = (short)(q.x & 0xffff); v[1] = (short)(q.x >> 16); v[2] = (short)(q.y & 0xffff); v[3] = (short)(q.y >> 16);
        return 15;
    }
    int ok = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = 0; if (x + k < w) { v[k] = row[x + k]; ok |= 1 << k; } }
    return ok;
}

enum { LV = 0, LL = 1, LU = 2 };                  // the bit planes of a tile row: live, link-left, link-up

template <typename T>
__global__ __launch_bounds__(64) void k_spk_tile(const Frame* __restrict__ frames, int w, int h, Rule R, Scr s)
{
    __shared__ uint32_t par[STRIP_H * TILE_W];
    __shared__ uint64_t wd[3][STRIP_H][WORDS];
    __shared__ uint64_t st[STRIP_H][WORDS];       // the run starts: live & ~link-left
    const int lane = threadIdx.x, x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * STRIP_H, rows = min(STRIP_H, h - y0);
    const Frame F = frames[blockIdx.z];
    int up[4] = {0, 0, 0, 0}, upLive = 0;
    for (int r = 0; r < rows; r++) {
        int v[4];
        const int ok = load4<T>(rowOf<T>(F, y0 + r), x0 + 4 * lane, w, v);
        int lv = 0, ll = 0, lu = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) if (((ok >> k) & 1) && spk::live(v[k], R.newVal)) lv |= 1 << k;
        const int leftV = __shfl_up(v[3], 1, 64), leftLive = __shfl_up(lv >> 3, 1, 64);
        if (lane > 0 && (lv & 1) && leftLive && spk::linked(v[0], leftV, R.maxDiff)) ll |= 1;
#pragma unroll
        for (int k = 1; k < 4; k++) if (((lv >> k) & 1) && ((lv >> (k - 1)) & 1) && spk::linked(v[k], v[k - 1], R.maxDiff)) ll |= 1 << k;
        if (r > 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) if (((lv >> k) & 1) && ((upLive >> k) & 1) && spk::linked(v[k], up[k], R.maxDiff)) lu |= 1 << k;
        }
        const int plane[3] = {lv, ll, lu};
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const uint64_t b0 = __ballot(plane[q] & 1), b1 = __ballot(plane[q] & 2), b2 = __ballot(plane[q] & 4), b3 = __ballot(plane[q] & 8);
            if (lane < WORDS) wd[q][r][lane] = ccl::rowWord(b0, b1, b2, b3, lane);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) up[k] = v[k];
        upLive = lv;
    }
    __syncthreads();
    for (int i = lane; i < rows * WORDS; i += 64) { const int r = i / WORDS, j = i % WORDS; st[r][j] = wd[LV][r][j] & ~wd[LL][r][j]; }
    __syncthreads();
    for (int r = 0; r < rows; r++)                                            // a node per run: its first pixel
        for (int j = 0; j < WORDS; j++)
            if ((st[r][j] >> lane) & 1) { const int c = r * TILE_W + 64 * j + lane; par[c] = c; }
    __syncthreads();
    LdsMem m{par};
    for (int r = 1; r < rows; r++)                                            // the pairs (run, run of the row above) that are linked
        for (int j = 0; j < WORDS; j++) {
            const uint64_t d = spk::upDirect(wd[LU][r][j], wd[LL][r][j], wd[LL][r - 1][j], j ? wd[LU][r][j - 1] >> 63 : 0);
            if ((d >> lane) & 1) spk::unite(m, (uint32_t)(r * TILE_W + spk::runStartOf(st[r], j, lane)), (uint32_t)((r - 1) * TILE_W + spk::runStartOf(st[r - 1], j, lane)));
        }
    __syncthreads();
    uint32_t* P = s.P + (size_t)blockIdx.z * s.frame;
    uint32_t* C = s.C + (size_t)blockIdx.z * s.frame;
    for (int r = 0; r < rows; r++)
        for (int j = 0; j < WORDS; j++) {
            const int x = x0 + 64 * j + lane;
            if (x >= w) continue;
            uint32_t p = DEAD;
            if ((wd[LV][r][j] >> lane) & 1) {
                const uint32_t root = spk::find(m, (uint32_t)(r * TILE_W + spk::runStartOf(st[r], j, lane)));
                p = (uint32_t)(y0 + (int)(root / TILE_W)) * (uint32_t)w + (uint32_t)(x0 + (int)(root % TILE_W));
            }
            const size_t g = (size_t)(y0 + r) * w + x;
            P[g] = p;
            C[g] = 0;
        }
}

// pixel (y, x - 1) against (y, x), x a multiple of TILE_W
template <typename T>
__global__ __launch_bounds__(64) void k_spk_vseam(const Frame* __restrict__ frames, int w, int h, Rule R, Scr s)
{
    const int y = blockIdx.x * 64 + threadIdx.x, x = (blockIdx.y + 1) * TILE_W;
    if (y >= h || x >= w) return;
    const T* row = rowOf<T>(frames[blockIdx.z], y);
    const int a = row[x - 1], b = row[x];
    if (!spk::live(a, R.newVal) || !spk::live(b, R.newVal) || !spk::linked(a, b, R.maxDiff)) return;
    GlobalMem m{s.P + (size_t)blockIdx.z * s.frame};
    const uint32_t g = (uint32_t)y * w + x;
    spk::unite(m, g, g - 1);
}

// pixel (y, x) against (y - 1, x), y a multiple of STRIP_H
template <typename T>
__global__ __launch_bounds__(256) void k_spk_hseam(const Frame* __restrict__ frames, int w, int h, Rule R, Scr s)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = (blockIdx.y + 1) * STRIP_H;
    if (x >= w || y >= h) return;
    const Frame F = frames[blockIdx.z];
    const int a = rowOf<T>(F, y - 1)[x], b = rowOf<T>(F, y)[x];
    if (!spk::live(a, R.newVal) || !spk::live(b, R.newVal) || !spk::linked(a, b, R.maxDiff)) return;
    GlobalMem m{s.P + (size_t)blockIdx.z * s.frame};
    const uint32_t g = (uint32_t)y * w + x;
    spk::unite(m, g, g - w);
}

// a wave per (row, tile)
__global__ __launch_bounds__(256) void k_spk_count_runs(int w, int h, Scr s)
{
    const int lane = threadIdx.x & 63, x0 = blockIdx.x * TILE_W, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    GlobalMem m{s.P + (size_t)blockIdx.z * s.frame};
    uint32_t* C = s.C + (size_t)blockIdx.z * s.frame;
#pragma unroll
    for (int j = 0; j < WORDS; j++) {
        const int x = x0 + 64 * j + lane;
        const uint32_t g = (uint32_t)y * w + x;
        const uint32_t p = x < w ? m.load(g) : DEAD;
        const bool lv = p != DEAD;
        uint32_t r = DEAD;
        if (lv) {
            r = spk::find(m, p);
            if (r != p) __hip_atomic_store(m.P + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const uint32_t left = __shfl_up(r, 1, 64);
        const bool cont = lv && lane > 0 && r == left;
        const uint64_t contBits = __ballot(cont);
        if (lv && !cont) atomicAdd(C + r, spk::runLen(contBits, lane));
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ erase
template <typename T>
__global__ __launch_bounds__(256) void k_spk_erase(const Frame* __restrict__ frames, int w, int h, Rule R, Scr s)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const Frame F = frames[blockIdx.z];
    const size_t f = (size_t)blockIdx.z * s.frame;
    const uint32_t p = s.P[f + (size_t)y * w + x];
    T* out = reinterpret_cast<T*>(F.dst + (size_t)y * F.dstep) + x;
    if (spk::erased(p != DEAD, p != DEAD ? s.C[f + p] : 0u, R.maxSize)) *out = (T)R.newVal;
    else if ((const uchar*)F.src != (const uchar*)F.dst) *out = rowOf<T>(F, y)[x];        // a staged map: the kept pixels travel too
}

// ------------------------------------------------------------------------------------------------------------------------------------ host side
std::atomic<int> g_kernelMode{-1};       // mi355cv_filterSpecklesSetKernel: -1 the rule below (the tile kernel for every shape), 0 always the plain kernels

template <typename T>
void launchAll(const Frame* dFrames, int W, int H, int nframes, Rule R, Scr s, bool fast, hipStream_t st)
{
    const dim3 pix(divUp(W, 256), H, nframes);
    if (fast) {
        const int ntx = divUp(W, TILE_W), nstrips = divUp(H, STRIP_H);
        hipLaunchKernelGGL(k_spk_tile<T>, dim3(ntx, nstrips, nframes), dim3(64), 0, st, dFrames, W, H, R, s);
        if (ntx > 1) hipLaunchKernelGGL(k_spk_vseam<T>, dim3(divUp(H, 64), ntx - 1, nframes), dim3(64), 0, st, dFrames, W, H, R, s);
        if (nstrips > 1) hipLaunchKernelGGL(k_spk_hseam<T>, dim3(divUp(W, 256), nstrips - 1, nframes), dim3(256), 0, st, dFrames, W, H, R, s);
        hipLaunchKernelGGL(k_spk_count_runs, dim3(ntx, divUp(H, 4), nframes), dim3(256), 0, st, W, H, s);
        noteKernel("k_spk_tile<%s> grid=%dx%dx%d x64 lds=%zu, k_spk_vseam + k_spk_hseam + k_spk_count_runs + k_spk_erase", sizeof(T) == 1 ? "8U" : "16S", ntx, nstrips, nframes,
                   sizeof(uint32_t) * STRIP_H * TILE_W + sizeof(uint64_t) * 4 * STRIP_H * WORDS);
    } else {
        hipLaunchKernelGGL(k_spk_init<T>, pix, dim3(256), 0, st, dFrames, W, H, R, s);
        hipLaunchKernelGGL(k_spk_link<T>, pix, dim3(256), 0, st, dFrames, W, H, R, s);
        hipLaunchKernelGGL(k_spk_count, pix, dim3(256), 0, st, W, H, s);
        noteKernel("k_spk_init<%s> grid=%ux%ux%u x256, k_spk_link + k_spk_count + k_spk_erase", sizeof(T) == 1 ? "8U" : "16S", pix.x, pix.y, pix.z);
    }
    hipLaunchKernelGGL(k_spk_erase<T>, pix, dim3(256), 0, st, dFrames, W, H, R, s);
}

int runSpeckles(const char* entry, uchar* img, size_t step, size_t frameStride, int nframes, int W, int H, int depth, int newVal, int maxSpeckleSize, int maxDiff)
{
    MI355_DECLINE_IF(disabled());
    if (depth != MI355CV_8U && depth != MI355CV_16S) return MI355_DECLINED("the image is neither CV_8UC1 nor CV_16SC1");
    MI355_DECLINE_IF(!img);
    MI355_DECLINE_IF(nframes < 1 || nframes > 65535);
    MI355_DECLINE_IF(W < 1 || H < 1 || W > lim::SPECKLE_MAX_DIM || H > lim::SPECKLE_MAX_DIM);
    const bool is16 = depth == MI355CV_16S;
    const size_t esz = is16 ? 2 : 1, rowBytes = (size_t)W * esz;
    MI355_DECLINE_IF(step < rowBytes);
    if (is16 && (((size_t)img | step | (nframes > 1 ? frameStride : 0)) & 1)) return MI355_DECLINED("CV_16S rows off their element's boundary");
    if (!spk::fitsDepth(newVal, is16)) return MI355_DECLINED("newVal outside the range of the image's depth");
    if (nframes > 1 && frameStride < span(step, H, rowBytes)) return MI355_DECLINED("two frames of the batch overlap (the frame stride is below the frame)");
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(img, (size_t)W * H, minPixels(HOST_HEAVY)));
    Scr s{};
    s.frame = ((size_t)W * H + 63) & ~(size_t)63;
    s.P = (uint32_t*)stg.scratch(s.frame * nframes * sizeof(uint32_t));
    s.C = (uint32_t*)stg.scratch(s.frame * nframes * sizeof(uint32_t));
    if (!s.P || !s.C) return MI355_DECLINED("no scratch for the parents and the sizes");
    std::vector<Frame> fr(nframes);
    for (int f = 0; f < nframes; f++) {
        uchar* p = img + (size_t)f * frameStride;
        Frame& F = fr[f];
        F.src = stg.in(p, step, rowBytes, H, &F.sstep);
        F.dst = stg.out(p, step, rowBytes, H, &F.dstep);
        if (!F.src || !F.dst) return MI355_DECLINED("staging failed");
    }
    const Frame* dFrames = (const Frame*)stg.param(fr.data(), fr.size() * sizeof(Frame));
    if (!dFrames) return MI355_DECLINED("no scratch");
    const Rule R{newVal, maxDiff, maxSpeckleSize};
    const bool fast = g_kernelMode.load(std::memory_order_relaxed) != 0;
    if (is16) launchAll<short>(dFrames, W, H, nframes, R, s, fast, stream());
    else launchAll<uchar>(dFrames, W, H, nframes, R, s, fast, stream());
    MI355_CHECK_LAUNCH(entry);
    return stg.finish(entry);
}

} // namespace

extern "C" {

// Host-resident maps are staged (HOST_HEAVY): the reference's flood fill is single-threaded.
MI355CV_API int mi355cv_filterSpeckles(uchar* img, size_t step, int width, int height, int depth, int newVal, int maxSpeckleSize, int maxDiff)
{
    mi355::EntryGuard entry_(__func__);
    return runSpeckles("filterSpeckles", img, step, 0, 1, width, height, depth, newVal, maxSpeckleSize, maxDiff);
}

MI355CV_API int mi355cv_filterSpecklesBatch(uchar* img, size_t step, size_t frame_stride, int nframes, int width, int height, int depth, int newVal, int maxSpeckleSize,
                                            int maxDiff)
{
    mi355::EntryGuard entry_(__func__);
    return runSpeckles("filterSpecklesBatch", img, step, frame_stride, nframes, width, height, depth, newVal, maxSpeckleSize, maxDiff);
}

MI355CV_API int mi355cv_filterSpecklesSetKernel(int mode)
{
    if (mode < -1 || mode > 0) return MI355CV_ERROR_UNKNOWN;
    g_kernelMode.store(mode, std::memory_order_relaxed);
    return MI355CV_OK;
}

} // extern "C"
