// undistort.hip -- the two ends of the stereo pipeline of calib3d: cv::initUndistortRectifyMap, cv::undistort and the rectifying warp in front of the matchers,
// cv::reprojectImageTo3D behind them (the reference has no HAL hook for any of them).  The definition is the project's restatement (tests/undistort_restate.py,
// DESIGN 6.21); every line of arithmetic is in undistort_math.h, which the CPU suite compiles for the host.
//
//   k_undist_map        a lane per destination pixel: the map rule, written as a CV_32FC1 pair, CV_32FC2 or CV_16SC2 + CV_16UC1
//   k_undist8_tile<CN>  CV_8U with 1, 3 or 4 channels, INTER_LINEAR: a workgroup owns a 128 x 32 (16 for 3 / 4 channels) destination tile.  Every lane evaluates the
//                       rule for its pixels once and keeps the fixed-point coordinates in registers; the workgroup reduces their extremes (waves by shuffles, then
//                       LDS) to the EXACT source box -- a distortion map need not be monotone, so no corner argument --, stages the box with warp8::stage's aligned
//                       dwords, samples with (Q + 512) >> 10 and stores four pixels as one dword.  In a batch the same workgroup then walks `fpw` frames with the
//                       coordinates it already holds: stage, sample, store per frame, no map traffic at all.  The rim, the border rules other than CONSTANT and
//                       boxes beyond the LDS allotment take und::sampleGeneric8, the arithmetic of k_warp's fixed-point bilinear branch.
//   k_reproject3d       four pixels per lane, one 48-byte run of stores per lane; the frame's minimum (handleMissingValues) is read from HBM where
//                       mi355cv_minMaxLocBatch left it: no host synchronisation
// The result of mi355cv_undistortRectify is BY DEFINITION mi355cv_remap with the CV_16SC2 + CV_16UC1 maps of the rule; the composed arm is that sentence as code
// (the maps into scratch, then the existing remap kernels) and serves every class the tile kernel does not.
#include "rt.h"
#include "undistort_math.h"
#include <atomic>
#include <algorithm>
#include <math.h>
#include <string.h>

using namespace mi355;

namespace {

constexpr int T32FC1 = MI355CV_MAKETYPE(MI355CV_32F, 1), T32FC2 = MI355CV_MAKETYPE(MI355CV_32F, 2), T16SC2 = MI355CV_MAKETYPE(MI355CV_16S, 2), T16UC1 = MI355CV_MAKETYPE(MI355CV_16U, 1);
static_assert(lim::UNDIST_TILE_COLS == warp8::TW && lim::UNDIST_TILE_ROWS == warp8::tileRows<1>(), "the limits report the tile of warp8.h");

__global__ __launch_bounds__(256) void k_undist_map(und::Rule q, int w, int h, int m1type, uchar* __restrict__ m1, size_t s1, uchar* __restrict__ m2, size_t s2)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    if (m1type == T16SC2) {
        int iu, iv;
        und::fixedUV(q, x, y, iu, iv);
        reinterpret_cast<uint32_t*>(m1 + (size_t)y * s1)[x] = und::entryOf(iu, iv);
        reinterpret_cast<unsigned short*>(m2 + (size_t)y * s2)[x] = (unsigned short)und::fracOf(iu, iv);
        return;
    }
    double u, v;
    und::mapUV(q, x, y, u, v);
    if (m1type == T32FC2) reinterpret_cast<float2*>(m1 + (size_t)y * s1)[x] = make_float2((float)u, (float)v);
    else { reinterpret_cast<float*>(m1 + (size_t)y * s1)[x] = (float)u; reinterpret_cast<float*>(m2 + (size_t)y * s2)[x] = (float)v; }
}

__device__ __forceinline__ int waveMin(int v) { for (int m = 32; m; m >>= 1) v = min(v, __shfl_xor(v, m, 64)); return v; }
__device__ __forceinline__ int waveMax(int v) { for (int m = 32; m; m >>= 1) v = max(v, __shfl_xor(v, m, 64)); return v; }

template <int CN>
__global__ __launch_bounds__(256) void k_undist8_tile(const uchar* __restrict__ src, uchar* __restrict__ dst, const und::TileArgs* __restrict__ args)
{
    const und::TileArgs& a = *args;                   // in HBM, not in the kernel's arguments: 25 doubles of rule held in SGPRs from the entry on spilled a dozen of them
    extern __shared__ __align__(16) uchar lds[];
    constexpr int NS = und::steps<CN>();
    const int tid = threadIdx.x, x0 = blockIdx.x * warp8::TW, y0 = blockIdx.y * warp8::tileRows<CN>();
    uint32_t pk[NS][4], fr[NS][4];
    int mm[4];
    und::coords<CN>(a, x0, y0, tid, pk, fr, mm);
    int* ext = reinterpret_cast<int*>(lds);
    mm[0] = waveMin(mm[0]); mm[1] = waveMax(mm[1]); mm[2] = waveMin(mm[2]); mm[3] = waveMax(mm[3]);
    if ((tid & 63) == 0) { ext[4 * (tid >> 6)] = mm[0]; ext[4 * (tid >> 6) + 1] = mm[1]; ext[4 * (tid >> 6) + 2] = mm[2]; ext[4 * (tid >> 6) + 3] = mm[3]; }
    __syncthreads();
    // wave-uniform: the box arithmetic runs on the scalar unit
    const int mnx = __builtin_amdgcn_readfirstlane(min(min(ext[0], ext[4]), min(ext[8], ext[12]))), mxx = __builtin_amdgcn_readfirstlane(max(max(ext[1], ext[5]), max(ext[9], ext[13])));
    const int mny = __builtin_amdgcn_readfirstlane(min(min(ext[2], ext[6]), min(ext[10], ext[14]))), mxy = __builtin_amdgcn_readfirstlane(max(max(ext[3], ext[7]), max(ext[11], ext[15])));
    int pitch;
    const warp8::Box b = und::boxOf<CN>(a, mnx, mxx, mny, mxy, pitch);
    const warp8::Args sa = und::stageArgs(a, pitch);
    uchar* tile = lds + und::TILE_OFF;
    const int f0 = blockIdx.z * a.fpw, f1 = min(a.nframes, f0 + a.fpw);
    for (int f = f0; f < f1; f++) {                                                       // uniform
        const uchar* S = src + (size_t)f * a.sframe;
        uchar* D = dst + (size_t)f * a.dframe;
        if (b.cw) {
            if (f > f0) __syncthreads();                                                  // the previous frame's pixels are no longer read
            warp8::stage(sa, b, CN, S, tile, tid);
            __syncthreads();
        }
        // the coordinates are the same for every frame, and a compiler that sees it keeps every pixel's offsets, weights and border indices of both samplers alive
        // across the loop (506 VGPRs on one channel, spilled SGPRs); behind an empty asm they are re-derived per frame, a handful of integer operations a pixel
#pragma unroll
        for (int i = 0; i < NS; i++)
#pragma unroll
            for (int p = 0; p < 4; p++) asm volatile("" : "+v"(pk[i][p]), "+v"(fr[i][p]));
        const unsigned mask = und::sampleTile<CN>(a, b, pitch, x0, y0, tile, D, tid, pk, fr);
        if (mask) und::redo<CN>(a, mask, x0, y0, S, D, tid, pk, fr);
    }
}

struct Q16 { double q[16]; };

__global__ __launch_bounds__(256) void k_reproject3d(const uchar* __restrict__ src, size_t sstep, size_t sframe, int depth, uchar* __restrict__ dst, size_t dstep, size_t dframe,
                                                     int w, int h, Q16 Q, const double* __restrict__ vals /* {min, max} per frame, or null */, int vec)
{
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uchar* row = src + (size_t)blockIdx.z * sframe + (size_t)y * sstep;
    float* out = reinterpret_cast<float*>(dst + (size_t)blockIdx.z * dframe + (size_t)y * dstep) + (size_t)x * 3;
    const double dmin = vals ? vals[2 * (size_t)blockIdx.z] : 0.0;
    float o[12];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const double d = und::dispAt(row, depth, x + p < w ? x + p : w - 1);
        und::reprojPoint(Q.q, x + p, y, d, vals && und::isMissing(d, dmin), o + 3 * p);
    }
    if (vec && x + 4 <= w) {
        float4* o4 = reinterpret_cast<float4*>(out);
        o4[0] = make_float4(o[0], o[1], o[2], o[3]); o4[1] = make_float4(o[4], o[5], o[6], o[7]); o4[2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) if (x + i / 3 < w) out[i] = o[i];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ host side
std::atomic<int> g_kernelMode{-1};      // mi355cv_undistortSetKernel: -1 the built-in rule, 0 composed (maps into scratch, then remap), 1 the tile kernel wherever it applies
std::atomic<int> g_ldsBytes{0};         // mi355cv_undistortSetLds: the tile kernel's LDS allotment in bytes, 0 = UNDIST_LDS_KIB
std::atomic<int> g_fpw{0};              // mi355cv_undistortSetFramesPerGroup: frames a workgroup walks, 0 = UNDIST_FRAMES_PER_GROUP

// the refusals of the camera, none needs a device; -> the rule
int ruleOf(const double* K, const double* dist, int ndist, const double* R, const double* newK, und::Rule* q)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!K);
    if (!(ndist == 0 || ndist == 4 || ndist == 5 || ndist == 8 || ndist == 12 || ndist == 14)) return MI355_DECLINED("ndist is none of 0, 4, 5, 8, 12, 14");
    MI355_DECLINE_IF(ndist > 0 && !dist);
    if (ndist == 14 && (dist[12] != 0 || dist[13] != 0)) return MI355_DECLINED("a non-zero tauX / tauY (the tilted sensor model) is not served");
    static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    memset(q, 0, sizeof *q);
    if (!und::inverse3x3(newK ? newK : K, R ? R : I, q->ir)) return MI355_DECLINED("newCameraMatrix * R is singular (its determinant is 0 or not finite)");
    for (int i = 0; i < std::min(ndist, 12); i++) q->k[i] = dist[i];
    q->fx = K[0]; q->fy = K[4]; q->u0 = K[2]; q->v0 = K[5];
    return MI355CV_OK;
}

int checkSize(int width, int height)
{
    MI355_DECLINE_IF(width < 1 || height < 1);
    if (width > lim::UNDIST_MAX_DIM || height > lim::UNDIST_MAX_DIM) return MI355_DECLINED("width or height above UNDIST_MAX_DIM = 16384");
    return MI355CV_OK;
}

// pitches, frame strides, src and dst that share bytes (host or device)
int checkFrames(const uchar* src, size_t sstep, size_t sframe, size_t srow, int sh, const uchar* dst, size_t dstep, size_t dframe, size_t drow, int dh, int nframes)
{
    MI355_DECLINE_IF(!src || !dst || nframes < 1);
    MI355_DECLINE_IF(sstep < srow || dstep < drow);
    if (nframes > 1) MI355_DECLINE_IF(sframe < span(sstep, sh, srow) || dframe < span(dstep, dh, drow));
    const size_t shull = (size_t)(nframes - 1) * sframe + span(sstep, sh, srow), dhull = (size_t)(nframes - 1) * dframe + span(dstep, dh, drow);
    if (src < dst + dhull && dst < src + shull) return MI355_DECLINED("src and dst overlap");
    return MI355CV_OK;
}

void launchMap(const und::Rule& q, int w, int h, int m1type, uchar* m1, size_t s1, uchar* m2, size_t s2)
{
    hipLaunchKernelGGL(k_undist_map, dim3(divUp(w, 64), divUp(h, 4)), dim3(256), 0, stream(), q, w, h, m1type, m1, s1, m2, s2);
}

// The built-in rule: the tile kernel in the classes (single / batch x channels) where profiles/undistort_bench.jsonl shows it ahead of remap with maps
// built beforehand, the times of a class's rows added up: every batch (2.3 to 4.2 times ahead), single frames of 3 and 4 channels; a single one-channel frame goes
// to the composed arm (1080p 19.0 against 13.5 us, 4K 44.9 against 37.4: the 40 double operations and two divisions a pixel outweigh the 6 bytes of map).
bool fusedByRule(int cn, bool batch) { return batch || cn != 1; }

struct Rectify {
    const char* entry; int src_type; const uchar* src; size_t sstep, sframe; int sw, sh; uchar* dst; size_t dstep, dframe; int dw, dh, nframes;
    und::Rule rule; int interpolation, border; const double* bv;
};

int runFused(const Rectify& c, int cn)
{
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(c.src, (size_t)c.dw * c.dh, minPixels(HOST_HEAVY)));
    und::TileArgs a;
    memset(&a, 0, sizeof a);
    a.rule = c.rule; a.sw = c.sw; a.sh = c.sh; a.dw = c.dw; a.dh = c.dh; a.nframes = c.nframes; a.border = c.border;
    const uchar* ds = c.src; uchar* dd = c.dst;
    size_t dss = c.sstep, dds = c.dstep;
    if (c.nframes == 1) {
        ds = stg.in(c.src, c.sstep, (size_t)c.sw * cn, c.sh, &dss);
        dd = stg.out(c.dst, c.dstep, (size_t)c.dw * cn, c.dh, &dds);
        MI355_DECLINE_IF(!ds || !dd);
    } else MI355_DECLINE_IF(!isDevicePtr(c.src) || !isDevicePtr(c.dst));
    a.sframe = c.nframes > 1 ? c.sframe : 0; a.dframe = c.nframes > 1 ? c.dframe : 0;
    MI355_DECLINE_IF(dss > 0xFFFFFFFFull || dds > 0xFFFFFFFFull);
    a.sstep = (uint32_t)dss; a.dstep = (uint32_t)dds;
    a.dwords = ((((uintptr_t)ds) | ((uintptr_t)dd) | dss | dds | a.sframe | a.dframe) & 3) == 0 && span(dss, c.sh, (size_t)c.sw * cn) < (1ull << 32);
    for (int k = 0; k < 4; k++) {                                                       // saturate_cast<uchar> of the border value as the samplers of warp.hip take it
        const float v = c.bv ? (float)c.bv[k] : 0.f;
        a.cval |= (uint32_t)(int)fminf(fmaxf(rintf(v), 0.f), 255.f) << (8 * k);
    }
    int lds = g_ldsBytes.load(std::memory_order_relaxed), fpw = g_fpw.load(std::memory_order_relaxed);
    a.ldsBytes = lds > 0 ? lds : lim::UNDIST_LDS_KIB << 10;
    a.fpw = fpw > 0 ? fpw : lim::UNDIST_FRAMES_PER_GROUP;
    const size_t ldsAsk = und::TILE_OFF + (size_t)std::max(a.ldsBytes, 256);
    const int th = cn == 1 ? warp8::tileRows<1>() : warp8::tileRows<3>();
    const int perLaunch = (int)std::min<long long>(c.nframes, (long long)MAX_GRID_FRAMES * a.fpw);           // the frame group is the grid's z
    int launches = 0;
    for (int f0 = 0; f0 < c.nframes; f0 += perLaunch, launches++) {
        a.nframes = std::min(perLaunch, c.nframes - f0);
        const dim3 grid(divUp(c.dw, warp8::TW), divUp(c.dh, th), divUp(a.nframes, a.fpw));
        const uchar* s = ds + (size_t)f0 * a.sframe; uchar* d = dd + (size_t)f0 * a.dframe;
        const und::TileArgs* da = (const und::TileArgs*)stg.param(&a, sizeof a);
        if (!da) return MI355_DECLINED("no scratch for the kernel's arguments");
        if (cn == 1) hipLaunchKernelGGL(k_undist8_tile<1>, grid, dim3(256), ldsAsk, stream(), s, d, da);
        else if (cn == 3) hipLaunchKernelGGL(k_undist8_tile<3>, grid, dim3(256), ldsAsk, stream(), s, d, da);
        else hipLaunchKernelGGL(k_undist8_tile<4>, grid, dim3(256), ldsAsk, stream(), s, d, da);
    }
    MI355_CHECK_LAUNCH(c.entry);
    noteKernel("k_undist8_tile<%d> grid=%dx%dx%d x256 lds=%d fpw=%d dwords=%d, %d frame(s) in %d launch(es)", cn, divUp(c.dw, warp8::TW), divUp(c.dh, th),
               divUp(std::min(perLaunch, c.nframes), a.fpw), a.ldsBytes, a.fpw, a.dwords, c.nframes, launches);
    return stg.finish(c.entry);
}

int runComposed(const Rectify& c)
{
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(c.src, (size_t)c.dw * c.dh, minPixels(HOST_HEAVY)));
    const size_t s1 = pad256((size_t)c.dw * 4), s2 = pad256((size_t)c.dw * 2);
    uchar* m1 = (uchar*)stg.scratch(s1 * c.dh);
    uchar* m2 = (uchar*)stg.scratch(s2 * c.dh);
    if (!m1 || !m2) return MI355_DECLINED("no scratch for the maps");
    launchMap(c.rule, c.dw, c.dh, T16SC2, m1, s1, m2, s2);
    MI355_CHECK_LAUNCH(c.entry);
    for (int f = 0; f < c.nframes; f++)          // nested entries: same stream, same scratch pool, no synchronisation of their own
        if (const int rc = mi355cv_remap(c.src_type, c.src + (size_t)f * c.sframe, c.sstep, c.sw, c.sh, c.dst + (size_t)f * c.dframe, c.dstep, c.dw, c.dh, m1, s1, T16SC2, m2, s2,
                                         T16UC1, c.interpolation, c.border, c.bv)) return rc;
    noteKernel("k_undist_map grid=%dx%d x256 + remap per frame (composed), %d frame(s)", divUp(c.dw, 64), divUp(c.dh, 4), c.nframes);
    return stg.finish(c.entry);
}

int runRectify(const char* entry, int src_type, const uchar* src, size_t sstep, size_t sframe, int sw, int sh, uchar* dst, size_t dstep, size_t dframe, int dw, int dh, int nframes,
               const double* K, const double* dist, int ndist, const double* R, const double* newK, int interpolation, int border, const double* bv)
{
    Rectify c = {entry, src_type, src, sstep, nframes == 1 ? 0 : sframe, sw, sh, dst, dstep, nframes == 1 ? 0 : dframe, dw, dh, nframes, {}, interpolation, border, bv};
    if (const int rc = ruleOf(K, dist, ndist, R, newK, &c.rule)) return rc;
    if (const int rc = checkSize(dw, dh)) return rc;
    MI355_DECLINE_IF(sw < 1 || sh < 1);
    if (sw > lim::UNDIST_MAX_SRC_DIM || sh > lim::UNDIST_MAX_SRC_DIM) return MI355_DECLINED("source width or height above UNDIST_MAX_SRC_DIM = 32767 (map entries are 16 bits)");
    const int depth = MI355CV_MAT_DEPTH(src_type), cn = MI355CV_MAT_CN(src_type);
    MI355_DECLINE_IF(depth < 0 || depth > 6 || cn < 1 || cn > 512);
    MI355_DECLINE_IF(border < 0 || border > B_TRANSPARENT);
    const size_t pix = (size_t)cn * depthBytes(depth);
    if (const int rc = checkFrames(src, sstep, sframe, pix * sw, sh, dst, dstep, dframe, pix * dw, dh, nframes)) return rc;
    if (nframes > 1 && hostBatchEligible(src, dst, nframes)) {        // frames in host memory
        if (border == B_TRANSPARENT) {               // the pipeline's device buffers do not hold the caller's pixels: frame by frame, which stages dst in as well
            for (int f = 0; f < nframes; f++)
                if (const int rc = mi355cv_undistortRectify(src_type, src + (size_t)f * sframe, sstep, sw, sh, dst + (size_t)f * dframe, dstep, dw, dh, K, dist, ndist, R, newK,
                                                            interpolation, border, bv)) return rc;
            return MI355CV_OK;
        }
        const HostBatch hb = {src, sstep, sframe, pix * sw, sh, dst, dstep, dframe, pix * dw, dh, nframes};
        return runHostBatch(entry, hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_undistortRectifyBatch(src_type, s, ss, sf, sw, sh, d, ds, df, dw, dh, nf, K, dist, ndist, R, newK, interpolation, border, bv); });
    }
    const int interp = (interpolation & 7) == MI355CV_INTER_AREA ? MI355CV_INTER_LINEAR : interpolation;
    const bool tileClass = depth == MI355CV_8U && (cn == 1 || cn == 3 || cn == 4) && interp == MI355CV_INTER_LINEAR && border != B_TRANSPARENT;
    const int mode = g_kernelMode.load(std::memory_order_relaxed);
    if (tileClass && (mode == 1 || (mode == -1 && fusedByRule(cn, nframes > 1)))) return runFused(c, cn);
    return runComposed(c);
}

int runReproject(const char* entry, const uchar* src, size_t sstep, size_t sframe, int disp_type, uchar* dst, size_t dstep, size_t dframe, int w, int h, int nframes, const double* Q,
                 int handleMissing, int ddepth)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!Q);
    const int depth = MI355CV_MAT_DEPTH(disp_type);
    if (MI355CV_MAT_CN(disp_type) != 1 || !(depth == MI355CV_8U || depth == MI355CV_16S || depth == MI355CV_32S || depth == MI355CV_32F))
        return MI355_DECLINED("the disparity is none of CV_8UC1, CV_16SC1, CV_32SC1, CV_32FC1");
    if (ddepth == MI355CV_16S || ddepth == MI355CV_32S) return MI355_DECLINED("CV_16SC3 / CV_32SC3 output is not served");
    MI355_DECLINE_IF(ddepth != -1 && ddepth != MI355CV_32F);
    MI355_DECLINE_IF(w < 1 || h < 1);
    if (w > lim::REPROJECT_MAX_DIM || h > lim::REPROJECT_MAX_DIM) return MI355_DECLINED("width or height above REPROJECT_MAX_DIM = 16384");
    const size_t esz = (size_t)depthBytes(depth), srow = (size_t)w * esz, drow = (size_t)w * 12;
    if (const int rc = checkFrames(src, sstep, sframe, srow, h, dst, dstep, dframe, drow, h, nframes)) return rc;
    if (sstep % esz || sframe % esz || (uintptr_t)src % esz || dstep % 4 || dframe % 4 || (uintptr_t)dst % 4)
        return MI355_DECLINED("an image, a pitch or a frame stride is no multiple of its element size");
    if (nframes > 1 && hostBatchEligible(src, dst, nframes)) {        // frames in host memory
        const HostBatch hb = {src, sstep, sframe, srow, h, dst, dstep, dframe, drow, h, nframes};
        return runHostBatch(entry, hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_reprojectImageTo3DBatch(s, ss, sf, disp_type, d, ds, df, w, h, nf, Q, handleMissing, ddepth); });
    }
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_CHEAP)));
    const uchar* ds = src; uchar* dd = dst;
    size_t dss = sstep, dds = dstep, dsf = nframes == 1 ? 0 : sframe, ddf = nframes == 1 ? 0 : dframe;
    if (nframes == 1) {
        ds = stg.in(src, sstep, srow, h, &dss);
        dd = stg.out(dst, dstep, drow, h, &dds);
        MI355_DECLINE_IF(!ds || !dd);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(dst));
    Q16 q;
    memcpy(q.q, Q, sizeof q.q);
    const int vec = ((((uintptr_t)dd) | dds | ddf) & 15) == 0;
    for (int f0 = 0; f0 < nframes; f0 += MAX_GRID_FRAMES) {
        const int nf = std::min(MAX_GRID_FRAMES, nframes - f0);
        const uchar* s = ds + (size_t)f0 * dsf;
        double* vals = nullptr;
        if (handleMissing) {                     // the frames' minima stay in HBM: the nested entry writes them where k_reproject3d reads them, in stream order
            vals = (double*)stg.scratch((size_t)nf * (2 * sizeof(double) + 4 * sizeof(int)));
            if (!vals) return MI355_DECLINED("no scratch for the minima");
            if (const int rc = mi355cv_minMaxLocBatch(s, dss, dsf, w, h, depth, nullptr, 0, 0, nf, vals, (int*)(vals + 2 * (size_t)nf))) return rc;
        }
        hipLaunchKernelGGL(k_reproject3d, dim3(divUp(w, 256), divUp(h, 4), nf), dim3(256), 0, stream(), s, dss, dsf, depth, dd + (size_t)f0 * ddf, dds, ddf, w, h, q, vals, vec);
    }
    MI355_CHECK_LAUNCH(entry);
    noteKernel("k_reproject3d grid=%dx%dx%d x256 depth=%d missing=%d vec=%d, %d frame(s)", divUp(w, 256), divUp(h, 4), std::min(nframes, MAX_GRID_FRAMES), depth, handleMissing ? 1 : 0,
               vec, nframes);
    return stg.finish(entry);
}

} // namespace

extern "C" {

MI355CV_API int mi355cv_initUndistortRectifyMap(const double* K, const double* dist, int ndist, const double* R, const double* newK, int width, int height, int m1type, void* map1,
                                                size_t map1_step, void* map2, size_t map2_step)
{
    mi355::EntryGuard entry_(__func__);
    und::Rule q;
    if (const int rc = ruleOf(K, dist, ndist, R, newK, &q)) return rc;
    if (const int rc = checkSize(width, height)) return rc;
    if (m1type != T32FC1 && m1type != T32FC2 && m1type != T16SC2) return MI355_DECLINED("m1type is none of CV_32FC1, CV_32FC2, CV_16SC2");
    const bool two = m1type != T32FC2;
    MI355_DECLINE_IF(!map1 || (two && !map2));
    const size_t r1 = (size_t)width * (m1type == T32FC2 ? 8 : 4), r2 = (size_t)width * (m1type == T16SC2 ? 2 : 4);
    MI355_DECLINE_IF(map1_step < r1 || (two && map2_step < r2));
    if (two && (uchar*)map1 < (uchar*)map2 + span(map2_step, height, r2) && (uchar*)map2 < (uchar*)map1 + span(map1_step, height, r1)) return MI355_DECLINED("map1 and map2 overlap");
    MI355_DECLINE_IF((uintptr_t)map1 % 4 || map1_step % 4 || (two && ((uintptr_t)map2 % (m1type == T16SC2 ? 2 : 4) || map2_step % (m1type == T16SC2 ? 2 : 4))));
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    size_t s1 = 0, s2 = 0;
    uchar* d1 = stg.out((uchar*)map1, map1_step, r1, height, &s1);
    uchar* d2 = two ? stg.out((uchar*)map2, map2_step, r2, height, &s2) : nullptr;
    MI355_DECLINE_IF(!d1 || (two && !d2));
    launchMap(q, width, height, m1type, d1, s1, d2, s2);
    MI355_CHECK_LAUNCH("initUndistortRectifyMap");
    noteKernel("k_undist_map grid=%dx%d x256 m1type=%d", divUp(width, 64), divUp(height, 4), m1type);
    return stg.finish("initUndistortRectifyMap");
}

MI355CV_API int mi355cv_undistortRectify(int src_type, const uchar* src, size_t src_step, int src_width, int src_height, uchar* dst, size_t dst_step, int dst_width, int dst_height,
                                         const double* K, const double* dist, int ndist, const double* R, const double* newK, int interpolation, int border_type,
                                         const double* border_value)
{
    mi355::EntryGuard entry_(__func__);
    return runRectify("undistortRectify", src_type, src, src_step, 0, src_width, src_height, dst, dst_step, 0, dst_width, dst_height, 1, K, dist, ndist, R, newK, interpolation,
                      border_type, border_value);
}

MI355CV_API int mi355cv_undistortRectifyBatch(int src_type, const uchar* src, size_t src_step, size_t src_frame_stride, int src_width, int src_height, uchar* dst, size_t dst_step,
                                              size_t dst_frame_stride, int dst_width, int dst_height, int nframes, const double* K, const double* dist, int ndist, const double* R,
                                              const double* newK, int interpolation, int border_type, const double* border_value)
{
    mi355::EntryGuard entry_(__func__);
    return runRectify("undistortRectifyBatch", src_type, src, src_step, src_frame_stride, src_width, src_height, dst, dst_step, dst_frame_stride, dst_width, dst_height, nframes, K,
                      dist, ndist, R, newK, interpolation, border_type, border_value);
}

MI355CV_API int mi355cv_reprojectImageTo3D(const uchar* disp, size_t disp_step, int disp_type, uchar* dst, size_t dst_step, int width, int height, const double* Q,
                                           int handleMissingValues, int ddepth)
{
    mi355::EntryGuard entry_(__func__);
    return runReproject("reprojectImageTo3D", disp, disp_step, 0, disp_type, dst, dst_step, 0, width, height, 1, Q, handleMissingValues, ddepth);
}

MI355CV_API int mi355cv_reprojectImageTo3DBatch(const uchar* disp, size_t disp_step, size_t disp_frame_stride, int disp_type, uchar* dst, size_t dst_step, size_t dst_frame_stride,
                                                int width, int height, int nframes, const double* Q, int handleMissingValues, int ddepth)
{
    mi355::EntryGuard entry_(__func__);
    return runReproject("reprojectImageTo3DBatch", disp, disp_step, disp_frame_stride, disp_type, dst, dst_step, dst_frame_stride, width, height, nframes, Q, handleMissingValues,
                        ddepth);
}

MI355CV_API int mi355cv_undistortSetKernel(int mode)
{
    if (mode < -1 || mode > 1) return MI355CV_ERROR_UNKNOWN;
    g_kernelMode.store(mode, std::memory_order_relaxed);
    return MI355CV_OK;
}

MI355CV_API int mi355cv_undistortSetLds(int bytes)
{
    if (bytes < 0 || bytes > (lim::UNDIST_MAX_LDS_KIB << 10)) return MI355CV_ERROR_UNKNOWN;
    g_ldsBytes.store(bytes, std::memory_order_relaxed);
    return MI355CV_OK;
}

MI355CV_API int mi355cv_undistortSetFramesPerGroup(int frames)
{
    if (frames < 0 || frames > lim::UNDIST_MAX_FRAMES_PER_GROUP) return MI355CV_ERROR_UNKNOWN;
    g_fpw.store(frames, std::memory_order_relaxed);
    return MI355CV_OK;
}

} // extern "C"
