// resize.hip -- row a7 of SURVEY.md §8: cv::resize (the warps that share its helpers are in warp.hip, the helpers in imgwarp_common.h).
//
// Reference semantics restated (all coordinate arithmetic is integer or IEEE double/float without contraction, so the
// device reproduces it bit for bit):
//   resize   hal::resize resize.cpp:3826-4194.  NEAREST: sx = min(floor(dx/fx), w-1) (:1026-1100).  LINEAR:
//            fx = float((dx+.5)*scale-.5), sx = floor(fx) (:4097-4190); 8U runs in fixed point -- 11-bit taps,
//            dst = ((b0*(t0>>4))>>16) + ((b1*(t1>>4))>>16) + 2) >> 2 (:1963-1989); other depths float mul/mul/add
//            (HResizeLinear :1877, VResizeLinear :1931; resize.cpp is built without FMA).  LINEAR at exactly 1/2 and
//            INTER_AREA with integer ratios take resizeAreaFast_ (:2919-3060): (a+b+c+d+2)>>2 for 2x2 integers.
// runResize at the end of the file is the dispatch rule: which kernel serves which call.
#include "rt.h"
#include <type_traits>
#include <map>
#include <tuple>
#include <memory>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>
#include <algorithm>
#include "warp8.h"
#include "resize_tab8.h"
#include "imgwarp_common.h"

using namespace mi355;

namespace {

// ---------------------------------------------------------------------------------- resize
struct ResizeArgs { int sw, sh, dw, dh, depth, cn; double scale_x, scale_y, inv_x, inv_y; int mode /*0 nn,1 linear,2 area-as-linear,3 areafast*/; int isx, isy;
                    int nnExact, ifx, ifx0, ify, ify0;   /* INTER_NEAREST_EXACT: 16.16 steps and half-pixel offsets of resizeNN_bitexact (resize.cpp:1267-1289) */
                    size_t sframe, dframe; /* bytes between the frames of a batch (grid z = frame) */ };

__device__ __forceinline__ void linCoef(int d, double scale, double inv, int areaMode, int& s, float& f)
{
    if (!areaMode) { f = (float)((d + 0.5) * scale - 0.5); s = cvFloorF(f); f -= s; }
    else { s = cvFloorD(d * scale); f = (float)((d + 1) - (s + 1) * inv); f = f <= 0 ? 0.f : f - cvFloorF(f); }
}

__global__ __launch_bounds__(256) void k_resize(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, ResizeArgs a)
{
    src += (size_t)blockIdx.z * a.sframe; dst += (size_t)blockIdx.z * a.dframe;
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= a.dw || dy >= a.dh) return;
    const int e = eszOf(a.depth), cn = a.cn;
    uchar* D = dst + (size_t)dy * dstep;
    if (a.mode == 0) {
        int sy = a.nnExact ? (a.ify * dy + a.ify0) >> 16 : cvFloorD(dy * a.scale_y); sy = sy > a.sh - 1 ? a.sh - 1 : sy;
        int sx = a.nnExact ? (a.ifx * dx + a.ifx0) >> 16 : cvFloorD(dx * a.scale_x); sx = sx > a.sw - 1 ? a.sw - 1 : sx;
        copyPix(D + (size_t)dx * cn * e, src + (size_t)sy * sstep + (size_t)sx * cn * e, cn * e);
        return;
    }
    if (a.mode == 3) {
        const int area = a.isx * a.isy;
        const float scale = 1.f / area;
        const bool fast2 = a.isx == 2 && a.isy == 2 && (cn == 1 || cn == 3 || cn == 4) && a.depth != D32F;
        const int sy0 = dy * a.isy;
        const int wfull = sy0 + a.isy <= a.sh ? a.sw / a.isx : 0;
        for (int c = 0; c < cn; c++) {
            const int idx = dx * cn + c;
            if (sy0 >= a.sh) { stRound(D, a.depth, idx, 0.f); continue; }
            if (dx < wfull) {
                if (fast2) {
                    int s = 0;
                    for (int sy = 0; sy < 2; sy++) for (int sx = 0; sx < 2; sx++)
                        s += (int)ldV(src + (size_t)(sy0 + sy) * sstep, a.depth, (dx * 2 + sx) * cn + c);
                    s = (s + 2) >> 2;
                    if (a.depth == D8U) D[idx] = (uchar)s; else if (a.depth == D16U) reinterpret_cast<unsigned short*>(D)[idx] = (unsigned short)s;
                    else reinterpret_cast<short*>(D)[idx] = (short)s;
                } else if (a.depth == D8U) {
                    int s = 0;
                    for (int sy = 0; sy < a.isy; sy++) for (int sx = 0; sx < a.isx; sx++)
                        s += src[(size_t)(sy0 + sy) * sstep + (dx * a.isx + sx) * cn + c];
                    stRound(D, a.depth, idx, s * scale);
                } else if (a.depth == D32F && a.isx == 2 && a.isy == 2) {
                    const float* r0 = reinterpret_cast<const float*>(src + (size_t)sy0 * sstep);
                    const float* r1 = reinterpret_cast<const float*>(src + (size_t)(sy0 + 1) * sstep);
                    // ResizeAreaFastVec_SIMD_32f (resize.cpp:2856-2905) sums pairwise, (s00 + s01) + (s10 + s11), for 1 channel below the last multiple of its 4 lanes and
                    // for every 4-channel pixel; the scalar loop behind it (:3013-3025: the 1-channel tail, 2 and 3 channels) sums in order, ((s00 + s01) + s10) + s11
                    const float s00 = r0[(dx * 2) * cn + c], s01 = r0[(dx * 2 + 1) * cn + c], s10 = r1[(dx * 2) * cn + c], s11 = r1[(dx * 2 + 1) * cn + c];
                    const bool pairwise = cn == 4 || (cn == 1 && dx < (wfull / 4) * 4);
                    const float s = pairwise ? __fadd_rn(__fadd_rn(s00, s01), __fadd_rn(s10, s11)) : __fadd_rn(__fadd_rn(__fadd_rn(s00, s01), s10), s11);
                    reinterpret_cast<float*>(D)[idx] = __fmul_rn(s, 0.25f);
                } else {
                    float s = 0;
                    for (int sy = 0; sy < a.isy; sy++) for (int sx = 0; sx < a.isx; sx++)
                        s += ldV(src + (size_t)(sy0 + sy) * sstep, a.depth, (dx * a.isx + sx) * cn + c);
                    stRound(D, a.depth, idx, s * scale);
                }
            } else {
                float s = 0; int is = 0, count = 0;
                const int sx0 = dx * a.isx * cn + c;
                for (int sy = 0; sy < a.isy; sy++) {
                    if (sy0 + sy >= a.sh) break;
                    for (int sx = 0; sx < a.isx * cn; sx += cn) {
                        if (sx0 - c + sx >= a.sw * cn) break;
                        if (a.depth == D8U) is += src[(size_t)(sy0 + sy) * sstep + sx0 + sx];
                        else s += ldV(src + (size_t)(sy0 + sy) * sstep, a.depth, sx0 + sx);
                        count++;
                    }
                }
                if (count == 0) { stRound(D, a.depth, idx, 0.f); continue; }
                stRound(D, a.depth, idx, (a.depth == D8U ? (float)is : s) / count);
            }
        }
        return;
    }
    const int areaMode = a.mode == 2;
    int sy, sx; float fy, fx;
    linCoef(dy, a.scale_y, a.inv_y, areaMode, sy, fy);
    linCoef(dx, a.scale_x, a.inv_x, areaMode, sx, fx);
    const int y0 = clipI(sy, 0, a.sh), y1 = clipI(sy + 1, 0, a.sh);
    if (sx < 0) { fx = 0; sx = 0; }
    bool edge = false;
    if (sx + 1 >= a.sw) { edge = true; if (sx >= a.sw - 1) { fx = 0; sx = a.sw - 1; } }
    const float b0f = 1.f - fy, b1f = fy, a0f = 1.f - fx, a1f = fx;
    const uchar* r0 = src + (size_t)y0 * sstep;
    const uchar* r1 = src + (size_t)y1 * sstep;
    if (a.depth == D8U) {
        const int b0 = satShort(__float2int_rn(b0f * 2048)), b1 = satShort(__float2int_rn(b1f * 2048));
        const int a0 = satShort(__float2int_rn(a0f * 2048)), a1 = satShort(__float2int_rn(a1f * 2048));
        for (int c = 0; c < cn; c++) {
            const int i0 = sx * cn + c, i1 = i0 + cn;
            const int t0 = edge ? r0[i0] * 2048 : r0[i0] * a0 + r0[i1] * a1;
            const int t1 = edge ? r1[i0] * 2048 : r1[i0] * a0 + r1[i1] * a1;
            D[dx * cn + c] = (uchar)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2);
        }
        return;
    }
    for (int c = 0; c < cn; c++) {
        const int i0 = sx * cn + c, i1 = i0 + cn;
        const float p00 = ldV(r0, a.depth, i0), p10 = ldV(r1, a.depth, i0);
        float t0, t1;
        if (edge) { t0 = p00; t1 = p10; }
        else {
            const float p01 = ldV(r0, a.depth, i1), p11 = ldV(r1, a.depth, i1);
            t0 = __fadd_rn(__fmul_rn(p00, a0f), __fmul_rn(p01, a1f));
            t1 = __fadd_rn(__fmul_rn(p10, a0f), __fmul_rn(p11, a1f));
        }
        stRound(D, a.depth, dx * cn + c, __fadd_rn(__fmul_rn(t0, b0f), __fmul_rn(t1, b1f)));
    }
}

// INTER_AREA by exactly 2 x 2 on CV_8U (resizeAreaFast_, ResizeAreaFastVec_SIMD_8u, resize.cpp:2806-2900: (s00 + s01 + s10 + s11 + 2) >> 2), even
// source sizes: a lane produces FOUR destination pixels from 8 CN source bytes of each of the two source rows -- 8-byte loads, 4 CN-byte stores --
// instead of a thread per destination pixel with byte loads; HBM-bound (5 bytes per destination byte)
template <int CN>
__global__ __launch_bounds__(256) void k_area2x2_u8(const uchar* __restrict__ src, size_t sstep, size_t sframe, uchar* __restrict__ dst, size_t dstep, size_t dframe,
                                                    int dw, int dh)
{
    constexpr int NS = 2 * CN;                                     // source dwords per row and lane (8 CN bytes)
    const int g = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int ng = (dw + 3) >> 2;
    if (g >= ng || dy >= dh) return;
    const uchar* r0 = src + (size_t)blockIdx.z * sframe + (size_t)(2 * dy) * sstep + (size_t)g * 8 * CN;
    const uchar* r1 = r0 + sstep;
    uchar* D = dst + (size_t)blockIdx.z * dframe + (size_t)dy * dstep + (size_t)g * 4 * CN;
    if (4 * g + 4 <= dw) {
        uint32_t a[NS], b[NS];
#pragma unroll
        for (int i = 0; i < CN; i++) {
            const uint2 va = reinterpret_cast<const uint2*>(r0)[i], vb = reinterpret_cast<const uint2*>(r1)[i];
            a[2 * i] = va.x; a[2 * i + 1] = va.y; b[2 * i] = vb.x; b[2 * i + 1] = vb.y;
        }
        uint32_t o[CN] = {};
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const int i0 = (2 * p) * CN + c, i1 = i0 + CN, ob = p * CN + c;
                const uint32_t s = ((a[i0 >> 2] >> (8 * (i0 & 3))) & 255u) + ((a[i1 >> 2] >> (8 * (i1 & 3))) & 255u) +
                                   ((b[i0 >> 2] >> (8 * (i0 & 3))) & 255u) + ((b[i1 >> 2] >> (8 * (i1 & 3))) & 255u);
                o[ob >> 2] |= ((s + 2) >> 2) << (8 * (ob & 3));
            }
#pragma unroll
        for (int i = 0; i < CN; i++) reinterpret_cast<uint32_t*>(D)[i] = o[i];
    } else {
        for (int p = 0; 4 * g + p < dw; p++)
            for (int c = 0; c < CN; c++) {
                const int i0 = (2 * p) * CN + c, i1 = i0 + CN;
                D[p * CN + c] = (uchar)((r0[i0] + r0[i1] + r1[i0] + r1[i1] + 2) >> 2);
            }
    }
}

// INTER_AREA by exactly 2 x 2 on CV_32FC1 (cfg3's 8K -> 4K; ResizeAreaFastVec_SIMD_32f resize.cpp:2928-2960: (s00 + s01) + (s10 + s11), times 0.25f), even
// source sizes: a lane produces FOUR destination floats from two dwordx4 loads of each of the two source rows and stores one dwordx4 -- the thread-per-pixel
// form ran at 54 % of HBM (its 8-byte loads and 4-byte stores leave the memory system half-used); 20 bytes per destination float
__global__ __launch_bounds__(256) void k_area2x2_f32(const uchar* __restrict__ src, size_t sstep, size_t sframe, uchar* __restrict__ dst, size_t dstep, size_t dframe,
                                                     int dw, int dh)
{
    const int g = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (4 * g >= dw || dy >= dh) return;
    const float* r0 = reinterpret_cast<const float*>(src + (size_t)blockIdx.z * sframe + (size_t)(2 * dy) * sstep) + 8 * (size_t)g;
    const float* r1 = reinterpret_cast<const float*>(reinterpret_cast<const uchar*>(r0) + sstep);
    float* D = reinterpret_cast<float*>(dst + (size_t)blockIdx.z * dframe + (size_t)dy * dstep) + 4 * (size_t)g;
    if (4 * g + 4 <= dw) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const f32x4 a0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(r0)), a1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(r0) + 1);
        const f32x4 b0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(r1)), b1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(r1) + 1);
        f32x4 o;
        o.x = __fmul_rn(__fadd_rn(__fadd_rn(a0.x, a0.y), __fadd_rn(b0.x, b0.y)), 0.25f);
        o.y = __fmul_rn(__fadd_rn(__fadd_rn(a0.z, a0.w), __fadd_rn(b0.z, b0.w)), 0.25f);
        o.z = __fmul_rn(__fadd_rn(__fadd_rn(a1.x, a1.y), __fadd_rn(b1.x, b1.y)), 0.25f);
        o.w = __fmul_rn(__fadd_rn(__fadd_rn(a1.z, a1.w), __fadd_rn(b1.z, b1.w)), 0.25f);
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(D));
    } else {
        // the last dw % 4 columns are the reference's scalar tail (resize.cpp:3013-3025): ((s00 + s01) + s10) + s11, not the vector body's pairwise sums
        for (int p = 0; 4 * g + p < dw; p++) D[p] = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(r0[2 * p], r0[2 * p + 1]), r1[2 * p]), r1[2 * p + 1]), 0.25f);
    }
}

// resize, bilinear (and INTER_AREA upscaling, which is bilinear with other coefficients), single channel CV_32F / CV_8U: the
// arithmetic of k_resize specialised.  A thread owns a destination column for RROWS rows: its horizontal coefficient is
// computed once, both horizontal taps come from one unaligned 8-byte / 2-byte load per source row, and a wave walks down
// so that the source rows shared by consecutive destination rows are L1 hits.
constexpr int RROWS = 8;
template <typename T>
__global__ __launch_bounds__(256) void k_resize_lin1(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, ResizeArgs a)
{
    src += (size_t)blockIdx.z * a.sframe; dst += (size_t)blockIdx.z * a.dframe;
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int yb = (blockIdx.y * 4 + (threadIdx.x >> 6)) * RROWS;
    if (dx >= a.dw || yb >= a.dh) return;
    const int areaMode = a.mode == 2;
    int sx; float fx;
    linCoef(dx, a.scale_x, a.inv_x, areaMode, sx, fx);
    if (sx < 0) { fx = 0; sx = 0; }
    bool edge = false;
    if (sx + 1 >= a.sw) { edge = true; if (sx >= a.sw - 1) { fx = 0; sx = a.sw - 1; } }
    const float a0f = 1.f - fx, a1f = fx;
    const int a0 = satShort(__float2int_rn(a0f * 2048)), a1 = satShort(__float2int_rn(a1f * 2048));
    const int xoff = (edge ? sx - 1 : sx);                  // the pair (xoff, xoff+1) is always inside the row when sw >= 2
    const int ye = min(yb + RROWS, a.dh);
    for (int dy = yb; dy < ye; dy++) {
        int sy; float fy;
        linCoef(dy, a.scale_y, a.inv_y, areaMode, sy, fy);
        const int y0 = clipI(sy, 0, a.sh), y1 = clipI(sy + 1, 0, a.sh);
        const float b0f = 1.f - fy, b1f = fy;
        const uchar* r0 = src + (size_t)y0 * sstep + (size_t)xoff * sizeof(T);
        const uchar* r1 = src + (size_t)y1 * sstep + (size_t)xoff * sizeof(T);
        if (sizeof(T) == 4) {
            typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
            const f2u p0 = *reinterpret_cast<const f2u*>(r0), p1 = *reinterpret_cast<const f2u*>(r1);
            float t0, t1;
            if (edge) { t0 = p0.y; t1 = p1.y; }
            else { t0 = __fadd_rn(__fmul_rn(p0.x, a0f), __fmul_rn(p0.y, a1f)); t1 = __fadd_rn(__fmul_rn(p1.x, a0f), __fmul_rn(p1.y, a1f)); }
            reinterpret_cast<float*>(dst + (size_t)dy * dstep)[dx] = __fadd_rn(__fmul_rn(t0, b0f), __fmul_rn(t1, b1f));
        } else {
            typedef unsigned short u16u __attribute__((aligned(1)));
            const int q0 = *reinterpret_cast<const u16u*>(r0), q1 = *reinterpret_cast<const u16u*>(r1);
            const int b0 = satShort(__float2int_rn(b0f * 2048)), b1 = satShort(__float2int_rn(b1f * 2048));
            const int t0 = edge ? (q0 >> 8) * 2048 : (q0 & 255) * a0 + (q0 >> 8) * a1;
            const int t1 = edge ? (q1 >> 8) * 2048 : (q1 & 255) * a0 + (q1 >> 8) * a1;
            (dst + (size_t)dy * dstep)[dx] = (uchar)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

// the same for interleaved channels: a thread owns one destination PIXEL column; the 2*CN source elements of its two
// horizontal taps are adjacent in memory and come from one unaligned load per source row (8 bytes for 3 or 4 8-bit channels,
// CN float pairs otherwise); the last source columns, where that load would leave the row, read element by element
template <typename T, int CN>
__global__ __launch_bounds__(256) void k_resize_linC(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, ResizeArgs a)
{
    src += (size_t)blockIdx.z * a.sframe; dst += (size_t)blockIdx.z * a.dframe;
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int yb = (blockIdx.y * 4 + (threadIdx.x >> 6)) * RROWS;
    if (dx >= a.dw || yb >= a.dh) return;
    const int areaMode = a.mode == 2;
    int sx; float fx;
    linCoef(dx, a.scale_x, a.inv_x, areaMode, sx, fx);
    if (sx < 0) { fx = 0; sx = 0; }
    bool edge = false;
    if (sx + 1 >= a.sw) { edge = true; if (sx >= a.sw - 1) { fx = 0; sx = a.sw - 1; } }
    const float a0f = 1.f - fx, a1f = fx;
    const int a0 = satShort(__float2int_rn(a0f * 2048)), a1 = satShort(__float2int_rn(a1f * 2048));
    const bool wide = sizeof(T) == 4 ? !edge : (sx * CN + 8 <= a.sw * CN);       // the 8-byte load stays inside the row
    const int ye = min(yb + RROWS, a.dh);
    for (int dy = yb; dy < ye; dy++) {
        int sy; float fy;
        linCoef(dy, a.scale_y, a.inv_y, areaMode, sy, fy);
        const int y0 = clipI(sy, 0, a.sh), y1 = clipI(sy + 1, 0, a.sh);
        const float b0f = 1.f - fy, b1f = fy;
        const uchar* r0 = src + (size_t)y0 * sstep + (size_t)sx * CN * sizeof(T);
        const uchar* r1 = src + (size_t)y1 * sstep + (size_t)sx * CN * sizeof(T);
        if (sizeof(T) == 4) {
            float* D = reinterpret_cast<float*>(dst + (size_t)dy * dstep) + (size_t)dx * CN;
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const float p00 = reinterpret_cast<const float*>(r0)[c], p10 = reinterpret_cast<const float*>(r1)[c];
                float t0 = p00, t1 = p10;
                if (!edge) {
                    const float p01 = reinterpret_cast<const float*>(r0)[CN + c], p11 = reinterpret_cast<const float*>(r1)[CN + c];
                    t0 = __fadd_rn(__fmul_rn(p00, a0f), __fmul_rn(p01, a1f)); t1 = __fadd_rn(__fmul_rn(p10, a0f), __fmul_rn(p11, a1f));
                }
                D[c] = __fadd_rn(__fmul_rn(t0, b0f), __fmul_rn(t1, b1f));
            }
        } else {
            const int b0 = satShort(__float2int_rn(b0f * 2048)), b1 = satShort(__float2int_rn(b1f * 2048));
            unsigned long long q0 = 0, q1 = 0;
            if (wide) {
                typedef unsigned long long u64u __attribute__((aligned(1)));
                q0 = *reinterpret_cast<const u64u*>(r0); q1 = *reinterpret_cast<const u64u*>(r1);
            } else {
                const int nb = edge ? CN : 2 * CN;
                for (int k = 0; k < nb; k++) { q0 |= (unsigned long long)r0[k] << (8 * k); q1 |= (unsigned long long)r1[k] << (8 * k); }
            }
            uchar* D = dst + (size_t)dy * dstep + (size_t)dx * CN;
            unsigned pk = 0;
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const int p00 = (int)((q0 >> (8 * c)) & 255), p01 = (int)((q0 >> (8 * (CN + c))) & 255);
                const int p10 = (int)((q1 >> (8 * c)) & 255), p11 = (int)((q1 >> (8 * (CN + c))) & 255);
                const int t0 = edge ? p00 * 2048 : p00 * a0 + p01 * a1;
                const int t1 = edge ? p10 * 2048 : p10 * a0 + p11 * a1;
                const unsigned r = (unsigned)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2) & 255u;
                pk |= r << (8 * c);
            }
            if (CN == 4) *reinterpret_cast<unsigned*>(D) = pk;
            else { D[0] = (uchar)pk; D[1] = (uchar)(pk >> 8); D[2] = (uchar)(pk >> 16); }
        }
    }
}

// true INTER_AREA (shrinking by non-integer ratios): computeResizeAreaTab resize.cpp:3334 + ResizeArea_Invoker :3181.  The two
// tap tables are built on the host exactly as the reference builds them (double arithmetic, float weights); per output element
// sum = b0*buf0, sum += bj*bufj with bufj = ((0 + S[k0]*a0) + S[k1]*a1) + ..., float multiply and add kept separate, then
// saturate_cast<T>.  Thread per output element; the taps of a 4K -> 720p shrink are 3-4 per axis.
struct AreaTap { int si; float alpha; };

template <typename T>
__global__ __launch_bounds__(256) void k_resize_area(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, int dw, int dh, int cn, int depth,
                                                     const AreaTap* __restrict__ xt, const int* __restrict__ xo, const AreaTap* __restrict__ yt, const int* __restrict__ yo)
{
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (e >= dw * cn || dy >= dh) return;
    const int dx = e / cn, c = e - dx * cn;
    const int k0 = xo[dx], k1 = xo[dx + 1], j0 = yo[dy], j1 = yo[dy + 1];
    float sum = 0.f;
    for (int j = j0; j < j1; j++) {
        const T* S = reinterpret_cast<const T*>(src + (size_t)yt[j].si * sstep);
        float buf = 0.f;
        for (int k = k0; k < k1; k++) buf = __fadd_rn(buf, __fmul_rn((float)S[xt[k].si * cn + c], xt[k].alpha));
        const float t = __fmul_rn(yt[j].alpha, buf);
        sum = j == j0 ? t : __fadd_rn(sum, t);
    }
    stRound(dst + (size_t)dy * dstep, depth, e, sum);
}

int buildAreaTab(int ssize, int dsize, double scale, std::vector<AreaTap>& tab, std::vector<int>& ofs)
{
    tab.clear(); ofs.assign((size_t)dsize + 1, 0);
    for (int dx = 0; dx < dsize; dx++) {
        ofs[(size_t)dx] = (int)tab.size();
        const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
        const double cellWidth = std::min(scale, ssize - fsx1);
        int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
        sx2 = std::min(sx2, ssize - 1);
        sx1 = std::min(sx1, sx2);
        if (sx1 - fsx1 > 1e-3) tab.push_back({sx1 - 1, (float)((sx1 - fsx1) / cellWidth)});
        for (int sx = sx1; sx < sx2; sx++) tab.push_back({sx, (float)(1.0 / cellWidth)});
        if (fsx2 - sx2 > 1e-3) tab.push_back({sx2, (float)(std::min(std::min(fsx2 - sx2, 1.), cellWidth) / cellWidth)});
    }
    ofs[(size_t)dsize] = (int)tab.size();
    return (int)tab.size();
}

// INTER_CUBIC for CV_8U / CV_32F (resize.cpp: coefficient set-up :4097-4190, interpolateCubic :964, HResizeCubic :1993,
// VResizeCubic :2045).  The per-column / per-row taps are built on the host exactly as the reference builds them (float, A = -0.75;
// 8U: * 2048 rounded to short).  The reference's vertical pass has a SIMD body and a scalar tail that round differently; both are
// reproduced per element index: body = float S0*b0 + (S1*b1 + (S2*b2 + S3*b3)) (8U: taps * 2^-22, round half-even, saturate) for
// e < (dw*cn / 8) * 8 (8U) or (dw*cn / 4) * 4 (32F); tail = exact integers (sum + 2^21) >> 22 (8U) / left-to-right float (32F).
// CV_16U / CV_16S take the float path of CV_32F (HResizeCubic / HResizeLanczos4 <ushort | short, float, float>, resize.cpp:3890-3925): samples converted to
// float, vertical result through Cast<float, T> = cvRound + saturation.  Their vector bodies are 8 elements wide (VResizeCubicVec_32f16u / 32f16s :1444-1488,
// VResizeLanczos4Vec_32f16s :1562-1594: nested from the last row, like CV_32F's); CV_16U Lanczos runs the SSE4.1 routine on x86, which sums
// left to right like the scalar tail (resize.sse4_1.cpp:189-226), so its body and tail coincide.
template <typename T> __device__ __forceinline__ float ldE(const uchar* row, int idx) { return (float)reinterpret_cast<const T*>(row)[idx]; }
template <typename T> __device__ __forceinline__ void stE(uchar* row, int idx, float v)
{
    if constexpr (sizeof(T) == 4) reinterpret_cast<float*>(row)[idx] = v;
    else if constexpr (std::is_same<T, unsigned short>::value) { const int r = __float2int_rn(v); reinterpret_cast<unsigned short*>(row)[idx] = (unsigned short)(r < 0 ? 0 : r > 65535 ? 65535 : r); }
    else { const int r = __float2int_rn(v); reinterpret_cast<short*>(row)[idx] = (short)(r < -32768 ? -32768 : r > 32767 ? 32767 : r); }
}
template <typename T, int NT> __device__ __forceinline__ int vecBody(int width)      // elements the reference's nested (last row first) vector form covers
{
    if (NT == 8 && std::is_same<T, unsigned short>::value) return 0;
    return sizeof(T) == 4 ? (width / 4) * 4 : (width / 8) * 8;
}

typedef rt8::Tap<4> CubicTap;                                            // resize_tab8.h: {int s; float f[4]; short i[4];}

template <typename T>
__global__ __launch_bounds__(256) void k_resize_cubic(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, int sw, int sh, int dw, int dh, int cn,
                                                      const CubicTap* __restrict__ xt, const CubicTap* __restrict__ yt)
{
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int width = dw * cn;
    if (e >= width || dy >= dh) return;
    const int dx = e / cn, c = e - dx * cn;
    const CubicTap tx = xt[dx], ty = yt[dy];
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; j++) xs[j] = clipI(tx.s - 1 + j, 0, sw) * cn + c;
    if (sizeof(T) == 1) {
        int S[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uchar* R = src + (size_t)clipI(ty.s - 1 + k, 0, sh) * sstep;
            S[k] = R[xs[0]] * tx.i[0] + R[xs[1]] * tx.i[1] + R[xs[2]] * tx.i[2] + R[xs[3]] * tx.i[3];
        }
        int r;
        if (e < (width / 8) * 8) {
            const float sc = 1.f / (2048.f * 2048.f);
            float t = __fmul_rn((float)S[3], __fmul_rn((float)ty.i[3], sc));
            t = __fadd_rn(__fmul_rn((float)S[2], __fmul_rn((float)ty.i[2], sc)), t);
            t = __fadd_rn(__fmul_rn((float)S[1], __fmul_rn((float)ty.i[1], sc)), t);
            t = __fadd_rn(__fmul_rn((float)S[0], __fmul_rn((float)ty.i[0], sc)), t);
            r = __float2int_rn(t);
        } else
            r = (S[0] * ty.i[0] + S[1] * ty.i[1] + S[2] * ty.i[2] + S[3] * ty.i[3] + (1 << 21)) >> 22;
        (dst + (size_t)dy * dstep)[e] = (uchar)(r < 0 ? 0 : r > 255 ? 255 : r);
    } else {
        float S[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uchar* R = src + (size_t)clipI(ty.s - 1 + k, 0, sh) * sstep;
            float v = __fmul_rn(ldE<T>(R, xs[0]), tx.f[0]);
            v = __fadd_rn(v, __fmul_rn(ldE<T>(R, xs[1]), tx.f[1]));
            v = __fadd_rn(v, __fmul_rn(ldE<T>(R, xs[2]), tx.f[2]));
            v = __fadd_rn(v, __fmul_rn(ldE<T>(R, xs[3]), tx.f[3]));
            S[k] = v;
        }
        float r;
        if (e < vecBody<T, 4>(width)) {
            float t = __fmul_rn(S[3], ty.f[3]);
            t = __fadd_rn(__fmul_rn(S[2], ty.f[2]), t);
            t = __fadd_rn(__fmul_rn(S[1], ty.f[1]), t);
            r = __fadd_rn(__fmul_rn(S[0], ty.f[0]), t);
        } else {
            float t = __fmul_rn(S[0], ty.f[0]);
            t = __fadd_rn(t, __fmul_rn(S[1], ty.f[1]));
            t = __fadd_rn(t, __fmul_rn(S[2], ty.f[2]));
            r = __fadd_rn(t, __fmul_rn(S[3], ty.f[3]));
        }
        stE<T>(dst + (size_t)dy * dstep, e, r);
    }
}

using rt8::buildCubicTab;                                                // coefficients: resize_tab8.h

// INTER_LANCZOS4 (resize.cpp:974-1003 coefficients, :2066-2158 passes): 8 x 8 taps at s-3 .. s+4, clamped.  CV_8U is integer throughout
// (taps * 2048 as shorts, (sum + 2^21) >> 22); CV_32F sums the row left to right and the column as the reference's vector body does
// (S0*b0 + (S1*b1 + ( ... + S7*b7))) below the last multiple of four elements, left to right in its scalar tail.
typedef rt8::Tap<8> LanczosTap;

template <typename T>
__global__ __launch_bounds__(256) void k_resize_lanczos(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, int sw, int sh, int dw, int dh, int cn,
                                                        const LanczosTap* __restrict__ xt, const LanczosTap* __restrict__ yt)
{
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int width = dw * cn;
    if (e >= width || dy >= dh) return;
    const int dx = e / cn, c = e - dx * cn;
    const LanczosTap tx = xt[dx], ty = yt[dy];
    int xs[8];
#pragma unroll
    for (int j = 0; j < 8; j++) xs[j] = clipI(tx.s - 3 + j, 0, sw) * cn + c;
    if (sizeof(T) == 1) {
        int r = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uchar* R = src + (size_t)clipI(ty.s - 3 + k, 0, sh) * sstep;
            int v = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) v += R[xs[j]] * tx.i[j];
            r += v * ty.i[k];
        }
        r = (r + (1 << 21)) >> 22;
        (dst + (size_t)dy * dstep)[e] = (uchar)(r < 0 ? 0 : r > 255 ? 255 : r);
    } else {
        float S[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uchar* R = src + (size_t)clipI(ty.s - 3 + k, 0, sh) * sstep;
            float v = __fmul_rn(ldE<T>(R, xs[0]), tx.f[0]);
#pragma unroll
            for (int j = 1; j < 8; j++) v = __fadd_rn(v, __fmul_rn(ldE<T>(R, xs[j]), tx.f[j]));
            S[k] = v;
        }
        float r;
        if (e < vecBody<T, 8>(width)) {
            r = __fmul_rn(S[7], ty.f[7]);
#pragma unroll
            for (int k = 6; k >= 0; k--) r = __fadd_rn(__fmul_rn(S[k], ty.f[k]), r);
        } else {
            r = __fmul_rn(S[0], ty.f[0]);
#pragma unroll
            for (int k = 1; k < 8; k++) r = __fadd_rn(r, __fmul_rn(S[k], ty.f[k]));
        }
        stE<T>(dst + (size_t)dy * dstep, e, r);
    }
}

using rt8::buildLanczosTab;

// The separable form of the two kernels above for tiles of 64 x 16 output elements: the horizontal sums of every source row a tile
// needs are computed ONCE into LDS (they are exactly the S_k of the per-output kernels, same tap order), then each output combines NT of
// them vertically with the reference's body / tail formulas.  A 2x cubic upscale goes from 16 gathers + 20 MACs per output to about 3 + 7.
// The host checks that no tile needs more than RMAX source rows (strong minification does; it stays on the per-output kernels).
template <int NT> using TapT = rt8::Tap<NT>;                             // CubicTap (NT = 4) and LanczosTap (NT = 8)

template <typename T, int NT>
__global__ __launch_bounds__(256) void k_resize_tiled(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, int sw, int sh, int dw, int dh, int cn,
                                                      const TapT<NT>* __restrict__ xt, const TapT<NT>* __restrict__ yt)
{
    constexpr int TW = 64, TH = 16, OFF = NT / 2 - 1;
    typedef typename std::conditional<sizeof(T) == 1, int, float>::type HT;
    extern __shared__ __attribute__((aligned(16))) uchar ldsRaw[];
    HT* H = reinterpret_cast<HT*>(ldsRaw);
    const int width = dw * cn;
    const int lx = threadIdx.x & 63, e = blockIdx.x * TW + lx;
    const int dy0 = blockIdx.y * TH, dyLast = min(dy0 + TH, dh) - 1;
    const int rmin = yt[dy0].s - OFF, R = yt[dyLast].s - OFF + NT - 1 - rmin + 1;
    if (e < width) {
        const int dx = e / cn, c = e - dx * cn;
        const TapT<NT> tx = xt[dx];
        int xs[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) xs[j] = clipI(tx.s - OFF + j, 0, sw) * cn + c;
        for (int r = threadIdx.x >> 6; r < R; r += 4) {
            const uchar* rowp = src + (size_t)clipI(rmin + r, 0, sh) * sstep;
            if (sizeof(T) == 1) {
                int v = 0;
#pragma unroll
                for (int j = 0; j < NT; j++) v += rt8::mul24((int)rowp[xs[j]], (int)tx.i[j]);      // a byte times a tap * 2048: 24-bit multiply (full rate)
                H[r * TW + lx] = (HT)v;
            } else {
                float v = __fmul_rn(ldE<T>(rowp, xs[0]), tx.f[0]);
#pragma unroll
                for (int j = 1; j < NT; j++) v = __fadd_rn(v, __fmul_rn(ldE<T>(rowp, xs[j]), tx.f[j]));
                H[r * TW + lx] = (HT)v;
            }
        }
    }
    __syncthreads();
    if (e >= width) return;
#pragma unroll
    for (int k4 = 0; k4 < TH / 4; k4++) {
        const int dy = dy0 + (threadIdx.x >> 6) + 4 * k4;
        if (dy >= dh) continue;
        const TapT<NT> ty = yt[dy];
        const HT* S = H + (ty.s - OFF - rmin) * TW + lx;                // S[k * TW] = horizontal sum of window row k
        if (sizeof(T) == 1) {
            int r;
            if (NT == 4 && e < (width / 8) * 8) {                       // VResizeCubicVec_32s8u: float, taps * 2^-22, nested from the last row
                const float sc = 1.f / (2048.f * 2048.f);
                float t = __fmul_rn((float)S[3 * TW], __fmul_rn((float)ty.i[3], sc));
                t = __fadd_rn(__fmul_rn((float)S[2 * TW], __fmul_rn((float)ty.i[2], sc)), t);
                t = __fadd_rn(__fmul_rn((float)S[1 * TW], __fmul_rn((float)ty.i[1], sc)), t);
                t = __fadd_rn(__fmul_rn((float)S[0], __fmul_rn((float)ty.i[0], sc)), t);
                r = __float2int_rn(t);
            } else {
                int acc = 0;
#pragma unroll
                for (int k = 0; k < NT; k++) acc += rt8::mul24((int)S[k * TW], (int)ty.i[k]);
                r = (acc + (1 << 21)) >> 22;
            }
            (dst + (size_t)dy * dstep)[e] = (uchar)(r < 0 ? 0 : r > 255 ? 255 : r);
        } else {
            float r;
            if (e < vecBody<T, NT>(width)) {
                r = __fmul_rn((float)S[(NT - 1) * TW], ty.f[NT - 1]);
#pragma unroll
                for (int k = NT - 2; k >= 0; k--) r = __fadd_rn(__fmul_rn((float)S[k * TW], ty.f[k]), r);
            } else {
                r = __fmul_rn((float)S[0], ty.f[0]);
#pragma unroll
                for (int k = 1; k < NT; k++) r = __fadd_rn(r, __fmul_rn((float)S[k * TW], ty.f[k]));
            }
            stE<T>(dst + (size_t)dy * dstep, e, r);
        }
    }
}

// CV_8U cubic / Lanczos on tiles of 256 x 16 elements, four per lane, source bytes staged in LDS (resize_tab8.h; `rows`: the most source rows any tile needs)
template <int NT>
__global__ __launch_bounds__(256) void k_resize_tab8(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, rt8::Geom g,
                                                     const rt8::Tap<NT>* __restrict__ xt, const rt8::Tap<NT>* __restrict__ yt, int rows)
{
    extern __shared__ __attribute__((aligned(16))) uchar ldsRaw[];
    int* H = reinterpret_cast<int*>(ldsRaw);
    uchar* ldsSrc = ldsRaw + (size_t)rows * rt8::TW * 4;
    const rt8::Tile<NT> t = rt8::tileOf<NT>(g, blockIdx.x, blockIdx.y, xt, yt);
    rt8::HTaps<NT> ht; rt8::VTaps<NT> vt;
    rt8::loadTaps<NT>(threadIdx.x, g, t, xt, yt, ht, vt);
    rt8::stage<NT>(threadIdx.x, g, t, src, sstep, ldsSrc);
    __syncthreads();
    rt8::hpass<NT>(threadIdx.x, g, t, ht, ldsSrc, H);
    __syncthreads();
    rt8::vpass<NT>(threadIdx.x, g, t, vt, H, dst, dstep);
}

// INTER_LINEAR_EXACT (resize_bitExact<ET, interpolationLinear<ET>>, resize.cpp:789-950): per-axis tables of (offset, weight of the second tap in
// Q8 for 8U / Q16 for 16U and 16S) built on the host in the reference's arithmetic; horizontal pass exact in Q(shift), vertical pass a two-term dot
// product rounded once.  A weight of 0 means the second tap is not read (left of the image / from the last pixel on: the clamped cases).
struct ExactTap { int ofs; int c1; };
template <typename T, int SHIFT>
__global__ __launch_bounds__(256) void k_resize_exact(const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep, int dw, int dh, int cn,
                                                      const ExactTap* __restrict__ tx, const ExactTap* __restrict__ ty)
{
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (e >= dw * cn || y >= dh) return;
    const int x = e / cn, c = e - x * cn;
    const ExactTap ax = tx[x], ay = ty[y];
    if constexpr (sizeof(T) == 1) {
        // CV_8U, Q8 weights: every term fits 24 bits (255 * 256 * 256 < 2^24), so the two passes are 24-bit multiply-adds at full rate
        // instead of 64-bit products (cv::ORB builds its pyramid with this kernel)
        int H[2] = {0, 0};
#pragma unroll
        for (int r = 0; r < 2; r++) {
            if (r == 1 && ay.c1 == 0) break;
            const uchar* row = src + (size_t)(ay.ofs + r) * sstep;
            const int b0 = rt8::mul24(ax.ofs, cn) + c;
            const int p0 = row[b0], p1 = ax.c1 ? (int)row[b0 + cn] : 0;
            H[r] = rt8::mul24(256 - ax.c1, p0) + rt8::mul24(ax.c1, p1);
        }
        const int v = rt8::mul24(256 - ay.c1, H[0]) + rt8::mul24(ay.c1, H[1]);
        const int r8 = (v + (1 << 15)) >> 16;
        dst[(size_t)y * dstep + e] = (uchar)(r8 > 255 ? 255 : r8);
        return;
    }
    const long long one = 1LL << SHIFT;
    long long H[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r == 1 && ay.c1 == 0) break;
        const T* row = reinterpret_cast<const T*>(src + (size_t)(ay.ofs + r) * sstep);
        const long long p0 = (long long)row[ax.ofs * cn + c];
        const long long p1 = ax.c1 ? (long long)row[(ax.ofs + 1) * cn + c] : 0;
        H[r] = (one - ax.c1) * p0 + (long long)ax.c1 * p1;
    }
    const long long v = (one - ay.c1) * H[0] + (long long)ay.c1 * H[1];
    const long long r = (v + (1LL << (2 * SHIFT - 1))) >> (2 * SHIFT);
    T* D = reinterpret_cast<T*>(dst + (size_t)y * dstep);
    if (sizeof(T) == 1) D[e] = (T)(r < 0 ? 0 : r > 255 ? 255 : r);
    else if (T(-1) > T(0)) D[e] = (T)(r < 0 ? 0 : r > 65535 ? 65535 : r);
    else D[e] = (T)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}

// interpolationLinear<ET>::getCoeffs / getMinMax (resize.cpp:794-826); softdouble there, IEEE double here (same roundings: built with -ffp-contract=off)
void buildExactTaps(double inv_scale, int ssize, int dsize, int shift, std::vector<ExactTap>& t)
{
    t.assign((size_t)dsize, ExactTap{0, 0});
    const double scale = 1.0 / inv_scale;
    int minofst = 0, maxofst = dsize;
    for (int d = 0; d < dsize; d++) {
        const double fval = scale * ((double)d + 0.5) - 0.5;
        const int ival = (int)std::floor(fval);
        if (ival >= 0 && ssize > 1) {
            if (ival < ssize - 1) { t[(size_t)d].ofs = ival; t[(size_t)d].c1 = (int)std::nearbyint((fval - (double)ival) * (double)(1 << shift)); }
            else { t[(size_t)d].ofs = ssize - 1; maxofst = std::min(maxofst, d); }
        } else minofst = std::max(minofst, d + 1);
    }
    for (int d = 0; d < dsize; d++) {
        if (d < minofst) t[(size_t)d] = ExactTap{0, 0};
        else if (d >= maxofst) t[(size_t)d] = ExactTap{ssize - 1, 0};
    }
}

// rows of LDS the tiled kernel needs for the tallest tile, or 0 when that exceeds what it may use
template <class Tab> int tiledRows(const std::vector<Tab>& yt, int nt)
{
    int mx = 0;
    const int dh = (int)yt.size();
    for (int dy0 = 0; dy0 < dh; dy0 += 16) mx = std::max(mx, yt[(size_t)std::min(dy0 + 16, dh) - 1].s - yt[(size_t)dy0].s + nt);
    static const int tiledOn = envInt("MI355CV_RESIZE_TILED", 1);
    return (mx <= 64 && tiledOn) ? mx : 0;
}

// Tap tables depend on (interpolation, destination length, scale) only, and building one costs more host time than the kernel that uses
// it takes (Lanczos: two libm calls and eight divisions per entry, 0.2 ms for a 4K axis): keep the most recent ones resident in HBM.
// An entry stays alive while the cache or a hook that fetched it holds a reference: eviction only drops the cache's, and the last owner frees
// (hipFree waits for the kernels that still read the table), so a table cannot disappear between a fetch and the launch that uses it.
struct DevBlock { void* p; ~DevBlock() { if (p) (void)hipFree(p); } };
typedef std::shared_ptr<DevBlock> DevRef;
DevRef toDevice(const void* host, size_t bytes)
{
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    DevRef mem(new DevBlock{d});
    return hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) == hipSuccess ? mem : nullptr;
}
// the cache: at most `cap` tables, the least recently used one leaves first.  Key is a tuple that starts with the device; build(Info&) makes and uploads the table of a
// key that is not resident (toDevice) and says in Info what else the caller needs to know about it
template <class Key, class Info>
class TabCache {
public:
    explicit TabCache(size_t cap) : cap_(cap) {}
    template <class Build> bool get(const Key& key, Build build, DevRef* keep, Info* info)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = cache_.find(key);
        if (it == cache_.end()) {
            if (cache_.size() >= cap_) {
                auto old = cache_.begin();
                for (auto j = cache_.begin(); j != cache_.end(); ++j) if (j->second.stamp < old->second.stamp) old = j;
                cache_.erase(old);
            }
            Entry e{nullptr, Info(), 0};
            e.mem = build(e.info);
            if (!e.mem) return false;
            it = cache_.emplace(key, e).first;
        }
        it->second.stamp = ++clock_;
        *keep = it->second.mem; *info = it->second.info;
        return true;
    }
private:
    struct Entry { DevRef mem; Info info; unsigned long long stamp; };
    const size_t cap_;
    std::mutex mu_;
    std::map<Key, Entry> cache_;
    unsigned long long clock_ = 0;
};

// the cubic (kind 5) and Lanczos (kind 6) tables, one cache each, with the LDS rows the tiled kernel needs for them
template <class Tab, class Build>
bool cachedTab(int kind, int n, double scale, int nt, Build build, const Tab** dev, int* tileRows, DevRef* keep)
{
    static TabCache<std::tuple<int, int, int, double>, int> cache(32);
    const auto make = [&](int& rows) { std::vector<Tab> host; build(n, scale, host); rows = tiledRows(host, nt); return toDevice(host.data(), host.size() * sizeof(Tab)); };
    if (!cache.get({activeDevice(), kind, n, scale}, make, keep, tileRows)) return false;
    *dev = (const Tab*)(*keep)->p;
    return true;
}

// the same residency for the INTER_AREA tables (taps + per-output offsets in one allocation), keyed by (source length, destination length, scale)
struct AreaDev { const AreaTap* tab; const int* ofs; DevRef keep; };
bool cachedAreaTab(int ssize, int dsize, double scale, AreaDev* out)
{
    static TabCache<std::tuple<int, int, int, double>, size_t> cache(32);
    const auto make = [&](size_t& ofsAt) {
        std::vector<AreaTap> tab; std::vector<int> ofs;
        buildAreaTab(ssize, dsize, scale, tab, ofs);
        ofsAt = (tab.size() * sizeof(AreaTap) + 15) & ~(size_t)15;
        std::vector<uchar> both(ofsAt + ofs.size() * sizeof(int));
        if (!tab.empty()) memcpy(both.data(), tab.data(), tab.size() * sizeof(AreaTap));
        if (!ofs.empty()) memcpy(both.data() + ofsAt, ofs.data(), ofs.size() * sizeof(int));
        return toDevice(both.data(), both.size());
    };
    size_t ofsAt = 0;
    if (!cache.get({activeDevice(), ssize, dsize, scale}, make, &out->keep, &ofsAt)) return false;
    out->tab = (const AreaTap*)out->keep->p; out->ofs = (const int*)((const uchar*)out->keep->p + ofsAt);
    return true;
}

// and for the INTER_LINEAR_EXACT tap tables, keyed by (source length, destination length, fixed-point shift, scale): a caller that resizes the same
// geometry frame after frame (cv::ORB's pyramid: fourteen tables per frame) finds them resident instead of building and uploading them per call
bool cachedExactTab(double inv_scale, int ssize, int dsize, int shift, const ExactTap** dev, DevRef* keep)
{
    static TabCache<std::tuple<int, int, int, int, double>, int> cache(96);
    const auto make = [&](int&) { std::vector<ExactTap> tab; buildExactTaps(inv_scale, ssize, dsize, shift, tab); return toDevice(tab.data(), tab.size() * sizeof(ExactTap)); };
    int unused;
    if (!cache.get({activeDevice(), ssize, dsize, shift, inv_scale}, make, keep, &unused)) return false;
    *dev = (const ExactTap*)(*keep)->p;
    return true;
}


// ---- CV_8U bilinear resize through the lean kernel's LDS pipeline (warp8.h "bilinear resize ... on the lean kernel's machinery") ------------------------------
__global__ __launch_bounds__(256) void k_resize8_terms(warp8::Args a, int* __restrict__ colT, int* __restrict__ rowT)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.dw) { int sx; uint32_t a01; warp8::rzColTerm(a, i, sx, a01); colT[i] = sx; colT[a.dw + i] = (int)a01; }
    if (i < a.dh) { int y0, y1; uint32_t b0, b1; warp8::rzRowTerm(a, i, y0, y1, b0, b1); rowT[i] = y0; rowT[a.dh + i] = y1; rowT[2 * a.dh + i] = (int)b0; rowT[3 * a.dh + i] = (int)b1; }
}

template <int CN, int LW, int NR>
__global__ __launch_bounds__(256) void k_resize8_lean(const uchar* __restrict__ src, uchar* __restrict__ dst, warp8::Args a, int tpw)
{
    extern __shared__ __align__(16) uchar w8lds[];
    src += (size_t)blockIdx.z * a.sframe; dst += (size_t)blockIdx.z * a.dframe;
    const int tid = threadIdx.x, y0 = blockIdx.y * a.th, tx0 = blockIdx.x * tpw, n = min(tpw, a.gx - tx0);
    warp8::RzRowT rt;
    warp8::rzRowTerms<CN>(a, y0, tid, rt);
    uint32_t v[NR];
    auto load = [&](const warp8::LBox& b) {
        if (b.kind == warp8::LEAN_INSIDE) warp8::leanLoad<CN, LW, NR, false>(a, b, src, tid, v);
        else if (b.kind == warp8::LEAN_RIM) warp8::leanLoad<CN, LW, NR, true>(a, b, src, tid, v);
    };
    warp8::LBox b = warp8::rzClassify<CN>(a, tx0 * warp8::TW, y0);
    load(b);
    for (int t = 0; t < n; t++) {                                                        // uniform
        uchar* buf = w8lds + (t & 1) * a.leanBuf;
        const int x0 = (tx0 + t) * warp8::TW;
        if (b.kind != warp8::LEAN_NO) warp8::leanStore<CN, LW, NR>(a, b, buf, tid, v);
        warp8::LBox bn = b; bn.kind = warp8::LEAN_NO;
        if (t + 1 < n) { bn = warp8::rzClassify<CN>(a, x0 + warp8::TW, y0); load(bn); }
        __syncthreads();
        if (b.kind != warp8::LEAN_NO) warp8::rzRows<CN>(a, b, x0, y0, buf, dst, tid, rt);
        b = bn;
    }
}

// One resolved call of cv::resize, as runResize hands it to the paths below: the images where the kernels find them, the geometry, the mode.  Every path is named after
// its kernel and answers NEXT_PATH when the call is not its to serve; runResize tries them in the order they stand here.
struct ResizeCall {
    const char* entry; Stager& stg;
    const uchar* ds; size_t dss; uchar* dd; size_t dds;                            // device pointers and steps
    ResizeArgs a; int depth, cn, e, src_width, src_height, dst_width, dst_height, nframes; double inv_scale_x, inv_scale_y;

    int cubicLanczos()                                                             // k_resize_tab8, k_resize_tiled, k_resize_cubic / k_resize_lanczos
    {
        if (!(a.mode == 5 || a.mode == 6)) return NEXT_PATH;
        dim3 gt(divUp(dst_width * cn, 64), divUp(dst_height, 16)), g1(divUp(dst_width * cn, 64), divUp(dst_height, 4));
        int rows = 0, unused = 0;
        DevRef keepX, keepY;                                        // the tables stay alive until the launches below are enqueued
        // CV_8U: tiles of 256 x 16 elements with the source bytes staged in LDS (resize_tab8.h) where a tile's rows fit.  Measured against the 64 x 16 kernel
        // (profiles/r03_resize_tab8_ab.txt): 1080p -> 4K cubic 8UC3 46.7 against 59.9 us, 8UC1 20.1 / 21.5, Lanczos 68.5 / 66.7, a 1.5 x cubic downscale
        // 53.2 / 52.1 -- so it serves cubic upscales.  MI355CV_RESIZE_TAB8=1: wherever it is eligible, =0: never.
        static const int tab8Env = envInt("MI355CV_RESIZE_TAB8", -1);
        rt8::Geom geom8 = {src_width, src_height, dst_width, dst_height, cn, 0};
        size_t lds8 = 0;
        const dim3 g8(divUp(dst_width * cn, rt8::TW), divUp(dst_height, rt8::TH));
        auto tab8 = [&](int nt) {
            if (tab8Env == 0 || (tab8Env < 0 && !(nt == 4 && a.scale_x <= 1.0 && a.scale_y <= 1.0))) return false;
            geom8.sp = rt8::stagePitch(cn, a.scale_x, nt);
            lds8 = (size_t)rows * ((size_t)rt8::TW * 4 + (size_t)geom8.sp);
            return lds8 <= 48 * 1024;                                 // within what a workgroup gets without asking for more
        };
        if (a.mode == 5) {
            const CubicTap *dxt, *dyt;
            MI355_DECLINE_IF(!cachedTab<CubicTap>(5, dst_width, a.scale_x, 4, buildCubicTab, &dxt, &unused, &keepX) || !cachedTab<CubicTap>(5, dst_height, a.scale_y, 4, buildCubicTab, &dyt, &rows, &keepY));
            const TapT<4>* tx = reinterpret_cast<const TapT<4>*>(dxt); const TapT<4>* ty = reinterpret_cast<const TapT<4>*>(dyt);
#define RZ_TILED(T_, NT_) hipLaunchKernelGGL((k_resize_tiled<T_, NT_>), gt, dim3(256), (size_t)rows * 256, stream(), ds, dss, dd, dds, src_width, src_height, dst_width, dst_height, cn, tx, ty)
#define RZ_BY_DEPTH(M_) do { if (depth == D8U) M_(uchar); else if (depth == D16U) M_(unsigned short); else if (depth == D16S) M_(short); else M_(float); } while (0)
#define RZ_T4(T_) RZ_TILED(T_, 4)
#define RZ_C(T_) hipLaunchKernelGGL(k_resize_cubic<T_>, g1, dim3(256), 0, stream(), ds, dss, dd, dds, src_width, src_height, dst_width, dst_height, cn, dxt, dyt)
            if (rows && depth == D8U && tab8(4)) {
                hipLaunchKernelGGL(k_resize_tab8<4>, g8, dim3(256), lds8, stream(), ds, dss, dd, dds, geom8, tx, ty, rows);
                noteKernel("k_resize_tab8<4> grid=%ux%u x256 lds=%zu", g8.x, g8.y, lds8);
            } else if (rows) { RZ_BY_DEPTH(RZ_T4); noteKernel("k_resize_tiled<depth %d,4> grid=%ux%u x256 lds=%zu", depth, gt.x, gt.y, (size_t)rows * 256); }
            else { RZ_BY_DEPTH(RZ_C); noteKernel("k_resize_cubic<depth %d> grid=%ux%u x256", depth, g1.x, g1.y); }
        } else {
            const LanczosTap *dxt, *dyt;
            MI355_DECLINE_IF(!cachedTab<LanczosTap>(6, dst_width, a.scale_x, 8, buildLanczosTab, &dxt, &unused, &keepX) || !cachedTab<LanczosTap>(6, dst_height, a.scale_y, 8, buildLanczosTab, &dyt, &rows, &keepY));
            const TapT<8>* tx = reinterpret_cast<const TapT<8>*>(dxt); const TapT<8>* ty = reinterpret_cast<const TapT<8>*>(dyt);
#define RZ_T8(T_) RZ_TILED(T_, 8)
#define RZ_L(T_) hipLaunchKernelGGL(k_resize_lanczos<T_>, g1, dim3(256), 0, stream(), ds, dss, dd, dds, src_width, src_height, dst_width, dst_height, cn, dxt, dyt)
            if (rows && depth == D8U && tab8(8)) {
                hipLaunchKernelGGL(k_resize_tab8<8>, g8, dim3(256), lds8, stream(), ds, dss, dd, dds, geom8, tx, ty, rows);
                noteKernel("k_resize_tab8<8> grid=%ux%u x256 lds=%zu", g8.x, g8.y, lds8);
            } else if (rows) { RZ_BY_DEPTH(RZ_T8); noteKernel("k_resize_tiled<depth %d,8> grid=%ux%u x256 lds=%zu", depth, gt.x, gt.y, (size_t)rows * 256); }
            else { RZ_BY_DEPTH(RZ_L); noteKernel("k_resize_lanczos<depth %d> grid=%ux%u x256", depth, g1.x, g1.y); }
#undef RZ_T8
#undef RZ_L
#undef RZ_T4
#undef RZ_C
#undef RZ_BY_DEPTH
#undef RZ_TILED
        }
        return stg.finish(entry);
    }
    int exact()                                                                    // k_resize_exact
    {
        if (!(a.mode == 7)) return NEXT_PATH;
        const int shift = depth == D8U ? 8 : 16;
        const ExactTap *dx, *dy;
        DevRef keepX, keepY;                                        // the tables stay alive until the launch below is enqueued
        MI355_DECLINE_IF(!cachedExactTab(inv_scale_x, src_width, dst_width, shift, &dx, &keepX) || !cachedExactTab(inv_scale_y, src_height, dst_height, shift, &dy, &keepY));
        dim3 g7(divUp(dst_width * cn, 64), divUp(dst_height, 4));
        if (depth == D8U) hipLaunchKernelGGL((k_resize_exact<uchar, 8>), g7, dim3(256), 0, stream(), ds, dss, dd, dds, dst_width, dst_height, cn, dx, dy);
        else if (depth == D16U) hipLaunchKernelGGL((k_resize_exact<unsigned short, 16>), g7, dim3(256), 0, stream(), ds, dss, dd, dds, dst_width, dst_height, cn, dx, dy);
        else hipLaunchKernelGGL((k_resize_exact<short, 16>), g7, dim3(256), 0, stream(), ds, dss, dd, dds, dst_width, dst_height, cn, dx, dy);
        noteKernel("k_resize_exact<depth %d,%d> grid=%ux%u x256", depth, shift, g7.x, g7.y);
        return stg.finish(entry);
    }
    int area2x2u8()                                                                // k_area2x2_u8
    {
        if (!(a.mode == 3 && depth == D8U && a.isx == 2 && a.isy == 2 && (cn == 1 || cn == 3 || cn == 4) && src_width == 2 * dst_width && src_height == 2 * dst_height &&
              ((((uintptr_t)ds) | dss | a.sframe) & 7) == 0 && ((((uintptr_t)dd) | dds | a.dframe) & 3) == 0)) return NEXT_PATH;
        dim3 g3(divUp(divUp(dst_width, 4), 64), divUp(dst_height, 4), nframes);
        if (cn == 1) hipLaunchKernelGGL(k_area2x2_u8<1>, g3, dim3(256), 0, stream(), ds, dss, a.sframe, dd, dds, a.dframe, dst_width, dst_height);
        else if (cn == 3) hipLaunchKernelGGL(k_area2x2_u8<3>, g3, dim3(256), 0, stream(), ds, dss, a.sframe, dd, dds, a.dframe, dst_width, dst_height);
        else hipLaunchKernelGGL(k_area2x2_u8<4>, g3, dim3(256), 0, stream(), ds, dss, a.sframe, dd, dds, a.dframe, dst_width, dst_height);
        noteKernel("k_area2x2_u8<%d> grid=%ux%ux%u x256", cn, g3.x, g3.y, g3.z);
        return stg.finish(entry);
    }
    int area2x2f32()                                                               // k_area2x2_f32
    {
        if (!(a.mode == 3 && depth == D32F && cn == 1 && a.isx == 2 && a.isy == 2 && src_width == 2 * dst_width && src_height == 2 * dst_height &&
              ((((uintptr_t)ds) | dss | a.sframe) & 15) == 0 && ((((uintptr_t)dd) | dds | a.dframe) & 15) == 0)) return NEXT_PATH;
        dim3 g3(divUp(divUp(dst_width, 4), 64), divUp(dst_height, 4), nframes);
        hipLaunchKernelGGL(k_area2x2_f32, g3, dim3(256), 0, stream(), ds, dss, a.sframe, dd, dds, a.dframe, dst_width, dst_height);
        noteKernel("k_area2x2_f32 grid=%ux%ux%u x256", g3.x, g3.y, g3.z);
        return stg.finish(entry);
    }
    int area()                                                                     // k_resize_area
    {
        if (!(a.mode == 4)) return NEXT_PATH;
        AreaDev ax, ay;
        MI355_DECLINE_IF(!cachedAreaTab(src_width, dst_width, a.scale_x, &ax) || !cachedAreaTab(src_height, dst_height, a.scale_y, &ay));
        const AreaTap* dxt = ax.tab; const int* dxo = ax.ofs; const AreaTap* dyt = ay.tab; const int* dyo = ay.ofs;
        dim3 g4(divUp(dst_width * cn, 64), divUp(dst_height, 4));
#define RA(T_) hipLaunchKernelGGL(k_resize_area<T_>, g4, dim3(256), 0, stream(), ds, dss, dd, dds, dst_width, dst_height, cn, depth, dxt, dxo, dyt, dyo)
        switch (depth) { case D8U: RA(uchar); break; case D16U: RA(unsigned short); break; case D16S: RA(short); break; default: RA(float); }
#undef RA
        noteKernel("k_resize_area<depth %d> grid=%ux%u x256", depth, g4.x, g4.y);
        return stg.finish(entry);
    }
    int lean8()                                                                    // k_resize8_lean
    {
        if (!((a.mode == 1 || a.mode == 2) && depth == D8U && (cn == 1 || cn == 3))) return NEXT_PATH;
        // the LDS pipeline of the lean warp kernel (four pixels per lane, dword stores, taps out of a staged tile); the plan bounds every tile's source box from the
        // scale factors, so a planned call has no tile the kernel cannot take.  MI355CV_RESIZE8_LEAN=0 keeps the column-owning kernels (A/B runs)
        static const int rzOn = envInt("MI355CV_RESIZE8_LEAN", 1);
        warp8::Args a8; size_t ldsR = 0;
        if (rzOn && framesOnDwords(a.sframe, a.dframe) && warp8::planResize(a8, cn, src_width, src_height, dst_width, dst_height, dss, dds, ds, dd, a.scale_x, a.inv_x, a.scale_y, a.inv_y, a.mode == 2, &ldsR)) {
            int* tt = (int*)stg.scratch((size_t)(2 * dst_width + 4 * dst_height) * sizeof(int));
            if (tt) {
                a8.sframe = a.sframe; a8.dframe = a.dframe;
                hipLaunchKernelGGL(k_resize8_terms, dim3(divUp(std::max(dst_width, dst_height), 256)), dim3(256), 0, stream(), a8, tt, tt + 2 * dst_width);
                a8.colT = tt; a8.rowT = tt + 2 * dst_width;
                const int tpw = 6;
                dim3 gl(divUp(a8.gx, tpw), a8.gy, nframes);
#define RZN(CN_, LW_, NR_) if (cn == CN_ && a8.leanLW == LW_ && a8.leanNR == NR_) hipLaunchKernelGGL((k_resize8_lean<CN_, LW_, NR_>), gl, dim3(256), ldsR, stream(), ds, dd, a8, tpw)
                WARP8_LEAN_SHAPES(RZN);
#undef RZN
                noteKernel("k_resize8_lean<%d,%d,%d> grid=%ux%ux%u x256 tpw=%d lds=%zu box<=%dx%d", cn, a8.leanLW, a8.leanNR, gl.x, gl.y, gl.z, tpw, ldsR, (a8.ldsPitch - 8) / cn, a8.ldsRows);
                return stg.finish(entry);
            }
        }
        return NEXT_PATH;
    }
    int lin1()                                                                     // k_resize_lin1
    {
        if (!((a.mode == 1 || a.mode == 2) && cn == 1 && (depth == D32F || depth == D8U) && src_width >= 2 && (dss % e) == 0 && ((uintptr_t)ds % e) == 0)) return NEXT_PATH;
        dim3 g2(divUp(dst_width, 64), divUp(dst_height, 4 * RROWS), nframes);
        if (depth == D32F) hipLaunchKernelGGL(k_resize_lin1<float>, g2, dim3(256), 0, stream(), ds, dss, dd, dds, a);
        else hipLaunchKernelGGL(k_resize_lin1<uchar>, g2, dim3(256), 0, stream(), ds, dss, dd, dds, a);
        noteKernel("k_resize_lin1<depth %d> grid=%ux%ux%u x256", depth, g2.x, g2.y, g2.z);
        return stg.finish(entry);
    }
    int linC()                                                                     // k_resize_linC
    {
        if (!((a.mode == 1 || a.mode == 2) && (cn == 3 || cn == 4) && (depth == D32F || depth == D8U) && (dss % e) == 0 && ((uintptr_t)ds % e) == 0)) return NEXT_PATH;
        dim3 g2(divUp(dst_width, 64), divUp(dst_height, 4 * RROWS), nframes);
#define RLC(T_, CN_) hipLaunchKernelGGL((k_resize_linC<T_, CN_>), g2, dim3(256), 0, stream(), ds, dss, dd, dds, a)
        if (depth == D32F) { if (cn == 3) RLC(float, 3); else RLC(float, 4); }
        else { if (cn == 3) RLC(uchar, 3); else RLC(uchar, 4); }
#undef RLC
        noteKernel("k_resize_linC<depth %d,%d> grid=%ux%ux%u x256", depth, cn, g2.x, g2.y, g2.z);
        return stg.finish(entry);
    }
    int generic()                                                                  // k_resize: every other mode, depth and channel count
    {
        dim3 grid(divUp(dst_width, 64), divUp(dst_height, 4), nframes);
        hipLaunchKernelGGL(k_resize, grid, dim3(256), 0, stream(), ds, dss, dd, dds, a);
        noteKernel("k_resize grid=%ux%ux%u x256 mode=%d", grid.x, grid.y, grid.z, a.mode);
        return stg.finish(entry);
    }
};

} // namespace

static int runResize(const char* entry, int src_type, const uchar* src_data, size_t src_step, size_t src_frame, int src_width, int src_height,
                     uchar* dst_data, size_t dst_step, size_t dst_frame, int dst_width, int dst_height, int nframes, double inv_scale_x, double inv_scale_y,
                     int interpolation)
{
    MI355_DECLINE_IF(disabled() || nframes < 1);
    const int depth = MI355CV_MAT_DEPTH(src_type), cn = MI355CV_MAT_CN(src_type);
    MI355_DECLINE_IF(!depthOk(depth) || cn < 1 || cn > 512 || src_width <= 0 || src_height <= 0 || dst_width <= 0 || dst_height <= 0);
    if (inv_scale_x < 2.220446049250313e-16 || inv_scale_y < 2.220446049250313e-16) {        // resize.cpp:3834-3838
        inv_scale_x = (double)dst_width / src_width; inv_scale_y = (double)dst_height / src_height;
    }
    ResizeArgs a; memset(&a, 0, sizeof a);
    a.sw = src_width; a.sh = src_height; a.dw = dst_width; a.dh = dst_height; a.depth = depth; a.cn = cn;
    a.inv_x = inv_scale_x; a.inv_y = inv_scale_y; a.scale_x = 1. / inv_scale_x; a.scale_y = 1. / inv_scale_y;
    a.isx = (int)nearbyint(a.scale_x); a.isy = (int)nearbyint(a.scale_y);
    const bool areaFast = std::fabs(a.scale_x - a.isx) < 2.220446049250313e-16 && std::fabs(a.scale_y - a.isy) < 2.220446049250313e-16;
    if (interpolation == MI355CV_INTER_NEAREST) a.mode = 0;
    else if (interpolation == MI355CV_INTER_NEAREST_EXACT) {
        // resizeNN_bitexact (resize.cpp:1267-1289): source pixel = (ifx * x + ifx0) >> 16 in int arithmetic, steps rounded to 16.16, pixel centres aligned
        MI355_DECLINE_IF(src_width >= 32768 || src_height >= 32768);          // (size << 16) must stay an int, as in the reference
        a.mode = 0; a.nnExact = 1;
        a.ifx = ((src_width << 16) + dst_width / 2) / dst_width; a.ifx0 = a.ifx / 2 - src_width % 2;
        a.ify = ((src_height << 16) + dst_height / 2) / dst_height; a.ify0 = a.ify / 2 - src_height % 2;
    } else {
        if (interpolation == MI355CV_INTER_LINEAR && areaFast && a.isx == 2 && a.isy == 2) interpolation = MI355CV_INTER_AREA;   // :4011
        if (interpolation == MI355CV_INTER_AREA && a.scale_x >= 1 && a.scale_y >= 1) {
            a.mode = areaFast ? 3 : 4;                                                       // 4: true area (resizeArea_)
        } else if (interpolation == MI355CV_INTER_LINEAR) a.mode = 1;
        else if (interpolation == MI355CV_INTER_AREA) a.mode = 2;
        else if (interpolation == MI355CV_INTER_LINEAR_EXACT && (depth == D8U || depth == D16U || depth == D16S)) {
            // resize.cpp:3976-3990: exactly-half sizes are the (bit-exact) 2x2 area mean, except for 2 channels
            if (areaFast && a.isx == 2 && a.isy == 2 && cn != 2) a.mode = 3; else a.mode = 7;
        }
        else if (interpolation == 2 /*INTER_CUBIC*/) a.mode = 5;
        else if (interpolation == 4 /*INTER_LANCZOS4*/) a.mode = 6;
        else return MI355_DECLINED(nullptr);                                                // LINEAR_EXACT on other depths
    }
    if (a.mode == 4 && cn > 4) return MI355_DECLINED("true INTER_AREA of more than 4 channels (the reference asserts on it, resize.cpp:4045)");
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src_data, (size_t)dst_width * dst_height, minPixels(a.mode >= 3 ? HOST_HEAVY : HOST_CHEAP)));
    const int e = eszOf(depth);
    if (nframes > 1) {
        // batches are an HBM-resident construct; nearest / bilinear / area-fast run as ONE launch (grid z = frame), the table-driven modes frame by frame
        if (!isDevicePtr(src_data) || !isDevicePtr(dst_data)) return setError(MI355CV_NOT_IMPLEMENTED, "%s: batch entry needs device-resident frames", entry);
        if (a.mode >= 4) {
            for (int f = 0; f < nframes; f++) {
                const int rc = runResize(entry, src_type, src_data + (size_t)f * src_frame, src_step, 0, src_width, src_height, dst_data + (size_t)f * dst_frame, dst_step, 0,
                                         dst_width, dst_height, 1, inv_scale_x, inv_scale_y, interpolation);
                if (rc != MI355CV_OK) return rc;
            }
            return MI355CV_OK;
        }
        a.sframe = src_frame; a.dframe = dst_frame;
    }
    size_t dss, dds;
    const uchar* ds = stg.in(src_data, src_step, (size_t)src_width * cn * e, src_height, &dss);
    uchar* dd = stg.out(dst_data, dst_step, (size_t)dst_width * cn * e, dst_height, &dds);
    MI355_DECLINE_IF(!ds || !dd);
    ResizeCall c = {entry, stg, ds, dss, dd, dds, a, depth, cn, e, src_width, src_height, dst_width, dst_height, nframes, inv_scale_x, inv_scale_y};
    // the dispatch rule: the first path that takes the call serves it
    static int (ResizeCall::* const paths[])() = {&ResizeCall::cubicLanczos, &ResizeCall::exact, &ResizeCall::area2x2u8, &ResizeCall::area2x2f32, &ResizeCall::area,
                                                  &ResizeCall::lean8, &ResizeCall::lin1, &ResizeCall::linC};
    for (auto path : paths) { const int rc = (c.*path)(); if (rc != NEXT_PATH) return rc; }
    return c.generic();
}

extern "C" {

MI355CV_API int mi355cv_resize(int src_type, const uchar* src_data, size_t src_step, int src_width, int src_height,
        uchar* dst_data, size_t dst_step, int dst_width, int dst_height, double inv_scale_x, double inv_scale_y, int interpolation)
{
    mi355::EntryGuard entry_(__func__);
    return runResize("resize", src_type, src_data, src_step, 0, src_width, src_height, dst_data, dst_step, 0, dst_width, dst_height, 1, inv_scale_x, inv_scale_y, interpolation);
}

// batches of device-resident frames (frames are the unit that shards): every frame through the same transform, one launch where
// the kernel takes a frame index (nearest / bilinear / area-fast resize, every warp), frame strides in bytes
MI355CV_API int mi355cv_resizeBatch(int src_type, const uchar* src_data, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
        uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes, double inv_scale_x, double inv_scale_y, int interpolation)
{
    mi355::EntryGuard entry_(__func__);
    if (src_width > 0 && src_height > 0 && dst_width > 0 && dst_height > 0 && hostBatchEligible(src_data, dst_data, nframes)) {        // frames in host memory
        const size_t pix = (size_t)MI355CV_MAT_CN(src_type) * depthBytes(MI355CV_MAT_DEPTH(src_type));
        const HostBatch hb = {src_data, src_step, src_frame_stride, pix * src_width, src_height, dst_data, dst_step, dst_frame_stride, pix * dst_width, dst_height, nframes};
        return runHostBatch("resizeBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_resizeBatch(src_type, s, ss, sf, src_width, src_height, d, ds, df, dst_width, dst_height, nf, inv_scale_x, inv_scale_y, interpolation); });
    }
    if (nframes > MAX_GRID_FRAMES)                                                                                                      // the kernels take the frame from blockIdx.z
        return sliceFrames(nframes, [&](size_t f0, int nf) {
            return mi355cv_resizeBatch(src_type, src_data + f0 * src_frame_stride, src_step, src_frame_stride, src_width, src_height, dst_data + f0 * dst_frame_stride, dst_step,
                                       dst_frame_stride, dst_width, dst_height, nf, inv_scale_x, inv_scale_y, interpolation); });
    return runResize("resizeBatch", src_type, src_data, src_step, src_frame_stride, src_width, src_height, dst_data, dst_step, dst_frame_stride, dst_width, dst_height,
                     nframes, inv_scale_x, inv_scale_y, interpolation);
}

} // extern "C"
