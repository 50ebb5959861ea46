// imgwarp_common.h -- what resize.hip (cv::resize) and warp.hip (warpAffine / warpPerspective / remap / convertMaps / warpPolar) both use: the depth codes, the
// reference's rounding and saturation helpers, the per-depth element load / store of the generic kernels, and the frame rule of their dispatchers (NEXT_PATH, their other convention, is rt.h's).
#pragma once
#include "rt.h"

namespace {

enum { D8U = MI355CV_8U, D16U = MI355CV_16U, D16S = MI355CV_16S, D32F = MI355CV_32F };
__host__ __device__ inline int eszOf(int d) { return d == D8U ? 1 : d == D32F ? 4 : 2; }

__device__ __forceinline__ int cvFloorD(double v) { int i = (int)v; return i - (i > v); }
__device__ __forceinline__ int cvFloorF(float v) { int i = (int)v; return i - (i > v); }
__device__ __forceinline__ int satIntD(double v) { return v >= 2147483647.0 ? 2147483647 : v <= -2147483648.0 ? (int)-2147483648LL : (int)__double2int_rn(v); }
__device__ __forceinline__ int satShort(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }
__device__ __forceinline__ int clipI(int x, int a, int b) { return x >= a ? (x < b ? x : b - 1) : a; }

__device__ __forceinline__ float ldV(const uchar* p, int depth, int idx)
{
    switch (depth) { case D8U: return (float)p[idx]; case D16U: return (float)reinterpret_cast<const unsigned short*>(p)[idx];
                     case D16S: return (float)reinterpret_cast<const short*>(p)[idx]; default: return reinterpret_cast<const float*>(p)[idx]; }
}
__device__ __forceinline__ void stRound(uchar* p, int depth, int idx, float v)
{
    const float r = rintf(v);
    switch (depth) {
    case D8U:  p[idx] = (uchar)(int)fminf(fmaxf(r, 0.f), 255.f); break;
    case D16U: reinterpret_cast<unsigned short*>(p)[idx] = (unsigned short)(int)fminf(fmaxf(r, 0.f), 65535.f); break;
    case D16S: reinterpret_cast<short*>(p)[idx] = (short)(int)fminf(fmaxf(r, -32768.f), 32767.f); break;
    default:   reinterpret_cast<float*>(p)[idx] = v;
    }
}
__device__ __forceinline__ void copyPix(uchar* d, const uchar* s, int bytes) { for (int i = 0; i < bytes; i++) d[i] = s[i]; }

inline bool depthOk(int d) { return d == D8U || d == D16U || d == D16S || d == D32F; }
// the LDS kernels of warp8.h move whole dwords: every frame of a batch starts on a dword (their plans judge pointers and steps; the frames start at multiples of the strides)
inline bool framesOnDwords(size_t sframe, size_t dframe) { return ((sframe | dframe) & 3) == 0; }

} // namespace
