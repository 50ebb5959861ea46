// calchist_math.h -- the arithmetic of calchist.hip (cv::calcHist, cv::calcBackProject) that can be wrong, __host__ __device__ so that the CPU suite compiles the very
// same lines (tests/hostemu/calchist_emu.cpp): the bin rule of uniform and non-uniform ranges, the per-dimension tables the 8- and 16-bit kernels walk, the rounding
// of a back-projected value and the float <-> int32 conversions of `accumulate`.  The definition is tests/calchist_restate.py.
//
//   uniform      a = n / ((double)hi - (double)lo), b = -a * lo, t = v * a + b with the product and the sum rounded SEPARATELY (mulThenAdd: __dmul_rn / __dadd_rn on
//                the device, a volatile intermediate on the host -- a fused multiply-add is another function).  CV_8U / CV_16U: counted iff lo <= v < hi, bin =
//                min(max(floor(t), 0), n - 1).  CV_32F: counted iff 0 <= t < n (NaN and +-inf fail the comparison), bin = floor(t).
//   non-uniform  n + 1 strictly ascending boundaries r: the bin is the k with r[k] <= v < r[k + 1]; outside [r[0], r[n]) not counted.  CV_8U / CV_16U only.
//   table        one int32 per value of the depth (256 or 65536) and dimension: bin * mult, mult the row-major multiplier of the dimension, or SKIP.  SKIP is so
//                negative that a sum of up to three entries of which one is SKIP stays negative: "counted" is one sign test on the summed cell offset.
//   cvRound      round to nearest, ties to even (rint under the default rounding mode; v_rndne_f64 on the device), then saturated.
#pragma once
#include <math.h>
#include <stdint.h>
#include "hd.h"

namespace calchist {

constexpr int MAX_DIM = 16384;                 // width and height
constexpr int MAX_BINS = 1 << 20;              // the cells of a histogram, the product of its sizes
constexpr int MAX_BINS_PER_DIM = 65536;
constexpr int MAX_DIMS = 3;
constexpr int MAX_FRAMES = 65535;
constexpr int32_t SKIP = -(1 << 28);           // 3 * SKIP > INT32_MIN and SKIP + 2 * MAX_BINS < 0

// v * a + b, two roundings
MI355_HD_PLAIN double mulThenAdd(double v, double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(__dmul_rn(v, a), b);
#else
    volatile double p = v * a;
    return p + b;
#endif
}

struct Uniform { double a, b; };
MI355_HD_PLAIN Uniform uniformCoef(int n, float lo, float hi)
{
    Uniform u;
    u.a = (double)n / ((double)hi - (double)lo);
    u.b = -u.a * (double)lo;
    return u;
}

// the bin of an 8- or 16-bit value under uniform ranges, -1: not counted
MI355_HD_PLAIN int binUniformInt(int v, int n, float lo, float hi, Uniform u)
{
    if (!((double)v >= (double)lo && (double)v < (double)hi)) return -1;
    const double f = floor(mulThenAdd((double)v, u.a, u.b));
    return f < 0.0 ? 0 : f > (double)(n - 1) ? n - 1 : (int)f;
}

// the bin of a CV_32F value under uniform ranges, -1: not counted
MI355_HD_PLAIN int binUniformF32(float v, int n, Uniform u)
{
    const double t = mulThenAdd((double)v, u.a, u.b);
    if (!(t >= 0.0 && t < (double)n)) return -1;
    return (int)floor(t);
}

// the k with r[k] <= v < r[k + 1] among n + 1 ascending boundaries, -1 outside [r[0], r[n]); v is exact as a float (8- and 16-bit values)
MI355_HD_PLAIN int binNonUniform(float v, const float* r, int n)
{
    if (!(v >= r[0] && v < r[n])) return -1;
    int lo = 0, hi = n;                        // r[lo] <= v < r[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= r[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

// the table of one dimension: tab[v] = bin(v) * mult or SKIP, v < levels (256 / 65536).  ranges: {lo, hi} when uniform, else the n + 1 boundaries
inline void buildTable(int levels, int n, bool uniform, const float* ranges, int mult, int32_t* tab)
{
    const Uniform u = uniform ? uniformCoef(n, ranges[0], ranges[1]) : Uniform{0, 0};
    for (int v = 0; v < levels; v++) {
        const int bin = uniform ? binUniformInt(v, n, ranges[0], ranges[1], u) : binNonUniform((float)v, ranges, n);
        tab[v] = bin < 0 ? SKIP : bin * mult;
    }
}

// cvRound(p) saturated to [0, top] (top = 255 / 65535); NaN -> 0
MI355_HD_PLAIN uint32_t roundSat(double p, uint32_t top)
{
    const double r = rint(p);
    return !(r > 0.0) ? 0u : r >= (double)top ? top : (uint32_t)r;
}

// accumulate: a CV_32F cell as the starting count, cvRound saturated to int32; NaN -> 0
MI355_HD_PLAIN int32_t countOfFloat(float f)
{
    const double r = rint((double)f);
    return r != r ? 0 : r <= -2147483648.0 ? INT32_MIN : r >= 2147483647.0 ? INT32_MAX : (int32_t)r;
}
// ... and a count as a CV_32F cell: round to nearest even
MI355_HD_PLAIN float floatOfCount(int32_t c) { return (float)c; }

// one back-projected value: hist[bin] * scale in double, then the destination's rounding
MI355_HD_PLAIN uint32_t backProjectInt(float h, double scale, uint32_t top) { return roundSat((double)h * scale, top); }
MI355_HD_PLAIN float backProjectF32(float h, double scale) { return (float)((double)h * scale); }

} // namespace calchist
