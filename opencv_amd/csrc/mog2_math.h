// mog2_math.h -- the arithmetic of mog2.hip (cv::BackgroundSubtractorMOG2) that can be wrong, __host__ __device__ so that the CPU suite compiles the very same lines
// (tests/hostemu/mog2_emu.cpp) and holds them against the restatement (tests/mog2_restate.py): the per-pixel update of the mixture, the shadow test and the
// background mean.  Every product, sum and quotient is rounded on its own (-ffp-contract=off), `/` is the correctly rounded division, evaluation is left to right.
//
// A pixel's model lives in a Pixel<CN>: up to MAX_MIXTURES modes {weight, variance, mean[CN]} sorted by descending weight.  Every loop over the modes is unrolled to
// MAX_MIXTURES and predicated on the live count, so that all indices are compile-time constants and the arrays stay in registers on the GPU.
#pragma once
#include <math.h>
#include <float.h>
#include "hd.h"

namespace mog2 {

constexpr int MAX_DIM = 16384;       // width and height: a frame has at most 2^28 pixels, a pixel index and a plane offset in floats stay below 2^31
constexpr int MAX_MIXTURES = 5;      // modes held in registers per pixel (the reference's default)

struct Params {
    float Tb, TB, Tg, varInit, varMin, varMax, CT, tau;
    int nmixtures, detectShadows, shadowValue;
};

template <int CN>
struct Pixel {
    float w[MAX_MIXTURES], var[MAX_MIXTURES], mean[MAX_MIXTURES][CN];
    int nmodes;
};

template <int CN>
MI355_HD_PLAIN void clear(Pixel<CN>& p)
{
#pragma unroll
    for (int m = 0; m < MAX_MIXTURES; m++) {
        p.w[m] = 0.f; p.var[m] = 0.f;
#pragma unroll
        for (int c = 0; c < CN; c++) p.mean[m][c] = 0.f;
    }
    p.nmodes = 0;
}

// modes a and b change places (a, b compile-time constants at every call site)
template <int CN>
MI355_HD_PLAIN void swapModes(Pixel<CN>& p, int a, int b)
{
    float t = p.w[a]; p.w[a] = p.w[b]; p.w[b] = t;
    t = p.var[a]; p.var[a] = p.var[b]; p.var[b] = t;
#pragma unroll
    for (int c = 0; c < CN; c++) { t = p.mean[a][c]; p.mean[a][c] = p.mean[b][c]; p.mean[b][c] = t; }
}

// One frame's value x into the model; true when the pixel is background.
// The reference writes the updated weight to weight[mode - swaps] after the bubble; here the value is stored in slot `mode` BEFORE the bubble and travels with the
// swaps (the comparisons of the bubble only look at slots below the travelling one), which needs no computed index.
template <int CN>
MI355_HD_PLAIN bool update(Pixel<CN>& p, const float (&x)[CN], const Params& P, float alphaT)
{
    const float alpha1 = 1.f - alphaT, prune = -alphaT * P.CT;
    bool background = false, fits = false;
    float total = 0.f;
    int nmodes = p.nmodes;
#pragma unroll
    for (int mode = 0; mode < MAX_MIXTURES; mode++) {
        if (mode < nmodes) {                                  // the LIVE count: a prune below shortens the loop
            float w = alpha1 * p.w[mode] + prune;
            bool fitHere = false;
            if (!fits) {
                const float var = p.var[mode];
                float d[CN], dist2 = 0.f;
#pragma unroll
                for (int c = 0; c < CN; c++) { d[c] = p.mean[mode][c] - x[c]; dist2 = dist2 + d[c] * d[c]; }
                if (total < P.TB && dist2 < P.Tb * var) background = true;
                if (dist2 < P.Tg * var) {
                    fits = true; fitHere = true;
                    w += alphaT;
                    const float k = alphaT / w;
#pragma unroll
                    for (int c = 0; c < CN; c++) p.mean[mode][c] -= k * d[c];
                    float v = var + k * (dist2 - var);
                    v = v > P.varMin ? v : P.varMin;
                    v = v < P.varMax ? v : P.varMax;
                    p.var[mode] = v;
                }
            }
            const bool pruned = w < -prune;
            p.w[mode] = pruned ? 0.f : w;
            if (fitHere) {
                bool stop = false;
#pragma unroll
                for (int i = mode; i > 0; i--) {
                    if (!stop) {
                        if (w < p.w[i - 1]) stop = true;
                        else swapModes(p, i, i - 1);
                    }
                }
            }
            if (pruned) { w = 0.f; nmodes--; }
            total += w;
        }
    }
    const float inv = fabsf(total) > FLT_EPSILON ? 1.f / total : 0.f;
#pragma unroll
    for (int m = 0; m < MAX_MIXTURES; m++) if (m < nmodes) p.w[m] *= inv;
    if (!fits && alphaT > 0.f) {
        int mode;
        if (nmodes == P.nmixtures) mode = P.nmixtures - 1; else mode = nmodes++;
#pragma unroll
        for (int m = 0; m < MAX_MIXTURES; m++) {
            if (m == mode) {
                p.w[m] = nmodes == 1 ? 1.f : alphaT;
                p.var[m] = P.varInit;
#pragma unroll
                for (int c = 0; c < CN; c++) p.mean[m][c] = x[c];
            } else if (nmodes != 1 && m < nmodes - 1) p.w[m] *= alpha1;
        }
        bool stop = false;
#pragma unroll
        for (int i = MAX_MIXTURES - 1; i > 0; i--) {
            if (i <= nmodes - 1 && !stop) {
                if (alphaT < p.w[i - 1]) stop = true;
                else swapModes(p, i - 1, i);
            }
        }
    }
    p.nmodes = nmodes;
    return background;
}

// detectShadowGMM on the updated model
template <int CN>
MI355_HD_PLAIN bool shadow(const Pixel<CN>& p, const float (&x)[CN], const Params& P)
{
    float t = 0.f;
    bool done = false, res = false;
#pragma unroll
    for (int m = 0; m < MAX_MIXTURES; m++) {
        if (m < p.nmodes && !done) {
            float num = 0.f, den = 0.f;
#pragma unroll
            for (int c = 0; c < CN; c++) { num = num + x[c] * p.mean[m][c]; den = den + p.mean[m][c] * p.mean[m][c]; }
            if (den == 0.f) done = true;
            else {
                if (num <= den && num >= P.tau * den) {
                    const float a = num / den;
                    float dist2a = 0.f;
#pragma unroll
                    for (int c = 0; c < CN; c++) { const float dd = a * p.mean[m][c] - x[c]; dist2a = dist2a + dd * dd; }
                    if (dist2a < P.Tb * p.var[m] * a * a) { res = true; done = true; }
                }
                if (!done) { t += p.w[m]; if (t > P.TB) done = true; }
            }
        }
    }
    return res;
}

// the mask value of a pixel after update()
template <int CN>
MI355_HD_PLAIN unsigned maskValue(bool background, const Pixel<CN>& p, const float (&x)[CN], const Params& P)
{
    if (background) return 0u;
    return (P.detectShadows && shadow(p, x, P)) ? (unsigned)P.shadowValue : 255u;
}

// getBackgroundImage_intern: the weighted mean of the modes up to the one that carries the sum of weights past TB
template <int CN>
MI355_HD_PLAIN void backgroundMean(const Pixel<CN>& p, const Params& P, float (&out)[CN])
{
    float m[CN], t = 0.f;
#pragma unroll
    for (int c = 0; c < CN; c++) m[c] = 0.f;
    bool done = false;
#pragma unroll
    for (int k = 0; k < MAX_MIXTURES; k++) {
        if (k < p.nmodes && !done) {
#pragma unroll
            for (int c = 0; c < CN; c++) m[c] += p.w[k] * p.mean[k][c];
            t += p.w[k];
            if (t > P.TB) done = true;
        }
    }
    const float inv = fabsf(t) > FLT_EPSILON ? 1.f / t : 0.f;
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = m[c] * inv;
}

// CV_8U result: round to nearest even, saturate
MI355_HD_PLAIN unsigned roundSat8(float v)
{
    const float r = rintf(v);
    return r <= 0.f ? 0u : r >= 255.f ? 255u : (unsigned)r;
}

} // namespace mog2
