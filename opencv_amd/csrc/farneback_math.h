// farneback_math.h -- the arithmetic of cv::calcOpticalFlowFarneback (video/src/optflowgf.cpp; no HAL hook) as the project restates it (tests/farneback_restate.py), for the
// kernels of farneback.hip and, compiled by g++ with -ffp-contract=off, for tests/hostemu/farneback_emu.cpp.  All image arithmetic is float32, one rounding per operation,
// every sum in a fixed order that no tiling changes; the taps and the four inverse-moment constants are prepared on the host in double and rounded to float once.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hd.h"

namespace fb {

constexpr int MAX_DIM = 16384;          // mi355cv_limit("farneback_max_dim"): 32-bit element offsets into a plane of five floats per pixel are formed in size_t
constexpr int MAX_WINSIZE = 25;         // ("farneback_max_winsize"): the M tile with its halo and the vertical sums of k_fb_update_flow fit 64 KiB of LDS
constexpr int MAX_POLY_N = 7;           // ("farneback_max_poly_n"): the taps travel in the kernel arguments, the tiles of k_fb_polyexp are sized for it
constexpr int MAX_SMOOTH_TAPS = 255;    // ("farneback_max_smooth_taps"): the level Gaussian, max(cvRound(5 sigma) | 1, 3) taps; a level that needs more is declined
constexpr int MAX_LEVELS = 32;
constexpr int BORDER = 5;
constexpr int MIN_SIZE = 32;
constexpr int USE_INITIAL_FLOW = 4, FARNEBACK_GAUSSIAN = 256;

struct PolyTaps {
    float g[MAX_POLY_N + 1], xg[MAX_POLY_N + 1], xxg[MAX_POLY_N + 1];
    float ig11, ig03, ig33, ig55;
    int n;
};

struct WinTaps {                         // the window of the flow update: 2 m + 1 taps (ones for the box window) and the factor applied to the five sums
    float t[MAX_WINSIZE];
    float scale;
    int m;
};

MI355_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

MI355_HD int reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * (len - 1) - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

// ---- bilinear resize: source coordinate (float)((d + 0.5) * scale - 0.5) with scale = src / dst in double, floor, zero fraction where it clamps
MI355_HD void resizeCoord(int d, double scale, int srcLen, int& i0, int& i1, float& f)
{
    const float c = (float)((d + 0.5) * scale - 0.5);
    const float fl = floorf(c);
    int s = (int)fl;
    f = c - fl;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= srcLen - 1) { s = srcLen - 1; f = 0.f; }
    i0 = s;
    i1 = s + 1 < srcLen ? s + 1 : srcLen - 1;
}
MI355_HD float lerp(float a, float b, float f) { return a * (1.f - f) + b * f; }

// ---- polynomial expansion.  col(k): the source at row offset k (replicated rows); three sums in the order centre, k = 1 .. n
template <typename Col>
MI355_HD void polyVertical(const PolyTaps& T, Col col, float (&v)[3])
{
    v[0] = col(0) * T.g[0]; v[1] = 0.f; v[2] = 0.f;
    for (int k = 1; k <= T.n; k++) {
        const float up = col(-k), dn = col(k);
        const float p = up + dn;
        v[0] = v[0] + T.g[k] * p;
        v[1] = v[1] + T.xg[k] * (dn - up);
        v[2] = v[2] + T.xxg[k] * p;
    }
}
// row(k, c): vertical sum c at column offset k (replicated columns); the five channels: y-linear, x-linear, yy, xx, xy
template <typename Row>
MI355_HD void polyHorizontal(const PolyTaps& T, Row row, float (&r)[5])
{
    const float g0 = T.g[0];
    float b1 = row(0, 0) * g0, b2 = 0.f, b3 = row(0, 1) * g0, b4 = 0.f, b5 = row(0, 2) * g0, b6 = 0.f;
    for (int k = 1; k <= T.n; k++) {
        const float l0 = row(-k, 0), r0 = row(k, 0), l1 = row(-k, 1), r1 = row(k, 1), l2 = row(-k, 2), r2 = row(k, 2);
        const float tg = r0 + l0;
        b1 = b1 + tg * T.g[k];
        b4 = b4 + tg * T.xxg[k];
        b2 = b2 + (r0 - l0) * T.xg[k];
        b3 = b3 + (r1 + l1) * T.g[k];
        b6 = b6 + (r1 - l1) * T.xg[k];
        b5 = b5 + (r2 + l2) * T.g[k];
    }
    r[0] = b3 * T.ig11;
    r[1] = b2 * T.ig11;
    r[2] = b1 * T.ig03 + b5 * T.ig33;
    r[3] = b1 * T.ig03 + b4 * T.ig33;
    r[4] = b6 * T.ig55;
}

// ---- update matrices
MI355_HD float borderWeight1(int p, int len)
{
    const float B[BORDER] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    const float a = p < BORDER ? B[p] : 1.f;
    const float b = p >= len - BORDER ? B[len - p - 1] : 1.f;
    return a * b;
}
MI355_HD float borderWeight(int x, int y, int w, int h) { return borderWeight1(x, w) * borderWeight1(y, h); }

// r0: the five floats of R0 at (x, y); R1: the second expansion, `pitch1` floats per row; d: the flow at (x, y); M: five floats out
MI355_HD void updateMatrix(const float* r0, const float* R1, size_t pitch1, int x, int y, int w, int h, float dx, float dy, float (&M)[5])
{
    const float fx = (float)x + dx, fy = (float)y + dy;
    const float x1f = floorf(fx), y1f = floorf(fy);
    float r2, r3, r4, r5, r6;
    if (x1f >= 0.f && x1f < (float)(w - 1) && y1f >= 0.f && y1f < (float)(h - 1)) {
        const float ax = fx - x1f, ay = fy - y1f;
        const float a00 = (1.f - ax) * (1.f - ay), a01 = ax * (1.f - ay), a10 = (1.f - ax) * ay, a11 = ax * ay;
        const float* p = R1 + (size_t)(int)y1f * pitch1 + (size_t)(int)x1f * 5;
        const float* q = p + pitch1;
        r2 = a00 * p[0] + a01 * p[5] + a10 * q[0] + a11 * q[5];
        r3 = a00 * p[1] + a01 * p[6] + a10 * q[1] + a11 * q[6];
        r4 = a00 * p[2] + a01 * p[7] + a10 * q[2] + a11 * q[7];
        r5 = a00 * p[3] + a01 * p[8] + a10 * q[3] + a11 * q[8];
        r6 = a00 * p[4] + a01 * p[9] + a10 * q[4] + a11 * q[9];
        r4 = (r0[2] + r4) * 0.5f;
        r5 = (r0[3] + r5) * 0.5f;
        r6 = (r0[4] + r6) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = r0[2];
        r5 = r0[3];
        r6 = r0[4] * 0.5f;
    }
    r2 = (r0[0] - r2) * 0.5f;
    r3 = (r0[1] - r3) * 0.5f;
    r2 = r2 + (r4 * dy + r6 * dx);
    r3 = r3 + (r6 * dy + r5 * dx);
    const float s = borderWeight(x, y, w, h);
    r2 = r2 * s; r3 = r3 * s; r4 = r4 * s; r5 = r5 * s; r6 = r6 * s;
    M[0] = r4 * r4 + r6 * r6;
    M[1] = (r4 + r5) * r6;
    M[2] = r5 * r5 + r6 * r6;
    M[3] = r4 * r2 + r6 * r3;
    M[4] = r6 * r2 + r5 * r3;
}

// ---- update flow.  at(i): the i-th value under the window; taps in ascending order
template <typename At>
MI355_HD float tapSum(const float* t, int n, At at)
{
    float s = t[0] * at(0);
    for (int i = 1; i < n; i++) s = s + t[i] * at(i);
    return s;
}
MI355_HD void solveFlow(const float (&s)[5], float scale, float& fx, float& fy)
{
    const float g11 = s[0] * scale, g12 = s[1] * scale, g22 = s[2] * scale, h1 = s[3] * scale, h2 = s[4] * scale;
    const float idet = 1.f / (g11 * g22 - g12 * g12 + 1e-3f);
    fx = (g11 * h2 - g12 * h1) * idet;
    fy = (g22 * h1 - g12 * h2) * idet;
}

// ------------------------------------------------------------------ host side: taps, constants and the level plan, all in double
inline long roundHalfEven(double v) { return lrint(v); }             // cvRound (the default rounding mode)

// getGaussianKernel's rule: the fixed tables for sigma <= 0 and up to 7 taps, else exp(-x^2 / 2 sigma^2) normalised, sigma <= 0 meaning 0.3 ((n - 1) / 2 - 1) + 0.8
inline void gaussianTaps(int n, double sigma, float* out)
{
    static const float tab[4][7] = {{1.f}, {0.25f, 0.5f, 0.25f}, {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}, {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    if (sigma <= 0 && (n & 1) && n <= 7) { for (int i = 0; i < n; i++) out[i] = tab[n >> 1][i]; return; }
    const double sg = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2 = -0.5 / (sg * sg);
    double sum = 0;
    for (int i = 0; i < n; i++) { const double x = i - (n - 1) * 0.5; sum += exp(scale2 * x * x); }
    const double inv = 1. / sum;
    for (int i = 0; i < n; i++) { const double x = i - (n - 1) * 0.5; out[i] = (float)(exp(scale2 * x * x) * inv); }
}

inline void polySetup(int n, double sigma, PolyTaps& T)
{
    if (sigma < 1.1920928955078125e-7) sigma = n * 0.3;               // FLT_EPSILON
    float g[2 * MAX_POLY_N + 1];
    double s = 0;
    for (int x = -n; x <= n; x++) { g[x + n] = (float)exp(-x * x / (2 * sigma * sigma)); s += g[x + n]; }
    s = 1. / s;
    for (int x = -n; x <= n; x++) g[x + n] = (float)(g[x + n] * s);
    T = PolyTaps{};
    T.n = n;
    for (int k = 0; k <= n; k++) { T.g[k] = g[k + n]; T.xg[k] = (float)(k * (double)g[k + n]); T.xxg[k] = (float)(k * k * (double)g[k + n]); }
    // the moments of g (x) g over the basis (1, x, y, x^2, y^2, xy): a = G00, b = G11 = G22 = G03 = G04, c = G33 = G44, d = G55 = G34; the inverse in closed form
    double a = 0, b = 0, c = 0, d = 0;
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            const double gg = (double)g[y + n] * (double)g[x + n];
            a += gg; b += gg * (x * x); c += gg * (x * x * x * x); d += gg * (x * x * y * y);
        }
    const double D = a * (c + d) - 2 * b * b;
    T.ig11 = (float)(1. / b);
    T.ig03 = (float)(-b / D);
    T.ig33 = (float)((a * c - b * b) / ((c - d) * D));
    T.ig55 = (float)(1. / d);
}

inline void winSetup(int winsize, bool gaussian, WinTaps& W)
{
    const int m = winsize / 2;
    W = WinTaps{};
    W.m = m;
    if (gaussian) { gaussianTaps(2 * m + 1, 0.3 * m, W.t); W.scale = 1.f; }
    else { for (int i = 0; i <= 2 * m; i++) W.t[i] = 1.f; W.scale = (float)(1. / ((2 * m + 1) * (2 * m + 1))); }
}

struct Level { double scale; int w, h, ksize; double sigma; };
// levels k = 0 .. count - 1 with scale = pyr_scale^k, cut at the first k >= 1 whose scaled width or height falls below 32
inline int levelPlan(int w, int h, double pyrScale, int levels, Level* out)
{
    int n = 0;
    for (int k = 0; k < levels && k < MAX_LEVELS; k++) {
        double scale = 1;
        for (int i = 0; i < k; i++) scale *= pyrScale;
        if (k > 0 && (w * scale < MIN_SIZE || h * scale < MIN_SIZE)) break;
        Level& L = out[n++];
        L.scale = scale;
        L.sigma = (1. / scale - 1) * 0.5;
        const long ks = roundHalfEven(L.sigma * 5) | 1;
        L.ksize = (int)(ks > 3 ? (ks > (1 << 20) ? (1 << 20) + 1 : ks) : 3);
        L.w = (int)roundHalfEven(w * scale);
        L.h = (int)roundHalfEven(h * scale);
    }
    return n;
}

} // namespace fb
