// stereobm_math.h -- the per-pixel pieces of stereobm.hip (cv::StereoBM) that can be wrong, __host__ __device__ so that the CPU suite compiles the very same lines
// (tests/hostemu/stereobm_emu.cpp) and holds them against tests/stereobm_restate.py bit for bit.  The definition is the project's restatement.
//
//   prefilter    XSOBEL: P = clip(c + g(y-1) + 2 g(y) + g(y+1), 0, 2c), g(r) = I[r'][x+1] - I[r'][x-1], r' under BORDER_REFLECT_101; the two border columns are c.
//   geometry     Dmax = m + n - 1; pixel X is computed iff xlo <= X < xhi; the left column of a window is clamped to [0, W-1], the right one to [rlo, rhi] BEFORE the
//                disparity is subtracted, so the right column read is always inside the image.
//   decision     texture reject, the smallest index i = Dmax - D with the smallest SAD, the uniqueness reject, the sub-pixel quotient (C division), (.. + 15) >> 4.
//                The pieces (minKey, outsideCost, uniqRejects, subpixel) are what the fast kernel runs in parallel over a pixel's disparities; decide() is their serial
//                composition, used by the generic kernel and by the host.
//   left-right   one 64-bit key (cost, x, d) per target column x2, the smallest wins: independent of execution order.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "hd.h"

namespace sbm {

enum { PREFILTER_NORMALIZED_RESPONSE = 0, PREFILTER_XSOBEL = 1 };
constexpr int DISP_SHIFT = 4, DISP_SCALE = 16;

constexpr int MAX_DISPARITIES = 256;      // mi355cv_limit("stereobm_max_disparities"): a workgroup of the fast kernel is 64 lanes x n / 16 waves <= 1024 lanes
constexpr int MAX_BLOCK = 51;             // ("stereobm_max_block"): the generic kernel's tiles of w rows fit 64 KiB of LDS at n = 256; a SAD stays below 2^19
constexpr int MAX_DIM = 16384;            // ("stereobm_max_dim"): a column fits the 14 bits the left-right key gives it
constexpr int ROLL_MAX_BLOCK = 21;        // ("stereobm_roll_max_block"): the fast kernel keeps SADs in 16 bits: 21 * 21 * 126 = 55 566
constexpr int ROLL_CHUNK = 16;            // ("stereobm_chunk"): disparities a lane of the fast kernel keeps running sums for
constexpr int ROLL_TILE = 64;             // ("stereobm_tile_cols"): window columns of a workgroup of the fast kernel; it produces 64 - (w - 1) pixels of a row
constexpr int ROLL_STRIP = 32;            // ("stereobm_strip_rows"): rows a workgroup of the fast kernel walks down
constexpr int GENERIC_TILE = 32;          // ("stereobm_generic_tile_cols"): pixels of a row per workgroup of the generic kernel

MI355_HD_PLAIN int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
MI355_HD_PLAIN int reflect101(int r, int len)
{
    if (len == 1) return 0;
    while (r < 0 || r >= len) r = r < 0 ? -r : 2 * (len - 1) - r;
    return r;
}

struct Geom { int m, n, Dmax, xlo, xhi, rlo, rhi, filtered; };
MI355_HD_PLAIN Geom geomOf(int W, int m, int n)
{
    Geom g;
    g.m = m; g.n = n; g.Dmax = m + n - 1;
    g.xlo = g.Dmax > 0 ? g.Dmax : 0;
    g.xhi = W + m < W ? W + m : W;
    g.rlo = g.Dmax;
    g.rhi = W - 1 + m < W - 1 ? W - 1 + m : W - 1;
    g.filtered = (m - 1) * 16;
    return g;
}
MI355_HD_PLAIN int leftCol(int u, int W) { return clampi(u, 0, W - 1); }
// the right image's column for window column u and disparity D
MI355_HD_PLAIN int rightCol(int u, int D, const Geom& g) { return clampi(u, g.rlo, g.rhi) - D; }

// one XSOBEL pixel from the three rows (already reflected) of the image
MI355_HD_PLAIN uint8_t xsobelPixel(const uint8_t* rm, const uint8_t* r0, const uint8_t* rp, int x, int W, int cap)
{
    if (x < 1 || x > W - 2) return (uint8_t)cap;
    const int v = cap + ((int)rm[x + 1] - (int)rm[x - 1]) + 2 * ((int)r0[x + 1] - (int)r0[x - 1]) + ((int)rp[x + 1] - (int)rp[x - 1]);
    return (uint8_t)clampi(v, 0, 2 * cap);
}

// acc + |a - b| for two byte values: one v_sad_u8 on the device
MI355_HD_PLAIN uint32_t absdiffAcc(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    return acc + (a > b ? a - b : b - a);
#endif
}

// ---- the decision of one pixel over its n SADs, index i = Dmax - D
// (cost, i) as one unsigned: the smallest key is the smallest i among the smallest costs.  cost < 2^19, i < 2^8
MI355_HD_PLAIN uint32_t minKey(uint32_t cost, int i) { return (cost << 8) | (uint32_t)i; }
MI355_HD_PLAIN int keyCost(uint32_t key) { return (int)(key >> 8); }
MI355_HD_PLAIN int keyIndex(uint32_t key) { return (int)(key & 255u); }
MI355_HD_PLAIN long long uniqThresh(int ms, int uniquenessRatio) { return (long long)ms + (long long)ms * uniquenessRatio / 100; }
// the uniqueness test looks at the smallest SAD outside [mi - 1, mi + 1]: `cost` for such an index, NO_COST inside (no compare: (1 - s * s) is negative iff |s| > 1)
constexpr uint32_t NO_COST = 0xffffffffu;
MI355_HD_PLAIN uint32_t outsideCost(int i, int mi, uint32_t cost) { const int s = i - mi; return cost | ~(uint32_t)((1 - s * s) >> 31); }
MI355_HD_PLAIN bool uniqRejects(uint32_t minOutside, int ms, int uniquenessRatio) { return minOutside != NO_COST && (long long)minOutside <= uniqThresh(ms, uniquenessRatio); }
// p = SAD[mi + 1] (SAD[n - 2] at mi = n - 1), nn = SAD[mi - 1] (SAD[1] at mi = 0)
MI355_HD_PLAIN int subpixel(int ms, int p, int nn, int Dmax, int mi)
{
    const int ad = p > nn ? p - nn : nn - p;
    const int dd = p + nn - 2 * ms + ad;
    const int q = dd ? (p - nn) * 256 / dd : 0;                 // C division: toward zero
    return ((Dmax - mi) * 256 + q + 15) >> 4;                   // arithmetic shift
}
MI355_HD_PLAIN int nextIndex(int mi, int n) { return mi + 1 < n ? mi + 1 : n - 2; }
MI355_HD_PLAIN int prevIndex(int mi) { return mi > 0 ? mi - 1 : 1; }

// sad(i): the pixel's SAD at index i.  *winCost: the winner's SAD when the pixel is kept
template <class F> MI355_HD_PLAIN int decide(F sad, int n, int T, int textureThreshold, int uniquenessRatio, const Geom& g, int* winCost)
{
    if (T < textureThreshold) return g.filtered;
    uint32_t best = 0xffffffffu;
    for (int i = 0; i < n; i++) { const uint32_t k = minKey((uint32_t)sad(i), i); if (k < best) best = k; }
    const int ms = keyCost(best), mi = keyIndex(best);
    if (uniquenessRatio > 0) {
        uint32_t mo = NO_COST;
        for (int i = 0; i < n; i++) { const uint32_t v = outsideCost(i, mi, (uint32_t)sad(i)); if (v < mo) mo = v; }
        if (uniqRejects(mo, ms, uniquenessRatio)) return g.filtered;
    }
    if (winCost) *winCost = ms;
    return subpixel(ms, sad(nextIndex(mi, n)), sad(prevIndex(mi)), g.Dmax, mi);
}

// ---- the left-right check: pixel x with disparity d (16S, not FILTERED) and winner's cost votes for column x2 with this key
constexpr unsigned long long LR_NONE = ~0ull;
MI355_HD_PLAIN int lrTarget(int x, int d) { return x - ((d + 8) >> 4); }
MI355_HD_PLAIN unsigned long long lrKey(int cost, int x, int d) { return ((unsigned long long)(uint32_t)cost << 32) | ((unsigned long long)(uint32_t)x << 16) | (uint16_t)(int16_t)d; }
MI355_HD_PLAIN int lrDisp(unsigned long long key, int filtered) { return key == LR_NONE ? filtered : (int)(int16_t)(uint16_t)(key & 0xffffu); }
// d2At(xk): the disparity voted into column xk (FILTERED when none); true: d[x] becomes FILTERED
template <class F> MI355_HD_PLAIN bool lrRejects(F d2At, int x, int d, int W, int disp12MaxDiff, int filtered)
{
    const long long lim = 16ll * disp12MaxDiff;
    const int xs[2] = {x - (d >> 4), x - ((d + 15) >> 4)};
    for (int k = 0; k < 2; k++) {
        const int xk = xs[k];
        if (xk < 0 || xk >= W) return false;
        const int e = d2At(xk);
        if (!(e > filtered)) return false;
        const long long df = (long long)e - d;
        if (!((df < 0 ? -df : df) > lim)) return false;
    }
    return true;
}

} // namespace sbm
