// sgbm_math.h -- the pieces of sgbm.hip (cv::StereoSGBM) that can be wrong, written once, __host__ __device__ so that the CPU suite compiles the very same lines
// (tests/hostemu/sgbm_emu.cpp) and holds them against tests/sgbm_restate.py bit for bit.  The definition is the project's restatement.
//
//   prefilter    G = clip(2 g(y) + g(y-) + g(y+), -ft, ft) + ft, g(r) = I[r][x+1] - I[r][x-1], rows REPLICATED (StereoBM reflects), border columns ft
//   pixel cost   Birchfield-Tomasi: a pixel with its two half-way neighbours is packed as (value, lo, hi) in one word, a cost is made from two such words
//   paths        a direction's paths as (first pixel, pixel stride, length): every kernel and the host walk the same enumeration; one step of the recurrence
//   decision     (S, k) as one key, the uniqueness test of one k, the sub-pixel quotient (C division)
//   left-right   one 64-bit key (S, -X, best) per target column, the smallest wins: independent of execution order
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "hd.h"

namespace sgbm {

enum { MODE_SGBM = 0, MODE_HH = 1, MODE_SGBM_3WAY = 2, MODE_HH4 = 3 };

constexpr int MAX_DISPARITIES = 256;      // mi355cv_limit("sgbm_max_disparities"): four values per lane of a wave in the fast path kernel, 16 waves in the cost kernel
constexpr int MAX_DIM = 16384;            // ("sgbm_max_dim"): a column fits the 16 bits the left-right key gives it
constexpr int MAX_COST = 32767;           // ("sgbm_max_cost"): blockSize^2 * (2 ft + 63) + P2 may not pass it, so that every C and every L_r fits 16 bits
constexpr int TILE = 64;                  // ("sgbm_tile_cols"): window columns of a workgroup of the cost kernel; it produces 64 - (w - 1) pixels of a row
constexpr int STRIP = 32;                 // ("sgbm_strip_rows"): rows a workgroup of the cost kernel walks down
constexpr int CHUNK = 16;                 // ("sgbm_chunk"): disparities a lane of the cost kernel keeps running sums for
constexpr int PATH_BLOCK = 16;            // ("sgbm_path_block"): steps of a path per block of loads of the fast path kernel at n <= 64; 8 at n <= 128, 4 above
constexpr int MAX_SCRATCH_MIB = 16384;    // ("sgbm_max_scratch_mib"): the volumes C (16 bit) and S (32 bit) of the frames in flight; 4K at n = 256 takes 11.4 GiB
constexpr int BIG = 1 << 28;              // an absent neighbour of the recurrence

MI355_HD_PLAIN int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
MI355_HD_PLAIN int mini(int a, int b) { return a < b ? a : b; }
MI355_HD_PLAIN int maxi(int a, int b) { return a > b ? a : b; }

struct Geom { int m, n, Dmax, xlo, xhi, W1, filtered; };
MI355_HD_PLAIN Geom geomOf(int W, int m, int n)
{
    Geom g;
    g.m = m; g.n = n; g.Dmax = m + n - 1;
    g.xlo = maxi(g.Dmax, 0);
    g.xhi = mini(W, W + m);
    g.W1 = g.xhi - g.xlo;
    g.filtered = (m - 1) * 16;
    return g;
}
MI355_HD_PLAIN int ftOf(int preFilterCap) { return maxi(preFilterCap, 15) | 1; }
// the largest value a C or an L_r can take: per pixel of the window 2 ft from the prefiltered plane and 255 >> 2 from the raw one; L_r <= C + P2
MI355_HD_PLAIN long long costBound(int w, int ft, int P2) { return (long long)w * w * (2ll * ft + 63) + P2; }
// bytes of scratch one frame takes: C, S, the two prefiltered planes, the winners, the left-right keys, a CV_16S map
MI355_HD_PLAIN unsigned long long frameScratch(int W, int H, int W1, int n)
{
    const unsigned long long vol = (unsigned long long)(W1 > 0 ? W1 : 0) * H * n, px = (unsigned long long)W * H;
    return vol * 6 + px * (2 + 4 + 8 + 2) + 32ull * H + 4096;
}

// one prefiltered pixel from the three rows (already replicated) of the image
MI355_HD_PLAIN uint8_t prefilterPixel(const uint8_t* rm, const uint8_t* r0, const uint8_t* rp, int x, int W, int ft)
{
    if (x < 1 || x > W - 2) return (uint8_t)ft;
    const int v = 2 * ((int)r0[x + 1] - (int)r0[x - 1]) + ((int)rm[x + 1] - (int)rm[x - 1]) + ((int)rp[x + 1] - (int)rp[x - 1]);
    return (uint8_t)(clampi(v, -ft, ft) + ft);
}

// ---- Birchfield-Tomasi.  a pixel a with its row neighbours (the border columns repeat themselves): value | lo << 8 | hi << 16
MI355_HD_PLAIN uint32_t btPack(int a, int left, int right)
{
    const int am = (a + left) >> 1, ap = (a + right) >> 1;
    const int lo = mini(mini(am, ap), a), hi = maxi(maxi(am, ap), a);
    return (uint32_t)a | ((uint32_t)lo << 8) | ((uint32_t)hi << 16);
}
MI355_HD_PLAIN uint32_t btPackAt(const uint8_t* row, int x, int W) { return btPack(row[x], row[maxi(x - 1, 0)], row[mini(x + 1, W - 1)]); }
MI355_HD_PLAIN int btCost(uint32_t l, uint32_t r)
{
    const int u = (int)(l & 255u), loL = (int)((l >> 8) & 255u), hiL = (int)((l >> 16) & 255u);
    const int v = (int)(r & 255u), loR = (int)((r >> 8) & 255u), hiR = (int)((r >> 16) & 255u);
    const int c0 = maxi(0, maxi(u - hiR, loR - u)), c1 = maxi(0, maxi(v - hiL, loL - v));
    return mini(c0, c1);
}
// the two planes: prefiltered (shift 0) and raw (shift 2)
MI355_HD_PLAIN int pixelCost(uint32_t gl, uint32_t gr, uint32_t il, uint32_t ir) { return btCost(gl, gr) + (btCost(il, ir) >> 2); }

// ---- paths.  A direction (ry, rx) is the step from the predecessor to the pixel
MI355_HD_PLAIN int dirCount(int mode) { return mode == MODE_HH ? 8 : mode == MODE_SGBM ? 5 : 4; }
MI355_HD_PLAIN void dirOf(int mode, int i, int* ry, int* rx)
{
    // MODE_HH: all eight; MODE_SGBM: the first five of them; MODE_HH4: the four axis directions
    const int hy[8] = {0, 1, 1, 1, 0, -1, -1, -1}, hx[8] = {1, 1, 0, -1, -1, -1, 0, 1};
    const int qy[4] = {0, 0, 1, -1}, qx[4] = {1, -1, 0, 0};
    if (mode == MODE_HH4) { *ry = qy[i]; *rx = qx[i]; } else { *ry = hy[i]; *rx = hx[i]; }
}
// the paths of one direction over the W1 x H valid pixels.  Horizontal: a path per row.  Otherwise a path per starting column x0 of row 0 (rows counted in the
// direction of ry), x0 running over the columns outside the image too from which a diagonal enters it; such a path begins where it enters.
MI355_HD_PLAIN int pathCount(int ry, int rx, int W1, int H) { return ry == 0 ? H : W1 + (rx != 0 ? H - 1 : 0); }
struct Path { long long p0, dp; int count; };       // first pixel (y * W1 + x), pixel stride, pixels
MI355_HD_PLAIN Path pathOf(int ry, int rx, int W1, int H, int idx)
{
    Path P;
    if (ry == 0) {
        P.p0 = (long long)idx * W1 + (rx > 0 ? 0 : W1 - 1); P.dp = rx; P.count = W1;
        return P;
    }
    const int x0 = idx - (rx > 0 ? H - 1 : 0);
    // step t is at x = x0 + rx t: inside [0, W1) for t0 <= t < t1
    int t0 = 0, t1 = H;
    if (rx > 0) { t0 = maxi(0, -x0); t1 = mini(H, W1 - x0); }
    if (rx < 0) { t0 = maxi(0, x0 - (W1 - 1)); t1 = mini(H, x0 + 1); }
    const int y0 = ry > 0 ? t0 : H - 1 - t0;
    P.p0 = (long long)y0 * W1 + (x0 + rx * t0);
    P.dp = (long long)ry * W1 + rx;
    P.count = t1 > t0 ? t1 - t0 : 0;
    return P;
}
// one step: prev = L(p - r, k), dn = L(p - r, k - 1), up = L(p - r, k + 1) (BIG where absent), M = min_k L(p - r, k)
MI355_HD_PLAIN int pathStep(int c, int prev, int dn, int up, int M, int P1, int P2) { return c + mini(mini(prev, M + P2), mini(dn, up) + P1) - M; }

// ---- the decision over S (at most 8 * 32767 < 2^18)
MI355_HD_PLAIN uint32_t minKey(uint32_t S, int k) { return (S << 8) | (uint32_t)k; }
MI355_HD_PLAIN int keyCost(uint32_t key) { return (int)(key >> 8); }
MI355_HD_PLAIN int keyIndex(uint32_t key) { return (int)(key & 255u); }
MI355_HD_PLAIN bool uniqFails(int Sk, int k, int best, int ms, int uniquenessRatio)
{
    const int s = k - best;
    return (s > 1 || s < -1) && (long long)Sk * (100 - uniquenessRatio) < (long long)ms * 100;
}
// the CV_16S value of a kept pixel: sm = S[best - 1], sp = S[best + 1] (unused at the ends of the range)
MI355_HD_PLAIN int disparity16(int best, int ms, int sm, int sp, int n, int m)
{
    int d = best * 16;
    if (best > 0 && best < n - 1) {
        const int den = maxi(sm + sp - 2 * ms, 1);
        d += ((sm - sp) * 16 + den) / (2 * den);                 // C division: toward zero
    }
    return d + 16 * m;
}
// what a pixel leaves for the left-right check: S of the winner and the winner, or NOT_KEPT
constexpr uint32_t NOT_KEPT = 0xffffffffu;
MI355_HD_PLAIN uint32_t winOf(int ms, int best) { return minKey((uint32_t)ms, best); }

// ---- the left-right check
constexpr unsigned long long LR_NONE = ~0ull;
MI355_HD_PLAIN unsigned long long lrKey(int ms, int X, int best) { return ((unsigned long long)(uint32_t)ms << 32) | ((unsigned long long)(uint32_t)(0xffff - X) << 16) | (uint32_t)best; }
MI355_HD_PLAIN int lrDisp(unsigned long long key, int m) { return key == LR_NONE ? m - 1 : (int)(key & 0xffffu) + m; }
// d2At(xk): the disparity voted into column xk (m - 1 when none); true: d1 becomes FILTERED
template <class F> MI355_HD_PLAIN bool lrRejects(F d2At, int X, int d1, int W, int m, int disp12MaxDiff)
{
    const int q = disp12MaxDiff > 0 ? disp12MaxDiff : 1;
    const int dks[2] = {d1 >> 4, (d1 + 15) >> 4};               // arithmetic shifts
    for (int i = 0; i < 2; i++) {
        const int dk = dks[i], xk = X - dk;
        if (xk < 0 || xk >= W) return false;
        const int e = d2At(xk);
        if (e < m) return false;
        const int df = e > dk ? e - dk : dk - e;
        if (!(df > q)) return false;
    }
    return true;
}

} // namespace sgbm
