// disttransform_math.h -- the arithmetic of the distance transform served by disttransform.hip (cv::distanceTransform with DIST_L2 + DIST_MASK_PRECISE,
// DIST_L1 and DIST_C), shared by the kernels and by a host build of the same lines that the CPU test-suite checks against the numpy restatement
// (tests/hostemu/disttransform_emu.cpp, tests/disttransform_restate.py).
//
// A pixel is a site iff it is 0.  Two separable steps, both in exact integer arithmetic:
//   columns   g(y, x) = distance from row y to the nearest site of column x, up or down; CAP where the column holds none.  A column is cut into segments of
//             SEG = 64 rows whose sites are the bits of one 64-bit word (bit i = row 64 s + i); the nearest site outside a segment is a carry found from
//             the words of the other segments (carryUp / carryDown), the distance inside it two bit scans (colDist).
//   rows      out(y, q) = min over r of  r^2 + g(y, q +- r)^2 (L2),  r + g (L1),  max(r, g) (C): an outward scan from r = 0 that stops once r alone is no
//             better than the best value so far (L2: r^2 >= best; L1 and C: r >= best) or both sides have left the row (scanRow).
// Bounds: width and height <= MAX_DIM = 16384, so a real g is <= 16383, a real squared distance < 2^30 and a real L1 distance <= 32766.  CAP = 32768 is above
// every real g and L1 / C distance, CAP^2 = 2^30 above every real squared distance, and r^2 + CAP^2 < 2^31 cannot overflow the scan.  A row whose g are all
// CAP belongs to a frame without any site: the row pass writes the library's own value there (NO_SITE_32F / NO_SITE_8U), not a distance.
//   root      the L2 output: the exact integer d2, square-rooted and correctly rounded to float.  Below 2^24 the integer is a float and sqrtf is that rounding
//             (both correctly rounded; the composition was checked exhaustively against the double root); from 2^24 on the cast would round first, so the
//             root is taken in double and rounded once more, which is the contract's definition.
#pragma once
#include <stdint.h>
#include <math.h>

#include "hd.h"

namespace disttransform {

enum { L1 = 1, L2 = 2, C = 3 };                   // cv::DIST_L1, DIST_L2, DIST_C
constexpr int SEG = 64;                           // rows per column segment = bits of a site word
constexpr int MAX_DIM = 16384;                    // largest width and height served
constexpr uint32_t CAP = 32768;                   // g of a column without a site
constexpr float NO_SITE_32F = 31622776.0f;        // sqrtf(1e15f): every pixel of a frame without a site (CV_32F)
constexpr int NO_SITE_8U = 255;

using mi355::clz64;
using mi355::ctz64;

// words[k * stride]: the site word of segment k of one column.  Distance from the FIRST row of segment s up to the nearest site above the segment, CAP if none
MI355_HD uint32_t carryUp(const uint64_t* words, size_t stride, int s)
{
    for (int k = s - 1; k >= 0; k--) {
        const uint64_t m = words[(size_t)k * stride];
        if (m) return (uint32_t)((s - k) * SEG - (63 - clz64(m)));
    }
    return CAP;
}
// distance from the LAST row (row 63, whether or not the image has it) of segment s down to the nearest site below the segment, CAP if none
MI355_HD uint32_t carryDown(const uint64_t* words, size_t stride, int s, int nseg)
{
    for (int k = s + 1; k < nseg; k++) {
        const uint64_t m = words[(size_t)k * stride];
        if (m) return (uint32_t)((k - s - 1) * SEG + 1 + ctz64(m));
    }
    return CAP;
}
// g of row i (0..63) of a segment with site word m; up / down as returned by carryUp / carryDown
MI355_HD uint32_t colDist(uint64_t m, int i, uint32_t up, uint32_t down)
{
    const uint64_t lo = m & ((uint64_t(2) << i) - 1), hi = m >> i;            // sites at rows <= i, sites at rows >= i
    const uint32_t du = lo ? (uint32_t)(i - (63 - clz64(lo))) : (up == CAP ? CAP : up + (uint32_t)i);
    const uint32_t dd = hi ? (uint32_t)ctz64(hi) : (down == CAP ? CAP : down + (uint32_t)(63 - i));
    return du < dd ? du : dd;
}

// one output of the row pass: g[0..w-1] the column distances of its row, q its column.  L2: the squared distance; L1 / C: the distance.
template <int METRIC, typename G> MI355_HD uint32_t scanRow(const G* g, int w, int q)
{
    const uint32_t g0 = g[q];
    uint32_t best = METRIC == L2 ? g0 * g0 : g0;
    const int reach = q > w - 1 - q ? q : w - 1 - q;
    for (int r = 1; r <= reach; r++) {
        const uint32_t rr = METRIC == L2 ? (uint32_t)r * (uint32_t)r : (uint32_t)r;
        if (rr >= best) break;
        if (r <= q) {
            const uint32_t v = g[q - r], c = METRIC == L2 ? rr + v * v : METRIC == L1 ? rr + v : (rr > v ? rr : v);
            best = c < best ? c : best;
        }
        if (q + r < w) {
            const uint32_t v = g[q + r], c = METRIC == L2 ? rr + v * v : METRIC == L1 ? rr + v : (rr > v ? rr : v);
            best = c < best ? c : best;
        }
    }
    return best;
}

MI355_HD float root(uint32_t d2) { return d2 < (1u << 24) ? sqrtf((float)d2) : (float)sqrt((double)d2); }

// the served outputs of one pixel of a frame that has a site
template <int METRIC> MI355_HD float out32f(uint32_t v) { return METRIC == L2 ? root(v) : (float)v; }
MI355_HD unsigned char out8u(uint32_t v) { return (unsigned char)(v > 255u ? 255u : v); }

} // namespace disttransform
