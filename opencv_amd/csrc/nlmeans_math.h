// nlmeans_math.h -- cv::fastNlMeansDenoising on CV_8U (photo module, fast_nlmeans_denoising_invoker.hpp with the DistSquared policy), the lines shared by the kernels of
// nlmeans.hip and the host emulation tests/hostemu/nlmeans_emu.cpp: the BORDER_REFLECT_101 index, the geometry and the integer weight table, the patch distance and
// the final division.  The rule is the project's restatement (tests/nlmeans_restate.py); everything after the table is exact integer arithmetic, so the
// order in which a kernel forms its sums does not show in the result.
#pragma once
#include "hd.h"
#include <limits.h>
#include <math.h>

namespace nlm {

// borderInterpolate(p, len, BORDER_REFLECT_101): the reference's loop, any distance outside the image; a dimension of length 1 maps everything to 0
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

// the sizes in use: an even argument counts as the next odd value
struct Geom { int th, sh, T, S, b, shift, mult, len; };

MI355_HD int shiftOf(int T)                       // the smallest p with (1 << p) >= T * T
{
    int p = 0;
    while ((1 << p) < T * T) p++;
    return p;
}
MI355_HD int multOf(int S) { return INT_MAX / (S * S * 255); }       // S <= 181: the divisor stays far inside an int and the quotient below INT_MAX

// tws, sws >= 1 and the sizes in use <= 181 (the entries refuse the rest before they come here)
MI355_HD Geom geomOf(int tws, int sws, int cn)
{
    Geom g;
    g.th = tws / 2; g.sh = sws / 2;
    g.T = 2 * g.th + 1; g.S = 2 * g.sh + 1;
    g.b = g.th + g.sh;
    g.shift = shiftOf(g.T);
    g.mult = multOf(g.S);
    const double k = (double)(1 << g.shift) / (double)(g.T * g.T);
    g.len = (int)(255.0 * 255.0 * (double)cn / k + 1.0);
    return g;
}

// entry a of the table: cvRound(mult * exp(-a k / (h h cn))), h h cn in float, the rest in double, NaN counts as 1; 0 below 0.001 mult
inline int weightOf(int a, const Geom& g, float h, int cn)
{
    const double k = (double)(1 << g.shift) / (double)(g.T * g.T);
    const float hh = h * h * (float)cn;
    const double d = (double)a * k;
    double w = exp(-d / (double)hh);
    if (w != w) w = 1.0;
    int weight = (int)nearbyint((double)g.mult * w);            // cvRound: to nearest, ties to even (the default rounding mode)
    if ((double)weight < 0.001 * (double)g.mult) weight = 0;
    return weight;
}

// The table is non-increasing, so its non-zero entries are a prefix.  Fills table[0, min(len, cap)) (zeros after the prefix) when table != nullptr; -> the prefix length
inline int buildTable(const Geom& g, float h, int cn, int* table, int cap)
{
    int prefix = 0;
    bool zero = false;
    for (int a = 0; a < g.len; a++) {
        const int w = zero ? 0 : weightOf(a, g, h, cn);
        if (!w) {
            zero = true;
            if (!table || a >= cap) break;
        } else prefix = a + 1;
        if (table && a < cap) table[a] = w;
    }
    return prefix;
}

MI355_HD uint32_t sqDiff(int a, int b) { const int d = a - b; return (uint32_t)(d * d); }

// the distance of the patches around (y, x) and (y + dy, x + dx): px(row, column, channel) reads the extended image
template <class Px> MI355_HD unsigned long long patchDist(Px px, int y, int x, int dy, int dx, int th, int cn)
{
    unsigned long long D = 0;
    for (int ty = -th; ty <= th; ty++)
        for (int tx = -th; tx <= th; tx++)
            for (int c = 0; c < cn; c++) D += sqDiff(px(y + ty, x + tx, c), px(y + dy + ty, x + dx + tx, c));
    return D;
}

// (uint32)(est + weights_sum / 2) / weights_sum, saturated: est <= INT_MAX fits an int, the rounded sum only an unsigned
MI355_HD uint8_t finish(uint32_t est, uint32_t wsum)
{
    const uint32_t v = (est + wsum / 2u) / wsum;
    return (uint8_t)(v > 255u ? 255u : v);
}

// squared differences per pixel of the rule as written, S^2 T^2 cn, with the sizes in use: what one lane of the plain kernel does
MI355_HD unsigned long long pixelWork(int tws, int sws, int cn)
{
    const unsigned long long T = 2 * (tws / 2) + 1, S = 2 * (sws / 2) + 1;
    return S * S * T * T * (unsigned long long)cn;
}
// rows per launch of the plain kernel: at most `work` squared differences per launch over nf frames of W columns, a multiple of the workgroup's 4 rows, 4 at least
MI355_HD int plainBand(int T, int S, int cn, int W, int nf, unsigned long long work)
{
    const unsigned long long rows = work / ((unsigned long long)S * S * T * T * cn * (unsigned long long)W * nf);
    return rows < 4 ? 4 : rows > 16384 ? 16384 : (int)(rows & ~3ull);
}

// ---- the geometry of the tile kernel (k_nlm_tile), shared with its emulation.  A workgroup of 2 x 2 waves; a wave's 64 lanes are 64 columns of squared differences,
// which give 64 - 2 th patch centres, and it walks WAVE_ROWS output rows.  The LDS image holds the workgroup's pixels with a halo of b = th + sh, one plane per channel.
constexpr int WAVE_ROWS = 16;
struct Tile { int WC, LW, LH, PL; };        // output columns per wave; columns, rows and bytes of one plane
MI355_HD Tile tileOf(int th, int sh)
{
    Tile t;
    t.WC = 64 - 2 * th;
    t.LW = 2 * t.WC + 2 * (th + sh);
    t.LH = 2 * WAVE_ROWS + 2 * (th + sh);
    t.PL = t.LW * t.LH;
    return t;
}
// the table's non-zero prefix in LDS: 16-bit words where the largest weight, mult, fits them (S >= 13: mult = INT_MAX / (S^2 255) <= 49830), else 32-bit; the planes
// follow at a multiple of 16 bytes
MI355_HD bool wideTable(int mult) { return mult > 0xffff; }
MI355_HD int tableBytes(int prefix, bool wide) { return (prefix * (wide ? 4 : 2) + 15) & ~15; }
// plane index of the first squared difference of a lane's walk: image column X0 + wx WC - th + lane, image row Y0 + wy WAVE_ROWS - th
MI355_HD int walkStart(const Tile& t, int wx, int wy, int sh, int lane) { return (wy * WAVE_ROWS + sh) * t.LW + wx * t.WC + sh + lane; }
// ... and, relative to the walk's start shifted by the offset, of the pixel the weight of output row j multiplies: the patch summed over lanes lane - 2 th .. lane and
// walk rows j .. j + 2 th is centred th columns to the left and th rows down
MI355_HD int centreOf(const Tile& t, int j, int th) { return (j + th) * t.LW - th; }

} // namespace nlm
