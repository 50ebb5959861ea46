// houghcircles_math.h -- the arithmetic of the circle transform served by houghcircles.hip (cv::HoughCircles, HOUGH_GRADIENT: HoughCirclesGradient in
// imgproc/src/hough.cpp), shared by the kernels and by a host build of the same lines that the CPU test-suite checks against the Python restatement
// (tests/hostemu/houghcircles_emu.cpp, tests/houghcircles_restate.py).  "float" is IEEE binary32 with every operation rounded on its own: both builds switch
// contraction off (-ffp-contract=off); sqrtf and / are correctly rounded; cvRound is round-half-to-even (hough::cvRoundF).  SHIFT = 10, ONE = 1024.
//   arguments  dp = max((float)dp, 1.f), idp = 1.f / dp; canny = cvRound(param1), accT = cvRound(param2); minRadius = max(0, minRadius); centersOnly = maxRadius < 0;
//              maxRadius <= 0 -> max(rows, cols), else maxRadius <= minRadius -> minRadius + 2.
//   accum      acols = ceil(cols * idp), arows = ceil(rows * idp) (the product in float); (arows + 2) x (acols + 2) CV_32S, astep = acols + 2.
//   vote       a pixel with edges != 0, (vx, vy) != (0, 0) and mag = sqrtf((float)(vx vx + vy vy)) >= 1: sx = cvRound((vx * idp) * ONE / mag), sy likewise,
//              x0 = cvRound((x * idp) * ONE), y0 likewise; for both signs of (sx, sy) and r = minRadius .. maxRadius: x2 = (x0 + r sx) >> SHIFT, y2 likewise; the ray
//              ends at the first r with (x2, y2) outside [0, acols) x [0, arows); otherwise cell y2 * astep + x2 gains one.  x2 and y2 are monotone in r, so the steps
//              that vote are those that lie inside while the ray's FIRST step does too: rayStarts() && inside(), which needs no walk and holds for every input.
//   centres    cells b = y * astep + x, y in 1 .. arows, x in 1 .. acols, that pass hough::isMaximum with accT; order hough::sortKey(a[b], b); (x + 0.5f) * dp.
//   radius     nBins = cvRound((maxRadius - minRadius) / dp * 10); a point with (float)minRadius^2 <= r2 <= (float)maxRadius^2, r2 = ex ex + ey ey, adds one to bin
//              clamp(cvRound((sqrtf(r2) - minRadius) / dp * 10), 0, nBins - 1); the scan from the top bin down over windows of 10 bins (scanBins / scanWindow).
//   suppress   circles ordered by hough::sortKey(votes, b); one is kept unless one kept before it has ddx ddx + ddy ddy < minDist * minDist.
// Bounds: width and height <= MAX_DIM (a packed point holds both, counts stay below 2^28); (arows + 2)(acols + 2) <= MAX_ACCUM (a cell index is the low word of the
// key); the prepared maxRadius <= MAX_RADIUS, so that x0 + r sx (at most 2^24 + 2^15 * 2^10) stays inside 31 bits; max_circles <= MAX_CIRCLES.
#pragma once
#include <stdint.h>
#include <math.h>

#include "hd.h"
#include "hough_math.h"

namespace houghcircles {

constexpr int SHIFT = 10, ONE = 1 << SHIFT;
constexpr int BINS_PER_DR = 10;                   // nBinsPerDr
constexpr int MAX_DIM = 16384;                    // largest width and height served
constexpr int MAX_ACCUM = 1 << 26;                // largest accumulator served, in cells ((arows + 2) x (acols + 2))
constexpr int MAX_RADIUS = 32768;                 // largest prepared maxRadius served
constexpr int MAX_CIRCLES = 65536;                // largest max_circles served
constexpr int LDS_BINS = 40960;                   // radius histograms of at most this many bins live in LDS (160 KiB, a CU's whole LDS; 4K's default 38400 fit); longer ones in HBM
constexpr int TILE = 64;                          // side of the accumulator tile a workgroup of k_hc_vote_tile owns (16 KiB of LDS)
constexpr int STEP_BLOCK = 16;                    // consecutive steps of a ray one lane of k_hc_vote walks
constexpr int HOUGH_GRADIENT = 3;                 // cv::HOUGH_GRADIENT
constexpr int HOUGH_GRADIENT_ALT = 4;
constexpr float EPSILON = 1.1920929e-07f;         // FLT_EPSILON

struct Params {
    int w, h;
    float dp, idp, minDist, minDist2;
    int canny, accT, minRadius, maxRadius, centersOnly;
    int arows, acols, astep, nBins;
    float minR2, maxR2;                           // (float)minRadius^2, (float)maxRadius^2
};

MI355_HD int cvRoundD(double v) { return (int)lrint(v); }   // host only in practice: the thresholds

// 0 when served; 1: dp, minDist, cvRound(param1) or cvRound(param2) not positive (or NaN); 2: the accumulator above MAX_ACCUM; 3: maxRadius above MAX_RADIUS; 4: nBins < 1.
// w and h are already known to be in 1 .. MAX_DIM.
inline int prepare(int w, int h, double dp, double minDist, double param1, double param2, int minRadius, int maxRadius, Params* p)
{
    if (!(dp > 0) || !(minDist > 0) || !(param1 > 0) || !(param2 > 0) || !(param1 < 1e9) || !(param2 < 1e9)) return 1;
    const float dpF = (float)dp, mdF = (float)minDist;
    if (!(dpF > 0) || !(mdF > 0) || !(dpF < 3.0e38f) || !(mdF < 1.8e19f)) return 1;
    p->canny = cvRoundD(param1); p->accT = cvRoundD(param2);
    if (p->canny <= 0 || p->accT <= 0) return 1;
    p->w = w; p->h = h;
    p->dp = dpF > 1.f ? dpF : 1.f;
    p->idp = 1.f / p->dp;
    p->minDist = mdF; p->minDist2 = mdF * mdF;
    p->minRadius = minRadius > 0 ? minRadius : 0;
    p->centersOnly = maxRadius < 0;
    if (maxRadius <= 0) maxRadius = w > h ? w : h;
    else if (maxRadius <= p->minRadius) {
        if (p->minRadius > MAX_RADIUS) return 3;
        maxRadius = p->minRadius + 2;
    }
    if (maxRadius > MAX_RADIUS) return 3;
    p->maxRadius = maxRadius;
    p->acols = (int)ceilf((float)w * p->idp); p->arows = (int)ceilf((float)h * p->idp);
    p->astep = p->acols + 2;
    if ((int64_t)(p->arows + 2) * (p->acols + 2) > MAX_ACCUM) return 2;
    const float span = (float)(p->maxRadius - p->minRadius) / p->dp;
    p->nBins = hough::cvRoundF(span * (float)BINS_PER_DR);
    if (p->nBins < 1) return 4;
    p->minR2 = (float)((int64_t)p->minRadius * p->minRadius); p->maxR2 = (float)((int64_t)p->maxRadius * p->maxRadius);
    return 0;
}

// the fixed-point ray of an edge pixel: false when the pixel does not vote
struct Ray { int x0, y0, sx, sy; };
MI355_HD bool makeRay(int x, int y, int vx, int vy, float idp, Ray* r)
{
    if (vx == 0 && vy == 0) return false;
    const float mag = sqrtf((float)((int64_t)vx * vx + (int64_t)vy * vy));
    if (!(mag >= 1.f)) return false;
    const float ax = (float)vx * idp, ay = (float)vy * idp;
    const float bx = ax * (float)ONE, by = ay * (float)ONE;
    r->sx = hough::cvRoundF(bx / mag); r->sy = hough::cvRoundF(by / mag);
    const float cx = (float)x * idp, cy = (float)y * idp;
    r->x0 = hough::cvRoundF(cx * (float)ONE); r->y0 = hough::cvRoundF(cy * (float)ONE);
    return true;
}
// step r of the ray with sign sg (+1 / -1): the cell's column and row; inside(): does it vote
MI355_HD void rayCell(const Ray& r, int sg, int step, int* x2, int* y2)
{
    *x2 = (r.x0 + step * sg * r.sx) >> SHIFT;
    *y2 = (r.y0 + step * sg * r.sy) >> SHIFT;
}
MI355_HD bool inside(int x2, int y2, int acols, int arows) { return (unsigned)x2 < (unsigned)acols && (unsigned)y2 < (unsigned)arows; }
// the ray's first step (r = minRadius) lies inside: a ray that does not start votes nowhere (the reference leaves its loop at once)
MI355_HD bool rayStarts(const Ray& r, int sg, int minRadius, int acols, int arows)
{
    int x2, y2;
    rayCell(r, sg, minRadius, &x2, &y2);
    return inside(x2, y2, acols, arows);
}

MI355_HD float centreCoord(int cell, float dp) { return ((float)cell + 0.5f) * dp; }
// the most centres a frame can yield (no row holds two maxima side by side), the capacity of the candidate list
MI355_HD int64_t maxCentres(int arows, int acols) { return (int64_t)arows * ((acols + 1) / 2); }

// the bin a point at (px, py) adds to for the centre (cx, cy), -1 when its distance is outside [minRadius, maxRadius]
MI355_HD int radiusBin(float cx, float cy, int px, int py, const Params& p)
{
    const float ex = cx - (float)px, ey = cy - (float)py;
    const float a = ex * ex, b = ey * ey;
    const float r2 = a + b;
    if (!(p.minR2 <= r2 && r2 <= p.maxR2)) return -1;
    const float r = sqrtf(r2);
    const float q = (r - (float)p.minRadius) / p.dp;
    int bin = hough::cvRoundF(q * (float)BINS_PER_DR);
    bin = bin < 0 ? 0 : bin;
    return bin > p.nBins - 1 ? p.nBins - 1 : bin;
}

// one window of the scan: bins upbin .. j + 1 held `cur` points (j = max(upbin - 10, -1), where the inner loop stopped)
MI355_HD void scanWindow(int upbin, int j, int cur, const Params& p, float* rBest, int* maxCount)
{
    const float mid = (float)(upbin + j) / 2.f;
    const float rCur = mid / (float)BINS_PER_DR * p.dp + (float)p.minRadius;
    if ((float)cur * *rBest >= (float)*maxCount * rCur || (*rBest < EPSILON && cur >= *maxCount)) { *rBest = rCur; *maxCount = cur; }
}
// the scan as written, one bin per step (the kernel skips runs of empty bins and calls scanWindow with the same numbers)
inline void scanBins(const int* bins, const Params& p, float* rBest, int* maxCount)
{
    *rBest = 0.f; *maxCount = 0;
    for (int j = p.nBins - 1; j > 0; j--) {
        if (!bins[j]) continue;
        const int upbin = j;
        int cur = 0;
        for (; j > upbin - BINS_PER_DR && j >= 0; j--) cur += bins[j];
        scanWindow(upbin, j, cur, p, rBest, maxCount);
    }
}

// is a candidate at (x, y) shadowed by a kept circle at (kx, ky)
MI355_HD bool tooClose(float kx, float ky, float x, float y, float minDist2)
{
    const float ddx = kx - x, ddy = ky - y;
    const float a = ddx * ddx, b = ddy * ddy;
    return a + b < minDist2;
}

} // namespace houghcircles
