// houghcircles_emu.cpp -- opencv_amd/csrc/houghcircles_math.h (the arithmetic of the kernels of houghcircles.hip) compiled for the CPU with -ffp-contract=off: the
// kernel sequence run serially -- the point list row by row, every step of every ray on its own under rayStarts / inside (as the lanes take them), isMaximum per
// cell, sortKey, radiusBin per point, the scan both as written (scanBins) and in the kernel's 64-bins-at-a-time form, the suppression walk -- for
// tests/test_houghcircles_cpu.py to hold against tests/houghcircles_restate.py.
#include <algorithm>
#include <vector>
#include "houghcircles_math.h"

namespace hc = houghcircles;

// out: arows, acols, nBins, minRadius, maxRadius, centersOnly, canny, accT
extern "C" int emu_hc_prepare(int w, int h, double dp, double minDist, double param1, double param2, int minRadius, int maxRadius, int* out)
{
    hc::Params p;
    const int rc = hc::prepare(w, h, dp, minDist, param1, param2, minRadius, maxRadius, &p);
    if (rc == 0) { out[0] = p.arows; out[1] = p.acols; out[2] = p.nBins; out[3] = p.minRadius; out[4] = p.maxRadius; out[5] = p.centersOnly; out[6] = p.canny; out[7] = p.accT; }
    return rc;
}

extern "C" int emu_hc_make_ray(int x, int y, int vx, int vy, float idp, int* out)
{
    hc::Ray r;
    if (!hc::makeRay(x, y, vx, vy, idp, &r)) return 0;
    out[0] = r.x0; out[1] = r.y0; out[2] = r.sx; out[3] = r.sy;
    return 1;
}

// acc: (arows + 2) x (acols + 2) ints, dense; pts: w * h packed points; gstep in shorts.  Returns the number of points, -1 when the arguments are refused
extern "C" int emu_hc_accum(const unsigned char* edges, size_t estep, const short* dx, const short* dy, size_t gstep, int w, int h, double dp, int minRadius, int maxRadius,
                            int* acc, uint32_t* pts)
{
    hc::Params p;
    if (hc::prepare(w, h, dp, 1.0, 1.0, 1.0, minRadius, maxRadius, &p)) return -1;
    std::fill(acc, acc + (size_t)(p.arows + 2) * p.astep, 0);
    int np = 0;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            if (edges[(size_t)y * estep + x] && (dx[(size_t)y * gstep + x] | dy[(size_t)y * gstep + x])) pts[np++] = hough::packPoint(x, y);
    for (int i = 0; i < np; i++) {
        const int x = hough::pointX(pts[i]), y = hough::pointY(pts[i]);
        hc::Ray ray;
        if (!hc::makeRay(x, y, dx[(size_t)y * gstep + x], dy[(size_t)y * gstep + x], p.idp, &ray)) return -2;      // a point is a pixel that votes
        for (int sg = 1; sg >= -1; sg -= 2) {
            if (!hc::rayStarts(ray, sg, p.minRadius, p.acols, p.arows)) continue;
            for (int r = p.maxRadius; r >= p.minRadius; r--) {              // a lane per step, in no particular order
                int x2, y2;
                hc::rayCell(ray, sg, r, &x2, &y2);
                if (hc::inside(x2, y2, p.acols, p.arows)) acc[(size_t)y2 * p.astep + x2]++;
            }
        }
    }
    return np;
}

// the scan as wave 0 of k_hc_radius walks it
static void scanSkipping(const int* bins, const hc::Params& p, float* rBest, int* maxCount)
{
    *rBest = 0.f; *maxCount = 0;
    int j = p.nBins - 1;
    while (j > 0) {
        int first = -1;
        for (int lane = 0; lane < 64 && first < 0; lane++) if (j - lane > 0 && bins[j - lane]) first = lane;
        if (first < 0) { j -= 64; continue; }
        const int upbin = j - first;
        int cur = 0;
        for (int lane = 0; lane < hc::BINS_PER_DR; lane++) if (upbin - lane >= 0) cur += bins[upbin - lane];
        j = upbin - hc::BINS_PER_DR < -1 ? -1 : upbin - hc::BINS_PER_DR;
        hc::scanWindow(upbin, j, cur, p, rBest, maxCount);
        j--;
    }
}

// circles: maxCircles rows of cn floats; accT < 0: the prepared one.  Returns the number written; -1 refused, -3 the two forms of the scan disagree
extern "C" int emu_hc_circles(const int* accIn, const uint32_t* pts, int np, int w, int h, double dp, double minDist, double param1, double param2, int minRadius, int maxRadius,
                              int accT, int cn, int maxCircles, float* circles)
{
    hc::Params p;
    if (hc::prepare(w, h, dp, minDist, param1, param2, minRadius, maxRadius, &p)) return -1;
    if (accT >= 0) p.accT = accT;
    std::vector<int> acc(accIn, accIn + (size_t)(p.arows + 2) * p.astep);
    std::vector<uint64_t> keys;
    for (int y = 0; y < p.arows; y++)
        for (int x = 0; x < p.acols; x++) {
            const int b = (y + 1) * p.astep + x + 1;
            if (hough::isMaximum(acc.data(), b, p.acols, p.accT)) keys.push_back(hough::sortKey(acc[b], b));
        }
    if ((int64_t)keys.size() > hc::maxCentres(p.arows, p.acols)) return -2;
    std::sort(keys.begin(), keys.end());
    if (!p.centersOnly) {
        std::vector<uint64_t> keys2;
        std::vector<int> bins(p.nBins);
        for (uint64_t key : keys) {
            const int b = hough::keyCell(key);
            const float cx = hc::centreCoord(b % p.astep, p.dp), cy = hc::centreCoord(b / p.astep, p.dp);
            std::fill(bins.begin(), bins.end(), 0);
            for (int i = 0; i < np; i++) {
                const int bin = hc::radiusBin(cx, cy, hough::pointX(pts[i]), hough::pointY(pts[i]), p);
                if (bin >= 0) bins[bin]++;
            }
            float rBest, rSeq; int maxCount, mSeq;
            scanSkipping(bins.data(), p, &rBest, &maxCount);
            hc::scanBins(bins.data(), p, &rSeq, &mSeq);
            if (rBest != rSeq || maxCount != mSeq) return -3;
            if (maxCount > p.accT) keys2.push_back(hough::sortKey(maxCount, b));
            union { float f; int i; } u; u.f = rBest;
            acc[b] = u.i;                                                   // the radius takes the cell's place, as in the kernel
        }
        std::sort(keys2.begin(), keys2.end());
        keys.swap(keys2);
    }
    std::vector<float> kx, ky;
    for (uint64_t key : keys) {
        const int b = hough::keyCell(key);
        const float cx = hc::centreCoord(b % p.astep, p.dp), cy = hc::centreCoord(b / p.astep, p.dp);
        bool shadowed = false;
        for (size_t k = 0; k < kx.size() && !shadowed; k++) shadowed = hc::tooClose(kx[k], ky[k], cx, cy, p.minDist2);
        if (shadowed) continue;
        float* row = circles + kx.size() * cn;
        union { float f; int i; } u; u.i = acc[b];
        row[0] = cx; row[1] = cy; row[2] = p.centersOnly ? 0.f : u.f;
        if (cn == 4) row[3] = (float)hough::keyVotes(key);
        kx.push_back(cx); ky.push_back(cy);
        if ((int)kx.size() == maxCircles) break;
    }
    return (int)kx.size();
}

extern "C" int emu_hc_limit(int which)
{
    const int v[] = {hc::MAX_DIM, hc::MAX_ACCUM, hc::MAX_RADIUS, hc::MAX_CIRCLES, hc::LDS_BINS, hc::TILE, hc::STEP_BLOCK, hc::SHIFT, hc::ONE, hc::BINS_PER_DR,
                     hc::HOUGH_GRADIENT, hc::HOUGH_GRADIENT_ALT};
    return which >= 0 && which < (int)(sizeof(v) / sizeof(v[0])) ? v[which] : -1;
}
