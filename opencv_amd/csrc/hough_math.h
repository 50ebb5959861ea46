// hough_math.h -- the arithmetic of the standard Hough transform served by hough.hip (cv::HoughLines / HoughLinesWithAccumulator, HoughLinesStandard in
// imgproc/src/hough.cpp), shared by the kernels and by a host build of the same lines that the CPU test-suite checks against the Python restatement
// (tests/hostemu/hough_emu.cpp, tests/hough_restate.py).  "float" is IEEE binary32 with every operation rounded on its own: both builds switch contraction off
// (-ffp-contract=off), so no product below is fused into the addition that follows it.  cvRound is round-half-to-even.
//   geometry  max_rho = w + h, min_rho = -max_rho; numangle = floor((max_theta - min_theta) / theta) + 1 in double, one fewer when the last angle would land within
//             theta / 2 of pi; numrho = cvRound(float(max_rho - min_rho + 1) / (float)rho); irho = 1.f / (float)rho.
//   table     ang = (float)min_theta; tabSin[n] = (float)(sin((double)ang) * irho), tabCos[n] likewise (the product in double); ang += (float)theta in float.
//   vote      r = cvRound(x * tabCos[n] + y * tabSin[n]) + (numrho - 1) / 2; cell (n + 1)(numrho + 2) + r + 1 of the (numangle + 2) x (numrho + 2) CV_32S accumulator.
//   maximum   a[b] > threshold, > the cell to its left and the one above, >= the cell to its right and the one below.
//   order     votes descending, equal votes by accumulator index ascending: the 64-bit key (~votes << 32) | b, ascending.
//   emit      rho = (r - (numrho - 1) * 0.5f) * (float)rho, theta = (float)min_theta + n * (float)theta.
// Bounds: width and height <= MAX_DIM = 16384 (the bound of the neighbouring entries), so a packed point (y << 16 | x) holds both coordinates, the number of edge
// pixels and every vote count fit 2^28, the point list of a frame stays within 1 GiB,
// and float(2 (w + h) + 1) is exact; the accumulator has at most MAX_ACCUM = 2^26 cells, so a cell index fits the low word of the key (and an int).
#pragma once
#include <stdint.h>
#include <math.h>

#include "hd.h"

namespace hough {

constexpr int MAX_DIM = 16384;                    // largest width and height served
constexpr int MAX_ACCUM = 1 << 26;                // largest accumulator served, in cells ((numangle + 2) x (numrho + 2))
constexpr int VOTE_CHUNK = 4096;                  // points a workgroup of k_hough_vote walks between two looks at the list's length
constexpr int VOTE_SPLIT = 16;                    // at most this many workgroups share one angle row
constexpr int LDS_BINS = 16384;                   // a row of at most this many bins (numrho + 2) is voted in LDS (64 KiB); longer rows vote straight into HBM
constexpr double PI = 3.1415926535897932384626433832795;      // CV_PI

struct Geom { int numangle, numrho; float rho, theta, irho, minTheta; };

MI355_HD int cvRoundF(float v)                    // round half to even
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(v);
#else
    return (int)lrintf(v);
#endif
}

// 0 when served; 1: arguments outside the function's domain; 2: the accumulator would exceed MAX_ACCUM cells.  w, h are already known to be in 1 .. MAX_DIM.
inline int geometry(int w, int h, double rho, double theta, double minTheta, double maxTheta, Geom* g)
{
    if (!(rho > 0) || !(theta > 0) || !(minTheta >= 0) || !(minTheta < maxTheta) || !(maxTheta <= PI)) return 1;
    const float rhoF = (float)rho, thetaF = (float)theta;
    if (!(rhoF > 0) || !(thetaF > 0)) return 1;
    const int maxRho = w + h, minRho = -maxRho;
    const double na = floor((maxTheta - minTheta) / theta) + 1;
    if (!(na < (double)MAX_ACCUM)) return 2;
    int numangle = (int)na;
    if (numangle > 1 && fabs(PI - (numangle - 1) * theta) < theta / 2) numangle--;
    const float nr = (float)(maxRho - minRho + 1) / rhoF;
    if (!(nr < (float)MAX_ACCUM)) return 2;
    const int numrho = cvRoundF(nr);
    if ((int64_t)(numangle + 2) * (numrho + 2) > MAX_ACCUM) return 2;
    g->numangle = numangle; g->numrho = numrho; g->rho = rhoF; g->theta = thetaF; g->irho = 1.f / rhoF; g->minTheta = (float)minTheta;
    return 0;
}

// host only: libm's sin / cos in double
inline void trigTable(const Geom& g, float* tabSin, float* tabCos)
{
    float ang = g.minTheta;
    for (int n = 0; n < g.numangle; n++) {
        tabSin[n] = (float)(sin((double)ang) * g.irho);
        tabCos[n] = (float)(cos((double)ang) * g.irho);
        ang += g.theta;
    }
}

MI355_HD uint32_t packPoint(int x, int y) { return (uint32_t)y << 16 | (uint32_t)x; }
MI355_HD int pointX(uint32_t p) { return (int)(p & 0xffffu); }
MI355_HD int pointY(uint32_t p) { return (int)(p >> 16); }

// the column (r + 1) of the accumulator row of an angle that pixel (x, y) votes for; 0 <= column < numrho + 2 for every geometry the reference itself keeps
// inside its row, and the callers send anything else through cellIndex / inAccum
MI355_HD int voteColumn(int x, int y, float c, float s, int numrho)
{
    const float a = (float)x * c, b = (float)y * s;
    return cvRoundF(a + b) + (numrho - 1) / 2 + 1;
}
MI355_HD int64_t cellIndex(int n, int column, int numrho) { return (int64_t)(n + 1) * (numrho + 2) + column; }
MI355_HD bool inAccum(int64_t cell, int numangle, int numrho) { return cell >= 0 && cell < (int64_t)(numangle + 2) * (numrho + 2); }

// a: the accumulator, b: the index of an inner cell
MI355_HD bool isMaximum(const int* a, int b, int numrho, int threshold)
{
    const int v = a[b];
    return v > threshold && v > a[b - 1] && v >= a[b + 1] && v > a[b - numrho - 2] && v >= a[b + numrho + 2];
}

MI355_HD uint64_t sortKey(int votes, int b) { return (uint64_t)(~(uint32_t)votes) << 32 | (uint32_t)b; }
MI355_HD int keyVotes(uint64_t key) { return (int)~(uint32_t)(key >> 32); }
MI355_HD int keyCell(uint64_t key) { return (int)(uint32_t)key; }
// no row holds two maxima side by side (the test against the left neighbour is strict): the most a frame can yield, and the capacity of the candidate list
MI355_HD int64_t maxCandidates(int numangle, int numrho) { return (int64_t)numangle * ((numrho + 1) / 2); }

// line i of the output: lines_cn floats (2, or 3 with the votes)
MI355_HD void emitLine(uint64_t key, const Geom& g, int cn, float* out)
{
    const int b = keyCell(key);
    const int n = b / (g.numrho + 2) - 1;
    const int r = b - (n + 1) * (g.numrho + 2) - 1;
    const float half = (float)(g.numrho - 1) * 0.5f;
    out[0] = ((float)r - half) * g.rho;
    const float t = (float)n * g.theta;
    out[1] = g.minTheta + t;
    if (cn == 3) out[2] = (float)keyVotes(key);
}

} // namespace hough
