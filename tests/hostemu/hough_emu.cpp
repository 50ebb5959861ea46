// hough_emu.cpp -- opencv_amd/csrc/hough_math.h (the arithmetic of the kernels of hough.hip) compiled for the CPU with -ffp-contract=off: the kernel sequence run
// serially -- pack the points, vote through voteColumn / cellIndex / inAccum, test isMaximum per inner cell, order by sortKey, emitLine -- for
// tests/test_hough_cpu.py to hold against tests/hough_restate.py.
#include <algorithm>
#include <vector>
#include "hough_math.h"

extern "C" int emu_hough_geometry(int w, int h, double rho, double theta, double minTheta, double maxTheta, int* numangle, int* numrho)
{
    hough::Geom g;
    const int rc = hough::geometry(w, h, rho, theta, minTheta, maxTheta, &g);
    if (rc == 0) { *numangle = g.numangle; *numrho = g.numrho; }
    return rc;
}

extern "C" int emu_hough_table(int w, int h, double rho, double theta, double minTheta, double maxTheta, float* tabSin, float* tabCos)
{
    hough::Geom g;
    if (hough::geometry(w, h, rho, theta, minTheta, maxTheta, &g)) return -1;
    hough::trigTable(g, tabSin, tabCos);
    return g.numangle;
}

// acc: (numangle + 2) x (numrho + 2) ints, dense; returns the number of points, -1 when the geometry is refused
extern "C" int emu_hough_accum(const unsigned char* img, size_t step, int w, int h, double rho, double theta, double minTheta, double maxTheta, int* acc)
{
    hough::Geom g;
    if (hough::geometry(w, h, rho, theta, minTheta, maxTheta, &g)) return -1;
    std::vector<float> tab(2 * (size_t)g.numangle);
    hough::trigTable(g, tab.data(), tab.data() + g.numangle);
    std::vector<uint32_t> pts;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            if (img[(size_t)y * step + x]) pts.push_back(hough::packPoint(x, y));
    const int bins = g.numrho + 2;
    std::fill(acc, acc + (size_t)(g.numangle + 2) * bins, 0);
    std::vector<int> row(bins);
    for (int n = 0; n < g.numangle; n++) {                                   // a workgroup: its row apart, the rest by flat index
        std::fill(row.begin(), row.end(), 0);
        for (uint32_t p : pts) {
            const int col = hough::voteColumn(hough::pointX(p), hough::pointY(p), tab[g.numangle + n], tab[n], g.numrho);
            if ((unsigned)col < (unsigned)bins) row[col]++;
            else {
                const int64_t cell = hough::cellIndex(n, col, g.numrho);
                if (hough::inAccum(cell, g.numangle, g.numrho)) acc[cell]++;
            }
        }
        for (int i = 0; i < bins; i++) acc[(size_t)(n + 1) * bins + i] += row[i];
    }
    return (int)pts.size();
}

// lines: maxLines rows of cn floats; returns the total number of maxima
extern "C" int emu_hough_lines(const int* acc, int w, int h, double rho, double theta, double minTheta, double maxTheta, int threshold, int cn, int maxLines, float* lines)
{
    hough::Geom g;
    if (hough::geometry(w, h, rho, theta, minTheta, maxTheta, &g)) return -1;
    std::vector<uint64_t> keys;
    for (int n = 0; n < g.numangle; n++)
        for (int r = 0; r < g.numrho; r++) {
            const int b = (n + 1) * (g.numrho + 2) + r + 1;
            if (hough::isMaximum(acc, b, g.numrho, threshold)) keys.push_back(hough::sortKey(acc[b], b));
        }
    if ((int64_t)keys.size() > hough::maxCandidates(g.numangle, g.numrho)) return -2;
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < keys.size() && i < (size_t)maxLines; i++) hough::emitLine(keys[i], g, cn, lines + i * cn);
    return (int)keys.size();
}

extern "C" int emu_hough_cv_round(float v) { return hough::cvRoundF(v); }
extern "C" unsigned long long emu_hough_sort_key(int votes, int b) { return hough::sortKey(votes, b); }
extern "C" int emu_hough_max_dim(void) { return hough::MAX_DIM; }
extern "C" int emu_hough_max_accum(void) { return hough::MAX_ACCUM; }
extern "C" int emu_hough_vote_chunk(void) { return hough::VOTE_CHUNK; }
extern "C" int emu_hough_vote_split(void) { return hough::VOTE_SPLIT; }
extern "C" int emu_hough_lds_bins(void) { return hough::LDS_BINS; }
