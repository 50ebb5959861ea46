// disttransform_emu.cpp -- opencv_amd/csrc/disttransform_math.h (the arithmetic of k_dist_sites, k_dist_cols and k_dist_row) compiled for the CPU with
// -ffp-contract=off: a whole distance transform run serially through the same lines -- site words per column segment, carries, column distances as u16, the
// outward row scan, the root and the casts.  tests/test_disttransform_cpu.py compares it with the numpy restatement (tests/disttransform_restate.py).
// Test infrastructure.
#include "disttransform_math.h"
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dt = disttransform;

namespace {
// g[y * w + x] as k_dist_sites + k_dist_cols leave it in HBM
void columns(const unsigned char* src, size_t sstep, int w, int h, std::vector<uint16_t>& g)
{
    const int nseg = (h + dt::SEG - 1) / dt::SEG;
    std::vector<uint64_t> words((size_t)nseg * w, 0);
    for (int s = 0; s < nseg; s++)
        for (int x = 0; x < w; x++) {
            uint64_t m = 0;
            for (int i = 0; i < dt::SEG && s * dt::SEG + i < h; i++) m |= (uint64_t)(src[(size_t)(s * dt::SEG + i) * sstep + x] == 0) << i;
            words[(size_t)s * w + x] = m;
        }
    g.assign((size_t)w * h, 0);
    for (int s = 0; s < nseg; s++)
        for (int x = 0; x < w; x++) {
            const uint64_t* col = &words[x];
            const uint32_t up = dt::carryUp(col, w, s), down = dt::carryDown(col, w, s, nseg);
            for (int i = 0; i < dt::SEG && s * dt::SEG + i < h; i++) g[(size_t)(s * dt::SEG + i) * w + x] = (uint16_t)dt::colDist(col[(size_t)s * w], i, up, down);
        }
}

template <int METRIC, typename T> void rows(const std::vector<uint16_t>& g, int w, int h, unsigned char* dst, size_t dstep)
{
    for (int y = 0; y < h; y++) {
        const uint16_t* row = &g[(size_t)y * w];
        bool site = false;
        for (int x = 0; x < w; x++) site |= row[x] < dt::CAP;
        T* out = (T*)(dst + (size_t)y * dstep);
        for (int q = 0; q < w; q++) {
            if (sizeof(T) == 1) out[q] = (T)(site ? dt::out8u(dt::scanRow<METRIC>(row, w, q)) : (unsigned char)dt::NO_SITE_8U);
            else out[q] = (T)(site ? dt::out32f<METRIC>(dt::scanRow<METRIC>(row, w, q)) : dt::NO_SITE_32F);
        }
    }
}
}

// metric 1 / 2 / 3 = DIST_L1 / L2 / C; depth as in the C ABI: 0 CV_8U (L1 only), 5 CV_32F.  Returns -1 for anything else.
extern "C" int emu_disttransform(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int w, int h, int metric, int depth)
{
    if (w <= 0 || h <= 0 || w > dt::MAX_DIM || h > dt::MAX_DIM) return -1;
    if (!(depth == 5 && (metric == dt::L1 || metric == dt::L2 || metric == dt::C)) && !(depth == 0 && metric == dt::L1)) return -1;
    std::vector<uint16_t> g;
    columns(src, sstep, w, h, g);
    if (depth == 0) rows<dt::L1, unsigned char>(g, w, h, dst, dstep);
    else if (metric == dt::L2) rows<dt::L2, float>(g, w, h, dst, dstep);
    else if (metric == dt::L1) rows<dt::L1, float>(g, w, h, dst, dstep);
    else rows<dt::C, float>(g, w, h, dst, dstep);
    return 0;
}

// the column pass alone: g as u16 [h][w], CAP = 32768 in a column without a site
extern "C" int emu_dist_columns(const unsigned char* src, size_t sstep, uint16_t* g, int w, int h)
{
    if (w <= 0 || h <= 0 || w > dt::MAX_DIM || h > dt::MAX_DIM) return -1;
    std::vector<uint16_t> v;
    columns(src, sstep, w, h, v);
    for (size_t i = 0; i < v.size(); i++) g[i] = v[i];
    return 0;
}

// root() over n exact squared distances
extern "C" void emu_dist_root(const uint32_t* d2, float* out, size_t n)
{
    for (size_t i = 0; i < n; i++) out[i] = dt::root(d2[i]);
}

extern "C" int emu_dist_seg(void) { return dt::SEG; }
extern "C" int emu_dist_max_dim(void) { return dt::MAX_DIM; }
extern "C" unsigned emu_dist_cap(void) { return dt::CAP; }
