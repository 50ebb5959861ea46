// demosaic_emu.cpp -- opencv_amd/csrc/demosaic_math.h (the arithmetic of k_demosaic and k_demosaic_roll) compiled for the CPU: a whole demosaicing run serially
// through the per-pixel lines of k_demosaic for both depths, and through the four-pixels-per-dword lines of k_demosaic_roll for CV_8U (v_lerp_u8 and v_perm_b32
// by their definitions).  tests/test_demosaic_cpu.py compares both with the numpy restatement (tests/demosaic_restate.py).
// Test infrastructure.
#include "demosaic_math.h"
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {
template <typename T>
void run(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int w, int h, int dcn, int pattern)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int sx = demosaic::clampIdx(x, w), sy = demosaic::clampIdx(y, h);
            const T* r0 = (const T*)(src + (size_t)(sy - 1) * sstep) + sx;
            const T* r1 = (const T*)(src + (size_t)sy * sstep) + sx;
            const T* r2 = (const T*)(src + (size_t)(sy + 1) * sstep) + sx;
            const uint32_t c = r1[0], H = (uint32_t)r1[-1] + r1[1], V = (uint32_t)r0[0] + r2[0], D = (uint32_t)r0[-1] + r0[1] + r2[-1] + r2[1];
            const int green = demosaic::isGreen(pattern, sy, sx), rb = demosaic::rowBlue(pattern, sy);
            T* d = (T*)(dst + (size_t)y * dstep) + (size_t)x * dcn;
            if (dcn == 1) d[0] = (T)demosaic::gray(demosaic::grayWeights(green, rb), c, H, V, D);
            else {
                uint32_t b, g, r;
                demosaic::bgr(green, rb, c, H, V, D, b, g, r);
                d[0] = (T)b; d[1] = (T)g; d[2] = (T)r;
                if (dcn == 4) d[3] = (T)~(T)0;
            }
        }
}
}

// depth as in the C ABI: 0 CV_8U, 2 CV_16U; pattern 0..3 = BG, GB, RG, GR.  Returns -1 for anything the library declines.
extern "C" int emu_demosaic(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int w, int h, int depth, int dcn, int pattern)
{
    if (w < 3 || h < 3 || !(dcn == 1 || dcn == 3 || dcn == 4) || pattern < 0 || pattern > 3) return -1;
    if (depth == 0) run<uint8_t>(src, sstep, dst, dstep, w, h, dcn, pattern);
    else if (depth == 2) run<uint16_t>(src, sstep, dst, dstep, w, h, dcn, pattern);
    else return -1;
    return 0;
}

// CV_8U through the packed lines of k_demosaic_roll: per row and dword the pair sums and averages of the left / right neighbours, then per output row the
// planes (or the gray quad) from three such rows and the interleave; the border columns and rows are copies of finished pixels, as in the kernel
extern "C" int emu_demosaic_packed(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int w, int h, int dcn, int pattern)
{
    if (w < 3 || h < 3 || !(dcn == 1 || dcn == 3 || dcn == 4) || pattern < 0 || pattern > 3) return -1;
    const int nd = (w + 3) / 4;
    struct Row { std::vector<uint32_t> c, se, so, hl; };
    std::vector<Row> rows(h);
    for (int y = 0; y < h; y++) {
        std::vector<uint32_t> X(nd + 2, 0u);                                     // X[1 + k] = columns 4k .. 4k+3, zeros outside the row
        std::vector<unsigned char> padded(4 * (size_t)nd, 0);
        memcpy(padded.data(), src + (size_t)y * sstep, (size_t)w);
        for (int k = 0; k < nd; k++) X[1 + k] = padded[4 * k] | (padded[4 * k + 1] << 8) | (padded[4 * k + 2] << 16) | ((uint32_t)padded[4 * k + 3] << 24);
        Row& o = rows[y];
        o.c.resize(nd); o.se.resize(nd); o.so.resize(nd); o.hl.resize(nd);
        for (int k = 0; k < nd; k++) {
            const uint32_t l = demosaic::leftOf(X[k], X[k + 1]), r = demosaic::rightOf(X[k + 1], X[k + 2]);
            o.c[k] = X[k + 1]; o.se[k] = demosaic::sum2e(l, r); o.so[k] = demosaic::sum2o(l, r); o.hl[k] = demosaic::avg2(l, r);
        }
    }
    std::vector<unsigned char> line(4 * (size_t)nd * dcn);
    for (int y = 1; y <= h - 2; y++) {
        const Row &u = rows[y - 1], &m = rows[y], &d = rows[y + 1];
        const int ge = demosaic::greenEven(pattern, y), rb = demosaic::rowBlue(pattern, y);
        for (int k = 0; k < nd; k++) {
            uint32_t o[4];
            if (dcn == 1) {
                const demosaic::GrayW we = demosaic::grayWeights(ge, rb), wo = demosaic::grayWeights(ge ^ 1, rb);
                o[0] = demosaic::grayQuad(we, wo, m.c[k], m.se[k], m.so[k], demosaic::sum2e(u.c[k], d.c[k]), demosaic::sum2o(u.c[k], d.c[k]), u.se[k] + d.se[k], u.so[k] + d.so[k]);
            } else {
                uint32_t pb, pg, pr;
                const uint32_t v = demosaic::avg2(u.c[k], d.c[k]);
                const uint32_t hv = demosaic::avg4(m.se[k], m.so[k], demosaic::sum2e(u.c[k], d.c[k]), demosaic::sum2o(u.c[k], d.c[k]));
                const uint32_t dg = demosaic::avg4(u.se[k], u.so[k], d.se[k], d.so[k]);
                demosaic::planes(demosaic::greenMask(ge), rb, m.c[k], m.hl[k], v, hv, dg, pb, pg, pr);
                if (dcn == 3) { uint32_t t[3]; demosaic::interleave3(pb, pg, pr, t); o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; }
                else demosaic::interleave4(pb, pg, pr, o);
            }
            memcpy(&line[4 * (size_t)k * dcn], o, 4 * (size_t)dcn);          // little endian, like the device
        }
        unsigned char* drow = dst + (size_t)y * dstep;
        memcpy(drow + dcn, &line[dcn], (size_t)(w - 2) * dcn);
        memcpy(drow, drow + dcn, dcn);
        memcpy(drow + (size_t)(w - 1) * dcn, drow + (size_t)(w - 2) * dcn, dcn);
    }
    memcpy(dst, dst + dstep, (size_t)w * dcn);
    memcpy(dst + (size_t)(h - 1) * dstep, dst + (size_t)(h - 2) * dstep, (size_t)w * dcn);
    return 0;
}

extern "C" int emu_demosaic_gray_weights(unsigned* out) { out[0] = demosaic::KB; out[1] = demosaic::KG; out[2] = demosaic::KR; return 0; }
