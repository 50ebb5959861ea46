// pyrup_emu.cpp -- opencv_amd/csrc/pyrup_math.h (the arithmetic of k_pyrup and k_pyrup_roll) compiled for the CPU with -ffp-contract=off: a whole pyrUp run
// serially through the per-element block of k_pyrup for every depth, and through the packed 2 x u16 sums of k_pyrup_roll for CV_8UC1.
// tests/test_pyrup_cpu.py compares both with the numpy restatement (tests/pyrup_restate.py).
// Test infrastructure.
#include "pyrup_math.h"
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

namespace {
template <typename T, typename W>
void run(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int w, int h, int cn)
{
    for (int y = 0; y < h; y++)
        for (int e = 0; e < w * cn; e++) {
            const int x = e / cn, c = e - x * cn;
            const int xs[3] = {pyrup::lowIdx(x - 1, w) * cn + c, e, pyrup::highIdx(x + 1, w) * cn + c};
            const int ys[3] = {pyrup::lowIdx(y - 1, h), y, pyrup::highIdx(y + 1, h)};
            W s[3][3], o[4];
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) s[r][k] = (W)((const T*)(src + (size_t)ys[r] * sstep))[xs[k]];
            pyrup::block<W>(s, o);
            T* d0 = (T*)(dst + (size_t)(2 * y) * dstep) + (size_t)(2 * x) * cn + c;
            T* d1 = (T*)(dst + (size_t)(2 * y + 1) * dstep) + (size_t)(2 * x) * cn + c;
            if constexpr (std::is_same<W, float>::value) {
                d0[0] = pyrup::castFlt(o[0]); d0[cn] = pyrup::castFlt(o[1]); d1[0] = pyrup::castFlt(o[2]); d1[cn] = pyrup::castFlt(o[3]);
            } else {
                d0[0] = (T)pyrup::castInt(o[0]); d0[cn] = (T)pyrup::castInt(o[1]); d1[0] = (T)pyrup::castInt(o[2]); d1[cn] = (T)pyrup::castInt(o[3]);
            }
        }
}
}

// depth as in the C ABI: 0 CV_8U, 2 CV_16U, 3 CV_16S, 5 CV_32F.  Returns -1 for anything else.
extern "C" int emu_pyrup(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int w, int h, int depth, int cn)
{
    if (w <= 0 || h <= 0 || cn < 1 || cn > 4) return -1;
    if (depth == 0) run<uint8_t, int>(src, sstep, dst, dstep, w, h, cn);
    else if (depth == 2) run<uint16_t, int>(src, sstep, dst, dstep, w, h, cn);
    else if (depth == 3) run<int16_t, int>(src, sstep, dst, dstep, w, h, cn);
    else if (depth == 5) run<float, float>(src, sstep, dst, dstep, w, h, cn);
    else return -1;
    return 0;
}

// CV_8UC1 through the packed pairs of k_pyrup_roll: rows of hpair, then vEven / vOdd down the columns
extern "C" int emu_pyrup_packed(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int w, int h)
{
    if (w <= 0 || h <= 0) return -1;
    std::vector<uint32_t> hs((size_t)w * h);
    for (int y = 0; y < h; y++) {
        const unsigned char* r = src + (size_t)y * sstep;
        for (int x = 0; x < w; x++) hs[(size_t)y * w + x] = pyrup::hpair(r[pyrup::lowIdx(x - 1, w)], r[x], r[pyrup::highIdx(x + 1, w)]);
    }
    for (int y = 0; y < h; y++) {
        const uint32_t* h0 = &hs[(size_t)pyrup::lowIdx(y - 1, h) * w];
        const uint32_t* h1 = &hs[(size_t)y * w];
        const uint32_t* h2 = &hs[(size_t)pyrup::highIdx(y + 1, h) * w];
        unsigned char* d0 = dst + (size_t)(2 * y) * dstep;
        unsigned char* d1 = d0 + dstep;
        for (int x = 0; x < w; x++) {
            const uint32_t e = pyrup::vEven(h0[x], h1[x], h2[x]), o = pyrup::vOdd(h1[x], h2[x]);
            d0[2 * x] = (unsigned char)e; d0[2 * x + 1] = (unsigned char)(e >> 16);
            d1[2 * x] = (unsigned char)o; d1[2 * x + 1] = (unsigned char)(o >> 16);
        }
    }
    return 0;
}
