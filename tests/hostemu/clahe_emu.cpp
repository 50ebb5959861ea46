// clahe_emu.cpp -- opencv_amd/csrc/clahe_math.h (the arithmetic of k_clahe_lut8 / 16 and k_clahe_interp8 / 16) compiled for the CPU with -ffp-contract=off:
// the per-bin clip / redistribution / LUT lines over a given histogram, and a whole CLAHE (plan, reflected tile reads, histograms, LUTs, per-pixel blend)
// run serially.  tests/test_clahe_cpu.py compares both with the numpy restatement (tests/clahe_restate.py).
// Test infrastructure.
#include "clahe_math.h"
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// lut[i] of one tile from its histogram; clip 0: no clipping
extern "C" void emu_clahe_lut(const int* hist, int histSize, int clip, float lutScale, int maxValue, int* lut)
{
    clahe::Redist r = {0, 0, 1};
    if (clip > 0) {
        int clipped = 0;
        for (int i = 0; i < histSize; i++) clipped += clahe::excess(hist[i], clip);
        r = clahe::redist(clipped, histSize);
    }
    int sum = 0;
    for (int i = 0; i < histSize; i++) {
        sum += clahe::binAfterClip(hist[i], i, clip, r);
        lut[i] = clahe::lutEntry(sum, lutScale, maxValue);
    }
}

namespace {
template <typename T>
void run(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int W, int H, const clahe::Plan& p, int histSize)
{
    const int nT = p.tilesX * p.tilesY, maxv = histSize - 1;
    auto at = [&](int y, int x) { return (int)((const T*)(src + (size_t)y * sstep))[x]; };
    std::vector<int> lut((size_t)nT * histSize), hist(histSize);
    for (int k = 0; k < nT; k++) {
        const int ty = k / p.tilesX, tx = k % p.tilesX;
        std::fill(hist.begin(), hist.end(), 0);
        for (int r = 0; r < p.th; r++)
            for (int c = 0; c < p.tw; c++) hist[at(clahe::reflect101(ty * p.th + r, p.readH), clahe::reflect101(tx * p.tw + c, p.readW))]++;
        emu_clahe_lut(hist.data(), histSize, p.clip, p.lutScale, maxv, lut.data() + (size_t)k * histSize);
    }
    const float invTw = 1.0f / (float)p.tw, invTh = 1.0f / (float)p.th;
    std::vector<T> row(W);
    for (int y = 0; y < H; y++) {
        const clahe::Axis ay = clahe::axis(y, invTh, p.tilesY);
        const int* L1 = lut.data() + (size_t)ay.t1 * p.tilesX * histSize;
        const int* L2 = lut.data() + (size_t)ay.t2 * p.tilesX * histSize;
        for (int x = 0; x < W; x++) {
            const int v = at(y, x);
            const clahe::Axis ax = clahe::axis(x, invTw, p.tilesX);
            const size_t t1 = (size_t)ax.t1 * histSize + v, t2 = (size_t)ax.t2 * histSize + v;
            row[x] = (T)clahe::blend(L1[t1], L1[t2], L2[t1], L2[t2], ax, ay, maxv);
        }
        for (int x = 0; x < W; x++) ((T*)(dst + (size_t)y * dstep))[x] = row[x];       // after the row is read: in place is allowed
    }
}
}

// depth 0: CV_8U, 2: CV_16U.  Returns -1 where the plan refuses the arguments.
extern "C" int emu_clahe(const unsigned char* src, size_t sstep, unsigned char* dst, size_t dstep, int W, int H, int depth, int marginRight, int marginBottom,
                         double clipLimit, int tilesX, int tilesY)
{
    const int histSize = depth == 0 ? 256 : 65536;
    clahe::Plan p;
    if ((depth != 0 && depth != 2) || !clahe::plan(W, H, marginRight, marginBottom, tilesX, tilesY, clipLimit, histSize, p)) return -1;
    if (depth == 0) run<uint8_t>(src, sstep, dst, dstep, W, H, p, histSize);
    else run<uint16_t>(src, sstep, dst, dstep, W, H, p, histSize);
    return 0;
}
