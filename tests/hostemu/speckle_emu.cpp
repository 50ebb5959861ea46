// speckle_emu.cpp -- opencv_amd/csrc/speckle_math.h (the pieces of the kernels of speckle.hip) and unionfind.h (their find / unite loops, over its host memory
// policy) compiled for the CPU, and the whole kernel sequence of either path
// emulated serially around them -- k_spk_init / k_spk_link / k_spk_count, or k_spk_tile (ballots, bit planes, runs, the merge in LDS) / k_spk_vseam / k_spk_hseam /
// k_spk_count_runs, then k_spk_erase -- for tests/test_speckle_cpu.py to hold against tests/speckle_restate.py bit for bit.  `stride` permutes the order in which the
// emulated threads of a kernel run (thread i runs as (i * stride) mod n, gcd(stride, n) = 1): the image must not depend on it.
#include "speckle_math.h"
#include <stddef.h>
#include <vector>

namespace {

using uf::PlainMem;

struct Img {
    uint8_t* p; size_t step; int w, h, is16;
    int at(int y, int x) const { return is16 ? (int)*(const int16_t*)(p + (size_t)y * step + (size_t)x * 2) : (int)p[(size_t)y * step + x]; }
    void set(int y, int x, int v) const { if (is16) *(int16_t*)(p + (size_t)y * step + (size_t)x * 2) = (int16_t)v; else p[(size_t)y * step + x] = (uint8_t)v; }
};

size_t gcd(size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }
// the i-th thread to run of n
size_t perm(size_t i, size_t n, size_t stride) { return gcd(stride, n) == 1 ? (i * stride) % n : i; }

void plainPath(const Img& I, int newVal, int maxDiff, std::vector<uint32_t>& P, std::vector<uint32_t>& C, size_t stride)
{
    const int w = I.w, h = I.h;
    const size_t n = (size_t)w * h;
    for (size_t g = 0; g < n; g++) { P[g] = spk::live(I.at((int)(g / w), (int)(g % w)), newVal) ? (uint32_t)g : spk::DEAD; C[g] = 0; }
    PlainMem m{P.data()};
    for (size_t i = 0; i < n; i++) {
        const size_t g = perm(i, n, stride);
        const int y = (int)(g / w), x = (int)(g % w), v = I.at(y, x);
        if (!spk::live(v, newVal)) continue;
        if (x > 0) { const int a = I.at(y, x - 1); if (spk::live(a, newVal) && spk::linked(v, a, maxDiff)) spk::unite(m, (uint32_t)g, (uint32_t)g - 1); }
        if (y > 0) { const int a = I.at(y - 1, x); if (spk::live(a, newVal) && spk::linked(v, a, maxDiff)) spk::unite(m, (uint32_t)g, (uint32_t)(g - w)); }
    }
    for (size_t i = 0; i < n; i++) {
        const size_t g = perm(i, n, stride);
        if (P[g] == spk::DEAD) continue;
        const uint32_t r = spk::find(m, P[g]);
        P[g] = r;
        C[r] += 1;
    }
}

void tile(const Img& I, int newVal, int maxDiff, int x0, int y0, uint32_t* P, uint32_t* C, size_t stride)
{
    using namespace spk;
    const int w = I.w, rows = (I.h - y0 < STRIP_H) ? I.h - y0 : STRIP_H;
    std::vector<uint32_t> par((size_t)STRIP_H * TILE_W, 0xdeadbeefu);
    uint64_t wd[3][STRIP_H][WORDS] = {}, st[STRIP_H][WORDS] = {};
    for (int r = 0; r < rows; r++) {
        uint64_t b[3][4] = {};                                               // the ballots: bit l of b[q][k] = plane q of pixel 4 l + k
        for (int lane = 0; lane < 64; lane++)
            for (int k = 0; k < 4; k++) {
                const int x = x0 + 4 * lane + k, y = y0 + r;
                if (x >= w) continue;
                const int v = I.at(y, x);
                if (!live(v, newVal)) continue;
                b[0][k] |= uint64_t(1) << lane;
                if (4 * lane + k > 0) { const int a = I.at(y, x - 1); if (live(a, newVal) && linked(v, a, maxDiff)) b[1][k] |= uint64_t(1) << lane; }
                if (r > 0) { const int a = I.at(y - 1, x); if (live(a, newVal) && linked(v, a, maxDiff)) b[2][k] |= uint64_t(1) << lane; }
            }
        for (int q = 0; q < 3; q++)
            for (int j = 0; j < WORDS; j++) wd[q][r][j] = ccl::rowWord(b[q][0], b[q][1], b[q][2], b[q][3], j);
        for (int j = 0; j < WORDS; j++) st[r][j] = wd[0][r][j] & ~wd[1][r][j];
    }
    for (int r = 0; r < rows; r++)
        for (int j = 0; j < WORDS; j++)
            for (int lane = 0; lane < 64; lane++)
                if ((st[r][j] >> lane) & 1) { const int c = r * TILE_W + 64 * j + lane; par[c] = c; }
    PlainMem m{par.data()};
    const size_t nth = (size_t)(rows > 1 ? rows - 1 : 0) * WORDS * 64;
    for (size_t i = 0; i < nth; i++) {
        const size_t t = perm(i, nth, stride);
        const int lane = (int)(t % 64), j = (int)(t / 64 % WORDS), r = 1 + (int)(t / 64 / WORDS);
        const uint64_t d = upDirect(wd[2][r][j], wd[1][r][j], wd[1][r - 1][j], j ? wd[2][r][j - 1] >> 63 : 0);
        if ((d >> lane) & 1) unite(m, (uint32_t)(r * TILE_W + runStartOf(st[r], j, lane)), (uint32_t)((r - 1) * TILE_W + runStartOf(st[r - 1], j, lane)));
    }
    for (int r = 0; r < rows; r++)
        for (int j = 0; j < WORDS; j++)
            for (int lane = 0; lane < 64; lane++) {
                const int x = x0 + 64 * j + lane;
                if (x >= w) continue;
                uint32_t p = DEAD;
                if ((wd[0][r][j] >> lane) & 1) {
                    const uint32_t root = find(m, (uint32_t)(r * TILE_W + runStartOf(st[r], j, lane)));
                    p = (uint32_t)(y0 + (int)(root / TILE_W)) * (uint32_t)w + (uint32_t)(x0 + (int)(root % TILE_W));
                }
                const size_t g = (size_t)(y0 + r) * w + x;
                P[g] = p; C[g] = 0;
            }
}

void fastPath(const Img& I, int newVal, int maxDiff, std::vector<uint32_t>& P, std::vector<uint32_t>& C, size_t stride)
{
    using namespace spk;
    const int w = I.w, h = I.h, ntx = (w + TILE_W - 1) / TILE_W, nstrips = (h + STRIP_H - 1) / STRIP_H;
    for (int ty = 0; ty < nstrips; ty++)
        for (int tx = 0; tx < ntx; tx++) tile(I, newVal, maxDiff, tx * TILE_W, ty * STRIP_H, P.data(), C.data(), stride);
    PlainMem m{P.data()};
    const size_t nv = (size_t)h * (ntx - 1);
    for (size_t i = 0; i < nv; i++) {                                         // k_spk_vseam
        const size_t t = perm(i, nv, stride);
        const int y = (int)(t % h), x = ((int)(t / h) + 1) * TILE_W;
        const int a = I.at(y, x - 1), b = I.at(y, x);
        if (!live(a, newVal) || !live(b, newVal) || !linked(a, b, maxDiff)) continue;
        const uint32_t g = (uint32_t)y * w + x;
        unite(m, g, g - 1);
    }
    const size_t nh = (size_t)w * (nstrips - 1);
    for (size_t i = 0; i < nh; i++) {                                         // k_spk_hseam
        const size_t t = perm(i, nh, stride);
        const int x = (int)(t % w), y = ((int)(t / w) + 1) * STRIP_H;
        const int a = I.at(y - 1, x), b = I.at(y, x);
        if (!live(a, newVal) || !live(b, newVal) || !linked(a, b, maxDiff)) continue;
        const uint32_t g = (uint32_t)y * w + x;
        unite(m, g, g - w);
    }
    for (int y = 0; y < h; y++)                                               // k_spk_count_runs: a wave per 64 columns of a row
        for (int xw = 0; xw < ntx * TILE_W; xw += 64) {
            uint32_t r[64]; bool lv[64]; uint64_t cont = 0;
            for (int lane = 0; lane < 64; lane++) {
                const int x = xw + lane;
                const uint32_t g = (uint32_t)y * w + x;
                const uint32_t p = x < w ? P[g] : DEAD;
                lv[lane] = p != DEAD; r[lane] = DEAD;
                if (lv[lane]) { r[lane] = find(m, p); P[g] = r[lane]; }
            }
            for (int lane = 1; lane < 64; lane++) if (lv[lane] && r[lane] == r[lane - 1]) cont |= uint64_t(1) << lane;
            for (int lane = 0; lane < 64; lane++) if (lv[lane] && !((cont >> lane) & 1)) C[r[lane]] += runLen(cont, lane);
        }
}

} // namespace

// img: h rows of w elements at pitch `step` bytes, filtered in place.  fast: 0 the plain kernels, 1 the tile path
extern "C" void emu_spk_filter(uint8_t* img, size_t step, int w, int h, int is16, int newVal, int maxSpeckleSize, int maxDiff, int fast, int stride)
{
    const Img I{img, step, w, h, is16};
    std::vector<uint32_t> P((size_t)w * h), C((size_t)w * h, 0x55555555u);    // the counters start dirty: scratch is reused between calls
    if (fast) fastPath(I, newVal, maxDiff, P, C, (size_t)stride); else plainPath(I, newVal, maxDiff, P, C, (size_t)stride);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t p = P[(size_t)y * w + x];
            if (spk::erased(p != spk::DEAD, p != spk::DEAD ? C[p] : 0u, maxSpeckleSize)) I.set(y, x, newVal);
        }
}

extern "C" int emu_spk_linked(int a, int b, int maxDiff) { return spk::linked(a, b, maxDiff); }
extern "C" int emu_spk_fits(int newVal, int is16) { return spk::fitsDepth(newVal, is16 != 0); }
extern "C" int emu_spk_runlen(unsigned long long cont, int lane) { return (int)spk::runLen(cont, lane); }
extern "C" int emu_spk_limit(int i) { const int v[3] = {spk::MAX_DIM, spk::TILE_W, spk::STRIP_H}; return i >= 0 && i < 3 ? v[i] : -1; }
