// ccl_emu.cpp -- opencv_amd/csrc/ccl_math.h (the arithmetic of the kernels of ccl.hip) and unionfind.h (their find / unite loops, over its host memory policy)
// compiled for the CPU with -ffp-contract=off: a whole labelling run serially
// through the same lines and in the kernels' order -- row words from the four byte ballots of a tile row, run nodes, the links of every row to the row above
// merged per tile, the vertical and horizontal seams, flatten, the flags in pixel or block key space, the two-level scan, rank + 1 -- and the statistics from runs
// of equal label.  tests/test_ccl_cpu.py compares it with the numpy restatement (tests/ccl_restate.py).  Test infrastructure.
#include "ccl_math.h"
#include "unionfind.h"
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {
using ccl::BG; using ccl::STRIP_H; using ccl::TILE_W; using ccl::WORDS;

// k_ccl_strip for the tile at (x0, y0)
void strip(const unsigned char* src, size_t sstep, int w, int h, int conn8, int x0, int y0, std::vector<uint32_t>& P)
{
    const int rows = std::min(STRIP_H, h - y0);
    uint64_t wd[STRIP_H][WORDS];
    std::vector<uint32_t> par(STRIP_H * TILE_W, 0);
    for (int r = 0; r < rows; r++) {
        uint64_t b[4] = {0, 0, 0, 0};
        for (int lane = 0; lane < 64; lane++)
            for (int k = 0; k < 4; k++) { const int x = x0 + 4 * lane + k; if (x < w && src[(size_t)(y0 + r) * sstep + x]) b[k] |= uint64_t(1) << lane; }
        for (int j = 0; j < WORDS; j++) wd[r][j] = ccl::rowWord(b[0], b[1], b[2], b[3], j);
    }
    for (int r = 0; r < rows; r++)
        for (int j = 0; j < WORDS; j++)
            for (int lane = 0; lane < 64; lane++)
                if ((wd[r][j] >> lane) & 1) { const int c = 64 * j + lane; if (ccl::tileRunStart(wd[r], j, lane) == c) par[r * TILE_W + c] = r * TILE_W + c; }
    uf::PlainMem m{par.data()};
    for (int r = 1; r < rows; r++) {
        const uint64_t* W = wd[r]; const uint64_t* U = wd[r - 1];
        for (int j = 0; j < WORDS; j++) {
            const uint64_t Wl = j ? W[j - 1] >> 63 : 0, Ul = j ? U[j - 1] >> 63 : 0, Wr = j + 1 < WORDS ? W[j + 1] & 1 : 0, Ur = j + 1 < WORDS ? U[j + 1] & 1 : 0;
            const uint64_t direct = ccl::linkDirect(W[j], U[j], Wl, Ul);
            const uint64_t left = conn8 ? ccl::linkLeft(W[j], U[j], Wl, Ul) : 0, right = conn8 ? ccl::linkRight(W[j], U[j], Wr, Ur) : 0;
            for (int lane = 0; lane < 64; lane++) {
                if (!(((direct | left | right) >> lane) & 1)) continue;
                const uint32_t a = r * TILE_W + ccl::tileRunStart(W, j, lane);
                if ((direct >> lane) & 1) uf::unite(m, a, (r - 1) * TILE_W + ccl::tileRunStart(U, j, lane));
                if ((left >> lane) & 1) { const int c = 64 * j + lane - 1; uf::unite(m, a, (r - 1) * TILE_W + ccl::tileRunStart(U, c >> 6, c & 63)); }
                if ((right >> lane) & 1) { const int c = 64 * j + lane + 1; uf::unite(m, a, (r - 1) * TILE_W + ccl::tileRunStart(U, c >> 6, c & 63)); }
            }
        }
    }
    for (int r = 0; r < rows; r++)
        for (int j = 0; j < WORDS; j++)
            for (int lane = 0; lane < 64; lane++) {
                const int x = x0 + 64 * j + lane;
                if (x >= w) continue;
                uint32_t p = BG;
                if ((wd[r][j] >> lane) & 1) {
                    const uint32_t root = uf::find(m, r * TILE_W + ccl::tileRunStart(wd[r], j, lane));
                    p = (uint32_t)(y0 + (int)(root / TILE_W)) * (uint32_t)w + (uint32_t)(x0 + (int)(root % TILE_W));
                }
                P[(size_t)(y0 + r) * w + x] = p;
            }
}

void vseam(std::vector<uint32_t>& P, int w, int h, int conn8, int x)
{
    uf::PlainMem m{P.data()};
    for (int y = 0; y < h; y++) {
        const uint32_t b = (uint32_t)y * w + x, a = b - 1;
        const bool fa = m.load(a) != BG, fb = m.load(b) != BG;
        if (fa && fb) uf::unite(m, a, b);
        if (conn8 && y > 0) {
            if (fa && m.load(b - w) != BG) uf::unite(m, a, b - w);
            if (fb && m.load(a - w) != BG) uf::unite(m, b, a - w);
        }
    }
}

void hseam(std::vector<uint32_t>& P, int w, int conn8, int x0, int y)
{
    uf::PlainMem m{P.data()};
    const uint32_t* cur = &P[(size_t)y * w]; const uint32_t* up = cur - w;
    uint64_t W[WORDS + 2], U[WORDS + 2];
    W[0] = x0 > 0 && cur[x0 - 1] != BG ? ~uint64_t(0) : 0; U[0] = x0 > 0 && up[x0 - 1] != BG ? ~uint64_t(0) : 0;
    W[WORDS + 1] = x0 + TILE_W < w && cur[x0 + TILE_W] != BG; U[WORDS + 1] = x0 + TILE_W < w && up[x0 + TILE_W] != BG;
    for (int j = 0; j < WORDS; j++) {
        W[j + 1] = U[j + 1] = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int x = x0 + 64 * j + lane;
            if (x < w && cur[x] != BG) W[j + 1] |= uint64_t(1) << lane;
            if (x < w && up[x] != BG) U[j + 1] |= uint64_t(1) << lane;
        }
    }
    for (int j = 1; j <= WORDS; j++) {
        const uint64_t Wl = W[j - 1] >> 63, Ul = U[j - 1] >> 63, Wr = W[j + 1] & 1, Ur = U[j + 1] & 1;
        const uint64_t direct = ccl::linkDirect(W[j], U[j], Wl, Ul);
        const uint64_t left = conn8 ? ccl::linkLeft(W[j], U[j], Wl, Ul) : 0, right = conn8 ? ccl::linkRight(W[j], U[j], Wr, Ur) : 0;
        for (int lane = 0; lane < 64; lane++) {
            const uint32_t a = (uint32_t)y * w + x0 + 64 * (j - 1) + lane;
            if ((direct >> lane) & 1) uf::unite(m, a, a - w);
            if ((left >> lane) & 1) uf::unite(m, a, a - w - 1);
            if ((right >> lane) & 1) uf::unite(m, a, a - w + 1);
        }
    }
}
}

// labels: int32, dense (w per row).  Returns N, or -1 for arguments that are not served.
extern "C" int emu_ccl(const unsigned char* src, size_t sstep, int w, int h, int connectivity, int ccltype, int32_t* labels)
{
    const int order = ccl::orderOf(connectivity, ccltype);
    if (w <= 0 || h <= 0 || w > ccl::MAX_DIM || h > ccl::MAX_DIM || (connectivity != 4 && connectivity != 8) || order < 0) return -1;
    const int conn8 = connectivity == 8, ntx = (w + TILE_W - 1) / TILE_W, nstrips = (h + STRIP_H - 1) / STRIP_H;
    std::vector<uint32_t> P((size_t)w * h, 0);
    for (int ty = 0; ty < nstrips; ty++) for (int tx = 0; tx < ntx; tx++) strip(src, sstep, w, h, conn8, tx * TILE_W, ty * STRIP_H, P);
    for (int k = 1; k < ntx; k++) vseam(P, w, h, conn8, k * TILE_W);
    for (int s = 1; s < nstrips; s++) for (int tx = 0; tx < ntx; tx++) hseam(P, w, conn8, tx * TILE_W, s * STRIP_H);
    // flatten and flags
    const uint32_t nblocks = (uint32_t)((h + 1) >> 1) * (uint32_t)((w + 1) >> 1), npos = order == ccl::ORDER_BLOCK ? nblocks : (uint32_t)w * h;
    const uint32_t nW = (npos + 63) >> 6, nchunk = (nW + ccl::CHUNK_WORDS - 1) / ccl::CHUNK_WORDS;
    std::vector<uint64_t> B(nW, 0);
    std::vector<uint32_t> K(order == ccl::ORDER_BLOCK ? nblocks : 0, BG), wpre(nW), chunk(nchunk);
    uf::PlainMem m{P.data()};
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t g = (uint32_t)y * w + x;
            if (P[g] == BG) continue;
            const uint32_t r = uf::find(m, m.load(g));
            P[g] = r;
            if (order == ccl::ORDER_PIXEL) { if (r == g) B[g >> 6] |= uint64_t(1) << (g & 63); }
            else if (r >= (uint32_t)(y & ~1) * w && ((x & 63) == 0 || P[g - 1] == BG)) {       // the first pixel of a run inside its 64-column word
                const int ry = r / (uint32_t)w, rx = r - ry * w;
                uint32_t& k = K[ccl::blockKey(rx, ry, w)];
                k = std::min(k, ccl::blockKey(x, y, w));
            }
        }
    for (uint32_t b = 0; b < K.size(); b++) if (K[b] != BG) B[K[b] >> 6] |= uint64_t(1) << (K[b] & 63);
    uint32_t total = 0;
    for (uint32_t c = 0; c < nchunk; c++) {
        uint32_t in = 0;
        for (uint32_t i = c * ccl::CHUNK_WORDS; i < std::min(nW, (c + 1) * ccl::CHUNK_WORDS); i++) { wpre[i] = in; in += ccl::popc64(B[i]); }
        chunk[c] = total; total += in;
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint32_t p = P[(size_t)y * w + x];
            uint32_t lab = 0;
            if (p != BG) {
                uint32_t pos = p;
                if (order == ccl::ORDER_BLOCK) { const int py = p / (uint32_t)w, px = p - py * w; pos = K[ccl::blockKey(px, py, w)]; }
                lab = ccl::rank(chunk.data(), wpre.data(), B.data(), pos) + 1;
            }
            labels[(size_t)y * w + x] = (int32_t)lab;
        }
    return (int)total + 1;
}

// k_ccl_stats_init + k_ccl_stats + k_ccl_stats_finish over a dense int32 label image; stats: n x 5 int32, centroids: n x 2 double
extern "C" int emu_ccl_stats(const int32_t* labels, int w, int h, int n, int32_t* stats, double* centroids)
{
    if (w <= 0 || h <= 0 || n < 1) return -1;
    std::vector<ccl::Acc> acc(n, ccl::accEmpty());
    for (int y = 0; y < h; y++)
        for (int x0 = 0; x0 < w; x0 += 64) {
            uint64_t V = 0, E = 0;
            for (int lane = 0; lane < 64 && x0 + lane < w; lane++) {
                V |= uint64_t(1) << lane;
                if (lane == 0 || labels[(size_t)y * w + x0 + lane] != labels[(size_t)y * w + x0 + lane - 1]) E |= uint64_t(1) << lane;
            }
            for (int lane = 0; lane < 64; lane++) {
                if (!((E >> lane) & 1)) continue;
                const uint32_t v = (uint32_t)labels[(size_t)y * w + x0 + lane];
                if (v >= (uint32_t)n) continue;
                const uint64_t above = lane < 63 ? E >> (lane + 1) : 0;
                const uint32_t len = above ? (uint32_t)ccl::ctz64(above) + 1 : (uint32_t)(ccl::popc64(V) - lane);
                const int x = x0 + lane;
                ccl::Acc& a = acc[v];
                a.area += len; a.sx += ccl::runSumX((uint32_t)x, len); a.sy += (unsigned long long)y * len;
                a.minx = std::min(a.minx, x); a.maxx = std::max(a.maxx, (int)(x + len - 1)); a.miny = std::min(a.miny, y); a.maxy = std::max(a.maxy, y);
            }
        }
    for (int i = 0; i < n; i++) ccl::accFinish(acc[i], stats + 5 * i, centroids ? centroids + 2 * i : nullptr);
    return 0;
}

extern "C" int emu_ccl_run_start(uint64_t mask, int lane) { return ccl::runStart(mask, lane); }
extern "C" int emu_ccl_run_end(uint64_t mask, int lane) { return ccl::runEnd(mask, lane); }
extern "C" int emu_ccl_tile_run_start(const uint64_t* W, int j, int lane) { return ccl::tileRunStart(W, j, lane); }
extern "C" uint64_t emu_ccl_row_word(uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3, int j) { return ccl::rowWord(b0, b1, b2, b3, j); }
extern "C" uint64_t emu_ccl_link8(uint64_t W, uint64_t P, int Pl, int Pr) { return ccl::link8(W, P, Pl, Pr); }
extern "C" uint64_t emu_ccl_link_direct(uint64_t W, uint64_t P, int Wl, int Pl) { return ccl::linkDirect(W, P, Wl, Pl); }
extern "C" uint64_t emu_ccl_link_left(uint64_t W, uint64_t P, int Wl, int Pl) { return ccl::linkLeft(W, P, Wl, Pl); }
extern "C" uint64_t emu_ccl_link_right(uint64_t W, uint64_t P, int Wr, int Pr) { return ccl::linkRight(W, P, Wr, Pr); }
extern "C" uint64_t emu_ccl_run_sum_x(uint32_t x, uint32_t len) { return ccl::runSumX(x, len); }
extern "C" uint32_t emu_ccl_block_key(int x, int y, int w) { return ccl::blockKey(x, y, w); }
extern "C" int emu_ccl_order_of(int connectivity, int ccltype) { return ccl::orderOf(connectivity, ccltype); }
extern "C" int emu_ccl_tile_w(void) { return TILE_W; }
extern "C" int emu_ccl_strip_h(void) { return STRIP_H; }
extern "C" int emu_ccl_max_dim(void) { return ccl::MAX_DIM; }
