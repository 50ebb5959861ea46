// ccl_math.h -- the arithmetic of connected-component labelling served by ccl.hip (cv::connectedComponents / connectedComponentsWithStats), shared by the
// kernels and by a host build of the same lines that the CPU test-suite checks against the numpy restatement (tests/hostemu/ccl_emu.cpp, tests/ccl_restate.py).
//
// A pixel is foreground iff it is non-zero.  A frame is cut into tiles of TILE_W = 256 columns x STRIP_H = 16 rows, one wave each.  A row of a tile is four
// 64-bit words, bit i of word j = column 64 j + i of the tile (a lane loads one dword = 4 pixels; the four ballots of its bytes are interleaved into the words by
// rowWord); lane i of the wave owns bit i of every word.
//   runs      a lane's horizontal run starts after the highest zero bit below it (runStart); a run that begins at bit 0 continues the run that ends at bit 63 of
//             the word to its left (tileRunStart).  The node of a pixel in the union-find is the first pixel of its run.
//   links     the pairs (run of this row, run of the row above) that touch: 4-connected, one per maximal run of W & P (linkDirect); 8-connected, W against P
//             widened by one bit each way with the carry bits of the neighbouring words (link8) -- cut into the direct pairs plus the purely diagonal ones
//             (linkLeft / linkRight), which names every touching pair at least once and few of them twice.
//   roots     the union-find keeps the SMALLEST linear pixel index as the root and parents only ever decrease, so the root of a component is its first raster
//             pixel whatever the interleaving of the unions.  Its find / unite loops are not here: they are unionfind.h's, which the kernels and the host build
//             both include.
//   order     components are numbered by a key of the component: its first pixel (ORDER_PIXEL), or its first 2 x 2 block, blockKey (ORDER_BLOCK).  The keys are
//             flags in a bitmap over key space; a label is 1 + the number of flags below the component's key (rank).
//   stats     per row, runs of equal label; a run [x, x + len) adds len to the area, runSumX to the sum of x and y * len to the sum of y.
// Bounds: width and height <= MAX_DIM = 16384, so a pixel index and an area fit 2^28 and a coordinate sum stays below 2^42 < 2^53: the centroid's double
// division sees two exactly represented integers.
#pragma once
#include "hd.h"

namespace ccl {

using mi355::clz64;
using mi355::ctz64;
using mi355::popc64;

enum { ORDER_PIXEL = 0, ORDER_BLOCK = 1 };
constexpr int TILE_W = 256;                       // columns of a tile = 64 lanes x 4 pixels
constexpr int STRIP_H = 16;                       // rows of a tile: merged in LDS
constexpr int WORDS = TILE_W / 64;
constexpr int MAX_DIM = 16384;                    // largest width and height served
constexpr uint32_t BG = 0xFFFFFFFFu;              // parent of a background pixel; "no key yet" in the block-key table
constexpr int CHUNK_WORDS = 256;                  // bitmap words per scan chunk

// the numbering a (connectivity, ccltype) pair of the reference yields; -1 for an unknown ccltype.  CCL_WU = 0 and CCL_SAUF = 3 create a provisional label at a
// component's first raster pixel; CCL_DEFAULT = -1, CCL_GRANA = 1, CCL_BOLELLI = 2, CCL_BBDT = 4 and CCL_SPAGHETTI = 5 scan 2 x 2 blocks when connectivity is 8
MI355_HD int orderOf(int connectivity, int ccltype)
{
    if (ccltype < -1 || ccltype > 5) return -1;
    if (connectivity == 4 || ccltype == 0 || ccltype == 3) return ORDER_PIXEL;
    return ORDER_BLOCK;
}

MI355_HD uint64_t below(int lane) { return (uint64_t(1) << lane) - 1; }             // the bits under `lane`, 0 <= lane < 64

// bit i of a 16-bit value to bit 4 i
MI355_HD uint64_t spread4(uint64_t v)
{
    v &= 0xffff;
    v = (v | (v << 24)) & 0x000000ff000000ffull;
    v = (v | (v << 12)) & 0x000f000f000f000full;
    v = (v | (v << 6)) & 0x0303030303030303ull;
    v = (v | (v << 3)) & 0x1111111111111111ull;
    return v;
}
// word j of a tile row from the four ballots of a dword-per-lane load: bit l of b[k] = pixel 4 l + k is non-zero
MI355_HD uint64_t rowWord(uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3, int j)
{
    const int s = 16 * j;
    return spread4(b0 >> s) | (spread4(b1 >> s) << 1) | (spread4(b2 >> s) << 2) | (spread4(b3 >> s) << 3);
}

// first bit of the run of ones that holds bit `lane` (which is set)
MI355_HD int runStart(uint64_t mask, int lane)
{
    const uint64_t z = ~mask & below(lane);
    return z ? 64 - clz64(z) : 0;
}
// one past its last bit
MI355_HD int runEnd(uint64_t mask, int lane)
{
    const uint64_t z = ~mask >> lane;
    return z ? lane + ctz64(z) : 64;
}
// column in the tile of the first pixel of the run that holds bit `lane` of word j: a run that reaches bit 0 goes on in the word to the left
MI355_HD int tileRunStart(const uint64_t* W, int j, int lane)
{
    int s = runStart(W[j], lane);
    while (s == 0 && j > 0 && (W[j - 1] >> 63)) { j--; s = runStart(W[j], 63); }
    return 64 * j + s;
}

MI355_HD uint64_t shl1(uint64_t v, uint64_t carry) { return (v << 1) | (carry & 1); }          // bit c = v's bit c - 1; carry = bit 63 of the word to the left
MI355_HD uint64_t shr1(uint64_t v, uint64_t carry) { return (v >> 1) | ((carry & 1) << 63); }  // bit c = v's bit c + 1; carry = bit 0 of the word to the right

// the pixels of W with an 8-connected neighbour in the row above: P widened by one bit each way
MI355_HD uint64_t link8(uint64_t W, uint64_t P, uint64_t Pl, uint64_t Pr) { return W & (P | shl1(P, Pl) | shr1(P, Pr)); }
// one bit per maximal run of W & P: each is one pair (run below, run above); Wl / Pl = bit 63 of the words to the left
MI355_HD uint64_t linkDirect(uint64_t W, uint64_t P, uint64_t Wl, uint64_t Pl)
{
    const uint64_t L = W & P;
    return L & ~shl1(L, Wl & Pl);
}
// pixel c joined to the pixel above-left only: above c is empty (else above-left is the run of above c, a direct pair) and c - 1 is empty (else c - 1 has
// that pixel right above it)
MI355_HD uint64_t linkLeft(uint64_t W, uint64_t P, uint64_t Wl, uint64_t Pl) { return W & shl1(P, Pl) & ~P & ~shl1(W, Wl); }
MI355_HD uint64_t linkRight(uint64_t W, uint64_t P, uint64_t Wr, uint64_t Pr) { return W & shr1(P, Pr) & ~P & ~shr1(W, Wr); }

// key of the 2 x 2 block of pixel (x, y) in a frame w wide
MI355_HD uint32_t blockKey(int x, int y, int w) { return (uint32_t)(y >> 1) * (uint32_t)((w + 1) >> 1) + (uint32_t)(x >> 1); }

// number of flags below position `pos`: chunk = exclusive scan of the flags per CHUNK_WORDS words, wpre = exclusive scan of the words inside their chunk
MI355_HD uint32_t rank(const uint32_t* chunk, const uint32_t* wpre, const uint64_t* bits, uint32_t pos)
{
    const uint32_t wi = pos >> 6;
    return chunk[wi / CHUNK_WORDS] + wpre[wi] + (uint32_t)popc64(bits[wi] & below(pos & 63));
}

// sum of x over the run [x, x + len)
MI355_HD uint64_t runSumX(uint32_t x, uint32_t len) { return (uint64_t)len * x + ((uint64_t)len * (len - 1) >> 1); }

// the accumulator of one label and what the finishing step makes of it
struct Acc { uint32_t area; int32_t minx, maxx, miny, maxy; uint32_t pad; unsigned long long sx, sy; };
MI355_HD Acc accEmpty() { Acc a; a.area = 0; a.minx = a.miny = 0x7fffffff; a.maxx = a.maxy = -1; a.pad = 0; a.sx = a.sy = 0; return a; }
// stats[5] = left, top, width, height, area; c[2] = centroid.  A label without a pixel: zeros and (NaN, NaN)
MI355_HD void accFinish(const Acc& a, int32_t* stats, double* c)
{
    if (a.area == 0) {
        stats[0] = stats[1] = stats[2] = stats[3] = stats[4] = 0;
        if (c) c[0] = c[1] = __builtin_nan("");
        return;
    }
    stats[0] = a.minx; stats[1] = a.miny; stats[2] = a.maxx - a.minx + 1; stats[3] = a.maxy - a.miny + 1; stats[4] = (int32_t)a.area;
    if (c) { c[0] = (double)a.sx / (double)a.area; c[1] = (double)a.sy / (double)a.area; }
}

} // namespace ccl
