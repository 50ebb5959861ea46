// speckle_math.h -- the pieces of speckle.hip (cv::filterSpeckles) that can be wrong, __host__ __device__ so that the CPU suite compiles the very same lines
// (tests/hostemu/speckle_emu.cpp) and holds them against tests/speckle_restate.py bit for bit.  The definition is the project's restatement.
//
//   live      a pixel is live iff its value != newVal
//   linked    two live 4-neighbours are linked iff |a - b| <= maxDiff, in int: a CV_16S difference reaches 65535 and does not wrap; maxDiff < 0 links nothing
//   roots     a union-find over pixels whose root is the SMALLEST linear pixel index of the set, parents only ever decrease.  It is unionfind.h's find / unite over
//             a memory policy (agent-scope loads and atomicMin on HBM, atomicMin on LDS, plain loads and stores in the host build), the one ccl.hip merges
//             with; the bit helpers and the tile geometry are ccl_math.h's, shared, not copied
//   tile      the fast kernel cuts a frame into tiles of TILE_W x STRIP_H.  Per row three bit planes: live, link-left (pixel c is linked to c - 1 of the same tile
//             row; never set in column 0 of a tile) and link-up (linked to the pixel above; never set in row 0 of a tile).  A run starts at a live pixel whose
//             link-left bit is 0 (runStartOf); the node of a pixel is the first pixel of its run.  upDirect keeps one link-up bit per pair (run, run above).
//   sizes     a component's size is added at its root, one add of runLen per run of equal root inside 64 columns of a row (fast) or one per pixel (plain)
//   erase     a live pixel of a component with size <= maxSpeckleSize becomes newVal (erased); maxSpeckleSize <= 0 erases nothing since a size is >= 1
#pragma once
#include "ccl_math.h"
#include "unionfind.h"

namespace spk {

constexpr int TILE_W = ccl::TILE_W;              // mi355cv_limit("speckle_tile_cols"): 64 lanes x 4 pixels
constexpr int STRIP_H = ccl::STRIP_H;            // ("speckle_tile_rows"): rows of a tile, merged in LDS
constexpr int WORDS = ccl::WORDS;
constexpr int MAX_DIM = 16384;                   // ("speckle_max_dim"): a pixel index and a component size stay below 2^28
constexpr uint32_t DEAD = ccl::BG;               // parent of a pixel that is not live
using uf::find;                                  // spk::find / spk::unite are unionfind.h's
using uf::unite;

MI355_HD bool live(int v, int newVal) { return v != newVal; }
MI355_HD bool linked(int a, int b, int maxDiff) { const int d = a - b; return (d < 0 ? -d : d) <= maxDiff; }
MI355_HD bool erased(bool isLive, uint32_t size, int maxSpeckleSize) { return isLive && (long long)size <= (long long)maxSpeckleSize; }
// newVal as the depth stores it
MI355_HD bool fitsDepth(int newVal, bool is16s) { return is16s ? (newVal >= -32768 && newVal <= 32767) : (newVal >= 0 && newVal <= 255); }

// S = live & ~link-left, the run starts of a tile row; (j, lane) is a live pixel: the column in the tile of the first pixel of its run
MI355_HD int runStartOf(const uint64_t* S, int j, int lane)
{
    uint64_t m = S[j] & (ccl::below(lane) | (uint64_t(1) << lane));
    while (!m && j > 0) { j--; m = S[j]; }                  // column 0 of a tile never has its link-left bit set: the walk ends inside the tile
    return m ? 64 * j + 63 - ccl::clz64(m) : 0;
}
// of the link-up bits LU of a row the one per pair (run, run above): bit c goes when c - 1 has its bit too and c is linked left in both rows.
// carry = bit 63 of LU of the word to the left
MI355_HD uint64_t upDirect(uint64_t LU, uint64_t LLrow, uint64_t LLabove, uint64_t carry) { return LU & ~(ccl::shl1(LU, carry) & LLrow & LLabove); }
// cont: bit l = lane l goes on the run of lane l - 1.  The length of the run that starts at `lane`, inside the 64 lanes
MI355_HD uint32_t runLen(uint64_t cont, int lane)
{
    if (lane >= 63) return 1;
    const uint64_t z = ~cont >> (lane + 1);
    return 1 + (uint32_t)(z ? ccl::ctz64(z) : 63 - lane);
}

} // namespace spk
