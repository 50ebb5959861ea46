// pyrup_math.h -- the arithmetic of cv::pyrUp (imgproc/src/pyramids.cpp, pyrUp_<CastOp>), shared by the kernels of pyrup.hip and by a host build of the
// same lines that the CPU test-suite checks against the numpy restatement (tests/hostemu/pyrup_emu.cpp, tests/pyrup_restate.py).
//
// cv::pyrUp inserts the source pixels at the even positions of a (2w x 2h) image and convolves with the 5 x 5 kernel that is [1 4 6 4 1] / 8 per axis.
// Separable, in the wide type W (int for 8U / 16U / 16S, float for 32F); per axis, for a source line s[0..n-1]:
//     s[-1] := s[min(1, n-1)]   (reflect-101 at the low edge)        s[n] := s[n-1]   (replicate at the high edge)
//     even output 2i   : e = s[i-1] + s[i]*6 + s[i+1]
//     odd  output 2i+1 : o = (s[i] + s[i+1])*4
// rows first (into wide rows), then the same two formulas down the columns of the wide rows, then the cast: (v + 32) >> 6 for the integers (an arithmetic
// shift on the signed int, no saturation needed: the result is a rounded convex combination), v * (1.f/64) for float.  Channels are independent.
//   lowIdx / highIdx    the two edge rules as indices
//   even / odd          the two formulas in the wide type, every float operation rounded separately (the library builds with -ffp-contract=off)
//   castInt / castFlt   the casts
//   block               the 2 x 2 destination block of one source element from its 3 x 3 neighbourhood (k_pyrup)
//   hpair / vEven / vOdd  the same sums on packed 2 x u16 pairs for CV_8U (k_pyrup_roll): horizontal sums <= 8 * 255, vertical sums <= 64 * 255 + 32,
//                       so neither half ever carries into the other
#pragma once
#include <stdint.h>

#include "hd.h"

// (a << n) + b: pyrup.hip maps it to one v_lshl_add_u32 in device code (rt.h lshlAdd); the value is the same
#ifndef PYRUP_LSHL_ADD
#  define PYRUP_LSHL_ADD(a, n, b) (((a) << (n)) + (b))
#endif

namespace pyrup {

MI355_HD int lowIdx(int i, int n) { return i >= 0 ? i : (n > 1 ? 1 : 0); }       // index of s[i], i >= -1
MI355_HD int highIdx(int i, int n) { return i < n ? i : n - 1; }                 // index of s[i], i <= n

template <typename W> MI355_HD W even(W a, W b, W c) { return a + b * (W)6 + c; }
template <typename W> MI355_HD W odd(W b, W c) { return (b + c) * (W)4; }

MI355_HD int castInt(int v) { return (v + 32) >> 6; }
MI355_HD float castFlt(float v) { return v * (1.f / 64); }

// s[r][c]: the 3 x 3 neighbourhood of source element (y, x) with the edge rules applied (r, c = 0: y-1 / x-1, 1: y / x, 2: y+1 / x+1);
// out[0..3] = wide sums of destination (2y, 2x), (2y, 2x+1), (2y+1, 2x), (2y+1, 2x+1), before the cast
template <typename W> MI355_HD void block(const W (&s)[3][3], W (&out)[4])
{
    W he[3], ho[3];
    for (int r = 0; r < 3; r++) { he[r] = even<W>(s[r][0], s[r][1], s[r][2]); ho[r] = odd<W>(s[r][1], s[r][2]); }
    out[0] = even<W>(he[0], he[1], he[2]); out[1] = even<W>(ho[0], ho[1], ho[2]);
    out[2] = odd<W>(he[1], he[2]);         out[3] = odd<W>(ho[1], ho[2]);
}

// ---- CV_8U on packed pairs: low half = the even output, high half = the odd output of one source pixel
// horizontal: sm1, s0, sp1 = s[i-1], s[i], s[i+1] as plain bytes -> (e, o) = (sm1 + 6 s0 + sp1, 4 s0 + 4 sp1)
// (the operands are known to be below 2^8, so the two products are 24-bit multiply-adds)
MI355_HD uint32_t hpair(uint32_t sm1, uint32_t s0, uint32_t sp1)
{
    return sm1 + s0 * 0x00040006u + sp1 * 0x00040001u;
}
// vertical, rows i-1, i, i+1 of packed horizontal sums -> the packed pixels of destination row 2i: ((h0 + 6 h1 + h2 + 32) >> 6) per half
MI355_HD uint32_t vEven(uint32_t h0, uint32_t h1, uint32_t h2)
{
    const uint32_t v = PYRUP_LSHL_ADD(h1, 2, PYRUP_LSHL_ADD(h1, 1, h0 + h2 + 0x00200020u));
    return (v >> 6) & 0x00ff00ffu;
}
// rows i, i+1 -> destination row 2i+1: ((4 (h1 + h2) + 32) >> 6) = ((h1 + h2 + 8) >> 4) per half
MI355_HD uint32_t vOdd(uint32_t h1, uint32_t h2)
{
    return ((h1 + h2 + 0x00080008u) >> 4) & 0x00ff00ffu;
}

} // namespace pyrup
