// demosaic_math.h -- the arithmetic of bilinear Bayer demosaicing (cv::demosaicing / the Bayer codes of cv::cvtColor: imgproc/src/demosaicing.cpp, Bayer2RGB_ and
// Bayer2Gray_), shared by the kernels of demosaic.hip and by a host build of the same lines that the CPU test-suite checks against the numpy restatement
// (tests/hostemu/demosaic_emu.cpp, tests/demosaic_restate.py).
//
// pattern 0..3 = BG, GB, RG, GR (the reference names a pattern after the colours of row 1, columns 1 and 2); sites relative to the origin of the image handed in:
//     BG: R G / G B     GB: G R / B G     RG: B G / G R     GR: G B / R G
// so  site (y, x) is green            iff (x + y + pattern) & 1           isGreen / greenEven (the even columns of row y are the green ones)
//     the other sites of row y are blue iff ((y & 1) ^ (pattern >> 1))      rowBlue            (red otherwise)
// Interior pixel, c = centre, H = left + right, V = up + down, D = the four diagonals, integer arithmetic:
//     R / B site:  own colour c,  green (H + V + 2) >> 2,  opposite colour (D + 2) >> 2
//     G site:      green c,  the colour of the row (H + 1) >> 1,  the colour of the column (V + 1) >> 1
//     gray, K_B = 1868, K_G = 9617, K_R = 4899 (sum 2^14):
//     R / B site:  (4 c K_own + D K_opposite + (H + V) K_G + 2^15) >> 16          G site:  (H K_row + V K_column + 2 c K_G + 2^14) >> 15
//     here both as (c wc + H wh + V wv + D wd + 2^15) >> 16 with the G site's weights doubled (exactly the same value); for CV_16U the sum reaches
//     2^32 - 2^18 + 2^15: unsigned 32 bits, never int.
// Border: output (y, x) is the interior result of site (clamp(y, 1, h-2), clamp(x, 1, w-2)), colour assignment of THAT site included (clampIdx).
//
//   bgr / grayWeights / gray     the scalar lines (k_demosaic<T, DCN>)
//   leftOf / rightOf / avg2 / sum2e / sum2o / avg4 / planes / grayQuad / interleave3 / interleave4 / bytePerm
//                                CV_8U on four pixels per dword (k_demosaic_roll): two-neighbour averages are one v_lerp_u8, four-neighbour averages exact
//                                16-bit pair sums (a lerp of lerps would round twice)
#pragma once
#include <stdint.h>

#include "hd.h"

namespace demosaic {

constexpr uint32_t KB = 1868, KG = 9617, KR = 4899;

MI355_HD int isGreen(int pattern, int y, int x) { return (x + y + pattern) & 1; }
MI355_HD int greenEven(int pattern, int y) { return (y + pattern) & 1; }
MI355_HD int rowBlue(int pattern, int y) { return (y ^ (pattern >> 1)) & 1; }
MI355_HD int clampIdx(int i, int n) { return i < 1 ? 1 : (i > n - 2 ? n - 2 : i); }              // n >= 3

// ---- scalar
MI355_HD void bgr(int green, int rowIsBlue, uint32_t c, uint32_t H, uint32_t V, uint32_t D, uint32_t& b, uint32_t& g, uint32_t& r)
{
    uint32_t rowc, othc;
    if (green) { g = c; rowc = (H + 1) >> 1; othc = (V + 1) >> 1; }
    else { g = (H + V + 2) >> 2; rowc = c; othc = (D + 2) >> 2; }
    b = rowIsBlue ? rowc : othc;
    r = rowIsBlue ? othc : rowc;
}

struct GrayW { uint32_t wc, wh, wv, wd; };
MI355_HD GrayW grayWeights(int green, int rowIsBlue)
{
    const uint32_t krow = rowIsBlue ? KB : KR, koth = rowIsBlue ? KR : KB;
    GrayW w;
    if (green) { w.wc = 4 * KG; w.wh = 2 * krow; w.wv = 2 * koth; w.wd = 0; }
    else { w.wc = 4 * krow; w.wh = KG; w.wv = KG; w.wd = koth; }
    return w;
}
MI355_HD uint32_t gray(const GrayW& w, uint32_t c, uint32_t H, uint32_t V, uint32_t D)
{
    return (c * w.wc + H * w.wh + V * w.wv + D * w.wd + (1u << 15)) >> 16;
}

// ---- CV_8U, four pixels (columns x .. x+3, x a multiple of 4) per dword, byte j = column x + j
// v_perm_b32: result byte j = byte sel[j] of the pair (hi: 4..7, lo: 0..3), 0x0c -> 0x00, 0x0d -> 0xff
MI355_HD uint32_t bytePerm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t pair = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int j = 0; j < 4; j++) {
        const uint32_t s = (sel >> (8 * j)) & 0xffu;
        const uint32_t v = s < 8 ? (uint32_t)(pair >> (8 * s)) & 0xffu : (s == 0x0c ? 0u : 0xffu);      // (the sign-replicating selectors 8..11 are not used here)
        r |= v << (8 * j);
    }
    return r;
#endif
}
// columns x-1 .. x+2 and x+1 .. x+4 from the dword itself and its neighbours (one v_alignbit each)
MI355_HD uint32_t leftOf(uint32_t prev, uint32_t cur) { return (cur << 8) | (prev >> 24); }
MI355_HD uint32_t rightOf(uint32_t cur, uint32_t next) { return (cur >> 8) | (next << 24); }
// (a + b + 1) >> 1 per byte
MI355_HD uint32_t avg2(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_lerp(a, b, 0x01010101u);                // v_lerp_u8: (a + b + (c & 1)) >> 1 per byte
#else
    uint32_t r = 0;
    for (int j = 0; j < 4; j++) r |= ((((a >> (8 * j)) & 0xffu) + ((b >> (8 * j)) & 0xffu) + 1u) >> 1) << (8 * j);
    return r;
#endif
}
// a + b per byte as 16-bit pairs: the even bytes (columns x, x+2) and the odd bytes (x+1, x+3)
MI355_HD uint32_t sum2e(uint32_t a, uint32_t b) { return (a & 0x00ff00ffu) + (b & 0x00ff00ffu); }
MI355_HD uint32_t sum2o(uint32_t a, uint32_t b) { return ((a >> 8) & 0x00ff00ffu) + ((b >> 8) & 0x00ff00ffu); }
// (s1 + s2 + 2) >> 2 per column from two such pair sums (each half <= 510, so 1022 at most: no carry between the halves), back to four bytes
MI355_HD uint32_t avg4(uint32_t e1, uint32_t o1, uint32_t e2, uint32_t o2)
{
    const uint32_t e = ((e1 + e2 + 0x00020002u) >> 2) & 0x00ff00ffu;
    const uint32_t o = ((o1 + o2 + 0x00020002u) >> 2) & 0x00ff00ffu;
    return e | (o << 8);
}
// the B, G, R planes of four pixels of one row.  mg: byte mask of its green sites (greenMask); c centre, h = avg2(left, right), v = avg2(up, down),
// hv = avg4(left + right, up + down), d = avg4 of the diagonals
MI355_HD uint32_t greenMask(int greenIsEven) { return greenIsEven ? 0x00ff00ffu : 0xff00ff00u; }
MI355_HD void planes(uint32_t mg, int rowIsBlue, uint32_t c, uint32_t h, uint32_t v, uint32_t hv, uint32_t d, uint32_t& b, uint32_t& g, uint32_t& r)
{
    g = (c & mg) | (hv & ~mg);
    const uint32_t rowc = (h & mg) | (c & ~mg), othc = (v & mg) | (d & ~mg);
    b = rowIsBlue ? rowc : othc;
    r = rowIsBlue ? othc : rowc;
}
// gray of four pixels: c the centre bytes, (hE, hO) / (vE, vO) / (dE, dO) the pair sums left + right / up + down / diagonals; we / wo the weights of the
// even / odd columns' sites
MI355_HD uint32_t grayQuad(const GrayW& we, const GrayW& wo, uint32_t c, uint32_t hE, uint32_t hO, uint32_t vE, uint32_t vO, uint32_t dE, uint32_t dO)
{
    const uint32_t p0 = gray(we, c & 0xffu, hE & 0xffffu, vE & 0xffffu, dE & 0xffffu);
    const uint32_t p1 = gray(wo, (c >> 8) & 0xffu, hO & 0xffffu, vO & 0xffffu, dO & 0xffffu);
    const uint32_t p2 = gray(we, (c >> 16) & 0xffu, hE >> 16, vE >> 16, dE >> 16);
    const uint32_t p3 = gray(wo, c >> 24, hO >> 16, vO >> 16, dO >> 16);
    return p0 | (p1 << 8) | (p2 << 16) | (p3 << 24);
}
// planes of four pixels -> 12 interleaved bytes B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
MI355_HD void interleave3(uint32_t b, uint32_t g, uint32_t r, uint32_t (&o)[3])
{
    const uint32_t bg01 = bytePerm(g, b, 0x05010400u), bg23 = bytePerm(g, b, 0x07030602u);        // B0 G0 B1 G1, B2 G2 B3 G3
    o[0] = bytePerm(r, bg01, 0x02040100u);
    o[1] = bytePerm(r, bytePerm(bg23, bg01, 0x05040003u), 0x03020500u);
    o[2] = bytePerm(r, bg23, 0x07030206u);
}
// ... -> 16 bytes B G R 255 per pixel
MI355_HD void interleave4(uint32_t b, uint32_t g, uint32_t r, uint32_t (&o)[4])
{
    const uint32_t bg01 = bytePerm(g, b, 0x05010400u), bg23 = bytePerm(g, b, 0x07030602u);
    o[0] = bytePerm(r, bg01, 0x0d040100u);
    o[1] = bytePerm(r, bg01, 0x0d050302u);
    o[2] = bytePerm(r, bg23, 0x0d060100u);
    o[3] = bytePerm(r, bg23, 0x0d070302u);
}

} // namespace demosaic
