// bfmatch_math.h -- the arithmetic of bfmatch.hip (cv::BFMatcher) that can be wrong, __host__ __device__ so that the CPU suite compiles the very same lines
// (tests/hostemu/bfmatch_emu.cpp) and holds them against tests/bfmatch_restate.py bit for bit.
//
//   distance     NORM_HAMMING: sum of popcount(q ^ t); NORM_HAMMING2: the non-zero 2-bit groups of q ^ t; both exact integers.
//                NORM_L1: s = fl(s + fl(|fl(q - t)|)), NORM_L2SQR: x = fl(q - t), s = fl(s + fl(x * x)), elements ascending, every operation rounded to float32 and
//                never fused (the library is built with -ffp-contract=off, the host emulation too); NORM_L2: the correctly rounded square root of L2SQR (through double, see sqrtRn).
//   key          64 bits, high word the distance (a Hamming count itself, the bit pattern of a non-negative float32 otherwise: monotone as an unsigned integer),
//                low word the GLOBAL train row (the rows of the collection concatenated in list order).  One unsigned compare is the whole order rule
//                (distance, imgIdx, trainIdx).  A NaN distance and a masked pair have no key (NO_KEY, which compares above every key).
//   k-list       the K smallest keys in ascending order, held with compile-time indices (registers on the device); insert() keeps it so.
#pragma once
#include <stdint.h>
#include <string.h>
#if !defined(__HIPCC__)
#include <math.h>
#endif
#include "hd.h"

namespace bfm {

enum { NORM_L1 = 2, NORM_L2 = 4, NORM_L2SQR = 5, NORM_HAMMING = 6, NORM_HAMMING2 = 7 };     // core/base.hpp NormTypes

constexpr int MAX_ROWS = 1 << 24;         // mi355cv_limit("bfmatch_max_rows"): rows per matrix and per collection (the global row is the key's low word; nq x k x 16 bytes of matches stay addressable)
constexpr int MAX_K = 8;                  // ("bfmatch_max_k"): the k-list lives in registers with compile-time indices
constexpr int MAX_ROW_BYTES = 2048;       // ("bfmatch_max_row_bytes"): 512 floats
constexpr int MAX_IMAGES = 64;            // ("bfmatch_max_images"): train matrices per collection (the emit kernel searches their bases linearly)
constexpr int MAX_RADIUS_ROW = 4096;      // ("bfmatch_max_radius_row"): matches of ONE query radiusMatch sorts in LDS (32 KiB of keys)
constexpr int TILE_ROWS = 256;            // ("bfmatch_tile_rows"): train rows the fast Hamming kernel stages into LDS at a time
constexpr int SPLIT_ROWS = 512;           // ("bfmatch_split_rows"): train rows per workgroup when the train set is split over workgroups
constexpr int MAX_SPLITS = 256;           // ... and the most parts; beyond it a part grows by whole multiples of SPLIT_ROWS

typedef unsigned long long Key;
constexpr Key NO_KEY = ~0ull;

using mi355::popc32;
// NORM_HAMMING2 on a word of xor-ed bytes: one bit per non-zero 2-bit group
MI355_HD_PLAIN uint32_t pairs32(uint32_t x) { return (x | (x >> 1)) & 0x55555555u; }

template <bool H2> MI355_HD_PLAIN uint32_t hammingWord(uint32_t q, uint32_t t) { return popc32(H2 ? pairs32(q ^ t) : (q ^ t)); }

// rows of n bytes at any address
MI355_HD_PLAIN uint32_t hammingBytes(const uint8_t* q, const uint8_t* t, int n, bool h2)
{
    uint32_t s = 0;
    for (int i = 0; i < n; i++) { const uint32_t x = (uint32_t)(q[i] ^ t[i]); s += popc32(h2 ? pairs32(x) : x); }
    return s;
}

// the correctly rounded float32 square root: the double root is correctly rounded and 53 >= 2 * 24 + 2 bits make the second rounding harmless.  (The device's
// __fsqrt_rn was measured one ulp off on gfx950: sqrt(6) came back as 0x401CC470, the nearest float is 0x401CC471.)
MI355_HD_PLAIN float sqrtRn(float v) { return (float)sqrt((double)v); }

// NORM_L1 / NORM_L2SQR / NORM_L2 of two rows of n floats
MI355_HD_PLAIN float floatDistance(const float* q, const float* t, int n, int norm)
{
    float s = 0.f;
    if (norm == NORM_L1) for (int i = 0; i < n; i++) { const float x = q[i] - t[i]; s = s + (x < 0.f ? -x : x); }
    else for (int i = 0; i < n; i++) { const float x = q[i] - t[i]; const float p = x * x; s = s + p; }
    return norm == NORM_L2 ? sqrtRn(s) : s;
}

MI355_HD_PLAIN uint32_t floatBits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
MI355_HD_PLAIN float bitsFloat(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

MI355_HD_PLAIN Key keyOf(uint32_t dist, uint32_t row) { return ((Key)dist << 32) | row; }
// a float distance: NaN has no key.  -x of a NaN, |x| and x * x never give -0, so the sign bit is clear and the pattern is monotone
MI355_HD_PLAIN Key keyOfFloat(float d, uint32_t row) { return d != d ? NO_KEY : keyOf(floatBits(d), row); }
MI355_HD_PLAIN uint32_t keyRow(Key k) { return (uint32_t)k; }
MI355_HD_PLAIN float keyDistance(Key k, bool isFloat) { const uint32_t h = (uint32_t)(k >> 32); return isFloat ? bitsFloat(h) : (float)h; }

template <int K> struct KList { Key v[K]; };

template <int K> MI355_HD_PLAIN void clear(KList<K>& l)
{
#pragma unroll
    for (int i = 0; i < K; i++) l.v[i] = NO_KEY;
}

// keeps the K smallest keys in ascending order; keys are unique, NO_KEY is never inserted (it is not below the last element)
template <int K> MI355_HD_PLAIN void insert(KList<K>& l, Key key)
{
    if (!(key < l.v[K - 1])) return;
    l.v[K - 1] = key;
#pragma unroll
    for (int i = K - 1; i > 0; i--) {
        const Key a = l.v[i - 1], b = l.v[i];
        const bool sw = b < a;
        l.v[i - 1] = sw ? b : a;
        l.v[i] = sw ? a : b;
    }
}

} // namespace bfm
