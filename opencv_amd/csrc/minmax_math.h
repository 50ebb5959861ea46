// minmax_math.h -- the arithmetic of minmax.hip (cv::minMaxLoc) that can be wrong, __host__ __device__ so that the CPU suite compiles the very same lines
// (tests/hostemu/minmax_emu.cpp): the order-preserving key of each depth, NaN detection, the canonical zero, decoding a key back to the value, and the order on
// (key, index) pairs every combine step of the reduction uses.
//
//   key      an unsigned integer K (32 bits for CV_8U .. CV_32F, 64 for CV_64F) with  a < b  <=>  key(a) < key(b)  for every two candidate values.  Unsigned
//            depths: the value itself.  Signed depths: the two's complement pattern with its sign bit flipped.  Floats: -0 is first replaced by +0 (they compare
//            equal, so they must share a key); then a pattern with the sign bit set is complemented (larger magnitude = smaller value) and one without gets the
//            sign bit set (above every negative).  +-inf are ordinary patterns.  A NaN (exponent all ones, mantissa non-zero) is no candidate and has no key.
//   Best     the pair (key, idx): idx is the pixel's raster index y * width + x (< 2^28, rt.h MINMAX_MAX_DIM), NONE when there is no candidate.  The minimum is the
//            least pair in the lexicographic order (key, idx); the maximum is the least pair of (~key, idx) -- the complement turns "greatest key" into "least"
//            and leaves "smallest index on ties" as it is, so ONE order serves both and both keep the first pixel in raster order.  The order is total and
//            (all ones, NONE) is its greatest element, hence the identity of the combine: a candidate whose key is all ones (INT_MAX of CV_32S as a minimum)
//            still has an index below NONE and wins over it.  min over a total order is associative and commutative: the result cannot depend on how the
//            pixels were grouped into lanes, waves, workgroups and grid passes.
#pragma once
#include <stdint.h>
#include <string.h>
#include "hd.h"

namespace minmax {

constexpr int MAX_DIM = 16384;                 // width and height: a raster index stays below 2^28
constexpr uint32_t NONE = 0xFFFFFFFFu;         // the index of "no candidate"
constexpr int MAX_FRAMES = 65535;

template <class K> MI355_HD_PLAIN K least(K a, K b) { return b < a ? b : a; }
template <class K> MI355_HD_PLAIN K greatest(K a, K b) { return a < b ? b : a; }

template <class K> struct Best { K key; uint32_t idx; };

template <class K> MI355_HD_PLAIN Best<K> identity() { Best<K> b; b.key = (K)~(K)0; b.idx = NONE; return b; }
// a comes before b in the total order
template <class K> MI355_HD_PLAIN bool before(const Best<K>& a, const Best<K>& b) { return a.key < b.key || (a.key == b.key && a.idx < b.idx); }
template <class K> MI355_HD_PLAIN Best<K> combine(const Best<K>& a, const Best<K>& b) { return before(b, a) ? b : a; }

// Depth<d>: U the element as raw bits, K the key; valid(bits) -- a candidate value; key(bits); value(key) -- exactly (double)element
template <int DEPTH> struct Depth;

template <> struct Depth<0> {                  // CV_8U
    typedef uint8_t U; typedef uint32_t K;
    static MI355_HD_PLAIN bool valid(U) { return true; }
    static MI355_HD_PLAIN K key(U v) { return v; }
    static MI355_HD_PLAIN double value(K k) { return (double)k; }
};
template <> struct Depth<1> {                  // CV_8S
    typedef uint8_t U; typedef uint32_t K;
    static MI355_HD_PLAIN bool valid(U) { return true; }
    static MI355_HD_PLAIN K key(U v) { return (K)(v ^ 0x80u); }
    static MI355_HD_PLAIN double value(K k) { return (double)((int32_t)k - 128); }
};
template <> struct Depth<2> {                  // CV_16U
    typedef uint16_t U; typedef uint32_t K;
    static MI355_HD_PLAIN bool valid(U) { return true; }
    static MI355_HD_PLAIN K key(U v) { return v; }
    static MI355_HD_PLAIN double value(K k) { return (double)k; }
};
template <> struct Depth<3> {                  // CV_16S
    typedef uint16_t U; typedef uint32_t K;
    static MI355_HD_PLAIN bool valid(U) { return true; }
    static MI355_HD_PLAIN K key(U v) { return (K)(v ^ 0x8000u); }
    static MI355_HD_PLAIN double value(K k) { return (double)((int32_t)k - 32768); }
};
template <> struct Depth<4> {                  // CV_32S
    typedef uint32_t U; typedef uint32_t K;
    static MI355_HD_PLAIN bool valid(U) { return true; }
    static MI355_HD_PLAIN K key(U v) { return v ^ 0x80000000u; }
    static MI355_HD_PLAIN double value(K k) { return (double)(int32_t)(k ^ 0x80000000u); }
};
template <> struct Depth<5> {                  // CV_32F
    typedef uint32_t U; typedef uint32_t K;
    static MI355_HD_PLAIN bool valid(U v) { return (v & 0x7FFFFFFFu) <= 0x7F800000u; }
    static MI355_HD_PLAIN K key(U v)
    {
        if (v == 0x80000000u) v = 0;                                         // -0 == +0
        return (v & 0x80000000u) ? ~v : (v | 0x80000000u);
    }
    static MI355_HD_PLAIN double value(K k)
    {
        const uint32_t v = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
        float f;
        memcpy(&f, &v, 4);
        return (double)f;
    }
};
template <> struct Depth<6> {                  // CV_64F
    typedef uint64_t U; typedef uint64_t K;
    static MI355_HD_PLAIN bool valid(U v) { return (v & 0x7FFFFFFFFFFFFFFFull) <= 0x7FF0000000000000ull; }
    static MI355_HD_PLAIN K key(U v)
    {
        if (v == 0x8000000000000000ull) v = 0;
        return (v & 0x8000000000000000ull) ? ~v : (v | 0x8000000000000000ull);
    }
    static MI355_HD_PLAIN double value(K k)
    {
        const uint64_t v = (k & 0x8000000000000000ull) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
        double d;
        memcpy(&d, &v, 8);
        return d;
    }
};

// what a frame's two winning pairs become: vals = {min, max}, locs = {minX, minY, maxX, maxY}; an empty candidate set gives 0, 0 and (-1, -1) twice.
// mx carries the COMPLEMENTED key.
template <int DEPTH> MI355_HD_PLAIN void emit(const Best<typename Depth<DEPTH>::K>& mn, const Best<typename Depth<DEPTH>::K>& mx, int width, double* vals, int* locs)
{
    typedef typename Depth<DEPTH>::K K;
    if (mn.idx == NONE || mx.idx == NONE) {                                  // both or neither: they range over the same set
        vals[0] = vals[1] = 0.0;
        locs[0] = locs[1] = locs[2] = locs[3] = -1;
        return;
    }
    vals[0] = Depth<DEPTH>::value(mn.key);
    vals[1] = Depth<DEPTH>::value((K)~mx.key);
    locs[0] = (int)(mn.idx % (uint32_t)width); locs[1] = (int)(mn.idx / (uint32_t)width);
    locs[2] = (int)(mx.idx % (uint32_t)width); locs[3] = (int)(mx.idx / (uint32_t)width);
}

} // namespace minmax
