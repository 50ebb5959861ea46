// minmax_emu.cpp -- opencv_amd/csrc/minmax_math.h (the arithmetic of the kernels of minmax.hip) compiled for the CPU: the key of each depth, its validity test and
// its decode, the combine of (key, index) pairs, and a whole reduction of a frame with the combine applied in several association orders, for
// tests/test_minmax_cpu.py to hold against tests/minmax_restate.py.
#include <vector>
#include "minmax_math.h"

using minmax::Best;
using minmax::Depth;

namespace {

template <int D> void keysOf(const void* elems, int n, uint64_t* keys, unsigned char* valid)
{
    typedef typename Depth<D>::U U;
    const U* e = (const U*)elems;
    for (int i = 0; i < n; i++) { valid[i] = Depth<D>::valid(e[i]); keys[i] = valid[i] ? (uint64_t)Depth<D>::key(e[i]) : 0; }
}

template <int D> void valuesOf(const uint64_t* keys, int n, double* out)
{
    typedef typename Depth<D>::K K;
    for (int i = 0; i < n; i++) out[i] = Depth<D>::value((K)keys[i]);
}

template <class K> Best<K> fold(const std::vector<Best<K>>& p, int order)
{
    const int n = (int)p.size();
    Best<K> r = minmax::identity<K>();
    if (order == 0) { for (int i = 0; i < n; i++) r = minmax::combine(r, p[i]); return r; }                  // a left fold
    if (order == 1) { for (int i = n - 1; i >= 0; i--) r = minmax::combine(p[i], r); return r; }             // a right fold from the end
    if (order == 2) {                                                                                        // a balanced tree, the later half as the first operand
        std::vector<Best<K>> q(p);
        for (int m = n; m > 1; m = (m + 1) / 2)
            for (int i = 0; i < m / 2; i++) q[i] = minmax::combine(q[m - 1 - i], q[i]);
        return n ? q[0] : r;
    }
    if (order == 3) {                                                                                        // 64 strided lanes, then a butterfly as the wave does
        Best<K> lane[64];
        for (int l = 0; l < 64; l++) { lane[l] = minmax::identity<K>(); for (int i = l; i < n; i += 64) lane[l] = minmax::combine(lane[l], p[i]); }
        for (int m = 32; m; m >>= 1) { Best<K> t[64]; for (int l = 0; l < 64; l++) t[l] = minmax::combine(lane[l], lane[l ^ m]); for (int l = 0; l < 64; l++) lane[l] = t[l]; }
        return lane[17];
    }
    std::vector<Best<K>> c;                                                                                  // runs of 7, the runs combined from the last to the first
    for (int i = 0; i < n; i += 7) { Best<K> b = minmax::identity<K>(); for (int k = i; k < n && k < i + 7; k++) b = minmax::combine(b, p[k]); c.push_back(b); }
    for (int i = (int)c.size() - 1; i >= 0; i--) r = minmax::combine(r, c[i]);
    return r;
}

template <int D> void reduce(const unsigned char* src, size_t step, int w, int h, const unsigned char* mask, size_t mstep, int order, double* vals, int* locs)
{
    typedef typename Depth<D>::U U;
    typedef typename Depth<D>::K K;
    std::vector<Best<K>> mn, mx;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const U e = ((const U*)(src + (size_t)y * step))[x];
            if ((mask && !mask[(size_t)y * mstep + x]) || !Depth<D>::valid(e)) continue;
            Best<K> a, b;
            a.key = Depth<D>::key(e); a.idx = (uint32_t)(y * w + x);
            b.key = (K)~a.key; b.idx = a.idx;
            mn.push_back(a); mx.push_back(b);
        }
    minmax::emit<D>(fold(mn, order), fold(mx, order), w, vals, locs);
}

} // namespace

extern "C" int emu_minmax_keys(int depth, const void* elems, int n, uint64_t* keys, unsigned char* valid)
{
    switch (depth) {
    case 0: keysOf<0>(elems, n, keys, valid); break; case 1: keysOf<1>(elems, n, keys, valid); break; case 2: keysOf<2>(elems, n, keys, valid); break;
    case 3: keysOf<3>(elems, n, keys, valid); break; case 4: keysOf<4>(elems, n, keys, valid); break; case 5: keysOf<5>(elems, n, keys, valid); break;
    case 6: keysOf<6>(elems, n, keys, valid); break; default: return -1;
    }
    return 0;
}

extern "C" int emu_minmax_values(int depth, const uint64_t* keys, int n, double* out)
{
    switch (depth) {
    case 0: valuesOf<0>(keys, n, out); break; case 1: valuesOf<1>(keys, n, out); break; case 2: valuesOf<2>(keys, n, out); break;
    case 3: valuesOf<3>(keys, n, out); break; case 4: valuesOf<4>(keys, n, out); break; case 5: valuesOf<5>(keys, n, out); break;
    case 6: valuesOf<6>(keys, n, out); break; default: return -1;
    }
    return 0;
}

// the combine of two pairs, as 32-bit keys (wide = 0) or 64-bit ones; returns 0 when the first operand is the result, 1 for the second
extern "C" int emu_minmax_combine(int wide, uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib, uint64_t* ko, uint32_t* io)
{
    if (wide) {
        Best<uint64_t> a{ka, ia}, b{kb, ib}, r = minmax::combine(a, b);
        *ko = r.key; *io = r.idx;
    } else {
        Best<uint32_t> a{(uint32_t)ka, ia}, b{(uint32_t)kb, ib}, r = minmax::combine(a, b);
        *ko = r.key; *io = r.idx;
    }
    return (*ko == ka && *io == ia) ? 0 : 1;
}

extern "C" int emu_minmax_reduce(int depth, const unsigned char* src, size_t step, int w, int h, const unsigned char* mask, size_t mstep, int order, double* vals,
                                 int* locs)
{
    switch (depth) {
    case 0: reduce<0>(src, step, w, h, mask, mstep, order, vals, locs); break; case 1: reduce<1>(src, step, w, h, mask, mstep, order, vals, locs); break;
    case 2: reduce<2>(src, step, w, h, mask, mstep, order, vals, locs); break; case 3: reduce<3>(src, step, w, h, mask, mstep, order, vals, locs); break;
    case 4: reduce<4>(src, step, w, h, mask, mstep, order, vals, locs); break; case 5: reduce<5>(src, step, w, h, mask, mstep, order, vals, locs); break;
    case 6: reduce<6>(src, step, w, h, mask, mstep, order, vals, locs); break; default: return -1;
    }
    return 0;
}

extern "C" int emu_minmax_max_dim(void) { return minmax::MAX_DIM; }
extern "C" unsigned emu_minmax_none(void) { return minmax::NONE; }
extern "C" int emu_minmax_orders(void) { return 5; }
