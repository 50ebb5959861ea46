// bfmatch_emu.cpp -- opencv_amd/csrc/bfmatch_math.h (the arithmetic of the kernels of bfmatch.hip) compiled for the CPU: the distances, the 64-bit key and the ordered
// insertion into a k-list, for tests/test_bfmatch_cpu.py to hold against tests/bfmatch_restate.py bit for bit.
#include "bfmatch_math.h"

namespace {

template <int K>
void knnT(int isFloat, int norm, const uint8_t* Q, int nq, const uint8_t* T, int nt, int len, int stride, unsigned long long* keys)
{
    const size_t rowBytes = (size_t)len * (isFloat ? 4 : 1);
    for (int q = 0; q < nq; q++) {
        bfm::KList<K> l;
        bfm::clear(l);
        // the rows in a scrambled order (stride coprime to nt): the list must not depend on the order of insertion
        for (int j = 0; j < nt; j++) {
            const uint32_t r = (uint32_t)(((long long)j * stride) % nt);
            const uint8_t* a = Q + q * rowBytes; const uint8_t* b = T + r * rowBytes;
            const bfm::Key key = isFloat ? bfm::keyOfFloat(bfm::floatDistance((const float*)a, (const float*)b, len, norm), r)
                                         : bfm::keyOf(bfm::hammingBytes(a, b, len, norm == bfm::NORM_HAMMING2), r);
            bfm::insert(l, key);
        }
        for (int i = 0; i < K; i++) keys[(size_t)q * K + i] = l.v[i];
    }
}

} // namespace

extern "C" float emu_bf_distance(int isFloat, int norm, const void* q, const void* t, int len)
{
    if (isFloat) return bfm::floatDistance((const float*)q, (const float*)t, len, norm);
    return (float)bfm::hammingBytes((const uint8_t*)q, (const uint8_t*)t, len, norm == bfm::NORM_HAMMING2);
}

// the word form the fast kernel uses, on rows of whole dwords
extern "C" unsigned emu_bf_hamming_words(int h2, const uint32_t* q, const uint32_t* t, int ndwords)
{
    unsigned s = 0;
    for (int i = 0; i < ndwords; i++) s += h2 ? bfm::hammingWord<true>(q[i], t[i]) : bfm::hammingWord<false>(q[i], t[i]);
    return s;
}

extern "C" unsigned long long emu_bf_key_float(float d, unsigned row) { return bfm::keyOfFloat(d, row); }
extern "C" unsigned long long emu_bf_key_int(unsigned d, unsigned row) { return bfm::keyOf(d, row); }
extern "C" float emu_bf_key_distance(unsigned long long key, int isFloat) { return bfm::keyDistance(key, isFloat != 0); }
extern "C" unsigned long long emu_bf_no_key(void) { return bfm::NO_KEY; }

// rows dense; keys: nq x k, ascending, NO_KEY where a query has fewer candidates.  k is 1, 2, 4 or 8.
extern "C" int emu_bf_knn(int isFloat, int norm, const void* Q, int nq, const void* T, int nt, int len, int k, int stride, unsigned long long* keys)
{
    switch (k) {
    case 1: knnT<1>(isFloat, norm, (const uint8_t*)Q, nq, (const uint8_t*)T, nt, len, stride, keys); return 0;
    case 2: knnT<2>(isFloat, norm, (const uint8_t*)Q, nq, (const uint8_t*)T, nt, len, stride, keys); return 0;
    case 4: knnT<4>(isFloat, norm, (const uint8_t*)Q, nq, (const uint8_t*)T, nt, len, stride, keys); return 0;
    case 8: knnT<8>(isFloat, norm, (const uint8_t*)Q, nq, (const uint8_t*)T, nt, len, stride, keys); return 0;
    }
    return -1;
}

extern "C" int emu_bf_limit(int which)
{
    const int v[] = {bfm::MAX_ROWS, bfm::MAX_K, bfm::MAX_ROW_BYTES, bfm::MAX_IMAGES, bfm::MAX_RADIUS_ROW, bfm::TILE_ROWS, bfm::SPLIT_ROWS};
    return which >= 0 && which < 7 ? v[which] : -1;
}
