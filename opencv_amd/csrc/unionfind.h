// unionfind.h -- the one union-find of the library: ccl.hip (cv::connectedComponents) and speckle.hip (cv::filterSpeckles) merge with it, and the CPU suite runs the
// same lines (tests/hostemu/ccl_emu.cpp, speckle_emu.cpp).  A root is its own parent and every other parent is smaller than its child; the root of a set is its
// SMALLEST index and parents only ever decrease, so the root does not depend on the order the unions land in.  find / unite are written once over a memory policy M:
//   load(i)      the parent of i
//   amin(i, v)   the old parent of i, which becomes min(old, v)
// A find may read a parent that another workgroup of the same kernel has just written.  unite retries until its amin returns the value it read, so a stale read
// only costs another round.
#pragma once
#include "hd.h"

namespace uf {

template <class M> MI355_HD uint32_t find(M& m, uint32_t x)
{
    for (;;) { const uint32_t p = m.load(x); if (p >= x) return x; x = p; }
}
template <class M> MI355_HD void unite(M& m, uint32_t a, uint32_t b)
{
    for (;;) {
        a = find(m, a); b = find(m, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = m.amin(a, b);                  // a was a root when read: old == a unless another union got there first
        if (old == a) return;
        a = old;                                            // the set a pointed to still has to meet b
    }
}

// the host build: one thread, plain loads and stores
struct PlainMem {
    uint32_t* P;
    uint32_t load(uint32_t i) const { return P[i]; }
    uint32_t amin(uint32_t i, uint32_t v) const { const uint32_t old = P[i]; if (v < old) P[i] = v; return old; }
};

#if defined(__HIPCC__)
// parents in HBM, shared by the workgroups of a kernel: every load is an agent-scope atomic load.  at(p) is that load for a kernel that walks the parents by
// pointer (a row and the row above it)
struct GlobalMem {
    uint32_t* P;
    static __device__ __forceinline__ uint32_t at(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return at(P + i); }
    __device__ __forceinline__ uint32_t amin(uint32_t i, uint32_t v) const { return atomicMin(P + i, v); }
};
// parents in LDS, shared by the lanes of a workgroup
struct LdsMem {
    uint32_t* par;
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return ((volatile uint32_t*)par)[i]; }
    __device__ __forceinline__ uint32_t amin(uint32_t i, uint32_t v) const { return atomicMin(par + i, v); }
};
#endif

} // namespace uf
