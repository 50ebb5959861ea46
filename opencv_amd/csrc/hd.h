// hd.h -- the base of every header that is compiled twice: by hipcc for the kernels and by g++ for the CPU suite (tests/hostemu).  The two function qualifiers and
// the bit scans whose spelling differs between the two builds are defined here and nowhere else.
#pragma once
#include <stdint.h>

// MI355_HD forces inlining into the kernels; MI355_HD_PLAIN leaves the choice to the compiler.  A header keeps the one it was written with: swapping them moves
// the compiler's inlining choices, and with them the generated code.
#if defined(__HIPCC__)
#  define MI355_HD __host__ __device__ __forceinline__
#  define MI355_HD_PLAIN __host__ __device__ inline
#else
#  define MI355_HD inline
#  define MI355_HD_PLAIN inline
#endif

namespace mi355 {

MI355_HD int clz64(uint64_t v)                    // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}
MI355_HD int ctz64(uint64_t v)                    // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}
MI355_HD int popc64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}
MI355_HD_PLAIN uint32_t popc32(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}

} // namespace mi355
