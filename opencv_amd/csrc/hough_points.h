// hough_points.h -- the ballot compaction of the non-zero pixels of a CV_8UC1 row into packed points (hough::packPoint), shared by k_hough_points (hough.hip) and
// k_hc_rowcount / k_hc_points (houghcircles.hip): a lane loads one dword (4 pixels), four 64-bit ballots count the non-zero ones of the wave's 256 columns and
// give every lane the number of points the lanes below it hold.
#pragma once
#include "rt.h"
#include "hough_math.h"

namespace mi355 {

// bytes x .. x + 3 of a row w wide as a dword, 0 for the ones past its end
__device__ __forceinline__ uint32_t loadPix4(const uchar* row, int x, int w)
{
    if (x + 4 <= w && ((uintptr_t)(row + x) & 3) == 0) return *reinterpret_cast<const uint32_t*>(row + x);
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) if (x + k < w) v |= (uint32_t)row[x + k] << (8 * k);
    return v;
}

// v: the lane's four pixels.  Returns the wave's number of non-zero pixels; *pre: those of the lanes below this one.  Every lane of the wave must call it.
__device__ __forceinline__ uint32_t ballotPoints4(uint32_t v, int lane, uint32_t* pre)
{
    const uint64_t b0 = __ballot(v & 0xffu), b1 = __ballot(v & 0xff00u), b2 = __ballot(v & 0xff0000u), b3 = __ballot(v & 0xff000000u);
    const uint64_t below = (uint64_t(1) << lane) - 1;
    *pre = __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below);
    return __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
}

// the lane's non-zero pixels of columns x .. x + 3 of row y, as packed points from out on
__device__ __forceinline__ void storePoints4(uint32_t v, int x, int y, uint32_t* out)
{
#pragma unroll
    for (int k = 0; k < 4; k++) if ((v >> (8 * k)) & 0xffu) *out++ = hough::packPoint(x + k, y);
}

} // namespace mi355
