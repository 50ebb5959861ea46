// deriv_taps.h -- the integer taps of cv::Sobel / cv::Scharr for filter.hip (the derivative hooks) and corner.hip (the derivatives inside cornerHarris / cornerMinEigenVal).
#pragma once
#include <vector>

namespace mi355 {

// getSobelKernels / getScharrKernels (deriv.cpp:55-162) as integer taps; false: an order / ksize the reference has no kernel for, or a ksize above maxKsize (what the
// caller's kernels hold)
inline bool derivKernel(int order, int ksize, bool scharr, int maxKsize, std::vector<int>& k)
{
    if (scharr) {
        if (order == 0) k = {3, 10, 3}; else if (order == 1) k = {-1, 0, 1}; else return false;
        return true;
    }
    if (ksize == 1 && order > 0) ksize = 3;
    if (ksize % 2 == 0 || ksize > maxKsize || ksize <= order) return false;
    if (ksize == 1) { k = {1}; return true; }
    if (ksize == 3) {
        if (order == 0) k = {1, 2, 1}; else if (order == 1) k = {-1, 0, 1}; else k = {1, -2, 1};
        return true;
    }
    std::vector<int> kerI(ksize + 1, 0);
    kerI[0] = 1;
    for (int i = 0; i < ksize - order - 1; i++) {
        int oldval = kerI[0];
        for (int j = 1; j <= ksize; j++) { int nv = kerI[j] + kerI[j - 1]; kerI[j - 1] = oldval; oldval = nv; }
    }
    for (int i = 0; i < order; i++) {
        int oldval = -kerI[0];
        for (int j = 1; j <= ksize; j++) { int nv = kerI[j - 1] - kerI[j]; kerI[j - 1] = oldval; oldval = nv; }
    }
    k.assign(kerI.begin(), kerI.begin() + ksize);
    return true;
}

} // namespace mi355
