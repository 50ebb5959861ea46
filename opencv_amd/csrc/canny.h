// canny.h -- cv::Canny: what the circle transform (houghcircles.hip) takes from canny.hip, the stages after the two Sobel calls
#pragma once
#include "rt.h"
namespace mi355 {
// elements per row of the hysteresis map, and the bytes of a frame's map (HBM scratch)
size_t cannyMapPitch(int width);
size_t cannyMapBytes(int width, int height);
// stages 2-5 of mi355cv_canny from the CV_16S gradient planes dx / dy (rows gstep BYTES apart, cn interleaved channels): magnitude, non-maximum suppression and
// the double threshold (m > low a candidate, m > high an edge), the hysteresis to its fixed point and dst = 255 on edges, 0 elsewhere (W x H bytes, rows dstep
// apart).  map: cannyMapBytes of scratch; flag: 256 bytes of scratch.  The hysteresis reads its last flag back once per burst of passes, so the call synchronises
// the stream.  false when a runtime call failed.
bool cannyFromGradients(const short* dx, const short* dy, size_t gstep, int width, int height, int cn, int L2, int low, int high, uchar* map, int* flag,
                        uchar* dst, size_t dstep, hipStream_t st);
}
