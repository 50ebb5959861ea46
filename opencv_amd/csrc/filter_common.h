// filter_common.h -- what filter.hip (filter2D / sepFilter2D / Sobel / Scharr) and box.hip (boxFilter) both use: the depth codes, the saturating per-depth store of
// their generic kernels, and the description of a call's images that their dispatchers hand to the ordered list of served paths.
#pragma once
#include "rt.h"

namespace {

enum { D8U = MI355CV_8U, D16U = MI355CV_16U, D16S = MI355CV_16S, D32F = MI355CV_32F, D64F = MI355CV_64F };

// saturate_cast<DT>(float): cvRound (round-half-even) then clamp (core/saturate.hpp:103-142)
__device__ __forceinline__ void stF(uchar* row, int idx, int depth, float s)
{
    switch (depth) {
    case D8U:  { float r = rintf(s); r = fminf(fmaxf(r, 0.f), 255.f); row[idx] = (uchar)(int)r; break; }
    case D16U: { float r = rintf(s); r = fminf(fmaxf(r, 0.f), 65535.f); reinterpret_cast<unsigned short*>(row)[idx] = (unsigned short)(int)r; break; }
    case D16S: { float r = rintf(s); r = fminf(fmaxf(r, -32768.f), 32767.f); reinterpret_cast<short*>(row)[idx] = (short)(int)r; break; }
    default:   reinterpret_cast<float*>(row)[idx] = s;
    }
}

// The device-side images of one call: nframes frames of W x H pixels, frame f at src + f * sframe / dst + f * dframe.  A frame is the window at (offX, offY) of a
// fullW x fullH parent whose pixels around the window are real memory (the HAL's offset / full-size and margin contracts): borders are the parent's.
//   the hook        one image: nframes = 1, both frame strides 0, the parent geometry as the caller gave it (the image itself for a whole image)
//   a batch entry   every frame is its own parent: fullW = W, fullH = H, off = 0
struct CallImages {
    const uchar* src; size_t sstep, sframe;
    uchar* dst; size_t dstep, dframe;
    int nframes, W, H, fullW, fullH, offX, offY;
    bool whole() const { return fullW == W && fullH == H; }        // no real pixels around the window: the rolling launchers get roi = nullptr
};

} // namespace
