// clahe_math.h -- the arithmetic of cv::CLAHE (imgproc/src/clahe.cpp: CLAHE_Impl::apply, CLAHE_CalcLut_Body, CLAHE_Interpolation_Body), shared by the
// kernels of clahe.hip and by a host build of the same lines that the CPU test-suite checks against the numpy restatement (tests/hostemu/clahe_emu.cpp).
//   plan          tile geometry, the copyMakeBorder(BORDER_REFLECT_101) padding rule and the clip limit of CLAHE_Impl::apply
//   binAfterClip  one bin of the clipped and redistributed tile histogram, in closed form: the reference's residual loop adds 1 to bins 0, step, 2 step, ...
//                 while residual-- > 0, i.e. to bin i iff i % step == 0 && i / step < residual -- so every bin can be computed on its own lane
//   lutEntry      saturate_cast<T>((float)sum * lutScale): a float product and a round-half-even, single IEEE operations in any order of the bins
//   axis / blend  the per-pixel bilinear weights and the four-LUT blend, every multiply and add rounded separately (the library builds with -ffp-contract=off)
#pragma once
#include <math.h>

#include "hd.h"

namespace clahe {

struct Plan {
    int tilesX, tilesY;
    int tw, th;            // tile size in the (possibly padded) LUT source
    int area;              // tw * th
    int readW, readH;      // real pixels the LUT source is cut from: the image plus the parent margins copyMakeBorder takes in (= width, height without padding)
    int clip;              // clipped bin height, 0: no clipping
    float lutScale;        // (histSize - 1) / area
};

// false where the reference itself would fail (tile grid with a non-positive side, empty image, a tile area beyond int)
inline bool plan(int width, int height, int marginRight, int marginBottom, int tilesX, int tilesY, double clipLimit, int histSize, Plan& p)
{
    if (width <= 0 || height <= 0 || tilesX <= 0 || tilesY <= 0 || marginRight < 0 || marginBottom < 0) return false;
    p.tilesX = tilesX; p.tilesY = tilesY;
    long long extW = width, extH = height;
    p.readW = width; p.readH = height;
    if (width % tilesX != 0 || height % tilesY != 0) {
        // both sides are padded as soon as one is not divisible: a divisible side still gains a whole tilesX / tilesY (clahe.cpp, CLAHE_Impl::apply)
        const int padR = tilesX - width % tilesX, padB = tilesY - height % tilesY;
        extW += padR; extH += padB;
        // copyMakeBorder on a submatrix (copy.cpp): the parent's real pixels right of / below the ROI first, the rest reflected about that enlarged image
        p.readW = width + (marginRight < padR ? marginRight : padR);
        p.readH = height + (marginBottom < padB ? marginBottom : padB);
    }
    const long long tw = extW / tilesX, th = extH / tilesY;
    if (tw * th > 0x7fffffffLL) return false;
    p.tw = (int)tw; p.th = (int)th; p.area = (int)(tw * th);
    p.lutScale = (float)(histSize - 1) / (float)p.area;
    p.clip = 0;
    if (clipLimit > 0.0) {
        // static_cast<int> of the double; past INT_MAX x86-64's cvttsd2si answers INT_MIN, which the reference's max(clip, 1) then turns into 1
        const double d = clipLimit * p.area / histSize;
        const int c = d < 2147483648.0 ? (int)d : (int)(-2147483647 - 1);
        p.clip = c > 1 ? c : 1;
    }
    return true;
}

// the pixel of the LUT source at (x, y): BORDER_REFLECT_101 about the enlarged image of readW x readH (borderInterpolate, copy.cpp)
MI355_HD int reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = len - 1 - (p - len) - 1;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

MI355_HD int excess(int h, int clip) { return h > clip ? h - clip : 0; }

// the redistribution constants of a tile from its clipped pixel count (clip > 0)
struct Redist { int batch, residual, step; };
MI355_HD Redist redist(int clipped, int histSize)
{
    Redist r;
    r.batch = clipped / histSize;
    r.residual = clipped - r.batch * histSize;
    const int s = r.residual ? histSize / r.residual : 1;
    r.step = s > 1 ? s : 1;
    return r;
}

// bin i of the tile histogram after clipping and redistribution (clip == 0: unchanged)
MI355_HD int binAfterClip(int h, int i, int clip, Redist r)
{
    if (clip <= 0) return h;
    h = (h < clip ? h : clip) + r.batch;
    if (r.residual != 0 && i % r.step == 0 && i / r.step < r.residual) h += 1;
    return h;
}

MI355_HD int roundHalfEven(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(v);
#else
    return (int)nearbyintf(v);                 // cvRound (round half to even in the default rounding mode)
#endif
}

// saturate_cast<T>((float)sum * lutScale), T of maxValue 255 or 65535
MI355_HD int lutEntry(int sum, float lutScale, int maxValue)
{
    const int v = roundHalfEven((float)sum * lutScale);
    return v < 0 ? 0 : v > maxValue ? maxValue : v;
}

// one axis of CLAHE_Interpolation_Body: the weight `a` is taken before the two tile indices are clamped
struct Axis { int t1, t2; float a, a1; };
MI355_HD Axis axis(int x, float invT, int tiles)
{
    Axis r;
    const float tf = (float)x * invT - 0.5f;
    int t1 = (int)floorf(tf);
    r.a = tf - (float)t1;
    r.a1 = 1.0f - r.a;
    int t2 = t1 + 1;
    t1 = t1 > 0 ? t1 : 0;
    t1 = t1 < tiles - 1 ? t1 : tiles - 1;      // never taken for pixels of the image (x < tiles * tile size); keeps every LUT read in bounds
    t2 = t2 < tiles - 1 ? t2 : tiles - 1;
    r.t2 = t2; r.t1 = t1;
    return r;
}

// (L1[tx1] * xa1 + L1[tx2] * xa) * ya1 + (L2[tx1] * xa1 + L2[tx2] * xa) * ya, saturated to [0, maxValue] with round half to even
MI355_HD int blend(int l11, int l12, int l21, int l22, const Axis& ax, const Axis& ay, int maxValue)
{
    const float top = (float)l11 * ax.a1 + (float)l12 * ax.a;
    const float bot = (float)l21 * ax.a1 + (float)l22 * ax.a;
    const float res = top * ay.a1 + bot * ay.a;
    const int v = roundHalfEven(res);
    return v < 0 ? 0 : v > maxValue ? maxValue : v;
}

} // namespace clahe
