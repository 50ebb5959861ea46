// box.hip -- row a5 of SURVEY.md §8: cv::boxFilter / cv::blur.
//
// The hook (one image, margins, host or device) and the batch entry (device-resident whole frames) derive the reference's parameters once (boxRun), describe their
// images (filter_common.h CallImages) and hand them to ONE ordered list of served paths (boxServe): the rolling kernels of seproll.hip, k_sepmx on the matrix cores
// (sepmx.hip), the two-pass running sums k_box_rows / k_box_cols, and k_box_generic -- one thread per output element, correct for every depth pair / border / anchor /
// ROI the entry accepts.
//
// Reference semantics restated here:
// cv::boxFilter (box_filter.dispatch.cpp:440, createBoxFilter box_filter.simd.hpp:1250):
//   8U->8U, area <= 256 : u16 sums; normalised result = ((s + dd) * ds) >> 23 with the reciprocal pair (ds, dd) of
//                         ColumnSum<ushort,uchar> (:429-455); un-normalised = saturate_u8(s)
//   other integer inputs: int32 sums; normalised = cvRound(float(s) * float(1/area)) (the SIMD body of
//                         ColumnSum<int,uchar> :340-372), un-normalised = saturate(s)
//   float input         : double sums (RowSum<float,double>, ColumnSum<double,float>), result = float(s * scale)
#include "filter_common.h"
#include "seproll.h"
#include "sepmx.h"
#include <cmath>
#include <cstring>

using namespace mi355;

namespace {

struct BoxParams { int kw, kh, ax, ay, normalize, mode /*0 u16, 1 int, 2 double*/, divScale, divDelta; float scaleF; double scaleD; };

__global__ __launch_bounds__(256) void k_box_generic(
    const uchar* __restrict__ src, size_t sstep, uchar* __restrict__ dst, size_t dstep,
    int W, int H, int cn, int sdepth, int ddepth, int fullW, int fullH, int offX, int offY, int border, BoxParams p)
{
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (e >= W * cn || y >= H) return;
    const int x = e / cn, ch = e - x * cn;
    const int fx0 = x + offX - p.ax, fy0 = y + offY - p.ay;
    uchar* drow = dst + (size_t)y * dstep;
    if (p.mode == 2) {
        double s = 0.0;
        for (int j = 0; j < p.kh; j++) {
            const int yy = mi355_borderInterpolate(fy0 + j, fullH, border);
            if (yy < 0) continue;
            const uchar* row = src + (ptrdiff_t)(yy - offY) * (ptrdiff_t)sstep;
            double rs = 0.0;
            for (int i = 0; i < p.kw; i++) {
                const int xx = mi355_borderInterpolate(fx0 + i, fullW, border);
                if (xx >= 0) rs += sdepth == D64F ? reinterpret_cast<const double*>(row)[(xx - offX) * cn + ch] : (double)reinterpret_cast<const float*>(row)[(xx - offX) * cn + ch];
            }
            s += rs;
        }
        if (ddepth == D64F) reinterpret_cast<double*>(drow)[e] = p.normalize ? s * p.scaleD : s;
        else reinterpret_cast<float*>(drow)[e] = (float)(p.normalize ? s * p.scaleD : s);
        return;
    }
    int s = 0;
    for (int j = 0; j < p.kh; j++) {
        const int yy = mi355_borderInterpolate(fy0 + j, fullH, border);
        if (yy < 0) continue;
        const uchar* row = src + (ptrdiff_t)(yy - offY) * (ptrdiff_t)sstep;
        for (int i = 0; i < p.kw; i++) {
            const int xx = mi355_borderInterpolate(fx0 + i, fullW, border);
            if (xx < 0) continue;
            const int idx = (xx - offX) * cn + ch;
            s += sdepth == D8U ? (int)row[idx] : sdepth == D16U ? (int)reinterpret_cast<const unsigned short*>(row)[idx]
                                                              : (int)reinterpret_cast<const short*>(row)[idx];
        }
    }
    // from here on: the same arithmetic as boxFinish<int> below -- the two must change together
    if (p.mode == 0) {
        unsigned r = p.normalize ? (((unsigned)s + (unsigned)p.divDelta) * (unsigned)p.divScale) >> 23 : (unsigned)s;
        drow[e] = (uchar)(p.normalize ? r : (r > 255u ? 255u : r));
        return;
    }
    if (ddepth == D64F) {           // ColumnSum<int, double> (box_filter.simd.hpp:1195-1240): the exact int sum, one multiply in double
        reinterpret_cast<double*>(drow)[e] = p.normalize ? (double)s * p.scaleD : (double)s;
        return;
    }
    if (ddepth == D32F) {
        // ColumnSum<int, float> (box_filter.simd.hpp:1109-1130): the vector body multiplies in float, the last (W*cn) % 4 elements of a row in double
        reinterpret_cast<float*>(drow)[e] = !p.normalize ? (float)s : e < ((W * cn) & ~3) ? __fmul_rn((float)s, p.scaleF) : (float)((double)s * p.scaleD);
        return;
    }
    if (p.normalize && e >= ((W * cn) & ~7)) {
        // the reference's scalar tail (the last (W*cn) % 8 elements of a row, box_filter.simd.hpp:380-385) multiplies in double
        const double r = rint((double)s * p.scaleD);
        if (ddepth == D8U) drow[e] = (uchar)(int)fmin(fmax(r, 0.0), 255.0);
        else if (ddepth == D16U) reinterpret_cast<unsigned short*>(drow)[e] = (unsigned short)(int)fmin(fmax(r, 0.0), 65535.0);
        else reinterpret_cast<short*>(drow)[e] = (short)(int)fmin(fmax(r, -32768.0), 32767.0);
        return;
    }
    float v = p.normalize ? rintf((float)s * p.scaleF) : (float)s;
    stF(drow, e, ddepth, v);
}

// ---------------------------------------------------------------------------------- box filter in two passes (what neither the rolling kernels nor k_sepmx take)
// RowSum then ColumnSum like the reference (box_filter.simd.hpp:60-180, 182-1240) instead of k_box_generic's kw * kh gathers per output (a 121 x 121 window of a guided
// filter on a 4K float frame: 14 641 loads per element, slower than the CPU's running sums):
//   k_box_rows   window sums along x of every parent row the call touches, into a scratch image of int (integer sources: exact) or double (float sources: the reference's
//                sum type) -- a workgroup stages 1024 + kw - 1 values of one channel of one row in LDS (border rule resolved there), a lane takes 4 neighbouring windows:
//                one sum of kw values, three slides;
//   k_box_cols   a lane owns an output column and walks down a segment with the running column sum (add the row entering, subtract the row leaving -- ColumnSum's own
//                recurrence), and finishes every sum exactly as k_box_generic does (the reference's normalisations per depth pair).
// Integer results are those of k_box_generic bit for bit; double sums differ from it in the last bits of the DOUBLE (the order of the additions), i.e. not at all after
// the rounding to float in all but isolated elements -- the float bar of the path is 1e-4.
template <typename SUM> struct BoxStage { typedef int L; };
template <> struct BoxStage<double> { typedef float L; };

template <typename ST, typename SUM>
__global__ __launch_bounds__(256) void k_box_rows(const uchar* __restrict__ src, size_t sstep, SUM* __restrict__ R, size_t rpitch, int W, int cn, int fullW, int offX, int offY,
                                                  int r0, int kw, int ax, int border)
{
    typedef typename BoxStage<SUM>::L LT;
    extern __shared__ __attribute__((aligned(16))) uchar boxlds_[];
    LT* L = reinterpret_cast<LT*>(boxlds_);
    const int tid = threadIdx.x, ch = blockIdx.z, prow = r0 + blockIdx.y, xb = blockIdx.x * 1024;
    const ST* row = reinterpret_cast<const ST*>(src + (ptrdiff_t)(prow - offY) * (ptrdiff_t)sstep);
    const int nout = min(1024, W - xb), nst = nout + kw + 3;
    for (int j = tid; j < nst; j += 256) {
        int fx = xb + j + offX - ax;
        if ((unsigned)fx >= (unsigned)fullW) fx = mi355_borderInterpolate(fx, fullW, border);
        L[j] = (fx >= 0 && j < nout + kw - 1) ? (LT)row[(fx - offX) * cn + ch] : (LT)0;
    }
    __syncthreads();
    const int x = 4 * tid;
    if (x >= nout) return;
    typedef LT l4 __attribute__((ext_vector_type(4)));
    const LT* q = L + x;
    SUM s = 0;
    int t = 0;
    for (; t + 4 <= kw; t += 4) { const l4 v = *reinterpret_cast<const l4*>(q + t); s += (SUM)v.x; s += (SUM)v.y; s += (SUM)v.z; s += (SUM)v.w; }
    for (; t < kw; t++) s += (SUM)q[t];
    SUM* out = R + (size_t)blockIdx.y * rpitch + (size_t)(xb + x) * cn + ch;
    out[0] = s;
#pragma unroll
    for (int i = 1; i < 4; i++) {
        if (x + i >= nout) break;
        s += (SUM)q[kw + i - 1]; s -= (SUM)q[i - 1];
        out[(size_t)i * cn] = s;
    }
}

template <typename SUM>
__device__ __forceinline__ void boxFinish(uchar* drow, int e, SUM s, int W, int cn, int ddepth, const BoxParams& p);
template <>
__device__ __forceinline__ void boxFinish<double>(uchar* drow, int e, double s, int W, int cn, int ddepth, const BoxParams& p)
{
    if (ddepth == D64F) reinterpret_cast<double*>(drow)[e] = p.normalize ? s * p.scaleD : s;
    else reinterpret_cast<float*>(drow)[e] = (float)(p.normalize ? s * p.scaleD : s);
}
// the same arithmetic as the tail of k_box_generic above -- the two must change together
template <>
__device__ __forceinline__ void boxFinish<int>(uchar* drow, int e, int s, int W, int cn, int ddepth, const BoxParams& p)
{
    if (p.mode == 0) {
        unsigned r = p.normalize ? (((unsigned)s + (unsigned)p.divDelta) * (unsigned)p.divScale) >> 23 : (unsigned)s;
        drow[e] = (uchar)(p.normalize ? r : (r > 255u ? 255u : r));
        return;
    }
    if (ddepth == D64F) { reinterpret_cast<double*>(drow)[e] = p.normalize ? (double)s * p.scaleD : (double)s; return; }
    if (ddepth == D32F) { reinterpret_cast<float*>(drow)[e] = !p.normalize ? (float)s : e < ((W * cn) & ~3) ? __fmul_rn((float)s, p.scaleF) : (float)((double)s * p.scaleD); return; }
    if (p.normalize && e >= ((W * cn) & ~7)) {
        const double r = rint((double)s * p.scaleD);
        if (ddepth == D8U) drow[e] = (uchar)(int)fmin(fmax(r, 0.0), 255.0);
        else if (ddepth == D16U) reinterpret_cast<unsigned short*>(drow)[e] = (unsigned short)(int)fmin(fmax(r, 0.0), 65535.0);
        else reinterpret_cast<short*>(drow)[e] = (short)(int)fmin(fmax(r, -32768.0), 32767.0);
        return;
    }
    const float v = p.normalize ? rintf((float)s * p.scaleF) : (float)s;
    stF(drow, e, ddepth, v);
}

template <typename SUM>
__global__ __launch_bounds__(256) void k_box_cols(const SUM* __restrict__ R, size_t rpitch, int r0, uchar* __restrict__ dst, size_t dstep, int W, int H, int cn, int ddepth,
                                                  int fullH, int offY, int border, BoxParams p, int seg)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= W * cn) return;
    const int y0 = blockIdx.y * seg, y1 = min(H, y0 + seg);
    auto rowSum = [&](int fy) -> SUM {                                                 // (fy is uniform: the row's address is scalar work)
        if ((unsigned)fy >= (unsigned)fullH) fy = mi355_borderInterpolate(fy, fullH, border);
        return fy < 0 ? (SUM)0 : R[(size_t)(fy - r0) * rpitch + e];
    };
    SUM s = 0;
    for (int j = 0; j < p.kh; j++) s += rowSum(y0 + offY - p.ay + j);
    for (int y = y0; y < y1; y++) {
        boxFinish<SUM>(dst + (size_t)y * dstep, e, s, W, cn, ddepth, p);
        if (y + 1 < y1) { s += rowSum(y + 1 + offY - p.ay + p.kh - 1); s -= rowSum(y + offY - p.ay); }
    }
}

// the two-pass box filter (k_box_rows / k_box_cols) for one image; false: not its case (the caller falls back to k_box_generic)
// parent rows the windows can touch: the window's own rows, and what a mirroring border rule folds back into them; BORDER_WRAP reaches across the image
static void boxRowRange(int H, int kh, int fullH, int offY, int border, int* r0, int* r1)
{
    *r0 = std::max(0, offY - kh); *r1 = std::min(fullH, offY + H + kh);
    if (border == B_WRAP) { *r0 = 0; *r1 = fullH; }
}

template <typename ST, typename SUM>
static bool boxTwoPassT(void* scratch, const BoxParams& p, const uchar* src, size_t sstep, uchar* dst, size_t dstep, int W, int H, int cn, int ddepth,
                        int fullW, int fullH, int offX, int offY, int border, hipStream_t st)
{
    int r0, r1;
    boxRowRange(H, p.kh, fullH, offY, border, &r0, &r1);
    const int nr = r1 - r0;
    const size_t rpitch = ((size_t)W * cn + 3) & ~(size_t)3;
    SUM* R = (SUM*)scratch;
    const size_t lds = (size_t)(1024 + p.kw + 8) * 4;
    hipLaunchKernelGGL((k_box_rows<ST, SUM>), dim3(divUp(W, 1024), nr, cn), dim3(256), lds, st, src, sstep, R, rpitch, W, cn, fullW, offX, offY, r0, p.kw, p.ax, border);
    const int seg = 32;
    hipLaunchKernelGGL((k_box_cols<SUM>), dim3(divUp(W * cn, 256), divUp(H, seg)), dim3(256), 0, st, R, rpitch, r0, dst, dstep, W, H, cn, ddepth, fullH, offY, border, p, seg);
    return true;
}

bool boxTwoPass(Stager& stg, const BoxParams& p, const CallImages& im, int cn, int sdepth, int ddepth, int border)
{
    static const bool off = [] { const char* v = getenv("MI355CV_BOX_TWOPASS"); return v && atoi(v) == 0; }();
    if (off || p.kw * p.kh < 16 || p.kw > 1024 || cn > 64 || sdepth == D64F || divUp(im.H, 32) > 65535) return false;
    hipStream_t st = stream();
    int r0, r1;
    boxRowRange(im.H, p.kh, im.fullH, im.offY, border, &r0, &r1);
    if (r1 - r0 < 1 || r1 - r0 > 65535 || (sdepth != D8U && sdepth != D16U && sdepth != D16S && sdepth != D32F)) return false;
    // ONE scratch image of row sums (int or double) for the whole batch: the frames go through it one after the other, in stream order
    void* R = stg.scratch((((size_t)im.W * cn + 3) & ~(size_t)3) * (size_t)(r1 - r0) * (sdepth == D32F ? sizeof(double) : sizeof(int)));
    if (!R) return false;
    for (int f = 0; f < im.nframes; f++) {
        const uchar* s = im.src + (size_t)f * im.sframe; uchar* d = im.dst + (size_t)f * im.dframe;
        switch (sdepth) {
        case D8U:  boxTwoPassT<uchar, int>(R, p, s, im.sstep, d, im.dstep, im.W, im.H, cn, ddepth, im.fullW, im.fullH, im.offX, im.offY, border, st); break;
        case D16U: boxTwoPassT<unsigned short, int>(R, p, s, im.sstep, d, im.dstep, im.W, im.H, cn, ddepth, im.fullW, im.fullH, im.offX, im.offY, border, st); break;
        case D16S: boxTwoPassT<short, int>(R, p, s, im.sstep, d, im.dstep, im.W, im.H, cn, ddepth, im.fullW, im.fullH, im.offX, im.offY, border, st); break;
        default:   boxTwoPassT<float, double>(R, p, s, im.sstep, d, im.dstep, im.W, im.H, cn, ddepth, im.fullW, im.fullH, im.offX, im.offY, border, st); break;
        }
    }
    noteKernel("k_box_rows + k_box_cols %dx%d window, depth %d -> %d, %d channel(s), %d frame(s)", p.kw, p.kh, sdepth, ddepth, cn, im.nframes);
    return true;
}

// CV_8U -> CV_8U windows the rolling kernels do not take (9 .. 129 per axis, any anchor, 2 channels, ROI windows): the window sum is two products with banded matrices of
// ones -- k_sepmx (sepmx.hip) computes it exactly on the matrix cores, nx + ny "taps" per byte instead of the kw * kh loads of k_box_generic, and finishes with the
// reference's own normalisation.
bool boxOnMatrixCores(Stager& stg, const BoxParams& p, const CallImages& im, int cn, int sdepth, int ddepth, int border)
{
    if (sdepth != D8U || ddepth != D8U || cn > 4 || p.mode == 2 || p.kw > lim::BOX_MAX_KSIZE || p.kh > lim::BOX_MAX_KSIZE) return false;      // (the kernel declines rows of taps beyond its K steps: 255 for one channel)
    if (std::getenv("MI355CV_SEPMX") && std::getenv("MI355CV_SEPMX")[0] == '0') return false;
    uint16_t ones[lim::BOX_MAX_KSIZE];
    for (int i = 0; i < lim::BOX_MAX_KSIZE; i++) ones[i] = 1;
    const SepmxBox b = {!p.normalize ? 3 : p.mode == 0 ? 1 : 2, p.divScale, p.divDelta, p.scaleF, p.scaleD};
    return sepmxRun(stg, im.src, im.sstep, im.sframe, im.dst, im.dstep, im.dframe, im.nframes, im.W, im.H, cn, im.fullW, im.fullH, im.offX, im.offY, border, ones, p.kw, p.ax, ones, p.kh, p.ay, stream(), &b);
}

// the served paths in order, for the hook's image and for a batch alike: the first that takes the call launches it
int boxServe(Stager& stg, const char* entry, const BoxParams& p, const CallImages& im, int cn, int sdepth, int ddepth, int border)
{
    const Roi roiv = {im.fullW, im.fullH, im.offX, im.offY};
    const Roi* roi = im.whole() ? nullptr : &roiv;                     // a submatrix with real pixels around it: the rolling kernels store the window
    const bool centred = p.kw == p.kh && p.ax == p.kw / 2 && p.ay == p.kh / 2;
    if (p.mode == 0 && p.normalize && centred &&
        seprollBox(im.src, im.sstep, im.sframe, im.dst, im.dstep, im.dframe, im.nframes, im.W, im.H, cn, p.kw, (unsigned)p.divScale, (unsigned)p.divDelta, border, stream(), roi))
        return stg.finish(entry);
    if (p.mode == 2 && sdepth == D32F && ddepth == D32F && cn == 1 && centred &&
        seprollBoxF32(im.src, im.sstep, im.sframe, im.dst, im.dstep, im.dframe, im.nframes, im.W, im.H, p.kw, p.normalize != 0, border, stream(), roi))
        return stg.finish(entry);
    if (boxOnMatrixCores(stg, p, im, cn, sdepth, ddepth, border)) return stg.finish(entry);
    if (boxTwoPass(stg, p, im, cn, sdepth, ddepth, border)) return stg.finish(entry);
    const dim3 grid(divUp(im.W * cn, 64), divUp(im.H, 4));
    for (int f = 0; f < im.nframes; f++)
        hipLaunchKernelGGL(k_box_generic, grid, dim3(256), 0, stream(), im.src + (size_t)f * im.sframe, im.sstep, im.dst + (size_t)f * im.dframe, im.dstep, im.W, im.H, cn,
                           sdepth, ddepth, im.fullW, im.fullH, im.offX, im.offY, border, p);
    noteKernel("k_box_generic %dx%d window, depth %d -> %d, %d channel(s)", p.kw, p.kh, sdepth, ddepth, cn);
    return stg.finish(entry);
}

// nframes == 0: the hook (one image, margins, host or device); nframes >= 1: a batch of device-resident whole frames
int boxRun(const char* entry, const uchar* src_data, size_t src_step, size_t sframe, uchar* dst_data, size_t dst_step, size_t dframe, int nframes, int width, int height,
           int src_depth, int dst_depth, int cn, int margin_left, int margin_top, int margin_right, int margin_bottom,
           size_t ksize_width, size_t ksize_height, int anchor_x, int anchor_y, bool normalize, int border_type)
{
    MI355_DECLINE_IF(disabled() || width <= 0 || height <= 0 || cn < 1 || cn > 512 || inPlaceOnDevice(src_data, dst_data));
    // cv::boxFilter hands its `ddepth` argument through as the caller gave it (box_filter.dispatch.cpp:451-474): a caller that passed a TYPE there (CV_8UC2 = 8 --
    // the reference's own Imgproc_Blur test does) arrives with channel bits set; the destination Mat was created from CV_MAKETYPE(ddepth, cn), i.e. from the depth bits
    src_depth = MI355CV_MAT_DEPTH(src_depth); dst_depth = MI355CV_MAT_DEPTH(dst_depth);
    const int kw = (int)ksize_width, kh = (int)ksize_height;
    MI355_DECLINE_IF(kw < 1 || kh < 1 || kw > lim::BOX_MAX_KSIZE || kh > lim::BOX_MAX_KSIZE);
    const int border = border_type & ~MI355CV_BORDER_ISOLATED;
    MI355_DECLINE_IF(border < 0 || border > B_REFLECT_101);
    // integer sources: int sums into any of the destination depths the reference has a ColumnSum<int, T> for (8U -> 16S is what an un-normalised cv::boxFilter of
    // bytes usually asks for); a signed source into an unsigned destination is left to the caller's path
    const bool okDepth = (src_depth == D8U && (dst_depth == D8U || dst_depth == D16U || dst_depth == D16S || dst_depth == D32F)) ||
                         (src_depth == D16U && (dst_depth == D8U || dst_depth == D16U || dst_depth == D16S || dst_depth == D32F)) ||
                         (src_depth == D16S && (dst_depth == D16S || dst_depth == D32F)) ||
                         (src_depth == D32F && (dst_depth == D32F || dst_depth == D64F)) || (src_depth == D64F && dst_depth == D64F) ||
                         ((src_depth == D8U || src_depth == D16U || src_depth == D16S) && dst_depth == D64F);
    if (!okDepth) return setError(MI355CV_NOT_IMPLEMENTED, "boxFilter: depth pair %d -> %d outside the GPU path", src_depth, dst_depth);
    BoxParams p; memset(&p, 0, sizeof p);
    p.kw = kw; p.kh = kh;
    p.ax = anchor_x < 0 ? kw / 2 : anchor_x; p.ay = anchor_y < 0 ? kh / 2 : anchor_y;
    MI355_DECLINE_IF(p.ax >= kw || p.ay >= kh);
    p.normalize = normalize ? 1 : 0;
    const int area = kw * kh;
    const double scale = 1.0 / area;
    p.scaleD = scale; p.scaleF = (float)scale;
    if (normalize && area == 1) p.normalize = 0;                       // scale == 1: the reference skips the multiply
    if (src_depth == D32F || src_depth == D64F) p.mode = 2;
    else if (src_depth == D8U && dst_depth == D8U && area <= 256) {
        p.mode = 0;
        // ColumnSum<ushort,uchar> constructor (box_filter.simd.hpp:441-455)
        const int d = (int)nearbyint(1.0 / scale);
        double scalef = ((double)(1 << 23)) / d;
        p.divScale = (int)std::floor(scalef);
        scalef -= p.divScale;
        p.divDelta = d / 2;
        if (scalef < 0.5) p.divDelta++; else p.divScale++;
    } else {
        p.mode = 1;
        const long long lim = src_depth == D8U ? (1LL << 23) : src_depth == D16U ? (1LL << 15) : (1LL << 16);
        MI355_DECLINE_IF(normalize && area > lim);    // the reference switches to double sums there
    }
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src_data, (size_t)width * height, minPixels(HOST_HEAVY)));
    if (nframes >= 1) {
        if (!isDevicePtr(src_data) || !isDevicePtr(dst_data)) return setError(MI355CV_NOT_IMPLEMENTED, "%s: batch entry needs device-resident frames", entry);
        if (nframes == 1) { sframe = 0; dframe = 0; }
        const CallImages im = {src_data, src_step, sframe, dst_data, dst_step, dframe, nframes, width, height, width, height, 0, 0};
        return boxServe(stg, entry, p, im, cn, src_depth, dst_depth, border);
    }
    // the hook: stage the whole parent region so that non-isolated borders can read real neighbours
    const int se = depthBytes(src_depth), de = depthBytes(dst_depth);
    const int fullW = margin_left + width + margin_right, fullH = margin_top + height + margin_bottom;
    size_t dss, dds;
    const uchar* top = src_data - (ptrdiff_t)margin_top * (ptrdiff_t)src_step - (ptrdiff_t)margin_left * cn * se;
    const uchar* dtop = stg.in(top, src_step, (size_t)fullW * cn * se, fullH, &dss);
    uchar* dd = stg.out(dst_data, dst_step, (size_t)width * cn * de, height, &dds);
    MI355_DECLINE_IF(!dtop || !dd);
    const CallImages im = {dtop + (size_t)margin_top * dss + (size_t)margin_left * cn * se, dss, 0, dd, dds, 0, 1, width, height, fullW, fullH, margin_left, margin_top};
    return boxServe(stg, entry, p, im, cn, src_depth, dst_depth, border);
}

} // namespace

extern "C" {

// ---- a batch of device-resident whole frames (frame strides in bytes; borders are per frame, i.e. isolated)
MI355CV_API int mi355cv_boxFilterBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, uchar* dst_data, size_t dst_step, size_t dst_frame_stride,
        int nframes, int width, int height, int src_depth, int dst_depth, int cn, size_t ksize_width, size_t ksize_height, int anchor_x, int anchor_y, bool normalize,
        int border_type)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(nframes < 1);
    if (width > 0 && height > 0 && hostBatchEligible(src_data, dst_data, nframes)) {            // frames in host memory: chunks through two sets of device buffers
        const HostBatch hb = {src_data, src_step, src_frame_stride, (size_t)width * cn * depthBytes(src_depth), height, dst_data, dst_step, dst_frame_stride, (size_t)width * cn * depthBytes(dst_depth), height, nframes};
        return runHostBatch("boxFilterBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_boxFilterBatch(s, ss, sf, d, ds, df, nf, width, height, src_depth, dst_depth, cn, ksize_width, ksize_height, anchor_x, anchor_y, normalize, border_type); });
    }
    return boxRun("boxFilterBatch", src_data, src_step, src_frame_stride, dst_data, dst_step, dst_frame_stride, nframes, width, height, src_depth, dst_depth, cn,
                  0, 0, 0, 0, ksize_width, ksize_height, anchor_x, anchor_y, normalize, border_type);
}

MI355CV_API int mi355cv_boxFilter(const uchar* src_data, size_t src_step, uchar* dst_data, size_t dst_step, int width, int height,
        int src_depth, int dst_depth, int cn, int margin_left, int margin_top, int margin_right, int margin_bottom,
        size_t ksize_width, size_t ksize_height, int anchor_x, int anchor_y, bool normalize, int border_type)
{
    mi355::EntryGuard entry_(__func__);
    return boxRun("boxFilter", src_data, src_step, 0, dst_data, dst_step, 0, 0, width, height, src_depth, dst_depth, cn, margin_left, margin_top, margin_right, margin_bottom,
                  ksize_width, ksize_height, anchor_x, anchor_y, normalize, border_type);
}

} // extern "C"
