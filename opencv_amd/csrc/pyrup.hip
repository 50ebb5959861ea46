// pyrup.hip -- cv::pyrUp (imgproc/src/pyramids.cpp, pyrUp_<CastOp>; the reference has no HAL hook for it): the upward half of the image pyramid.
//
// Reference semantics (restated in pyrup_math.h, which holds every line of arithmetic used here): destination 2w x 2h, the source pixels at the even
// positions convolved with [1 4 6 4 1] / 8 per axis -- per axis  even 2i: s[i-1] + 6 s[i] + s[i+1],  odd 2i+1: 4 (s[i] + s[i+1]),  with
// s[-1] := s[min(1, n-1)] and s[n] := s[n-1] -- rows first, then columns, in int (8U / 16U / 16S, cast (v + 32) >> 6) or float (32F, cast v * (1/64)).
// Only BORDER_DEFAULT exists (the reference asserts it).
//
//   k_pyrup_roll   CV_8UC1, width a multiple of 8, 8-byte aligned source rows and 16-byte aligned destination rows.  The roll.h skeleton inverted: a lane
//                  owns 8 consecutive source bytes of a row (one dwordx2 load, neighbours from the adjacent lanes by DPP) and walks down a segment of
//                  rows, keeping the last three horizontally filtered rows in registers as 2 x u16 pairs (even sum, odd sum); every source row yields
//                  two destination rows of 16 bytes per lane, one dwordx4 store each, so a wave writes 1 KiB contiguous per row.  Compulsory traffic
//                  5 bytes per source pixel (1 read, 4 written).
//   k_pyrup<T>     everything else served: a thread per source element reads its 3 x 3 neighbourhood (index clamps at the edges) and writes the 2 x 2
//                  destination block.
#include "rt.h"
#include "roll.h"
#if defined(__HIP_DEVICE_COMPILE__)
#  define PYRUP_LSHL_ADD(a, n, b) mi355::lshlAdd((a), (n), (b))
#endif
#include "pyrup_math.h"
#include <algorithm>

using namespace mi355;

namespace {

enum { D8U = MI355CV_8U, D16U = MI355CV_16U, D16S = MI355CV_16S, D32F = MI355CV_32F };

// ---------------------------------------------------------------------------------- generic
template <typename T, typename W>
__global__ __launch_bounds__(256) void k_pyrup(const uchar* __restrict__ src, size_t sstep, size_t sframe, int sw, int sh,
                                               uchar* __restrict__ dst, size_t dstep, size_t dframe, int cn, int ybase)
{
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = ybase + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (e >= sw * cn || y >= sh) return;
    src += (size_t)blockIdx.z * sframe; dst += (size_t)blockIdx.z * dframe;
    const int x = e / cn, c = e - x * cn;
    const int xs[3] = {pyrup::lowIdx(x - 1, sw) * cn + c, e, pyrup::highIdx(x + 1, sw) * cn + c};
    const int ys[3] = {pyrup::lowIdx(y - 1, sh), y, pyrup::highIdx(y + 1, sh)};
    W s[3][3], o[4];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const T* row = reinterpret_cast<const T*>(src + (size_t)ys[r] * sstep);
#pragma unroll
        for (int k = 0; k < 3; k++) s[r][k] = (W)row[xs[k]];
    }
    pyrup::block<W>(s, o);
    T* d0 = reinterpret_cast<T*>(dst + (size_t)(2 * y) * dstep) + (size_t)(2 * x) * cn + c;
    T* d1 = reinterpret_cast<T*>(dst + (size_t)(2 * y + 1) * dstep) + (size_t)(2 * x) * cn + c;
    if constexpr (std::is_same<W, float>::value) {
        d0[0] = pyrup::castFlt(o[0]); d0[cn] = pyrup::castFlt(o[1]); d1[0] = pyrup::castFlt(o[2]); d1[cn] = pyrup::castFlt(o[3]);
    } else {
        d0[0] = (T)pyrup::castInt(o[0]); d0[cn] = (T)pyrup::castInt(o[1]); d1[0] = (T)pyrup::castInt(o[2]); d1[cn] = (T)pyrup::castInt(o[3]);
    }
}

// ---------------------------------------------------------------------------------- rolling, CV_8UC1
// D source rows in flight per wave.  Work items (strip of 64 chunks x segment of source rows x frame) as in roll.h, every segment walked downwards: the two
// rows a segment shares with its neighbours are 2 bytes against the 5 x segRows it moves per column.
template <int D>
__global__ __launch_bounds__(256) void k_pyrup_roll(const uchar* __restrict__ src, size_t sstep, size_t sframe, uchar* __restrict__ dst, size_t dstep, size_t dframe,
                                                    int W, int H, int nchunks, int nstrips, int segRows, int nseg, int nframes)
{
    typedef roll::Ctx<1, 0, 1, 8> Cx;
    typedef typename Cx::RawT RawT;
    Cx cx;
    if (!cx.init(src, sstep, sframe, W, H, nchunks, nstrips, segRows, nseg, nframes, B_REFLECT_101, 0)) return;      // left halo of the row: s[-1] = s[1]
    roll::selSetByte(cx.es.ra[0], cx.es.rb[0], cx.es.rc[0], 0, 7);                                                    // right halo: s[W] = s[W-1], byte 7 of the last chunk
    dst += (size_t)cx.frame * dframe + 16 * (size_t)cx.c;
    struct HRow { uint32_t h[8]; };                    // h[k] = (even sum, odd sum) of the lane's source pixel k as 2 x u16
    auto hpass = [&](HRow& o, const RawT& raw) {
        uint32_t X[Cx::NW];                            // X[0] = columns x0-4..x0-1, X[1..2] own, X[3] = x0+8..x0+11
        cx.window(X, raw);
        uint32_t b[10];                                // columns x0-1 .. x0+8
        b[0] = X[0] >> 24; b[9] = X[3] & 0xffu;
#pragma unroll
        for (int k = 0; k < 8; k++) b[1 + k] = (X[1 + (k >> 2)] >> (8 * (k & 3))) & 0xffu;
#pragma unroll
        for (int k = 0; k < 8; k++) o.h[k] = pyrup::hpair(b[k], b[k + 1], b[k + 2]);
    };
    auto rowOf = [&](int g) { return g < 0 ? pyrup::lowIdx(g, H) : pyrup::highIdx(g, H); };      // source row g in [-1, ...) -> a row of the image
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    HRow h0, h1;
    {
        RawT r0, r1; int v;
        cx.issueImg(r0, rowOf(cx.y0 - 1), v); cx.issueImg(r1, cx.y0, v);
        hpass(h0, r0); hpass(h1, r1);
    }
    RawT raw[D]; int rv;
#pragma unroll
    for (int u = 0; u < D; u++) cx.issueImg(raw[u], rowOf(cx.y0 + 1 + u), rv);
    for (int t = 0; t < cx.nrows; t += D) {
#pragma unroll
        for (int u = 0; u < D; u++) {
            if (t + u < cx.nrows) {
                HRow h2;
                hpass(h2, raw[u]);
                cx.issueImg(raw[u], rowOf(cx.y0 + 1 + t + u + D), rv);
                uint32_t we[8], wo[8];
#pragma unroll
                for (int k = 0; k < 8; k++) { we[k] = pyrup::vEven(h0.h[k], h1.h[k], h2.h[k]); wo[k] = pyrup::vOdd(h1.h[k], h2.h[k]); }
                if (cx.active) {
                    uchar* p = dst + (size_t)(2 * (cx.y0 + t + u)) * dstep;
                    u32x4 oe, oo;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        oe[j] = __builtin_amdgcn_perm(we[2 * j + 1], we[2 * j], 0x06040200u);
                        oo[j] = __builtin_amdgcn_perm(wo[2 * j + 1], wo[2 * j], 0x06040200u);
                    }
                    __builtin_nontemporal_store(oe, reinterpret_cast<u32x4*>(p));
                    __builtin_nontemporal_store(oo, reinterpret_cast<u32x4*>(p + dstep));
                }
                h0 = h1; h1 = h2;
            }
        }
    }
}

// grid.y and grid.z hold 65535 each: taller images and longer batches take several launches
template <typename T, typename W>
void launchGeneric(const uchar* ds, size_t dss, size_t sframe, int sw, int sh, uchar* dd, size_t dds, size_t dframe, int nframes, int cn, hipStream_t st)
{
    for (int f0 = 0; f0 < nframes; f0 += 65535)
        for (int y0 = 0; y0 < sh; y0 += 4 * 65535) {
            const dim3 grid(divUp(sw * cn, 64), divUp(std::min(4 * 65535, sh - y0), 4), std::min(65535, nframes - f0));
            hipLaunchKernelGGL((k_pyrup<T, W>), grid, dim3(256), 0, st, ds + (size_t)f0 * sframe, dss, sframe, sw, sh, dd + (size_t)f0 * dframe, dds, dframe, cn, y0);
        }
}

// one level up on device-resident images: the rolling kernel where its geometry applies, the per-element kernel otherwise
void launchPyrUp(const uchar* ds, size_t dss, size_t sframe, int sw, int sh, uchar* dd, size_t dds, size_t dframe, int nframes, int depth, int cn, hipStream_t st)
{
    if (depth == D8U && cn == 1 && sw % 8 == 0 && (((uintptr_t)ds | dss | sframe) & 7) == 0 && (((uintptr_t)dd | dds | dframe) & 15) == 0) {
        // segments of at most 32 source rows, down to 4 when the batch is small, so that every SIMD still gets several waves.  The tuning overrides
        // roll::geometry reads from the environment (MI355CV_ROLL_SEG / MI355CV_ROLL_WAVES) change these lengths; any length is valid for the kernel
        const roll::Geom g = roll::geometry(sw, sh, 1, nframes, 32, 4, 8, 4096);
        hipLaunchKernelGGL(k_pyrup_roll<4>, dim3(g.blocks), dim3(256), 0, st, ds, dss, sframe, dd, dds, dframe, sw, sh, g.nchunks, g.nstrips, g.seg, g.nseg, nframes);
        noteKernel("k_pyrup_roll<4> blocks=%u x256 strips=%d seg=%d rows x %d, %d frame(s)", g.blocks, g.nstrips, g.seg, g.nseg, nframes);
        return;
    }
    if (depth == D8U) launchGeneric<uchar, int>(ds, dss, sframe, sw, sh, dd, dds, dframe, nframes, cn, st);
    else if (depth == D16U) launchGeneric<unsigned short, int>(ds, dss, sframe, sw, sh, dd, dds, dframe, nframes, cn, st);
    else if (depth == D16S) launchGeneric<short, int>(ds, dss, sframe, sw, sh, dd, dds, dframe, nframes, cn, st);
    else launchGeneric<float, float>(ds, dss, sframe, sw, sh, dd, dds, dframe, nframes, cn, st);
    noteKernel("k_pyrup<depth %d> grid=%dx%dx%d x256 cn=%d, %d launch(es)", depth, divUp(sw * cn, 64), divUp(std::min(4 * 65535, sh), 4), std::min(65535, nframes), cn,
               divUp(sh, 4 * 65535) * divUp(nframes, 65535));
}

// the refusals that need no device; 0 when the arguments are served
int pyrUpArgs(const void* src, int sw, int sh, const void* dst, int dw, int dh, int nframes, int depth, int cn, int border)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!src || !dst || nframes < 1);
    if ((border & ~MI355CV_BORDER_ISOLATED) != B_REFLECT_101) return MI355_DECLINED("border != BORDER_DEFAULT");      // the reference asserts it
    MI355_DECLINE_IF(!(depth == D8U || depth == D16U || depth == D16S || depth == D32F) || cn < 1 || cn > 4);
    // 2 * sw * cn and 2 * sh are ints in the kernels
    MI355_DECLINE_IF(sw <= 0 || sh <= 0 || sw > (1 << 27) || sh > (1 << 29));
    // the reference also admits 2w +- 1 / 2h +- 1 (its last column / row then repeats or is dropped): left to it
    MI355_DECLINE_IF(dw != 2 * sw || dh != 2 * sh);
    return 0;
}

int runPyrUp(const char* entry, const uchar* src, size_t sstep, size_t sframe, int sw, int sh, uchar* dst, size_t dstep, size_t dframe, int dw, int dh,
             int nframes, int depth, int cn, int border)
{
    if (const int rc = pyrUpArgs(src, sw, sh, dst, dw, dh, nframes, depth, cn, border)) return rc;
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)sw * sh, minPixels()));
    const size_t e = (size_t)cn * depthBytes(depth);
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(sh - 1) * sstep + sw * e, dspan = (size_t)(nframes - 1) * dframe + (size_t)(dh - 1) * dstep + dw * e;
    MI355_DECLINE_IF(overlapOnDevice(src, sspan, dst, dspan));
    size_t dss = sstep, dds = dstep;
    const uchar* ds = src; uchar* dd = dst;
    if (nframes == 1) {
        ds = stg.in(src, sstep, sw * e, sh, &dss);
        dd = stg.out(dst, dstep, dw * e, dh, &dds);
        MI355_DECLINE_IF(!ds || !dd);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(dst));
    launchPyrUp(ds, dss, sframe, sw, sh, dd, dds, dframe, nframes, depth, cn, stream());
    MI355_CHECK_LAUNCH(entry);
    return stg.finish(entry);
}

} // namespace

extern "C" {

MI355CV_API int mi355cv_pyrup(const uchar* src_data, size_t src_step, int src_width, int src_height, uchar* dst_data, size_t dst_step,
                              int dst_width, int dst_height, int depth, int cn, int border_type)
{
    mi355::EntryGuard entry_(__func__);
    return runPyrUp("pyrup", src_data, src_step, 0, src_width, src_height, dst_data, dst_step, 0, dst_width, dst_height, 1, depth, cn, border_type);
}

MI355CV_API int mi355cv_pyrupBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int src_width, int src_height,
                                   uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int dst_width, int dst_height, int nframes,
                                   int depth, int cn, int border_type)
{
    mi355::EntryGuard entry_(__func__);
    if (const int rc = pyrUpArgs(src_data, src_width, src_height, dst_data, dst_width, dst_height, nframes, depth, cn, border_type)) return rc;
    if (hostBatchEligible(src_data, dst_data, nframes)) {        // frames in host memory
        const size_t pix = (size_t)cn * depthBytes(depth);
        const HostBatch hb = {src_data, src_step, src_frame_stride, pix * src_width, src_height, dst_data, dst_step, dst_frame_stride, pix * dst_width, dst_height, nframes};
        return runHostBatch("pyrupBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_pyrupBatch(s, ss, sf, src_width, src_height, d, ds, df, dst_width, dst_height, nf, depth, cn, border_type); });
    }
    return runPyrUp("pyrupBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, src_width, src_height, dst_data, dst_step,
                    nframes == 1 ? 0 : dst_frame_stride, dst_width, dst_height, nframes, depth, cn, border_type);
}

} // extern "C"
