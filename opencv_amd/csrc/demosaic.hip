// demosaic.hip -- cv::demosaicing / the Bayer codes of cv::cvtColor (imgproc/src/demosaicing.cpp, Bayer2RGB_ / Bayer2Gray_; the reference has no HAL hook for
// them): bilinear interpolation of a CV_8UC1 / CV_16UC1 Bayer mosaic into BGR (dcn 3), BGRA (dcn 4, alpha = the depth's maximum) or gray (dcn 1).
//
// Reference semantics (restated in demosaic_math.h, which holds every line of arithmetic used here): pattern 0..3 = BG, GB, RG, GR relative to the origin of the
// image handed in; interior pixels from their 3 x 3 neighbourhood with round-half-up integer averages; the one-pixel border is a copy of the neighbouring interior
// column, then row (so output (y, x) is the interior result of site (clamp(y, 1, h-2), clamp(x, 1, w-2))).  RGB order is the callers' business: they pass the pattern
// with red and blue exchanged.
//
//   k_demosaic_roll<DCN>  CV_8UC1 with at least 16 columns and 16-byte aligned source rows.  The roll.h skeleton (RX = RY = 1, CN = 1): a lane owns 16 source
//                         bytes of a row and walks down a segment of rows with the last three rows in registers -- per row its own bytes, the 16-bit pair sums
//                         left + right and the v_lerp_u8 average of left and right -- loads running D rows ahead through a ring, neighbours by DPP and one side
//                         load per row at the wave edge, ragged widths by the skeleton's last-chunk rule.  The pattern phase of a row (which columns are green,
//                         whether the others are blue) is wave-uniform and follows the ABSOLUTE row, so a segment may start on either row of the pattern.  Border
//                         columns are byte moves inside the finished colour planes (column 0 := column 1, column w-1 := column w-2, the latter from the
//                         previous lane by DPP when it is the only column of the last chunk); border rows are a second store of rows 1 / h-2.  A lane's 48 / 64
//                         destination bytes go out as dwordx4 stores, transposed through LDS into row-contiguous 1 KiB pieces per wave (roll.h storeT) unless
//                         MI355CV_DEMOSAIC_STORE=lanes asks for the lane-contiguous layout.  Compulsory traffic 1 + dcn bytes per pixel.
//   k_demosaic<T, DCN>    everything else served (CV_16U, unaligned rows, narrow images): a thread per destination pixel, the border as index clamps on the
//                         output coordinate.
#include "rt.h"
#include "roll.h"
#include "demosaic_math.h"
#include <algorithm>
#include <cstring>

using namespace mi355;

namespace {

enum { D8U = MI355CV_8U, D16U = MI355CV_16U };

// ---------------------------------------------------------------------------------- generic
template <typename T, int DCN>
__global__ __launch_bounds__(256) void k_demosaic(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h,
                                                  uchar* __restrict__ dst, size_t dstep, size_t dframe, int pattern, int ybase)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = ybase + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    src += (size_t)blockIdx.z * sframe; dst += (size_t)blockIdx.z * dframe;
    const int sx = demosaic::clampIdx(x, w), sy = demosaic::clampIdx(y, h);
    const T* r0 = reinterpret_cast<const T*>(src + (size_t)(sy - 1) * sstep) + sx;
    const T* r1 = reinterpret_cast<const T*>(src + (size_t)sy * sstep) + sx;
    const T* r2 = reinterpret_cast<const T*>(src + (size_t)(sy + 1) * sstep) + sx;
    const uint32_t c = r1[0], H = (uint32_t)r1[-1] + r1[1], V = (uint32_t)r0[0] + r2[0], D = (uint32_t)r0[-1] + r0[1] + r2[-1] + r2[1];
    const int green = demosaic::isGreen(pattern, sy, sx), rb = demosaic::rowBlue(pattern, sy);
    T* d = reinterpret_cast<T*>(dst + (size_t)y * dstep) + (size_t)x * DCN;
    if constexpr (DCN == 1) d[0] = (T)demosaic::gray(demosaic::grayWeights(green, rb), c, H, V, D);
    else {
        uint32_t b, g, r;
        demosaic::bgr(green, rb, c, H, V, D, b, g, r);
        d[0] = (T)b; d[1] = (T)g; d[2] = (T)r;
        if constexpr (DCN == 4) d[3] = (T)~(T)0;
    }
}

// ---------------------------------------------------------------------------------- rolling, CV_8UC1
// Work items (strip of 64 chunks x segment of rows x frame) as in roll.h, every segment walked downwards.  A segment [y0, y1) computes the interior rows
// clamp(y0) .. clamp(y1 - 1) and stores each to every row of the segment it stands for, so a segment that holds only row h-1 recomputes row h-2.
template <int DCN, int D>
__global__ __launch_bounds__(256) void k_demosaic_roll(const uchar* __restrict__ src, size_t sstep, size_t sframe, uchar* __restrict__ dst, size_t dstep, size_t dframe,
                                                       int W, int H, int nchunks, int nstrips, int segRows, int nseg, int nframes, int pattern, int transposed)
{
    typedef roll::Ctx<1, 1, 1> Cx;
    typedef typename Cx::RawT RawT;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    Cx cx;
    if (!cx.init(src, sstep, sframe, W, H, nchunks, nstrips, segRows, nseg, nframes, B_REFLECT_101, 0)) return;      // (the halo columns outside the image feed
                                                                                                                      // only columns 0 and w-1, which are replaced)
    if constexpr (DCN > 1) {
        __shared__ __attribute__((aligned(16))) uchar tscratch[4 * Cx::template tldsBytesPerWave<DCN>()];           // roll.h: transposed stores
        if (transposed) cx.useLds(tscratch, Cx::template tldsBytesPerWave<DCN>());
    }
    dst += (size_t)cx.frame * dframe;
    // the border columns as byte selectors on (previous dword, dword) of a finished plane: identity everywhere but column 0 := column 1 and column W-1 := column W-2
    uint32_t bsel[4] = {0x03020100u, 0x03020100u, 0x03020100u, 0x03020100u};
    const bool edges = cx.hasFirst || cx.hasLast;                       // wave-uniform
    {
        const int e = W - 1 - 16 * (nchunks - 1);                       // column W-1 inside the last chunk
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k == 0 && cx.c == 0) bsel[k] = 0x03020101u;
            if (cx.isLastChunk && k == (e >> 2)) {
                const uint32_t sh = 8u * (uint32_t)(e & 3);
                bsel[k] = (bsel[k] & ~(0xffu << sh)) | (((e & 3) ? (uint32_t)(e & 3) - 1u : 7u) << sh);
            }
        }
    }
    auto fixEdges = [&](uint32_t (&p)[4]) {
        const uint32_t fromLeft = __builtin_amdgcn_update_dpp(0u, p[3], 0x138, 0xf, 0xf, false);      // wave_shr:1 -- the previous lane's columns 12 .. 15
        uint32_t q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = demosaic::bytePerm(k ? p[k - 1] : fromLeft, p[k], bsel[k]);
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = q[k];
    };
    struct Row { uint32_t c[4], se[4], so[4], hl[4]; };              // own bytes, left + right as pair sums (even / odd columns), avg2(left, right)
    auto hpass = [&](Row& o, const RawT& raw) {
        uint32_t X[Cx::NW];                                         // X[0] = columns x0-4 .. x0-1, X[1..4] own, X[5] = x0+16 .. x0+19
        cx.window(X, raw);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t l = demosaic::leftOf(X[k], X[k + 1]), r = demosaic::rightOf(X[k + 1], X[k + 2]);
            o.c[k] = X[k + 1]; o.se[k] = demosaic::sum2e(l, r); o.so[k] = demosaic::sum2o(l, r);
            o.hl[k] = DCN > 1 ? demosaic::avg2(l, r) : 0u;                   // (gray needs no averages)
        }
    };
    auto storeRow = [&](int y, const uint32_t (&o)[4 * DCN]) {
        if constexpr (DCN > 1) {
            if (cx.transposes()) { cx.template storeT<DCN>(dst, dstep, y, o); return; }
        }
        if (!cx.active) return;
        uchar* p = dst + (size_t)y * dstep + (size_t)cx.c * (16 * DCN);
        const int n = (cx.rag && cx.isLastChunk) ? cx.vb : 16;      // columns of this chunk inside the image
        if (n == 16) {
#pragma unroll
            for (int q = 0; q < DCN; q++) __builtin_nontemporal_store(u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]}, reinterpret_cast<u32x4*>(p) + q);
        } else {
#pragma unroll
            for (int e = 0; e < 16 * DCN; e++)
                if (e < n * DCN) p[e] = (uchar)(o[e >> 2] >> (8 * (e & 3)));
        }
    };
    // row y from the rows above, at and below it
    auto emit = [&](int y, const Row& u, const Row& m, const Row& d) {
        const int ge = demosaic::greenEven(pattern, y), rb = demosaic::rowBlue(pattern, y);
        uint32_t o[4 * DCN];
        if constexpr (DCN == 1) {
            const demosaic::GrayW we = demosaic::grayWeights(ge, rb), wo = demosaic::grayWeights(ge ^ 1, rb);
#pragma unroll
            for (int k = 0; k < 4; k++)
                o[k] = demosaic::grayQuad(we, wo, m.c[k], m.se[k], m.so[k], demosaic::sum2e(u.c[k], d.c[k]), demosaic::sum2o(u.c[k], d.c[k]), u.se[k] + d.se[k], u.so[k] + d.so[k]);
            if (edges) fixEdges(o);
        } else {
            const uint32_t mg = demosaic::greenMask(ge);
            uint32_t pb[4], pg[4], pr[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t v = demosaic::avg2(u.c[k], d.c[k]);
                const uint32_t hv = demosaic::avg4(m.se[k], m.so[k], demosaic::sum2e(u.c[k], d.c[k]), demosaic::sum2o(u.c[k], d.c[k]));
                const uint32_t dg = demosaic::avg4(u.se[k], u.so[k], d.se[k], d.so[k]);
                demosaic::planes(mg, rb, m.c[k], m.hl[k], v, hv, dg, pb[k], pg[k], pr[k]);
            }
            if (edges) { fixEdges(pb); fixEdges(pg); fixEdges(pr); }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t t[DCN];
                if constexpr (DCN == 3) demosaic::interleave3(pb[k], pg[k], pr[k], t);
                else demosaic::interleave4(pb[k], pg[k], pr[k], t);
#pragma unroll
                for (int j = 0; j < DCN; j++) o[DCN * k + j] = t[j];
            }
        }
        if (y >= cx.y0 && y < cx.y1) storeRow(y, o);                  // (a segment that holds only row 0 or row h-1 computes a row of its neighbour's)
        if (y == 1 && cx.y0 == 0) storeRow(0, o);
        if (y == H - 2 && cx.y1 == H) storeRow(H - 1, o);
    };
    const int r0 = demosaic::clampIdx(cx.y0, H), r1 = demosaic::clampIdx(cx.y1 - 1, H);      // interior rows this segment computes; rows r0-1 .. r1+1 are all inside the image
    Row a, b;
    {
        RawT ra, rb; int v;
        cx.issueImg(ra, r0 - 1, v); cx.issueImg(rb, r0, v);
        hpass(a, ra); hpass(b, rb);
    }
    RawT raw[D]; int rv;
#pragma unroll
    for (int u = 0; u < D; u++) cx.issueImg(raw[u], min(r0 + 1 + u, H - 1), rv);
    for (int t = 0; r0 + t <= r1; t += D) {
#pragma unroll
        for (int u = 0; u < D; u++) {
            if (r0 + t + u <= r1) {
                Row c;
                hpass(c, raw[u]);
                cx.issueImg(raw[u], min(r0 + 1 + t + u + D, H - 1), rv);
                emit(r0 + t + u, a, b, c);
                a = b; b = c;
            }
        }
    }
}

constexpr int ROLL_D = 4;

// grid.y and grid.z hold 65535 each: longer batches take several launches (the height is bounded by DEMOSAIC_MAX_DIM)
template <typename T, int DCN>
void launchGeneric(const uchar* s, size_t ss, size_t sf, int w, int h, uchar* d, size_t ds, size_t df, int nframes, int pattern, hipStream_t st)
{
    for (int f0 = 0; f0 < nframes; f0 += 65535) {
        const dim3 grid(divUp(w, 64), divUp(h, 4), std::min(65535, nframes - f0));
        hipLaunchKernelGGL((k_demosaic<T, DCN>), grid, dim3(256), 0, st, s + (size_t)f0 * sf, ss, sf, w, h, d + (size_t)f0 * df, ds, df, pattern, 0);
    }
}

template <int DCN>
void launchRoll(const uchar* s, size_t ss, size_t sf, int w, int h, uchar* d, size_t ds, size_t df, int nframes, int pattern, int transposed, const roll::Geom& g, hipStream_t st)
{
    hipLaunchKernelGGL((k_demosaic_roll<DCN, ROLL_D>), dim3(g.blocks), dim3(256), 0, st, s, ss, sf, d, ds, df, w, h, g.nchunks, g.nstrips, g.seg, g.nseg, nframes, pattern, transposed);
}

// device-resident images: the rolling kernel where its geometry applies, the per-pixel kernel otherwise
void launchDemosaic(const uchar* s, size_t ss, size_t sf, int w, int h, uchar* d, size_t ds, size_t df, int nframes, int depth, int dcn, int pattern, hipStream_t st)
{
    if (depth == D8U && (((uintptr_t)s | ss | sf) & 15) == 0 && roll::eligible(s, ss, sf, d, ds, df, w, 1, 1, B_REFLECT_101)) {
        // segments of at most 32 rows, down to 7 when the batch is small, so that every SIMD still gets several waves.  Any length is valid for the kernel (the
        // tuning overrides roll::geometry reads from the environment change it); the odd minimum makes the segments of a single call start on rows of both parities
        const roll::Geom g = roll::geometry(w, h, 1, nframes, 32, 7, 16, 4096);
        const char* lay = std::getenv("MI355CV_DEMOSAIC_STORE");            // "lanes": lane-contiguous 48 / 64-byte stores instead of the transposed ones (measurements)
        const int transposed = !(lay && !strcmp(lay, "lanes"));
        if (dcn == 1) launchRoll<1>(s, ss, sf, w, h, d, ds, df, nframes, pattern, transposed, g, st);
        else if (dcn == 3) launchRoll<3>(s, ss, sf, w, h, d, ds, df, nframes, pattern, transposed, g, st);
        else launchRoll<4>(s, ss, sf, w, h, d, ds, df, nframes, pattern, transposed, g, st);
        noteKernel("k_demosaic_roll<%d,%d> blocks=%u x256 strips=%d seg=%d rows x %d, %d frame(s), %s stores", dcn, ROLL_D, g.blocks, g.nstrips, g.seg, g.nseg, nframes,
                   dcn == 1 ? "row" : transposed ? "transposed" : "lane");
        return;
    }
    if (depth == D8U) {
        if (dcn == 1) launchGeneric<uchar, 1>(s, ss, sf, w, h, d, ds, df, nframes, pattern, st);
        else if (dcn == 3) launchGeneric<uchar, 3>(s, ss, sf, w, h, d, ds, df, nframes, pattern, st);
        else launchGeneric<uchar, 4>(s, ss, sf, w, h, d, ds, df, nframes, pattern, st);
    } else {
        if (dcn == 1) launchGeneric<unsigned short, 1>(s, ss, sf, w, h, d, ds, df, nframes, pattern, st);
        else if (dcn == 3) launchGeneric<unsigned short, 3>(s, ss, sf, w, h, d, ds, df, nframes, pattern, st);
        else launchGeneric<unsigned short, 4>(s, ss, sf, w, h, d, ds, df, nframes, pattern, st);
    }
    noteKernel("k_demosaic<depth %d,%d> grid=%dx%dx%d x256, %d launch(es)", depth, dcn, divUp(w, 64), divUp(h, 4), std::min(65535, nframes), divUp(nframes, 65535));
}

// the refusals that need no device; 0 when the arguments are served
int demosaicArgs(const void* src, size_t sstep, size_t sframe, const void* dst, size_t dstep, size_t dframe, int w, int h, int nframes, int depth, int dcn, int pattern)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!src || !dst || nframes < 1);
    MI355_DECLINE_IF(!(depth == D8U || depth == D16U));
    MI355_DECLINE_IF(!(dcn == 1 || dcn == 3 || dcn == 4));
    MI355_DECLINE_IF(pattern < 0 || pattern > 3);
    // below 3 x 3 there is no interior pixel (the reference fills such a destination with zeros): left to it
    MI355_DECLINE_IF(w < 3 || h < 3);
    MI355_DECLINE_IF(w > lim::DEMOSAIC_MAX_DIM || h > lim::DEMOSAIC_MAX_DIM);
    const size_t e = depthBytes(depth);
    MI355_DECLINE_IF(sstep < (size_t)w * e || dstep < (size_t)w * dcn * e);
    if (((uintptr_t)src | sstep | sframe | (uintptr_t)dst | dstep | dframe) & (e - 1)) return MI355_DECLINED("pointer, pitch or frame stride not a multiple of the element size");
    return 0;
}

int runDemosaic(const char* entry, const uchar* src, size_t sstep, size_t sframe, uchar* dst, size_t dstep, size_t dframe, int w, int h, int nframes, int depth, int dcn, int pattern)
{
    if (const int rc = demosaicArgs(src, sstep, sframe, dst, dstep, dframe, w, h, nframes, depth, dcn, pattern)) return rc;
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels()));
    const size_t e = depthBytes(depth);
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + w * e, dspan = (size_t)(nframes - 1) * dframe + (size_t)(h - 1) * dstep + w * dcn * e;
    MI355_DECLINE_IF(overlapOnDevice(src, sspan, dst, dspan));
    size_t dss = sstep, dds = dstep;
    const uchar* ds = src; uchar* dd = dst;
    if (nframes == 1) {
        ds = stg.in(src, sstep, w * e, h, &dss);
        dd = stg.out(dst, dstep, w * dcn * e, h, &dds);
        MI355_DECLINE_IF(!ds || !dd);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(dst));
    launchDemosaic(ds, dss, sframe, w, h, dd, dds, dframe, nframes, depth, dcn, pattern, stream());
    MI355_CHECK_LAUNCH(entry);
    return stg.finish(entry);
}

} // namespace

extern "C" {

MI355CV_API int mi355cv_demosaic(const uchar* src, size_t src_step, uchar* dst, size_t dst_step, int width, int height, int depth, int dcn, int pattern)
{
    mi355::EntryGuard entry_(__func__);
    return runDemosaic("demosaic", src, src_step, 0, dst, dst_step, 0, width, height, 1, depth, dcn, pattern);
}

MI355CV_API int mi355cv_demosaicBatch(const uchar* src, size_t src_step, size_t src_frame_stride, uchar* dst, size_t dst_step, size_t dst_frame_stride,
                                      int width, int height, int nframes, int depth, int dcn, int pattern)
{
    mi355::EntryGuard entry_(__func__);
    if (const int rc = demosaicArgs(src, src_step, src_frame_stride, dst, dst_step, dst_frame_stride, width, height, nframes, depth, dcn, pattern)) return rc;
    if (hostBatchEligible(src, dst, nframes)) {        // frames in host memory
        const size_t e = depthBytes(depth);
        const HostBatch hb = {src, src_step, src_frame_stride, e * width, height, dst, dst_step, dst_frame_stride, e * dcn * width, height, nframes};
        return runHostBatch("demosaicBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_demosaicBatch(s, ss, sf, d, ds, df, width, height, nf, depth, dcn, pattern); });
    }
    return runDemosaic("demosaicBatch", src, src_step, nframes == 1 ? 0 : src_frame_stride, dst, dst_step, nframes == 1 ? 0 : dst_frame_stride, width, height,
                       nframes, depth, dcn, pattern);
}

} // extern "C"
