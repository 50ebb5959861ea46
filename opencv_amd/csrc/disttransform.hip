// disttransform.hip -- cv::distanceTransform (imgproc/src/distransform.cpp; the reference has no HAL hook for it) on CV_8UC1: DIST_L2 with DIST_MASK_PRECISE,
// DIST_L1 and DIST_C, the exact distance to the nearest zero pixel.  Every line of arithmetic is in disttransform_math.h.
//
//   k_dist_sites   a thread per (column, segment of 64 rows): the zero pixels of the segment as the bits of one 64-bit word.  Lanes run along x.
//   k_dist_cols    a thread per (column, segment): the nearest site above and below the segment from the words of the other segments (the carry), then the
//                  vertical distance g of its 64 rows from two bit scans each, written as u16 to HBM scratch; CAP for a column without a site.
//                  A 4K frame is 60 waves x 34 segments instead of 60 waves walking 2160 rows.
//   k_dist_row     a workgroup per row: the row of g into LDS (2 bytes per column, at most 32 KiB), then every thread scans outward from its own columns
//                  (scanRow) and writes the final value -- the root for L2, the integer as float for L1 / C, saturated for L1 into CV_8U.  A row whose g
//                  are all CAP belongs to a frame without a site and gets NO_SITE_32F / NO_SITE_8U, so no pass needs the host to know.
// Neighbouring lanes read neighbouring u16 of the LDS row (two lanes per bank, one dword: a broadcast), so the scan is free of bank conflicts; its length is
// the distance itself, short on ordinary masks and O(width) per pixel for a lone site.
#include "rt.h"
#include "disttransform_math.h"
#include <algorithm>

using namespace mi355;
namespace dt = disttransform;

namespace {

typedef unsigned short ushort;

__global__ __launch_bounds__(256) void k_dist_sites(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h,
                                                    uint64_t* __restrict__ words, size_t wpitch, size_t wframe)
{
    const int x = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (x >= w) return;
    const uchar* p = src + (size_t)blockIdx.z * sframe + (size_t)s * dt::SEG * sstep + x;
    const int n = min(dt::SEG, h - s * dt::SEG);
    uint64_t m = 0;
    if (n == dt::SEG) {
#pragma unroll 16
        for (int i = 0; i < dt::SEG; i++) m |= (uint64_t)(p[(size_t)i * sstep] == 0) << i;
    } else {
        for (int i = 0; i < n; i++) m |= (uint64_t)(p[(size_t)i * sstep] == 0) << i;
    }
    words[(size_t)blockIdx.z * wframe + (size_t)s * wpitch + x] = m;
}

__global__ __launch_bounds__(256) void k_dist_cols(const uint64_t* __restrict__ words, size_t wpitch, size_t wframe, int w, int h, int nseg,
                                                   ushort* __restrict__ g, size_t gpitch, size_t gframe)
{
    const int x = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (x >= w) return;
    const uint64_t* col = words + (size_t)blockIdx.z * wframe + x;
    const uint64_t m = col[(size_t)s * wpitch];
    const uint32_t up = dt::carryUp(col, wpitch, s), down = dt::carryDown(col, wpitch, s, nseg);
    ushort* o = g + (size_t)blockIdx.z * gframe + (size_t)s * dt::SEG * gpitch + x;
    const int n = min(dt::SEG, h - s * dt::SEG);
    for (int i = 0; i < n; i++) o[(size_t)i * gpitch] = (ushort)dt::colDist(m, i, up, down);
}

template <int METRIC, typename T>
__global__ __launch_bounds__(256) void k_dist_row(const ushort* __restrict__ g, size_t gpitch, size_t gframe, int w,
                                                  uchar* __restrict__ dst, size_t dstep, size_t dframe)
{
    extern __shared__ ushort row[];                                  // w entries
    const ushort* gr = g + (size_t)blockIdx.y * gframe + (size_t)blockIdx.x * gpitch;
    int site = 0;
    for (int x = threadIdx.x; x < w; x += 256) { const ushort v = gr[x]; row[x] = v; site |= v < dt::CAP; }
    site = __syncthreads_or(site);
    T* out = reinterpret_cast<T*>(dst + (size_t)blockIdx.y * dframe + (size_t)blockIdx.x * dstep);
    for (int q = threadIdx.x; q < w; q += 256) {
        if constexpr (sizeof(T) == 1) out[q] = site ? dt::out8u(dt::scanRow<METRIC>(row, w, q)) : (uchar)dt::NO_SITE_8U;
        else out[q] = site ? dt::out32f<METRIC>(dt::scanRow<METRIC>(row, w, q)) : dt::NO_SITE_32F;
    }
}

const char* metricName(int metric) { return metric == dt::L2 ? "L2" : metric == dt::L1 ? "L1" : "C"; }

// HBM scratch of one frame: the site words (8 bytes per column and segment) and g (2 bytes per pixel), rows padded to 128 bytes
struct Geom { int nseg; size_t wpitch, wframe, gpitch, gframe, bytes; };
Geom geometry(int w, int h)
{
    Geom q;
    q.nseg = divUp(h, dt::SEG);
    q.wpitch = ((size_t)w + 15) & ~size_t(15);
    q.wframe = q.wpitch * q.nseg;
    q.gpitch = ((size_t)w + 63) & ~size_t(63);
    q.gframe = q.gpitch * h;
    q.bytes = q.wframe * sizeof(uint64_t) + q.gframe * sizeof(ushort);
    return q;
}

// the three passes over device-resident frames; the scratch is reused by groups of frames (one stream: a group starts after the one before it)
bool launchDist(Stager& stg, const uchar* ds, size_t dss, size_t sframe, int w, int h, uchar* dd, size_t dds, size_t dframe, int nframes, int metric, int depth,
                hipStream_t st)
{
    const Geom q = geometry(w, h);
    const int group = (int)std::min<size_t>({(size_t)nframes, (size_t)65535, std::max<size_t>(1, (size_t(128) << 20) / q.bytes)});
    uchar* scratch = (uchar*)stg.scratch(q.bytes * group);
    if (!scratch) return false;
    uint64_t* words = reinterpret_cast<uint64_t*>(scratch);
    ushort* g = reinterpret_cast<ushort*>(scratch + q.wframe * sizeof(uint64_t) * group);
    const size_t lds = (size_t)w * sizeof(ushort);
    for (int f0 = 0; f0 < nframes; f0 += group) {
        const int nf = std::min(group, nframes - f0);
        const uchar* s = ds + (size_t)f0 * sframe; uchar* d = dd + (size_t)f0 * dframe;
        const dim3 cgrid(divUp(w, 256), q.nseg, nf), rgrid(h, nf);
        hipLaunchKernelGGL(k_dist_sites, cgrid, dim3(256), 0, st, s, dss, sframe, w, h, words, q.wpitch, q.wframe);
        hipLaunchKernelGGL(k_dist_cols, cgrid, dim3(256), 0, st, words, q.wpitch, q.wframe, w, h, q.nseg, g, q.gpitch, q.gframe);
        if (metric == dt::L2) hipLaunchKernelGGL((k_dist_row<dt::L2, float>), rgrid, dim3(256), lds, st, g, q.gpitch, q.gframe, w, d, dds, dframe);
        else if (metric == dt::C) hipLaunchKernelGGL((k_dist_row<dt::C, float>), rgrid, dim3(256), lds, st, g, q.gpitch, q.gframe, w, d, dds, dframe);
        else if (depth == MI355CV_8U) hipLaunchKernelGGL((k_dist_row<dt::L1, uchar>), rgrid, dim3(256), lds, st, g, q.gpitch, q.gframe, w, d, dds, dframe);
        else hipLaunchKernelGGL((k_dist_row<dt::L1, float>), rgrid, dim3(256), lds, st, g, q.gpitch, q.gframe, w, d, dds, dframe);
    }
    noteKernel("k_dist_row<%s,%s> grid=%dx%d x256 lds=%zu, k_dist_sites + k_dist_cols grid=%dx%dx%d x256, %d frame(s) in groups of %d", metricName(metric),
               depth == MI355CV_8U ? "8U" : "32F", h, std::min(group, nframes), lds, divUp(w, 256), q.nseg, std::min(group, nframes), nframes, group);
    return true;
}

// the refusals that need no device; 0 when the arguments are served
int distArgs(const void* src, int w, int h, const void* dst, int nframes, int distanceType, int maskSize, int dstDepth)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!src || !dst || nframes < 1);
    if (distanceType != dt::L1 && distanceType != dt::L2 && distanceType != dt::C) return MI355_DECLINED("distanceType is not DIST_L1, DIST_L2 or DIST_C");
    if (maskSize != 0 && maskSize != 3 && maskSize != 5) return MI355_DECLINED("maskSize is not 0, 3 or 5");
    // DIST_L2 with a 3 x 3 or 5 x 5 mask is the reference's chamfer approximation, a raster-sequential recurrence: left to it
    if (distanceType == dt::L2 && maskSize != 0) return MI355_DECLINED("DIST_L2 with maskSize != DIST_MASK_PRECISE");
    if (dstDepth != MI355CV_32F && dstDepth != MI355CV_8U) return MI355_DECLINED("dstDepth is not CV_32F or CV_8U");
    if (dstDepth == MI355CV_8U && distanceType != dt::L1) return MI355_DECLINED("CV_8U output without DIST_L1");       // the reference asserts it
    // squared distances are 32-bit and g is 16-bit in the kernels (disttransform_math.h)
    MI355_DECLINE_IF(w <= 0 || h <= 0 || w > lim::DISTTRANSFORM_MAX_DIM || h > lim::DISTTRANSFORM_MAX_DIM);
    return 0;
}

int runDist(const char* entry, const uchar* src, size_t sstep, size_t sframe, int w, int h, uchar* dst, size_t dstep, size_t dframe, int nframes, int distanceType,
            int maskSize, int dstDepth)
{
    if (const int rc = distArgs(src, w, h, dst, nframes, distanceType, maskSize, dstDepth)) return rc;
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_HEAVY)));
    const size_t e = depthBytes(dstDepth);
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + w, dspan = (size_t)(nframes - 1) * dframe + (size_t)(h - 1) * dstep + w * e;
    MI355_DECLINE_IF(overlapOnDevice(src, sspan, dst, dspan));
    size_t dss = sstep, dds = dstep;
    const uchar* ds = src; uchar* dd = dst;
    if (nframes == 1) {
        ds = stg.in(src, sstep, w, h, &dss);
        dd = stg.out(dst, dstep, w * e, h, &dds);
        MI355_DECLINE_IF(!ds || !dd);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(dst));
    if (!launchDist(stg, ds, dss, sframe, w, h, dd, dds, dframe, nframes, distanceType, dstDepth, stream())) return MI355_DECLINED("no scratch");
    MI355_CHECK_LAUNCH(entry);
    return stg.finish(entry);
}

} // namespace

static_assert(lim::DISTTRANSFORM_MAX_DIM == dt::MAX_DIM, "one bound");

extern "C" {

MI355CV_API int mi355cv_distanceTransform(const uchar* src_data, size_t src_step, int width, int height, uchar* dst_data, size_t dst_step,
                                          int distance_type, int mask_size, int dst_depth)
{
    mi355::EntryGuard entry_(__func__);
    return runDist("distanceTransform", src_data, src_step, 0, width, height, dst_data, dst_step, 0, 1, distance_type, mask_size, dst_depth);
}

MI355CV_API int mi355cv_distanceTransformBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height,
                                               uchar* dst_data, size_t dst_step, size_t dst_frame_stride, int nframes,
                                               int distance_type, int mask_size, int dst_depth)
{
    mi355::EntryGuard entry_(__func__);
    if (const int rc = distArgs(src_data, width, height, dst_data, nframes, distance_type, mask_size, dst_depth)) return rc;
    if (hostBatchEligible(src_data, dst_data, nframes)) {        // frames in host memory
        const HostBatch hb = {src_data, src_step, src_frame_stride, (size_t)width, height, dst_data, dst_step, dst_frame_stride,
                              (size_t)width * depthBytes(dst_depth), height, nframes};
        return runHostBatch("distanceTransformBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_distanceTransformBatch(s, ss, sf, width, height, d, ds, df, nf, distance_type, mask_size, dst_depth); });
    }
    return runDist("distanceTransformBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, width, height, dst_data, dst_step,
                   nframes == 1 ? 0 : dst_frame_stride, nframes, distance_type, mask_size, dst_depth);
}

} // extern "C"
