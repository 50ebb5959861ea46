// probe.hip -- the streaming-copy yardsticks (mi355cv_copyProbe, mi355cv_copyProbeColwalk): what a kernel that moves one byte in and one byte out reaches on
// this device, measured in the same process as the kernel it is held against (bench.py, tools/*_bench.py).  They compute nothing and serve no hook.
#include "rt.h"

using namespace mi355;

namespace {

// 16 B/lane streaming copy with the same launch geometry as the rolling kernel's traffic (1 read :
// 1 write): the measured-copy denominator BASELINE.md asks for next to the 8 TB/s spec figure.
template <bool NT>
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ s, uint4* __restrict__ d, size_t n16, int perThread)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    size_t base = ((size_t)blockIdx.x * perThread) * 256 + threadIdx.x;
#pragma unroll 4
    for (int i = 0; i < perThread; i++) {
        size_t j = base + (size_t)i * 256;
        if (j < n16) {
            uint4 v = s[j];
            u32x4 ov = {v.x, v.y, v.z, v.w};
            if constexpr (NT) __builtin_nontemporal_store(ov, reinterpret_cast<u32x4*>(d + j));
            else d[j] = v;
        }
    }
}

// column-walk copy probe: the rolling kernel's work decomposition and access order (wave = 1 KB wide strip
// walking down `segRows` rows) with the arithmetic removed -- separates access-pattern effects from ALU/wait effects
template <int UNROLL>
__global__ __launch_bounds__(256) void k_copy_colwalk(const uchar* __restrict__ src, uchar* __restrict__ dst, size_t step, size_t frame,
                                                      int H, int nchunks, int nstrips, int segRows, int nseg, int nframes)
{
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int strip = wid % nstrips, t0 = wid / nstrips, seg = t0 % nseg, fr = t0 / nseg;
    if (fr >= nframes) return;
    const int c = strip * 64 + lane;
    if (c >= nchunks) return;
    const int y0 = seg * segRows, y1 = min(H, y0 + segRows);
    const uchar* s = src + (size_t)fr * frame + 16 * (size_t)c;
    uchar* d = dst + (size_t)fr * frame + 16 * (size_t)c;
    for (int y = y0; y < y1; y += UNROLL) {
        uint4 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) v[u] = *reinterpret_cast<const uint4*>(s + (size_t)min(y + u, y1 - 1) * step);
#pragma unroll
        for (int u = 0; u < UNROLL; u++) if (y + u < y1) *reinterpret_cast<uint4*>(d + (size_t)(y + u) * step) = v[u];
    }
}

} // namespace

extern "C" {

// streaming-copy probe: copies `bytes` (multiple of 16) device->device with 16 B/lane accesses
MI355CV_API int mi355cv_copyProbe(const void* src, void* dst, size_t bytes, int perThread, int nt)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(!ensureDevice() || (bytes & 15) || perThread < 1);
    size_t n16 = bytes / 16;
    size_t blocks = (n16 + (size_t)256 * perThread - 1) / ((size_t)256 * perThread);
    if (nt) hipLaunchKernelGGL((k_copy16<true>), dim3((unsigned)blocks), dim3(256), 0, stream(), (const uint4*)src, (uint4*)dst, n16, perThread);
    else    hipLaunchKernelGGL((k_copy16<false>), dim3((unsigned)blocks), dim3(256), 0, stream(), (const uint4*)src, (uint4*)dst, n16, perThread);
    if (hipGetLastError() != hipSuccess) return MI355CV_ERROR_UNKNOWN;
    if (!asyncMode()) (void)hipStreamSynchronize(stream());
    return MI355CV_OK;
}

MI355CV_API int mi355cv_copyProbeColwalk(const void* src, void* dst, int W, int H, int nframes, int segRows, int unroll)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(!ensureDevice() || (W & 15));
    const int nchunks = W / 16, nstrips = divUp(nchunks, 64), nseg = divUp(H, segRows);
    const long long items = (long long)nstrips * nseg * nframes;
    dim3 grid((unsigned)((items + 3) / 4));
    const uchar* s = (const uchar*)src; uchar* d = (uchar*)dst;
    if (unroll == 1) hipLaunchKernelGGL((k_copy_colwalk<1>), grid, dim3(256), 0, stream(), s, d, (size_t)W, (size_t)W * H, H, nchunks, nstrips, segRows, nseg, nframes);
    else if (unroll == 2) hipLaunchKernelGGL((k_copy_colwalk<2>), grid, dim3(256), 0, stream(), s, d, (size_t)W, (size_t)W * H, H, nchunks, nstrips, segRows, nseg, nframes);
    else if (unroll == 5) hipLaunchKernelGGL((k_copy_colwalk<5>), grid, dim3(256), 0, stream(), s, d, (size_t)W, (size_t)W * H, H, nchunks, nstrips, segRows, nseg, nframes);
    else hipLaunchKernelGGL((k_copy_colwalk<10>), grid, dim3(256), 0, stream(), s, d, (size_t)W, (size_t)W * H, H, nchunks, nstrips, segRows, nseg, nframes);
    if (hipGetLastError() != hipSuccess) return MI355CV_ERROR_UNKNOWN;
    if (!asyncMode()) (void)hipStreamSynchronize(stream());
    return MI355CV_OK;
}

} // extern "C"
