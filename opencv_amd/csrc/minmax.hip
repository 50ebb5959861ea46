// minmax.hip -- cv::minMaxLoc on one channel of CV_8U .. CV_64F with an optional CV_8UC1 mask, single frames and batches (mi355cv_minMaxLoc, ...Batch).  Every line
// of arithmetic that can be wrong -- the order-preserving key of each depth, NaN, -0, the decode and the order on (key, index) pairs -- is in minmax_math.h, which
// the CPU suite compiles for the host.  The reference was not available to pin the treatment of NaN (never a candidate), of +-inf (ordinary values) and of the empty
// candidate set (0, 0, (-1, -1), (-1, -1)); they are this project's restatement, tests/minmax_restate.py, and the kernels are held against it bit for bit.
//
//   k_minmax_partial<depth, masked>   grid (P, frames).  A row is cut into the 16-byte-aligned chunks of its own address range ("item" t = row * nch + chunk), so
//                    that a source whose base or pitch is aligned to the element only is still read with 16-byte loads: a chunk that lies wholly inside the row
//                    is one dwordx4 load, the first and last chunk of a row (the scalar head and tail) are read element by element, and nothing outside
//                    [row, row + width) is ever touched.  A lane walks items t, t + T, t + 2 T ... in ascending raster order.  Per chunk it reduces the VALUES only
//                    (min of the keys, max of the keys) and compares the chunk's pair against its running best with a strict "less", which keeps the first chunk;
//                    the index of the winning pixel is found once per lane at the end, by loading its winning chunk again (16 bytes, usually still in L2).  The
//                    alternative, an index carried per element, costs a compare and two selects more per pixel and would weigh most on CV_8U, 16 pixels per load (not timed).
//                    Then (key, index) pairs are combined with minmax::combine across the wave (__shfl_xor), the four waves (LDS) and written as the workgroup's
//                    partial.  The unmasked variant takes no mask pointer into account at all.
//   k_minmax_final<depth>   grid (frames): combines a frame's P partials in the same order and writes vals[2 f ..] and locs[4 f ..] (minmax::emit).
// No atomics: the partials go through HBM and a second launch, so CV_64F -- 64 key bits and 28 index bits, more than a 64-bit atomic holds -- uses the same code
// as the other depths with a wider compare, and there is nothing to zero before a call.  Every combine step is min over the total order of minmax_math.h, so the
// result does not depend on P, on the grid, or on scheduling.  Two launches whatever the number of frames.
#include "rt.h"
#include "minmax_math.h"
#include <algorithm>

using namespace mi355;

namespace {

using minmax::Best;
using minmax::Depth;
using minmax::NONE;

__device__ __forceinline__ uint32_t shx(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
__device__ __forceinline__ uint64_t shx(uint64_t v, int m) { return ((uint64_t)shx((uint32_t)(v >> 32), m) << 32) | shx((uint32_t)v, m); }

template <class K> __device__ __forceinline__ Best<K> waveBest(Best<K> b)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) {
        Best<K> o;
        o.key = shx(b.key, m); o.idx = shx(b.idx, m);
        b = minmax::combine(b, o);
    }
    return b;
}

// the workgroup's least pair, valid in thread 0; sk / si: one slot per wave
template <class K> __device__ __forceinline__ Best<K> groupBest(Best<K> b, K* sk, uint32_t* si)
{
    b = waveBest(b);
    if ((threadIdx.x & 63) == 0) { sk[threadIdx.x >> 6] = b.key; si[threadIdx.x >> 6] = b.idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < 4; i++) { Best<K> o; o.key = sk[i]; o.idx = si[i]; b = minmax::combine(b, o); }
    return b;
}

// Chunk j of the row at rp (mask row mp): the 16 bytes at (rp & ~15) + 16 j, cut to the row.  f(v, live, x0): v the N = 16 / sizeof(U) elements of the chunk,
// bit k of `live` set iff element k is a candidate (inside the row, selected by the mask, not NaN), x0 the column of element 0 (negative in a row's head chunk).
template <int D, bool MASKED, class F>
__device__ __forceinline__ void visitChunk(const uchar* rp, const uchar* mp, int w, uint32_t j, F f)
{
    typedef typename Depth<D>::U U;
    constexpr int N = 16 / (int)sizeof(U);
    const int b0 = 16 * (int)j - (int)((uintptr_t)rp & 15), rowBytes = w * (int)sizeof(U);
    const int x0 = b0 / (int)sizeof(U);                                      // exact: the row is aligned to its element
    U v[N];
    if (b0 >= 0 && b0 + 16 <= rowBytes) {
        const uint4 q = *reinterpret_cast<const uint4*>(rp + b0);
        __builtin_memcpy(v, &q, 16);
        uint32_t live = (1u << N) - 1;
        if (MASKED) {
            uint8_t m[N];
            __builtin_memcpy(m, mp + x0, N);
            live = 0;
#pragma unroll
            for (int k = 0; k < N; k++) live |= (uint32_t)(m[k] != 0) << k;
        }
#pragma unroll
        for (int k = 0; k < N; k++) if (!Depth<D>::valid(v[k])) live &= ~(1u << k);
        f(v, live, x0);
    } else {                                                                 // a row's head or tail, or a chunk past its end
        uint32_t live = 0;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int x = x0 + k;
            const bool in = x >= 0 && x < w;
            U e = 0;
            if (in) e = reinterpret_cast<const U*>(rp)[x];
            bool c = in && Depth<D>::valid(e);
            if (MASKED && c) c = mp[x] != 0;
            v[k] = e;
            live |= (uint32_t)c << k;
        }
        if (live) f(v, live, x0);
    }
}

// pk / pi: the partials, [(2 frame + s) * P + workgroup], s = 0 the minimum, 1 the maximum (complemented key)
template <int D, bool MASKED>
__global__ __launch_bounds__(256) void k_minmax_partial(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h, const uchar* __restrict__ mask,
                                                        size_t mstep, size_t mframe, uint32_t nch, typename Depth<D>::K* __restrict__ pk, uint32_t* __restrict__ pi)
{
    typedef typename Depth<D>::U U;
    typedef typename Depth<D>::K K;
    constexpr int N = 16 / (int)sizeof(U);
    __shared__ K sk[2][4];
    __shared__ uint32_t si[2][4];
    const uchar* S = src + (size_t)blockIdx.y * sframe;
    const uchar* M = MASKED ? mask + (size_t)blockIdx.y * mframe : nullptr;
    const uint32_t T = gridDim.x * 256u, items = (uint32_t)h * nch;          // items <= 16384 * 8194
    uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t row = t / nch, j = t - row * nch;
    const uint32_t dr = T / nch, dj = T - dr * nch;
    K mn = (K)~(K)0, mx = (K)~(K)0;                                          // mx: complemented
    uint32_t mnAt = NONE, mxAt = NONE;                                       // the item that holds the winner
    for (; t < items; t += T) {
        visitChunk<D, MASKED>(S + (size_t)row * sstep, MASKED ? M + (size_t)row * mstep : nullptr, w, j, [&](const U* v, uint32_t live, int) {
            K lo = (K)~(K)0, hi = 0;
#pragma unroll
            for (int k = 0; k < N; k++) {
                const K key = Depth<D>::key(v[k]);
                const bool c = (live >> k) & 1u;
                lo = minmax::least(lo, c ? key : (K)~(K)0);
                hi = minmax::greatest(hi, c ? key : (K)0);
            }
            if (live) {                                                      // (lo, t) before (mn, mnAt): t only grows, so an equal key loses unless nothing was found yet
                const K chi = (K)~hi;
                if (lo < mn || mnAt == NONE) { mn = lo; mnAt = t; }
                if (chi < mx || mxAt == NONE) { mx = chi; mxAt = t; }
            }
        });
        row += dr; j += dj;
        if (j >= nch) { j -= nch; row++; }
    }
    // the first candidate of the winning chunk that holds the winning key
    Best<K> bmn = minmax::identity<K>(), bmx = minmax::identity<K>();
    if (mnAt != NONE) {
        const uint32_t r = mnAt / nch;
        uint32_t at = NONE;
        visitChunk<D, MASKED>(S + (size_t)r * sstep, MASKED ? M + (size_t)r * mstep : nullptr, w, mnAt - r * nch, [&](const U* v, uint32_t live, int x0) {
#pragma unroll
            for (int k = N - 1; k >= 0; k--) if (((live >> k) & 1u) && Depth<D>::key(v[k]) == mn) at = r * (uint32_t)w + (uint32_t)(x0 + k);
        });
        bmn.key = mn; bmn.idx = at;
    }
    if (mxAt != NONE) {
        const uint32_t r = mxAt / nch;
        uint32_t at = NONE;
        visitChunk<D, MASKED>(S + (size_t)r * sstep, MASKED ? M + (size_t)r * mstep : nullptr, w, mxAt - r * nch, [&](const U* v, uint32_t live, int x0) {
#pragma unroll
            for (int k = N - 1; k >= 0; k--) if (((live >> k) & 1u) && (K)~Depth<D>::key(v[k]) == mx) at = r * (uint32_t)w + (uint32_t)(x0 + k);
        });
        bmx.key = mx; bmx.idx = at;
    }
    bmn = groupBest(bmn, sk[0], si[0]);
    bmx = groupBest(bmx, sk[1], si[1]);
    if (threadIdx.x == 0) {
        const size_t o = (size_t)2 * blockIdx.y * gridDim.x + blockIdx.x;
        pk[o] = bmn.key; pi[o] = bmn.idx;
        pk[o + gridDim.x] = bmx.key; pi[o + gridDim.x] = bmx.idx;
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_minmax_final(const typename Depth<D>::K* __restrict__ pk, const uint32_t* __restrict__ pi, int P, int w,
                                                      double* __restrict__ vals, int* __restrict__ locs)
{
    typedef typename Depth<D>::K K;
    __shared__ K sk[2][4];
    __shared__ uint32_t si[2][4];
    const size_t o = (size_t)2 * blockIdx.x * P;
    Best<K> bmn = minmax::identity<K>(), bmx = minmax::identity<K>();
    for (int p = threadIdx.x; p < P; p += 256) {
        Best<K> a, b;
        a.key = pk[o + p]; a.idx = pi[o + p];
        b.key = pk[o + P + p]; b.idx = pi[o + P + p];
        bmn = minmax::combine(bmn, a);
        bmx = minmax::combine(bmx, b);
    }
    bmn = groupBest(bmn, sk[0], si[0]);
    bmx = groupBest(bmx, sk[1], si[1]);
    if (threadIdx.x == 0) minmax::emit<D>(bmn, bmx, w, vals + 2 * (size_t)blockIdx.x, locs + 4 * (size_t)blockIdx.x);
}

// ---- host side
const char* const DEPTH_NAME[7] = {"8u", "8s", "16u", "16s", "32s", "32f", "64f"};

struct Launch {
    const uchar* src; size_t sstep, sframe; int w, h;
    const uchar* mask; size_t mstep, mframe;
    uint32_t nch; int P, nf;
    void* pk; uint32_t* pi; double* vals; int* locs;
};

template <int D> void launchDepth(const Launch& a, hipStream_t st)
{
    typedef typename Depth<D>::K K;
    const dim3 grid(a.P, a.nf);
    if (a.mask) hipLaunchKernelGGL((k_minmax_partial<D, true>), grid, dim3(256), 0, st, a.src, a.sstep, a.sframe, a.w, a.h, a.mask, a.mstep, a.mframe, a.nch, (K*)a.pk, a.pi);
    else hipLaunchKernelGGL((k_minmax_partial<D, false>), grid, dim3(256), 0, st, a.src, a.sstep, a.sframe, a.w, a.h, (const uchar*)nullptr, (size_t)0, (size_t)0, a.nch, (K*)a.pk, a.pi);
    hipLaunchKernelGGL((k_minmax_final<D>), dim3(a.nf), dim3(256), 0, st, (const K*)a.pk, (const uint32_t*)a.pi, a.P, a.w, a.vals, a.locs);
}

void launch(int depth, const Launch& a, hipStream_t st)
{
    switch (depth) {
    case 0: launchDepth<0>(a, st); break;
    case 1: launchDepth<1>(a, st); break;
    case 2: launchDepth<2>(a, st); break;
    case 3: launchDepth<3>(a, st); break;
    case 4: launchDepth<4>(a, st); break;
    case 5: launchDepth<5>(a, st); break;
    default: launchDepth<6>(a, st); break;
    }
}

// host-resident frames into dense device rows of pitch dstep
bool upload(const uchar* p, size_t step, size_t frame, size_t rowBytes, int h, int nf, uchar* dev, size_t dstep, hipStream_t st)
{
    for (int f = 0; f < nf; f++)
        if (hipMemcpy2DAsync(dev + (size_t)f * dstep * h, dstep, p + (size_t)f * frame, step, rowBytes, h, hipMemcpyHostToDevice, st) != hipSuccess) return false;
    noteStagedBytes((long long)rowBytes * h * nf);
    return true;
}

int runMinMax(const char* entry, const uchar* src, size_t sstep, size_t sframe, int w, int h, int depth, const uchar* mask, size_t mstep, size_t mframe, int nframes,
              double* vals, int* locs)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!src || !vals || !locs);
    if (depth < 0 || depth > 6) return MI355_DECLINED("depth is not CV_8U .. CV_64F");
    MI355_DECLINE_IF(w <= 0 || h <= 0 || w > lim::MINMAX_MAX_DIM || h > lim::MINMAX_MAX_DIM);
    if (nframes < 1 || nframes > minmax::MAX_FRAMES) return MI355_DECLINED("nframes < 1 || nframes > 65535");
    const size_t esz = (size_t)depthBytes(depth), rowBytes = (size_t)w * esz;
    if (sstep < rowBytes || (mask && mstep < (size_t)w)) return MI355_DECLINED("src_step or mask_step is smaller than a row");
    if (sstep % esz || sframe % esz || (uintptr_t)src % esz) return MI355_DECLINED("src, src_step or src_frame_stride is no multiple of the element size");
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    const int skind = ptrKind(src), mkind = mask ? ptrKind(mask) : skind, vkind = ptrKind(vals), lkind = ptrKind(locs);
    if (skind == PTR_FOREIGN || mkind == PTR_FOREIGN || vkind == PTR_FOREIGN || lkind == PTR_FOREIGN)
        return MI355_DECLINED("an argument lives on another device");
    if (skind != mkind) return MI355_DECLINED("src and mask must both live on this thread's device or both on the host");
    if (vkind != lkind) return MI355_DECLINED("vals and locs must both live on this thread's device or both on the host");
    const bool shost = skind == PTR_HOST, rhost = vkind == PTR_HOST;
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_CHEAP)));
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + rowBytes, mspan = (size_t)(nframes - 1) * mframe + (size_t)(h - 1) * mstep + w;
    const size_t vspan = (size_t)nframes * 2 * sizeof(double), lspan = (size_t)nframes * 4 * sizeof(int);
    if (overlapOnDevice(src, sspan, vals, vspan) || overlapOnDevice(src, sspan, locs, lspan) || (mask && (overlapOnDevice(mask, mspan, vals, vspan) || overlapOnDevice(mask, mspan, locs, lspan))))
        return MI355_DECLINED("the results overlap the source or the mask in HBM");
    if (!rhost && overlapOnDevice(vals, vspan, locs, lspan)) return MI355_DECLINED("vals and locs overlap");

    Launch a;
    a.w = w; a.h = h;
    a.nch = (uint32_t)((rowBytes + 15) / 16 + 1);                            // the most 16-byte lines a row can touch
    const size_t items = (size_t)h * a.nch;
    a.P = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((items + 1023) / 1024, (size_t)(8192 + nframes - 1) / nframes), 1024));
    const size_t ksz = depth == 6 ? 8 : 4, slots = (size_t)2 * a.P * nframes;
    uchar* part = (uchar*)stg.scratch(pad256(slots * ksz) + slots * 4);
    double* dvals = rhost ? (double*)stg.scratch(vspan + lspan) : vals;
    char* landing = rhost ? (char*)stg.pinned(vspan + lspan) : nullptr;
    if (!part || !dvals || (rhost && !landing)) return MI355_DECLINED("no scratch");
    int* dlocs = rhost ? (int*)(dvals + 2 * (size_t)nframes) : locs;
    a.pk = part; a.pi = (uint32_t*)(part + pad256(slots * ksz));
    // host-resident frames: dense copies of a group of at most 1 GiB of them; a mask shared by all frames goes up once
    const bool sharedMask = mask && (nframes == 1 || mframe == 0);
    const size_t hstep = pad256(rowBytes), hmstep = pad256((size_t)w);
    const size_t perFrame = hstep * h + (mask && !sharedMask ? hmstep * h : 0);
    const int group = shost ? (int)std::min<size_t>((size_t)nframes, std::max<size_t>(1, (size_t(1) << 30) / perFrame)) : nframes;
    uchar* hsrc = shost ? (uchar*)stg.scratch(hstep * h * group) : nullptr;
    uchar* hmask = shost && mask ? (uchar*)stg.scratch(hmstep * h * (sharedMask ? 1 : group)) : nullptr;
    if (shost && (!hsrc || (mask && !hmask))) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    if (shost && sharedMask && !upload(mask, mstep, 0, (size_t)w, h, 1, hmask, hmstep, st))
        return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
    for (int f0 = 0; f0 < nframes; f0 += group) {
        a.nf = std::min(group, nframes - f0);
        a.src = src + (size_t)f0 * sframe; a.sstep = sstep; a.sframe = sframe;
        a.mask = mask ? mask + (size_t)f0 * mframe : nullptr; a.mstep = mstep; a.mframe = sharedMask ? 0 : mframe;
        if (shost) {
            if (!upload(a.src, sstep, sframe, rowBytes, h, a.nf, hsrc, hstep, st) || (mask && !sharedMask && !upload(a.mask, mstep, mframe, (size_t)w, h, a.nf, hmask, hmstep, st)))
                return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
            a.src = hsrc; a.sstep = hstep; a.sframe = hstep * h;
            if (mask) { a.mask = hmask; a.mstep = hmstep; a.mframe = sharedMask ? 0 : hmstep * h; }
        }
        a.vals = dvals + 2 * (size_t)f0; a.locs = dlocs + 4 * (size_t)f0;
        launch(depth, a, st);                                                // the partials of a group are consumed by its own final launch, in stream order
    }
    MI355_CHECK_LAUNCH(entry);
    if (rhost) {                                                             // the call's one read-back
        if (hipMemcpyAsync(landing, dvals, vspan + lspan, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
        memcpy(vals, landing, vspan);
        memcpy(locs, landing + vspan, lspan);
        noteStagedBytes((long long)(vspan + lspan));
    }
    noteKernel("k_minmax_partial<%s,%s> grid=%dx%d x256 nch=%u + k_minmax_final grid=%d x256, %d frame(s)", DEPTH_NAME[depth], mask ? "mask" : "nomask", a.P,
               std::min(group, nframes), a.nch, std::min(group, nframes), nframes);
    return stg.finish(entry);
}

} // namespace

static_assert(lim::MINMAX_MAX_DIM == minmax::MAX_DIM, "one bound");
static_assert((long long)minmax::MAX_DIM * minmax::MAX_DIM <= (1ll << 28), "a raster index below 2^28, far from NONE");
static_assert((long long)minmax::MAX_DIM * (minmax::MAX_DIM * 8 / 16 + 2) + 1024 * 256 < (1ll << 32), "k_minmax_partial counts items in 32 bits");

extern "C" {

MI355CV_API int mi355cv_minMaxLoc(const uchar* src_data, size_t src_step, int width, int height, int depth, const uchar* mask_data, size_t mask_step, double* vals,
                                  int* locs)
{
    mi355::EntryGuard entry_(__func__);
    return runMinMax("minMaxLoc", src_data, src_step, 0, width, height, depth, mask_data, mask_step, 0, 1, vals, locs);
}

MI355CV_API int mi355cv_minMaxLocBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, int depth, const uchar* mask_data,
                                       size_t mask_step, size_t mask_frame_stride, int nframes, double* vals, int* locs)
{
    mi355::EntryGuard entry_(__func__);
    return runMinMax("minMaxLocBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, width, height, depth, mask_data, mask_step,
                     nframes == 1 ? 0 : mask_frame_stride, nframes, vals, locs);
}

} // extern "C"
