// nlmeans.hip -- cv::fastNlMeansDenoising / fastNlMeansDenoisingColored (photo module, fast_nlmeans_denoising_invoker.hpp with the DistSquared policy; the reference has
// no HAL hook for them) on CV_8U with 1 .. 4 channels, single images and batches.  The rule is the project's restatement (tests/nlmeans_restate.py): a
// weight table built once per call on the host in double precision, everything after it exact integer arithmetic, so the result is determined bit for bit however a
// kernel orders its sums.
//
// Two kernels behind mi355cv_fastNlMeansSetKernel:
//   k_nlm_plain  a lane per pixel, the rule as written: every offset of the search window, every pixel of the patch, reflected indices into HBM, the table in HBM.
//                Serves every admitted parameter set, in bands of rows of at most 2^40 squared differences per launch; the A/B baseline.
//   k_nlm_tile   a workgroup of 2 x 2 waves owns 2 (64 - (T - 1)) x 32 output pixels.  The source with its halo of th + sh goes into LDS once, one plane per channel,
//                the reflected indices applied at load time (no padded copy in HBM), and the non-zero prefix of the table beside it (16-bit words from S = 13 on, up to 160 KiB in all).  For each of the S^2 offsets a
//                wave walks down its 16 + (T - 1) rows: a lane holds the squared differences of its column for the last T rows in registers (compile-time indices:
//                the walk is unrolled) and their running sum, the T columns of a patch are summed across lanes by T - 1 DPP shifts of the wave.  An offset costs a few
//                operations per pixel instead of T^2 cn; a distance whose table index lies past the prefix has weight 0 and skips the accumulation.
// Both take a pixel stride, a first channel and a channel count: the Colored entry denoises L and ab straight out of the Lab image into the output Lab image.
#include "rt.h"
#include "nlmeans_math.h"
#include <atomic>
#include <stdio.h>
#include <algorithm>
#include <vector>

using namespace mi355;

namespace {

constexpr int NORM_L1 = 2, NORM_L2 = 4;                  // cv::NormTypes
static_assert(lim::NLM_TILE_ROWS == 2 * nlm::WAVE_ROWS && lim::NLM_TILE_COLS == 128, "the limits report the tile of nlmeans_math.h");
constexpr size_t TILE_LDS_BYTES = (size_t)lim::NLM_TILE_LDS_KIB << 10;   // what a workgroup of the tile kernel may ask for: the LDS of a CU
constexpr unsigned long long PLAIN_LAUNCH_WORK = 1ull << 40;               // squared differences per launch of the plain kernel, about a second of the chip: a longer call is cut into row bands so that one launch never holds a shared card

// `cn` channels starting at byte ch0 of pixels `pix` bytes apart; frame f at src + f * sframe, dst + f * dframe
struct View { const uchar* src; size_t sstep, sframe; uchar* dst; size_t dstep, dframe; int W, H, pix, ch0; };

template <int CN>
__global__ __launch_bounds__(256) void k_nlm_plain(View v, const int* __restrict__ table, int prefix, int th, int sh, int shift, int y0, int y1)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= v.W || y >= y1) return;
    const uchar* s = v.src + (size_t)blockIdx.z * v.sframe + v.ch0;
    const int W = v.W, H = v.H, pix = v.pix;
    const size_t sstep = v.sstep;
    auto px = [s, W, H, pix, sstep](int yy, int xx, int c) { return (int)s[(size_t)nlm::reflect101(yy, H) * sstep + (size_t)nlm::reflect101(xx, W) * pix + c]; };
    uint32_t wsum = 0, est[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) est[c] = 0;
    for (int dy = -sh; dy <= sh; dy++)
        for (int dx = -sh; dx <= sh; dx++) {
            const unsigned long long idx = nlm::patchDist(px, y, x, dy, dx, th, CN) >> shift;
            if (idx >= (unsigned long long)prefix) continue;
            const uint32_t w = (uint32_t)table[idx];
            wsum += w;
#pragma unroll
            for (int c = 0; c < CN; c++) est[c] += w * (uint32_t)px(y + dy, x + dx, c);
        }
    uchar* d = v.dst + (size_t)blockIdx.z * v.dframe + (size_t)y * v.dstep + (size_t)x * pix + v.ch0;
#pragma unroll
    for (int c = 0; c < CN; c++) d[c] = nlm::finish(est[c], wsum);
}

// lane i takes the value of lane i - 1 (DPP wave_shr:1; what lane 0 gets is never used)
__device__ __forceinline__ uint32_t fromLaneBelow(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }

template <int CN, int TH>
__global__ __launch_bounds__(256) void k_nlm_tile(View v, const int* __restrict__ table, int prefix, int sh, int shift, int wide)
{
    constexpr int T = 2 * TH + 1, WC = 64 - 2 * TH, R = nlm::WAVE_ROWS;
    extern __shared__ uint32_t lds[];
    const nlm::Tile tile = nlm::tileOf(TH, sh);
    const int b = TH + sh, LW = tile.LW, PL = tile.PL;
    // the table's words: 16 bits where mult fits them (S >= 13), 32 otherwise; wave-uniform
    uint32_t* tab32 = lds;
    uint16_t* tab16 = (uint16_t*)lds;
    uchar* plane = (uchar*)lds + nlm::tableBytes(prefix, wide);
    const int X0 = blockIdx.x * (2 * WC), Y0 = blockIdx.y * (2 * R);
    {
        const uchar* s = v.src + (size_t)blockIdx.z * v.sframe + v.ch0;
        if (wide) for (int i = threadIdx.x; i < prefix; i += 256) tab32[i] = (uint32_t)table[i];
        else for (int i = threadIdx.x; i < prefix; i += 256) tab16[i] = (uint16_t)table[i];
        for (int i = threadIdx.x; i < PL; i += 256) {
            const int ly = i / LW, lx = i - ly * LW;
            const uchar* p = s + (size_t)nlm::reflect101(Y0 - b + ly, v.H) * v.sstep + (size_t)nlm::reflect101(X0 - b + lx, v.W) * v.pix;
#pragma unroll
            for (int c = 0; c < CN; c++) plane[c * PL + i] = p[c];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wx = wave & 1, wy = wave >> 1;
    // the lane's column of squared differences is image column X0 + wx WC - TH + lane, its walk starts at image row Y0 + wy R - TH
    const uchar* own = plane + nlm::walkStart(tile, wx, wy, sh, lane);
    const bool valid = lane >= 2 * TH;                   // the sum over lanes lane - 2 TH .. lane is the patch centred on the column of lane - TH
    uint32_t wsum[R], est[R][CN];
#pragma unroll
    for (int j = 0; j < R; j++) {
        wsum[j] = 0;
#pragma unroll
        for (int c = 0; c < CN; c++) est[j][c] = 0;
    }
    for (int dy = -sh; dy <= sh; dy++)
        for (int dx = -sh; dx <= sh; dx++) {
            const uchar* other = own + dy * LW + dx;
            uint32_t ring[T], V = 0;
#pragma unroll
            for (int r = 0; r < R + 2 * TH; r++) {
                uint32_t d2 = 0;
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    const int d = (int)own[c * PL + r * LW] - (int)other[c * PL + r * LW];
                    d2 += (uint32_t)__mul24(d, d);
                }
                V += d2;
                if (r >= T) V -= ring[r % T];
                ring[r % T] = d2;
                if (r >= 2 * TH) {
                    uint32_t D = V, t = V;
#pragma unroll
                    for (int k = 0; k < 2 * TH; k++) { t = fromLaneBelow(t); D += t; }
                    const uint32_t idx = D >> shift;
                    if (valid && idx < (uint32_t)prefix) {
                        const int j = r - 2 * TH;
                        const uint32_t w = wide ? tab32[idx] : (uint32_t)tab16[idx];
                        const uchar* q = other + nlm::centreOf(tile, j, TH);
                        wsum[j] += w;
#pragma unroll
                        for (int c = 0; c < CN; c++) est[j][c] += __umul24(w, (uint32_t)q[c * PL]);
                    }
                }
            }
        }
    const int x = X0 + wx * WC + lane - 2 * TH;
    if (!valid || x >= v.W) return;
    uchar* d = v.dst + (size_t)blockIdx.z * v.dframe + (size_t)x * v.pix + v.ch0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int y = Y0 + wy * R + j;
        if (y < v.H) {
#pragma unroll
            for (int c = 0; c < CN; c++) d[(size_t)y * v.dstep + c] = nlm::finish(est[j][c], wsum[j]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ host side
std::atomic<int> g_kernelMode{-1};      // mi355cv_fastNlMeansSetKernel: -1 the rule, 0 always the plain kernel, 1 the tile kernel wherever it applies
std::atomic<int> g_chunk{0};            // mi355cv_fastNlMeansSetChunk: frames per launch of a device-resident batch, 0 = MAX_GRID_FRAMES

// the refusals of the parameters, none needs a device
int checkParams(int depth, int cn, const float* h, int hn, int tws, int sws, int normType, int width, int height)
{
    MI355_DECLINE_IF(disabled());
    if (depth == MI355CV_16U) return MI355_DECLINED("CV_16U is not served (the reference admits it under NORM_L1 only)");
    MI355_DECLINE_IF(depth != MI355CV_8U);
    MI355_DECLINE_IF(cn < 1 || cn > 4);
    if (normType == NORM_L1) return MI355_DECLINED("NORM_L1 is not served");
    MI355_DECLINE_IF(normType != NORM_L2);
    MI355_DECLINE_IF(!h || hn < 1);
    if (hn != 1) return MI355_DECLINED("a per-channel h vector is not served");
    MI355_DECLINE_IF(tws < 1 || sws < 1);
    if (tws / 2 * 2 + 1 > lim::NLM_MAX_WINDOW) return MI355_DECLINED("templateWindowSize above NLM_MAX_WINDOW = 181: T * T > 2^15");
    if (sws / 2 * 2 + 1 > lim::NLM_MAX_WINDOW) return MI355_DECLINED("searchWindowSize above NLM_MAX_WINDOW = 181 (the bound of the template, far inside the S for which S * S * 255 overflows: the cost of a call grows with S^2)");
    MI355_DECLINE_IF(width < 1 || height < 1);
    if (width > lim::NLM_MAX_DIM || height > lim::NLM_MAX_DIM) return MI355_DECLINED("width or height above NLM_MAX_DIM = 16384");
    return MI355CV_OK;
}

// ... and of the images: pitches, frame strides, src and dst that share bytes (host or device: a lane reads a whole search window of src while others write dst)
int checkImages(const uchar* src, size_t sstep, size_t sframe, const uchar* dst, size_t dstep, size_t dframe, int nframes, int width, int height, int cn, int tws, int sws)
{
    if (nlm::pixelWork(tws, sws, cn) > (unsigned long long)lim::NLM_MAX_PIXEL_WORK)
        return MI355_DECLINED("S^2 T^2 cn above NLM_MAX_PIXEL_WORK = 2^24 squared differences per pixel: one lane of the plain kernel would run for seconds, whatever the image");
    MI355_DECLINE_IF(!src || !dst || nframes < 1);
    const size_t row = (size_t)width * cn;
    MI355_DECLINE_IF(sstep < row || dstep < row);
    if (nframes > 1) MI355_DECLINE_IF(sframe < span(sstep, height, row) || dframe < span(dstep, height, row));
    const size_t shull = (size_t)(nframes - 1) * sframe + span(sstep, height, row), dhull = (size_t)(nframes - 1) * dframe + span(dstep, height, row);
    if (src < dst + dhull && dst < src + shull) return MI355_DECLINED("src and dst overlap");
    return MI355CV_OK;
}

struct Table { nlm::Geom g; std::vector<int> w; };      // the non-zero prefix

Table tableOf(float h, int cn, int tws, int sws)
{
    Table t;
    t.g = nlm::geomOf(tws, sws, cn);
    for (int a = 0; a < t.g.len; a++) {              // one pass: the table is non-increasing, the first zero ends the prefix
        const int w = nlm::weightOf(a, t.g, h, cn);
        if (!w) break;
        t.w.push_back(w);
    }
    return t;
}

size_t tileLds(const nlm::Geom& g, int cn, int prefix)
{
    return (size_t)nlm::tableBytes(prefix, nlm::wideTable(g.mult)) + (size_t)nlm::tileOf(g.th, g.sh).PL * cn;
}
bool tileServes(const nlm::Geom& g, int cn, int prefix)
{
    return g.T <= lim::NLM_TILE_MAX_TEMPLATE && prefix <= lim::NLM_LDS_TABLE && tileLds(g, cn, prefix) <= TILE_LDS_BYTES;
}

template <int CN> void launchTile(const View& v, const int* dtab, int prefix, const nlm::Geom& g, dim3 grid, size_t ldsBytes, hipStream_t st)
{
    // more than 64 KiB of dynamic LDS has to be asked for per kernel; a refusal shows as the launch's error
#define NLM_TILE(TH_) do { if (ldsBytes > (64u << 10)) (void)hipFuncSetAttribute((const void*)k_nlm_tile<CN, TH_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TILE_LDS_BYTES); \
                           hipLaunchKernelGGL((k_nlm_tile<CN, TH_>), grid, dim3(256), ldsBytes, st, v, dtab, prefix, g.sh, g.shift, nlm::wideTable(g.mult) ? 1 : 0); } while (0)
    switch (g.th) {
    case 0: NLM_TILE(0); break;
    case 1: NLM_TILE(1); break;
    case 2: NLM_TILE(2); break;
    case 3: NLM_TILE(3); break;
    default: NLM_TILE(4); break;
    }
#undef NLM_TILE
}

int plainBand(const nlm::Geom& g, int cn, int W, int nf) { return nlm::plainBand(g.T, g.S, cn, W, nf, PLAIN_LAUNCH_WORK); }

// Denoises `cn` channels of device-resident frames.  -> true when the tile kernel served
bool launchPlanes(const View& v, int nframes, int cn, const Table& t, const int* dtab, hipStream_t st, int* launches)
{
    const int prefix = (int)t.w.size(), mode = g_kernelMode.load(std::memory_order_relaxed);
    const bool fast = mode != 0 && tileServes(t.g, cn, prefix);
    int chunk = g_chunk.load(std::memory_order_relaxed);
    if (chunk < 1 || chunk > MAX_GRID_FRAMES) chunk = MAX_GRID_FRAMES;
    const size_t ldsBytes = fast ? tileLds(t.g, cn, prefix) : 0;
    *launches = 0;
    for (int f0 = 0; f0 < nframes; f0 += chunk, ++*launches) {
        const int nf = std::min(chunk, nframes - f0);
        View c = v;
        c.src += (size_t)f0 * v.sframe; c.dst += (size_t)f0 * v.dframe;
        if (fast) {
            const dim3 grid(divUp(v.W, 2 * (64 - 2 * t.g.th)), divUp(v.H, lim::NLM_TILE_ROWS), nf);
            if (cn == 1) launchTile<1>(c, dtab, prefix, t.g, grid, ldsBytes, st);
            else if (cn == 2) launchTile<2>(c, dtab, prefix, t.g, grid, ldsBytes, st);
            else if (cn == 3) launchTile<3>(c, dtab, prefix, t.g, grid, ldsBytes, st);
            else launchTile<4>(c, dtab, prefix, t.g, grid, ldsBytes, st);
        } else {
            const int band = plainBand(t.g, cn, v.W, nf);
            for (int y0 = 0; y0 < v.H; y0 += band) {
                const int y1 = std::min(v.H, y0 + band);
                const dim3 grid(divUp(v.W, 64), divUp(y1 - y0, 4), nf);
#define NLM_PLAIN(CN_) hipLaunchKernelGGL(k_nlm_plain<CN_>, grid, dim3(256), 0, st, c, dtab, prefix, t.g.th, t.g.sh, t.g.shift, y0, y1)
                if (cn == 1) NLM_PLAIN(1); else if (cn == 2) NLM_PLAIN(2); else if (cn == 3) NLM_PLAIN(3); else NLM_PLAIN(4);
#undef NLM_PLAIN
            }
        }
    }
    return fast;
}

void note(bool fast, const Table& t, int cn, int W, int H, int nframes, int launches, const char* tail)
{
    if (fast)
        noteKernel("k_nlm_tile<%d,%d> T=%d S=%d prefix=%zu grid=%dx%d x256 lds=%zu, %d launch(es) of <= %d frames%s", cn, t.g.th, t.g.T, t.g.S, t.w.size(),
                   divUp(W, 2 * (64 - 2 * t.g.th)), divUp(H, lim::NLM_TILE_ROWS), tileLds(t.g, cn, (int)t.w.size()), launches, divUp(nframes, launches), tail);
    else
        noteKernel("k_nlm_plain<%d> T=%d S=%d prefix=%zu grid=%dx%d x256 band=%d, %d launch(es) of <= %d frames%s", cn, t.g.T, t.g.S, t.w.size(), divUp(W, 64),
                   divUp(H, 4), plainBand(t.g, cn, W, std::min(nframes, divUp(nframes, launches))), launches, divUp(nframes, launches), tail);
}

int runNlm(const char* entry, const uchar* src, size_t sstep, size_t sframe, uchar* dst, size_t dstep, size_t dframe, int nframes, int width, int height, int depth, int cn,
           const float* h, int hn, int tws, int sws, int normType)
{
    if (const int rc = checkParams(depth, cn, h, hn, tws, sws, normType, width, height)) return rc;
    if (const int rc = checkImages(src, sstep, sframe, dst, dstep, dframe, nframes, width, height, cn, tws, sws)) return rc;
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)width * height, minPixels(HOST_HEAVY)));
    View v{src, sstep, nframes == 1 ? 0 : sframe, dst, dstep, nframes == 1 ? 0 : dframe, width, height, cn, 0};
    if (nframes == 1) {
        v.src = stg.in(src, sstep, (size_t)width * cn, height, &v.sstep);
        v.dst = stg.out(dst, dstep, (size_t)width * cn, height, &v.dstep);
        MI355_DECLINE_IF(!v.src || !v.dst);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(dst));
    const Table t = tableOf(h[0], cn, tws, sws);
    const int* dtab = (const int*)stg.param(t.w.data(), t.w.size() * sizeof(int));
    if (!dtab) return MI355_DECLINED("no scratch for the weight table");
    int launches = 0;
    const bool fast = launchPlanes(v, nframes, cn, t, dtab, stream(), &launches);
    MI355_CHECK_LAUNCH(entry);
    note(fast, t, cn, width, height, nframes, launches, "");
    return stg.finish(entry);
}

int runColored(const char* entry, const uchar* src, size_t sstep, size_t sframe, uchar* dst, size_t dstep, size_t dframe, int nframes, int width, int height, int depth, int cn,
               float h, float hColor, int tws, int sws)
{
    if (cn == 4) return MI355_DECLINED("CV_8UC4 is not served by the Colored entries");
    MI355_DECLINE_IF(cn != 3);
    const float hs[1] = {h};
    if (const int rc = checkParams(depth, cn, hs, 1, tws, sws, NORM_L2, width, height)) return rc;
    if (const int rc = checkImages(src, sstep, sframe, dst, dstep, dframe, nframes, width, height, cn, tws, sws)) return rc;
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)width * height, minPixels(HOST_HEAVY)));
    const size_t row = (size_t)width * 3;
    const uchar* ds = src; uchar* dd = dst;
    size_t dss = sstep, dds = dstep;
    if (nframes == 1) {
        ds = stg.in(src, sstep, row, height, &dss);
        dd = stg.out(dst, dstep, row, height, &dds);
        MI355_DECLINE_IF(!ds || !dd);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(dst));
    // frames go through two Lab images of scratch in groups: LBGR2Lab per frame, one launch per group for L and one for ab, Lab2LBGR per frame
    int chunk = g_chunk.load(std::memory_order_relaxed);
    if (chunk < 1 || chunk > 16) chunk = 16;
    chunk = std::min(chunk, nframes);
    const size_t lstep = pad256(row), lframe = lstep * height;
    uchar* labIn = (uchar*)stg.scratch(lframe * chunk);
    uchar* labOut = (uchar*)stg.scratch(lframe * chunk);
    if (!labIn || !labOut) return MI355_DECLINED("no scratch for the Lab images");
    const Table tl = tableOf(h, 1, tws, sws), tc = tableOf(hColor, 2, tws, sws);
    const int* dtl = (const int*)stg.param(tl.w.data(), tl.w.size() * sizeof(int));
    const int* dtc = (const int*)stg.param(tc.w.data(), tc.w.size() * sizeof(int));
    if (!dtl || !dtc) return MI355_DECLINED("no scratch for the weight tables");
    hipStream_t st = stream();
    bool fastL = false, fastC = false;
    int launches = 0, groups = 0;
    for (int f0 = 0; f0 < nframes; f0 += chunk, groups++) {
        const int nf = std::min(chunk, nframes - f0);
        for (int f = 0; f < nf; f++)         // nested entries: same stream, same scratch pool, no synchronisation of their own
            if (const int rc = mi355cv_cvtBGRtoLab(ds + (size_t)(f0 + f) * sframe, dss, labIn + f * lframe, lstep, width, height, MI355CV_8U, 3, false, true, false)) return rc;
        fastL = launchPlanes(View{labIn, lstep, lframe, labOut, lstep, lframe, width, height, 3, 0}, nf, 1, tl, dtl, st, &launches);
        fastC = launchPlanes(View{labIn, lstep, lframe, labOut, lstep, lframe, width, height, 3, 1}, nf, 2, tc, dtc, st, &launches);
        MI355_CHECK_LAUNCH(entry);
        for (int f = 0; f < nf; f++)
            if (const int rc = mi355cv_cvtLabtoBGR(labOut + f * lframe, lstep, dd + (size_t)(f0 + f) * dframe, dds, width, height, MI355CV_8U, 3, false, true, false)) return rc;
    }
    // after the nested conversions, which name their own kernels
    char tail[96];
    snprintf(tail, sizeof tail, "; L by %s, ab by %s, in groups of %d", fastL ? "k_nlm_tile" : "k_nlm_plain", fastC ? "k_nlm_tile" : "k_nlm_plain", chunk);
    note(fastC, tc, 2, width, height, nframes, groups, tail);
    return stg.finish(entry);
}

} // namespace

extern "C" {

// Host-resident images are staged (HOST_HEAVY): the reference spends S^2 T^2 operations per pixel on host threads against 2 bytes per pixel and channel over PCIe.
MI355CV_API int mi355cv_fastNlMeansDenoising(const uchar* src, size_t src_step, uchar* dst, size_t dst_step, int width, int height, int depth, int cn, const float* h, int hn,
                                             int templateWindowSize, int searchWindowSize, int normType)
{
    mi355::EntryGuard entry_(__func__);
    return runNlm("fastNlMeansDenoising", src, src_step, 0, dst, dst_step, 0, 1, width, height, depth, cn, h, hn, templateWindowSize, searchWindowSize, normType);
}

MI355CV_API int mi355cv_fastNlMeansDenoisingBatch(const uchar* src, size_t src_step, size_t src_frame_stride, uchar* dst, size_t dst_step, size_t dst_frame_stride, int nframes,
                                                  int width, int height, int depth, int cn, const float* h, int hn, int templateWindowSize, int searchWindowSize, int normType)
{
    mi355::EntryGuard entry_(__func__);
    if (const int rc = checkParams(depth, cn, h, hn, templateWindowSize, searchWindowSize, normType, width, height)) return rc;
    if (const int rc = checkImages(src, src_step, src_frame_stride, dst, dst_step, dst_frame_stride, nframes, width, height, cn, templateWindowSize, searchWindowSize)) return rc;
    if (hostBatchEligible(src, dst, nframes)) {        // frames in host memory
        const HostBatch hb = {src, src_step, src_frame_stride, (size_t)width * cn, height, dst, dst_step, dst_frame_stride, (size_t)width * cn, height, nframes};
        return runHostBatch("fastNlMeansDenoisingBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_fastNlMeansDenoisingBatch(s, ss, sf, d, ds, df, nf, width, height, depth, cn, h, hn, templateWindowSize, searchWindowSize, normType); });
    }
    return runNlm("fastNlMeansDenoisingBatch", src, src_step, src_frame_stride, dst, dst_step, dst_frame_stride, nframes, width, height, depth, cn, h, hn, templateWindowSize,
                  searchWindowSize, normType);
}

MI355CV_API int mi355cv_fastNlMeansDenoisingColored(const uchar* src, size_t src_step, uchar* dst, size_t dst_step, int width, int height, int depth, int cn, float h, float hColor,
                                                    int templateWindowSize, int searchWindowSize)
{
    mi355::EntryGuard entry_(__func__);
    return runColored("fastNlMeansDenoisingColored", src, src_step, 0, dst, dst_step, 0, 1, width, height, depth, cn, h, hColor, templateWindowSize, searchWindowSize);
}

MI355CV_API int mi355cv_fastNlMeansDenoisingColoredBatch(const uchar* src, size_t src_step, size_t src_frame_stride, uchar* dst, size_t dst_step, size_t dst_frame_stride,
                                                         int nframes, int width, int height, int depth, int cn, float h, float hColor, int templateWindowSize, int searchWindowSize)
{
    mi355::EntryGuard entry_(__func__);
    if (cn == 4) return MI355_DECLINED("CV_8UC4 is not served by the Colored entries");
    MI355_DECLINE_IF(cn != 3);
    const float hs[1] = {h};
    if (const int rc = checkParams(depth, cn, hs, 1, templateWindowSize, searchWindowSize, NORM_L2, width, height)) return rc;
    if (const int rc = checkImages(src, src_step, src_frame_stride, dst, dst_step, dst_frame_stride, nframes, width, height, cn, templateWindowSize, searchWindowSize)) return rc;
    if (hostBatchEligible(src, dst, nframes)) {        // frames in host memory
        const HostBatch hb = {src, src_step, src_frame_stride, (size_t)width * cn, height, dst, dst_step, dst_frame_stride, (size_t)width * cn, height, nframes};
        return runHostBatch("fastNlMeansDenoisingColoredBatch", hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            return mi355cv_fastNlMeansDenoisingColoredBatch(s, ss, sf, d, ds, df, nf, width, height, depth, cn, h, hColor, templateWindowSize, searchWindowSize); });
    }
    return runColored("fastNlMeansDenoisingColoredBatch", src, src_step, src_frame_stride, dst, dst_step, dst_frame_stride, nframes, width, height, depth, cn, h, hColor,
                      templateWindowSize, searchWindowSize);
}

// Host only, touches no device: the weight table of (h, cn, templateWindowSize, searchWindowSize).  info[0 .. 3] = len, shift, mult, the length of the non-zero prefix;
// table (may be NULL) gets min(len, capacity) entries.
MI355CV_API int mi355cv_fastNlMeansWeights(float h, int cn, int templateWindowSize, int searchWindowSize, int* table, int capacity, int* info)
{
    mi355::EntryGuard entry_(__func__);
    const float hs[1] = {h};
    if (const int rc = checkParams(MI355CV_8U, cn, hs, 1, templateWindowSize, searchWindowSize, NORM_L2, 1, 1)) return rc;
    MI355_DECLINE_IF(!info || capacity < 0);
    const nlm::Geom g = nlm::geomOf(templateWindowSize, searchWindowSize, cn);
    info[0] = g.len; info[1] = g.shift; info[2] = g.mult;
    info[3] = nlm::buildTable(g, h, cn, table, table ? capacity : 0);
    return MI355CV_OK;
}

MI355CV_API int mi355cv_fastNlMeansSetKernel(int mode)
{
    if (mode < -1 || mode > 1) return MI355CV_ERROR_UNKNOWN;
    g_kernelMode.store(mode, std::memory_order_relaxed);
    return MI355CV_OK;
}

MI355CV_API int mi355cv_fastNlMeansSetChunk(int frames)
{
    if (frames < 0) return MI355CV_ERROR_UNKNOWN;
    g_chunk.store(frames, std::memory_order_relaxed);
    return MI355CV_OK;
}

} // extern "C"
