// hough.hip -- cv::HoughLines / cv::HoughLinesWithAccumulator, the standard transform (HoughLinesStandard, imgproc/src/hough.cpp; the reference has no HAL hook for
// it) on CV_8UC1.  Every line of arithmetic is in hough_math.h.  The accumulator is integer, so every result is a pure function of the input whatever order the
// votes land in, and lines are ordered by (votes descending, accumulator index ascending), so the line list is one too.  The reference was not available to pin
// the semantics; they are restated in tests/hough_restate.py (plain loops and an independent vectorised form) and the kernels are held against that bit for bit.
//
//   k_hough_points   a wave per 256 columns of a row: a lane loads one dword (4 pixels), four 64-bit ballots count the non-zero ones, lane 0 adds the count to
//                    the frame's counter (one atomic per wave) and every lane appends its packed points (y << 16 | x) behind the lanes below it.  The order
//                    of the list depends on the order of those atomics; only integer counts follow from it.
//   k_hough_vote     a workgroup owns one angle and every VOTE_SPLIT-th chunk of VOTE_CHUNK points.  It keeps the numrho + 2 bins of its accumulator row in
//                    LDS (12003 ints = 48 KB at 4K with rho = 1), votes with LDS atomic adds and adds its non-zero bins to the accumulator in HBM with integer
//                    atomicAdd.  A row of more than LDS_BINS = 16384 bins (64 KiB) votes straight into HBM with the same arithmetic (k_hough_vote<false>); a
//                    vote that leaves its row (the reference does not clamp) goes to its flat cell in HBM, or nowhere when that is outside the accumulator.
//   k_hough_maxima   a thread per cell: the five-way predicate; a wave appends its candidates behind one atomic add on the frame's counter.
//   sort             rocPRIM's radix sort (gftt_sort.hip) over the whole candidate buffer of a frame, descending on the COMPLEMENT of the key, the unused tail
//                    being zeros: the number of candidates stays on the device, so the call has one host synchronisation, the read-back of the counts.
//   k_hough_emit     line i < min(count, max_lines) from sorted key i; rows past the count are never written.
// Limits (mi355cv_limit): "hough_max_dim" = 16384 -- a packed point needs both coordinates <= 65535; 16384 is the bound of the neighbouring entries, keeps the
// point list of a frame within 1 GiB and every count within 2^28.  "hough_max_accum" = 2^26 cells -- 256 MiB of accumulator per frame, a cell index fits the low
// word of the sort key; 4K at rho = 0.25, theta = pi / 720 (34.6 M cells) is inside it.
#include "rt.h"
#include "hough_math.h"
#include "hough_points.h"
#include <algorithm>
#include <vector>

using namespace mi355;

namespace mi355 {
size_t sortKeysDescTemp(unsigned n);                                                                             // gftt_sort.hip (rocPRIM)
bool sortKeysDesc(void* temp, size_t bytes, const unsigned long long* in, unsigned long long* out, unsigned n, hipStream_t st);
}

namespace {

using hough::Geom;

// ctr: two counters per frame, [2 f] the points, [2 f + 1] the candidates
__global__ __launch_bounds__(256) void k_hough_points(const uchar* __restrict__ src, size_t sstep, size_t sframe, int w, int h, uint32_t* __restrict__ pts, size_t pframe,
                                                      uint32_t* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63, x = blockIdx.x * 256 + 4 * lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;                                                      // the whole wave
    const uint32_t v = loadPix4(src + (size_t)blockIdx.z * sframe + (size_t)y * sstep, x, w);
    uint32_t pre;
    const uint32_t total = ballotPoints4(v, lane, &pre);
    if (!total) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(ctr + 2 * blockIdx.z, total);
    base = __shfl(base, 0, 64);
    uint32_t* out = pts + (size_t)blockIdx.z * pframe + base + pre;         // base + total <= w * h: every pixel is counted once
    storePoints4(v, x, y, out);
}

// tab: numangle sines, then numangle cosines, both already divided by rho
template <bool LDS>
__global__ __launch_bounds__(256) void k_hough_vote(const uint32_t* __restrict__ pts, size_t pframe, const uint32_t* __restrict__ ctr, const float* __restrict__ tab,
                                                    int numangle, int numrho, int* __restrict__ acc, size_t aframe)
{
    extern __shared__ int row[];
    const int n = blockIdx.y, bins = numrho + 2;
    const uint32_t np = ctr[2 * blockIdx.z], nchunks = (np + hough::VOTE_CHUNK - 1) / hough::VOTE_CHUNK;
    if (blockIdx.x >= nchunks) return;                                       // the whole workgroup
    if (LDS) {
        for (int i = threadIdx.x; i < bins; i += 256) row[i] = 0;
        __syncthreads();
    }
    const float s = tab[n], c = tab[numangle + n];
    const uint32_t* P = pts + (size_t)blockIdx.z * pframe;
    int* A = acc + (size_t)blockIdx.z * aframe;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint32_t end = min(np, (chunk + 1) * (uint32_t)hough::VOTE_CHUNK);
        for (uint32_t i = chunk * hough::VOTE_CHUNK + threadIdx.x; i < end; i += 256) {
            const uint32_t p = P[i];
            const int col = hough::voteColumn(hough::pointX(p), hough::pointY(p), c, s, numrho);
            if (LDS && (unsigned)col < (unsigned)bins) atomicAdd(&row[col], 1);
            else {
                const int64_t cell = hough::cellIndex(n, col, numrho);
                if (hough::inAccum(cell, numangle, numrho)) atomicAdd(A + cell, 1);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        int* R = A + (size_t)(n + 1) * bins;
        for (int i = threadIdx.x; i < bins; i += 256) { const int v = row[i]; if (v) atomicAdd(R + i, v); }
    }
}

// cand: the COMPLEMENT of the sort key (the device sort is a descending one), zeros behind the candidates
__global__ __launch_bounds__(256) void k_hough_maxima(const int* __restrict__ acc, size_t aframe, int numangle, int numrho, int threshold,
                                                      unsigned long long* __restrict__ cand, size_t cframe, uint32_t capacity, uint32_t* __restrict__ ctr)
{
    const int lane = threadIdx.x & 63, r = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    const int* A = acc + (size_t)blockIdx.z * aframe;
    const int b = (n + 1) * (numrho + 2) + r + 1;
    const bool is = r < numrho && hough::isMaximum(A, b, numrho, threshold);
    const uint64_t m = __ballot(is);
    if (!m) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(ctr + 2 * blockIdx.z + 1, (uint32_t)__popcll(m));
    base = __shfl(base, 0, 64);
    if (!is) return;
    const uint32_t at = base + __popcll(m & ((uint64_t(1) << lane) - 1));
    if (at < capacity) cand[(size_t)blockIdx.z * cframe + at] = ~hough::sortKey(A[b], b);
}

__global__ __launch_bounds__(256) void k_hough_emit(const unsigned long long* __restrict__ sorted, size_t cframe, const uint32_t* __restrict__ ctr, Geom g, int cn,
                                                    int top, float* __restrict__ lines, size_t lframe)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint32_t)top || i >= ctr[2 * blockIdx.y + 1]) return;              // top = min(max_lines, capacity of the candidate list)
    hough::emitLine(~sorted[(size_t)blockIdx.y * cframe + i], g, cn, lines + (size_t)blockIdx.y * lframe + (size_t)i * cn);
}

// ---- host side
// the refusals that need no device; 0 when the arguments are served
int houghArgs(const void* src, int w, int h, double rho, double theta, double srn, double stn, double minTheta, double maxTheta, int useEdgeval, Geom* g)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!src);
    if (srn != 0 || stn != 0) return MI355_DECLINED("srn != 0 || stn != 0 (the multi-scale transform)");
    if (useEdgeval) return MI355_DECLINED("use_edgeval");
    MI355_DECLINE_IF(w <= 0 || h <= 0 || w > lim::HOUGH_MAX_DIM || h > lim::HOUGH_MAX_DIM);
    const int rc = hough::geometry(w, h, rho, theta, minTheta, maxTheta, g);
    if (rc == 1) return MI355_DECLINED("rho <= 0, theta <= 0 or not 0 <= min_theta < max_theta <= CV_PI");
    if (rc) return MI355_DECLINED("(numangle + 2) * (numrho + 2) > lim::HOUGH_MAX_ACCUM");
    if (g->numangle > 65535) return MI355_DECLINED("numangle > 65535 (k_hough_vote has one grid row per angle)");
    return 0;
}

struct Scr {
    uint32_t* pts; int* acc; unsigned long long* cand; unsigned long long* sorted; void* temp; uint32_t* ctr; float* tab;
    size_t pf, af, cf, tempBytes;             // frame strides in elements
    uint32_t capacity;
    int group;
    std::vector<float> table;                 // the host's copy of tab: alive until the call has synchronised
};

// scratch for groups of frames, the trig table and the zeroed counters of all frames; with `lines` the candidate buffers too
bool houghScratch(Stager& stg, const Geom& g, int w, int h, int nframes, bool lines, Scr* s)
{
    const size_t cells = (size_t)(g.numangle + 2) * (g.numrho + 2);
    s->capacity = lines ? (uint32_t)hough::maxCandidates(g.numangle, g.numrho) : 0;
    const size_t pB = pad256((size_t)w * h * 4), aB = pad256(cells * 4), cB = pad256((size_t)s->capacity * 8);
    s->group = (int)std::min<size_t>((size_t)nframes, std::max<size_t>(1, (size_t(1) << 30) / (pB + aB + 2 * cB)));
    s->pf = pB / 4; s->af = aB / 4; s->cf = cB / 8;
    s->tempBytes = s->capacity > 1 ? sortKeysDescTemp(s->capacity) : 0;
    if (s->capacity > 1 && !s->tempBytes) return false;
    uchar* at = (uchar*)stg.scratch((pB + aB + 2 * cB) * s->group + pad256(s->tempBytes) + pad256((size_t)nframes * 8));
    s->table.resize(2 * (size_t)g.numangle);
    hough::trigTable(g, s->table.data(), s->table.data() + g.numangle);
    s->tab = (float*)stg.param(s->table.data(), s->table.size() * sizeof(float));
    if (!at || !s->tab) return false;
    s->pts = (uint32_t*)at; at += pB * s->group;
    s->acc = (int*)at; at += aB * s->group;
    s->cand = (unsigned long long*)at; at += cB * s->group;
    s->sorted = (unsigned long long*)at; at += cB * s->group;
    s->temp = at; at += pad256(s->tempBytes);
    s->ctr = (uint32_t*)at;
    return hipMemsetAsync(s->ctr, 0, (size_t)nframes * 8, stream()) == hipSuccess;
}

// points and votes of nf frames (dense device frames at sp); ctr points at the first of them
bool launchVotes(const Scr& s, const Geom& g, const uchar* sp, size_t sstep, size_t sframe, int w, int h, int nf, uint32_t* ctr, hipStream_t st)
{
    if (hipMemsetAsync(s.acc, 0, s.af * 4 * nf, st) != hipSuccess) return false;
    hipLaunchKernelGGL(k_hough_points, dim3(divUp(w, 256), divUp(h, 4), nf), dim3(256), 0, st, sp, sstep, sframe, w, h, s.pts, s.pf, ctr);
    const int gx = (int)std::min<size_t>(hough::VOTE_SPLIT, ((size_t)w * h + hough::VOTE_CHUNK - 1) / hough::VOTE_CHUNK), bins = g.numrho + 2;
    const dim3 grid(gx, g.numangle, nf);
    if (bins <= hough::LDS_BINS) hipLaunchKernelGGL(k_hough_vote<true>, grid, dim3(256), (size_t)bins * 4, st, s.pts, s.pf, ctr, s.tab, g.numangle, g.numrho, s.acc, s.af);
    else hipLaunchKernelGGL(k_hough_vote<false>, grid, dim3(256), 0, st, s.pts, s.pf, ctr, s.tab, g.numangle, g.numrho, s.acc, s.af);
    return true;
}

void noteVote(const Geom& g, int w, int h, int nframes, int group)
{
    const int gx = (int)std::min<size_t>(hough::VOTE_SPLIT, ((size_t)w * h + hough::VOTE_CHUNK - 1) / hough::VOTE_CHUNK), bins = g.numrho + 2;
    noteKernel("k_hough_vote<%s> grid=%dx%dx%d x256 lds=%zu, numangle=%d numrho=%d, k_hough_points + k_hough_maxima + sort + k_hough_emit, %d frame(s) in groups of %d",
               bins <= hough::LDS_BINS ? "lds" : "hbm", gx, g.numangle, std::min(group, nframes), bins <= hough::LDS_BINS ? (size_t)bins * 4 : (size_t)0, g.numangle, g.numrho,
               nframes, group);
}

// host-resident frames f0 .. f0 + nf - 1 into dense device rows
bool uploadFrames(const uchar* src, size_t sstep, size_t sframe, int w, int h, int nf, uchar* dev, size_t dstep, hipStream_t st)
{
    for (int f = 0; f < nf; f++)
        if (hipMemcpy2DAsync(dev + (size_t)f * dstep * h, dstep, src + (size_t)f * sframe, sstep, (size_t)w, h, hipMemcpyHostToDevice, st) != hipSuccess) return false;
    noteStagedBytes((long long)w * h * nf);
    return true;
}

int runHough(const char* entry, const uchar* src, size_t sstep, size_t sframe, int w, int h, float* lines, int cn, int maxLines, size_t lframeBytes, int nframes,
             double rho, double theta, int threshold, double srn, double stn, double minTheta, double maxTheta, int* nlines)
{
    Geom g;
    MI355_DECLINE_IF(!lines || !nlines || nframes < 1);
    if (const int rc = houghArgs(src, w, h, rho, theta, srn, stn, minTheta, maxTheta, 0, &g)) return rc;
    if (cn != 2 && cn != 3) return MI355_DECLINED("lines_cn is not 2 or 3");
    if (maxLines < 1) return MI355_DECLINED("max_lines < 1");
    const size_t lrow = (size_t)cn * 4;
    if (nframes > 1 && (lframeBytes % 4 || lframeBytes < lrow * maxLines)) return MI355_DECLINED("lines_frame_stride is no multiple of 4 or below max_lines rows");
    MI355_DECLINE_IF(nframes > 65535);
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    const int skind = ptrKind(src), lkind = ptrKind(lines);
    if (skind == PTR_FOREIGN || lkind == PTR_FOREIGN || skind != lkind)
        return MI355_DECLINED("image and lines must both live on this thread's device or both on the host");
    const bool host = skind == PTR_HOST;
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_HEAVY)));
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + w, lspan = (size_t)(nframes - 1) * lframeBytes + lrow * maxLines;
    MI355_DECLINE_IF(overlapOnDevice(src, sspan, lines, lspan));

    Scr s;
    if (!houghScratch(stg, g, w, h, nframes, true, &s)) return MI355_DECLINED("no scratch");
    uint32_t* hostN = (uint32_t*)stg.pinned((size_t)nframes * 8);
    // host-resident frames: dense copies of a group of sources, and the lines of all frames, in HBM
    const size_t hstep = pad256((size_t)w), hl = lrow * maxLines;
    uchar* hsrc = host ? (uchar*)stg.scratch(hstep * h * s.group) : nullptr;
    float* hlines = host ? (float*)stg.scratch(hl * nframes) : nullptr;
    if (!hostN || (host && (!hsrc || !hlines))) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    for (int f0 = 0; f0 < nframes; f0 += s.group) {
        const int nf = std::min(s.group, nframes - f0);
        const uchar* sp = src + (size_t)f0 * sframe;
        size_t ss = sstep, sf = sframe;
        if (host) {
            if (!uploadFrames(sp, sstep, sframe, w, h, nf, hsrc, hstep, st)) return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
            sp = hsrc; ss = hstep; sf = hstep * h;
        }
        uint32_t* ctr = s.ctr + 2 * (size_t)f0;
        if (!launchVotes(s, g, sp, ss, sf, w, h, nf, ctr, st)) return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed: %s", entry, hipGetErrorString(hipGetLastError()));
        if (!s.capacity) continue;                                           // numrho == 0: no inner cell, no line
        if (hipMemsetAsync(s.cand, 0, s.cf * 8 * nf, st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed: %s", entry, hipGetErrorString(hipGetLastError()));
        hipLaunchKernelGGL(k_hough_maxima, dim3(divUp(g.numrho, 256), g.numangle, nf), dim3(256), 0, st, s.acc, s.af, g.numangle, g.numrho, threshold, s.cand, s.cf, s.capacity, ctr);
        const unsigned long long* sorted = s.cand;
        if (s.capacity > 1) {
            for (int f = 0; f < nf; f++)
                if (!sortKeysDesc(s.temp, s.tempBytes, s.cand + (size_t)f * s.cf, s.sorted + (size_t)f * s.cf, s.capacity, st))
                    return setError(MI355CV_ERROR_UNKNOWN, "%s: sort failed: %s", entry, hipGetErrorString(hipGetLastError()));
            sorted = s.sorted;
        }
        float* lp = host ? hlines + (size_t)f0 * (hl / 4) : lines + (size_t)f0 * (lframeBytes / 4);
        const int top = (int)std::min<uint32_t>((uint32_t)maxLines, s.capacity);
        hipLaunchKernelGGL(k_hough_emit, dim3(divUp(top, 256), nf), dim3(256), 0, st, sorted, s.cf, ctr, g, cn, top, lp, host ? hl / 4 : lframeBytes / 4);
    }
    MI355_CHECK_LAUNCH(entry);
    // the call's one host synchronisation: the counts
    if (hipMemcpyAsync(hostN, s.ctr, (size_t)nframes * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
    if (host) {                                                              // only the rows that were written go back; then the host may look
        for (int f = 0; f < nframes; f++) {
            const size_t rows = std::min<size_t>(hostN[2 * f + 1], (size_t)maxLines);
            if (rows && hipMemcpyAsync((uchar*)lines + (size_t)f * lframeBytes, (uchar*)hlines + (size_t)f * hl, rows * lrow, hipMemcpyDeviceToHost, st) != hipSuccess)
                return setError(MI355CV_ERROR_UNKNOWN, "%s: D2H failed: %s", entry, hipGetErrorString(hipGetLastError()));
            noteStagedBytes((long long)(rows * lrow));
        }
        if (hipStreamSynchronize(st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: D2H failed: %s", entry, hipGetErrorString(hipGetLastError()));
    }
    for (int f = 0; f < nframes; f++) nlines[f] = (int)hostN[2 * f + 1];
    noteVote(g, w, h, nframes, s.group);
    return stg.finish(entry);
}

} // namespace

static_assert(lim::HOUGH_MAX_DIM == hough::MAX_DIM && lim::HOUGH_MAX_ACCUM == hough::MAX_ACCUM, "one bound");
static_assert(hough::MAX_DIM <= 65535, "packed points");
static_assert(hough::LDS_BINS * sizeof(int) <= 65536, "the row of k_hough_vote<true> in LDS");

extern "C" {

MI355CV_API int mi355cv_houghLines(const uchar* src_data, size_t src_step, int width, int height, float* lines, int lines_cn, int max_lines,
                                   double rho, double theta, int threshold, double srn, double stn, double min_theta, double max_theta, int* nlines)
{
    mi355::EntryGuard entry_(__func__);
    return runHough("houghLines", src_data, src_step, 0, width, height, lines, lines_cn, max_lines, 0, 1, rho, theta, threshold, srn, stn, min_theta, max_theta, nlines);
}

MI355CV_API int mi355cv_houghLinesBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, int width, int height, float* lines, int lines_cn,
                                        int max_lines, size_t lines_frame_stride, int nframes, double rho, double theta, int threshold, double srn, double stn,
                                        double min_theta, double max_theta, int* nlines)
{
    mi355::EntryGuard entry_(__func__);
    return runHough("houghLinesBatch", src_data, src_step, nframes == 1 ? 0 : src_frame_stride, width, height, lines, lines_cn, max_lines,
                    nframes == 1 ? 0 : lines_frame_stride, nframes, rho, theta, threshold, srn, stn, min_theta, max_theta, nlines);
}

MI355CV_API int mi355cv_houghLinesAccum(const uchar* src_data, size_t src_step, int width, int height, double rho, double theta, double min_theta, double max_theta,
                                        int* accum, size_t accum_step, int* numangle, int* numrho)
{
    mi355::EntryGuard entry_(__func__);
    const char* entry = "houghLinesAccum";
    Geom g;
    MI355_DECLINE_IF(!numangle || !numrho);
    if (const int rc = houghArgs(src_data, width, height, rho, theta, 0, 0, min_theta, max_theta, 0, &g)) return rc;
    const size_t rowBytes = (size_t)(g.numrho + 2) * 4;
    const int rows = g.numangle + 2;
    if (!accum) { *numangle = g.numangle; *numrho = g.numrho; return MI355CV_OK; }        // the geometry alone: no device is touched
    if (accum_step < rowBytes || accum_step % 4) return MI355_DECLINED("accum_step is below (numrho + 2) ints or no multiple of 4");
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    const int skind = ptrKind(src_data), akind = ptrKind(accum);
    if (skind == PTR_FOREIGN || akind == PTR_FOREIGN || skind != akind)
        return MI355_DECLINED("image and accumulator must both live on this thread's device or both on the host");
    const bool host = skind == PTR_HOST;
    MI355_DECLINE_IF(hostImageTooSmall(src_data, (size_t)width * height, minPixels(HOST_HEAVY)));
    MI355_DECLINE_IF(overlapOnDevice(src_data, (size_t)(height - 1) * src_step + width, accum, (size_t)(rows - 1) * accum_step + rowBytes));
    Scr s;
    if (!houghScratch(stg, g, width, height, 1, false, &s)) return MI355_DECLINED("no scratch");
    const size_t hstep = pad256((size_t)width);
    uchar* hsrc = host ? (uchar*)stg.scratch(hstep * height) : nullptr;
    if (host && !hsrc) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    const uchar* sp = src_data; size_t ss = src_step;
    if (host) {
        if (!uploadFrames(src_data, src_step, 0, width, height, 1, hsrc, hstep, st)) return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D failed: %s", entry, hipGetErrorString(hipGetLastError()));
        sp = hsrc; ss = hstep;
    }
    if (!launchVotes(s, g, sp, ss, 0, width, height, 1, s.ctr, st)) return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed: %s", entry, hipGetErrorString(hipGetLastError()));
    MI355_CHECK_LAUNCH(entry);
    if (hipMemcpy2DAsync(accum, accum_step, s.acc, rowBytes, rowBytes, rows, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st) != hipSuccess)
        return setError(MI355CV_ERROR_UNKNOWN, "%s: copy failed: %s", entry, hipGetErrorString(hipGetLastError()));
    if (host) {
        noteStagedBytes((long long)(rowBytes * rows));
        if (hipStreamSynchronize(st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: execution failed: %s", entry, hipGetErrorString(hipGetLastError()));
    }
    *numangle = g.numangle; *numrho = g.numrho;
    noteVote(g, width, height, 1, 1);
    return stg.finish(entry);
}

} // extern "C"
