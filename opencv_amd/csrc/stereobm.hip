// stereobm.hip -- cv::StereoBM on the GPU: XSOBEL prefilter, SAD block matching, texture / uniqueness rejects, sub-pixel disparity, the left-right check, CV_16S and
// CV_32F maps, single pairs and batches.  The definition is the project's own restatement (tests/stereobm_restate.py); the per-pixel pieces are in
// stereobm_math.h, compiled for the host by tests/hostemu/stereobm_emu.cpp.  All arithmetic is integer: the maps are held bit for bit.
//
//   k_sbm_prefilter     both images of every frame into dense 16-byte-aligned planes; a lane makes 16 pixels, with 16-byte loads where the source row allows
//   k_sbm_fill          FILTERED into the columns outside [xlo, xhi)
//   k_sbm_cost_generic  any parameter set within the limits: a workgroup stages w rows of both planes around GENERIC_TILE pixels of one row into LDS and recomputes the
//                       window per (pixel, disparity); one lane per pixel runs sbm::decide over the 32-bit SADs in LDS
//   k_sbm_cost_roll     the fast kernel, w <= ROLL_MAX_BLOCK: a workgroup of n / 16 waves owns ROLL_TILE window columns and walks down ROLL_STRIP rows.  Wave k, lane l keeps
//                       the vertical sums of window column l for the 16 disparity indices of chunk k in registers, adds the entering row's |L - R| and takes off the
//                       leaving row's (both rows staged in LDS, so the shifted reads are LDS reads), hands the sums over in LDS, where the w columns of a window are
//                       added with a sliding sum; the decision runs in parallel over a pixel's chunks.  SADs fit 16 bits.
//   k_sbm_lr_vote / k_sbm_lr_apply   the left-right check: one 64-bit atomicMin per pixel into its target column, then the reject
//   k_sbm_to32f         CV_16S -> CV_32F, exact
// A batch is one sequence of launches: the frame is the grid's z.
#include "rt.h"
#include "stereobm_math.h"
#include <algorithm>
#include <atomic>
#include <vector>

namespace {
using namespace mi355;
using sbm::Geom;

static_assert(sbm::MAX_DISPARITIES == lim::STEREOBM_MAX_DISPARITIES && sbm::MAX_BLOCK == lim::STEREOBM_MAX_BLOCK && sbm::MAX_DIM == lim::STEREOBM_MAX_DIM &&
              sbm::ROLL_MAX_BLOCK == lim::STEREOBM_ROLL_MAX_BLOCK && sbm::ROLL_CHUNK == lim::STEREOBM_CHUNK && sbm::ROLL_TILE == lim::STEREOBM_TILE_COLS &&
              sbm::ROLL_STRIP == lim::STEREOBM_STRIP_ROWS && sbm::GENERIC_TILE == lim::STEREOBM_GENERIC_TILE_COLS, "mi355cv_limit(\"stereobm_*\")");
static_assert(sbm::ROLL_MAX_BLOCK * sbm::ROLL_MAX_BLOCK * 126 < 65536 && sbm::MAX_BLOCK * sbm::MAX_BLOCK * 126 < (1 << 19), "SADs of the fast kernel in 16 bits; the key of minKey");
static_assert(sbm::MAX_DISPARITIES / sbm::ROLL_CHUNK * 64 <= 1024 && sbm::ROLL_TILE == 64, "a wave per chunk, a lane per window column");

// one frame of a call: the two images, the CV_16S map the cost kernels write (the destination itself or scratch) and the destination
struct Frame { const uchar* l; size_t ls; const uchar* r; size_t rs; uchar* d16; size_t d16s; uchar* out; size_t outs; };
// the dense planes of a call: prefiltered left / right (bytes), the winners' costs and the left-right keys (only with disp12MaxDiff >= 0)
struct Planes { uchar* pl; uchar* pr; size_t pstep, pframe; uint32_t* cost; unsigned long long* keys; size_t cstep, cframe; };
struct Decision { int textureThreshold, uniquenessRatio; };

// ------------------------------------------------------------------------------------------------------------------------------------ prefilter
// dst: `aligned` says that every destination row starts on a 16-byte boundary and has room for whole groups of 16
__global__ __launch_bounds__(256) void k_sbm_prefilter(const uchar* __restrict__ src0, size_t sstep, size_t sframe, uchar* __restrict__ dst0, size_t dstep, size_t dframe,
                                                       const Frame* __restrict__ frames, int which, int W, int H, int cap, int srcAligned, int dstAligned)
{
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 16, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= W || y >= H) return;
    const uchar* src; uchar* dst;
    if (frames) { const Frame F = frames[blockIdx.z]; src = which ? F.r : F.l; sstep = which ? F.rs : F.ls; dst = dst0 + (size_t)blockIdx.z * dframe; }
    else { src = src0 + (size_t)blockIdx.z * sframe; dst = dst0 + (size_t)blockIdx.z * dframe; }
    const uchar* rows[3] = {src + (size_t)sbm::reflect101(y - 1, H) * sstep, src + (size_t)y * sstep, src + (size_t)sbm::reflect101(y + 1, H) * sstep};
    uchar out[16];
    if (srcAligned && x0 + 16 <= W) {
        // 18 bytes of each row: the 16 of the group and one neighbour on either side (the image's own border columns are not read: they answer `cap`)
        uchar b[3][18];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const uint4 v = *(const uint4*)(rows[r] + x0);
            const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; i++) b[r][i + 1] = (uchar)(q[i >> 2] >> (8 * (i & 3)));
            b[r][0] = x0 > 0 ? rows[r][x0 - 1] : 0;
            b[r][17] = x0 + 16 < W ? rows[r][x0 + 16] : 0;
        }
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int x = x0 + i;
            const int v = cap + ((int)b[0][i + 2] - (int)b[0][i]) + 2 * ((int)b[1][i + 2] - (int)b[1][i]) + ((int)b[2][i + 2] - (int)b[2][i]);
            out[i] = (x < 1 || x > W - 2) ? (uchar)cap : (uchar)sbm::clampi(v, 0, 2 * cap);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) out[i] = x0 + i < W ? sbm::xsobelPixel(rows[0], rows[1], rows[2], x0 + i, W, cap) : (uchar)0;
    }
    uchar* drow = dst + (size_t)y * dstep + x0;
    if (dstAligned) {
        uint32_t q[4];
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = (uint32_t)out[4 * i] | ((uint32_t)out[4 * i + 1] << 8) | ((uint32_t)out[4 * i + 2] << 16) | ((uint32_t)out[4 * i + 3] << 24);
        *(uint4*)drow = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) if (x0 + i < W) drow[i] = out[i];
    }
}

__global__ __launch_bounds__(256) void k_sbm_fill(const Frame* __restrict__ frames, int W, int H, Geom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W || (x >= g.xlo && x < g.xhi)) return;
    const Frame F = frames[blockIdx.z];
    *(short*)(F.d16 + (size_t)y * F.d16s + (size_t)x * 2) = (short)g.filtered;
}

// ------------------------------------------------------------------------------------------------------------------------------------ generic cost kernel
// dynamic LDS: Lt[w][lw] bytes, Rt[w][rw] bytes, cost[GENERIC_TILE][n + 1] ints (index n: the texture sum)
__global__ __launch_bounds__(256) void k_sbm_cost_generic(const Frame* __restrict__ frames, Planes P, int W, int H, Geom g, int w, Decision dec, int cap, int lw, int rw)
{
    extern __shared__ __attribute__((aligned(16))) uchar smem[];
    constexpr int GP = sbm::GENERIC_TILE;
    const int h = w >> 1, n = g.n, S = n + 1;
    uchar* Lt = smem;
    uchar* Rt = Lt + w * lw;
    int* cost = (int*)(smem + (((size_t)w * (lw + rw) + 15) & ~(size_t)15));
    const int X0 = g.xlo + blockIdx.x * GP, y = blockIdx.y, t = threadIdx.x;
    const uchar* pl = P.pl + (size_t)blockIdx.z * P.pframe;
    const uchar* pr = P.pr + (size_t)blockIdx.z * P.pframe;
    // left tile: window columns u = X0 - h + j; right tile: image columns base + j, base = the smallest column any (u, D) of the tile reads
    const int base = sbm::rightCol(X0 - h, g.Dmax, g);
    for (int i = t; i < w * lw; i += 256) {
        const int r = i / lw, j = i - r * lw;
        Lt[i] = pl[(size_t)sbm::clampi(y - h + r, 0, H - 1) * P.pstep + sbm::leftCol(X0 - h + j, W)];
    }
    for (int i = t; i < w * rw; i += 256) {
        const int r = i / rw, j = i - r * rw;
        Rt[i] = pr[(size_t)sbm::clampi(y - h + r, 0, H - 1) * P.pstep + min(base + j, W - 1)];
    }
    __syncthreads();
    for (int item = t; item < GP * S; item += 256) {
        const int p = item % GP, i = item / GP, X = X0 + p;
        if (X >= g.xhi) continue;
        uint32_t s = 0;
        if (i < n) {
            const int D = g.Dmax - i;
            for (int dy = 0; dy < w; dy++)
                for (int dx = 0; dx < w; dx++)
                    s = sbm::absdiffAcc(Lt[dy * lw + p + dx], Rt[dy * rw + sbm::rightCol(X - h + dx, D, g) - base], s);
        } else {
            for (int dy = 0; dy < w; dy++)
                for (int dx = 0; dx < w; dx++) s = sbm::absdiffAcc(Lt[dy * lw + p + dx], (uint32_t)cap, s);
        }
        cost[p * S + i] = (int)s;
    }
    __syncthreads();
    if (t >= GP || X0 + t >= g.xhi) return;
    const int X = X0 + t;
    const Frame F = frames[blockIdx.z];
    const int* c = cost + t * S;
    int win = 0;
    const int d = sbm::decide([c](int i) { return c[i]; }, n, c[n], dec.textureThreshold, dec.uniquenessRatio, g, &win);
    *(short*)(F.d16 + (size_t)y * F.d16s + (size_t)X * 2) = (short)d;
    if (P.cost) P.cost[(size_t)blockIdx.z * P.cframe + (size_t)y * P.cstep + X] = (uint32_t)win;
}

// ------------------------------------------------------------------------------------------------------------------------------------ fast cost kernel
constexpr int RT = sbm::ROLL_TILE, RC = sbm::ROLL_CHUNK;

// a staged row, one run of bytes: Ls[j] = PL[row][leftCol(u0 + j)], j < 64, then Rs[j] = PR[row][min(base + j, W - 1)], j < 64 + n
__device__ __forceinline__ void stageRow(uchar* Ls, const uchar* __restrict__ pl, const uchar* __restrict__ pr, size_t pstep, int row, int u0, int base, int W, int n,
                                         int t, int nthreads)
{
    // one byte per lane and pass: the left row's 64 first, then the right row's; the trip count is the same for every lane
    const size_t off = (size_t)row * pstep;
#pragma unroll 1
    for (int j0 = 0; j0 < RT + RT + n; j0 += nthreads) {
        const int j = j0 + t;
        if (j >= RT + RT + n) continue;
        const bool left = j < RT;
        const int col = left ? sbm::leftCol(u0 + j, W) : min(base + (j - RT), W - 1);
        Ls[j] = (left ? pl : pr)[off + (uint32_t)col];
    }
}

// dynamic LDS (n disparities, S = n + 2 halfwords per row): rowbuf[2][64 + 64 + n] bytes | Vs[64][S] u16 (the per-chunk minima alias it later) | cost[60][S] u16 | rej[64] ints
__global__ __launch_bounds__(1024) void k_sbm_cost_roll(const Frame* __restrict__ frames, Planes P, int W, int H, Geom g, int w, Decision dec, int cap)
{
    extern __shared__ __attribute__((aligned(16))) uchar smem[];
    const int h = w >> 1, n = g.n, S = n + 2, TW = RT - 2 * h, nthreads = blockDim.x;
    const int rowBytes = RT + RT + n;
    uchar* rowbuf = smem;
    uint16_t* Vs = (uint16_t*)(smem + 2 * rowBytes);
    uint16_t* cost = Vs + RT * S;
    int* rej = (int*)(cost + (RT - 4) * S);
    uint32_t* part = (uint32_t*)Vs;
    const int t = threadIdx.x, l = t & 63, k = t >> 6, nchunks = n / RC;
    const int X0 = g.xlo + blockIdx.x * TW, u0 = X0 - h, y0 = blockIdx.y * sbm::ROLL_STRIP, y1 = min(H, y0 + sbm::ROLL_STRIP);
    const int npix = min(TW, g.xhi - X0);
    const uchar* pl = P.pl + (size_t)blockIdx.z * P.pframe;
    const uchar* pr = P.pr + (size_t)blockIdx.z * P.pframe;
    uchar* const d16 = frames[blockIdx.z].d16;
    const size_t d16s = frames[blockIdx.z].d16s;
    const int base = sbm::rightCol(u0, g.Dmax, g);
    // this lane's first byte in a staged right row: index i = 16 k + j reads column rightCol(u, Dmax - i) = rightCol(u, Dmax) + i
    const int ridx = sbm::rightCol(u0 + l, g.Dmax, g) + RC * k - base;
    uint32_t V[RC], Vt = 0;
#pragma unroll
    for (int j = 0; j < RC; j++) V[j] = 0;
    if (t < 64) rej[t] = 0;

    // the window's rows of the strip's first pixel row, two at a time
#pragma unroll 1
    for (int r = 0; r < w; r += 2) {
        __syncthreads();
        stageRow(rowbuf, pl, pr, P.pstep, sbm::clampi(y0 - h + r, 0, H - 1), u0, base, W, n, t, nthreads);
        if (r + 1 < w) stageRow(rowbuf + rowBytes, pl, pr, P.pstep, sbm::clampi(y0 - h + r + 1, 0, H - 1), u0, base, W, n, t, nthreads);
        __syncthreads();
#pragma unroll 1
        for (int b = 0; b < 2 && r + b < w; b++) {
            const uchar* Ls = rowbuf + b * rowBytes;
            const uchar* Rs = Ls + RT + ridx;
            const uint32_t a = Ls[l];
#pragma unroll
            for (int j = 0; j < RC; j++) V[j] = sbm::absdiffAcc(a, Rs[j], V[j]);
            if (k == 0) Vt = sbm::absdiffAcc(a, (uint32_t)cap, Vt);
        }
    }

#pragma unroll 1
    for (int y = y0; y < y1; y++) {
        if (y > y0) {
            // row y + h enters, row y - 1 - h leaves (the row buffers were last read before the three barriers of the row above)
            stageRow(rowbuf, pl, pr, P.pstep, sbm::clampi(y + h, 0, H - 1), u0, base, W, n, t, nthreads);
            stageRow(rowbuf + rowBytes, pl, pr, P.pstep, sbm::clampi(y - 1 - h, 0, H - 1), u0, base, W, n, t, nthreads);
            __syncthreads();
            const uchar* Le = rowbuf; const uchar* Re = Le + RT + ridx;
            const uchar* Ll = rowbuf + rowBytes; const uchar* Rl = Ll + RT + ridx;
            const uint32_t ae = Le[l], al = Ll[l];
#pragma unroll
            for (int j = 0; j < RC; j++) V[j] = sbm::absdiffAcc(ae, Re[j], V[j]) - sbm::absdiffAcc(al, Rl[j], 0);
            if (k == 0) Vt = sbm::absdiffAcc(ae, (uint32_t)cap, Vt) - sbm::absdiffAcc(al, (uint32_t)cap, 0);
        }
        // the vertical sums of window column l, indices 16 k .. 16 k + 15 (and the texture column at index n)
        {
            uint32_t* row = (uint32_t*)(Vs + l * S + RC * k);
#pragma unroll
            for (int j = 0; j < RC; j += 2) row[j >> 1] = V[j] | (V[j + 1] << 16);
            if (k == 0) Vs[l * S + n] = (uint16_t)Vt;
        }
        __syncthreads();
        // the w columns of a window: index i, a third of the tile's pixels per lane, a sliding sum
        if (t < 3 * (n + 1)) {
            const int i = t % (n + 1), seg = t / (n + 1), SL = (TW + 2) / 3;
            const int p0 = seg * SL, p1 = min(npix, p0 + SL);
            if (p0 < p1) {
                uint32_t s = 0;
#pragma unroll 1
                for (int u = p0; u < p0 + w; u++) s += Vs[u * S + i];
                cost[p0 * S + i] = (uint16_t)s;
#pragma unroll 1
                for (int p = p0 + 1; p < p1; p++) {
                    s += Vs[(p + w - 1) * S + i];
                    s -= Vs[(p - 1) * S + i];
                    cost[p * S + i] = (uint16_t)s;
                }
            }
        }
        __syncthreads();
        // the decision, lane l = pixel, wave k = chunk: the chunk's minimum, then the pixel's, then the chunk's uniqueness votes
        uint32_t c[RC];
        const bool live = l < npix;
        if (live) {
            const uint32_t* row = (const uint32_t*)(cost + l * S + RC * k);
            uint32_t best = 0xffffffffu;
#pragma unroll
            for (int j = 0; j < RC; j += 2) {
                const uint32_t v = row[j >> 1];
                c[j] = v & 0xffffu; c[j + 1] = v >> 16;
            }
#pragma unroll
            for (int j = 0; j < RC; j++) best = min(best, sbm::minKey(c[j], RC * k + j));
            part[l * nchunks + k] = best;
        }
        __syncthreads();
        uint32_t best = 0xffffffffu;
        if (live) {
#pragma unroll 1
            for (int q = 0; q < nchunks; q++) best = min(best, part[l * nchunks + q]);
            if (dec.uniquenessRatio > 0) {
                const int ms = sbm::keyCost(best), mi = sbm::keyIndex(best);
                uint32_t mo = sbm::NO_COST;
#pragma unroll
                for (int j = 0; j < RC; j++) mo = min(mo, sbm::outsideCost(RC * k + j, mi, c[j]));
                if (sbm::uniqRejects(mo, ms, dec.uniquenessRatio)) rej[l] = 1;
            }
        }
        __syncthreads();
        if (live && k == 0) {
            const uint16_t* cr = cost + l * S;
            const int ms = sbm::keyCost(best), mi = sbm::keyIndex(best);
            int d = g.filtered;
            if (!((int)cr[n] < dec.textureThreshold) && !rej[l]) d = sbm::subpixel(ms, cr[sbm::nextIndex(mi, n)], cr[sbm::prevIndex(mi)], g.Dmax, mi);
            rej[l] = 0;
            const int X = X0 + l;
            *(short*)(d16 + (size_t)y * d16s + (size_t)X * 2) = (short)d;
            if (P.cost) P.cost[(size_t)blockIdx.z * P.cframe + (size_t)y * P.cstep + X] = (uint32_t)ms;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ left-right check, CV_32F
__global__ __launch_bounds__(256) void k_sbm_lr_vote(const Frame* __restrict__ frames, Planes P, int W, int H, Geom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const Frame F = frames[blockIdx.z];
    const int d = *(const short*)(F.d16 + (size_t)y * F.d16s + (size_t)x * 2);
    if (d == g.filtered) return;
    const int x2 = sbm::lrTarget(x, d);
    if (x2 < 0 || x2 >= W) return;
    const size_t rowOff = (size_t)blockIdx.z * P.cframe + (size_t)y * P.cstep;
    atomicMin(P.keys + rowOff + x2, sbm::lrKey((int)P.cost[rowOff + x], x, d));
}

__global__ __launch_bounds__(256) void k_sbm_lr_apply(const Frame* __restrict__ frames, Planes P, int W, int H, Geom g, int disp12MaxDiff)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const Frame F = frames[blockIdx.z];
    short* dp = (short*)(F.d16 + (size_t)y * F.d16s + (size_t)x * 2);
    const int d = *dp;
    if (d == g.filtered) return;
    const unsigned long long* keys = P.keys + (size_t)blockIdx.z * P.cframe + (size_t)y * P.cstep;
    const int filtered = g.filtered;
    if (sbm::lrRejects([keys, filtered](int xk) { return sbm::lrDisp(keys[xk], filtered); }, x, d, W, disp12MaxDiff, filtered)) *dp = (short)filtered;
}

__global__ __launch_bounds__(256) void k_sbm_to32f(const Frame* __restrict__ frames, int W, int H)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const Frame F = frames[blockIdx.z];
    *(float*)(F.out + (size_t)y * F.outs + (size_t)x * 4) = (float)*(const short*)(F.d16 + (size_t)y * F.d16s + (size_t)x * 2) * 0.0625f;
}

// ------------------------------------------------------------------------------------------------------------------------------------ host side
std::atomic<int> g_kernelMode{-1};       // mi355cv_stereoBMSetKernel: -1 the rule below, 0 always the generic kernel (the A/B's other arm)

struct Args { int m, n, w, cap, tex, uniq, lr; };

// refusals that need no device
int checkParams(const mi355cv_StereoBMParams* p, int width, int height, int disp_depth, Args* A)
{
    MI355_DECLINE_IF(disabled() || !p);
    MI355_DECLINE_IF(width < 1 || height < 1 || width > lim::STEREOBM_MAX_DIM || height > lim::STEREOBM_MAX_DIM);
    if (disp_depth != MI355CV_16S && disp_depth != MI355CV_32F) return MI355_DECLINED("the disparity map is neither CV_16SC1 nor CV_32FC1");
    if (p->preFilterType != sbm::PREFILTER_XSOBEL) return MI355_DECLINED("preFilterType other than PREFILTER_XSOBEL (PREFILTER_NORMALIZED_RESPONSE is not served)");
    if (p->speckleWindowSize > 0) return MI355_DECLINED("speckleWindowSize > 0: cv::filterSpeckles is not served");
    if (p->roi1[2] || p->roi1[3] || p->roi2[2] || p->roi2[3]) return MI355_DECLINED("roi1 / roi2: ROI-based validity is not served");
    const int n = p->numDisparities <= 0 ? 64 : p->numDisparities;
    MI355_DECLINE_IF(n % 16 != 0 || n > lim::STEREOBM_MAX_DISPARITIES);
    const int w = p->blockSize;
    MI355_DECLINE_IF(w % 2 == 0 || w < 5 || w > lim::STEREOBM_MAX_BLOCK || w > std::min(width, height));
    MI355_DECLINE_IF(p->preFilterCap < 1 || p->preFilterCap > 63);
    MI355_DECLINE_IF(p->textureThreshold < 0 || p->uniquenessRatio < 0);
    // the CV_16S map holds 16 D + 8 at most and (m - 1) * 16 at least
    if (p->minDisparity < -2047 || (long long)p->minDisparity + n - 1 > 2046) return MI355_DECLINED("minDisparity .. minDisparity + numDisparities - 1 leaves the range of a CV_16S map (-2047 .. 2046)");
    *A = Args{p->minDisparity, n, w, p->preFilterCap, p->textureThreshold, p->uniquenessRatio, p->disp12MaxDiff};
    return MI355CV_OK;
}

void launchPrefilter(const uchar* src, size_t sstep, size_t sframe, uchar* dst, size_t dstep, size_t dframe, const Frame* frames, int which, int W, int H, int cap, int nframes,
                     bool srcAligned, bool dstAligned, hipStream_t st)
{
    hipLaunchKernelGGL(k_sbm_prefilter, dim3(divUp(divUp(W, 16), 64), divUp(H, 4), nframes), dim3(256), 0, st, src, sstep, sframe, dst, dstep, dframe, frames, which, W, H, cap,
                       srcAligned ? 1 : 0, dstAligned ? 1 : 0);
}

struct HostFrame { const uchar* l; const uchar* r; uchar* d; };

int runStereo(const char* entry, const HostFrame* hf, int nframes, size_t lstep, size_t rstep, size_t dstep, int W, int H, int depth, const mi355cv_StereoBMParams* params)
{
    Args A;
    if (const int rc = checkParams(params, W, H, depth, &A)) return rc;
    const size_t esz = depth == MI355CV_16S ? 2 : 4;
    MI355_DECLINE_IF(nframes < 1 || nframes > 65535);
    MI355_DECLINE_IF(lstep < (size_t)W || rstep < (size_t)W || dstep < (size_t)W * esz);
    for (int f = 0; f < nframes; f++) {
        MI355_DECLINE_IF(!hf[f].l || !hf[f].r || !hf[f].d);
        if (((size_t)hf[f].d | dstep) & (esz - 1)) return MI355_DECLINED("disparity rows off their element's boundary");
    }
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(hf[0].l, (size_t)W * H, minPixels(HOST_HEAVY)));
    const size_t dspan = span(dstep, H, (size_t)W * esz);
    for (int f = 0; f < nframes; f++) {
        if (overlapOnDevice(hf[f].l, span(lstep, H, W), hf[f].d, dspan) || overlapOnDevice(hf[f].r, span(rstep, H, W), hf[f].d, dspan))
            return MI355_DECLINED("the disparity map overlaps an input");
        for (int j = 0; j < nframes; j++) {
            if (j != f && (overlapOnDevice(hf[j].l, span(lstep, H, W), hf[f].d, dspan) || overlapOnDevice(hf[j].r, span(rstep, H, W), hf[f].d, dspan)))
                return MI355_DECLINED("the disparity map overlaps an input");
            if (j < f && overlapOnDevice(hf[j].d, dspan, hf[f].d, dspan)) return MI355_DECLINED("two disparity maps of the batch overlap");
        }
    }
    const Geom g = sbm::geomOf(W, A.m, A.n);
    const bool lr = A.lr >= 0;
    // the dense planes
    Planes P{};
    P.pstep = ((size_t)W + 15) & ~(size_t)15;
    P.pframe = P.pstep * H;
    P.pl = (uchar*)stg.scratch(P.pframe * nframes);
    P.pr = (uchar*)stg.scratch(P.pframe * nframes);
    if (!P.pl || !P.pr) return MI355_DECLINED("no scratch for the prefiltered planes");
    P.cstep = W; P.cframe = (size_t)W * H;
    if (lr) {
        P.cost = (uint32_t*)stg.scratch(P.cframe * nframes * sizeof(uint32_t));
        P.keys = (unsigned long long*)stg.scratch(P.cframe * nframes * sizeof(unsigned long long));
        if (!P.cost || !P.keys) return MI355_DECLINED("no scratch for the left-right check");
    }
    short* d16 = nullptr;
    const size_t d16step = (size_t)W * 2;
    if (depth == MI355CV_32F) { d16 = (short*)stg.scratch(d16step * H * nframes); if (!d16) return MI355_DECLINED("no scratch for the CV_16S map"); }
    std::vector<Frame> fr(nframes);
    bool srcAligned = true;
    for (int f = 0; f < nframes; f++) {
        Frame& F = fr[f];
        F.l = stg.in(hf[f].l, lstep, (size_t)W, H, &F.ls);
        F.r = stg.in(hf[f].r, rstep, (size_t)W, H, &F.rs);
        F.out = stg.out(hf[f].d, dstep, (size_t)W * esz, H, &F.outs);
        if (!F.l || !F.r || !F.out) return MI355_DECLINED("staging failed");
        if (d16) { F.d16 = (uchar*)d16 + d16step * H * f; F.d16s = d16step; } else { F.d16 = F.out; F.d16s = F.outs; }
        if (((size_t)F.l | F.ls | (size_t)F.r | F.rs) & 15) srcAligned = false;
    }
    const Frame* dFrames = (const Frame*)stg.param(fr.data(), fr.size() * sizeof(Frame));
    if (!dFrames) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    launchPrefilter(nullptr, 0, 0, P.pl, P.pstep, P.pframe, dFrames, 0, W, H, A.cap, nframes, srcAligned, true, st);
    launchPrefilter(nullptr, 0, 0, P.pr, P.pstep, P.pframe, dFrames, 1, W, H, A.cap, nframes, srcAligned, true, st);
    if (g.xlo > 0 || g.xhi < W) hipLaunchKernelGGL(k_sbm_fill, dim3(divUp(W, 256), H, nframes), dim3(256), 0, st, dFrames, W, H, g);
    const Decision dec{A.tex, A.uniq};
    const int valid = g.xhi - g.xlo;
    if (valid > 0) {
        const int h = A.w / 2;
        const bool roll = A.w <= sbm::ROLL_MAX_BLOCK && g_kernelMode.load(std::memory_order_relaxed) != 0;
        if (roll) {
            const int TW = sbm::ROLL_TILE - 2 * h, S = A.n + 2;
            const size_t lds = 2 * (size_t)(2 * sbm::ROLL_TILE + A.n) + (size_t)sbm::ROLL_TILE * S * 2 + (size_t)(sbm::ROLL_TILE - 4) * S * 2 + 64 * sizeof(int);
            const dim3 grid(divUp(valid, TW), divUp(H, sbm::ROLL_STRIP), nframes), block(64 * (A.n / sbm::ROLL_CHUNK));
            hipLaunchKernelGGL(k_sbm_cost_roll, grid, block, lds, st, dFrames, P, W, H, g, A.w, dec, A.cap);
            noteKernel("k_sbm_cost_roll grid=%ux%ux%u x%u lds=%zu, n=%d w=%d, %d pixel(s) x %d row(s) per workgroup%s", grid.x, grid.y, grid.z, block.x, lds, A.n, A.w, TW,
                       sbm::ROLL_STRIP, lr ? ", k_sbm_lr_vote + k_sbm_lr_apply" : "");
        } else {
            const int lw = sbm::GENERIC_TILE + A.w - 1, rw = lw + A.n - 1;
            const size_t lds = (((size_t)A.w * (lw + rw) + 15) & ~(size_t)15) + (size_t)sbm::GENERIC_TILE * (A.n + 1) * sizeof(int);
            const dim3 grid(divUp(valid, sbm::GENERIC_TILE), H, nframes);
            hipLaunchKernelGGL(k_sbm_cost_generic, grid, dim3(256), lds, st, dFrames, P, W, H, g, A.w, dec, A.cap, lw, rw);
            noteKernel("k_sbm_cost_generic grid=%ux%ux%u x256 lds=%zu, n=%d w=%d%s", grid.x, grid.y, grid.z, lds, A.n, A.w, lr ? ", k_sbm_lr_vote + k_sbm_lr_apply" : "");
        }
        if (lr) {
            if (hipMemsetAsync(P.keys, 0xff, P.cframe * nframes * sizeof(unsigned long long), st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed", entry);
            const dim3 grid(divUp(W, 256), H, nframes);
            hipLaunchKernelGGL(k_sbm_lr_vote, grid, dim3(256), 0, st, dFrames, P, W, H, g);
            hipLaunchKernelGGL(k_sbm_lr_apply, grid, dim3(256), 0, st, dFrames, P, W, H, g, A.lr);
        }
    } else noteKernel("k_sbm_fill grid=%dx%dx%d x256: no valid column", divUp(W, 256), H, nframes);
    if (depth == MI355CV_32F) hipLaunchKernelGGL(k_sbm_to32f, dim3(divUp(W, 256), H, nframes), dim3(256), 0, st, dFrames, W, H);
    MI355_CHECK_LAUNCH(entry);
    return stg.finish(entry);
}

} // namespace

extern "C" {

// Host-resident frames are staged (HOST_HEAVY): numDisparities x blockSize^2 byte differences per pixel on the host against 4 bytes per pixel over PCIe.
MI355CV_API int mi355cv_stereoBM(const uchar* left, size_t left_step, const uchar* right, size_t right_step, uchar* disp, size_t disp_step, int width, int height, int disp_depth,
                                 const mi355cv_StereoBMParams* params)
{
    mi355::EntryGuard entry_(__func__);
    const HostFrame h{left, right, disp};
    return runStereo("stereoBM", &h, 1, left_step, right_step, disp_step, width, height, disp_depth, params);
}

// Host-resident batches are staged whole, frame by frame, through the Stager: the pipeline of runHostBatch carries one source per frame, a stereo frame has two.
MI355CV_API int mi355cv_stereoBMBatch(const uchar* left, size_t left_step, size_t left_frame_stride, const uchar* right, size_t right_step, size_t right_frame_stride, uchar* disp,
                                      size_t disp_step, size_t disp_frame_stride, int nframes, int width, int height, int disp_depth, const mi355cv_StereoBMParams* params)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !left || !right || !disp);
    MI355_DECLINE_IF(nframes < 1 || nframes > 65535);
    MI355_DECLINE_IF(width < 1 || height < 1);
    const size_t esz = disp_depth == MI355CV_32F ? 4 : 2;
    MI355_DECLINE_IF(left_step < (size_t)width || right_step < (size_t)width || disp_step < (size_t)width * esz);
    if (nframes > 1) {
        MI355_DECLINE_IF(left_frame_stride < span(left_step, height, width) || right_frame_stride < span(right_step, height, width));
        MI355_DECLINE_IF(disp_frame_stride < span(disp_step, height, (size_t)width * esz) || (disp_frame_stride & (esz - 1)));
    }
    std::vector<HostFrame> hf(nframes);
    for (int f = 0; f < nframes; f++) hf[f] = HostFrame{left + (size_t)f * left_frame_stride, right + (size_t)f * right_frame_stride, disp + (size_t)f * disp_frame_stride};
    return runStereo("stereoBMBatch", hf.data(), nframes, left_step, right_step, disp_step, width, height, disp_depth, params);
}

// the stage entry: the XSOBEL prefilter of one CV_8UC1 image
MI355CV_API int mi355cv_stereoPrefilterXSobel(const uchar* src, size_t src_step, uchar* dst, size_t dst_step, int width, int height, int cap)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !src || !dst);
    MI355_DECLINE_IF(width < 1 || height < 1 || width > lim::STEREOBM_MAX_DIM || height > lim::STEREOBM_MAX_DIM);
    MI355_DECLINE_IF(cap < 1 || cap > 63);
    MI355_DECLINE_IF(src_step < (size_t)width || dst_step < (size_t)width);
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)width * height, minPixels(HOST_HEAVY)));
    MI355_DECLINE_IF(overlapOnDevice(src, span(src_step, height, width), dst, span(dst_step, height, width)));
    size_t ss, ds;
    const uchar* s = stg.in(src, src_step, (size_t)width, height, &ss);
    uchar* d = stg.out(dst, dst_step, (size_t)width, height, &ds);
    MI355_DECLINE_IF(!s || !d);
    // whole groups of 16 may only be stored where the destination has them: a row of a wider image does not
    launchPrefilter(s, ss, 0, d, ds, 0, nullptr, 0, width, height, cap, 1, !(((size_t)s | ss) & 15), false, stream());
    MI355_CHECK_LAUNCH("stereoPrefilterXSobel");
    noteKernel("k_sbm_prefilter grid=%dx%d x256, cap %d", divUp(divUp(width, 16), 64), divUp(height, 4), cap);
    return stg.finish("stereoPrefilterXSobel");
}

MI355CV_API void mi355cv_stereoBMDefaults(mi355cv_StereoBMParams* p)
{
    if (!p) return;
    *p = mi355cv_StereoBMParams{};
    p->numDisparities = 64; p->blockSize = 21; p->preFilterType = sbm::PREFILTER_XSOBEL; p->preFilterSize = 9; p->preFilterCap = 31; p->textureThreshold = 10;
    p->uniquenessRatio = 15; p->disp12MaxDiff = -1;
}

MI355CV_API int mi355cv_stereoBMSetKernel(int mode)
{
    if (mode < -1 || mode > 0) return MI355CV_ERROR_UNKNOWN;
    g_kernelMode.store(mode, std::memory_order_relaxed);
    return MI355CV_OK;
}

} // extern "C"
