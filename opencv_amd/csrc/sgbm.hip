// sgbm.hip -- cv::StereoSGBM on the GPU: the replicated-row prefilter, Birchfield-Tomasi pixel costs on two planes, w x w block costs, 4 / 5 / 8 path aggregations, the
// decision with uniqueness and sub-pixel step, the left-right check, the speckle filter (the served mi355cv_filterSpecklesBatch, in place), CV_16S and CV_32F maps,
// single pairs and batches.  The definition is the project's own restatement (tests/sgbm_restate.py); the pieces are in sgbm_math.h, compiled for the
// host by tests/hostemu/sgbm_emu.cpp.  All arithmetic is integer: the maps are held bit for bit.
//
//   k_sgbm_prefilter    both images of every frame into dense planes
//   k_sgbm_fill         FILTERED into the columns outside [xlo, xhi)
//   k_sgbm_cost         the 16-bit volume C[y][x][k]: a workgroup of n / 16 waves owns TILE window columns and walks down STRIP rows.  Wave c, lane l keeps the
//                       vertical sums of window column l for the 16 disparity indices of chunk c in registers, adds the entering row's pixel costs and takes off the
//                       leaving row's (both rows staged in LDS as packed Birchfield-Tomasi triples), hands the sums over in LDS, where the w columns of a window are added
//   k_sgbm_path_plain   one direction, the A/B baseline: a workgroup per path, a lane per k, the previous pixel's L and its minimum through LDS
//   k_sgbm_path_fast    one direction: LP lanes across k with V values each per path (16 x 1, 32 x 1, 64 x 1, 64 x 2, 64 x 4), 64 / LP paths per wave; k +- 1 by
//                       DPP wave shifts, the minimum by DPP row operations and the rows' first lanes; the C vectors of the next block of steps and the S vectors of
//                       S vectors are loaded a block of steps ahead of the dependent chain, which then runs over registers
//   k_sgbm_decide       16 lanes per pixel over S: winner, uniqueness, sub-pixel value
//   k_sgbm_lr_vote / k_sgbm_lr_apply   the left-right check: one 64-bit atomicMin per kept pixel into its target column, then the reject
//   k_sgbm_store        the dense CV_16S map into the destination, as CV_16S or CV_32F (exact)
// S is 32 bit: the directions are separate launches on one stream, the first stores, the others read-modify-write.  A batch is one sequence of launches per chunk of
// frames whose volumes fit the scratch bound: the frame is the grid's z.
#include "rt.h"
#include "sgbm_math.h"
#include <algorithm>
#include <atomic>
#include <vector>

namespace {
using namespace mi355;
using sgbm::Geom;

static_assert(sgbm::MAX_DISPARITIES == lim::SGBM_MAX_DISPARITIES && sgbm::MAX_DIM == lim::SGBM_MAX_DIM && sgbm::MAX_COST == lim::SGBM_MAX_COST && sgbm::TILE == lim::SGBM_TILE_COLS &&
              sgbm::STRIP == lim::SGBM_STRIP_ROWS && sgbm::CHUNK == lim::SGBM_CHUNK && sgbm::PATH_BLOCK == lim::SGBM_PATH_BLOCK &&
              (long long)sgbm::MAX_SCRATCH_MIB << 20 == lim::SGBM_MAX_SCRATCH_BYTES, "mi355cv_limit(\"sgbm_*\")");
static_assert(sgbm::MAX_DISPARITIES / sgbm::CHUNK * 64 <= 1024 && sgbm::TILE == 64 && sgbm::CHUNK == 16, "a wave per chunk, a lane per window column");
static_assert(8 * sgbm::MAX_COST < (1 << 24), "S and k in one 32-bit key");

// one frame of a call: the two images, the CV_16S map the decision writes (the destination itself or scratch) and the destination
struct Frame { const uchar* l; size_t ls; const uchar* r; size_t rs; uchar* d16; size_t d16s; uchar* out; size_t outs; };
// the scratch of a chunk of frames: prefiltered planes, the volumes (vframe elements per frame), the winners and the left-right keys (cframe = W * H per frame)
struct Vol { uchar* gl; uchar* gr; size_t pstep, pframe; uint16_t* C; uint32_t* S; size_t vframe; uint32_t* win; unsigned long long* keys; size_t cframe; };

// ------------------------------------------------------------------------------------------------------------------------------------ prefilter, fill
__global__ __launch_bounds__(256) void k_sgbm_prefilter(const Frame* __restrict__ frames, int which, uchar* __restrict__ dst0, size_t dstep, size_t dframe, int W, int H, int ft)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const Frame F = frames[blockIdx.z];
    const uchar* src = which ? F.r : F.l;
    const size_t sstep = which ? F.rs : F.ls;
    const uchar* rm = src + (size_t)max(y - 1, 0) * sstep;
    const uchar* r0 = src + (size_t)y * sstep;
    const uchar* rp = src + (size_t)min(y + 1, H - 1) * sstep;
    dst0[(size_t)blockIdx.z * dframe + (size_t)y * dstep + x] = sgbm::prefilterPixel(rm, r0, rp, x, W, ft);
}

__global__ __launch_bounds__(256) void k_sgbm_fill(const Frame* __restrict__ frames, int W, int H, Geom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W || (x >= g.xlo && x < g.xhi)) return;
    const Frame F = frames[blockIdx.z];
    *(short*)(F.d16 + (size_t)y * F.d16s + (size_t)x * 2) = (short)g.filtered;
}

// ------------------------------------------------------------------------------------------------------------------------------------ the cost volume
constexpr int CT = sgbm::TILE, CC = sgbm::CHUNK;

// a staged row, packed triples: [0, 64) the left pixels of the tile's window columns, [64, 64 + nR) the right pixels rb .. rb + nR - 1; the prefiltered plane first, then,
// rowWords / 2 further on, the raw one
__device__ __forceinline__ void stageRow(uint32_t* buf, int half, const uchar* __restrict__ gl, const uchar* __restrict__ gr, const uchar* __restrict__ il,
                                         const uchar* __restrict__ ir, int u0, int xlo, int W1, int rb, int nR, int W, int t, int nthreads)
{
#pragma unroll 1
    for (int j0 = 0; j0 < CT + nR; j0 += nthreads) {
        const int j = j0 + t;
        if (j >= CT + nR) continue;
        const bool left = j < CT;
        const int col = left ? xlo + sgbm::clampi(u0 + j, 0, W1 - 1) : rb + (j - CT);
        buf[j] = sgbm::btPackAt(left ? gl : gr, col, W);
        buf[half + j] = sgbm::btPackAt(left ? il : ir, col, W);
    }
}

// dynamic LDS: rowbuf[2][2][64 + 64 + n] words | Vs[64][n + 2] u16
__global__ __launch_bounds__(1024) void k_sgbm_cost(const Frame* __restrict__ frames, Vol V, int W, int H, Geom g, int w)
{
    extern __shared__ __attribute__((aligned(16))) uchar smem[];
    const int h = w >> 1, n = g.n, SV = n + 2, TW = CT - 2 * h, nthreads = blockDim.x, W1 = g.W1;
    const int half = CT + CT + n, rowWords = 2 * half;
    uint32_t* rowbuf = (uint32_t*)smem;
    uint16_t* Vs = (uint16_t*)(rowbuf + 2 * rowWords);
    const int t = threadIdx.x, l = t & 63, c = t >> 6;
    const int x0 = blockIdx.x * TW, u0 = x0 - h, y0 = blockIdx.y * sgbm::STRIP, y1 = min(H, y0 + sgbm::STRIP);
    const int npix = min(TW, W1 - x0);
    const Frame F = frames[blockIdx.z];
    const uchar* gl = V.gl + (size_t)blockIdx.z * V.pframe;
    const uchar* gr = V.gr + (size_t)blockIdx.z * V.pframe;
    // the window columns of the tile, clamped into the valid range, are ucmin .. ucmax; the right pixels they meet are image columns rb .. rb + nR - 1, all inside the image
    const int ucmin = sgbm::clampi(u0, 0, W1 - 1), ucmax = sgbm::clampi(u0 + CT - 1, 0, W1 - 1);
    const int rb = g.xlo + ucmin - g.Dmax, nR = ucmax - ucmin + n;
    // index k = 16 c + j of lane l meets right pixel X - (k + m) = rb + (uc - ucmin) + (n - 1 - k)
    const int ridx = CT + (sgbm::clampi(u0 + l, 0, W1 - 1) - ucmin) + (n - 1 - CC * c);
    int Vsum[CC];
#pragma unroll
    for (int j = 0; j < CC; j++) Vsum[j] = 0;

#define SGBM_STAGE(buf, row) stageRow(buf, half, gl + (size_t)(row) * V.pstep, gr + (size_t)(row) * V.pstep, F.l + (size_t)(row) * F.ls, F.r + (size_t)(row) * F.rs, u0, g.xlo, \
                                      W1, rb, nR, W, t, nthreads)
    // the window's rows of the strip's first pixel row
#pragma unroll 1
    for (int r = 0; r < w; r++) {
        __syncthreads();
        SGBM_STAGE(rowbuf, sgbm::clampi(y0 - h + r, 0, H - 1));
        __syncthreads();
        const uint32_t a = rowbuf[l], b = rowbuf[half + l];
#pragma unroll
        for (int j = 0; j < CC; j++) Vsum[j] += sgbm::pixelCost(a, rowbuf[ridx - j], b, rowbuf[half + ridx - j]);
    }

#pragma unroll 1
    for (int y = y0; y < y1; y++) {
        if (y > y0) {
            // row y + h enters, row y - 1 - h leaves (the row buffers were last read before the barrier that follows the sums' hand-over of the row above)
            SGBM_STAGE(rowbuf, sgbm::clampi(y + h, 0, H - 1));
            SGBM_STAGE(rowbuf + rowWords, sgbm::clampi(y - 1 - h, 0, H - 1));
            __syncthreads();
            const uint32_t* lv = rowbuf + rowWords;
            const uint32_t ae = rowbuf[l], be = rowbuf[half + l], al = lv[l], bl = lv[half + l];
#pragma unroll
            for (int j = 0; j < CC; j++)
                Vsum[j] += sgbm::pixelCost(ae, rowbuf[ridx - j], be, rowbuf[half + ridx - j]) - sgbm::pixelCost(al, lv[ridx - j], bl, lv[half + ridx - j]);
        }
        {
            uint32_t* row = (uint32_t*)(Vs + l * SV + CC * c);
#pragma unroll
            for (int j = 0; j < CC; j += 2) row[j >> 1] = (uint32_t)Vsum[j] | ((uint32_t)Vsum[j + 1] << 16);
        }
        __syncthreads();
        if (l < npix) {
            uint32_t s[CC / 2];
#pragma unroll
            for (int j = 0; j < CC / 2; j++) s[j] = 0;
#pragma unroll 1
            for (int dx = 0; dx < w; dx++) {
                const uint32_t* row = (const uint32_t*)(Vs + (l + dx) * SV + CC * c);
#pragma unroll
                for (int j = 0; j < CC / 2; j++) s[j] += row[j];           // two 16-bit sums per word: a block cost fits 16 bits, so no carry crosses
            }
            uint4* out = (uint4*)(V.C + (size_t)blockIdx.z * V.vframe + ((size_t)y * W1 + (x0 + l)) * n + CC * c);
            out[0] = make_uint4(s[0], s[1], s[2], s[3]);
            out[1] = make_uint4(s[4], s[5], s[6], s[7]);
        }
        __syncthreads();
    }
#undef SGBM_STAGE
}

// ------------------------------------------------------------------------------------------------------------------------------------ paths
struct PathArgs { int ry, rx, W1, H, n, P1, P2, first, npaths; };

// the A/B baseline.  A workgroup of n lanes per path
__global__ __launch_bounds__(256) void k_sgbm_path_plain(Vol V, PathArgs A)
{
    __shared__ int prev[sgbm::MAX_DISPARITIES + 2], red[sgbm::MAX_DISPARITIES];
    const int k = threadIdx.x, n = A.n;
    const sgbm::Path P = sgbm::pathOf(A.ry, A.rx, A.W1, A.H, blockIdx.x);
    const uint16_t* C = V.C + (size_t)blockIdx.z * V.vframe;
    uint32_t* S = V.S + (size_t)blockIdx.z * V.vframe;
    if (k == 0) { prev[0] = sgbm::BIG; prev[n + 1] = sgbm::BIG; }
    long long p = P.p0;
    for (int t = 0; t < P.count; t++, p += P.dp) {
        const size_t at = (size_t)p * n + k;
        const int c = C[at];
        const int L = t ? sgbm::pathStep(c, prev[k + 1], prev[k], prev[k + 2], red[0], A.P1, A.P2) : c;
        __syncthreads();
        prev[k + 1] = L; red[k] = L;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (k < s && k + s < n) red[k] = min(red[k], red[k + s]);
            __syncthreads();
        }
        S[at] = A.first ? (uint32_t)L : S[at] + (uint32_t)L;
    }
}

template <int V> struct Vec;
template <> struct Vec<1> { typedef uint16_t C; typedef uint32_t S; };
template <> struct Vec<2> { typedef uint32_t C; typedef uint2 S; };
template <> struct Vec<4> { typedef uint2 C; typedef uint4 S; };

template <int V> __device__ __forceinline__ void loadC(const uint16_t* p, int* c)
{
    const typename Vec<V>::C v = *(const typename Vec<V>::C*)p;
    if constexpr (V == 1) c[0] = v;
    if constexpr (V == 2) { c[0] = v & 0xffffu; c[1] = v >> 16; }
    if constexpr (V == 4) { c[0] = v.x & 0xffffu; c[1] = v.x >> 16; c[2] = v.y & 0xffffu; c[3] = v.y >> 16; }
}
template <int V> __device__ __forceinline__ void loadS(const uint32_t* p, uint32_t* s)
{
    const typename Vec<V>::S v = *(const typename Vec<V>::S*)p;
    if constexpr (V == 1) s[0] = v;
    if constexpr (V == 2) { s[0] = v.x; s[1] = v.y; }
    if constexpr (V == 4) { s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w; }
}
template <int V> __device__ __forceinline__ void storeS(uint32_t* p, const uint32_t* s)
{
    if constexpr (V == 1) *p = s[0];
    if constexpr (V == 2) *(uint2*)p = make_uint2(s[0], s[1]);
    if constexpr (V == 4) *(uint4*)p = make_uint4(s[0], s[1], s[2], s[3]);
}

// the minimum over the LP lanes of a path: inside a row of 16 lanes by DPP (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror); two rows by
// __shfl_xor; a whole wave from the four rows' first lanes, which makes it a scalar
template <int LP> __device__ __forceinline__ int groupMin(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));
    if constexpr (LP == 32) v = min(v, __shfl_xor(v, 16, 64));
    if constexpr (LP == 64)
        v = min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
    return v;
}
// the value of the lane below / above (DPP wave_shr:1 / wave_shl:1); the wave's first / last lane gets `none`
__device__ __forceinline__ int fromLaneBelow(int v, int none) { return __builtin_amdgcn_update_dpp(none, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int fromLaneAbove(int v, int none) { return __builtin_amdgcn_update_dpp(none, v, 0x130, 0xf, 0xf, false); }

// LP lanes x V values across k, 64 / LP paths per wave, four waves per workgroup; PF steps per block
template <int LP, int V, int PF>
__global__ __launch_bounds__(256) void k_sgbm_path_fast(Vol Vl, PathArgs A)
{
    const int lane = threadIdx.x & 63, sub = lane & (LP - 1), n = A.n;
    const int path = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / LP) + lane / LP;
    const bool kact = sub * V < n;                                  // n is a multiple of 16 and V divides 16: a lane is inside the range with all its values or with none
    sgbm::Path P{0, 0, 0};
    if (path < A.npaths) P = sgbm::pathOf(A.ry, A.rx, A.W1, A.H, path);
    const int cnt = P.count;
    if (cnt == 0) return;                                           // a whole group of LP lanes leaves together
    const size_t base = (size_t)blockIdx.z * Vl.vframe + (size_t)P.p0 * n + (kact ? sub * V : 0);
    const long long stride = P.dp * n;
    const uint16_t* Cp = Vl.C + base;
    uint32_t* Sp = Vl.S + base;
    int Lp[V], cc[PF][V], cn[PF][V];
    uint32_t sc[PF][V], sn[PF][V];
#pragma unroll
    for (int j = 0; j < V; j++) Lp[j] = sgbm::BIG;
    // loads past the end of the path re-read its last pixel: no branch splits a block's loads.  The S vectors of a block are read a block ahead like the C vectors: a
    // path's pixels are its own, nothing else writes them meanwhile
#pragma unroll
    for (int i = 0; i < PF; i++) {
        loadC<V>(Cp + (long long)min(i, cnt - 1) * stride, cc[i]);
        if (!A.first) loadS<V>(Sp + (long long)min(i, cnt - 1) * stride, sc[i]);
        else {
#pragma unroll
            for (int j = 0; j < V; j++) sc[i][j] = sn[i][j] = 0;
        }
    }
#pragma unroll 1
    for (int t0 = 0; t0 < cnt; t0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; i++) {
            loadC<V>(Cp + (long long)min(t0 + PF + i, cnt - 1) * stride, cn[i]);
            if (!A.first) loadS<V>(Sp + (long long)min(t0 + PF + i, cnt - 1) * stride, sn[i]);
        }
#pragma unroll
        for (int i = 0; i < PF; i++) {
            if (t0 + i < cnt) {
                int L[V];
                if (t0 + i == 0) {
#pragma unroll
                    for (int j = 0; j < V; j++) L[j] = cc[i][j];
                } else {
                    int mloc = Lp[0];
#pragma unroll
                    for (int j = 1; j < V; j++) mloc = min(mloc, Lp[j]);
                    const int M = groupMin<LP>(mloc);
                    int dnEdge = fromLaneBelow(Lp[V - 1], sgbm::BIG), upEdge = fromLaneAbove(Lp[0], sgbm::BIG);
                    if (sub == 0) dnEdge = sgbm::BIG;
                    if (sub == LP - 1) upEdge = sgbm::BIG;
#pragma unroll
                    for (int j = 0; j < V; j++) L[j] = sgbm::pathStep(cc[i][j], Lp[j], j ? Lp[j - 1] : dnEdge, j < V - 1 ? Lp[j + 1] : upEdge, M, A.P1, A.P2);
                }
#pragma unroll
                for (int j = 0; j < V; j++) { Lp[j] = kact ? L[j] : sgbm::BIG; sc[i][j] += (uint32_t)L[j]; }
                if (kact) storeS<V>(Sp + (long long)(t0 + i) * stride, sc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < PF; i++)
#pragma unroll
            for (int j = 0; j < V; j++) { cc[i][j] = cn[i][j]; sc[i][j] = sn[i][j]; }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ decision, left-right check, store
// 16 lanes per pixel, 16 pixels per workgroup.  Lane `sub` holds k = 64 i + 4 sub + j, i < 4, j < 4, in registers: a group reads 256 contiguous bytes of S per load
__global__ __launch_bounds__(256) void k_sgbm_decide(const Frame* __restrict__ frames, Vol V, int W, int H, Geom g, int uniquenessRatio)
{
    const int sub = threadIdx.x & 15, n = g.n;
    const size_t pix = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (pix >= (size_t)g.W1 * H) return;
    const uint32_t* S = V.S + (size_t)blockIdx.z * V.vframe + pix * n;
    uint32_t v[4][4];
    uint32_t key = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k0 = 64 * i + 4 * sub;
        if (k0 < n) {
            const uint4 q = *(const uint4*)(S + k0);
            v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
#pragma unroll
            for (int j = 0; j < 4; j++) key = min(key, sgbm::minKey(v[i][j], k0 + j));
        }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 16));
    const int ms = sgbm::keyCost(key), best = sgbm::keyIndex(key);
    int bad = 0;
    if (uniquenessRatio > 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k0 = 64 * i + 4 * sub;
            if (k0 < n) {
#pragma unroll
                for (int j = 0; j < 4; j++) bad |= sgbm::uniqFails((int)v[i][j], k0 + j, best, ms, uniquenessRatio) ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 16);
    }
    if (sub) return;
    const int y = (int)(pix / g.W1), X = g.xlo + (int)(pix % g.W1);
    const Frame F = frames[blockIdx.z];
    int d = g.filtered;
    if (!bad) d = sgbm::disparity16(best, ms, best > 0 ? (int)S[best - 1] : 0, best < n - 1 ? (int)S[best + 1] : 0, n, g.m);
    *(short*)(F.d16 + (size_t)y * F.d16s + (size_t)X * 2) = (short)d;
    V.win[(size_t)blockIdx.z * V.cframe + (size_t)y * W + X] = bad ? sgbm::NOT_KEPT : sgbm::winOf(ms, best);
}

__global__ __launch_bounds__(256) void k_sgbm_lr_vote(Vol V, int W, int H, Geom g)
{
    const int X = g.xlo + blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (X >= g.xhi) return;
    const size_t rowOff = (size_t)blockIdx.z * V.cframe + (size_t)y * W;
    const uint32_t win = V.win[rowOff + X];
    if (win == sgbm::NOT_KEPT) return;
    const int best = sgbm::keyIndex(win), x2 = X - (best + g.m);
    if (x2 < 0 || x2 >= W) return;
    atomicMin(V.keys + rowOff + x2, sgbm::lrKey(sgbm::keyCost(win), X, best));
}

__global__ __launch_bounds__(256) void k_sgbm_lr_apply(const Frame* __restrict__ frames, Vol V, int W, int H, Geom g, int disp12MaxDiff)
{
    const int X = g.xlo + blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (X >= g.xhi) return;
    const size_t rowOff = (size_t)blockIdx.z * V.cframe + (size_t)y * W;
    if (V.win[rowOff + X] == sgbm::NOT_KEPT) return;
    const Frame F = frames[blockIdx.z];
    short* dp = (short*)(F.d16 + (size_t)y * F.d16s + (size_t)X * 2);
    const unsigned long long* keys = V.keys + rowOff;
    const int m = g.m;
    if (sgbm::lrRejects([keys, m](int xk) { return sgbm::lrDisp(keys[xk], m); }, X, *dp, W, m, disp12MaxDiff)) *dp = (short)g.filtered;
}

__global__ __launch_bounds__(256) void k_sgbm_store(const Frame* __restrict__ frames, int W, int H, int to32f)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const Frame F = frames[blockIdx.z];
    const short v = *(const short*)(F.d16 + (size_t)y * F.d16s + (size_t)x * 2);
    if (to32f) *(float*)(F.out + (size_t)y * F.outs + (size_t)x * 4) = (float)v * 0.0625f;
    else *(short*)(F.out + (size_t)y * F.outs + (size_t)x * 2) = v;
}

// ------------------------------------------------------------------------------------------------------------------------------------ host side
std::atomic<int> g_kernelMode{-1};                  // mi355cv_stereoSGBMSetKernel: -1 the rule (the fast path kernel), 0 always the plain one, 1 always the fast one
std::atomic<unsigned long long> g_scratchLimit{0};  // mi355cv_stereoSGBMSetScratchLimit: 0 = lim::SGBM_MAX_SCRATCH_BYTES

struct Args { int m, n, w, P1, P2, lr, ft, uniq, spw, spr, mode; };

// refusals that need no device
int checkParams(const mi355cv_StereoSGBMParams* p, int width, int height, int disp_depth, Args* A)
{
    MI355_DECLINE_IF(disabled() || !p);
    MI355_DECLINE_IF(width < 1 || height < 1 || width > lim::SGBM_MAX_DIM || height > lim::SGBM_MAX_DIM);
    if (disp_depth != MI355CV_16S && disp_depth != MI355CV_32F) return MI355_DECLINED("the disparity map is neither CV_16SC1 nor CV_32FC1");
    if (p->mode == sgbm::MODE_SGBM_3WAY) return MI355_DECLINED("MODE_SGBM_3WAY is not served");
    if (p->mode != sgbm::MODE_SGBM && p->mode != sgbm::MODE_HH && p->mode != sgbm::MODE_HH4) return MI355_DECLINED("mode is none of MODE_SGBM, MODE_HH, MODE_HH4");
    const int n = p->numDisparities, w = p->blockSize;
    MI355_DECLINE_IF(n < 16 || n % 16 != 0 || n > lim::SGBM_MAX_DISPARITIES);
    MI355_DECLINE_IF(w < 1 || w % 2 == 0);
    MI355_DECLINE_IF(p->preFilterCap < 0);
    MI355_DECLINE_IF(p->P1 < 0 || p->P2 < p->P1);
    MI355_DECLINE_IF(p->uniquenessRatio < 0 || p->uniquenessRatio > 100);
    MI355_DECLINE_IF(p->speckleWindowSize < 0 || p->speckleRange < 0);
    const int ft = sgbm::ftOf(p->preFilterCap > 65535 ? 65535 : p->preFilterCap);
    if (w > 181 || sgbm::costBound(w, ft, p->P2) > lim::SGBM_MAX_COST)
        return MI355_DECLINED("blockSize^2 * (2 ft + 63) + P2 > SGBM_MAX_COST = 32767, ft = max(preFilterCap, 15) | 1: a block cost or a path cost would leave 16 bits");
    // the CV_16S map holds 16 D + 8 at most and (m - 1) * 16 at least
    if (p->minDisparity < -2047 || (long long)p->minDisparity + n - 1 > 2046) return MI355_DECLINED("minDisparity .. minDisparity + numDisparities - 1 leaves the range of a CV_16S map (-2047 .. 2046)");
    *A = Args{p->minDisparity, n, w, p->P1, p->P2, p->disp12MaxDiff, ft, p->uniquenessRatio, p->speckleWindowSize, p->speckleRange, p->mode};
    return MI355CV_OK;
}

template <int LP, int V, int PF> void launchFast(const Vol& V_, const PathArgs& A, int nf, hipStream_t st)
{
    const int perBlock = 4 * (64 / LP);
    hipLaunchKernelGGL((k_sgbm_path_fast<LP, V, PF>), dim3(divUp(A.npaths, perBlock), 1, nf), dim3(256), 0, st, V_, A);
}

void launchPaths(const Vol& V, const Args& A, const Geom& g, int H, int nf, bool fast, hipStream_t st)
{
    for (int i = 0; i < sgbm::dirCount(A.mode); i++) {
        PathArgs P{0, 0, g.W1, H, A.n, A.P1, A.P2, i == 0, 0};
        sgbm::dirOf(A.mode, i, &P.ry, &P.rx);
        P.npaths = sgbm::pathCount(P.ry, P.rx, g.W1, H);
        if (!fast) hipLaunchKernelGGL(k_sgbm_path_plain, dim3(P.npaths, 1, nf), dim3(A.n), 0, st, V, P);
        else if (A.n == 16) launchFast<16, 1, sgbm::PATH_BLOCK>(V, P, nf, st);
        else if (A.n == 32) launchFast<32, 1, sgbm::PATH_BLOCK>(V, P, nf, st);
        else if (A.n <= 64) launchFast<64, 1, sgbm::PATH_BLOCK>(V, P, nf, st);
        else if (A.n <= 128) launchFast<64, 2, sgbm::PATH_BLOCK / 2>(V, P, nf, st);
        else launchFast<64, 4, sgbm::PATH_BLOCK / 4>(V, P, nf, st);
    }
}

struct HostFrame { const uchar* l; const uchar* r; uchar* d; };

int runSgbm(const char* entry, const HostFrame* hf, int nframes, size_t lstep, size_t rstep, size_t dstep, int W, int H, int depth, const mi355cv_StereoSGBMParams* params)
{
    Args A;
    if (const int rc = checkParams(params, W, H, depth, &A)) return rc;
    const size_t esz = depth == MI355CV_16S ? 2 : 4;
    MI355_DECLINE_IF(nframes < 1);
    MI355_DECLINE_IF(lstep < (size_t)W || rstep < (size_t)W || dstep < (size_t)W * esz);
    for (int f = 0; f < nframes; f++) {
        MI355_DECLINE_IF(!hf[f].l || !hf[f].r || !hf[f].d);
        if (((size_t)hf[f].d | dstep) & (esz - 1)) return MI355_DECLINED("disparity rows off their element's boundary");
    }
    const Geom g = sgbm::geomOf(W, A.m, A.n);
    const bool any = g.W1 > 0;
    const unsigned long long perFrame = sgbm::frameScratch(W, H, g.W1, A.n);
    unsigned long long bound = g_scratchLimit.load(std::memory_order_relaxed);
    if (!bound || bound > (unsigned long long)lim::SGBM_MAX_SCRATCH_BYTES) bound = (unsigned long long)lim::SGBM_MAX_SCRATCH_BYTES;
    if (perFrame > bound) return MI355_DECLINED("the volumes of one frame, 6 bytes per valid pixel and disparity, exceed SGBM_MAX_SCRATCH_BYTES");
    const int chunk = (int)std::min<unsigned long long>(std::min<unsigned long long>(bound / perFrame, (unsigned long long)MAX_GRID_FRAMES), (unsigned long long)nframes);
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(hf[0].l, (size_t)W * H, minPixels(HOST_HEAVY)));
    const size_t dspan = span(dstep, H, (size_t)W * esz);
    {
        // the frames of a batch lie at one stride: the stacks are judged by their hulls, first byte of the first frame to last byte of the last
        const int e = nframes - 1;
        const size_t lhull = (size_t)(hf[e].l - hf[0].l) + span(lstep, H, W), rhull = (size_t)(hf[e].r - hf[0].r) + span(rstep, H, W), dhull = (size_t)(hf[e].d - hf[0].d) + dspan;
        if (overlapOnDevice(hf[0].l, lhull, hf[0].d, dhull) || overlapOnDevice(hf[0].r, rhull, hf[0].d, dhull)) return MI355_DECLINED("the disparity map overlaps an input");
        if (nframes > 1 && overlapOnDevice(hf[0].d, dspan, hf[1].d, dspan)) return MI355_DECLINED("two disparity maps of the batch overlap");
    }
    Vol V{};
    V.pstep = ((size_t)W + 15) & ~(size_t)15;
    V.pframe = V.pstep * H;
    V.vframe = any ? (size_t)g.W1 * H * A.n : 0;
    V.cframe = (size_t)W * H;
    const bool dense = depth == MI355CV_32F || A.spw > 0;       // the decision writes a dense CV_16S map in scratch: the speckle filter works on it in place
    short* d16 = nullptr;
    const size_t d16step = (size_t)W * 2, d16frame = d16step * H;
    if (any) {
        V.gl = (uchar*)stg.scratch(V.pframe * chunk);
        V.gr = (uchar*)stg.scratch(V.pframe * chunk);
        V.C = (uint16_t*)stg.scratch(V.vframe * chunk * sizeof(uint16_t));
        V.S = (uint32_t*)stg.scratch(V.vframe * chunk * sizeof(uint32_t));
        V.win = (uint32_t*)stg.scratch(V.cframe * chunk * sizeof(uint32_t));
        V.keys = (unsigned long long*)stg.scratch(V.cframe * chunk * sizeof(unsigned long long));
        if (!V.gl || !V.gr || !V.C || !V.S || !V.win || !V.keys) return MI355_DECLINED("no scratch for the volumes");
    }
    if (dense) { d16 = (short*)stg.scratch(d16frame * chunk); if (!d16) return MI355_DECLINED("no scratch for the CV_16S map"); }
    std::vector<Frame> fr(nframes);
    for (int f = 0; f < nframes; f++) {
        Frame& F = fr[f];
        F.l = stg.in(hf[f].l, lstep, (size_t)W, H, &F.ls);
        F.r = stg.in(hf[f].r, rstep, (size_t)W, H, &F.rs);
        F.out = stg.out(hf[f].d, dstep, (size_t)W * esz, H, &F.outs);
        if (!F.l || !F.r || !F.out) return MI355_DECLINED("staging failed");
        if (dense) { F.d16 = (uchar*)d16 + d16frame * (f % chunk); F.d16s = d16step; } else { F.d16 = F.out; F.d16s = F.outs; }
    }
    const Frame* dFrames = (const Frame*)stg.param(fr.data(), fr.size() * sizeof(Frame));
    if (!dFrames) return MI355_DECLINED("no scratch");
    hipStream_t st = stream();
    const bool fast = g_kernelMode.load(std::memory_order_relaxed) != 0;
    const int TW = sgbm::TILE - 2 * (A.w / 2);
    const size_t lds = 2 * 2 * (size_t)(2 * sgbm::TILE + A.n) * sizeof(uint32_t) + (size_t)sgbm::TILE * (A.n + 2) * sizeof(uint16_t);
    for (int f0 = 0; f0 < nframes; f0 += chunk) {
        const int nf = std::min(chunk, nframes - f0);
        const Frame* cf = dFrames + f0;
        const dim3 pix(divUp(W, 256), H, nf);
        if (g.xlo > 0 || g.xhi < W) hipLaunchKernelGGL(k_sgbm_fill, pix, dim3(256), 0, st, cf, W, H, g);
        if (any) {
            hipLaunchKernelGGL(k_sgbm_prefilter, pix, dim3(256), 0, st, cf, 0, V.gl, V.pstep, V.pframe, W, H, A.ft);
            hipLaunchKernelGGL(k_sgbm_prefilter, pix, dim3(256), 0, st, cf, 1, V.gr, V.pstep, V.pframe, W, H, A.ft);
            const dim3 cgrid(divUp(g.W1, TW), divUp(H, sgbm::STRIP), nf);
            hipLaunchKernelGGL(k_sgbm_cost, cgrid, dim3(64 * (A.n / sgbm::CHUNK)), lds, st, cf, V, W, H, g, A.w);
            launchPaths(V, A, g, H, nf, fast, st);
            hipLaunchKernelGGL(k_sgbm_decide, dim3((unsigned)(((size_t)g.W1 * H + 15) / 16), 1, nf), dim3(256), 0, st, cf, V, W, H, g, A.uniq);
            if (hipMemsetAsync(V.keys, 0xff, V.cframe * nf * sizeof(unsigned long long), st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: memset failed", entry);
            const dim3 vgrid(divUp(g.W1, 256), H, nf);
            hipLaunchKernelGGL(k_sgbm_lr_vote, vgrid, dim3(256), 0, st, V, W, H, g);
            hipLaunchKernelGGL(k_sgbm_lr_apply, vgrid, dim3(256), 0, st, cf, V, W, H, g, A.lr);
            MI355_CHECK_LAUNCH(entry);
        }
        if (A.spw > 0) {
            // the served filter, in place on the dense map (a nested entry: same stream, same scratch pool, no synchronisation of its own)
            const long long maxDiff = 16ll * A.spr;
            const int rc = mi355cv_filterSpecklesBatch((uchar*)d16, d16step, d16frame, nf, W, H, MI355CV_16S, g.filtered, A.spw, maxDiff > 0x7fffffffll ? 0x7fffffff : (int)maxDiff);
            if (rc != MI355CV_OK) return rc;
        }
        if (dense) hipLaunchKernelGGL(k_sgbm_store, pix, dim3(256), 0, st, cf, W, H, depth == MI355CV_32F ? 1 : 0);
        MI355_CHECK_LAUNCH(entry);
    }
    // after the nested speckle entry, which names its own kernels
    if (any)
        noteKernel("%s n=%d mode=%d: %d direction(s), k_sgbm_cost grid=%dx%dx%d x%d lds=%zu w=%d, %d frame(s) per chunk%s", fast ? "k_sgbm_path_fast" : "k_sgbm_path_plain", A.n, A.mode,
                   sgbm::dirCount(A.mode), divUp(g.W1, TW), divUp(H, sgbm::STRIP), chunk, 64 * (A.n / sgbm::CHUNK), lds, A.w, chunk, A.spw > 0 ? ", mi355cv_filterSpecklesBatch" : "");
    else noteKernel("k_sgbm_fill grid=%dx%dx%d x256: no valid column", divUp(W, 256), H, chunk);
    return stg.finish(entry);
}

} // namespace

extern "C" {

// Host-resident frames are staged (HOST_HEAVY): the reference's aggregation is tens of milliseconds per frame on the host against 4 bytes per pixel over PCIe.
MI355CV_API int mi355cv_stereoSGBM(const uchar* left, size_t left_step, const uchar* right, size_t right_step, uchar* disp, size_t disp_step, int width, int height, int disp_depth,
                                   const mi355cv_StereoSGBMParams* params)
{
    mi355::EntryGuard entry_(__func__);
    const HostFrame h{left, right, disp};
    return runSgbm("stereoSGBM", &h, 1, left_step, right_step, disp_step, width, height, disp_depth, params);
}

// Host-resident batches are staged whole, frame by frame, through the Stager, as mi355cv_stereoBMBatch stages them.
MI355CV_API int mi355cv_stereoSGBMBatch(const uchar* left, size_t left_step, size_t left_frame_stride, const uchar* right, size_t right_step, size_t right_frame_stride, uchar* disp,
                                        size_t disp_step, size_t disp_frame_stride, int nframes, int width, int height, int disp_depth, const mi355cv_StereoSGBMParams* params)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !left || !right || !disp);
    MI355_DECLINE_IF(nframes < 1);
    MI355_DECLINE_IF(width < 1 || height < 1);
    const size_t esz = disp_depth == MI355CV_32F ? 4 : 2;
    MI355_DECLINE_IF(left_step < (size_t)width || right_step < (size_t)width || disp_step < (size_t)width * esz);
    if (nframes > 1) {
        MI355_DECLINE_IF(left_frame_stride < span(left_step, height, width) || right_frame_stride < span(right_step, height, width));
        MI355_DECLINE_IF(disp_frame_stride < span(disp_step, height, (size_t)width * esz) || (disp_frame_stride & (esz - 1)));
    }
    std::vector<HostFrame> hf(nframes);
    for (int f = 0; f < nframes; f++) hf[f] = HostFrame{left + (size_t)f * left_frame_stride, right + (size_t)f * right_frame_stride, disp + (size_t)f * disp_frame_stride};
    return runSgbm("stereoSGBMBatch", hf.data(), nframes, left_step, right_step, disp_step, width, height, disp_depth, params);
}

MI355CV_API void mi355cv_stereoSGBMDefaults(mi355cv_StereoSGBMParams* p)
{
    if (!p) return;
    *p = mi355cv_StereoSGBMParams{};
    p->numDisparities = 16; p->blockSize = 3; p->mode = sgbm::MODE_SGBM;
}

MI355CV_API int mi355cv_stereoSGBMSetKernel(int mode)
{
    if (mode < -1 || mode > 1) return MI355CV_ERROR_UNKNOWN;
    g_kernelMode.store(mode, std::memory_order_relaxed);
    return MI355CV_OK;
}

MI355CV_API int mi355cv_stereoSGBMSetScratchLimit(size_t bytes)
{
    g_scratchLimit.store((unsigned long long)bytes, std::memory_order_relaxed);
    return MI355CV_OK;
}

} // extern "C"
