// integral.hip -- cv::integral for 8-bit single-channel sources (cv_hal_integral, hal_replacement.hpp:977; sumpixels.simd.hpp) in two passes
// over the pixels instead of three passes over the 4-8x larger sum image.
//
//   S[y+1][x+1] = sum_{i<=y, j<=x} p[i][j],  row 0 and column 0 of S are zero.
//
// The image is cut into tiles of TH pixel rows x 256 S-columns; ONE WAVE owns a tile (a lane owns 4 consecutive S columns = one dword of
// pixels and one 16-byte store per row):
//   pass A  k_integral_tilesums  per tile: column sums of its pixels (one u32 per pixel column), row sums (one u32 per pixel row), total
//                                -> colsum[ty][x], rowsum[tx][y], tileTot[ty][tx]: (H/TH) x W + (W/256) x H words, ~2 MB for a 4K frame;
//   scan    k_integral_carries   exclusive scans of those along ty resp. tx, in place (W + H threads, <= H/TH resp. W/256 steps each), and
//                                the 2-D exclusive prefix of the tile totals (one workgroup, in LDS) = every tile's corner value;
//   pass B  k_integral_tiles     per tile: top edge = corner + prefix of its column carries, then row by row: lane-local prefix of 4 pixels
//                                + DPP wave scan + the row's carry, added into the running column accumulators, stored.
// Traffic: the pixels twice (the second time from L2 / Infinity Cache), the carries (~2 % of the output), the output once: within a few per
// cent of the compulsory 1 B read + 4 (8) B written per pixel, against ~4x that for the row pass + two column passes it replaces.
// All sums are exact integers (u32 partials, int32 / u64 accumulators); CV_64F outputs are those integers converted once, so they equal the
// reference's double sums bit for bit.
//
// Below the tiled kernels: the general scan (rows + column segments: any channel count, float sources; also the matcher's double sum and squared-sum
// images, integralSumSq) and the two hooks, mi355cv_integral and mi355cv_integralBatch.  The order-dependent outputs are integral_seq.hip's.
#include "rt.h"
#include "integral.h"

namespace mi355 {
namespace {

constexpr int ITH = 16;            // pixel rows per tile (a wave issues all of a tile's pixel loads before it consumes the first)
constexpr int ITW = 256;           // S columns per tile (64 lanes x 4)

typedef unsigned u32u __attribute__((aligned(1)));

// inclusive prefix sum over the 64 lanes of a wave (row_shr 1/2/4/8 inside each row of 16, then row_bcast 15 / 31 across rows)
__device__ __forceinline__ unsigned waveScanIncl(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ unsigned long long waveScanIncl64(unsigned long long v)
{
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long a = __shfl_up(v, o);
        if ((int)(threadIdx.x & 63) >= o) v += a;
    }
    return v;
}

// the 4 pixels of a lane: S columns c..c+3 of the tile use pixel columns c-1..c+2; `x` = c - 1 may be -1 (S column 0) and the dword may run past
// the row's end -- those bytes read as 0.  Interior lanes take one (possibly unaligned) dword load.
__device__ __forceinline__ unsigned loadPix4(const uchar* __restrict__ row, int x, int W)
{
    if (x >= 0 && x + 4 <= W) return *reinterpret_cast<const u32u*>(row + x);
    unsigned w = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) if (x + b >= 0 && x + b < W) w |= (unsigned)row[x + b] << (8 * b);
    return w;
}

// ---- pass A: tile sums.  colsum / colsq indexed [ty][pixel x] (pitch Wp), rowsum / rowsq indexed [tx][pixel y] (pitch H)
template <bool SQ>
__global__ __launch_bounds__(256) void k_integral_tilesums(const uchar* __restrict__ src, size_t sstep, size_t sframe, int W, int H, int nTx, int nTy, int nframes,
                                                           unsigned* __restrict__ colsum, unsigned* __restrict__ colsq, unsigned* __restrict__ rowsum,
                                                           unsigned* __restrict__ rowsq, unsigned* __restrict__ tileTot, unsigned* __restrict__ tileTotQ,
                                                           int Wp, size_t auxFrame)
{
    const int lane = threadIdx.x & 63;
    const int wid = (int)xcdContiguous(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6);     // neighbouring tiles (shared output lines) behind the same L2
    const int tx = wid % nTx, ty = (wid / nTx) % nTy, f = wid / (nTx * nTy);
    if (f >= nframes) return;
    src += (size_t)f * sframe;
    colsum += (size_t)f * auxFrame; rowsum += (size_t)f * auxFrame; tileTot += (size_t)f * auxFrame;
    if (SQ) { colsq += (size_t)f * auxFrame; rowsq += (size_t)f * auxFrame; tileTotQ += (size_t)f * auxFrame; }
    // aligned pixel strips here: pixel columns [256 tx, 256 tx + 256); the shift by one S column is pass B's business
    const int x = tx * ITW + 4 * lane, y0 = ty * ITH, y1 = min(H, y0 + ITH);
    unsigned cs[4] = {0, 0, 0, 0}, cq[4] = {0, 0, 0, 0};
    unsigned myRow = 0, myRowQ = 0;
    unsigned wv[ITH];
#pragma unroll
    for (int r = 0; r < ITH; r++) wv[r] = (x < W && y0 + r < y1) ? loadPix4(src + (size_t)(y0 + r) * sstep, x, W) : 0u;
#pragma unroll
    for (int r = 0; r < ITH; r++) {
        const unsigned w = wv[r];
        unsigned s = 0, q = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const unsigned p = (w >> (8 * b)) & 255u;
            cs[b] += p; s += p;
            if (SQ) { cq[b] += p * p; q += p * p; }
        }
        const unsigned rs = (unsigned)__builtin_amdgcn_readlane((int)waveScanIncl(s), 63);      // the row's sum over the strip
        if (lane == r) myRow = rs;
        if (SQ) {
            const unsigned rq = (unsigned)__builtin_amdgcn_readlane((int)waveScanIncl(q), 63);
            if (lane == r) myRowQ = rq;
        }
    }
    if (x < W) {
#pragma unroll
        for (int b = 0; b < 4; b++) if (x + b < W) {
            colsum[(size_t)ty * Wp + x + b] = cs[b];
            if (SQ) colsq[(size_t)ty * Wp + x + b] = cq[b];
        }
    }
    if (lane < y1 - y0) {
        rowsum[(size_t)tx * H + y0 + lane] = myRow;
        if (SQ) rowsq[(size_t)tx * H + y0 + lane] = myRowQ;
    }
    // the tile's total (lanes >= rows hold 0), for the 2-D prefix over tiles that gives every tile its corner value
    const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)waveScanIncl(myRow), 63);
    if (lane == 0) tileTot[(size_t)ty * nTx + tx] = tot;
    if (SQ) {
        const unsigned totq = (unsigned)__builtin_amdgcn_readlane((int)waveScanIncl(myRowQ), 63);
        if (lane == 0) tileTotQ[(size_t)ty * nTx + tx] = totq;
    }
}

// ---- scan: colsum[ty][x] -> sum over tiles above (exclusive, along ty); rowsum[tx][y] -> sum over strips to the left (exclusive, along tx)
__global__ __launch_bounds__(256) void k_integral_carries(const unsigned* __restrict__ colsum, const unsigned* __restrict__ colsq, const unsigned* __restrict__ rowsum,
                                                          const unsigned* __restrict__ rowsq, unsigned* __restrict__ colcar, unsigned* __restrict__ colcarQ,
                                                          unsigned* __restrict__ rowcar, unsigned* __restrict__ rowcarQ,
                                                          const unsigned* __restrict__ tileTot, const unsigned* __restrict__ tileTotQ,
                                                          unsigned long long* __restrict__ corner, unsigned long long* __restrict__ cornerQ,
                                                          int W, int H, int Wp, int nTx, int nTy, size_t auxFrame, int sq)
{
    const size_t fo = (size_t)blockIdx.z * auxFrame;
    const int which = blockIdx.y;                                   // 0: sums, 1: squares
    if (which && !sq) return;
    if (blockIdx.x == gridDim.x - 1) {
        // last block: corner[ty][tx] = sum of the totals of the tiles above-left (t < ty, s < tx), in LDS.  Along tx first (one thread per tile
        // row, <= 64 steps), then along ty -- the long direction -- in three short phases: 16 chunks per strip column are summed in parallel,
        // the 16 chunk sums are scanned, and every chunk rewrites its entries as exclusive prefixes.
        extern __shared__ unsigned long long tt[];                  // nTy x nTx, then 16 x nTx chunk sums
        const unsigned* src = (which ? tileTotQ : tileTot) + fo;
        unsigned long long* dst = (unsigned long long*)((char*)(which ? cornerQ : corner) + fo * 4);      // the corner arrays are 2 words per entry
        const int n = nTx * nTy;
        unsigned long long* cs = tt + n;
        for (int i = threadIdx.x; i < n; i += 256) tt[i] = src[i];
        __syncthreads();
        for (int t = threadIdx.x; t < nTy; t += 256) {               // exclusive prefix along tx
            unsigned long long run = 0;
            for (int sx = 0; sx < nTx; sx++) { const unsigned long long v = tt[t * nTx + sx]; tt[t * nTx + sx] = run; run += v; }
        }
        __syncthreads();
        const int per = (nTy + 15) / 16;                             // tile rows per chunk
        for (int i = threadIdx.x; i < 16 * nTx; i += 256) {
            const int k = i / nTx, sx = i - k * nTx;
            unsigned long long sum = 0;
            for (int t = k * per; t < min(nTy, (k + 1) * per); t++) sum += tt[t * nTx + sx];
            cs[i] = sum;
        }
        __syncthreads();
        for (int sx = threadIdx.x; sx < nTx; sx += 256) {
            unsigned long long run = 0;
            for (int k = 0; k < 16; k++) { const unsigned long long v = cs[k * nTx + sx]; cs[k * nTx + sx] = run; run += v; }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 16 * nTx; i += 256) {
            const int k = i / nTx, sx = i - k * nTx;
            unsigned long long run = cs[i];
            for (int t = k * per; t < min(nTy, (k + 1) * per); t++) { const unsigned long long v = tt[t * nTx + sx]; dst[t * nTx + sx] = run; run += v; }
        }
        return;
    }
    const unsigned* cs = (which ? colsq : colsum) + fo;
    const unsigned* rs = (which ? rowsq : rowsum) + fo;
    unsigned* co = (which ? colcarQ : colcar) + fo;
    unsigned* ro = (which ? rowcarQ : rowcar) + fo;
    const int colBlocks = (W + 31) / 32;
    if ((int)blockIdx.x < colBlocks) {
        // column carries: a workgroup takes 32 columns x 8 chunks of tile rows.  Every thread loads its chunk at once (one memory round trip for
        // the whole scan instead of nTy dependent ones in a handful of waves), the chunk sums are exchanged through LDS, and the exclusive
        // prefixes are written from the registers.
        __shared__ unsigned part[8][33];
        const int c = threadIdx.x & 31, ck = threadIdx.x >> 5, col = blockIdx.x * 32 + c;
        const int per = (nTy + 7) / 8, t0 = ck * per, t1 = min(nTy, t0 + per);
        unsigned v[32];
        unsigned sum = 0;
        if (per <= 32) {
#pragma unroll
            for (int u = 0; u < 32; u++) { v[u] = (col < W && t0 + u < t1) ? cs[(size_t)(t0 + u) * Wp + col] : 0u; sum += v[u]; }
        } else {
            for (int t = t0; t < t1; t++) if (col < W) sum += cs[(size_t)t * Wp + col];
        }
        part[ck][c] = sum;
        __syncthreads();
        unsigned run = 0;
        for (int k = 0; k < ck; k++) run += part[k][c];
        if (col < W) {
            if (per <= 32) {
#pragma unroll
                for (int u = 0; u < 32; u++) if (t0 + u < t1) { co[(size_t)(t0 + u) * Wp + col] = run; run += v[u]; }
            } else {
                for (int t = t0; t < t1; t++) { const unsigned x = cs[(size_t)t * Wp + col]; co[(size_t)t * Wp + col] = run; run += x; }
            }
        }
        return;
    }
    const int y = ((int)blockIdx.x - colBlocks) * 256 + threadIdx.x;
    if (y < H) {
        unsigned run = 0;
#pragma unroll 8
        for (int tx = 0; tx < nTx; tx++) { const unsigned x = rs[(size_t)tx * H + y]; ro[(size_t)tx * H + y] = run; run += x; }
    }
}

// ---- pass B.  TS = int (CV_32S sums, wrapping like the reference's int arithmetic) or double (exact integers accumulated in u64).
template <typename TS> struct Acc;
template <> struct Acc<int>    { typedef unsigned T; static __device__ __forceinline__ int    out(unsigned v) { return (int)v; } };
template <> struct Acc<double> { typedef unsigned long long T; static __device__ __forceinline__ double out(unsigned long long v) { return (double)v; } };

template <typename TS>
__device__ __forceinline__ void storeRow4(TS* __restrict__ drow, int c, int Wc, const typename Acc<TS>::T (&a)[4], bool nt = false)
{
    if (c + 4 <= Wc) {
        if (sizeof(TS) == 4) {
            typedef int i4u __attribute__((ext_vector_type(4), aligned(4)));
            i4u v; v.x = (int)a[0]; v.y = (int)a[1]; v.z = (int)a[2]; v.w = (int)a[3];
            if (nt) __builtin_nontemporal_store(v, reinterpret_cast<i4u*>(drow + c)); else *reinterpret_cast<i4u*>(drow + c) = v;
        } else {
            typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));
            d2u v0, v1; v0.x = (double)a[0]; v0.y = (double)a[1]; v1.x = (double)a[2]; v1.y = (double)a[3];
            *reinterpret_cast<d2u*>(drow + c) = v0; *reinterpret_cast<d2u*>(drow + c + 2) = v1;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) if (c + k < Wc) drow[c + k] = Acc<TS>::out(a[k]);
    }
}

template <typename TS, bool SQ>
__global__ __launch_bounds__(256) void k_integral_tiles(const uchar* __restrict__ src, size_t sstep, size_t sframe, int W, int H, int nTx, int nTy, int nframes,
                                                        TS* __restrict__ sum, size_t sumStep, size_t sumFrame, double* __restrict__ sq, size_t sqStep, size_t sqFrame,
                                                        const unsigned* __restrict__ colsum, const unsigned* __restrict__ colsq, const unsigned* __restrict__ rowsum,
                                                        const unsigned* __restrict__ rowsq, const unsigned long long* __restrict__ cornerArr,
                                                        const unsigned long long* __restrict__ cornerArrQ, int Wp, size_t auxFrame, int nt)
{
    typedef typename Acc<TS>::T A;
    const int lane = threadIdx.x & 63;
    const int wid = (int)xcdContiguous(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6);     // neighbouring tiles (shared output lines) behind the same L2
    const int tx = wid % nTx, ty = (wid / nTx) % nTy, f = wid / (nTx * nTy);
    if (f >= nframes) return;
    src += (size_t)f * sframe; sum += (size_t)f * sumFrame;
    colsum += (size_t)f * auxFrame; rowsum += (size_t)f * auxFrame;
    cornerArr = (const unsigned long long*)((const char*)cornerArr + (size_t)f * auxFrame * 4);
    if (SQ) { sq += (size_t)f * sqFrame; colsq += (size_t)f * auxFrame; rowsq += (size_t)f * auxFrame;
              cornerArrQ = (const unsigned long long*)((const char*)cornerArrQ + (size_t)f * auxFrame * 4); }
    const int Wc = W + 1;                                            // S columns
    const int X0 = tx * ITW, c = X0 + 4 * lane;                      // this lane's S columns c..c+3; its pixels are c-1..c+2
    const int y0 = ty * ITH, y1 = min(H, y0 + ITH);

    // ---- top edge of the tile: S[y0][cc] = sum of the column carries (sums of the tiles above) of the pixel columns j < cc, for cc = c..c+3
    A top[4]; unsigned long long topq[4] = {0, 0, 0, 0};
    {
        const unsigned* cc = colsum + (size_t)ty * Wp;
        const unsigned* cq = SQ ? colsq + (size_t)ty * Wp : nullptr;
        // corner = everything above-left of the tile: the 2-D prefix of the (aligned) tile totals covers the pixel columns < X0; the tile's own
        // first pixel column is X0 - 1, so its carry comes off again
        A corner = (A)cornerArr[(size_t)ty * nTx + tx];
        unsigned long long cornerq = SQ ? cornerArrQ[(size_t)ty * nTx + tx] : 0ull;
        if (X0 > 0) { corner -= (A)cc[X0 - 1]; if (SQ) cornerq -= cq[X0 - 1]; }
        // this lane's four carries: pixel columns c-1, c, c+1, c+2 (out of range -> 0); S column c+k takes k4[0..k]
        unsigned k4[4], q4[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = c - 1 + k;
            const bool in = j >= 0 && j < W;
            k4[k] = in ? cc[j] : 0u;
            q4[k] = (SQ && in) ? cq[j] : 0u;
        }
        A loc[4]; unsigned long long locq[4];
        loc[0] = k4[0]; loc[1] = loc[0] + k4[1]; loc[2] = loc[1] + k4[2]; loc[3] = loc[2] + k4[3];
        locq[0] = q4[0]; locq[1] = locq[0] + q4[1]; locq[2] = locq[1] + q4[2]; locq[3] = locq[2] + q4[3];
        A excl; unsigned long long exclq = 0;
        if (sizeof(A) == 4) excl = (A)(waveScanIncl((unsigned)loc[3]) - (unsigned)loc[3]);
        else excl = (A)(waveScanIncl64((unsigned long long)loc[3]) - (unsigned long long)loc[3]);
        if (SQ) exclq = waveScanIncl64(locq[3]) - locq[3];
#pragma unroll
        for (int k = 0; k < 4; k++) { top[k] = corner + excl + loc[k]; if (SQ) topq[k] = cornerq + exclq + locq[k]; }
    }
    // row 0 of S is zero: written by the first row of tiles
    if (ty == 0 && c < Wc) {
        const A z[4] = {0, 0, 0, 0};
        const unsigned long long zq[4] = {0, 0, 0, 0};
        storeRow4<TS>(sum, c, Wc, z);
        if (SQ) storeRow4<double>(sq, c, Wc, zq);
    }
    // the row carries of this tile's rows (sum of the pixels left of pixel column X0 -- aligned strips, see pass A): lane r holds row y0 + r
    const unsigned rcAll = lane < y1 - y0 ? rowsum[(size_t)tx * H + y0 + lane] : 0u;
    const unsigned rqAll = (SQ && lane < y1 - y0) ? rowsq[(size_t)tx * H + y0 + lane] : 0u;
    // pixels X0 + 4 lane .. + 3 (aligned strip) of every row of the tile, all loads in flight before the first is consumed
    const int x = X0 + 4 * lane;
    unsigned wv[ITH];
#pragma unroll
    for (int r = 0; r < ITH; r++) wv[r] = (x < W && y0 + r < y1) ? loadPix4(src + (size_t)(y0 + r) * sstep, x, W) : 0u;
#pragma unroll
    for (int r = 0; r < ITH; r++) {
        if (y0 + r >= y1) break;
        const int y = y0 + r;
        // shifted by one pixel: q = {previous lane's p3, p0, p1, p2}; lane 0's first is the strip boundary pixel X0 - 1, which the row carry
        // already contains -> 0
        const unsigned w = wv[r];
        unsigned prev = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0x138, 0xf, 0xf, false);      // wave_shr:1, lane 0 gets 0
        const unsigned p0 = prev >> 24, p1 = w & 255u, p2 = (w >> 8) & 255u, p3 = (w >> 16) & 255u;
        const unsigned a0 = p0, a1 = a0 + p1, a2 = a1 + p2, a3 = a2 + p3;
        const unsigned rc = (unsigned)__builtin_amdgcn_readlane((int)rcAll, r);
        const unsigned base = rc + (waveScanIncl(a3) - a3);
        top[0] += (A)(base + a0); top[1] += (A)(base + a1); top[2] += (A)(base + a2); top[3] += (A)(base + a3);
        if (c < Wc) storeRow4<TS>(sum + (size_t)(y + 1) * sumStep, c, Wc, top, nt != 0);
        if (SQ) {
            const unsigned b0 = p0 * p0, b1 = b0 + p1 * p1, b2 = b1 + p2 * p2, b3 = b2 + p3 * p3;
            const unsigned rq = (unsigned)__builtin_amdgcn_readlane((int)rqAll, r);
            const unsigned baseq = rq + (waveScanIncl(b3) - b3);
            topq[0] += baseq + b0; topq[1] += baseq + b1; topq[2] += baseq + b2; topq[3] += baseq + b3;
            if (c < Wc) storeRow4<double>(sq + (size_t)(y + 1) * sqStep, c, Wc, topq);
        }
    }
}

} // namespace

// aux layout per frame and per kind (sums / squares), in 4-byte words:
//   colsum nTy x W | rowsum nTx x H | colcarry nTy x W | rowcarry nTx x H | tileTot nTy x nTx | (pad to 8 bytes) | corner 2 x nTy x nTx
static size_t auxWordsPerFrame(int W, int H, int* nTxOut, int* nTyOut)
{
    const int nTx = divUp(W + 1, ITW), nTy = divUp(H, ITH);
    if (nTxOut) *nTxOut = nTx;
    if (nTyOut) *nTyOut = nTy;
    size_t w = 2 * ((size_t)nTy * W + (size_t)nTx * H) + (size_t)nTy * nTx;
    w = (w + 1) & ~(size_t)1;                                        // the u64 corner array starts 8-byte aligned
    return w + 2 * (size_t)nTy * nTx;
}

size_t integralTiledAuxBytes(int W, int H, int nframes, bool sq)
{
    return auxWordsPerFrame(W, H, nullptr, nullptr) * 4 * (sq ? 2 : 1) * (size_t)nframes + 16;
}

bool integralTiledU8(const uchar* src, size_t sstep, size_t sframe, int W, int H, int nframes, void* sum, size_t sumStepElems, size_t sumFrameElems, bool sumIsDouble,
                     double* sq, size_t sqStepElems, size_t sqFrameElems, void* aux, hipStream_t st)
{
    if (W < 1 || H < 1 || nframes < 1 || !aux || !sum) return false;
    // the squared partial sums (row / column carries of Q) are u32: 65025 * max(W, H) must stay below 2^32 (W, H <= 66051); beyond, the
    // general three-pass path with its 64-bit sums serves the call
    if (sq && (W > 66051 || H > 66051)) return false;
    int nTx, nTy;
    const size_t perFrame = auxWordsPerFrame(W, H, &nTx, &nTy);       // even: every array of every frame keeps its 8-byte alignment
    if (((size_t)nTx * nTy + 16 * (size_t)nTx) * 8 > 60 * 1024) return false;   // the 2-D prefix of the tile totals runs in one workgroup's LDS
    const int Wp = W;
    unsigned* base = (unsigned*)(((uintptr_t)aux + 7) & ~(uintptr_t)7);
    struct Arrays { unsigned *colsum, *rowsum, *colcar, *rowcar, *tileTot; unsigned long long* corner; };
    auto layout = [&](unsigned* b) {
        Arrays a;
        const size_t cw = (size_t)nTy * Wp, rw = (size_t)nTx * H;
        a.colsum = b; a.rowsum = a.colsum + cw; a.colcar = a.rowsum + rw; a.rowcar = a.colcar + cw; a.tileTot = a.rowcar + rw;
        size_t w = 2 * (cw + rw) + (size_t)nTy * nTx; w = (w + 1) & ~(size_t)1;
        a.corner = (unsigned long long*)(b + w);
        return a;
    };
    const Arrays S = layout(base);
    Arrays Q = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (sq) Q = layout(base + perFrame * nframes);
    const long long waves = (long long)nTx * nTy * nframes;
    const dim3 grid((unsigned)((waves + 3) / 4)), blk(256);
    if (sq) hipLaunchKernelGGL((k_integral_tilesums<true>), grid, blk, 0, st, src, sstep, sframe, W, H, nTx, nTy, nframes, S.colsum, Q.colsum, S.rowsum, Q.rowsum, S.tileTot, Q.tileTot, Wp, perFrame);
    else    hipLaunchKernelGGL((k_integral_tilesums<false>), grid, blk, 0, st, src, sstep, sframe, W, H, nTx, nTy, nframes, S.colsum, Q.colsum, S.rowsum, Q.rowsum, S.tileTot, Q.tileTot, Wp, perFrame);
    hipLaunchKernelGGL(k_integral_carries, dim3(divUp(W, 32) + divUp(H, 256) + 1, sq ? 2 : 1, nframes), blk, ((size_t)nTx * nTy + 16 * (size_t)nTx) * 8, st,
                       S.colsum, Q.colsum, S.rowsum, Q.rowsum, S.colcar, Q.colcar, S.rowcar, Q.rowcar, S.tileTot, Q.tileTot, S.corner, Q.corner,
                       W, H, Wp, nTx, nTy, perFrame, sq ? 1 : 0);
    constexpr int nt = 0;                                          // (non-temporal sum stores measured 7-10 % slower, profiles/r04_integral_aligned_stores_ab.txt)
#define ITILES(TS_, SQ_) hipLaunchKernelGGL((k_integral_tiles<TS_, SQ_>), grid, blk, 0, st, src, sstep, sframe, W, H, nTx, nTy, nframes, (TS_*)sum, sumStepElems, sumFrameElems, \
                                            sq, sqStepElems, sqFrameElems, S.colcar, Q.colcar, S.rowcar, Q.rowcar, S.corner, Q.corner, Wp, perFrame, nt)
    if (sumIsDouble) { if (sq) ITILES(double, true); else ITILES(double, false); }
    else             { if (sq) ITILES(int, true); else ITILES(int, false); }
#undef ITILES
    noteKernel("k_integral_tiles<%s,%s> grid=%u x256, %d frame(s) (after k_integral_tilesums + k_integral_carries)", sumIsDouble ? "double" : "int", sq ? "true" : "false", grid.x, nframes);
    return true;
}

// ---------------------------------------------------------------------------------- the general scan: any channel count, 8-bit and float sources
// cv::integral layout (sumpixels.simd.hpp): (H+1) x (W+1) x cn, first row / column zero.  sum in int32 (8-bit sources: exact, the
// reference's default) or double, squared sum in double.  Three passes, each with enough independent work to fill the chip:
//   rows    one workgroup per (row, channel): chunked scan of the row -> row-wise prefix sums
//   colseg  one thread per (column, segment of IS_SEG rows): prefix down the segment in place, segment total to `aux`
//   coladd  one thread per (column, segment >= 1): adds the totals of the segments above
// (a single thread walking a whole column would leave all but ~16 CUs idle and serialise 2160 dependent adds).
namespace {

enum { D8U = MI355CV_8U, D32S = MI355CV_32S, D32F = MI355CV_32F, D64F = MI355CV_64F };

constexpr int IS_SEG = 64;

template <typename TS>
__global__ __launch_bounds__(256) void k_integral_rows(const uchar* __restrict__ src, size_t sstep, size_t sframe, int W, int H, int cn, int depth,
                                                       TS* __restrict__ sum, size_t sumStep /*elements*/, size_t sumFrame,
                                                       double* __restrict__ sq, size_t sqStep, size_t sqFrame)
{
    const int y = blockIdx.x, c = blockIdx.y;
    src += (size_t)blockIdx.z * sframe; sum += (size_t)blockIdx.z * sumFrame; if (sq) sq += (size_t)blockIdx.z * sqFrame;
    const uchar* row = src + (size_t)y * sstep;
    const int chunk = (W + 255) / 256;
    const int x0 = threadIdx.x * chunk, x1 = min(W, x0 + chunk);
    auto px = [&](int x) -> double { return depth == D8U ? (double)row[x * cn + c] : (double)reinterpret_cast<const float*>(row)[x * cn + c]; };
    TS s = 0; double q = 0;
    for (int x = x0; x < x1; x++) { const double v = px(x); s += (TS)v; q += v * v; }
    __shared__ TS ss[256];
    __shared__ double qq[256];
    ss[threadIdx.x] = s; qq[threadIdx.x] = q;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                      // Hillis-Steele inclusive scan over the 256 chunk totals
        TS a = 0; double b = 0;
        if ((int)threadIdx.x >= o) { a = ss[threadIdx.x - o]; b = qq[threadIdx.x - o]; }
        __syncthreads();
        ss[threadIdx.x] += a; qq[threadIdx.x] += b;
        __syncthreads();
    }
    TS ps = threadIdx.x ? ss[threadIdx.x - 1] : (TS)0; double pq = threadIdx.x ? qq[threadIdx.x - 1] : 0.0;
    TS* srow = sum + (size_t)(y + 1) * sumStep;
    double* qrow = sq ? sq + (size_t)(y + 1) * sqStep : nullptr;
    if (threadIdx.x == 0) { srow[c] = 0; if (qrow) qrow[c] = 0; }
    for (int x = x0; x < x1; x++) {
        const double v = px(x);
        ps += (TS)v; pq += v * v;
        srow[(x + 1) * cn + c] = ps;
        if (qrow) qrow[(x + 1) * cn + c] = pq;
    }
}

// single-channel 8-bit rows, the common case: a thread owns 16 consecutive pixels (one 16-byte load when the row allows), the
// 256 thread totals are scanned with wave shuffles + one LDS exchange, and the finished row goes through LDS so that the
// global stores are lane-consecutive (a thread writing its own 16 results would touch 16 different 64-byte segments).
template <typename TS>
__global__ __launch_bounds__(256) void k_integral_rows_u8c1(const uchar* __restrict__ src, size_t sstep, size_t sframe, int W,
                                                            TS* __restrict__ sum, size_t sumStep, size_t sumFrame,
                                                            double* __restrict__ sq, size_t sqStep, size_t sqFrame)
{
    extern __shared__ __attribute__((aligned(16))) uchar ldsraw[];
    const int y = blockIdx.x;
    src += (size_t)blockIdx.z * sframe; sum += (size_t)blockIdx.z * sumFrame; if (sq) sq += (size_t)blockIdx.z * sqFrame;
    const uchar* row = src + (size_t)y * sstep;
    const int per = 16 * ((((W + 255) / 256) + 15) / 16);          // pixels per thread, a multiple of 16
    TS* LS = reinterpret_cast<TS*>(ldsraw);                          // W + 1 sums
    double* LQ = reinterpret_cast<double*>(ldsraw + (((size_t)(W + 1) * sizeof(TS) + 15) & ~(size_t)15));   // W + 1 squared sums
    const int x0 = threadIdx.x * per, x1 = min(W, x0 + per);
    const bool vec = ((((uintptr_t)row) | sstep) & 15) == 0;
    unsigned s = 0; unsigned long long q = 0;                      // exact: 255 * per and 255^2 * per are far below 2^32 / 2^64
    for (int x = x0; x < x1; x += 16) {
        unsigned w[4] = {0, 0, 0, 0};
        if (vec && x + 16 <= W) { const uint4 v = *reinterpret_cast<const uint4*>(row + x); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
        else for (int b = 0; b < 16 && x + b < W; b++) w[b >> 2] |= (unsigned)row[x + b] << (8 * (b & 3));
#pragma unroll
        for (int b = 0; b < 16; b++) { const unsigned p = (w[b >> 2] >> (8 * (b & 3))) & 255u; s += p; q += p * p; }
    }
    // block-wide exclusive scan of (s, q): wave shuffle scan, then the four wave totals through LDS
    __shared__ unsigned long long ws[4], wq[4];
    unsigned long long ps = s, pq = q;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long a = __shfl_up(ps, o), b = __shfl_up(pq, o);
        if (lane >= o) { ps += a; pq += b; }
    }
    if (lane == 63) { ws[wave] = ps; wq[wave] = pq; }
    __syncthreads();
    unsigned long long os = ps - s, oq = pq - q;                   // exclusive within the wave
    for (int k = 0; k < wave; k++) { os += ws[k]; oq += wq[k]; }
    if (threadIdx.x == 0) { LS[0] = 0; if (sq) LQ[0] = 0; }
    TS rs = (TS)os; double rq = (double)oq;
    for (int x = x0; x < x1; x++) {
        const unsigned p = row[x];
        rs += (TS)p; rq += (double)(p * p);
        LS[x + 1] = rs; if (sq) LQ[x + 1] = rq;
    }
    __syncthreads();
    TS* srow = sum + (size_t)(y + 1) * sumStep;
    for (int x = threadIdx.x; x <= W; x += 256) srow[x] = LS[x];
    if (sq) { double* qrow = sq + (size_t)(y + 1) * sqStep; for (int x = threadIdx.x; x <= W; x += 256) qrow[x] = LQ[x]; }
}

template <typename T>
__global__ __launch_bounds__(256) void k_integral_colseg(T* __restrict__ a, size_t step, size_t frame, int Wc /* (W+1)*cn */, int H, T* __restrict__ aux, size_t auxFrame)
{
    const int x = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (x >= Wc) return;
    a += (size_t)blockIdx.z * frame + x; aux += (size_t)blockIdx.z * auxFrame;
    const int y0 = 1 + seg * IS_SEG, y1 = min(H + 1, y0 + IS_SEG);
    if (seg == 0) a[0] = 0;
    T s = 0;
    int y = y0;
    for (; y + 8 <= y1; y += 8) {
        T v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = a[(size_t)(y + u) * step];
#pragma unroll
        for (int u = 0; u < 8; u++) { s += v[u]; a[(size_t)(y + u) * step] = s; }
    }
    for (; y < y1; y++) { s += a[(size_t)y * step]; a[(size_t)y * step] = s; }
    aux[(size_t)seg * Wc + x] = s;
}

template <typename T>
__global__ __launch_bounds__(256) void k_integral_coladd(T* __restrict__ a, size_t step, size_t frame, int Wc, int H, const T* __restrict__ aux, size_t auxFrame)
{
    const int x = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y + 1;
    if (x >= Wc) return;
    a += (size_t)blockIdx.z * frame + x; aux += (size_t)blockIdx.z * auxFrame;
    T off = 0;
    for (int s = 0; s < seg; s++) off += aux[(size_t)s * Wc + x];
    const int y0 = 1 + seg * IS_SEG, y1 = min(H + 1, y0 + IS_SEG);
#pragma unroll 8
    for (int y = y0; y < y1; y++) a[(size_t)y * step] += off;
}

// column passes over one array; aux = nseg x Wc scratch elements per frame
template <typename T>
void integralColumns(T* a, size_t step, size_t frame, int Wc, int H, int nframes, T* aux, hipStream_t st)
{
    const int nseg = divUp(H, IS_SEG);
    hipLaunchKernelGGL(k_integral_colseg<T>, dim3(divUp(Wc, 256), nseg, nframes), dim3(256), 0, st, a, step, frame, Wc, H, aux, (size_t)nseg * Wc);
    if (nseg > 1)
        hipLaunchKernelGGL(k_integral_coladd<T>, dim3(divUp(Wc, 256), nseg - 1, nframes), dim3(256), 0, st, a, step, frame, Wc, H, aux, (size_t)nseg * Wc);
}

} // namespace

size_t integralSumSqAuxBytes(int W, int H, int cn, int nframes)
{
    return (size_t)divUp(H, IS_SEG) * (W + 1) * cn * nframes * sizeof(double);
}

void integralSumSq(const uchar* src, size_t sstep, size_t sframe, int W, int H, int cn, int depth, int nframes, double* dsum, double* dsq, double* aux, hipStream_t st)
{
    const size_t isteps = (size_t)(W + 1) * cn, iframeD = isteps * (H + 1);
    hipLaunchKernelGGL(k_integral_rows<double>, dim3(H, cn, nframes), dim3(256), 0, st, src, sstep, sframe, W, H, cn, depth, dsum, isteps, iframeD, dsq, isteps, iframeD);
    integralColumns<double>(dsum, isteps, iframeD, (int)isteps, H, nframes, aux, st);
    integralColumns<double>(dsq, isteps, iframeD, (int)isteps, H, nframes, aux, st);
}

namespace {

// One call of mi355cv_integral past the depth table, under the hook's own argument names (a decline's reason is its condition's text).  Three routes: the ordered
// kernels of integral_seq.hip for everything whose bits depend on the order of the additions (ordered); for 8-bit sources with CV_32S / CV_64F sums -- exact integers
// in any order -- exact() stages the call and hands it to the tiled kernels above (one channel), else to the general scan
struct IntegralCall {
    int depth, sdepth, sqdepth; const uchar* src_data; size_t src_step; uchar* sum_data; size_t sum_step; uchar* sqsum_data; size_t sqsum_step;
    uchar* tilted_data; size_t tilted_step; int width, height, cn;
    const uchar* ds; size_t dss, d1, d2, d3; uchar* s1; uchar* s2; uchar* s3;      // stage(): the source, the sum, the squared and the tilted sum where the kernels find them
    size_t se() const { return sdepth == D32S ? 4 : 8; }

    // es, e1, e2: bytes per element of the source, of the sum (and the tilted sum), of the squared sum; an output the caller did not give, or that could not be staged, is null
    void stage(Stager& stg, size_t es, size_t e1, size_t e2)
    {
        d2 = d3 = 0;
        ds = stg.in(src_data, src_step, (size_t)width * cn * es, height, &dss);
        s1 = stg.out(sum_data, sum_step, (size_t)(width + 1) * cn * e1, height + 1, &d1);
        s2 = sqsum_data ? stg.out(sqsum_data, sqsum_step, (size_t)(width + 1) * cn * e2, height + 1, &d2) : nullptr;
        s3 = tilted_data ? stg.out(tilted_data, tilted_step, (size_t)(width + 1) * cn * e1, height + 1, &d3) : nullptr;
    }

    int ordered()                                                                  // k_iseq_*: float sources, CV_32F sums, CV_32F / CV_32S squared sums, tilted sums
    {
        if (depth == D8U && sdepth == D32F && !sqsum_data && !tilted_data && (double)width * height * 255.0 >= 16777216.0)
            return setError(MI355CV_NOT_IMPLEMENTED, "integral: CV_8U -> CV_32F sums past 2^24 without a squared / tilted sum depend on the CPU's vector width");
        const size_t e1 = sdepth == D64F ? 8 : 4, e2 = sqdepth == D64F ? 8 : 4, es = depth == D8U ? 1 : depth == D32F ? 4 : depth == D64F ? 8 : 2;
        if (width <= 0 || height <= 0 || (sum_step % e1) || (sqsum_data && (sqsum_step % e2)) || (tilted_data && (tilted_step % e1)) || (src_step % es))
            return MI355_DECLINED("width <= 0 || height <= 0 || a step that is not a multiple of its element size");
        if ((double)(width + 1) * cn * (height + 1) >= 2147483647.0) return MI355_DECLINED("more than 2^31 elements");
        Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
        MI355_DECLINE_IF(!ensureDevice());
        // (HOST_HEAVY: the reference's scalar loops take 10-60 ms per 4K image on one core -- worth two PCIe crossings, unlike the 8-bit vector paths of the tiled kind)
        MI355_DECLINE_IF(hostImageTooSmall(src_data, (size_t)width * height, minPixels(HOST_HEAVY)));
        stage(stg, es, e1, e2);
        void* aux = tilted_data ? stg.scratch(integralOrderedAuxBytes(width, height, cn, sdepth, true)) : nullptr;
        if (!ds || !s1 || (sqsum_data && !s2) || (tilted_data && (!s3 || !aux))) return MI355_DECLINED("staging / scratch for the ordered integral");
        if (!integralOrdered(depth, sdepth, sqdepth, ds, dss, s1, d1, s2, d2, s3, d3, width, height, cn, aux, stream()))
            return MI355_DECLINED("!integralOrdered(...)");
        noteKernel("k_iseq_rows + k_iseq_cols%s (ordered sums, depths %d -> %d / %d)", tilted_data ? " + k_iseq_tbuf / tcol0 / tdiag" : "", depth, sdepth, sqdepth);
        return stg.finish("integral");
    }
    int exact()                                                                    // the staging of the two exact routes, then the first of them that takes the call
    {
        MI355_DECLINE_IF(width <= 0 || height <= 0 || (sum_step % se()) || (sqsum_data && (sqsum_step % 8)));
        Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
        MI355_DECLINE_IF(!ensureDevice());
        MI355_DECLINE_IF(hostImageTooSmall(src_data, (size_t)width * height, minPixels()));
        stage(stg, 1, se(), 8);
        MI355_DECLINE_IF(!ds || !s1 || (sqsum_data && !s2));
        const int rc = tiled(stg);
        return rc != NEXT_PATH ? rc : scan(stg);
    }
    int tiled(Stager& stg)                                                         // k_integral_tiles: one channel, two passes over the pixels + carries instead of a row pass
    {                                                                              // and two column passes over the sum image
        static const bool tiledOff = envInt("MI355CV_INTEGRAL_TILED", 1) == 0;
        if (!(depth == D8U && cn == 1 && !tiledOff)) return NEXT_PATH;
        void* taux = stg.scratch(integralTiledAuxBytes(width, height, 1, s2 != nullptr));
        if (taux && integralTiledU8(ds, dss, 0, width, height, 1, s1, d1 / se(), 0, sdepth == D64F, (double*)s2, d2 / 8, 0, taux, stream()))
            return stg.finish("integral");
        return NEXT_PATH;
    }
    template <typename TS> void scanRows(bool fastRows, size_t ldsFast, hipStream_t st)
    {
        if (fastRows) hipLaunchKernelGGL(k_integral_rows_u8c1<TS>, dim3(height, 1, 1), dim3(256), ldsFast, st, ds, dss, 0, width, (TS*)s1, d1 / sizeof(TS), 0, (double*)s2, d2 / 8, 0);
        else hipLaunchKernelGGL(k_integral_rows<TS>, dim3(height, cn, 1), dim3(256), 0, st, ds, dss, 0, width, height, cn, depth, (TS*)s1, d1 / sizeof(TS), 0, (double*)s2, d2 / 8, 0);
    }
    int scan(Stager& stg)                                                          // k_integral_rows / k_integral_rows_u8c1, then the column segments of the sum and the squared sum
    {
        const int Wc = (width + 1) * cn, nseg = divUp(height, IS_SEG);
        hipStream_t st = stream();
        void* aux = stg.scratch((size_t)nseg * Wc * 8);
        MI355_DECLINE_IF(!aux);
        const size_t ldsFast = (((size_t)(width + 1) * se() + 15) & ~(size_t)15) + (s2 ? (size_t)(width + 1) * 8 : 0);
        const bool fastRows = depth == D8U && cn == 1 && ldsFast <= 60 * 1024;
        if (sdepth == D32S) { scanRows<int>(fastRows, ldsFast, st); integralColumns<int>((int*)s1, d1 / 4, 0, Wc, height, 1, (int*)aux, st); }
        else { scanRows<double>(fastRows, ldsFast, st); integralColumns<double>((double*)s1, d1 / 8, 0, Wc, height, 1, (double*)aux, st); }
        if (s2) integralColumns<double>((double*)s2, d2 / 8, 0, Wc, height, 1, (double*)aux, st);
        noteKernel("%s<%s> grid=%dx%dx1 x256 + k_integral_colseg / coladd in %d segment(s)", fastRows ? "k_integral_rows_u8c1" : "k_integral_rows", sdepth == D32S ? "int" : "double",
                   height, fastRows ? 1 : cn, nseg);
        return stg.finish("integral");
    }
};

} // namespace
} // namespace mi355

using namespace mi355;

extern "C" {

// replaces hal_ni_integral (hal_replacement.hpp:977; caller cv::integral sumpixels.dispatch.cpp:415): every depth triple of the reference's table (:383-406), with or
// without the squared and the tilted sum.  CV_8U sources with CV_32S / CV_64F sums (squared sum in CV_64F, no tilted sum) take the tiled / scanned kernels above -- exact
// integers in any order; everything whose value depends on the order of the additions -- float sources, CV_32F sums, CV_32F / CV_32S squared sums, tilted sums -- takes
// integral_seq.hip, which adds in the reference's order (bit for bit).  One case is left to the CPU: CV_8U -> CV_32F sums without a squared or tilted sum beyond 2^24
// (the reference's vector body recovers the row prefix in its scalar tail by a subtraction, sumpixels.simd.hpp:528-533, so the bits depend on the CPU's vector width).
MI355CV_API int mi355cv_integral(int depth, int sdepth, int sqdepth, const uchar* src_data, size_t src_step, uchar* sum_data, size_t sum_step,
                                 uchar* sqsum_data, size_t sqsum_step, uchar* tilted_data, size_t tilted_step, int width, int height, int cn)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !sum_data || !src_data);
    if (!integralOrderedTriple(depth, sdepth, sqdepth) || cn < 1)
        return setError(MI355CV_NOT_IMPLEMENTED, "integral: depths %d -> sum %d, sqsum %d%s, %d channels: not a row of the reference's table", depth, sdepth, sqdepth, sqsum_data ? "" : " (no sqsum)", cn);
    const bool tiledKind = !tilted_data && cn <= 4 && depth == D8U && (sdepth == D32S || sdepth == D64F) && (!sqsum_data || sqdepth == D64F) &&
                           !(sdepth == D32S && (double)width * height * 255.0 > 2147483647.0);          // (sums that wrap: the ordered kernels wrap like the reference)
    IntegralCall c = {depth, sdepth, sqdepth, src_data, src_step, sum_data, sum_step, sqsum_data, sqsum_step, tilted_data, tilted_step, width, height, cn};
    return tiledKind ? c.exact() : c.ordered();
}

// frame-batched form for device-resident CV_8UC1 frames: every frame's (H+1) x (W+1) CV_32S (or CV_64F) sum [+ CV_64F squared sum] from the
// same three launches that serve one frame (the tile index carries the frame) -- the per-frame launches of a single 4K image are
// latency-bound (2160 waves), a batch fills the machine.  Strides in bytes.
MI355CV_API int mi355cv_integralBatch(const uchar* src_data, size_t src_step, size_t src_frame_stride, uchar* sum_data, size_t sum_step, size_t sum_frame_stride,
                                      uchar* sqsum_data, size_t sqsum_step, size_t sqsum_frame_stride, int nframes, int width, int height, int sdepth)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !src_data || !sum_data || nframes < 1 || width <= 0 || height <= 0 || (sdepth != D32S && sdepth != D64F));
    const size_t se = sdepth == D32S ? 4 : 8;
    MI355_DECLINE_IF((sum_step % se) || (sum_frame_stride % se) || (sqsum_data && ((sqsum_step % 8) || (sqsum_frame_stride % 8))));
    MI355_DECLINE_IF(sdepth == D32S && (double)width * height * 255.0 > 2147483647.0);
    if (nframes > MAX_GRID_FRAMES)                                                              // the kernels take the frame from blockIdx.z; the carries are scratch per call
        return sliceFrames(nframes, [&](size_t f0, int nf) {
            return mi355cv_integralBatch(src_data + f0 * src_frame_stride, src_step, src_frame_stride, sum_data + f0 * sum_frame_stride, sum_step, sum_frame_stride,
                                         sqsum_data ? sqsum_data + f0 * sqsum_frame_stride : nullptr, sqsum_step, sqsum_frame_stride, nf, width, height, sdepth); });
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    if (!ensureDevice() || !isDevicePtr(src_data) || !isDevicePtr(sum_data) || (sqsum_data && !isDevicePtr(sqsum_data)))
        return setError(MI355CV_NOT_IMPLEMENTED, "integralBatch: device-resident frames only");
    if (nframes == 1) { src_frame_stride = 0; sum_frame_stride = 0; sqsum_frame_stride = 0; }
    void* taux = stg.scratch(integralTiledAuxBytes(width, height, nframes, sqsum_data != nullptr));
    if (!taux || !integralTiledU8(src_data, src_step, src_frame_stride, width, height, nframes, sum_data, sum_step / se, sum_frame_stride / se, sdepth == D64F,
                                  (double*)sqsum_data, sqsum_step / 8, sqsum_frame_stride / 8, taux, stream()))
        return setError(MI355CV_NOT_IMPLEMENTED, "integralBatch: frame geometry outside the tiled path");
    return stg.finish("integralBatch");
}

} // extern "C"
