// farneback.hip -- cv::calcOpticalFlowFarneback (video/src/optflowgf.cpp; no HAL hook) on CV_8UC1 frames, single pairs and runs of consecutive frames.  The arithmetic is
// farneback_math.h; the definition it is held against, bit for bit, is tests/farneback_restate.py.
//   k_fb_smooth3            the level Gaussian with 3 taps (the only one that runs at full resolution on the finest level): both passes per pixel from the 8-bit frame
//   k_fb_smooth_h / _v      any tap count up to mi355cv_limit("farneback_max_smooth_taps"): a plain two-pass filter (coarse levels only)
//   k_fb_resize<CN, SCALED> the bilinear resize of the level image (CN = 1) and of the coarser flow with its factor 1 / pyr_scale (CN = 2)
//   k_fb_polyexp            both passes of the polynomial expansion over an LDS tile of 64 x 16 pixels with an n-pixel halo: 4 bytes in, 20 out per pixel
//   k_fb_update_matrices    pointwise, with the four-point gather of R1
//   k_fb_update_flow        the window sums of the five planes of M from an LDS tile of 32 x 16 pixels with an m-pixel halo (vertical pass into LDS, then horizontal), the solve
// R0, R1 and M are five interleaved floats per pixel, as the reference keeps them.  Workspace comes from Stager::scratch.
// Limits (mi355cv_limit): "farneback_max_dim" = 16384, "farneback_max_winsize" = 25, "farneback_max_poly_n" = 7, "farneback_max_smooth_taps" = 255.
#include "rt.h"
#include "farneback_math.h"
#include <vector>

using namespace mi355;

namespace {

static_assert(fb::MAX_DIM == lim::FARNEBACK_MAX_DIM && fb::MAX_WINSIZE == lim::FARNEBACK_MAX_WINSIZE && fb::MAX_POLY_N == lim::FARNEBACK_MAX_POLY_N &&
              fb::MAX_SMOOTH_TAPS == lim::FARNEBACK_MAX_SMOOTH_TAPS, "mi355cv_limit(\"farneback_*\")");

constexpr int PE_TW = 64, PE_TH = 16;                                   // k_fb_polyexp: output tile
constexpr int PE_COLS = PE_TW + 2 * fb::MAX_POLY_N, PE_ROWS = PE_TH + 2 * fb::MAX_POLY_N;
constexpr int UF_TW = 32, UF_TH = 16;                                   // k_fb_update_flow: output tile
constexpr size_t ufLdsBytes(int m) { return (size_t)5 * ((UF_TH + 2 * m) * (UF_TW + 2 * m) + UF_TH * (UF_TW + 2 * m)) * sizeof(float); }
static_assert(ufLdsBytes(fb::MAX_WINSIZE / 2) <= 65536, "the M tile and the vertical sums of k_fb_update_flow fit 64 KiB of LDS");

// ------------------------------------------------------------------ level images
__global__ __launch_bounds__(256) void k_fb_smooth3(const uchar* __restrict__ src, size_t sstep, float* __restrict__ dst, size_t dpitch, int w, int h, float t0, float t1, float t2)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const int xl = fb::reflect101(x - 1, w), xr = fb::reflect101(x + 1, w);
    float hs[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const uchar* r = src + (size_t)fb::reflect101(y + j - 1, h) * sstep;
        float s = t0 * (float)r[xl];
        s = s + t1 * (float)r[x];
        hs[j] = s + t2 * (float)r[xr];
    }
    float s = t0 * hs[0];
    s = s + t1 * hs[1];
    dst[(size_t)y * dpitch + x] = s + t2 * hs[2];
}

__global__ __launch_bounds__(256) void k_fb_smooth_h(const uchar* __restrict__ src, size_t sstep, float* __restrict__ dst, size_t dpitch, int w, int h,
                                                     const float* __restrict__ taps, int n)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const uchar* r = src + (size_t)y * sstep;
    const int x0 = x - n / 2;
    dst[(size_t)y * dpitch + x] = fb::tapSum(taps, n, [&](int i) { return (float)r[fb::reflect101(x0 + i, w)]; });
}

__global__ __launch_bounds__(256) void k_fb_smooth_v(const float* __restrict__ src, size_t spitch, float* __restrict__ dst, size_t dpitch, int w, int h,
                                                     const float* __restrict__ taps, int n)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const int y0 = y - n / 2;
    dst[(size_t)y * dpitch + x] = fb::tapSum(taps, n, [&](int i) { return src[(size_t)fb::reflect101(y0 + i, h) * spitch + x]; });
}

// pitches in floats; sx = sw / dw, sy = sh / dh in double; SCALED: every result times `factor` in double, rounded once
template <int CN, bool SCALED>
__global__ __launch_bounds__(256) void k_fb_resize(const float* __restrict__ src, size_t spitch, int sw, int sh, float* __restrict__ dst, size_t dpitch, int dw, int dh,
                                                   double sx, double sy, double factor)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dw || y >= dh) return;
    int x0, x1, y0, y1;
    float fx, fy;
    fb::resizeCoord(x, sx, sw, x0, x1, fx);
    fb::resizeCoord(y, sy, sh, y0, y1, fy);
    const float* a = src + (size_t)y0 * spitch;
    const float* b = src + (size_t)y1 * spitch;
    float* o = dst + (size_t)y * dpitch + (size_t)x * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const float top = fb::lerp(a[(size_t)x0 * CN + c], a[(size_t)x1 * CN + c], fx);
        const float bot = fb::lerp(b[(size_t)x0 * CN + c], b[(size_t)x1 * CN + c], fx);
        const float v = fb::lerp(top, bot, fy);
        o[c] = SCALED ? (float)((double)v * factor) : v;
    }
}

// ------------------------------------------------------------------ polynomial expansion
__global__ __launch_bounds__(256) void k_fb_polyexp(const float* __restrict__ src, size_t spitch, float* __restrict__ dst, size_t dpitch, int w, int h, fb::PolyTaps T)
{
    __shared__ float tile[PE_ROWS * PE_COLS];
    __shared__ float vs[3][PE_TH * PE_COLS];
    const int n = T.n, cols = PE_TW + 2 * n, rows = PE_TH + 2 * n;
    const int x0 = blockIdx.x * PE_TW, y0 = blockIdx.y * PE_TH;
    const int tid = threadIdx.x;
    // the source under the tile and its halo; replicated rows and columns are the clamped coordinates
    for (int e = tid; e < rows * cols; e += 256) {
        const int r = e / cols, c = e - r * cols;
        const int yy = fb::clampi(y0 + r - n, 0, h - 1), xx = fb::clampi(x0 + c - n, 0, w - 1);
        tile[r * PE_COLS + c] = src[(size_t)yy * spitch + xx];
    }
    __syncthreads();
    // vertical pass: the three sums of every column of the tile with its halo
    for (int e = tid; e < PE_TH * cols; e += 256) {
        const int r = e / cols, c = e - r * cols;
        const float* p = tile + (r + n) * PE_COLS + c;
        float v[3];
        fb::polyVertical(T, [&](int k) { return p[k * PE_COLS]; }, v);
        vs[0][r * PE_COLS + c] = v[0]; vs[1][r * PE_COLS + c] = v[1]; vs[2][r * PE_COLS + c] = v[2];
    }
    __syncthreads();
    for (int e = tid; e < PE_TH * PE_TW; e += 256) {
        const int r = e / PE_TW, c = e - r * PE_TW;
        const int x = x0 + c, y = y0 + r;
        if (x >= w || y >= h) continue;
        const int at = r * PE_COLS + c + n;
        float out[5];
        fb::polyHorizontal(T, [&](int k, int ch) { return vs[ch][at + k]; }, out);
        float* o = dst + (size_t)y * dpitch + (size_t)x * 5;
#pragma unroll
        for (int ch = 0; ch < 5; ch++) o[ch] = out[ch];
    }
}

// ------------------------------------------------------------------ update matrices (pitches in floats)
__global__ __launch_bounds__(256) void k_fb_update_matrices(const float* __restrict__ R0, size_t p0, const float* __restrict__ R1, size_t p1, const float* __restrict__ flow,
                                                            size_t pf, float* __restrict__ M, size_t pm, int w, int h)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const float* r0 = R0 + (size_t)y * p0 + (size_t)x * 5;
    const float* f = flow + (size_t)y * pf + (size_t)x * 2;
    const float r[5] = {r0[0], r0[1], r0[2], r0[3], r0[4]};
    float m[5];
    fb::updateMatrix(r, R1, p1, x, y, w, h, f[0], f[1], m);
    float* o = M + (size_t)y * pm + (size_t)x * 5;
#pragma unroll
    for (int c = 0; c < 5; c++) o[c] = m[c];
}

// ------------------------------------------------------------------ update flow
__global__ __launch_bounds__(256) void k_fb_update_flow(const float* __restrict__ M, size_t pm, float* __restrict__ flow, size_t pf, int w, int h, fb::WinTaps W)
{
    extern __shared__ float lds[];
    const int m = W.m, nt = 2 * m + 1, cols = UF_TW + 2 * m, rows = UF_TH + 2 * m;
    float* mt = lds;                                                    // [5][rows][cols]
    float* vs = lds + 5 * rows * cols;                                  // [5][UF_TH][cols]
    const int x0 = blockIdx.x * UF_TW, y0 = blockIdx.y * UF_TH;
    const int tid = threadIdx.x;
    for (int e = tid; e < rows * cols * 5; e += 256) {
        const int pix = e / 5, c = e - pix * 5;
        const int r = pix / cols, col = pix - r * cols;
        const int yy = fb::clampi(y0 + r - m, 0, h - 1), xx = fb::clampi(x0 + col - m, 0, w - 1);
        mt[c * rows * cols + pix] = M[(size_t)yy * pm + (size_t)xx * 5 + c];
    }
    __syncthreads();
    for (int e = tid; e < 5 * UF_TH * cols; e += 256) {
        const int c = e / (UF_TH * cols), rc = e - c * (UF_TH * cols);
        const int r = rc / cols, col = rc - r * cols;
        const float* p = mt + c * rows * cols + r * cols + col;
        vs[e] = fb::tapSum(W.t, nt, [&](int i) { return p[i * cols]; });
    }
    __syncthreads();
    for (int e = tid; e < UF_TH * UF_TW; e += 256) {
        const int r = e / UF_TW, col = e - r * UF_TW;
        const int x = x0 + col, y = y0 + r;
        if (x >= w || y >= h) continue;
        float s[5];
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const float* p = vs + c * UF_TH * cols + r * cols + col;
            s[c] = fb::tapSum(W.t, nt, [&](int i) { return p[i]; });
        }
        float fx, fy;
        fb::solveFlow(s, W.scale, fx, fy);
        float* o = flow + (size_t)y * pf + (size_t)x * 2;
        o[0] = fx; o[1] = fy;
    }
}

// ------------------------------------------------------------------ launches
inline dim3 grid64x4(int w, int h) { return dim3((unsigned)divUp(w, 64), (unsigned)divUp(h, 4)); }

void launchPolyExp(const float* src, size_t spitch, float* dst, size_t dpitch, int w, int h, const fb::PolyTaps& T, hipStream_t st)
{
    hipLaunchKernelGGL(k_fb_polyexp, dim3((unsigned)divUp(w, PE_TW), (unsigned)divUp(h, PE_TH)), dim3(256), 0, st, src, spitch, dst, dpitch, w, h, T);
}
void launchUpdateMatrices(const float* R0, size_t p0, const float* R1, size_t p1, const float* flow, size_t pf, float* M, size_t pm, int w, int h, hipStream_t st)
{
    hipLaunchKernelGGL(k_fb_update_matrices, grid64x4(w, h), dim3(64, 4), 0, st, R0, p0, R1, p1, flow, pf, M, pm, w, h);
}
void launchUpdateFlow(const float* M, size_t pm, float* flow, size_t pf, int w, int h, const fb::WinTaps& W, hipStream_t st)
{
    hipLaunchKernelGGL(k_fb_update_flow, dim3((unsigned)divUp(w, UF_TW), (unsigned)divUp(h, UF_TH)), dim3(256), ufLdsBytes(W.m), st, M, pm, flow, pf, w, h, W);
}

struct Args { double pyrScale; int levels, winsize, iterations, polyN; double polySigma; int flags; };

// the refusals that need no device; 0 when served.  On success plan[0 .. *nlev) is the level plan
int checkArgs(int w, int h, const Args& a, fb::Level* plan, int* nlev)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(w < 1 || h < 1 || w > lim::FARNEBACK_MAX_DIM || h > lim::FARNEBACK_MAX_DIM);
    MI355_DECLINE_IF(a.winsize < 1 || a.winsize > lim::FARNEBACK_MAX_WINSIZE);
    MI355_DECLINE_IF(a.polyN < 1 || a.polyN > lim::FARNEBACK_MAX_POLY_N);
    MI355_DECLINE_IF(a.iterations < 0 || a.levels < 1 || a.levels > fb::MAX_LEVELS);
    MI355_DECLINE_IF(!(a.pyrScale > 0 && a.pyrScale < 1) || !(a.polySigma >= 0));
    MI355_DECLINE_IF(a.flags & ~(fb::USE_INITIAL_FLOW | fb::FARNEBACK_GAUSSIAN));
    *nlev = fb::levelPlan(w, h, a.pyrScale, a.levels, plan);
    if ((a.flags & fb::USE_INITIAL_FLOW) && *nlev > 1) return MI355_DECLINED("OPTFLOW_USE_INITIAL_FLOW with more than one effective pyramid level");
    for (int k = 0; k < *nlev; k++) MI355_DECLINE_IF(plan[k].ksize > lim::FARNEBACK_MAX_SMOOTH_TAPS);
    return 0;
}

inline bool misaligned4(const void* p, size_t step) { return (((uintptr_t)p | step) & 3) != 0; }

struct Work {                                                          // scratch of one call
    float* fimg; float* tmp; float* limg; float* M;
    float* R[2][fb::MAX_LEVELS];                                       // the expansions of two frames, every level
    float* flow[fb::MAX_LEVELS];                                       // level flows above level 0 (dense)
    const float* taps[fb::MAX_LEVELS];                                 // device taps of the levels with more than 3
    float t3[fb::MAX_LEVELS][3];
};

bool allocWork(Stager& stg, Work& wk, int w, int h, const fb::Level* plan, int nlev)
{
    const size_t px = (size_t)w * h;
    wk.fimg = (float*)stg.scratch(px * 4); wk.tmp = (float*)stg.scratch(px * 4); wk.limg = (float*)stg.scratch(px * 4); wk.M = (float*)stg.scratch(px * 20);
    if (!wk.fimg || !wk.tmp || !wk.limg || !wk.M) return false;
    for (int k = 0; k < nlev; k++) {
        const size_t lp = (size_t)plan[k].w * plan[k].h;
        for (int s = 0; s < 2; s++) if (!(wk.R[s][k] = (float*)stg.scratch(lp * 20))) return false;
        wk.flow[k] = nullptr;
        if (k > 0 && !(wk.flow[k] = (float*)stg.scratch(lp * 8))) return false;
        std::vector<float> t(plan[k].ksize);
        fb::gaussianTaps(plan[k].ksize, plan[k].sigma, t.data());
        wk.taps[k] = nullptr;
        if (plan[k].ksize == 3) { wk.t3[k][0] = t[0]; wk.t3[k][1] = t[1]; wk.t3[k][2] = t[2]; }
        else if (!(wk.taps[k] = (const float*)stg.param(t.data(), t.size() * 4))) return false;
    }
    return true;
}

// the level images and polynomial expansions of one device-resident frame into wk.R[slot]
void expandFrame(const Work& wk, int slot, const uchar* img, size_t step, int w, int h, const fb::Level* plan, int nlev, const fb::PolyTaps& T, hipStream_t st)
{
    for (int k = 0; k < nlev; k++) {
        const fb::Level& L = plan[k];
        const bool same = L.w == w && L.h == h;                        // the resize to the same size returns its source bit for bit (fractions 0): skipped
        float* sm = same ? wk.limg : wk.fimg;
        if (L.ksize == 3) hipLaunchKernelGGL(k_fb_smooth3, grid64x4(w, h), dim3(64, 4), 0, st, img, step, sm, (size_t)w, w, h, wk.t3[k][0], wk.t3[k][1], wk.t3[k][2]);
        else {
            hipLaunchKernelGGL(k_fb_smooth_h, grid64x4(w, h), dim3(64, 4), 0, st, img, step, wk.tmp, (size_t)w, w, h, wk.taps[k], L.ksize);
            hipLaunchKernelGGL(k_fb_smooth_v, grid64x4(w, h), dim3(64, 4), 0, st, (const float*)wk.tmp, (size_t)w, sm, (size_t)w, w, h, wk.taps[k], L.ksize);
        }
        if (!same)
            hipLaunchKernelGGL((k_fb_resize<1, false>), grid64x4(L.w, L.h), dim3(64, 4), 0, st, (const float*)wk.fimg, (size_t)w, w, h, wk.limg, (size_t)L.w, L.w, L.h,
                               (double)w / L.w, (double)h / L.h, 1.0);
        launchPolyExp(wk.limg, (size_t)L.w, wk.R[slot][k], (size_t)L.w * 5, L.w, L.h, T, st);
    }
}

// the flow from the frame in slot a to the frame in slot b, coarse to fine, into `flow` (pitch pf floats; holds the initial flow with OPTFLOW_USE_INITIAL_FLOW)
int flowOfPair(const char* entry, const Work& wk, int a, int b, float* flow, size_t pf, int w, int h, const fb::Level* plan, int nlev, const Args& A, const fb::WinTaps& W,
               hipStream_t st)
{
    for (int k = nlev - 1; k >= 0; k--) {
        const fb::Level& L = plan[k];
        float* f = k == 0 ? flow : wk.flow[k];
        const size_t p = k == 0 ? pf : (size_t)L.w * 2;
        if (k == nlev - 1) {
            if (!(A.flags & fb::USE_INITIAL_FLOW) && hipMemset2DAsync(f, p * 4, 0, (size_t)L.w * 8, L.h, st) != hipSuccess)
                return setError(MI355CV_ERROR_UNKNOWN, "%s: hipMemset2DAsync failed", entry);
        } else {
            const fb::Level& C = plan[k + 1];
            hipLaunchKernelGGL((k_fb_resize<2, true>), grid64x4(L.w, L.h), dim3(64, 4), 0, st, (const float*)wk.flow[k + 1], (size_t)C.w * 2, C.w, C.h, f, p, L.w, L.h,
                               (double)C.w / L.w, (double)C.h / L.h, 1.0 / A.pyrScale);
        }
        const size_t pr = (size_t)L.w * 5;
        launchUpdateMatrices(wk.R[a][k], pr, wk.R[b][k], pr, f, p, wk.M, pr, L.w, L.h, st);
        for (int i = 0; i < A.iterations; i++) {
            launchUpdateFlow(wk.M, pr, f, p, L.w, L.h, W, st);
            if (i < A.iterations - 1) launchUpdateMatrices(wk.R[a][k], pr, wk.R[b][k], pr, f, p, wk.M, pr, L.w, L.h, st);
        }
    }
    MI355_CHECK_LAUNCH(entry);
    return MI355CV_OK;
}

// frames[0 .. nf) -> flows[0 .. nf - 1): each shared frame is expanded once
int runFlows(const char* entry, const uchar* const* frames, const size_t* fsteps, int nf, uchar* const* flows, const size_t* flsteps, int w, int h, const Args& A)
{
    fb::Level plan[fb::MAX_LEVELS];
    int nlev = 0;
    if (const int rc = checkArgs(w, h, A, plan, &nlev)) return rc;
    MI355_DECLINE_IF(nf < 2);
    for (int i = 0; i < nf; i++) MI355_DECLINE_IF(!frames[i] || fsteps[i] < (size_t)w);
    for (int i = 0; i + 1 < nf; i++) MI355_DECLINE_IF(!flows[i] || flsteps[i] < (size_t)w * 8 || misaligned4(flows[i], flsteps[i]));
    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(frames[0], (size_t)w * h, minPixels(HOST_HEAVY)));
    const size_t fspan = (size_t)(h - 1) * fsteps[0] + w;
    for (int i = 0; i + 1 < nf; i++) {
        const size_t ospan = (size_t)(h - 1) * flsteps[i] + (size_t)w * 8;
        for (int j = 0; j < nf; j++) MI355_DECLINE_IF(overlapOnDevice(frames[j], fspan, flows[i], ospan));
        for (int j = 0; j < i; j++) MI355_DECLINE_IF(overlapOnDevice(flows[j], ospan, flows[i], ospan));
    }
    std::vector<const uchar*> df(nf);
    std::vector<size_t> ds(nf);
    for (int i = 0; i < nf; i++) {
        df[i] = i > 0 && frames[i] == frames[i - 1] ? df[i - 1] : stg.in(frames[i], fsteps[i], (size_t)w, h, &ds[i]);
        if (i > 0 && frames[i] == frames[i - 1]) ds[i] = ds[i - 1];
        MI355_DECLINE_IF(!df[i]);
    }
    Work wk;
    if (!allocWork(stg, wk, w, h, plan, nlev)) return MI355_DECLINED("scratch for the level images, expansions and flows could not be allocated");
    fb::PolyTaps T;
    fb::WinTaps W;
    fb::polySetup(A.polyN, A.polySigma, T);
    fb::winSetup(A.winsize, (A.flags & fb::FARNEBACK_GAUSSIAN) != 0, W);
    hipStream_t st = stream();
    expandFrame(wk, 0, df[0], ds[0], w, h, plan, nlev, T, st);
    for (int i = 0; i + 1 < nf; i++) {
        expandFrame(wk, (i + 1) & 1, df[i + 1], ds[i + 1], w, h, plan, nlev, T, st);
        size_t os;
        uchar* o = stg.out(flows[i], flsteps[i], (size_t)w * 8, h, &os);
        MI355_DECLINE_IF(!o);
        if ((A.flags & fb::USE_INITIAL_FLOW) && o != flows[i]) {       // a host-resident initial flow: up into the staged destination
            if (hipMemcpy2DAsync(o, os, flows[i], flsteps[i], (size_t)w * 8, h, hipMemcpyHostToDevice, st) != hipSuccess)
                return setError(MI355CV_ERROR_UNKNOWN, "%s: H2D of the initial flow failed", entry);
            noteStagedBytes((long long)w * 8 * h);
        }
        if (const int rc = flowOfPair(entry, wk, i & 1, (i + 1) & 1, (float*)o, os / 4, w, h, plan, nlev, A, W, st)) return rc;
    }
    if (A.iterations > 0)
        noteKernel("k_fb_update_flow<%s> grid=%dx%d x256, winsize %d, %d level(s), %d iteration(s), %d flow(s); k_fb_polyexp n=%d", (A.flags & fb::FARNEBACK_GAUSSIAN) ? "gauss" : "box",
                   divUp(w, UF_TW), divUp(h, UF_TH), A.winsize, nlev, A.iterations, nf - 1, A.polyN);
    else noteKernel("k_fb_update_matrices grid=%dx%d x256, %d level(s), no iterations, %d flow(s); k_fb_polyexp n=%d", divUp(w, 64), divUp(h, 4), nlev, nf - 1, A.polyN);
    return stg.finish(entry);
}

} // namespace

extern "C" {

// Host-resident frames are staged (HOST_HEAVY): about 100 bytes per pixel and iteration cross memory on either side, against 10 bytes per pixel over PCIe.
MI355CV_API int mi355cv_calcOpticalFlowFarneback(const uchar* prev, size_t prev_step, const uchar* next, size_t next_step, uchar* flow, size_t flow_step, int width, int height,
                                                 double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags)
{
    mi355::EntryGuard entry_(__func__);
    const uchar* frames[2] = {prev, next};
    const size_t steps[2] = {prev_step, next_step};
    uchar* flows[1] = {flow};
    const size_t fls[1] = {flow_step};
    return runFlows("calcOpticalFlowFarneback", frames, steps, 2, flows, fls, width, height, Args{pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags});
}

// Host-resident batches are staged whole, frame by frame, through the Stager: the pipeline of runHostBatch hands its callback one chunk of frames and takes one output per
// input frame, and a flow needs the frame before its chunk too.
MI355CV_API int mi355cv_calcOpticalFlowFarnebackBatch(const uchar* frames, size_t step, size_t frame_stride, int nframes, uchar* flows, size_t flow_step, size_t flow_frame_stride,
                                                      int width, int height, double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !frames || !flows);
    MI355_DECLINE_IF(nframes < 2 || nframes > 4096);
    MI355_DECLINE_IF(width < 1 || height < 1);
    MI355_DECLINE_IF(step < (size_t)width || flow_step < (size_t)width * 8);
    MI355_DECLINE_IF(frame_stride < (size_t)(height - 1) * step + (size_t)width);
    MI355_DECLINE_IF(nframes > 2 && flow_frame_stride < (size_t)(height - 1) * flow_step + (size_t)width * 8);
    MI355_DECLINE_IF(flow_frame_stride & 3);
    MI355_DECLINE_IF(flags & fb::USE_INITIAL_FLOW);                    // one initial flow per pair would be read from `flows`; not served for batches
    std::vector<const uchar*> f(nframes);
    std::vector<uchar*> o(nframes - 1);
    std::vector<size_t> fs(nframes, step), os(nframes - 1, flow_step);
    for (int i = 0; i < nframes; i++) f[i] = frames + (size_t)i * frame_stride;
    for (int i = 0; i + 1 < nframes; i++) o[i] = flows + (size_t)i * flow_frame_stride;
    return runFlows("calcOpticalFlowFarnebackBatch", f.data(), fs.data(), nframes, o.data(), os.data(), width, height,
                    Args{pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags});
}

// ---- the stages, one kernel each (CV_32F images; R and M are five floats per pixel, flow two)
MI355CV_API int mi355cv_farnebackPolyExp(const uchar* src, size_t src_step, uchar* dst, size_t dst_step, int width, int height, int poly_n, double poly_sigma)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !src || !dst);
    MI355_DECLINE_IF(width < 1 || height < 1 || width > lim::FARNEBACK_MAX_DIM || height > lim::FARNEBACK_MAX_DIM);
    MI355_DECLINE_IF(poly_n < 1 || poly_n > lim::FARNEBACK_MAX_POLY_N || !(poly_sigma >= 0));
    MI355_DECLINE_IF(src_step < (size_t)width * 4 || dst_step < (size_t)width * 20 || misaligned4(src, src_step) || misaligned4(dst, dst_step));
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(overlapOnDevice(src, (size_t)(height - 1) * src_step + (size_t)width * 4, dst, (size_t)(height - 1) * dst_step + (size_t)width * 20));
    size_t ss, ds;
    const uchar* s = stg.in(src, src_step, (size_t)width * 4, height, &ss);
    uchar* d = stg.out(dst, dst_step, (size_t)width * 20, height, &ds);
    MI355_DECLINE_IF(!s || !d);
    fb::PolyTaps T;
    fb::polySetup(poly_n, poly_sigma, T);
    launchPolyExp((const float*)s, ss / 4, (float*)d, ds / 4, width, height, T, stream());
    MI355_CHECK_LAUNCH("farnebackPolyExp");
    noteKernel("k_fb_polyexp grid=%dx%d x256, n=%d", divUp(width, PE_TW), divUp(height, PE_TH), poly_n);
    return stg.finish("farnebackPolyExp");
}

MI355CV_API int mi355cv_farnebackUpdateMatrices(const uchar* R0, size_t r0_step, const uchar* R1, size_t r1_step, const uchar* flow, size_t flow_step, uchar* M, size_t m_step,
                                                int width, int height)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !R0 || !R1 || !flow || !M);
    MI355_DECLINE_IF(width < 1 || height < 1 || width > lim::FARNEBACK_MAX_DIM || height > lim::FARNEBACK_MAX_DIM);
    const size_t rb = (size_t)width * 20, fbytes = (size_t)width * 8;
    MI355_DECLINE_IF(r0_step < rb || r1_step < rb || m_step < rb || flow_step < fbytes);
    MI355_DECLINE_IF(misaligned4(R0, r0_step) || misaligned4(R1, r1_step) || misaligned4(flow, flow_step) || misaligned4(M, m_step));
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    const size_t mspan = (size_t)(height - 1) * m_step + rb;
    MI355_DECLINE_IF(overlapOnDevice(R0, (size_t)(height - 1) * r0_step + rb, M, mspan) || overlapOnDevice(R1, (size_t)(height - 1) * r1_step + rb, M, mspan) ||
                     overlapOnDevice(flow, (size_t)(height - 1) * flow_step + fbytes, M, mspan));
    size_t s0, s1, sf, sm;
    const uchar* a = stg.in(R0, r0_step, rb, height, &s0);
    const uchar* b = stg.in(R1, r1_step, rb, height, &s1);
    const uchar* f = stg.in(flow, flow_step, fbytes, height, &sf);
    uchar* m = stg.out(M, m_step, rb, height, &sm);
    MI355_DECLINE_IF(!a || !b || !f || !m);
    launchUpdateMatrices((const float*)a, s0 / 4, (const float*)b, s1 / 4, (const float*)f, sf / 4, (float*)m, sm / 4, width, height, stream());
    MI355_CHECK_LAUNCH("farnebackUpdateMatrices");
    noteKernel("k_fb_update_matrices grid=%dx%d x256", divUp(width, 64), divUp(height, 4));
    return stg.finish("farnebackUpdateMatrices");
}

// one iteration: flow from the window sums of M; with R0, R1 and M_next given, M_next is the update matrix of the new flow (every iteration but the last)
MI355CV_API int mi355cv_farnebackUpdateFlow(const uchar* M, size_t m_step, uchar* flow, size_t flow_step, const uchar* R0, size_t r0_step, const uchar* R1, size_t r1_step,
                                            uchar* M_next, size_t m_next_step, int width, int height, int winsize, int flags)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !M || !flow);
    MI355_DECLINE_IF(width < 1 || height < 1 || width > lim::FARNEBACK_MAX_DIM || height > lim::FARNEBACK_MAX_DIM);
    MI355_DECLINE_IF(winsize < 1 || winsize > lim::FARNEBACK_MAX_WINSIZE);
    MI355_DECLINE_IF(flags & ~fb::FARNEBACK_GAUSSIAN);
    const bool update = R0 || R1 || M_next;
    MI355_DECLINE_IF(update && (!R0 || !R1 || !M_next));
    const size_t rb = (size_t)width * 20, fbytes = (size_t)width * 8;
    MI355_DECLINE_IF(m_step < rb || flow_step < fbytes || misaligned4(M, m_step) || misaligned4(flow, flow_step));
    if (update) MI355_DECLINE_IF(r0_step < rb || r1_step < rb || m_next_step < rb || misaligned4(R0, r0_step) || misaligned4(R1, r1_step) || misaligned4(M_next, m_next_step));
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    const size_t mspan = (size_t)(height - 1) * m_step + rb, fspan = (size_t)(height - 1) * flow_step + fbytes;
    MI355_DECLINE_IF(overlapOnDevice(M, mspan, flow, fspan));
    if (update) {
        const size_t nspan = (size_t)(height - 1) * m_next_step + rb;
        MI355_DECLINE_IF(overlapOnDevice(M, mspan, M_next, nspan) || overlapOnDevice(flow, fspan, M_next, nspan) ||
                         overlapOnDevice(R0, (size_t)(height - 1) * r0_step + rb, M_next, nspan) || overlapOnDevice(R1, (size_t)(height - 1) * r1_step + rb, M_next, nspan) ||
                         overlapOnDevice(R0, (size_t)(height - 1) * r0_step + rb, flow, fspan) || overlapOnDevice(R1, (size_t)(height - 1) * r1_step + rb, flow, fspan));
    }
    size_t sm, sf, s0 = 0, s1 = 0, sn = 0;
    const uchar* m = stg.in(M, m_step, rb, height, &sm);
    uchar* f = stg.out(flow, flow_step, fbytes, height, &sf);
    MI355_DECLINE_IF(!m || !f);
    const uchar* a = nullptr; const uchar* b = nullptr; uchar* mn = nullptr;
    if (update) {
        a = stg.in(R0, r0_step, rb, height, &s0);
        b = stg.in(R1, r1_step, rb, height, &s1);
        mn = stg.out(M_next, m_next_step, rb, height, &sn);
        MI355_DECLINE_IF(!a || !b || !mn);
    }
    fb::WinTaps W;
    fb::winSetup(winsize, (flags & fb::FARNEBACK_GAUSSIAN) != 0, W);
    launchUpdateFlow((const float*)m, sm / 4, (float*)f, sf / 4, width, height, W, stream());
    if (update) launchUpdateMatrices((const float*)a, s0 / 4, (const float*)b, s1 / 4, (const float*)f, sf / 4, (float*)mn, sn / 4, width, height, stream());
    MI355_CHECK_LAUNCH("farnebackUpdateFlow");
    noteKernel("k_fb_update_flow<%s> grid=%dx%d x256, winsize %d%s", (flags & fb::FARNEBACK_GAUSSIAN) ? "gauss" : "box", divUp(width, UF_TW), divUp(height, UF_TH), winsize,
               update ? "; k_fb_update_matrices" : "");
    return stg.finish("farnebackUpdateFlow");
}

} // extern "C"
