// farneback_emu.cpp -- opencv_amd/csrc/farneback_math.h (the arithmetic of the kernels of farneback.hip) compiled for the CPU: every stage over dense images and the whole
// call with the control flow of farneback.hip's host side, for tests/test_farneback_cpu.py to hold against tests/farneback_restate.py.  R and M are five floats per pixel,
// flow two.
#include "farneback_math.h"
#include <string.h>
#include <vector>

namespace {

void smooth(const uint8_t* src, int w, int h, const float* taps, int n, float* dst)
{
    std::vector<float> tmp((size_t)w * h);
    const int r = n / 2;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            tmp[(size_t)y * w + x] = fb::tapSum(taps, n, [&](int i) { return (float)src[(size_t)y * w + fb::reflect101(x - r + i, w)]; });
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            dst[(size_t)y * w + x] = fb::tapSum(taps, n, [&](int i) { return tmp[(size_t)fb::reflect101(y - r + i, h) * w + x]; });
}

void resize(const float* src, int sw, int sh, int cn, float* dst, int dw, int dh, bool scaled, double factor)
{
    const double sx = (double)sw / dw, sy = (double)sh / dh;
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            int x0, x1, y0, y1;
            float fx, fy;
            fb::resizeCoord(x, sx, sw, x0, x1, fx);
            fb::resizeCoord(y, sy, sh, y0, y1, fy);
            for (int c = 0; c < cn; c++) {
                const float top = fb::lerp(src[((size_t)y0 * sw + x0) * cn + c], src[((size_t)y0 * sw + x1) * cn + c], fx);
                const float bot = fb::lerp(src[((size_t)y1 * sw + x0) * cn + c], src[((size_t)y1 * sw + x1) * cn + c], fx);
                const float v = fb::lerp(top, bot, fy);
                dst[((size_t)y * dw + x) * cn + c] = scaled ? (float)((double)v * factor) : v;
            }
        }
}

void polyExp(const float* src, int w, int h, const fb::PolyTaps& T, float* dst)
{
    std::vector<float> vs((size_t)w * h * 3);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float v[3];
            fb::polyVertical(T, [&](int k) { return src[(size_t)fb::clampi(y + k, 0, h - 1) * w + x]; }, v);
            for (int c = 0; c < 3; c++) vs[((size_t)y * w + x) * 3 + c] = v[c];
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float r[5];
            fb::polyHorizontal(T, [&](int k, int c) { return vs[((size_t)y * w + fb::clampi(x + k, 0, w - 1)) * 3 + c]; }, r);
            for (int c = 0; c < 5; c++) dst[((size_t)y * w + x) * 5 + c] = r[c];
        }
}

void updateMatrices(const float* R0, const float* R1, const float* flow, int w, int h, float* M)
{
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float m[5];
            const size_t p = (size_t)y * w + x;
            fb::updateMatrix(R0 + p * 5, R1, (size_t)w * 5, x, y, w, h, flow[p * 2], flow[p * 2 + 1], m);
            for (int c = 0; c < 5; c++) M[p * 5 + c] = m[c];
        }
}

void updateFlow(const float* M, int w, int h, const fb::WinTaps& W, float* flow)
{
    const int m = W.m, nt = 2 * m + 1;
    std::vector<float> vs((size_t)w * h * 5);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 5; c++)
                vs[((size_t)y * w + x) * 5 + c] = fb::tapSum(W.t, nt, [&](int i) { return M[((size_t)fb::clampi(y - m + i, 0, h - 1) * w + x) * 5 + c]; });
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float s[5];
            for (int c = 0; c < 5; c++) s[c] = fb::tapSum(W.t, nt, [&](int i) { return vs[((size_t)y * w + fb::clampi(x - m + i, 0, w - 1)) * 5 + c]; });
            fb::solveFlow(s, W.scale, flow[((size_t)y * w + x) * 2], flow[((size_t)y * w + x) * 2 + 1]);
        }
}

void levelImage(const uint8_t* img, int w, int h, const fb::Level& L, std::vector<float>& out)
{
    std::vector<float> taps(L.ksize), sm((size_t)w * h);
    fb::gaussianTaps(L.ksize, L.sigma, taps.data());
    smooth(img, w, h, taps.data(), L.ksize, sm.data());
    out.resize((size_t)L.w * L.h);
    resize(sm.data(), w, h, 1, out.data(), L.w, L.h, false, 1.0);
}

} // namespace

extern "C" {

int emu_fb_limit(int which) { return which == 0 ? fb::MAX_DIM : which == 1 ? fb::MAX_WINSIZE : which == 2 ? fb::MAX_POLY_N : fb::MAX_SMOOTH_TAPS; }

void emu_fb_gaussian_taps(int n, double sigma, float* out) { fb::gaussianTaps(n, sigma, out); }

// g, xg, xxg: n + 1 floats each; ig: ig11, ig03, ig33, ig55
void emu_fb_poly_setup(int n, double sigma, float* g, float* xg, float* xxg, float* ig)
{
    fb::PolyTaps T;
    fb::polySetup(n, sigma, T);
    for (int k = 0; k <= n; k++) { g[k] = T.g[k]; xg[k] = T.xg[k]; xxg[k] = T.xxg[k]; }
    ig[0] = T.ig11; ig[1] = T.ig03; ig[2] = T.ig33; ig[3] = T.ig55;
}

// out: (width, height, taps of the Gaussian) per level; returns the effective level count
int emu_fb_level_plan(int w, int h, double pyrScale, int levels, int* out)
{
    fb::Level plan[fb::MAX_LEVELS];
    const int n = fb::levelPlan(w, h, pyrScale, levels, plan);
    for (int k = 0; k < n; k++) { out[3 * k] = plan[k].w; out[3 * k + 1] = plan[k].h; out[3 * k + 2] = plan[k].ksize; }
    return n;
}

void emu_fb_smooth(const uint8_t* src, int w, int h, int ksize, double sigma, float* dst)
{
    std::vector<float> taps(ksize);
    fb::gaussianTaps(ksize, sigma, taps.data());
    smooth(src, w, h, taps.data(), ksize, dst);
}

void emu_fb_resize(const float* src, int sw, int sh, int cn, float* dst, int dw, int dh, int scaled, double factor) { resize(src, sw, sh, cn, dst, dw, dh, scaled != 0, factor); }

void emu_fb_poly_exp(const float* src, int w, int h, int n, double sigma, float* dst)
{
    fb::PolyTaps T;
    fb::polySetup(n, sigma, T);
    polyExp(src, w, h, T, dst);
}

void emu_fb_update_matrices(const float* R0, const float* R1, const float* flow, int w, int h, float* M) { updateMatrices(R0, R1, flow, w, h, M); }

void emu_fb_update_flow(const float* M, int w, int h, int winsize, int gaussian, float* flow)
{
    fb::WinTaps W;
    fb::winSetup(winsize, gaussian != 0, W);
    updateFlow(M, w, h, W, flow);
}

// the whole call; flow holds the initial flow with OPTFLOW_USE_INITIAL_FLOW.  Returns 0, or 1 where farneback.hip declines
int emu_fb_calc(const uint8_t* prev, const uint8_t* next, float* flow, int w, int h, double pyrScale, int levels, int winsize, int iterations, int polyN, double polySigma,
                int flags)
{
    if (w < 1 || h < 1 || w > fb::MAX_DIM || h > fb::MAX_DIM || winsize < 1 || winsize > fb::MAX_WINSIZE || polyN < 1 || polyN > fb::MAX_POLY_N || iterations < 0 ||
        levels < 1 || levels > fb::MAX_LEVELS || !(pyrScale > 0 && pyrScale < 1) || !(polySigma >= 0) || (flags & ~(fb::USE_INITIAL_FLOW | fb::FARNEBACK_GAUSSIAN)))
        return 1;
    fb::Level plan[fb::MAX_LEVELS];
    const int nlev = fb::levelPlan(w, h, pyrScale, levels, plan);
    if ((flags & fb::USE_INITIAL_FLOW) && nlev > 1) return 1;
    for (int k = 0; k < nlev; k++) if (plan[k].ksize > fb::MAX_SMOOTH_TAPS) return 1;
    fb::PolyTaps T;
    fb::WinTaps W;
    fb::polySetup(polyN, polySigma, T);
    fb::winSetup(winsize, (flags & fb::FARNEBACK_GAUSSIAN) != 0, W);
    std::vector<float> cur, coarse, img, R0, R1, M;
    for (int k = nlev - 1; k >= 0; k--) {
        const fb::Level& L = plan[k];
        const size_t lp = (size_t)L.w * L.h;
        if (k == nlev - 1) {
            cur.assign(lp * 2, 0.f);
            if (flags & fb::USE_INITIAL_FLOW) memcpy(cur.data(), flow, lp * 2 * sizeof(float));
        } else {
            coarse.swap(cur);
            cur.resize(lp * 2);
            resize(coarse.data(), plan[k + 1].w, plan[k + 1].h, 2, cur.data(), L.w, L.h, true, 1.0 / pyrScale);
        }
        R0.resize(lp * 5); R1.resize(lp * 5); M.resize(lp * 5);
        levelImage(prev, w, h, L, img);
        polyExp(img.data(), L.w, L.h, T, R0.data());
        levelImage(next, w, h, L, img);
        polyExp(img.data(), L.w, L.h, T, R1.data());
        updateMatrices(R0.data(), R1.data(), cur.data(), L.w, L.h, M.data());
        for (int i = 0; i < iterations; i++) {
            updateFlow(M.data(), L.w, L.h, W, cur.data());
            if (i < iterations - 1) updateMatrices(R0.data(), R1.data(), cur.data(), L.w, L.h, M.data());
        }
    }
    memcpy(flow, cur.data(), (size_t)w * h * 2 * sizeof(float));
    return 0;
}

} // extern "C"
