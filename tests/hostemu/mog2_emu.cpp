// mog2_emu.cpp -- opencv_amd/csrc/mog2_math.h (the arithmetic of the kernels of mog2.hip) compiled for the CPU: the per-pixel update of the mixture, the shadow test,
// the mask value and the background mean, for tests/test_mog2_cpu.py to hold against tests/mog2_restate.py.  The model crosses in the reference's order
// (modes, {weight, variance} pairs per mode, means per mode), slots at and above a pixel's count zero.
#include "mog2_math.h"
#include <stdint.h>

namespace {

// par: Tb, TB, Tg, varInit, varMin, varMax, CT, tau
mog2::Params paramsOf(const float* par, int nmix, int detectShadows, int shadowValue)
{
    mog2::Params P;
    P.Tb = par[0]; P.TB = par[1]; P.Tg = par[2]; P.varInit = par[3]; P.varMin = par[4]; P.varMax = par[5]; P.CT = par[6]; P.tau = par[7];
    P.nmixtures = nmix; P.detectShadows = detectShadows; P.shadowValue = shadowValue;
    return P;
}

template <int CN>
void load(mog2::Pixel<CN>& px, int p, int nmix, const uint8_t* modes, const float* gmm, const float* mean)
{
    mog2::clear(px);
    px.nmodes = modes[p];
    for (int m = 0; m < px.nmodes; m++) {
        px.w[m] = gmm[((size_t)p * nmix + m) * 2]; px.var[m] = gmm[((size_t)p * nmix + m) * 2 + 1];
        for (int c = 0; c < CN; c++) px.mean[m][c] = mean[((size_t)p * nmix + m) * CN + c];
    }
}

template <int CN>
void store(const mog2::Pixel<CN>& px, int p, int nmix, uint8_t* modes, float* gmm, float* mean)
{
    modes[p] = (uint8_t)px.nmodes;
    for (int m = 0; m < nmix; m++) {
        const bool used = m < px.nmodes;
        gmm[((size_t)p * nmix + m) * 2] = used ? px.w[m] : 0.f; gmm[((size_t)p * nmix + m) * 2 + 1] = used ? px.var[m] : 0.f;
        for (int c = 0; c < CN; c++) mean[((size_t)p * nmix + m) * CN + c] = used ? px.mean[m][c] : 0.f;
    }
}

template <int CN>
void applyT(int isFloat, const void* frame, int npix, int nmix, uint8_t* modes, float* gmm, float* mean, const mog2::Params& P, float alphaT, uint8_t* mask)
{
    for (int p = 0; p < npix; p++) {
        mog2::Pixel<CN> px;
        load(px, p, nmix, modes, gmm, mean);
        float x[CN];
        for (int c = 0; c < CN; c++) x[c] = isFloat ? ((const float*)frame)[(size_t)p * CN + c] : (float)((const uint8_t*)frame)[(size_t)p * CN + c];
        const bool bg = mog2::update(px, x, P, alphaT);
        mask[p] = (uint8_t)mog2::maskValue(bg, px, x, P);
        store(px, p, nmix, modes, gmm, mean);
    }
}

template <int CN>
void backgroundT(int npix, int nmix, const uint8_t* modes, const float* gmm, const float* mean, const mog2::Params& P, float* out)
{
    for (int p = 0; p < npix; p++) {
        mog2::Pixel<CN> px;
        load(px, p, nmix, modes, gmm, mean);
        float v[CN];
        mog2::backgroundMean(px, P, v);
        for (int c = 0; c < CN; c++) out[(size_t)p * CN + c] = v[c];
    }
}

} // namespace

extern "C" void emu_mog2_apply(int cn, int isFloat, const void* frame, int npix, int nmix, uint8_t* modes, float* gmm, float* mean, const float* par, int detectShadows,
                               int shadowValue, float alphaT, uint8_t* mask)
{
    const mog2::Params P = paramsOf(par, nmix, detectShadows, shadowValue);
    if (cn == 1) applyT<1>(isFloat, frame, npix, nmix, modes, gmm, mean, P, alphaT, mask);
    else applyT<3>(isFloat, frame, npix, nmix, modes, gmm, mean, P, alphaT, mask);
}

extern "C" void emu_mog2_background(int cn, int npix, int nmix, const uint8_t* modes, const float* gmm, const float* mean, const float* par, float* out)
{
    const mog2::Params P = paramsOf(par, nmix, 0, 0);
    if (cn == 1) backgroundT<1>(npix, nmix, modes, gmm, mean, P, out);
    else backgroundT<3>(npix, nmix, modes, gmm, mean, P, out);
}

extern "C" unsigned emu_mog2_round8(float v) { return mog2::roundSat8(v); }
extern "C" int emu_mog2_max_dim(void) { return mog2::MAX_DIM; }
extern "C" int emu_mog2_max_mixtures(void) { return mog2::MAX_MIXTURES; }
