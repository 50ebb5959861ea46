// mog2.hip -- cv::BackgroundSubtractorMOG2 (video/src/bgfg_gaussmix2.cpp; no HAL hook) on CV_8UC1 / CV_8UC3 / CV_32FC1 / CV_32FC3, single frames and runs of
// consecutive frames of one camera.  The arithmetic is mog2_math.h; the definition it is held against is tests/mog2_restate.py.
// The model is a structure of arrays in HBM, owned by the handle: planes weight[m], variance[m], mean[m][c] of h*w floats each (m < nmixtures) and modesUsed as bytes,
// so that a wave's loads of one plane are contiguous.
//   k_mog2_apply_seq<T, CN, PPT>   a lane owns PPT neighbouring pixels: loads the planes below their mode counts ONCE, folds `nframes` consecutive frames into the
//                                  model in registers in time order (one mask stored per frame, the next frame's pixels in flight meanwhile), stores the planes below
//                                  the new counts ONCE.  mi355cv_mog2Apply is the same kernel with nframes = 1.  PPT = 4 is CV_8UC1 where every row of source and
//                                  mask starts on a dword and the width is a multiple of 4: one dword of pixels in, one dword of mask out, float4 of every plane;
//                                  PPT = 1 serves any base, pitch and type.
//   k_mog2_background<T, CN>       getBackgroundImage
//   k_mog2_export<CN>              the model in the reference's array-of-structs order (modesUsed, {weight, variance} pairs per mode, means per mode), unused slots zero
// Limits (mi355cv_limit): "mog2_max_dim" = 16384, "mog2_max_mixtures" = 5.
#include "rt.h"
#include "mog2_math.h"
#include <algorithm>
#include <new>
#include <string.h>
#include <limits.h>
#include <vector>

using namespace mi355;

namespace {

static_assert(mog2::MAX_DIM == lim::MOG2_MAX_DIM && mog2::MAX_MIXTURES == lim::MOG2_MAX_MIXTURES, "mi355cv_limit(\"mog2_max_dim\"), (\"mog2_max_mixtures\")");

constexpr int M = mog2::MAX_MIXTURES;
constexpr int SEQ_MAX = 64;                 // frames per launch: their rates travel in the kernel arguments
constexpr int MOG2_MAGIC = 0x4d4f4732;

struct Model { float* weight; float* var; float* mean; uchar* modes; size_t plane; };   // plane: h*w, the distance in floats between two planes
struct SeqRates { float alphaT[SEQ_MAX]; };

template <typename T> __device__ __forceinline__ float toFloat(T v) { return (float)v; }

// the planes of pixel `p` below its mode count into registers
template <int CN>
__device__ __forceinline__ void loadPixel(const Model& md, int p, mog2::Pixel<CN>& px)
{
    mog2::clear(px);
    const int n = md.modes[p];
    px.nmodes = n;
#pragma unroll
    for (int m = 0; m < M; m++) {
        if (m < n) {
            px.w[m] = md.weight[(size_t)m * md.plane + p];
            px.var[m] = md.var[(size_t)m * md.plane + p];
#pragma unroll
            for (int c = 0; c < CN; c++) px.mean[m][c] = md.mean[(size_t)(m * CN + c) * md.plane + p];
        }
    }
}

template <int CN>
__device__ __forceinline__ void storePixel(const Model& md, int p, const mog2::Pixel<CN>& px)
{
    md.modes[p] = (uchar)px.nmodes;
#pragma unroll
    for (int m = 0; m < M; m++) {
        if (m < px.nmodes) {
            md.weight[(size_t)m * md.plane + p] = px.w[m];
            md.var[(size_t)m * md.plane + p] = px.var[m];
#pragma unroll
            for (int c = 0; c < CN; c++) md.mean[(size_t)(m * CN + c) * md.plane + p] = px.mean[m][c];
        }
    }
}

// four neighbouring pixels (p a multiple of 4, plane a multiple of 4): float4 per plane, below the largest of the four counts.  Lanes of a pixel with fewer modes
// carry zeros in and whatever the update left out; nothing reads a slot at or above a pixel's own count.
__device__ __forceinline__ void loadQuad(const Model& md, int p, mog2::Pixel<1> (&px)[4])
{
    const uchar4 n4 = *reinterpret_cast<const uchar4*>(md.modes + p);
#pragma unroll
    for (int j = 0; j < 4; j++) mog2::clear(px[j]);
    px[0].nmodes = n4.x; px[1].nmodes = n4.y; px[2].nmodes = n4.z; px[3].nmodes = n4.w;
    const int n = max(max((int)n4.x, (int)n4.y), max((int)n4.z, (int)n4.w));
#pragma unroll
    for (int m = 0; m < M; m++) {
        if (m < n) {
            const float4 w = *reinterpret_cast<const float4*>(md.weight + (size_t)m * md.plane + p);
            const float4 v = *reinterpret_cast<const float4*>(md.var + (size_t)m * md.plane + p);
            const float4 u = *reinterpret_cast<const float4*>(md.mean + (size_t)m * md.plane + p);
            px[0].w[m] = w.x; px[1].w[m] = w.y; px[2].w[m] = w.z; px[3].w[m] = w.w;
            px[0].var[m] = v.x; px[1].var[m] = v.y; px[2].var[m] = v.z; px[3].var[m] = v.w;
            px[0].mean[m][0] = u.x; px[1].mean[m][0] = u.y; px[2].mean[m][0] = u.z; px[3].mean[m][0] = u.w;
        }
    }
}

__device__ __forceinline__ void storeQuad(const Model& md, int p, const mog2::Pixel<1> (&px)[4])
{
    *reinterpret_cast<uchar4*>(md.modes + p) = make_uchar4((uchar)px[0].nmodes, (uchar)px[1].nmodes, (uchar)px[2].nmodes, (uchar)px[3].nmodes);
    const int n = max(max(px[0].nmodes, px[1].nmodes), max(px[2].nmodes, px[3].nmodes));
#pragma unroll
    for (int m = 0; m < M; m++) {
        if (m < n) {
            *reinterpret_cast<float4*>(md.weight + (size_t)m * md.plane + p) = make_float4(px[0].w[m], px[1].w[m], px[2].w[m], px[3].w[m]);
            *reinterpret_cast<float4*>(md.var + (size_t)m * md.plane + p) = make_float4(px[0].var[m], px[1].var[m], px[2].var[m], px[3].var[m]);
            *reinterpret_cast<float4*>(md.mean + (size_t)m * md.plane + p) = make_float4(px[0].mean[m][0], px[1].mean[m][0], px[2].mean[m][0], px[3].mean[m][0]);
        }
    }
}

// npix = W * H pixels, lane i owns pixels [PPT i, PPT i + PPT) of the raster (PPT = 4: W % 4 == 0, so the four share a row)
template <typename T, int CN, int PPT>
__global__ __launch_bounds__(256) void k_mog2_apply_seq(const uchar* __restrict__ src, size_t sstep, size_t sframe, uchar* __restrict__ mask, size_t mstep, size_t mframe,
                                                        int W, int npix, int nframes, Model md, mog2::Params P, SeqRates rates)
{
    const int p = (int)(blockIdx.x * 256u + threadIdx.x) * PPT;
    if (p >= npix) return;
    const int y = p / W, x0 = p - y * W;
    const uchar* s = src + (size_t)y * sstep + (size_t)x0 * CN * sizeof(T);
    uchar* d = mask + (size_t)y * mstep + x0;
    if constexpr (PPT == 4) {
        static_assert(CN == 1 && sizeof(T) == 1, "the quad path is CV_8UC1");
        mog2::Pixel<1> px[4];
        loadQuad(md, p, px);
        unsigned raw = *reinterpret_cast<const unsigned*>(s);
        for (int t = 0; t < nframes; t++) {
            const unsigned cur = raw;
            if (t + 1 < nframes) raw = *reinterpret_cast<const unsigned*>(s + (size_t)(t + 1) * sframe);
            const float alphaT = rates.alphaT[t];
            unsigned out = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float x[1] = {(float)((cur >> (8 * j)) & 255u)};
                const bool bg = mog2::update(px[j], x, P, alphaT);
                out |= mog2::maskValue(bg, px[j], x, P) << (8 * j);
            }
            *reinterpret_cast<unsigned*>(d + (size_t)t * mframe) = out;
        }
        storeQuad(md, p, px);
    } else {
        mog2::Pixel<CN> px;
        loadPixel(md, p, px);
        T raw[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) raw[c] = reinterpret_cast<const T*>(s)[c];
        for (int t = 0; t < nframes; t++) {
            float x[CN];
#pragma unroll
            for (int c = 0; c < CN; c++) x[c] = toFloat(raw[c]);
            if (t + 1 < nframes) {
#pragma unroll
                for (int c = 0; c < CN; c++) raw[c] = reinterpret_cast<const T*>(s + (size_t)(t + 1) * sframe)[c];
            }
            const bool bg = mog2::update(px, x, P, rates.alphaT[t]);
            d[(size_t)t * mframe] = (uchar)mog2::maskValue(bg, px, x, P);
        }
        storePixel(md, p, px);
    }
}

template <typename T, int CN>
__global__ __launch_bounds__(256) void k_mog2_background(uchar* __restrict__ dst, size_t dstep, int W, int npix, Model md, mog2::Params P)
{
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= npix) return;
    const int y = p / W, x = p - y * W;
    mog2::Pixel<CN> px;
    loadPixel(md, p, px);
    float v[CN];
    mog2::backgroundMean(px, P, v);
    T* o = reinterpret_cast<T*>(dst + (size_t)y * dstep) + (size_t)x * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        if constexpr (sizeof(T) == 1) o[c] = (uchar)mog2::roundSat8(v[c]);
        else o[c] = v[c];
    }
}

// gmm: npix x nmix x {weight, variance}; mean: npix x nmix x CN
template <int CN>
__global__ __launch_bounds__(256) void k_mog2_export(uchar* __restrict__ modes, float* __restrict__ gmm, float* __restrict__ mean, int npix, int nmix, Model md)
{
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= npix) return;
    mog2::Pixel<CN> px;
    loadPixel(md, p, px);
    modes[p] = (uchar)px.nmodes;
    float* g = gmm + (size_t)p * nmix * 2;
    float* u = mean + (size_t)p * nmix * CN;
#pragma unroll
    for (int m = 0; m < M; m++) {
        if (m < nmix) {
            g[2 * m] = px.w[m]; g[2 * m + 1] = px.var[m];        // (loadPixel left the slots at and above the count zero)
#pragma unroll
            for (int c = 0; c < CN; c++) u[m * CN + c] = px.mean[m][c];
        }
    }
}

// ------------------------------------------------------------------ the handle
struct Mog2Ctx {
    int magic = MOG2_MAGIC;
    int history = 500, nmixtures = M, detectShadows = 1, shadowValue = 127;
    float Tb = 16.f, TB = 0.9f, Tg = 9.f, varInit = 15.f, varMin = 4.f, varMax = 75.f, CT = 0.05f, tau = 0.5f;
    // the model
    int nframes = 0, w = 0, h = 0, type = -1, modelMix = 0, device = -1;
    bool mixChanged = false;
    void* buf = nullptr;
    Model md = {};
};

Mog2Ctx* ctxOf(void* c) { Mog2Ctx* x = (Mog2Ctx*)c; return x && x->magic == MOG2_MAGIC ? x : nullptr; }

mog2::Params paramsOf(const Mog2Ctx& c)
{
    mog2::Params P;
    P.Tb = c.Tb; P.TB = c.TB; P.Tg = c.Tg; P.varInit = c.varInit; P.varMin = c.varMin; P.varMax = c.varMax; P.CT = c.CT; P.tau = c.tau;
    P.nmixtures = c.modelMix; P.detectShadows = c.detectShadows; P.shadowValue = c.shadowValue;
    return P;
}

inline int typeCn(int type) { return (type >> 3) + 1; }
inline int typeDepth(int type) { return type & 7; }
inline bool typeServed(int type) { return type == MI355CV_8U || type == MI355CV_8U + 16 || type == MI355CV_32F || type == MI355CV_32F + 16; }

void freeModel(Mog2Ctx& c)
{
    if (c.buf) { (void)hipFree(c.buf); (void)hipGetLastError(); }
    c.buf = nullptr; c.md = Model{}; c.nframes = 0; c.w = c.h = 0; c.type = -1; c.modelMix = 0; c.device = -1;
}

// planes for w x h pixels of `type` and `nmix` modes on the calling thread's device; the old model goes only once the new one exists
bool allocModel(Mog2Ctx& c, int w, int h, int type, int nmix)
{
    const size_t plane = ((size_t)w * h + 3) & ~(size_t)3;                      // every plane starts on 16 bytes
    const int cn = typeCn(type);
    const size_t floats = plane * (size_t)nmix * (2 + cn);
    void* p = nullptr;
    if (hipMalloc(&p, floats * sizeof(float) + plane) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (c.buf) { (void)hipFree(c.buf); (void)hipGetLastError(); }
    c.buf = p;
    c.md.weight = (float*)p; c.md.var = c.md.weight + plane * nmix; c.md.mean = c.md.var + plane * nmix; c.md.modes = (uchar*)(c.md.mean + plane * nmix * cn);
    c.md.plane = plane;
    c.w = w; c.h = h; c.type = type; c.modelMix = nmix; c.device = activeDevice();
    return true;
}

template <typename T, int CN>
void launchSeq(bool quad, const uchar* s, size_t ss, size_t sf, uchar* m, size_t ms, size_t mf, int w, int npix, int nf, const Model& md, const mog2::Params& P,
               const SeqRates& r, hipStream_t st)
{
    if constexpr (CN == 1 && sizeof(T) == 1) {
        if (quad) {
            hipLaunchKernelGGL((k_mog2_apply_seq<T, CN, 4>), dim3((unsigned)divUp(npix / 4, 256)), dim3(256), 0, st, s, ss, sf, m, ms, mf, w, npix, nf, md, P, r);
            return;
        }
    }
    hipLaunchKernelGGL((k_mog2_apply_seq<T, CN, 1>), dim3((unsigned)divUp(npix, 256)), dim3(256), 0, st, s, ss, sf, m, ms, mf, w, npix, nf, md, P, r);
}

// `nf` device-resident frames in time order into the model, rates alphaT[0 .. nf)
void launchFrames(const Mog2Ctx& c, const uchar* s, size_t ss, size_t sf, uchar* m, size_t ms, size_t mf, int nf, const float* alphaT)
{
    const int npix = c.w * c.h;
    const mog2::Params P = paramsOf(c);
    const bool quad = c.type == MI355CV_8U && (c.w & 3) == 0 && (((uintptr_t)s | ss | (uintptr_t)m | ms | (nf > 1 ? (sf | mf) : 0)) & 3) == 0;
    hipStream_t st = stream();
    for (int f0 = 0; f0 < nf; f0 += SEQ_MAX) {
        const int g = std::min(SEQ_MAX, nf - f0);
        SeqRates r;
        for (int i = 0; i < SEQ_MAX; i++) r.alphaT[i] = i < g ? alphaT[f0 + i] : 0.f;
        const uchar* sp = s + (size_t)f0 * sf;
        uchar* mp = m + (size_t)f0 * mf;
        switch (c.type) {
        case MI355CV_8U:        launchSeq<uchar, 1>(quad, sp, ss, sf, mp, ms, mf, c.w, npix, g, c.md, P, r, st); break;
        case MI355CV_8U + 16:   launchSeq<uchar, 3>(false, sp, ss, sf, mp, ms, mf, c.w, npix, g, c.md, P, r, st); break;
        case MI355CV_32F:       launchSeq<float, 1>(false, sp, ss, sf, mp, ms, mf, c.w, npix, g, c.md, P, r, st); break;
        default:                launchSeq<float, 3>(false, sp, ss, sf, mp, ms, mf, c.w, npix, g, c.md, P, r, st); break;
        }
    }
    noteKernel("k_mog2_apply_seq<type %d,%s> grid=%d x256, %d frame(s) in %d launch(es)", c.type, quad ? "quad" : "pixel", divUp(quad ? npix / 4 : npix, 256), nf,
               divUp(nf, SEQ_MAX));
}

// the refusals of apply / applyBatch that need no device; 0 when the arguments are served
int applyArgs(const Mog2Ctx* c, const void* src, size_t sstep, size_t sframe, const void* mask, size_t mstep, size_t mframe, int nframes, int w, int h, int type)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!c || !src || !mask || nframes < 1);
    MI355_DECLINE_IF(!typeServed(type));
    MI355_DECLINE_IF(c->nmixtures < 1 || c->nmixtures > lim::MOG2_MAX_MIXTURES || c->history < 1);
    MI355_DECLINE_IF(w < 1 || h < 1 || w > lim::MOG2_MAX_DIM || h > lim::MOG2_MAX_DIM);
    const size_t e = depthBytes(typeDepth(type)), rowb = (size_t)w * typeCn(type) * e;
    MI355_DECLINE_IF(sstep < rowb || mstep < (size_t)w);
    if (nframes > 1) MI355_DECLINE_IF(sframe < (size_t)(h - 1) * sstep + rowb || mframe < (size_t)(h - 1) * mstep + (size_t)w);
    if (((uintptr_t)src | sstep | (nframes > 1 ? sframe : 0)) & (e - 1)) return MI355_DECLINED("source pointer, pitch or frame stride not a multiple of the element size");
    return 0;
}

// the rates of the next `n` frames (nf: frames the model has seen), each computed in double and rounded to float as the reference does
void ratesFor(const Mog2Ctx& c, int nf, int n, double learningRate, std::vector<float>& out)
{
    out.resize(n);
    for (int i = 0; i < n; i++) {
        if (nf < INT_MAX) ++nf;
        const double lr = (learningRate >= 0 && nf > 1) ? learningRate : 1.0 / (double)std::min<long long>(2LL * nf, c.history);
        out[i] = (float)lr;
    }
}

int runApply(const char* entry, void* ctx, const uchar* src, size_t sstep, size_t sframe, uchar* mask, size_t mstep, size_t mframe, int nframes, int w, int h, int type,
             double learningRate)
{
    Mog2Ctx* c = ctxOf(ctx);
    if (const int rc = applyArgs(c, src, sstep, sframe, mask, mstep, mframe, nframes, w, h, type)) return rc;
    const bool reinit = c->nframes == 0 || !c->buf || learningRate >= 1 || w != c->w || h != c->h || type != c->type || c->mixChanged || c->modelMix != c->nmixtures;
    std::vector<float> alphaT;
    ratesFor(*c, reinit ? 0 : c->nframes, nframes, learningRate, alphaT);
    const size_t rowb = (size_t)w * typeCn(type) * depthBytes(typeDepth(type));

    if (nframes > 1 && hostBatchEligible(src, mask, nframes)) {        // frames in host memory: chunks through two sets of device buffers, the model stays in HBM
        MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_HEAVY)));
        Stager stg;
        MI355_DECLINE_IF(!ensureDevice());
        if (!reinit) MI355_DECLINE_IF(c->device != activeDevice());
        if (reinit) {
            if (!allocModel(*c, w, h, type, c->nmixtures)) return MI355_DECLINED("hipMalloc of the model planes failed");
            c->mixChanged = false; c->nframes = 0;
            if (hipMemsetAsync(c->md.modes, 0, c->md.plane, stream()) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: hipMemsetAsync failed", entry);
        }
        int done = 0;
        const HostBatch hb = {src, sstep, sframe, rowb, h, mask, mstep, mframe, (size_t)w, h, nframes};
        const int rc = runHostBatch(entry, hb, [&](const uchar* s, size_t ss, size_t sf, uchar* d, size_t ds, size_t df, int nf) {
            launchFrames(*c, s, ss, sf, d, ds, df, nf, alphaT.data() + done);
            MI355_CHECK_LAUNCH(entry);
            done += nf;
            return (int)MI355CV_OK; });
        c->nframes = (int)std::min<long long>((long long)c->nframes + done, INT_MAX);
        return rc;
    }

    Stager stg;                                  // first: a declined call must also put the host's device back (~Stager)
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(hostImageTooSmall(src, (size_t)w * h, minPixels(HOST_HEAVY)));
    const size_t sspan = (size_t)(nframes - 1) * sframe + (size_t)(h - 1) * sstep + rowb, mspan = (size_t)(nframes - 1) * mframe + (size_t)(h - 1) * mstep + (size_t)w;
    MI355_DECLINE_IF(overlapOnDevice(src, sspan, mask, mspan));
    if (!reinit) MI355_DECLINE_IF(c->device != activeDevice());
    size_t dss = sstep, dms = mstep;
    const uchar* ds = src; uchar* dm = mask;
    if (nframes == 1) {
        ds = stg.in(src, sstep, rowb, h, &dss);
        dm = stg.out(mask, mstep, (size_t)w, h, &dms);
        MI355_DECLINE_IF(!ds || !dm);
    } else MI355_DECLINE_IF(!isDevicePtr(src) || !isDevicePtr(mask));
    if (reinit) {
        if (!allocModel(*c, w, h, type, c->nmixtures)) return MI355_DECLINED("hipMalloc of the model planes failed");
        c->mixChanged = false; c->nframes = 0;
        if (hipMemsetAsync(c->md.modes, 0, c->md.plane, stream()) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "%s: hipMemsetAsync failed", entry);
    }
    launchFrames(*c, ds, dss, sframe, dm, dms, mframe, nframes, alphaT.data());
    MI355_CHECK_LAUNCH(entry);
    c->nframes = (int)std::min<long long>((long long)c->nframes + nframes, INT_MAX);
    return stg.finish(entry);
}

// GetBackgroundImage / GetModel: a model must exist and have the geometry asked for
int modelArgs(const Mog2Ctx* c, int w, int h, int type)
{
    MI355_DECLINE_IF(disabled());
    MI355_DECLINE_IF(!c);
    MI355_DECLINE_IF(!c->buf || c->nframes == 0);
    MI355_DECLINE_IF(w != c->w || h != c->h || type != c->type);
    return 0;
}

struct ParamRef { const char* name; int kind; size_t off; };       // kind 0: float, 1: int
#define MOG2_P(n, k, f) {n, k, offsetof(Mog2Ctx, f)}
const ParamRef PARAMS[] = {MOG2_P("history", 1, history), MOG2_P("nmixtures", 1, nmixtures), MOG2_P("varThreshold", 0, Tb), MOG2_P("backgroundRatio", 0, TB),
                           MOG2_P("varThresholdGen", 0, Tg), MOG2_P("varInit", 0, varInit), MOG2_P("varMin", 0, varMin), MOG2_P("varMax", 0, varMax),
                           MOG2_P("complexityReductionThreshold", 0, CT), MOG2_P("detectShadows", 1, detectShadows), MOG2_P("shadowValue", 1, shadowValue),
                           MOG2_P("shadowThreshold", 0, tau)};
#undef MOG2_P
const ParamRef* findParam(const char* name)
{
    if (!name) return nullptr;
    for (const ParamRef& p : PARAMS) if (!strcmp(name, p.name)) return &p;
    return nullptr;
}

} // namespace

extern "C" {

MI355CV_API int mi355cv_mog2Create(void** ctx, int history, double varThreshold, int detectShadows)
{
    mi355::EntryGuard entry_(__func__);
    MI355_DECLINE_IF(disabled() || !ctx);
    MI355_DECLINE_IF(history < 1);
    Mog2Ctx* c = new (std::nothrow) Mog2Ctx();
    MI355_DECLINE_IF(!c);
    c->history = history; c->Tb = (float)varThreshold; c->detectShadows = detectShadows ? 1 : 0;
    *ctx = c;
    return MI355CV_OK;
}

MI355CV_API int mi355cv_mog2Free(void* ctx)
{
    mi355::EntryGuard entry_(__func__);
    Mog2Ctx* c = ctxOf(ctx);
    if (!c) return MI355CV_OK;
    if (c->buf) {
        Stager stg;                              // the model goes on the device that owns it
        if (ensureDevice()) freeModel(*c);
    }
    c->magic = 0;
    delete c;
    return MI355CV_OK;
}

MI355CV_API int mi355cv_mog2SetParam(void* ctx, const char* name, double v)
{
    mi355::EntryGuard entry_(__func__);
    Mog2Ctx* c = ctxOf(ctx);
    const ParamRef* p = findParam(name);
    MI355_DECLINE_IF(!c || !p);
    if (!strcmp(name, "nmixtures")) MI355_DECLINE_IF(!(v >= 1 && v <= lim::MOG2_MAX_MIXTURES));
    if (!strcmp(name, "history")) MI355_DECLINE_IF(!(v >= 1 && v <= INT_MAX));
    if (!strcmp(name, "shadowValue")) MI355_DECLINE_IF(!(v >= 0 && v <= 255));
    if (p->kind == 1) {
        int& f = *(int*)((char*)c + p->off);
        const int nv = !strcmp(name, "detectShadows") ? (v != 0) : (int)v;
        if (!strcmp(name, "nmixtures")) c->mixChanged = true;      // setNMixtures re-initialises at the next apply, whatever the value
        f = nv;
    } else *(float*)((char*)c + p->off) = (float)v;
    return MI355CV_OK;
}

MI355CV_API int mi355cv_mog2GetParam(void* ctx, const char* name, double* v)
{
    mi355::EntryGuard entry_(__func__);
    Mog2Ctx* c = ctxOf(ctx);
    const ParamRef* p = findParam(name);
    MI355_DECLINE_IF(!c || !p || !v);
    *v = p->kind == 1 ? (double)*(int*)((char*)c + p->off) : (double)*(float*)((char*)c + p->off);
    return MI355CV_OK;
}

// Host-resident frames are staged (HOST_HEAVY): the model stays in HBM either way, and the reference's CPU path streams ~100 bytes of model per pixel each way.
MI355CV_API int mi355cv_mog2Apply(void* ctx, const uchar* src, size_t src_step, uchar* mask, size_t mask_step, int width, int height, int type, double learningRate)
{
    mi355::EntryGuard entry_(__func__);
    return runApply("mog2Apply", ctx, src, src_step, 0, mask, mask_step, 0, 1, width, height, type, learningRate);
}

MI355CV_API int mi355cv_mog2ApplyBatch(void* ctx, const uchar* src, size_t src_step, size_t src_frame_stride, uchar* mask, size_t mask_step, size_t mask_frame_stride,
                                       int nframes, int width, int height, int type, double learningRate)
{
    mi355::EntryGuard entry_(__func__);
    return runApply("mog2ApplyBatch", ctx, src, src_step, nframes == 1 ? 0 : src_frame_stride, mask, mask_step, nframes == 1 ? 0 : mask_frame_stride, nframes, width, height,
                    type, learningRate);
}

MI355CV_API int mi355cv_mog2GetBackgroundImage(void* ctx, uchar* dst, size_t dst_step, int width, int height, int type)
{
    mi355::EntryGuard entry_(__func__);
    Mog2Ctx* c = ctxOf(ctx);
    if (const int rc = modelArgs(c, width, height, type)) return rc;
    const size_t e = depthBytes(typeDepth(type)), rowb = (size_t)width * typeCn(type) * e;
    MI355_DECLINE_IF(!dst || dst_step < rowb || (((uintptr_t)dst | dst_step) & (e - 1)));
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(c->device != activeDevice());
    size_t dds;
    uchar* dd = stg.out(dst, dst_step, rowb, height, &dds);
    MI355_DECLINE_IF(!dd);
    const int npix = c->w * c->h;
    const dim3 grid((unsigned)divUp(npix, 256));
    const mog2::Params P = paramsOf(*c);
    hipStream_t st = stream();
    switch (type) {
    case MI355CV_8U:      hipLaunchKernelGGL((k_mog2_background<uchar, 1>), grid, dim3(256), 0, st, dd, dds, c->w, npix, c->md, P); break;
    case MI355CV_8U + 16: hipLaunchKernelGGL((k_mog2_background<uchar, 3>), grid, dim3(256), 0, st, dd, dds, c->w, npix, c->md, P); break;
    case MI355CV_32F:     hipLaunchKernelGGL((k_mog2_background<float, 1>), grid, dim3(256), 0, st, dd, dds, c->w, npix, c->md, P); break;
    default:              hipLaunchKernelGGL((k_mog2_background<float, 3>), grid, dim3(256), 0, st, dd, dds, c->w, npix, c->md, P); break;
    }
    MI355_CHECK_LAUNCH("mog2GetBackgroundImage");
    noteKernel("k_mog2_background<type %d> grid=%u x256", type, grid.x);
    return stg.finish("mog2GetBackgroundImage");
}

MI355CV_API int mi355cv_mog2GetModel(void* ctx, uchar* modesUsed, float* gmm, float* mean)
{
    mi355::EntryGuard entry_(__func__);
    Mog2Ctx* c = ctxOf(ctx);
    if (const int rc = modelArgs(c, c ? c->w : 0, c ? c->h : 0, c ? c->type : -1)) return rc;
    MI355_DECLINE_IF(!modesUsed || !gmm || !mean);
    Stager stg;
    MI355_DECLINE_IF(!ensureDevice());
    MI355_DECLINE_IF(c->device != activeDevice());
    const int cn = typeCn(c->type), nmix = c->modelMix, npix = c->w * c->h;
    // the export writes dense arrays; a destination in host memory gets its array through scratch and one copy
    const size_t bytes[3] = {(size_t)npix, (size_t)npix * nmix * 2 * sizeof(float), (size_t)npix * nmix * cn * sizeof(float)};
    void* const user[3] = {modesUsed, gmm, mean};
    void* dev[3];
    for (int i = 0; i < 3; i++) {
        const int kind = ptrKind(user[i]);
        MI355_DECLINE_IF(kind == PTR_FOREIGN);
        dev[i] = kind == PTR_DEVICE ? user[i] : stg.scratch(bytes[i]);
        MI355_DECLINE_IF(!dev[i]);
    }
    hipStream_t st = stream();
    const dim3 grid((unsigned)divUp(npix, 256));
    if (cn == 1) hipLaunchKernelGGL((k_mog2_export<1>), grid, dim3(256), 0, st, (uchar*)dev[0], (float*)dev[1], (float*)dev[2], npix, nmix, c->md);
    else         hipLaunchKernelGGL((k_mog2_export<3>), grid, dim3(256), 0, st, (uchar*)dev[0], (float*)dev[1], (float*)dev[2], npix, nmix, c->md);
    MI355_CHECK_LAUNCH("mog2GetModel");
    bool anyHost = false;
    for (int i = 0; i < 3; i++)
        if (dev[i] != user[i]) {
            anyHost = true;
            if (hipMemcpyAsync(user[i], dev[i], bytes[i], hipMemcpyDeviceToHost, st) != hipSuccess)
                return setError(MI355CV_ERROR_UNKNOWN, "mog2GetModel: D2H failed: %s", hipGetErrorString(hipGetLastError()));
            noteStagedBytes((long long)bytes[i]);
        }
    if (anyHost && hipStreamSynchronize(st) != hipSuccess) return setError(MI355CV_ERROR_UNKNOWN, "mog2GetModel: %s", hipGetErrorString(hipGetLastError()));
    noteKernel("k_mog2_export<%d> grid=%u x256", cn, grid.x);
    return stg.finish("mog2GetModel");
}

} // extern "C"
