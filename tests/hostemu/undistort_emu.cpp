// undistort_emu.cpp -- opencv_amd/csrc/undistort_math.h (the arithmetic of undistort.hip) compiled for the CPU with -ffp-contract=off: the inverse, the map rule, the
// saturating conversion, the three map forms, one pixel of reprojectImageTo3D, and the tile kernel put together as k_undist8_tile orders the work -- workgroup by
// workgroup, thread by thread: coordinates, the reduction of the extremes, the box, then per frame of the group staging, sampling and the generic sampler -- for
// tests/test_undistort_cpu.py to hold against tests/undistort_restate.py bit for bit, stage by stage.
#include "undistort_math.h"
#include <string.h>
#include <vector>

static und::Rule ruleOf(const double* ir, const double* k12, const double* cam4)
{
    und::Rule q;
    memcpy(q.ir, ir, sizeof q.ir); memcpy(q.k, k12, sizeof q.k);
    q.fx = cam4[0]; q.fy = cam4[1]; q.u0 = cam4[2]; q.v0 = cam4[3];
    return q;
}

extern "C" int emu_und_inverse(const double* newK, const double* R, double* ir) { return und::inverse3x3(newK, R, ir) ? 1 : 0; }
extern "C" int emu_und_sat(double v) { return und::satIntND(v); }

extern "C" void emu_und_uv(const double* ir, const double* k12, const double* cam4, int w, int h, double* u, double* v)
{
    const und::Rule q = ruleOf(ir, k12, cam4);
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) und::mapUV(q, j, i, u[(size_t)i * w + j], v[(size_t)i * w + j]);
}

// form 0: CV_32FC1 pair, 1: CV_32FC2 into m1, 2: CV_16SC2 into m1 + CV_16UC1 into m2; dense rows
extern "C" void emu_und_maps(const double* ir, const double* k12, const double* cam4, int w, int h, int form, void* m1, void* m2)
{
    const und::Rule q = ruleOf(ir, k12, cam4);
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            const size_t at = (size_t)i * w + j;
            if (form == 2) {
                int iu, iv;
                und::fixedUV(q, j, i, iu, iv);
                ((uint32_t*)m1)[at] = und::entryOf(iu, iv); ((uint16_t*)m2)[at] = (uint16_t)und::fracOf(iu, iv);
                continue;
            }
            double u, v;
            und::mapUV(q, j, i, u, v);
            if (form == 1) { ((float*)m1)[2 * at] = (float)u; ((float*)m1)[2 * at + 1] = (float)v; }
            else { ((float*)m1)[at] = (float)u; ((float*)m2)[at] = (float)v; }
        }
}

extern "C" void emu_und_reproject(const unsigned char* disp, int depth, int w, int h, const double* Q, int handleMissing, double dmin, float* out)
{
    const size_t esz = depth == 0 ? 1 : depth == 3 ? 2 : 4;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const double d = und::dispAt(disp + (size_t)y * w * esz, depth, x);
            und::reprojPoint(Q, x, y, d, handleMissing && und::isMissing(d, dmin), out + ((size_t)y * w + x) * 3);
        }
}

// the tile kernel on dense frames of `cn` channels; boxes (may be null): per tile, row by row, (mnx, mxx, mny, mxy, cw, ch)
template <int CN>
static void tileKernel(const und::Rule& q, const unsigned char* src, int sw, int sh, unsigned char* dst, int dw, int dh, int nframes, int fpw, int ldsBytes, int border,
                       uint32_t cval, int dwords, int* boxes)
{
    constexpr int NS = und::steps<CN>();
    und::TileArgs a;
    memset(&a, 0, sizeof a);
    a.rule = q; a.sw = sw; a.sh = sh; a.dw = dw; a.dh = dh; a.sstep = (uint32_t)(sw * CN); a.dstep = (uint32_t)(dw * CN);
    a.sframe = (unsigned long long)sw * sh * CN; a.dframe = (unsigned long long)dw * dh * CN;
    a.nframes = nframes; a.fpw = fpw; a.ldsBytes = ldsBytes; a.border = border; a.cval = cval; a.dwords = dwords;
    struct Lane { uint32_t pk[NS][4], fr[NS][4]; };
    std::vector<Lane> lanes(256);
    std::vector<uint32_t> lds((und::TILE_OFF + (size_t)(ldsBytes > 256 ? ldsBytes : 256)) / 4 + 4);
    unsigned char* tile = reinterpret_cast<unsigned char*>(lds.data()) + und::TILE_OFF;
    const int th = warp8::tileRows<CN>();
    for (int g = 0; g * fpw < nframes; g++)
        for (int y0 = 0, t = 0; y0 < dh; y0 += th)
            for (int x0 = 0; x0 < dw; x0 += warp8::TW, t++) {
                int ext[4] = {32767, -32768, 32767, -32768};
                for (int tid = 0; tid < 256; tid++) {
                    int mm[4];
                    und::coords<CN>(a, x0, y0, tid, lanes[tid].pk, lanes[tid].fr, mm);
                    ext[0] = mm[0] < ext[0] ? mm[0] : ext[0]; ext[1] = mm[1] > ext[1] ? mm[1] : ext[1];
                    ext[2] = mm[2] < ext[2] ? mm[2] : ext[2]; ext[3] = mm[3] > ext[3] ? mm[3] : ext[3];
                }
                int pitch;
                const warp8::Box b = und::boxOf<CN>(a, ext[0], ext[1], ext[2], ext[3], pitch);
                if (boxes && g == 0) { int* o = boxes + 6 * t; o[0] = ext[0]; o[1] = ext[1]; o[2] = ext[2]; o[3] = ext[3]; o[4] = b.cw; o[5] = b.ch; }
                const warp8::Args sa = und::stageArgs(a, pitch);
                for (int f = g * fpw; f < nframes && f < (g + 1) * fpw; f++) {
                    const unsigned char* S = src + (size_t)f * a.sframe;
                    unsigned char* D = dst + (size_t)f * a.dframe;
                    if (b.cw) for (int tid = 0; tid < 256; tid++) warp8::stage(sa, b, CN, S, tile, tid);
                    for (int tid = 0; tid < 256; tid++) {
                        const unsigned mask = und::sampleTile<CN>(a, b, pitch, x0, y0, tile, D, tid, lanes[tid].pk, lanes[tid].fr);
                        if (mask) und::redo<CN>(a, mask, x0, y0, S, D, tid, lanes[tid].pk, lanes[tid].fr);
                    }
                }
            }
}

extern "C" void emu_und_tile(const double* ir, const double* k12, const double* cam4, const unsigned char* src, int sw, int sh, int cn, unsigned char* dst, int dw, int dh,
                             int nframes, int fpw, int ldsBytes, int border, unsigned cval, int dwords, int* boxes)
{
    const und::Rule q = ruleOf(ir, k12, cam4);
    if (cn == 1) tileKernel<1>(q, src, sw, sh, dst, dw, dh, nframes, fpw, ldsBytes, border, cval, dwords, boxes);
    else if (cn == 3) tileKernel<3>(q, src, sw, sh, dst, dw, dh, nframes, fpw, ldsBytes, border, cval, dwords, boxes);
    else tileKernel<4>(q, src, sw, sh, dst, dw, dh, nframes, fpw, ldsBytes, border, cval, dwords, boxes);
}
