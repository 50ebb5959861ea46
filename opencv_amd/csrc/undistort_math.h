// undistort_math.h -- the arithmetic of undistort.hip (cv::initUndistortRectifyMap, cv::undistort, the rectifying warp, cv::reprojectImageTo3D), __host__ __device__
// and free of wave intrinsics so that tests/hostemu/undistort_emu.cpp runs the very same lines on the CPU, thread by thread, against tests/undistort_restate.py
// (DESIGN 6.21).  Every floating-point step is a separately rounded IEEE double operation (dmul / dadd / ddiv of warp8.h: the __d*_rn intrinsics on the device, plain
// operators under -ffp-contract=off on the host), in the association the restatement spells out.
//
//   inverse3x3    ir = (newK R)^-1 on the host, once per call: the product row by row, the adjugate, one reciprocal of the determinant
//   mapUV         the map rule of one destination pixel (j = column, i = row) -> (u, v) in source pixels
//   satIntND      round half to even, clamp to int, INT_MIN for a non-finite argument (tested first, on both sides)
//   fixedOf       (u, v) -> the CV_16SC2 entry and the CV_16UC1 fraction word of cv::convertMaps' fixed-point form
//   reprojPoint   one pixel of reprojectImageTo3D
//   the tile kernel's phases: coords (a lane's 4 x steps pixels, kept in registers), boxOf (the exact source box from the reduced extremes), sampleTile (from the LDS
//   tile staged by warp8::stage, (Q + 512) >> 10 by warp8::bilinearOf), sampleGeneric8 (the per-pixel sampler of the rim, the border rules and oversized boxes)
#pragma once
#include "hd.h"
#include "warp8.h"

namespace und {

using warp8::dadd;
using warp8::ddiv;
using warp8::dmul;

enum { B_CONSTANT = 0, B_REPLICATE = 1, B_REFLECT = 2, B_WRAP = 3, B_REFLECT_101 = 4 };
enum { TILE_OFF = 64 };                         // bytes of LDS in front of the source tile: the waves' extremes (4 waves x 4 ints)

// what a pixel needs of the call: ir, the distortion terms k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, the camera's fx fy u0 v0
struct Rule { double ir[9]; double k[12]; double fx, fy, u0, v0; };

// ir = (newK R)^-1; -> false when the determinant is 0 or not finite (ir untouched then).  A = newK R: A[r][c] = (nK[r][0] R[0][c] + nK[r][1] R[1][c]) + nK[r][2] R[2][c];
// det = (a C0 + b C1) + c C2 over the first row's cofactors; ir = adjugate times (1 / det), each entry one product
MI355_HD_PLAIN bool inverse3x3(const double* nK, const double* R, double* ir)
{
    double A[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            A[3 * r + c] = dadd(dadd(dmul(nK[3 * r], R[c]), dmul(nK[3 * r + 1], R[3 + c])), dmul(nK[3 * r + 2], R[6 + c]));
    const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5], g = A[6], h = A[7], i = A[8];
    const double C0 = dadd(dmul(e, i), -dmul(f, h)), C1 = dadd(dmul(f, g), -dmul(d, i)), C2 = dadd(dmul(d, h), -dmul(e, g));
    const double det = dadd(dadd(dmul(a, C0), dmul(b, C1)), dmul(c, C2));
    if (det == 0 || !(det - det == 0)) return false;
    const double id = ddiv(1.0, det);
    ir[0] = dmul(C0, id); ir[1] = dmul(dadd(dmul(c, h), -dmul(b, i)), id); ir[2] = dmul(dadd(dmul(b, f), -dmul(c, e)), id);
    ir[3] = dmul(C1, id); ir[4] = dmul(dadd(dmul(a, i), -dmul(c, g)), id); ir[5] = dmul(dadd(dmul(c, d), -dmul(a, f)), id);
    ir[6] = dmul(C2, id); ir[7] = dmul(dadd(dmul(b, g), -dmul(a, h)), id); ir[8] = dmul(dadd(dmul(a, e), -dmul(b, d)), id);
    return true;
}

MI355_HD void mapUV(const Rule& q, int j, int i, double& u, double& v)
{
    const double dj = (double)j, di = (double)i;
    const double _x = dadd(dmul(dj, q.ir[0]), dadd(dmul(di, q.ir[1]), q.ir[2]));
    const double _y = dadd(dmul(dj, q.ir[3]), dadd(dmul(di, q.ir[4]), q.ir[5]));
    const double _w = dadd(dmul(dj, q.ir[6]), dadd(dmul(di, q.ir[7]), q.ir[8]));
    const double w = ddiv(1.0, _w), x = dmul(_x, w), y = dmul(_y, w);
    const double x2 = dmul(x, x), y2 = dmul(y, y), r2 = dadd(x2, y2), _2xy = dmul(dmul(2.0, x), y);
    const double k1 = q.k[0], k2 = q.k[1], p1 = q.k[2], p2 = q.k[3], k3 = q.k[4], k4 = q.k[5], k5 = q.k[6], k6 = q.k[7], s1 = q.k[8], s2 = q.k[9], s3 = q.k[10], s4 = q.k[11];
    const double num = dadd(1.0, dmul(dadd(dmul(dadd(dmul(k3, r2), k2), r2), k1), r2));
    const double den = dadd(1.0, dmul(dadd(dmul(dadd(dmul(k6, r2), k5), r2), k4), r2));
    const double kr = ddiv(num, den);
    const double xd = dadd(dadd(dadd(dadd(dmul(x, kr), dmul(p1, _2xy)), dmul(p2, dadd(r2, dmul(2.0, x2)))), dmul(s1, r2)), dmul(dmul(s2, r2), r2));
    const double yd = dadd(dadd(dadd(dadd(dmul(y, kr), dmul(p1, dadd(r2, dmul(2.0, y2)))), dmul(p2, _2xy)), dmul(s3, r2)), dmul(dmul(s4, r2), r2));
    u = dadd(dmul(q.fx, xd), q.u0);
    v = dadd(dmul(q.fy, yd), q.v0);
}

MI355_HD int satIntND(double v)
{
    unsigned long long bits;
    __builtin_memcpy(&bits, &v, 8);
    if ((bits & 0x7FF0000000000000ull) == 0x7FF0000000000000ull) return (int)-2147483648LL;       // NaN, +-inf: what the reference's x86 conversion yields
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (int)-2147483648LL;
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__double2int_rn(v);
#else
    return (int)__builtin_rint(v);                       // round half to even
#endif
}

// the coordinates of the fixed-point form in 1/32 px
MI355_HD void fixedUV(const Rule& q, int j, int i, int& iu, int& iv)
{
    double u, v;
    mapUV(q, j, i, u, v);
    iu = satIntND(dmul(u, 32.0)); iv = satIntND(dmul(v, 32.0));
}
// ... as map entries: (short)(iu >> 5) | (short)(iv >> 5) << 16, a plain wrap, and (iv & 31) * 32 + (iu & 31)
MI355_HD uint32_t entryOf(int iu, int iv) { return ((uint32_t)(iu >> 5) & 0xFFFFu) | ((uint32_t)(iv >> 5) << 16); }
MI355_HD uint32_t fracOf(int iu, int iv) { return (uint32_t)((iv & 31) * 32 + (iu & 31)); }

// ---- reprojectImageTo3D: h_r = ((Q[r][0] x + Q[r][1] y) + Q[r][2] d) + Q[r][3], point = (float)(h_r / h_3 as h_r * (1 / h_3)); missing: z = 10000
MI355_HD void reprojPoint(const double* Q, int x, int y, double d, bool missing, float* out)
{
    double h[4];
    for (int r = 0; r < 4; r++) h[r] = dadd(dadd(dadd(dmul(Q[4 * r], (double)x), dmul(Q[4 * r + 1], (double)y)), dmul(Q[4 * r + 2], d)), Q[4 * r + 3]);
    const double iw = ddiv(1.0, h[3]);
    out[0] = (float)dmul(h[0], iw); out[1] = (float)dmul(h[1], iw); out[2] = missing ? 10000.f : (float)dmul(h[2], iw);
}
MI355_HD bool isMissing(double d, double dmin)
{
    const double t = dadd(d, -dmin);
    return (t < 0 ? -t : t) <= 1.1920928955078125e-7;                                              // FLT_EPSILON
}
// a disparity element as a double: depth 0 CV_8U, 3 CV_16S, 4 CV_32S, 5 CV_32F
MI355_HD double dispAt(const unsigned char* row, int depth, int x)
{
    if (depth == 0) return (double)row[x];
    if (depth == 3) return (double)reinterpret_cast<const short*>(row)[x];
    if (depth == 4) return (double)reinterpret_cast<const int*>(row)[x];
    return (double)reinterpret_cast<const float*>(row)[x];
}

// ---- the tile kernel --------------------------------------------------------------------------------------------------------------------------------------
// cv::borderInterpolate; -1 under BORDER_CONSTANT
MI355_HD int borderIdx(int p, int len, int border)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (border == B_REPLICATE) return p < 0 ? 0 : len - 1;
    if (border == B_REFLECT || border == B_REFLECT_101) {
        const int delta = border == B_REFLECT_101;
        if (len == 1) return 0;
        do {
            if (p < 0) p = -p - 1 + delta;
            else p = len - 1 - (p - len) - delta;
        } while ((unsigned)p >= (unsigned)len);
        return p;
    }
    if (border == B_WRAP) {
        if (p < 0) p -= ((p - len + 1) / len) * len;
        if (p >= len) p %= len;
        return p;
    }
    return -1;
}

struct TileArgs {
    Rule rule;
    int sw, sh, dw, dh;
    uint32_t sstep, dstep;          // bytes
    unsigned long long sframe, dframe;
    int nframes, fpw;               // frames of the launch, frames a workgroup walks with the coordinates it holds
    int ldsBytes;                   // the source tile's allotment
    int border; uint32_t cval;      // the border value's channels as bytes
    int dwords;                     // both images and their pitches and frame strides on 4 bytes, below 4 GB: aligned dword staging and stores; 0: every pixel by the generic sampler
};

template <int CN> MI355_HD constexpr int steps() { return warp8::tileRows<CN>() / warp8::ROWS_PER_STEP; }

// A lane's pixels, the geometry of warp8: lane -> 4 adjacent columns x0 + 4 (lane & 31) .., rows y0 + 8 st + 2 wave + (lane >> 5).  pk = the map entry (sx | sy << 16),
// fr = ax | ay << 5; mm = the lane's (min sx, max sx, min sy, max sy).  A lane past the image's edge evaluates the edge pixel, which leaves the extremes alone.
template <int CN>
MI355_HD void coords(const TileArgs& a, int x0, int y0, int tid, uint32_t (&pk)[steps<CN>()][4], uint32_t (&fr)[steps<CN>()][4], int (&mm)[4])
{
    const int wave = tid >> 6, lane = tid & 63, lx = lane & 31, ly = lane >> 5;
    mm[0] = mm[2] = 32767; mm[1] = mm[3] = -32768;
    for (int st = 0; st < steps<CN>(); st++) {
        const int y = y0 + st * warp8::ROWS_PER_STEP + wave * 2 + ly, yc = y < a.dh ? y : a.dh - 1;
        for (int p = 0; p < 4; p++) {
            const int x = x0 + lx * 4 + p, xc = x < a.dw ? x : a.dw - 1;
            int iu, iv;
            fixedUV(a.rule, xc, yc, iu, iv);
            pk[st][p] = entryOf(iu, iv); fr[st][p] = (uint32_t)(iu & 31) | ((uint32_t)(iv & 31) << 5);
            const int sx = (short)(pk[st][p] & 0xFFFFu), sy = (int)pk[st][p] >> 16;
            mm[0] = sx < mm[0] ? sx : mm[0]; mm[1] = sx > mm[1] ? sx : mm[1];
            mm[2] = sy < mm[2] ? sy : mm[2]; mm[3] = sy > mm[3] ? sy : mm[3];
        }
    }
}

MI355_HD int tilePitch(int cx0, int cw, int cn) { return ((((cx0 * cn) & 3) + cw * cn + 3) & ~3) + 8; }

// The box of the tile's 2 x 2 footprints, [mnx, mxx + 1] x [mny, mxy + 1], clipped to the source (warp8::Box's conventions: cw == 0 nothing staged -- ch == -1: less
// than a footprint of source under the box, every pixel still classifiable; ch == 0: the box exceeds the allotment, the generic sampler takes the tile).  -> LDS pitch
template <int CN>
MI355_HD warp8::Box boxOf(const TileArgs& a, int mnx, int mxx, int mny, int mxy, int& pitch)
{
    warp8::Box b = {0, 0, 0, 0, 0, 0};
    const int bx1 = mxx + 1, by1 = mxy + 1;
    b.cx0 = mnx < 0 ? 0 : mnx; b.cy0 = mny < 0 ? 0 : mny;
    const int ex = bx1 > a.sw - 1 ? a.sw - 1 : bx1, ey = by1 > a.sh - 1 ? a.sh - 1 : by1;
    b.cw = ex - b.cx0 + 1; b.ch = ey - b.cy0 + 1;
    b.shift = (b.cx0 * CN) & 3;
    pitch = 0;
    if (b.cw < 2 || b.ch < 2) { b.cw = 0; b.ch = -1; b.shift = 0; return b; }
    pitch = tilePitch(b.cx0, b.cw, CN);
    if (!a.dwords || (long long)pitch * b.ch > (long long)a.ldsBytes) { b.cw = 0; b.ch = 0; b.shift = 0; pitch = 0; return b; }
    b.all = mnx >= 0 && mny >= 0 && bx1 <= a.sw - 1 && by1 <= a.sh - 1;
    return b;
}

// what warp8::stage reads of its Args
MI355_HD warp8::Args stageArgs(const TileArgs& a, int pitch)
{
    warp8::Args t = {};
    t.sw = a.sw; t.sh = a.sh; t.sstep = a.sstep; t.ldsPitch = pitch;
    t.pitchMagic = pitch ? 0xFFFFFFFFu / ((uint32_t)pitch >> 2) + 1u : 0u;             // dword index -> row by one mul_hi (indices stay below 2^16)
    return t;
}

// One pixel from HBM, the arithmetic of the fixed-point bilinear branch of k_warp: the four taps through cv::borderInterpolate (the border value's byte where
// BORDER_CONSTANT has none), (Q + 512) >> 10 -- equal to the Q15 table's (sum + 2^14) >> 15 on bytes (warp8.h).  A BORDER_CONSTANT pixel whose whole footprint is
// outside is the border value itself.
template <int CN>
MI355_HD void sampleGeneric8(const TileArgs& a, const unsigned char* src, int sx, int sy, int ax, int ay, unsigned char* D)
{
    if (a.border == B_CONSTANT && (sx >= a.sw || sx + 1 < 0 || sy >= a.sh || sy + 1 < 0)) {
        for (int k = 0; k < CN; k++) D[k] = (unsigned char)(a.cval >> (8 * k));
        return;
    }
    int x0, x1, y0, y1;
    if ((unsigned)sx < (unsigned)(a.sw - 1) && (unsigned)sy < (unsigned)(a.sh - 1)) { x0 = sx; x1 = sx + 1; y0 = sy; y1 = sy + 1; }
    else { x0 = borderIdx(sx, a.sw, a.border); x1 = borderIdx(sx + 1, a.sw, a.border); y0 = borderIdx(sy, a.sh, a.border); y1 = borderIdx(sy + 1, a.sh, a.border); }
    const unsigned char* r0 = src + (size_t)(y0 < 0 ? 0 : y0) * a.sstep;
    const unsigned char* r1 = src + (size_t)(y1 < 0 ? 0 : y1) * a.sstep;
    for (int k = 0; k < CN; k++) {
        const uint32_t cv = (a.cval >> (8 * k)) & 255u;
        const uint32_t v0 = (x0 >= 0 && y0 >= 0) ? r0[x0 * CN + k] : cv, v1 = (x1 >= 0 && y0 >= 0) ? r0[x1 * CN + k] : cv;
        const uint32_t v2 = (x0 >= 0 && y1 >= 0) ? r1[x0 * CN + k] : cv, v3 = (x1 >= 0 && y1 >= 0) ? r1[x1 * CN + k] : cv;
        const uint32_t Q = (v0 * (uint32_t)(32 - ax) + v1 * (uint32_t)ax) * (uint32_t)(32 - ay) + (v2 * (uint32_t)(32 - ax) + v3 * (uint32_t)ax) * (uint32_t)ay;
        D[k] = (unsigned char)((Q + 512u) >> 10);
    }
}

// The lane's pixels of one frame from the staged tile: four pixels of a row as one dword (12 / 16 bytes for 3 / 4 channels) when all four are sampled from the box
// or are BORDER_CONSTANT pixels wholly outside the source; otherwise the step's bit is set in the returned mask and redo() gives the group to the generic sampler.
template <int CN, bool ALL>
MI355_HD unsigned rowsOf(const TileArgs& a, const warp8::Box& b, int pitch, int x0, int y0, const unsigned char* tile, unsigned char* dst, int tid,
                         const uint32_t (&pk)[steps<CN>()][4], const uint32_t (&fr)[steps<CN>()][4])
{
    const int wave = tid >> 6, lane = tid & 63, lx = lane & 31, ly = lane >> 5;
    const int x = x0 + lx * 4;
    if (x >= a.dw) return 0;
    const bool fullLane = x + 4 <= a.dw, constBorder = a.border == B_CONSTANT;
    const uint32_t cwm = b.cw > 0 ? (uint32_t)(b.cw - 1) : 0u, chm = b.ch > 0 ? (uint32_t)(b.ch - 1) : 0u;
    const uint32_t cval = CN == 4 ? a.cval : a.cval & ((1u << (8 * (CN & 3))) - 1u);            // the border value's bytes of the channels there are
    unsigned redo = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int st = 0; st < steps<CN>(); st++) {
        const int y = y0 + st * warp8::ROWS_PER_STEP + wave * 2 + ly;
        uint32_t px[4], off[4], tap[4][4]; bool outp[4], ok = fullLane;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int p = 0; p < 4; p++) {
            const int sx = (short)(pk[st][p] & 0xFFFFu), sy = (int)pk[st][p] >> 16;
            const int rx = sx - b.cx0, ry = sy - b.cy0;
            off[p] = warp8::mad24((uint32_t)ry, (uint32_t)pitch, (uint32_t)(rx * CN + b.shift));
            outp[p] = false;
            if (!ALL) {
                const bool in = (uint32_t)rx < cwm && (uint32_t)ry < chm;
                outp[p] = constBorder && (sx >= a.sw || sx + 1 < 0 || sy >= a.sh || sy + 1 < 0);
                off[p] = in ? off[p] : 0u; ok = ok && (in || outp[p]);
            }
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int p = 0; p < 4; p++) warp8::fetchTaps<CN, 1>(tile + off[p], (uint32_t)pitch, tap[p]);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int p = 0; p < 4; p++) {
            const uint32_t ax = fr[st][p] & 31u, ay = fr[st][p] >> 5, wxa = ax | (ax << 16);
            px[p] = warp8::bilinearOf<CN>(tap[p], 0x00200020u - wxa, wxa, (32u - ay) | (ay << 16));
            if (!ALL) px[p] = outp[p] ? cval : px[p];
        }
        if (y < a.dh) {
            if (ok) {
                uint32_t* d = reinterpret_cast<uint32_t*>(dst + (size_t)y * a.dstep + (size_t)x * CN);
                if (CN == 1) d[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
                else if (CN == 3) { d[0] = px[0] | (px[1] << 24); d[1] = (px[1] >> 8) | (px[2] << 16); d[2] = (px[2] >> 16) | (px[3] << 8); }
                else { d[0] = px[0]; d[1] = px[1]; d[2] = px[2]; d[3] = px[3]; }
            } else redo |= 1u << st;
        }
    }
    return redo;
}

template <int CN>
MI355_HD unsigned sampleTile(const TileArgs& a, const warp8::Box& b, int pitch, int x0, int y0, const unsigned char* tile, unsigned char* dst, int tid,
                             const uint32_t (&pk)[steps<CN>()][4], const uint32_t (&fr)[steps<CN>()][4])
{
    if (b.cw == 0 && !(a.dwords && a.border == B_CONSTANT && b.ch == -1)) {             // nothing staged and nothing to classify: every group is redone
        const int x = x0 + ((tid & 63) & 31) * 4;
        return x < a.dw ? (1u << steps<CN>()) - 1 : 0;
    }
    return b.all ? rowsOf<CN, true>(a, b, pitch, x0, y0, tile, dst, tid, pk, fr) : rowsOf<CN, false>(a, b, pitch, x0, y0, tile, dst, tid, pk, fr);
}

template <int CN>
MI355_HD void redo(const TileArgs& a, unsigned mask, int x0, int y0, const unsigned char* src, unsigned char* dst, int tid, const uint32_t (&pk)[steps<CN>()][4],
                   const uint32_t (&fr)[steps<CN>()][4])
{
    const int wave = tid >> 6, lane = tid & 63, x = x0 + (lane & 31) * 4;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int st = 0; st < steps<CN>(); st++) {
        if (!((mask >> st) & 1)) continue;
        const int y = y0 + st * warp8::ROWS_PER_STEP + wave * 2 + (lane >> 5);
        if (y >= a.dh) continue;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int p = 0; p < 4; p++)
            if (x + p < a.dw)
                sampleGeneric8<CN>(a, src, (short)(pk[st][p] & 0xFFFFu), (int)pk[st][p] >> 16, (int)(fr[st][p] & 31u), (int)(fr[st][p] >> 5),
                                   dst + (size_t)y * a.dstep + (size_t)(x + p) * CN);
    }
}

} // namespace und
