// stereobm_emu.cpp -- opencv_amd/csrc/stereobm_math.h (the per-pixel pieces of the kernels of stereobm.hip) compiled for the CPU: the XSOBEL pixel, the column clamps,
// the decision -- serial as the generic kernel runs it and in chunks as the fast kernel does -- and the left-right key, for tests/test_stereobm_cpu.py to hold against
// tests/stereobm_restate.py bit for bit, stage by stage.
#include "stereobm_math.h"
#include <vector>

extern "C" void emu_sbm_geom(int W, int m, int n, int* out)
{
    const sbm::Geom g = sbm::geomOf(W, m, n);
    out[0] = g.xlo; out[1] = g.xhi; out[2] = g.rlo; out[3] = g.rhi; out[4] = g.Dmax; out[5] = g.filtered;
}

// dense rows
extern "C" void emu_sbm_prefilter(const uint8_t* src, int W, int H, int cap, uint8_t* dst)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            dst[(size_t)y * W + x] = sbm::xsobelPixel(src + (size_t)sbm::reflect101(y - 1, H) * W, src + (size_t)y * W, src + (size_t)sbm::reflect101(y + 1, H) * W, x, W, cap);
}

// sad: H x W x n ints, index i = Dmax - D; T: H x W ints; columns outside [xlo, xhi) are left alone
extern "C" void emu_sbm_volumes(const uint8_t* PL, const uint8_t* PR, int W, int H, int m, int n, int w, int cap, int* sad, int* T)
{
    const sbm::Geom g = sbm::geomOf(W, m, n);
    const int h = w / 2;
    for (int y = 0; y < H; y++)
        for (int X = g.xlo; X < g.xhi; X++) {
            for (int i = 0; i <= n; i++) {
                uint32_t s = 0;
                for (int dy = -h; dy <= h; dy++) {
                    const size_t row = (size_t)sbm::clampi(y + dy, 0, H - 1) * W;
                    for (int dx = -h; dx <= h; dx++) {
                        const uint32_t a = PL[row + sbm::leftCol(X + dx, W)];
                        s = sbm::absdiffAcc(a, i < n ? (uint32_t)PR[row + sbm::rightCol(X + dx, g.Dmax - i, g)] : (uint32_t)cap, s);
                    }
                }
                if (i < n) sad[((size_t)y * W + X) * n + i] = (int)s; else T[(size_t)y * W + X] = (int)s;
            }
        }
}

// chunked != 0: the pieces in the order of the fast kernel (a minimum per chunk of 16, the pixel's minimum, uniqueness votes per chunk)
extern "C" void emu_sbm_decide(const int* sad, const int* T, int W, int H, int m, int n, int tex, int uniq, int chunked, short* d, int* winCost)
{
    const sbm::Geom g = sbm::geomOf(W, m, n);
    for (int y = 0; y < H; y++)
        for (int X = 0; X < W; X++) {
            const size_t px = (size_t)y * W + X;
            if (X < g.xlo || X >= g.xhi) { d[px] = (short)g.filtered; winCost[px] = 0; continue; }
            const int* c = sad + px * n;
            int win = 0, v;
            if (!chunked) v = sbm::decide([c](int i) { return c[i]; }, n, T[px], tex, uniq, g, &win);
            else {
                std::vector<uint32_t> part(n / sbm::ROLL_CHUNK, 0xffffffffu);
                for (int k = 0; k < n / sbm::ROLL_CHUNK; k++)
                    for (int j = 0; j < sbm::ROLL_CHUNK; j++) { const uint32_t key = sbm::minKey((uint32_t)c[k * sbm::ROLL_CHUNK + j], k * sbm::ROLL_CHUNK + j); if (key < part[k]) part[k] = key; }
                uint32_t best = 0xffffffffu;
                for (uint32_t p : part) if (p < best) best = p;
                const int ms = sbm::keyCost(best), mi = sbm::keyIndex(best);
                bool rej = false;
                if (uniq > 0)
                    for (int k = 0; k < n / sbm::ROLL_CHUNK; k++) {
                        uint32_t mo = sbm::NO_COST;
                        for (int j = 0; j < sbm::ROLL_CHUNK; j++) { const uint32_t o = sbm::outsideCost(k * sbm::ROLL_CHUNK + j, mi, (uint32_t)c[k * sbm::ROLL_CHUNK + j]); if (o < mo) mo = o; }
                        rej |= sbm::uniqRejects(mo, ms, uniq);
                    }
                win = ms;
                v = (T[px] < tex || rej) ? g.filtered : sbm::subpixel(ms, c[sbm::nextIndex(mi, n)], c[sbm::prevIndex(mi)], g.Dmax, mi);
                if (T[px] < tex) win = 0;
            }
            d[px] = (short)v; winCost[px] = win;
        }
}

// the votes arrive in the order x = start, start + stride, ... (mod W): the result must not depend on it
extern "C" void emu_sbm_leftright(const short* d, const int* cost, int W, int H, int m, int n, int disp12MaxDiff, int stride, short* out)
{
    const sbm::Geom g = sbm::geomOf(W, m, n);
    std::vector<unsigned long long> keys(W);
    for (int y = 0; y < H; y++) {
        const short* dr = d + (size_t)y * W;
        for (auto& k : keys) k = sbm::LR_NONE;
        for (int j = 0; j < W; j++) {
            const int x = (int)(((long long)j * stride + 3) % W);
            if (dr[x] == g.filtered) continue;
            const int x2 = sbm::lrTarget(x, dr[x]);
            if (x2 < 0 || x2 >= W) continue;
            const unsigned long long key = sbm::lrKey(cost[(size_t)y * W + x], x, dr[x]);
            if (key < keys[x2]) keys[x2] = key;
        }
        const unsigned long long* kp = keys.data();
        const int filtered = g.filtered;
        for (int x = 0; x < W; x++) {
            short v = dr[x];
            if (v != g.filtered && sbm::lrRejects([kp, filtered](int xk) { return sbm::lrDisp(kp[xk], filtered); }, x, v, W, disp12MaxDiff, filtered)) v = (short)filtered;
            out[(size_t)y * W + x] = v;
        }
    }
}

extern "C" int emu_sbm_subpixel(int ms, int p, int nn, int Dmax, int mi) { return sbm::subpixel(ms, p, nn, Dmax, mi); }

extern "C" int emu_sbm_limit(int which)
{
    const int v[] = {sbm::MAX_DIM, sbm::MAX_DISPARITIES, sbm::MAX_BLOCK, sbm::ROLL_MAX_BLOCK, sbm::ROLL_CHUNK, sbm::ROLL_TILE, sbm::ROLL_STRIP, sbm::GENERIC_TILE};
    return which >= 0 && which < 8 ? v[which] : -1;
}
