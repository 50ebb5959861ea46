// sgbm_emu.cpp -- opencv_amd/csrc/sgbm_math.h (the pieces of the kernels of sgbm.hip) compiled for the CPU: the prefiltered pixel, the packed Birchfield-Tomasi costs,
// the block sums, the path enumeration with one step of the recurrence, the decision and the left-right key, for tests/test_sgbm_cpu.py to hold against
// tests/sgbm_restate.py bit for bit, stage by stage.
#include "sgbm_math.h"
#include <vector>

extern "C" void emu_sgbm_geom(int W, int m, int n, int* out)
{
    const sgbm::Geom g = sgbm::geomOf(W, m, n);
    out[0] = g.xlo; out[1] = g.xhi; out[2] = g.W1; out[3] = g.Dmax; out[4] = g.filtered;
}

extern "C" int emu_sgbm_ft(int cap) { return sgbm::ftOf(cap); }
extern "C" long long emu_sgbm_bound(int w, int ft, int P2) { return sgbm::costBound(w, ft, P2); }
extern "C" unsigned long long emu_sgbm_frame_scratch(int W, int H, int W1, int n) { return sgbm::frameScratch(W, H, W1, n); }

// dense rows
extern "C" void emu_sgbm_prefilter(const uint8_t* src, int W, int H, int ft, uint8_t* dst)
{
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            dst[(size_t)y * W + x] = sgbm::prefilterPixel(src + (size_t)sgbm::maxi(y - 1, 0) * W, src + (size_t)y * W, src + (size_t)sgbm::mini(y + 1, H - 1) * W, x, W, ft);
}

// pc: H x W1 x n ints from the prefiltered planes GL, GR and the raw images IL, IR
extern "C" void emu_sgbm_pixel_cost(const uint8_t* GL, const uint8_t* GR, const uint8_t* IL, const uint8_t* IR, int W, int H, int m, int n, int* pc)
{
    const sgbm::Geom g = sgbm::geomOf(W, m, n);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < g.W1; x++)
            for (int k = 0; k < n; k++) {
                const size_t row = (size_t)y * W;
                const int X = g.xlo + x, XR = X - (k + m);
                pc[((size_t)y * g.W1 + x) * n + k] = sgbm::pixelCost(sgbm::btPackAt(GL + row, X, W), sgbm::btPackAt(GR + row, XR, W), sgbm::btPackAt(IL + row, X, W), sgbm::btPackAt(IR + row, XR, W));
            }
}

// the cost kernel's order: vertical sums of clamped rows per clamped window column, then the w columns of a window
extern "C" void emu_sgbm_block_cost(const int* pc, int W1, int H, int n, int w, int* C)
{
    const int h = w / 2;
    std::vector<int> V((size_t)W1 * n);
    for (int y = 0; y < H; y++) {
        for (int u = 0; u < W1; u++)
            for (int k = 0; k < n; k++) {
                int s = 0;
                for (int dy = -h; dy <= h; dy++) s += pc[((size_t)sgbm::clampi(y + dy, 0, H - 1) * W1 + u) * n + k];
                V[(size_t)u * n + k] = s;
            }
        for (int x = 0; x < W1; x++)
            for (int k = 0; k < n; k++) {
                int s = 0;
                for (int dx = -h; dx <= h; dx++) s += V[(size_t)sgbm::clampi(x + dx, 0, W1 - 1) * n + k];
                C[((size_t)y * W1 + x) * n + k] = s;
            }
    }
}

// S += L_r for every direction of the mode, walking pathOf's enumeration; visits: how often each pixel was visited per direction (must be 1)
extern "C" void emu_sgbm_aggregate(const int* C, int W1, int H, int n, int P1, int P2, int mode, int* S, int* visits)
{
    std::vector<int> prev(n + 2), cur(n + 2);
    for (int i = 0; i < sgbm::dirCount(mode); i++) {
        int ry, rx;
        sgbm::dirOf(mode, i, &ry, &rx);
        for (int idx = 0; idx < sgbm::pathCount(ry, rx, W1, H); idx++) {
            const sgbm::Path P = sgbm::pathOf(ry, rx, W1, H, idx);
            long long p = P.p0;
            for (int t = 0; t < P.count; t++, p += P.dp) {
                int M = sgbm::BIG;
                for (int k = 0; k < n; k++) M = sgbm::mini(M, prev[k + 1]);
                cur[0] = cur[n + 1] = sgbm::BIG;
                for (int k = 0; k < n; k++) {
                    const int c = C[(size_t)p * n + k];
                    cur[k + 1] = t ? sgbm::pathStep(c, prev[k + 1], prev[k], prev[k + 2], M, P1, P2) : c;
                    S[(size_t)p * n + k] += cur[k + 1];
                }
                visits[(size_t)i * W1 * H + p]++;
                prev = cur;
            }
        }
    }
}

// the decision as k_sgbm_decide takes it: 16 partial keys, their minimum, the uniqueness votes, the value; win = NOT_KEPT or (ms << 8 | best)
extern "C" void emu_sgbm_decide(const int* S, int W1, int H, int m, int n, int uniq, int* d, unsigned* win)
{
    const int filtered = (m - 1) * 16;
    for (size_t pix = 0; pix < (size_t)W1 * H; pix++) {
        const int* s = S + pix * n;
        uint32_t key = 0xffffffffu;
        for (int sub = 0; sub < 16; sub++) {
            uint32_t part = 0xffffffffu;
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) {
                    const int k = 64 * i + 4 * sub + j;                 // the kernel's lanes: four neighbours of every 64
                    if (64 * i + 4 * sub >= n) continue;
                    const uint32_t q = sgbm::minKey((uint32_t)s[k], k);
                    if (q < part) part = q;
                }
            if (part < key) key = part;
        }
        const int ms = sgbm::keyCost(key), best = sgbm::keyIndex(key);
        bool bad = false;
        if (uniq > 0) for (int k = 0; k < n; k++) bad |= sgbm::uniqFails(s[k], k, best, ms, uniq);
        d[pix] = bad ? filtered : sgbm::disparity16(best, ms, best > 0 ? s[best - 1] : 0, best < n - 1 ? s[best + 1] : 0, n, m);
        win[pix] = bad ? sgbm::NOT_KEPT : sgbm::winOf(ms, best);
    }
}

// the votes arrive in the order x = start, start + stride, ... (mod W1): the result must not depend on it.  d, win: H x W1 (valid columns); out: H x W1
extern "C" void emu_sgbm_leftright(const int* d, const unsigned* win, int W, int H, int m, int n, int disp12MaxDiff, int stride, int* out)
{
    const sgbm::Geom g = sgbm::geomOf(W, m, n);
    std::vector<unsigned long long> keys(W);
    for (int y = 0; y < H; y++) {
        for (auto& k : keys) k = sgbm::LR_NONE;
        for (int j = 0; j < g.W1; j++) {
            const int x = (int)(((long long)j * stride + 3) % g.W1), X = g.xlo + x;
            const unsigned wv = win[(size_t)y * g.W1 + x];
            if (wv == sgbm::NOT_KEPT) continue;
            const int best = sgbm::keyIndex(wv), x2 = X - (best + m);
            if (x2 < 0 || x2 >= W) continue;
            const unsigned long long key = sgbm::lrKey(sgbm::keyCost(wv), X, best);
            if (key < keys[x2]) keys[x2] = key;
        }
        const unsigned long long* kp = keys.data();
        for (int x = 0; x < g.W1; x++) {
            int v = d[(size_t)y * g.W1 + x];
            if (win[(size_t)y * g.W1 + x] != sgbm::NOT_KEPT && sgbm::lrRejects([kp, m](int xk) { return sgbm::lrDisp(kp[xk], m); }, g.xlo + x, v, W, m, disp12MaxDiff)) v = g.filtered;
            out[(size_t)y * g.W1 + x] = v;
        }
    }
}

extern "C" int emu_sgbm_disparity16(int best, int ms, int sm, int sp, int n, int m) { return sgbm::disparity16(best, ms, sm, sp, n, m); }

extern "C" int emu_sgbm_limit(int which)
{
    const int v[] = {sgbm::MAX_DIM, sgbm::MAX_DISPARITIES, sgbm::MAX_COST, sgbm::MAX_SCRATCH_MIB, sgbm::TILE, sgbm::STRIP, sgbm::CHUNK, sgbm::PATH_BLOCK};
    return which >= 0 && which < 8 ? v[which] : -1;
}
