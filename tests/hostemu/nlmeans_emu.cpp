// nlmeans_emu.cpp -- opencv_amd/csrc/nlmeans_math.h (the pieces of the kernels of nlmeans.hip) compiled for the CPU: the reflected index, the geometry and the weight
// table, the patch distance, the final division, the rule put together from them as k_nlm_plain does, and the walk of k_nlm_tile lane by lane (the plane image, the
// ring of T rows, the sum over the lanes below), for tests/test_nlmeans_cpu.py to hold against tests/nlmeans_restate.py bit for bit, stage by stage.
#include "nlmeans_math.h"
#include <vector>

extern "C" int emu_nlm_reflect(int p, int len) { return nlm::reflect101(p, len); }

extern "C" void emu_nlm_geom(int tws, int sws, int cn, int* out)
{
    const nlm::Geom g = nlm::geomOf(tws, sws, cn);
    out[0] = g.th; out[1] = g.sh; out[2] = g.T; out[3] = g.S; out[4] = g.b; out[5] = g.shift; out[6] = g.mult; out[7] = g.len;
}

extern "C" int emu_nlm_table(float h, int cn, int tws, int sws, int* table, int cap) { return nlm::buildTable(nlm::geomOf(tws, sws, cn), h, cn, table, cap); }

struct Image {
    const uint8_t* p; int W, H, cn;
    int operator()(int y, int x, int c) const { return p[((size_t)nlm::reflect101(y, H) * W + nlm::reflect101(x, W)) * cn + c]; }
};

extern "C" unsigned long long emu_nlm_dist(const uint8_t* src, int W, int H, int cn, int y, int x, int dy, int dx, int th)
{
    return nlm::patchDist(Image{src, W, H, cn}, y, x, dy, dx, th, cn);
}

extern "C" unsigned long long emu_nlm_pixel_work(int tws, int sws, int cn) { return nlm::pixelWork(tws, sws, cn); }
extern "C" int emu_nlm_plain_band(int T, int S, int cn, int W, int nf, unsigned long long work) { return nlm::plainBand(T, S, cn, W, nf, work); }
extern "C" int emu_nlm_table_bytes(int prefix, int mult) { return nlm::tableBytes(prefix, nlm::wideTable(mult)); }
extern "C" int emu_nlm_finish(unsigned est, unsigned wsum) { return nlm::finish(est, wsum); }

// dense rows, cn interleaved channels: a lane per pixel
extern "C" void emu_nlm_plain(const uint8_t* src, int W, int H, int cn, float h, int tws, int sws, uint8_t* dst)
{
    const nlm::Geom g = nlm::geomOf(tws, sws, cn);
    std::vector<int> table(g.len);
    const int prefix = nlm::buildTable(g, h, cn, table.data(), g.len);
    const Image px{src, W, H, cn};
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            uint32_t wsum = 0, est[4] = {0, 0, 0, 0};
            for (int dy = -g.sh; dy <= g.sh; dy++)
                for (int dx = -g.sh; dx <= g.sh; dx++) {
                    const unsigned long long idx = nlm::patchDist(px, y, x, dy, dx, g.th, cn) >> g.shift;
                    if (idx >= (unsigned long long)prefix) continue;
                    const uint32_t w = (uint32_t)table[idx];
                    wsum += w;
                    for (int c = 0; c < cn; c++) est[c] += w * (uint32_t)px(y + dy, x + dx, c);
                }
            for (int c = 0; c < cn; c++) dst[((size_t)y * W + x) * cn + c] = nlm::finish(est[c], wsum);
        }
}

// the tile kernel, workgroup by workgroup, wave by wave, all 64 lanes of a wave in step
extern "C" void emu_nlm_tile(const uint8_t* src, int W, int H, int cn, float h, int tws, int sws, uint8_t* dst)
{
    const nlm::Geom g = nlm::geomOf(tws, sws, cn);
    std::vector<int> table(g.len);
    const int prefix = nlm::buildTable(g, h, cn, table.data(), g.len);
    const nlm::Tile t = nlm::tileOf(g.th, g.sh);
    const int R = nlm::WAVE_ROWS, th = g.th, T = g.T;
    const Image px{src, W, H, cn};
    std::vector<uint8_t> plane((size_t)t.PL * cn);
    for (int Y0 = 0; Y0 < H; Y0 += 2 * R)
        for (int X0 = 0; X0 < W; X0 += 2 * t.WC) {
            for (int i = 0; i < t.PL; i++)
                for (int c = 0; c < cn; c++) plane[(size_t)c * t.PL + i] = (uint8_t)px(Y0 - g.b + i / t.LW, X0 - g.b + i % t.LW, c);
            for (int wave = 0; wave < 4; wave++) {
                const int wx = wave & 1, wy = wave >> 1;
                std::vector<uint32_t> wsum(64 * R, 0), est((size_t)64 * R * 4, 0), ring(64 * T), V(64), D(64), s(64), n(64);
                for (int dy = -g.sh; dy <= g.sh; dy++)
                    for (int dx = -g.sh; dx <= g.sh; dx++) {
                        std::fill(V.begin(), V.end(), 0u);
                        for (int r = 0; r < R + 2 * th; r++) {
                            for (int lane = 0; lane < 64; lane++) {
                                const int own = nlm::walkStart(t, wx, wy, g.sh, lane), other = own + dy * t.LW + dx;
                                uint32_t d2 = 0;
                                for (int c = 0; c < cn; c++) d2 += nlm::sqDiff(plane[(size_t)c * t.PL + own + r * t.LW], plane[(size_t)c * t.PL + other + r * t.LW]);
                                V[lane] += d2;
                                if (r >= T) V[lane] -= ring[lane * T + r % T];
                                ring[lane * T + r % T] = d2;
                            }
                            if (r < 2 * th) continue;
                            D = V; s = V;
                            for (int k = 0; k < 2 * th; k++) {
                                for (int lane = 0; lane < 64; lane++) n[lane] = lane ? s[lane - 1] : 0u;        // every lane takes the value of the lane below
                                s = n;
                                for (int lane = 0; lane < 64; lane++) D[lane] += s[lane];
                            }
                            const int j = r - 2 * th;
                            for (int lane = 2 * th; lane < 64; lane++) {
                                const uint32_t idx = D[lane] >> g.shift;
                                if (idx >= (uint32_t)prefix) continue;
                                const uint32_t w = (uint32_t)table[idx];
                                const int q = nlm::walkStart(t, wx, wy, g.sh, lane) + dy * t.LW + dx + nlm::centreOf(t, j, th);
                                wsum[lane * R + j] += w;
                                for (int c = 0; c < cn; c++) est[((size_t)lane * R + j) * 4 + c] += w * plane[(size_t)c * t.PL + q];
                            }
                        }
                    }
                for (int lane = 2 * th; lane < 64; lane++)
                    for (int j = 0; j < R; j++) {
                        const int x = X0 + wx * t.WC + lane - 2 * th, y = Y0 + wy * R + j;
                        if (x >= W || y >= H) continue;
                        for (int c = 0; c < cn; c++) dst[((size_t)y * W + x) * cn + c] = nlm::finish(est[((size_t)lane * R + j) * 4 + c], wsum[lane * R + j]);
                    }
            }
        }
}
