// calchist_emu.cpp -- opencv_amd/csrc/calchist_math.h (the arithmetic of the kernels of calchist.hip) compiled for the CPU: the per-dimension tables, the CV_32F
// bin rule, the non-uniform search, the back-projection rounding and the float <-> int32 conversions of `accumulate`, for tests/test_calchist_cpu.py to hold
// against tests/calchist_restate.py.
#include "calchist_math.h"

// tab[v] for v < levels: bin * mult, or SKIP.  ranges: {lo, hi} when uniform, else n + 1 boundaries
extern "C" void emu_calchist_table(int levels, int n, int uniform, const float* ranges, int mult, int32_t* tab)
{
    calchist::buildTable(levels, n, uniform != 0, ranges, mult, tab);
}

extern "C" void emu_calchist_bins_f32(const float* v, int count, int n, float lo, float hi, int* bins)
{
    const calchist::Uniform u = calchist::uniformCoef(n, lo, hi);
    for (int i = 0; i < count; i++) bins[i] = calchist::binUniformF32(v[i], n, u);
}

extern "C" void emu_calchist_coef(int n, float lo, float hi, double* ab)
{
    const calchist::Uniform u = calchist::uniformCoef(n, lo, hi);
    ab[0] = u.a; ab[1] = u.b;
}

extern "C" int emu_calchist_bin_nonuniform(float v, const float* r, int n) { return calchist::binNonUniform(v, r, n); }

// depth 0 / 2: cvRound saturated into out32; depth 5: the float's bits
extern "C" void emu_calchist_backproject(int depth, const float* h, int count, double scale, uint32_t* out32)
{
    for (int i = 0; i < count; i++) {
        if (depth == 5) { const float f = calchist::backProjectF32(h[i], scale); __builtin_memcpy(&out32[i], &f, 4); }
        else out32[i] = calchist::backProjectInt(h[i], scale, depth == 0 ? 255u : 65535u);
    }
}

extern "C" void emu_calchist_count_of_float(const float* f, int count, int32_t* out)
{
    for (int i = 0; i < count; i++) out[i] = calchist::countOfFloat(f[i]);
}

extern "C" void emu_calchist_float_of_count(const int32_t* c, int count, float* out)
{
    for (int i = 0; i < count; i++) out[i] = calchist::floatOfCount(c[i]);
}

extern "C" int emu_calchist_skip(void) { return calchist::SKIP; }
extern "C" int emu_calchist_max_dim(void) { return calchist::MAX_DIM; }
extern "C" int emu_calchist_max_bins(void) { return calchist::MAX_BINS; }
extern "C" int emu_calchist_max_bins_per_dim(void) { return calchist::MAX_BINS_PER_DIM; }
