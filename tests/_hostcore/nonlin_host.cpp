// Host harness of tests/test_nonlin_math_host.py: the per-lane functions of nflows_amd/csrc/nonlin_math.hpp behind a C
// interface, with the kernels' rule for the row sum (float64, rounded once).  Compiled by the test; CPU only.
#define __device__
#define __host__
#define __forceinline__ inline
#include <stdint.h>
#include "nflows_amd.h"
#include "nonlin_math.hpp"
using namespace nfa;

template <int KIND, bool INVERSE>
static int run(int64_t rows, int64_t n, const NonlinConst& k, double scale, const float* x, float* y, float* lad) {
    int status = 0;
    for (int64_t b = 0; b < rows; ++b) {
        double acc = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double v, c;
            status |= nonlin_eval<KIND, INVERSE>(x[b * n + i], k, v, c);
            y[b * n + i] = (float)v;
            acc += c;
        }
        lad[b] = (float)(acc * scale);
    }
    return status;
}

template <int KIND, bool INVERSE>
static void run_grad(int64_t rows, int64_t n, const NonlinConst& k, const float* x, const float* g, const float* gl, float* gx,
                     double* gt) {
    double acc = 0.0;
    for (int64_t b = 0; b < rows; ++b)
        for (int64_t i = 0; i < n; ++i) {
            double dy, dc, dy_t, dc_t;
            nonlin_grad<KIND, INVERSE>(x[b * n + i], k, dy, dc, dy_t, dc_t);
            gx[b * n + i] = (float)((double)g[b * n + i] * dy + (double)gl[b] * dc);
            acc += (double)g[b * n + i] * dy_t + (double)gl[b] * dc_t;
        }
    *gt = acc;
}

#define KINDS(FN, ...)                                                                                              \
    switch (kind) {                                                                                                 \
        case NFA_NONLIN_EXP: return inverse ? FN<NFA_NONLIN_EXP, true>(__VA_ARGS__) : FN<NFA_NONLIN_EXP, false>(__VA_ARGS__); \
        case NFA_NONLIN_TANH: return inverse ? FN<NFA_NONLIN_TANH, true>(__VA_ARGS__) : FN<NFA_NONLIN_TANH, false>(__VA_ARGS__); \
        case NFA_NONLIN_LOG_TANH: return inverse ? FN<NFA_NONLIN_LOG_TANH, true>(__VA_ARGS__) : FN<NFA_NONLIN_LOG_TANH, false>(__VA_ARGS__); \
        case NFA_NONLIN_LEAKY_RELU: return inverse ? FN<NFA_NONLIN_LEAKY_RELU, true>(__VA_ARGS__) : FN<NFA_NONLIN_LEAKY_RELU, false>(__VA_ARGS__); \
        case NFA_NONLIN_SIGMOID: return inverse ? FN<NFA_NONLIN_SIGMOID, true>(__VA_ARGS__) : FN<NFA_NONLIN_SIGMOID, false>(__VA_ARGS__); \
        default: return inverse ? FN<NFA_NONLIN_CAUCHY_CDF, true>(__VA_ARGS__) : FN<NFA_NONLIN_CAUCHY_CDF, false>(__VA_ARGS__); \
    }

extern "C" int host_nonlin(int kind, int inverse, int64_t rows, int64_t n, double p0, double p1, double p2, float temperature,
                           const float* x, float* y, float* lad) {
    const NonlinConst k = nonlin_constants(kind, p0, p1, p2, temperature);
    const double scale = nonlin_row_scale(kind, inverse != 0, p0);
    KINDS(run, rows, n, k, scale, x, y, lad)
}

extern "C" void host_nonlin_grad(int kind, int inverse, int64_t rows, int64_t n, double p0, double p1, double p2,
                                 float temperature, const float* x, const float* g, const float* gl, float* gx, double* gt) {
    const NonlinConst k = nonlin_constants(kind, p0, p1, p2, temperature);
    KINDS(run_grad, rows, n, k, x, g, gl, gx, gt)
}
