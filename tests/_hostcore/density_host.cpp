// Host harness of tests/test_density_math_host.py: the per-element functions of nflows_amd/csrc/density_math.hpp behind a C
// interface, with the kernels' rule for the row sum (float64, rounded once), and the launch plan's coverage of a row.
// Compiled by the test; CPU only.
#define __device__
#define __host__
#define __forceinline__ inline
#include <stdint.h>
#include <vector>
#include "density_math.hpp"
#include "launch_plan.hpp"
using namespace nfa;

extern "C" void host_diag(int64_t rows, int64_t n, int64_t stride, double log_z, const float* x, const float* m, const float* ls,
                          const float* add, float* lp) {
    for (int64_t b = 0; b < rows; ++b) {
        double acc = 0.0;
        for (int64_t i = 0; i < n; ++i) acc += diag_normal_term(x[b * n + i], m[b * stride + i], ls[b * stride + i]);
        lp[b] = (float)((acc - log_z) + (add ? (double)add[b] : 0.0));
    }
}

// per-element gradients; gm / gls [rows, n] (the caller sums a shared row's over the batch in float64)
extern "C" void host_diag_grad(int64_t rows, int64_t n, int64_t stride, const float* x, const float* m, const float* ls,
                               const float* g, double* gx, double* gls) {
    for (int64_t b = 0; b < rows; ++b)
        for (int64_t i = 0; i < n; ++i)
            diag_normal_grad(x[b * n + i], m[b * stride + i], ls[b * stride + i], (double)g[b], gx[b * n + i], gls[b * n + i]);
}

extern "C" void host_mog(int64_t rows, int64_t D, int K, double epsilon, const float* x, const float* o, const float* add,
                         float* lp) {
    for (int64_t b = 0; b < rows; ++b) {
        double acc = 0.0;
        for (int64_t d = 0; d < D; ++d) acc += mog_term(x[b * D + d], o + (b * D + d) * 3 * K, K, epsilon);
        lp[b] = (float)(acc + (add ? (double)add[b] : 0.0));
    }
}

extern "C" void host_mog_grad(int64_t rows, int64_t D, int K, double epsilon, const float* x, const float* o, const float* g,
                              float* gx, float* go) {
    for (int64_t b = 0; b < rows; ++b)
        for (int64_t d = 0; d < D; ++d) {
            const int64_t e = b * D + d;
            gx[e] = (float)mog_grad(x[e], o + e * 3 * K, go + e * 3 * K, K, epsilon, (double)g[b]);
        }
}

// log_softmax of a single logit through the kernel's expression: must be 0 exactly
extern "C" double host_mog_lsm_single(float logit) { return (double)logit - mog_logit_lse(&logit, 1); }

// how often the plan's workgroups visit each of the batch * n elements (rows regime: whole rows; pieces: pieces of a row),
// by the arithmetic of density.hip's density_range; returns the number of workgroups
extern "C" int64_t host_plan_cover(int64_t batch, int64_t n, int32_t* visits, int32_t* rows_regime, int32_t* pieces) {
    const RowSumPlan p = plan_row_sum(batch, n);
    *rows_regime = p.rows > 0;
    *pieces = p.pieces;
    for (int64_t w = 0; w < p.groups; ++w) {
        int64_t first, count;
        if (p.rows > 0) {
            const int64_t row0 = w * p.rows;
            const int64_t rows = (batch - row0) < p.rows ? (batch - row0) : p.rows;
            first = row0 * n;
            count = rows * n;
            if (count > kRowSumTile) return -1;
        } else {
            const int64_t row = w / p.pieces, col0 = (w - row * p.pieces) * p.piece;
            count = (n - col0) < p.piece ? (n - col0) : p.piece;
            first = row * n + col0;
        }
        if (count < 1 || first < 0 || first + count > batch * n) return -1;
        for (int64_t i = 0; i < count; ++i) ++visits[first + i];
    }
    return p.groups;
}

extern "C" int host_mog_tile(int K) { return plan_mog_tile(K); }
extern "C" int64_t host_mog_lds(int K) { return (int64_t)mog_tile_bytes(plan_mog_tile(K), K) + kMogStaticLds; }
