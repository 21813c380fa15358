// Per-element arithmetic of the learned base densities (K20, density.hip; reference: distributions/normal.py:95-114 and
// :155-174 -- ConditionalDiagonalNormal, DiagonalNormal --, nn/nde/made.py:328-353 -- MixtureOfGaussiansMADE.log_prob).  For
// each mode one function gives an element's term of the row's log-density and one the element's gradients.  No wave-level
// operation and no HIP type in here: the CPU suite compiles this file for the host (tests/test_density_math_host.py) and
// holds it to the reference's vectors.
//
// Everything is evaluated in float64 from the float32 operands and rounded ONCE by the caller, as K18's arithmetic is
// (nonlin_math.hpp): the parity rule allows twice the reference's own error on the mean and the 99.9 % quantile, which a
// float32 exp / log that is one or two ulps off does not meet and a float64 evaluation rounded once cannot miss.  The
// reference's sequence is kept where it decides the result: softplus with its threshold of 20 (and, in the gradient, the
// derivative 1 above it), std = softplus(u) + epsilon, the logsumexp with its maximum subtracted.
#pragma once
#include <math.h>

namespace nfa {

constexpr double kDensityLog2Pi = 1.83787706640934548356;
constexpr int kMogMaxComponents = 64;

// ---- mode "diag": term = -0.5 ((x - m) exp(-ls))^2 - ls; the row's result is the terms' sum - log_z (+ add)
__device__ __forceinline__ double diag_normal_term(float x, float m, float ls) {
    const double z = ((double)x - (double)m) * exp(-(double)ls);
    return -0.5 * (z * z) - (double)ls;
}

// gradients of g * term: with e2 = exp(-2 ls), gx = -g (x - m) e2 (the mean's is -gx), gls = g ((x - m)^2 e2 - 1)
__device__ __forceinline__ void diag_normal_grad(float x, float m, float ls, double g, double& gx, double& gls) {
    const double d = (double)x - (double)m;
    const double e2 = exp(-2.0 * (double)ls);
    gx = -g * d * e2;
    gls = g * (d * d * e2 - 1.0);
}

// ---- mode "mog": an element's 3K floats `o` = (logit, mean, unconstrained std) x K, the reference's interleaving
// F.softplus, beta = 1, threshold = 20
__device__ __forceinline__ double mog_softplus(double u) { return u > 20.0 ? u : log1p(exp(u)); }

// log sum_k exp(logit_k), maximum subtracted: K = 1 gives logit_0 + log(1) = logit_0, so lsm_0 = 0 exactly
__device__ __forceinline__ double mog_logit_lse(const float* o, int K) {
    double top = (double)o[0];
    for (int k = 1; k < K; ++k) top = fmax(top, (double)o[3 * k]);
    double sum = 0.0;
    for (int k = 0; k < K; ++k) sum += exp((double)o[3 * k] - top);
    return top + log(sum);
}

// t_k = lsm_k - 0.5 (log 2pi + 2 log std_k + ((x - m_k) / std_k)^2)
__device__ __forceinline__ double mog_component(double x, const float* o, int k, double lse_logits, double epsilon,
                                                double& std, double& z) {
    std = mog_softplus((double)o[3 * k + 2]) + epsilon;
    z = (x - (double)o[3 * k + 1]) / std;
    return ((double)o[3 * k] - lse_logits) - 0.5 * (kDensityLog2Pi + 2.0 * log(std) + z * z);
}

// logsumexp_k t_k with its maximum subtracted: the running maximum is carried along (one pass, one exp per component);
// what it returns is max_k t_k + log sum_k exp(t_k - max_k t_k)
__device__ __forceinline__ double mog_lse(double x, const float* o, int K, double lse_logits, double epsilon) {
    double std, z;
    double top = mog_component(x, o, 0, lse_logits, epsilon, std, z);
    double sum = 1.0;
    for (int k = 1; k < K; ++k) {
        const double t = mog_component(x, o, k, lse_logits, epsilon, std, z);
        if (t > top) {
            sum = sum * exp(top - t) + 1.0;
            top = t;
        } else {
            sum += exp(t - top);
        }
    }
    return top + log(sum);
}

// the element's term of the row's log-density
__device__ __forceinline__ double mog_term(float x, const float* o, int K, double epsilon) {
    return mog_lse((double)x, o, K, mog_logit_lse(o, K), epsilon);
}

// gradients of g * term: `go` (3K floats; may be `o` itself -- component k is written after its last read) and the return
// value, the gradient of x.  r_k = exp(t_k - lse):
//   d/dlogit_k = g (r_k - softmax_k)   d/dm_k = g r_k (x - m_k) / std_k^2
//   d/du_k = g r_k (((x - m_k) / std_k)^2 - 1) / std_k * softplus'(u_k)   d/dx = -sum_k d/dm_k
__device__ __forceinline__ double mog_grad(float xf, const float* o, float* go, int K, double epsilon, double g) {
    const double x = (double)xf;
    const double lse_logits = mog_logit_lse(o, K);
    const double lse = mog_lse(x, o, K, lse_logits, epsilon);
    double gx = 0.0;
    for (int k = 0; k < K; ++k) {
        double std, z;
        const double logit = (double)o[3 * k], u = (double)o[3 * k + 2];
        const double r = exp(mog_component(x, o, k, lse_logits, epsilon, std, z) - lse);
        const double gm = g * r * z / std;
        const double slope = u > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-u));
        go[3 * k] = (float)(g * (r - exp(logit - lse_logits)));
        go[3 * k + 1] = (float)gm;
        go[3 * k + 2] = (float)(g * r * (z * z - 1.0) / std * slope);
        gx -= gm;
    }
    return gx;
}

}  // namespace nfa
