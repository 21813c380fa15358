// Per-element arithmetic of the elementwise nonlinearity transforms (K18, nonlin.hip; reference:
// transforms/nonlinearities.py -- Exp :18-32, Tanh :35-48, LogTanh :51-113, LeakyReLU :116-136, Sigmoid :139-169,
// CauchyCDF :192-211).  For every kind and direction `nonlin_eval` gives the output element and that element's term of
// the log-determinant, `nonlin_grad` the two factors of the input gradient (and of Sigmoid's temperature gradient).  No
// wave-level operation and no HIP type in here: the CPU suite compiles this file for the host
// (tests/test_nonlin_math_host.py) and holds it to the reference's vectors.
//
// Everything is evaluated in float64 from the float32 element and rounded ONCE by the caller.  The reference's float32
// results come from a vector libm whose tanh / exp / log are right to about half an ulp, and the parity rule allows twice
// the reference's own error on the mean and the 99.9 % quantile: a float32 libm that is one to two ulps off (the device's
// tanhf, atanf, tanf, log1pf) does not meet it, a float64 evaluation rounded once cannot miss it.  The reference's sequence
// is kept where it decides the result (Sigmoid: the term log T - softplus(-Tx) - softplus(Tx) with softplus' threshold of
// 20, the inverse's clamp to [eps, 1 - eps] before anything else; LogTanh: alpha and beta from the host's float64); where
// its expression cancels -- log(1 - tanh(x)^2), log((1 + x) / (1 - x)) near 0 -- the same quantity is taken from a form that
// does not (log 4 - 2|x| - 2 log1p(exp(-2|x|)), log1p(x) - log1p(-x)).
#pragma once
#include <math.h>

#include "nflows_amd.h"   // NFA_NONLIN_*, NFA_STATUS_*

namespace nfa {

// what a kind needs beside the element (nonlin_constants fills it; unused fields stay 0)
struct NonlinConst {
    double a = 0.0;   // LOG_TANH: cut_point        LEAKY_RELU: slope        SIGMOID: temperature T
    double b = 0.0;   //           tanh(cut_point)              1 / slope             log T
    double c = 0.0;   //           alpha                                              1 / T
    double d = 0.0;   //           beta                                               eps
    double e = 0.0;   //           -log(alpha beta)                                   1 - eps
};

// p0, p1, p2 as the C ABI takes them (include/nflows_amd.h); `temperature`: the value read from the module's tensor
__host__ __device__ __forceinline__ NonlinConst nonlin_constants(int kind, double p0, double p1, double p2, float temperature) {
    NonlinConst k;
    if (kind == NFA_NONLIN_LOG_TANH) {
        k.a = p0;
        k.b = tanh(p0);
        k.c = p1;
        k.d = p2;
        k.e = -log(p1 * p2);
    } else if (kind == NFA_NONLIN_LEAKY_RELU) {
        k.a = p0;
        k.b = 1.0 / p0;
    } else if (kind == NFA_NONLIN_SIGMOID) {
        k.a = (double)temperature;
        k.b = log(k.a);
        k.c = 1.0 / k.a;
        k.d = p0;
        k.e = 1.0 - p0;
    }
    return k;
}

constexpr double kNonlinPi = 3.14159265358979323846;
constexpr double kNonlinLogPi = 1.14472988584940017414;
constexpr double kNonlinLog4 = 1.38629436111989061883;

// F.softplus, beta = 1, threshold = 20
__device__ __forceinline__ double nonlin_softplus(double u) { return u > 20.0 ? u : log1p(exp(u)); }

// log(1 - tanh(x)^2) = log 4 - 2|x| - 2 log1p(exp(-2|x|))
__device__ __forceinline__ double nonlin_log_sech2(double x) {
    const double t = 2.0 * fabs(x);
    return (kNonlinLog4 - t) - 2.0 * log1p(exp(-t));
}

// Output element `y` and the element's term `c` of the log-determinant, both before their rounding; returns
// NFA_STATUS_OUTSIDE_DOMAIN where the reference raises InputOutsideDomain (y and c are then unspecified, never a fault),
// else 0.  LEAKY_RELU's term is the COUNT of the slope's use (1 or 0): the caller multiplies the row's count by
// +-log(slope) (nonlin_row_scale).
template <int KIND, bool INVERSE>
__device__ __forceinline__ int nonlin_eval(float xf, const NonlinConst& k, double& y, double& c) {
    const double x = (double)xf;
    int status = 0;
    if (KIND == NFA_NONLIN_EXP) {
        if (!INVERSE) {
            y = exp(x);
            c = x;
        } else {
            if (!(xf > 0.0f)) status = NFA_STATUS_OUTSIDE_DOMAIN;
            y = log(x);
            c = -y;
        }
    } else if (KIND == NFA_NONLIN_TANH || KIND == NFA_NONLIN_LOG_TANH) {
        const bool log_tanh = KIND == NFA_NONLIN_LOG_TANH;
        if (!INVERSE) {
            if (log_tanh && x > k.a) {
                y = k.c * log(k.d * x);
                c = log(k.c / x);
            } else if (log_tanh && x < -k.a) {
                y = -(k.c * log(-k.d * x));
                c = log(-k.c / x);
            } else {
                y = tanh(x);
                c = nonlin_log_sech2(x);
            }
        } else {
            if (log_tanh && x > k.b) {
                const double q = x / k.c;
                y = exp(q) / k.d;
                c = k.e + q;
            } else if (log_tanh && x < -k.b) {
                const double q = x / k.c;
                y = -exp(-q) / k.d;
                c = k.e - q;
            } else {
                if (!log_tanh && !(xf > -1.0f && xf < 1.0f)) status = NFA_STATUS_OUTSIDE_DOMAIN;
                const double up = log1p(x), down = log1p(-x);
                y = 0.5 * (up - down);
                c = -(up + down);
            }
        }
    } else if (KIND == NFA_NONLIN_LEAKY_RELU) {
        y = xf > 0.0f ? x : x * (INVERSE ? k.b : k.a);
        c = xf < 0.0f ? 1.0 : 0.0;
    } else if (KIND == NFA_NONLIN_SIGMOID) {
        if (!INVERSE) {
            const double t = k.a * x;
            y = 1.0 / (1.0 + exp(-t));
            c = (k.b - nonlin_softplus(-t)) - nonlin_softplus(t);
        } else {
            if (!(xf >= 0.0f && xf <= 1.0f)) status = NFA_STATUS_OUTSIDE_DOMAIN;
            const double xc = x < k.d ? k.d : (x > k.e ? k.e : x);
            const double l = log(xc) - log1p(-xc);
            y = k.c * l;
            c = -((k.b - nonlin_softplus(-l)) - nonlin_softplus(l));   // (temperature * outputs = l)
        }
    } else {   // NFA_NONLIN_CAUCHY_CDF
        if (!INVERSE) {
            y = atan(x) / kNonlinPi + 0.5;
            c = -kNonlinLogPi - log1p(x * x);
        } else {
            if (!(xf >= 0.0f && xf <= 1.0f)) status = NFA_STATUS_OUTSIDE_DOMAIN;
            y = tan(kNonlinPi * (x - 0.5));
            c = kNonlinLogPi + log1p(y * y);
        }
    }
    return status;
}

// the factor of a row's sum of terms before its single rounding
__host__ __device__ __forceinline__ double nonlin_row_scale(int kind, bool inverse, double p0) {
    if (kind != NFA_NONLIN_LEAKY_RELU) return 1.0;
    return inverse ? -log(p0) : log(p0);
}

// dy/dx and d(term)/dx at the input x of the pass that is differentiated; Sigmoid also dy/dT and d(term)/dT.
// (LEAKY_RELU's term is piecewise constant: dc = 0.)
template <int KIND, bool INVERSE>
__device__ __forceinline__ void nonlin_grad(float xf, const NonlinConst& k, double& dy, double& dc, double& dy_t, double& dc_t) {
    const double x = (double)xf;
    dy_t = 0.0;
    dc_t = 0.0;
    if (KIND == NFA_NONLIN_EXP) {
        if (!INVERSE) {
            dy = exp(x);
            dc = 1.0;
        } else {
            dy = 1.0 / x;
            dc = -dy;
        }
    } else if (KIND == NFA_NONLIN_TANH || KIND == NFA_NONLIN_LOG_TANH) {
        const bool log_tanh = KIND == NFA_NONLIN_LOG_TANH;
        if (!INVERSE) {
            if (log_tanh && (x > k.a || x < -k.a)) {
                dy = (x > k.a ? k.c : -k.c) / x;
                dc = -1.0 / x;
            } else {
                const double e = exp(-2.0 * fabs(x)), r = 1.0 / (1.0 + e);
                dy = 4.0 * e * r * r;                       // 1 - tanh(x)^2
                dc = (x < 0.0 ? 2.0 : -2.0) * (1.0 - e) * r;   // -2 tanh(x)
            }
        } else {
            if (log_tanh && x > k.b) {
                dy = (exp(x / k.c) / k.d) / k.c;
                dc = 1.0 / k.c;
            } else if (log_tanh && x < -k.b) {
                dy = (exp(-x / k.c) / k.d) / k.c;
                dc = -1.0 / k.c;
            } else {
                const double r = 1.0 / ((1.0 - x) * (1.0 + x));
                dy = r;
                dc = (2.0 * x) * r;
            }
        }
    } else if (KIND == NFA_NONLIN_LEAKY_RELU) {
        dy = xf > 0.0f ? 1.0 : (INVERSE ? k.b : k.a);
        dc = 0.0;
    } else if (KIND == NFA_NONLIN_SIGMOID) {
        if (!INVERSE) {
            const double t = k.a * x;
            const double y = 1.0 / (1.0 + exp(-t)), w = 1.0 / (1.0 + exp(t));   // sigmoid(t), sigmoid(-t)
            const double s = y * w;
            dy = k.a * s;
            dc = k.a * (w - y);
            dy_t = x * s;
            dc_t = k.c + x * (w - y);
        } else {
            const bool inside = x >= k.d && x <= k.e;   // (clamp passes the gradient on its closed interval)
            const double xc = x < k.d ? k.d : (x > k.e ? k.e : x);
            const double r = 1.0 / (xc * (1.0 - xc));
            dy = inside ? k.c * r : 0.0;
            dc = inside ? (xc - (1.0 - xc)) * r : 0.0;
            dy_t = -(k.c * k.c) * (log(xc) - log1p(-xc));
            dc_t = -k.c;
        }
    } else {   // NFA_NONLIN_CAUCHY_CDF
        if (!INVERSE) {
            const double r = 1.0 / (1.0 + x * x);
            dy = r / kNonlinPi;
            dc = -(2.0 * x) * r;
        } else {
            const double y = tan(kNonlinPi * (x - 0.5));
            dy = kNonlinPi * (1.0 + y * y);
            dc = (2.0 * kNonlinPi) * y;
        }
    }
}

}  // namespace nfa
