// K24 (householder.hip), the arithmetic of one row: the blocked dot product, one Householder reflection, a staged run of
// reflections, the diagonal, and the walk through the stages that surround the triangular step.  No HIP in this file:
// the kernels include it, and tests/_hostcore/householder_host.cpp compiles the same text for the host (with
// -ffp-contract=off, as the library is built: every fused multiply-add below is written as one).
//
// A row lives in NB * 16 floats (features rounded up to 16; the padding is zero and stays zero), a reflection vector in
// the same number of floats, 16-byte aligned, with zero padding.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NFA_HD __host__ __device__ __forceinline__
#else
#define NFA_HD inline
#endif

namespace nfa {

constexpr int kHhBlk = 16;             // terms of one partial sum
constexpr int kHhMaxFeatures = 128;
constexpr int kHhMaxTransforms = 128;  // reflections per sequence
constexpr int kHhChunk = 32;           // reflections staged together (launch_plan.hpp: hh_region_floats)

struct alignas(16) HhVec4 {
    float x, y, z, w;
};

NFA_HD double softplus_f64(double u) {
    return u > 20.0 ? u : log1p(exp(u));   // F.softplus, beta = 1, threshold = 20
}

// d = eps + softplus(logit) in float64; the caller rounds it once
NFA_HD double hh_diagonal_f64(float logit, double eps) { return eps + softplus_f64((double)logit); }

// c = 2 / (v . v) from the float64 sum of squares of v[0 .. n); the float32 stages round it once
NFA_HD double hh_reflection_scale_f64(const float* v, int n) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += (double)v[j] * (double)v[j];
    return 2.0 / s;   // v = 0: +inf, and the row turns non-finite as the reference's does
}
NFA_HD float hh_reflection_scale(const float* v, int n) { return (float)hh_reflection_scale_f64(v, n); }

// x . v in blocks: 16 fused multiply-adds into a fresh partial, the partial added to the total (K16's remedy: the error
// of a 128-term sum grows like 16 + 8 roundings, not 128)
template <int NB>
NFA_HD float hh_dot(const float (&x)[NB * kHhBlk], const float* v) {
    const HhVec4* v4 = reinterpret_cast<const HhVec4*>(v);
    float total = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        float p = 0.f;
#pragma unroll
        for (int q = 0; q < kHhBlk / 4; ++q) {
            const HhVec4 m = v4[b * (kHhBlk / 4) + q];
            const int j = b * kHhBlk + 4 * q;
            p = (q == 0) ? m.x * x[j] : fmaf(m.x, x[j], p);
            p = fmaf(m.y, x[j + 1], p);
            p = fmaf(m.z, x[j + 2], p);
            p = fmaf(m.w, x[j + 3], p);
        }
        total = (b == 0) ? p : total + p;
    }
    return total;
}

// x <- x - t (c v): the second half of a reflection, t = x . v taken before
template <int NB>
NFA_HD void hh_update(float (&x)[NB * kHhBlk], const float* v, float c, float t) {
    const HhVec4* v4 = reinterpret_cast<const HhVec4*>(v);
#pragma unroll
    for (int q = 0; q < NB * kHhBlk / 4; ++q) {
        const HhVec4 m = v4[q];
        x[4 * q] = fmaf(-t, c * m.x, x[4 * q]);
        x[4 * q + 1] = fmaf(-t, c * m.y, x[4 * q + 1]);
        x[4 * q + 2] = fmaf(-t, c * m.z, x[4 * q + 2]);
        x[4 * q + 3] = fmaf(-t, c * m.w, x[4 * q + 3]);
    }
}

// Between two passes over a vector: the second pass reads it again (in the kernel: LDS broadcasts) rather than holding
// all of it in registers beside the row.
#define NFA_HH_READ_AGAIN() asm volatile("" ::: "memory")

template <int NB>
NFA_HD void hh_reflect(float (&x)[NB * kHhBlk], const float* v, float c) {
    const float t = hh_dot<NB>(x, v);
    NFA_HH_READ_AGAIN();
    hh_update<NB>(x, v, c, t);
}

// the n staged reflections V [n, DP] with scales c [n], first to last or (descending) last to first
template <int NB>
NFA_HD void hh_reflect_run(float (&x)[NB * kHhBlk], const float* V, const float* c, int n, bool descending) {
    constexpr int DP = NB * kHhBlk;
    for (int s = 0; s < n; ++s) {
        const int k = descending ? n - 1 - s : s;
        hh_reflect<NB>(x, V + k * DP, c[k]);
    }
}

// the diagonal stage: x <- d x, or x <- x / d (correctly rounded division)
template <int NB>
NFA_HD void hh_diagonal(float (&x)[NB * kHhBlk], const float* d, bool divide) {
#pragma unroll
    for (int j = 0; j < NB * kHhBlk; ++j) x[j] = divide ? x[j] / d[j] : x[j] * d[j];
}

template <int NB>
NFA_HD void hh_add(float (&x)[NB * kHhBlk], const float* b, float sign) {
#pragma unroll
    for (int j = 0; j < NB * kHhBlk; ++j) x[j] = sign < 0.f ? x[j] - b[j] : x[j] + b[j];
}

// The chunks a sequence of K reflections is staged in, in the order they are applied: chunk i of hh_chunks(K) holds the
// reflections [first, first + count) of the sequence.
NFA_HD int hh_chunks(int K) { return (K + kHhChunk - 1) / kHhChunk; }
struct HhChunk {
    int first, count;
};
NFA_HD HhChunk hh_chunk(int K, int i, bool descending) {
    const int c = descending ? hh_chunks(K) - 1 - i : i;
    HhChunk ch;
    ch.first = c * kHhChunk;
    ch.count = K - ch.first < kHhChunk ? K - ch.first : kHhChunk;
    return ch;
}

// a staged chunk: the vectors V [count, NB * 16] and their scales c [count]
struct HhStaged {
    const float* V;
    const float* c;
};

// The stage program of one layer call (include/nflows_amd.h, nfa_householder_f32), each stage optional, in this order:
//   - bias | reflect by set 0 | triangular | diagonal | reflect by set 1 | + bias
struct HhProgram {
    int K[2] = {0, 0};         // reflections of set 0 and of set 1
    bool descending = false;   // both sets last to first
    bool solve = false;        // the diagonal divides (and the triangular step substitutes)
    bool has_tri = false, has_diag = false, sub_bias = false, add_bias = false;
    const float* d = nullptr;     // [NB * 16] diagonal, padding 1
    const float* bias = nullptr;  // [NB * 16], padding 0
};

// One row through the program.  `stage(set, first, count)` makes the reflections [first, first + count) of a set
// available (the kernel copies them into LDS between two barriers, so every lane of
// the workgroup walks in step; the host points into the whole set); `tri(x)` is the triangular step.
template <int NB, typename Stage, typename Tri>
NFA_HD void hh_walk(float (&x)[NB * kHhBlk], const HhProgram& p, Stage&& stage, Tri&& tri) {
    if (p.sub_bias) hh_add<NB>(x, p.bias, -1.f);
    for (int set = 0; set < 2; ++set) {
        if (set == 1) {
            if (p.has_tri) tri(x);
            if (p.has_diag) hh_diagonal<NB>(x, p.d, p.solve);
        }
        const int K = set == 0 ? p.K[0] : p.K[1];
        for (int i = 0; i < hh_chunks(K); ++i) {
            const HhChunk ch = hh_chunk(K, i, p.descending);
            const HhStaged st = stage(set, ch.first, ch.count);
            hh_reflect_run<NB>(x, st.V, st.c, ch.count, p.descending);
        }
    }
    if (p.add_bias) hh_add<NB>(x, p.bias, 1.f);
}

}  // namespace nfa
