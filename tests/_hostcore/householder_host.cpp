// Host build of K24's per-row arithmetic: nflows_amd/csrc/householder_math.hpp as the kernels include it -- the blocked
// reflection, the diagonal and the stage walk -- for tests/test_householder_host.py.  Nothing of the arithmetic is
// restated here: this file pads the parameters as the kernel's staging does and calls hh_walk row by row.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "householder_math.hpp"

namespace {

struct Set {
    float* V = nullptr;   // [K, DP], 16-byte aligned, zero padded
    std::vector<float> c;
    void fill(const float* q, int K, int D, int DP) {
        if (K == 0) return;
        V = static_cast<float*>(aligned_alloc(16, sizeof(float) * K * DP));
        memset(V, 0, sizeof(float) * K * DP);
        c.resize(K);
        for (int k = 0; k < K; ++k) {
            memcpy(V + k * DP, q + k * D, sizeof(float) * D);
            c[k] = nfa::hh_reflection_scale(V + k * DP, D);
        }
    }
    ~Set() { free(V); }
};

template <int NB>
void run(const float* x, float* out, int64_t rows, int D, const Set (&sets)[2], const nfa::HhProgram& p) {
    constexpr int DP = NB * nfa::kHhBlk;
    auto stage = [&](int set, int first, int) { return nfa::HhStaged{sets[set].V + first * DP, sets[set].c.data() + first}; };
    auto tri = [](float (&)[DP]) {};
    for (int64_t r = 0; r < rows; ++r) {
        float row[DP] = {};
        memcpy(row, x + r * D, sizeof(float) * D);
        nfa::hh_walk<NB>(row, p, stage, tri);
        memcpy(out + r * D, row, sizeof(float) * D);
    }
}

}  // namespace

// the program of nfa_householder_f32 without a triangular stage; returns the layer's logabsdet (float64 sum, rounded once)
extern "C" float host_householder(const float* x, float* out, int64_t rows, int D, const float* q_first, int num_first,
                                  const float* q_second, int num_second, const float* unconstrained_diagonal,
                                  const float* bias, double eps, int inverse) {
    const int DP = (D + nfa::kHhBlk - 1) / nfa::kHhBlk * nfa::kHhBlk;
    Set sets[2];
    sets[0].fill(q_first, num_first, D, DP);
    sets[1].fill(q_second, num_second, D, DP);
    std::vector<float> d(DP, 1.f), b(DP, 0.f);
    double lad = 0.0;
    for (int j = 0; j < D; ++j) {
        if (unconstrained_diagonal) {
            const double dj = nfa::hh_diagonal_f64(unconstrained_diagonal[j], eps);
            d[j] = (float)dj;
            lad += log(dj);
        }
        if (bias) b[j] = bias[j];
    }
    nfa::HhProgram p;
    p.K[0] = num_first, p.K[1] = num_second;
    p.descending = p.solve = inverse != 0;
    p.has_diag = unconstrained_diagonal != nullptr;
    p.sub_bias = bias && inverse, p.add_bias = bias && !inverse;
    p.d = d.data(), p.bias = b.data();
    switch (DP / nfa::kHhBlk) {
        case 1: run<1>(x, out, rows, D, sets, p); break;
        case 2: run<2>(x, out, rows, D, sets, p); break;
        case 3: run<3>(x, out, rows, D, sets, p); break;
        case 4: run<4>(x, out, rows, D, sets, p); break;
        case 5: run<5>(x, out, rows, D, sets, p); break;
        case 6: run<6>(x, out, rows, D, sets, p); break;
        case 7: run<7>(x, out, rows, D, sets, p); break;
        default: run<8>(x, out, rows, D, sets, p); break;
    }
    return (float)(inverse ? 0.0 - lad : lad);
}
