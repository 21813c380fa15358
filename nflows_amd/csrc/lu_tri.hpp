// The triangular steps K16 / K19 (lu_linear.hip) and K24 (householder.hip) share: the dense [DP, DP] LDS image of a
// layer's triangular factors and one row's product with, or substitution through, one triangle of it.
#pragma once

#include "common.hpp"
#include "householder_math.hpp"   // softplus_f64 (the header without HIP, which the host tests compile too)

namespace nfa {

constexpr int kLuBlk = 16;        // register block

// The off-diagonal elements of the dense image M [DP, DP] (row stride DP; DP = features rounded up to 16): the strict
// lower triangle from `lower` (np.tril_indices(D, -1) order; NULL: zeros), the strict upper triangle from `upper`
// (np.triu_indices(D, 1) order), zeros in the padding; TRANSPOSED: the image of the transposed matrix.  The diagonal
// is the caller's.  `lanes` threads of the workgroup, `tid` among them; no barrier inside.
__device__ __forceinline__ void expand_tri_image(float* __restrict__ M, const float* __restrict__ lower,
                                                 const float* __restrict__ upper, int D, int DP, FastDiv div_DP,
                                                 bool transposed, int tid, int lanes) {
    for (int e = tid; e < DP * DP; e += lanes) {
        const int i = (int)fastdiv((uint32_t)e, div_DP);
        const int j = e - i * DP;
        if (i == j) continue;
        const int si = transposed ? j : i, sj = transposed ? i : j;   // the element of L / U this image element is
        float m = 0.f;
        if (si < D && sj < D) {
            if (si > sj) m = lower ? lower[(si * (si - 1)) / 2 + sj] : 0.f;
            else m = upper[si * D - (si * (si + 1)) / 2 + (sj - si - 1)];
        }
        M[e] = m;
    }
}

// v <- T v (SOLVE = false) or v <- T^-1 v (SOLVE = true) for one row, in place.  T is the UPPER or the lower triangle
// of the LDS image M (row stride DP) with its diagonal, or a unit diagonal (UNIT).  `col` points at the lane's row in
// the column-major tile (element j at col[j * RS]).  nb = DP / 16.
template <bool UPPER, bool UNIT, bool SOLVE>
__device__ __forceinline__ void tri_apply(const float* __restrict__ M, int DP, int nb, float* col, int RS) {
    constexpr bool kAscending = (UPPER != SOLVE);   // the order in which a block's inputs are still (or already) valid
    for (int step = 0; step < nb; ++step) {
        const int I = kAscending ? step : nb - 1 - step;
        float v[kLuBlk], acc[kLuBlk], o[kLuBlk];
#pragma unroll
        for (int i = 0; i < kLuBlk; ++i) {
            v[i] = col[(I * kLuBlk + i) * RS];
            acc[i] = 0.f;
        }
        const int j0 = UPPER ? I + 1 : 0, j1 = UPPER ? nb : I;
        for (int J = j0; J < j1; ++J) {
            float xj[kLuBlk];
#pragma unroll
            for (int j = 0; j < kLuBlk; ++j) xj[j] = col[(J * kLuBlk + j) * RS];
            const float* Mb = M + (I * kLuBlk) * DP + J * kLuBlk;
#pragma unroll
            for (int i = 0; i < kLuBlk; ++i) {
                const float4* row = reinterpret_cast<const float4*>(Mb + i * DP);
                float p = 0.f;
#pragma unroll
                for (int q = 0; q < kLuBlk / 4; ++q) {
                    const float4 m = row[q];
                    p = (q == 0) ? m.x * xj[0] : fmaf(m.x, xj[4 * q], p);
                    p = fmaf(m.y, xj[4 * q + 1], p);
                    p = fmaf(m.z, xj[4 * q + 2], p);
                    p = fmaf(m.w, xj[4 * q + 3], p);
                }
                acc[i] += p;
            }
        }
        const float* Md = M + (I * kLuBlk) * DP + I * kLuBlk;
        if (!SOLVE) {
#pragma unroll
            for (int i = 0; i < kLuBlk; ++i) {
                float p = UNIT ? v[i] : Md[i * DP + i] * v[i];
#pragma unroll
                for (int j = 0; j < kLuBlk; ++j)
                    if (UPPER ? j > i : j < i) p = fmaf(Md[i * DP + j], v[j], p);
                o[i] = p + acc[i];
            }
        } else {
#pragma unroll
            for (int s = 0; s < kLuBlk; ++s) {
                const int i = UPPER ? kLuBlk - 1 - s : s;
                float t = v[i] - acc[i];
#pragma unroll
                for (int j = 0; j < kLuBlk; ++j)
                    if (UPPER ? j > i : j < i) t = fmaf(-Md[i * DP + j], o[j], t);
                o[i] = UNIT ? t : t / Md[i * DP + i];
            }
        }
#pragma unroll
        for (int i = 0; i < kLuBlk; ++i) col[(I * kLuBlk + i) * RS] = o[i];
    }
}

}  // namespace nfa
