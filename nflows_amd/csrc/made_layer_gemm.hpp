// The two GEMMs of a MADE inside a layer kernel whose k-steps are counted at run time: the context term and the initial
// layer.  Shared by K29 (made_rqs_kernel.hpp) and K31 (made_mog_kernel.hpp); the includer defines NFA_BF16X3_SPLIT_ACC.
#pragma once

#include "bf16x3_gemm.hpp"

namespace nfa {

// K22's context terms (affine_mlp_kernel.hpp: gemm_context), here with a run-time number of k-steps: nks k-steps of
// Wc[128 x 16 nks] x ctx^T on the accumulators of a k-major GEMM, the small products merged at the end.
__device__ __forceinline__ void made_rqs_context(f32x16 (&acc)[4], const float* s_ctx, int ce, int nks, int half, int r,
                                                 WeightStream& sm, int lane) {
    f32x16 small[4] = {{0}, {0}, {0}, {0}};
    for (int ks = 0; ks < nks; ++ks) {
        stream_request(sm);
        const vec4f* cur = sm.ring + sm.slot * kStageVec4 + lane;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = ks * 16 + half * 8 + j;
            const float cv = s_ctx[(i < ce ? i : 0) * kRowPad + r];
            v[j] = i < ce ? cv : 0.0f;
        }
        bf16x2 hh[4], mm[4], ll[4];
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) split3(vec2f{v[j2 * 2], v[j2 * 2 + 1]}, hh[j2], mm[j2], ll[j2]);
        const bf16x8 bh = join4(hh[0], hh[1], hh[2], hh[3]);
        const bf16x8 bm = join4(mm[0], mm[1], mm[2], mm[3]);
        const bf16x8 bl = join4(ll[0], ll[1], ll[2], ll[3]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bf16x8 ah = __builtin_bit_cast(bf16x8, cur[(t * 3 + 0) * 64]);
            const bf16x8 am = __builtin_bit_cast(bf16x8, cur[(t * 3 + 1) * 64]);
            const bf16x8 al = __builtin_bit_cast(bf16x8, cur[(t * 3 + 2) * 64]);
            NFA_MFMA6_SPLIT(acc[t], small[t], ah, am, al, bh, bm, bl);
        }
        stream_advance(sm);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] += small[t];
}

// gemm_kmajor<kActNone, NKS> with NKS = 2 or 4 chosen at run time: the four k-steps are unrolled (the pieces keep static
// register indices) and the last two sit behind a workgroup-uniform branch -- `nks` is a kernel argument, every wave takes
// the same side, the barriers inside stay matched.
__device__ __forceinline__ void made_rqs_initial(f32x16 (&acc)[4], const bf16x8 (&ph)[8], const bf16x8 (&pm)[8],
                                                 const bf16x8 (&pl)[8], int nks, WeightStream& sm, int lane) {
    f32x16 small[4] = {{0}, {0}, {0}, {0}};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        if (ks < nks) {
            stream_request(sm);
            const vec4f* cur = sm.ring + sm.slot * kStageVec4 + lane;
            const bf16x8 bh = ph[ks], bm = pm[ks], bl = pl[ks];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bf16x8 ah = __builtin_bit_cast(bf16x8, cur[(t * 3 + 0) * 64]);
                const bf16x8 am = __builtin_bit_cast(bf16x8, cur[(t * 3 + 1) * 64]);
                const bf16x8 al = __builtin_bit_cast(bf16x8, cur[(t * 3 + 2) * 64]);
                NFA_MFMA6_SPLIT(acc[t], small[t], ah, am, al, bh, bm, bl);
            }
            stream_advance(sm);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] += small[t];
}

}  // namespace nfa
