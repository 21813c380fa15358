// The kernel body of K31 (made_mog.hip: MixtureOfGaussiansMADE.log_prob -- the density-estimator MADE, its final Linear and
// the mixture-of-Gaussians log-density -- in one launch).  K29's skeleton (made_rqs_kernel.hpp): one workgroup of four waves
// per CU, persistent over the 128-row blocks, a wave's 32 rows in an LDS row tile and its context rows in a second one, the
// weights on the LDS-DMA ring, every hidden activation in registers as three bf16 pieces, and a final tile loop whose MFMA
// accumulators ARE a feature's parameters.  What differs is the density-estimator MADE (nn/nde/made.py): the context term of
// the initial layer is not rectified, the initial layer is raw in front of feed-forward blocks, the final Linear reads the
// blocks' result as it is; and the element: density_math.hpp's mixture term in float64 on the accumulator values.
//
// The template has ONE axis, T = ceil(3 K / 16), the 32-row tiles per pair of features: three instances serve K = 1 .. 16.
// The 16 T accumulator values of lane-half h are the (logit, mean, unconstrained std) x K of feature 2 g + h in the
// module's own interleaving, zero rows behind them; the element's loops are unrolled to KMAX = floor(16 T / 3) components and
// those beyond the run-time K are skipped under a scalar test, so every register index is static: nothing goes to scratch.
#pragma once

// (the split accumulators of K11 / K22 / K29: see NFA_MFMA6_SPLIT, fused_common.hpp)
#define NFA_BF16X3_SPLIT_ACC
#include "made_layer_gemm.hpp"
#include "density_math.hpp"

#include <hip/hip_ext.h>
#include <math.h>
#include <stdlib.h>

namespace nfa {

struct MadeMogArgs {
    const float* x;         // [B, D]
    const vec4f* w;         // [num_stages][768] x 16 bytes
    const float* bias;      // accumulator-order biases of all GEMMs
    const float* ctx;       // with a context: [B, ce]
    const float* add;       // [B] or null: joins the row's float64 sum
    float* out;             // [B] log_prob
    int64_t batch;          // multiple of 128
    int D;                  // features = row length (any of 1 .. 64)
    int num_hidden;         // hidden Linears: two per residual block, one per feed-forward block
    int num_stages;
    int init_ks;            // k-steps of the initial layer: 2 (features <= 32) or 4
    int resnet;             // residual blocks / feed-forward blocks
    int ce, ctx_ks;         // context features, their k-steps (ceil(ce / 16))
    int K;                  // mixture components, 3 K <= 16 T
    double epsilon;
};

// a wave's 32 rows of n floats -> its tile ([column][kRowPad]), four bytes per lane (the context rows; input rows whose
// length is no multiple of four)
__device__ __forceinline__ void load_rows(float* tile, const float* rows, int n, int lane) {
    const int count = 32 * n;
    for (int e0 = lane; e0 < count; e0 += kWave * 4) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * kWave;
            v[u] = rows[e < count ? e : 0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * kWave;
            if (e < count) {
                const int rr = e / n, c = e - rr * n;
                tile[c * kRowPad + rr] = v[u];
            }
        }
    }
}

template <int T>
__global__ void __launch_bounds__(kBlock, 1) made_mog_kernel(const MadeMogArgs a) {
#pragma clang fp contract(off)
    constexpr int KMAX = 16 * T / 3;   // 5, 10, 16
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D;

    WeightStream sm;
    sm.w = a.w;
    sm.ring = reinterpret_cast<vec4f*>(lds_dyn);
    sm.slot = 1;
    sm.fetch = 0;
    sm.num_stages = a.num_stages;
    sm.tid = tid;
    stream_request(sm);  // stage 0 -> slot 0
    sm.slot = 2;
    stream_request(sm);  // stage 1 -> slot 1
    sm.slot = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    float* s_row = lds_dyn + kRing * kStageVec4 * 4 + wave * D * kRowPad;
    const bool ctx = a.ce > 0, resnet = a.resnet != 0;
    float* s_ctx = lds_dyn + kRing * kStageVec4 * 4 + (kBlock / kWave) * D * kRowPad + wave * a.ce * kRowPad;
    const int64_t num_quads = a.batch >> 7;

    for (int64_t quad = blockIdx.x; quad < num_quads; quad += gridDim.x) {
        const int64_t row0 = (quad << 7) + (wave << 5);
        int lane_here = lane;
        asm volatile("" : "+v"(lane_here));
        // (`lane_here` is opaque to the compiler: what is derived from it is computed per row block and holds no register
        //  across the GEMMs)
        const int half = lane_here >> 5, r = lane_here & 31;
        // ---- the wave's 32 rows, read once: slot j of the tile = column j.  16 bytes per lane where the row length allows
        //      it, four bytes otherwise (32 rows start on a 128-byte boundary either way)
        if ((D & 3) == 0) {
            const vec4f* xv = reinterpret_cast<const vec4f*>(a.x + row0 * D);
            const int nvec = D * 8;
            for (int e0 = lane_here; e0 < nvec; e0 += kWave * 4) {
                vec4f v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kWave;
                    v[u] = xv[e < nvec ? e : 0];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kWave;
                    if (e < nvec) {
                        const int rr = (e * 4) / D, c0 = e * 4 - rr * D;
                        s_row[(c0 + 0) * kRowPad + rr] = v[u].x;
                        s_row[(c0 + 1) * kRowPad + rr] = v[u].y;
                        s_row[(c0 + 2) * kRowPad + rr] = v[u].z;
                        s_row[(c0 + 3) * kRowPad + rr] = v[u].w;
                    }
                }
            }
        } else {
            load_rows(s_row, a.x + row0 * D, D, lane_here);
        }
        if (ctx) load_rows(s_ctx, a.ctx + row0 * a.ce, a.ce, lane_here);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const float* bias = a.bias + half * 16;  // + 32 per tile
        bf16x8 ph[8], pm[8], pl[8];  // the current activations (128 k per sample) as bf16 pieces

        // ---- the input columns: k = ks*16 + half*8 + j (k-steps beyond init_ks are not consumed)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (ks >= a.init_ks) continue;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = ks * 16 + half * 8 + j;
                const float xv = s_row[(i < D ? i : 0) * kRowPad + r];
                v[j] = i < D ? xv : 0.0f;
            }
            bf16x2 hh[4], mm[4], ll[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) split3(vec2f{v[j2 * 2], v[j2 * 2 + 1]}, hh[j2], mm[j2], ll[j2]);
            ph[ks] = join4(hh[0], hh[1], hh[2], hh[3]);
            pm[ks] = join4(mm[0], mm[1], mm[2], mm[3]);
            pl[ks] = join4(ll[0], ll[1], ll[2], ll[3]);
        }

        // ---- initial layer: h = W_0 x + b_0 [+ Wc ctx + bc] (nde/made.py:143-146: the context term is NOT rectified, so
        //      one set of accumulators takes both GEMMs; the context stages come first in the stream)
        {
            f32x16 h[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) load_bias_tile(h[t], bias + t * 32);
            if (ctx) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f32x16 bc;
                    load_bias_tile(bc, bias + 128 + t * 32);
                    h[t] += bc;
                }
                made_rqs_context(h, s_ctx, a.ce, a.ctx_ks, half, r, sm, lane);
            }
            made_rqs_initial(h, ph, pm, pl, a.init_ks, sm, lane);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                tile_to_pieces<false>(h[t], ph[2 * t], pm[2 * t], pl[2 * t], ph[2 * t + 1], pm[2 * t + 1], pl[2 * t + 1]);
        }
        bias += ctx ? 256 : 128;

        if (resnet) {
            // ---- residual blocks: h += W_1 relu(W_0 relu(h) + b_0 [+ Wcb ctx]) + b_1 (nde/made.py:98-111; the block's
            //      context bias is folded into b_0 by the packer)
            for (int blk = 0; blk < (a.num_hidden >> 1); ++blk) {
                bf16x8 qh[8], qm[8], ql[8];
                {
                    f32x16 u[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) load_bias_tile(u[t], bias + t * 32);
                    gemm_kmajor<true, 8>(u, ph, pm, pl, sm, lane);
                    if (ctx) made_rqs_context(u, s_ctx, a.ce, a.ctx_ks, half, r, sm, lane);
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        tile_to_pieces<true>(u[t], qh[2 * t], qm[2 * t], ql[2 * t], qh[2 * t + 1], qm[2 * t + 1], ql[2 * t + 1]);
                }
                f32x16 v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    load_bias_tile(v[t], bias + 128 + t * 32);
                    add_pieces(v[t], 0, ph[2 * t], pm[2 * t], pl[2 * t]);
                    add_pieces(v[t], 8, ph[2 * t + 1], pm[2 * t + 1], pl[2 * t + 1]);
                }
                gemm_kmajor<false, 8>(v, qh, qm, ql, sm, lane);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    tile_to_pieces<false>(v[t], ph[2 * t], pm[2 * t], pl[2 * t], ph[2 * t + 1], pm[2 * t + 1], pl[2 * t + 1]);
                bias += 256;
            }
        } else {
            // ---- feed-forward blocks: h = relu(W h + b) (nde/made.py:64-66), the first one on the RAW initial layer: the
            //      ReLU sits where a block's result becomes pieces, not on a GEMM's input
            for (int hl = 0; hl < a.num_hidden; ++hl) {
                f32x16 u[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) load_bias_tile(u[t], bias + t * 32);
                gemm_kmajor<false, 8>(u, ph, pm, pl, sm, lane);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    tile_to_pieces<true>(u[t], ph[2 * t], pm[2 * t], pl[2 * t], ph[2 * t + 1], pm[2 * t + 1], pl[2 * t + 1]);
                bias += 128;
            }
        }

        // ---- final layer and mixture element, a pair of features at a time: T tiles give lane-half h the 16 T values
        //      (3 K of them the feature's (logit, mean, unconstrained std) x K, the rest from zero rows) of feature 2 g + h.
        //      A lane adds its features' terms in float64, pair after pair.  With an odd number of features the last
        //      pair's second lane-half has none: its term is replaced by exactly 0.
        double row_sum = 0.0;
        for (int g = 0; g < ((D + 1) >> 1); ++g) {
            const int f = g * 2 + half;
            const bool live = f < D;
            const float held = s_row[(live ? f : 0) * kRowPad + r];
            const float xin = live ? held : 0.0f;
            float p[16 * T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                // (products first, the bias last: the order of K29 and of K30's step loop)
                f32x16 acc = {0}, b;
                gemm_tile<false>(acc, ph, pm, pl, sm, lane);
                load_bias_tile(b, bias + (g * T + t) * 32);
#pragma unroll
                for (int q = 0; q < 16; ++q) p[16 * t + q] = acc[q] + b[q];
            }
            const double term = mog_term<KMAX>(xin, p, a.K, a.epsilon);
            row_sum += live ? term : 0.0;
        }

        // ---- the lane pair's two sums joined by one shuffle, `add` inside the float64 sum, ONE rounding
        row_sum += __shfl_xor(row_sum, 32, kWave);
        if (half == 0) {
            if (a.add) row_sum += (double)a.add[row0 + r];
            a.out[row0 + r] = (float)row_sum;
        }
        // stores and LDS-DMA requests complete out of order with each other: drain before the next
        // row block counts outstanding requests again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the two stages requested past the end
}

}  // namespace nfa
