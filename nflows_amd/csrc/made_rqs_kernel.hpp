// The kernel body of K29 (made_rqs.hip and its made_rqs_bins_*.hip: the density pass of a run of masked autoregressive
// rational-quadratic spline layers in one launch).  Two parents: K22's MADE inside the layer kernel (affine_mlp_kernel.hpp in
// its AUTOREG (+ CTX) mode: masked weights from the packer, the wave's 32 rows resident in an LDS row tile across the layers
// of the run, every hidden activation in registers as pieces before the output tiles overwrite the row's slots in place) and
// K8's final-layer loop for any bin count (rqs_resnet_kernel.hpp: T = ceil((3 K - 1) / 16) tiles per pair of features, the
// 16 T accumulator values of lane-half h being the logits of feature 2 g + h, evaluated by rqs_math.hpp's register instance).
// The template has ONE axis, the bin count; residual / feed-forward blocks, the context and the initial layer's k-steps are
// wave-uniform run-time branches around the same register arrays (statically indexed: nothing goes to scratch).
#pragma once

// (the split accumulators of K11 / K22 / K13: see NFA_MFMA6_SPLIT, fused_common.hpp)
#define NFA_BF16X3_SPLIT_ACC
#include "bf16x3_gemm.hpp"

#include <hip/hip_ext.h>
#include <math.h>
#include <stdlib.h>

namespace nfa {

struct MadeRqsArgs {
    const float* x;         // [B, D]
    const vec4f* w;         // [num_layers * num_stages][768] x 16 bytes
    const float* bias;      // accumulator-order biases of all GEMMs, layer after layer
    const int32_t* tables;  // [num_layers][128] slots of the features (both halves), then [128] final
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;          // multiple of 128
    int D, dt;              // row length (multiple of 4), features
    int num_hidden, num_layers, num_stages, bias_per_layer, accumulate;
    int init_ks;            // k-steps of the initial layer: 2 (features <= 32) or 4
    int resnet;             // residual blocks (two Linears each) / feed-forward blocks (one)
    int normal, skip_out;   // NFA_FLAG_STANDARD_NORMAL_LOG_PROB / NFA_FLAG_SKIP_OUTPUTS
    float log_z;
    int Ds;                 // columns the density sums over (row length minus NFA_FLAG_PAD_COLUMNS)
    const float* ctx;       // with a context: [B, ce]
    int ce, ctx_ks;         // context features, their k-steps (ceil(ce / 16))
    RqsDev sp;              // (divisor 0: 1/sqrt(hidden_features) is folded into the packed rows)
};

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

// One workgroup of four waves per CU (512 registers per wave: the two sets of accumulators, as K22), persistent over the
// 128-row blocks.  Per layer: the MADE (made.py:233-311, masks in the weights) on the row tile's columns, then per pair of
// features T output tiles whose accumulators ARE the 3 KB - 1 logits of the lane-half's feature, the spline on them
// (autoregressive.py:404-495, linear tails) and the result back into the feature's slot.  A row's log-determinant is summed
// feature pair after feature pair, layer after layer, then across the lane pair: an order the shape alone fixes.
template <int KB>
__global__ void __launch_bounds__(kBlock, 1) made_rqs_kernel(const MadeRqsArgs a) {
#pragma clang fp contract(off)
    constexpr int T = (3 * KB - 1 + 15) / 16;   // 32-row tiles per pair of features
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    __shared__ int s_tab[2][kTabLayer];
    __shared__ int s_final[128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, dt = a.dt;
    int my_status = 0;
    auto checked = [&](int v, bool used) {
        if (used && (v < 0 || v >= D)) my_status |= NFA_STATUS_BAD_INDEX;
        return v < 0 ? 0 : (v >= D ? D - 1 : v);
    };
    if (tid < kTabLayer) {
        s_tab[0][tid] = checked(a.tables[tid], (tid < kTabTr ? tid : tid - kTabTr) < dt);
        s_final[tid] = checked(a.tables[a.num_layers * kTabLayer + tid], tid < D);
    }

    WeightStream sm;
    sm.w = a.w;
    sm.ring = reinterpret_cast<vec4f*>(lds_dyn);
    sm.slot = 1;
    sm.fetch = 0;
    sm.num_stages = a.num_stages * a.num_layers;
    sm.tid = tid;
    stream_request(sm);  // stage 0 -> slot 0
    sm.slot = 2;
    stream_request(sm);  // stage 1 -> slot 1
    sm.slot = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    float* s_row = lds_dyn + kRing * kStageVec4 * 4 + wave * D * kRowPad;
    const bool ctx = a.ce > 0, resnet = a.resnet != 0;
    const float* s_ctx = lds_dyn + kRing * kStageVec4 * 4 + (kBlock / kWave) * D * kRowPad + wave * a.ce * kRowPad;
    const int64_t num_quads = a.batch >> 7;
    const float outside = 2.0f * a.sp.right + 1.0f;   // what a lane-half without a feature evaluates: passes through, adds 0
    int tb = 0;

    for (int64_t quad = blockIdx.x; quad < num_quads; quad += gridDim.x) {
        const int64_t row0 = (quad << 7) + (wave << 5);
        int lane_here = lane;
        asm volatile("" : "+v"(lane_here));
        const int half = lane_here >> 5, r = lane_here & 31;
        // ---- the wave's 32 rows: one coalesced read; slot j of the tile = input column j
        {
            const vec4f* xv = reinterpret_cast<const vec4f*>(a.x + row0 * D);
            const int nvec = D * 8;
            for (int e0 = lane; e0 < nvec; e0 += kWave * 4) {
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
        }
        if (ctx) {   // ---- the wave's 32 context rows: slot c of the context tile = context column c
            float* ctile = const_cast<float*>(s_ctx);
            const float* crow = a.ctx + row0 * a.ce;
            const int nctx = 32 * a.ce;
            for (int e0 = lane; e0 < nctx; e0 += kWave * 4) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kWave;
                    v[u] = crow[e < nctx ? e : 0];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kWave;
                    if (e < nctx) {
                        const int rr = e / a.ce, c = e - rr * a.ce;
                        ctile[c * kRowPad + rr] = v[u];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        float lad_acc = 0.0f;
        for (int layer = 0; layer < a.num_layers; ++layer) {
            const int* tab = s_tab[tb];
            // the next layer's table goes to the other half now (read after this layer's stage barriers); a SCALAR branch
            // over whole waves (affine_mlp_kernel.hpp has the story of the per-lane form)
            static_assert(kTabLayer % kWave == 0, "the table is copied by whole waves");
            if (__builtin_amdgcn_readfirstlane(wave) < kTabLayer / kWave) {
                const int nl = layer + 1 < a.num_layers ? layer + 1 : 0;
                s_tab[tb ^ 1][tid] = checked(a.tables[nl * kTabLayer + tid], (tid < kTabTr ? tid : tid - kTabTr) < dt);
            }
            const float* bias = a.bias + (size_t)layer * a.bias_per_layer + half * 16;  // + 32 per tile
            bf16x8 ph[8], pm[8], pl[8];  // the current activations (128 k per sample) as bf16 pieces

            // ---- the layer's input columns: k = ks*16 + half*8 + j (k-steps beyond init_ks are not consumed)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks >= a.init_ks) continue;
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int i = ks * 16 + half * 8 + j;
                    const float xv = s_row[tab[kTabId + i] * kRowPad + r];
                    v[j] = i < dt ? xv : 0.0f;
                }
                bf16x2 hh[4], mm[4], ll[4];
#pragma unroll
                for (int j2 = 0; j2 < 4; ++j2) split3(vec2f{v[j2 * 2], v[j2 * 2 + 1]}, hh[j2], mm[j2], ll[j2]);
                ph[ks] = join4(hh[0], hh[1], hh[2], hh[3]);
                pm[ks] = join4(mm[0], mm[1], mm[2], mm[3]);
                pl[ks] = join4(ll[0], ll[1], ll[2], ll[3]);
            }

            // ---- initial layer: h = W_0 x + b_0 [+ relu(Wc ctx + bc)] (made.py:274-281; its ReLU is the next GEMM's)
            {
                f32x16 h[4];
                if (ctx) {
                    // the context term first, so that one set of accumulators serves both GEMMs
#pragma unroll
                    for (int t = 0; t < 4; ++t) load_bias_tile(h[t], bias + 128 + t * 32);
                    made_rqs_context(h, s_ctx, a.ce, a.ctx_ks, half, r, sm, lane);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        f32x16 b0;
                        load_bias_tile(b0, bias + t * 32);
#pragma unroll
                        for (int q = 0; q < 16; ++q) h[t][q] = b0[q] + activate<kActRelu>(h[t][q]);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) load_bias_tile(h[t], bias + t * 32);
                }
                made_rqs_initial(h, ph, pm, pl, a.init_ks, sm, lane);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    tile_to_pieces<false>(h[t], ph[2 * t], pm[2 * t], pl[2 * t], ph[2 * t + 1], pm[2 * t + 1], pl[2 * t + 1]);
            }
            bias += ctx ? 256 : 128;

            if (resnet) {
                // ---- residual blocks: h += W_1 relu(W_0 relu(h) + b_0 [+ Wcb ctx]) + b_1 (made.py:187-198; the block's
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
                // ---- feed-forward blocks: h = W relu(h) + b, and the ReLU in front of the output layer (made.py:303-311)
                for (int hl = 0; hl < a.num_hidden; ++hl) {
                    f32x16 u[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) load_bias_tile(u[t], bias + t * 32);
                    gemm_kmajor<true, 8>(u, ph, pm, pl, sm, lane);
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        tile_to_pieces<false>(u[t], ph[2 * t], pm[2 * t], pl[2 * t], ph[2 * t + 1], pm[2 * t + 1], pl[2 * t + 1]);
                    bias += 128;
                }
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) relu_pieces(ph[ks], pm[ks], pl[ks]);
            }

            // ---- output layer and spline, a pair of features at a time: T tiles give lane-half h the 16 T (3 KB - 1, zero
            //      padded) logits of feature 2 g + h; the result replaces the input in its slot.  With an odd number of
            //      features the last pair's second lane-half has none: it evaluates a value outside the box on its zero
            //      rows (passes through, log-derivative exactly 0) and writes nothing.
            for (int g = 0; g < ((dt + 1) >> 1); ++g) {
                const int f = g * 2 + half;
                const bool live = f < dt;
                float* slot = s_row + tab[kTabTr + (live ? f : 0)] * kRowPad + r;
                const float held = *slot;
                const float xin = live ? held : outside;
                float p[16 * T];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    // (products first, the bias last -- the order of K28's step loop and of the reference's addmm: the
                    //  logits of the density pass and of the sampling pass then differ by the products' rounding alone)
                    f32x16 acc = {0}, b;
                    gemm_tile<false>(acc, ph, pm, pl, sm, lane);
                    load_bias_tile(b, bias + (g * T + t) * 32);
#pragma unroll
                    for (int q = 0; q < 16; ++q) p[16 * t + q] = acc[q] + b[q];
                }
                float y, l;
                my_status |= rqs_eval<KB, false, true, true>(xin, p, a.sp, y, l);
                if (live) *slot = y;
                lad_acc += l;
            }
            tb ^= 1;
            // this wave's results must be visible to its own gathers of the next layer
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }

        // ---- output rows: position p of a row comes from slot final[p]; 16 bytes per lane per store
        if (!a.skip_out) {
            vec4f* ov = reinterpret_cast<vec4f*>(a.out + row0 * D);
            const int nvec = D * 8;
            for (int e = lane; e < nvec; e += kWave) {
                const int rr = (e * 4) / D, c0 = e * 4 - rr * D;
                vec4f v;
                v.x = s_row[s_final[c0 + 0] * kRowPad + rr];
                v.y = s_row[s_final[c0 + 1] * kRowPad + rr];
                v.z = s_row[s_final[c0 + 2] * kRowPad + rr];
                v.w = s_row[s_final[c0 + 3] * kRowPad + rr];
                ov[e] = v;
            }
        }
        lad_acc += __shfl_xor(lad_acc, 32, kWave);
        float sumsq = 0.0f;
        if (a.normal) sumsq = tile_row_sumsq(s_row, a.Ds, half, r);
        if (half == 0) {
            float* dst = a.lad + row0 + r;
            float v = a.accumulate ? *dst + lad_acc : lad_acc;
            if (a.normal) v = (-0.5f * sumsq - a.log_z) + v;   // normal.py:31-33, flows/base.py:49
            *dst = v;
        }
        // stores and LDS-DMA requests complete out of order with each other: drain before the next
        // row block counts outstanding requests again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the two stages requested past the end
    if (my_status && a.status) atomicOr(a.status, my_status);
}

typedef void (*MadeRqsKernelFn)(const MadeRqsArgs);
MadeRqsKernelFn made_rqs_bins_low(int K);    // 2 .. 5 bins (one tile per pair of features), made_rqs_bins_a.hip
MadeRqsKernelFn made_rqs_bins_mid(int K);    // 6 .. 11 (two tiles), made_rqs_bins_b.hip
MadeRqsKernelFn made_rqs_bins_high(int K);   // 12 .. 16 (three tiles), made_rqs_bins_c.hip

}  // namespace nfa
