// The kernel body of K34 (made_rqs_wide.hip and its made_rqs_wide_bins_*.hip): the density pass of ONE masked autoregressive
// rational-quadratic spline layer (autoregressive.py:404-495) whose MADE (made.py:233-311) has 129 .. 256 hidden units --
// zero-padded by the packer to Hp, a multiple of 32 -- in one launch: the MADE, its final Linear, the spline on the logits
// while they are accumulators, the per-row logabsdet.  The logits never reach memory.
//
// Arithmetic: K8's (three bf16 pieces per fp32 operand, six products per k-step on v_mfma_f32_32x32x16_bf16): the full fp32
// range, no redo pass -- on K29's split accumulators (NFA_MFMA6_SPLIT) in every GEMM but the final layer's at 12 .. 16
// bins (see gemm_exchange_split).  The 0/1 masks are multiplied into the weights by the packer (K22 / K29's rule): a
// masked-out weight is an exact zero in all three pieces, so a feature's result does not depend on the features behind
// it, bit for bit.
//
// Work split: K32's (rqs_resnet_wide_kernel.hpp, whose fragment load, exchange store and barrier are used as they are).
// One workgroup of eight waves per CU on 64 rows (two 32-row tiles), persistent over the batch's 64-row blocks; wave w owns
// hidden columns 32 w .. 32 w + 31 of every hidden GEMM; its slice of the residual stream (or of the feed-forward
// activation) stays in fp32 in two accumulator tiles; weight fragments go from global memory straight into registers, one
// k-step ahead, the last request of a GEMM being the first fragment of the wave's next one; activations travel as
// bf16 pieces through the LDS exchange buffer [k-step][row tile][piece][lane] x 16 B between two barriers.
//
// What a MADE changes against K32's ResidualNet:
//   * Every feature is read by the conditioner AND transformed: all D <= 64 columns of the 64 rows sit in one LDS tile
//     [Dp][65] (Dp = D rounded up to 4: <= 16 640 B); the initial layer reads it in ceil(D / 16) k-steps, the spline takes
//     feature f's input from slot f and leaves z there; a slot has one reader and one writer behind the initial layer,
//     the lane-half that owns the feature.  The tile is stored once.
//   * Blocks come in two forms (a workgroup-uniform run-time branch around the same GEMM loop, as in K29): residual,
//     h += W_1 relu(W_0 relu(h) + b_0) + b_1, and feed-forward, h = relu(W h + b) with h_0 = relu(W_i x + b_i)
//     (made.py:197-206): kept here as pre = W relu(pre) + b with the ReLU applied once in front of every exchange, the
//     final layer's included; there is no skip.  Feed-forward MADEs may have random masks: masks are data at pack time.
//   * The final Linear has ceil(D / 2) pairs of features, T = ceil((3 K - 1) / 16) tiles each, dealt over the eight waves.
//     With an odd D the last pair's second lane-half has no feature: its rows are zero, it evaluates a value outside the
//     box (passes through, log-derivative exactly 0) and writes nothing.
//   * A row's logabsdet: pair after pair within a wave, the two lane-halves, then the waves in their order -- an order the
//     shape alone fixes, so results are the same bits for any batch, grid and call.
//
// LDS: exchange buffer Hp / 16 x 6 KB (96 KB at Hp = 256) + row tile (<= 16 640 B) + logabsdet shares 2 KB + tables 1 KB:
// 118 016 B at the largest shape.
#pragma once

#include "rqs_resnet_wide_kernel.hpp"

namespace nfa {
namespace k34 {

using k32::Frag;
using k32::kFragVec4;
using k32::kPad;
using k32::kRows;
using k32::kStepVec4;
using k32::kThreads;
using k32::kWaves;

struct MadeWideArgs {
    const float* x;          // [B, D]
    const vec4f* w;          // fragments: initial [tiles][init_ks], num_hidden x [tiles][nks], final [pairs * T][nks]
    const float* bias;       // accumulator order: initial [Hp], per hidden Linear [Hp], final [pairs * T * 32]
    const int32_t* tables;   // [128] slots of the features (both halves), [128] final
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;           // multiple of 128
    int D, dt;               // row length (multiple of 4), features
    int num_hidden;          // hidden Linears: two per residual block, one per feed-forward block
    int resnet;              // residual blocks / feed-forward blocks
    int accumulate;
    int tiles, nks, init_ks; // Hp / 32, Hp / 16, k-steps of the initial layer (ceil(dt / 16))
    RqsDev sp;
};

// K32's k-step and GEMM loop on split accumulators (NFA_MFMA6_SPLIT, fused_common.hpp, as K29 has them): the leading product
// accumulates alone, the five small ones in `small`, added once at the end of the GEMM -- the main accumulator is rounded
// once per k-step instead of six times.  SPLIT = false is K32's single accumulator: the final layer's at three tiles per pair of
// features (12 .. 16 bins), where 96 logits stay in registers beside the GEMM and a second set of accumulators does not fit.
template <bool SPLIT>
__device__ __forceinline__ void kstep_split(f32x16 (&acc)[2], f32x16 (&small)[2], const Frag& f, const uvec4* xk) {
    const bf16x8 ah = __builtin_bit_cast(bf16x8, f.h), am = __builtin_bit_cast(bf16x8, f.m), al = __builtin_bit_cast(bf16x8, f.l);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const bf16x8 bh = __builtin_bit_cast(bf16x8, xk[(rt * 3 + 0) * kWave]);
        const bf16x8 bm = __builtin_bit_cast(bf16x8, xk[(rt * 3 + 1) * kWave]);
        const bf16x8 bl = __builtin_bit_cast(bf16x8, xk[(rt * 3 + 2) * kWave]);
        if constexpr (SPLIT) {
            NFA_MFMA6_SPLIT(acc[rt], small[rt], ah, am, al, bh, bm, bl);
        } else {
            NFA_MFMA6(acc[rt], ah, am, al, bh, bm, bl);
        }
    }
}

// acc[rt] += W_tile[32 x 16 nks] x act^T[16 nks x 32 rows of tile rt], the activations as pieces in the exchange buffer.
// f0: the fragment of k-step 0 on entry, that of `wnext` (the wave's next GEMM) on exit.  The second set of accumulators
// takes the registers of K32's second pair of fragments in flight: one k-step (twelve MFMAs, and the other wave of the
// SIMD's twelve) hides a fragment's latency here.  wl / wnext are wave-uniform; the lane is added at the load.
template <bool SPLIT>
__device__ __forceinline__ void gemm_exchange_split(f32x16 (&acc)[2], const vec4f* wl, const vec4f* wnext, int nks, Frag& f0,
                                                    const uvec4* xl, int lane) {
    f32x16 small[2] = {{0}, {0}};
    for (int ks = 0; ks < nks; ++ks) {
        const Frag f1 = k32::load_frag((ks + 1 < nks ? wl + (size_t)(ks + 1) * kFragVec4 : wnext) + lane);
        kstep_split<SPLIT>(acc, small, f0, xl + ks * kStepVec4);
        f0 = f1;
    }
    if constexpr (SPLIT) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc[rt] += small[rt];
    }
}

template <int KB>
__global__ void __launch_bounds__(kThreads, 1) made_rqs_wide_kernel(const MadeWideArgs a) {
#pragma clang fp contract(off)
    constexpr int T = (3 * KB - 1 + 15) / 16;   // 32-row tiles per pair of features
    // dynamic LDS: the exchange buffer (nks x 6 KB), the row tile [D][65], the waves' logabsdet shares [8][64]
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    __shared__ int s_tab[kTabLayer];
    __shared__ int s_final[128];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, dt = a.dt, nks = a.nks, tiles = a.tiles, nh = a.num_hidden;
    const bool resnet = a.resnet != 0;
    int my_status = 0;
    if (tid < kTabLayer) {
        const bool used = (tid < kTabTr ? tid : tid - kTabTr) < dt;
        int v = a.tables[tid], f = a.tables[kTabLayer + tid];
        if ((used && (v < 0 || v >= D)) || (tid < D && (f < 0 || f >= D))) my_status |= NFA_STATUS_BAD_INDEX;
        s_tab[tid] = v < 0 ? 0 : (v >= D ? D - 1 : v);
        s_final[tid] = f < 0 ? 0 : (f >= D ? D - 1 : f);
    }
    uvec4* X = reinterpret_cast<uvec4*>(lds_dyn);
    float* s_row = lds_dyn + (size_t)nks * kStepVec4 * 4;
    float* s_lad = s_row + D * kPad;
    const uvec4* xl = X + lane;

    // where this wave's fragments live (wave-uniform pointers: the lane is added at the load)
    const bool active = wave < tiles;                               // owns a column tile of the hidden GEMMs
    const int pairs = (dt + 1) >> 1;
    const size_t hidden_vec4 = (size_t)tiles * nks * kFragVec4;     // one hidden GEMM
    const vec4f* w_init = a.w + (size_t)(active ? wave : 0) * a.init_ks * kFragVec4;
    const vec4f* w_hidden = a.w + (size_t)tiles * a.init_ks * kFragVec4 + (size_t)(active ? wave : 0) * nks * kFragVec4;
    const vec4f* w_final = a.w + (size_t)tiles * a.init_ks * kFragVec4 + nh * hidden_vec4;   // + tile * nks * kFragVec4
    const vec4f* w_my_final = w_final + (size_t)(wave < pairs ? wave : 0) * T * nks * kFragVec4;
    // the wave's first GEMM behind the initial layer, and the one behind its last hidden GEMM (a wave without a pair of
    // features goes straight to the next row block)
    const vec4f* w_first = active && nh > 0 ? w_hidden : w_my_final;
    const vec4f* w_behind_hidden = wave < pairs ? w_my_final : w_first;
    RqsDev sp = a.sp;
    sp.divisor = 0.0f;   // 1/sqrt(hidden_features) is folded into the weight rows
    sp.rdivisor = 0.0f;
    const float outside = 2.0f * sp.right + 1.0f;   // what a lane-half without a feature evaluates

    // the first fragment of the wave's first GEMM: every GEMM leaves that of the wave's next one behind
    Frag f0 = k32::load_frag(w_first + lane);

    const int64_t num_blocks64 = a.batch >> 6;
    for (int64_t blk = blockIdx.x; blk < num_blocks64; blk += gridDim.x) {
        const int64_t row0 = blk << 6;
        int lane_here = lane;
        asm volatile("" : "+v"(lane_here));
        const int half = lane_here >> 5, r = lane_here & 31;
        // ---- the 64 rows: one coalesced read; slot j of the tile = input column j
        {
            const vec4f* xv = reinterpret_cast<const vec4f*>(a.x + row0 * D);
            const int nvec = D * (kRows / 4);
            for (int e0 = tid; e0 < nvec; e0 += kThreads * 4) {
                vec4f v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kThreads;
                    v[u] = xv[e < nvec ? e : 0];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * kThreads;
                    if (e < nvec) {
                        const int rr = (e * 4) / D, c0 = e * 4 - rr * D;
                        s_row[(c0 + 0) * kPad + rr] = v[u].x;
                        s_row[(c0 + 1) * kPad + rr] = v[u].y;
                        s_row[(c0 + 2) * kPad + rr] = v[u].z;
                        s_row[(c0 + 3) * kPad + rr] = v[u].w;
                    }
                }
            }
        }
        __syncthreads();

        f32x16 h[2];   // the wave's slice of the stream: columns 32 w .. 32 w + 31 of both row tiles
        // ---- initial layer: h = W_i x + b_i over ALL features (masked); k = ks*16 + half*8 + j
        if (active) {
            const float* bias = a.bias + wave * 32 + half * 16;
            load_bias_tile(h[0], bias);
            h[1] = h[0];
            for (int ks = 0; ks < a.init_ks; ++ks) {
                const Frag f = k32::load_frag(w_init + (size_t)ks * kFragVec4 + lane);
                const bf16x8 ah = __builtin_bit_cast(bf16x8, f.h), am = __builtin_bit_cast(bf16x8, f.m),
                             al = __builtin_bit_cast(bf16x8, f.l);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int i = ks * 16 + half * 8 + j;   // (< 64: init_ks <= 4)
                        const float xv = s_row[s_tab[kTabId + i] * kPad + rt * 32 + r];
                        v[j] = i < dt ? xv : 0.0f;
                    }
                    bf16x2 hh[4], mm[4], ll[4];
#pragma unroll
                    for (int j2 = 0; j2 < 4; ++j2) split3(vec2f{v[j2 * 2], v[j2 * 2 + 1]}, hh[j2], mm[j2], ll[j2]);
                    const bf16x8 bh = join4(hh[0], hh[1], hh[2], hh[3]), bm = join4(mm[0], mm[1], mm[2], mm[3]),
                                 bl = join4(ll[0], ll[1], ll[2], ll[3]);
                    NFA_MFMA6(h[rt], ah, am, al, bh, bm, bl);
                }
            }
        }

        const float* hbias = a.bias + (size_t)tiles * 32 + wave * 32 + half * 16;   // + tiles * 32 per hidden Linear
        if (resnet) {
            // ---- residual blocks: h += W_1 relu(W_0 relu(h) + b_0) + b_1 (made.py:129-137, no context)
            for (int j = 0; j < nh; j += 2) {
                const float* bias = hbias + (size_t)j * tiles * 32;
                const vec4f* w0 = w_hidden + (size_t)j * hidden_vec4;
                f32x16 u[2];
                if (j > 0) NFA_K32_BARRIER();   // (the first block: nobody has read the buffer in this row block)
                if (active) k32::exchange_store<kActRelu>(h, X, wave, lane);
                NFA_K32_BARRIER();
                if (active) {
                    load_bias_tile(u[0], bias);
                    u[1] = u[0];
                    gemm_exchange_split<true>(u, w0, w0 + hidden_vec4, nks, f0, xl, lane);
                }
                NFA_K32_BARRIER();
                if (active) k32::exchange_store<kActRelu>(u, X, wave, lane);
                NFA_K32_BARRIER();
                if (active) {
                    f32x16 b1;
                    load_bias_tile(b1, bias + tiles * 32);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        h[0][q] += b1[q];
                        h[1][q] += b1[q];
                    }
                    gemm_exchange_split<true>(h, w0 + hidden_vec4, j + 2 < nh ? w0 + 2 * hidden_vec4 : w_behind_hidden, nks, f0, xl, lane);
                }
            }
        } else {
            // ---- feed-forward blocks: pre = W relu(pre) + b (made.py:96-98 with the ReLU moved in front of the Linear)
            for (int j = 0; j < nh; ++j) {
                const vec4f* wj = w_hidden + (size_t)j * hidden_vec4;
                if (j > 0) NFA_K32_BARRIER();
                if (active) k32::exchange_store<kActRelu>(h, X, wave, lane);
                NFA_K32_BARRIER();
                if (active) {
                    load_bias_tile(h[0], hbias + (size_t)j * tiles * 32);
                    h[1] = h[0];
                    gemm_exchange_split<true>(h, wj, j + 1 < nh ? wj + hidden_vec4 : w_behind_hidden, nks, f0, xl, lane);
                }
            }
        }
        // ---- the final layer's B operand: the residual stream as it is, the feed-forward activation through its ReLU
        if (nh > 0) NFA_K32_BARRIER();
        if (active) {
            if (resnet) k32::exchange_store<kActNone>(h, X, wave, lane);
            else k32::exchange_store<kActRelu>(h, X, wave, lane);
        }
        NFA_K32_BARRIER();

        // ---- final Linear and spline, a pair of features at a time: T tiles give lane-half `half` the 16 T (3 KB - 1,
        //      zero padded) logits of feature 2 g + half for both row tiles; the results replace the inputs in their slots
        float lad_acc[2] = {0.0f, 0.0f};
        const float* fbias = a.bias + (size_t)(1 + nh) * tiles * 32 + half * 16;
        for (int g = wave; g < pairs; g += kWaves) {
            const int f = g * 2 + half;
            const bool live = f < dt;   // (odd dt: the last pair's second half reads its neighbour's slot, writes nothing)
            float* slot = s_row + s_tab[kTabTr + (live ? f : dt - 1)] * kPad + r;
            const float held0 = slot[0], held1 = slot[32];
            const float x0 = live ? held0 : outside, x1 = live ? held1 : outside;
            float p0[16 * T], p1[16 * T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int tile = g * T + t;
                const vec4f* wl = w_final + (size_t)tile * nks * kFragVec4;
                const vec4f* wnext = t + 1 < T ? wl + (size_t)nks * kFragVec4
                                     : g + kWaves < pairs ? w_final + (size_t)(g + kWaves) * T * nks * kFragVec4 : w_first;
                f32x16 acc[2];
                load_bias_tile(acc[0], fbias + tile * 32);
                acc[1] = acc[0];
                gemm_exchange_split<(T < 3)>(acc, wl, wnext, nks, f0, xl, lane);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    p0[16 * t + q] = acc[0][q];
                    p1[16 * t + q] = acc[1][q];
                }
            }
            float y, l;
            my_status |= rqs_eval<KB, false, true, true>(x0, p0, sp, y, l);
            if (live) slot[0] = y;
            lad_acc[0] += l;
            my_status |= rqs_eval<KB, false, true, true>(x1, p1, sp, y, l);
            if (live) slot[32] = y;
            lad_acc[1] += l;
        }
        // ---- a row's logabsdet: the two lane-halves of every wave, then the waves in their order
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            const float s = lad_acc[rt] + __shfl_xor(lad_acc[rt], 32, kWave);
            if (half == 0) s_lad[wave * kRows + rt * 32 + r] = s;
        }
        __syncthreads();
        if (tid < kRows) {
            float s = s_lad[tid];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) s += s_lad[w * kRows + tid];
            float* dst = a.lad + row0 + tid;
            *dst = a.accumulate ? *dst + s : s;
        }
        // ---- output rows: position p of a row comes from slot final[p]; 16 bytes per lane per store
        {
            vec4f* ov = reinterpret_cast<vec4f*>(a.out + row0 * D);
            const int nvec = D * (kRows / 4);
            for (int e = tid; e < nvec; e += kThreads) {
                const int rr = (e * 4) / D, c0 = e * 4 - rr * D;
                vec4f v;
                v.x = s_row[s_final[c0 + 0] * kPad + rr];
                v.y = s_row[s_final[c0 + 1] * kPad + rr];
                v.z = s_row[s_final[c0 + 2] * kPad + rr];
                v.w = s_row[s_final[c0 + 3] * kPad + rr];
                ov[e] = v;
            }
        }
        __syncthreads();   // the row tile, the exchange buffer and the logabsdet shares are free for the next row block
    }
    if (my_status && a.status) atomicOr(a.status, my_status);
}

typedef void (*MadeWideKernelFn)(const MadeWideArgs);
MadeWideKernelFn made_wide_bins_low(int K);    // 2 .. 5 bins (one tile per pair of features) and 12 .. 16 (three),
                                               // made_rqs_wide_bins_a.hip
MadeWideKernelFn made_wide_bins_mid(int K);    // 6 .. 11 (two tiles), made_rqs_wide_bins_b.hip

}  // namespace k34
}  // namespace nfa
