// The kernel body of K32 (rqs_resnet_wide.hip and its rqs_resnet_wide_bins_*.hip): ONE spline coupling layer whose
// ResidualNet conditioner (nn/nets/resnet.py:55-100) is wider than the 128 hidden units of K8 -- 129 .. 256, zero-padded by
// the packer to Hp, a multiple of 32 -- in one launch, both directions: gather of the identity columns, conditioner, final
// Linear, spline on the logits while they are accumulators (coupling.py:73-130, :549-582), per-row logabsdet, scatter.
//
// Arithmetic: K8's (three bf16 pieces per fp32 operand, six products per k-step on v_mfma_f32_32x32x16_bf16, NFA_MFMA6):
// the full fp32 range, no row block is ever given up, no redo pass.
//
// Work split.  A wave of K8 keeps its 32 rows x 128 activations in registers as pieces; at 256 columns that is 192
// registers for one set of activations, and a residual block needs two sets beside its accumulators.  So the GEMMs are
// split by COLUMNS (K8c's idea, on K8's 32 x 32 tiles): one workgroup of eight waves per CU works on two 32-row tiles
// (64 rows), persistent over the 64-row blocks of the batch.  Wave w owns hidden columns 32 w .. 32 w + 31 of every
// hidden GEMM for both row tiles: two accumulator tiles.  Its slice of the residual stream stays in fp32 in those
// accumulators across the blocks (the skip connection is the second Linear accumulating on top of it).
//   * Weights: a wave reads only its own column tile's fragments, from global memory straight into registers -- no other
//     wave needs them, so there is nothing to share through LDS.  Two k-steps are in flight beside the two in use; the
//     last two requests of a GEMM fetch the first fragments of the wave's NEXT GEMM, so the exchange and its barriers
//     hide that latency.
//   * Exchange buffer: after a GEMM the wave applies the ReLU where the next Linear wants it, splits its 32 columns x
//     64 rows into three bf16 pieces and stores them in LDS in B-fragment layout, [k-step of 16][row tile][piece][lane]
//     x 16 B: k-steps 2 w, 2 w + 1 of the next GEMM ARE wave w's block (ops._k8_column_order, over Hp columns).
//     16 k-steps x 2 x 3 x 1 KB = 96 KB at Hp = 256; with the row tile ([Dp <= 128][65] floats, 33 KB) a second half
//     as in K8c does not fit the CU's 160 KB.  Double-buffering only some pieces would still need the second barrier
//     for the others, so TWO barriers go around each exchange (all waves have read the old pieces | the new ones are
//     visible): ~1 us of barriers per residual block against its two GEMMs' 2 x 16 k-steps x 12 MFMAs per wave, two
//     waves per SIMD -- about 10 us.
//   * Narrow widths: tile count Hp / 32 and k-step count Hp / 16 are run-time values; a wave whose column tile lies
//     beyond Hp computes nothing in the hidden GEMMs, keeps every barrier and takes its share of the final layer.
//   * Final Linear and spline (K29's scheme, made_rqs_kernel.hpp): per pair of transformed features T = ceil((3 K - 1)
//     / 16) output tiles whose accumulators are the lane-half's feature's logits, evaluated by the register instance
//     of rqs_math.hpp; the pairs are dealt over the eight waves; the B operand -- all Hp k of both row tiles, 384
//     registers -- is read from the exchange buffer k-step by k-step.  Results replace the inputs in their slots of the
//     row tile; the waves' logabsdet shares meet in LDS and are summed per row in wave order.
#pragma once

#include "bf16x3_gemm.hpp"

#include <hip/hip_ext.h>
#include <stdlib.h>

namespace nfa {
namespace k32 {

constexpr int kWaves = 8, kThreads = kWaves * kWave;
constexpr int kRows = 64, kPad = 65;          // rows of a workgroup; row tile [column][65]
constexpr int kFragVec4 = 3 * kWave;          // one (column tile, k-step) of a weight: [piece][lane] x 16 B
constexpr int kStepVec4 = 2 * 3 * kWave;      // one k-step of the exchange buffer: [row tile][piece][lane] x 16 B

struct WideArgs {
    const float* x;          // [B, D]
    const vec4f* w;          // fragments: initial [tiles][init_ks], 2 num_blocks x [tiles][nks], final [dt / 2 * T][nks]
    const float* bias;       // accumulator order: initial [Hp], per block [Hp][Hp], final [dt / 2 * T * 32]
    const int32_t* tables;   // [128] slots of the identity / transformed features, [128] final
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;           // multiple of 128
    int D, dt, di, num_blocks, accumulate;
    int tiles, nks, init_ks; // Hp / 32, Hp / 16, k-steps of the initial layer (ceil(di / 16))
    RqsDev sp;
};

struct Frag {
    vec4f h, m, l;
};
__device__ __forceinline__ Frag load_frag(const vec4f* p) { return Frag{p[0], p[kWave], p[2 * kWave]}; }

// one k-step: the wave's weight fragment against the pieces of both row tiles
__device__ __forceinline__ void kstep(f32x16 (&acc)[2], const Frag& f, const uvec4* xk) {
    const bf16x8 ah = __builtin_bit_cast(bf16x8, f.h), am = __builtin_bit_cast(bf16x8, f.m), al = __builtin_bit_cast(bf16x8, f.l);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        const bf16x8 bh = __builtin_bit_cast(bf16x8, xk[(rt * 3 + 0) * kWave]);
        const bf16x8 bm = __builtin_bit_cast(bf16x8, xk[(rt * 3 + 1) * kWave]);
        const bf16x8 bl = __builtin_bit_cast(bf16x8, xk[(rt * 3 + 2) * kWave]);
        NFA_MFMA6(acc[rt], ah, am, al, bh, bm, bl);
    }
}

// acc[rt] += W_tile[32 x 16 nks] x act^T[16 nks x 32 rows of tile rt], the activations as pieces in the exchange buffer.
// f0 / f1: the fragments of k-steps 0, 1 on entry, those of `wnext` (the wave's next GEMM) on exit.  nks is even.
__device__ __forceinline__ void gemm_exchange(f32x16 (&acc)[2], const vec4f* wl, const vec4f* wnext, int nks, Frag& f0,
                                              Frag& f1, const uvec4* xl) {
    for (int ks = 0; ks < nks; ks += 2) {
        const vec4f* ahead = ks + 2 < nks ? wl + (size_t)(ks + 2) * kFragVec4 : wnext;
        const Frag f2 = load_frag(ahead), f3 = load_frag(ahead + kFragVec4);
        kstep(acc, f0, xl + ks * kStepVec4);
        kstep(acc, f1, xl + (ks + 1) * kStepVec4);
        f0 = f2;
        f1 = f3;
    }
}

// the wave's 32 columns x 64 rows (activated) -> pieces of k-steps 2 w, 2 w + 1 in the exchange buffer
template <int ACT>
__device__ __forceinline__ void exchange_store(const f32x16 (&acc)[2], uvec4* X, int wave, int lane) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
        bf16x8 h0, m0, l0, h1, m1, l1;
        tile_to_pieces<ACT>(acc[rt], h0, m0, l0, h1, m1, l1);
        uvec4* p = X + (2 * wave) * kStepVec4 + rt * 3 * kWave + lane;
        p[0 * kWave] = __builtin_bit_cast(uvec4, h0);
        p[1 * kWave] = __builtin_bit_cast(uvec4, m0);
        p[2 * kWave] = __builtin_bit_cast(uvec4, l0);
        p[kStepVec4 + 0 * kWave] = __builtin_bit_cast(uvec4, h1);
        p[kStepVec4 + 1 * kWave] = __builtin_bit_cast(uvec4, m1);
        p[kStepVec4 + 2 * kWave] = __builtin_bit_cast(uvec4, l1);
    }
}

// every wave has read the old pieces | the new ones are visible
#define NFA_K32_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

template <bool INVERSE, int KB>
__global__ void __launch_bounds__(kThreads, 1) rqs_resnet_wide_kernel(const WideArgs a) {
#pragma clang fp contract(off)
    constexpr int T = (3 * KB - 1 + 15) / 16;   // 32-row tiles per pair of features
    // dynamic LDS: the exchange buffer (nks x 6 KB), the row tile [D][65], the waves' logabsdet shares [8][64]
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    __shared__ int s_tab[kTabLayer];
    __shared__ int s_final[128];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, dt = a.dt, nks = a.nks, tiles = a.tiles, nb = a.num_blocks;
    int my_status = 0;
    if (tid < kTabLayer) {
        const bool used = tid < kTabTr ? tid < a.di : tid - kTabTr < dt;
        int v = a.tables[tid], f = a.tables[kTabLayer + tid];
        if ((used && (v < 0 || v >= D)) || (tid < D && (f < 0 || f >= D))) my_status |= NFA_STATUS_BAD_INDEX;
        s_tab[tid] = v < 0 ? 0 : (v >= D ? D - 1 : v);
        s_final[tid] = f < 0 ? 0 : (f >= D ? D - 1 : f);
    }
    uvec4* X = reinterpret_cast<uvec4*>(lds_dyn);
    float* s_row = lds_dyn + (size_t)nks * kStepVec4 * 4;
    float* s_lad = s_row + D * kPad;
    const uvec4* xl = X + lane;

    // where this wave's fragments live
    const bool active = wave < tiles;                               // owns a column tile of the hidden GEMMs
    const int pairs = dt >> 1;
    const size_t hidden_vec4 = (size_t)tiles * nks * kFragVec4;     // one hidden GEMM
    const vec4f* w_init = a.w + (size_t)(active ? wave : 0) * a.init_ks * kFragVec4 + lane;
    const vec4f* w_hidden = a.w + (size_t)tiles * a.init_ks * kFragVec4 + (size_t)(active ? wave : 0) * nks * kFragVec4 + lane;
    const vec4f* w_final = a.w + (size_t)tiles * a.init_ks * kFragVec4 + 2 * nb * hidden_vec4 + lane;   // + tile * nks * kFragVec4
    const vec4f* w_my_final = w_final + (size_t)(wave < pairs ? wave : 0) * T * nks * kFragVec4;
    // the wave's first GEMM behind the initial layer, and the one behind its last hidden GEMM (a wave without a pair of
    // features goes straight to the next row block)
    const vec4f* w_first = active && nb > 0 ? w_hidden : w_my_final;
    const vec4f* w_behind_hidden = wave < pairs ? w_my_final : w_first;
    RqsDev sp = a.sp;
    sp.divisor = 0.0f;   // 1/sqrt(hidden_features) is folded into the weight rows

    // the first two fragments of the wave's first GEMM: every GEMM leaves those of the wave's next one behind
    Frag f0 = load_frag(w_first), f1 = load_frag(w_first + kFragVec4);

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

        f32x16 h[2];   // the wave's slice of the residual stream: columns 32 w .. 32 w + 31 of both row tiles
        // ---- initial layer: h = W_i x + b_i; every wave gathers the identity features itself (k = ks*16 + half*8 + j)
        if (active) {
            const float* bias = a.bias + wave * 32 + half * 16;
            load_bias_tile(h[0], bias);
            h[1] = h[0];
            for (int ks = 0; ks < a.init_ks; ++ks) {
                const Frag f = load_frag(w_init + (size_t)ks * kFragVec4);
                const bf16x8 ah = __builtin_bit_cast(bf16x8, f.h), am = __builtin_bit_cast(bf16x8, f.m),
                             al = __builtin_bit_cast(bf16x8, f.l);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int i = ks * 16 + half * 8 + j;
                        const float xv = s_row[s_tab[kTabId + i] * kPad + rt * 32 + r];
                        v[j] = i < a.di ? xv : 0.0f;
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

        // ---- residual blocks: h += W_1 relu(W_0 relu(h) + b_0) + b_1 (resnet.py:36-52, no context)
        for (int b = 0; b < nb; ++b) {
            const float* bias = a.bias + (size_t)(1 + 2 * b) * tiles * 32 + wave * 32 + half * 16;
            const vec4f* w0 = w_hidden + (size_t)(2 * b) * hidden_vec4;
            f32x16 u[2];
            if (b > 0) NFA_K32_BARRIER();   // (the first block: nobody has read the buffer in this row block)
            if (active) exchange_store<kActRelu>(h, X, wave, lane);
            NFA_K32_BARRIER();
            if (active) {
                load_bias_tile(u[0], bias);
                u[1] = u[0];
                gemm_exchange(u, w0, w0 + hidden_vec4, nks, f0, f1, xl);
            }
            NFA_K32_BARRIER();
            if (active) exchange_store<kActRelu>(u, X, wave, lane);
            NFA_K32_BARRIER();
            if (active) {
                f32x16 b1;
                load_bias_tile(b1, bias + tiles * 32);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    h[0][q] += b1[q];
                    h[1][q] += b1[q];
                }
                gemm_exchange(h, w0 + hidden_vec4, b + 1 < nb ? w0 + 2 * hidden_vec4 : w_behind_hidden, nks, f0, f1, xl);
            }
        }
        // ---- the stream as it is (resnet.py:99) becomes the final layer's B operand
        if (nb > 0) NFA_K32_BARRIER();
        if (active) exchange_store<kActNone>(h, X, wave, lane);
        NFA_K32_BARRIER();

        // ---- final Linear and spline, a pair of features at a time: T tiles give lane-half `half` the 16 T (3 KB - 1,
        //      zero padded) logits of feature 2 g + half for both row tiles; the results replace the inputs in their slots
        float lad_acc[2] = {0.0f, 0.0f};
        const float* fbias = a.bias + (size_t)(1 + 2 * nb) * tiles * 32 + half * 16;
        for (int g = wave; g < pairs; g += kWaves) {
            float* slot = s_row + s_tab[kTabTr + g * 2 + half] * kPad + r;
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
                gemm_exchange(acc, wl, wnext, nks, f0, f1, xl);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    p0[16 * t + q] = acc[0][q];
                    p1[16 * t + q] = acc[1][q];
                }
            }
            float y, l;
            my_status |= rqs_eval<KB, INVERSE, true, true>(slot[0], p0, sp, y, l);
            slot[0] = y;
            lad_acc[0] += l;
            my_status |= rqs_eval<KB, INVERSE, true, true>(slot[32], p1, sp, y, l);
            slot[32] = y;
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

typedef void (*WideKernelFn)(const WideArgs);
WideKernelFn wide_bins_low(int K, bool inverse);    // 2 .. 5 bins (one tile per pair of features) and 12 .. 16 (three),
                                                    // rqs_resnet_wide_bins_a.hip
WideKernelFn wide_bins_mid(int K, bool inverse);    // 6 .. 11 (two tiles), rqs_resnet_wide_bins_b.hip

}  // namespace k32
}  // namespace nfa
