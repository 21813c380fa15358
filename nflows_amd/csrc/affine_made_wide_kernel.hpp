// The kernel body of K36 (affine_made_wide.hip; instances in affine_made_wide_plain.hip / affine_made_wide_ctx.hip): the
// density pass of ONE masked autoregressive affine layer (MaskedAffineAutoregressiveTransform.forward, autoregressive.py:64-128)
// whose MADE (made.py:233-311) has 129 .. 256 hidden units -- zero-padded by the packer to Hp, a multiple of 32 -- in one
// launch: the MADE, its context terms, its final Linear, the affine element on the (shift, unconstrained scale) pairs while
// they are accumulators, the per-row logabsdet.  The [B, 2 D] parameters never reach memory.  K22 (affine_mlp_kernel.hpp)
// serves widths up to 128.
//
// Arithmetic, work split, exchange buffer and the shared pieces of the layer loop: wide_layer_common.hpp.  K36 runs on the
// split-accumulator policy (`gemm_exchange_split<true>`) in every GEMM that reads the exchange buffer, the final one
// included: its tile holds 2 x 16 accumulators per wave, so the second set fits.  The 0/1 masks are multiplied into the
// weights by the packer: a masked-out weight is an exact zero in all three pieces, so a feature's result does not depend on
// the features behind it, bit for bit.  Per element the instructions are K22's and K2b's: `affine_element<false>` on
// `scale_of(u, NFA_SCALE_SOFTPLUS)` under fp contract(off).
//
// What the affine layer changes against K34 (made_rqs_wide_kernel.hpp):
//   * Final Linear: 2 D rows, which the packer puts in K11 / K22's order ([8 shifts | 8 unconstrained scales] per
//     lane-half, ops._made_row_order): one 32-row tile gives lane-half `half` BOTH parameters of features 16 t + 8 half ..
//     + 7 for both row tiles -- ceil(D / 16) <= 4 tiles, tile t on wave t.  Waves 4 .. 7 have no final tile.
//   * Features past D in the last tile have zero weight rows and zero bias, i.e. (shift, u) = (0, 0) -- but
//     log(softplus(0) + 1e-3) is not 0: such a feature is SKIPPED by the `f < dt` test around the element, not evaluated.
//     It reads and writes no slot and adds nothing (not even + 0.0f) to the logabsdet.
//   * A row's logabsdet: the features of a lane in index order, then the two lane-halves (lane r + lane r + 32), then the
//     waves 0 .. 7 in their order through an LDS share (waves without a tile contribute + 0.0f) -- an order the shape alone
//     fixes, so the bits are the same for any batch, grid and call.
//   * CTX (template parameter; the instances without it carry no register or LDS for it): MADE's context terms, K22's two
//     (made.py:187-201).  The 64 rows' context columns sit in a second LDS tile [C][65] behind the logabsdet shares,
//     loaded once per row block; context weights are fragments of ceil(C / 16) k-steps in the packed stream where they are
//     consumed, every wave taking its own 32 columns:
//       - relu(Wc ctx + bc) is computed FIRST; b_i + relu(...) is the initial value of the accumulators the initial
//         layer's products are added to;
//       - per residual block Wcb ctx runs as extra k-steps on the first Linear's accumulators, in front of its ReLU (the
//         packer adds bcb into b_0): the residual loop's `after_w0` hook.  Feed-forward blocks take no context, as the module.
//     Context and initial layer use the same gather + split3 + NFA_MFMA6 loop (`gemm_gather`).
//
// LDS: exchange buffer Hp / 16 x 6 KB (98 304 B at Hp = 256) + row tile [D][65] (<= 16 640 B) + logabsdet shares 2 048 B +
// context tile [C][65] (<= 16 640 B) + tables 1 KB: 134 656 B at the largest shape (Hp 256, D 64, C 64) of the CU's 160 KB.
#pragma once

#include "wide_layer_common.hpp"

namespace nfa {
namespace k36 {

using namespace wide;

struct AffineWideArgs {
    const float* x;          // [B, D]
    const float* ctx;        // [B, ce] (CTX)
    const vec4f* w;          // fragments in the order consumed, see nflows_amd.h (nfa_affine_layer_made_wide_f32)
    const float* bias;       // accumulator order: initial [Hp], context [Hp] (CTX), per hidden Linear [Hp], final [32 per tile]
    const int32_t* tables;   // [128] slots of the features (both halves), [128] final
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;           // multiple of 128
    int D, dt;               // row length (multiple of 4), features
    int ce, ctx_ks;          // context features, their k-steps (ceil(ce / 16))
    int num_hidden;          // hidden Linears: two per residual block, one per feed-forward block
    int resnet;              // residual blocks / feed-forward blocks
    int accumulate;
    int tiles, nks, init_ks; // Hp / 32, Hp / 16, k-steps of the initial layer (ceil(dt / 16))
    int final_tiles;         // ceil(dt / 16)
};

template <bool CTX>
__global__ void __launch_bounds__(kThreads, 1) affine_made_wide_kernel(const AffineWideArgs a) {
#pragma clang fp contract(off)
    // dynamic LDS: the common carve-up, then the context tile [ce][65] (CTX)
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    __shared__ int s_tab[kTabLayer];
    __shared__ int s_final[128];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, dt = a.dt, nks = a.nks, tiles = a.tiles, nh = a.num_hidden;
    const bool resnet = a.resnet != 0;
    int my_status = load_tables(a.tables, tid, D, s_tab, s_final, [&](int t) { return (t < kTabTr ? t : t - kTabTr) < dt; });
    // dynamic LDS, as every wide kernel carves it: exchange buffer (nks x 6 KB), row tile [D][65], logabsdet shares
    uvec4* X = reinterpret_cast<uvec4*>(lds_dyn);
    float* s_row = lds_dyn + (size_t)nks * kStepVec4 * 4;
    float* s_lad = s_row + D * kPad;
    [[maybe_unused]] float* s_ctx = s_lad + kWaves * kRows;
    const uvec4* xl = X + lane;

    // where this wave's fragments live (wave-uniform pointers: the lane is added at the load).  The stream, in the order
    // consumed: [context_layer] initial_layer, per residual block W_0 [block context_layer] W_1 / per feed-forward block W,
    // final_layer; every GEMM is [32-row tile][k-step].
    const bool active = wave < tiles;                               // owns a column tile of the hidden GEMMs
    const int wt = active ? wave : 0;
    const int cks = CTX ? a.ctx_ks : 0;
    const size_t hidden_vec4 = (size_t)tiles * nks * kFragVec4;     // one hidden GEMM
    const size_t ctx_vec4 = (size_t)tiles * cks * kFragVec4;        // one context GEMM
    const size_t block_vec4 = resnet ? 2 * hidden_vec4 + ctx_vec4 : hidden_vec4;   // one block
    const vec4f* w_ctx = a.w + (size_t)wt * cks * kFragVec4;
    const vec4f* w_init = a.w + ctx_vec4 + (size_t)wt * a.init_ks * kFragVec4;
    const vec4f* hidden0 = a.w + ctx_vec4 + (size_t)tiles * a.init_ks * kFragVec4;
    const vec4f* w_hidden = hidden0 + (size_t)wt * nks * kFragVec4;   // the wave's tile of the first hidden Linear
    const vec4f* w_final = hidden0 + (size_t)(resnet ? nh >> 1 : nh) * block_vec4;
    const bool has_final = wave < a.final_tiles;                    // (final_tiles <= 4 < tiles: such a wave is active)
    const vec4f* w_my_final = w_final + (size_t)(has_final ? wave : 0) * nks * kFragVec4;
    // the wave's first GEMM on the exchange buffer, and the one behind its last hidden GEMM (a wave without a final tile
    // goes straight to the next row block)
    const vec4f* w_first = active && nh > 0 ? w_hidden : w_my_final;
    const vec4f* w_behind_hidden = has_final ? w_my_final : w_first;
    const int Hp = tiles * 32;
    const int nbias = CTX ? 2 : 1;                                  // bias vectors in front of the hidden Linears'

    // the first fragment of the wave's first GEMM: every GEMM leaves that of the wave's next one behind
    Frag f0 = load_frag(w_first + lane);
    const auto gemm = [&](f32x16 (&acc)[2], const vec4f* wl, const vec4f* wnext) {
        gemm_exchange_split<true>(acc, wl, wnext, nks, f0, xl, lane);
    };

    const int64_t num_blocks64 = a.batch >> 6;
    for (int64_t blk = blockIdx.x; blk < num_blocks64; blk += gridDim.x) {
        const int64_t row0 = blk << 6;
        int lane_here = lane;
        asm volatile("" : "+v"(lane_here));
        const int half = lane_here >> 5, r = lane_here & 31;
        load_row_tile(a.x + row0 * D, D, s_row, tid);
        if constexpr (CTX) {   // ---- the 64 context rows (64 ce floats from a 256 ce-byte boundary): slot c = context column c
            const int ce = a.ce;
            const vec4f* cv = reinterpret_cast<const vec4f*>(a.ctx + row0 * ce);
            const int nvec = ce * (kRows / 4);   // <= 1024: two per thread
            vec4f v[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = tid + u * kThreads;
                v[u] = cv[e < nvec ? e : 0];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = tid + u * kThreads;
                if (e < nvec) {
                    const float q[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int idx = e * 4 + c, rr = idx / ce;
                        s_ctx[(idx - rr * ce) * kPad + rr] = q[c];
                    }
                }
            }
        }
        __syncthreads();

        f32x16 h[2];   // the wave's slice of the stream: columns 32 w .. 32 w + 31 of both row tiles
        // ---- initial layer: h = W_i x + b_i over ALL features (masked), on top of relu(Wc ctx + bc) where there is a context
        if (active) {
            const float* bias = a.bias + wave * 32 + half * 16;
            if constexpr (CTX) {
                load_bias_tile(h[0], bias + Hp);
                h[1] = h[0];
                gemm_gather<false>(h, w_ctx + lane, cks, s_ctx, nullptr, a.ce, half, r);
                f32x16 b0;
                load_bias_tile(b0, bias);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    h[0][q] = b0[q] + activate<kActRelu>(h[0][q]);
                    h[1][q] = b0[q] + activate<kActRelu>(h[1][q]);
                }
            } else {
                load_bias_tile(h[0], bias);
                h[1] = h[0];
            }
            gemm_gather<true>(h, w_init + lane, a.init_ks, s_row, s_tab + kTabId, dt, half, r);
        }

        // ---- blocks: residual, h += W_1 relu(W_0 relu(h) + b_0 [+ Wcb ctx + bcb]) + b_1 (made.py:129-137), or feed-forward
        //      (made.py:96-98); then the final layer's B operand
        const float* hbias = a.bias + (size_t)nbias * Hp + wave * 32 + half * 16;
        if (resnet)
            residual_blocks(h, nh, active, X, wave, lane, hbias, Hp, w_hidden, block_vec4, hidden_vec4 + ctx_vec4,
                            w_behind_hidden, gemm, [&](f32x16 (&u)[2], const vec4f* w0) {
                                if constexpr (CTX)   // (the block's context GEMM lies behind W_0: its tile `wt` from W_0's tile `wt`)
                                    gemm_gather<false>(u, w0 + (ptrdiff_t)hidden_vec4 + (ptrdiff_t)wt * (cks - nks) * kFragVec4 + lane,
                                                       cks, s_ctx, nullptr, a.ce, half, r);
                            });
        else
            feedforward_blocks(h, nh, active, X, wave, lane, hbias, Hp, w_hidden, hidden_vec4, w_behind_hidden, gemm);
        handover(h, !resnet, nh > 0, active, X, wave, lane);

        // ---- final Linear and affine element: tile `wave` gives lane-half `half` the shifts (registers 0 .. 7) and the
        //      unconstrained scales (8 .. 15) of features 16 wave + 8 half + j for both row tiles; the results replace the
        //      inputs in their slots (one reader and one writer per slot behind the initial layer)
        float lad_acc[2] = {0.0f, 0.0f};
        if (has_final) {
            f32x16 acc[2];
            load_bias_tile(acc[0], a.bias + (size_t)(nbias + nh) * Hp + wave * 32 + half * 16);
            acc[1] = acc[0];
            gemm(acc, w_my_final, w_first);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int f = (wave * 2 + half) * 8 + j;
                if (f < dt) {   // (a feature past dt is skipped, not evaluated: log(softplus(0) + 1e-3) != 0)
                    float* slot = s_row + s_tab[kTabTr + f] * kPad + r;
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) {
                        float y, l;
                        affine_element<false>(slot[rt * 32], acc[rt][j], scale_of(acc[rt][8 + j], NFA_SCALE_SOFTPLUS), y, l);
                        slot[rt * 32] = y;
                        lad_acc[rt] += l;
                    }
                }
            }
        }
        reduce_logabsdet(lad_acc, s_lad, wave, half, r, tid, a.lad + row0, a.accumulate);
        scatter_rows(a.out + row0 * D, D, s_row, s_final, tid);
    }
    if (my_status && a.status) atomicOr(a.status, my_status);
}

typedef void (*AffineWideKernelFn)(const AffineWideArgs);
AffineWideKernelFn affine_wide_plain();     // affine_made_wide_plain.hip
AffineWideKernelFn affine_wide_context();   // affine_made_wide_ctx.hip

}  // namespace k36
}  // namespace nfa
