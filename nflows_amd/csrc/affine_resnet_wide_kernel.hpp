// The kernel body of K37 (affine_resnet_wide.hip, affine_resnet_wide_mlp.hip): ONE affine or additive coupling layer
// (coupling.py:73-130, :212-269) whose conditioner -- a ResidualNet (nn/nets/resnet.py:55-100) or a ReLU MLP
// (nn/nets/mlp.py:47-68) -- has 129 .. 256 hidden units, zero-padded by the packer to Hp, a multiple of 32, in one launch,
// both directions: gather of the identity columns, conditioner, final Linear, the affine element on the (shift,
// unconstrained scale) pairs while they are accumulators, per-row logabsdet, scatter.  The [B, 2 d_t] parameters never
// reach memory.  K11 (affine_mlp_kernel.hpp) serves widths up to 128.
//
// Arithmetic, work split, exchange buffer and the shared pieces of the layer loop: wide_layer_common.hpp.  K37 runs on the
// split-accumulator policy (NFA_MFMA6_SPLIT, as K11 and K36 have it) in every GEMM that reads the exchange buffer, the
// final one included.  An affine layer shows the shift's error in y as it is, where a spline damps its logits': with the
// single accumulator the outputs of a 129-wide layer came out at 1.8 x (mean) and 2.3 x (99.9 % quantile) the float32
// yardstick's error against float64, outside the project's 2 x rule.  Per element the instructions are K2's and K11's:
// `affine_element<INVERSE>` on `scale_of` under fp contract(off); the additive layer is x + shift / x - shift, exact, with
// a logabsdet of exactly 0.
//
// What is K37's own: the final Linear and the element step.
//   * The final Linear has 2 d_t rows [shift block | unconstrained scale block] (d_t for the additive layer).  The packer
//     puts them in K11's order (ops._affine_row_order): one 32-row output tile gives lane-half `half` the shifts
//     (registers 0 .. 7) and the unconstrained scales (8 .. 15) of features 16 t + 8 half + j; an additive tile the shifts
//     of features 32 t + 16 half + q.  That is at most four tiles.  K32 / K36 give a final tile to one wave for both row
//     tiles, which here would leave four waves idle through a GEMM as long as a hidden one; instead a UNIT is (final tile,
//     row tile): up to 4 x 2 = 8 units, unit u = 2 t + rt on wave u.  A unit's GEMM is one accumulator tile against ONE
//     row tile's pieces (`gemm_exchange_unit`, six MFMAs per k-step), so the final layer takes half a hidden GEMM's time
//     on every wave at 64 transformed features, and the two waves of a tile read the same fragments (the second from L2).
//   * Element step: on the accumulators; x comes from the unit's rows of the row tile in LDS and y goes back into the same
//     slot -- one reader and one writer per (slot, row), no barrier in between.
//   * Features past d_t in the last tile have zero weight rows and zero bias, (shift, u) = (0, 0) -- but log(scale_of(0)) is
//     not 0: such a feature is SKIPPED by the `f < dt` test, not evaluated.  d_t needs no padding to fours.
//   * A row's logabsdet: the features of a lane in index order, then the two lane-halves (lane r + lane r + 32), then the
//     units of the row's tile in tile order through an LDS share [8 units][32 rows] (a wave without a unit contributes
//     + 0.0f) -- an order the shape alone fixes, so the bits are the same for any batch, grid and call.
//
// LDS: exchange buffer Hp / 16 x 6 KB (98 304 B at Hp = 256) + row tile [D][65] (<= 33 280 B) + logabsdet shares 1 KB +
// tables 1 KB: 133 632 B at the largest shape (Hp 256, D 128) of the CU's 160 KB.
#pragma once

#include "wide_layer_common.hpp"

namespace nfa {
namespace k37 {

using namespace wide;

struct AffineWideArgs {
    const float* x;          // [B, D]
    const vec4f* w;          // fragments: initial [tiles][init_ks], num_hidden x [tiles][nks], final [final_tiles][nks]
    const float* bias;       // accumulator order: initial [Hp], per hidden Linear [Hp], final [32 per tile]
    const int32_t* tables;   // [128] slots of the identity / transformed features, [128] final
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;           // multiple of 128
    int D, dt, di;           // row length (multiple of 4), transformed and identity features
    int num_hidden;          // hidden Linears: two per residual block, one per hidden layer of an MLP
    int activation;          // NFA_SCALE_DEFAULT / NFA_SCALE_GENERAL (not read by the additive instances)
    int accumulate;
    int tiles, nks, init_ks; // Hp / 32, Hp / 16, k-steps of the initial layer (ceil(di / 16))
    int final_tiles;         // ceil(dt / 16), additive: ceil(dt / 32)
};

// acc += W_tile[32 x 16 nks] x act^T[16 nks x 32 rows of ONE row tile]: `gemm_exchange_split<true>` for a unit of the final
// layer.  `xu`: the exchange buffer at the unit's row tile and the lane.  f0: the fragment of k-step 0 on entry, that of
// `wnext` (the wave's next GEMM) on exit.  wl / wnext are wave-uniform; the lane is added at the load.
__device__ __forceinline__ void gemm_exchange_unit(f32x16& acc, const vec4f* wl, const vec4f* wnext, int nks, Frag& f0,
                                                   const uvec4* xu, int lane) {
    f32x16 small = {0};
    for (int ks = 0; ks < nks; ++ks) {
        const Frag f1 = load_frag((ks + 1 < nks ? wl + (size_t)(ks + 1) * kFragVec4 : wnext) + lane);
        const uvec4* xk = xu + ks * kStepVec4;
        const bf16x8 ah = __builtin_bit_cast(bf16x8, f0.h), am = __builtin_bit_cast(bf16x8, f0.m),
                     al = __builtin_bit_cast(bf16x8, f0.l);
        const bf16x8 bh = __builtin_bit_cast(bf16x8, xk[0 * kWave]), bm = __builtin_bit_cast(bf16x8, xk[1 * kWave]),
                     bl = __builtin_bit_cast(bf16x8, xk[2 * kWave]);
        NFA_MFMA6_SPLIT(acc, small, ah, am, al, bh, bm, bl);
        f0 = f1;
    }
    acc += small;
}

template <bool INVERSE, bool ADDITIVE, bool RESNET>
__global__ void __launch_bounds__(kThreads, 1) affine_resnet_wide_kernel(const AffineWideArgs a) {
#pragma clang fp contract(off)
    // dynamic LDS: the common carve-up with the units' logabsdet shares [8][32] for the waves'
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    __shared__ int s_tab[kTabLayer];
    __shared__ int s_final[128];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, dt = a.dt, nks = a.nks, tiles = a.tiles, nh = a.num_hidden;
    int my_status = load_tables(a.tables, tid, D, s_tab, s_final, [&](int t) { return t < kTabTr ? t < a.di : t - kTabTr < dt; });
    // dynamic LDS, as every wide kernel carves it: exchange buffer (nks x 6 KB), row tile [D][65], logabsdet shares
    uvec4* X = reinterpret_cast<uvec4*>(lds_dyn);
    float* s_row = lds_dyn + (size_t)nks * kStepVec4 * 4;
    float* s_lad = s_row + D * kPad;
    const uvec4* xl = X + lane;

    // where this wave's fragments live (wave-uniform pointers: the lane is added at the load)
    const bool active = wave < tiles;                               // owns a column tile of the hidden GEMMs
    const int wt = active ? wave : 0;
    const size_t hidden_vec4 = (size_t)tiles * nks * kFragVec4;     // one hidden GEMM
    const vec4f* w_init = a.w + (size_t)wt * a.init_ks * kFragVec4;
    const vec4f* w_hidden = a.w + (size_t)tiles * a.init_ks * kFragVec4 + (size_t)wt * nks * kFragVec4;
    const vec4f* w_final = a.w + (size_t)tiles * a.init_ks * kFragVec4 + nh * hidden_vec4;
    // the wave's unit of the final layer: (final tile, row tile)
    const bool has_unit = wave < 2 * a.final_tiles;
    const int utile = has_unit ? wave >> 1 : 0, urt = wave & 1;
    const vec4f* w_my_final = w_final + (size_t)utile * nks * kFragVec4;
    const uvec4* xu = xl + urt * 3 * kWave;
    // the wave's first GEMM behind the initial layer, and the one behind its last hidden GEMM (a wave without a unit goes
    // straight to the next row block)
    const vec4f* w_first = active && nh > 0 ? w_hidden : w_my_final;
    const vec4f* w_behind_hidden = has_unit ? w_my_final : w_first;
    const int Hp = tiles * 32;
    constexpr int kPerHalf = ADDITIVE ? 16 : 8;   // features of a lane-half per final tile

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
        __syncthreads();

        f32x16 h[2];   // the wave's slice of the stream: columns 32 w .. 32 w + 31 of both row tiles
        // ---- initial layer: h = W_i x + b_i; every wave gathers the identity features itself (k = ks*16 + half*8 + j)
        if (active) {
            load_bias_tile(h[0], a.bias + wave * 32 + half * 16);
            h[1] = h[0];
            gemm_gather<true>(h, w_init + lane, a.init_ks, s_row, s_tab + kTabId, a.di, half, r);
        }
        // ---- residual blocks (resnet.py:36-52, no context) / hidden layers of the MLP (mlp.py:60-66); then the final
        //      layer's B operand: the residual stream as it is (resnet.py:99), the MLP's through its ReLU
        const float* hbias = a.bias + Hp + wave * 32 + half * 16;
        if constexpr (RESNET)
            residual_blocks(h, nh, active, X, wave, lane, hbias, Hp, w_hidden, 2 * hidden_vec4, hidden_vec4, w_behind_hidden,
                            gemm, [](f32x16 (&)[2], const vec4f*) {});
        else
            feedforward_blocks(h, nh, active, X, wave, lane, hbias, Hp, w_hidden, hidden_vec4, w_behind_hidden, gemm);
        handover(h, !RESNET, nh > 0, active, X, wave, lane);

        // ---- final Linear and element step of the wave's unit: tile `utile` against row tile `urt`; the results replace
        //      the inputs in their slots
        float lad_acc = 0.0f;
        if (has_unit) {
            f32x16 acc;
            load_bias_tile(acc, a.bias + (size_t)(1 + nh) * Hp + utile * 32 + half * 16);
            gemm_exchange_unit(acc, w_my_final, w_first, nks, f0, xu, lane);
#pragma unroll
            for (int j = 0; j < kPerHalf; ++j) {
                const int f = (utile * 2 + half) * kPerHalf + j;
                if (f < dt) {   // (a feature past dt is skipped, not evaluated: log(scale_of(0)) != 0)
                    float* slot = s_row + s_tab[kTabTr + f] * kPad + urt * 32 + r;
                    const float xin = *slot, shift = acc[j];
                    float y;
                    if constexpr (ADDITIVE) {
                        y = INVERSE ? xin - shift : xin + shift;   // scale == 1: exact, logabsdet 0
                    } else {
                        float l;
                        affine_element<INVERSE>(xin, shift, scale_of(acc[8 + j], a.activation), y, l);
                        lad_acc += l;
                    }
                    *slot = y;
                }
            }
        }
        // ---- a row's logabsdet: the two lane-halves of every unit, then the units of the row's tile in tile order
        {
            const float sum = lad_acc + __shfl_xor(lad_acc, 32, kWave);
            if (half == 0) s_lad[wave * 32 + r] = sum;
        }
        __syncthreads();
        if (tid < kRows) {
            const int rt = tid >> 5, rr = tid & 31;
            float sum = s_lad[rt * 32 + rr];
#pragma unroll
            for (int t = 1; t < kWaves / 2; ++t) sum += s_lad[(2 * t + rt) * 32 + rr];
            float* dst = a.lad + row0 + tid;
            *dst = a.accumulate ? *dst + sum : sum;
        }
        scatter_rows(a.out + row0 * D, D, s_row, s_final, tid);
    }
    if (my_status && a.status) atomicOr(a.status, my_status);
}

typedef void (*AffineWideKernelFn)(const AffineWideArgs);
AffineWideKernelFn affine_wide_resnet(bool inverse, bool additive);   // affine_resnet_wide.hip
AffineWideKernelFn affine_wide_mlp(bool inverse, bool additive);      // affine_resnet_wide_mlp.hip

}  // namespace k37
}  // namespace nfa
