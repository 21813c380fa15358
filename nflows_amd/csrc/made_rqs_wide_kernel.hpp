// The kernel body of K34 (made_rqs_wide.hip and its made_rqs_wide_bins_*.hip): the density pass of ONE masked autoregressive
// rational-quadratic spline layer (autoregressive.py:404-495) whose MADE (made.py:233-311) has 129 .. 256 hidden units --
// zero-padded by the packer to Hp, a multiple of 32 -- in one launch: the MADE, its final Linear, the spline on the logits
// while they are accumulators, the per-row logabsdet.  The logits never reach memory.
//
// Arithmetic, work split, exchange buffer and the shared pieces of the layer loop: wide_layer_common.hpp.  K34 runs on the
// split-accumulator policy (`gemm_exchange_split<true>`) in every GEMM but the final layer's at 12 .. 16 bins.  The 0/1
// masks are multiplied into the weights by the packer (K22 / K29's rule): a masked-out weight is an exact zero in all three
// pieces, so a feature's result does not depend on the features behind it, bit for bit.
//
// What a MADE changes against K32's ResidualNet:
//   * Every feature is read by the conditioner AND transformed: all D <= 64 columns of the 64 rows sit in one LDS tile
//     [Dp][65] (Dp = D rounded up to 4: <= 16 640 B); the initial layer reads it in ceil(D / 16) k-steps, the spline takes
//     feature f's input from slot f and leaves z there; a slot has one reader and one writer behind the initial layer,
//     the lane-half that owns the feature.  The tile is stored once.
//   * Blocks come in two forms (a workgroup-uniform run-time branch, as in K29): residual and feed-forward, h = relu(W h + b)
//     with h_0 = relu(W_i x + b_i) (made.py:197-206).  Feed-forward MADEs may have random masks: masks are data at pack time.
//   * The final Linear has ceil(D / 2) pairs of features, T = ceil((3 K - 1) / 16) tiles each, dealt over the eight waves.
//     With an odd D the last pair's second lane-half has no feature: its rows are zero, it evaluates a value outside the
//     box (passes through, log-derivative exactly 0) and writes nothing.
//   * A row's logabsdet: pair after pair within a wave, the two lane-halves, then the waves in their order -- an order the
//     shape alone fixes, so results are the same bits for any batch, grid and call.
//
// LDS: exchange buffer Hp / 16 x 6 KB (96 KB at Hp = 256) + row tile (<= 16 640 B) + logabsdet shares 2 KB + tables 1 KB:
// 118 016 B at the largest shape.
#pragma once

#include "wide_layer_common.hpp"

namespace nfa {
namespace k34 {

using namespace wide;

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

template <int KB>
__global__ void __launch_bounds__(kThreads, 1) made_rqs_wide_kernel(const MadeWideArgs a) {
#pragma clang fp contract(off)
    constexpr int T = (3 * KB - 1 + 15) / 16;   // 32-row tiles per pair of features
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
        // ---- initial layer: h = W_i x + b_i over ALL features (masked); k = ks*16 + half*8 + j
        if (active) {
            load_bias_tile(h[0], a.bias + wave * 32 + half * 16);
            h[1] = h[0];
            gemm_gather<true>(h, w_init + lane, a.init_ks, s_row, s_tab + kTabId, dt, half, r);
        }
        // ---- blocks (made.py:129-137 without context / made.py:96-98), then the final layer's B operand
        const float* hbias = a.bias + (size_t)tiles * 32 + wave * 32 + half * 16;
        if (resnet)
            residual_blocks(h, nh, active, X, wave, lane, hbias, tiles * 32, w_hidden, 2 * hidden_vec4, hidden_vec4,
                            w_behind_hidden, gemm, [](f32x16 (&)[2], const vec4f*) {});
        else
            feedforward_blocks(h, nh, active, X, wave, lane, hbias, tiles * 32, w_hidden, hidden_vec4, w_behind_hidden, gemm);
        handover(h, !resnet, nh > 0, active, X, wave, lane);

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
        reduce_logabsdet(lad_acc, s_lad, wave, half, r, tid, a.lad + row0, a.accumulate);
        scatter_rows(a.out + row0 * D, D, s_row, s_final, tid);
    }
    if (my_status && a.status) atomicOr(a.status, my_status);
}

typedef void (*MadeWideKernelFn)(const MadeWideArgs);
MadeWideKernelFn made_wide_bins_low(int K);    // 2 .. 5 bins (one tile per pair of features) and 12 .. 16 (three),
                                               // made_rqs_wide_bins_a.hip
MadeWideKernelFn made_wide_bins_mid(int K);    // 6 .. 11 (two tiles), made_rqs_wide_bins_b.hip

}  // namespace k34
}  // namespace nfa
