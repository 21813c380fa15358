// The kernel body of K32 (rqs_resnet_wide.hip and its rqs_resnet_wide_bins_*.hip): ONE spline coupling layer whose
// ResidualNet conditioner (nn/nets/resnet.py:55-100) is wider than the 128 hidden units of K8 -- 129 .. 256, zero-padded by
// the packer to Hp, a multiple of 32 -- in one launch, both directions: gather of the identity columns, conditioner, final
// Linear, spline on the logits while they are accumulators (coupling.py:73-130, :549-582), per-row logabsdet, scatter.
//
// Arithmetic, work split, exchange buffer and the shared pieces of the layer loop: wide_layer_common.hpp.  K32 runs every
// GEMM on the single-accumulator policy (`gemm_exchange`: two k-steps in flight beside the two in use).
//
// What is K32's own: the final Linear and the spline (K29's scheme, made_rqs_kernel.hpp).  Per pair of transformed
// features T = ceil((3 K - 1) / 16) output tiles whose accumulators are the lane-half's feature's logits, evaluated by the
// register instance of rqs_math.hpp; the pairs are dealt over the eight waves; the B operand -- all Hp k of both row
// tiles, 384 registers -- is read from the exchange buffer k-step by k-step.  Results replace the inputs in their slots of
// the row tile; the waves' logabsdet shares meet in LDS and are summed per row in wave order.
#pragma once

#include "wide_layer_common.hpp"

namespace nfa {
namespace k32 {

using namespace wide;

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

template <bool INVERSE, int KB>
__global__ void __launch_bounds__(kThreads, 1) rqs_resnet_wide_kernel(const WideArgs a) {
#pragma clang fp contract(off)
    constexpr int T = (3 * KB - 1 + 15) / 16;   // 32-row tiles per pair of features
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    __shared__ int s_tab[kTabLayer];
    __shared__ int s_final[128];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, dt = a.dt, nks = a.nks, tiles = a.tiles, nb = a.num_blocks;
    int my_status = load_tables(a.tables, tid, D, s_tab, s_final, [&](int t) { return t < kTabTr ? t < a.di : t - kTabTr < dt; });
    // dynamic LDS, as every wide kernel carves it: exchange buffer (nks x 6 KB), row tile [D][65], logabsdet shares
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
    const auto gemm = [&](f32x16 (&acc)[2], const vec4f* wl, const vec4f* wnext) { gemm_exchange(acc, wl, wnext, nks, f0, f1, xl); };

    const int64_t num_blocks64 = a.batch >> 6;
    for (int64_t blk = blockIdx.x; blk < num_blocks64; blk += gridDim.x) {
        const int64_t row0 = blk << 6;
        int lane_here = lane;
        asm volatile("" : "+v"(lane_here));
        const int half = lane_here >> 5, r = lane_here & 31;
        load_row_tile(a.x + row0 * D, D, s_row, tid);
        __syncthreads();

        f32x16 h[2];   // the wave's slice of the residual stream: columns 32 w .. 32 w + 31 of both row tiles
        // ---- initial layer: h = W_i x + b_i; every wave gathers the identity features itself (k = ks*16 + half*8 + j)
        if (active) {
            load_bias_tile(h[0], a.bias + wave * 32 + half * 16);
            h[1] = h[0];
            gemm_gather<true>(h, w_init, a.init_ks, s_row, s_tab + kTabId, a.di, half, r);
        }
        // ---- residual blocks (resnet.py:36-52, no context), then the stream as it is (resnet.py:99) to the final layer
        residual_blocks(h, 2 * nb, active, X, wave, lane, a.bias + (size_t)tiles * 32 + wave * 32 + half * 16, tiles * 32,
                        w_hidden, 2 * hidden_vec4, hidden_vec4, w_behind_hidden, gemm, [](f32x16 (&)[2], const vec4f*) {});
        handover(h, false, nb > 0, active, X, wave, lane);

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
                gemm(acc, wl, wnext);
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
        reduce_logabsdet(lad_acc, s_lad, wave, half, r, tid, a.lad + row0, a.accumulate);
        scatter_rows(a.out + row0 * D, D, s_row, s_final, tid);
    }
    if (my_status && a.status) atomicOr(a.status, my_status);
}

typedef void (*WideKernelFn)(const WideArgs);
WideKernelFn wide_bins_low(int K, bool inverse);    // 2 .. 5 bins (one tile per pair of features) and 12 .. 16 (three),
                                                    // rqs_resnet_wide_bins_a.hip
WideKernelFn wide_bins_mid(int K, bool inverse);    // 6 .. 11 (two tiles), rqs_resnet_wide_bins_b.hip

}  // namespace k32
}  // namespace nfa
