// What the whole-layer kernels for conditioners of 129 .. 256 hidden units share: K32 (rqs_resnet_wide_kernel.hpp), K33
// (resnet_train_wide.hip), K34 (made_rqs_wide_kernel.hpp), K36 (affine_made_wide_kernel.hpp), K37
// (affine_resnet_wide_kernel.hpp).  Each of those keeps its Args, its pointers into the packed stream, its final Linear and
// its element step; the work split below, the pieces of the layer loop and the launchers' tail live here.
//
// Arithmetic: K8's (three bf16 pieces per fp32 operand, six products per k-step on v_mfma_f32_32x32x16_bf16, NFA_MFMA6):
// the full fp32 range, no row block is ever given up, no redo pass.
//
// Work split.  A wave of K8 keeps its 32 rows x 128 activations in registers as pieces; at 256 columns that is 192
// registers for one set of activations, and a residual block needs two sets beside its accumulators.  So the GEMMs are
// split by COLUMNS (K8c's idea, on K8's 32 x 32 tiles): one workgroup of eight waves per CU works on two 32-row tiles
// (64 rows), persistent over the 64-row blocks of the batch.  Wave w owns hidden columns 32 w .. 32 w + 31 of every
// hidden GEMM for both row tiles: two accumulator tiles.  Its slice of the stream stays in fp32 in those accumulators
// across the blocks (a residual block's skip connection is its second Linear accumulating on top of it).
//   * Weights: a wave reads only its own column tile's fragments, from global memory straight into registers -- no other
//     wave needs them, so there is nothing to share through LDS.  The last requests of a GEMM fetch the first fragments
//     of the wave's NEXT GEMM, so the exchange and its barriers hide that latency.
//   * Exchange buffer: after a GEMM the wave applies the ReLU where the next Linear wants it, splits its 32 columns x
//     64 rows into three bf16 pieces and stores them in LDS in B-fragment layout, [k-step of 16][row tile][piece][lane]
//     x 16 B: k-steps 2 w, 2 w + 1 of the next GEMM ARE wave w's block (ops._wide_column_order, over Hp columns).
//     16 k-steps x 2 x 3 x 1 KB = 96 KB at Hp = 256; with the row tile ([D <= 128][65] floats, 33 KB) a second half
//     as in K8c does not fit the CU's 160 KB.  Double-buffering only some pieces would still need the second barrier
//     for the others, so TWO barriers go around each exchange (all waves have read the old pieces | the new ones are
//     visible): ~1 us of barriers per residual block against its two GEMMs' 2 x 16 k-steps x 12 MFMAs per wave, two
//     waves per SIMD -- about 10 us.
//   * Narrow widths: tile count Hp / 32 and k-step count Hp / 16 are run-time values; a wave whose column tile lies
//     beyond Hp computes nothing in the hidden GEMMs, keeps every barrier and takes its share of the final layer.
//   * Row tile: the 64 rows sit in LDS as [column][65]; the element step replaces the inputs in their slots, and the
//     output rows are gathered from the slots through the layer's `final` table.
//
// Two GEMM policies, which differ in result bits and stay apart:
//   * `gemm_exchange` (K32, K33): one accumulator set, two k-steps in flight beside the two in use, the lane folded into
//     the fragment pointers;
//   * `gemm_exchange_split` (K34, K36, K37): K29's split accumulators, one k-step in flight (the second set of
//     accumulators takes the registers of the second pair of fragments), wave-uniform pointers, the lane added at the load.
// The block loops take the GEMM as a callable `gemm(acc, wl, wnext)`; K36's block-context k-steps are the residual loop's
// `after_w0` hook.  Not shared, because it could only be by asking which kernel calls: K37's per-unit logabsdet sum
// (shares [8 units][32 rows], not [8 waves][64 rows]) and every final Linear / element step.  The four lines that carve
// the dynamic LDS (exchange buffer | row tile [D][65] | logabsdet shares | a kernel's own) also stay in each kernel: handed
// out by a function, the same pointers cost K37's MLP instances two VGPRs (127 -> 129) and with them a wave of occupancy.
#pragma once

#include "bf16x3_gemm.hpp"

#include <hip/hip_ext.h>
#include <stdlib.h>

namespace nfa {
namespace wide {

constexpr int kWaves = 8, kThreads = kWaves * kWave;
constexpr int kRows = 64, kPad = 65;          // rows of a workgroup; row tile [column][65]
constexpr int kFragVec4 = 3 * kWave;          // one (column tile, k-step) of a weight: [piece][lane] x 16 B
constexpr int kStepVec4 = 2 * 3 * kWave;      // one k-step of the exchange buffer: [row tile][piece][lane] x 16 B

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

// `kstep` and `gemm_exchange` on split accumulators (NFA_MFMA6_SPLIT, fused_common.hpp, as K29 has them): the leading
// product accumulates alone, the five small ones in `small`, added once at the end of the GEMM -- the main accumulator is
// rounded once per k-step instead of six times.  SPLIT = false is the single accumulator: K34's final layer at three tiles
// per pair of features (12 .. 16 bins), where 96 logits stay in registers beside the GEMM and a second set does not fit.
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

// f0: the fragment of k-step 0 on entry, that of `wnext` (the wave's next GEMM) on exit: one k-step (twelve MFMAs, and the
// other wave of the SIMD's twelve) hides a fragment's latency.  wl / wnext are wave-uniform; the lane is added at the load.
template <bool SPLIT>
__device__ __forceinline__ void gemm_exchange_split(f32x16 (&acc)[2], const vec4f* wl, const vec4f* wnext, int nks, Frag& f0,
                                                    const uvec4* xl, int lane) {
    f32x16 small[2] = {{0}, {0}};
    for (int ks = 0; ks < nks; ++ks) {
        const Frag f1 = load_frag((ks + 1 < nks ? wl + (size_t)(ks + 1) * kFragVec4 : wnext) + lane);
        kstep_split<SPLIT>(acc, small, f0, xl + ks * kStepVec4);
        f0 = f1;
    }
    if constexpr (SPLIT) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc[rt] += small[rt];
    }
}

// acc[rt] += W_tile[32 x 16 ksteps] x cols^T, the columns gathered from an LDS tile [column][65] and split into pieces at
// the use (the initial layer, K36's context terms): k = ks * 16 + half * 8 + j reads column tab[k] (TABLE) or k itself;
// k >= n is zero.  `wl`: the lane's fragments of this GEMM.  ksteps <= 4.
template <bool TABLE>
__device__ __forceinline__ void gemm_gather(f32x16 (&acc)[2], const vec4f* wl, int ksteps, const float* tile, const int* tab,
                                            int n, int half, int r) {
    for (int ks = 0; ks < ksteps; ++ks) {
        const Frag f = load_frag(wl + (size_t)ks * kFragVec4);
        const bf16x8 ah = __builtin_bit_cast(bf16x8, f.h), am = __builtin_bit_cast(bf16x8, f.m), al = __builtin_bit_cast(bf16x8, f.l);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = ks * 16 + half * 8 + j;   // (< 64)
                const int col = TABLE ? tab[i] : (i < n ? i : 0);
                const float xv = tile[col * kPad + rt * 32 + r];
                v[j] = i < n ? xv : 0.0f;
            }
            bf16x2 hh[4], mm[4], ll[4];
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) split3(vec2f{v[j2 * 2], v[j2 * 2 + 1]}, hh[j2], mm[j2], ll[j2]);
            const bf16x8 bh = join4(hh[0], hh[1], hh[2], hh[3]), bm = join4(mm[0], mm[1], mm[2], mm[3]),
                         bl = join4(ll[0], ll[1], ll[2], ll[3]);
            NFA_MFMA6(acc[rt], ah, am, al, bh, bm, bl);
        }
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

// The layer's tables -> LDS, clamped into the row; a slot the layer uses (`used(tid)`, the caller's rule for its two halves)
// or a final position that lies outside it is the thread's NFA_STATUS_BAD_INDEX.
template <class Used>
__device__ __forceinline__ int load_tables(const int32_t* tables, int tid, int D, int* s_tab, int* s_final, Used&& used) {
    int status = 0;
    if (tid < kTabLayer) {
        const bool u = used(tid);
        int v = tables[tid], f = tables[kTabLayer + tid];
        if ((u && (v < 0 || v >= D)) || (tid < D && (f < 0 || f >= D))) status |= NFA_STATUS_BAD_INDEX;
        s_tab[tid] = v < 0 ? 0 : (v >= D ? D - 1 : v);
        s_final[tid] = f < 0 ? 0 : (f >= D ? D - 1 : f);
    }
    return status;
}

// the 64 rows at `x`: one coalesced read, four vec4f in flight per thread; slot j of the tile = input column j
__device__ __forceinline__ void load_row_tile(const float* x, int D, float* s_row, int tid) {
    const vec4f* xv = reinterpret_cast<const vec4f*>(x);
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

// Residual blocks: h += W_1 relu(W_0 relu(h) + b_0) + b_1 over the hidden Linears 0 .. nh - 1, two per block.  `hbias`: the
// lane's 16 of the first hidden Linear's bias, + Hp per Linear; `w_hidden`: the wave's tile of the first W_0, + block_vec4
// per block, W_1 at + w1_vec4 inside it; `w_behind`: the wave's GEMM behind the last block.  `after_w0(u, w0)` runs on
// W_0's accumulators in front of their ReLU.
template <class Gemm, class AfterW0>
__device__ __forceinline__ void residual_blocks(f32x16 (&h)[2], int nh, bool active, uvec4* X, int wave, int lane,
                                                const float* hbias, int Hp, const vec4f* w_hidden, size_t block_vec4,
                                                size_t w1_vec4, const vec4f* w_behind, Gemm&& gemm, AfterW0&& after_w0) {
    for (int j = 0; j < nh; j += 2) {
        const float* bias = hbias + (size_t)j * Hp;
        const vec4f* w0 = w_hidden + (size_t)(j >> 1) * block_vec4;
        const vec4f* w1 = w0 + w1_vec4;
        f32x16 u[2];
        if (j > 0) NFA_K32_BARRIER();   // (the first block: nobody has read the buffer in this row block)
        if (active) exchange_store<kActRelu>(h, X, wave, lane);
        NFA_K32_BARRIER();
        if (active) {
            load_bias_tile(u[0], bias);
            u[1] = u[0];
            gemm(u, w0, w1);
            after_w0(u, w0);
        }
        NFA_K32_BARRIER();
        if (active) exchange_store<kActRelu>(u, X, wave, lane);
        NFA_K32_BARRIER();
        if (active) {
            f32x16 b1;
            load_bias_tile(b1, bias + Hp);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                h[0][q] += b1[q];
                h[1][q] += b1[q];
            }
            gemm(h, w1, j + 2 < nh ? w0 + block_vec4 : w_behind);
        }
    }
}

// Feed-forward blocks / an MLP's hidden layers: pre = W relu(pre) + b (the ReLU moved in front of the Linear, the final
// layer's included: `handover`); there is no skip.  Parameters as `residual_blocks`, one Linear of hidden_vec4 per block.
template <class Gemm>
__device__ __forceinline__ void feedforward_blocks(f32x16 (&h)[2], int nh, bool active, uvec4* X, int wave, int lane,
                                                   const float* hbias, int Hp, const vec4f* w_hidden, size_t hidden_vec4,
                                                   const vec4f* w_behind, Gemm&& gemm) {
    for (int j = 0; j < nh; ++j) {
        const vec4f* wj = w_hidden + (size_t)j * hidden_vec4;
        if (j > 0) NFA_K32_BARRIER();
        if (active) exchange_store<kActRelu>(h, X, wave, lane);
        NFA_K32_BARRIER();
        if (active) {
            load_bias_tile(h[0], hbias + (size_t)j * Hp);
            h[1] = h[0];
            gemm(h, wj, j + 1 < nh ? wj + hidden_vec4 : w_behind);
        }
    }
}

// the final layer's B operand: the residual stream as it is, a feed-forward activation through its ReLU (`relu`)
__device__ __forceinline__ void handover(const f32x16 (&h)[2], bool relu, bool after_gemm, bool active, uvec4* X, int wave,
                                         int lane) {
    if (after_gemm) NFA_K32_BARRIER();
    if (active) {
        if (relu) exchange_store<kActRelu>(h, X, wave, lane);
        else exchange_store<kActNone>(h, X, wave, lane);
    }
    NFA_K32_BARRIER();
}

// a row's logabsdet: the two lane-halves of every wave, then the waves in their order -- an order the shape alone fixes
__device__ __forceinline__ void reduce_logabsdet(const float (&lad_acc)[2], float* s_lad, int wave, int half, int r, int tid,
                                                 float* lad, int accumulate) {
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
        float* dst = lad + tid;
        *dst = accumulate ? *dst + s : s;
    }
}

// output rows: position p of a row comes from slot final[p]; 16 bytes per lane per store.  Behind the closing barrier the
// row tile, the exchange buffer and the logabsdet shares are free for the next row block.
__device__ __forceinline__ void scatter_rows(float* out, int D, const float* s_row, const int* s_final, int tid) {
    vec4f* ov = reinterpret_cast<vec4f*>(out);
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
    __syncthreads();
}

// ---- host: the tail of the four launchers.  The entry point has answered its argument rules and family limits; this
// answers, in this order, the LDS limit, batch 0, missing buffers and a missing instance, fills the fields every Args has
// (init_ks and the kernel's own are the caller's), and launches batch / 64 workgroups, at most one per CU.
struct Call {
    const float* x;
    const void* w;
    const float* bias;
    const int32_t* tables;
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;
    int D, dt, hidden_features;
    int32_t flags;
    void* stream;
    size_t extra_lds;          // behind the exchange buffer and the row tile: logabsdet shares, K36's context tile
    bool others_given = true;  // a buffer of the kernel's own (K36's context) is there
};

template <class Args, class Note>
inline int launch(Args& a, void (*kern)(const Args), const Call& c, Note&& note) {
    a.tiles = (c.hidden_features + 31) / 32;
    a.nks = 2 * a.tiles;
    const size_t lds = (size_t)a.nks * kStepVec4 * 16 + (size_t)c.D * kPad * sizeof(float) + c.extra_lds;
    if (lds > (size_t)kCuLds - 2048) return NFA_ERR_UNSUPPORTED;
    if (c.batch == 0) return NFA_OK;
    if (!c.x || !c.w || !c.bias || !c.tables || !c.out || !c.lad || !c.others_given) return NFA_ERR_INVALID_ARGUMENT;
    if (!kern) return NFA_ERR_UNSUPPORTED;
    a.x = c.x;
    a.w = reinterpret_cast<const vec4f*>(c.w);
    a.bias = c.bias;
    a.tables = c.tables;
    a.out = c.out;
    a.lad = c.lad;
    a.status = c.status;
    a.batch = c.batch;
    a.D = c.D;
    a.dt = c.dt;
    a.accumulate = (c.flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0;
    int64_t blocks = c.batch >> 6;
    if (blocks > device_cu_count()) blocks = device_cu_count();
    note();   // note_layer_kernel with the instance's label
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)c.stream, a, kCuLds - 2048);
}

}  // namespace wide
}  // namespace nfa
