// The kernel of rqs_resnet_f16x3.hip (K8x) as a header: the template is instantiated in several translation units
// (rqs_resnet_f16x3.hip: 8 bins and the diagnostic instances; rqs_resnet_f16x3_bins_{a,b}.hip: the other bin counts) so that
// the instances compile side by side.  Design notes: rqs_resnet_f16x3.hip, f16x3_gemm.hpp.
#pragma once

#include "f16x3_gemm.hpp"
#include "rqs_resnet_f16_kernel.hpp"   // FusedSteps' unit slicing (k8h::spline_unit_range)

#include <hip/hip_ext.h>
#include <stdlib.h>
#include <type_traits>

namespace nfa {
namespace k8x {

struct Args {
    const float* x;          // [B, D]
    const vec4f* w;          // [num_layers * num_stages][768] x 16 bytes
    const float* bias;       // accumulator-order biases of all GEMMs (x the scale of their accumulators), layer after layer
    const float* scales;     // [num_layers][1 + 2 num_blocks + 1][2]
    const int32_t* tables;   // [num_layers][128] slots of the identity / transformed features, then [128] final
    float* out;
    float* lad;
    int32_t* redo;           // [batch / 128]
    int32_t* status;
    int64_t batch;
    int D, dt, di, num_blocks, num_layers, num_stages, bias_per_layer, accumulate;
    RqsDev sp;
    int normal, skip_out;
    float log_z, act_scale;
    int Ds;
    float* dbg_logits;       // DBG: [batch][dt * 24], packed row order (tile, lane-half, register)
};

// LDS addresses as 32-bit LDS pointers: a generic pointer into the row tile is a 64-bit register pair and its arithmetic
// 64-bit VALU (the group loop spent 23 v_lshl_add_u64 / v_mad_*64 per iteration on five of them, and they were among the
// values the layer loop kept in scratch)
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) int lds_i32;

using nfa::load_bias_tile;   // (global biases: the instances without the bias area; the overload below reads LDS)

__device__ __forceinline__ void load_bias_tile(f32x16& acc, const lds_f32* bias_tile_half) {
    typedef __attribute__((address_space(3))) const vec4f lds_vec4f;
    lds_vec4f* bp = reinterpret_cast<lds_vec4f*>(bias_tile_half);
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const vec4f b = bp[q4];
        acc[q4 * 4 + 0] = b.x;
        acc[q4 * 4 + 1] = b.y;
        acc[q4 * 4 + 2] = b.z;
        acc[q4 * 4 + 3] = b.w;
    }
}

// The bias area (BIAS_LDS instances): a layer's biases and the next layer's raw table in LDS, fetched ahead as LDS-DMA pieces
// by the mechanism of the weight stream (f16x3_gemm.hpp: request_stage) -- a buffer resource over the source (scalar), the
// piece's offset as soffset, the lane's as voffset.  A piece is one wave instruction: 64 lanes x BYTES contiguous bytes, 1 KB
// (BYTES 16) or 256 B (BYTES 4).  Pieces are issued IN FRONT of a stage's request_stage: they are then older than the three
// requests the stage's counted wait (stream_advance: vmcnt(3)) leaves in flight, so that wait covers them, whatever their
// number and whichever waves issue them, and the stage's barrier publishes them -- the ring's invariants stay as they are.
// The resource covers the PIECE: its base is the piece's first byte and its size what is left of the source from there (the
// range check compares the lane's voffset with the size and does not see an soffset), so lanes past the source's end read
// nothing; what they write, if anything, must be padding.
//   [hidden: 128 + 256 num_blocks floats][raw table of the next layer: 128 ints][final: dt x kFinalRows floats, padded to 1 KB]
template <int BYTES>
__device__ __forceinline__ void bias_area_piece(const void* src, int src_bytes, int piece_off, lds_f32* dst) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(static_cast<const char*>(src) + piece_off), (short)0, src_bytes - piece_off, 0x00020000);
    // (the lane index made afresh: carried from the kernel's entry it would hold a register through the whole layer)
    unsigned all = ~0u;
    asm volatile("" : "+s"(all));
    const unsigned lane = __builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
    static_assert(BYTES == 16 || BYTES == 4, "dwordx4 or dword pieces");
    // (the builtin takes its size as a literal)
    if constexpr (BYTES == 16)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)dst, 16, lane * 16, 0, 0, 0);
    else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)dst, 4, lane * 4, 0, 0, 0);
}
__host__ __device__ constexpr int bias_area_hidden_floats(int num_blocks) { return 128 + 256 * num_blocks; }
__host__ __device__ constexpr int bias_area_final_floats(int final_floats) { return (final_floats + 255) & ~255; }
__host__ __device__ constexpr int bias_area_floats(int num_blocks, int final_floats) {
    return bias_area_hidden_floats(num_blocks) + kTabLayer + bias_area_final_floats(final_floats);
}

// Two or four wave-uniform floats through the scalar cache.  The kernel stores to global memory, so the compiler cannot prove the
// per-layer scales unchanged and reads them with a VECTOR load -- whose wait, vmcnt(0), also drains the weight stream's
// LDS-DMA requests in flight.  The wait of a scalar load is lgkmcnt(0).
template <int N>
__device__ __forceinline__ void uniform_load(const float* p, float (&v)[N]) {
    static_assert(N == 2 || N == 4, "one or two pairs");
    uint64_t v01, v23 = 0;
    if constexpr (N == 2)
        asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v01) : "s"(p) : "memory");
    else
        asm volatile("s_load_dwordx2 %0, %2, 0x0\n\ts_load_dwordx2 %1, %2, 0x8\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(v01), "=&s"(v23) : "s"(p) : "memory");
    v[0] = __builtin_bit_cast(float, (unsigned)v01);
    v[1] = __builtin_bit_cast(float, (unsigned)(v01 >> 32));
    if constexpr (N == 4) {
        v[2] = __builtin_bit_cast(float, (unsigned)v23);
        v[3] = __builtin_bit_cast(float, (unsigned)(v23 >> 32));
    }
}

// What runs behind the MFMAs of a final-layer tile: a tile's 24 f16 MFMAs count one time unit each, its four bf8 MFMAs two
// (64 against 32 cycles): 32 units per tile, a weave's slices spread evenly over them.
struct NoWeave {
    template <int U0, int U1>
    __device__ __forceinline__ void span() {}
};
// 8 bins: the three evaluation units of K8h's two-features-per-three-tiles scheme (rqs_resnet_f16_kernel.hpp)
template <int UNIT, class Steps>
struct UnitWeave {
    Steps &fa, &fb;
    const RqsDev& sp;
    template <int U0, int U1>
    __device__ __forceinline__ void span() {
        constexpr int N = k8h::spline_unit_slices<UNIT, Steps>();
        k8h::spline_unit_range<UNIT, (U0 * N) / 32, (U1 * N) / 32>(fa, fb, sp);
    }
};
// any other bin count: the slice sequence MASK names (numerators of the widths / heights, the rest), one feature per lane-half
template <int MASK, class Steps>
struct SeqWeave {
    Steps& f;
    const RqsDev& sp;
    template <int U0, int U1>
    __device__ __forceinline__ void span() {
        constexpr int N = k8h::spline_seq_count<MASK, Steps>();
        k8h::spline_seq_range<MASK, (U0 * N) / 32, (U1 * N) / 32>(f, sp);
    }
};

#define NFA_K8X_PUMP_F16(U, A_, B_)                                         \
    acc = NFA_K8X_F16(A_, B_, acc);                                         \
    __builtin_amdgcn_sched_barrier(0);                                      \
    w.template span<(U), (U) + 1>();                                        \
    __builtin_amdgcn_sched_barrier(0)
#define NFA_K8X_PUMP_BF8(U, A_, B_)                                         \
    acc = NFA_K8X_BF8(A_, B_, acc);                                         \
    __builtin_amdgcn_sched_barrier(0);                                      \
    w.template span<(U), (U) + 2>();                                        \
    __builtin_amdgcn_sched_barrier(0)

// one stage of the final layer = four k-steps of the tile: two pairs of k-steps, each three f16 products per k-step and one
// bf8 instruction, a slice of the evaluation behind every MFMA.  Stage layout: fragments [H0, L0, H1, L1][H2, L2, H3, L3]
// [X01 lo, X01 hi, X23 lo, X23 hi].  The first pair's f16 fragments arrive in `lead` (read behind the previous stage's
// barrier), the second pair's are requested behind the MFMAs that free the first pair's registers, and the stage's own
// barrier stands in front of its last bf8 instruction: the next stage's lead fragments land while that one runs.
template <int HS, int WAVES, class W>
__device__ __forceinline__ void stage_pumped(f32x16& acc, const Pieces (&p)[8], const i32x8 (&bx)[4], WeightStream& sm, int lane,
                                             Lead& lead, W& w) {
    request_stage<WAVES, HS>(sm);
    const vec4f* cur = sm.ring + sm.slot * kStageVec4 + lane;
    vec4f xa = cur[8 * 64], xb = cur[9 * 64];
    vec4f fh0 = lead.h0, fl0 = lead.l0, fh1 = lead.h1, fl1 = lead.l1;
    {
        const Pieces& b0 = p[HS * 4 + 0];
        const Pieces& b1 = p[HS * 4 + 1];
        const f16x8 bh0 = __builtin_bit_cast(f16x8, b0.h), bl0 = __builtin_bit_cast(f16x8, b0.l);
        const f16x8 bh1 = __builtin_bit_cast(f16x8, b1.h), bl1 = __builtin_bit_cast(f16x8, b1.l);
        const f16x8 ah0 = __builtin_bit_cast(f16x8, fh0), al0 = __builtin_bit_cast(f16x8, fl0);
        const f16x8 ah1 = __builtin_bit_cast(f16x8, fh1), al1 = __builtin_bit_cast(f16x8, fl1);
        const i32x8 ax = join_x(xa, xb);
        NFA_K8X_PUMP_F16(HS * 16 + 0, ah0, bl0);
        NFA_K8X_PUMP_F16(HS * 16 + 1, al0, bh0);
        NFA_K8X_PUMP_F16(HS * 16 + 2, ah0, bh0);
        fh0 = cur[4 * 64];
        fl0 = cur[5 * 64];
        NFA_K8X_PUMP_F16(HS * 16 + 3, ah1, bl1);
        NFA_K8X_PUMP_F16(HS * 16 + 4, al1, bh1);
        NFA_K8X_PUMP_F16(HS * 16 + 5, ah1, bh1);
        fh1 = cur[6 * 64];
        fl1 = cur[7 * 64];
        NFA_K8X_PUMP_BF8(HS * 16 + 6, ax, bx[HS * 2 + 0]);
        xa = cur[10 * 64];
        xb = cur[11 * 64];
    }
    {
        const Pieces& b0 = p[HS * 4 + 2];
        const Pieces& b1 = p[HS * 4 + 3];
        const f16x8 bh0 = __builtin_bit_cast(f16x8, b0.h), bl0 = __builtin_bit_cast(f16x8, b0.l);
        const f16x8 bh1 = __builtin_bit_cast(f16x8, b1.h), bl1 = __builtin_bit_cast(f16x8, b1.l);
        const f16x8 ah0 = __builtin_bit_cast(f16x8, fh0), al0 = __builtin_bit_cast(f16x8, fl0);
        const f16x8 ah1 = __builtin_bit_cast(f16x8, fh1), al1 = __builtin_bit_cast(f16x8, fl1);
        const i32x8 ax = join_x(xa, xb);
        NFA_K8X_PUMP_F16(HS * 16 + 8, ah0, bl0);
        NFA_K8X_PUMP_F16(HS * 16 + 9, al0, bh0);
        NFA_K8X_PUMP_F16(HS * 16 + 10, ah0, bh0);
        NFA_K8X_PUMP_F16(HS * 16 + 11, ah1, bl1);
        NFA_K8X_PUMP_F16(HS * 16 + 12, al1, bh1);
        NFA_K8X_PUMP_F16(HS * 16 + 13, ah1, bh1);
        stream_advance<WAVES, HS>(sm);   // every read of this stage has landed in registers; the next stage is complete
        lead = read_lead(sm.ring + sm.slot * kStageVec4 + lane);
        __builtin_amdgcn_sched_barrier(0);
        NFA_K8X_PUMP_BF8(HS * 16 + 14, ax, bx[HS * 2 + 1]);
    }
}
#undef NFA_K8X_PUMP_F16
#undef NFA_K8X_PUMP_BF8

// (WAVES: the ring's form, f16x3_gemm.hpp -- a tile's two stages are the halves of a wide pair)
template <int WAVES = 4, class W>
__device__ __forceinline__ void gemm_tile_pumped(f32x16& acc, const Pieces (&p)[8], const i32x8 (&bx)[4], WeightStream& sm, int lane,
                                                 Lead& lead, W&& w) {
    stage_pumped<0, WAVES>(acc, p, bx, sm, lane, lead, w);
    stage_pumped<1, WAVES>(acc, p, bx, sm, lane, lead, w);
}

// tiles TI .. T - 1 of a group of the general final layer (K8h's any_group_tiles on this kernel's GEMM): biases, the tile's
// MFMAs with their share of the evaluation, the tile's sixteen logits into the evaluation's arrays
template <int TI, int T, int KB, class Steps, class BiasPtr>
__device__ __forceinline__ void any_group_tiles(f32x16& acc, Steps& f, BiasPtr gb, const Pieces (&p)[8], const i32x8 (&bx)[4],
                                                WeightStream& sm, int lane, Lead& lead, const RqsDev& sp) {
    if constexpr (TI < T) {
        constexpr int kMask = k8h::any_tile_mask(KB, TI);
        load_bias_tile(acc, gb + TI * 32);
        if constexpr (kMask != 0) gemm_tile_pumped(acc, p, bx, sm, lane, lead, SeqWeave<kMask, Steps>{f, sp});
        else gemm_tile_pumped(acc, p, bx, sm, lane, lead, NoWeave{});
        k8h::take_chunk<TI, KB>(f, acc);
        any_group_tiles<TI + 1, T, KB, Steps, BiasPtr>(acc, f, gb, p, bx, sm, lane, lead, sp);
    }
}

__device__ __forceinline__ bool not_finite(float v) { return !(__builtin_fabsf(v) < INFINITY); }

// BIAS_LDS: the layer's biases and tables come through the bias area (above); without it every hidden bias tile is read
// from global memory in front of its GEMM and the final layer's are copied through registers, each with a vmcnt(0) that
// drains the weight ring -- kept for the geometries whose launch the larger area would take from two workgroups per CU
// to one (rqs_resnet_f16x3.hip: launch_f16x3).
//
// WAVES: 4 -- the narrow form: a workgroup of four waves owns one 128-row block per pass and a ring of its own, two workgroups
// per CU, each streaming the layer's weights into LDS for itself.  8 -- the wide form: ONE workgroup of eight waves per CU
// on ONE ring of three 24 KB slots (f16x3_gemm.hpp: a slot holds a pair of stages, one barrier per pair), so a CU moves
// every stage from L2 into LDS once instead of twice.  The workgroup owns two consecutive row blocks per pass: waves 0 .. 3
// run block 2 q, waves 4 .. 7 block 2 q + 1, each wave the narrow form's program on its 32 rows -- same fragments, same
// order, same bits.  The redo flag, the vote on non-finite results and the status are kept per half (per 128 rows).  With
// an odd number of row blocks the last workgroup's upper half has none: it computes the lower half's block again (every
// request and every barrier is the workgroup's) and stores nothing.
// The skip connection on eight values of a residual tile, IN PLACE: h = fma(h, skip, b1).  Written as asm for the register
// it names, not for the instruction: left to the compiler the result took the freshly loaded bias tile's registers (a
// two-address v_fmac_f32 onto its addend), the second Linear accumulated there, and the last k-step pair of every block
// copied the four tiles back to the registers the block loop carries h in -- 32 v_mov_b64 behind four waits for the
// matrix pipe's write-back.  Volatile keeps the blocks in front of the second Linear's first piece split, far from the
// first MFMA that reads the tile (the compiler does not see a VALU write inside an asm statement as one).
template <int B0>
__device__ __forceinline__ void skip_half(f32x16& h, const f32x16& b1, float skip) {
#if defined(NFA_K8X_NO_ASM)
#pragma unroll
    for (int q = B0; q < B0 + 8; ++q) h[q] = __builtin_fmaf(h[q], skip, b1[q]);
#else
    float e0 = h[B0], e1 = h[B0 + 1], e2 = h[B0 + 2], e3 = h[B0 + 3], e4 = h[B0 + 4], e5 = h[B0 + 5], e6 = h[B0 + 6], e7 = h[B0 + 7];
    NFA_K8X_ASM(
        "v_fma_f32 %0, %0, %8, %9\n\t"
        "v_fma_f32 %1, %1, %8, %10\n\t"
        "v_fma_f32 %2, %2, %8, %11\n\t"
        "v_fma_f32 %3, %3, %8, %12\n\t"
        "v_fma_f32 %4, %4, %8, %13\n\t"
        "v_fma_f32 %5, %5, %8, %14\n\t"
        "v_fma_f32 %6, %6, %8, %15\n\t"
        "v_fma_f32 %7, %7, %8, %16"
        : "+v"(e0), "+v"(e1), "+v"(e2), "+v"(e3), "+v"(e4), "+v"(e5), "+v"(e6), "+v"(e7)
        : "v"(skip), "v"(b1[B0]), "v"(b1[B0 + 1]), "v"(b1[B0 + 2]), "v"(b1[B0 + 3]), "v"(b1[B0 + 4]), "v"(b1[B0 + 5]),
          "v"(b1[B0 + 6]), "v"(b1[B0 + 7]));
    h[B0] = e0;
    h[B0 + 1] = e1;
    h[B0 + 2] = e2;
    h[B0 + 3] = e3;
    h[B0 + 4] = e4;
    h[B0 + 5] = e5;
    h[B0 + 6] = e6;
    h[B0 + 7] = e7;
#endif
}

template <bool INVERSE, int INIT_KS, bool DBG, int KB, bool BIAS_LDS, int WAVES = 4>
__device__ __forceinline__ void rqs_resnet_f16x3_body(const Args& a) {
    static_assert(!DBG || KB == 8, "the diagnostic instances: 8 bins");
    constexpr bool WIDE = WAVES == 8;
    static_assert(WAVES == 4 || (WIDE && KB == 8 && BIAS_LDS && !DBG), "the wide form: 8 bins, bias area, no diagnostics");
    constexpr int kRingFloats = kRing * kStageVec4 * 4 * (WIDE ? 2 : 1);
    // rows of the final layer per transformed feature: 8 bins: 23 logits padded to 24, two features share three 32-row tiles;
    // otherwise 3 K - 1 padded to whole 16-row lane-half shares (one feature per lane-half and group of T tiles)
    constexpr int kFinalRows = KB == 8 ? 24 : 16 * ((3 * KB - 1 + 15) / 16);
    constexpr int NW = WAVES;
    // dynamic LDS: the weight ring, per wave a [D][33] row tile, the bias area (without it: the final layer's biases)
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    __shared__ int s_tab[2][kTabLayer];   // tables of the current and the next layer
    __shared__ int s_final[128];
    __shared__ int s_bad[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, dt = a.dt;
    int my_status = 0;
    auto checked = [&](int v, bool used) {
        my_status |= (used && (v < 0 || v >= D)) ? NFA_STATUS_BAD_INDEX : 0;
        return v < 0 ? 0 : (v >= D ? D - 1 : v);
    };
    // (every thread takes part -- entry tid mod 128, the two halves of the workgroup write the same values: a divergent
    //  region here or at the head of the layer loop is where hipcc put this kernel's spill stores in FRONT of the region's
    //  exec restore -- the d_i > 32 instances lost the running log-determinant and status of waves 2, 3 that way, round 6;
    //  tests/test_host_logic.py scans every translation unit's assembly for the pattern)
    const int te = tid & (kTabLayer - 1);
    s_tab[0][te] = checked(a.tables[te], te < kTabTr ? te < a.di : te - kTabTr < dt);
    s_final[te] = checked(a.tables[a.num_layers * kTabLayer + te], te < D);

    WeightStream sm;
    sm.w = a.w;
    sm.ring = reinterpret_cast<vec4f*>(lds_dyn);
    sm.slot = 1;  // so that the first two requests go to slots 0 and 1
    sm.fetch = 0;
    sm.num_stages = a.num_stages * a.num_layers;
    sm.tid = tid;
    lds_f32* s_area = (lds_f32*)lds_dyn + kRingFloats + NW * D * kRowPad;
    lds_f32* s_traw = s_area + bias_area_hidden_floats(a.num_blocks);
    // hidden biases of a layer: the initial layer's 512 B as two 256 B pieces, a block's 1 KB as one piece
    auto request_hidden = [&](int layer) {
        const float* src = a.bias + (size_t)layer * a.bias_per_layer;
        const int bytes = bias_area_hidden_floats(a.num_blocks) * 4;
        if (wave >= NW - 2) bias_area_piece<4>(src, bytes, (wave - (NW - 2)) * 256, s_area + (wave - (NW - 2)) * 64);
        for (int j = wave; j < a.num_blocks; j += NW) bias_area_piece<16>(src, bytes, 512 + j * 1024, s_area + 128 + j * 256);
    };
    if constexpr (BIAS_LDS) request_hidden(0);
    if constexpr (WIDE) {
        sm.slot = 2;
        request_stage<WAVES, 0>(sm);  // stages 0, 1 -> slot 0 (halves 0, 1)
        sm.slot = 4;
        request_stage<WAVES, 0>(sm);  // stages 2, 3 -> slot 1 (halves 2, 3)
    } else {
        request_stage(sm);  // stage 0 -> slot 0
        sm.slot = 2;
        request_stage(sm);  // stage 1 -> slot 1
    }
    sm.slot = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

#ifdef NFA_K8X_STAGGER   // (measurement builds: the upper half of the grid -- the partners of the lower half's workgroups on
                         //  their CUs -- starts NFA_K8X_STAGGER x 8 128 cycles late; measured at 8, half a layer, and not
                         //  kept: DESIGN.md section 4, K8x item 9, profiles/r8/k8x_bias_lds_timing.txt)
    if (blockIdx.x >= (gridDim.x >> 1))
        for (int i = 0; i < NFA_K8X_STAGGER; ++i) __builtin_amdgcn_s_sleep(127);
#endif
    lds_f32* s_row = (lds_f32*)lds_dyn + kRingFloats + wave * D * kRowPad;
    lds_f32* s_fbias = BIAS_LDS ? s_traw + kTabLayer : s_area;
    // final-layer biases of a layer: 1 KB pieces, the last one's lanes past the end land in the area's padding
    auto request_final = [&](int layer) {
        const float* src = a.bias + (size_t)layer * a.bias_per_layer + bias_area_hidden_floats(a.num_blocks);
        const int bytes = dt * kFinalRows * 4;
        for (int j = wave; j * 1024 < bytes; j += NW) bias_area_piece<16>(src, bytes, j * 1024, s_fbias + j * 256);
    };
    // raw table of a layer: two 256 B pieces
    auto request_table = [&](int layer) {
        if (wave < 2) bias_area_piece<4>(a.tables + layer * kTabLayer, kTabLayer * 4, wave * 256, s_traw + wave * 64);
    };
    const int groups = dt >> 2;
    const int64_t num_quads = a.batch >> 7;
    const int gemms = 2 + 2 * a.num_blocks;   // per layer
    const float S = a.act_scale;
    int tb = 0;  // which half of s_tab holds the current layer's table

    const int64_t num_passes = WIDE ? (num_quads + 1) >> 1 : num_quads;
    for (int64_t pass = blockIdx.x; pass < num_passes; pass += gridDim.x) {
        // (wide: the upper half of the last workgroup of an odd number of row blocks runs the lower half's block and stores
        //  nothing -- arithmetic, no branch: see the kernel's head)
        const int64_t quad_mine = WIDE ? 2 * pass + (wave >> 2) : pass;
        // (the sign of the wrapping difference, not a compare and a select: the instance keeps the narrow form's v_cndmask count)
        const int live_bit = WIDE ? (int)(((uint64_t)quad_mine - (uint64_t)num_quads) >> 63) : 1;
        const bool live = live_bit != 0;
        const int64_t quad = quad_mine - 1 + live_bit;
        const int64_t row0 = (quad << 7) + ((WIDE ? wave & 3 : wave) << 5);
        // (lane-derived values are made opaque per iteration: hoisted out of this loop they would stay live through
        //  the whole kernel and push the register allocation into scratch)
        int lane_here = lane, di = a.di;
        asm volatile("" : "+v"(lane_here), "+s"(di));
        const int half = lane_here >> 5, r = lane_here & 31;
        // ---- the wave's 32 rows: one coalesced read; slot j of the tile = input column j
        {
            const vec4f* xv = reinterpret_cast<const vec4f*>(a.x + row0 * D);
            const int nvec = D * 8;  // 32 * D / 4
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
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        float lad_acc = 0.0f;
        int quad_status = 0;
        for (int layer = 0; layer < a.num_layers; ++layer) {
            // the two workgroups resident on a CU take turns at the higher issue priority (see rqs_resnet_kernel.hpp)
            // (wide: the two halves of the workgroup.  NFA_K8X_WIDE_NOPRIO, measurement builds: the wide form without it)
#ifdef NFA_K8X_WIDE_NOPRIO
            if constexpr (!WIDE)
#endif
            {
                if ((layer + ((WIDE ? wave >= 4 : blockIdx.x >= (gridDim.x >> 1)) ? 1 : 0)) & 1) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
            }
            const int* tab = s_tab[tb];
            const int nl = layer + 1 < a.num_layers ? layer + 1 : 0;   // (after the last layer: the next row block's first)
            // the next layer's table goes to the other half now; it is read only after this layer's many stage barriers
            if constexpr (!BIAS_LDS) {
                // (te made afresh from the lane count: carried from the kernel's entry it held a register through the
                //  whole layer, one of the values the layer loop kept in scratch)
                unsigned all = ~0u;
                asm volatile("" : "+s"(all));
                const int te_l = (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u)) + ((wave & 1) << 6);
                s_tab[tb ^ 1][te_l] = checked(a.tables[nl * kTabLayer + te_l], te_l < kTabTr ? te_l < a.di : te_l - kTabTr < dt);
            }
            // this layer's final biases and the next layer's raw table, in front of the initial GEMM's first request: landed
            // and published by that stage's barrier.  (Their last readers: the previous layer's last final tile, two stage
            // barriers back; this layer's clamp below, a whole final layer back.)
            if constexpr (BIAS_LDS) {
                request_final(layer);
                request_table(nl);
                __builtin_amdgcn_sched_barrier(0);
            }
            std::conditional_t<BIAS_LDS, const lds_f32*, const float*> bias;   // + 32 per tile
            if constexpr (BIAS_LDS) bias = s_area + half * 16;
            else bias = a.bias + (size_t)layer * a.bias_per_layer + half * 16;
            const float* sc = a.scales + (size_t)layer * gemms * 2;   // {1 / T, T} per GEMM (uniform)
            Pieces p[8];   // f16 pieces at scale S: the identity features, then the final layer's input

            // ---- identity features: k = ks*16 + half*8 + j
#pragma unroll
            for (int ks = 0; ks < INIT_KS; ++ks) {
#pragma unroll
                for (int j2 = 0; j2 < 4; ++j2) {
                    const int i0 = ks * 16 + half * 8 + j2 * 2;
                    float v0 = s_row[tab[kTabId + i0] * kRowPad + r], v1 = s_row[tab[kTabId + i0 + 1] * kRowPad + r];
                    v0 = i0 < di ? v0 : 0.0f;
                    v1 = i0 + 1 < di ? v1 : 0.0f;
                    unsigned hi, lo;   // (the pair's last pieces: two bytes, one half-word of r[j2 / 2])
                    if (j2 & 1) split3_scaled<false, true>(v0, v1, S, hi, lo, p[ks].r[j2 >> 1]);
                    else split3_scaled<false, false>(v0, v1, S, hi, lo, p[ks].r[j2 >> 1]);
                    p[ks].h[j2] = hi;
                    p[ks].l[j2] = lo;
                }
            }

            // ---- initial layer: h = W_i x + b_i   (accumulators: S T_0 h).  The residual stream stays in these 64 fp32
            //      accumulators, at the scale of the GEMM that made it: h * hs = S h (hs = 1 / T, a power of two)
            f32x16 h[4];
            float hs;
            {
#pragma unroll
                for (int t = 0; t < 4; ++t) load_bias_tile(h[t], bias + t * 32);
                gemm_kmajor<INIT_KS, WAVES>(h, p, sm, lane);
                float s0[2];
                uniform_load(sc, s0);
                hs = s0[0];
            }
            bias += 128;
            sc += 2;
            if constexpr (BIAS_LDS) {
                // the raw table has landed (a stage barrier of this layer is behind every wave): clamped into the other half
                // of s_tab, which the final layer's barriers publish.  (Every thread takes part, entry tid mod 128: see
                // the kernel's head.)
                unsigned all = ~0u;
                asm volatile("" : "+s"(all));
                const int te_l = (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u)) + ((wave & 1) << 6);
                s_tab[tb ^ 1][te_l] = checked(((const lds_i32*)s_traw)[te_l], te_l < kTabTr ? te_l < a.di : te_l - kTabTr < dt);
            } else {
                // (every wave has passed a stage barrier of this layer: nobody reads the previous layer's biases any
                //  more; the blocks' barriers come before the first use)
                const float* fbias = a.bias + (size_t)layer * a.bias_per_layer + 128 + 256 * a.num_blocks;
                for (int i = tid; i < dt * kFinalRows; i += kBlock) s_fbias[i] = fbias[i];
                if (a.num_blocks == 0) __syncthreads();   // without blocks the final layer follows at once
            }

            // ---- residual blocks: h += W_1 relu(W_0 relu(h) + b_0) + b_1, both Linears k-major, each splitting the ReLU of
            //      its input accumulators into pieces one pair of k-steps at a time (gemm_kmajor_relu).  Registers: h (64),
            //      u (64) and one pair's pieces (24) -- the pieces of h (96) and of relu(u) (96) are never all live.
            //   first Linear    u = b_0 + W_0 relu(h)
            //   skip            v = b_1 + T_1 h = fma(h, hs T_1, b_1): one rounding, as from exact pieces; in place of h
            //   second Linear   v += W_1 relu(u); v is the next h, at hs = 1 / T_1
            for (int blk = 0; blk < a.num_blocks; ++blk) {
                float sb[4];
                f32x16 u[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) load_bias_tile(u[t], bias + t * 32);
                gemm_kmajor_relu<WAVES>(u, h, hs, sm, lane);
                uniform_load(sc, sb);
                const float skip = hs * sb[3];   // (powers of two: exact)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f32x16 b1;
                    load_bias_tile(b1, bias + 128 + t * 32);
                    skip_half<0>(h[t], b1, skip);
                    skip_half<8>(h[t], b1, skip);
                }
                gemm_kmajor_relu<WAVES>(h, u, sb[0], sm, lane);
                hs = sb[2];
                bias += 256;
                sc += 4;
            }

            // the next layer's hidden biases, in front of the final layer's first request: every wave is past a stage barrier
            // behind this layer's last hidden bias read (the last block's second Linear, or the initial GEMM)
            if constexpr (BIAS_LDS) {
                request_hidden(nl);
                __builtin_amdgcn_sched_barrier(0);
            }
            // the residual stream's pieces for the final layer's 24 tiles
#pragma unroll
            for (int t = 0; t < 4; ++t) tile_to_pieces<false>(h[t], hs, p[2 * t], p[2 * t + 1]);

            // ---- final layer with the spline evaluation woven into the MFMAs: the three tiles of a group hold the
            //      logits of this lane's two features A, B (A = T0 + T1[0:8], B = T1[8:16] + T2), at scale 1 / kappa
            if constexpr (KB == 8) {
                using Steps = FusedSteps<INVERSE, 8>;
                // (value-initialised although the first group reads nothing of them: the fields the group loop carries
                //  from one group to the next were undefined on entry, and hipcc merged them with the PREVIOUS layer's
                //  values -- a dozen registers kept across the whole layer, through scratch)
                Steps fa{}, fb{};
                float sf[2];
                uniform_load(sc, sf);
                const float kappa = sf[0];
                fa.kappa = fb.kappa = kappa;
                fa.kl2e = fb.kl2e = 1.44269502162933349609375f * kappa;
                fa.tail_s = fb.tail_s = a.sp.tail_logit * sf[1];
                lds_f32* slot_b = s_row;   // (written from the second group on)
                const lds_f32* fbias = s_fbias + half * 16;
                // the bf8 B operands of the four k-step pairs, made once for the layer's 24 tiles (the r' pieces are read by
                // nothing else from here on: their registers are these)
                i32x8 bx[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) bx[j] = bf8_operand(p[2 * j], p[2 * j + 1]);
                // (the first stage's lead fragments: the final layer's 48 stages read ahead of one another from here on; the
                //  last one reads the next layer's first stage, which nobody uses -- the next GEMM reads its own)
                Lead lead = read_lead(sm.ring + sm.slot * kStageVec4 + lane);
                f32x16 acc[3];
                auto commit = [&](Steps& f, lds_f32* slot) {
                    *slot = f.y;
                    lad_acc += f.lad;
                    quad_status |= f.status;
                };
                [[maybe_unused]] auto store_logits = [&](const f32x16& t, int tile) {
                    if constexpr (DBG) {
                        if (layer == a.num_layers - 1) {
                            float* dst = a.dbg_logits + (size_t)(row0 + r) * (dt * kFinalRows) + tile * 32 + half * 16;
#pragma unroll
                            for (int q_ = 0; q_ < 16; ++q_) dst[q_] = t[q_] * kappa;
                            // (stores and LDS-DMA requests share vmcnt and complete out of order with each other: the
                            //  counted waits of the stream must not see them)
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        }
                    }
                };
                UnitWeave<k8h::kUnitNumA, Steps> w0{fa, fb, a.sp};
                UnitWeave<k8h::kUnitFinishA, Steps> w1{fa, fb, a.sp};
                UnitWeave<k8h::kUnitFinishB, Steps> w2{fa, fb, a.sp};
                for (int g = 0; g < groups; ++g) {
                    lds_f32* slot0 = s_row + tab[kTabTr + g * 4 + half * 2] * kRowPad + r;
                    lds_f32* slot1 = s_row + tab[kTabTr + g * 4 + half * 2 + 1] * kRowPad + r;
                    load_bias_tile(acc[0], fbias + (g * 3 + 0) * 32);
                    if (g > 0) {
                        gemm_tile_pumped<WAVES>(acc[0], p, bx, sm, lane, lead, w2);
                        commit(fb, slot_b);
                    } else {
                        gemm_tile_pumped<WAVES>(acc[0], p, bx, sm, lane, lead, NoWeave{});
                    }
                    store_logits(acc[0], g * 3 + 0);
                    fa.x = *slot0;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        fa.ew[j] = acc[0][j];
                        fa.eh[j] = acc[0][8 + j];
                    }
                    load_bias_tile(acc[1], fbias + (g * 3 + 1) * 32);
                    gemm_tile_pumped<WAVES>(acc[1], p, bx, sm, lane, lead, w0);
                    store_logits(acc[1], g * 3 + 1);
                    fb.x = *slot1;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (j < 7) fa.sd[j] = acc[1][j];
                        fb.ew[j] = acc[1][8 + j];
                    }
                    load_bias_tile(acc[2], fbias + (g * 3 + 2) * 32);
                    gemm_tile_pumped<WAVES>(acc[2], p, bx, sm, lane, lead, w1);
                    store_logits(acc[2], g * 3 + 2);
                    commit(fa, slot0);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        fb.eh[j] = acc[2][j];
                        if (j < 7) fb.sd[j] = acc[2][8 + j];
                    }
                    slot_b = slot1;
                }
                k8h::spline_unit_range<k8h::kUnitFinishB, 0, k8h::spline_unit_slices<k8h::kUnitFinishB, Steps>()>(fa, fb, a.sp);
                commit(fb, slot_b);
            }
            else {
                // ---- any other bin count (K8h's general scheme): T tiles per group of two features, one per lane-half; the
                //      lane-half's 16 T accumulator values are the feature's 3 K - 1 logits, then padding
                constexpr int T = kFinalRows / 16;
                static_assert(T >= 1 && T <= 6, "2 .. 32 bins");
                using Steps = FusedSteps<INVERSE, KB>;
                constexpr int kRest = k8h::any_rest_mask(KB);   // what is left for the next group's first tile
                Steps f{};   // (value-initialised: see the 8-bin branch)
                float sf[2];
                uniform_load(sc, sf);
                const float kappa = sf[0];
                f.kappa = kappa;
                f.kl2e = 1.44269502162933349609375f * kappa;
                f.tail_s = a.sp.tail_logit * sf[1];
                const lds_f32* fbias = s_fbias + half * 16;
                i32x8 bx[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) bx[j] = bf8_operand(p[2 * j], p[2 * j + 1]);
                Lead lead = read_lead(sm.ring + sm.slot * kStageVec4 + lane);
                const int groups_any = dt >> 1;
                f32x16 acc;
                lds_f32* slot = s_row + tab[kTabTr + half] * kRowPad + r;
                load_bias_tile(acc, fbias);
                gemm_tile_pumped(acc, p, bx, sm, lane, lead, NoWeave{});
                for (int g = 0; g < groups_any; ++g) {
                    const lds_f32* gb = fbias + g * T * 32;
                    f.x = *slot;
                    k8h::take_chunk<0, KB>(f, acc);
                    any_group_tiles<1, T, KB, Steps>(acc, f, gb, p, bx, sm, lane, lead, a.sp);
                    if (g + 1 < groups_any) {
                        lds_f32* next_slot = s_row + tab[kTabTr + (g + 1) * 2 + half] * kRowPad + r;
                        load_bias_tile(acc, gb + T * 32);
                        gemm_tile_pumped(acc, p, bx, sm, lane, lead, SeqWeave<kRest, Steps>{f, a.sp});
                        *slot = f.y;
                        slot = next_slot;
                    } else {
                        k8h::spline_seq_range<kRest, 0, k8h::spline_seq_count<kRest, Steps>()>(f, a.sp);
                        *slot = f.y;
                    }
                    lad_acc += f.lad;
                    quad_status |= f.status;
                }
            }
            tb ^= 1;
            // this wave's spline results must be visible to its own gathers of the next layer
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }

        // ---- results: position p of a row comes from slot final[p].  A block with any non-finite value (f16 range
        //      exceeded somewhere, or non-finite inputs) is not written at all: the exact kernel redoes it.
        lad_acc += __shfl_xor(lad_acc, 32, kWave);
        const float sumsq = tile_row_sumsq((const float*)s_row, a.Ds, half, r);
        const bool bad = not_finite(lad_acc) || not_finite(sumsq);
        const bool wave_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
        if (lane == 0) s_bad[wave] = wave_bad ? 1 : 0;
        // stores and LDS-DMA requests complete out of order with each other: drain before the ordinary stores, and
        // before the next row block counts outstanding requests again
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int any_bad = 0;
#pragma unroll
        for (int w_ = 0; w_ < 4; ++w_) any_bad |= s_bad[(WIDE ? wave & 4 : 0) + w_];   // (this wave's 128 rows)
        if (!any_bad && live) {
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
            if (half == 0) {
                float* dst = a.lad + row0 + r;
                float v = a.accumulate ? *dst + lad_acc : lad_acc;
                if (a.normal) v = (-0.5f * sumsq - a.log_z) + v;   // normal.py:31-33, flows/base.py:49
                *dst = v;
            }
            my_status |= quad_status;
        }
        if ((WIDE ? (tid & 255) == 0 && live : tid == 0)) a.redo[quad] = any_bad ? 1 : 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // s_bad is rewritten by the next row block
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the two stages requested past the end
    if (my_status && a.status) atomicOr(a.status, my_status);
}

// (two kernel templates over one body, not a fifth template parameter: the instances keep their names)
template <bool INVERSE, int INIT_KS, bool DBG = false, int KB = 8>
__global__ void __launch_bounds__(kBlock, 2) rqs_resnet_f16x3_kernel(const Args a) {
    rqs_resnet_f16x3_body<INVERSE, INIT_KS, DBG, KB, true>(a);
}
template <bool INVERSE, int INIT_KS, bool DBG = false, int KB = 8>
__global__ void __launch_bounds__(kBlock, 2) rqs_resnet_f16x3_global_bias_kernel(const Args a) {
    rqs_resnet_f16x3_body<INVERSE, INIT_KS, DBG, KB, false>(a);
}

// row blocks per CU from which the launcher takes the wide form (rqs_resnet_f16x3.hip: launch_f16x3)
constexpr int kWideBlocksPerCu = 2;

// the wide form (8 bins, bias area): one workgroup of eight waves per CU
template <bool INVERSE, int INIT_KS>
__global__ void __launch_bounds__(2 * kBlock, 1) rqs_resnet_f16x3_kernel_wide(const Args a) {
    rqs_resnet_f16x3_body<INVERSE, INIT_KS, false, 8, true, 8>(a);
}

}  // namespace k8x
}  // namespace nfa


namespace nfa {
namespace k8x {
typedef void (*KernelFn)(const Args);
// the instances of the other translation units: nullptr when the unit does not hold the combination
KernelFn bins_kernel_a(int K, bool inverse, int init_ks, bool bias_lds);   // 2 .. 7, 9 .. 12 bins
KernelFn bins_kernel_b(int K, bool inverse, int init_ks, bool bias_lds);   // 13 .. 16, 20, 24, 32 bins
}  // namespace k8x
}  // namespace nfa
