// K12: the sequential part of the autoregressive spline layer's inverse (sampling direction) as ONE
// persistent kernel -- AutoregressiveTransform.inverse (autoregressive.py:43-52) for
// MaskedPiecewiseRationalQuadraticAutoregressiveTransform (autoregressive.py:404-495) over a MADE
// conditioner (made.py:233-311, masked residual / feed-forward blocks :67-231).
//
// The reference runs the whole MADE D times.  What actually changes from one iteration to the next is
// little: a hidden unit of degree d is connected to inputs of degree <= d only (made.py:60-63), i.e. it
// is a function of features 0 .. d-1 and final as soon as feature d-1 has been found.  So step t
//   1. evaluates the hidden units of degree t, layer by layer (for H < D - 1 sequential degrees that is
//      one unit per layer: five 256-term dot products instead of four 256 x 256 products per sample),
//   2. takes feature t's P rows of the output layer on the hidden vector as it stands (units of higher
//      degree are still zero and meet exactly-zero masked weights),
//   3. inverts the spline of feature t and records x_t.
// After step T - 1 (T = largest hidden degree) plus one more round of unit updates nothing changes
// any more; the caller finishes features T .. D-1 with one GEMM and one elementwise launch
// (transforms/autoregressive.py).  Same sums as the reference's masked GEMMs in another order.
//
// Samples are independent, so there is no grid-wide step: a workgroup of four waves owns 16 samples for
// all steps.  Round 3: every wave owns FOUR of them for the whole step -- unit chain, output rows, spline --
// with SIXTEEN lanes per sample (lane = (sample sw = lane / 16, part q = lane % 16)): a 256-term dot product
// is four 16-byte chunks per lane and a four-stage DPP butterfly (quad_perm x 2, row_half_mirror,
// row_mirror: no LDS round trip), all sixteen lanes end up with every sum, so the 3K - 1 logits of a
// feature never leave the registers.  (Round 2 gave the chain to wave 0 with four lanes per sample -- 16
// chunks per lane and two ds_bpermute exchanges per unit, 14.7 k of the step's 18.8 k cycles -- and the
// output rows to waves 1..3, joined by three workgroup barriers and a rank-1 correction.)  The waves only
// meet once per step, for the hand-over of the staged block.
// Per-sample state lives in LDS as [vector][16 samples][chunks, padded to a multiple of 16][4 floats]: the
// sixteen lanes of a sample read sixteen consecutive chunks (conflict-free; the samples of a wave are a
// multiple of 64 banks apart), a weight read is one address per part q, broadcast to the four samples.
//
// Everything step t needs from global memory is ONE contiguous block prepared by the host (weights
// pre-masked, rows sorted by degree, zero-padded): a header with the number of units per layer, the
// units' rows, the feature's output rows, the biases and unit indices.  Which block comes next does not
// depend on data, so block t + 1 is pulled into the other half of an LDS double buffer by LDS-DMA
// (global_load_lds, no registers, no waiting) while step t computes; the dot products read weights and
// state from LDS only (a weight read is a 4-address broadcast).  The first version read the rows from
// global memory inside the dot-product loops and spent its time waiting for L2: 35 us per step.
//
// Supported: 8 or 10 bins with linear tails (P = 23 / 29), ReLU, residual blocks (sequential masks) or
// feed-forward blocks (any masks), no context, no batch norm; state that fits the LDS.
// K28 (below, `made_inverse_kernel<KT, 16, true>`, nfa_made_rqs_inverse_ctx_f32): the same with a context, 2 .. 16 bins
// (P = 5 .. 47; no instance uses scratch, none is left out) and steps cut into continuation blocks -- K23's loop.

#include "fused_common.hpp"

#include <hip/hip_ext.h>
#include <stdlib.h>

namespace nfa {

constexpr int kMadeMaxLinears = 12;
constexpr int kMadeSamples = 16;     // per workgroup
constexpr int kMadeWaves = 4;
constexpr int kMadeHeader = 16;      // ints in front of a step block: {units, offset of the unit rows, of the output rows, of the output biases, K23: 1 = the step continues in the next block}
constexpr int kMadeUnitWords = 8;    // per unit, right behind the header: {bias, index, columns, src vector, dst vector, add_stream, set_stream, K23: context vector + 1 (K12: 0)}
#ifndef NFA_K12_ROWS_AHEAD
#define NFA_K12_ROWS_AHEAD 4   // groups of the output rows' dot products requested ahead (dot_rows_64); measured 2: 5.2 k, 3: 4.6 k, 4: 4.0 k cycles per step
#endif
constexpr int kMadeUnitsAhead = 4;   // unit entries every lane reads together with the header (more units: read one by one)
constexpr int kMadeGrain = 256;      // blocks are multiples of 256 floats (one LDS-DMA request of the wave)

struct MadeInvArgs {
    const float* z;          // [B, D] values to invert
    float* x;                // [B, D] features found (columns < T written)
    float* lad;              // [B]   sum of the log-derivatives of columns < T
    float* hidden;           // [B, H] the output layer's input once all hidden units are final
    const float* blocks;     // the step blocks, one after the other
    const int32_t* block_at; // [T + 2] start of block t in grains (K23: [num_blocks + 2])
    int32_t* status;
    int64_t batch;
    int D, H, Hp, Xp, T, num_linears, residual, final_src, stream_vec, num_vectors, max_block;  // max_block in floats
    int kp[kMadeMaxLinears], src[kMadeMaxLinears], dst[kMadeMaxLinears], add_stream[kMadeMaxLinears],
        set_stream[kMadeMaxLinears];
    RqsDev sp;
    unsigned long long* trace;   // debug (nfa_debug_k7_trace): cycle stamps of workgroup 0, wave 0 over the first steps
    // K23 (the affine element): the context terms [B, num_ctx, Hp] and the number of blocks (a step may span several)
    const float* ctx;
    int num_ctx, num_blocks, group;   // group: units of one Linear in groups of eight (NFA_K23_GROUP)
    // K30 (the mixture element; `z` holds the standard normals): the uniforms [B, D], the components chosen (may be null),
    // the number of components and what is added to softplus(unconstrained std)
    const float* uniforms;
    int32_t* components;
    int mog_k;
    float mog_eps;
};

// sum over the sixteen lanes of a sample (a DPP row), every lane gets it
__device__ __forceinline__ float row_sum16(float v) {
    auto dpp = [](float x, int ctrl) {
        return __builtin_bit_cast(float, ctrl == 0xB1   ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false)
                                       : ctrl == 0x4E  ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, false)
                                       : ctrl == 0x141 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, false)
                                                       : __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, false));
    };
    v += dpp(v, 0xB1);    // quad_perm [1, 0, 3, 2]
    v += dpp(v, 0x4E);    // quad_perm [2, 3, 0, 1]
    v += dpp(v, 0x141);   // row_half_mirror: the other quad of the half row
    v += dpp(v, 0x140);   // row_mirror: the other half row
    return v;
}

// sum over the LPS lanes of a sample (LPS = 16: a DPP row; LPS = 32 -- round 4, two samples per wave --: the two
// rows of a 32-lane half exchange their sums through ds_swizzle, lane i <-> i ^ 16)
template <int LPS>
__device__ __forceinline__ float sample_sum(float v) {
    v = row_sum16(v);
    if constexpr (LPS == 32)
        v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));   // and 0x1f, or 0, xor 0x10
    return v;
}

// `R` dot products of weight rows (`pitch` floats apart) with one sample's state vector `vec` (its `chunks`
// 16-byte chunks), both in LDS: this lane takes chunks q, q + 16, ...; every lane of the sample gets the sums
template <int R, int UNROLL, int LPS = 16>
__device__ __forceinline__ void dot_rows(float (&acc)[R], const float* rows, int pitch, const float* vec, int chunks,
                                         int q, int nrows) {
    // (no conditionals inside the loop: rows beyond `nrows` re-read row 0 and their sums are ignored --
    // a branch per row would keep the compiler from batching the LDS reads of several chunks)
    const float* rp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = 0.0f;
        rp[r] = rows + (r < nrows ? r : 0) * pitch;
    }
#pragma unroll UNROLL
    for (int c = q; c < chunks; c += LPS) {
        const vec4f v = *reinterpret_cast<const vec4f*>(vec + c * 4);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const vec4f w = *reinterpret_cast<const vec4f*>(rp[r] + c * 4);
            acc[r] = __builtin_fmaf(w.x, v.x, acc[r]);
            acc[r] = __builtin_fmaf(w.y, v.y, acc[r]);
            acc[r] = __builtin_fmaf(w.z, v.z, acc[r]);
            acc[r] = __builtin_fmaf(w.w, v.w, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = sample_sum<LPS>(acc[r]);
}

// the same for exactly 64 chunks (256 columns: BASELINE configs[4]'s hidden width), software-pipelined by hand:
// the reads of the next 16 chunks are in flight while the current ones are multiplied (hipcc waits for ALL
// outstanding LDS reads in front of the first FMA of a loop body otherwise: four exposed round trips per call)
template <int R, int AHEAD_, int LPS = 16>
__device__ __forceinline__ void dot_rows_64(float (&acc)[R], const float* rows, int pitch, const float* vec, int q, int nrows) {
    // G groups of LPS chunks (LPS = 16: four, LPS = 32: two); AHEAD = how many groups are requested before the first
    // one is multiplied (G = everything up front: right for a single row, whose four FMAs per group hide nothing)
    constexpr int G = 64 / LPS;
    constexpr int AHEAD = AHEAD_ < G ? AHEAD_ : G;
    static_assert(AHEAD >= 1, "");
    const float* rp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) rp[r] = rows + (r < nrows ? r : 0) * pitch + q * 4;
    const float* vp = vec + q * 4;
    vec4f v[G], w[G][R];
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) {
        v[i] = *reinterpret_cast<const vec4f*>(vp + i * LPS * 4);
#pragma unroll
        for (int r = 0; r < R; ++r) w[i][r] = *reinterpret_cast<const vec4f*>(rp[r] + i * LPS * 4);
    }
    float part[G][R];   // one partial sum per group: short dependency chains instead of one of sixteen
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i + AHEAD < G) {
            v[i + AHEAD] = *reinterpret_cast<const vec4f*>(vp + (i + AHEAD) * LPS * 4);
#pragma unroll
            for (int r = 0; r < R; ++r) w[i + AHEAD][r] = *reinterpret_cast<const vec4f*>(rp[r] + (i + AHEAD) * LPS * 4);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float t = w[i][r].x * v[i].x;
            t = __builtin_fmaf(w[i][r].y, v[i].y, t);
            t = __builtin_fmaf(w[i][r].z, v[i].z, t);
            part[i][r] = __builtin_fmaf(w[i][r].w, v[i].w, t);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float t;
        if constexpr (G == 4) t = (part[0][r] + part[1][r]) + (part[2][r] + part[3][r]);
        else t = part[0][r] + part[1][r];
        acc[r] = sample_sum<LPS>(t);
    }
}

// float offset of element k of a sample's vector whose samples are `pitch` chunks apart
__device__ __forceinline__ int state_index(int k, int s, int pitch) { return (s * pitch + (k >> 2)) * 4 + (k & 3); }

// block `t` -> LDS at `dst`: a wave requests one grain (64 lanes x 16 bytes) per instruction, grain g is
// wave g % 4's
template <int NW>
__device__ __forceinline__ void request_block(const MadeInvArgs& a, int t, float* dst, int lane, int wave) {
    const int g0 = a.block_at[t], g1 = a.block_at[t + 1];
    const char* src = reinterpret_cast<const char*>(a.blocks) + (size_t)g0 * (kMadeGrain * 4) + lane * 16;
    char* d = reinterpret_cast<char*>(dst);
    for (int g = wave; g < g1 - g0; g += NW)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)g * (kMadeGrain * 4)),
                                         (__attribute__((address_space(3))) void*)(d + g * (kMadeGrain * 4)), 16, 0, 0);
}

// K23: the same step loop with the affine element of MaskedAffineAutoregressiveTransform (autoregressive.py:96-128) in
// place of the spline -- KT = 0: P = 2 output rows per feature, (unconstrained scale, shift), K2b's arithmetic -- and what
// a MAF needs beside it:
//   * all D features are steps (T = D): steps beyond the largest hidden degree have no units, only output rows, so the
//     kernel writes the complete [B, D] result and there is no tail GEMM and no `hidden` output;
//   * a context enters a MADE as per-sample constants (made.py:274-281 and :187-198): relu(context_layer(ctx)) on the initial
//     layer, blocks[i].context_layer(ctx) on a residual block's first Linear.  The caller computes them with one GEMM,
//     [B, num_ctx, Hp]; every sample's vectors are staged into LDS once, behind the state, and a unit entry's last word
//     names the vector it adds (1-based, 0 = none) after `acc + bias` and before the residual add and the ReLU;
//   * a MAF step is wide (H / (D - 1) units per Linear): a step whose block would not fit twice beside the state is cut
//     into continuation blocks (header word 4 = 1: another block of this step follows; it carries units only, the step's
//     last block the output rows).  The loop runs over blocks; t advances -- and the z prefetch with it -- on a step's
//     last block only.  The hand-over of a block is K12's, unchanged.
// The RQ instances compile to what they were (`if constexpr`): for them a block is a step.
//
// LPS = lanes per sample.  16: four waves x four samples (round 3).  32 (round 4): EIGHT waves x two samples -- the same
// sixteen samples and the same LDS per workgroup, but two waves per SIMD: a batch that gives every CU at most one
// workgroup (configs[4]: 4 096 samples = 256 workgroups) has nothing else to hide the chain's LDS round trips with.
//
// K28: the RQ element inside K23's loop (FULL_): which element a step inverts (AFFINE) and which loop carries it (FULL:
// context vectors, continuation blocks, groups of eight, the float64 total) are two questions.  <KT, 16, true> is the
// sampling kernel of a conditional autoregressive spline layer: T <= D steps, `hidden` written for the caller's tail.
//
// K30: the mixture-of-Gaussians element of nn.nde.MixtureOfGaussiansMADE.sample (nde/made.py:355-388) in K23's loop --
// KT = -1, the number of components K <= 16 at run time (two passes of eight logit rows at most: one instance, no scratch).
// A feature's 3K output rows arrive as [K logit rows][K x (mean, unconstrained std) rows].  Step t:
//   logits l_k = row k . h + bias;  m = max_k l_k, e_k = exp(l_k - m), S = sum_k e_k in index order;  u = uniforms[row, t];
//   THE SELECTION RULE: c = the smallest index whose running sum e_0 + .. + e_c exceeds u * S; K - 1 if none does;
//   then ONLY component c's two rows (an address per sample: `dot_rows` with a per-lane base) -- K + 2 dot products per step
//   instead of 3K --, x_t = mean_c + normals[row, t] * (softplus(ustd_c) + epsilon) in fp32 (`softplus1`, affine_math.hpp).
// All D features are steps; no logabsdet, no `hidden`.  The density-estimator MADE (nde/made.py) differs from the
// transforms' in two places, both settled by the packer: the initial context term is not rectified (the caller's GEMM), and
// a feed-forward block takes the initial layer's output as it is -- bit 1 of a unit's set_stream word: store the unit
// without the ReLU (read by this instance only; the other instances never meet it).
template <int KT, int LPS, bool FULL_ = false>
__global__ void __launch_bounds__((LPS / 4) * kWave) made_inverse_kernel(const MadeInvArgs a) {
#pragma clang fp contract(off)
    constexpr bool AFFINE = KT == 0;
    constexpr bool MOG = KT < 0;                                    // K30: the mixture element
    constexpr bool FULL = AFFINE || MOG || FULL_;                   // K23's loop around the element
    constexpr int P = AFFINE || MOG ? 2 : 3 * KT - 1;
    constexpr int RB = AFFINE ? 2 : 8;                              // output rows per pass of dot_rows
    constexpr int NW = LPS / 4;                                     // waves per workgroup (16 samples)
    constexpr int SPW = kWave / LPS;                                // samples per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & (LPS - 1), s = wave * SPW + lane / LPS;
    const int64_t row = (int64_t)blockIdx.x * kMadeSamples + s;
    const bool live = row < a.batch;
    const int64_t rrow = live ? row : a.batch - 1;
    const int px = ((a.Xp >> 2) + 15) & ~15, ph = ((a.Hp >> 2) + 15) & ~15;   // chunks between two samples
    const int x_floats = kMadeSamples * px * 4, vec_floats = kMadeSamples * ph * 4;
    const int state_floats = x_floats + a.num_vectors * vec_floats;
    float* xs = lds;                                                // [16][px][4]
    float* vecs = lds + x_floats;                                   // [num_vectors][16][ph][4]
    const int ctx_floats = FULL ? a.num_ctx * vec_floats : 0;
    float* ctxs = lds + state_floats;                               // [num_ctx][16][ph][4] (K23)
    float* buf0 = lds + state_floats + ctx_floats;                  // two step blocks
    float* buf1 = buf0 + a.max_block;
    request_block<NW>(a, 0, buf0, lane, wave);
    for (int i = threadIdx.x; i < state_floats; i += NW * kWave) lds[i] = 0.0f;
    if constexpr (FULL) {
        // this sample's context terms, read by its own sixteen lanes only (a dead sample stages the last row's)
        for (int c = 0; c < a.num_ctx; ++c) {
            const float* from = a.ctx + ((size_t)rrow * a.num_ctx + c) * a.Hp;
            float* to = ctxs + c * vec_floats + s * ph * 4;
            for (int k = q; k < (a.Hp >> 2); k += LPS)
                *reinterpret_cast<vec4f*>(to + k * 4) = *reinterpret_cast<const vec4f*>(from + k * 4);
        }
    }

    float lad_acc = 0.0f;
    // (K23 adds D terms where K12 adds T: one after the other in fp32 the sum was 2.1 x as far from float64 as the
    //  reference's pairwise torch.sum at D = 64, so the affine element keeps its total in float64 and rounds once)
    double lad_wide = 0.0;
    int my_status = 0;
    const float* zrow = a.z + rrow * a.D;
    float* stream = a.residual ? vecs + a.stream_vec * vec_floats : nullptr;
    float z_next = zrow[0];
    const float* urow = nullptr;
    float u_next = 0.0f, u_held = 0.0f;
    if constexpr (MOG) {
        urow = a.uniforms + rrow * a.D;
        u_next = urow[0];
    }
    unsigned long long* tr = (a.trace && blockIdx.x == 0 && threadIdx.x == 0) ? a.trace : nullptr;
    int ti = 0;
#define NFA_K12_STAMP() if (tr && ti < 250) tr[ti++] = __builtin_readcyclecounter();
    // (K12: block b is step b.  K23 / K28: `t` advances on a step's last block, `fresh` = the block opens a step)
    const int nb = FULL ? a.num_blocks : 0;
    int t_affine = 0;
    bool fresh = true;
    float z_held = 0.0f;
    for (int b = 0; FULL ? b < nb : b <= a.T; ++b) {
        const int t = FULL ? t_affine : b;
        float* blk = (b & 1) ? buf1 : buf0;
        NFA_K12_STAMP()
        // block t has landed (every wave's share, requested a whole step ago), every wave is done with the
        // other buffer half (and, at t = 0, the state is zeroed)
        asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        NFA_K12_STAMP()
        if constexpr (FULL) {
            if (b + 1 < nb) request_block<NW>(a, b + 1, (b & 1) ? buf0 : buf1, lane, wave);
            if (fresh) {   // (the z prefetch follows t, not the block index)
                z_held = z_next;
                if (t + 1 < a.T) z_next = zrow[t + 1];
                if constexpr (MOG) {
                    u_held = u_next;
                    if (t + 1 < a.T) u_next = urow[t + 1];
                }
            }
        }
        const float z_t = FULL ? z_held : z_next;
        if constexpr (!FULL) {
            if (t < a.T) {
                request_block<NW>(a, t + 1, (t & 1) ? buf0 : buf1, lane, wave);
                if (t + 1 < a.T) z_next = zrow[t + 1];
            }
        }
        // ---- the step's control data in ONE round trip: header and the first unit entries (a dependent LDS
        //      read per field was most of the unit chain's time: five to six round trips per unit)
        typedef int vec4i __attribute__((ext_vector_type(4)));
        const vec4i* bv = reinterpret_cast<const vec4i*>(blk);
        const vec4i h0 = bv[0];
        vec4i ue[kMadeUnitsAhead][2];
#pragma unroll
        for (int u = 0; u < kMadeUnitsAhead; ++u) {
            ue[u][0] = bv[kMadeHeader / 4 + 2 * u];
            ue[u][1] = bv[kMadeHeader / 4 + 2 * u + 1];
        }
        const int units = __builtin_amdgcn_readfirstlane(h0.x);
        const float* rows = blk + __builtin_amdgcn_readfirstlane(h0.y);
        const float* wf = blk + __builtin_amdgcn_readfirstlane(h0.z);
        const float* fbias = blk + __builtin_amdgcn_readfirstlane(h0.w);
        bool continued = false;   // another block of this step follows
        if constexpr (FULL) continued = __builtin_amdgcn_readfirstlane(bv[1].x) != 0;
        // ---- 1. hidden units of degree t in layer order (typically one unit per layer), for this wave's samples
        auto unit = [&](vec4i e0, vec4i e1) {
            const float bias = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(e0.x));
            const int j = __builtin_amdgcn_readfirstlane(e0.y), kp = __builtin_amdgcn_readfirstlane(e0.z);
            const int src_v = __builtin_amdgcn_readfirstlane(e0.w), dst_v = __builtin_amdgcn_readfirstlane(e1.x);
            const bool add_stream = __builtin_amdgcn_readfirstlane(e1.y) != 0;
            const int stream_word = __builtin_amdgcn_readfirstlane(e1.z);
            const bool set_stream = MOG ? (stream_word & 1) != 0 : stream_word != 0;
            const bool raw = MOG && (stream_word & 2) != 0;     // K30: the unit enters the next Linear as it is
            const float* src = src_v < 0 ? xs + s * px * 4 : vecs + src_v * vec_floats + s * ph * 4;
            const int at = state_index(j, s, ph);
            const float carried = add_stream ? stream[at] : 0.0f;   // (in flight beside the dot product's reads)
            int ctx_v = 0;
            float ctx_term = 0.0f;
            if constexpr (FULL) {
                ctx_v = __builtin_amdgcn_readfirstlane(e1.w);
                if (ctx_v) ctx_term = ctxs[(ctx_v - 1) * vec_floats + at];
            }
            float acc[1];
            if (kp == 256) dot_rows_64<1, 4, LPS>(acc, rows, kp, src, q, 1);
            else dot_rows<1, 4, LPS>(acc, rows, kp, src, kp >> 2, q, 1);
            rows += kp;
            float v = acc[0] + bias;
            if constexpr (FULL) {
                if (ctx_v) v = v + ctx_term;                    // h + relu(context_layer(ctx)) / lower(h) + context_layer(ctx)
            }
            if (add_stream) v = carried + v;                    // residual connection (made.py:128)
            if (q == 0) {
                if (set_stream) stream[at] = v;
                if (dst_v >= 0) vecs[dst_v * vec_floats + at] = v < 0.0f && !raw ? 0.0f : v;   // ReLU'd for the next Linear (NaN stays)
            }
            // a unit just written is an input of the next Linear (same wave: LDS is in order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        };
        bool one_by_one = true;
        if constexpr (FULL) {
            // K23, NFA_K23_GROUP: a MAF step has many units per Linear -- consecutive in the block, the same source vector and
            // width, independent of each other.  Up to eight of them per pass of dot_rows: the source vector is read once
            // for the eight rows, one fence per group.  Every dot product keeps its summation order (dot_rows<R> sums row
            // by row as dot_rows<1> does), so the results are the one-by-one path's bit for bit.
            if (a.group) {
                one_by_one = false;
                constexpr int RG = 8;
                const int* words = reinterpret_cast<const int*>(blk);
                for (int u = 0; u < units;) {
                    const vec4i f0 = bv[kMadeHeader / 4 + 2 * u];
                    const int kp = __builtin_amdgcn_readfirstlane(f0.z), src_v = __builtin_amdgcn_readfirstlane(f0.w);
                    // the run of units of this Linear from u on (at most RG).  (The seven entries behind u are read whether
                    // they exist or not: 16 + 8 (units + 7) words are inside a block of >= 256 words that holds the units' rows.)
                    int next_src[RG - 1];
#pragma unroll
                    for (int i = 1; i < RG; ++i) next_src[i - 1] = words[kMadeHeader + kMadeUnitWords * (u + i) + 3];
                    int g = 1;
#pragma unroll
                    for (int i = 1; i < RG; ++i)
                        if (g == i && u + i < units && __builtin_amdgcn_readfirstlane(next_src[i - 1]) == src_v) g = i + 1;
                    const float* src = src_v < 0 ? xs + s * px * 4 : vecs + src_v * vec_floats + s * ph * 4;
                    float acc[RG];
                    if (kp == 256) dot_rows_64<RG, NFA_K12_ROWS_AHEAD, LPS>(acc, rows, kp, src, q, g);
                    else dot_rows<RG, 4, LPS>(acc, rows, kp, src, kp >> 2, q, g);
                    rows += g * kp;
#pragma unroll
                    for (int i = 0; i < RG; ++i) {
                        if (i < g) {
                            const vec4i e0 = bv[kMadeHeader / 4 + 2 * (u + i)], e1 = bv[kMadeHeader / 4 + 2 * (u + i) + 1];
                            const float bias = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(e0.x));
                            const int j = __builtin_amdgcn_readfirstlane(e0.y), dst_v = __builtin_amdgcn_readfirstlane(e1.x);
                            const bool add_stream = __builtin_amdgcn_readfirstlane(e1.y) != 0;
                            const int stream_word = __builtin_amdgcn_readfirstlane(e1.z);
                            const bool set_stream = MOG ? (stream_word & 1) != 0 : stream_word != 0;
                            const bool raw = MOG && (stream_word & 2) != 0;
                            const int ctx_v = __builtin_amdgcn_readfirstlane(e1.w);
                            const int at = state_index(j, s, ph);
                            float v = acc[i] + bias;
                            if (ctx_v) v = v + ctxs[(ctx_v - 1) * vec_floats + at];
                            if (add_stream) v = stream[at] + v;
                            if (q == 0) {
                                if (set_stream) stream[at] = v;
                                if (dst_v >= 0) vecs[dst_v * vec_floats + at] = v < 0.0f && !raw ? 0.0f : v;
                            }
                        }
                    }
                    // the group's units are inputs of the next Linear (same wave: LDS is in order)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    u += g;
                }
            }
        }
        if (one_by_one) {
#pragma unroll
            for (int u = 0; u < kMadeUnitsAhead; ++u)
                if (u < units) unit(ue[u][0], ue[u][1]);
            for (int u = kMadeUnitsAhead; u < units; ++u) unit(bv[kMadeHeader / 4 + 2 * u], bv[kMadeHeader / 4 + 2 * u + 1]);
        }
        NFA_K12_STAMP()
        if constexpr (FULL) {
            fresh = !continued;
            if (continued) continue;
        }
        if (t == a.T) break;
        // ---- 2. feature t's P output rows on the hidden vector as it stands: all sums in every lane of the sample
        const float* fin = vecs + a.final_src * vec_floats + s * ph * 4;
        if constexpr (MOG) {
            // ---- 2. K30: the K logits of feature t (rows 0 .. K - 1 of its output rows), all sums in every lane of the sample
            const int K = a.mog_k;
            float lg[16];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                const int left = K - g * 8;
                if (left > 0) {
                    if (a.Hp == 256) dot_rows_64<8, NFA_K12_ROWS_AHEAD, LPS>(acc, wf + g * 8 * a.Hp, a.Hp, fin, q, left < 8 ? left : 8);
                    else dot_rows<8, 4, LPS>(acc, wf + g * 8 * a.Hp, a.Hp, fin, a.Hp >> 2, q, left < 8 ? left : 8);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) lg[g * 8 + i] = i < left ? acc[i] + fbias[g * 8 + i] : -INFINITY;
            }
            // ---- 3. the component: the smallest c with e_0 + .. + e_c > u S, K - 1 if there is none (e_k = 0 behind K - 1)
            float m = lg[0];
#pragma unroll
            for (int k = 1; k < 16; ++k) m = lg[k] > m ? lg[k] : m;
            float e[16], S = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                e[k] = k < K ? expf(lg[k] - m) : 0.0f;
                S += e[k];
            }
            const float bar = u_held * S;
            float run = 0.0f;
            int c = K - 1;
            bool found = false;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                run += e[k];
                if (!found && run > bar) {
                    c = k;
                    found = true;
                }
            }
            // ---- 4. component c's mean and unconstrained std: two rows at an address of the SAMPLE's own
            float ms[2];
            const float* crow = wf + (K + 2 * c) * a.Hp;
            if (a.Hp == 256) dot_rows_64<2, NFA_K12_ROWS_AHEAD, LPS>(ms, crow, a.Hp, fin, q, 2);
            else dot_rows<2, 4, LPS>(ms, crow, a.Hp, fin, a.Hp >> 2, q, 2);
            const float mean = ms[0] + fbias[K + 2 * c], ustd = ms[1] + fbias[K + 2 * c + 1];
            const float y = mean + z_t * (softplus1(ustd) + a.mog_eps);   // (nde/made.py:376-386)
            ++t_affine;
            if (q == 0) {
                xs[state_index(t, s, px)] = y;
                if (a.components && live) a.components[row * a.D + t] = c;   // (diagnostic: a global store per step)
            }
        } else {
            float p[P];
#pragma unroll
            for (int g = 0; g < (P + RB - 1) / RB; ++g) {
                float acc[RB];
                const int left = P - g * RB;
                if (a.Hp == 256) dot_rows_64<RB, NFA_K12_ROWS_AHEAD, LPS>(acc, wf + g * RB * a.Hp, a.Hp, fin, q, left < RB ? left : RB);
                else dot_rows<RB, 4, LPS>(acc, wf + g * RB * a.Hp, a.Hp, fin, a.Hp >> 2, q, left < RB ? left : RB);
#pragma unroll
                for (int i = 0; i < RB; ++i)
                    if (g * RB + i < P) p[g * RB + i] = acc[i] + fbias[g * RB + i];
            }
            NFA_K12_STAMP()
            // ---- 3. invert feature t (rational_quadratic.py:66-181 through the same evaluation as K5); every
            //      lane of a sample does it, one records the result
            float y, l;
            if constexpr (AFFINE) {
                affine_element<true>(z_t, p[1], scale_of(p[0], NFA_SCALE_SOFTPLUS), y, l);   // (K2b: autoregressive.py:96-121)
            } else {
                my_status |= rqs_eval<KT, true, true, true>(z_t, p, a.sp, y, l);
            }
            if constexpr (FULL) ++t_affine;
            if constexpr (FULL) lad_wide += (double)l;
            else lad_acc += l;
            // (kept in LDS only: a global store per step would sit in front of the next step's vmcnt(0))
            if (q == 0) xs[state_index(t, s, px)] = y;
        }
        NFA_K12_STAMP()
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the features found -> the first T columns of the samples' rows; the final hidden vector of every sample:
    // input of the output layer for features >= T
    if (live) {
        for (int k = q; k < a.T; k += LPS) a.x[row * a.D + k] = xs[state_index(k, s, px)];
        if constexpr (!MOG) {
            if (q == 0) a.lad[row] = FULL ? (float)lad_wide : lad_acc;
        }
        if constexpr (!AFFINE && !MOG) {
            const float* fin = vecs + a.final_src * vec_floats;
            for (int k = q; k < a.H; k += LPS) a.hidden[row * a.H + k] = fin[state_index(k, s, ph)];
        }
    } else {
        my_status = 0;
    }
    if (my_status && a.status) atomicOr(a.status, my_status);
}


// the `layout` words of ops.pack_made_schedule -> `a`
static int read_made_layout(const int32_t* layout, int32_t layout_len, int32_t hidden_features, MadeInvArgs& a) {
    // layout: [num_linears, residual, final_src, stream_vec, num_vectors, Hp, Xp, max_block,
    //          then per Linear: padded_columns, src, dst, add_stream, set_stream]
    const int n = layout[0];
    if (n < 1 || n > kMadeMaxLinears || layout_len != 8 + 5 * n) return NFA_ERR_INVALID_ARGUMENT;
    a.num_linears = n;
    a.residual = layout[1];
    a.final_src = layout[2];
    a.stream_vec = layout[3];
    a.num_vectors = layout[4];
    a.Hp = layout[5];
    a.Xp = layout[6];
    a.max_block = layout[7];
    for (int l = 0; l < n; ++l) {
        const int32_t* e = layout + 8 + 5 * l;
        a.kp[l] = e[0];
        a.src[l] = e[1];
        a.dst[l] = e[2];
        a.add_stream[l] = e[3];
        a.set_stream[l] = e[4];
        if ((a.kp[l] & 15) != 0 || a.src[l] >= a.num_vectors || a.dst[l] >= a.num_vectors) return NFA_ERR_INVALID_ARGUMENT;
    }
    if ((a.Hp & 15) != 0 || (a.Xp & 15) != 0 || a.Hp < hidden_features || a.final_src < 0 || a.num_vectors < 1 ||
        a.final_src >= a.num_vectors || a.max_block < kMadeGrain || (a.max_block % kMadeGrain) != 0 ||
        (a.residual && (a.stream_vec < 0 || a.stream_vec >= a.num_vectors)))
        return NFA_ERR_INVALID_ARGUMENT;
    return NFA_OK;
}

// bytes of LDS: the state of sixteen samples (the features, one vector per Linear, `extra_vectors` more) and two blocks
static size_t made_lds_bytes(const MadeInvArgs& a, int extra_vectors) {
    const size_t px = (((size_t)a.Xp >> 2) + 15) & ~(size_t)15, ph = (((size_t)a.Hp >> 2) + 15) & ~(size_t)15;   // chunks per sample
    return ((px + (size_t)(a.num_vectors + extra_vectors) * ph) * 4 * kMadeSamples + 2 * (size_t)a.max_block) * sizeof(float);
}

}  // namespace nfa

using namespace nfa;

extern "C" int nfa_made_rqs_inverse_f32(const float* inputs, const float* step_blocks, const int32_t* block_starts,
                                        const int32_t* layout, int32_t layout_len, float* outputs,
                                        float* logabsdet, float* hidden_out, int32_t* status, int64_t batch,
                                        int32_t features, int32_t hidden_features, int32_t sequential_steps,
                                        const nfa_rqs_spec* spec, void* stream) {
    if (batch < 0 || features < 1 || hidden_features < 1 || sequential_steps < 0 || sequential_steps > features ||
        !layout || layout_len < 8)
        return NFA_ERR_INVALID_ARGUMENT;
    MadeInvArgs a;
    int rc = make_dev_spec(spec, &a.sp);
    if (rc != NFA_OK) return rc;
    if (a.sp.beta != 1.0f || !a.sp.linear || (a.sp.K != 8 && a.sp.K != 10)) return NFA_ERR_UNSUPPORTED;
    rc = read_made_layout(layout, layout_len, hidden_features, a);
    if (rc != NFA_OK) return rc;
    const size_t lds = made_lds_bytes(a, 0);
    if (lds + 4096 > (size_t)kCuLds) return NFA_ERR_UNSUPPORTED;   // (+ the 2 KB of logits and alignment)
    if (batch == 0) return NFA_OK;
    if (!inputs || !step_blocks || !block_starts || !outputs || !logabsdet || !hidden_out) return NFA_ERR_INVALID_ARGUMENT;
    a.z = inputs;
    a.x = outputs;
    a.lad = logabsdet;
    a.hidden = hidden_out;
    a.blocks = step_blocks;
    a.block_at = block_starts;
    a.status = status;
    a.batch = batch;
    a.D = features;
    a.H = hidden_features;
    a.T = sequential_steps;
    a.trace = g_k7_trace;
    a.ctx = nullptr;
    a.num_ctx = 0;
    a.num_blocks = sequential_steps + 1;
    a.group = 0;
    // 32 lanes per sample (eight waves per workgroup: two per SIMD) was built in round 4 on the theory that the step
    // is a chain of LDS round trips which a second wave on the SIMD would hide; it is slower (every lane of a sample
    // repeats the spline inversion, the DPP sum grows a ds_swizzle stage): NFA_K12_LPS=32 selects it, 16 is the default
    const int64_t blocks = (batch + kMadeSamples - 1) / kMadeSamples;
    const char* lps_env = getenv("NFA_K12_LPS");
    const int lps = lps_env && atoi(lps_env) == 32 ? 32 : 16;   // (measured: 32 is SLOWER, 2.15 vs 1.97 ms at configs[4] -- profiles/r4/k12_lanes_per_sample.txt)
    void (*kern)(const MadeInvArgs) = a.sp.K == 8 ? (lps == 32 ? made_inverse_kernel<8, 32> : made_inverse_kernel<8, 16>)
                                                  : (lps == 32 ? made_inverse_kernel<10, 32> : made_inverse_kernel<10, 16>);
    note_layer_kernel("made_rqs_inverse_kernel<K=%d, lanes_per_sample=%d>", a.sp.K, lps);
    return launch_kernel(kern, dim3((unsigned)blocks), dim3((lps / 4) * kWave), lds, (hipStream_t)stream, a,
                         kCuLds - 4096, false);
}

// K23: AutoregressiveTransform.inverse of MaskedAffineAutoregressiveTransform, all features, context included
extern "C" int nfa_made_affine_inverse_f32(const float* inputs, const float* context_terms, int32_t context_vectors,
                                           const float* step_blocks, const int32_t* block_starts, int32_t num_blocks,
                                           const int32_t* layout, int32_t layout_len, float* outputs, float* logabsdet,
                                           int64_t batch, int32_t features, int32_t hidden_features, void* stream) {
    if (batch < 0 || features < 1 || hidden_features < 1 || context_vectors < 0 || !layout || layout_len < 8)
        return NFA_ERR_INVALID_ARGUMENT;
    MadeInvArgs a = {};
    int rc = read_made_layout(layout, layout_len, hidden_features, a);
    if (rc != NFA_OK) return rc;
    // one block per step at least, t = 0 .. features (the last one holds nothing); at most one context vector per Linear
    if (a.Xp < features || num_blocks < features + 1 || context_vectors > a.num_linears) return NFA_ERR_INVALID_ARGUMENT;
    const size_t lds = made_lds_bytes(a, context_vectors);
    if (lds + 4096 > (size_t)kCuLds) return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    if (!inputs || !step_blocks || !block_starts || !outputs || !logabsdet || (context_vectors > 0 && !context_terms))
        return NFA_ERR_INVALID_ARGUMENT;
    const int64_t blocks = (batch + kMadeSamples - 1) / kMadeSamples;
    if (blocks > 0x7fffffff) return NFA_ERR_UNSUPPORTED;
    a.z = inputs;
    a.x = outputs;
    a.lad = logabsdet;
    a.hidden = nullptr;
    a.blocks = step_blocks;
    a.block_at = block_starts;
    a.status = nullptr;
    a.batch = batch;
    a.D = features;
    a.H = hidden_features;
    a.T = features;
    a.trace = nullptr;
    a.ctx = context_terms;
    a.num_ctx = context_vectors;
    a.num_blocks = num_blocks;
    // units in groups of eight where a Linear has at least five units per step (hidden / (features - 1)): measured 1.2-1.3 x
    // faster at 6.4, 8.5 and 18 units, 0.88 x and 0.70 x at 3 and 2 (profiles/maf_sample_time.json); NFA_K23_GROUP=0 / 1
    // forces either (A/B: the same bits)
    const char* group_env = getenv("NFA_K23_GROUP");
    a.group = group_env && group_env[0] ? (atoi(group_env) != 0 ? 1 : 0)
                                        : (hidden_features >= 5 * (features > 1 ? features - 1 : 1) ? 1 : 0);
    note_layer_kernel("made_inverse_kernel<element=affine, context=%d, continuation_blocks=%d, group=%d>",
                      context_vectors > 0 ? 1 : 0, num_blocks - (features + 1), a.group);
    return launch_kernel(made_inverse_kernel<0, 16>, dim3((unsigned)blocks), dim3(4 * kWave), lds, (hipStream_t)stream, a,
                         kCuLds - 4096, false);
}

// K28: the sequential features of MaskedPiecewiseRationalQuadraticAutoregressiveTransform.inverse in K23's loop -- context,
// continuation blocks, groups, float64 total -- with K12's outputs (columns < T, `hidden_out`, `status`)
template <int KT>
static void (*made_rqs_full_kernel(int K))(const MadeInvArgs) {
    if constexpr (KT > 16) return nullptr;
    else return K == KT ? made_inverse_kernel<KT, 16, true> : made_rqs_full_kernel<KT + 1>(K);
}

extern "C" int nfa_made_rqs_inverse_ctx_f32(const float* inputs, const float* context_terms, int32_t context_vectors,
                                            const float* step_blocks, const int32_t* block_starts, int32_t num_blocks,
                                            const int32_t* layout, int32_t layout_len, float* outputs, float* logabsdet,
                                            float* hidden_out, int32_t* status, int64_t batch, int32_t features,
                                            int32_t hidden_features, int32_t sequential_steps, const nfa_rqs_spec* spec,
                                            void* stream) {
    if (batch < 0 || features < 1 || hidden_features < 1 || sequential_steps < 0 || sequential_steps > features ||
        context_vectors < 0 || !layout || layout_len < 8)
        return NFA_ERR_INVALID_ARGUMENT;
    MadeInvArgs a = {};
    int rc = make_dev_spec(spec, &a.sp);
    if (rc != NFA_OK) return rc;
    if (a.sp.beta != 1.0f || !a.sp.linear || a.sp.K < 2 || a.sp.K > 16) return NFA_ERR_UNSUPPORTED;
    rc = read_made_layout(layout, layout_len, hidden_features, a);
    if (rc != NFA_OK) return rc;
    // one block per step at least and one behind the last step; at most one context vector per Linear
    if (a.Xp < sequential_steps || num_blocks < sequential_steps + 1 || context_vectors > a.num_linears)
        return NFA_ERR_INVALID_ARGUMENT;
    const size_t lds = made_lds_bytes(a, context_vectors);
    if (lds + 4096 > (size_t)kCuLds) return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    if (!inputs || !step_blocks || !block_starts || !outputs || !logabsdet || !hidden_out ||
        (context_vectors > 0 && !context_terms))
        return NFA_ERR_INVALID_ARGUMENT;
    const int64_t blocks = (batch + kMadeSamples - 1) / kMadeSamples;
    if (blocks > 0x7fffffff) return NFA_ERR_UNSUPPORTED;
    a.z = inputs;
    a.x = outputs;
    a.lad = logabsdet;
    a.hidden = hidden_out;
    a.blocks = step_blocks;
    a.block_at = block_starts;
    a.status = status;
    a.batch = batch;
    a.D = features;
    a.H = hidden_features;
    a.T = sequential_steps;
    a.trace = nullptr;
    a.ctx = context_terms;
    a.num_ctx = context_vectors;
    a.num_blocks = num_blocks;
    // K23's rule for the groups of eight (units per Linear and step: hidden / (features - 1)); NFA_K23_GROUP=0 / 1 forces either
    const char* group_env = getenv("NFA_K23_GROUP");
    a.group = group_env && group_env[0] ? (atoi(group_env) != 0 ? 1 : 0)
                                        : (hidden_features >= 5 * (features > 1 ? features - 1 : 1) ? 1 : 0);
    void (*kern)(const MadeInvArgs) = made_rqs_full_kernel<2>(a.sp.K);
    if (!kern) return NFA_ERR_UNSUPPORTED;
    note_layer_kernel("made_inverse_kernel<element=rqs, K=%d, context=%d, continuation_blocks=%d, group=%d>", a.sp.K,
                      context_vectors > 0 ? 1 : 0, num_blocks - (sequential_steps + 1), a.group);
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(4 * kWave), lds, (hipStream_t)stream, a, kCuLds - 4096, false);
}

// K30: MixtureOfGaussiansMADE.sample (nde/made.py:355-388) -- all features, context included, one launch
extern "C" int nfa_made_mog_sample_f32(const float* uniforms, const float* normals, const float* context_terms,
                                       int32_t context_vectors, const float* step_blocks, const int32_t* block_starts,
                                       int32_t num_blocks, const int32_t* layout, int32_t layout_len, float* outputs,
                                       int32_t* components_out, int64_t batch, int32_t features, int32_t hidden_features,
                                       int32_t num_components, double epsilon, void* stream) {
    if (batch < 0 || features < 1 || hidden_features < 1 || context_vectors < 0 || num_components < 1 || !layout ||
        layout_len < 8)
        return NFA_ERR_INVALID_ARGUMENT;
    if (num_components > 16) return NFA_ERR_UNSUPPORTED;
    MadeInvArgs a = {};
    int rc = read_made_layout(layout, layout_len, hidden_features, a);
    if (rc != NFA_OK) return rc;
    // one block per step at least, t = 0 .. features (the last one holds nothing); at most one context vector per Linear
    if (a.Xp < features || num_blocks < features + 1 || context_vectors > a.num_linears) return NFA_ERR_INVALID_ARGUMENT;
    const size_t lds = made_lds_bytes(a, context_vectors);
    if (lds + 4096 > (size_t)kCuLds) return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    if (!uniforms || !normals || !step_blocks || !block_starts || !outputs || (context_vectors > 0 && !context_terms))
        return NFA_ERR_INVALID_ARGUMENT;
    const int64_t blocks = (batch + kMadeSamples - 1) / kMadeSamples;
    if (blocks > 0x7fffffff) return NFA_ERR_UNSUPPORTED;
    a.z = normals;
    a.x = outputs;
    a.blocks = step_blocks;
    a.block_at = block_starts;
    a.batch = batch;
    a.D = features;
    a.H = hidden_features;
    a.T = features;
    a.ctx = context_terms;
    a.num_ctx = context_vectors;
    a.num_blocks = num_blocks;
    a.uniforms = uniforms;
    a.components = components_out;
    a.mog_k = num_components;
    a.mog_eps = (float)epsilon;
    // K23's rule for the groups of eight (units per Linear and step: hidden / (features - 1)); NFA_K23_GROUP=0 / 1 forces either
    const char* group_env = getenv("NFA_K23_GROUP");
    a.group = group_env && group_env[0] ? (atoi(group_env) != 0 ? 1 : 0)
                                        : (hidden_features >= 5 * (features > 1 ? features - 1 : 1) ? 1 : 0);
    note_layer_kernel("made_inverse_kernel<element=mog, K=%d, context=%d, continuation_blocks=%d, group=%d>", num_components,
                      context_vectors > 0 ? 1 : 0, num_blocks - (features + 1), a.group);
    return launch_kernel(made_inverse_kernel<-1, 16>, dim3((unsigned)blocks), dim3(4 * kWave), lds, (hipStream_t)stream, a,
                         kCuLds - 4096, false);
}
