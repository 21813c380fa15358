// K33: K14's pair of training kernels (resnet_train.hip) for a ResidualNet conditioner of 129 .. 256 hidden units, on K32's
// work split (wide_layer_common.hpp): the hidden part of nn/nets/resnet.py:92-100 -- initial Linear, blocks
// h += W_1 relu(W_0 relu(h) + b_0) + b_1, optionally the final Linear -- forward in one kernel that also leaves behind what
// the backward pass and K10 (linear_wgrad.hip) need, and the whole chain of input gradients in a second one.
//
//   forward  (nfa_resnet_wide_forward_f32):  x [B, d_i] -> hidden [B, Hp], saved[2 k] = relu(h_k), saved[2 k + 1] =
//            relu(a_k) as [B, Hp] planes (K10's `inputs`, and the ReLU masks of the backward pass), params [B, out].
//   backward (nfa_resnet_wide_backward_f32): g_params [B, out] (or g_hidden [B, Hp]) -> grad_hidden, grads[2 k + 1] =
//            (W_1^T g_h) . [a_k > 0], grads[2 k] = g_h += (W_0^T g_a) . [h_k > 0], g_x = W_in^T g_h_0.
//
// Work split.  K14's wave owns 32 rows x 128 columns in registers; at 256 columns that does not fit.  As in K32 one
// workgroup of eight waves per CU works on 64 rows (two 32-row tiles), persistent over the batch's 64-row blocks; wave w
// owns hidden columns 32 w .. 32 w + 31 of every hidden GEMM for both row tiles, and the operand of the next GEMM goes
// through the exchange buffer in LDS as three bf16 pieces (exchange_store / gemm_exchange), two barriers around each
// exchange.  Hp = the width padded to a multiple of 32; tile and k-step counts are run-time values, a wave beyond Hp
// computes nothing in the hidden GEMMs, keeps every barrier and takes its share of the final Linear (forward) or feeds
// its columns of g_params (backward).  Weights: the wave's own fragments from global memory straight into registers, two
// k-steps ahead; the last requests of a GEMM fetch the first fragments of the wave's next GEMM.
//
// Arithmetic: K8's -- three bf16 pieces per operand, six products on v_mfma_f32_32x32x16_bf16, the full fp32 range, so
// gradients need no scaling.  A block's second Linear (and the backward pass's second product) has accumulators of its
// own and joins the stream with ONE addition (DESIGN.md section 4 "K14 / K10: how they are tested").
//
// Stores: in the accumulator layout a lane holds 16-byte pieces of 32 different 128-byte lines (a third of K14's forward
// kernel until its NFA_K14_LDS_STORES).  Every 32 x 32 tile goes through a wave-private 32 x 36-float LDS image and
// leaves (or arrives: g_params, g_hidden, the saved planes the masks are re-derived from) as whole 128-byte lines.  No
// packed mask words: a wave's 64 x 32 slice of a saved plane is 128 bytes per row, read once.
//
// LDS: exchange buffer 16 k-steps x 6 KB = 96 KB (always 16: a chunk of the final Linear's input gradient is 256
// columns of g_params whatever Hp is) + eight staging images of 4 608 bytes = 36 KB: 132 KB of the CU's 160 KB.
// Deterministic: no atomics, every sum in a fixed order.

#include "wide_layer_common.hpp"

namespace nfa {
namespace k33 {

using namespace wide;

constexpr int kPitch = 36;                      // floats per row of a staging image (32 + 4: b128 accesses)
constexpr int kImageFloats = 32 * kPitch;       // per wave
constexpr int kXSteps = 16;                     // k-steps of the exchange buffer
constexpr size_t kLdsBytes = (size_t)kXSteps * kStepVec4 * 16 + (size_t)kWaves * kImageFloats * sizeof(float);

struct WideTrainArgs {
    const float* x;         // forward: [B, d_i];  backward: g_hidden [B, Hp] (null: start from gparams)
    const vec4f* w;         // fragments, [column tile][k-step][piece][lane] x 16 B per GEMM
    const float* bias;      // forward: accumulator order, Hp (1 + 2 nb), then 32 per final tile
    float* saved;           // [2 nb][B][Hp] (forward: written, backward: read)
    float* hidden;          // forward: hidden [B, Hp];  backward: grad_hidden [B, Hp] (with gparams)
    float* params;          // forward: [B, out]
    const float* gparams;   // backward: [B, out]
    float* grads;           // backward: [2 nb][B][Hp]
    float* gx;              // backward: [B, d_i]
    int64_t batch;          // multiple of 64
    int di, nb, tiles, nks, init_ks;   // Hp / 32, Hp / 16, k-steps of the initial Linear (2 or 4)
    int out, ftiles, fks;   // final Linear: columns, 32-column tiles, k-steps of its input gradient (2 ftiles)
};

// The staging images carry data from lane to lane of ONE wave without a workgroup barrier.  The compiler knows nothing of
// that: around the store's `if (4 * c < cols)` it moved the NEXT tile's image writes of the lanes that skip the store in
// front of the other lanes' reads of this tile (rows 8 j + 5 .. 7 of a 20-column tile came out as the next tile's).  A
// convergent operation that clobbers memory between the phases keeps every lane's accesses on their side of it.
#define NFA_K33_WAVE_FENCE()                \
    do {                                    \
        __builtin_amdgcn_wave_barrier();    \
        asm volatile("" ::: "memory");      \
    } while (0)

// accumulator tile (lane (half, r): row r, columns 8 q4 + 4 half + 0..3) -> rows row0 .. row0 + 31, columns col0 .. of a
// [., ld] array through the wave's image: four stores of eight full 128-byte lines; `cols` valid columns (multiple of 4)
template <bool RELU>
__device__ __forceinline__ void store_tile(float* base, int64_t row0, int col0, int ld, int cols, const f32x16& a,
                                           float* image, int lane) {
    float* mine = image + (lane & 31) * kPitch + 4 * (lane >> 5);
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        vec4f v = {a[4 * q4], a[4 * q4 + 1], a[4 * q4 + 2], a[4 * q4 + 3]};
        if (RELU) {   // NaN stays NaN (torch.relu)
            v.x = v.x < 0.0f ? 0.0f : v.x;
            v.y = v.y < 0.0f ? 0.0f : v.y;
            v.z = v.z < 0.0f ? 0.0f : v.z;
            v.w = v.w < 0.0f ? 0.0f : v.w;
        }
        *reinterpret_cast<vec4f*>(mine + 8 * q4) = v;
    }
    NFA_K33_WAVE_FENCE();
    const int c = lane & 7, rr = lane >> 3;
    float* dst = base + row0 * ld + col0 + 4 * c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const vec4f w = *reinterpret_cast<const vec4f*>(image + (8 * j + rr) * kPitch + 4 * c);
        if (4 * c < cols) *reinterpret_cast<vec4f*>(dst + (int64_t)(8 * j + rr) * ld) = w;
    }
    NFA_K33_WAVE_FENCE();
}

// the reverse: whole lines in, the accumulator layout out; zeros past `cols` (which may be <= 0)
__device__ __forceinline__ void load_tile(f32x16& a, const float* base, int64_t row0, int col0, int ld, int cols,
                                          float* image, int lane) {
    const int c = lane & 7, rr = lane >> 3;
    const float* src = base + row0 * ld + col0 + 4 * c;
    vec4f w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        w[j] = 4 * c < cols ? *reinterpret_cast<const vec4f*>(src + (int64_t)(8 * j + rr) * ld) : vec4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<vec4f*>(image + (8 * j + rr) * kPitch + 4 * c) = w[j];
    NFA_K33_WAVE_FENCE();
    const float* mine = image + (lane & 31) * kPitch + 4 * (lane >> 5);
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const vec4f v = *reinterpret_cast<const vec4f*>(mine + 8 * q4);
        a[4 * q4] = v.x;
        a[4 * q4 + 1] = v.y;
        a[4 * q4 + 2] = v.z;
        a[4 * q4 + 3] = v.w;
    }
    NFA_K33_WAVE_FENCE();
}

// the ReLU mask of a saved tile, bit q = value > 0 (NaN: 0, as threshold_backward's `output > 0`)
__device__ __forceinline__ unsigned load_mask(const float* base, int64_t row0, int col0, int ld, float* image, int lane) {
    f32x16 v;
    load_tile(v, base, row0, col0, ld, 32, image, lane);
    unsigned bits = 0u;
#pragma unroll
    for (int q = 0; q < 16; ++q) bits |= (v[q] > 0.0f ? 1u : 0u) << q;
    return bits;
}

__device__ __forceinline__ void apply_mask(f32x16& acc, unsigned m) {
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = ((m >> q) & 1u) ? acc[q] : 0.0f;
}

__device__ __forceinline__ void zero_tiles(f32x16 (&acc)[2]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[0][q] = acc[1][q] = 0.0f;
}

__global__ void __launch_bounds__(kThreads, 1) resnet_wide_forward_kernel(const WideTrainArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uvec4* X = reinterpret_cast<uvec4*>(lds_dyn);
    float* image = lds_dyn + kXSteps * kStepVec4 * 4 + wave * kImageFloats;
    const uvec4* xl = X + lane;
    const int nks = a.nks, tiles = a.tiles, nb = a.nb, Hp = tiles * 32, di = a.di;
    const int64_t plane = a.batch * Hp;

    // where this wave's fragments live: initial [tiles][init_ks], 2 nb x [tiles][nks], final [ftiles][nks]
    const bool active = wave < tiles;            // owns a column tile of the hidden GEMMs
    const bool has_final = wave < a.ftiles;      // final tiles wave, wave + 8, ...
    const size_t hidden_vec4 = (size_t)tiles * nks * kFragVec4;
    const vec4f* w_init = a.w + (size_t)(active ? wave : 0) * a.init_ks * kFragVec4 + lane;
    const vec4f* w_hidden = a.w + (size_t)tiles * a.init_ks * kFragVec4 + (size_t)(active ? wave : 0) * nks * kFragVec4 + lane;
    const vec4f* w_final = a.w + (size_t)tiles * a.init_ks * kFragVec4 + 2 * nb * hidden_vec4 + lane;
    // the wave's first GEMM of a row block, and the one behind its last hidden GEMM (a wave without a GEMM prefetches
    // fragments it never uses)
    const vec4f* w_first = active ? w_init : has_final ? w_final + (size_t)wave * nks * kFragVec4 : w_init;
    const vec4f* w_behind_hidden = has_final ? w_final + (size_t)wave * nks * kFragVec4 : w_first;
    const float* fbias = a.bias + (size_t)(1 + 2 * nb) * Hp;

    Frag f0 = load_frag(w_first), f1 = load_frag(w_first + kFragVec4);

    const int64_t num_blocks64 = a.batch >> 6;
    for (int64_t blk = blockIdx.x; blk < num_blocks64; blk += gridDim.x) {
        const int64_t row0 = blk << 6;
        int lane_here = lane;
        asm volatile("" : "+v"(lane_here));
        const int half = lane_here >> 5, r = lane_here & 31;
        // ---- x -> pieces, the initial Linear's B operand: thread (k-step, row tile, lane) splits the eight values
        //      k = 16 ks + 8 half + j of row 32 rt + r (zeros past d_i)
        NFA_K32_BARRIER();   // (the previous row block's final tiles have read the buffer)
        if (tid < a.init_ks * 2 * kWave) {
            const int ks = wave >> 1, rt = wave & 1, k0 = ks * 16 + half * 8;
            const float* xr = a.x + (row0 + rt * 32 + r) * di + k0;
            const vec4f zero = {0.0f, 0.0f, 0.0f, 0.0f};
            const vec4f v0 = k0 < di ? *reinterpret_cast<const vec4f*>(xr) : zero;
            const vec4f v1 = k0 + 4 < di ? *reinterpret_cast<const vec4f*>(xr + 4) : zero;
            bf16x2 hh[4], mm[4], ll[4];
            split3(vec2f{v0.x, v0.y}, hh[0], mm[0], ll[0]);
            split3(vec2f{v0.z, v0.w}, hh[1], mm[1], ll[1]);
            split3(vec2f{v1.x, v1.y}, hh[2], mm[2], ll[2]);
            split3(vec2f{v1.z, v1.w}, hh[3], mm[3], ll[3]);
            uvec4* p = X + ks * kStepVec4 + rt * 3 * kWave + lane_here;
            p[0 * kWave] = __builtin_bit_cast(uvec4, join4(hh[0], hh[1], hh[2], hh[3]));
            p[1 * kWave] = __builtin_bit_cast(uvec4, join4(mm[0], mm[1], mm[2], mm[3]));
            p[2 * kWave] = __builtin_bit_cast(uvec4, join4(ll[0], ll[1], ll[2], ll[3]));
        }
        NFA_K32_BARRIER();

        f32x16 h[2];   // the wave's slice of the residual stream: columns 32 w .. 32 w + 31 of both row tiles, fp32
        // ---- initial Linear: h = W_in x + b_in
        if (active) {
            load_bias_tile(h[0], a.bias + wave * 32 + half * 16);
            h[1] = h[0];
            gemm_exchange(h, w_init, nb > 0 ? w_hidden : w_behind_hidden, a.init_ks, f0, f1, xl);
        }
        // ---- residual blocks: a = W_0 relu(h) + b_0;  h += W_1 relu(a) + b_1
        for (int b = 0; b < nb; ++b) {
            const float* bias = a.bias + (size_t)(1 + 2 * b) * Hp + wave * 32 + half * 16;
            const vec4f* w0 = w_hidden + (size_t)(2 * b) * hidden_vec4;
            float* in0 = a.saved + (2 * b) * plane;
            float* in1 = in0 + plane;
            f32x16 u[2];
            NFA_K32_BARRIER();
            if (active) {
                exchange_store<kActRelu>(h, X, wave, lane_here);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) store_tile<true>(in0, row0 + rt * 32, wave * 32, Hp, 32, h[rt], image, lane_here);
            }
            NFA_K32_BARRIER();
            if (active) {
                load_bias_tile(u[0], bias);
                u[1] = u[0];
                gemm_exchange(u, w0, w0 + hidden_vec4, nks, f0, f1, xl);
            }
            NFA_K32_BARRIER();
            if (active) {
                exchange_store<kActRelu>(u, X, wave, lane_here);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) store_tile<true>(in1, row0 + rt * 32, wave * 32, Hp, 32, u[rt], image, lane_here);
            }
            NFA_K32_BARRIER();
            if (active) {
                // the second Linear sums into accumulators of its own and joins the stream with one addition
                f32x16 v[2], b1;
                zero_tiles(v);
                gemm_exchange(v, w0 + hidden_vec4, b + 1 < nb ? w0 + 2 * hidden_vec4 : w_behind_hidden, nks, f0, f1, xl);
                load_bias_tile(b1, bias + Hp);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    h[0][q] += v[0][q] + b1[q];
                    h[1][q] += v[1][q] + b1[q];
                }
            }
        }
        if (active) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) store_tile<false>(a.hidden, row0 + rt * 32, wave * 32, Hp, 32, h[rt], image, lane_here);
        }
        // ---- the final Linear: params = W_f h + b_f, its 32-column tiles dealt over the eight waves, h as pieces from
        //      the exchange buffer
        if (a.ftiles > 0) {
            NFA_K32_BARRIER();
            if (active) exchange_store<kActNone>(h, X, wave, lane_here);
            NFA_K32_BARRIER();
            for (int t = wave; t < a.ftiles; t += kWaves) {
                const vec4f* wl = w_final + (size_t)t * nks * kFragVec4;
                f32x16 acc[2];
                load_bias_tile(acc[0], fbias + t * 32 + half * 16);
                acc[1] = acc[0];
                gemm_exchange(acc, wl, t + kWaves < a.ftiles ? wl + (size_t)kWaves * nks * kFragVec4 : w_first, nks, f0, f1, xl);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
                    store_tile<false>(a.params, row0 + rt * 32, 32 * t, a.out, a.out - 32 * t, acc[rt], image, lane_here);
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads, 1) resnet_wide_backward_kernel(const WideTrainArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uvec4* X = reinterpret_cast<uvec4*>(lds_dyn);
    float* image = lds_dyn + kXSteps * kStepVec4 * 4 + wave * kImageFloats;
    const uvec4* xl = X + lane;
    const int nks = a.nks, tiles = a.tiles, nb = a.nb, Hp = tiles * 32, di = a.di, fks = a.fks, out = a.out;
    const int64_t plane = a.batch * Hp;

    // the backward stream: W_f^T [tiles][fks], per block from the last to the first W_1^T, W_0^T [tiles][nks], W_in^T
    // [ceil(d_i / 32)][nks]
    const bool active = wave < tiles;
    const bool does_x = wave < ((di + 31) >> 5);   // (at most two tiles: waves 0 and 1, always active)
    const size_t hidden_vec4 = (size_t)tiles * nks * kFragVec4;
    const vec4f* w_f = a.w + (size_t)(active ? wave : 0) * fks * kFragVec4 + lane;
    const vec4f* w_hid = a.w + (size_t)tiles * fks * kFragVec4 + (size_t)(active ? wave : 0) * nks * kFragVec4 + lane;
    const vec4f* w_x = a.w + (size_t)tiles * fks * kFragVec4 + 2 * nb * hidden_vec4 + (size_t)(does_x ? wave : 0) * nks * kFragVec4 + lane;
    const vec4f* w_first = fks > 0 ? w_f : nb > 0 ? w_hid : w_x;
    const vec4f* w_behind_hidden = does_x ? w_x : w_first;
    const vec4f* w_behind_final = nb > 0 ? w_hid : w_behind_hidden;

    Frag f0 = load_frag(w_first), f1 = load_frag(w_first + kFragVec4);

    const int64_t num_blocks64 = a.batch >> 6;
    for (int64_t blk = blockIdx.x; blk < num_blocks64; blk += gridDim.x) {
        const int64_t row0 = blk << 6;
        int lane_here = lane;
        asm volatile("" : "+v"(lane_here));
        f32x16 g[2];   // g_h: the gradient of the wave's slice of the residual stream
        if (fks > 0) {
            // ---- g_h = W_f^T g_params, `out` walked in chunks of at most 16 k-steps (256 columns): wave w brings columns
            //      32 w .. of the chunk (zeros past `out`) as pieces, the active waves multiply
            zero_tiles(g);
            for (int c0 = 0; c0 < fks; c0 += kXSteps) {
                const int cks = fks - c0 < kXSteps ? fks - c0 : kXSteps;
                const bool feeds = 2 * wave < cks;
                const int col0 = c0 * 16 + wave * 32;
                f32x16 gp[2];
                if (feeds) {
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) load_tile(gp[rt], a.gparams, row0 + rt * 32, col0, out, out - col0, image, lane_here);
                }
                NFA_K32_BARRIER();
                if (feeds) exchange_store<kActNone>(gp, X, wave, lane_here);
                NFA_K32_BARRIER();
                if (active) {
                    // a chunk sums into accumulators of its own and joins g_h with one addition: accumulated in place, every
                    // one of `out` / 16 x 6 MFMAs rounds at the size of the whole sum (2.1 x the fp32 chain's error at out = 736)
                    f32x16 part[2];
                    zero_tiles(part);
                    gemm_exchange(part, w_f + (size_t)c0 * kFragVec4, c0 + kXSteps < fks ? w_f + (size_t)(c0 + kXSteps) * kFragVec4 : w_behind_final,
                                  cks, f0, f1, xl);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        g[0][q] += part[0][q];
                        g[1][q] += part[1][q];
                    }
                }
            }
            if (active) {   // K10's grad_outputs of the last block's second Linear
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) store_tile<false>(a.hidden, row0 + rt * 32, wave * 32, Hp, 32, g[rt], image, lane_here);
            }
        } else if (active) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) load_tile(g[rt], a.x, row0 + rt * 32, wave * 32, Hp, 32, image, lane_here);
        }
        // ---- blocks, last to first: g_a = (W_1^T g_h) . [a > 0];  g_h += (W_0^T g_a) . [h > 0]
        for (int b = nb - 1; b >= 0; --b) {
            const vec4f* w1 = w_hid + (size_t)(2 * (nb - 1 - b)) * hidden_vec4;
            const float* s0 = a.saved + (2 * b) * plane;
            float* ga = a.grads + (2 * b + 1) * plane;
            float* gh = a.grads + (2 * b) * plane;
            unsigned m[2] = {0u, 0u};
            f32x16 u[2];
            if (active) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) m[rt] = load_mask(s0 + plane, row0 + rt * 32, wave * 32, Hp, image, lane_here);
            }
            NFA_K32_BARRIER();
            if (active) exchange_store<kActNone>(g, X, wave, lane_here);
            NFA_K32_BARRIER();
            if (active) {
                zero_tiles(u);
                gemm_exchange(u, w1, w1 + hidden_vec4, nks, f0, f1, xl);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    apply_mask(u[rt], m[rt]);
                    store_tile<false>(ga, row0 + rt * 32, wave * 32, Hp, 32, u[rt], image, lane_here);
                    m[rt] = load_mask(s0, row0 + rt * 32, wave * 32, Hp, image, lane_here);
                }
            }
            NFA_K32_BARRIER();
            if (active) exchange_store<kActNone>(u, X, wave, lane_here);
            NFA_K32_BARRIER();
            if (active) {
                // the product in accumulators of its own, masked, then ONE addition into the stream's gradient
                f32x16 v[2];
                zero_tiles(v);
                gemm_exchange(v, w1 + hidden_vec4, b > 0 ? w1 + 2 * hidden_vec4 : w_behind_hidden, nks, f0, f1, xl);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    apply_mask(v[rt], m[rt]);
#pragma unroll
                    for (int q = 0; q < 16; ++q) g[rt][q] += v[rt][q];
                    store_tile<false>(gh, row0 + rt * 32, wave * 32, Hp, 32, g[rt], image, lane_here);
                }
            }
        }
        // ---- initial Linear: g_x = W_in^T g_h_0, output tile t on wave t
        NFA_K32_BARRIER();
        if (active) exchange_store<kActNone>(g, X, wave, lane_here);
        NFA_K32_BARRIER();
        if (does_x) {
            f32x16 acc[2];
            zero_tiles(acc);
            gemm_exchange(acc, w_x, w_first, nks, f0, f1, xl);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) store_tile<false>(a.gx, row0 + rt * 32, 32 * wave, di, di - 32 * wave, acc[rt], image, lane_here);
        }
        // (the next row block writes the buffer behind its first barrier)
    }
}

// ---- the packer: fp32 parameters -> both fragment streams and the biases, one launch per training step.  One wave per
//      fragment (column tile, k-step) of one of at most 16 matrices; the last workgroup writes the biases.
constexpr int kPackMats = 16, kPackBlock = 256;

struct PackMat {
    const float* src;   // [rows][cols], contiguous
    bf16x8* dst;        // [tiles][nks][piece][lane]
    int rows, cols;
    int transpose;      // A = src^T
    int acc_order;      // k-step ks, lane-half hf, element j reads column acc_col(ks, hf, j) (ops._k8_column_order over all
                        // columns) instead of 16 ks + 8 hf + j
    int tiles, nks;
};

struct PackArgs {
    PackMat m[kPackMats];
    int first[kPackMats + 1];   // first fragment of matrix q in the launch
    int n;
    const float* hidden_bias[7];   // b_in, (b_0, b_1) per block
    const float* b_f;
    float* bias;                   // [Hp (1 + 2 nb)] then [32 ftiles]
    int H, Hp, nb, out, ftiles;
};

__global__ void __launch_bounds__(kPackBlock) pack_resnet_wide_kernel(const PackArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    if ((int)blockIdx.x * (kPackBlock / kWave) >= a.first[a.n]) {   // biases: [tile][half][q] = b[32 tile + 8 (q / 4) + 4 half + q % 4]
        const int hidden_n = a.Hp * (1 + 2 * a.nb);
        for (int e = tid; e < hidden_n + 32 * a.ftiles; e += kPackBlock) {
            const bool fin = e >= hidden_n;
            const int v = fin ? 0 : e / a.Hp, rem = fin ? e - hidden_n : e - v * a.Hp;
            const int tile = rem >> 5, half = (rem >> 4) & 1, q = rem & 15;
            const int src = 32 * tile + 8 * (q >> 2) + 4 * half + (q & 3);
            a.bias[e] = fin ? (src < a.out ? a.b_f[src] : 0.0f) : (src < a.H ? a.hidden_bias[v][src] : 0.0f);
        }
        return;
    }
    const int frag = blockIdx.x * (kPackBlock / kWave) + (tid >> 6);
    if (frag >= a.first[a.n]) return;
    int q = 0;
    while (frag >= a.first[q + 1]) ++q;
    const PackMat& mt = a.m[q];
    const int local = frag - a.first[q], tile = local / mt.nks, ks = local - tile * mt.nks;
    const int hf = lane >> 5, row = 32 * tile + (lane & 31);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = mt.acc_order ? 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * hf + (j & 3) : 16 * ks + 8 * hf + j;
        const int sr = mt.transpose ? col : row, sc = mt.transpose ? row : col;
        v[j] = (sr < mt.rows && sc < mt.cols) ? mt.src[(size_t)sr * mt.cols + sc] : 0.0f;
    }
    bf16x2 hh[4], mm[4], ll[4];
#pragma unroll
    for (int j2 = 0; j2 < 4; ++j2) split3(vec2f{v[2 * j2], v[2 * j2 + 1]}, hh[j2], mm[j2], ll[j2]);
    bf16x8* dst = mt.dst + (size_t)local * 3 * kWave + lane;
    dst[0 * kWave] = join4(hh[0], hh[1], hh[2], hh[3]);
    dst[1 * kWave] = join4(mm[0], mm[1], mm[2], mm[3]);
    dst[2 * kWave] = join4(ll[0], ll[1], ll[2], ll[3]);
}

static int check_wide_train(int64_t batch, int32_t num_identity, int32_t hidden_features, int32_t num_blocks,
                            int32_t out_features) {
    if (batch < 0 || num_identity < 1 || num_blocks < 0 || hidden_features < 1 || out_features < 0)
        return NFA_ERR_INVALID_ARGUMENT;
    if (hidden_features < 129 || hidden_features > 256 || num_identity > 64 || (num_identity & 3) != 0 ||
        (batch & 63) != 0 || num_blocks > 3 || (out_features & 3) != 0 || out_features > 32 * 1024)
        return NFA_ERR_UNSUPPORTED;
    return NFA_OK;
}

static void set_shape(WideTrainArgs& a, int64_t batch, int32_t num_identity, int32_t hidden_features, int32_t num_blocks,
                      int32_t out_features) {
    a.batch = batch;
    a.di = num_identity;
    a.nb = num_blocks;
    a.tiles = (hidden_features + 31) / 32;
    a.nks = 2 * a.tiles;
    a.init_ks = num_identity > 32 ? 4 : 2;
    a.out = out_features;
    a.ftiles = (out_features + 31) / 32;
    a.fks = 2 * a.ftiles;
}

static dim3 wide_grid(int64_t batch) {
    int64_t blocks = batch >> 6;
    if (blocks > device_cu_count()) blocks = device_cu_count();
    return dim3((unsigned)blocks);
}

}  // namespace k33
}  // namespace nfa

using namespace nfa;
using namespace nfa::k33;

extern "C" int nfa_resnet_wide_forward_f32(const float* identity_inputs, const void* fragments, const float* bias_packed,
                                           float* saved, float* hidden, float* params, int32_t out_features,
                                           int64_t batch, int32_t num_identity, int32_t hidden_features,
                                           int32_t num_blocks, void* stream) {
    const int rc = check_wide_train(batch, num_identity, hidden_features, num_blocks, out_features);
    if (rc != NFA_OK) return rc;
    if (batch == 0) return NFA_OK;
    if (!identity_inputs || !fragments || !bias_packed || !hidden || (num_blocks > 0 && !saved) || (out_features > 0 && !params))
        return NFA_ERR_INVALID_ARGUMENT;
    WideTrainArgs a = {};
    set_shape(a, batch, num_identity, hidden_features, num_blocks, out_features);
    a.x = identity_inputs;
    a.w = reinterpret_cast<const vec4f*>(fragments);
    a.bias = bias_packed;
    a.saved = saved;
    a.hidden = hidden;
    a.params = params;
    return launch_kernel(resnet_wide_forward_kernel, wide_grid(batch), dim3(kThreads), kLdsBytes, (hipStream_t)stream, a);
}

extern "C" int nfa_resnet_wide_backward_f32(const float* grad_hidden, const float* grad_params, int32_t out_features,
                                            const void* fragments, const float* saved, float* grads,
                                            float* grad_hidden_out, float* grad_identity_inputs, int64_t batch,
                                            int32_t num_identity, int32_t hidden_features, int32_t num_blocks,
                                            void* stream) {
    const int rc = check_wide_train(batch, num_identity, hidden_features, num_blocks, out_features);
    if (rc != NFA_OK) return rc;
    if (batch == 0) return NFA_OK;
    // exactly one incoming gradient: g_params with the final Linear's width, or g_hidden
    if ((grad_hidden != nullptr) == (grad_params != nullptr) || (grad_params != nullptr) != (out_features > 0) ||
        (grad_params && !grad_hidden_out) || !fragments || !grad_identity_inputs || (num_blocks > 0 && (!saved || !grads)))
        return NFA_ERR_INVALID_ARGUMENT;
    WideTrainArgs a = {};
    set_shape(a, batch, num_identity, hidden_features, num_blocks, out_features);
    a.x = grad_hidden;
    a.w = reinterpret_cast<const vec4f*>(fragments);
    a.saved = const_cast<float*>(saved);
    a.hidden = grad_hidden_out;
    a.gparams = grad_params;
    a.grads = grads;
    a.gx = grad_identity_inputs;
    return launch_kernel(resnet_wide_backward_kernel, wide_grid(batch), dim3(kThreads), kLdsBytes, (hipStream_t)stream, a);
}

extern "C" int nfa_pack_resnet_wide_train_f32(const float* initial_weight, const float* initial_bias,
                                              const float* const* block_params, const float* final_weight,
                                              const float* final_bias, int32_t out_features, int32_t src_identity,
                                              int32_t num_identity, int32_t hidden_features, int32_t num_blocks,
                                              void* forward_fragments, float* bias_packed, void* backward_fragments,
                                              void* stream) {
    const int rc = check_wide_train(0, num_identity, hidden_features, num_blocks, out_features);
    if (rc != NFA_OK) return rc;
    if (src_identity < 1 || src_identity > num_identity) return NFA_ERR_INVALID_ARGUMENT;
    if (!initial_weight || !initial_bias || !forward_fragments || !bias_packed || !backward_fragments ||
        (num_blocks > 0 && !block_params) || (out_features > 0 && (!final_weight || !final_bias)))
        return NFA_ERR_INVALID_ARGUMENT;
    for (int q = 0; q < 4 * num_blocks; ++q)
        if (!block_params[q]) return NFA_ERR_INVALID_ARGUMENT;
    WideTrainArgs s = {};
    set_shape(s, 0, num_identity, hidden_features, num_blocks, out_features);
    const int H = hidden_features, nb = num_blocks;
    PackArgs a = {};
    a.first[0] = 0;
    bf16x8* fwd = reinterpret_cast<bf16x8*>(forward_fragments);
    bf16x8* bwd = reinterpret_cast<bf16x8*>(backward_fragments);
    auto add = [&a](bf16x8*& dst, const float* src, int rows, int cols, int transpose, int acc_order, int tiles, int nks) {
        a.m[a.n] = PackMat{src, dst, rows, cols, transpose, acc_order, tiles, nks};
        a.first[a.n + 1] = a.first[a.n] + tiles * nks;
        dst += (size_t)tiles * nks * 3 * kWave;
        ++a.n;
    };
    // forward: W_in, (W_0, W_1) per block, W_f
    add(fwd, initial_weight, H, src_identity, 0, 0, s.tiles, s.init_ks);
    for (int k = 0; k < nb; ++k) {
        add(fwd, block_params[4 * k], H, H, 0, 1, s.tiles, s.nks);
        add(fwd, block_params[4 * k + 2], H, H, 0, 1, s.tiles, s.nks);
    }
    if (out_features > 0) add(fwd, final_weight, out_features, H, 0, 1, s.ftiles, s.nks);
    // backward: W_f^T, (W_1^T, W_0^T) per block from the last to the first, W_in^T
    if (out_features > 0) add(bwd, final_weight, out_features, H, 1, 1, s.tiles, s.fks);
    for (int k = nb - 1; k >= 0; --k) {
        add(bwd, block_params[4 * k + 2], H, H, 1, 1, s.tiles, s.nks);
        add(bwd, block_params[4 * k], H, H, 1, 1, s.tiles, s.nks);
    }
    add(bwd, initial_weight, H, src_identity, 1, 1, (num_identity + 31) / 32, s.nks);
    a.hidden_bias[0] = initial_bias;
    for (int k = 0; k < nb; ++k) {
        a.hidden_bias[1 + 2 * k] = block_params[4 * k + 1];
        a.hidden_bias[2 + 2 * k] = block_params[4 * k + 3];
    }
    a.b_f = final_bias;
    a.bias = bias_packed;
    a.H = H;
    a.Hp = s.tiles * 32;
    a.nb = nb;
    a.out = out_features;
    a.ftiles = s.ftiles;
    const int per_block = kPackBlock / kWave;
    const int blocks = (a.first[a.n] + per_block - 1) / per_block + 1;
    return launch_kernel(pack_resnet_wide_kernel, dim3(blocks), dim3(kPackBlock), 0, (hipStream_t)stream, a, 0, false);
}
