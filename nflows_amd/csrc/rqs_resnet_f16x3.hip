// K8x (round 6): the whole-layer kernel -- ResidualNet conditioner, nn/nets/resnet.py:55-100 (forward :92-100, blocks
// :39-52), + everything K1 replaces, coupling.py:73-130, :549-582, for a RUN of layers in one launch -- with its GEMMs
// on the matrix pipe from THREE f16 pieces per fp32 operand (f16x3_gemm.hpp): operands carried at the reference's width
// (nn/nets/resnet.py:92-100 is F.linear on fp32: 24-bit significands; the three pieces hold 33).  Five cross products
// per multiply-add: hi hi, hi lo, lo hi on v_mfma_f32_32x32x16_f16; the two at the 2^-22 level, hi r and r hi, need
// two significant bits of each factor and run on ONE v_mfma_scale_f32_32x32x64_f8f6f4 (bf8 x bf8) per two k-steps --
// the activation's bf8 bytes are the HIGH BYTES of its f16 pieces (one v_perm_b32 per register), the weight's are
// packed by the host, the last pieces are kept x 2^8 and the instruction's e8m0 block scale takes the factor out:
// 4 instruction times per k-step against the three-piece bf16 kernel's 6 (K8, rqs_resnet.hip), whose structure this
// kernel keeps:
//
//   * a wave owns 32 rows for the whole run; the rows live in an LDS tile by slot, every GEMM is computed transposed
//     and chained through the register file (the accumulator tiles of one GEMM are the B operand of the next, up to
//     a column permutation the host applies to the weights);
//   * the residual stream stays in fp32, in the accumulators of the GEMM that made it (64 registers, at that GEMM's
//     power-of-two scale): each Linear splits the ReLU of its input accumulators into pieces one pair of k-steps at a
//     time (v_maximum3_f32 + the split), the skip connection is the second Linear's accumulator init, one fma per
//     value (v = bias + T h), and h is split once more only for the final layer;
//   * weights: 12 KB stages of twelve 1 KB fragments ([64 lanes] x 16 B) -- k-major: two k-steps of two output tiles,
//     [H0, L0, H1, L1, X lo, X hi] per tile; tile-major final layer: four k-steps of a tile, [H0, L0, H1, L1][H2, L2,
//     H3, L3][X01 lo, X01 hi, X23 lo, X23 hi] -- through the three-slot LDS-DMA ring of bf16x3_gemm.hpp (requested with buffer
//     loads: f16x3_gemm.hpp, request_stage), four waves per
//     workgroup, two workgroups per CU; fragments 0 .. 3 of every stage are read right behind the PREVIOUS stage's
//     barrier (f16x3_gemm.hpp: Lead), the barrier stands in front of a stage's last MFMAs;
//   * the wide form (8 bins, from two 128-row blocks per CU on: launch_f16x3): ONE workgroup of eight waves per CU on one
//     ring of three 24 KB slots, a slot = a pair of stages, one barrier per pair -- the CU moves every stage from L2
//     into LDS once, not once per workgroup (the narrow form's two rings move 64.5 GB per launch at the headline
//     shape); waves 0 .. 3 and 4 .. 7 run two consecutive row blocks with the narrow form's program: same bits;
//   * biases and tables: a layer's biases and the next layer's table are fetched a layer ahead into a bias area in LDS, as
//     LDS-DMA pieces issued in front of a stage's weight requests (rqs_resnet_f16x3_kernel.hpp: bias_area_piece) -- the
//     layer loop holds no per-lane global load and no vmcnt(0);
//   * the final layer is tile-major with the spline evaluation (rqs_fused8.hpp: one walk over fp32 running knot
//     sums, logits read at scale 1 / kappa straight from the accumulators) woven between its MFMAs: 32 time units per
//     tile (an f16 MFMA one, a bf8 MFMA two).
//
// What f16 pieces need that bf16 pieces did not -- range.  Every GEMM's weights are multiplied by a power of two T
// before the split (host: max |w T| in [2^13, 2^14)), activations -- the row tile's identity features included -- are
// split at scale S (a power of two, host: 16): a value keeps all its 24 bits while |v S| >= 2^-9 (the last piece,
// kept x 2^8, then is >= 2^-24, f16's smallest subnormal), below that the absolute error is <= 2^-33 / S; |v S| >=
// 65520 overflows.  Accumulators hold S T x (the reference's pre-activation); `scales` = per GEMM {1 / T, T}: 1 / T
// takes an accumulator to the next pieces' scale (exact), T / T' takes the residual stream (at the scale S T' of the GEMM
// that made it) to the second Linear's accumulator scale; the final layer's pair is {kappa = 1 / (S T), S T} for the spline evaluation.  Overflow poisons
// (hi = inf, lo = -inf, r = NaN, and ReLU's v_maximum3_f32 keeps NaN): a row block with any non-finite result writes
// nothing and raises its entry of `redo`, the caller runs K8 (three bf16 pieces: full fp32 range) on the flagged
// blocks right behind (nfa_rqs_flow_resnet_redo_f32), as for K8h.
//
// Served: 2 .. 16, 20, 24 or 32 bins (8: the two-features-per-three-tiles final layer; the others K8h's general scheme:
// rqs_resnet_f16x3_bins_{a,b}.hip), linear tails, ReLU blocks, no context, hidden width 128 (narrower: zero-padded by
// the host), d_i <= 64, d_t % 4 == 0, d_t <= 64, D % 4 == 0, D <= 128, batch % 128 == 0.  DBG instances (tests, 8
// bins): the logits of the run's LAST layer (accumulators x kappa) are stored as well.

#include "rqs_resnet_f16x3_kernel.hpp"

using namespace nfa;

// The instance of a launch: 8 bins (the diagnostic instances beside), the other bin counts in their own translation units.
static k8x::KernelFn f16x3_kernel(bool inverse, int init_ks, int K, bool dbg, bool bias_lds) {
    if (K != 8) {
        const k8x::KernelFn kern = k8x::bins_kernel_a(K, inverse, init_ks, bias_lds);
        return kern ? kern : k8x::bins_kernel_b(K, inverse, init_ks, bias_lds);
    }
    if (!bias_lds) {
        if (init_ks == 4)
            return dbg ? (inverse ? k8x::rqs_resnet_f16x3_global_bias_kernel<true, 4, true> : k8x::rqs_resnet_f16x3_global_bias_kernel<false, 4, true>)
                       : (inverse ? k8x::rqs_resnet_f16x3_global_bias_kernel<true, 4> : k8x::rqs_resnet_f16x3_global_bias_kernel<false, 4>);
        return dbg ? (inverse ? k8x::rqs_resnet_f16x3_global_bias_kernel<true, 2, true> : k8x::rqs_resnet_f16x3_global_bias_kernel<false, 2, true>)
                   : (inverse ? k8x::rqs_resnet_f16x3_global_bias_kernel<true, 2> : k8x::rqs_resnet_f16x3_global_bias_kernel<false, 2>);
    }
    if (init_ks == 4)
        return dbg ? (inverse ? k8x::rqs_resnet_f16x3_kernel<true, 4, true> : k8x::rqs_resnet_f16x3_kernel<false, 4, true>)
                   : (inverse ? k8x::rqs_resnet_f16x3_kernel<true, 4> : k8x::rqs_resnet_f16x3_kernel<false, 4>);
    return dbg ? (inverse ? k8x::rqs_resnet_f16x3_kernel<true, 2, true> : k8x::rqs_resnet_f16x3_kernel<false, 2, true>)
               : (inverse ? k8x::rqs_resnet_f16x3_kernel<true, 2> : k8x::rqs_resnet_f16x3_kernel<false, 2>);
}

// The wide form's instance (rqs_resnet_f16x3_kernel.hpp: one eight-wave workgroup per CU on one ring): 8 bins, bias area
static k8x::KernelFn f16x3_wide_kernel(bool inverse, int init_ks) {
    if (init_ks == 4) return inverse ? k8x::rqs_resnet_f16x3_kernel_wide<true, 4> : k8x::rqs_resnet_f16x3_kernel_wide<false, 4>;
    return inverse ? k8x::rqs_resnet_f16x3_kernel_wide<true, 2> : k8x::rqs_resnet_f16x3_kernel_wide<false, 2>;
}

static int launch_f16x3(const LayerCall& c, const float* scales, float act_scale, float* dbg_logits = nullptr) {
    // (a power of two: the pieces' scale must come out again exactly)
    int exponent = 0;
    if (!(act_scale > 0.0f) || frexpf(act_scale, &exponent) != 0.5f) return NFA_ERR_INVALID_ARGUMENT;
    k8x::Args a;
    int activation = 0;
    int rc = check_layer_call(c, {NFA_FLAG_ACTIVATION_MASK | NFA_FLAG_K8X_FORM_MASK, true, false, false}, &a.sp, &activation);
    if (rc != NFA_OK) return rc;
    const int form = (c.flags & NFA_FLAG_K8X_FORM_MASK) >> NFA_FLAG_K8X_FORM_SHIFT;
    if (form > NFA_K8X_FORM_WIDE) return NFA_ERR_INVALID_ARGUMENT;
    if (activation != NFA_ACTIVATION_RELU || (dbg_logits && a.sp.K != 8)) return NFA_ERR_UNSUPPORTED;
    if (c.batch == 0) return NFA_OK;
    if (!layer_buffers_given(c) || !c.bias || !scales || !c.redo) return NFA_ERR_INVALID_ARGUMENT;
    rc = fill_layer_args(a, c);
    if (rc != NFA_OK) return rc;
    a.act_scale = act_scale;
    a.bias = c.bias;
    a.scales = scales;
    a.tables = c.tables;
    a.redo = c.redo;
    a.dbg_logits = dbg_logits;
    const int init_ks = c.num_identity > 32 ? 4 : 2;
    const int rows_per_feature = spline_rows_per_feature(a.sp.K);
    a.num_stages = init_ks + 16 * c.num_blocks + 2 * (c.num_transform * rows_per_feature / 32);
    a.bias_per_layer = 128 + 256 * c.num_blocks + c.num_transform * rows_per_feature;
    // dynamic LDS: ring, row tiles, then the bias area (a layer's hidden and final biases, the next layer's raw table) --
    // or, where that area would take the launch from two workgroups per CU to one, the final layer's biases alone and the
    // instance that reads the hidden ones from global memory.  (The diagnostic instances take the area whenever it fits the launch.)
    const size_t lds_rows = (size_t)kRing * kStageVec4 * 16 + (size_t)(kBlock / kWave) * c.features * kRowPad * sizeof(float);
    const int final_floats = c.num_transform * rows_per_feature;
    const size_t lds_area = lds_rows + (size_t)k8x::bias_area_floats(c.num_blocks, final_floats) * sizeof(float);
    const size_t lds_plain = lds_rows + (size_t)final_floats * sizeof(float);
    const size_t two_per_cu = 80 * 1024 - 2048;
    // (and the area must fit the launch at all: 64 blocks at D = 128 do not)
    const size_t launch_limit = kCuLds - 2048;
    const bool bias_lds = lds_area <= launch_limit && (dbg_logits || lds_area <= two_per_cu || lds_plain > two_per_cu);
    const size_t lds = bias_lds ? lds_area : lds_plain;
    int64_t blocks = c.batch >> 7;
    const bool inv = (c.flags & NFA_FLAG_INVERSE) != 0;
    // The wide form: where an instance exists (8 bins, no diagnostics), its LDS -- a ring of twice the size, eight row tiles,
    // the bias area -- fits the launch, and every CU gets at least two row blocks (below that the narrow form keeps all CUs
    // busy and the wide form would halve them).  NFA_FLAG_K8X_FORM forces either form where the first two hold.
    const size_t lds_wide = 2 * lds_rows + (size_t)k8x::bias_area_floats(c.num_blocks, final_floats) * sizeof(float);
    const bool wide_fits = a.sp.K == 8 && !dbg_logits && lds_wide <= launch_limit;
    const bool wide = wide_fits && form != NFA_K8X_FORM_NARROW &&
                      (form == NFA_K8X_FORM_WIDE || blocks >= (int64_t)k8x::kWideBlocksPerCu * device_cu_count());
    if (wide) {
        int64_t grid = (blocks + 1) >> 1;
        if (grid > device_cu_count()) grid = device_cu_count();
        note_layer_kernel("k8x::rqs_resnet_f16x3_kernel<inverse=%d, init_ks=%d, K=%d, dbg=0, waves=8, bias=lds>", inv ? 1 : 0, init_ks,
                          a.sp.K);
        return launch_kernel(f16x3_wide_kernel(inv, init_ks), dim3((unsigned)grid), dim3(2 * kBlock), lds_wide, (hipStream_t)c.stream,
                             a, kCuLds - 2048);
    }
    const int64_t per_cu = lds <= two_per_cu ? 2 : 1;
    const int64_t cap = (int64_t)device_cu_count() * per_cu;
    if (blocks > cap) blocks = cap;
    const k8x::KernelFn kern = f16x3_kernel(inv, init_ks, a.sp.K, dbg_logits, bias_lds);
    if (!kern) return NFA_ERR_UNSUPPORTED;
    note_layer_kernel("k8x::rqs_resnet_f16x3_kernel<inverse=%d, init_ks=%d, K=%d, dbg=%d, bias=%s>", inv ? 1 : 0, init_ks, a.sp.K,
                      dbg_logits ? 1 : 0, bias_lds ? "lds" : "global");
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(kBlock), lds, (hipStream_t)c.stream, a, kCuLds - 2048);
}

extern "C" int nfa_rqs_flow_resnet_f16x3_f32(const float* inputs, const void* weights_packed, const float* bias_packed,
                                             const float* scales, const int32_t* flow_tables, int32_t num_layers,
                                             float* outputs, float* logabsdet, int32_t* redo_blocks, int32_t* status,
                                             int64_t batch, int32_t features, int32_t num_transform,
                                             int32_t num_identity, int32_t hidden_features, int32_t num_blocks,
                                             float act_scale, const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    return launch_f16x3({inputs, weights_packed, bias_packed, flow_tables, num_layers, outputs, logabsdet, redo_blocks,
                         status, batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags,
                         stream, nullptr, 0, 0},
                        scales, act_scale);
}

extern "C" int nfa_rqs_flow_resnet_f16x3_logits_f32(const float* inputs, const void* weights_packed,
                                                    const float* bias_packed, const float* scales,
                                                    const int32_t* flow_tables, int32_t num_layers, float* outputs,
                                                    float* logabsdet, int32_t* redo_blocks, int32_t* status,
                                                    int64_t batch, int32_t features, int32_t num_transform,
                                                    int32_t num_identity, int32_t hidden_features, int32_t num_blocks,
                                                    float act_scale, const nfa_rqs_spec* spec, int32_t flags,
                                                    void* stream, float* logits) {
    if (!logits) return NFA_ERR_INVALID_ARGUMENT;
    return launch_f16x3({inputs, weights_packed, bias_packed, flow_tables, num_layers, outputs, logabsdet, redo_blocks,
                         status, batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags,
                         stream, nullptr, 0, 0},
                        scales, act_scale, logits);
}
