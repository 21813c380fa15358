// K8h: the whole-layer kernel (ResidualNet conditioner, nn/nets/resnet.py:55-100, + everything K1
// replaces, coupling.py:73-130, :549-582, for a run of layers in one launch) with its GEMMs on the
// f16 matrix pipe from TWO pieces per fp32 operand.
//
//   x = hi + lo,  hi = RN16(x),  lo = RN16(x - hi)        |x - hi - lo| <= 2^-24 |x|
//   x * w ~= hi_x hi_w + hi_x lo_w + lo_x hi_w            dropped: lo_x lo_w <= 2^-24 |x w|
//
// Three v_mfma_f32_32x32x16_f16 per k-step and tile instead of the six bf16 products of the
// three-piece scheme (rqs_resnet.hip): half the matrix-pipe time, 4 bytes per weight instead of 6,
// a piece conversion of ~8 instead of 11+ VALU instructions per pair.  Measured on the GPU against
// float64 (tools/f16x2_probe.hip, K = 128): max 5.9e-7 / rms 5.2e-8 -- the figures of a sequential
// fp32 fma chain (5.2e-7 / 5.2e-8), better than the six-product bf16 scheme (6.6e-7 / 5.8e-8).
//
// What f16 needs that bf16 did not:
//   * range of the LOW pieces: a low piece below 2^-14 is subnormal (gfx950's f16 MFMA honours
//     subnormals, checked by the probe) and keeps only absolute precision 2^-25.  Weights are
//     therefore pre-scaled per GEMM by a power of two T (host: max |w T| in [2^13, 2^14)); the scale
//     comes back out when accumulators are converted to the next layer's pieces (a product with a
//     power of two: exact) or, for the final layer, inside the spline evaluation.  Activations stay
//     at scale S (1 by default): an activation below 0.25 / S carries an absolute error <= 2^-25 / S,
//     ~3e-8 absolute on a layer output (probe) -- invisible next to the fp32 rounding of the sum.
//   * range of the HIGH pieces: |activation| * S > 65504 overflows.  Every row block checks its
//     results: a block with any non-finite output writes nothing and raises its entries of `redo`;
//     the caller then runs the exact kernel (nfa_rqs_flow_resnet_redo_f32, three bf16 pieces: full
//     fp32 range) on the flagged blocks.  Overflow always poisons: an f16 infinity enters the
//     products, its low piece is x - inf = -inf, and inf - inf = NaN reaches every logit that depends
//     on it.  Rows with NaN / inf INPUTS take the same route (the reference's propagation rules).
//
// Structure (32 samples per wave, rows in an LDS tile by slot, GEMMs transposed and chained through
// the register file as in rqs_resnet.hip), and what is different here:
//   * ONE stream of 16 KB stages per layer feeds everything through LDS-DMA: first the layer's
//     PARAMETER stage(s) -- column tables, per-GEMM headers {out_scale, skip_scale}, all biases --
//     then the weights.  Inside the layer loop a wave issues no global load other than its LDS-DMA
//     requests: a `s_waitcnt vmcnt(n)` of the compiler for an ordinary load counts on in-order
//     return, which LDS-DMA requests sharing the counter do not give it.  (The stream is drained
//     before the ordinary loads / stores at the two ends of a row block.)
//   * The ring is deep (four 16 KB slots, three stages in flight) and shared by EIGHT waves (one workgroup
//     per CU) where the batch allows: a request lands 1-2 us after it was issued, so bytes per
//     second = bytes in flight / latency; eight waves per stream also halve the bytes per CU.
//   * Weight fragments are read from LDS one MFMA group ahead by asm reads with a counted lgkmcnt
//     (hipcc waits with lgkmcnt(0), i.e. also for the reads just issued for the next group).
//   * The final layer is tile-major (a 32-row output tile = 24 MFMAs = two stages) with the spline
//     evaluation woven between its MFMAs, one slice behind each MFMA (~5 independent VALU
//     instructions behind an MFMA are free, tools/weave_probe.hip); the hidden Linears are k-major
//     (four accumulators, every input piece read once).
//   * The residual stream h lives in fp32 accumulator registers across a block (hacc): the block's
//     second Linear accumulates straight into it (skip connection = one fma per value when the
//     accumulator is prepared), ReLU is applied when a tile is converted into pieces, not per k-step.
//   * No packed fp32 arithmetic (see split2).
//
// Restrictions: 2 .. 16, 20, 24 or 32 bins (8 and 10: tuned final-layer loops and conditioners with a context), linear tails, hidden width 128 (narrower: zero-padded by the host), ReLU
// blocks, d_i <= 64, d_t % 4 == 0, d_t <= 64, D % 4 == 0, D <= 128, batch % 128 == 0 (other feature counts
// and batches: padded by the host); with a context: up to 32 context features beside d_i <= 32.



#include "rqs_resnet_f16_kernel.hpp"

using namespace nfa;

template <int IKS, int NW, int KB, bool CTX = false, int RING = k8h::kRing>
static k8h::KernelFn f16_instance(bool inverse) {
    return inverse ? k8h::rqs_resnet_f16_kernel<true, IKS, NW, KB, CTX, RING> : k8h::rqs_resnet_f16_kernel<false, IKS, NW, KB, CTX, RING>;
}

// The instance of a launch, one ordered decision: the diagnostic instances, a context or an activation or a bin count
// beyond the tuned 8 / 10 bins with ReLU (their own translation units), then the tuned instances (the elastic stream
// of the experiment builds, a context: init_ks 4).
static k8h::KernelFn f16_kernel(bool inverse, int init_ks, int waves, int K, int activation, bool with_ctx, bool elastic,
                                bool dbg) {
    const bool tuned = (K == 8 || K == 10) && activation == NFA_ACTIVATION_RELU;
    if (dbg) return k8h::debug_kernel(inverse, init_ks, waves);
    if (with_ctx && !tuned) {   // (round 5: rqs_resnet_f16_ctx_{a,b}.hip)
        const k8h::KernelFn kern = k8h::context_kernel_a(K, activation, inverse, waves);
        return kern ? kern : k8h::context_kernel_b(K, activation, inverse, waves);
    }
    if (activation != NFA_ACTIVATION_RELU) return k8h::activation_kernel(activation, K, inverse, init_ks, waves);
    if (!tuned)
        return K <= 9 ? k8h::bins_kernel_a(K, inverse, init_ks, waves)
               : K <= 16 ? k8h::bins_kernel_b(K, inverse, init_ks, waves) : k8h::bins_kernel_c(K, inverse, init_ks, waves);
#ifdef NFA_K8H_ELASTIC   // (experiment builds only: measured 3 % slower than the rigid stream, profiles/r3/k8h_elastic_stream.txt)
    if (elastic)
        return init_ks == 4 ? f16_instance<4, 8, 8, false, k8h::kRingElastic>(inverse)
                            : f16_instance<2, 8, 8, false, k8h::kRingElastic>(inverse);
#else
    (void)elastic;
#endif
    const bool k10 = K == 10;
    if (with_ctx)
        return waves == 8 ? (k10 ? f16_instance<4, 8, 10, true>(inverse) : f16_instance<4, 8, 8, true>(inverse))
                          : (k10 ? f16_instance<4, 4, 10, true>(inverse) : f16_instance<4, 4, 8, true>(inverse));
    if (waves == 8)
        return init_ks == 4 ? (k10 ? f16_instance<4, 8, 10>(inverse) : f16_instance<4, 8, 8>(inverse))
                            : (k10 ? f16_instance<2, 8, 10>(inverse) : f16_instance<2, 8, 8>(inverse));
    return init_ks == 4 ? (k10 ? f16_instance<4, 4, 10>(inverse) : f16_instance<4, 4, 8>(inverse))
                        : (k10 ? f16_instance<2, 4, 10>(inverse) : f16_instance<2, 4, 8>(inverse));
}

static int launch_f16(const LayerCall& c, int32_t* dbg_bins = nullptr, float* dbg_logits = nullptr) {
    k8h::Args a;
    int activation = 0;
    int rc = check_layer_call(c, {NFA_FLAG_ACTIVATION_MASK, true, false, true}, &a.sp, &activation);
    if (rc != NFA_OK) return rc;
    // bin counts: 8 and 10 have their own final-layer loops; 2 .. 16 and 20, 24, 32 otherwise
    const bool any_bins = a.sp.K != 8 && a.sp.K != 10, with_ctx = c.context_features > 0;
    // activations other than ReLU: the two tuned bin counts (with or, round 5, without a context)
    if (activation != NFA_ACTIVATION_RELU && any_bins) return NFA_ERR_UNSUPPORTED;
    // with a context: two identity k-steps + two context k-steps in the initial layer
    if (with_ctx && (c.context_features > 32 || c.num_identity > 32)) return NFA_ERR_UNSUPPORTED;
    const int param_words = k8h::param_words(c, a.sp.K);
    if (!param_words) return NFA_ERR_INVALID_ARGUMENT;
    if (c.batch == 0) return NFA_OK;
    if (!layer_buffers_given(c) || !c.redo) return NFA_ERR_INVALID_ARGUMENT;
    // the diagnostic instances (nfa_rqs_flow_resnet_f16x2_bins_f32): the bench's kernel family only
    if (dbg_bins && (a.sp.K != 8 || with_ctx || activation != NFA_ACTIVATION_RELU)) return NFA_ERR_UNSUPPORTED;
    rc = k8h::fill_args(a, c, param_words, dbg_bins, dbg_logits);
    if (rc != NFA_OK) return rc;
    const int init_ks = (with_ctx || c.num_identity > 32) ? 4 : 2;
    a.num_stages = c.param_stages + init_ks / 2 + (with_ctx ? 9 : 8) * c.num_blocks +
                   c.num_transform * spline_rows_per_feature(a.sp.K) / 32;
    a.trace = g_k7_trace;
    // workgroups of eight waves (256 rows, one per CU, one weight stream per CU) when the batch gives
    // every CU one; otherwise four waves (128 rows)
    const int cus = device_cu_count();
    static const int force_nw = getenv("NFA_K8H_WAVES") ? atoi(getenv("NFA_K8H_WAVES")) : 0;
    static const int force_ring = getenv("NFA_K8H_RING") ? atoi(getenv("NFA_K8H_RING")) : 0;   // 5: elastic stream (experiment, slower)
    int nw = ((c.batch & 255) == 0 && (c.batch >> 8) >= cus) ? 8 : 4;
    if (force_nw == 4 || (force_nw == 8 && (c.batch & 255) == 0)) nw = force_nw;
    const size_t lds_static = 1024;   // s_final, s_bad, s_sync (rounded up)
    const size_t lds_cap = kCuLds - lds_static;
    auto lds_for = [&](int n, int ring) {
        return (size_t)ring * k8h::kStageVec4 * 16 + (size_t)n * c.features * k8h::kRowPad * sizeof(float) +
               (size_t)2 * ((param_words + 3) & ~3) * sizeof(float);
    };
    if (lds_for(nw, k8h::kRing) > lds_cap) nw = 4;
    if (lds_for(nw, k8h::kRing) > lds_cap) return NFA_ERR_UNSUPPORTED;
    // the elastic stream (five slots, counters instead of the per-stage barrier) where it fits: eight-wave
    // workgroups of the 8-bin kernel without a context (the bench's shape: 161 984 bytes at D = 64)
#ifdef NFA_K8H_ELASTIC
    const bool elastic = !dbg_bins && nw == 8 && !with_ctx && a.sp.K == 8 && force_ring == 5 && lds_for(8, k8h::kRingElastic) <= lds_cap;
#else
    const bool elastic = false;
    (void)force_ring;
#endif
    const size_t lds_launch = lds_for(nw, elastic ? k8h::kRingElastic : k8h::kRing);
    int64_t blocks = c.batch / (32 * nw);
    const int64_t per_cu = (nw == 4 && lds_launch + 2048 <= 80 * 1024) ? 2 : 1;
    const int64_t cap = (int64_t)cus * per_cu;
    if (blocks > cap) blocks = cap;
    const bool inv = (c.flags & NFA_FLAG_INVERSE) != 0;
    const k8h::KernelFn kern = f16_kernel(inv, init_ks, nw, a.sp.K, activation, with_ctx, elastic, dbg_bins);
    if (!kern) return NFA_ERR_UNSUPPORTED;
    static const char* const act_names[] = {"relu", "leaky_relu", "elu", "tanh"};
    note_layer_kernel("k8h::rqs_resnet_f16_kernel<inverse=%d, init_ks=%d, waves=%d, K=%d, ctx=%d, ring=%d, act=%s>", inv ? 1 : 0,
                      init_ks, nw, a.sp.K, with_ctx ? 1 : 0, elastic ? k8h::kRingElastic : k8h::kRing, act_names[activation]);
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(nw * kWave), lds_launch, (hipStream_t)c.stream, a, (int)lds_cap);
}

extern "C" int nfa_rqs_flow_resnet_f16x2_f32(const float* inputs, const void* stream_packed, int32_t param_stages,
                                             const int32_t* final_positions, int32_t num_layers, float* outputs,
                                             float* logabsdet, int32_t* redo_blocks, int32_t* status, int64_t batch,
                                             int32_t features, int32_t num_transform, int32_t num_identity,
                                             int32_t hidden_features, int32_t num_blocks,
                                             const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    return launch_f16({inputs, stream_packed, nullptr, final_positions, num_layers, outputs, logabsdet, redo_blocks, status,
                       batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags, stream,
                       nullptr, 0, param_stages});
}

// the same launch through the diagnostic instances: bin_idx [batch, num_transform] receives the bin every evaluation of
// the LAST layer of the run chose (include/nflows_amd.h)
extern "C" int nfa_rqs_flow_resnet_f16x2_bins_f32(const float* inputs, const void* stream_packed, int32_t param_stages,
                                                  const int32_t* final_positions, int32_t num_layers, float* outputs,
                                                  float* logabsdet, int32_t* redo_blocks, int32_t* status, int64_t batch,
                                                  int32_t features, int32_t num_transform, int32_t num_identity,
                                                  int32_t hidden_features, int32_t num_blocks,
                                                  const nfa_rqs_spec* spec, int32_t flags, void* stream, int32_t* bin_idx) {
    if (!bin_idx) return NFA_ERR_INVALID_ARGUMENT;
    return launch_f16({inputs, stream_packed, nullptr, final_positions, num_layers, outputs, logabsdet, redo_blocks, status,
                       batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags, stream,
                       nullptr, 0, param_stages},
                      bin_idx);
}

// the diagnostic instances once more, with the logits of the LAST layer (the final Linear's accumulators x kappa: the
// conditioner's output as the spline evaluation reads it) stored beside the bins (include/nflows_amd.h)
extern "C" int nfa_rqs_flow_resnet_f16x2_logits_f32(const float* inputs, const void* stream_packed, int32_t param_stages,
                                                    const int32_t* final_positions, int32_t num_layers, float* outputs,
                                                    float* logabsdet, int32_t* redo_blocks, int32_t* status, int64_t batch,
                                                    int32_t features, int32_t num_transform, int32_t num_identity,
                                                    int32_t hidden_features, int32_t num_blocks,
                                                    const nfa_rqs_spec* spec, int32_t flags, void* stream, int32_t* bin_idx,
                                                    float* logits) {
    if (!bin_idx || !logits) return NFA_ERR_INVALID_ARGUMENT;
    return launch_f16({inputs, stream_packed, nullptr, final_positions, num_layers, outputs, logabsdet, redo_blocks, status,
                       batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags, stream,
                       nullptr, 0, param_stages},
                      bin_idx, logits);
}

extern "C" int nfa_rqs_flow_resnet_context_f16x2_f32(const float* inputs, const float* context,
                                                     int32_t context_features, const void* stream_packed,
                                                     int32_t param_stages, const int32_t* final_positions,
                                                     int32_t num_layers, float* outputs, float* logabsdet,
                                                     int32_t* redo_blocks, int32_t* status, int64_t batch,
                                                     int32_t features, int32_t num_transform, int32_t num_identity,
                                                     int32_t hidden_features, int32_t num_blocks,
                                                     const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    if (context_features < 1) return NFA_ERR_INVALID_ARGUMENT;
    return launch_f16({inputs, stream_packed, nullptr, final_positions, num_layers, outputs, logabsdet, redo_blocks, status,
                       batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags, stream,
                       context, context_features, param_stages});
}
