// K8: a whole neural-spline coupling layer in ONE kernel -- the ResidualNet conditioner
// (nn/nets/resnet.py:55-100: Linear(d_i -> 128), num_blocks x [ReLU, Linear, ReLU, Linear, +skip],
// Linear(128 -> d_t*23)) followed by everything K1 replaces (coupling.py:73-130, :549-582).
//
//   * A wave owns 32 samples for the whole layer.  Their rows are read once, coalesced, into a
//     wave-private LDS tile laid out by OUTPUT position (both fused permutations applied); the
//     conditioner inputs and the spline inputs are picked from that tile, the spline results
//     overwrite their positions, and the tile is written out as whole rows: HBM sees one coalesced
//     read of the inputs and one coalesced write of the outputs, pass-through columns bit-exact.
//   * Activations never leave the register file: every GEMM is computed transposed
//     (out^T = W x act^T), so the 32x32 accumulator tiles a lane holds after one layer are -- up to
//     a fixed permutation of the k index that the host applies to the next layer's weight
//     columns -- exactly the MFMA B operand of the next layer.
//   * GEMMs run on the bf16 matrix pipe at fp32 accuracy: operands are split into three bf16
//     pieces (x = hi + mid + lo), six cross products per k-step (see K7b in rqs_fused_linear.hip).
//     Weights are split on the host, activations in registers right after each layer.
//   * The weights of the whole layer (984 KB as bf16 triples at the BASELINE shape) are streamed
//     by LDS-DMA (global_load_lds, no staging registers) through a ring of three 12 KB stages
//     shared by the four waves of the workgroup, two stages ahead of the MFMAs.
//   * The residual input is not kept in fp32: it is rebuilt from its three pieces (exact to
//     2^-25 |h|) when the skip connection is added, and the first ReLU of a block is applied to
//     the pieces on the fly (sign of the leading piece), which keeps the kernel inside 256 VGPRs.
//   * The last GEMM's accumulators are the spline logits of the lane's own two features per
//     group; they are evaluated straight from registers (as in K7).  The 1/sqrt(hidden) scale of
//     the width / height logits (coupling.py:554-556) is folded into those weight rows by the host.
//
// Restrictions (the host falls back to PyTorch GEMMs + K7/K1 otherwise): K = 8 or 10 bins, linear
// tails, hidden width 128, ReLU, no context / batch norm / active dropout, d_i <= 64,
// d_t % 4 == 0, d_t <= 64, D % 4 == 0, D <= 128, batch % 128 == 0 here (leftover rows: other path).

#include "rqs_resnet_kernel.hpp"

using namespace nfa;

template <int PRE, int PIPE, int KB, bool CTX = false>
static ResnetKernelFn resnet_pick(bool inverse, int init_ks) {
    return init_ks == 4 ? (inverse ? rqs_resnet_kernel<true, PRE, 4, PIPE, KB, CTX> : rqs_resnet_kernel<false, PRE, 4, PIPE, KB, CTX>)
                        : (inverse ? rqs_resnet_kernel<true, PRE, 2, PIPE, KB, CTX> : rqs_resnet_kernel<false, PRE, 2, PIPE, KB, CTX>);
}

// The instance of a launch, one ordered decision: tails=None, the diagnostic instances, a context or an activation or a
// bin count beyond the tuned 8 / 10 bins with ReLU (their own translation units), then the tuned instances: a context
// (the woven default form), 10 bins (woven or plain), the log2(e) fold (woven or plain) and 8 bins (pipe 2, 1 or 0).
static ResnetKernelFn resnet_kernel(bool inverse, int init_ks, int K, int activation, bool with_ctx, bool l2e, int pipe,
                                    bool no_tails, bool dbg) {
    const bool tuned = (K == 8 || K == 10) && activation == NFA_ACTIVATION_RELU;
    if (no_tails) return resnet_tails_kernel(K, inverse, init_ks);
    if (dbg) return resnet_debug_kernel(inverse, init_ks);
    if (with_ctx && !tuned) return resnet_context_kernel(K, activation, inverse, init_ks);
    if (activation != NFA_ACTIVATION_RELU) return resnet_activation_kernel(activation, K, inverse, init_ks);
    if (!tuned) return resnet_bins_kernel(K, inverse, init_ks);
    if (with_ctx) return K == 10 ? resnet_pick<1, 2, 10, true>(inverse, init_ks) : resnet_pick<1, 2, 8, true>(inverse, init_ks);
    if (K == 10) return pipe ? resnet_pick<1, 2, 10>(inverse, init_ks) : resnet_pick<1, 0, 10>(inverse, init_ks);
    if (l2e) return pipe ? resnet_pick<2, 2, 8>(inverse, init_ks) : resnet_pick<2, 0, 8>(inverse, init_ks);
    return pipe == 2 ? resnet_pick<1, 2, 8>(inverse, init_ks)
                     : pipe ? resnet_pick<1, 1, 8>(inverse, init_ks) : resnet_pick<1, 0, 8>(inverse, init_ks);
}

// redo: the second pass over the row blocks an f16 engine flagged (not the measured kernel: no profile events, the
// last layer kernel's label stays the first pass's)
static int launch_resnet_layers(const LayerCall& c, const int32_t* redo = nullptr, float* dbg_logits = nullptr) {
    ResnetArgs a;
    int activation = 0;
    int rc = check_layer_call(c, {NFA_FLAG_LOGITS_LOG2E | NFA_FLAG_ACTIVATION_MASK, true, true, false}, &a.sp, &activation);
    if (rc != NFA_OK) return rc;
    const bool relu = activation == NFA_ACTIVATION_RELU, l2e = (c.flags & NFA_FLAG_LOGITS_LOG2E) != 0;
    const bool any_bins = a.sp.K != 8 && a.sp.K != 10;   // 2 .. 16, 20, 24, 32 bins: the plain loop, no log2(e) fold
    const bool no_tails = !a.sp.linear, with_ctx = c.context_features > 0;
    // activations other than ReLU: 8 or 10 bins, the plain loop, no log2(e) fold; the log2(e) fold: 8 bins
    if ((!relu && (any_bins || l2e)) || (l2e && a.sp.K != 8)) return NFA_ERR_UNSUPPORTED;
    // tails=None (round 6): 3 K + 1 logits per feature, the plain loop, ReLU, no context, no log2(e) fold, no redo role
    if (no_tails && (!relu || l2e || with_ctx || dbg_logits || redo)) return NFA_ERR_UNSUPPORTED;
    // with a context: the default evaluation, identity features + context within the initial layer's 64 input columns
    if (with_ctx && (l2e || c.num_identity + c.context_features > 64)) return NFA_ERR_UNSUPPORTED;
    if (c.batch == 0) return NFA_OK;
    if (!layer_buffers_given(c) || !c.bias) return NFA_ERR_INVALID_ARGUMENT;
    // the diagnostic instances (nfa_rqs_flow_resnet_logits_f32): the bench's kernel family only
    if (dbg_logits && (a.sp.K != 8 || with_ctx || !relu || l2e || redo)) return NFA_ERR_UNSUPPORTED;
    rc = fill_layer_args(a, c);
    if (rc != NFA_OK) return rc;
    a.bias = c.bias;
    a.tables = c.tables;
    a.ctx = with_ctx ? c.context : nullptr;
    a.ce = c.context_features;
    a.dbg_logits = dbg_logits;
    a.trace = g_k7_trace;
    a.redo = redo;
    const int rows_per_feature = no_tails ? 16 * ((3 * a.sp.K + 1 + 15) / 16) : spline_rows_per_feature(a.sp.K);
    const int init_ks = c.num_identity + c.context_features > 32 ? 4 : 2;
    a.num_stages = init_ks + (with_ctx ? (c.context_features <= 16 ? 17 : 20) : 16) * c.num_blocks +
                   2 * (c.num_transform * rows_per_feature / 32);
    a.bias_per_layer = 128 + (with_ctx ? 384 : 256) * c.num_blocks + c.num_transform * rows_per_feature;
    // final layer with the spline evaluation woven into its MFMAs (not with the log2(e) fold):
    //   2 (default)  woven, FlatSteps<FAST>: cheaper rounding sequence, same error class
    //   1            woven, same results bit for bit as the plain loop
    //   0            the plain loop
    static const int use_pipe = [] {
        const char* e = getenv("NFA_K8_PIPE");
        return e ? atoi(e) : 2;
    }();
    // `pipe`: the woven form in use, 0 for the plain loop (with the log2(e) fold and at 10 bins only the default woven
    // form exists)
    const int pipe = !no_tails && !dbg_logits && !any_bins && relu && use_pipe &&
                             ((a.sp.K == 8 && (!l2e || use_pipe == 2)) || (a.sp.K == 10 && use_pipe == 2))
                         ? use_pipe : 0;
    // a context: the woven default form at 8 / 10 bins with ReLU; the plain loop for the other bin counts and
    // activations (round 5: rqs_resnet_ctx.hip)
    if (with_ctx && !any_bins && relu && pipe != 2) return NFA_ERR_UNSUPPORTED;
    const size_t lds = (size_t)kRing * kStageVec4 * 16 + (size_t)(kBlock / kWave) * c.features * kRowPad * sizeof(float) +
                       (pipe ? (size_t)c.num_transform * rows_per_feature * sizeof(float) : 0) +
                       (size_t)(kBlock / kWave) * c.context_features * kRowPad * sizeof(float) +
                       (with_ctx ? (size_t)(kBlock / kWave) * 64 * kWave * sizeof(float) : 0);
    int64_t blocks = c.batch >> 7;
    const int64_t per_cu = lds + 2048 <= 80 * 1024 ? 2 : 1;
    const int64_t cap = (int64_t)device_cu_count() * per_cu;
    if (blocks > cap) blocks = cap;
    const bool inv = (c.flags & NFA_FLAG_INVERSE) != 0;
    const ResnetKernelFn kern = resnet_kernel(inv, init_ks, a.sp.K, activation, with_ctx, l2e, pipe, no_tails, dbg_logits);
    if (!kern) return NFA_ERR_UNSUPPORTED;
    if (!redo)
        note_layer_kernel("rqs_resnet_kernel<inverse=%d, init_ks=%d, pipe=%d, K=%d, ctx=%d, act=%d%s>", inv ? 1 : 0, init_ks,
                          pipe, a.sp.K, with_ctx ? 1 : 0, activation, no_tails ? ", tails=none" : "");
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(kBlock), lds, (hipStream_t)c.stream, a, kCuLds - 2048,
                         !redo);
}

extern "C" int nfa_rqs_coupling_resnet_f32(const float* inputs, const void* weights_packed,
                                           const float* bias_packed, const int32_t* layer_tables,
                                           float* outputs, float* logabsdet, int32_t* status,
                                           int64_t batch, int32_t features, int32_t num_transform,
                                           int32_t num_identity, int32_t hidden_features,
                                           int32_t num_blocks, const nfa_rqs_spec* spec, int32_t flags,
                                           void* stream) {
    return launch_resnet_layers({inputs, weights_packed, bias_packed, layer_tables, 1, outputs, logabsdet, nullptr, status,
                                 batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags,
                                 stream, nullptr, 0, 0});
}

extern "C" int nfa_rqs_flow_resnet_f32(const float* inputs, const void* weights_packed,
                                       const float* bias_packed, const int32_t* flow_tables,
                                       int32_t num_layers, float* outputs, float* logabsdet,
                                       int32_t* status, int64_t batch, int32_t features,
                                       int32_t num_transform, int32_t num_identity,
                                       int32_t hidden_features, int32_t num_blocks,
                                       const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    return launch_resnet_layers({inputs, weights_packed, bias_packed, flow_tables, num_layers, outputs, logabsdet, nullptr,
                                 status, batch, features, num_transform, num_identity, hidden_features, num_blocks, spec,
                                 flags, stream, nullptr, 0, 0});
}

// the diagnostic instances: the same launch with the LAST layer's logits stored (include/nflows_amd.h)
extern "C" int nfa_rqs_flow_resnet_logits_f32(const float* inputs, const void* weights_packed,
                                              const float* bias_packed, const int32_t* flow_tables,
                                              int32_t num_layers, float* outputs, float* logabsdet,
                                              int32_t* status, int64_t batch, int32_t features,
                                              int32_t num_transform, int32_t num_identity,
                                              int32_t hidden_features, int32_t num_blocks,
                                              const nfa_rqs_spec* spec, int32_t flags, void* stream, float* logits) {
    if (!logits) return NFA_ERR_INVALID_ARGUMENT;
    return launch_resnet_layers({inputs, weights_packed, bias_packed, flow_tables, num_layers, outputs, logabsdet, nullptr,
                                 status, batch, features, num_transform, num_identity, hidden_features, num_blocks, spec,
                                 flags, stream, nullptr, 0, 0},
                                nullptr, logits);
}

extern "C" int nfa_rqs_flow_resnet_redo_f32(const float* inputs, const void* weights_packed,
                                            const float* bias_packed, const int32_t* flow_tables,
                                            int32_t num_layers, float* outputs, float* logabsdet,
                                            const int32_t* redo_blocks, int32_t* status, int64_t batch,
                                            int32_t features, int32_t num_transform, int32_t num_identity,
                                            int32_t hidden_features, int32_t num_blocks,
                                            const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    if (!redo_blocks) return NFA_ERR_INVALID_ARGUMENT;
    return launch_resnet_layers({inputs, weights_packed, bias_packed, flow_tables, num_layers, outputs, logabsdet, nullptr,
                                 status, batch, features, num_transform, num_identity, hidden_features, num_blocks, spec,
                                 flags, stream, nullptr, 0, 0},
                                redo_blocks);
}

extern "C" int nfa_rqs_flow_resnet_context_f32(const float* inputs, const float* context, int32_t context_features,
                                               const void* weights_packed, const float* bias_packed,
                                               const int32_t* flow_tables, int32_t num_layers, float* outputs,
                                               float* logabsdet, int32_t* status, int64_t batch, int32_t features,
                                               int32_t num_transform, int32_t num_identity,
                                               int32_t hidden_features, int32_t num_blocks,
                                               const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    if (context_features < 1) return NFA_ERR_INVALID_ARGUMENT;
    return launch_resnet_layers({inputs, weights_packed, bias_packed, flow_tables, num_layers, outputs, logabsdet, nullptr,
                                 status, batch, features, num_transform, num_identity, hidden_features, num_blocks, spec,
                                 flags, stream, context, context_features, 0});
}

extern "C" int nfa_rqs_flow_resnet_context_redo_f32(const float* inputs, const float* context,
                                                    int32_t context_features, const void* weights_packed,
                                                    const float* bias_packed, const int32_t* flow_tables,
                                                    int32_t num_layers, float* outputs, float* logabsdet,
                                                    const int32_t* redo_blocks, int32_t* status, int64_t batch,
                                                    int32_t features, int32_t num_transform, int32_t num_identity,
                                                    int32_t hidden_features, int32_t num_blocks,
                                                    const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    if (context_features < 1 || !redo_blocks) return NFA_ERR_INVALID_ARGUMENT;
    return launch_resnet_layers({inputs, weights_packed, bias_packed, flow_tables, num_layers, outputs, logabsdet, nullptr,
                                 status, batch, features, num_transform, num_identity, hidden_features, num_blocks, spec,
                                 flags, stream, context, context_features, 0},
                                redo_blocks);
}
