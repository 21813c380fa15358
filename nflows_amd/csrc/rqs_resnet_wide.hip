// K32: one neural-spline coupling layer whose ResidualNet conditioner is 129 .. 256 hidden units wide, in ONE launch
// (design notes and the kernel: rqs_resnet_wide_kernel.hpp; instances: rqs_resnet_wide_bins_*.hip).  The conditioner is
// nn/nets/resnet.py:55-100 -- Linear(d_i -> H), num_blocks x [ReLU, Linear, ReLU, Linear, + skip], Linear(H -> d_t (3 K - 1))
// -- followed by everything K1 replaces (coupling.py:73-130, :549-582).  Three bf16 pieces per operand, six products: the
// full fp32 range, so there is no redo pass and no `redo_blocks`.
//
// Restrictions (the caller keeps stock GEMMs + K1 otherwise): 2 .. 16 bins, linear tails, ReLU blocks, no context, hidden
// width <= 256 (packed to a multiple of 32), d_i <= 64, d_t % 4 == 0, d_t <= 64, D % 4 == 0, D <= 128, batch % 128 == 0,
// the exchange buffer and the row tile within the CU's LDS.

#include "rqs_resnet_wide_kernel.hpp"

using namespace nfa;
using namespace nfa::k32;

static int launch_wide_layer(const LayerCall& c) {
    WideArgs a;
    int activation = 0;
    if (c.hidden_features < 1) return NFA_ERR_INVALID_ARGUMENT;
    // the shared checks on the family's other limits; the width is this engine's own
    LayerCall family = c;
    family.hidden_features = 128;
    int rc = check_layer_call(family, {0, true, false, false}, &a.sp, &activation);
    if (rc != NFA_OK) return rc;
    const int K = a.sp.K;
    if (K > 16 || c.hidden_features > 256) return NFA_ERR_UNSUPPORTED;
    // (one layer per launch: the base density is not folded in; an empty batch is answered before this rule)
    if (c.batch != 0 && (c.flags & (NFA_FLAG_STANDARD_NORMAL_LOG_PROB | NFA_FLAG_SKIP_OUTPUTS))) return NFA_ERR_UNSUPPORTED;
    a.init_ks = (c.num_identity + 15) / 16;
    a.di = c.num_identity;
    a.num_blocks = c.num_blocks;
    const bool inv = (c.flags & NFA_FLAG_INVERSE) != 0;
    const int T = (3 * K - 1 + 15) / 16;
    return wide::launch(a, T == 2 ? wide_bins_mid(K, inv) : wide_bins_low(K, inv),
                        {c.inputs, c.weights, c.bias, c.tables, c.outputs, c.logabsdet, c.status, c.batch, c.features,
                         c.num_transform, c.hidden_features, c.flags, c.stream, kWaves * kRows * sizeof(float)},
                        [&] { note_layer_kernel("k32::rqs_resnet_wide_kernel<inverse=%d, K=%d, tiles=%d>", inv ? 1 : 0, K, a.tiles); });
}

extern "C" int nfa_rqs_layer_resnet_wide_f32(const float* inputs, const void* weights_packed, const float* bias_packed,
                                             const int32_t* layer_tables, float* outputs, float* logabsdet,
                                             int32_t* status, int64_t batch, int32_t features, int32_t num_transform,
                                             int32_t num_identity, int32_t hidden_features, int32_t num_blocks,
                                             const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    return launch_wide_layer({inputs, weights_packed, bias_packed, layer_tables, 1, outputs, logabsdet, nullptr, status,
                              batch, features, num_transform, num_identity, hidden_features, num_blocks, spec, flags,
                              stream, nullptr, 0, 0});
}
