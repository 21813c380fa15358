// K37: one affine / additive coupling layer (coupling.py:73-130, :212-269) whose conditioner is 129 .. 256 hidden units wide,
// in ONE launch, both directions (design notes and the kernel: affine_resnet_wide_kernel.hpp; the MLP-form instances:
// affine_resnet_wide_mlp.hip).  The conditioner is a ResidualNet (nn/nets/resnet.py:55-100: Linear(d_i -> H), num_blocks x
// [ReLU, Linear, ReLU, Linear, + skip], Linear(H -> 2 d_t)) with NFA_FLAG_RESIDUAL_BLOCKS, otherwise a ReLU MLP
// (nn/nets/mlp.py:47-68: Linear(d_i -> H), [ReLU, Linear(H -> H)] x n, ReLU, Linear(H -> 2 d_t)); the additive layer has
// d_t outputs.  K11 serves widths up to 128; this is K32's column split with a final layer and an element step of its own.
// Three bf16 pieces per operand, six products: the full fp32 range, so there is no redo pass.
//
// Restrictions (the caller keeps stock GEMMs + K2 otherwise): ReLU, no context, hidden width <= 256 (packed to a multiple of
// 32), d_i <= 64, d_t <= 64, D % 4 == 0, D <= 128, batch % 128 == 0, scale activation default / general / additive, one
// layer per launch (no folded base density), the exchange buffer and the row tile within the CU's LDS.

#include "affine_resnet_wide_kernel.hpp"

using namespace nfa;
using namespace nfa::k37;

AffineWideKernelFn nfa::k37::affine_wide_resnet(bool inverse, bool additive) {
    return inverse ? (additive ? affine_resnet_wide_kernel<true, true, true> : affine_resnet_wide_kernel<true, false, true>)
                   : (additive ? affine_resnet_wide_kernel<false, true, true> : affine_resnet_wide_kernel<false, false, true>);
}

extern "C" int nfa_affine_layer_resnet_wide_f32(const float* inputs, const void* weights_packed, const float* bias_packed,
                                                const int32_t* layer_tables, float* outputs, float* logabsdet,
                                                int32_t* status, int64_t batch, int32_t features, int32_t num_transform,
                                                int32_t num_identity, int32_t hidden_features, int32_t num_hidden_layers,
                                                int32_t scale_activation, int32_t flags, void* stream) {
    int activation = 0;   // (no activation bits here)
    int rc = check_layer_flags(flags, NFA_FLAG_RESIDUAL_BLOCKS, &activation);
    if (rc != NFA_OK) return rc;
    const bool resnet = (flags & NFA_FLAG_RESIDUAL_BLOCKS) != 0;
    if (batch < 0 || features < 1 || num_transform < 1 || num_identity < 1 || num_transform + num_identity > features ||
        hidden_features < 1 || num_hidden_layers < 0 || (resnet && (num_hidden_layers & 1)))   // (two Linears per block)
        return NFA_ERR_INVALID_ARGUMENT;
    if (scale_activation != NFA_SCALE_DEFAULT && scale_activation != NFA_SCALE_GENERAL &&
        scale_activation != NFA_SCALE_ADDITIVE)
        return NFA_ERR_UNSUPPORTED;
    // (one layer per launch: the base density is not folded in)
    if ((flags & (NFA_FLAG_STANDARD_NORMAL_LOG_PROB | NFA_FLAG_SKIP_OUTPUTS)) || hidden_features > 256 ||
        num_transform > 64 || num_identity > 64 || features > 128 || (features & 3) != 0 || (batch & 127) != 0 ||
        num_hidden_layers > 128)
        return NFA_ERR_UNSUPPORTED;
    const bool additive = scale_activation == NFA_SCALE_ADDITIVE;
    AffineWideArgs a;
    a.init_ks = (num_identity + 15) / 16;
    a.final_tiles = additive ? (num_transform + 31) / 32 : (num_transform + 15) / 16;
    a.di = num_identity;
    a.num_hidden = num_hidden_layers;
    a.activation = scale_activation;
    const bool inv = (flags & NFA_FLAG_INVERSE) != 0;
    // (behind the row tile: the units' logabsdet shares)
    return wide::launch(a, resnet ? affine_wide_resnet(inv, additive) : affine_wide_mlp(inv, additive),
                        {inputs, weights_packed, bias_packed, layer_tables, outputs, logabsdet, status, batch, features,
                         num_transform, hidden_features, flags, stream, kWaves * 32 * sizeof(float)},
                        [&] {
                            note_layer_kernel("k37::affine_resnet_wide_kernel<inverse=%d, additive=%d, resnet=%d, tiles=%d>",
                                              inv ? 1 : 0, additive ? 1 : 0, resnet ? 1 : 0, a.tiles);
                        });
}
