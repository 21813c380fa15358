// K36: the density pass of ONE masked autoregressive affine layer (MaskedAffineAutoregressiveTransform.forward,
// autoregressive.py:64-128) whose MADE (made.py:233-311) is 129 .. 256 hidden units wide, with or without a context, in ONE
// launch (design notes and the kernel: affine_made_wide_kernel.hpp; instances: affine_made_wide_plain.hip,
// affine_made_wide_ctx.hip).  K22 serves widths up to 128; this is K34's column split with the affine element and K22's
// context terms.  Three bf16 pieces per operand, six products: the full fp32 range, so there is no redo pass.
//
// Restrictions (the caller keeps the MADE's GEMMs + K2b otherwise): forward only, ReLU, hidden width 129 .. 256 (packed to a
// multiple of 32), features <= 64, context features <= 64, row_length % 4 == 0 and <= 64 (pad columns pass through),
// batch % 128 == 0, one layer per launch (no folded base density).

#include "affine_made_wide_kernel.hpp"

using namespace nfa;
using namespace nfa::k36;

extern "C" int nfa_affine_layer_made_wide_f32(const float* inputs, const float* context, int32_t context_features,
                                              const void* weights_packed, const float* bias_packed,
                                              const int32_t* layer_tables, float* outputs, float* logabsdet, int32_t* status,
                                              int64_t batch, int32_t row_length, int32_t features, int32_t hidden_features,
                                              int32_t num_hidden_layers, int32_t flags, void* stream) {
    int activation = 0;   // (no activation bits here)
    int rc = check_layer_flags(flags, NFA_FLAG_RESIDUAL_BLOCKS, &activation);
    if (rc != NFA_OK) return rc;
    const bool resnet = (flags & NFA_FLAG_RESIDUAL_BLOCKS) != 0;
    if (batch < 0 || features < 1 || row_length < features || context_features < 0 || hidden_features < 1 ||
        num_hidden_layers < 0 || (resnet && (num_hidden_layers & 1)))   // (residual blocks: two Linears each)
        return NFA_ERR_INVALID_ARGUMENT;
    // (one layer per launch: the base density is not folded in)
    if ((flags & (NFA_FLAG_INVERSE | NFA_FLAG_STANDARD_NORMAL_LOG_PROB | NFA_FLAG_SKIP_OUTPUTS)) || hidden_features > 256 ||
        hidden_features <= 128 || features > 64 || context_features > 64 || row_length > 64 || (row_length & 3) != 0 ||
        (batch & 127) != 0 || num_hidden_layers > 128)
        return NFA_ERR_UNSUPPORTED;
    AffineWideArgs a;
    a.init_ks = (features + 15) / 16;
    a.final_tiles = (features + 15) / 16;
    a.ctx = context;
    a.ce = context_features;
    a.ctx_ks = (context_features + 15) / 16;
    a.num_hidden = num_hidden_layers;
    a.resnet = resnet ? 1 : 0;
    const bool ctx = context_features > 0;
    // (behind the row tile: the logabsdet shares, the context tile)
    return wide::launch(a, ctx ? affine_wide_context() : affine_wide_plain(),
                        {inputs, weights_packed, bias_packed, layer_tables, outputs, logabsdet, status, batch, row_length,
                         features, hidden_features, flags, stream,
                         (kWaves * kRows + (size_t)context_features * kPad) * sizeof(float), !ctx || context != nullptr},
                        [&] {
                            note_layer_kernel("k36::affine_made_wide_kernel<context=%d, tiles=%d, resnet=%d>", ctx ? 1 : 0,
                                              a.tiles, resnet ? 1 : 0);
                        });
}
