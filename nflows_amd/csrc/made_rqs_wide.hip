// K34: the density pass of ONE masked autoregressive rational-quadratic spline layer
// (MaskedPiecewiseRationalQuadraticAutoregressiveTransform.forward, autoregressive.py:404-495) whose MADE (made.py:233-311)
// is 129 .. 256 hidden units wide, in ONE launch (design notes and the kernel: made_rqs_wide_kernel.hpp; instances:
// made_rqs_wide_bins_*.hip).  K29 serves widths up to 128; this is K32's column split with a MADE's dataflow.  Three bf16
// pieces per operand, six products: the full fp32 range, so there is no redo pass.
//
// Restrictions (the caller keeps the MADE's GEMMs + K13 / K1 otherwise): forward only, 2 .. 16 bins, linear tails, ReLU, no
// context, hidden width <= 256 (packed to a multiple of 32), features <= 64, row_length % 4 == 0 and <= 64 (pad columns pass
// through), batch % 128 == 0, one layer per launch (no folded base density).

#include "made_rqs_wide_kernel.hpp"

using namespace nfa;
using namespace nfa::k34;

extern "C" int nfa_rqs_layer_made_wide_f32(const float* inputs, const void* weights_packed, const float* bias_packed,
                                           const int32_t* layer_tables, float* outputs, float* logabsdet, int32_t* status,
                                           int64_t batch, int32_t row_length, int32_t features, int32_t hidden_features,
                                           int32_t num_hidden_layers, const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    int activation = 0;   // (no activation bits here)
    int rc = check_layer_flags(flags, NFA_FLAG_RESIDUAL_BLOCKS, &activation);
    if (rc != NFA_OK) return rc;
    const bool resnet = (flags & NFA_FLAG_RESIDUAL_BLOCKS) != 0;
    if (batch < 0 || features < 1 || row_length < features || hidden_features < 1 || num_hidden_layers < 0 ||
        (resnet && (num_hidden_layers & 1)))   // (residual blocks: two Linears each)
        return NFA_ERR_INVALID_ARGUMENT;
    MadeWideArgs a;
    rc = make_dev_spec(spec, &a.sp);
    if (rc != NFA_OK) return rc;
    const int K = a.sp.K;
    // (one layer per launch: the base density is not folded in)
    if ((flags & (NFA_FLAG_INVERSE | NFA_FLAG_STANDARD_NORMAL_LOG_PROB | NFA_FLAG_SKIP_OUTPUTS)) || K < 2 || K > 16 ||
        !a.sp.linear || a.sp.beta != 1.0f || hidden_features > 256 || features > 64 || row_length > 64 ||
        (row_length & 3) != 0 || (batch & 127) != 0 || num_hidden_layers > 128)
        return NFA_ERR_UNSUPPORTED;
    a.init_ks = (features + 15) / 16;
    a.num_hidden = num_hidden_layers;
    a.resnet = resnet ? 1 : 0;
    const int T = (3 * K - 1 + 15) / 16;
    return wide::launch(a, T == 2 ? made_wide_bins_mid(K) : made_wide_bins_low(K),
                        {inputs, weights_packed, bias_packed, layer_tables, outputs, logabsdet, status, batch, row_length,
                         features, hidden_features, flags, stream, kWaves * kRows * sizeof(float)},
                        [&] { note_layer_kernel("k34::made_rqs_wide_kernel<K=%d, tiles=%d, resnet=%d>", K, a.tiles, resnet ? 1 : 0); });
}
