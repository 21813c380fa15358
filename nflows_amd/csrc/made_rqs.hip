// K29: the density pass of a run of masked autoregressive rational-quadratic spline layers
// (MaskedPiecewiseRationalQuadraticAutoregressiveTransform.forward, autoregressive.py:404-495, over a MADE,
// made.py:233-311) in ONE launch -- the kernel body is made_rqs_kernel.hpp, its instances (one per bin count) live in
// made_rqs_bins_{a,b,c}.hip.  Per element the arithmetic is K1's (`rqs_eval<K, false, linear tails, registers>`).
//
// The inverse (sampling) is sequential in the features and is not served here (K12 / K28).
//
// Restrictions (the host takes the MADE's GEMMs + K13 / K1 otherwise): hidden width 128 (narrower nets zero-padded by the
// packer), ReLU, features <= 64, context_features <= 64, 2 .. 16 bins, linear tails, row_length % 4 == 0 (pad columns
// pass through, the density epilogue skips them), batch % 128 == 0.

#include "made_rqs_kernel.hpp"

using namespace nfa;

extern "C" int nfa_rqs_flow_made_f32(const float* inputs, const float* context, int32_t context_features,
                                     const void* weights_packed, const float* bias_packed, const int32_t* tables,
                                     int32_t num_layers, float* outputs, float* logabsdet, int32_t* status, int64_t batch,
                                     int32_t row_length, int32_t features, int32_t hidden_features,
                                     int32_t num_hidden_layers, const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    int activation = 0;   // (no activation bits here)
    int rc = check_layer_flags(flags, NFA_FLAG_RESIDUAL_BLOCKS, &activation);
    if (rc != NFA_OK) return rc;
    const bool resnet = (flags & NFA_FLAG_RESIDUAL_BLOCKS) != 0;
    if (batch < 0 || features < 1 || row_length < features || context_features < 0 || num_hidden_layers < 0 ||
        num_layers < 1 || (resnet && (num_hidden_layers & 1)))   // (residual blocks: two Linears each)
        return NFA_ERR_INVALID_ARGUMENT;
    MadeRqsArgs a;
    rc = make_dev_spec(spec, &a.sp);
    if (rc != NFA_OK) return rc;
    const int K = a.sp.K;
    if ((flags & NFA_FLAG_INVERSE) || context_features > 64 || K < 2 || K > 16 || !a.sp.linear || a.sp.beta != 1.0f ||
        !layer_family(batch, row_length, features, features, hidden_features, num_hidden_layers, num_layers))
        return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    const bool ctx = context_features > 0;
    if (!inputs || !weights_packed || !bias_packed || !tables || !logabsdet || (ctx && !context) ||
        (!outputs && !(flags & NFA_FLAG_SKIP_OUTPUTS)))
        return NFA_ERR_INVALID_ARGUMENT;
    rc = fill_density(a, flags, row_length);
    if (rc != NFA_OK) return rc;
    a.sp.divisor = 0.0f;   // 1/sqrt(hidden_features) is folded into the packed rows
    a.sp.rdivisor = 0.0f;
    a.x = inputs;
    a.ctx = context;
    a.ce = context_features;
    a.ctx_ks = (context_features + 15) / 16;
    a.w = reinterpret_cast<const vec4f*>(weights_packed);
    a.bias = bias_packed;
    a.tables = tables;
    a.out = outputs;
    a.lad = logabsdet;
    a.status = status;
    a.batch = batch;
    a.D = row_length;
    a.dt = features;
    a.num_hidden = num_hidden_layers;
    a.num_layers = num_layers;
    a.resnet = resnet ? 1 : 0;
    a.init_ks = features > 32 ? 4 : 2;
    const int T = (3 * K - 1 + 15) / 16;
    const int final_tiles = ((features + 1) / 2) * T;
    // context stages: in front of the initial layer's, and behind the first Linear's of every residual block
    const int ctx_stages = ctx ? a.ctx_ks * (1 + (resnet ? num_hidden_layers / 2 : 0)) : 0;
    a.num_stages = a.init_ks + 8 * num_hidden_layers + ctx_stages + 2 * final_tiles;
    a.bias_per_layer = 128 + (ctx ? 128 : 0) + 128 * num_hidden_layers + 32 * final_tiles;
    a.accumulate = (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0;
    const size_t lds = (size_t)kRing * kStageVec4 * 16 +
                       (size_t)(kBlock / kWave) * (row_length + context_features) * kRowPad * sizeof(float);
    int64_t blocks = batch >> 7;
    const int64_t cap = (int64_t)device_cu_count();   // (one workgroup per CU: 512 registers per wave)
    if (blocks > cap) blocks = cap;
    MadeRqsKernelFn kern = T == 1 ? made_rqs_bins_low(K) : T == 2 ? made_rqs_bins_mid(K) : made_rqs_bins_high(K);
    if (!kern) return NFA_ERR_UNSUPPORTED;
    note_layer_kernel("made_rqs_kernel<K=%d, resnet=%d, context=%d>", K, resnet ? 1 : 0, ctx ? 1 : 0);
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(kBlock), lds, (hipStream_t)stream, a, kCuLds - 2048);
}
