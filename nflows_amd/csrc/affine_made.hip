// K22: the density pass of a run of masked autoregressive affine layers (MaskedAffineAutoregressiveTransform.forward,
// autoregressive.py:64-128, over a MADE, made.py:233-311) in ONE launch -- K11's kernel body (affine_mlp_kernel.hpp) in
// its autoregressive mode.  With the masks multiplied into the weights at pack time a MADE is K11's conditioner with
// d_i = d_t = features: residual blocks are its RESNET form, feed-forward blocks its MLP form; the scale is
// softplus(u) + 1e-3 and every feature is read by the initial layer and overwritten by the output layer's tiles.
// Per element the arithmetic is K2b's (`affine_element<false>`, `scale_of(u, NFA_SCALE_SOFTPLUS)`).
//
// The inverse (sampling) is sequential in the features and is not served here.
//
// Restrictions (the host takes the MADE's GEMMs + K2b otherwise): hidden width 128 (narrower nets zero-padded by the
// packer), ReLU, features <= 64, context_features <= 64, row_length % 4 == 0 (pad columns pass through, the density
// epilogue skips them), batch % 128 == 0.

#include "affine_mlp_kernel.hpp"

using namespace nfa;

template <int IKS, bool RESNET>
static void (*affine_made_instance(bool ctx))(const AffineMlpArgs) {
    return ctx ? affine_mlp_kernel<false, IKS, false, RESNET, true, true>
               : affine_mlp_kernel<false, IKS, false, RESNET, true, false>;
}

extern "C" int nfa_affine_flow_made_f32(const float* inputs, const float* context, int32_t context_features,
                                        const void* weights_packed, const float* bias_packed, const int32_t* tables,
                                        int32_t num_layers, float* outputs, float* logabsdet, int32_t* status,
                                        int64_t batch, int32_t row_length, int32_t features, int32_t hidden_features,
                                        int32_t num_hidden_layers, int32_t flags, void* stream) {
    int activation = 0;   // (no activation bits here)
    int rc = check_layer_flags(flags, NFA_FLAG_RESIDUAL_BLOCKS, &activation);
    if (rc != NFA_OK) return rc;
    const bool resnet = (flags & NFA_FLAG_RESIDUAL_BLOCKS) != 0;
    if (batch < 0 || features < 1 || row_length < features || context_features < 0 || num_hidden_layers < 0 ||
        num_layers < 1 || (resnet && (num_hidden_layers & 1)))   // (residual blocks: two Linears each)
        return NFA_ERR_INVALID_ARGUMENT;
    if ((flags & NFA_FLAG_INVERSE) || context_features > 64 ||
        !layer_family(batch, row_length, features, features, hidden_features, num_hidden_layers, num_layers))
        return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    const bool ctx = context_features > 0;
    if (!inputs || !weights_packed || !bias_packed || !tables || !logabsdet || (ctx && !context) ||
        (!outputs && !(flags & NFA_FLAG_SKIP_OUTPUTS)))
        return NFA_ERR_INVALID_ARGUMENT;
    AffineMlpArgs a;
    rc = fill_density(a, flags, row_length);
    if (rc != NFA_OK) return rc;
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
    a.di = features;
    a.num_hidden = num_hidden_layers;
    a.num_layers = num_layers;
    a.activation = NFA_SCALE_SOFTPLUS;
    a.final_tiles = (features + 15) / 16;
    const int init_ks = features > 32 ? 4 : 2;
    // context stages: in front of the initial layer's, and behind the first Linear's of every residual block
    const int ctx_stages = ctx ? a.ctx_ks * (1 + (resnet ? num_hidden_layers / 2 : 0)) : 0;
    a.num_stages = init_ks + 8 * num_hidden_layers + ctx_stages + 2 * a.final_tiles;
    a.bias_per_layer = 128 + (ctx ? 128 : 0) + 128 * num_hidden_layers + 32 * a.final_tiles;
    a.accumulate = (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0;
    const size_t lds = (size_t)kRing * kStageVec4 * 16 +
                       (size_t)(kBlock / kWave) * (row_length + context_features) * kRowPad * sizeof(float);
    int64_t blocks = batch >> 7;
    const int64_t cap = (int64_t)device_cu_count();   // (one workgroup per CU: 512 registers per wave)
    if (blocks > cap) blocks = cap;
    void (*kern)(const AffineMlpArgs) =
        resnet ? (init_ks == 4 ? affine_made_instance<4, true>(ctx) : affine_made_instance<2, true>(ctx))
               : (init_ks == 4 ? affine_made_instance<4, false>(ctx) : affine_made_instance<2, false>(ctx));
    note_layer_kernel("affine_mlp_kernel<autoregressive=1, init_ks=%d, resnet=%d, context=%d>", init_ks, resnet ? 1 : 0,
                      ctx ? 1 : 0);
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(kBlock), lds, (hipStream_t)stream, a, kCuLds - 2048);
}
