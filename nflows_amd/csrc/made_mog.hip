// K31: MixtureOfGaussiansMADE.log_prob (nn/nde/made.py: the density-estimator MADE's forward pass, then per element
// logsumexp_k(log_softmax(logits)_k + log N(x; m_k, softplus(u_k) + epsilon)) summed over the features) in ONE launch -- the
// kernel body is made_mog_kernel.hpp, its three instances (T = 1, 2, 3 tiles per pair of features: K <= 5, <= 10, <= 16)
// live here.  Per element the arithmetic is K20's (density_math.hpp, float64, rounded once per row).  Only `batch` floats
// leave the chip; the [batch, features * K * 3] parameters never exist.
//
// Restrictions (the host takes the MADE's stock ops + K20 otherwise): hidden width 128 (narrower nets zero-padded by the
// packer), ReLU, 1 .. 64 features, context_features <= 64, 1 .. 16 components, batch % 128 == 0, forward only.

#include "made_mog_kernel.hpp"

using namespace nfa;

extern "C" int nfa_made_mog_log_prob_f32(const float* inputs, const float* context, int32_t context_features,
                                         const void* weights_packed, const float* bias_packed, const float* add,
                                         float* log_prob, int64_t batch, int32_t features, int32_t hidden_features,
                                         int32_t num_hidden_layers, int32_t num_components, double epsilon, int32_t flags,
                                         void* stream) {
    if (flags & ~NFA_FLAG_RESIDUAL_BLOCKS) return NFA_ERR_INVALID_ARGUMENT;
    const bool resnet = (flags & NFA_FLAG_RESIDUAL_BLOCKS) != 0;
    if (batch < 0 || features < 1 || context_features < 0 || num_hidden_layers < 0 || num_components < 1 ||
        (resnet && (num_hidden_layers & 1)))   // (residual blocks: two Linears each)
        return NFA_ERR_INVALID_ARGUMENT;
    const int K = num_components;
    // (layer_family's row length is a multiple of four; this kernel reads any, so the family is asked about the next one)
    if (context_features > 64 || K > 16 ||
        !layer_family(batch, (features + 3) & ~3, features, features, hidden_features, num_hidden_layers, 1))
        return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    const bool ctx = context_features > 0;
    if (!inputs || !weights_packed || !bias_packed || !log_prob || (ctx && !context)) return NFA_ERR_INVALID_ARGUMENT;
    MadeMogArgs a;
    a.x = inputs;
    a.ctx = context;
    a.ce = context_features;
    a.ctx_ks = (context_features + 15) / 16;
    a.w = reinterpret_cast<const vec4f*>(weights_packed);
    a.bias = bias_packed;
    a.add = add;
    a.out = log_prob;
    a.batch = batch;
    a.D = features;
    a.num_hidden = num_hidden_layers;
    a.resnet = resnet ? 1 : 0;
    a.init_ks = features > 32 ? 4 : 2;
    a.K = K;
    a.epsilon = epsilon;
    const int T = (3 * K + 15) / 16;
    const int final_tiles = ((features + 1) / 2) * T;
    // context stages: in front of the initial layer's, and behind the first Linear's of every residual block
    const int ctx_stages = ctx ? a.ctx_ks * (1 + (resnet ? num_hidden_layers / 2 : 0)) : 0;
    a.num_stages = a.init_ks + 8 * num_hidden_layers + ctx_stages + 2 * final_tiles;
    const size_t lds = (size_t)kRing * kStageVec4 * 16 +
                       (size_t)(kBlock / kWave) * (features + context_features) * kRowPad * sizeof(float);
    int64_t blocks = batch >> 7;
    const int64_t cap = (int64_t)device_cu_count();   // (one workgroup per CU: 512 registers per wave)
    if (blocks > cap) blocks = cap;
    void (*kern)(const MadeMogArgs) = T == 1 ? made_mog_kernel<1> : T == 2 ? made_mog_kernel<2> : made_mog_kernel<3>;
    note_layer_kernel("made_mog_kernel<K=%d, resnet=%d, context=%d>", K, resnet ? 1 : 0, ctx ? 1 : 0);
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(kBlock), lds, (hipStream_t)stream, a, kCuLds - 2048);
}
