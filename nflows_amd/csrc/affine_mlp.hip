// K11: a whole affine / additive coupling layer in ONE kernel, a run of such layers in one launch --
// the MLP conditioner (nn/nets/mlp.py:47-68: Linear(d_i -> 128), [ReLU, Linear(128 -> 128)] x n,
// ReLU, Linear(128 -> 2 d_t)) followed by everything K2 replaces (coupling.py:73-130, :212-269):
// split, scale activation, x * scale + shift (or its inverse), the log-determinant row sum, scatter,
// and the neighbouring permutations.
//
// The kernel body is in affine_mlp_kernel.hpp (K22, affine_made.hip, instantiates it too); this file holds K11's entry point.
// Same skeleton as K8 (rqs_resnet.hip), same GEMM machinery (bf16x3_gemm.hpp): a wave owns 32 samples
// for the whole run, their rows live in a wave-private LDS tile indexed by slot, activations stay in
// registers as three bf16 pieces (fp32-accurate products on the bf16 matrix pipe, full fp32 range: no
// second pass needed), weights arrive through the LDS-DMA ring.  What differs:
//   * ReLU sits between the Linears (no skip connections): every GEMM applies it to its input pieces
//     on the fly, the accumulators are converted to pieces unchanged.
//   * The last Linear has 2 d_t rows (d_t for the additive layer).  The host orders them so that the
//     16 accumulator values of a lane-half are [shift of 8 features | unconstrained scale of the same 8
//     features] (affine) or [shift of 16 features] (additive): tile t covers features 16 t .. 16 t + 15
//     (32 t .. for additive), padded with zero rows.
//   * Per element the arithmetic is K2's, instruction for instruction (`scale_of`, logf, the IEEE
//     division of the inverse), so the only difference to "MLP by GEMMs, then K2" is the rounding of
//     the GEMM sums.
//
// Restrictions (the host takes GEMMs + K2 otherwise): hidden width 128 in every hidden layer, ReLU,
// d_i <= 64, d_t <= 64, D % 4 == 0, D <= 128, batch % 128 == 0 here (leftover rows: other path),
// scale activation default / general / additive.

#include "affine_mlp_kernel.hpp"

using namespace nfa;

template <int IKS, bool ADDITIVE, bool RESNET>
static void (*affine_mlp_instance(bool inverse))(const AffineMlpArgs) {
    return inverse ? affine_mlp_kernel<true, IKS, ADDITIVE, RESNET> : affine_mlp_kernel<false, IKS, ADDITIVE, RESNET>;
}

extern "C" int nfa_affine_flow_mlp_f32(const float* inputs, const void* weights_packed, const float* bias_packed,
                                       const int32_t* tables, int32_t num_layers, float* outputs,
                                       float* logabsdet, int32_t* status, int64_t batch, int32_t features,
                                       int32_t num_transform, int32_t num_identity, int32_t hidden_features,
                                       int32_t num_hidden_layers, int32_t scale_activation, int32_t flags,
                                       void* stream) {
    int activation = 0;   // (no activation bits here)
    int rc = check_layer_flags(flags, NFA_FLAG_RESIDUAL_BLOCKS, &activation);
    if (rc != NFA_OK) return rc;
    const bool resnet = (flags & NFA_FLAG_RESIDUAL_BLOCKS) != 0;
    if (batch < 0 || features < 1 || num_transform < 1 || num_identity < 1 ||
        num_transform + num_identity > features || num_hidden_layers < 0 || num_layers < 1 ||
        (resnet && (num_hidden_layers & 1)))   // (residual blocks: two Linears each)
        return NFA_ERR_INVALID_ARGUMENT;
    if (scale_activation != NFA_SCALE_DEFAULT && scale_activation != NFA_SCALE_GENERAL &&
        scale_activation != NFA_SCALE_ADDITIVE)
        return NFA_ERR_UNSUPPORTED;
    if (!layer_family(batch, features, num_transform, num_identity, hidden_features, num_hidden_layers, num_layers))
        return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    if (!inputs || !weights_packed || !bias_packed || !tables || !logabsdet ||
        (!outputs && !(flags & NFA_FLAG_SKIP_OUTPUTS)))
        return NFA_ERR_INVALID_ARGUMENT;
    const bool additive = scale_activation == NFA_SCALE_ADDITIVE;
    AffineMlpArgs a;
    rc = fill_density(a, flags, features);
    if (rc != NFA_OK) return rc;
    a.x = inputs;
    a.ctx = nullptr;   // (K22's context: affine_made.hip)
    a.ce = a.ctx_ks = 0;
    a.w = reinterpret_cast<const vec4f*>(weights_packed);
    a.bias = bias_packed;
    a.tables = tables;
    a.out = outputs;
    a.lad = logabsdet;
    a.status = status;
    a.batch = batch;
    a.D = features;
    a.dt = num_transform;
    a.di = num_identity;
    a.num_hidden = num_hidden_layers;
    a.num_layers = num_layers;
    a.activation = scale_activation;
    a.final_tiles = additive ? (num_transform + 31) / 32 : (num_transform + 15) / 16;
    const int init_ks = num_identity > 32 ? 4 : 2;
    a.num_stages = init_ks + 8 * num_hidden_layers + 2 * a.final_tiles;
    a.bias_per_layer = 128 + 128 * num_hidden_layers + 32 * a.final_tiles;
    a.accumulate = (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0;
    const size_t lds = (size_t)kRing * kStageVec4 * 16 + (size_t)(kBlock / kWave) * features * kRowPad * sizeof(float);
    int64_t blocks = batch >> 7;
    const int64_t cap = (int64_t)device_cu_count();   // (one workgroup per CU: 512 registers per wave)
    if (blocks > cap) blocks = cap;
    const bool inv = (flags & NFA_FLAG_INVERSE) != 0;
    void (*kern)(const AffineMlpArgs) =
        resnet ? (init_ks == 4 ? (additive ? affine_mlp_instance<4, true, true>(inv) : affine_mlp_instance<4, false, true>(inv))
                               : (additive ? affine_mlp_instance<2, true, true>(inv) : affine_mlp_instance<2, false, true>(inv)))
               : (init_ks == 4 ? (additive ? affine_mlp_instance<4, true, false>(inv) : affine_mlp_instance<4, false, false>(inv))
                               : (additive ? affine_mlp_instance<2, true, false>(inv) : affine_mlp_instance<2, false, false>(inv)));
    if (resnet) note_layer_kernel("affine_mlp_kernel<inverse=%d, init_ks=%d, additive=%d, resnet=1>", inv ? 1 : 0, init_ks, additive ? 1 : 0);
    else note_layer_kernel("affine_mlp_kernel<inverse=%d, init_ks=%d, additive=%d>", inv ? 1 : 0, init_ks, additive ? 1 : 0);
    return launch_kernel(kern, dim3((unsigned)blocks), dim3(kBlock), lds, (hipStream_t)stream, a, kCuLds - 2048);
}
