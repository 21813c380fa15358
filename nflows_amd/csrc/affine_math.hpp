// Per-element arithmetic of the affine layers (K2 `affine_coupling_kernel`, K2b `affine_ar_kernel`, K11
// `affine_mlp_kernel`): the scale activations and the map x -> x * scale + shift with its log-derivative.  No
// wave-level operation and no HIP type in here: the CPU suite compiles this file for the host
// (tests/test_affine_host.py) and holds it to the reference's vectors.
#pragma once
#include <math.h>

namespace nfa {

__device__ __forceinline__ float softplus1(float x) {
#pragma clang fp contract(off)
    return x > 20.0f ? x : log1pf(expf(x));
}

// scale activations, coupling.py:224-225 / autoregressive.py:101
__device__ __forceinline__ float scale_of(float u, int activation) {
#pragma clang fp contract(off)
    if (activation == NFA_SCALE_DEFAULT) {
        const float v = u + 2.0f;
        return 1.0f / (1.0f + expf(-v)) + 1e-3f;
    } else if (activation == NFA_SCALE_GENERAL) {
        float s = softplus1(u) + 1e-3f;
        s = s < 0.0f ? 0.0f : s;  // clamp(0, 3); NaN propagates like aten's clamp
        s = s > 3.0f ? 3.0f : s;
        return s;
    } else {  // NFA_SCALE_SOFTPLUS
        return softplus1(u) + 1e-3f;
    }
}



// one element of an affine layer given its scale: coupling.py:242-252 (forward y = x * scale + shift, logabsdet +=
// log scale; inverse x = (y - shift) / scale, logabsdet -= log scale), autoregressive.py:96-121
template <bool INVERSE>
__device__ __forceinline__ void affine_element(float xin, float shift, float sc, float& y, float& l) {
#pragma clang fp contract(off)
    const float ls = logf(sc);
    if (INVERSE) {
        y = (xin - shift) / sc;
        l = -ls;
    } else {
        y = xin * sc + shift;
        l = ls;
    }
}

// gradients of one element of the affine autoregressive layer (K25, `affine_ar_backward_kernel`) given the incoming
// gradients g_y of its output and g_l of its row's logabsdet: scale = softplus(u) + 1e-3 with d scale / d u =
// sigmoid(u), exactly 1 where softplus1 returns u.  `other` is the layer's input x in the forward direction and
// its OUTPUT in the inverse direction (x = (y - shift) / scale: d x / d scale = -x / scale).
template <bool INVERSE>
__device__ __forceinline__ void affine_element_grad(float other, float u, float g_y, float g_l, float& g_x, float& g_u,
                                                    float& g_shift) {
#pragma clang fp contract(off)
    const float s = scale_of(u, NFA_SCALE_SOFTPLUS);
    const float e = expf(u);
    const float ds = u > 20.0f ? 1.0f : e / (1.0f + e);
    if (INVERSE) {
        g_x = g_y / s;
        g_shift = -g_x;
        g_u = (-g_x * other - g_l / s) * ds;
    } else {
        g_x = g_y * s;
        g_shift = g_y;
        g_u = (g_y * other + g_l / s) * ds;
    }
}

}  // namespace nfa
