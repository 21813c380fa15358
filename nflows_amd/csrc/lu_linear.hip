// K16: the LU-parameterised linear layer (reference: transforms/lu.py, transforms/linear.py).
//   forward   y = L (U x) + b          inverse   x = U^-1 (L^-1 (y - b))   (substitution, never an inverse matrix)
//   L unit lower triangular, U upper triangular with diagonal softplus(unconstrained_upper_diag) + eps,
//   logabsdet = +- sum_i log U_ii, the same for every row.
// and the input gradients of both (the same two triangular steps with the factors transposed).
//
// The kernel reads the four parameter tensors as the module holds them (np.tril_indices / np.triu_indices order) and
// every workgroup expands them ONCE into one dense [DP, DP] LDS image (strict lower triangle = L, upper triangle and
// diagonal = U; DP = features rounded up to 16, the padding is the identity).  Nothing is packed or cached on the host.
//
// One lane owns one row.  A tile of R rows is read coalesced, stored column-major in LDS ([column][row], odd row
// stride) and each lane then walks ITS row through both triangular steps IN PLACE: U x ascending (row i needs x_j,
// j >= i, which are still the originals), L h descending.  No barrier is needed between the two steps.  The steps run
// on 16 x 16 register blocks: the factor's elements are LDS broadcasts (one ds_read_b128 feeds four FMAs), the row's
// own 16 values sit in registers.  A dot product is summed in blocks: 16 fused multiply-adds into a fresh partial, the
// partial added to the running total -- the error of a 128-term sum grows like 16 + 8 roundings, not 128 (the
// reference's library GEMM sums in blocks as well; K11 needed the same remedy).
// The result of a row depends on nothing but that row and the parameters: not on the batch, the tile or the grid.
//
// The diagonal and the log-determinant are computed in float64 from the float32 logits (features values per
// workgroup) and rounded once: logabsdet is ONE number per layer, so its error is not averaged over anything -- the
// correctly rounded value is the only one that is never further from the float64 result than another float32 evaluation.
//
// K19: the same layer over the channel dimension of a contiguous [B, C, H, W] tensor (reference: transforms/conv.py,
// OneByOneConvolution) is a second addressing mode of this kernel (NCHW = true).  A "row" is a pixel g in [0, B HW),
// b = g / HW, p = g % HW; its element c sits at b C HW + perm[c] HW + p.  A lane still owns one row, so in NCHW it
// loads and stores its own column of the tile channel by channel: the lanes of a wave touch consecutive addresses of one
// plane, and the coalesced read already IS the column-major tile -- no transposition in either direction, the channel
// permutation is "read plane perm[c]".  logabsdet is one value per image, +- HW sum_i log U_ii (float64, rounded once),
// written by the lane that owns the image's pixel 0.  Everything between load and store is K16's code.
#include "common.hpp"
#include "lu_tri.hpp"   // tri_apply, expand_tri_image, softplus_f64, kLuBlk (shared with K24)

namespace nfa {
namespace {

constexpr int kLuMaxFeatures = 128;

enum LuMode { kLuForward = 0, kLuInverse = 1, kLuForwardGrad = 2, kLuInverseGrad = 3 };

struct LuArgs {
    const float* x;
    const float* lower;
    const float* upper;
    const float* udiag;
    const float* bias;
    const int64_t* perm;
    const int64_t* scatter;
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;   // rows: the [batch, features] rows of K16, the batch * height * width pixels of K19
    int64_t hw;      // K19: height * width
    double eps;
    int D, DP, R, RS;
    int accumulate;
    FastDiv div_D, div_DP;
};

// LDS image (offsets in floats from a 16-byte aligned base):
//   double logd[DP] | float M[DP*DP] | float bias[DP] | int perm[DP] | int scatter[DP] | float lad | float tile[DP*RS]
inline size_t lu_lds_bytes(int DP, int R) {
    return (size_t)4 * (2 * DP + DP * DP + 3 * DP + 4 + DP * (R + 1));
}

template <int MODE, bool NCHW>
__global__ void __launch_bounds__(kBlock) lu_linear_kernel(const LuArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = a.D, DP = a.DP, R = a.R, RS = a.RS;
    double* s_logd = reinterpret_cast<double*>(lds);
    float* s_M = lds + 2 * DP;
    float* s_bias = s_M + DP * DP;
    int* s_perm = reinterpret_cast<int*>(s_bias + DP);
    int* s_scat = s_perm + DP;
    float* s_lad = reinterpret_cast<float*>(s_scat + DP);
    float* s_tile = s_lad + 4;
    const int tid = threadIdx.x;
    constexpr bool kTransposed = (MODE == kLuForwardGrad || MODE == kLuInverseGrad);
    constexpr bool kHasBias = (MODE == kLuForward || MODE == kLuInverse);

    // ---- the layer's parameters, once per workgroup
    int bad = 0;
    for (int c = tid; c < DP; c += R) {
        double d = 1.0;
        if (c < D) d = softplus_f64((double)a.udiag[c]) + a.eps;
        s_logd[c] = c < D ? log(d) : 0.0;
        s_M[c * DP + c] = (float)d;
        s_bias[c] = (kHasBias && c < D) ? a.bias[c] : 0.f;
        int p = c, s = c;
        if (c < D && a.perm) {
            const int64_t q = a.perm[c];
            if (q < 0 || q >= D) bad = NFA_STATUS_BAD_INDEX;
            p = (int)(q < 0 ? 0 : (q >= D ? D - 1 : q));
        }
        if (c < D && a.scatter) {
            const int64_t q = a.scatter[c];
            if (q < 0 || q >= D) bad = NFA_STATUS_BAD_INDEX;
            s = (int)(q < 0 ? 0 : (q >= D ? D - 1 : q));
        }
        s_perm[c] = p;
        s_scat[c] = s;
    }
    expand_tri_image(s_M, a.lower, a.upper, D, DP, a.div_DP, kTransposed, tid, R);
    __syncthreads();
    if (tid == 0) {   // one fixed order, whatever the grid
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += s_logd[c];
        if (NCHW) s *= (double)a.hw;   // every pixel of an image contributes the same term
        s_lad[0] = (float)(MODE == kLuInverse ? -s : s);
    }
    __syncthreads();
    const float layer_lad = s_lad[0];
    const int nb = DP / kLuBlk;

    const int64_t num_tiles = (a.batch + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int rows = (int)((a.batch - row0) < R ? (a.batch - row0) : R);
        // K19: this lane's pixel -- image b, position p; element c at pix + plane * hw (64-bit: B C HW may pass 2^31)
        int64_t img = 0, pix = 0;
        bool first_pixel = false;
        if (NCHW && tid < rows) {
            img = (row0 + tid) / a.hw;
            const int64_t p = (row0 + tid) - img * a.hw;
            first_pixel = p == 0;
            pix = img * D * a.hw + p;
        }
        if (NCHW) {
            // ---- channel by channel: the wave reads consecutive pixels of plane perm[c] into column c of the tile
            if (tid < rows) {
#pragma unroll 4
                for (int c = 0; c < D; ++c) {
                    float val = a.x[pix + s_perm[c] * a.hw];
                    if (MODE == kLuInverse) val -= s_bias[c];
                    s_tile[c * RS + tid] = val;
                }
            }
        } else {
            const float* src = a.x + row0 * D;
            // ---- coalesced read of rows * D floats -> column-major tile (gather through in_perm, minus the bias going back)
            for (int e = tid; e < rows * D; e += R) {
                const int r = (int)fastdiv((uint32_t)e, a.div_D);
                const int c = e - r * D;
                float val = src[r * D + s_perm[c]];
                if (MODE == kLuInverse) val -= s_bias[c];
                s_tile[c * RS + r] = val;
            }
        }
        for (int e = tid; e < (DP - D) * R; e += R) {   // identity padding: zeros stay zeros
            const int c = D + e / R;
            s_tile[c * RS + (e - (c - D) * R)] = 0.f;
        }
        if (tid >= rows)
            for (int c = 0; c < D; ++c) s_tile[c * RS + tid] = 0.f;   // rows past the batch: computed, never stored
        __syncthreads();
        float* col = s_tile + tid;
        if (MODE == kLuForward) {
            tri_apply<true, false, false>(s_M, DP, nb, col, RS);    // h = U x
            tri_apply<false, true, false>(s_M, DP, nb, col, RS);    // y = L h
        } else if (MODE == kLuInverse) {
            tri_apply<false, true, true>(s_M, DP, nb, col, RS);     // z = L^-1 (y - b)
            tri_apply<true, false, true>(s_M, DP, nb, col, RS);     // x = U^-1 z
        } else if (MODE == kLuForwardGrad) {                        // image = (L U)^T: upper = L^T (unit), lower = U^T
            tri_apply<true, true, false>(s_M, DP, nb, col, RS);     // gh = L^T gy
            tri_apply<false, false, false>(s_M, DP, nb, col, RS);   // gx = U^T gh
        } else {
            tri_apply<false, false, true>(s_M, DP, nb, col, RS);    // gz = U^-T gx
            tri_apply<true, true, true>(s_M, DP, nb, col, RS);      // gy = L^-T gz
        }
        __syncthreads();
        if (NCHW) {
            if (tid < rows) {
#pragma unroll 4
                for (int c = 0; c < D; ++c) {
                    float val = s_tile[c * RS + tid];
                    if (MODE == kLuForward) val += s_bias[c];
                    a.out[pix + s_scat[c] * a.hw] = val;
                }
            }
            if (kHasBias && a.lad && first_pixel) {   // one value per image, from the lane that owns its pixel 0
                float* l = a.lad + img;
                *l = a.accumulate ? *l + layer_lad : layer_lad;
            }
        } else {
            float* dst = a.out + row0 * D;
            for (int e = tid; e < rows * D; e += R) {
                const int r = (int)fastdiv((uint32_t)e, a.div_D);
                const int c = e - r * D;
                float val = s_tile[c * RS + r];
                if (MODE == kLuForward) val += s_bias[c];
                dst[r * D + s_scat[c]] = val;
            }
            if (kHasBias && a.lad && tid < rows) {
                float* l = a.lad + row0 + tid;
                *l = a.accumulate ? *l + layer_lad : layer_lad;
            }
        }
        __syncthreads();
    }
    if (bad && a.status) atomicOr(a.status, bad);
}

int lu_launch(int mode, const float* inputs, const float* lower, const float* upper, const float* udiag,
              const float* bias, const int64_t* in_perm, const int64_t* out_scatter, float* outputs, float* logabsdet,
              int32_t* status, int64_t batch, int32_t features, double eps, int accumulate, void* stream,
              int64_t hw = 0) {   // hw > 0: K19, `batch` images of `features` planes of hw pixels
    if (batch < 0 || features < 1) return NFA_ERR_INVALID_ARGUMENT;
    if (features < 2 || features > kLuMaxFeatures) return NFA_ERR_UNSUPPORTED;
    if (!(eps >= 0.0)) return NFA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return NFA_OK;
    const bool has_bias = mode == kLuForward || mode == kLuInverse;
    if (!inputs || !lower || !upper || !udiag || !outputs) return NFA_ERR_INVALID_ARGUMENT;
    if (has_bias && (!bias || !logabsdet)) return NFA_ERR_INVALID_ARGUMENT;
    const int D = features, DP = (D + kLuBlk - 1) / kLuBlk * kLuBlk;
    if (hw > 0) batch *= hw;   // from here on: rows
    const int cus = device_cu_count();
    // rows per workgroup (= its lanes): the most waves a CU can hold under the 160 KB of LDS, more workgroups on a
    // tie (their load / compute / store phases overlap), and small enough that every CU gets a tile
    int R = 64, best = 0;
    for (int r = kBlock; r >= 64; r -= 64) {
        const size_t lds = lu_lds_bytes(DP, r);
        if (lds > (size_t)kCuLds) continue;
        int blocks = (int)((size_t)kCuLds / lds);
        if (blocks > 8) blocks = 8;
        int waves = blocks * (r / 64);
        if (waves > 16) waves = 16;
        if (waves > best || (waves == best && r < R)) {
            best = waves;
            R = r;
        }
    }
    if (best == 0) return NFA_ERR_UNSUPPORTED;
    while (R > 64 && (batch + R - 1) / R < (int64_t)cus) R -= 64;
    const size_t lds = lu_lds_bytes(DP, R);
    int per_cu = (int)((size_t)kCuLds / lds);
    if (per_cu > 8) per_cu = 8;
    LuArgs a;
    a.x = inputs;
    a.lower = lower;
    a.upper = upper;
    a.udiag = udiag;
    a.bias = bias;
    a.perm = in_perm;
    a.scatter = out_scatter;
    a.out = outputs;
    a.lad = logabsdet;
    a.status = status;
    a.batch = batch;
    a.hw = hw;
    a.eps = eps;
    a.D = D;
    a.DP = DP;
    a.R = R;
    a.RS = R + 1;
    a.accumulate = accumulate;
    a.div_D = make_fastdiv((uint32_t)D);
    a.div_DP = make_fastdiv((uint32_t)DP);
    const int64_t tiles = (batch + R - 1) / R;
    int64_t g = (int64_t)cus * per_cu;
    if (g > tiles) g = tiles;
    void (*const kerns[2][4])(LuArgs) = {
        {lu_linear_kernel<kLuForward, false>, lu_linear_kernel<kLuInverse, false>,
         lu_linear_kernel<kLuForwardGrad, false>, lu_linear_kernel<kLuInverseGrad, false>},
        {lu_linear_kernel<kLuForward, true>, lu_linear_kernel<kLuInverse, true>,
         lu_linear_kernel<kLuForwardGrad, true>, lu_linear_kernel<kLuInverseGrad, true>}};
    void (*kern)(LuArgs) = kerns[hw > 0][mode];
    return launch_kernel(kern, dim3((unsigned)g), dim3((unsigned)R), lds, (hipStream_t)stream, a, kCuLds, false);
}

}  // namespace
}  // namespace nfa

extern "C" int nfa_lu_linear_f32(const float* inputs, const float* lower_entries, const float* upper_entries,
                                 const float* unconstrained_upper_diag, const float* bias, const int64_t* in_perm,
                                 const int64_t* out_scatter, float* outputs, float* logabsdet, int32_t* status,
                                 int64_t batch, int32_t features, double eps, int32_t flags, void* stream) {
    if (flags & ~(NFA_FLAG_INVERSE | NFA_FLAG_ACCUMULATE_LOGABSDET)) return NFA_ERR_INVALID_ARGUMENT;
    return nfa::lu_launch((flags & NFA_FLAG_INVERSE) ? nfa::kLuInverse : nfa::kLuForward, inputs, lower_entries,
                          upper_entries, unconstrained_upper_diag, bias, in_perm, out_scatter, outputs, logabsdet,
                          status, batch, features, eps, (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0, stream);
}

extern "C" int nfa_lu_linear_backward_f32(const float* grad_outputs, const float* lower_entries,
                                          const float* upper_entries, const float* unconstrained_upper_diag,
                                          const int64_t* in_perm, const int64_t* out_scatter, float* grad_inputs,
                                          int32_t* status, int64_t batch, int32_t features, double eps, int32_t flags,
                                          void* stream) {
    if (flags & ~NFA_FLAG_INVERSE) return NFA_ERR_INVALID_ARGUMENT;
    return nfa::lu_launch((flags & NFA_FLAG_INVERSE) ? nfa::kLuInverseGrad : nfa::kLuForwardGrad, grad_outputs,
                          lower_entries, upper_entries, unconstrained_upper_diag, nullptr,
                          /*gather=*/out_scatter, /*scatter=*/in_perm,   // the transposes of the forward call's two
                          grad_inputs, nullptr, status, batch, features, eps, 0, stream);
}

// K19: the layer over the channels of [batch, channels, height, width]; channel_perm is the module's fixed permutation,
// gathered going forward (the layer sees inputs[:, channel_perm]) and scattered coming back.
extern "C" int nfa_lu_conv1x1_f32(const float* inputs, const float* lower_entries, const float* upper_entries,
                                  const float* unconstrained_upper_diag, const float* bias, const int64_t* channel_perm,
                                  float* outputs, float* logabsdet, int32_t* status, int64_t batch, int32_t channels,
                                  int32_t height, int32_t width, double eps, int32_t flags, void* stream) {
    if (flags & ~(NFA_FLAG_INVERSE | NFA_FLAG_ACCUMULATE_LOGABSDET)) return NFA_ERR_INVALID_ARGUMENT;
    if (height <= 0 || width <= 0) return NFA_ERR_INVALID_ARGUMENT;
    const bool inverse = (flags & NFA_FLAG_INVERSE) != 0;
    return nfa::lu_launch(inverse ? nfa::kLuInverse : nfa::kLuForward, inputs, lower_entries, upper_entries,
                          unconstrained_upper_diag, bias, inverse ? nullptr : channel_perm,
                          inverse ? channel_perm : nullptr, outputs, logabsdet, status, batch, channels, eps,
                          (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0, stream, (int64_t)height * width);
}

extern "C" int nfa_lu_conv1x1_backward_f32(const float* grad_outputs, const float* lower_entries,
                                           const float* upper_entries, const float* unconstrained_upper_diag,
                                           const int64_t* channel_perm, float* grad_inputs, int32_t* status,
                                           int64_t batch, int32_t channels, int32_t height, int32_t width, double eps,
                                           int32_t flags, void* stream) {
    if (flags & ~NFA_FLAG_INVERSE) return NFA_ERR_INVALID_ARGUMENT;
    if (height <= 0 || width <= 0) return NFA_ERR_INVALID_ARGUMENT;
    const bool inverse = (flags & NFA_FLAG_INVERSE) != 0;
    return nfa::lu_launch(inverse ? nfa::kLuInverseGrad : nfa::kLuForwardGrad, grad_outputs, lower_entries,
                          upper_entries, unconstrained_upper_diag, nullptr,
                          /*gather=*/inverse ? channel_perm : nullptr, /*scatter=*/inverse ? nullptr : channel_perm,
                          grad_inputs, nullptr, status, batch, channels, eps, 0, stream, (int64_t)height * width);
}
