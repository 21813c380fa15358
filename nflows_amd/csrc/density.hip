// K20: the learned base densities (reference: distributions/normal.py -- DiagonalNormal, ConditionalDiagonalNormal --,
// nn/nde/made.py:328-353 -- MixtureOfGaussiansMADE.log_prob) as one launch that reads the operands once and writes the B
// float32 log-densities (the reference: four passes and two row sums for the diagonal normals, about fifteen tensor
// operations with [B, D, K] temporaries for the mixture).  The per-element arithmetic is density_math.hpp -- float64 from the
// float32 operands --; who visits which element is plan_row_sum (launch_plan.hpp), a function of the shape only, and the
// order of a row's float64 sum is row_sum.hpp, the code K18 uses.  A row's sum, - log_z, + the optional `add` term (the
// flow's logabsdet) is rounded ONCE.  No atomics: the same input gives the same bits on every run, and a row's result
// depends on that row and the batch's plan only.
//
//   "diag"  x [B, N]; means / log_stds: pointers with one row stride in elements (0: one shared row, DiagonalNormal; 2N: the
//           two halves of the encoder's [B, 2N] output read in place, ConditionalDiagonalNormal).  The backward is one
//           elementwise launch over the same plan that writes grad_x and, row by row at `grad_param_stride`, the two
//           parameter gradients (for the shared row the caller takes them from K17's column reduction of grad_x).
//   "mog"   x [B, D], outputs [B, D * K * 3] in the reference's interleaving (..., K, 3) = logit, mean, unconstrained std,
//           1 <= K <= 64.  A workgroup's elements are one contiguous range, so their 3K-float records are one contiguous
//           range of `outputs`: it goes through LDS (tile_load: float4 lanes on the 16-byte window) in sub-tiles of T
//           elements (plan_mog_tile), because a lane striding 12K bytes through global memory wastes the coalescer.  Lane l
//           takes the range's elements l, l + 256, ... whatever T is.  The backward walks the same ranges, overwrites the
//           sub-tile in LDS with the record's gradients and stores it the way it was loaded; no reduction but over k.
#include "common.hpp"
#include "density_math.hpp"
#include "row_sum.hpp"

namespace nfa {
namespace {

struct DensityArgs {
    const float* x;
    const float* means;      // diag        mog: outputs
    const float* log_stds;   // diag
    const float* add;        // forward: optional [B] term inside the sum
    const float* g;          // backward: grad_log_prob [B]
    float* out;              // forward: log_prob [B]; backward: grad_x
    float* g_means;          // backward, diag (may be null)       mog: grad_outputs
    float* g_log_stds;       // backward, diag (may be null)
    double* ws;              // forward: piece sums [B][pieces]
    int64_t batch, n, piece, param_stride, grad_param_stride;
    double log_z, epsilon;
    int rows, group, pieces, K, T;
    FastDiv div_n;
};

__device__ __forceinline__ void density_put(const DensityArgs& p, int64_t row, double sum) {
    p.out[row] = (float)((sum - p.log_z) + (p.add ? (double)p.add[row] : 0.0));
}

// the workgroup's range: `first` global element, `count` elements; rows regime: whole rows from row0, pieces: part of `row0`
struct DensityRange {
    int64_t first, count, row0, col0;
    int rows;
};

__device__ __forceinline__ DensityRange density_range(const DensityArgs& p) {
    DensityRange r;
    if (p.rows > 0) {
        r.row0 = (int64_t)blockIdx.x * p.rows;
        r.rows = (p.batch - r.row0) < p.rows ? (int)(p.batch - r.row0) : p.rows;
        r.col0 = 0;
        r.first = r.row0 * p.n;
        r.count = (int64_t)r.rows * p.n;
    } else {
        r.row0 = (int64_t)blockIdx.x / p.pieces;
        const int piece = (int)((int64_t)blockIdx.x - r.row0 * p.pieces);
        r.rows = 0;
        r.col0 = (int64_t)piece * p.piece;
        r.count = (p.n - r.col0) < p.piece ? (p.n - r.col0) : p.piece;
        r.first = r.row0 * p.n + r.col0;
    }
    return r;
}

// (row, column) of the range's element e
__device__ __forceinline__ void density_where(const DensityArgs& p, const DensityRange& r, int64_t e, int64_t& row, int64_t& col) {
    if (p.rows > 0) {
        const uint32_t q = fastdiv((uint32_t)e, p.div_n);   // e < kRowSumTile
        row = r.row0 + q;
        col = e - (int64_t)q * p.n;
    } else {
        row = r.row0;
        col = r.col0 + e;
    }
}

// the tail of both forward kernels: the rows' sums from the terms in LDS, or the piece's sum from the lanes' partial sums
__device__ __forceinline__ void density_finish(const DensityArgs& p, const DensityRange& r, const double* s_c, double* s_w,
                                               double acc, int tid) {
    if (p.rows > 0) {
        __syncthreads();
        rowsum_rows(s_c, r.rows, (int)p.n, p.group, tid, [&](int i, double sum) { density_put(p, r.row0 + i, sum); });
    } else {
        const double total = rowsum_block_sum(acc, s_w, tid);
        if (tid == 0) {
            if (p.pieces == 1) density_put(p, r.row0, total);
            else p.ws[blockIdx.x] = total;   // [row][piece]
        }
    }
}

template <int V>
__global__ void __launch_bounds__(kBlock) diag_normal_kernel(const DensityArgs p) {
    __shared__ double s_c[kRowSumTile];
    __shared__ double s_w[kBlock / kWave];
    const int tid = threadIdx.x;
    const DensityRange r = density_range(p);
    const float* src = p.x + r.first;
    // a lane takes four consecutive elements per pass, as one float4 (V == 4) or one by one: the same order either way
    const int64_t body = r.count & ~(int64_t)3;
    double acc = 0.0;
    for (int64_t i = (int64_t)tid * 4; i < body; i += kBlock * 4) {
        float v[4];
        if (V == 4) {
            rowsum_load<4>(src + i, v);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[i + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int64_t row, col;
            density_where(p, r, i + j, row, col);
            const int64_t at = row * p.param_stride + col;
            const double term = diag_normal_term(v[j], p.means[at], p.log_stds[at]);
            if (p.rows > 0) s_c[i + j] = term;
            else acc += term;
        }
    }
    if (body + tid < r.count) {   // what is left of a range that is no whole number of float4s
        const int64_t e = body + tid;
        int64_t row, col;
        density_where(p, r, e, row, col);
        const int64_t at = row * p.param_stride + col;
        const double term = diag_normal_term(src[e], p.means[at], p.log_stds[at]);
        if (p.rows > 0) s_c[e] = term;
        else acc += term;
    }
    density_finish(p, r, s_c, s_w, acc, tid);
}

// the pieces of a row, in piece order
__global__ void __launch_bounds__(kBlock) density_fold_kernel(const DensityArgs p) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= p.batch) return;
    density_put(p, row, rowsum_pieces(p.ws, row, p.pieces));
}

__global__ void __launch_bounds__(kBlock) diag_normal_backward_kernel(const DensityArgs p) {
    const int tid = threadIdx.x;
    const DensityRange r = density_range(p);
    for (int64_t e = tid; e < r.count; e += kBlock) {
        int64_t row, col;
        density_where(p, r, e, row, col);
        const int64_t at = row * p.param_stride + col;
        double gx, gls;
        diag_normal_grad(p.x[r.first + e], p.means[at], p.log_stds[at], (double)p.g[row], gx, gls);
        p.out[r.first + e] = (float)gx;
        const int64_t to = row * p.grad_param_stride + col;
        if (p.g_means) p.g_means[to] = (float)(-gx);
        if (p.g_log_stds) p.g_log_stds[to] = (float)gls;
    }
}

// BACKWARD: grad_outputs and grad_x; else the terms of the row sums
template <bool BACKWARD>
__global__ void __launch_bounds__(kBlock) mog_kernel(const DensityArgs p) {
    __shared__ double s_c[BACKWARD ? 1 : kRowSumTile];
    __shared__ double s_w[kBlock / kWave];
    extern __shared__ __align__(16) float s_tile[];   // mog_tile_bytes(T, K)
    const int tid = threadIdx.x;
    const DensityRange r = density_range(p);
    const int K = p.K, T = p.T, P = 3 * K;
    const float* src = p.means + r.first * P;
    double acc = 0.0;
    for (int64_t c = 0; c < r.count; c += T) {
        const int ne = (r.count - c) < T ? (int)(r.count - c) : T;
        __syncthreads();   // the previous sub-tile has been read (and, BACKWARD, stored)
        const int mis = tile_load(src + c * P, ne * P, s_tile, tid);
        __syncthreads();
        const int local = tid - (int)(c & (kBlock - 1));   // lane l takes the elements l, l + kBlock, ... whatever T is
        if (local >= 0 && local < ne) {
            const int64_t e = c + local;
            float* rec = s_tile + mis + local * P;
            if (BACKWARD) {
                int64_t row, col;
                density_where(p, r, e, row, col);
                p.out[r.first + e] = (float)mog_grad(p.x[r.first + e], rec, rec, K, p.epsilon, (double)p.g[row]);
            } else {
                const double term = mog_term(p.x[r.first + e], rec, K, p.epsilon);
                if (p.rows > 0) s_c[e] = term;
                else acc += term;
            }
        }
        if (BACKWARD) {
            __syncthreads();
            float* dst = p.g_means + (r.first + c) * P;
            if (tile_store_offset(dst) == mis) {   // (workgroup-uniform)
                tile_store(dst, ne * P, s_tile, tid);
            } else {
                for (int i = tid; i < ne * P; i += kBlock) dst[i] = s_tile[mis + i];
            }
        }
    }
    if (!BACKWARD) density_finish(p, r, s_c, s_w, acc, tid);
}

int density_plan(DensityArgs& p, int64_t batch, int64_t n, RowSumPlan& plan) {
    plan = plan_row_sum(batch, n);
    if (plan.groups < 1 || plan.groups > 0x7fffffff) return NFA_ERR_UNSUPPORTED;
    p.batch = batch;
    p.n = n;
    p.piece = plan.piece;
    p.rows = plan.rows;
    p.group = plan.group;
    p.pieces = plan.pieces;
    p.div_n = make_fastdiv((uint32_t)(plan.rows > 0 ? n : 1));
    return NFA_OK;
}

int density_fold(const DensityArgs& p, const RowSumPlan& plan, hipStream_t st) {
    if (plan.pieces <= 1) return NFA_OK;
    return launch_kernel(density_fold_kernel, dim3((unsigned)((p.batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, p, 0, false);
}

}  // namespace
}  // namespace nfa

using namespace nfa;

extern "C" size_t nfa_diag_normal_workspace_bytes(int64_t batch, int64_t n) {
    const RowSumPlan plan = plan_row_sum(batch, n);
    return plan.pieces > 1 ? (size_t)batch * plan.pieces * sizeof(double) : 0;
}

extern "C" size_t nfa_mog_workspace_bytes(int64_t batch, int64_t features) {
    return nfa_diag_normal_workspace_bytes(batch, features);
}

extern "C" int nfa_diag_normal_log_prob_f32(const float* inputs, const float* means, const float* log_stds, const float* add,
                                            float* log_prob, void* workspace, int64_t batch, int64_t n, int64_t param_stride,
                                            double log_z, void* stream) {
    if (batch < 0 || n < 1 || param_stride < 0 || (param_stride > 0 && param_stride < n)) return NFA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return NFA_OK;
    if (!inputs || !means || !log_stds || !log_prob) return NFA_ERR_INVALID_ARGUMENT;
    DensityArgs p = {};
    RowSumPlan plan;
    const int rc = density_plan(p, batch, n, plan);
    if (rc != NFA_OK) return rc;
    if (plan.pieces > 1 && !workspace) return NFA_ERR_INVALID_ARGUMENT;
    p.x = inputs;
    p.means = means;
    p.log_stds = log_stds;
    p.add = add;
    p.out = log_prob;
    p.ws = (double*)workspace;
    p.param_stride = param_stride;
    p.log_z = log_z;
    const hipStream_t st = (hipStream_t)stream;
    const bool wide = plan.vec4 && aligned16(inputs);
    const int rc2 = launch_kernel(wide ? diag_normal_kernel<4> : diag_normal_kernel<1>, dim3((unsigned)plan.groups), dim3(kBlock),
                                  0, st, p, 0, false);
    return rc2 != NFA_OK ? rc2 : density_fold(p, plan, st);
}

extern "C" int nfa_diag_normal_backward_f32(const float* inputs, const float* means, const float* log_stds,
                                            const float* grad_log_prob, float* grad_inputs, float* grad_means,
                                            float* grad_log_stds, int64_t batch, int64_t n, int64_t param_stride,
                                            int64_t grad_param_stride, void* stream) {
    if (batch < 0 || n < 1 || param_stride < 0 || (param_stride > 0 && param_stride < n)) return NFA_ERR_INVALID_ARGUMENT;
    if ((grad_means || grad_log_stds) && grad_param_stride < n) return NFA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return NFA_OK;
    if (!inputs || !means || !log_stds || !grad_log_prob || !grad_inputs) return NFA_ERR_INVALID_ARGUMENT;
    DensityArgs p = {};
    RowSumPlan plan;
    const int rc = density_plan(p, batch, n, plan);
    if (rc != NFA_OK) return rc;
    p.x = inputs;
    p.means = means;
    p.log_stds = log_stds;
    p.g = grad_log_prob;
    p.out = grad_inputs;
    p.g_means = grad_means;
    p.g_log_stds = grad_log_stds;
    p.param_stride = param_stride;
    p.grad_param_stride = grad_param_stride;
    return launch_kernel(diag_normal_backward_kernel, dim3((unsigned)plan.groups), dim3(kBlock), 0, (hipStream_t)stream, p, 0,
                         false);
}

static int mog_launch(bool backward, DensityArgs& p, int64_t batch, int64_t features, int32_t components, double epsilon,
                      void* workspace, void* stream) {
    if (batch < 0 || features < 1 || components < 1 || !(epsilon >= 0.0)) return NFA_ERR_INVALID_ARGUMENT;
    if (components > kMogMaxComponents) return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    if (!p.x || !p.means || !p.out || (backward ? (!p.g || !p.g_means) : false)) return NFA_ERR_INVALID_ARGUMENT;
    RowSumPlan plan;
    const int rc = density_plan(p, batch, features, plan);
    if (rc != NFA_OK) return rc;
    if (!backward && plan.pieces > 1 && !workspace) return NFA_ERR_INVALID_ARGUMENT;
    p.ws = (double*)workspace;
    p.K = components;
    p.T = plan_mog_tile(components);
    p.epsilon = epsilon;
    if (p.T < 1) return NFA_ERR_UNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    const int rc2 = launch_kernel(backward ? mog_kernel<true> : mog_kernel<false>, dim3((unsigned)plan.groups), dim3(kBlock),
                                  mog_tile_bytes(p.T, components), st, p, 0, false);
    if (rc2 != NFA_OK || backward) return rc2;
    return density_fold(p, plan, st);
}

extern "C" int nfa_mog_log_prob_f32(const float* inputs, const float* outputs, const float* add, float* log_prob,
                                    void* workspace, int64_t batch, int64_t features, int32_t components, double epsilon,
                                    void* stream) {
    DensityArgs p = {};
    p.x = inputs;
    p.means = outputs;
    p.add = add;
    p.out = log_prob;
    return mog_launch(false, p, batch, features, components, epsilon, workspace, stream);
}

extern "C" int nfa_mog_backward_f32(const float* inputs, const float* outputs, const float* grad_log_prob, float* grad_inputs,
                                    float* grad_outputs, int64_t batch, int64_t features, int32_t components, double epsilon,
                                    void* stream) {
    DensityArgs p = {};
    p.x = inputs;
    p.means = outputs;
    p.g = grad_log_prob;
    p.out = grad_inputs;
    p.g_means = grad_outputs;
    return mog_launch(true, p, batch, features, components, epsilon, nullptr, stream);
}
