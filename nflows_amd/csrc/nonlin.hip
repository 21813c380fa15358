// K18: the elementwise nonlinearity transforms (reference: transforms/nonlinearities.py -- Exp, Tanh, LogTanh, LeakyReLU,
// Sigmoid / Logit, CauchyCDF / CauchyCDFInverse) on a float32 [B, N] view, N = everything but the batch dimension.
//
// One launch reads the tensor once, writes the outputs once and writes the B row sums of the log-determinant's terms (the
// reference: six or seven stock launches over [B, N] and a reduction).  The per-element arithmetic is nonlin_math.hpp --
// float64 from the float32 element, every output rounded once --; who
// visits which element and the order of every sum is plan_row_sum (launch_plan.hpp), a function of (B, N) only:
//   * N <= 2048: a workgroup takes R whole rows as ONE contiguous range (float4 lanes where the range starts on a float4,
//     scalar lanes for what is left of it), leaves every element's float64 term in LDS, and `group` lanes add a row's terms -- lane g the terms g, g + group, ... in order, then a shuffle tree;
//   * N > 2048: a row is cut into pieces, one workgroup each; a lane adds its elements' terms in float64 in order, the
//     lanes are merged in a shuffle tree per wave and the four waves in wave order; with more than one piece the piece
//     sums go to a float64 workspace and a second small launch adds them in piece order.
// Every row sum is rounded ONCE.  No atomics on data: the same input gives the same bits on every run, and a row's result
// depends on that row, N and the batch's plan only.
//
// Sigmoid's temperature is read from the module's [1] tensor by every workgroup; nothing is packed or cached.  Elements
// outside a map's domain set NFA_STATUS_OUTSIDE_DOMAIN in the status word (one atomicOr per lane that saw one).
//
// The backward kernel walks the same plan: grad_in = g_out * dy/dx + g_lad[row] * dterm/dx, and for a learnable
// temperature one float64 partial per workgroup, folded by a single workgroup in a fixed order and rounded once.
#include "common.hpp"
#include "nonlin_math.hpp"
#include "row_sum.hpp"   // the row sums' device code, shared with K20

namespace nfa {
namespace {

struct NonlinArgs {
    const float* x;
    const float* temperature;
    float* out;          // forward: outputs; backward: grad_inputs
    float* lad;
    double* ws;          // forward: piece sums [B][pieces]; backward: temperature partials [workgroups]
    int32_t* status;
    const float* g_out;  // backward
    const float* g_lad;
    int64_t batch, n, piece;
    double p0, p1, p2, scale;
    int rows, group, pieces, accumulate;
    FastDiv div_n;
};

__device__ __forceinline__ void nonlin_put_lad(const NonlinArgs& p, int64_t row, double sum) {
    const float v = (float)(sum * p.scale);
    p.lad[row] = p.accumulate ? p.lad[row] + v : v;
}

template <int KIND, bool INVERSE, int V>
__global__ void __launch_bounds__(kBlock) nonlin_kernel(const NonlinArgs p) {
    __shared__ double s_c[kRowSumTile];
    __shared__ double s_w[kBlock / kWave];
    const int tid = threadIdx.x;
    const NonlinConst k = nonlin_constants(KIND, p.p0, p.p1, p.p2, KIND == NFA_NONLIN_SIGMOID ? p.temperature[0] : 0.0f);
    int bad = 0;
    if (p.rows > 0) {   // ---- whole rows, one contiguous range (workgroup-uniform branch)
        const int64_t row0 = (int64_t)blockIdx.x * p.rows;
        const int n = (int)p.n;
        const int rows = (p.batch - row0) < p.rows ? (int)(p.batch - row0) : p.rows;
        const int count = rows * n;
        const float* src = p.x + row0 * p.n;
        float* dst = p.out + row0 * p.n;
        const int body = V == 4 ? (count & ~3) : count;
        for (int i = tid * V; i < body; i += kBlock * V) {
            float v[V], o[V];
            rowsum_load<V>(src + i, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                double y;
                bad |= nonlin_eval<KIND, INVERSE>(v[j], k, y, s_c[i + j]);
                o[j] = (float)y;
            }
            rowsum_store<V>(dst + i, o);
        }
        if (V == 4 && body + tid < count) {   // what is left of a range that is no whole number of float4s
            double y;
            bad |= nonlin_eval<KIND, INVERSE>(src[body + tid], k, y, s_c[body + tid]);
            dst[body + tid] = (float)y;
        }
        __syncthreads();
        rowsum_rows(s_c, rows, n, p.group, tid, [&](int r, double sum) { nonlin_put_lad(p, row0 + r, sum); });
    } else {   // ---- one piece of one row
        const int64_t row = (int64_t)blockIdx.x / p.pieces;
        const int piece = (int)((int64_t)blockIdx.x - row * p.pieces);
        const int64_t c0 = (int64_t)piece * p.piece;
        const int64_t len = (p.n - c0) < p.piece ? (p.n - c0) : p.piece;
        const float* src = p.x + row * p.n + c0;
        float* dst = p.out + row * p.n + c0;
        double acc = 0.0;
        for (int64_t i = (int64_t)tid * V; i < len; i += kBlock * V) {
            float v[V], o[V];
            rowsum_load<V>(src + i, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                double y, c;
                bad |= nonlin_eval<KIND, INVERSE>(v[j], k, y, c);
                o[j] = (float)y;
                acc += c;
            }
            rowsum_store<V>(dst + i, o);
        }
        const double total = rowsum_block_sum(acc, s_w, tid);
        if (tid == 0) {
            if (p.pieces == 1) nonlin_put_lad(p, row, total);
            else p.ws[row * p.pieces + piece] = total;
        }
    }
    if (bad && p.status) atomicOr(p.status, bad);
}

// the pieces of a row, in piece order
__global__ void __launch_bounds__(kBlock) nonlin_fold_kernel(const NonlinArgs p) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= p.batch) return;
    nonlin_put_lad(p, row, rowsum_pieces(p.ws, row, p.pieces));
}

template <int KIND, bool INVERSE, int V>
__global__ void __launch_bounds__(kBlock) nonlin_backward_kernel(const NonlinArgs p) {
    __shared__ double s_w[kBlock / kWave];
    const int tid = threadIdx.x;
    const NonlinConst k = nonlin_constants(KIND, p.p0, p.p1, p.p2, KIND == NFA_NONLIN_SIGMOID ? p.temperature[0] : 0.0f);
    const bool want_t = KIND == NFA_NONLIN_SIGMOID && p.ws != nullptr;
    double acc = 0.0;
    if (p.rows > 0) {
        const int64_t row0 = (int64_t)blockIdx.x * p.rows;
        const int n = (int)p.n;
        const int rows = (p.batch - row0) < p.rows ? (int)(p.batch - row0) : p.rows;
        const int count = rows * n;
        const int64_t base = row0 * p.n;
        const int body = V == 4 ? (count & ~3) : count;
        for (int i = tid * V; i < body; i += kBlock * V) {
            float v[V], g[V], o[V];
            rowsum_load<V>(p.x + base + i, v);
            rowsum_load<V>(p.g_out + base + i, g);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float gl = p.g_lad[row0 + (int)fastdiv((uint32_t)(i + j), p.div_n)];
                double dy, dc, dy_t, dc_t;
                nonlin_grad<KIND, INVERSE>(v[j], k, dy, dc, dy_t, dc_t);
                o[j] = (float)((double)g[j] * dy + (double)gl * dc);
                if (want_t) acc += (double)g[j] * dy_t + (double)gl * dc_t;
            }
            rowsum_store<V>(p.out + base + i, o);
        }
        if (V == 4 && body + tid < count) {
            const int i = body + tid;
            const float gl = p.g_lad[row0 + (int)fastdiv((uint32_t)i, p.div_n)], g = p.g_out[base + i];
            double dy, dc, dy_t, dc_t;
            nonlin_grad<KIND, INVERSE>(p.x[base + i], k, dy, dc, dy_t, dc_t);
            p.out[base + i] = (float)((double)g * dy + (double)gl * dc);
            if (want_t) acc += (double)g * dy_t + (double)gl * dc_t;
        }
    } else {
        const int64_t row = (int64_t)blockIdx.x / p.pieces;
        const int piece = (int)((int64_t)blockIdx.x - row * p.pieces);
        const int64_t c0 = (int64_t)piece * p.piece;
        const int64_t len = (p.n - c0) < p.piece ? (p.n - c0) : p.piece;
        const int64_t base = row * p.n + c0;
        const float gl = p.g_lad[row];
        for (int64_t i = (int64_t)tid * V; i < len; i += kBlock * V) {
            float v[V], g[V], o[V];
            rowsum_load<V>(p.x + base + i, v);
            rowsum_load<V>(p.g_out + base + i, g);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                double dy, dc, dy_t, dc_t;
                nonlin_grad<KIND, INVERSE>(v[j], k, dy, dc, dy_t, dc_t);
                o[j] = (float)((double)g[j] * dy + (double)gl * dc);
                if (want_t) acc += (double)g[j] * dy_t + (double)gl * dc_t;
            }
            rowsum_store<V>(p.out + base + i, o);
        }
    }
    if (want_t) {   // (workgroup-uniform)
        const double total = rowsum_block_sum(acc, s_w, tid);
        if (tid == 0) p.ws[blockIdx.x] = total;
    }
}

struct NonlinFoldArgs {
    const double* partials;
    float* out;
    int64_t count;
};

// the workgroups' temperature partials -> one number: lane l adds partials l, l + 256, ... in order, then the lanes
__global__ void __launch_bounds__(kBlock) nonlin_temperature_fold_kernel(const NonlinFoldArgs p) {
    __shared__ double s_w[kBlock / kWave];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < p.count; i += kBlock) acc += p.partials[i];
    const double total = rowsum_block_sum(acc, s_w, threadIdx.x);
    if (threadIdx.x == 0) p.out[0] = (float)total;
}

template <int KIND, bool BACKWARD>
int nonlin_dispatch(bool inverse, bool wide, dim3 grid, hipStream_t st, const NonlinArgs& p) {
    void (*kern)(NonlinArgs);
    if (BACKWARD)
        kern = inverse ? (wide ? nonlin_backward_kernel<KIND, true, 4> : nonlin_backward_kernel<KIND, true, 1>)
                       : (wide ? nonlin_backward_kernel<KIND, false, 4> : nonlin_backward_kernel<KIND, false, 1>);
    else
        kern = inverse ? (wide ? nonlin_kernel<KIND, true, 4> : nonlin_kernel<KIND, true, 1>)
                       : (wide ? nonlin_kernel<KIND, false, 4> : nonlin_kernel<KIND, false, 1>);
    return launch_kernel(kern, grid, dim3(kBlock), 0, st, p, 0, false);
}

template <bool BACKWARD>
int nonlin_launch(const float* inputs, const float* temperature, const float* g_out, const float* g_lad, float* outputs,
                  float* lad, float* grad_temperature, void* workspace, int32_t* status, int64_t batch, int64_t n, int kind,
                  double p0, double p1, double p2, int flags, void* stream) {
    if (flags & ~(BACKWARD ? NFA_FLAG_INVERSE : (NFA_FLAG_INVERSE | NFA_FLAG_ACCUMULATE_LOGABSDET))) return NFA_ERR_INVALID_ARGUMENT;
    if (batch < 0 || n < 1) return NFA_ERR_INVALID_ARGUMENT;
    if (kind < NFA_NONLIN_EXP || kind > NFA_NONLIN_CAUCHY_CDF) return NFA_ERR_INVALID_ARGUMENT;
    if (kind == NFA_NONLIN_LOG_TANH && !(p0 > 0.0 && p1 > 0.0 && p2 > 0.0)) return NFA_ERR_INVALID_ARGUMENT;
    if (kind == NFA_NONLIN_LEAKY_RELU && !(p0 > 0.0)) return NFA_ERR_INVALID_ARGUMENT;
    if (kind == NFA_NONLIN_SIGMOID && !(p0 >= 0.0 && p0 < 0.5)) return NFA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return NFA_OK;
    if (!inputs || !outputs || (kind == NFA_NONLIN_SIGMOID && !temperature)) return NFA_ERR_INVALID_ARGUMENT;
    if (BACKWARD ? (!g_out || !g_lad) : !lad) return NFA_ERR_INVALID_ARGUMENT;
    const RowSumPlan plan = plan_row_sum(batch, n);
    if (plan.groups > 0x7fffffff) return NFA_ERR_UNSUPPORTED;
    const bool want_t = BACKWARD && kind == NFA_NONLIN_SIGMOID && grad_temperature;
    if (!workspace && (want_t || (!BACKWARD && plan.pieces > 1))) return NFA_ERR_INVALID_ARGUMENT;
    const bool inverse = (flags & NFA_FLAG_INVERSE) != 0;
    NonlinArgs p;
    p.x = inputs;
    p.temperature = temperature;
    p.out = outputs;
    p.lad = lad;
    p.ws = (BACKWARD && !want_t) ? nullptr : (double*)workspace;
    p.status = status;
    p.g_out = g_out;
    p.g_lad = g_lad;
    p.batch = batch;
    p.n = n;
    p.piece = plan.piece;
    p.p0 = p0;
    p.p1 = p1;
    p.p2 = p2;
    p.scale = nonlin_row_scale(kind, inverse, p0);
    p.rows = plan.rows;
    p.group = plan.group;
    p.pieces = plan.pieces;
    p.accumulate = (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0;
    p.div_n = make_fastdiv((uint32_t)(plan.rows > 0 ? n : 1));
    const bool wide = plan.vec4 && aligned16(inputs) && aligned16(outputs) && (!BACKWARD || aligned16(g_out));
    const dim3 grid((unsigned)plan.groups);
    const hipStream_t st = (hipStream_t)stream;
    int rc;
    switch (kind) {
        case NFA_NONLIN_EXP: rc = nonlin_dispatch<NFA_NONLIN_EXP, BACKWARD>(inverse, wide, grid, st, p); break;
        case NFA_NONLIN_TANH: rc = nonlin_dispatch<NFA_NONLIN_TANH, BACKWARD>(inverse, wide, grid, st, p); break;
        case NFA_NONLIN_LOG_TANH: rc = nonlin_dispatch<NFA_NONLIN_LOG_TANH, BACKWARD>(inverse, wide, grid, st, p); break;
        case NFA_NONLIN_LEAKY_RELU: rc = nonlin_dispatch<NFA_NONLIN_LEAKY_RELU, BACKWARD>(inverse, wide, grid, st, p); break;
        case NFA_NONLIN_SIGMOID: rc = nonlin_dispatch<NFA_NONLIN_SIGMOID, BACKWARD>(inverse, wide, grid, st, p); break;
        default: rc = nonlin_dispatch<NFA_NONLIN_CAUCHY_CDF, BACKWARD>(inverse, wide, grid, st, p); break;
    }
    if (rc != NFA_OK) return rc;
    if (!BACKWARD && plan.pieces > 1)
        return launch_kernel(nonlin_fold_kernel, dim3((unsigned)((batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, p, 0, false);
    if (want_t) {
        NonlinFoldArgs f;
        f.partials = (const double*)workspace;
        f.out = grad_temperature;
        f.count = plan.groups;
        return launch_kernel(nonlin_temperature_fold_kernel, dim3(1), dim3(kBlock), 0, st, f, 0, false);
    }
    return NFA_OK;
}

}  // namespace
}  // namespace nfa

extern "C" int nfa_nonlin_pieces(int64_t batch, int64_t n) {
    return nfa::plan_row_sum(batch, n).groups > 0 ? nfa::plan_row_sum(batch, n).pieces : 0;
}

extern "C" size_t nfa_nonlin_workspace_bytes(int64_t batch, int64_t n) {
    const nfa::RowSumPlan plan = nfa::plan_row_sum(batch, n);
    return plan.pieces > 1 ? (size_t)batch * plan.pieces * sizeof(double) : 0;
}

extern "C" size_t nfa_nonlin_backward_workspace_bytes(int64_t batch, int64_t n) {
    return (size_t)nfa::plan_row_sum(batch, n).groups * sizeof(double);
}

extern "C" int nfa_nonlin_f32(const float* inputs, const float* temperature, float* outputs, float* logabsdet, void* workspace,
                              int32_t* status, int64_t batch, int64_t n, int32_t kind, double p0, double p1, double p2,
                              int32_t flags, void* stream) {
    return nfa::nonlin_launch<false>(inputs, temperature, nullptr, nullptr, outputs, logabsdet, nullptr, workspace, status,
                                     batch, n, kind, p0, p1, p2, flags, stream);
}

extern "C" int nfa_nonlin_backward_f32(const float* inputs, const float* temperature, const float* grad_outputs,
                                       const float* grad_logabsdet, float* grad_inputs, float* grad_temperature,
                                       void* workspace, int64_t batch, int64_t n, int32_t kind, double p0, double p1,
                                       double p2, int32_t flags, void* stream) {
    return nfa::nonlin_launch<true>(inputs, temperature, grad_outputs, grad_logabsdet, grad_inputs, nullptr, grad_temperature,
                                    workspace, nullptr, batch, n, kind, p0, p1, p2, flags, stream);
}
