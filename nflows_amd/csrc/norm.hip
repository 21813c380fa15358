// K17: the normalisation transforms (reference: transforms/normalization.py -- BatchNorm, ActNorm).
//
// Three kernel families over float32 [B, D] rows, 1 <= D <= 1024, all plain HIP C++:
//   * column reductions (the first kernels of this library that reduce OVER THE BATCH): per column the mean and the
//     unbiased variance, or the two sums  sum_b g[b, c]  and  sum_b g[b, c] * u[b, c]  of the backward pass;
//   * the per-column map  out[b, c] = a[c] * ((x[b, c] - m[c]) / s[c]) + t[c]  -- forward and inverse of both transforms --
//     and its input gradient (g * a) / s;
//   * the input gradient of BatchNorm with batch statistics.
//
// Layout.  Lanes run along columns.  D <= 256: a workgroup's 256 lanes are rl = 256 / D "row lanes" of D columns each, lane
// t = row lane t / D, column t % D, so the rl * D active lanes read rl consecutive rows as ONE contiguous range and a lane
// keeps its column for the whole kernel (its per-column constants stay in registers; D = 2 keeps all 256 lanes busy,
// D = 5 keeps 255).  D > 256: ceil(D / 256) column tiles of equal width (grid.y), one row per step.
//
// Reductions.  The batch is cut into S row slabs, S a function of (B, D) only (norm_slabs).  A lane accumulates in
// float64 around a shift (its first value): sum (x - K) and sum (x - K)^2 -- products of two float32 are exact in
// float64 --, turns them into (count, mean, M2), the row lanes of a workgroup are merged by Chan's pairwise formula in a
// fixed tree through LDS, and the slab's (mean, M2) go to the workspace.  A second small kernel folds the slabs of a column
// in a fixed order (64 interleaved lanes, then a tree) and rounds each statistic ONCE.  No atomics: the same input gives the same bits on every run.
//
// The map reads the module's tensors as they are and derives the per-column constants itself, once per workgroup, in
// float64 rounded once (weight = softplus(unconstrained_weight) + eps, sqrt(var + eps), exp(log_scale)); the
// log-determinant -- one number per call -- is summed in float64 in a fixed LDS tree and rounded once.  The element-wise
// expression is evaluated in exactly the written order (-ffp-contract=off, correctly rounded division): the reference's
// rounding sequence.  A row's result depends on that row and the parameters only.
#include "common.hpp"

namespace nfa {
namespace {

constexpr int kNormMaxFeatures = 1024;
constexpr int kNormUnroll = 4;          // independent row steps a lane has in flight
constexpr int kNormRowsPerLane = 32;    // a slab gives every row lane about this many rows ...
constexpr int kNormMaxGroups = 1024;    // ... until the grid has this many workgroups

struct NormShape {
    int col_tiles;   // grid.y
    int cw;          // columns per tile
    int rl;          // row lanes: rows a workgroup reads per step
};

inline NormShape norm_shape(int D) {
    NormShape s;
    s.col_tiles = (D + kBlock - 1) / kBlock;
    s.cw = (D + s.col_tiles - 1) / s.col_tiles;
    s.rl = s.col_tiles == 1 ? kBlock / D : 1;
    return s;
}

// The partition of the batch: rows per slab and the number of (non-empty) slabs.  Depends on (B, D) only.
inline void norm_slabs(int64_t B, int D, int64_t* rows_per_slab, int* slabs) {
    const NormShape sh = norm_shape(D);
    const int64_t target = (int64_t)sh.rl * kNormRowsPerLane;
    int64_t S = (B + target - 1) / target;
    const int64_t cap = kNormMaxGroups / sh.col_tiles;
    if (S > cap) S = cap;
    if (S < 1) S = 1;
    const int64_t rps = B > 0 ? (B + S - 1) / S : 1;
    *rows_per_slab = rps;
    *slabs = B > 0 ? (int)((B + rps - 1) / rps) : 1;
}

__device__ __forceinline__ double norm_softplus_f64(double u) {
    return u > 20.0 ? u : log1p(exp(u));   // F.softplus, beta = 1, threshold = 20
}

// lane -> (row lane, column); returns false for a lane without work
__device__ __forceinline__ bool norm_lane(int tid, int D, int cw, int rl, FastDiv div_D, int tile, int* rlane, int* col) {
    int r = 0, c = tid;
    if (rl > 1) {
        r = (int)fastdiv((uint32_t)tid, div_D);
        c = tid - r * D;
    }
    *rlane = r;
    *col = tile * cw + c;
    return r < rl && c < cw && *col < D;
}

__device__ __forceinline__ int norm_index(const int64_t* map, int c, int D, int* bad) {
    if (!map) return c;
    const int64_t q = map[c];
    if (q < 0 || q >= D) *bad = NFA_STATUS_BAD_INDEX;
    return (int)(q < 0 ? 0 : (q >= D ? D - 1 : q));
}

// ------------------------------------------------------------------------------------------ column reductions
struct NormReduceArgs {
    const float* a;         // statistics: x; sums: g
    const float* b;         // sums: u
    const int64_t* amap;    // sums: lane column c reads a[:, amap[c]] (NULL: c)
    const int64_t* bmap;
    double* ws;             // [slabs][2][D]
    int32_t* status;
    int64_t batch, rows_per_slab;
    int D, cw, rl;
    FastDiv div_D;
};

enum NormReduce { kNormStats = 0, kNormSums = 1 };

// (count, mean, M2) of a set and of another one -> of their union (Chan et al.); an empty side changes nothing
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& qa, double nb, double mb, double qb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb;
        ma = mb;
        qa = qb;
        return;
    }
    const double n = na + nb, delta = mb - ma, f = nb / n;
    ma = ma + delta * f;
    qa = qa + qb + delta * delta * (na * f);
    na = n;
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) norm_partial_kernel(const NormReduceArgs p) {
    __shared__ double s_n[kBlock], s_0[kBlock], s_1[kBlock];
    const int tid = threadIdx.x, D = p.D, rl = p.rl;
    int rlane, col, bad = 0;
    const bool active = norm_lane(tid, D, p.cw, rl, p.div_D, blockIdx.y, &rlane, &col);
    const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_slab;
    const int64_t r1 = (r0 + p.rows_per_slab) < p.batch ? (r0 + p.rows_per_slab) : p.batch;
    double n = 0.0, v0 = 0.0, v1 = 0.0;
    if (active) {
        const int ca = MODE == kNormSums ? norm_index(p.amap, col, D, &bad) : col;
        const int cb = MODE == kNormSums ? norm_index(p.bmap, col, D, &bad) : col;
        double shift = 0.0;
        if (MODE == kNormStats && r0 + rlane < r1) shift = (double)p.a[(r0 + rlane) * D + ca];
        for (int64_t r = r0 + rlane; r < r1; r += (int64_t)rl * kNormUnroll) {
            float xa[kNormUnroll], xb[kNormUnroll];
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) {
                const int64_t ru = r + (int64_t)u * rl;
                const bool in = ru < r1;
                xa[u] = in ? p.a[ru * D + ca] : 0.f;
                xb[u] = (MODE == kNormSums && in) ? p.b[ru * D + cb] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) {
                if (r + (int64_t)u * rl < r1) {
                    if (MODE == kNormStats) {
                        const double d = (double)xa[u] - shift;
                        n += 1.0;
                        v0 += d;
                        v1 += d * d;
                    } else {
                        v0 += (double)xa[u];
                        v1 += (double)xa[u] * (double)xb[u];
                    }
                }
            }
        }
        if (MODE == kNormStats && n > 0.0) {   // shifted sums -> (mean, M2)
            const double m = v0 / n;
            v1 = v1 - v0 * m;
            v0 = shift + m;
        }
    }
    s_n[tid] = n;
    s_0[tid] = v0;
    s_1[tid] = v1;
    __syncthreads();
    int top = 1;
    while (top < rl) top <<= 1;
    for (int stride = top >> 1; stride >= 1; stride >>= 1) {   // the row lanes of a column, a fixed tree
        if (active && rlane < stride && rlane + stride < rl) {
            const int other = tid + stride * D;
            if (MODE == kNormStats) {
                chan_merge(n, v0, v1, s_n[other], s_0[other], s_1[other]);
            } else {
                v0 += s_0[other];
                v1 += s_1[other];
            }
            s_n[tid] = n;
            s_0[tid] = v0;
            s_1[tid] = v1;
        }
        __syncthreads();
    }
    if (active && rlane == 0) {
        double* w = p.ws + (int64_t)blockIdx.x * 2 * D;
        w[col] = v0;
        w[D + col] = v1;
    }
    if (bad && p.status) atomicOr(p.status, bad);
}

struct NormFinalArgs {
    const double* ws;
    float* mean;     // statistics
    float* var;
    double* sums;    // sums: [2][D]; statistics: NULL or [2][D] = (mean, var) before the rounding to float32
    int64_t batch, rows_per_slab;
    int D, slabs;
};

constexpr int kNormFinalCols = 4;                         // columns per workgroup of the fold
constexpr int kNormFinalLanes = kBlock / kNormFinalCols;  // slab lanes per column

// The slabs of a column -> its result.  Slab lane l folds slabs l, l + 64, ... in slab order, the 64 lanes are merged in a
// fixed tree: the order is a function of the slab count only (a single lane folding 1024 slabs one after the other took
// longer than the pass over the data).
template <int MODE>
__global__ void __launch_bounds__(kBlock) norm_final_kernel(const NormFinalArgs p) {
    __shared__ double s_n[kBlock], s_0[kBlock], s_1[kBlock];
    const int tid = threadIdx.x, D = p.D;
    const int lane = tid / kNormFinalCols, col = blockIdx.x * kNormFinalCols + (tid - lane * kNormFinalCols);
    const bool active = col < D;
    double n = 0.0, v0 = 0.0, v1 = 0.0;
    if (active) {
        for (int s = lane; s < p.slabs; s += kNormFinalLanes) {
            const double a = p.ws[(int64_t)s * 2 * D + col], b = p.ws[(int64_t)s * 2 * D + D + col];
            if (MODE == kNormStats) {
                const int64_t left = p.batch - (int64_t)s * p.rows_per_slab;
                chan_merge(n, v0, v1, (double)(left < p.rows_per_slab ? left : p.rows_per_slab), a, b);
            } else {
                v0 += a;
                v1 += b;
            }
        }
    }
    s_n[tid] = n;
    s_0[tid] = v0;
    s_1[tid] = v1;
    __syncthreads();
    for (int stride = kNormFinalLanes >> 1; stride >= 1; stride >>= 1) {
        if (active && lane < stride) {
            const int other = tid + stride * kNormFinalCols;
            if (MODE == kNormStats) {
                chan_merge(n, v0, v1, s_n[other], s_0[other], s_1[other]);
            } else {
                v0 += s_0[other];
                v1 += s_1[other];
            }
            s_n[tid] = n;
            s_0[tid] = v0;
            s_1[tid] = v1;
        }
        __syncthreads();
    }
    if (!active || lane != 0) return;
    if (MODE == kNormStats) {
        p.mean[col] = (float)v0;
        p.var[col] = (float)(v1 / (n - 1.0));   // unbiased
        if (p.sums) {
            p.sums[col] = v0;
            p.sums[D + col] = v1 / (n - 1.0);
        }
    } else {
        p.sums[col] = v0;
        p.sums[D + col] = v1;
    }
}

int norm_reduce_launch(int mode, const float* a, const float* b, const int64_t* amap, const int64_t* bmap, float* mean,
                       float* var, double* sums, void* workspace, int32_t* status, int64_t batch, int32_t features,
                       void* stream) {
    if (batch < 0 || features < 1) return NFA_ERR_INVALID_ARGUMENT;
    if (features > kNormMaxFeatures) return NFA_ERR_UNSUPPORTED;
    if (mode == kNormStats && batch < 2) return NFA_ERR_UNSUPPORTED;   // the unbiased variance of one row is NaN
    if (mode == kNormStats ? (!a || !mean || !var) : (!sums || (batch > 0 && (!a || !b)))) return NFA_ERR_INVALID_ARGUMENT;
    if (!workspace) return NFA_ERR_INVALID_ARGUMENT;
    const NormShape sh = norm_shape(features);
    int64_t rps;
    int slabs;
    norm_slabs(batch, features, &rps, &slabs);
    NormReduceArgs p;
    p.a = a;
    p.b = b;
    p.amap = amap;
    p.bmap = bmap;
    p.ws = (double*)workspace;
    p.status = status;
    p.batch = batch;
    p.rows_per_slab = rps;
    p.D = features;
    p.cw = sh.cw;
    p.rl = sh.rl;
    p.div_D = make_fastdiv((uint32_t)features);
    NormFinalArgs f;
    f.ws = (const double*)workspace;
    f.mean = mean;
    f.var = var;
    f.sums = sums;
    f.batch = batch;
    f.rows_per_slab = rps;
    f.D = features;
    f.slabs = slabs;
    const dim3 grid((unsigned)slabs, (unsigned)sh.col_tiles), fgrid((unsigned)((features + kNormFinalCols - 1) / kNormFinalCols));
    int rc;
    if (mode == kNormStats) {
        rc = launch_kernel(norm_partial_kernel<kNormStats>, grid, dim3(kBlock), 0, (hipStream_t)stream, p, 0, false);
        if (rc != NFA_OK) return rc;
        return launch_kernel(norm_final_kernel<kNormStats>, fgrid, dim3(kBlock), 0, (hipStream_t)stream, f, 0, false);
    }
    rc = launch_kernel(norm_partial_kernel<kNormSums>, grid, dim3(kBlock), 0, (hipStream_t)stream, p, 0, false);
    if (rc != NFA_OK) return rc;
    return launch_kernel(norm_final_kernel<kNormSums>, fgrid, dim3(kBlock), 0, (hipStream_t)stream, f, 0, false);
}

// ------------------------------------------------------------------------------------------ the per-column map
struct NormMapArgs {
    const float* x;
    const float* p0;   // BatchNorm: unconstrained_weight   ActNorm: log_scale
    const float* p1;   //            bias                            shift
    const float* p2;   //            mean (batch or running)
    const float* p3;   //            var
    const int64_t* perm;
    const int64_t* scatter;
    float* out;
    float* lad;
    int32_t* status;
    int64_t batch;
    double eps;
    int D, cw, rl;
    int DV;            // lane columns: D / V, V = 4 (float4 lanes: D % 4 == 0, aligned rows, no gather / scatter) or 1
    int accumulate;
    FastDiv div_DV;
};

enum NormKind { kNormBatchNorm = 0, kNormActNorm = 1 };
enum NormMapMode { kNormForward = 0, kNormInverse = 1, kNormForwardGrad = 2, kNormInverseGrad = 3 };

// a, m, s, t of one column and the column's term of the log-determinant
template <int KIND, bool INVERSE>
__device__ __forceinline__ void norm_constants(const NormMapArgs& p, int c, float* a, float* m, float* s, float* t, double* term) {
    if (KIND == kNormBatchNorm) {
        const double w = norm_softplus_f64((double)p.p0[c]) + p.eps;
        const double ve = (double)p.p3[c] + p.eps;
        const double l = log(w) - 0.5 * log(ve);
        if (!INVERSE) {
            *a = (float)w;
            *m = p.p2[c];
            *s = (float)sqrt(ve);
            *t = p.p1[c];
            *term = l;
        } else {
            *a = (float)sqrt(ve);
            *m = p.p1[c];
            *s = (float)w;
            *t = p.p2[c];
            *term = -l;
        }
    } else {
        const double ls = (double)p.p0[c];
        if (!INVERSE) {
            *a = (float)exp(ls);
            *m = 0.f;
            *s = 1.f;
            *t = p.p1[c];
            *term = ls;
        } else {
            *a = 1.f;
            *m = p.p1[c];
            *s = (float)exp(ls);
            *t = 0.f;
            *term = -ls;
        }
    }
}

template <int V>
__device__ __forceinline__ void norm_load(const float* src, float* v) {
    if (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        v[0] = q.x;
        v[1] = q.y;
        v[2] = q.z;
        v[3] = q.w;
    } else {
        v[0] = *src;
    }
}

template <int V>
__device__ __forceinline__ void norm_store(float* dst, const float* v) {
    if (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else *dst = v[0];
}

template <int KIND, int MODE, int V>
__global__ void __launch_bounds__(kBlock) norm_map_kernel(const NormMapArgs p) {
    __shared__ double s_term[kNormMaxFeatures];
    __shared__ float s_a[kNormMaxFeatures], s_m[kNormMaxFeatures], s_s[kNormMaxFeatures], s_t[kNormMaxFeatures];
    constexpr bool kInverse = (MODE == kNormInverse || MODE == kNormInverseGrad);
    constexpr bool kGrad = (MODE == kNormForwardGrad || MODE == kNormInverseGrad);
    const int tid = threadIdx.x, D = p.D, rl = p.rl;
    // ---- the layer's constants, once per workgroup
    int top = 1;
    while (top < D) top <<= 1;
    for (int c = tid; c < top; c += kBlock) {
        double term = 0.0;
        if (c < D) norm_constants<KIND, kInverse>(p, c, &s_a[c], &s_m[c], &s_s[c], &s_t[c], &term);
        if (!kGrad) s_term[c] = term;
    }
    __syncthreads();
    float layer_lad = 0.f;
    if (!kGrad && p.lad) {   // (workgroup-uniform)
        for (int stride = top >> 1; stride >= 1; stride >>= 1) {   // one fixed tree for a given D, whatever the grid
            for (int i = tid; i < stride; i += kBlock) s_term[i] += s_term[i + stride];
            __syncthreads();
        }
        layer_lad = (float)s_term[0];
    }
    int rlane, vcol, bad = 0;
    const bool active = norm_lane(tid, p.DV, p.cw, rl, p.div_DV, blockIdx.y, &rlane, &vcol);
    if (active) {
        const int col = vcol * V;
        const int cin = V == 1 ? norm_index(p.perm, col, D, &bad) : col;
        const int cout = V == 1 ? norm_index(p.scatter, col, D, &bad) : col;
        float a[V], m[V], s[V], t[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            a[j] = s_a[col + j];
            m[j] = s_m[col + j];
            s[j] = s_s[col + j];
            t[j] = s_t[col + j];
        }
        const bool writes_lad = !kGrad && p.lad && col == 0;
        const int64_t step = (int64_t)rl * kNormUnroll;
        const int64_t chunks = (p.batch + step - 1) / step;
        for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
            const int64_t r = chunk * step + rlane;
            float v[kNormUnroll][V];
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) {
                const int64_t ru = r + (int64_t)u * rl;
                if (ru < p.batch) norm_load<V>(p.x + ru * D + cin, v[u]);
            }
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) {
                const int64_t ru = r + (int64_t)u * rl;
                if (ru < p.batch) {
                    float o[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) o[j] = kGrad ? (v[u][j] * a[j]) / s[j] : a[j] * ((v[u][j] - m[j]) / s[j]) + t[j];
                    norm_store<V>(p.out + ru * D + cout, o);
                    if (writes_lad) p.lad[ru] = p.accumulate ? p.lad[ru] + layer_lad : layer_lad;
                }
            }
        }
    }
    if (bad && p.status) atomicOr(p.status, bad);
}

template <int KIND, int V>
int norm_map_dispatch(int mode, dim3 grid, hipStream_t st, const NormMapArgs& p) {
    void (*kern)(NormMapArgs) = mode == kNormForward       ? norm_map_kernel<KIND, kNormForward, V>
                                : mode == kNormInverse     ? norm_map_kernel<KIND, kNormInverse, V>
                                : mode == kNormForwardGrad ? norm_map_kernel<KIND, kNormForwardGrad, V>
                                                           : norm_map_kernel<KIND, kNormInverseGrad, V>;
    return launch_kernel(kern, grid, dim3(kBlock), 0, st, p, 0, false);
}

inline unsigned norm_map_grid(int64_t batch, const NormShape& sh) {
    const int64_t step = (int64_t)sh.rl * kNormUnroll;
    int64_t chunks = (batch + step - 1) / step;
    const int64_t cap = 2 * kNormMaxGroups / sh.col_tiles;
    return (unsigned)(chunks < cap ? chunks : cap);
}

int norm_map_launch(int kind, int mode, const float* inputs, const float* p0, const float* p1, const float* p2,
                    const float* p3, const int64_t* gather, const int64_t* scatter, float* outputs, float* logabsdet,
                    int32_t* status, int64_t batch, int32_t features, double eps, int accumulate, void* stream) {
    if (batch < 0 || features < 1) return NFA_ERR_INVALID_ARGUMENT;
    if (kind != kNormBatchNorm && kind != kNormActNorm) return NFA_ERR_INVALID_ARGUMENT;
    if (features > kNormMaxFeatures) return NFA_ERR_UNSUPPORTED;
    if (!(eps >= 0.0)) return NFA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return NFA_OK;
    if (!inputs || !outputs || !p0 || !p1) return NFA_ERR_INVALID_ARGUMENT;
    if (kind == kNormBatchNorm && (!p2 || !p3)) return NFA_ERR_INVALID_ARGUMENT;
    if ((mode == kNormForward || mode == kNormInverse) && !logabsdet) return NFA_ERR_INVALID_ARGUMENT;
    // float4 lanes where a row is a whole number of aligned float4 and no column moves
    const bool wide = features % 4 == 0 && !gather && !scatter
                      && ((reinterpret_cast<uintptr_t>(inputs) | reinterpret_cast<uintptr_t>(outputs)) & 15) == 0;
    const int V = wide ? 4 : 1;
    const NormShape sh = norm_shape(features / V);
    NormMapArgs p;
    p.x = inputs;
    p.p0 = p0;
    p.p1 = p1;
    p.p2 = p2;
    p.p3 = p3;
    p.perm = gather;
    p.scatter = scatter;
    p.out = outputs;
    p.lad = logabsdet;
    p.status = status;
    p.batch = batch;
    p.eps = eps;
    p.D = features;
    p.cw = sh.cw;
    p.rl = sh.rl;
    p.DV = features / V;
    p.accumulate = accumulate;
    p.div_DV = make_fastdiv((uint32_t)p.DV);
    const dim3 grid(norm_map_grid(batch, sh), (unsigned)sh.col_tiles);
    const hipStream_t st = (hipStream_t)stream;
    if (kind == kNormBatchNorm)
        return wide ? norm_map_dispatch<kNormBatchNorm, 4>(mode, grid, st, p) : norm_map_dispatch<kNormBatchNorm, 1>(mode, grid, st, p);
    return wide ? norm_map_dispatch<kNormActNorm, 4>(mode, grid, st, p) : norm_map_dispatch<kNormActNorm, 1>(mode, grid, st, p);
}

// ------------------------------------------------------------------------------------------ input gradient, batch statistics
struct NormBatchGradArgs {
    const float* g;
    const float* x;
    const float* coef;   // [6][D]: mean, s, w / s, G1 / B, G2 / (B - 1), L / ((B - 1) (var + eps))
    const int64_t* perm;
    const int64_t* scatter;
    float* gx;
    int32_t* status;
    int64_t batch;
    int D, cw, rl;
    FastDiv div_D;
};

__global__ void __launch_bounds__(kBlock) norm_batch_grad_kernel(const NormBatchGradArgs p) {
    const int tid = threadIdx.x, D = p.D, rl = p.rl;
    int rlane, col, bad = 0;
    if (norm_lane(tid, D, p.cw, rl, p.div_D, blockIdx.y, &rlane, &col)) {
        const int cx = norm_index(p.perm, col, D, &bad), cg = norm_index(p.scatter, col, D, &bad);
        const float mean = p.coef[col], s = p.coef[D + col], c0 = p.coef[2 * D + col], c1 = p.coef[3 * D + col],
                    c2 = p.coef[4 * D + col], c3 = p.coef[5 * D + col];
        const int64_t step = (int64_t)rl * kNormUnroll;
        const int64_t chunks = (p.batch + step - 1) / step;
        for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
            const int64_t r = chunk * step + rlane;
            float g[kNormUnroll], x[kNormUnroll];
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) {
                const int64_t ru = r + (int64_t)u * rl;
                const bool in = ru < p.batch;
                g[u] = in ? p.g[ru * D + cg] : 0.f;
                x[u] = in ? p.x[ru * D + cx] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kNormUnroll; ++u) {
                const int64_t ru = r + (int64_t)u * rl;
                if (ru < p.batch) {
                    const float d = x[u] - mean, xh = d / s;
                    p.gx[ru * D + cx] = c0 * ((g[u] - c1) - xh * c2) - c3 * d;
                }
            }
        }
    }
    if (bad && p.status) atomicOr(p.status, bad);
}

}  // namespace
}  // namespace nfa

extern "C" size_t nfa_norm_workspace_bytes(int64_t batch, int32_t features) {
    if (batch < 0 || features < 1 || features > nfa::kNormMaxFeatures) return 0;
    int64_t rps;
    int slabs;
    nfa::norm_slabs(batch, features, &rps, &slabs);
    return (size_t)slabs * 2 * (size_t)features * sizeof(double);
}

extern "C" int nfa_norm_slab_count(int64_t batch, int32_t features) {
    if (batch < 0 || features < 1 || features > nfa::kNormMaxFeatures) return 0;
    int64_t rps;
    int slabs;
    nfa::norm_slabs(batch, features, &rps, &slabs);
    return slabs;
}

extern "C" int nfa_norm_column_stats_f32(const float* inputs, float* mean, float* var, double* stats_f64, void* workspace,
                                         int64_t batch, int32_t features, void* stream) {
    return nfa::norm_reduce_launch(nfa::kNormStats, inputs, nullptr, nullptr, nullptr, mean, var, stats_f64, workspace,
                                   nullptr, batch, features, stream);
}

extern "C" int nfa_norm_column_sums_f32(const float* g, const float* u, const int64_t* g_columns, const int64_t* u_columns,
                                        double* sums, void* workspace, int32_t* status, int64_t batch, int32_t features,
                                        void* stream) {
    return nfa::norm_reduce_launch(nfa::kNormSums, g, u, g_columns, u_columns, nullptr, nullptr, sums, workspace, status,
                                   batch, features, stream);
}

extern "C" int nfa_norm_map_f32(const float* inputs, const float* p0, const float* p1, const float* p2, const float* p3,
                                const int64_t* in_perm, const int64_t* out_scatter, float* outputs, float* logabsdet,
                                int32_t* status, int64_t batch, int32_t features, double eps, int32_t kind, int32_t flags,
                                void* stream) {
    if (flags & ~(NFA_FLAG_INVERSE | NFA_FLAG_ACCUMULATE_LOGABSDET)) return NFA_ERR_INVALID_ARGUMENT;
    return nfa::norm_map_launch(kind, (flags & NFA_FLAG_INVERSE) ? nfa::kNormInverse : nfa::kNormForward, inputs, p0, p1,
                                p2, p3, in_perm, out_scatter, outputs, logabsdet, status, batch, features, eps,
                                (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0, stream);
}

extern "C" int nfa_norm_map_backward_f32(const float* grad_outputs, const float* p0, const float* p1, const float* p2,
                                         const float* p3, const int64_t* in_perm, const int64_t* out_scatter,
                                         float* grad_inputs, int32_t* status, int64_t batch, int32_t features, double eps,
                                         int32_t kind, int32_t flags, void* stream) {
    if (flags & ~NFA_FLAG_INVERSE) return NFA_ERR_INVALID_ARGUMENT;
    return nfa::norm_map_launch(kind, (flags & NFA_FLAG_INVERSE) ? nfa::kNormInverseGrad : nfa::kNormForwardGrad,
                                grad_outputs, p0, p1, p2, p3, /*gather=*/out_scatter, /*scatter=*/in_perm, grad_inputs,
                                nullptr, status, batch, features, eps, 0, stream);
}

extern "C" int nfa_norm_batch_backward_f32(const float* grad_outputs, const float* inputs, const float* coefficients,
                                           const int64_t* in_perm, const int64_t* out_scatter, float* grad_inputs,
                                           int32_t* status, int64_t batch, int32_t features, void* stream) {
    if (batch < 0 || features < 1) return NFA_ERR_INVALID_ARGUMENT;
    if (features > nfa::kNormMaxFeatures) return NFA_ERR_UNSUPPORTED;
    if (batch == 0) return NFA_OK;
    if (!grad_outputs || !inputs || !coefficients || !grad_inputs) return NFA_ERR_INVALID_ARGUMENT;
    const nfa::NormShape sh = nfa::norm_shape(features);
    nfa::NormBatchGradArgs p;
    p.g = grad_outputs;
    p.x = inputs;
    p.coef = coefficients;
    p.perm = in_perm;
    p.scatter = out_scatter;
    p.gx = grad_inputs;
    p.status = status;
    p.batch = batch;
    p.D = features;
    p.cw = sh.cw;
    p.rl = sh.rl;
    p.div_D = nfa::make_fastdiv((uint32_t)features);
    const dim3 grid(nfa::norm_map_grid(batch, sh), (unsigned)sh.col_tiles);
    return nfa::launch_kernel(nfa::norm_batch_grad_kernel, grid, dim3(nfa::kBlock), 0, (hipStream_t)stream, p, 0, false);
}
