// K24: a short stage program applied to every row of a float32 [batch, features] tensor, one launch per layer call
// (reference: transforms/orthogonal.py HouseholderSequence, transforms/svd.py SVDLinear, transforms/qr.py QRLinear).
// The stages, each optional, in this order:
//   - bias | reflect by set 0 | triangular | diagonal | reflect by set 1 | + bias
//   reflect     for each vector v_k of the set, first to last or last to first:  t = x . v_k,  x <- x - t (c_k v_k),
//               c_k = 2 / (v_k . v_k) from a float64 sum, rounded once; the dot product is summed in blocks of 16
//   diagonal    d_i = eps + softplus(u_i), float64, rounded once; x <- d x or x <- x / d
//   triangular  R = triu(upper_entries) + diag(exp(log_upper_diag));  x <- R x or, by substitution, x <- R^-1 x:
//               K16's tri_apply on K16's dense LDS image (lu_tri.hpp)
// logabsdet is one number per call, +- sum log d_i or +- sum log_upper_diag_i, summed in float64, rounded once and
// stored to (or added to) every row.
//
// The kernel reads the parameter tensors as the modules hold them: nothing is packed or cached on the host.  A lane owns
// a row: a tile of R rows is read coalesced into a column-major LDS tile (odd row stride), each lane takes ITS row into
// registers (features rounded up to 16: NB blocks, a template parameter, so every index is a constant), walks it through
// the stages (householder_math.hpp: hh_walk, the same text the host tests compile) and puts it back; the tile is written
// out coalesced.  What a stage needs of the parameters is staged into ONE LDS region right before the stage, between
// two barriers the whole workgroup passes together: at most 32 reflection vectors at a time (zero padded, with their c_k),
// or the [DP, DP] triangular image.  Staging is cheap next to the work it feeds -- a lane copies chunk * DP / R floats
// and then spends chunk * DP * 3 operations on them -- and it keeps the region at 16 KB for reflections whatever their
// number, so that the LDS goes to rows.  An element of c_k v_k is formed as the product of the two float32 values where
// it is used: the same bits as a table of them, without the table.
// A row's result depends on nothing but that row and the parameters: not on the batch, the tile or the grid.
//
// Backward (householder_backward_kernel): the input gradient and the batch reductions of the parameter gradients in one
// pass, for programs without a triangular stage (QRLinear's triangular step is a launch of its own on either side,
// nflows_amd/autograd.py).  The tile of rows x (held in float64) and the tile of gradients g sit side by side in LDS.
// Every lane first walks its row forward through the program; then the stages are undone last to first.  A reflection
// is its own inverse, so its input is recomputed from its output, x_in = H x_out -- in float64, there and back, so that
// the recomputed rows are as good as exact -- and the gradient moves the same way in float32, g_in = H g_out.  With a = x_in . v and b = g_out . v, c = 2 / (v . v):
//   dL/dv = sum_rows [ c^2 a b v - c b x_in - c a g_out ]  =  - c sum_rows [ b x_in + a g_in ]
// (g_out = g_in + c b v: the first term cancels).  The lanes store a and b, pass a barrier and change roles: lane j sums
// column j of both tiles over the tile's rows (exact products, added in float64) and adds the sum to ITS
// element of the workgroup's slab in global memory; -c is applied by the caller in float64 when it adds the slabs in
// index order.  The same lane owns the same slab element throughout, in a fixed order: two runs give the same bits.
// The diagonal stage is undone by lane j for column j as well, which gives sum_rows g_out x_in (forward) or
// sum_rows g_in y (inverse) on the way.
#include "common.hpp"
#include "householder_math.hpp"
#include "lu_tri.hpp"

namespace nfa {
namespace {

struct HhArgs {
    const float* x;         // inputs (backward: the inputs of the forward call; NULL never reaches a kernel)
    const float* g;         // backward: grad_outputs
    const float* q[2];      // set 0 and set 1 [K, D], as the program applies them
    const float* diag;      // unconstrained_diagonal [D] or NULL
    const float* upper;     // upper_entries [D (D - 1) / 2] or NULL
    const float* log_diag;  // log_upper_diag [D] or NULL
    const float* bias;      // [D] or NULL
    float* out;             // outputs (backward: grad_inputs)
    float* lad;             // [batch] or NULL
    double* partials;       // backward: [grid][(K0 + K1 + 1) D]
    int64_t batch;
    double eps;
    int D, DP, R, RS, region;
    int K[2];
    int descending, solve, transposed, sub_bias, add_bias, negate_lad, accumulate;
    FastDiv div_D, div_DP;
};

struct HhLds {
    double* logd;
    float *d, *bias, *c, *a, *b, *lad, *region, *tile, *tile_g;
    double* cd;   // backward: the scales in float64
};

// launch_plan.hpp: hh_lds_bytes
__device__ __forceinline__ HhLds hh_lds(float* lds, int DP, int R, int RS, int region, bool backward) {
    HhLds s;
    s.logd = reinterpret_cast<double*>(lds);
    s.d = lds + 2 * DP;
    s.bias = s.d + DP;
    s.c = s.bias + DP;
    s.a = s.c + kHhChunk;
    s.b = s.a + (backward ? R : 0);
    s.cd = reinterpret_cast<double*>(s.b + (backward ? R : 0));
    s.lad = s.b + (backward ? R + 2 * kHhChunk : 0);
    s.region = s.lad + 4;
    s.tile = s.region + region;
    s.tile_g = s.tile + (backward ? 2 : 1) * DP * RS;   // backward: the first tile holds float64
    return s;
}

// the diagonal, the bias and the layer's log-determinant, once per workgroup
__device__ __forceinline__ void hh_prologue(const HhArgs& a, const HhLds& s, int tid) {
    for (int c = tid; c < a.DP; c += a.R) {
        double d = 1.0, ld = 0.0;
        if (c < a.D && a.diag) {
            d = hh_diagonal_f64(a.diag[c], a.eps);
            ld = log(d);
        } else if (c < a.D && a.log_diag) {
            ld = (double)a.log_diag[c];
        }
        s.logd[c] = ld;
        s.d[c] = (float)d;
        s.bias[c] = (a.bias && c < a.D) ? a.bias[c] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {   // one fixed order, whatever the grid
        double t = 0.0;
        for (int c = 0; c < a.D; ++c) t += s.logd[c];
        s.lad[0] = (float)(a.negate_lad ? 0.0 - t : t);   // (0 stays +0)
    }
    __syncthreads();
}

// reflections [first, first + count) of q [K, D] into the region, zero padded to DP, and their scales
__device__ __forceinline__ void hh_stage_chunk(const HhArgs& a, const HhLds& s, const float* q, int first, int count,
                                               int tid, double* cd = nullptr) {
    __syncthreads();   // every lane is done with what the region held
    const float* src = q + (size_t)first * a.D;
    for (int e = tid; e < count * a.DP; e += a.R) {
        const int k = (int)fastdiv((uint32_t)e, a.div_DP);
        const int j = e - k * a.DP;
        s.region[e] = j < a.D ? src[k * a.D + j] : 0.f;
    }
    __syncthreads();
    for (int k = tid; k < count; k += a.R) {
        const double c = hh_reflection_scale_f64(s.region + k * a.DP, a.D);
        s.c[k] = (float)c;
        if (cd) cd[k] = c;
    }
    __syncthreads();
}

// the dense image of R (TRANSPOSED: of R^T) into the region; the padding is the identity
__device__ __forceinline__ void hh_stage_tri(const HhArgs& a, const HhLds& s, int tid) {
    __syncthreads();
    expand_tri_image(s.region, nullptr, a.upper, a.D, a.DP, a.div_DP, a.transposed != 0, tid, a.R);
    for (int c = tid; c < a.DP; c += a.R)
        s.region[c * a.DP + c] = c < a.D ? (float)exp((double)a.log_diag[c]) : 1.f;
    __syncthreads();
}

// coalesced read of rows * D floats -> column-major tile; zero padding columns, zero rows past the batch (computed,
// never stored)
__device__ __forceinline__ void hh_load_tile(const HhArgs& a, const float* src, int rows, float* tile, int tid) {
    for (int e = tid; e < rows * a.D; e += a.R) {
        const int r = (int)fastdiv((uint32_t)e, a.div_D);
        const int c = e - r * a.D;
        tile[c * a.RS + r] = src[e];
    }
    for (int c = a.D; c < a.DP; ++c) tile[c * a.RS + tid] = 0.f;
    if (tid >= rows)
        for (int c = 0; c < a.D; ++c) tile[c * a.RS + tid] = 0.f;
}

__device__ __forceinline__ void hh_store_tile(const HhArgs& a, float* dst, int rows, const float* tile, int tid) {
    for (int e = tid; e < rows * a.D; e += a.R) {
        const int r = (int)fastdiv((uint32_t)e, a.div_D);
        const int c = e - r * a.D;
        dst[e] = tile[c * a.RS + r];
    }
}

template <int NB>
__device__ __forceinline__ void hh_row_in(float (&x)[NB * kHhBlk], const float* col, int RS) {
#pragma unroll
    for (int j = 0; j < NB * kHhBlk; ++j) x[j] = col[j * RS];
}
template <int NB>
__device__ __forceinline__ void hh_row_out(const float (&x)[NB * kHhBlk], float* col, int RS) {
#pragma unroll
    for (int j = 0; j < NB * kHhBlk; ++j) col[j * RS] = x[j];
}

__device__ __forceinline__ HhProgram hh_program(const HhArgs& a, const HhLds& s) {
    HhProgram p;
    p.K[0] = a.K[0];
    p.K[1] = a.K[1];
    p.descending = a.descending != 0;
    p.solve = a.solve != 0;
    p.has_tri = a.upper != nullptr;
    p.has_diag = a.diag != nullptr;
    p.sub_bias = a.sub_bias != 0;
    p.add_bias = a.add_bias != 0;
    p.d = s.d;
    p.bias = s.bias;
    return p;
}

// RW: waves of the workgroup; R = 64 RW and the tile's row stride R + 1 are constants, so that a row's elements sit at
// immediate offsets from one address (a run-time stride costs one address register per element)
template <int NB, int RW>
__global__ void __launch_bounds__(RW * kWave) householder_kernel(const HhArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    constexpr int R = RW * kWave, RS = R + 1;
    const HhLds s = hh_lds(lds, a.DP, R, RS, a.region, false);
    hh_prologue(a, s, tid);
    const float layer_lad = s.lad[0];
    const HhProgram p = hh_program(a, s);
    float* col = s.tile + tid;
    auto stage = [&](int set, int first, int count) {
        hh_stage_chunk(a, s, a.q[set], first, count, tid);
        return HhStaged{s.region, s.c};
    };
    auto tri = [&](float (&x)[NB * kHhBlk]) {
        hh_stage_tri(a, s, tid);
        hh_row_out<NB>(x, col, RS);
        if (!a.transposed) {
            if (!a.solve) tri_apply<true, false, false>(s.region, a.DP, NB, col, RS);    // R x
            else tri_apply<true, false, true>(s.region, a.DP, NB, col, RS);             // R^-1 x
        } else {                                                                       // the image holds R^T: lower
            if (!a.solve) tri_apply<false, false, false>(s.region, a.DP, NB, col, RS);   // R^T g
            else tri_apply<false, false, true>(s.region, a.DP, NB, col, RS);            // R^-T g
        }
        hh_row_in<NB>(x, col, RS);
    };

    const int64_t num_tiles = (a.batch + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int rows = (int)((a.batch - row0) < R ? (a.batch - row0) : R);
        hh_load_tile(a, a.x + row0 * a.D, rows, s.tile, tid);
        __syncthreads();
        float x[NB * kHhBlk];
        hh_row_in<NB>(x, col, RS);
        hh_walk<NB>(x, p, stage, tri);
        hh_row_out<NB>(x, col, RS);
        __syncthreads();
        hh_store_tile(a, a.out + row0 * a.D, rows, s.tile, tid);
        if (a.lad && tid < rows) {
            float* l = a.lad + row0 + tid;
            *l = a.accumulate ? *l + layer_lad : layer_lad;
        }
        __syncthreads();
    }
}

// lane j: the sum over the tile's rows of b x + a g in column j, added in float64 (a parameter gradient is ONE number
// summed over the whole batch: nothing averages a float32 sum's rounding out)
__device__ __forceinline__ double hh_column_sum(const double* xc, const float* gc, const float* sa, const float* sb,
                                                int R) {
    double total = 0.0;
#pragma unroll 8
    for (int r = 0; r < R; ++r) {
        total = fma((double)sb[r], xc[r], total);
        total = fma((double)sa[r], (double)gc[r], total);
    }
    return total;
}

// One reflection of a row that lives in LDS in float64 (element j at col[j * RS]): x <- x - (x . v) c v with c in float64.
// Returns x_new . v.
__device__ __forceinline__ double hh_reflect_f64(double* col, int RS, int DP, const float* v, double c) {
    double t = 0.0;
#pragma unroll 4
    for (int j = 0; j < DP; ++j) t = fma(col[j * RS], (double)v[j], t);
    const double tc = t * c;
    double a = 0.0;
#pragma unroll 4
    for (int j = 0; j < DP; ++j) {
        const double vj = (double)v[j];
        const double xn = fma(-tc, vj, col[j * RS]);
        col[j * RS] = xn;
        a = fma(xn, vj, a);
    }
    return a;
}

template <int NB>
__global__ void __launch_bounds__(kWave) householder_backward_kernel(const HhArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    constexpr int R = kWave, RS = R + 1, DP = NB * kHhBlk;
    const int D = a.D;
    const HhLds s = hh_lds(lds, DP, R, RS, a.region, true);
    hh_prologue(a, s, tid);
    // from here on logd holds the diagonal itself in float64 (padding 1)
    for (int c = tid; c < DP; c += R) s.logd[c] = (c < D && a.diag) ? hh_diagonal_f64(a.diag[c], a.eps) : 1.0;
    const double* d64 = s.logd;
    const bool descending = a.descending != 0, solve = a.solve != 0, has_diag = a.diag != nullptr;
    double* xt = reinterpret_cast<double*>(s.tile);   // the rows, float64, column-major
    double* col = xt + tid;
    float* colg = s.tile_g + tid;
    double* slab = a.partials + (size_t)blockIdx.x * (size_t)(a.K[0] + a.K[1] + 1) * D;

    const int64_t num_tiles = (a.batch + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int rows = (int)((a.batch - row0) < R ? (a.batch - row0) : R);
        __syncthreads();   // (d64 written; the previous tile stored)
        {
            const float* src = a.x + row0 * D;
            for (int e = tid; e < rows * D; e += R) {
                const int r = (int)fastdiv((uint32_t)e, a.div_D);
                const int c = e - r * D;
                xt[c * RS + r] = (double)src[e] - (a.sub_bias ? (double)s.bias[c] : 0.0);
            }
            for (int c = D; c < DP; ++c) xt[c * RS + tid] = 0.0;
            if (tid >= rows)
                for (int c = 0; c < D; ++c) xt[c * RS + tid] = 0.0;
        }
        hh_load_tile(a, a.g + row0 * D, rows, s.tile_g, tid);
        __syncthreads();
        // ---- forward, in float64: every lane's row to the output of set 1.  The rows the gradients are taken at are
        // then as good as exact on the way back too (H H x = x to float64 rounding); recomputed in float32 they would
        // carry the roundings of the whole walk there and back, where the reference's carry only those up to the stage.
        for (int set = 0; set < 2; ++set) {
            if (set == 1 && has_diag) {
#pragma unroll 4
                for (int j = 0; j < DP; ++j) col[j * RS] = solve ? col[j * RS] / d64[j] : col[j * RS] * d64[j];
            }
            const int K = set == 0 ? a.K[0] : a.K[1];
            for (int i = 0; i < hh_chunks(K); ++i) {
                const HhChunk ch = hh_chunk(K, i, descending);
                hh_stage_chunk(a, s, a.q[set], ch.first, ch.count, tid, s.cd);
                for (int step = 0; step < ch.count; ++step) {
                    const int k = descending ? ch.count - 1 - step : step;
                    hh_reflect_f64(col, RS, DP, s.region + k * DP, s.cd[k]);
                }
            }
        }
        // ---- and back, stage by stage
        for (int set = 1; set >= 0; --set) {
            if (set == 0 && has_diag) {
                __syncthreads();   // the rows are in the tiles
                for (int j = tid; j < D; j += R) {
                    double* xc = xt + j * RS;
                    float* gc = s.tile_g + j * RS;
                    const double d = d64[j];
                    const float df = s.d[j];
                    double total = 0.0;
#pragma unroll 4
                    for (int r = 0; r < R; ++r) {
                        const double xo = xc[r];
                        const float go = gc[r];
                        if (!solve) {   // y = d x:  x = y / d,  g_x = d g_y,  dL/dd += g_y x
                            const double xi = xo / d;
                            total = fma((double)go, xi, total);
                            xc[r] = xi;
                            gc[r] = go * df;
                        } else {        // y = x / d:  x = d y,  g_x = g_y / d,  dL/dd -= g_x y
                            const float gi = go / df;
                            total = fma((double)gi, xo, total);
                            xc[r] = xo * d;
                            gc[r] = gi;
                        }
                    }
                    slab[(size_t)(a.K[0] + a.K[1]) * D + j] += total;
                }
                __syncthreads();
            }
            const int K = set == 0 ? a.K[0] : a.K[1];
            const size_t slab_row0 = set == 0 ? 0 : (size_t)a.K[0];
            for (int i = hh_chunks(K) - 1; i >= 0; --i) {
                const HhChunk ch = hh_chunk(K, i, descending);
                const int first = ch.first, count = ch.count;
                hh_stage_chunk(a, s, a.q[set], first, count, tid, s.cd);
#pragma unroll 1
                for (int step = count - 1; step >= 0; --step) {
                    const int k = descending ? count - 1 - step : step;
                    const float* v = s.region + k * DP;
                    const float aa = (float)hh_reflect_f64(col, RS, DP, v, s.cd[k]);   // the reflection's input from its output
                    float bb;
                    {
                        float g[DP];
                        hh_row_in<NB>(g, colg, RS);
                        bb = hh_dot<NB>(g, v);
                        NFA_HH_READ_AGAIN();
                        hh_update<NB>(g, v, s.c[k], bb);
                        hh_row_out<NB>(g, colg, RS);
                    }
                    s.a[tid] = aa;
                    s.b[tid] = bb;
                    __syncthreads();
                    for (int j = tid; j < D; j += R)
                        slab[(slab_row0 + first + k) * D + j] +=
                            hh_column_sum(xt + j * RS, s.tile_g + j * RS, s.a, s.b, R);
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        hh_store_tile(a, a.out + row0 * D, rows, s.tile_g, tid);
    }
}

struct HhCall {
    const float* q[2] = {nullptr, nullptr};
    int K[2] = {0, 0};
    const float* diag = nullptr;
    const float* upper = nullptr;
    const float* log_diag = nullptr;
    const float* bias = nullptr;
    int64_t batch = 0;
    int features = 0;
    double eps = 0.0;
};

// the checks that need no device
int hh_check(const HhCall& c) {
    if (c.batch < 0 || c.features < 1 || c.K[0] < 0 || c.K[1] < 0) return NFA_ERR_INVALID_ARGUMENT;
    if (!(c.eps >= 0.0)) return NFA_ERR_INVALID_ARGUMENT;
    if (c.diag && (c.upper || c.log_diag)) return NFA_ERR_INVALID_ARGUMENT;   // one middle stage at the most
    if ((c.upper == nullptr) != (c.log_diag == nullptr)) return NFA_ERR_INVALID_ARGUMENT;
    if (c.features < 2 || c.features > kHhMaxFeatures) return NFA_ERR_UNSUPPORTED;
    if (c.K[0] > kHhMaxTransforms || c.K[1] > kHhMaxTransforms) return NFA_ERR_UNSUPPORTED;
    return NFA_OK;
}

template <int NB>
int hh_launch_nb(bool backward, const HhArgs& a, const HhTile& t, hipStream_t st) {
    if (backward)
        return launch_kernel(householder_backward_kernel<NB>, dim3((unsigned)t.grid), dim3((unsigned)t.R), t.lds, st, a,
                             kCuLds, false);
    void (*const kerns[3])(HhArgs) = {householder_kernel<NB, 1>, householder_kernel<NB, 2>, householder_kernel<NB, 4>};
    return launch_kernel(kerns[t.R / 128], dim3((unsigned)t.grid), dim3((unsigned)t.R), t.lds, st, a, kCuLds, false);
}

HhTile hh_plan(const HhCall& c, bool backward) {
    const int DP = (c.features + kHhBlk - 1) / kHhBlk * kHhBlk;
    const int region = hh_region_floats(DP, c.K[0] > c.K[1] ? c.K[0] : c.K[1], c.upper != nullptr, kHhChunk);
    return plan_hh_tile(DP, region, backward ? 3 : 1, kHhChunk, backward ? kWave : kBlock, c.batch, device_cu_count());
}

int hh_launch(bool backward, const HhCall& c, HhArgs a, void* stream) {
    const HhTile t = hh_plan(c, backward);
    if (t.R == 0) return NFA_ERR_UNSUPPORTED;
    a.batch = c.batch;
    a.eps = c.eps;
    a.D = c.features;
    a.DP = (c.features + kHhBlk - 1) / kHhBlk * kHhBlk;
    a.R = t.R;
    a.RS = t.R + 1;
    a.region = hh_region_floats(a.DP, c.K[0] > c.K[1] ? c.K[0] : c.K[1], c.upper != nullptr, kHhChunk);
    a.diag = c.diag;
    a.upper = c.upper;
    a.log_diag = c.log_diag;
    a.bias = c.bias;
    a.div_D = make_fastdiv((uint32_t)a.D);
    a.div_DP = make_fastdiv((uint32_t)a.DP);
    hipStream_t st = (hipStream_t)stream;
    switch (a.DP / kHhBlk) {
        case 1: return hh_launch_nb<1>(backward, a, t, st);
        case 2: return hh_launch_nb<2>(backward, a, t, st);
        case 3: return hh_launch_nb<3>(backward, a, t, st);
        case 4: return hh_launch_nb<4>(backward, a, t, st);
        case 5: return hh_launch_nb<5>(backward, a, t, st);
        case 6: return hh_launch_nb<6>(backward, a, t, st);
        case 7: return hh_launch_nb<7>(backward, a, t, st);
        default: return hh_launch_nb<8>(backward, a, t, st);
    }
}

}  // namespace
}  // namespace nfa

extern "C" int nfa_householder_f32(const float* inputs, const float* q_first, int32_t num_first, const float* q_second,
                                   int32_t num_second, const float* unconstrained_diagonal, const float* upper_entries,
                                   const float* log_upper_diag, const float* bias, float* outputs, float* logabsdet,
                                   int64_t batch, int32_t features, double eps, int32_t flags, void* stream) {
    if (flags & ~(NFA_FLAG_INVERSE | NFA_FLAG_ACCUMULATE_LOGABSDET)) return NFA_ERR_INVALID_ARGUMENT;
    nfa::HhCall c;
    c.q[0] = q_first, c.q[1] = q_second, c.K[0] = num_first, c.K[1] = num_second;
    c.diag = unconstrained_diagonal, c.upper = upper_entries, c.log_diag = log_upper_diag, c.bias = bias;
    c.batch = batch, c.features = features, c.eps = eps;
    const int rc = nfa::hh_check(c);
    if (rc != NFA_OK) return rc;
    if (batch == 0) return NFA_OK;
    if (!inputs || !outputs || (num_first > 0 && !q_first) || (num_second > 0 && !q_second)) return NFA_ERR_INVALID_ARGUMENT;
    const bool inverse = (flags & NFA_FLAG_INVERSE) != 0;
    nfa::HhArgs a = {};
    a.x = inputs, a.out = outputs, a.lad = logabsdet;
    a.q[0] = q_first, a.q[1] = q_second, a.K[0] = num_first, a.K[1] = num_second;
    a.descending = inverse, a.solve = inverse, a.negate_lad = inverse;
    a.sub_bias = bias && inverse, a.add_bias = bias && !inverse;
    a.accumulate = (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0;
    return nfa::hh_launch(false, c, a, stream);
}

extern "C" int nfa_householder_backward_slabs(int64_t batch, int32_t features, int32_t num_first, int32_t num_second) {
    nfa::HhCall c;
    c.K[0] = num_first, c.K[1] = num_second, c.batch = batch, c.features = features;
    if (nfa::hh_check(c) != NFA_OK || batch == 0) return 0;
    return (int)nfa::hh_plan(c, true).grid;
}

extern "C" int nfa_householder_backward_f32(const float* inputs, const float* grad_outputs, const float* q_first,
                                            int32_t num_first, const float* q_second, int32_t num_second,
                                            const float* unconstrained_diagonal, const float* upper_entries,
                                            const float* log_upper_diag, const float* bias, float* grad_inputs,
                                            double* partials, int64_t batch, int32_t features, double eps,
                                            int32_t flags, void* stream) {
    if (flags & ~NFA_FLAG_INVERSE) return NFA_ERR_INVALID_ARGUMENT;
    nfa::HhCall c;
    c.q[0] = q_first, c.q[1] = q_second, c.K[0] = num_first, c.K[1] = num_second;
    c.diag = unconstrained_diagonal, c.upper = upper_entries, c.log_diag = log_upper_diag, c.bias = bias;
    c.batch = batch, c.features = features, c.eps = eps;
    const int rc = nfa::hh_check(c);
    if (rc != NFA_OK) return rc;
    if ((inputs == nullptr) != (partials == nullptr)) return NFA_ERR_INVALID_ARGUMENT;
    if (inputs && upper_entries) return NFA_ERR_UNSUPPORTED;   // the reductions: programs without a triangular stage
    if (batch == 0) return NFA_OK;
    if (!grad_outputs || !grad_inputs || (num_first > 0 && !q_first) || (num_second > 0 && !q_second))
        return NFA_ERR_INVALID_ARGUMENT;
    const bool inverse = (flags & NFA_FLAG_INVERSE) != 0;
    nfa::HhArgs a = {};
    a.out = grad_inputs;
    a.solve = inverse;
    if (!inputs) {
        // the input gradient alone: the transposed stages in reverse -- the sets swapped and walked the other way, the
        // diagonal as it is, the triangular step on the transposed image, no bias
        a.x = grad_outputs;
        a.q[0] = q_second, a.q[1] = q_first, a.K[0] = num_second, a.K[1] = num_first;
        c.q[0] = q_second, c.q[1] = q_first, c.K[0] = num_second, c.K[1] = num_first;
        c.bias = nullptr;
        a.descending = !inverse;
        a.transposed = 1;
        return nfa::hh_launch(false, c, a, stream);
    }
    a.x = inputs, a.g = grad_outputs, a.partials = partials;
    a.q[0] = q_first, a.q[1] = q_second, a.K[0] = num_first, a.K[1] = num_second;
    a.descending = inverse;
    a.sub_bias = bias && inverse;
    return nfa::hh_launch(true, c, a, stream);
}
