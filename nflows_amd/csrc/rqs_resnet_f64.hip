// K26: a whole rational-quadratic spline coupling layer in float64, one launch per layer -- coupling.py:73-130 with a
// ResidualNet conditioner (nn/nets/resnet.py:55-100: initial Linear, blocks h += W_1 relu(W_0 relu(h) + b_0) + b_1, final
// Linear) and the functional of splines/rational_quadratic.py:13-181 on the conditioner's output, which never reaches
// HBM.  The GEMMs run on v_mfma_f64_16x16x4_f64; the per-element arithmetic is K5d's (rqs_f64_core.hpp, unchanged).
//
// A wave owns 16 rows.  The hidden stream (up to 128 wide) is up to 8 accumulator tiles of 4 doubles; an activation
// reaches the next GEMM's A operand through the wave's own LDS image (lane l reads A[l & 15][4 kk + (l >> 4)]: one
// ds_read_b64); the weights arrive as B fragments (launch_plan.hpp: the packed stream), staged through LDS in chunks of
// kc k-steps that the workgroup's four waves share: global_load -> registers -> ds_write into the buffer the previous
// chunk was read from, one barrier per chunk.  The final Linear is taken in column chunks of whole features; a chunk's
// logits go to the wave's LDS and the spline is evaluated from there, a lane per (row, feature).
//
// f64 fragment maps (they are not the f32 ones): C/D col = lane & 15, row = (lane >> 4) + 4 reg; A: lane l holds
// A[l & 15][l >> 4]; B: lane l holds B[l >> 4][l & 15].
//
// Every row's result depends on that row alone: a row of D is the k-ordered chain over that row of A, the k order is
// the stream's, and a row's log-derivatives are added in an order the shape fixes (lane group g = 0..3 adds the
// features g, g + 4, .. of every chunk in turn; the row's sum is (g0 + g1) + (g2 + g3)).
#include "common.hpp"
#include "rqs_f64_core.hpp"

namespace nfa {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

struct F64LayerArgs {
    const double* x;
    double* out;
    double* lad;
    const int64_t* idf;
    const int64_t* tf;
    const double* packed;
    int32_t* status;
    int64_t B, tiles;
    int D, di, dt, H, P, nb, accumulate;
    int NT, ks0, ksh, F, chunks, NTF, NTL;
    int AS, LS, kc, bufd;   // bufd: doubles of one weight buffer
    int64_t w_blocks, w_final, b_in, b_blocks, b_final;
    f64::Spec s;
};

__device__ __forceinline__ void wave_lds_fence() {
    // the wave's own LDS image: written by some lanes, read by others; LDS operations of one wave complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// acc[t] += A[16 x 4 ksteps] B[4 ksteps x 16] for the NT tiles of a stage, k-step by k-step
template <int NT>
__device__ __forceinline__ void mma_steps(double4_t (&acc)[8], const double* a, const double* w, int ksteps) {
#pragma unroll 2
    for (int k = 0; k < ksteps; ++k) {
        const double av = a[4 * k];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, w[(k * NT + t) * 64], acc[t], 0, 0, 0);
    }
}

__device__ __forceinline__ void mma_dispatch(int nt, double4_t (&acc)[8], const double* a, const double* w, int ksteps) {
    switch (nt) {
        case 1: mma_steps<1>(acc, a, w, ksteps); break;
        case 2: mma_steps<2>(acc, a, w, ksteps); break;
        case 3: mma_steps<3>(acc, a, w, ksteps); break;
        case 4: mma_steps<4>(acc, a, w, ksteps); break;
        case 5: mma_steps<5>(acc, a, w, ksteps); break;
        case 6: mma_steps<6>(acc, a, w, ksteps); break;
        case 7: mma_steps<7>(acc, a, w, ksteps); break;
        default: mma_steps<8>(acc, a, w, ksteps); break;
    }
}

// One Linear: acc += act[16 x 4 ks] W^T, W's ks x nt fragments at `wsrc`.  Every wave of the workgroup calls it with the
// same (nt, ks, wsrc); on return all of them have passed a barrier behind their last read of the buffers.
// `a`: the lane's A element of k-step 0 in its wave's image; `w`: the two weight buffers.
__device__ __forceinline__ void gemm_stage(double4_t (&acc)[8], int nt, int ks, const double* __restrict__ wsrc,
                                           const double* a, double* w, int kc, int bufd, int tid, int lane) {
    const int rowd = nt * 64;   // doubles of a k-step
    const int nchunk = (ks + kc - 1) / kc;
    {
        const int n2 = (ks < kc ? ks : kc) * (rowd / 2);
        const double2_t* g = reinterpret_cast<const double2_t*>(wsrc);
        double2_t* l = reinterpret_cast<double2_t*>(w);
        for (int v = tid; v < n2; v += kBlock) l[v] = g[v];
    }
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const int kthis = ks - c * kc < kc ? ks - c * kc : kc;
        const bool more = c + 1 < nchunk;
        const int knext = more ? (ks - (c + 1) * kc < kc ? ks - (c + 1) * kc : kc) : 0;
        const int n2 = knext * (rowd / 2);
        // (unconditional loads at clamped indices: the values stay in registers; lanes past the chunk store nothing)
        const double2_t* g = reinterpret_cast<const double2_t*>(more ? wsrc + (int64_t)(c + 1) * kc * rowd : wsrc);
        double2_t r[8];   // (kc nt <= 64: at most 2048 pairs a chunk)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int v = u * kBlock + tid;
            r[u] = g[v < n2 ? v : 0];
        }
        mma_dispatch(nt, acc, a + 4 * c * kc, w + (c & 1) * bufd + lane, kthis);
        double2_t* l = reinterpret_cast<double2_t*>(w + ((c + 1) & 1) * bufd);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int v = u * kBlock + tid;
            if (v < n2) l[v] = r[u];
        }
        __syncthreads();
    }
}

// the wave's accumulator tiles -> its LDS image [16][stride]; RELU: max(v, 0), NaN kept as torch's clamp_min keeps it.
// Columns from `ncols` on are the zero padding of the hidden width: they are stored as zeros whatever the accumulator
// holds (0 x inf = NaN from a zero weight row must not reach the next GEMM, where NaN x 0 would take the whole row).
template <bool RELU>
__device__ __forceinline__ void store_tiles(const double4_t (&acc)[8], int nt, int ncols, double* img, int stride, int lane) {
    double* p = img + (lane >> 4) * stride + (lane & 15);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < nt) {
            const bool real = 16 * t + (lane & 15) < ncols;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = acc[t][r];
                p[4 * r * stride + 16 * t] = real ? (RELU ? (v < 0.0 ? 0.0 : v) : v) : 0.0;
            }
        }
    }
}

__device__ __forceinline__ void clear_tiles(double4_t (&acc)[8], int nt) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (t < nt) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
}

// A Linear's sum starts at zero and takes its bias last, the skip connection takes the finished update in ONE addition:
// one rounding at the magnitude of the bias / of h per element, where a chain started at the bias or at h would round
// every one of its k-steps there (with a residual stream much larger than a block's update that cost an order of
// magnitude against the library GEMMs' beta C + A B).
__device__ __forceinline__ void add_bias(double4_t (&acc)[8], int nt, const double* __restrict__ b, int lane) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < nt) {
            const double v = b[16 * t + (lane & 15)];
            acc[t] += double4_t{v, v, v, v};
        }
    }
}

__device__ __forceinline__ void add_tiles(double4_t (&acc)[8], int nt, const double4_t (&u)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t)
        if (t < nt) acc[t] += u[t];
}

__global__ void __launch_bounds__(kBlock) rqs_resnet_layer_f64_kernel(const F64LayerArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, grp = lane >> 4;
    constexpr int kWaves = kBlock / kWave;
    double* act = lds + wave * 16 * a.AS;
    double* logits = lds + kWaves * 16 * a.AS + wave * 16 * a.LS;
    double* wbuf = lds + kWaves * 16 * (a.AS + a.LS);
    const double* a_lane = act + row * a.AS + grp;
    const int64_t hidden_d = (int64_t)a.ksh * a.NT * 64;
    const int HP = 16 * a.NT;
    int my_status = 0;

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t grow = tile * kF64Rows + wave * 16 + row;
        const bool live = grow < a.B;
        const double* xr = a.x + grow * a.D;
        double* outr = a.out + grow * a.D;

        // identity columns: through to the outputs bit for bit, and into the image as the first GEMM's A operand
        wave_lds_fence();
        for (int j = grp; j < 4 * a.ks0; j += 4) {
            double v = 0.0;
            if (live && j < a.di) {
                const int64_t col = a.idf[j];
                if (col >= 0 && col < a.D) {
                    v = xr[col];
                    outr[col] = v;
                } else {
                    my_status |= NFA_STATUS_BAD_INDEX;
                }
            }
            act[row * a.AS + j] = v;
        }
        wave_lds_fence();

        double4_t h[8], u[8];
        clear_tiles(h, a.NT);
        gemm_stage(h, a.NT, a.ks0, a.packed, a_lane, wbuf, a.kc, a.bufd, tid, lane);
        add_bias(h, a.NT, a.packed + a.b_in, lane);
        for (int b = 0; b < a.nb; ++b) {
            const double* wb = a.packed + a.w_blocks + 2 * b * hidden_d;
            const double* bb = a.packed + a.b_blocks + 2 * b * HP;
            wave_lds_fence();
            store_tiles<true>(h, a.NT, a.H, act, a.AS, lane);
            wave_lds_fence();
            clear_tiles(u, a.NT);
            gemm_stage(u, a.NT, a.ksh, wb, a_lane, wbuf, a.kc, a.bufd, tid, lane);
            add_bias(u, a.NT, bb, lane);
            wave_lds_fence();
            store_tiles<true>(u, a.NT, a.H, act, a.AS, lane);
            wave_lds_fence();
            clear_tiles(u, a.NT);
            gemm_stage(u, a.NT, a.ksh, wb + hidden_d, a_lane, wbuf, a.kc, a.bufd, tid, lane);
            add_bias(u, a.NT, bb + HP, lane);
            add_tiles(h, a.NT, u);
        }
        wave_lds_fence();
        store_tiles<false>(h, a.NT, a.H, act, a.AS, lane);
        wave_lds_fence();

        double lad_sum = 0.0;
        for (int c = 0; c < a.chunks; ++c) {
            const bool last = c == a.chunks - 1;
            const int nt = last ? a.NTL : a.NTF;
            const int fc = last ? a.dt - c * a.F : a.F;
            clear_tiles(u, nt);
            gemm_stage(u, nt, a.ksh, a.packed + a.w_final + (int64_t)c * a.ksh * a.NTF * 64, a_lane, wbuf, a.kc, a.bufd,
                       tid, lane);
            add_bias(u, nt, a.packed + a.b_final + (int64_t)c * a.NTF * 16, lane);
            wave_lds_fence();
            store_tiles<false>(u, nt, 16 * nt, logits, a.LS, lane);
            wave_lds_fence();
            if (live) {
                for (int f = grp; f < fc; f += 4) {
                    const int64_t col = a.tf[c * a.F + f];
                    if (col < 0 || col >= a.D) {
                        my_status |= NFA_STATUS_BAD_INDEX;
                        continue;
                    }
                    const double* lg = logits + row * a.LS + f * a.P;
                    double y, l;
                    f64::forward_element(a.s, xr[col], lg, lg + a.s.K, lg + 2 * a.s.K, y, l, my_status);
                    outr[col] = y;
                    lad_sum += l;
                }
            }
        }
        // the row's sum: (g0 + g1) + (g2 + g3), the same bits in every lane of the row
        lad_sum += __shfl_xor(lad_sum, 16, kWave);
        lad_sum += __shfl_xor(lad_sum, 32, kWave);
        if (live && grp == 0) a.lad[grow] = a.accumulate ? a.lad[grow] + lad_sum : lad_sum;
    }
    if (my_status && a.status) atomicOr(a.status, my_status);
}

// ---- the packer: one matrix (or one chunk of W_f's rows) into B fragments, one bias vector into its padded place
struct PackF64Args {
    const double* w;   // [rows, cols] row-major, leading dimension ld
    int64_t ld;
    int rows, cols, ks, nt;
    double* dst;       // ks * nt * 64
};

__global__ void __launch_bounds__(kBlock) pack_fragments_f64_kernel(const PackF64Args p) {
    const int n = p.ks * p.nt * 64;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int l = i & 63, t = (i >> 6) % p.nt, kk = (i >> 6) / p.nt;
        const int o = 16 * t + (l & 15), k = 4 * kk + (l >> 4);
        p.dst[i] = o < p.rows && k < p.cols ? p.w[o * p.ld + k] : 0.0;
    }
}

struct PackBiasF64Args {
    const double* b;
    int n, padded;
    double* dst;
};

__global__ void __launch_bounds__(kBlock) pack_bias_f64_kernel(const PackBiasF64Args p) {
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < p.padded; i += gridDim.x * kBlock) p.dst[i] = i < p.n ? p.b[i] : 0.0;
}

static int pack_matrix(const double* w, int64_t ld, int rows, int cols, int ks, int nt, double* dst, hipStream_t st) {
    PackF64Args p{w, ld, rows, cols, ks, nt, dst};
    const int n = ks * nt * 64;
    return launch_kernel(pack_fragments_f64_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, p, 0, false);
}

static int pack_bias(const double* b, int n, int padded, double* dst, hipStream_t st) {
    PackBiasF64Args p{b, n, padded, dst};
    return launch_kernel(pack_bias_f64_kernel, dim3((padded + kBlock - 1) / kBlock), dim3(kBlock), 0, st, p, 0, false);
}

static bool f64_layer_shape_ok(int di, int H, int nb, int dt, int P) {
    return di >= 1 && di <= 64 && dt >= 1 && dt <= 64 && H >= 1 && H <= 128 && nb >= 0 && P >= 1 && P <= 128;
}

}  // namespace nfa

using namespace nfa;

extern "C" int nfa_pack_resnet_f64(const double* initial_weight, const double* initial_bias,
                                   const double* const* block_params, const double* final_weight,
                                   const double* final_bias, int32_t num_identity, int32_t hidden_features,
                                   int32_t num_blocks, int32_t num_transform, int32_t params_per_feature, double* packed,
                                   int64_t packed_doubles, void* stream) {
    const int di = num_identity, H = hidden_features, nb = num_blocks, dt = num_transform, P = params_per_feature;
    if (!initial_weight || !initial_bias || !final_weight || !final_bias || !packed || (nb > 0 && !block_params))
        return NFA_ERR_INVALID_ARGUMENT;
    if (!f64_layer_shape_ok(di, H, nb, dt, P)) return NFA_ERR_UNSUPPORTED;
    for (int i = 0; i < 4 * nb; ++i)
        if (!block_params[i]) return NFA_ERR_INVALID_ARGUMENT;
    const F64LayerLayout l = f64_layer_layout(di, H, nb, dt, P);
    if (packed_doubles != l.total || !aligned16(packed)) return NFA_ERR_INVALID_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hidden = (int64_t)l.ksh * l.NT * 64;
    int rc = pack_matrix(initial_weight, di, H, di, l.ks0, l.NT, packed + l.w_in, st);
    if (rc == NFA_OK) rc = pack_bias(initial_bias, H, l.HP, packed + l.b_in, st);
    for (int j = 0; j < 2 * nb && rc == NFA_OK; ++j) {
        rc = pack_matrix(block_params[2 * j], H, H, H, l.ksh, l.NT, packed + l.w_blocks + j * hidden, st);
        if (rc == NFA_OK) rc = pack_bias(block_params[2 * j + 1], H, l.HP, packed + l.b_blocks + (int64_t)j * l.HP, st);
    }
    for (int c = 0; c < l.chunks && rc == NFA_OK; ++c) {
        const bool last = c == l.chunks - 1;
        const int nt = last ? l.NTL : l.NTF;
        const int rows = (last ? dt - c * l.F : l.F) * P;
        const int64_t row0 = (int64_t)c * l.F * P;
        rc = pack_matrix(final_weight + row0 * H, H, rows, H, l.ksh, nt, packed + l.w_final + (int64_t)c * l.ksh * l.NTF * 64, st);
        if (rc == NFA_OK) rc = pack_bias(final_bias + row0, rows, 16 * nt, packed + l.b_final + (int64_t)c * l.NTF * 16, st);
    }
    return rc;
}

extern "C" int nfa_rqs_resnet_layer_f64(const double* inputs, const double* packed, int64_t packed_doubles,
                                        const int64_t* identity_idx, const int64_t* transform_idx, double* outputs,
                                        double* logabsdet, int32_t* status, int64_t batch, int32_t features,
                                        int32_t num_identity, int32_t num_transform, int32_t hidden_features,
                                        int32_t num_blocks, const nfa_rqs_spec* spec, int32_t flags, void* stream) {
    if (!spec || batch < 0 || features < 1) return NFA_ERR_INVALID_ARGUMENT;
    if (flags & ~(NFA_FLAG_INVERSE | NFA_FLAG_ACCUMULATE_LOGABSDET)) return NFA_ERR_INVALID_ARGUMENT;
    if (spec->tails != NFA_TAILS_NONE && spec->tails != NFA_TAILS_LINEAR) return NFA_ERR_INVALID_ARGUMENT;
    if (spec->num_bins < 1) return NFA_ERR_INVALID_ARGUMENT;
    if (spec->min_bin_width * spec->num_bins > 1.0) return NFA_ERR_MIN_BIN_WIDTH;
    if (spec->min_bin_height * spec->num_bins > 1.0) return NFA_ERR_MIN_BIN_HEIGHT;
    const int K = spec->num_bins, linear = spec->tails == NFA_TAILS_LINEAR;
    const int di = num_identity, dt = num_transform, H = hidden_features, nb = num_blocks;
    if (K > 32) return NFA_ERR_UNSUPPORTED;
    const int P = linear ? 3 * K - 1 : 3 * K + 1;
    if (!f64_layer_shape_ok(di, H, nb, dt, P)) return NFA_ERR_UNSUPPORTED;
    if (di + dt > features) return NFA_ERR_INVALID_ARGUMENT;
    if (batch == 0) return NFA_OK;
    if (!inputs || !packed || !identity_idx || !transform_idx || !outputs || !logabsdet) return NFA_ERR_INVALID_ARGUMENT;
    const F64LayerLayout l = f64_layer_layout(di, H, nb, dt, P);
    if (packed_doubles != l.total || !aligned16(packed)) return NFA_ERR_INVALID_ARGUMENT;
    const F64LayerPlan p = plan_f64_layer(l, di, batch, device_cu_count());

    F64LayerArgs a;
    a.x = inputs;
    a.out = outputs;
    a.lad = logabsdet;
    a.idf = identity_idx;
    a.tf = transform_idx;
    a.packed = packed;
    a.status = status;
    a.B = batch;
    a.tiles = p.tiles;
    a.D = features;
    a.di = di;
    a.dt = dt;
    a.H = H;
    a.P = P;
    a.nb = nb;
    a.accumulate = (flags & NFA_FLAG_ACCUMULATE_LOGABSDET) ? 1 : 0;
    a.NT = l.NT;
    a.ks0 = l.ks0;
    a.ksh = l.ksh;
    a.F = l.F;
    a.chunks = l.chunks;
    a.NTF = l.NTF;
    a.NTL = l.NTL;
    a.AS = p.AS;
    a.LS = p.LS;
    a.kc = p.kc;
    a.bufd = p.kc * p.max_nt * 64;
    a.w_blocks = l.w_blocks;
    a.w_final = l.w_final;
    a.b_in = l.b_in;
    a.b_blocks = l.b_blocks;
    a.b_final = l.b_final;
    a.s.nd = P - 2 * K;
    a.s.K = K;
    a.s.linear = linear;
    a.s.inverse = (flags & NFA_FLAG_INVERSE) ? 1 : 0;
    a.s.left = linear ? -spec->right : spec->left;
    a.s.right = spec->right;
    a.s.bottom = linear ? -spec->right : spec->bottom;
    a.s.top = linear ? spec->right : spec->top;
    a.s.min_w = spec->min_bin_width;
    a.s.min_h = spec->min_bin_height;
    a.s.min_d = spec->min_derivative;
    a.s.beta = spec->softplus_beta;
    a.s.tail_logit = spec->tail_logit;
    a.s.divisor = spec->wh_divisor;
    note_layer_kernel("k26::rqs_resnet_layer_f64_kernel<inverse=%d, nt=%d, chunks=%d x %d features, kc=%d, lds=%d, grid=%d, tiles=%lld>",
                      a.s.inverse, l.NT, l.chunks, l.F, p.kc, (int)p.lds, (int)p.grid, (long long)p.tiles);
    return launch_kernel(rqs_resnet_layer_f64_kernel, dim3((unsigned)p.grid), dim3(kBlock), p.lds, (hipStream_t)stream, a);
}
