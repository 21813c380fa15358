// Device side of plan_row_sum (launch_plan.hpp), shared by the kernels that write one float64-summed number per row of an
// elementwise map: K18 (nonlin.hip) and K20 (density.hip).  The plan fixes who visits which element; what is here fixes the
// order in which a row's float64 terms are added, so two kernels on the same plan add in the same order:
//   rows regime    every element's term sits in LDS (`terms`, the workgroup's range in element order); `group` lanes share a
//                  row -- lane g adds the terms g, g + group, ... in order, then a shuffle tree --: rowsum_rows
//   pieces regime  a lane adds its own elements' terms in the order it visits them; the lanes are merged in a shuffle tree
//                  per wave and the four waves in wave order: rowsum_block_sum; with more than one piece per row the piece
//                  sums go to a float64 workspace [batch][pieces] and a second launch adds them in piece order: rowsum_pieces
// No atomics.  Include after common.hpp.
#pragma once

namespace nfa {

template <int V>
__device__ __forceinline__ void rowsum_load(const float* src, float* v) {
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
__device__ __forceinline__ void rowsum_store(float* dst, const float* v) {
    if (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else *dst = v[0];
}

// the sum of `v` over the workgroup's lanes: a shuffle tree per wave, the waves in wave order; valid in lane 0
// (s_w: kBlock / kWave doubles of LDS; contains a __syncthreads: call it from every lane)
__device__ __forceinline__ double rowsum_block_sum(double v, double* s_w, int tid) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if ((tid & (kWave - 1)) == 0) s_w[tid / kWave] = v;
    __syncthreads();
    double total = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) total += s_w[w];
    }
    return total;
}

// rows regime, after a __syncthreads behind the last write to `terms`: put(r, sum) is called once for each of the
// workgroup's `rows` rows of n terms, by the first lane of the row's group
template <typename Put>
__device__ __forceinline__ void rowsum_rows(const double* terms, int rows, int n, int G, int tid, Put&& put) {
    const int per_pass = kBlock / G;
    const int g = tid & (G - 1), slot = tid / G;
    for (int r0 = 0; r0 < rows; r0 += per_pass) {
        const int r = r0 + slot;
        double acc = 0.0;
        if (r < rows) {
            const double* c = terms + r * n;
            for (int i = g; i < n; i += G) acc += c[i];
        }
        for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, G);
        if (r < rows && g == 0) put(r, acc);
    }
}

// the pieces of a row, in piece order
__device__ __forceinline__ double rowsum_pieces(const double* ws, int64_t row, int pieces) {
    double acc = 0.0;
    for (int s = 0; s < pieces; ++s) acc += ws[row * pieces + s];
    return acc;
}

}  // namespace nfa
