// Measurement aid of tools/f64_layer_time.py: the float64 matrix rate of this device as a register-resident loop of
// v_mfma_f64_16x16x4_f64 reaches it -- eight independent accumulator tiles per wave, no memory traffic, `waves` waves
// per SIMD.  Prints one JSON line.  Not part of the product.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) mfma_f64_loop(double* out, int iters) {
    const double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
    double4_t acc[8];
    for (int t = 0; t < 8; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
    }
    double s = 0.0;
    for (int t = 0; t < 8; ++t) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

#define CHECK(e)                                                        \
    do {                                                                \
        hipError_t err_ = (e);                                          \
        if (err_ != hipSuccess) {                                       \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));   \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main(int argc, char** argv) {
    const int waves = argc > 1 ? atoi(argv[1]) : 1;   // waves per SIMD: 1 or 2
    const int iters = argc > 2 ? atoi(argv[2]) : 20000;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount * waves;
    double* out;
    CHECK(hipMalloc(&out, sizeof(double) * 256 * blocks));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(mfma_f64_loop, dim3(blocks), dim3(256), 0, 0, out, iters / 10);   // warm-up
    CHECK(hipDeviceSynchronize());
    double best = 0.0;
    for (int rep = 0; rep < 3; ++rep) {
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(mfma_f64_loop, dim3(blocks), dim3(256), 0, 0, out, iters);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        const double flop = 2048.0 * 8 * iters * 4.0 * blocks;
        const double rate = flop / (ms * 1e-3) / 1e12;
        if (rate > best) best = rate;
    }
    printf("{\"f64_mfma_tflops\": %.3f, \"waves_per_simd\": %d, \"cus\": %d}\n", best, waves, prop.multiProcessorCount);
    CHECK(hipFree(out));
    return 0;
}
