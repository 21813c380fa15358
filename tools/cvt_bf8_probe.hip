// Round 10 probe: v_cvt_scalef32_pk_bf8_f32 -- the instruction that could make the bf8 byte of K8x's last piece straight from
// d = t - lo (f16x3_gemm.hpp: r' = RN16(256 d), of which the matrix instruction only reads the high byte).
//   (1) scale semantics: is the value multiplied or divided by the scale operand's power of two?  Both 2^8 and 2^-8 are run.
//   (2) rounding: for every f16 bit pattern q (zero, subnormals, normals, both signs, +-inf, NaNs) the input is
//       d = float(q) / 256, exact in fp32; the byte is compared with
//         T  the high byte of q                         (what the kernel makes today: RN16 is exact here, then truncation)
//         R  float(q) rounded to nearest even e5m2      (overflow: both the saturating and the infinite form are counted)
//   (3) op_sel: the upper half-word form leaves the lower half-word alone and vice versa; the two sources land in byte order.
//   hipcc --offload-arch=gfx950 -O3 -Wno-unused-value tools/cvt_bf8_probe.hip -o tools/bin/cvt_bf8_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

constexpr int kN = 65536;

__global__ void convert(const float* d, unsigned* out_lo, unsigned* out_hi, float scale, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = d[i], b = d[i ^ 1];
    unsigned lo = 0xa5a5a5a5u, hi = 0xa5a5a5a5u;
    asm volatile("v_cvt_scalef32_pk_bf8_f32 %0, %1, %2, %3" : "+v"(lo) : "v"(a), "v"(b), "v"(scale));
    asm volatile("v_cvt_scalef32_pk_bf8_f32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(hi) : "v"(a), "v"(b), "v"(scale));
    out_lo[i] = lo;
    out_hi[i] = hi;
}

static float half_bits_to_float(unsigned q) {
    const int s = q >> 15, e = (q >> 10) & 31, m = q & 1023;
    float v;
    if (e == 0) v = ldexpf((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = ldexpf(1.0f + m / 1024.0f, e - 15);
    return s ? -v : v;
}

// float(q) rounded to nearest even e5m2; SAT: overflow gives the largest finite value instead of infinity
static unsigned char round_e5m2(unsigned q, bool sat) {
    const unsigned s = (q >> 8) & 0x80, mag = q & 0x7fff;
    if (mag > 0x7c00) return (unsigned char)(s | 0x7f);            // NaN (any payload counts as NaN in the comparison)
    if (mag == 0x7c00) return (unsigned char)(s | (sat ? 0x7b : 0x7c));
    unsigned top = mag >> 8, rest = mag & 0xff;
    if (rest > 0x80 || (rest == 0x80 && (top & 1))) ++top;          // carries into the exponent as it should
    if (top >= 0x7c) top = sat ? 0x7b : 0x7c;
    return (unsigned char)(s | top);
}

static bool same_byte(unsigned char got, unsigned char want) {
    const bool gn = (got & 0x7c) == 0x7c && (got & 3), wn = (want & 0x7c) == 0x7c && (want & 3);
    if (gn || wn) return gn && wn;
    return got == want;
}

int main() {
    std::vector<float> d(kN);
    for (int q = 0; q < kN; ++q) d[q] = half_bits_to_float(q) / 256.0f;
    float* dd;
    unsigned *dlo, *dhi;
    if (hipMalloc(&dd, kN * 4) != hipSuccess || hipMalloc(&dlo, kN * 4) != hipSuccess || hipMalloc(&dhi, kN * 4) != hipSuccess) return 2;
    hipMemcpy(dd, d.data(), kN * 4, hipMemcpyHostToDevice);
    std::vector<unsigned> lo(kN), hi(kN);
    int verdict = 1;
    for (int trial = 0; trial < 2; ++trial) {
        const float scale = trial == 0 ? 0.00390625f : 256.0f;
        printf("scale operand %g\n", scale);
        convert<<<kN / 256, 256>>>(dd, dlo, dhi, scale, kN);
        if (hipDeviceSynchronize() != hipSuccess) return 3;
        hipMemcpy(lo.data(), dlo, kN * 4, hipMemcpyDeviceToHost);
        hipMemcpy(hi.data(), dhi, kN * 4, hipMemcpyDeviceToHost);
        long bad_t = 0, bad_rs = 0, bad_ri = 0, bad_either = 0, bad_layout = 0, bad_finite_t = 0, bad_finite_r = 0;
        int shown = 0;
        for (int q = 0; q < kN; ++q) {
            const unsigned char g0 = lo[q] & 0xff, g1 = (lo[q] >> 8) & 0xff;
            // layout: low form writes bytes 0, 1 and keeps bytes 2, 3; high form writes bytes 2, 3 with the same values
            if ((lo[q] >> 16) != 0xa5a5u || (hi[q] & 0xffffu) != 0xa5a5u || (hi[q] >> 16) != (lo[q] & 0xffffu)) ++bad_layout;
            // second source = pattern q ^ 1: its byte must be what pattern q ^ 1 gives as FIRST source
            if (g1 != (unsigned char)(lo[q ^ 1] & 0xff)) ++bad_layout;
            const unsigned char t = (unsigned char)(q >> 8), rs = round_e5m2(q, true), ri = round_e5m2(q, false);
            const bool ok_t = same_byte(g0, t), ok_rs = same_byte(g0, rs), ok_ri = same_byte(g0, ri);
            const bool finite = (q & 0x7c00) != 0x7c00;
            bad_t += !ok_t; bad_rs += !ok_rs; bad_ri += !ok_ri; bad_either += !(ok_t || ok_rs || ok_ri);
            if (finite && (ri & 0x7c) != 0x7c) { bad_finite_t += !ok_t; bad_finite_r += !ok_rs; }
            if (!(ok_t || ok_rs || ok_ri) && shown < 8) {
                printf("    q = 0x%04x  d = %.9g  byte 0x%02x  (truncation 0x%02x, rounded 0x%02x / 0x%02x)\n", q, d[q], g0, t, rs, ri);
                ++shown;
            }
        }
        printf("    of %d patterns, byte differs from truncation %ld, from RNE saturating %ld, from RNE to infinity %ld, "
               "from all three %ld; finite results only: truncation %ld, RNE %ld; layout / op_sel mismatches %ld\n",
               kN, bad_t, bad_rs, bad_ri, bad_either, bad_finite_t, bad_finite_r, bad_layout);
        printf("    samples (q -> byte): 0x0000 -> 0x%02x, 0x8000 -> 0x%02x, 0x0001 -> 0x%02x, 0x00ff -> 0x%02x, 0x0180 -> 0x%02x, 0x3c00 -> 0x%02x, "
               "0x3d80 -> 0x%02x, 0x7bff -> 0x%02x, 0x7c00 -> 0x%02x, 0xfc00 -> 0x%02x, 0x7e00 -> 0x%02x\n",
               lo[0x0000] & 0xff, lo[0x8000] & 0xff, lo[0x0001] & 0xff, lo[0x00ff] & 0xff, lo[0x0180] & 0xff, lo[0x3c00] & 0xff,
               lo[0x3d80] & 0xff, lo[0x7bff] & 0xff, lo[0x7c00] & 0xff, lo[0xfc00] & 0xff, lo[0x7e00] & 0xff);
        if (bad_either == 0 && bad_layout == 0) verdict = 0;
    }
    printf(verdict == 0 ? "VERDICT: one scale setting gives truncation or correct rounding for every pattern\n"
                        : "VERDICT: the instruction does not behave as modelled\n");
    hipFree(dd); hipFree(dlo); hipFree(dhi);
    return verdict;
}
