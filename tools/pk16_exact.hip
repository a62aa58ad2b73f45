// pk16_exact.hip -- exactness of the packed f16 SW cell (batch_scores.hip.h, CELL16) on the device, over the scaled integers
// k * 2^-11, k in [-2048, 2048] -- the two adds over every pair, the three-input maximum over every pair and six third operands:
//   (1) v_pk_add_f16 ... clamp of every pair (a, b): must be clamp(a + b, 0, 2048) * 2^-11 in both halves (bit for bit, +0.0 below 0);
//       and the plain v_pk_add_f16 of every pair with |a + b| <= 2048: a + b exactly
//   (2) v_pk_maximum3_f16 of every pair (a, b) against c in {-0.0, +0.0, -2^-11, 2^-11, -1, 1}: the larger value, and +0.0 when the
//       largest value is a zero of either sign that meets +0.0
//   (3) v_perm_b32 selector bytes 12 and 13: 0x00 and 0xff whatever the sources
//   (4) the integer-coded profile cell (PROF16, integer form): bit patterns k in [0, 2304] read as f16 (k < 0x0400 are denormals):
//       v_pk_maximum3_f16 of every pair (a, b) against c in {0, 1, a, b, 2304, 0x3c00} must be the integer maximum in both halves, and
//       v_pk_sub_u16 ... clamp of every pair must be max(a - b, 0) / max(b - a, 0); under the mode register a HIP kernel starts with,
//       which is printed
//   hipcc --offload-arch=gfx950 -O2 -o tools/pk16_exact tools/pk16_exact.hip && tools/pk16_exact
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#define K 2048
#define NV (2 * K + 1)

__device__ uint32_t bits_of(int k) {   // f16 bit pattern of k * 2^-11 (|k| <= 2048)
    if (k == 0) return 0;
    const uint32_t sign = k < 0 ? 0x8000u : 0u, a = (uint32_t)(k < 0 ? -k : k);
    int e = 31 - __builtin_clz(a);
    return sign | ((uint32_t)(e + 4) << 10) | ((a - (1u << e)) << (10 - e));
}
__device__ unsigned long long fails[8];

__global__ void probe(uint32_t s_any) {
    const int a = (int)blockIdx.x - K;
    const uint32_t c3[6] = {0x8000u, 0u, 0x9000u, 0x1000u, 0xbc00u, 0x3c00u};   // -0, +0, -2^-11, 2^-11, -1, 1
    const float c3v[6] = {-0.0f, 0.0f, -1.0f / 2048, 1.0f / 2048, -1.0f, 1.0f};
    for (int b = (int)threadIdx.x - K; b <= K; b += blockDim.x) {
        const uint32_t x = bits_of(a) | (bits_of(b) << 16), y = bits_of(b) | (bits_of(a) << 16);
        uint32_t r;
        asm volatile("v_pk_add_f16 %0, %1, %2 clamp" : "=v"(r) : "v"(x), "v"(y));
        const int sum = a + b, cl = sum < 0 ? 0 : (sum > K ? K : sum);
        if (r != (bits_of(cl) | (bits_of(cl) << 16))) atomicAdd(&fails[0], 1ull);
        if (sum >= -K && sum <= K) {
            asm volatile("v_pk_add_f16 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
            const uint32_t want = bits_of(sum);   // (+0.0 for a + b = 0: round to nearest)
            if (r != (want | (want << 16))) atomicAdd(&fails[1], 1ull);
        }
        for (int i = 0; i < 6; ++i) {
            asm volatile("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(c3[i] | (c3[i] << 16)));
            const float fa = a / 2048.0f, fb = b / 2048.0f, fc = c3v[i];
            float mx = fmaxf(fmaxf(fa, fb), fc);
            uint32_t want;
            if (mx == 0.0f) {   // IEEE maximum: +0 > -0
                const bool pos = (fa == 0.0f && !signbit(fa)) || (fb == 0.0f && !signbit(fb)) || (fc == 0.0f && !signbit(fc));
                want = pos ? 0u : 0x8000u;
            } else {
                want = (mx == fc) ? c3[i] : bits_of((int)lrintf(mx * 2048.0f));
            }
            if (r != (want | (want << 16))) atomicAdd(&fails[2], 1ull);
        }
        asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(r) : "s"(s_any), "v"(x), "v"(0x0c0c0c0cu));
        if (r != 0u) atomicAdd(&fails[3], 1ull);
        asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(r) : "s"(s_any), "v"(x), "v"(0x0d0d0d0du));
        if (r != 0xffffffffu) atomicAdd(&fails[4], 1ull);
        atomicAdd(&fails[5], 1ull);
    }
}

#define KI 2304
__device__ unsigned long long ifails[8];
__device__ uint32_t mode_reg;

__global__ void probe_int() {
    const uint32_t a = blockIdx.x;
    if (a == 0 && threadIdx.x == 0) {
        uint32_t m;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_MODE)" : "=s"(m));
        mode_reg = m;
    }
    for (uint32_t b = threadIdx.x; b <= KI; b += blockDim.x) {
        const uint32_t x = a | (b << 16), y = b | (a << 16);
        const uint32_t c3[6] = {0u, 1u, a, b, (uint32_t)KI, 0x3c00u};
        const uint32_t mab = a > b ? a : b;
        uint32_t r;
        for (int i = 0; i < 6; ++i) {
            asm volatile("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(c3[i] | (c3[i] << 16)));
            const uint32_t want = mab > c3[i] ? mab : c3[i];
            if (r != (want | (want << 16))) {
                atomicAdd(&ifails[0], 1ull);
                if (want < 0x0400u) atomicAdd(&ifails[1], 1ull);   // the expected maximum is a denormal pattern
            }
        }
        asm volatile("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(x), "v"(y));
        if (r != ((a > b ? a - b : 0u) | ((b > a ? b - a : 0u) << 16))) atomicAdd(&ifails[2], 1ull);
        // the row step's one 32-bit add for both halves: no carry out of the low half below 2^16
        asm volatile("v_add_u32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
        if (r != ((a + b) | ((a + b) << 16))) atomicAdd(&ifails[3], 1ull);
        atomicAdd(&ifails[4], 1ull);
    }
}

int main() {
    unsigned long long z[8] = {}, h[8];
    (void)hipMemcpyToSymbol(HIP_SYMBOL(fails), z, sizeof z);
    hipLaunchKernelGGL(probe, dim3(NV), dim3(256), 0, 0, 0xdeadbeefu);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(fails), sizeof h);
    printf("pairs (a, b), a, b in [-2048, 2048]: %llu\n", h[5]);
    printf("v_pk_add_f16 clamp  == clamp(a+b, 0, 2048) * 2^-11 (both halves): %llu mismatches\n", h[0]);
    printf("v_pk_add_f16        == (a+b) * 2^-11 for |a+b| <= 2048:            %llu mismatches\n", h[1]);
    printf("v_pk_maximum3_f16   == max(a, b, c), c in {-0,+0,-2^-11,2^-11,-1,1}, +0 over -0: %llu mismatches (of %llu)\n", h[2], 6 * h[5]);
    printf("v_perm_b32 selector 12 -> 0x00: %llu mismatches; selector 13 -> 0xff: %llu mismatches\n", h[3], h[4]);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(ifails), z, sizeof z);
    hipLaunchKernelGGL(probe_int, dim3(KI + 1), dim3(256), 0, 0);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    unsigned long long hi[8];
    uint32_t mode = 0;
    (void)hipMemcpyFromSymbol(hi, HIP_SYMBOL(ifails), sizeof hi);
    (void)hipMemcpyFromSymbol(&mode, HIP_SYMBOL(mode_reg), sizeof mode);
    printf("integer patterns (a, b), a, b in [0, %d]: %llu pairs; MODE = 0x%08x (FP_DENORM bits 7:4 = 0x%x: f32 = %u, f64/f16 = %u; 3 = denormals kept)\n", KI,
           hi[4], mode, (mode >> 4) & 0xfu, (mode >> 4) & 3u, (mode >> 6) & 3u);
    printf("v_pk_maximum3_f16   == integer max(a, b, c), c in {0, 1, a, b, %d, 0x3c00} (both halves): %llu mismatches (of %llu), %llu of them with a\n"
           "                       denormal pattern (< 0x0400) expected%s\n", KI, hi[0], 6 * hi[4], hi[1],
           hi[1] ? ": THE MAXIMUM FLUSHES F16 DENORMALS IN THIS MODE" : " -- f16 denormals are not flushed");
    printf("v_pk_sub_u16 clamp  == max(a - b, 0), max(b - a, 0):                                      %llu mismatches\n", hi[2]);
    printf("v_add_u32           == (a + b) in both halves, no carry between them:                    %llu mismatches\n", hi[3]);
    return (h[0] | h[1] | h[2] | h[3] | h[4] | hi[0] | hi[2] | hi[3]) ? 2 : 0;
}
