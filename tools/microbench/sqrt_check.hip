// Exhaustive check of candidate fp32 square roots against the correctly rounded library sqrtf over every
// non-negative float (0 .. +inf, 2^31 bit patterns): which candidates are correctly rounded everywhere?
//   A: sqrt_rn_pos   (v_sqrt_f32 + two exact residual tests; defined below: the product's first routine, kept here as
//                     the cross-check of B)
//   B: sqrt_rn_mk    (v_rsq_f32 + one coupled Newton step for g ~ sqrt(x), h ~ 1/(2 sqrt(x)) + exact residual
//                     correction g + (x - g*g) * h; zero / subnormal / inf inputs returned as x; the product routine in
//                     ps_common.hpp)
//   C: raw v_sqrt_f32 (how often, and by how much, is the hardware instruction itself off?)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <cstring>
#include "../../protstruc_amd/csrc/ps_common.hpp"

// Correctly rounded sqrt for x >= 0 without the subnormal pre-scaling of the library routine: v_sqrt_f32 is within 1 ulp, so
// the answer is s-1ulp, s or s+1ulp and two exact fma residuals pick it.  0, inf and NaN fall through unchanged (every
// comparison with a NaN residual is false).  Equal to sqrtf for every x >= 4.6e-32; below that the residuals underflow and
// the result can be 1 ulp off.
__device__ __forceinline__ float sqrt_rn_pos(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float lo = __uint_as_float(__float_as_uint(s) - 1u);
    const float hi = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_lo = __builtin_fmaf(-lo, s, x);
    const float r_hi = __builtin_fmaf(-hi, s, x);
    float r = s;
    r = (r_lo <= 0.0f) ? lo : r;
    r = (r_hi > 0.0f) ? hi : r;
    return r;
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("ERR %s line %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

__global__ void check(unsigned long long* counts, unsigned* first_bad, unsigned* last_bad) {
    const unsigned long long n = 0x7F800001ull;  // 0 .. +inf inclusive
    unsigned long long badA = 0, badB = 0, badB_sub = 0, badC = 0, badC2 = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __uint_as_float((unsigned)i);
        const float ref = sqrtf(x);
        const float a = sqrt_rn_pos(x);
        const float b = sqrt_rn_mk(x);
        const bool sub = (i != 0) && (i < 0x00800000ull);
        if (!sub) {
            const int dc = (int)__float_as_uint(__builtin_amdgcn_sqrtf(x)) - (int)__float_as_uint(ref);
            if (dc != 0) ++badC;
            if (dc > 1 || dc < -1) ++badC2;
        }
        if (__float_as_uint(a) != __float_as_uint(ref) && !sub) {
            ++badA;
            atomicMax(&last_bad[0], (unsigned)i);
        }
        if (__float_as_uint(b) != __float_as_uint(ref)) {
            if (sub) ++badB_sub;
            else {
                ++badB;
                atomicMin(first_bad, (unsigned)i);
                atomicMax(&last_bad[1], (unsigned)i);
            }
        }
    }
    atomicAdd(&counts[0], badA);
    atomicAdd(&counts[1], badB);
    atomicAdd(&counts[2], badB_sub);
    atomicAdd(&counts[3], badC);
    atomicAdd(&counts[4], badC2);
}

int main() {
    unsigned long long* c; unsigned* fb; unsigned* lb;
    CK(hipMalloc(&lb, 8)); CK(hipMemset(lb, 0, 8));
    CK(hipMalloc(&c, 5 * sizeof(unsigned long long))); CK(hipMemset(c, 0, 5 * sizeof(unsigned long long)));
    CK(hipMalloc(&fb, 4)); CK(hipMemset(fb, 0xFF, 4));
    check<<<4096, 256>>>(c, fb, lb);
    CK(hipDeviceSynchronize());
    unsigned long long h[5]; unsigned hfb;
    CK(hipMemcpy(h, c, sizeof(h), hipMemcpyDeviceToHost)); CK(hipMemcpy(&hfb, fb, 4, hipMemcpyDeviceToHost));
    unsigned hlb[2]; CK(hipMemcpy(hlb, lb, 8, hipMemcpyDeviceToHost));
    { float fa, fb2; memcpy(&fa, &hlb[0], 4); memcpy(&fb2, &hlb[1], 4);
      printf("largest mismatching input: sqrt_rn_pos 0x%08x (%g), sqrt_rn_mk 0x%08x (%g)\n", hlb[0], fa, hlb[1], fb2); }
    printf("inputs checked: 0x7F800001 (every float in [0, +inf])\n");
    printf("sqrt_rn_pos  != sqrtf on normal/zero/inf inputs: %llu\n", h[0]);
    printf("sqrt_rn_mk   != sqrtf on normal/zero/inf inputs: %llu (first bad bits 0x%08x)\n", h[1], hfb);
    printf("sqrt_rn_mk   != sqrtf on subnormal inputs:       %llu of 8388607 (returned as x by design)\n", h[2]);
    printf("raw v_sqrt_f32 != sqrtf on normal/zero/inf inputs: %llu (%.2f %%), of which more than 1 ulp off: %llu\n", h[3], 100.0 * h[3] / 2139095041.0, h[4]);
    return 0;
}
