// Test-only probe of the float32 arithmetic primitives of csrc/ps_common.hpp and csrc/k3_arith.hpp: one C entry point that
// evaluates ONE primitive elementwise over caller-supplied arrays, so that tests/test_gpu_arith.py can hold each routine
// to float64 and the scalar / packed / multi-column forms to each other on inputs the geometry kernels never produce.
// Not part of the product: not declared in include/protstruc_hip.h, not linked into libprotstruc_hip.so; built by
// protstruc_amd.build.build_arith_probe() with exactly the library's flags (-ffp-contract=off is part of the contract).
//
//   int ps_arith_probe_f32(int which, const float* a, const float* b, float* out, long long n, void* stream)
//
// out[i] = f(a[i]) or f(a[i], b[i]); for the two-argument routines a is the FIRST argument (y of atan2(y, x), the
// numerator of a / b) and b the second.  Arms (tests/arith_probe.py names them):
//    0.. 6  scalar:  sqrt_rn_mk, atan2_ps, atan2_k3, acos_ps, atan2_lib, acos_lib, the compiler's a / b
//   10..13  packed (two elements per lane):  sqrt_rn_mk_v, atan2_ps_v, atan2_k3_v, acos_ps_v
//   20..24  two columns per lane:   atan2_k3_vn<2>, acos_ps_vn<2>, atan2_lib_vn<2>, acos_lib_vn<2>, div_ieee_vn<2>
//   30..34  four columns per lane:  the same with NC = 4 (the two instantiations pairwise_angles.hip / featuriser.hip use)
//   40..42  the device library:  atan2f, acosf, sqrtf
// Scalar and library arms run in a per-lane loop whose operands are loaded anew in every iteration: how the compiler lowers
// the library's `!fpmath` division depends on the call site (k3_arith.hpp), and this is the call site of
// tools/microbench/libm_identity.hip.
// Packed and NC-column arms: one lane owns 2 * NC consecutive elements (NC = 1 for the *_v forms); element e of the lane is
// column (e / 2) % NC, half e % 2.  Loads past n are replaced by 1.0f, stores past n are not made.
// Bad arguments (null pointer, n < 0, unknown arm) return hipErrorInvalidValue before anything is launched; n == 0
// launches nothing.  Plain vector loads and stores, 256-thread blocks, no LDS.
#include "k3_arith.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kLoop = 4;                       // iterations per lane the scalar grid is sized for
constexpr long long kMaxBlocks = 1ll << 22;    // the per-lane loop takes whatever a larger n leaves

enum Arm {
    SQRT_RN_MK = 0, ATAN2_PS = 1, ATAN2_K3 = 2, ACOS_PS = 3, ATAN2_LIB = 4, ACOS_LIB = 5, DIV = 6,
    SQRT_RN_MK_V = 10, ATAN2_PS_V = 11, ATAN2_K3_V = 12, ACOS_PS_V = 13,
    ATAN2_K3_VN = 0, ACOS_PS_VN = 1, ATAN2_LIB_VN = 2, ACOS_LIB_VN = 3, DIV_IEEE_VN = 4,   // + 20 (NC = 2), + 30 (NC = 4)
    LIB_ATAN2F = 40, LIB_ACOSF = 41, LIB_SQRTF = 42,
};

template <int W>
__device__ __forceinline__ float scalar_arm(float a, float b) {
    if constexpr (W == SQRT_RN_MK) return sqrt_rn_mk(a);
    else if constexpr (W == ATAN2_PS) return atan2_ps(a, b);
    else if constexpr (W == ATAN2_K3) return atan2_k3(a, b);
    else if constexpr (W == ACOS_PS) return acos_ps(a);
    else if constexpr (W == ATAN2_LIB) return atan2_lib(a, b);
    else if constexpr (W == ACOS_LIB) return acos_lib(a);
    else if constexpr (W == DIV) return a / b;
    else if constexpr (W == LIB_ATAN2F) return atan2f(a, b);
    else if constexpr (W == LIB_ACOSF) return acosf(a);
    else return sqrtf(a);
}

template <int W, bool TWO>
__global__ __launch_bounds__(kThreads) void scalar_kernel(const float* a, const float* b, float* out, long long n) {
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const float u = a[i];
        const float v = TWO ? b[i] : 0.0f;
        out[i] = scalar_arm<W>(u, v);
    }
}

// W: 10..13 with NC = 1, or the *_VN index with NC = 2 / 4
template <int W, int NC, bool TWO>
__global__ __launch_bounds__(kThreads) void packed_kernel(const float* a, const float* b, float* out, long long n) {
    const long long base = ((long long)blockIdx.x * kThreads + threadIdx.x) * (2 * NC);
    if (base >= n) return;
    f32x2 u[NC], v[NC], r[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const long long e0 = base + 2 * c, e1 = e0 + 1;
        u[c] = f32x2{e0 < n ? a[e0] : 1.0f, e1 < n ? a[e1] : 1.0f};
        v[c] = TWO ? f32x2{e0 < n ? b[e0] : 1.0f, e1 < n ? b[e1] : 1.0f} : f32x2{1.0f, 1.0f};
    }
    if constexpr (NC == 1) {
        if constexpr (W == SQRT_RN_MK_V) r[0] = sqrt_rn_mk_v(u[0]);
        else if constexpr (W == ATAN2_PS_V) r[0] = atan2_ps_v(u[0], v[0]);
        else if constexpr (W == ATAN2_K3_V) r[0] = atan2_k3_v(u[0], v[0]);
        else r[0] = acos_ps_v(u[0]);
    } else {
        if constexpr (W == ATAN2_K3_VN) atan2_k3_vn<NC>(u, v, r);
        else if constexpr (W == ACOS_PS_VN) acos_ps_vn<NC>(u, r);
        else if constexpr (W == ATAN2_LIB_VN) atan2_lib_vn<NC>(u, v, r);
        else if constexpr (W == ACOS_LIB_VN) acos_lib_vn<NC>(u, r);
        else div_ieee_vn<NC>(u, v, r);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const long long e0 = base + 2 * c, e1 = e0 + 1;
        if (e0 < n) out[e0] = r[c].x;
        if (e1 < n) out[e1] = r[c].y;
    }
}

template <int W, bool TWO>
int launch_scalar(const float* a, const float* b, float* out, long long n, hipStream_t stream) {
    const long long per_block = (long long)kThreads * kLoop;
    long long blocks = (n + per_block - 1) / per_block;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    return ps_launch(scalar_kernel<W, TWO>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, b, out, n);
}

template <int W, int NC, bool TWO>
int launch_packed(const float* a, const float* b, float* out, long long n, hipStream_t stream) {
    const long long per_block = (long long)kThreads * 2 * NC;
    const long long blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return (int)hipErrorInvalidValue;
    return ps_launch(packed_kernel<W, NC, TWO>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, b, out, n);
}

template <int NC>
int launch_vn(int w, const float* a, const float* b, float* out, long long n, hipStream_t stream) {
    switch (w) {
        case ATAN2_K3_VN: return launch_packed<ATAN2_K3_VN, NC, true>(a, b, out, n, stream);
        case ACOS_PS_VN: return launch_packed<ACOS_PS_VN, NC, false>(a, b, out, n, stream);
        case ATAN2_LIB_VN: return launch_packed<ATAN2_LIB_VN, NC, true>(a, b, out, n, stream);
        case ACOS_LIB_VN: return launch_packed<ACOS_LIB_VN, NC, false>(a, b, out, n, stream);
        default: return launch_packed<DIV_IEEE_VN, NC, true>(a, b, out, n, stream);
    }
}

// 1 or 2 arguments of a valid arm, 0 for an unknown one
int arity(int which) {
    switch (which) {
        case SQRT_RN_MK: case ACOS_PS: case ACOS_LIB: case SQRT_RN_MK_V: case ACOS_PS_V: case LIB_ACOSF: case LIB_SQRTF:
        case 20 + ACOS_PS_VN: case 20 + ACOS_LIB_VN: case 30 + ACOS_PS_VN: case 30 + ACOS_LIB_VN:
            return 1;
        case ATAN2_PS: case ATAN2_K3: case ATAN2_LIB: case DIV: case ATAN2_PS_V: case ATAN2_K3_V: case LIB_ATAN2F:
        case 20 + ATAN2_K3_VN: case 20 + ATAN2_LIB_VN: case 20 + DIV_IEEE_VN:
        case 30 + ATAN2_K3_VN: case 30 + ATAN2_LIB_VN: case 30 + DIV_IEEE_VN:
            return 2;
        default:
            return 0;
    }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int ps_arith_probe_f32(int which, const float* a, const float* b, float* out,
                                                                        long long n, void* stream_) {
    const int args = arity(which);
    if (args == 0 || n < 0 || a == nullptr || out == nullptr || (args == 2 && b == nullptr)) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    switch (which) {
        case SQRT_RN_MK: return launch_scalar<SQRT_RN_MK, false>(a, b, out, n, stream);
        case ATAN2_PS: return launch_scalar<ATAN2_PS, true>(a, b, out, n, stream);
        case ATAN2_K3: return launch_scalar<ATAN2_K3, true>(a, b, out, n, stream);
        case ACOS_PS: return launch_scalar<ACOS_PS, false>(a, b, out, n, stream);
        case ATAN2_LIB: return launch_scalar<ATAN2_LIB, true>(a, b, out, n, stream);
        case ACOS_LIB: return launch_scalar<ACOS_LIB, false>(a, b, out, n, stream);
        case DIV: return launch_scalar<DIV, true>(a, b, out, n, stream);
        case LIB_ATAN2F: return launch_scalar<LIB_ATAN2F, true>(a, b, out, n, stream);
        case LIB_ACOSF: return launch_scalar<LIB_ACOSF, false>(a, b, out, n, stream);
        case LIB_SQRTF: return launch_scalar<LIB_SQRTF, false>(a, b, out, n, stream);
        case SQRT_RN_MK_V: return launch_packed<SQRT_RN_MK_V, 1, false>(a, b, out, n, stream);
        case ATAN2_PS_V: return launch_packed<ATAN2_PS_V, 1, true>(a, b, out, n, stream);
        case ATAN2_K3_V: return launch_packed<ATAN2_K3_V, 1, true>(a, b, out, n, stream);
        case ACOS_PS_V: return launch_packed<ACOS_PS_V, 1, false>(a, b, out, n, stream);
        default: return which < 30 ? launch_vn<2>(which - 20, a, b, out, n, stream) : launch_vn<4>(which - 30, a, b, out, n, stream);
    }
}
