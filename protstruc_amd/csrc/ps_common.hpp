// Shared device helpers for the protstruc geometry kernels (gfx950 only).
//
// Every translation unit is compiled with -ffp-contract=off: the reference's
// arithmetic is a chain of separate ATen / numpy multiplies, adds and
// subtracts, and fused multiply-adds change results that must be *exact*
// zeros there (e.g. the diagonal of pairwise_dihedrals, SURVEY hard part 4).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <utility>

#define PS_WAVE 64

struct f3 {
    float x, y, z;
};

__device__ __forceinline__ f3 mk3(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 sub3(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 scale3(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ f3 div3(f3 a, float s) { return f3{a.x / s, a.y / s, a.z / s}; }

// (x*y).sum(-1): products first, then adds (geometry.py:24-26).  ATen's sum
// accumulates from +0, so a dot product whose three terms are all -0 is +0 in
// the reference; that sign decides atan2(0, x) on degenerate (i == j) pairs, so
// the leading `0 +` is part of the contract (it is exact for every other input).
__device__ __forceinline__ float dot3(f3 a, f3 b) {
    float px = a.x * b.x, py = a.y * b.y, pz = a.z * b.z;
    return ((0.0f + px) + py) + pz;
}

// Correctly rounded sqrt for x >= 0 from v_rsq_f32: one coupled Newton step for g ~ sqrt(x) and h ~ 1/(2 sqrt(x)),
// then the exact-residual correction g + (x - g*g) * h (fma).  Every operation is a mul or an fma, so two elements
// share one v_pk_* instruction: 4 + 3.5 + 2 issue slots per element against 4 + 9 for a v_sqrt_f32 with two exact
// residual tests (sqrt_rn_pos, the first routine; kept in tools/microbench/sqrt_check.hip as the cross-check).  Zero, subnormal
// and +inf inputs are returned as x (sqrt(0) = 0 and sqrt(inf) = inf exactly; a subnormal squared distance means
// atoms closer than 1e-19, error < 1.1e-19).  Held to sqrtf over every non-negative float and to the correctly rounded
// np.sqrt over whole binades of mantissas by tests/test_gpu_arith.py (first by tools/microbench/sqrt_check.hip): equal for
// every x >= 2.0e-31 (atoms further apart than 4.5e-16), at most 1 ulp off below (1.8e6 of the normal floats
// below are: profiles/arith_probe_errors.json).  In K1's pattern kernel this takes the inner loop from 66 to 50 VALU instructions per 16-byte
// slot, which is what lets it reach its store-only time (profiles/r01_k1_ab_sqrt_mk.log).
__device__ __forceinline__ float sqrt_rn_mk(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    float g = x * y;
    float h = 0.5f * y;
    const float r = __builtin_fmaf(-h, g, 0.5f);
    g = __builtin_fmaf(g, r, g);
    h = __builtin_fmaf(h, r, h);
    const float d = __builtin_fmaf(-g, g, x);
    g = __builtin_fmaf(d, h, g);
    return __builtin_amdgcn_classf(x, 0x2F0) ? x : g;   // +-0, +-subnormal, +inf
}

// The squared length as the reference's torch.norm(v, dim=-1) evaluates it (protstruc.py:477-479, geometry.py:29-31):
// fma(z, z, fma(y, y, x * x)) -- ATen's CPU norm accumulates with fused multiply-adds (pinned bit for bit against
// ATen by tests/test_reference_arithmetic.py).  Written with explicit fmas: -ffp-contract=off still holds everywhere else.
__device__ __forceinline__ float norm_sq3(float x, float y, float z) {
    return __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x));
}

// |a - b| exactly as the reference evaluates it: differences, then norm_sq3, then a correctly rounded sqrt
__device__ __forceinline__ float dist3(f3 a, f3 b) {
    return sqrt_rn_mk(norm_sq3(a.x - b.x, a.y - b.y, a.z - b.z));
}

// the same with K1's choice of square root (ps_k1_config.exact_sqrt): hardware v_sqrt_f32 or correctly rounded
template <bool EXACT>
__device__ __forceinline__ float dist3_t(f3 a, f3 b) {
    const float x = norm_sq3(a.x - b.x, a.y - b.y, a.z - b.z);
    return EXACT ? sqrt_rn_mk(x) : __builtin_amdgcn_sqrtf(x);
}

// x.norm(dim=-1) (geometry.py:29-31); correctly rounded sqrt in half the instructions of the library routine
// (identical result unless the squared norm is below 2.0e-31, i.e. |a| < 4.5e-16)
__device__ __forceinline__ float norm3(f3 a) { return sqrt_rn_mk(norm_sq3(a.x, a.y, a.z)); }

// torch.linalg.cross (the reference's frames, geometry.py:437): one rounded product, then a fused multiply-add per
// component, fma(u_i, v_j, -(u_j * v_i)) -- pinned against ATen like norm_sq3.  Not for dihedrals: those use np.cross
// (cross3 below), whose exact cancellation on coincident arms the +0 diagonal of pairwise_dihedrals depends on.
__device__ __forceinline__ f3 cross3_fused(f3 u, f3 v) {
    f3 r;
    r.x = __builtin_fmaf(u.y, v.z, -(u.z * v.y));
    r.y = __builtin_fmaf(u.z, v.x, -(u.x * v.z));
    r.z = __builtin_fmaf(u.x, v.y, -(u.y * v.x));
    return r;
}

// np.cross component order: u1*v2 - u2*v1, ... two products then one subtract
__device__ __forceinline__ f3 cross3(f3 u, f3 v) {
    f3 r;
    r.x = u.y * v.z - u.z * v.y;
    r.y = u.z * v.x - u.x * v.z;
    r.z = u.x * v.y - u.y * v.x;
    return r;
}

// atan2 for the torsion kernels: odd minimax polynomial of degree 17 on [0,1], argument reduction by min/max and the
// usual quadrant fix-ups.  Against float64 on the MI355X (tests/test_gpu_arith.py, 3.7e6 points of the plane incl. the
// octant boundaries and their neighbours; profiles/arith_probe_errors.json): 1.41e-7 in the first octant -- the
// polynomial's 1.0e-7 plus the 1-ulp v_rcp_f32 and the rounded quotient -- and 2.87e-7 over the plane, where the
// subtractions from fl(pi / 2) and fl(pi) add their roundings; the test holds them to the derived 1.9e-7 and 5.0e-7.
// That is for max(|x|, |y|) in [2^-126, 2^126): below, v_rcp_f32 overflows (two subnormal arguments give NaN or an
// infinity, not an angle); from 2^126 on it underflows and the result, still a finite angle, can be off by pi / 4.
// IEEE special cases are kept: signed zeros (atan2(+0,-0) = pi, atan2(-0,+0) = -0), NaN propagation, inf/inf.  About
// half the instructions of the library routine; K3 is VALU-bound, so this is where its time goes.  The reference's own
// np.arctan2 / libm results differ from each other by similar amounts.
__device__ __forceinline__ float atan2_ps(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float a = mn * __builtin_amdgcn_rcpf(mx);
    a = (mx == 0.0f) ? 0.0f : a;                          // atan2(+-0, +-0)
    a = (mn == __builtin_huge_valf()) ? 1.0f : a;         // atan2(+-inf, +-inf)
    const float s = a * a;
    float p = 0.0028340641874819994f;
    p = __builtin_fmaf(p, s, -0.016005029901862144f);
    p = __builtin_fmaf(p, s, 0.042587608098983765f);
    p = __builtin_fmaf(p, s, -0.07495445758104324f);
    p = __builtin_fmaf(p, s, 0.10636754333972931f);
    p = __builtin_fmaf(p, s, -0.14202570915222168f);
    p = __builtin_fmaf(p, s, 0.19992484152317047f);
    p = __builtin_fmaf(p, s, -0.3333306610584259f);
    p = __builtin_fmaf(p, s, 1.0f);
    float r = a * p;
    r = (ay > ax) ? (1.5707963267948966f - r) : r;
    r = (__float_as_uint(x) >> 31) ? (3.141592653589793f - r) : r;
    r = (x != x || y != y) ? __builtin_nanf("") : r;
    return copysignf(r, y);
}

// acos for the planar-angle kernels: acos(|x|) = sqrt(1 - |x|) * P(|x|) with the degree-7 polynomial of Abramowitz &
// Stegun 4.4.46 (|error| <= 2e-8 in exact arithmetic), reflected for negative arguments.  Against float64 on the MI355X
// (tests/test_gpu_arith.py, 2.5e6 cosines incl. 2^-24 from +-1 and every float within 64 ulp of 0, +-0.5, +-1;
// profiles/arith_probe_errors.json): 2.66e-7 for x >= 0 and 4.54e-7 = 1.05 ulp of pi for x < 0, held to the derived 5.1e-7
// and 7.2e-7 -- the size of the library routine's error (3.1e-7).  acos_ps(1) = 0 and acos_ps(-1) = fl(pi) exactly.  |x| > 1 gives NaN
// through the square root of a negative number, as acos without a clamp does in the reference (geometry.py:64-71); NaN
// propagates.  14 instructions instead of the library's ~40: K3's planar-angle path is VALU-issue bound.
__device__ __forceinline__ float acos_ps(float x) {
    const float ax = fabsf(x);
    float p = -0.0012624911f;
    p = __builtin_fmaf(p, ax, 0.0066700901f);
    p = __builtin_fmaf(p, ax, -0.0170881256f);
    p = __builtin_fmaf(p, ax, 0.0308918810f);
    p = __builtin_fmaf(p, ax, -0.0501743046f);
    p = __builtin_fmaf(p, ax, 0.0889789874f);
    p = __builtin_fmaf(p, ax, -0.2145988016f);
    p = __builtin_fmaf(p, ax, 1.5707963050f);
    const float r = p * __builtin_amdgcn_sqrtf(1.0f - ax);
    return (__float_as_uint(x) >> 31) ? (3.141592653589793f - r) : r;
}

// geometry.dihedral (geometry.py:108-124), with the 1e-5 parity tolerance spent on ONE algebraic step (round 3):
//   reference:  n1 = b0 x b1,  n2 = b2 x b1,  x = n1 . n2,  y = ((n1 x n2) . b1) / |b1|
//   here:       n1, n2, x bit for bit as the reference;  (n1 x n2) = -(n1 . b2) b1 exactly in real arithmetic, so
//               y = -(n1 . b2) |b1| and, atan2 being invariant under a common positive factor,
//               atan2(y, x) = atan2(n1 . (c - d), x / |b1|):
// one cross product (9 of ~47 flops) fewer and no square root, only v_rsq_f32.  What must stay EXACT stays exact:
//   * c - d is the exact negative of the reference's b2 = d - c, and n2 = b1 x (c - d) has the reference's two products
//     per component and their difference, i.e. the same bits as b2 x b1;
//   * on the diagonal of pairwise_dihedrals (i == j) n1 or n2 is exactly 0, both dot products start from +0 (dot3), so
//     y = +0 and x = +0 * rsq = +0 and the result is +0.0 with no sign bit, as in the reference (golden G3);
//   * b1 = 0 gives x = 0 * inf = NaN like the reference's 0 / 0; NaN coordinates propagate.
// Everywhere else the result differs from the reference's by rounding only (max 2.4e-7 off-diagonal at unit scale
// before and after, tools/k3_error_stats.py; the conditioning gates of tests/test_gpu_parity.py hold it to the oracle
// and to fp64).
__device__ __forceinline__ float dihedral4(f3 a, f3 b, f3 c, f3 d) {
    f3 b0 = sub3(a, b);
    f3 b1 = sub3(c, b);
    f3 b2n = sub3(c, d);
    f3 n1 = cross3(b0, b1);
    f3 n2 = cross3(b1, b2n);
    float x = dot3(n1, n2) * __builtin_amdgcn_rsqf(dot3(b1, b1));
    float y = dot3(n1, b2n);
    return atan2_ps(y, x);
}

// Dot product of the FAST pairwise forms (round 5): fma(a.z, b.z, fma(a.y, b.y, fma(a.x, b.x, +0))) -- three instructions
// instead of five (K3's time is the vector unit's).  The first fma keeps dot3's `0 +`: a sum of -0 terms is still +0, which is
// what makes the (i == j) diagonal of pairwise_dihedrals exactly +0.0; a sum of exact zeros stays an exact zero.  Elsewhere
// it differs from the reference's products-then-adds by rounding only (one rounding instead of three: closer to the
// real dot product).  The cross products keep their unfused form: a * b - a * b has to cancel exactly on the diagonal.  The
// faithful forms (dihedral4_ref, angle3_ref: k3_arith.hpp) do not use it.
__device__ __forceinline__ float dot3_fast(f3 a, f3 b) {
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, __builtin_fmaf(a.x, b.x, 0.0f)));
}

// geometry.angle (geometry.py:64-71): no clamp before acos.  The reference divides the dot product by the product of
// two norms; here cos = ((ba . bc) * rsq(ba . ba)) * rsq(bc . bc) -- two v_rsq_f32 (1 ulp each) instead of two correctly
// rounded square roots and an IEEE divide (4 instructions instead of ~29) -- and acos_ps above.  Each arm is scaled away
// before the next factor comes in (round 5; rounds 3-4 multiplied the two squared lengths first, which overflowed for
// arms beyond 4e9 and underflowed below 1e-10): any arm between 1e-19 and 1e19 is safe, as in the reference.  A
// zero-length arm (the diagonal of pairwise_planar_angles) is 0 * rsq(0) = 0 * inf = NaN like the reference's 0 / 0.
__device__ __forceinline__ float angle3(f3 a, f3 b, f3 c) {
    f3 ba = sub3(a, b);
    f3 bc = sub3(c, b);
    return acos_ps((dot3_fast(ba, bc) * __builtin_amdgcn_rsqf(dot3_fast(ba, ba))) * __builtin_amdgcn_rsqf(dot3_fast(bc, bc)));
}

// float2, which gfx950 issues as packed v_pk_*_f32 instructions (the packed angle arithmetic built on it: k3_arith.hpp)
typedef float f32x2 __attribute__((ext_vector_type(2)));

// geometry.gram_schmidt (geometry.py:428-439); e3 uses the last-axis cross, torch.linalg.cross's fused form
__device__ __forceinline__ void gram_schmidt3(f3 a, f3 b, f3 c, f3& e1, f3& e2, f3& e3) {
    f3 v1 = sub3(c, b);
    e1 = div3(v1, norm3(v1));
    f3 v2 = sub3(a, b);
    float p = dot3(e1, v2);
    f3 u2 = sub3(v2, scale3(e1, p));
    e2 = div3(u2, norm3(u2));
    e3 = cross3_fused(e1, e2);
}

// geometry.place_fourth_atom (geometry.py:127-168), op for op: the X with |X - c| = length, angle(X, c, b) = planar and
// dihedral(a, b, c, X) = dihedral.  The sines and cosines are the library's accurate sincosf, not __sinf / v_sin_f32: the
// backbone builder (nerf.hip) chains thousands of these, and an angle error d at one residue moves every later atom by up
// to (distance) * d.  What ps_pointwise_f32 mode 3 and the builder both evaluate, so the two cannot drift apart.
__device__ __forceinline__ f3 place4(f3 a, f3 b, f3 c, float length, float planar, float dihedral) {
    f3 bc = sub3(b, c);
    bc = div3(bc, norm3(bc));
    f3 n = cross3(sub3(b, a), bc);
    n = div3(n, norm3(n));
    const f3 m = cross3(n, bc);
    float sp, cp, sd, cd;
    sincosf(planar, &sp, &cp);
    sincosf(dihedral, &sd, &cd);
    const float m0 = length * cp, m1 = length * sp * cd, m2 = -length * sp * sd;
    // c + sum([m0 * bc, m1 * m, m2 * n]): Python's sum starts from 0
    return f3{c.x + (((0.0f + m0 * bc.x) + m1 * m.x) + m2 * n.x), c.y + (((0.0f + m0 * bc.y) + m1 * m.y) + m2 * n.y),
              c.z + (((0.0f + m0 * bc.z) + m1 * m.z) + m2 * n.z)};
}

__device__ __forceinline__ f3 load3(const float* __restrict__ p) { return f3{p[0], p[1], p[2]}; }

// Launch `kernel` and return THIS launch's status.  hipLaunchKernel reports the result of the launch it performs;
// the sticky per-thread "last error" (which unrelated earlier HIP / PyTorch calls may have left set, and which
// hipGetLastError would both consume and misattribute) is neither read nor cleared.  Arguments are converted to
// the kernel's exact parameter types before their addresses are taken.
template <typename... KArgs, size_t... I>
static inline int ps_launch_impl(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                                 std::tuple<KArgs...>& params, std::index_sequence<I...>) {
    void* ptrs[] = {static_cast<void*>(&std::get<I>(params))...};
    return (int)hipLaunchKernel(reinterpret_cast<const void*>(kernel), grid, block, ptrs, lds, stream);
}

template <typename... KArgs, typename... Args>
static inline int ps_launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                            Args&&... args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "argument count does not match the kernel's parameter list");
    std::tuple<KArgs...> params(static_cast<KArgs>(args)...);
    return ps_launch_impl(kernel, grid, block, lds, stream, params, std::index_sequence_for<KArgs...>{});
}
