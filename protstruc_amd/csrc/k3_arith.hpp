// Arithmetic that only the pairwise angle kernels use (K3: pairwise_angles.hip, and the fused featuriser: featuriser.hip),
// on top of the shared scalar helpers of ps_common.hpp:
//   * the FAITHFUL scalar forms: atan2_lib, acos_lib, dihedral4_ref, angle3_ref;
//   * the pairwise kernels' fast atan2 and dihedral: atan2_k3, dihedral4_k3;
//   * two problems per lane (f3v, *_v): packed v_pk_*_f32 arithmetic;
//   * NC column residues per lane (*_vn, *_n): the columns' dependent chains interleaved;
//   * the faithful forms in that packed, NC-column shape (div_ieee_vn, atan2_lib_vn, acos_lib_vn, dihedral4v_ref_n,
//     angle3v_ref_n).
// Each scalar / packed / NC-column variant of a routine performs the same operations in the same order per element, so
// they agree bit for bit; tests/test_gpu_arith.py holds each variant to its scalar form routine by routine (samples of the
// plane, special values in every (column, half) slot, tails), tests/test_gpu_parity.py the kernels built on them to each other.
#pragma once

#include "ps_common.hpp"

// ---- the FAITHFUL forms (round 4): geometry.dihedral / geometry.angle op for op in the reference's order ----
// What `exact_angles` of ps_pairwise_angles_f32 / ps_inter_residue_geometry_f32 selects, as `exact_sqrt` does for K1: three
// cross products, y divided by |b1| (correctly rounded square root, IEEE division), atan2 / acos in the device library's
// arithmetic (against float64 on the MI355X, tests/test_gpu_arith.py and profiles/arith_probe_errors.json: atan2 2.65 ulp
// = 3.0e-7, acos 1.44 ulp = 3.1e-7; the reference's np.arctan2 / torch.arccos are libm-grade as well) -- no algebraic
// rewriting, no reciprocal square roots, no polynomials of this file.
//
// atan2_lib / acos_lib (round 5) ARE the device library's atan2f / acosf (ROCm 7.2 ocml: __ocml_atan2_f32 with its
// __ocmlpriv_atanred_f32, __ocml_acos_f32; denormals on, finite-only off), written out instruction for instruction as hipcc
// -O3 emits a call of them on gfx950 -- read off ocml.bc's IR and the ISA of a one-line kernel -- instead of being called.
// Why not call them: the library asks for its v / u division with `!fpmath 2.5 ulp`, and whether the compiler then emits
// the cheap form (frexp mantissas, v_rcp_f32, v_ldexp_f32) or a full IEEE division turned out to depend on the CALL SITE
// (inside a loop body: the cheap form; hoisted out of a loop whose operands are all loop-invariant -- K3 with every point
// from the column residue -- the IEEE form): two kernels calling atan2f on the same arguments disagreed in the last bit on
// 13 % of them.  Written with builtins the sequence is the same everywhere; it is the cheap form, which is what a plain
// call gives, and tests/test_gpu_arith.py holds it to such calls on every run of the suite -- acosf on all 2^32 arguments,
// atan2f on 4e7 pairs (the plane, random bit patterns, the special values), scalar and packed forms alike; a ROCm whose
// ocml differs fails there.  (First checked over 2^32 pairs by tools/microbench/libm_identity.hip,
// profiles/r05_libm_identity.log.)
__device__ __forceinline__ float atan2_lib(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float v = __builtin_fminf(ax, ay), u = __builtin_fmaxf(ax, ay);
    const float m = __builtin_amdgcn_frexp_mantf(v) * __builtin_amdgcn_rcpf(__builtin_amdgcn_frexp_mantf(u));
    const float q = __builtin_amdgcn_ldexpf(m, __builtin_amdgcn_frexp_expf(v) - __builtin_amdgcn_frexp_expf(u));
    const float t = q * q;
    float p = __builtin_fmaf(t, __uint_as_float(0x3b2d2a58u), __uint_as_float(0xbc7a590cu));
    p = __builtin_fmaf(t, p, __uint_as_float(0x3d29fb3fu));
    p = __builtin_fmaf(t, p, __uint_as_float(0xbd97d4d7u));
    p = __builtin_fmaf(t, p, __uint_as_float(0x3dd931b2u));
    p = __builtin_fmaf(t, p, __uint_as_float(0xbe1160e6u));
    p = __builtin_fmaf(t, p, __uint_as_float(0x3e4cb8bfu));
    p = __builtin_fmaf(t, p, __uint_as_float(0xbeaaaa62u));
    p = t * p;
    float a = __builtin_fmaf(q, p, q);
    const float t1 = __uint_as_float(0x3fc90fdbu) - a;
    a = ay > ax ? t1 : a;
    const float t2 = __uint_as_float(0x40490fdbu) - a;
    a = x < 0.0f ? t2 : a;
    const float t3 = ((int)__float_as_uint(x) < 0) ? __uint_as_float(0x40490fdbu) : 0.0f;
    a = (y == 0.0f) ? t3 : a;
    const float t4 = (x < 0.0f) ? __uint_as_float(0x4016cbe4u) : __uint_as_float(0x3f490fdbu);
    a = (__builtin_isinf(x) && __builtin_isinf(y)) ? t4 : a;
    a = (x != x || y != y) ? __uint_as_float(0x7fc00000u) : a;
    return copysignf(a, y);
}

__device__ __forceinline__ float acos_lib(float x) {
    const float ax = fabsf(x);
    const float h = __builtin_fmaf(ax, -0.5f, 0.5f), s = x * x;
    const bool big = ax > 0.5f;
    const float w = big ? h : s;
    float p = __builtin_fmaf(w, __uint_as_float(0x3d1c21a7u), __uint_as_float(0x3c5fc5dau));
    p = __builtin_fmaf(w, p, __uint_as_float(0x3d034c3cu));
    p = __builtin_fmaf(w, p, __uint_as_float(0x3d3641b1u));
    p = __builtin_fmaf(w, p, __uint_as_float(0x3d999bc8u));
    p = __builtin_fmaf(w, p, __uint_as_float(0x3e2aaaacu));
    const float z = w * p;
    const float sq = __builtin_amdgcn_sqrtf(w);
    const float g = __builtin_fmaf(sq, z, sq);
    const float g2 = g + g;
    const float neg = __uint_as_float(0x40490fdbu) - g2;
    const float sm = __uint_as_float(0x3fc90fdbu) - __builtin_fmaf(x, z, x);
    return big ? (x < 0.0f ? neg : g2) : sm;
}

__device__ __forceinline__ float dihedral4_ref(f3 a, f3 b, f3 c, f3 d) {
    const f3 b0 = sub3(a, b), b1 = sub3(c, b), b2 = sub3(d, c);
    const f3 n1 = cross3(b0, b1);          // np.cross(b0, b1)
    const f3 n2 = cross3(b2, b1);          // np.cross(b2, b1)
    const f3 m = cross3(n1, n2);
    const float x = dot3(n1, n2);
    const float y = dot3(m, b1) / norm3(b1);   // an IEEE division: correctly rounded, hence the same bits however it is lowered
    return atan2_lib(y, x);
}

__device__ __forceinline__ float angle3_ref(f3 a, f3 b, f3 c) {
    const f3 ba = sub3(a, b), bc = sub3(c, b);
    const float cosine = dot3(ba, bc) / (norm3(ba) * norm3(bc));
    return acos_lib(cosine);               // no clamp, as geometry.py:64-71
}

// atan2 of the PAIRWISE kernels (K3 and the fused featuriser; K2 and the pointwise entry keep atan2_ps with every IEEE
// special case).  Same polynomial, same quadrant logic, same signed-zero behaviour (atan2(+0, +0) = +0, atan2(+0, -0) =
// pi); what is dropped are six per-element compare / select instructions that only matter for infinite arguments:
//   * max(|x|, |y|) is clamped below at FLT_MIN inside the same v_max3_f32, which makes 0 / 0 come out as 0 without the
//     separate (mx == 0) select;
//   * NaN: v_min / v_max drop NaNs, so a NaN x is re-injected with one fused multiply-add by zero (instead of two
//     compares, an or and a select).  y needs none: in dihedral4_k3 y = n1 . (c - d) is NaN only if a coordinate is, and
//     then x = (n1 . n2) * rsq is NaN as well; x alone is NaN when b1 = 0 (0 * inf), the reference's 0 / 0;
//   * atan2(+-inf, +-inf) and atan2(finite, +-inf) come out NaN instead of multiples of pi / 4.  x and y are dot
//     products of cross products of coordinate differences: they overflow only for coordinates beyond 4e9 A.
// Two more consequences, pinned with the rest by tests/test_gpu_arith.py: a NaN y next to a number x is NOT propagated (the
// result is an angle with y's sign bit); and the clamp makes the quotient of two subnormal arguments min / FLT_MIN
// instead of min / max, so atan2_k3(s, s) for a subnormal s is atan(s / FLT_MIN), not pi / 4 (errors up to pi / 4 below
// FLT_MIN; the result is always a finite angle, where atan2_ps gives NaN or an infinity).  Accuracy elsewhere is atan2_ps's: 1.41e-7 in
// the first octant, 2.87e-7 over the plane.
__device__ __forceinline__ float atan2_k3(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(fmaxf(ax, ay), 1.17549435e-38f), mn = fminf(ax, ay);
    const float a = mn * __builtin_amdgcn_rcpf(mx);
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
    r = __builtin_fmaf(x, 0.0f, r);   // r >= +0 here: adding +-0 leaves it, a NaN (or infinite) x poisons it
    return copysignf(r, y);
}

// dihedral4 with atan2_k3 and the three-instruction dot products (dot3_fast)
__device__ __forceinline__ float dihedral4_k3(f3 a, f3 b, f3 c, f3 d) {
    f3 b0 = sub3(a, b);
    f3 b1 = sub3(c, b);
    f3 b2n = sub3(c, d);
    f3 n1 = cross3(b0, b1);
    f3 n2 = cross3(b1, b2n);
    const float nn = dot3_fast(b1, b1);
    float x = dot3_fast(n1, n2) * __builtin_amdgcn_rsqf(nn);
    float y = dot3_fast(n1, b2n);
    return atan2_k3(y, x);
}

// ---- two problems per lane: the same arithmetic on float2, which gfx950 issues as packed v_pk_* instructions ----
// (K3 is VALU-issue bound; element for element the operations and their order are those of the scalar code above,
// so the results are bit-identical.)  f32x2 itself is ps_common.hpp's.
struct f3v {
    f32x2 x, y, z;
};

__device__ __forceinline__ f3v mk3v(f3 a, f3 b) { return f3v{f32x2{a.x, b.x}, f32x2{a.y, b.y}, f32x2{a.z, b.z}}; }
__device__ __forceinline__ f3v sub3v(f3v a, f3v b) { return f3v{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f32x2 dot3v(f3v a, f3v b) {
    const f32x2 px = a.x * b.x, py = a.y * b.y, pz = a.z * b.z;
    return ((f32x2{0.0f, 0.0f} + px) + py) + pz;
}
__device__ __forceinline__ f3v cross3v(f3v u, f3v v) {
    f3v r;
    r.x = u.y * v.z - u.z * v.y;
    r.y = u.z * v.x - u.x * v.z;
    r.z = u.x * v.y - u.y * v.x;
    return r;
}
// dot3_fast on both halves
__device__ __forceinline__ f32x2 dot3v_fast(f3v a, f3v b) {
    return __builtin_elementwise_fma(a.z, b.z, __builtin_elementwise_fma(a.y, b.y, __builtin_elementwise_fma(a.x, b.x, f32x2{0.0f, 0.0f})));
}
// atan2_ps on both halves: the polynomial, the squares and the quadrant subtractions as packed mul / fma / add
// (v_pk_*_f32 issue at the scalar rate, so every packed instruction retires two elements' worth); abs / min / max /
// rcp / selects have no packed fp32 form and stay per element.  Same operations in the same order per element as
// atan2_ps, hence the same bits (K3's odd last row and the fused featuriser use the scalar routine).
__device__ __forceinline__ f32x2 atan2_ps_v(f32x2 y, f32x2 x) {
    const f32x2 ax = {fabsf(x.x), fabsf(x.y)}, ay = {fabsf(y.x), fabsf(y.y)};
    const f32x2 mx = {fmaxf(ax.x, ay.x), fmaxf(ax.y, ay.y)}, mn = {fminf(ax.x, ay.x), fminf(ax.y, ay.y)};
    f32x2 a = mn * f32x2{__builtin_amdgcn_rcpf(mx.x), __builtin_amdgcn_rcpf(mx.y)};
    a.x = (mx.x == 0.0f) ? 0.0f : a.x;
    a.y = (mx.y == 0.0f) ? 0.0f : a.y;
    a.x = (mn.x == __builtin_huge_valf()) ? 1.0f : a.x;
    a.y = (mn.y == __builtin_huge_valf()) ? 1.0f : a.y;
    const f32x2 s = a * a;
    auto k2 = [](float c) { return f32x2{c, c}; };
    f32x2 p = k2(0.0028340641874819994f);
    p = __builtin_elementwise_fma(p, s, k2(-0.016005029901862144f));
    p = __builtin_elementwise_fma(p, s, k2(0.042587608098983765f));
    p = __builtin_elementwise_fma(p, s, k2(-0.07495445758104324f));
    p = __builtin_elementwise_fma(p, s, k2(0.10636754333972931f));
    p = __builtin_elementwise_fma(p, s, k2(-0.14202570915222168f));
    p = __builtin_elementwise_fma(p, s, k2(0.19992484152317047f));
    p = __builtin_elementwise_fma(p, s, k2(-0.3333306610584259f));
    p = __builtin_elementwise_fma(p, s, k2(1.0f));
    f32x2 r = a * p;
    const f32x2 rq = k2(1.5707963267948966f) - r;
    r.x = (ay.x > ax.x) ? rq.x : r.x;
    r.y = (ay.y > ax.y) ? rq.y : r.y;
    const f32x2 rh = k2(3.141592653589793f) - r;
    r.x = (__float_as_uint(x.x) >> 31) ? rh.x : r.x;
    r.y = (__float_as_uint(x.y) >> 31) ? rh.y : r.y;
    r.x = (x.x != x.x || y.x != y.x) ? __builtin_nanf("") : r.x;
    r.y = (x.y != x.y || y.y != y.y) ? __builtin_nanf("") : r.y;
    return f32x2{copysignf(r.x, y.x), copysignf(r.y, y.y)};
}

__device__ __forceinline__ f32x2 dihedral4v(f3v a, f3v b, f3v c, f3v d) {
    const f3v b0 = sub3v(a, b), b1 = sub3v(c, b), b2n = sub3v(c, d);
    const f3v n1 = cross3v(b0, b1), n2 = cross3v(b1, b2n);
    const f32x2 nn = dot3v(b1, b1);
    const f32x2 x = dot3v(n1, n2) * f32x2{__builtin_amdgcn_rsqf(nn.x), __builtin_amdgcn_rsqf(nn.y)};
    const f32x2 y = dot3v(n1, b2n);
    return atan2_ps_v(y, x);
}

// atan2_k3 / dihedral4_k3 on both halves (same operations in the same order per element, hence the same bits)
__device__ __forceinline__ f32x2 atan2_k3_v(f32x2 y, f32x2 x) {
    const f32x2 ax = {fabsf(x.x), fabsf(x.y)}, ay = {fabsf(y.x), fabsf(y.y)};
    const f32x2 mx = {fmaxf(fmaxf(ax.x, ay.x), 1.17549435e-38f), fmaxf(fmaxf(ax.y, ay.y), 1.17549435e-38f)};
    const f32x2 mn = {fminf(ax.x, ay.x), fminf(ax.y, ay.y)};
    const f32x2 a = mn * f32x2{__builtin_amdgcn_rcpf(mx.x), __builtin_amdgcn_rcpf(mx.y)};
    const f32x2 s = a * a;
    auto k2 = [](float c) { return f32x2{c, c}; };
    f32x2 p = k2(0.0028340641874819994f);
    p = __builtin_elementwise_fma(p, s, k2(-0.016005029901862144f));
    p = __builtin_elementwise_fma(p, s, k2(0.042587608098983765f));
    p = __builtin_elementwise_fma(p, s, k2(-0.07495445758104324f));
    p = __builtin_elementwise_fma(p, s, k2(0.10636754333972931f));
    p = __builtin_elementwise_fma(p, s, k2(-0.14202570915222168f));
    p = __builtin_elementwise_fma(p, s, k2(0.19992484152317047f));
    p = __builtin_elementwise_fma(p, s, k2(-0.3333306610584259f));
    p = __builtin_elementwise_fma(p, s, k2(1.0f));
    f32x2 r = a * p;
    const f32x2 rq = k2(1.5707963267948966f) - r;
    r.x = (ay.x > ax.x) ? rq.x : r.x;
    r.y = (ay.y > ax.y) ? rq.y : r.y;
    const f32x2 rh = k2(3.141592653589793f) - r;
    r.x = (__float_as_uint(x.x) >> 31) ? rh.x : r.x;
    r.y = (__float_as_uint(x.y) >> 31) ? rh.y : r.y;
    r = __builtin_elementwise_fma(x, k2(0.0f), r);
    return f32x2{copysignf(r.x, y.x), copysignf(r.y, y.y)};
}

__device__ __forceinline__ f32x2 dihedral4v_k3(f3v a, f3v b, f3v c, f3v d) {
    const f3v b0 = sub3v(a, b), b1 = sub3v(c, b), b2n = sub3v(c, d);
    const f3v n1 = cross3v(b0, b1), n2 = cross3v(b1, b2n);
    const f32x2 nn = dot3v_fast(b1, b1);
    const f32x2 x = dot3v_fast(n1, n2) * f32x2{__builtin_amdgcn_rsqf(nn.x), __builtin_amdgcn_rsqf(nn.y)};
    const f32x2 y = dot3v_fast(n1, b2n);
    return atan2_k3_v(y, x);
}

// ---- NC column residues per lane: the same arithmetic STEP BY STEP across the columns ----
// (round 4)  K3's time is the VALU's (tools/microbench/k3_valu_floor.hip), and a dependent v_pk_fma_f32 costs ~11 cycles
// where an independent one costs 4: left to itself the compiler evaluates one column's Horner chain after the other with
// an s_nop between the links.  Written across the columns, with a scheduling barrier after every link, the NC chains
// interleave and the loop needs no s_nop at all: 0.60 -> 0.53 us per (4 columns x 2 rows) trip on one SIMD.  Per element
// the operations and their order are those of atan2_k3 / acos_ps, hence the same bits.
template <int NC>
__device__ __forceinline__ void atan2_k3_vn(const f32x2 (&y)[NC], const f32x2 (&x)[NC], f32x2 (&r)[NC]) {
    auto k2 = [](float c) { return f32x2{c, c}; };
    f32x2 ax[NC], ay[NC], a[NC], s[NC], p[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        ax[c] = f32x2{fabsf(x[c].x), fabsf(x[c].y)};
        ay[c] = f32x2{fabsf(y[c].x), fabsf(y[c].y)};
        const f32x2 mx = {fmaxf(fmaxf(ax[c].x, ay[c].x), 1.17549435e-38f), fmaxf(fmaxf(ax[c].y, ay[c].y), 1.17549435e-38f)};
        const f32x2 mn = {fminf(ax[c].x, ay[c].x), fminf(ax[c].y, ay[c].y)};
        a[c] = mn * f32x2{__builtin_amdgcn_rcpf(mx.x), __builtin_amdgcn_rcpf(mx.y)};
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] = a[c] * a[c];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(k2(0.0028340641874819994f), s[c], k2(-0.016005029901862144f));
    constexpr float co[7] = {0.042587608098983765f, -0.07495445758104324f, 0.10636754333972931f, -0.14202570915222168f,
                             0.19992484152317047f, -0.3333306610584259f, 1.0f};
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(p[c], s[c], k2(co[t]));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) r[c] = a[c] * p[c];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x2 rq = k2(1.5707963267948966f) - r[c];
        r[c].x = (ay[c].x > ax[c].x) ? rq.x : r[c].x;
        r[c].y = (ay[c].y > ax[c].y) ? rq.y : r[c].y;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x2 rh = k2(3.141592653589793f) - r[c];
        r[c].x = (__float_as_uint(x[c].x) >> 31) ? rh.x : r[c].x;
        r[c].y = (__float_as_uint(x[c].y) >> 31) ? rh.y : r[c].y;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        r[c] = __builtin_elementwise_fma(x[c], k2(0.0f), r[c]);
        r[c] = f32x2{copysignf(r[c].x, y[c].x), copysignf(r[c].y, y[c].y)};
    }
}

// dot3v with the leading `0 +` folded into the first product: fma(a, b, +0) rounds a * b once and adds +0, which is
// bit for bit (0 + a * b) -- including the -0 -> +0 case the `0 +` exists for -- in one instruction instead of two.
// (The faithful forms' dot product: products first, then adds, as the reference.)
__device__ __forceinline__ f32x2 dot3v_f(f3v a, f3v b) {
    const f32x2 px = __builtin_elementwise_fma(a.x, b.x, f32x2{0.0f, 0.0f}), py = a.y * b.y, pz = a.z * b.z;
    return (px + py) + pz;
}

// dihedral4v_k3 for NC columns: the cross / dot part per column (independent work), then the NC atan2 chains together
template <int NC>
__device__ __forceinline__ void dihedral4v_k3_n(const f3v (&a)[NC], const f3v (&b)[NC], const f3v (&c)[NC],
                                                const f3v (&d)[NC], f32x2 (&out)[NC]) {
    f32x2 x[NC], y[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const f3v b0 = sub3v(a[q], b[q]), b1 = sub3v(c[q], b[q]), b2n = sub3v(c[q], d[q]);
        const f3v n1 = cross3v(b0, b1), n2 = cross3v(b1, b2n);
        const f32x2 nn = dot3v_fast(b1, b1);
        x[q] = dot3v_fast(n1, n2) * f32x2{__builtin_amdgcn_rsqf(nn.x), __builtin_amdgcn_rsqf(nn.y)};
        y[q] = dot3v_fast(n1, b2n);
    }
    atan2_k3_vn<NC>(y, x, out);
}

// acos_ps / angle3v for NC columns (same operations in the same order per element)
template <int NC>
__device__ __forceinline__ void acos_ps_vn(const f32x2 (&x)[NC], f32x2 (&r)[NC]) {
    auto k2 = [](float c) { return f32x2{c, c}; };
    f32x2 ax[NC], p[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) ax[c] = f32x2{fabsf(x[c].x), fabsf(x[c].y)};
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(k2(-0.0012624911f), ax[c], k2(0.0066700901f));
    constexpr float co[6] = {-0.0170881256f, 0.0308918810f, -0.0501743046f, 0.0889789874f, -0.2145988016f, 1.5707963050f};
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(p[c], ax[c], k2(co[t]));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x2 t = k2(1.0f) - ax[c];
        const f32x2 v = p[c] * f32x2{__builtin_amdgcn_sqrtf(t.x), __builtin_amdgcn_sqrtf(t.y)};
        const f32x2 rh = k2(3.141592653589793f) - v;
        r[c] = f32x2{(__float_as_uint(x[c].x) >> 31) ? rh.x : v.x, (__float_as_uint(x[c].y) >> 31) ? rh.y : v.y};
    }
}

// acos_ps on both halves (same operations in the same order per element)
__device__ __forceinline__ f32x2 acos_ps_v(f32x2 x) {
    const f32x2 ax = {fabsf(x.x), fabsf(x.y)};
    auto k2 = [](float c) { return f32x2{c, c}; };
    f32x2 p = k2(-0.0012624911f);
    p = __builtin_elementwise_fma(p, ax, k2(0.0066700901f));
    p = __builtin_elementwise_fma(p, ax, k2(-0.0170881256f));
    p = __builtin_elementwise_fma(p, ax, k2(0.0308918810f));
    p = __builtin_elementwise_fma(p, ax, k2(-0.0501743046f));
    p = __builtin_elementwise_fma(p, ax, k2(0.0889789874f));
    p = __builtin_elementwise_fma(p, ax, k2(-0.2145988016f));
    p = __builtin_elementwise_fma(p, ax, k2(1.5707963050f));
    const f32x2 t = k2(1.0f) - ax;
    const f32x2 r = p * f32x2{__builtin_amdgcn_sqrtf(t.x), __builtin_amdgcn_sqrtf(t.y)};
    const f32x2 rh = k2(3.141592653589793f) - r;
    return f32x2{(__float_as_uint(x.x) >> 31) ? rh.x : r.x, (__float_as_uint(x.y) >> 31) ? rh.y : r.y};
}

// sqrt_rn_mk on both halves: v_rsq_f32 and the class test per element, the Newton / residual steps as packed fma
// (element for element the operations of the scalar routine, hence the same bits)
__device__ __forceinline__ f32x2 sqrt_rn_mk_v(f32x2 x) {
    const f32x2 y = {__builtin_amdgcn_rsqf(x.x), __builtin_amdgcn_rsqf(x.y)};
    f32x2 g = x * y;
    f32x2 h = f32x2{0.5f, 0.5f} * y;
    const f32x2 r = __builtin_elementwise_fma(-h, g, f32x2{0.5f, 0.5f});
    g = __builtin_elementwise_fma(g, r, g);
    h = __builtin_elementwise_fma(h, r, h);
    const f32x2 d = __builtin_elementwise_fma(-g, g, x);
    g = __builtin_elementwise_fma(d, h, g);
    return f32x2{__builtin_amdgcn_classf(x.x, 0x2F0) ? x.x : g.x, __builtin_amdgcn_classf(x.y, 0x2F0) ? x.y : g.y};
}

// dist3 / angle3 for two problems per lane (same operations in the same order as the scalar functions of ps_common.hpp)
__device__ __forceinline__ f32x2 norm_sq3v(f32x2 x, f32x2 y, f32x2 z) {
    return __builtin_elementwise_fma(z, z, __builtin_elementwise_fma(y, y, x * x));
}
__device__ __forceinline__ f32x2 dist3v(f3v a, f3v b) {
    return sqrt_rn_mk_v(norm_sq3v(a.x - b.x, a.y - b.y, a.z - b.z));
}

template <bool EXACT>
__device__ __forceinline__ f32x2 dist3v_t(f3v a, f3v b) {
    const f32x2 x = norm_sq3v(a.x - b.x, a.y - b.y, a.z - b.z);
    if (EXACT) return sqrt_rn_mk_v(x);
    return f32x2{__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)};
}

// angle3 (ps_common.hpp, where the two-v_rsq_f32 cosine is explained) on both halves
__device__ __forceinline__ f32x2 angle3v(f3v a, f3v b, f3v c) {
    const f3v ba = sub3v(a, b), bc = sub3v(c, b);
    const f32x2 num = dot3v_fast(ba, bc);
    const f32x2 na = dot3v_fast(ba, ba), nb = dot3v_fast(bc, bc);
    return acos_ps_v((num * f32x2{__builtin_amdgcn_rsqf(na.x), __builtin_amdgcn_rsqf(na.y)}) * f32x2{__builtin_amdgcn_rsqf(nb.x), __builtin_amdgcn_rsqf(nb.y)});
}

template <int NC>
__device__ __forceinline__ void angle3v_n(const f3v (&a)[NC], const f3v (&b)[NC], const f3v (&c)[NC], f32x2 (&out)[NC]) {
    f32x2 cs[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const f3v ba = sub3v(a[q], b[q]), bc = sub3v(c[q], b[q]);
        const f32x2 num = dot3v_fast(ba, bc);
        const f32x2 na = dot3v_fast(ba, ba), nb = dot3v_fast(bc, bc);
        cs[q] = (num * f32x2{__builtin_amdgcn_rsqf(na.x), __builtin_amdgcn_rsqf(na.y)}) * f32x2{__builtin_amdgcn_rsqf(nb.x), __builtin_amdgcn_rsqf(nb.y)};
    }
    acos_ps_vn<NC>(cs, out);
}

// ---- the FAITHFUL forms for NC columns x two rows (round 5): dihedral4_ref / angle3_ref bit for bit, packed ----
// The same operations as dihedral4_ref / angle3_ref (atan2_lib, acos_lib, the IEEE division), with the multiplies, adds and
// fused multiply-adds of two rows issued as one v_pk_*_f32 and the NC columns' dependent chains interleaved.  An IEEE fma /
// mul / add gives the same bits whether it issues as v_fma_f32 or as half of v_pk_fma_f32, so the results equal the scalar
// forms' bit for bit; that equality is not assumed but tested: tests/test_gpu_parity.py holds the sweep kernels (these
// forms) to the one-column kernel (the scalar forms) on every split, length and special value, and
// tools/microbench/libm_identity.hip sweeps 2^32 argument pairs through both and through the library calls.
//
// a / b, IEEE-correct: the expansion of fdiv (v_div_scale_f32 x2, v_rcp_f32, the Newton / residual chain, v_div_fmas_f32,
// v_div_fixup_f32); the chain's six operations packed.
template <int NC>
__device__ __forceinline__ void div_ieee_vn(const f32x2 (&a)[NC], const f32x2 (&b)[NC], f32x2 (&o)[NC]) {
    f32x2 ds[NC], ns[NC], r[NC], q[NC], t[NC];
    bool fx[NC], fy[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        bool unused;
        ds[c] = f32x2{__builtin_amdgcn_div_scalef(a[c].x, b[c].x, false, &unused), __builtin_amdgcn_div_scalef(a[c].y, b[c].y, false, &unused)};
        ns[c] = f32x2{__builtin_amdgcn_div_scalef(a[c].x, b[c].x, true, &fx[c]), __builtin_amdgcn_div_scalef(a[c].y, b[c].y, true, &fy[c])};
        r[c] = f32x2{__builtin_amdgcn_rcpf(ds[c].x), __builtin_amdgcn_rcpf(ds[c].y)};
    }
    const f32x2 one = {1.0f, 1.0f};
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = __builtin_elementwise_fma(-ds[c], r[c], one);
#pragma unroll
    for (int c = 0; c < NC; ++c) r[c] = __builtin_elementwise_fma(t[c], r[c], r[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] = ns[c] * r[c];
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = __builtin_elementwise_fma(-ds[c], q[c], ns[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] = __builtin_elementwise_fma(t[c], r[c], q[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = __builtin_elementwise_fma(-ds[c], q[c], ns[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c)
        o[c] = f32x2{__builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(t[c].x, r[c].x, q[c].x, fx[c]), b[c].x, a[c].x),
                     __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(t[c].y, r[c].y, q[c].y, fy[c]), b[c].y, a[c].y)};
}

// atan2_lib on NC columns x two rows
template <int NC>
__device__ __forceinline__ void atan2_lib_vn(const f32x2 (&y)[NC], const f32x2 (&x)[NC], f32x2 (&o)[NC]) {
    auto k2 = [](float c) { return f32x2{c, c}; };
    f32x2 q[NC], t[NC], p[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float qq[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float ax = fabsf(h ? x[c].y : x[c].x), ay = fabsf(h ? y[c].y : y[c].x);
            const float v = __builtin_fminf(ax, ay), u = __builtin_fmaxf(ax, ay);
            const float m = __builtin_amdgcn_frexp_mantf(v) * __builtin_amdgcn_rcpf(__builtin_amdgcn_frexp_mantf(u));
            qq[h] = __builtin_amdgcn_ldexpf(m, __builtin_amdgcn_frexp_expf(v) - __builtin_amdgcn_frexp_expf(u));
        }
        q[c] = f32x2{qq[0], qq[1]};
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = q[c] * q[c];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(t[c], k2(__uint_as_float(0x3b2d2a58u)), k2(__uint_as_float(0xbc7a590cu)));
    constexpr uint32_t co[6] = {0x3d29fb3fu, 0xbd97d4d7u, 0x3dd931b2u, 0xbe1160e6u, 0x3e4cb8bfu, 0xbeaaaa62u};
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(t[c], p[c], k2(__uint_as_float(co[s])));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = t[c] * p[c];
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] = __builtin_elementwise_fma(q[c], p[c], q[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x2 t1 = k2(__uint_as_float(0x3fc90fdbu)) - q[c];
        f32x2 a = {fabsf(y[c].x) > fabsf(x[c].x) ? t1.x : q[c].x, fabsf(y[c].y) > fabsf(x[c].y) ? t1.y : q[c].y};
        const f32x2 t2 = k2(__uint_as_float(0x40490fdbu)) - a;
        float r[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float xe = h ? x[c].y : x[c].x, ye = h ? y[c].y : y[c].x;
            float e = (xe < 0.0f) ? (h ? t2.y : t2.x) : (h ? a.y : a.x);
            const float t3 = ((int)__float_as_uint(xe) < 0) ? __uint_as_float(0x40490fdbu) : 0.0f;
            e = (ye == 0.0f) ? t3 : e;
            const float t4 = (xe < 0.0f) ? __uint_as_float(0x4016cbe4u) : __uint_as_float(0x3f490fdbu);
            e = (__builtin_isinf(xe) && __builtin_isinf(ye)) ? t4 : e;
            e = (xe != xe || ye != ye) ? __uint_as_float(0x7fc00000u) : e;
            r[h] = copysignf(e, ye);
        }
        o[c] = f32x2{r[0], r[1]};
    }
}

// acos_lib on NC columns x two rows (the library's fma(c1, c2, -z) with c1 * c2 = pi, pi / 2 is, as hipcc folds it, a
// subtraction from the rounded constant)
template <int NC>
__device__ __forceinline__ void acos_lib_vn(const f32x2 (&x)[NC], f32x2 (&o)[NC]) {
    auto k2 = [](float c) { return f32x2{c, c}; };
    f32x2 w[NC], p[NC];
    bool big[NC][2];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x2 ax = {fabsf(x[c].x), fabsf(x[c].y)};
        const f32x2 h = __builtin_elementwise_fma(ax, k2(-0.5f), k2(0.5f)), s = x[c] * x[c];
        big[c][0] = ax.x > 0.5f; big[c][1] = ax.y > 0.5f;
        w[c] = f32x2{big[c][0] ? h.x : s.x, big[c][1] ? h.y : s.y};
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(w[c], k2(__uint_as_float(0x3d1c21a7u)), k2(__uint_as_float(0x3c5fc5dau)));
    constexpr uint32_t co[4] = {0x3d034c3cu, 0x3d3641b1u, 0x3d999bc8u, 0x3e2aaaacu};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NC; ++c) p[c] = __builtin_elementwise_fma(w[c], p[c], k2(__uint_as_float(co[s])));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const f32x2 z = w[c] * p[c];
        const f32x2 sq = {__builtin_amdgcn_sqrtf(w[c].x), __builtin_amdgcn_sqrtf(w[c].y)};
        const f32x2 g = __builtin_elementwise_fma(sq, z, sq);
        const f32x2 g2 = g + g;
        const f32x2 neg = k2(__uint_as_float(0x40490fdbu)) - g2;
        const f32x2 sm = k2(__uint_as_float(0x3fc90fdbu)) - __builtin_elementwise_fma(x[c], z, x[c]);
        o[c] = f32x2{big[c][0] ? (x[c].x < 0.0f ? neg.x : g2.x) : sm.x, big[c][1] ? (x[c].y < 0.0f ? neg.y : g2.y) : sm.y};
    }
}

// dihedral4_ref for NC columns x two rows (the same operations per element in the same order)
template <int NC>
__device__ __forceinline__ void dihedral4v_ref_n(const f3v (&a)[NC], const f3v (&b)[NC], const f3v (&c)[NC],
                                                 const f3v (&d)[NC], f32x2 (&out)[NC]) {
    f32x2 x[NC], y0[NC], nb[NC], y[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const f3v b0 = sub3v(a[q], b[q]), b1 = sub3v(c[q], b[q]), b2 = sub3v(d[q], c[q]);
        const f3v n1 = cross3v(b0, b1), n2 = cross3v(b2, b1);
        const f3v m = cross3v(n1, n2);
        x[q] = dot3v_f(n1, n2);
        y0[q] = dot3v_f(m, b1);
        nb[q] = sqrt_rn_mk_v(norm_sq3v(b1.x, b1.y, b1.z));
    }
    div_ieee_vn<NC>(y0, nb, y);
    atan2_lib_vn<NC>(y, x, out);
}

// angle3_ref for NC columns x two rows
template <int NC>
__device__ __forceinline__ void angle3v_ref_n(const f3v (&a)[NC], const f3v (&b)[NC], const f3v (&c)[NC], f32x2 (&out)[NC]) {
    f32x2 num[NC], den[NC], cs[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const f3v ba = sub3v(a[q], b[q]), bc = sub3v(c[q], b[q]);
        num[q] = dot3v_f(ba, bc);
        den[q] = sqrt_rn_mk_v(norm_sq3v(ba.x, ba.y, ba.z)) * sqrt_rn_mk_v(norm_sq3v(bc.x, bc.y, bc.z));
    }
    div_ieee_vn<NC>(num, den, cs);
    acos_lib_vn<NC>(cs, out);
}
