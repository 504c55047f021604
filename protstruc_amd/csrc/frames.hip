// K4 -- per-residue backbone frames: Gram-Schmidt orientation + translation.
// Replaces StructureBatch.backbone_orientations / backbone_translations
// (reference protstruc.py:543-587) and geometry.gram_schmidt
// (geometry.py:413-439).  One lane per residue: 36 (+12) bytes read,
// 36 + 12 bytes written; the basis vectors are the COLUMNS of the 3x3.
#include "ps_common.hpp"

namespace {

__global__ __launch_bounds__(256) void k4_frames(const float* __restrict__ xyz, float* __restrict__ rot,
                                                 float* __restrict__ trans, size_t n_res, int A, int a1, int a2,
                                                 int a3, int t_atom) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_res) return;
    const float* p = xyz + r * (size_t)A * 3;
    if (rot) {
        f3 e1, e2, e3;
        gram_schmidt3(load3(p + a1 * 3), load3(p + a2 * 3), load3(p + a3 * 3), e1, e2, e3);
        float* o = rot + r * 9;
        o[0] = e1.x; o[1] = e2.x; o[2] = e3.x;
        o[3] = e1.y; o[4] = e2.y; o[5] = e3.y;
        o[6] = e1.z; o[7] = e2.z; o[8] = e3.z;
    }
    if (trans) {
        f3 t = load3(p + t_atom * 3);
        float* o = trans + r * 3;
        o[0] = t.x; o[1] = t.y; o[2] = t.z;
    }
}

// Vector-Jacobian product of k4_frames, one lane per residue: the chain rule through gram_schmidt3 backwards (e3 = e1 x e2,
// e2 = u2 / |u2|, u2 = v2 - (e1 . v2) e1, e1 = v1 / |v1|) with the intermediates recomputed by the forward's own arithmetic.
// The lane writes its residue's whole (A,3) row: zeros, then the contributions of a1, a2, a3 and t_atom added in that
// order where slots coincide.  A masked residue gets zeros by selection.
__device__ __forceinline__ f3 add3(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ float dotf(f3 a, f3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }

__global__ __launch_bounds__(256) void k4_frames_backward(const float* __restrict__ xyz, const float* __restrict__ grad_rot,
                                                          const float* __restrict__ grad_trans,
                                                          const uint8_t* __restrict__ residue_mask,
                                                          float* __restrict__ grad_xyz, size_t n_res, int A, int a1, int a2,
                                                          int a3, int t_atom) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_res) return;
    const bool live = !residue_mask || residue_mask[r] != 0;
    const float* p = xyz + r * (size_t)A * 3;
    const f3 zero = f3{0.0f, 0.0f, 0.0f};
    f3 ga = zero, gb = zero, gc = zero, gt = zero;
    if (grad_rot) {
        const float* g = grad_rot + r * 9;
        f3 ge1 = f3{g[0], g[3], g[6]}, ge2 = f3{g[1], g[4], g[7]};
        const f3 ge3 = f3{g[2], g[5], g[8]};
        const f3 b = load3(p + a2 * 3);
        const f3 v1 = sub3(load3(p + a3 * 3), b), v2 = sub3(load3(p + a1 * 3), b);
        const float n1 = norm3(v1);
        const f3 e1 = div3(v1, n1);
        const float pr = dot3(e1, v2);
        const f3 u2 = sub3(v2, scale3(e1, pr));
        const float n2 = norm3(u2);
        const f3 e2 = div3(u2, n2);
        ge1 = add3(ge1, cross3_fused(e2, ge3));
        ge2 = add3(ge2, cross3_fused(ge3, e1));
        const f3 gu2 = div3(sub3(ge2, scale3(e2, dotf(ge2, e2))), n2);
        const float gp = -dotf(gu2, e1);
        ge1 = add3(ge1, sub3(scale3(v2, gp), scale3(gu2, pr)));
        const f3 gv2 = add3(gu2, scale3(e1, gp));
        const f3 gv1 = div3(sub3(ge1, scale3(e1, dotf(ge1, e1))), n1);
        ga = gv2;
        gc = gv1;
        gb = f3{-gv1.x - gv2.x, -gv1.y - gv2.y, -gv1.z - gv2.z};
    }
    if (grad_trans) gt = load3(grad_trans + r * 3);
    float* o = grad_xyz + r * (size_t)A * 3;
    for (int s = 0; s < A; ++s) {
        f3 v = zero;
        if (grad_rot) {
            if (s == a1) v = add3(v, ga);
            if (s == a2) v = add3(v, gb);
            if (s == a3) v = add3(v, gc);
        }
        if (grad_trans && s == t_atom) v = add3(v, gt);
        o[s * 3 + 0] = live ? v.x : 0.0f;
        o[s * 3 + 1] = live ? v.y : 0.0f;
        o[s * 3 + 2] = live ? v.z : 0.0f;
    }
}

// Point-wise forms of the geometry primitives for the free functions of protstruc.geometry
// (reference geometry.py:39-124, :413-439): a, b, c(, d) are (n,3) arrays.
//   mode 0: out[n]   = angle(a, b, c)        mode 1: out[n] = dihedral(a, b, c, d)
//   mode 2: out[n*9] = gram_schmidt(a, b, c) (3x3 row-major, basis vectors as columns)
//   mode 3: out[n*3] = place_fourth_atom(a, b, c, d[n][0], d[n][1], d[n][2])  (d packed [length, planar, dihedral])
__global__ __launch_bounds__(256) void k_pointwise(const float* __restrict__ a, const float* __restrict__ b,
                                                   const float* __restrict__ c, const float* __restrict__ d,
                                                   float* __restrict__ out, size_t n, int mode) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const f3 pa = load3(a + i * 3), pb = load3(b + i * 3), pc = load3(c + i * 3);
    if (mode == 0) {
        out[i] = angle3(pa, pb, pc);
    } else if (mode == 1) {
        out[i] = dihedral4(pa, pb, pc, load3(d + i * 3));
    } else if (mode == 2) {
        f3 e1, e2, e3;
        gram_schmidt3(pa, pb, pc, e1, e2, e3);
        float* o = out + i * 9;
        o[0] = e1.x; o[1] = e2.x; o[2] = e3.x;
        o[3] = e1.y; o[4] = e2.y; o[5] = e3.y;
        o[6] = e1.z; o[7] = e2.z; o[8] = e3.z;
    } else {
        const f3 x = place4(pa, pb, pc, d[i * 3], d[i * 3 + 1], d[i * 3 + 2]);
        float* o = out + i * 3;
        o[0] = x.x; o[1] = x.y; o[2] = x.z;
    }
}

}  // namespace

extern "C" int ps_pointwise_f32(int mode, const float* a, const float* b, const float* c, const float* d, float* out,
                                long long n, void* stream) {
    if (mode < 0 || mode > 3 || !a || !b || !c || !out || n < 0 || ((mode == 1 || mode == 3) && !d))
        return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    return ps_launch(k_pointwise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), a, b, c, d, out, (size_t)n, mode);
}

extern "C" int ps_frames_f32(const float* xyz, float* rot, float* trans, int B, int N, int A, int a1, int a2, int a3,
                             int t_atom, void* stream) {
    if (!xyz || (!rot && !trans) || B < 0 || N < 0 || A <= 0) return (int)hipErrorInvalidValue;
    if (rot && (a1 < 0 || a1 >= A || a2 < 0 || a2 >= A || a3 < 0 || a3 >= A)) return (int)hipErrorInvalidValue;
    if (trans && (t_atom < 0 || t_atom >= A)) return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    return ps_launch(k4_frames, dim3((unsigned)((n_res + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), xyz, rot, trans, n_res, A, a1, a2, a3, t_atom);
}

extern "C" int ps_frames_backward_f32(const float* xyz, const float* grad_rot, const float* grad_trans,
                                      const uint8_t* residue_mask, float* grad_xyz, int B, int N, int A, int a1, int a2,
                                      int a3, int t_atom, void* stream) {
    if (!xyz || !grad_xyz || (!grad_rot && !grad_trans) || B < 0 || N < 0 || A <= 0) return (int)hipErrorInvalidValue;
    if (grad_rot && (a1 < 0 || a1 >= A || a2 < 0 || a2 >= A || a3 < 0 || a3 >= A)) return (int)hipErrorInvalidValue;
    if (grad_trans && (t_atom < 0 || t_atom >= A)) return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    return ps_launch(k4_frames_backward, dim3((unsigned)((n_res + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), xyz, grad_rot, grad_trans, residue_mask, grad_xyz, n_res, A, a1,
                     a2, a3, t_atom);
}
