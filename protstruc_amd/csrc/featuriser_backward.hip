// The featuriser's backward pass (k3_inter_residue_geometry_backward, ps_inter_residue_geometry_backward_f32; the forward is
// featuriser.hip): grad_xyz = sum over planes and pairs of g_plane[b,i,j] * d plane[b,i,j] / d xyz.
// One workgroup owns IRGB_TILE consecutive residues of one structure and stages the four slots the featuriser reads (N, CA, O,
// CB: 48 bytes) and four presence bits of ALL of the structure's residues in LDS.  The gradient of residue r collects terms from
// row r of every plane (r in the i role: N_i, CA_i, CB_i move) and from column r (r in the j role: CA_j, O_j, CB_j move), so a
// workgroup makes two sweeps over the partner index k and no atomic is needed:
//   row sweep     a wave takes one owned row at a time, its 64 lanes 64 consecutive k: g[b, r, k] is read in 256-byte
//                 segments; the nine sums are reduced across the wave by a butterfly and lane 0 leaves them in LDS;
//   column sweep  lane % 32 is the owned residue, the eight half-waves take k = 0..7 (mod 8): g[b, k, r0 .. r0 + 31] is read
//                 in 128-byte segments; the two halves of a wave are added by one shuffle, the four waves through LDS.
// The sums are added in an order fixed by (N, lane), so two launches agree bit for bit.  An entry that is not ACTIVE -- an
// atom it reads is absent from atom_mask, or i == j in any plane but d_no -- is excluded by selection (v_cndmask), never by a
// multiplication: NaN coordinates of absent atoms and NaN upstream values at such entries do not reach the result.  An absent
// (NULL) upstream plane skips its block in every wave.  One arithmetic (not a function of exact_sqrt / exact_angles):
// differences, unfused cross products, fused dot products, v_rcp_f32 / v_rsq_f32 with one Newton step.  The closed forms, with F = a - b,
// G = b - c, H = d - c, A = F x G, B = H x G for dihedral(a, b, c, d) (Blondel & Karplus 1996; the sign is geometry.dihedral's):
//   d/da = -|G| A / |A|^2      d/dd = |G| B / |B|^2      s = F.G / |G|^2      t = H.G / |G|^2
//   d/db = -(1 + s) d/da - t d/dd                        d/dc = s d/da + (t - 1) d/dd
// and with u = a - b, v = c - b, n = u x v for angle(a, b, c): d/da = (u x n) / (|u|^2 |n|), d/dc = -(v x n) / (|v|^2 |n|), d/db
// minus their sum -- the cross-product form of -(v^ - cos u^) / (|u| sin) without the cancellation in 1 - cos^2.
#include "k3_launch.hpp"

constexpr int IRGB_TILE = 32, IRGB_THREADS = 256, IRGB_MAX_N = 2048;
constexpr unsigned irgb_lds_bytes(int N) { return (unsigned)N * 52u + IRGB_TILE * 9u * 4u * (1u + IRGB_THREADS / 64u); }

// 1 / x and 1 / sqrt(x) from v_rcp_f32 / v_rsq_f32 (1 ulp) with one Newton step each: within rounding of the IEEE quotient a
// float32 autograd of the same formulas divides by, for two and four more instructions
__device__ __forceinline__ float irgb_rcp(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.0f), r, r);
}
__device__ __forceinline__ float irgb_rsq(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    return __builtin_fmaf(0.5f * y, __builtin_fmaf(-(x * y), y, 1.0f), y);
}

struct IrgbResidue {
    f3 n, ca, o, cb;
    unsigned present;   // bit 0 N, 1 CA, 2 O, 3 CB
};

__device__ __forceinline__ IrgbResidue irgb_residue(const float* pts, const unsigned* bits, int k) {
    const k3_f32x4* p = reinterpret_cast<const k3_f32x4*>(pts + (size_t)k * 12);
    const k3_f32x4 a = p[0], b = p[1], c = p[2];
    return IrgbResidue{f3{a.x, a.y, a.z}, f3{a.w, b.x, b.y}, f3{b.z, b.w, c.x}, f3{c.y, c.z, c.w}, bits[k]};
}

// acc += (active ? w * v : 0)
__device__ __forceinline__ void irgb_add(f3& acc, bool active, float w, f3 v) {
    acc.x += active ? w * v.x : 0.0f;
    acc.y += active ? w * v.y : 0.0f;
    acc.z += active ? w * v.z : 0.0f;
}

// (p - q) / |p - q|: the gradient of |p - q| with respect to p
__device__ __forceinline__ f3 irgb_unit_difference(f3 p, f3 q) {
    const f3 d = sub3(p, q);
    return scale3(d, irgb_rsq(dot3_fast(d, d)));
}

__device__ __forceinline__ void irgb_dihedral_grad(f3 a, f3 b, f3 c, f3 d, f3& ga, f3& gb, f3& gc, f3& gd) {
    const f3 F = sub3(a, b), G = sub3(b, c), H = sub3(d, c);
    const f3 A = cross3(F, G), Bv = cross3(H, G);
    const float gg = dot3_fast(G, G), rgg = irgb_rcp(gg), gl = gg * irgb_rsq(gg);
    ga = scale3(A, -gl * irgb_rcp(dot3_fast(A, A)));
    gd = scale3(Bv, gl * irgb_rcp(dot3_fast(Bv, Bv)));
    const float s = dot3_fast(F, G) * rgg, t = dot3_fast(H, G) * rgg;
    const float s1 = -(1.0f + s), t1 = t - 1.0f;
    gb = f3{s1 * ga.x - t * gd.x, s1 * ga.y - t * gd.y, s1 * ga.z - t * gd.z};
    gc = f3{s * ga.x + t1 * gd.x, s * ga.y + t1 * gd.y, s * ga.z + t1 * gd.z};
}

__device__ __forceinline__ void irgb_angle_grad(f3 a, f3 b, f3 c, f3& ga, f3& gb, f3& gc) {
    const f3 u = sub3(a, b), v = sub3(c, b), n = cross3(u, v);
    const float rn = irgb_rsq(dot3_fast(n, n));
    ga = scale3(cross3(u, n), irgb_rcp(dot3_fast(u, u)) * rn);
    gc = scale3(cross3(v, n), -(irgb_rcp(dot3_fast(v, v)) * rn));
    gb = f3{-(ga.x + gc.x), -(ga.y + gc.y), -(ga.z + gc.z)};
}

struct IrgbUpstream {
    const float *d_ca, *d_cb, *d_no, *omega, *theta, *phi;
};

// One pair (i, j) at offset o of the planes.  ROW: the lane owns i and accumulates N_i, CA_i, CB_i in acc[0..2]; else it owns j
// and accumulates O_j, CA_j, CB_j.  What the other role needs is dead code here.
template <bool ROW>
__device__ __forceinline__ void irgb_pair(const IrgbResidue& I, const IrgbResidue& J, bool off_diagonal, const IrgbUpstream& g,
                                          size_t o, f3 (&acc)[3]) {
    const unsigned mi = I.present, mj = J.present;
    if (g.d_ca) {
        const bool act = off_diagonal && (mi & 2u) && (mj & 2u);
        const f3 e = irgb_unit_difference(I.ca, J.ca);
        irgb_add(acc[1], act, ROW ? g.d_ca[o] : -g.d_ca[o], e);
    }
    if (g.d_cb) {
        const bool act = off_diagonal && (mi & 8u) && (mj & 8u);
        const f3 e = irgb_unit_difference(I.cb, J.cb);
        irgb_add(acc[2], act, ROW ? g.d_cb[o] : -g.d_cb[o], e);
    }
    if (g.d_no) {
        const bool act = (mi & 1u) && (mj & 4u);      // the diagonal is an ordinary N_i - O_i distance
        const f3 e = irgb_unit_difference(I.n, J.o);
        irgb_add(acc[0], act, ROW ? g.d_no[o] : -g.d_no[o], e);
    }
    if (g.omega) {                                    // dihedral(CA_i, CB_i, CA_j, CB_j), as the forward codes it
        const bool act = off_diagonal && (mi & 10u) == 10u && (mj & 10u) == 10u;
        f3 ga, gb, gc, gd;
        irgb_dihedral_grad(I.ca, I.cb, J.ca, J.cb, ga, gb, gc, gd);
        const float w = g.omega[o];
        irgb_add(acc[1], act, w, ROW ? ga : gc);
        irgb_add(acc[2], act, w, ROW ? gb : gd);
    }
    if (g.theta) {                                    // dihedral(N_i, CA_i, CB_i, CB_j)
        const bool act = off_diagonal && (mi & 11u) == 11u && (mj & 8u);
        f3 ga, gb, gc, gd;
        irgb_dihedral_grad(I.n, I.ca, I.cb, J.cb, ga, gb, gc, gd);
        const float w = g.theta[o];
        if (ROW) {
            irgb_add(acc[0], act, w, ga);
            irgb_add(acc[1], act, w, gb);
            irgb_add(acc[2], act, w, gc);
        } else {
            irgb_add(acc[2], act, w, gd);
        }
    }
    if (g.phi) {                                      // angle(CA_i, CB_i, CB_j)
        const bool act = off_diagonal && (mi & 10u) == 10u && (mj & 8u);
        f3 ga, gb, gc;
        irgb_angle_grad(I.ca, I.cb, J.cb, ga, gb, gc);
        const float w = g.phi[o];
        if (ROW) {
            irgb_add(acc[1], act, w, ga);
            irgb_add(acc[2], act, w, gb);
        } else {
            irgb_add(acc[2], act, w, gc);
        }
    }
}

__global__ __launch_bounds__(IRGB_THREADS) void k3_inter_residue_geometry_backward(
    const float* __restrict__ xyz, const uint8_t* __restrict__ amask, const float* __restrict__ g_d_ca,
    const float* __restrict__ g_d_cb, const float* __restrict__ g_d_no, const float* __restrict__ g_omega,
    const float* __restrict__ g_theta, const float* __restrict__ g_phi, float* __restrict__ grad_xyz, int N, int A, int n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char irgb_lds[];
    float* pts = reinterpret_cast<float*>(irgb_lds);                 // [N][12]: N, CA, O, CB
    unsigned* bits = reinterpret_cast<unsigned*>(pts + (size_t)N * 12);   // [N]
    float* row_sum = reinterpret_cast<float*>(bits + N);             // [IRGB_TILE][9]: N_i, CA_i, CB_i
    float* col_part = row_sum + IRGB_TILE * 9;                       // [waves][IRGB_TILE][9]: O_j, CA_j, CB_j
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = (int)(blockIdx.x / (unsigned)n_tiles), r0 = (int)(blockIdx.x % (unsigned)n_tiles) * IRGB_TILE;
    const int rows = min(IRGB_TILE, N - r0);
    const IrgbUpstream g{g_d_ca, g_d_cb, g_d_no, g_omega, g_theta, g_phi};
    const bool any = g_d_ca || g_d_cb || g_d_no || g_omega || g_theta || g_phi;

    for (int q = t; q < N * 4; q += IRGB_THREADS) {
        const int k = q >> 2, s = q & 3;
        const int slot = s + (s >> 1);                               // 0, 1, 3, 4
        const float* src = xyz + (((size_t)b * N + k) * A + slot) * 3;
        float* dst = pts + (size_t)k * 12 + s * 3;
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
    for (int k = t; k < N; k += IRGB_THREADS) {
        unsigned m = 15u;
        if (amask) {
            const uint8_t* mk = amask + ((size_t)b * N + k) * A;
            m = (mk[0] ? 1u : 0u) | (mk[1] ? 2u : 0u) | (mk[3] ? 4u : 0u) | (mk[4] ? 8u : 0u);
        }
        bits[k] = m;
    }
    __syncthreads();

    // row sweep: the wave's rows one after the other, lanes over the partner index
    for (int rl = wave; rl < rows; rl += IRGB_THREADS / 64) {
        const int r = r0 + rl;
        f3 acc[3] = {f3{0.0f, 0.0f, 0.0f}, f3{0.0f, 0.0f, 0.0f}, f3{0.0f, 0.0f, 0.0f}};
        if (any) {
            const IrgbResidue own = irgb_residue(pts, bits, r);
            const size_t row = ((size_t)b * N + r) * N;
            for (int k = lane; k < N; k += 64) irgb_pair<true>(own, irgb_residue(pts, bits, k), k != r, g, row + k, acc);
        }
        float v[9] = {acc[0].x, acc[0].y, acc[0].z, acc[1].x, acc[1].y, acc[1].z, acc[2].x, acc[2].y, acc[2].z};
#pragma unroll
        for (int c = 0; c < 9; ++c) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v[c] += __shfl_xor(v[c], d, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) row_sum[rl * 9 + c] = v[c];
        }
    }

    // column sweep: lane % 32 is the owned residue, the eight half-waves stride the partner index
    {
        const int rl = t & (IRGB_TILE - 1), kg = t / IRGB_TILE;
        const bool valid = rl < rows;
        const int r = r0 + (valid ? rl : 0);
        f3 acc[3] = {f3{0.0f, 0.0f, 0.0f}, f3{0.0f, 0.0f, 0.0f}, f3{0.0f, 0.0f, 0.0f}};
        if (any && valid) {
            const IrgbResidue own = irgb_residue(pts, bits, r);
            for (int k = kg; k < N; k += IRGB_THREADS / IRGB_TILE)
                irgb_pair<false>(irgb_residue(pts, bits, k), own, k != r, g, ((size_t)b * N + k) * N + r, acc);
        }
        float v[9] = {acc[0].x, acc[0].y, acc[0].z, acc[1].x, acc[1].y, acc[1].z, acc[2].x, acc[2].y, acc[2].z};
#pragma unroll
        for (int c = 0; c < 9; ++c) v[c] += __shfl_xor(v[c], 32, 64);
        if (lane < IRGB_TILE) {
#pragma unroll
            for (int c = 0; c < 9; ++c) col_part[(wave * IRGB_TILE + rl) * 9 + c] = v[c];
        }
    }
    __syncthreads();

    // every slot of the owned residues: N, CA, O, CB from the sums, exact zeros elsewhere
    const int per_residue = A * 3;
    float* dst = grad_xyz + ((size_t)b * N + r0) * per_residue;
    for (int q = t; q < rows * per_residue; q += IRGB_THREADS) {
        const int rl = q / per_residue, rem = q - rl * per_residue, slot = rem / 3, c = rem - slot * 3;
        float val = 0.0f;
        if (slot == 0 || slot == 1 || slot == 3 || slot == 4) {
            const int rc = (slot == 0 ? 0 : slot == 1 ? 3 : 6) + c;      // row sums: N, CA, CB
            const int cc = (slot == 3 ? 0 : slot == 1 ? 3 : 6) + c;      // column sums: O, CA, CB
            const float rs = slot == 3 ? 0.0f : row_sum[rl * 9 + rc];
            float cs = 0.0f;
            if (slot != 0) {
                const float* p = col_part + rl * 9 + cc;
                cs = (p[0] + p[IRGB_TILE * 9]) + (p[2 * IRGB_TILE * 9] + p[3 * IRGB_TILE * 9]);
            }
            val = rs + cs;
        }
        dst[q] = val;
    }
}

extern "C" int ps_inter_residue_geometry_backward_f32(const float* xyz, const uint8_t* atom_mask, const float* g_d_ca,
                                                      const float* g_d_cb, const float* g_d_no, const float* g_omega,
                                                      const float* g_theta, const float* g_phi, float* grad_xyz, int B, int N,
                                                      int A, void* stream) {
    static_assert(IRGB_THREADS == 256 && IRGB_TILE == 32, "the sweeps' lane maps and the four-wave sum are written for 4 x 64 lanes, 32 residues");
    if (!xyz || !grad_xyz || B < 0 || N < 0 || A < 5 || N > IRGB_MAX_N) return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0) return 0;
    const int n_tiles = (N + IRGB_TILE - 1) / IRGB_TILE;
    const unsigned long long n_wg = (unsigned long long)n_tiles * (unsigned long long)B;
    if (n_wg > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned lds = irgb_lds_bytes(N);
    static unsigned long long prepared[1];
    if (lds > 64u * 1024u)
        if (const int e = k3_allow_big_lds(k3_inter_residue_geometry_backward, prepared, s)) return e;
    return ps_launch(k3_inter_residue_geometry_backward, dim3((unsigned)n_wg), dim3(IRGB_THREADS), lds, s, xyz, atom_mask, g_d_ca,
                     g_d_cb, g_d_no, g_omega, g_theta, g_phi, grad_xyz, N, A, n_tiles);
}
