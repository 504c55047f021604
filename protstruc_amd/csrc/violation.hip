// K17 - K20 -- structural violations (AlphaFold 2 suppl. 1.9.11, eq. 44-47): the steric clash energy per point with its
// gradient, and the peptide-bond geometry at every junction r -> r+1 with its gradient.
//
//   d_ij = sqrt(|x_i - x_j|^2 + eps)          s_ij = radius_i + radius_j - tolerance
//   c_ij = p_i p_j [i != j] [group_i != group_j] [not (link_i == link_j >= 0)]
//   v_ij = max(0, s_ij - d_ij)                E_i = sum_j c_ij v_ij          n_i = sum_j c_ij [v_ij > 0]
//
// The clash sweep is the one of lddt.hip: a workgroup is four waves that share 64 OWNERS, one point per lane in
// registers; the columns are staged through LDS in tiles of 256 raw points, one per thread, COMPACTED while staging (a
// masked point never reaches LDS, so NaN there never meets arithmetic); wave w takes the compacted items w, w + 4, ... --
// each read one address for the whole wave, an LDS broadcast -- and the four waves' sums are added in wave order through
// LDS.  No pair is ever written, there are no atomics and every sum has one fixed order: results repeat bit for bit.
//
// Almost no pair clashes: s is about 2 A and a structure has a handful of atoms that close to any one atom.  The test
// [s_ij > 0 and |x_i - x_j|^2 + eps < s_ij^2] is taken in fp32 on the squared distance -- a dozen instructions, no square
// root -- and a wave whose 64 owners all fail it for a column (one ballot) skips the rest of the pair.  It gives the same
// bits for (i, j) and (j, i): the differences are exact negatives and are only squared, and the radii are added, which
// commutes.  With c and the test symmetric, grad_x_i is one row sweep per owner.
//
// The survivors are evaluated in DOUBLE.  v = s - d is a difference of nearly equal numbers: in fp32 a pair that just
// clashes (v = 1e-4) would carry the rounding of s and d, 1e-7 each, as a relative error of 1e-3 in its owner's energy.
// The coordinates and radii are fp32 values, so their differences and sums are exact in double and the square root is
// correctly rounded there; only the few survivors pay for it.  E and the gradient are accumulated in double and rounded
// to fp32 once; n is counted in integers.
//
// The bond kernels are one lane per junction (forward) and one lane per residue (backward: it recomputes the residue's
// two junctions and writes the residue's whole (A,3) row, so no atomics are needed); a dozen loads and a few hundred
// flops per lane, evaluated in double for the same reason -- |l - l0| - tau sigma is a difference of small numbers.
#include "ps_common.hpp"
#include "owner_sweep.hpp"   // WAVES, compact_slot and the barrier protocol of staging a tile

#include <math.h>

#include "../../include/protstruc_hip.h"

namespace {

constexpr int OWNERS = PS_CLASH_POINT_TILE;   // owners per workgroup = lanes per wave
constexpr int THREADS = OWNERS * WAVES;       // = raw points staged per tile
constexpr int POINT_FLOATS = 8;               // x (3), radius, key, link, w, unused: two 16-byte broadcast reads
static_assert(OWNERS == PS_WAVE, "one owner per lane");

struct atom_t {
    f3 x;
    float radius;
    int key;    // the group, or the point's own index where there are no groups: a pair counts only if the keys differ
    int link;   // two points with the same non-negative link never clash; -1 where there are no links
    float w;    // dL/dE of the point (backward only)
};

__device__ __forceinline__ atom_t load_atom(const float* __restrict__ pts, const float* __restrict__ radius,
                                            const int* __restrict__ groups, const int* __restrict__ link,
                                            const float* __restrict__ w, size_t b, int M, int m) {
    const size_t at = b * M + m;
    return atom_t{load3(pts + at * 3), radius[at], groups ? groups[at] : m, link ? link[at] : -1, w ? w[at] : 0.0f};
}

// Stage raw points [m0, m0 + THREADS) of structure b, valid ones only, in index order; returns how many.
__device__ __forceinline__ int stage_atoms(const float* __restrict__ pts, const float* __restrict__ radius,
                                           const uint8_t* __restrict__ point_mask, const int* __restrict__ groups,
                                           const int* __restrict__ link, const float* __restrict__ w, size_t b, int M,
                                           int m0, float* tile, int* wave_counts) {
    const int m = m0 + threadIdx.x;
    const bool valid = m < M && (!point_mask || point_mask[b * M + m] != 0);
    int total;
    const int slot = compact_slot(valid, wave_counts, total);
    if (valid) {
        const atom_t a = load_atom(pts, radius, groups, link, w, b, M, m);
        float4* o = reinterpret_cast<float4*>(tile + slot * POINT_FLOATS);
        o[0] = make_float4(a.x.x, a.x.y, a.x.z, a.radius);
        o[1] = make_float4(__int_as_float(a.key), __int_as_float(a.link), a.w, 0.0f);
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ atom_t read_atom(const float* tile, int j) {
    const float4* p = reinterpret_cast<const float4*>(tile + j * POINT_FLOATS);
    const float4 a = p[0], c = p[1];
    return atom_t{f3{a.x, a.y, a.z}, a.w, __float_as_int(c.x), __float_as_int(c.y), c.z};
}

// The fp32 test that decides whether a pair is evaluated at all; false for NaN on either side, by comparison.
__device__ __forceinline__ bool may_clash(const atom_t& me, const atom_t& o, float tolerance, float eps) {
    const f3 diff = sub3(me.x, o.x);
    const float q = norm_sq3(diff.x, diff.y, diff.z) + eps;
    const float s = (me.radius + o.radius) - tolerance;
    const bool counts = me.key != o.key && !(me.link == o.link && me.link >= 0);
    return counts && s > 0.0f && q < s * s;
}

// The pair in double: v = s - d and the difference vector; exact inputs (fp32 values), a correctly rounded square root.
__device__ __forceinline__ double overlap(const atom_t& me, const atom_t& o, float tolerance, float eps, double (&diff)[3],
                                          double& d) {
    diff[0] = (double)me.x.x - (double)o.x.x;
    diff[1] = (double)me.x.y - (double)o.x.y;
    diff[2] = (double)me.x.z - (double)o.x.z;
    d = sqrt(((diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]) + (double)eps);
    return (((double)me.radius + (double)o.radius) - (double)tolerance) - d;
}

// ---- K17: owner i sums v_ij and counts [v_ij > 0] over every valid point j --------------------------------------------
__global__ __launch_bounds__(THREADS) void k_clash_forward(const float* __restrict__ pts, const float* __restrict__ radius,
                                                           const uint8_t* __restrict__ point_mask,
                                                           const int* __restrict__ groups, const int* __restrict__ link,
                                                           float tolerance, float eps, float* __restrict__ E,
                                                           float* __restrict__ count, int M) {
    __shared__ __attribute__((aligned(16))) float tile[THREADS * POINT_FLOATS];
    __shared__ double wave_sums[WAVES * OWNERS];
    __shared__ int wave_hits[WAVES * OWNERS];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int i = blockIdx.x * OWNERS + lane;
    const bool own = i < M && (!point_mask || point_mask[b * M + i] != 0);
    // lanes past the end compute on the last point and are dropped
    const atom_t me = load_atom(pts, radius, groups, link, nullptr, b, M, i < M ? i : M - 1);
    double acc = 0.0;
    int hits = 0;
    for (int m0 = 0; m0 < M; m0 += THREADS) {
        const int n = stage_atoms(pts, radius, point_mask, groups, link, nullptr, b, M, m0, tile, wave_counts);
        for (int j = wave; j < n; j += WAVES) {
            const atom_t o = read_atom(tile, j);
            const bool inc = may_clash(me, o, tolerance, eps);
            if (__ballot(inc) == 0ull) continue;   // no owner of this wave comes near column j
            double diff[3], d;
            const double v = overlap(me, o, tolerance, eps, diff, d);
            const bool hit = inc && v > 0.0;
            acc += hit ? v : 0.0;
            hits += hit;
        }
    }
    // the four waves' sums in wave order
    wave_sums[wave * OWNERS + lane] = acc;
    wave_hits[wave * OWNERS + lane] = hits;
    __syncthreads();
    if (wave != 0 || i >= M) return;
    const double sum = ((wave_sums[lane] + wave_sums[OWNERS + lane]) + wave_sums[2 * OWNERS + lane]) + wave_sums[3 * OWNERS + lane];
    const int nh = ((wave_hits[lane] + wave_hits[OWNERS + lane]) + wave_hits[2 * OWNERS + lane]) + wave_hits[3 * OWNERS + lane];
    // one rounding to float; a masked owner gets exact zeros by selection
    E[b * M + i] = own ? (float)sum : 0.0f;
    count[b * M + i] = own ? (float)nh : 0.0f;
}

// ---- K18: owner i sums its row of the pair gradient ---------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_clash_backward(const float* __restrict__ pts, const float* __restrict__ radius,
                                                            const uint8_t* __restrict__ point_mask,
                                                            const int* __restrict__ groups, const int* __restrict__ link,
                                                            float tolerance, float eps, const float* __restrict__ grad_E,
                                                            float* __restrict__ grad_pts, int M) {
    __shared__ __attribute__((aligned(16))) float tile[THREADS * POINT_FLOATS];
    __shared__ double wave_sums[WAVES * 3 * OWNERS];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int i = blockIdx.x * OWNERS + lane;
    const bool own = i < M && (!point_mask || point_mask[b * M + i] != 0);
    const atom_t me = load_atom(pts, radius, groups, link, grad_E, b, M, i < M ? i : M - 1);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int m0 = 0; m0 < M; m0 += THREADS) {
        const int n = stage_atoms(pts, radius, point_mask, groups, link, grad_E, b, M, m0, tile, wave_counts);
        for (int j = wave; j < n; j += WAVES) {
            const atom_t o = read_atom(tile, j);
            const bool inc = may_clash(me, o, tolerance, eps);
            if (__ballot(inc) == 0ull) continue;
            double diff[3], d;
            const double v = overlap(me, o, tolerance, eps, diff, d);
            // relu'(0) = 0, as under autograd; d = 0 (eps = 0, coincident points) gives 0 / 0 = NaN, as there
            const bool hit = inc && v > 0.0;
            const double pull = ((double)me.w + (double)o.w) / d;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] += hit ? pull * diff[k] : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) wave_sums[(wave * 3 + k) * OWNERS + lane] = acc[k];
    __syncthreads();
    if (wave != 0 || i >= M) return;
    float* o = grad_pts + (b * M + i) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double s = ((wave_sums[k * OWNERS + lane] + wave_sums[(3 + k) * OWNERS + lane]) +
                          wave_sums[(6 + k) * OWNERS + lane]) + wave_sums[(9 + k) * OWNERS + lane];
        o[k] = own ? (float)(-s) : 0.0f;   // exact zeros at masked points, by selection
    }
}

// ---- K19 / K20: the peptide bond -----------------------------------------------------------------------------------------
struct bond_constants_t {
    float v[PS_PEPTIDE_BOND_CONSTANTS];   // l0, sigma_l, l0_pro, sigma_l_pro, cos_cacn, sigma_cacn, cos_cnca, sigma_cnca, tau, eps, 0, 0
};

struct d3 {
    double x, y, z;
};

__device__ __forceinline__ d3 loadd(const float* __restrict__ p) { return d3{(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ d3 subd(d3 a, d3 b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 addd(d3 a, d3 b) { return d3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ d3 scaled(d3 a, double s) { return d3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dotd(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// max(0, |value - centre| - slack) and its derivative with respect to value; |.| and max(0, .) have derivative 0 at the kink
__device__ __forceinline__ double flat_bottom(double value, double centre, double slack, double& slope) {
    const double off = value - centre, over = fabs(off) - slack;
    slope = over > 0.0 ? (off > 0.0 ? 1.0 : (off < 0.0 ? -1.0 : 0.0)) : 0.0;
    return over > 0.0 ? over : 0.0;
}

// cos of the angle at the common origin of a and b, with unit(v) = v / sqrt(|v|^2 + eps); ga, gb: its gradients
__device__ __forceinline__ double cos_between(d3 a, d3 b, double eps, d3& ga, d3& gb) {
    const double na = sqrt(dotd(a, a) + eps), nb = sqrt(dotd(b, b) + eps);
    const d3 ua = scaled(a, 1.0 / na), ub = scaled(b, 1.0 / nb);
    const double c = dotd(ua, ub);
    ga = scaled(subd(ub, scaled(ua, c)), 1.0 / na);
    gb = scaled(subd(ua, scaled(ub, c)), 1.0 / nb);
    return c;
}

// The junction from a residue with atoms C, CA to the next with atoms N', CA': the three violations and, weighted by
// g[3], their gradient with respect to the four atoms.
struct junction_t {
    double viol[3];
    d3 g_c, g_ca, g_n, g_can;
};

__device__ __forceinline__ junction_t junction(const float* __restrict__ res, const float* __restrict__ next, int n_slot,
                                               int ca_slot, int c_slot, bool proline, const bond_constants_t& k,
                                               const double (&g)[3]) {
    const d3 C = loadd(res + c_slot * 3), CA = loadd(res + ca_slot * 3);
    const d3 N = loadd(next + n_slot * 3), CAn = loadd(next + ca_slot * 3);
    const double tau = (double)k.v[8], eps = (double)k.v[9];
    junction_t out;
    double slope;
    // the bond C - N'
    const d3 bond = subd(N, C);
    const double l = sqrt(dotd(bond, bond) + eps);
    out.viol[0] = flat_bottom(l, (double)(proline ? k.v[2] : k.v[0]), tau * (double)(proline ? k.v[3] : k.v[1]), slope);
    const d3 gl = scaled(bond, g[0] * slope / l);   // towards N'; its negative towards C
    // the angle CA - C - N'
    d3 ga, gb;
    out.viol[1] = flat_bottom(cos_between(subd(CA, C), bond, eps, ga, gb), (double)k.v[4], tau * (double)k.v[5], slope);
    ga = scaled(ga, g[1] * slope);
    gb = scaled(gb, g[1] * slope);
    // the angle C - N' - CA'
    d3 gc, ge;
    out.viol[2] = flat_bottom(cos_between(subd(C, N), subd(CAn, N), eps, gc, ge), (double)k.v[6], tau * (double)k.v[7], slope);
    gc = scaled(gc, g[2] * slope);
    ge = scaled(ge, g[2] * slope);
    out.g_ca = ga;
    out.g_can = ge;
    out.g_c = subd(gc, addd(gl, addd(ga, gb)));
    out.g_n = subd(addd(gl, gb), addd(gc, ge));
    return out;
}

__device__ __forceinline__ bool junction_valid(const uint8_t* __restrict__ junction_mask, size_t b, int N, int r) {
    return r >= 0 && r < N - 1 && (!junction_mask || junction_mask[b * N + r] != 0);
}

__global__ __launch_bounds__(256) void k_peptide_bond(const float* __restrict__ xyz, const uint8_t* __restrict__ junction_mask,
                                                      const uint8_t* __restrict__ next_is_proline, bond_constants_t k,
                                                      float* __restrict__ viol, size_t n_res, int N, int A, int n_slot,
                                                      int ca_slot, int c_slot) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n_res) return;
    const size_t b = at / N;
    const int r = (int)(at - b * N);
    const bool valid = junction_valid(junction_mask, b, N, r);
    const bool proline = valid && next_is_proline && next_is_proline[at] != 0;
    // the last residue of a structure reads itself as its successor and is dropped
    const float* res = xyz + at * (size_t)A * 3;
    const float* next = r < N - 1 ? res + (size_t)A * 3 : res;
    const double none[3] = {0.0, 0.0, 0.0};
    const junction_t j = junction(res, next, n_slot, ca_slot, c_slot, proline, k, none);
#pragma unroll
    for (int t = 0; t < 3; ++t) viol[at * 3 + t] = valid ? (float)j.viol[t] : 0.0f;   // exact zeros by selection
}

__global__ __launch_bounds__(256) void k_peptide_bond_backward(const float* __restrict__ xyz,
                                                               const uint8_t* __restrict__ junction_mask,
                                                               const uint8_t* __restrict__ next_is_proline,
                                                               bond_constants_t k, const float* __restrict__ grad_viol,
                                                               float* __restrict__ grad_xyz, size_t n_res, int N, int A,
                                                               int n_slot, int ca_slot, int c_slot) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n_res) return;
    const size_t b = at / N;
    const int r = (int)(at - b * N);
    const float* res = xyz + at * (size_t)A * 3;
    const d3 zero = d3{0.0, 0.0, 0.0};
    d3 g_n = zero, g_ca = zero, g_c = zero;
    // the junction r-1 -> r gives this residue's N and CA their share, the junction r -> r+1 its CA and C
    if (junction_valid(junction_mask, b, N, r - 1)) {
        const float* gv = grad_viol + (at - 1) * 3;
        const double g[3] = {(double)gv[0], (double)gv[1], (double)gv[2]};
        const bool proline = next_is_proline && next_is_proline[at - 1] != 0;
        const junction_t j = junction(res - (size_t)A * 3, res, n_slot, ca_slot, c_slot, proline, k, g);
        g_n = j.g_n;
        g_ca = j.g_can;
    }
    if (junction_valid(junction_mask, b, N, r)) {
        const float* gv = grad_viol + at * 3;
        const double g[3] = {(double)gv[0], (double)gv[1], (double)gv[2]};
        const bool proline = next_is_proline && next_is_proline[at] != 0;
        const junction_t j = junction(res, res + (size_t)A * 3, n_slot, ca_slot, c_slot, proline, k, g);
        g_ca = addd(g_ca, j.g_ca);
        g_c = j.g_c;
    }
    float* o = grad_xyz + at * (size_t)A * 3;
    for (int s = 0; s < A; ++s) {
        const d3 v = s == n_slot ? g_n : (s == ca_slot ? g_ca : (s == c_slot ? g_c : zero));
        o[s * 3 + 0] = (float)v.x;
        o[s * 3 + 1] = (float)v.y;
        o[s * 3 + 2] = (float)v.z;
    }
}

bool bad_clash_arguments(const float* pts, const float* radius, float tolerance, float eps, int B, int M) {
    return !pts || !radius || B < 0 || M < 0 || B > 65535 || M > (1 << 30) || isnan(tolerance) || isinf(tolerance) ||
           !(eps >= 0.0f) || isinf(eps);
}

// The arguments both bond entries share; fills what the kernels take by value.
bool bad_bond_arguments(const float* xyz, int B, int N, int A, int n_slot, int ca_slot, int c_slot, const float* constants,
                        bond_constants_t& k) {
    if (!xyz || !constants || B < 0 || N < 0 || A <= 0 || (long long)B * N > (1ll << 31)) return true;
    if (n_slot < 0 || n_slot >= A || ca_slot < 0 || ca_slot >= A || c_slot < 0 || c_slot >= A || n_slot == ca_slot ||
        n_slot == c_slot || ca_slot == c_slot)
        return true;
    for (int t = 0; t < PS_PEPTIDE_BOND_CONSTANTS; ++t) {
        k.v[t] = constants[t];
        if (isnan(k.v[t]) || isinf(k.v[t])) return true;
    }
    // the sigmas, tau and eps are non-negative
    return k.v[1] < 0.0f || k.v[3] < 0.0f || k.v[5] < 0.0f || k.v[7] < 0.0f || k.v[8] < 0.0f || k.v[9] < 0.0f;
}

}  // namespace

extern "C" int ps_clash_f32(const float* pts, const float* radius, const uint8_t* point_mask, const int32_t* groups,
                            const int32_t* link, float tolerance, float eps, float* E, float* count, int B, int M,
                            void* stream) {
    if (bad_clash_arguments(pts, radius, tolerance, eps, B, M) || !E || !count) return (int)hipErrorInvalidValue;
    if (B == 0 || M == 0) return 0;
    return ps_launch(k_clash_forward, dim3((unsigned)((M + OWNERS - 1) / OWNERS), (unsigned)B), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), pts, radius, point_mask, groups, link, tolerance, eps, E, count, M);
}

extern "C" int ps_clash_backward_f32(const float* pts, const float* radius, const uint8_t* point_mask,
                                     const int32_t* groups, const int32_t* link, float tolerance, float eps,
                                     const float* grad_E, float* grad_pts, int B, int M, void* stream) {
    if (bad_clash_arguments(pts, radius, tolerance, eps, B, M) || !grad_E || !grad_pts) return (int)hipErrorInvalidValue;
    if (B == 0 || M == 0) return 0;
    return ps_launch(k_clash_backward, dim3((unsigned)((M + OWNERS - 1) / OWNERS), (unsigned)B), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), pts, radius, point_mask, groups, link, tolerance, eps, grad_E,
                     grad_pts, M);
}

extern "C" int ps_peptide_bond_f32(const float* xyz, const uint8_t* junction_mask, const uint8_t* next_is_proline,
                                   int n_slot, int ca_slot, int c_slot, const float* constants, float* viol, int B, int N,
                                   int A, void* stream) {
    bond_constants_t k;
    if (bad_bond_arguments(xyz, B, N, A, n_slot, ca_slot, c_slot, constants, k) || !viol) return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    return ps_launch(k_peptide_bond, dim3((unsigned)((n_res + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), xyz, junction_mask, next_is_proline, k, viol, n_res, N, A, n_slot,
                     ca_slot, c_slot);
}

extern "C" int ps_peptide_bond_backward_f32(const float* xyz, const uint8_t* junction_mask, const uint8_t* next_is_proline,
                                            int n_slot, int ca_slot, int c_slot, const float* constants,
                                            const float* grad_viol, float* grad_xyz, int B, int N, int A, void* stream) {
    bond_constants_t k;
    if (bad_bond_arguments(xyz, B, N, A, n_slot, ca_slot, c_slot, constants, k) || !grad_viol || !grad_xyz)
        return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    return ps_launch(k_peptide_bond_backward, dim3((unsigned)((n_res + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), xyz, junction_mask, next_is_proline, k, grad_viol, grad_xyz, n_res,
                     N, A, n_slot, ca_slot, c_slot);
}
