// K15 / K16 -- lDDT (local distance difference test) per point, hard and smooth, and the gradient of the smooth form.
//
//   d_ij = sqrt(|x_i - x_j|^2 + eps)   d'_ij likewise on the target   delta_ij = |d_ij - d'_ij|
//   c_ij = p_i p_j [i != j] [group_i != group_j] [d'_ij < cutoff]
//   e_ij = (1/T) sum_t [delta_ij < thr_t]  (hard)      e_ij = (1/T) sum_t sigmoid(thr_t - delta_ij)  (smooth)
//   S_i  = sum_j c_ij e_ij             n_i = sum_j c_ij
//
// The sweep is the one of fape.hip: a workgroup is four waves that share 64 OWNERS, one point per lane, both sides in
// registers; the columns are staged through LDS in tiles of 256 raw points, one per thread, COMPACTED while staging (a
// masked point never reaches LDS, so NaN there never meets arithmetic); wave w takes the compacted items w, w + 4, ... --
// each read one address for the whole wave, an LDS broadcast -- and the four waves' sums are added in wave order through
// LDS.  No pair is ever written, there are no atomics and every sum has one fixed order: results repeat bit for bit.
//
// What differs from FAPE is that most pairs do not count: at cutoff = 15 a residue of a 512-residue chain has some
// dozens of neighbours.  The inclusion test needs the target side only, and no square root: it is taken on the squared
// distance, [|x'_i - x'_j|^2 + eps < cutoff^2], nine instructions, and a wave whose 64 owners all fail it for a column
// (one ballot) skips the rest of that pair -- two correctly rounded square roots, the exponential, T reciprocals.  The
// test is symmetric bit for bit (the differences are exact negatives of each other and are only squared), which the
// backward pass relies on: with c and e symmetric, grad_x_i is one row sweep per owner.
//
// The smooth pair costs one v_exp_f32 and T v_rcp_f32: sigmoid(thr - delta) = 1 / (1 + exp(delta) exp(-thr)) with
// exp(-thr_t) from the host.  exp's argument is capped at 2^126, so that its product with exp(-thr_t) (thresholds are
// at most 64: a normal float) is finite and the term is 0 to within 1e-10 where it should be.  S and the gradient are
// accumulated in double: only included pairs reach that add, and a sequential float sum of a hundred terms would lose
// what the terms themselves carry.
#include "ps_common.hpp"
#include "owner_sweep.hpp"   // WAVES, compact_slot and the barrier protocol of staging a tile

#include <math.h>

#include "../../include/protstruc_hip.h"

namespace {

constexpr int OWNERS = PS_LDDT_POINT_TILE;   // owners per workgroup = lanes per wave
constexpr int THREADS = OWNERS * WAVES;      // = raw points staged per tile
constexpr int POINT_FLOATS = 8;              // x (3), x' (3), key, w: two 16-byte broadcast reads
constexpr int MAX_T = PS_LDDT_MAX_THRESHOLDS;
static_assert(OWNERS == PS_WAVE, "one owner per lane");

struct thresholds_t {
    float thr[MAX_T];       // thr_t
    float exp_neg[MAX_T];   // exp(-thr_t)
    int count;
};

struct point_t {
    f3 xp, xt;
    int key;   // the group, or the point's own index where there are no groups: a pair counts iff the keys differ
    float w;   // dL/dS of the point (backward only)
};

// Stage raw points [m0, m0 + THREADS) of structure b, valid ones only, in index order; returns how many.
__device__ __forceinline__ int stage_points(const float* __restrict__ pts_p, const float* __restrict__ pts_t,
                                            const uint8_t* __restrict__ point_mask, const int* __restrict__ groups,
                                            const float* __restrict__ w, size_t b, int M, int m0, float* tile,
                                            int* wave_counts) {
    const int m = m0 + threadIdx.x;
    const bool valid = m < M && (!point_mask || point_mask[b * M + m] != 0);
    int total;
    const int slot = compact_slot(valid, wave_counts, total);
    if (valid) {
        const size_t at = b * M + m;
        const f3 xp = load3(pts_p + at * 3), xt = load3(pts_t + at * 3);
        const int key = groups ? groups[at] : m;
        float4* o = reinterpret_cast<float4*>(tile + slot * POINT_FLOATS);
        o[0] = make_float4(xp.x, xp.y, xp.z, xt.x);
        o[1] = make_float4(xt.y, xt.z, __int_as_float(key), w ? w[at] : 0.0f);
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ point_t read_point(const float* tile, int j) {
    const float4* p = reinterpret_cast<const float4*>(tile + j * POINT_FLOATS);
    const float4 a = p[0], c = p[1];
    return point_t{f3{a.x, a.y, a.z}, f3{a.w, c.x, c.y}, __float_as_int(c.z), c.w};
}

__device__ __forceinline__ point_t load_owner(const float* __restrict__ pts_p, const float* __restrict__ pts_t,
                                              const int* __restrict__ groups, const float* __restrict__ w, size_t b, int M,
                                              int i) {
    const int m = i < M ? i : M - 1;   // lanes past the end compute on the last point and are dropped
    const size_t at = b * M + m;
    return point_t{load3(pts_p + at * 3), load3(pts_t + at * 3), groups ? groups[at] : m, w ? w[at] : 0.0f};
}

// |a - b|^2 + eps: what both the inclusion test and the distances are taken from
__device__ __forceinline__ float sq_dist_eps(f3 a, f3 b, float eps, f3& diff) {
    diff = sub3(a, b);
    return norm_sq3(diff.x, diff.y, diff.z) + eps;
}

// exp(delta), capped at 2^126 (see the file header); v_exp_f32 is 2^x
__device__ __forceinline__ float exp_capped(float delta) {
    return __builtin_amdgcn_exp2f(fminf(delta * 1.44269504088896341f, 126.0f));
}

// ---- forward: owner i sums e_ij and counts c_ij over every valid point j -----------------------------------------------
template <bool SMOOTH>
__global__ __launch_bounds__(THREADS) void k_lddt_forward(const float* __restrict__ pts_p, const float* __restrict__ pts_t,
                                                          const uint8_t* __restrict__ point_mask,
                                                          const int* __restrict__ groups, float cutoff_sq,
                                                          thresholds_t th, float eps, float* __restrict__ S,
                                                          float* __restrict__ count, int M) {
    __shared__ __attribute__((aligned(16))) float tile[THREADS * POINT_FLOATS];
    __shared__ double wave_sums[WAVES * OWNERS];
    __shared__ int wave_pairs[WAVES * OWNERS];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int i = blockIdx.x * OWNERS + lane;
    const bool own = i < M && (!point_mask || point_mask[b * M + i] != 0);
    const point_t me = load_owner(pts_p, pts_t, groups, nullptr, b, M, i);
    double acc = 0.0;   // smooth: sum over pairs of sum_t sigmoid; an exact integer in the hard mode goes to hits
    int hits = 0, pairs = 0;
    for (int m0 = 0; m0 < M; m0 += THREADS) {
        const int n = stage_points(pts_p, pts_t, point_mask, groups, nullptr, b, M, m0, tile, wave_counts);
        for (int j = wave; j < n; j += WAVES) {
            const point_t o = read_point(tile, j);
            f3 dt, dp;
            const float qt = sq_dist_eps(me.xt, o.xt, eps, dt);
            const bool inc = qt < cutoff_sq && me.key != o.key;   // false for a NaN owner: by selection
            if (__ballot(inc) == 0ull) continue;                  // no owner of this wave counts column j
            pairs += inc;
            const float delta = fabsf(sqrt_rn_mk(sq_dist_eps(me.xp, o.xp, eps, dp)) - sqrt_rn_mk(qt));
            if (SMOOTH) {
                const float ex = exp_capped(delta);
                float sum = 0.0f;
                for (int t = 0; t < th.count; ++t) sum += __builtin_amdgcn_rcpf(__builtin_fmaf(ex, th.exp_neg[t], 1.0f));
                acc += (double)(inc ? sum : 0.0f);
            } else {
                int k = 0;
                for (int t = 0; t < th.count; ++t) k += delta < th.thr[t];
                hits += inc ? k : 0;
            }
        }
    }
    // the four waves' sums in wave order
    wave_sums[wave * OWNERS + lane] = SMOOTH ? acc : (double)hits;
    wave_pairs[wave * OWNERS + lane] = pairs;
    __syncthreads();
    if (wave != 0 || i >= M) return;
    const double sum = ((wave_sums[lane] + wave_sums[OWNERS + lane]) + wave_sums[2 * OWNERS + lane]) + wave_sums[3 * OWNERS + lane];
    const int np = ((wave_pairs[lane] + wave_pairs[OWNERS + lane]) + wave_pairs[2 * OWNERS + lane]) + wave_pairs[3 * OWNERS + lane];
    // one rounding to float; a masked owner, and an owner without a pair, get exact zeros
    S[b * M + i] = own && np > 0 ? (float)(sum / (double)th.count) : 0.0f;
    count[b * M + i] = own ? (float)np : 0.0f;
}

// ---- backward of the smooth form: owner i sums its row of the pair gradient ----------------------------------------------
__global__ __launch_bounds__(THREADS) void k_lddt_backward(const float* __restrict__ pts_p, const float* __restrict__ pts_t,
                                                           const uint8_t* __restrict__ point_mask,
                                                           const int* __restrict__ groups, float cutoff_sq,
                                                           thresholds_t th, float eps, const float* __restrict__ grad_S,
                                                           float* __restrict__ grad_pts, int M) {
    __shared__ __attribute__((aligned(16))) float tile[THREADS * POINT_FLOATS];
    __shared__ double wave_sums[WAVES * 3 * OWNERS];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int i = blockIdx.x * OWNERS + lane;
    const bool own = i < M && (!point_mask || point_mask[b * M + i] != 0);
    const point_t me = load_owner(pts_p, pts_t, groups, grad_S, b, M, i);
    // thousands of pulls of either sign add up to far less than their number: in double, as the sum of e in fape.hip
    double acc[3] = {0.0, 0.0, 0.0};
    for (int m0 = 0; m0 < M; m0 += THREADS) {
        const int n = stage_points(pts_p, pts_t, point_mask, groups, grad_S, b, M, m0, tile, wave_counts);
        for (int j = wave; j < n; j += WAVES) {
            const point_t o = read_point(tile, j);
            f3 dt, dp;
            const float qt = sq_dist_eps(me.xt, o.xt, eps, dt);
            const bool inc = qt < cutoff_sq && me.key != o.key;
            if (__ballot(inc) == 0ull) continue;
            const float d = sqrt_rn_mk(sq_dist_eps(me.xp, o.xp, eps, dp));
            const float diff = d - sqrt_rn_mk(qt);
            const float ex = exp_capped(fabsf(diff));
            float slope = 0.0f;   // sum_t s_t (1 - s_t)
            for (int t = 0; t < th.count; ++t) {
                const float s = __builtin_amdgcn_rcpf(__builtin_fmaf(ex, th.exp_neg[t], 1.0f));
                slope += s - s * s;
            }
            const float sign = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);   // sign(0) = 0, as autograd's abs
            const float pull = inc ? (me.w + o.w) * slope * sign * __builtin_amdgcn_rcpf(d) : 0.0f;
            acc[0] += (double)(pull * dp.x);
            acc[1] += (double)(pull * dp.y);
            acc[2] += (double)(pull * dp.z);
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
        o[k] = own ? (float)(-s / (double)th.count) : 0.0f;   // exact zeros at masked points, by selection
    }
}

// The arguments both entries share; fills what the kernels take by value.
bool bad_arguments(const float* pts_p, const float* pts_t, float cutoff, const float* thresholds, int T, float eps, int B,
                   int M, thresholds_t& th, float& cutoff_sq) {
    if (!pts_p || !pts_t || !thresholds || B < 0 || M < 0 || B > 65535 || M > (1 << 30) || T < 1 || T > MAX_T ||
        !(cutoff > 0.0f) || !(eps >= 0.0f) || isinf(cutoff) || isinf(eps))
        return true;
    for (int t = 0; t < MAX_T; ++t) th.thr[t] = th.exp_neg[t] = 0.0f;
    for (int t = 0; t < T; ++t) {
        const float v = thresholds[t];
        if (!(v > 0.0f) || !(v <= PS_LDDT_MAX_THRESHOLD) || (t > 0 && !(v > thresholds[t - 1]))) return true;
        th.thr[t] = v;
        th.exp_neg[t] = (float)exp(-(double)v);
    }
    th.count = T;
    cutoff_sq = cutoff * cutoff;
    return isinf(cutoff_sq);
}

}  // namespace

extern "C" int ps_lddt_f32(const float* pts_p, const float* pts_t, const uint8_t* point_mask, const int32_t* groups,
                           float cutoff, const float* thresholds, int T, int smooth, float eps, float* S, float* count,
                           int B, int M, void* stream) {
    thresholds_t th;
    float cutoff_sq;
    if (bad_arguments(pts_p, pts_t, cutoff, thresholds, T, eps, B, M, th, cutoff_sq) || !S || !count)
        return (int)hipErrorInvalidValue;
    if (B == 0 || M == 0) return 0;
    const dim3 grid((unsigned)((M + OWNERS - 1) / OWNERS), (unsigned)B);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (smooth)
        return ps_launch(k_lddt_forward<true>, grid, dim3(THREADS), 0, s, pts_p, pts_t, point_mask, groups, cutoff_sq, th,
                         eps, S, count, M);
    return ps_launch(k_lddt_forward<false>, grid, dim3(THREADS), 0, s, pts_p, pts_t, point_mask, groups, cutoff_sq, th, eps,
                     S, count, M);
}

extern "C" int ps_lddt_backward_f32(const float* pts_p, const float* pts_t, const uint8_t* point_mask,
                                    const int32_t* groups, float cutoff, const float* thresholds, int T, float eps,
                                    const float* grad_S, float* grad_pts, int B, int M, void* stream) {
    thresholds_t th;
    float cutoff_sq;
    if (bad_arguments(pts_p, pts_t, cutoff, thresholds, T, eps, B, M, th, cutoff_sq) || !grad_S || !grad_pts)
        return (int)hipErrorInvalidValue;
    if (B == 0 || M == 0) return 0;
    return ps_launch(k_lddt_backward, dim3((unsigned)((M + OWNERS - 1) / OWNERS), (unsigned)B), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), pts_p, pts_t, point_mask, groups, cutoff_sq, th, eps, grad_S,
                     grad_pts, M);
}
