// K13 / K14 -- frame-aligned point error (FAPE, AlphaFold 2 suppl. alg. 28) and its gradient, fused.
//
//   u_ij = R_i^T (x_j - t_i)   u'_ij = R'_i^T (x'_j - t'_i)   d_ij = sqrt(|u_ij - u'_ij|^2 + eps)
//   loss_b = (1 / scale) * sum_ij f_i p_j min(d_ij, clamp_b) / max(sum_ij f_i p_j, 1)
//
// An all-pairs sweep over tiny inputs: no pair is ever written.  A workgroup is four waves that share 64 OWNERS, one
// per lane (forward and the frame role of the backward: 64 frames, both sides in registers; the point role of the
// backward: 64 points).  The other side is staged through LDS in tiles of 256 raw items, one per thread, COMPACTED
// while staging: a masked-out item never reaches LDS, so the caller may pass the whole (B, N*A, 3) view of xyz with
// atom_mask as the point mask, and NaN at a masked item never reaches any arithmetic.  Wave w takes the compacted
// items w, w + 4, ... of every tile -- each read is one address for the whole wave, an LDS broadcast -- and the four
// waves' sums are added in wave order through LDS.  Owner-computes on both sides of the backward: nothing is saved
// from the forward, there are no atomics, and every sum has one fixed order, so results repeat bit for bit.
#include "ps_common.hpp"
#include "owner_sweep.hpp"   // WAVES, compact_slot and the barrier protocol of staging a tile

#include "../../include/protstruc_hip.h"

namespace {

constexpr int OWNERS = PS_FAPE_FRAME_TILE;   // owners per workgroup = lanes per wave
constexpr int THREADS = OWNERS * WAVES;      // = raw items staged per tile
constexpr int POINT_FLOATS = 8;              // x (3), x' (3), 2 of padding: two 16-byte broadcast reads
constexpr int FRAME_FLOATS = 24;             // R (9), t (3), R' (9), t' (3): six 16-byte broadcast reads
static_assert(OWNERS == PS_WAVE, "one owner per lane");

struct frame_t {
    float r[9];   // row-major; the basis vectors are the columns
    f3 t;
};

__device__ __forceinline__ frame_t load_frame(const float* __restrict__ rot, const float* __restrict__ trans, size_t i) {
    frame_t f;
#pragma unroll
    for (int k = 0; k < 9; ++k) f.r[k] = rot[i * 9 + k];
    f.t = load3(trans + i * 3);
    return f;
}

// R^T v: component c is column c of R dotted with v
__device__ __forceinline__ f3 rot_t_apply(const float (&r)[9], f3 v) {
    return f3{__builtin_fmaf(r[6], v.z, __builtin_fmaf(r[3], v.y, r[0] * v.x)),
              __builtin_fmaf(r[7], v.z, __builtin_fmaf(r[4], v.y, r[1] * v.x)),
              __builtin_fmaf(r[8], v.z, __builtin_fmaf(r[5], v.y, r[2] * v.x))};
}

// R v
__device__ __forceinline__ f3 rot_apply(const float (&r)[9], f3 v) {
    return f3{__builtin_fmaf(r[2], v.z, __builtin_fmaf(r[1], v.y, r[0] * v.x)),
              __builtin_fmaf(r[5], v.z, __builtin_fmaf(r[4], v.y, r[3] * v.x)),
              __builtin_fmaf(r[8], v.z, __builtin_fmaf(r[7], v.y, r[6] * v.x))};
}

// One pair: dp = x - t (the lever arm grad_rot needs), diff = u - u', and d.  x == t gives dp = 0, u = 0 exactly, so a
// frame's own origin on both sides gives d = sqrt(eps) exactly (correctly rounded square root).
__device__ __forceinline__ float pair_distance(const frame_t& fp, const frame_t& ft, f3 xp, f3 xt, float eps, f3& dp,
                                               f3& diff) {
    dp = sub3(xp, fp.t);
    const f3 u = rot_t_apply(fp.r, dp);
    const f3 v = rot_t_apply(ft.r, sub3(xt, ft.t));
    diff = sub3(u, v);
    return sqrt_rn_mk(norm_sq3(diff.x, diff.y, diff.z) + eps);
}

// Number of non-zero bytes of mask[0 .. n) (n if mask is NULL), the same value in every thread.  scratch: THREADS ints.
__device__ int count_mask(const uint8_t* __restrict__ mask, int n, int* scratch) {
    if (!mask) return n;
    int c = 0;
    for (int k = threadIdx.x; k < n; k += THREADS) c += mask[k] != 0;
    __syncthreads();
    scratch[threadIdx.x] = c;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) scratch[threadIdx.x] += scratch[threadIdx.x + s];
        __syncthreads();
    }
    c = scratch[0];
    __syncthreads();
    return c;
}

// Stage raw points [m0, m0 + THREADS) of structure b, valid ones only, in index order; returns how many.
__device__ __forceinline__ int stage_points(const float* __restrict__ pts_p, const float* __restrict__ pts_t,
                                            const uint8_t* __restrict__ point_mask, size_t b, int M, int m0, float* tile,
                                            int* wave_counts) {
    const int m = m0 + threadIdx.x;
    const bool valid = m < M && (!point_mask || point_mask[b * M + m] != 0);
    int total;
    const int slot = compact_slot(valid, wave_counts, total);
    if (valid) {
        const f3 xp = load3(pts_p + (b * M + m) * 3), xt = load3(pts_t + (b * M + m) * 3);
        float4* o = reinterpret_cast<float4*>(tile + slot * POINT_FLOATS);
        o[0] = make_float4(xp.x, xp.y, xp.z, xt.x);
        o[1] = make_float4(xt.y, xt.z, 0.0f, 0.0f);
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ void read_point(const float* tile, int j, f3& xp, f3& xt) {
    const float4* p = reinterpret_cast<const float4*>(tile + j * POINT_FLOATS);
    const float4 a = p[0], c = p[1];
    xp = f3{a.x, a.y, a.z};
    xt = f3{a.w, c.x, c.y};
}

// ---- forward: workgroup (tile, b) sums min(d, clamp) over its 64 frames and every valid point ------------------------
__global__ __launch_bounds__(THREADS) void k_fape_forward(
    const float* __restrict__ rot_p, const float* __restrict__ trans_p, const float* __restrict__ pts_p,
    const float* __restrict__ rot_t, const float* __restrict__ trans_t, const float* __restrict__ pts_t,
    const uint8_t* __restrict__ frame_mask, const uint8_t* __restrict__ point_mask, const float* __restrict__ clamp,
    float eps, double* __restrict__ partials, int N, int M) {
    __shared__ __attribute__((aligned(16))) float tile[THREADS * POINT_FLOATS];
    __shared__ double wave_sums[WAVES];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int i = blockIdx.x * OWNERS + lane;
    const bool own = i < N && (!frame_mask || frame_mask[b * N + i] != 0);
    const size_t fi = b * N + (i < N ? i : N - 1);   // lanes past the end compute on the last frame and are dropped
    const frame_t fp = load_frame(rot_p, trans_p, fi), ft = load_frame(rot_t, trans_t, fi);
    const float cl = clamp[b];
    // Every term is at least floor = min(sqrt(eps), clamp), the value of a perfectly placed point.  The sum is taken over
    // what exceeds it and the floor is added back once at the end (k_fape_finish): a structure compared with itself then
    // reports sqrt(eps) / scale exactly, and the accumulators carry only the part of the loss that says something.
    const float floor = fminf(sqrt_rn_mk(eps), cl);
    // The running sum is a double: more than half of the terms of a clamped structure are the SAME number (clamp - floor),
    // and adding one float to a growing float sum a thousand times rounds the same way every time, a bias that no averaging
    // over lanes removes.  One conversion and one v_add_f64 per pair.
    double acc = 0.0;
    for (int m0 = 0; m0 < M; m0 += THREADS) {
        const int n = stage_points(pts_p, pts_t, point_mask, b, M, m0, tile, wave_counts);
        for (int j = wave; j < n; j += WAVES) {
            f3 xp, xt, dp, diff;
            read_point(tile, j, xp, xt);
            acc += (double)(fminf(pair_distance(fp, ft, xp, xt, eps, dp, diff), cl) - floor);
        }
    }
    double sum = own ? acc : 0.0;   // by selection: NaN of a masked frame stops here
    // fixed-order reduction in double (once per workgroup): a butterfly over the wave's lanes, then the four waves in order
#pragma unroll
    for (int s = PS_WAVE / 2; s > 0; s >>= 1) sum += __shfl_xor(sum, s);
    if (lane == 0) wave_sums[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[b * gridDim.x + blockIdx.x] = ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

// One workgroup per structure: the tiles' partial sums in index order, the pair count from the masks.
__global__ __launch_bounds__(THREADS) void k_fape_finish(const double* __restrict__ partials, int tiles,
                                                         const uint8_t* __restrict__ frame_mask,
                                                         const uint8_t* __restrict__ point_mask,
                                                         const float* __restrict__ clamp, float scale, float eps,
                                                         float* __restrict__ loss, float* __restrict__ count, int N, int M) {
    __shared__ int scratch[THREADS];
    const size_t b = blockIdx.x;
    const long long nf = count_mask(frame_mask ? frame_mask + b * N : nullptr, N, scratch);
    const long long np = count_mask(point_mask ? point_mask + b * M : nullptr, M, scratch);
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int k = 0; k < tiles; ++k) sum += partials[b * tiles + k];
    const long long pairs = nf * np;
    count[b] = (float)pairs;
    const double floor = (double)fminf(sqrt_rn_mk(eps), clamp[b]);
    // one rounding to float; no valid pair: loss 0, whatever the masked data hold
    loss[b] = pairs > 0 ? (float)((floor + sum / (double)pairs) / (double)scale) : 0.0f;
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// Workgroups [0, frame_tiles) of a structure own 64 frames each and sweep the points (grad_rot, grad_trans); workgroups
// [frame_tiles, frame_tiles + point_tiles) own 64 points each and sweep the frames (grad_pts).  Either range may be empty.
__global__ __launch_bounds__(THREADS) void k_fape_backward(
    const float* __restrict__ rot_p, const float* __restrict__ trans_p, const float* __restrict__ pts_p,
    const float* __restrict__ rot_t, const float* __restrict__ trans_t, const float* __restrict__ pts_t,
    const uint8_t* __restrict__ frame_mask, const uint8_t* __restrict__ point_mask, const float* __restrict__ clamp,
    float scale, float eps, const float* __restrict__ grad_loss, float* __restrict__ grad_rot,
    float* __restrict__ grad_trans, float* __restrict__ grad_pts, int N, int M, int frame_tiles) {
    __shared__ __attribute__((aligned(16))) float tile[THREADS * FRAME_FLOATS];
    __shared__ int scratch[THREADS];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const float cl = clamp[b];

    if ((int)blockIdx.x < frame_tiles) {
        const int nf = count_mask(frame_mask ? frame_mask + b * N : nullptr, N, scratch);
        const int i = blockIdx.x * OWNERS + lane;
        const bool own = i < N && (!frame_mask || frame_mask[b * N + i] != 0);
        const size_t fi = b * N + (i < N ? i : N - 1);
        const frame_t fp = load_frame(rot_p, trans_p, fi), ft = load_frame(rot_t, trans_t, fi);
        float acc[12];   // [0, 9): sum of (x - t) e^T, row-major; [9, 12): sum of e
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
        // sum of e in double: thousands of unit vectors of either sign add up to about the square root of their number, and
        // a sequential float sum rounds at the size of its partial sums, not of its result.  The lever-arm products of
        // grad_rot are not cancelling sums.
        double es[3] = {0.0, 0.0, 0.0};
        int np = 0;
        for (int m0 = 0; m0 < M; m0 += THREADS) {
            const int n = stage_points(pts_p, pts_t, point_mask, b, M, m0, tile, wave_counts);
            np += n;
            for (int j = wave; j < n; j += WAVES) {
                f3 xp, xt, dp, diff;
                read_point(tile, j, xp, xt);
                const float d = pair_distance(fp, ft, xp, xt, eps, dp, diff);
                const float inv = d < cl ? __builtin_amdgcn_rcpf(d) : 0.0f;   // a clamped pair passes no gradient
                const f3 e = scale3(diff, inv);
                acc[0] = __builtin_fmaf(dp.x, e.x, acc[0]); acc[1] = __builtin_fmaf(dp.x, e.y, acc[1]); acc[2] = __builtin_fmaf(dp.x, e.z, acc[2]);
                acc[3] = __builtin_fmaf(dp.y, e.x, acc[3]); acc[4] = __builtin_fmaf(dp.y, e.y, acc[4]); acc[5] = __builtin_fmaf(dp.y, e.z, acc[5]);
                acc[6] = __builtin_fmaf(dp.z, e.x, acc[6]); acc[7] = __builtin_fmaf(dp.z, e.y, acc[7]); acc[8] = __builtin_fmaf(dp.z, e.z, acc[8]);
                es[0] += (double)e.x; es[1] += (double)e.y; es[2] += (double)e.z;
            }
        }
        // the four waves' sums in wave order (tile is free: stage_points ended with a barrier and nothing reads it now)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[9 + k] = (float)es[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) tile[(wave * 12 + k) * OWNERS + lane] = acc[k];
        __syncthreads();
        if (wave != 0 || i >= N) return;
#pragma unroll
        for (int k = 0; k < 12; ++k)
            acc[k] = ((tile[k * OWNERS + lane] + tile[(12 + k) * OWNERS + lane]) + tile[(24 + k) * OWNERS + lane]) +
                     tile[(36 + k) * OWNERS + lane];
        const long long pairs = (long long)nf * np;
        const bool live = own && pairs > 0;
        const float w = live ? grad_loss[b] / (scale * (float)pairs) : 0.0f;
        if (grad_rot) {
            float* o = grad_rot + (b * N + i) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) o[k] = live ? w * acc[k] : 0.0f;   // exact zeros at masked frames, by selection
        }
        if (grad_trans) {
            const f3 g = rot_apply(fp.r, f3{acc[9], acc[10], acc[11]});
            float* o = grad_trans + (b * N + i) * 3;
            o[0] = live ? -w * g.x : 0.0f;
            o[1] = live ? -w * g.y : 0.0f;
            o[2] = live ? -w * g.z : 0.0f;
        }
        return;
    }

    const int np = count_mask(point_mask ? point_mask + b * M : nullptr, M, scratch);
    const int j = (blockIdx.x - frame_tiles) * OWNERS + lane;
    const bool own = j < M && (!point_mask || point_mask[b * M + j] != 0);
    const size_t pj = b * M + (j < M ? j : M - 1);
    const f3 xp = load3(pts_p + pj * 3), xt = load3(pts_t + pj * 3);
    f3 acc = f3{0.0f, 0.0f, 0.0f};   // sum of R e
    int nf = 0;
    for (int i0 = 0; i0 < N; i0 += THREADS) {
        const int i = i0 + threadIdx.x;
        const bool valid = i < N && (!frame_mask || frame_mask[b * N + i] != 0);
        int n;
        const int slot = compact_slot(valid, wave_counts, n);
        if (valid) {
            const float* r0 = rot_p + (b * N + i) * 9;
            const float* r1 = rot_t + (b * N + i) * 9;
            const float* t0 = trans_p + (b * N + i) * 3;
            const float* t1 = trans_t + (b * N + i) * 3;
            float* o = tile + slot * FRAME_FLOATS;
#pragma unroll
            for (int k = 0; k < 9; ++k) { o[k] = r0[k]; o[12 + k] = r1[k]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { o[9 + k] = t0[k]; o[21 + k] = t1[k]; }
        }
        __syncthreads();
        nf += n;
        for (int k = wave; k < n; k += WAVES) {
            const float4* p = reinterpret_cast<const float4*>(tile + k * FRAME_FLOATS);
            const float4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3], q4 = p[4], q5 = p[5];
            const frame_t fp = {{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x}, f3{q2.y, q2.z, q2.w}};
            const frame_t ft = {{q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, q4.z, q4.w, q5.x}, f3{q5.y, q5.z, q5.w}};
            f3 dp, diff;
            const float d = pair_distance(fp, ft, xp, xt, eps, dp, diff);
            const float inv = d < cl ? __builtin_amdgcn_rcpf(d) : 0.0f;
            const f3 g = rot_apply(fp.r, scale3(diff, inv));
            acc.x += g.x; acc.y += g.y; acc.z += g.z;
        }
    }
    __syncthreads();
    tile[(wave * 3 + 0) * OWNERS + lane] = acc.x;
    tile[(wave * 3 + 1) * OWNERS + lane] = acc.y;
    tile[(wave * 3 + 2) * OWNERS + lane] = acc.z;
    __syncthreads();
    if (wave != 0 || j >= M) return;
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        s[k] = ((tile[k * OWNERS + lane] + tile[(3 + k) * OWNERS + lane]) + tile[(6 + k) * OWNERS + lane]) +
               tile[(9 + k) * OWNERS + lane];
    const long long pairs = (long long)nf * np;
    const bool live = own && pairs > 0;
    const float w = live ? grad_loss[b] / (scale * (float)pairs) : 0.0f;
    float* o = grad_pts + (b * M + j) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = live ? w * s[k] : 0.0f;   // exact zeros at masked points, by selection
}

bool bad_sizes(int B, int N, int M) {
    // a grid dimension per structure; 32-bit item indices inside a structure
    return B < 0 || N < 0 || M < 0 || B > 65535 || N > (1 << 30) || M > (1 << 30);
}

}  // namespace

extern "C" int ps_fape_f32(const float* rot_p, const float* trans_p, const float* pts_p, const float* rot_t,
                           const float* trans_t, const float* pts_t, const uint8_t* frame_mask,
                           const uint8_t* point_mask, const float* clamp, float scale, float eps, float* loss,
                           float* count, double* partials, int B, int N, int M, void* stream) {
    if (!rot_p || !trans_p || !pts_p || !rot_t || !trans_t || !pts_t || !clamp || !loss || !count || !partials ||
        bad_sizes(B, N, M) || !(scale > 0.0f) || !(eps >= 0.0f))
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int tiles = (N + OWNERS - 1) / OWNERS;
    if (tiles > 0 && M > 0) {
        const int rc = ps_launch(k_fape_forward, dim3((unsigned)tiles, (unsigned)B), dim3(THREADS), 0, s, rot_p, trans_p,
                                 pts_p, rot_t, trans_t, pts_t, frame_mask, point_mask, clamp, eps, partials, N, M);
        if (rc) return rc;
    }
    // no frame or no point: no partial sum is read (the finish kernel sees no pair), loss = 0 and count = 0
    return ps_launch(k_fape_finish, dim3((unsigned)B), dim3(THREADS), 0, s, partials, M > 0 ? tiles : 0, frame_mask,
                     point_mask, clamp, scale, eps, loss, count, N, M);
}

extern "C" int ps_fape_backward_f32(const float* rot_p, const float* trans_p, const float* pts_p, const float* rot_t,
                                    const float* trans_t, const float* pts_t, const uint8_t* frame_mask,
                                    const uint8_t* point_mask, const float* clamp, float scale, float eps,
                                    const float* grad_loss, float* grad_rot, float* grad_trans, float* grad_pts, int B,
                                    int N, int M, void* stream) {
    if (!rot_p || !trans_p || !pts_p || !rot_t || !trans_t || !pts_t || !clamp || !grad_loss ||
        (!grad_rot && !grad_trans && !grad_pts) || bad_sizes(B, N, M) || !(scale > 0.0f) || !(eps >= 0.0f))
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    // an empty side: the other side's outputs are all zeros (no pair), written by its owners sweeping nothing
    const int frame_tiles = (grad_rot || grad_trans) ? (N + OWNERS - 1) / OWNERS : 0;
    const int point_tiles = grad_pts ? (M + OWNERS - 1) / OWNERS : 0;
    if (frame_tiles + point_tiles == 0) return 0;
    return ps_launch(k_fape_backward, dim3((unsigned)(frame_tiles + point_tiles), (unsigned)B), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), rot_p, trans_p, pts_p, rot_t, trans_t, pts_t, frame_mask,
                     point_mask, clamp, scale, eps, grad_loss, grad_rot, grad_trans, grad_pts, N, M, frame_tiles);
}
