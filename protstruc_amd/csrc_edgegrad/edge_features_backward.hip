// K52 - K54 -- the backward kernels of the edge features (K25 / K26 of csrc/edge_features.hip, K50 / K51 of
// csrc_csredge/csr_edge_features.hip).  The definitions, the order of every sum and the error analysis are in
// include/protstruc_edgegrad.h; this file restates the forward's distance and Gaussian so that the gradient is taken of
// the values the forward wrote.
//
// Rows are found as in K49 - K51: r(p) = the number of t in 1 .. n_rows with row_ptr[t] <= p, by a bisection whose `lo` and
// `hi` start at 0 and n_rows and only move towards each other, so every index read is in [1, n_rows] whatever row_ptr holds.
//
// K52, ps_csr_edge_rbf_backward_f32, is a streaming-LOAD kernel: 1600 bytes of g_rbf in and 300 bytes out per edge at
// P = 25, R = 16.  Its unit of work is a SPAN of G of K50's chunks of 64 consecutive edge positions, G = 64 / P up to 4: as
// many as keep the span's distances inside the 16 KB of LDS one chunk has at P = 64 and its positions at one per lane, so
// that with few pairs per edge a set-up (the row search) still has something to stream.  Per span: (1) rows and range-checked
// cols to LDS; (2) the span's distances once, in double, into LDS (negative: the pair gets 0 and nothing of it is read);
// (3) LP = ceil(R / 4) consecutive lanes take a pair, lane k the floats 4k .. 4k + 3 of its R incoming gradients, so a
// wave's 16-byte loads are consecutive; a wave takes 64 / LP pairs per round and the workgroup four times that, and the loads
// of INFLIGHT rounds are issued before the first of them is used.  The partial sums meet across the LP lanes in the fixed
// order of the header -- by DPP (quad_perm, row_half_mirror, row_mirror: a butterfly whose lane 0 is the tree of the header,
// addition being commutative) where LP is a power of two, by shuffles otherwise -- and lane 0 of the pair forms the three
// components and stores them.  The loop over rounds is uniform over the workgroup, so every cross-lane step runs with all
// lanes active.  A lane's (position, pair) is split once per kernel and advanced by constants: no division in the loop.
//
// The 16-byte arm and the dword arm are one template and differ in the load alone.
#include "ps_common.hpp"

#include <math.h>

#include "../../include/protstruc_edgegrad.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int CHUNK = PS_EDGEGRAD_CHUNK;
constexpr int INFLIGHT = 4;   // rounds whose loads are issued before the first is used

constexpr int MAX_SPAN_CHUNKS = THREADS / CHUNK;   // a lane per position of a span

static_assert(CHUNK * MAX_SPAN_CHUNKS <= THREADS, "one lane per position of a span");

// The host arrays of the call, by value in the kernel's arguments: read on the host before the call returns.
struct PairTables {
    int pair_i[PS_EDGEGRAD_MAX_PAIRS];
    int pair_j[PS_EDGEGRAD_MAX_PAIRS];
};

struct Centers {
    float centers[PS_EDGEGRAD_MAX_RBF];
};

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ long long row_of(const long long* __restrict__ row_ptr, long long n_rows, long long p) {
    long long lo = 0, hi = n_rows;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);   // lo <= mid < hi <= n_rows: row_ptr[mid + 1] is inside the array
        if (row_ptr[mid + 1] <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long long clamp_ll(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// The tree of the header over the LP partial sums held by LP consecutive lanes (lane k of the pair holds s_k); the result is
// lane 0's.  Runs with every lane of the wave active.
__device__ __forceinline__ double meet(double v, int k, int LP) {
    if ((LP & (LP - 1)) == 0) {   // a power of two: pairs are aligned to their own size inside a row of 16 lanes
        if (LP >= 2) v = v + dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
        if (LP >= 4) v = v + dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
        if (LP >= 8) v = v + dpp_f64<0x141>(v);   // row_half_mirror: the other four, all equal by now
        if (LP >= 16) v = v + dpp_f64<0x140>(v);  // row_mirror: the other eight
        return v;
    }
    for (int stride = 1; stride < LP; stride <<= 1) {
        const double other = __shfl_down(v, stride);
        if ((k & (2 * stride - 1)) == 0 && k + stride < LP) v = v + other;
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_rbf_backward(
    const float* __restrict__ xyz, const uint8_t* __restrict__ atom_mask, const float* __restrict__ src_xyz,
    const uint8_t* __restrict__ src_mask, const long long* __restrict__ row_ptr, const int* __restrict__ col, long long E,
    long long n_rows, const PairTables tab, const Centers cen, int P, int R, int LP, int span, float s, double kappa,
    const float* __restrict__ g_dist, const float* __restrict__ g_rbf, float* __restrict__ pair_grad, int M, int A, int Q,
    int As) {
    __shared__ int nbr[THREADS];                    // the target of every position of the span, -1: padding
    __shared__ int src_b[THREADS], src_q[THREADS];  // its source, (b, q)
    __shared__ int slot_i[PS_EDGEGRAD_MAX_PAIRS], slot_j[PS_EDGEGRAD_MAX_PAIRS];
    __shared__ float centre[PS_EDGEGRAD_MAX_RBF + 4];   // four more, so that a lane's four reads stay inside whatever R is
    __shared__ float dl[CHUNK * PS_EDGEGRAD_MAX_PAIRS];   // [position][pair], span * P <= 64 * 64; negative: the pair gets 0
    const int t = threadIdx.x;
    if (t < P) {
        slot_i[t] = tab.pair_i[t];
        slot_j[t] = tab.pair_j[t];
    }
    if (t < PS_EDGEGRAD_MAX_RBF + 4) centre[t] = t < R ? cen.centers[t] : 0.0f;

    // the lane's place, the same in every span: pair `lp` of its wave's 64 / LP, float quad `k` of the pair
    const int lane = t & 63, wave = t >> 6;
    const int ppw = 64 / LP, step = WAVES * ppw;
    const int lp = lane / LP, k = lane - lp * LP;
    const bool lane_ok = lp < ppw;
    const int first = wave * ppw + lp;                  // its pair in round 0, counted within the span
    const int first_sl = first / P, first_t = first - first_sl * P;
    const int step_sl = step / P, step_t = step - step_sl * P;
    const int mine = R - 4 * k < 4 ? R - 4 * k : 4;     // how many of the lane's four floats exist (>= 1: LP = ceil(R / 4))
    const long long spans = (E + span - 1) / span;

    for (long long at = blockIdx.x; at < spans; at += gridDim.x) {
        const long long p0 = at * span;
        const int n = E - p0 < span ? (int)(E - p0) : span;   // the last one may be short
        // (1) rows and targets, a lane each: span <= THREADS.  The barrier also orders the tables above.
        if (t < n) {
            const long long r = row_of(row_ptr, n_rows, p0 + t);
            int j = -1, b = 0, q = 0;
            if (r < n_rows) {
                j = col[p0 + t];
                j = (unsigned)j < (unsigned)M ? j : -1;
                b = (int)(r / Q);
                q = (int)(r - (long long)b * Q);
            }
            nbr[t] = j;
            src_b[t] = b;
            src_q[t] = q;
        }
        __syncthreads();
        // (2) the distances, once; d == 0 has no derivative and is marked like the padding
        const int NP = n * P;
        for (int e = t; e < NP; e += THREADS) {
            const int sl = e / P, p = e - sl * P;
            const int j = nbr[sl];
            float d = -1.0f;
            if (j >= 0) {
                const size_t b = (size_t)src_b[sl];
                const size_t ai = (b * (size_t)Q + (size_t)src_q[sl]) * (size_t)As + (size_t)slot_i[p];
                const size_t aj = (b * (size_t)M + (size_t)j) * (size_t)A + (size_t)slot_j[p];
                if ((!src_mask || src_mask[ai] != 0) && (!atom_mask || atom_mask[aj] != 0)) {
                    const f3 xi = load3(src_xyz + ai * 3), xj = load3(xyz + aj * 3);
                    const double dx = (double)xj.x - (double)xi.x, dy = (double)xj.y - (double)xi.y,
                                 dz = (double)xj.z - (double)xi.z;
                    d = (float)sqrt((dx * dx + dy * dy) + dz * dz);
                    d = d == 0.0f ? -1.0f : d;
                }
            }
            dl[e] = d;
        }
        __syncthreads();
        // (3) the incoming gradients, INFLIGHT rounds at a time
        const size_t pair0 = (size_t)p0 * (size_t)P;
        const float* __restrict__ gin = g_rbf ? g_rbf + pair0 * (size_t)R + (size_t)(4 * k) : nullptr;
        int pr = first, sl = first_sl, tt = first_t;
        for (int base = 0; base < NP; base += INFLIGHT * step) {   // uniform over the workgroup
            f32x4_t g[INFLIGHT];
            float dd[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const int pu = pr + u * step;
                dd[u] = (lane_ok && pu < NP) ? dl[pu] : -1.0f;
                g[u] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
                if (gin && !(dd[u] < 0.0f)) {   // nothing of a pair that gets 0 is read
                    const float* __restrict__ at = gin + (size_t)pu * (size_t)R;
                    if (VEC) {
                        g[u] = *reinterpret_cast<const f32x4_t*>(at);
                    } else {
                        g[u][0] = at[0];
                        if (mine > 1) g[u][1] = at[1];
                        if (mine > 2) g[u][2] = at[2];
                        if (mine > 3) g[u][3] = at[3];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                const int pu = pr + u * step;
                const bool live = !(dd[u] < 0.0f);
                double sum = 0.0;
                if (gin) {   // uniform
                    const float d = live ? dd[u] : 0.0f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float w = (d - centre[4 * k + i]) * s;
                        const float ew = __builtin_amdgcn_exp2f(-(w * w)) * w;
                        const double term = (double)g[u][i] * (double)ew;
                        if (i == 0)
                            sum = term;
                        else if (i < mine)
                            sum = sum + term;
                    }
                    sum = meet(live ? sum : 0.0, k, LP);
                }
                if (k == 0 && lane_ok && pu < NP) {
                    float fx = 0.0f, fy = 0.0f, fz = 0.0f;
                    if (live) {
                        const size_t b = (size_t)src_b[sl];
                        const size_t ai = (b * (size_t)Q + (size_t)src_q[sl]) * (size_t)As + (size_t)slot_i[tt];
                        const size_t aj = (b * (size_t)M + (size_t)nbr[sl]) * (size_t)A + (size_t)slot_j[tt];
                        const f3 xi = load3(src_xyz + ai * 3), xj = load3(xyz + aj * 3);
                        double total = kappa * sum;
                        if (g_dist) total = gin ? (double)g_dist[pair0 + (size_t)pu] + total : (double)g_dist[pair0 + (size_t)pu];
                        const double c = total / (double)dd[u];
                        fx = (float)(c * ((double)xj.x - (double)xi.x));
                        fy = (float)(c * ((double)xj.y - (double)xi.y));
                        fz = (float)(c * ((double)xj.z - (double)xi.z));
                    }
                    float* __restrict__ out = pair_grad + (pair0 + (size_t)pu) * 3;
                    out[0] = fx;
                    out[1] = fy;
                    out[2] = fz;
                }
                sl += step_sl;
                tt += step_t;
                if (tt >= P) {
                    tt -= P;
                    ++sl;
                }
            }
            pr += INFLIGHT * step;
        }
        // Stage (3) reads nbr, src_b, src_q and dl to its last round, and stage (1) of this workgroup's next span overwrites
        // them before its own first barrier: no wave may start that span while another still forms f for this one.
        __syncthreads();
    }
}

// K53: one lane per (owner, slot).  `out_ptr` (the owners are sources: f is subtracted at pair_i) and `in_ptr` (the owners
// are targets: f is added at pair_j) may each be NULL; with both, the outgoing loop comes first.  P <= 64, so the pairs
// that name a slot are one 64-bit mask per table, made once per lane: a slot no pair names walks no list at all.
__global__ __launch_bounds__(THREADS) void k_pair_grad_sum(const float* __restrict__ pair_grad,
                                                           const long long* __restrict__ out_ptr, long long E,
                                                           const long long* __restrict__ in_ptr,
                                                           const long long* __restrict__ in_edge, long long E_in,
                                                           const PairTables tab, int P, float* __restrict__ grad,
                                                           long long n_owners, int A) {
    __shared__ int slot_i[PS_EDGEGRAD_MAX_PAIRS], slot_j[PS_EDGEGRAD_MAX_PAIRS];
    if ((int)threadIdx.x < P) {
        slot_i[threadIdx.x] = tab.pair_i[threadIdx.x];
        slot_j[threadIdx.x] = tab.pair_j[threadIdx.x];
    }
    __syncthreads();
    const long long total = n_owners * (long long)A;
    for (long long at = (long long)blockIdx.x * THREADS + threadIdx.x; at < total; at += (long long)gridDim.x * THREADS) {
        const long long o = at / A;
        const int a = (int)(at - o * A);
        // the pairs that name this lane's slot, as bits: walked from the lowest, which is t ascending
        unsigned long long mine_i = 0, mine_j = 0;
        for (int t = 0; t < P; ++t) {
            mine_i |= (unsigned long long)(slot_i[t] == a) << t;
            mine_j |= (unsigned long long)(slot_j[t] == a) << t;
        }
        double ax = 0.0, ay = 0.0, az = 0.0;
        if (out_ptr && mine_i) {
            const long long lo = clamp_ll(out_ptr[o], E), hi = clamp_ll(out_ptr[o + 1], E);
            for (long long p = lo; p < hi; ++p) {
                const float* __restrict__ f = pair_grad + (size_t)p * (size_t)P * 3;
                for (unsigned long long m = mine_i; m; m &= m - 1) {
                    const int t = __builtin_ctzll(m);
                    ax = ax - (double)f[3 * t];
                    ay = ay - (double)f[3 * t + 1];
                    az = az - (double)f[3 * t + 2];
                }
            }
        }
        if (in_ptr && mine_j) {
            const long long lo = clamp_ll(in_ptr[o], E_in), hi = clamp_ll(in_ptr[o + 1], E_in);
            for (long long e = lo; e < hi; ++e) {
                const long long p = in_edge[e];
                if (p < 0 || p >= E) continue;
                const float* __restrict__ f = pair_grad + (size_t)p * (size_t)P * 3;
                for (unsigned long long m = mine_j; m; m &= m - 1) {
                    const int t = __builtin_ctzll(m);
                    ax = ax + (double)f[3 * t];
                    ay = ay + (double)f[3 * t + 1];
                    az = az + (double)f[3 * t + 2];
                }
            }
        }
        float* __restrict__ out = grad + (size_t)at * 3;
        out[0] = (float)ax;
        out[1] = (float)ay;
        out[2] = (float)az;
    }
}

// (R g)[r] = (R[r][0]*g[0] + R[r][1]*g[1]) + R[r][2]*g[2]
__device__ __forceinline__ double row_dot(const double* __restrict__ R, int r, double g0, double g1, double g2) {
    return (R[3 * r] * g0 + R[3 * r + 1] * g1) + R[3 * r + 2] * g2;
}

// K54: one lane per owner.  With `do_out` the owners are sources (b, q) and take the outgoing terms; with `do_in` they are
// targets (b, m) and take the incoming ones; the self graph does both, in this order, into the same accumulators.
__global__ __launch_bounds__(THREADS) void k_frames_backward(
    const float* __restrict__ rot, const float* __restrict__ trans, const uint8_t* __restrict__ frame_mask,
    const float* __restrict__ src_rot, const float* __restrict__ src_trans, const uint8_t* __restrict__ src_mask,
    const long long* __restrict__ row_ptr, long long n_rows, const int* __restrict__ col, long long E,
    const long long* __restrict__ in_ptr, const long long* __restrict__ in_edge, long long E_in,
    const float* __restrict__ g_pos, const float* __restrict__ g_rot, float* __restrict__ out_rot,
    float* __restrict__ out_trans, long long n_owners, int M, int Q, int do_out, int do_in) {
    for (long long o = (long long)blockIdx.x * THREADS + threadIdx.x; o < n_owners; o += (long long)gridDim.x * THREADS) {
        double aR[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double aT[3] = {0.0, 0.0, 0.0};
        if (do_out && (!src_mask || src_mask[o] != 0)) {   // o = b * Q + q
            const long long lo = clamp_ll(row_ptr[o], E), hi = clamp_ll(row_ptr[o + 1], E);
            if (lo < hi) {
                const size_t fi = (size_t)o;
                const size_t b = (size_t)(o / Q);
                double Ri[9], ti[3];
                for (int m = 0; m < 9; ++m) Ri[m] = (double)src_rot[fi * 9 + m];
                for (int m = 0; m < 3; ++m) ti[m] = (double)src_trans[fi * 3 + m];
                for (long long p = lo; p < hi; ++p) {
                    const int j = col[p];
                    if ((unsigned)j >= (unsigned)M) continue;
                    const size_t fj = b * (size_t)M + (size_t)j;
                    if (frame_mask && frame_mask[fj] == 0) continue;
                    double gp[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
                    if (g_pos) {
                        for (int m = 0; m < 3; ++m) {
                            gp[m] = (double)g_pos[(size_t)p * 3 + m];
                            v[m] = (double)trans[fj * 3 + m] - ti[m];
                        }
                        for (int r = 0; r < 3; ++r) aT[r] = aT[r] - row_dot(Ri, r, gp[0], gp[1], gp[2]);
                    }
                    if (g_rot) {
                        double Rj[9], gr[9];
                        for (int m = 0; m < 9; ++m) {
                            Rj[m] = (double)rot[fj * 9 + m];
                            gr[m] = (double)g_rot[(size_t)p * 9 + m];
                        }
                        for (int r = 0; r < 3; ++r)
                            for (int c = 0; c < 3; ++c) {
                                const double rsum = row_dot(Rj, r, gr[3 * c], gr[3 * c + 1], gr[3 * c + 2]);
                                aR[3 * r + c] = aR[3 * r + c] + (g_pos ? v[r] * gp[c] + rsum : rsum);
                            }
                    } else {
                        for (int r = 0; r < 3; ++r)
                            for (int c = 0; c < 3; ++c) aR[3 * r + c] = aR[3 * r + c] + v[r] * gp[c];
                    }
                }
            }
        }
        if (do_in && (!frame_mask || frame_mask[o] != 0)) {   // o = b * M + m
            const long long lo = clamp_ll(in_ptr[o], E_in), hi = clamp_ll(in_ptr[o + 1], E_in);
            const long long b = o / M;
            const int m_own = (int)(o - b * M);
            for (long long e = lo; e < hi; ++e) {
                const long long p = in_edge[e];
                if (p < 0 || p >= E) continue;
                const long long r_src = row_of(row_ptr, n_rows, p);
                if (r_src >= n_rows || col[p] != m_own || r_src / Q != b) continue;   // no edge of this owner
                if (src_mask && src_mask[r_src] == 0) continue;
                const size_t fi = (size_t)r_src;
                double Ri[9];
                for (int m = 0; m < 9; ++m) Ri[m] = (double)src_rot[fi * 9 + m];
                if (g_pos) {
                    const double g0 = (double)g_pos[(size_t)p * 3], g1 = (double)g_pos[(size_t)p * 3 + 1],
                                 g2 = (double)g_pos[(size_t)p * 3 + 2];
                    for (int r = 0; r < 3; ++r) aT[r] = aT[r] + row_dot(Ri, r, g0, g1, g2);
                }
                if (g_rot) {
                    double gr[9];
                    for (int m = 0; m < 9; ++m) gr[m] = (double)g_rot[(size_t)p * 9 + m];
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 3; ++c)
                            aR[3 * r + c] = aR[3 * r + c] + row_dot(Ri, r, gr[c], gr[3 + c], gr[6 + c]);
                }
            }
        }
        for (int m = 0; m < 9; ++m) out_rot[(size_t)o * 9 + m] = (float)aR[m];
        for (int m = 0; m < 3; ++m) out_trans[(size_t)o * 3 + m] = (float)aT[m];
    }
}

bool bad_sizes(int B, int M, int Q, long long E) {
    return B < 0 || B > 65535 || M < 0 || M > (1 << 24) || Q < 0 || Q > (1 << 24) || E < 0;
}

unsigned grid_for(long long items, long long cap) { return (unsigned)(items < cap ? items : cap); }

bool fill_pairs(PairTables& tab, const int32_t* pair_i, const int32_t* pair_j, int P, int As, int A) {
    for (int p = 0; p < P; ++p) {
        if (pair_i[p] < 0 || pair_i[p] >= As || pair_j[p] < 0 || pair_j[p] >= A) return false;
        tab.pair_i[p] = pair_i[p];
        tab.pair_j[p] = pair_j[p];
    }
    return true;
}

}  // namespace

extern "C" int ps_edgegrad_api(void) { return PS_EDGEGRAD_API; }

extern "C" int ps_csr_edge_rbf_backward_f32(const float* xyz, const uint8_t* atom_mask, const float* src_xyz,
                                            const uint8_t* src_mask, const long long* row_ptr, const int32_t* col, long long E,
                                            const int32_t* pair_i, const int32_t* pair_j, int P, const float* centers, int R,
                                            float sigma, const float* g_dist, const float* g_rbf, float* pair_grad, int B, int M,
                                            int A, int Q, int As, void* stream) {
    if (!xyz || !row_ptr || !col || !pair_i || !pair_j || !centers || (!g_dist && !g_rbf) || !pair_grad || bad_sizes(B, M, Q, E) ||
        A < 1 || As < 1 || P < 1 || P > PS_EDGEGRAD_MAX_PAIRS || R < 1 || R > PS_EDGEGRAD_MAX_RBF || !(sigma > 0.0f))
        return (int)hipErrorInvalidValue;
    if (!src_xyz) {   // the sources are the targets
        if (Q != M || As != A || src_mask) return (int)hipErrorInvalidValue;
        src_xyz = xyz;
        src_mask = atom_mask;
    }
    const double root = sqrt(1.4426950408889634);                 // sqrt(log2 e)
    const float s = (float)(root / (double)sigma);                // the forward's: exp(-z^2) = exp2(-(s (d - mu))^2)
    if (!(s > 0.0f && s < INFINITY)) return (int)hipErrorInvalidValue;
    const double kappa = -2.0 / ((double)sigma * root);
    PairTables tab = {};
    Centers cen = {};
    if (!fill_pairs(tab, pair_i, pair_j, P, As, A)) return (int)hipErrorInvalidValue;
    for (int c = 0; c < R; ++c) cen.centers[c] = centers[c];
    if (B == 0 || E == 0) return 0;
    const int LP = g_rbf ? (R + 3) / 4 : 1;   // lanes per pair; without g_rbf there is nothing to share
    const bool vec = g_rbf && R % 4 == 0 && ((uintptr_t)g_rbf & 15u) == 0;
    int G = PS_EDGEGRAD_MAX_PAIRS / P;   // chunks to a span: span * P distances fit where 64 * PS_EDGEGRAD_MAX_PAIRS do
    G = G < 1 ? 1 : (G > MAX_SPAN_CHUNKS ? MAX_SPAN_CHUNKS : G);
    const int span = CHUNK * G;
    const long long spans = (E + span - 1) / span;
    return ps_launch(vec ? k_rbf_backward<true> : k_rbf_backward<false>, dim3(grid_for(spans, 8192)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), xyz, atom_mask, src_xyz, src_mask, row_ptr, col, E, (long long)B * Q,
                     tab, cen, P, R, LP, span, s, kappa, g_dist, g_rbf, pair_grad, M, A, Q, As);
}

extern "C" int ps_csr_edge_pair_grad_sum_f32(const float* pair_grad, const long long* row_ptr, long long E,
                                             const long long* in_ptr, const long long* in_edge, long long E_in,
                                             const int32_t* pair_i, const int32_t* pair_j, int P, float* grad, float* grad_src,
                                             int B, int M, int A, int Q, int As, void* stream) {
    if (!row_ptr || !in_ptr || !pair_i || !pair_j || !grad || bad_sizes(B, M, Q, E) || E_in < 0 || (E > 0 && !pair_grad) ||
        (E_in > 0 && !in_edge) || A < 1 || As < 1 || P < 1 || P > PS_EDGEGRAD_MAX_PAIRS)
        return (int)hipErrorInvalidValue;
    if (!grad_src && (Q != M || As != A)) return (int)hipErrorInvalidValue;
    PairTables tab = {};
    if (!fill_pairs(tab, pair_i, pair_j, P, As, A)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long targets = (long long)B * M * A, sources = (long long)B * Q * As;
    if (targets > 0) {
        const int rc = ps_launch(k_pair_grad_sum, dim3(grid_for((targets + THREADS - 1) / THREADS, 65536)), dim3(THREADS), 0, st,
                                 pair_grad, grad_src ? nullptr : row_ptr, E, in_ptr, in_edge, E_in, tab, P, grad,
                                 (long long)B * M, A);
        if (rc) return rc;
    }
    if (grad_src && sources > 0)
        return ps_launch(k_pair_grad_sum, dim3(grid_for((sources + THREADS - 1) / THREADS, 65536)), dim3(THREADS), 0, st,
                         pair_grad, row_ptr, E, nullptr, nullptr, 0LL, tab, P, grad_src, (long long)B * Q, As);
    return 0;
}

extern "C" int ps_csr_edge_frames_backward_f32(const float* rot, const float* trans, const uint8_t* frame_mask,
                                               const float* src_rot, const float* src_trans, const uint8_t* src_mask,
                                               const long long* row_ptr, const int32_t* col, long long E,
                                               const long long* in_ptr, const long long* in_edge, long long E_in,
                                               const float* g_pos, const float* g_rot, float* grad_rot, float* grad_trans,
                                               float* grad_src_rot, float* grad_src_trans, int B, int M, int Q, void* stream) {
    if (!rot || !trans || !row_ptr || !in_ptr || !grad_rot || !grad_trans || (!g_pos && !g_rot) || bad_sizes(B, M, Q, E) ||
        E_in < 0 || (E > 0 && !col) || (E_in > 0 && !in_edge) || (!src_rot) != (!src_trans))
        return (int)hipErrorInvalidValue;
    const bool bipartite = src_rot != nullptr;
    if (bipartite ? (!grad_src_rot || !grad_src_trans) : (Q != M || src_mask || grad_src_rot || grad_src_trans))
        return (int)hipErrorInvalidValue;
    if (!bipartite) {   // the sources are the targets
        src_rot = rot;
        src_trans = trans;
        src_mask = frame_mask;
    }
    if (B == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long targets = (long long)B * M, sources = (long long)B * Q, n_rows = sources;
    if (targets > 0) {
        const int rc = ps_launch(k_frames_backward, dim3(grid_for((targets + THREADS - 1) / THREADS, 65536)), dim3(THREADS), 0, st,
                                 rot, trans, frame_mask, src_rot, src_trans, src_mask, row_ptr, n_rows, col, E, in_ptr, in_edge,
                                 E_in, g_pos, g_rot, grad_rot, grad_trans, targets, M, Q, bipartite ? 0 : 1, 1);
        if (rc) return rc;
    }
    if (bipartite && sources > 0)
        return ps_launch(k_frames_backward, dim3(grid_for((sources + THREADS - 1) / THREADS, 65536)), dim3(THREADS), 0, st, rot,
                         trans, frame_mask, src_rot, src_trans, src_mask, row_ptr, n_rows, col, E, in_ptr, in_edge, E_in, g_pos,
                         g_rot, grad_src_rot, grad_src_trans, sources, M, Q, 1, 0);
    return 0;
}
