// K25 / K26 -- edge features on a neighbour graph: what a structure network computes from the lists of K24.
//
// K25, ps_edge_rbf_f32.  For an edge (i, s) with j = idx[b][i][s] and an atom pair p = (pair_i[p] on i, pair_j[p] on j):
//   X = (double)x      dx = Xj.x - Xi.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz     in double, in this order
//   d = (float)sqrt(d2)                                        -- K24's distance: defined bit for bit
//   rbf[p*R + c] = exp(-z*z),  z = (d - centers[c]) / sigma    -- in fp32, within 1e-6 absolute of the float64 value
// An edge is PADDING where j is outside [0, N) -- any such value, not only K24's -1, so nothing in idx can send a load out
// of bounds --, and a pair is MASKED where either atom is outside atom_mask: dist and rbf are exactly 0 there, and the
// coordinates are never read.  An unmasked NaN propagates.  Every output element is written; no atomics.
//
// How z is evaluated: w = (d - centers[c]) * s with s = fl32(sqrt(log2 e) / sigma), computed in double and rounded once on
// the host, and rbf = exp2(-(w*w)) by the hardware's v_exp_f32.  With t = z*z: the difference, the product and s carry
// half an ulp each and squaring doubles them, the square adds another half: under 4 ulp of 2^-24 relative on t, which
// moves exp(-t) by at most 4 * 2^-24 * max(t e^-t) = 4 * 6e-8 * 0.37 < 1e-7; the exp2 adds 1 ulp of a value <= 1.  A result
// below the normal range is flushed to 0, an error under 1.2e-38.
//
// The kernel is a streaming-store kernel: 180 bytes of neighbour coordinates come in per 1600 bytes that go out (k = 48,
// P = 25, R = 16), and neighbours are shared, so the loads are L2 hits.  A workgroup takes whole source residues.  Per
// residue: (1) the k neighbour indices go to LDS, range-checked; (2) the k*P distances are computed once, one per thread
// and round, into LDS (at most 64 * 64 * 4 = 16 KB; a negative value marks padding or a masked pair), and written to
// `dist` from there; (3) all lanes stream the row of k*P*R floats out, each lane four consecutive floats per round as one
// 16-byte store, consecutive lanes on consecutive 16 bytes.  The output base is only 4-byte aligned and a row's length
// need not be a multiple of 4, so the up to three floats before the first 16-byte boundary of the row's ACTUAL address
// and the up to three after the last whole 16 bytes are single stores: nothing outside the row is touched.  A lane's
// walk over (pair, centre) takes no division inside the loop: element e = q*R + c is split once per row and then
// advanced by the constant (1024 / R, 1024 % R) per round and by one per float.
//
// All output offsets are 64-bit: B*N*k*P*R passes 2^31 well inside the supported range (B = 128, N = 512, k = 48, P = 25,
// R = 16 is 1.26e9 already).  No test can cover the far side of 2^31 in seconds; the offsets below are size_t products
// of int factors, each widened before it is multiplied.  A row's own length k*P*R <= 2^18 stays an int.
//
// Plain against non-temporal stores: PS_EDGE_RBF_NT selects `nt` at build time; the library is built with plain stores.
// Both were measured once; the readings are in DESIGN.md section 4 (K25).
//
// K26, ps_edge_frames_f32: the neighbour's frame in the source residue's frame, 12 floats per edge, one lane per edge.
//   v = t_j - t_i
//   local_pos[c]  = (R_i[0][c]*v0 + R_i[1][c]*v1) + R_i[2][c]*v2                       = (R_i^T v)[c]
//   rel_rot[a][c] = (R_i[0][a]*R_j[0][c] + R_i[1][a]*R_j[1][c]) + R_i[2][a]*R_j[2][c]  = (R_i^T R_j)[a][c]
// in double on the fp32 inputs in exactly this order, each value rounded to fp32 once; -ffp-contract=off is part of the
// definition.  Exactly 0 at the padding and where i or j is outside frame_mask.
#include "ps_common.hpp"

#include <math.h>

#include "../../include/protstruc_hip.h"

#ifndef PS_EDGE_RBF_NT
#define PS_EDGE_RBF_NT 0
#endif

namespace {

constexpr int THREADS = 256;
constexpr int FLOATS_PER_ROUND = 4 * THREADS;   // what the workgroup streams out per round

// The host arrays of the call, by value in the kernel's arguments: read on the host before the call returns.
struct RbfTables {
    int pair_i[PS_EDGE_MAX_PAIRS];
    int pair_j[PS_EDGE_MAX_PAIRS];
    float centers[PS_EDGE_MAX_RBF];
};

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void store16(float* p, f32x4_t v) {
    if (PS_EDGE_RBF_NT)
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4_t*>(p));
    else
        *reinterpret_cast<f32x4_t*>(p) = v;
}

// d < 0 marks padding or a masked pair (a NaN distance compares false and propagates)
__device__ __forceinline__ float rbf_value(float d, float mu, float s) {
    const float w = (d - mu) * s;
    return d < 0.0f ? 0.0f : __builtin_amdgcn_exp2f(-(w * w));
}

__global__ __launch_bounds__(THREADS) void k_edge_rbf(const float* __restrict__ xyz, const uint8_t* __restrict__ atom_mask,
                                                      const int* __restrict__ idx, const RbfTables tab, int P, int R, float s,
                                                      float* __restrict__ dist, float* __restrict__ rbf, int N, int A, int k) {
    __shared__ int nbr[PS_KNN_MAX_K];
    __shared__ int slot_i[PS_EDGE_MAX_PAIRS], slot_j[PS_EDGE_MAX_PAIRS];
    __shared__ float centre[PS_EDGE_MAX_RBF];
    __shared__ float dl[PS_KNN_MAX_K * PS_EDGE_MAX_PAIRS];   // [slot][pair]
    const int t = threadIdx.x;
    const size_t b = blockIdx.y;
    if (t < P) {
        slot_i[t] = tab.pair_i[t];
        slot_j[t] = tab.pair_j[t];
    }
    if (t < R) centre[t] = tab.centers[t];
    const int KP = k * P, L = KP * R;
    const int dq = FLOATS_PER_ROUND / R, dc = FLOATS_PER_ROUND - dq * R;

    for (int i = blockIdx.x; i < N; i += gridDim.x) {
        const size_t row = b * N + i;
        // (1) the neighbours; anything outside [0, N) is padding.  The barrier also orders the tables above and, from the
        // second residue on, the last reads of `dl` before its next writes.
        if (t < k) {
            const int j = idx[row * k + t];
            nbr[t] = (unsigned)j < (unsigned)N ? j : -1;
        }
        __syncthreads();
        // (2) the distances, once
        for (int e = t; e < KP; e += THREADS) {
            const int sl = e / P, p = e - sl * P;
            const int j = nbr[sl];
            float d = -1.0f;
            if (j >= 0) {
                const size_t ai = row * A + slot_i[p], aj = (b * N + j) * A + slot_j[p];
                if (!atom_mask || (atom_mask[ai] != 0 && atom_mask[aj] != 0)) {
                    const f3 xi = load3(xyz + ai * 3), xj = load3(xyz + aj * 3);
                    const double dx = (double)xj.x - (double)xi.x, dy = (double)xj.y - (double)xi.y,
                                 dz = (double)xj.z - (double)xi.z;
                    d = (float)sqrt((dx * dx + dy * dy) + dz * dz);
                }
            }
            dl[e] = d;
            if (dist) dist[row * KP + e] = d < 0.0f ? 0.0f : d;
        }
        __syncthreads();
        if (!rbf) continue;
        // (3) the row of L floats
        float* __restrict__ out = rbf + row * (size_t)L;
        int head = (int)((4u - (unsigned)((uintptr_t)out >> 2)) & 3u);
        head = head < L ? head : L;
        const int body = (L - head) >> 2, tail = head + 4 * body;
        {   // at most three single floats on either side, by the first lanes
            const int e = t < head ? t : tail + (t - head);
            if (t < head || e < L) {
                const int q = e / R;
                out[e] = rbf_value(dl[q], centre[e - q * R], s);
            }
        }
        int e = head + 4 * t;
        int q = e / R, c = e - q * R;
        for (int v = t; v < body; v += THREADS) {
            f32x4_t x;
            int qq = q, cc = c;
            for (int u = 0; u < 4; ++u) {
                x[u] = rbf_value(dl[qq], centre[cc], s);
                if (++cc == R) {
                    cc = 0;
                    ++qq;
                }
            }
            store16(out + head + 4 * (size_t)v, x);
            q += dq;
            c += dc;
            if (c >= R) {
                c -= R;
                ++q;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_edge_frames(const float* __restrict__ rot, const float* __restrict__ trans,
                                                         const uint8_t* __restrict__ frame_mask,
                                                         const int* __restrict__ idx, float* __restrict__ local_pos,
                                                         float* __restrict__ rel_rot, int N, int k) {
    const size_t b = blockIdx.y;
    const size_t edges = (size_t)N * k;   // of one structure
    for (size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x; e < edges; e += (size_t)gridDim.x * THREADS) {
        const size_t i = e / (unsigned)k;
        const size_t at = b * edges + e, fi = b * N + i;
        const int j = idx[at];
        bool real = (unsigned)j < (unsigned)N;
        const size_t fj = b * N + (real ? j : 0);
        if (real && frame_mask) real = frame_mask[fi] != 0 && frame_mask[fj] != 0;
        float pos[3] = {0.0f, 0.0f, 0.0f};
        float rr[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (real) {
            double Ri[9];
            for (int m = 0; m < 9; ++m) Ri[m] = (double)rot[fi * 9 + m];
            if (local_pos) {
                const double v0 = (double)trans[fj * 3] - (double)trans[fi * 3],
                             v1 = (double)trans[fj * 3 + 1] - (double)trans[fi * 3 + 1],
                             v2 = (double)trans[fj * 3 + 2] - (double)trans[fi * 3 + 2];
                for (int c = 0; c < 3; ++c) pos[c] = (float)((Ri[c] * v0 + Ri[3 + c] * v1) + Ri[6 + c] * v2);
            }
            if (rel_rot) {
                double Rj[9];
                for (int m = 0; m < 9; ++m) Rj[m] = (double)rot[fj * 9 + m];
                for (int a = 0; a < 3; ++a)
                    for (int c = 0; c < 3; ++c)
                        rr[3 * a + c] = (float)((Ri[a] * Rj[c] + Ri[3 + a] * Rj[3 + c]) + Ri[6 + a] * Rj[6 + c]);
            }
        }
        if (local_pos)
            for (int c = 0; c < 3; ++c) local_pos[at * 3 + c] = pos[c];
        if (rel_rot)
            for (int m = 0; m < 9; ++m) rel_rot[at * 9 + m] = rr[m];
    }
}

bool bad_batch(int B, int N) { return B < 0 || N < 0 || B > 65535 || N > (1 << 24); }

}  // namespace

extern "C" int ps_edge_rbf_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* idx, const int32_t* pair_i,
                               const int32_t* pair_j, int P, const float* centers, int R, float sigma, float* dist,
                               float* rbf, int B, int N, int A, int k, void* stream) {
    if (!xyz || !idx || !pair_i || !pair_j || !centers || (!dist && !rbf) || bad_batch(B, N) || A < 1 || k < 1 ||
        k > PS_KNN_MAX_K || P < 1 || P > PS_EDGE_MAX_PAIRS || R < 1 || R > PS_EDGE_MAX_RBF || !(sigma > 0.0f))
        return (int)hipErrorInvalidValue;
    const float s = (float)(sqrt(1.4426950408889634) / (double)sigma);   // sqrt(log2 e) / sigma: exp(-z^2) = exp2(-(s (d - mu))^2)
    if (!(s > 0.0f && s < INFINITY)) return (int)hipErrorInvalidValue;    // sigma infinite, or too small for fp32
    RbfTables tab = {};
    for (int p = 0; p < P; ++p) {
        if (pair_i[p] < 0 || pair_i[p] >= A || pair_j[p] < 0 || pair_j[p] >= A) return (int)hipErrorInvalidValue;
        tab.pair_i[p] = pair_i[p];
        tab.pair_j[p] = pair_j[p];
    }
    for (int c = 0; c < R; ++c) tab.centers[c] = centers[c];
    if (B == 0 || N == 0) return 0;
    // a workgroup walks residues i, i + grid, ...: enough workgroups to fill any device, few enough to amortise the tables
    const unsigned gx = (unsigned)(N < 1024 ? N : 1024);
    return ps_launch(k_edge_rbf, dim3(gx, (unsigned)B), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz,
                     atom_mask, idx, tab, P, R, s, dist, rbf, N, A, k);
}

extern "C" int ps_edge_frames_f32(const float* rot, const float* trans, const uint8_t* frame_mask, const int32_t* idx,
                                  float* local_pos, float* rel_rot, int B, int N, int k, void* stream) {
    if (!rot || !trans || !idx || (!local_pos && !rel_rot) || bad_batch(B, N) || k < 1 || k > PS_KNN_MAX_K)
        return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0) return 0;
    const size_t blocks = ((size_t)N * k + THREADS - 1) / THREADS;
    const unsigned gx = (unsigned)(blocks < 4096 ? blocks : 4096);
    return ps_launch(k_edge_frames, dim3(gx, (unsigned)B), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), rot,
                     trans, frame_mask, idx, local_pos, rel_rot, N, k);
}
