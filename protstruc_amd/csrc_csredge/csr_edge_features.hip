// K49 - K51 -- edge features on a CSR graph: K25 / K26 (csrc/edge_features.hip) on lists of any length.  The definitions
// are in include/protstruc_csredge.h; this file restates the arithmetic of K25 / K26 so that the same edge gets the same bits.
//
// Every kernel finds the row of an edge position p by bisection over row_ptr[1 .. n_rows]:
//   r(p) = the number of t in 1 .. n_rows with row_ptr[t] <= p
// `lo` and `hi` start at 0 and n_rows and only ever move towards each other, so the result lies in [0, n_rows] whatever
// row_ptr holds, and every index read is in [1, n_rows].  r(p) == n_rows marks the tail of the buffers.
//
// K50, ps_csr_edge_rbf_f32, is a streaming-store kernel like K25, but its unit of work is a CHUNK of PS_CSREDGE_CHUNK
// consecutive edge positions, whatever rows they fall in -- rows have any length, zero included, so cutting by source
// would balance nothing.  A workgroup takes chunks blockIdx.x, + gridDim.x, ...  Per chunk: (1) the first 64 lanes find
// their position's row (one bisection each, side by side: the upper levels are the same addresses for every chunk and stay
// in cache) and split it into (b, q) -- the only divisions, once per position --, and read col, range-checked; (2) the
// 64 * P distances are computed once, one per thread and round, into LDS (at most 64 * 64 * 4 = 16 KB; a negative value
// marks padding or a masked pair), and written to `dist` from there; (3) all lanes stream the chunk's n * P * R floats out,
// each lane four consecutive floats per round as one 16-byte store, consecutive lanes on consecutive 16 bytes.  The output
// base is only 4-byte aligned and a chunk's length need not be a multiple of 4, so the up to three floats before the first
// 16-byte boundary of the chunk's ACTUAL address and the up to three after the last whole 16 bytes are single stores:
// nothing outside the chunk is touched, every float of it is written once, and chunks tile [0, E * P * R).  A lane's walk
// over (pair, centre) takes no division inside the loop: element e = q * R + c is split once per chunk and then advanced
// by the constant (1024 / R, 1024 % R) per round and by one per float.
//
// All output offsets are 64-bit: size_t products of factors that are widened before they are multiplied.  A chunk's own
// length 64 * P * R <= 2^18 stays an int.
#include "ps_common.hpp"

#include <math.h>

#include "../../include/protstruc_csredge.h"

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = PS_CSREDGE_CHUNK;
constexpr int FLOATS_PER_ROUND = 4 * THREADS;   // what the workgroup streams out per round

static_assert(CHUNK <= THREADS, "one lane per position of a chunk");

// The host arrays of the call, by value in the kernel's arguments: read on the host before the call returns.
struct RbfTables {
    int pair_i[PS_CSREDGE_MAX_PAIRS];
    int pair_j[PS_CSREDGE_MAX_PAIRS];
    float centers[PS_CSREDGE_MAX_RBF];
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

__global__ __launch_bounds__(THREADS) void k_csr_edge_rows(const long long* __restrict__ row_ptr, long long n_rows, int Q,
                                                           long long E, int* __restrict__ batch, int* __restrict__ row) {
    for (long long p = (long long)blockIdx.x * THREADS + threadIdx.x; p < E; p += (long long)gridDim.x * THREADS) {
        const long long r = row_of(row_ptr, n_rows, p);
        int b = -1, q = -1;
        if (r < n_rows) {
            b = (int)(r / Q);
            q = (int)(r - (long long)b * Q);
        }
        batch[p] = b;
        row[p] = q;
    }
}

// d < 0 marks padding or a masked pair (a NaN distance compares false and propagates)
__device__ __forceinline__ float rbf_value(float d, float mu, float s) {
    const float w = (d - mu) * s;
    return d < 0.0f ? 0.0f : __builtin_amdgcn_exp2f(-(w * w));
}

__global__ __launch_bounds__(THREADS) void k_csr_edge_rbf(const float* __restrict__ xyz, const uint8_t* __restrict__ atom_mask,
                                                          const float* __restrict__ src_xyz,
                                                          const uint8_t* __restrict__ src_mask,
                                                          const long long* __restrict__ row_ptr, const int* __restrict__ col,
                                                          long long E, long long n_rows, const RbfTables tab, int P, int R,
                                                          float s, float* __restrict__ dist, float* __restrict__ rbf, int M,
                                                          int A, int Q, int As) {
    __shared__ int nbr[CHUNK];                  // the target of every position of the chunk, -1: padding
    __shared__ int src_b[CHUNK], src_q[CHUNK];  // its source, (b, q)
    __shared__ int slot_i[PS_CSREDGE_MAX_PAIRS], slot_j[PS_CSREDGE_MAX_PAIRS];
    __shared__ float centre[PS_CSREDGE_MAX_RBF];
    __shared__ float dl[CHUNK * PS_CSREDGE_MAX_PAIRS];   // [position][pair]
    const int t = threadIdx.x;
    if (t < P) {
        slot_i[t] = tab.pair_i[t];
        slot_j[t] = tab.pair_j[t];
    }
    if (t < R) centre[t] = tab.centers[t];
    const int PR = P * R;
    const int dq = FLOATS_PER_ROUND / R, dc = FLOATS_PER_ROUND - dq * R;
    const long long chunks = (E + CHUNK - 1) / CHUNK;

    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const long long p0 = chunk * CHUNK;
        const int n = E - p0 < CHUNK ? (int)(E - p0) : CHUNK;   // the last chunk may be short
        // (1) rows and targets; anything outside [0, M) and anything past the last row is padding.  The barrier also orders
        // the tables above and, from the second chunk on, the last reads of `dl` before its next writes.
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
        // (2) the distances, once
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
                }
            }
            dl[e] = d;
            if (dist) dist[(size_t)p0 * (size_t)P + (size_t)e] = d < 0.0f ? 0.0f : d;
        }
        __syncthreads();
        if (!rbf) continue;
        // (3) the chunk's L floats
        const int L = NP * R;
        float* __restrict__ out = rbf + (size_t)p0 * (size_t)PR;
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
            *reinterpret_cast<f32x4_t*>(out + head + 4 * (size_t)v) = x;
            q += dq;
            c += dc;
            if (c >= R) {
                c -= R;
                ++q;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_csr_edge_frames(const float* __restrict__ rot, const float* __restrict__ trans,
                                                             const uint8_t* __restrict__ frame_mask,
                                                             const float* __restrict__ src_rot,
                                                             const float* __restrict__ src_trans,
                                                             const uint8_t* __restrict__ src_mask,
                                                             const long long* __restrict__ row_ptr,
                                                             const int* __restrict__ col, long long E, long long n_rows,
                                                             float* __restrict__ local_pos, float* __restrict__ rel_rot, int M,
                                                             int Q) {
    for (long long p = (long long)blockIdx.x * THREADS + threadIdx.x; p < E; p += (long long)gridDim.x * THREADS) {
        const long long r = row_of(row_ptr, n_rows, p);
        bool real = r < n_rows;
        size_t fi = 0, fj = 0;
        if (real) {
            const int j = col[p];
            real = (unsigned)j < (unsigned)M;
            if (real) {
                fi = (size_t)r;   // b * Q + q: the sources are the rows
                fj = (size_t)(r / Q) * (size_t)M + (size_t)j;
                real = (!src_mask || src_mask[fi] != 0) && (!frame_mask || frame_mask[fj] != 0);
            }
        }
        float pos[3] = {0.0f, 0.0f, 0.0f};
        float rr[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (real) {
            double Ri[9];
            for (int m = 0; m < 9; ++m) Ri[m] = (double)src_rot[fi * 9 + m];
            if (local_pos) {
                const double v0 = (double)trans[fj * 3] - (double)src_trans[fi * 3],
                             v1 = (double)trans[fj * 3 + 1] - (double)src_trans[fi * 3 + 1],
                             v2 = (double)trans[fj * 3 + 2] - (double)src_trans[fi * 3 + 2];
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
        const size_t at = (size_t)p;
        if (local_pos)
            for (int c = 0; c < 3; ++c) local_pos[at * 3 + c] = pos[c];
        if (rel_rot)
            for (int m = 0; m < 9; ++m) rel_rot[at * 9 + m] = rr[m];
    }
}

bool bad_sizes(int B, int M, int Q, long long E) {
    return B < 0 || B > 65535 || M < 0 || M > (1 << 24) || Q < 0 || Q > (1 << 24) || E < 0;
}

unsigned grid_for(long long items, long long cap) { return (unsigned)(items < cap ? items : cap); }

}  // namespace

extern "C" int ps_csredge_api(void) { return PS_CSREDGE_API; }

extern "C" int ps_csr_edge_rows_i32(const long long* row_ptr, long long n_rows, int Q, long long E, int32_t* batch,
                                    int32_t* row, void* stream) {
    if (!row_ptr || !batch || !row || Q < 0 || Q > (1 << 24) || n_rows < 0 || E < 0) return (int)hipErrorInvalidValue;
    if (Q == 0 ? n_rows != 0 : (n_rows % Q != 0 || n_rows / Q > 65535)) return (int)hipErrorInvalidValue;
    if (E == 0) return 0;
    const long long blocks = (E + THREADS - 1) / THREADS;
    return ps_launch(k_csr_edge_rows, dim3(grid_for(blocks, 65536)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     row_ptr, n_rows, Q, E, batch, row);
}

extern "C" int ps_csr_edge_rbf_f32(const float* xyz, const uint8_t* atom_mask, const float* src_xyz, const uint8_t* src_mask,
                                   const long long* row_ptr, const int32_t* col, long long E, const int32_t* pair_i,
                                   const int32_t* pair_j, int P, const float* centers, int R, float sigma, float* dist,
                                   float* rbf, int B, int M, int A, int Q, int As, void* stream) {
    if (!xyz || !row_ptr || !col || !pair_i || !pair_j || !centers || (!dist && !rbf) || bad_sizes(B, M, Q, E) || A < 1 ||
        As < 1 || P < 1 || P > PS_CSREDGE_MAX_PAIRS || R < 1 || R > PS_CSREDGE_MAX_RBF || !(sigma > 0.0f))
        return (int)hipErrorInvalidValue;
    if (!src_xyz) {   // the sources are the targets
        if (Q != M || As != A || src_mask) return (int)hipErrorInvalidValue;
        src_xyz = xyz;
        src_mask = atom_mask;
    }
    const float s = (float)(sqrt(1.4426950408889634) / (double)sigma);   // sqrt(log2 e) / sigma: exp(-z^2) = exp2(-(s (d - mu))^2)
    if (!(s > 0.0f && s < INFINITY)) return (int)hipErrorInvalidValue;    // sigma infinite, or too small for fp32
    RbfTables tab = {};
    for (int p = 0; p < P; ++p) {
        if (pair_i[p] < 0 || pair_i[p] >= As || pair_j[p] < 0 || pair_j[p] >= A) return (int)hipErrorInvalidValue;
        tab.pair_i[p] = pair_i[p];
        tab.pair_j[p] = pair_j[p];
    }
    for (int c = 0; c < R; ++c) tab.centers[c] = centers[c];
    if (B == 0 || E == 0) return 0;
    // a workgroup walks chunks c, c + grid, ...: enough workgroups to fill any device, few enough to amortise the tables
    const long long chunks = (E + CHUNK - 1) / CHUNK;
    return ps_launch(k_csr_edge_rbf, dim3(grid_for(chunks, 8192)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz,
                     atom_mask, src_xyz, src_mask, row_ptr, col, E, (long long)B * Q, tab, P, R, s, dist, rbf, M, A, Q, As);
}

extern "C" int ps_csr_edge_frames_f32(const float* rot, const float* trans, const uint8_t* frame_mask, const float* src_rot,
                                      const float* src_trans, const uint8_t* src_mask, const long long* row_ptr,
                                      const int32_t* col, long long E, float* local_pos, float* rel_rot, int B, int M, int Q,
                                      void* stream) {
    if (!rot || !trans || !row_ptr || !col || (!local_pos && !rel_rot) || bad_sizes(B, M, Q, E) || (!src_rot) != (!src_trans))
        return (int)hipErrorInvalidValue;
    if (!src_rot) {   // the sources are the targets
        if (Q != M || src_mask) return (int)hipErrorInvalidValue;
        src_rot = rot;
        src_trans = trans;
        src_mask = frame_mask;
    }
    if (B == 0 || E == 0) return 0;
    const long long blocks = (E + THREADS - 1) / THREADS;
    return ps_launch(k_csr_edge_frames, dim3(grid_for(blocks, 65536)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     rot, trans, frame_mask, src_rot, src_trans, src_mask, row_ptr, col, E, (long long)B * Q, local_pos, rel_rot,
                     M, Q);
}
