// K45 / K46 -- ensembles: the matrix of superposed RMSDs between the members of two batches (or of one batch with itself)
// and the clustering of such a matrix by a cutoff (Daura's "gromos" rule).  The definitions are stated in full in
// include/protstruc_ensemble.h.  Nothing here uses an atomic, and every loop has a bound that is a compile-time constant,
// a kernel argument or the number of items of a matrix.
//
// ---- K45.  Only five sums over the common points of a pair are needed -- sum x y^T, sum x, sum y, sum |x|^2, sum |y|^2 --,
// so the matrix is a GEMM-shaped double-precision product with the 3x3 solve as its epilogue.  A workgroup of 256 threads
// owns a tile of 32 x 32 pairs and walks M in chunks of 16 points.  Per chunk both sides are staged into LDS ONCE, as one
// 48-byte record per (point, structure): (x, y, z, |x|^2, m) in double about the structure's origin, zeros under the mask,
// past M and past the batch -- this is where masked coordinates are selected away -- together with one 16-bit word per
// structure of the points it counts and one of its counted points that are not finite.  Thread (tx, ty) holds the 17
// double accumulators of the 2 x 2 pairs (ty, ty + 16) x (tx, tx + 16): per point it reads four records (192 bytes) for 68
// fused multiply-adds, half the LDS traffic per FMA of one pair per lane (96 bytes for 17), which asks 0.71 of the LDS
// pipe (256 B/clk per CU) per clock of the four SIMDs' 64 fp64 FMA/clk where one pair per lane would ask 1.41.  n and
// "a counted point is not finite" are integer work on the mask words, one popcount per pair and chunk.  The next chunk's
// global loads are issued into registers before the current chunk is computed.  The epilogue runs the Jacobi solve once
// per pair and lane.  The kernel is held to 256 registers, two workgroups per CU (the second launch bound): the compiler
// then spills 14 registers of the epilogue to scratch, and B = 1024, M = 512 took 0.65 ms instead of 0.89 ms with one
// wave per SIMD and no spill, both on the square grid of an earlier build.
// Vector FMA, not the f64 MFMA: v_mfma_f64_16x16x4_f64 would compute the 5 x 5 stacked product (25 results for the 17
// that are used) and leave a pair's sums spread over several lanes and, 16 being no multiple of 5, over tile borders,
// i.e. a transpose through LDS before the solve, for a matrix pipe whose fp64 peak on this part equals the vector
// pipe's; see DESIGN.md.
// Self mode launches a 1-D grid over the tiles on and above the diagonal only, and mirrors on store.
//
// ---- K46.  Two launches.  cluster_adjacency: one lane per (item i, word w) writes the 32 bits adj(i, 32 w ..) -- from
// D[i][j] for j > i and D[j][i] for j < i, validity folded in, the diagonal clear -- into the workspace, transposed
// ([w][i]) so that the lanes of cluster_rounds, one per item, read consecutive words.  cluster_rounds: one workgroup per
// matrix; degrees in LDS; a round is an arg-max over (degree, lowest index), the centre's row ANDed with the active words
// -- the members --, and one popcount per item and NON-ZERO member word to lower the degrees: over all rounds at most
// B^2 / 32 ... B^2 word operations, however many clusters there are.
#include "ps_common.hpp"
#include "kabsch_solve.hpp"

#include <math.h>

#include "../../include/protstruc_ensemble.h"

namespace {

// ---- K45 -------------------------------------------------------------------------------------------------------------------
constexpr int RM_TILE = 32;                                  // structures per side of a tile
constexpr int RM_HALF = RM_TILE / 2;                         // a thread's two rows (columns) are RM_HALF apart
constexpr int RM_KC = 16;                                    // points per chunk: one 16-bit mask word per structure
constexpr int RM_THREADS = 256;
constexpr int RM_PER = 2 * RM_TILE * RM_KC / RM_THREADS;     // records a thread stages per chunk
constexpr int RM_SUMS = 17;                                  // Sxy[9], Sx[3], Sy[3], Qx, Qy
static_assert(RM_PER == 4 && RM_THREADS == RM_HALF * RM_HALF && RM_KC == 16, "the staging and the ballots assume these");

struct __align__(16) Rec {
    double x, y, z, q, m, pad;
};

struct RmsdTile {
    Rec rec[2][RM_KC][RM_TILE];          // [side][point of the chunk][structure of the tile]
    double origin[2][RM_TILE][3];
    uint32_t counted[2][RM_TILE];        // bit p: the structure counts point p of the chunk
    uint32_t broken[2][RM_TILE];         // bit p: ... and one of its coordinates is not finite
};

__device__ __forceinline__ void accumulate(double (&s)[RM_SUMS], const Rec& a, const Rec& b) {
    s[0] = __builtin_fma(a.x, b.x, s[0]), s[1] = __builtin_fma(a.x, b.y, s[1]), s[2] = __builtin_fma(a.x, b.z, s[2]);
    s[3] = __builtin_fma(a.y, b.x, s[3]), s[4] = __builtin_fma(a.y, b.y, s[4]), s[5] = __builtin_fma(a.y, b.z, s[5]);
    s[6] = __builtin_fma(a.z, b.x, s[6]), s[7] = __builtin_fma(a.z, b.y, s[7]), s[8] = __builtin_fma(a.z, b.z, s[8]);
    s[9] = __builtin_fma(a.x, b.m, s[9]), s[10] = __builtin_fma(a.y, b.m, s[10]), s[11] = __builtin_fma(a.z, b.m, s[11]);
    s[12] = __builtin_fma(a.m, b.x, s[12]), s[13] = __builtin_fma(a.m, b.y, s[13]), s[14] = __builtin_fma(a.m, b.z, s[14]);
    s[15] = __builtin_fma(a.q, b.m, s[15]);
    s[16] = __builtin_fma(a.m, b.q, s[16]);
}

// the RMSD of one pair from its sums; n > 0 and every counted coordinate finite
__device__ __forceinline__ float rmsd_from_sums(const double (&s)[RM_SUMS], int n) {
    const double dn = (double)n;
    double h[9], R[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) h[c * 3 + d] = s[c * 3 + d] - (s[9 + c] * s[12 + d]) / dn;
    const double gx = s[15] - ((s[9] * s[9] + s[10] * s[10]) + s[11] * s[11]) / dn;
    const double gy = s[16] - ((s[12] * s[12] + s[13] * s[13]) + s[14] * s[14]) / dn;
    ps_kabsch_solve(h, R);
    double tr = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int c = 0; c < 3; ++c) tr += R[d * 3 + c] * h[c * 3 + d];
    const double v = ((gx + gy) - 2.0 * tr) / dn;
    return (float)sqrt(v < 0.0 ? 0.0 : v);       // a NaN passes through
}

__global__ __launch_bounds__(RM_THREADS, 2) void rmsd_matrix(const float* __restrict__ a, const uint8_t* __restrict__ mask_a,
                                                          const float* __restrict__ b, const uint8_t* __restrict__ mask_b,
                                                          float* __restrict__ rmsd, int32_t* __restrict__ count, int Ba, int Bb, int M,
                                                          int self) {
    int tile_i = blockIdx.y, tile_j = blockIdx.x;
    if (self) {          // a 1-D grid over the tiles with tile_i <= tile_j: block k = tile_j (tile_j + 1) / 2 + tile_i
        const unsigned k = blockIdx.x;
        unsigned tj = (unsigned)((sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
        while ((tj + 1) * (tj + 2) / 2 <= k) ++tj;          // the square root may be one off either way
        while (tj * (tj + 1) / 2 > k) --tj;
        tile_j = (int)tj, tile_i = (int)(k - tj * (tj + 1) / 2);
    }
    __shared__ RmsdTile T;
    const int tid = threadIdx.x, lane = tid & (PS_WAVE - 1);
    const int first_of[2] = {tile_i * RM_TILE, tile_j * RM_TILE};
    auto pts = [&](int side) { return side ? b : a; };
    auto msk = [&](int side) { return side ? mask_b : mask_a; };
    auto batch = [&](int side) { return side ? Bb : Ba; };
    auto first = [&](int side) { return side ? first_of[1] : first_of[0]; };

    // ---- the origins: four lanes per structure look for its first counted point, each in its own residue class of p
    {
        const int side = tid >> 7, l = (tid >> 2) & (RM_TILE - 1), sub = tid & 3;
        const int g = first(side) + l;
        int lowest = M;
        if (g < batch(side)) {
            const uint8_t* __restrict__ m = msk(side);
            if (!m) {
                lowest = sub == 0 ? 0 : M;
            } else {
                const uint8_t* __restrict__ row = m + (size_t)g * (size_t)M;
                for (int p = sub; p < M; p += 4)
                    if (row[p]) {
                        lowest = p;
                        break;
                    }
            }
        }
        lowest = min(lowest, __shfl_xor(lowest, 1));
        lowest = min(lowest, __shfl_xor(lowest, 2));
        if (sub < 3)
            T.origin[side][l][sub] = lowest < M ? (double)pts(side)[((size_t)g * (size_t)M + (size_t)lowest) * 3 + sub] : 0.0;
    }

    // ---- staging: record r = k * 256 + tid is (side r / 512 = k / 2, structure (r % 512) / 16, point r % 16)
    float px[RM_PER], py[RM_PER], pz[RM_PER];
    bool pm[RM_PER];
    auto fetch = [&](int p0) {
#pragma unroll
        for (int k = 0; k < RM_PER; ++k) {
            const int r = k * RM_THREADS + tid, side = k >> 1, l = (r >> 4) & (RM_TILE - 1), p = p0 + (r & (RM_KC - 1));
            const int g = first(side) + l;
            bool on = g < batch(side) && p < M;
            const size_t at = (size_t)g * (size_t)M + (size_t)p;
            if (on && msk(side)) on = msk(side)[at] != 0;
            px[k] = py[k] = pz[k] = 0.0f;
            if (on) px[k] = pts(side)[at * 3], py[k] = pts(side)[at * 3 + 1], pz[k] = pts(side)[at * 3 + 2];
            pm[k] = on;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int k = 0; k < RM_PER; ++k) {
            const int r = k * RM_THREADS + tid, side = k >> 1, l = (r >> 4) & (RM_TILE - 1), p = r & (RM_KC - 1);
            const bool finite = fabsf(px[k]) <= 3.4028234663852886e38f && fabsf(py[k]) <= 3.4028234663852886e38f &&
                                fabsf(pz[k]) <= 3.4028234663852886e38f;
            const bool use = pm[k] && finite;
            Rec rec = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (use) {
                rec.x = (double)px[k] - T.origin[side][l][0];
                rec.y = (double)py[k] - T.origin[side][l][1];
                rec.z = (double)pz[k] - T.origin[side][l][2];
                rec.q = (rec.x * rec.x + rec.y * rec.y) + rec.z * rec.z;
                rec.m = 1.0;
            }
            T.rec[side][p][l] = rec;
            const unsigned long long counted = __ballot(pm[k]), broken = __ballot(pm[k] && !finite);
            if ((lane & (RM_KC - 1)) == 0) {
                T.counted[side][l] = (uint32_t)(counted >> (lane & 48)) & 0xffffu;
                T.broken[side][l] = (uint32_t)(broken >> (lane & 48)) & 0xffffu;
            }
        }
    };

    const int tx = tid & (RM_HALF - 1), ty = tid >> 4;
    double acc[4][RM_SUMS];
    int n[4] = {0, 0, 0, 0};
    uint32_t bad[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < RM_SUMS; ++k) acc[q][k] = 0.0;

    fetch(0);
    for (int p0 = 0; p0 < M; p0 += RM_KC) {
        __syncthreads();            // the origins are written; the readers of the chunk before are done
        stage();
        __syncthreads();
        if (p0 + RM_KC < M) fetch(p0 + RM_KC);       // in flight while this chunk is computed
#pragma unroll 2
        for (int p = 0; p < RM_KC; ++p) {
            const Rec a0 = T.rec[0][p][ty], a1 = T.rec[0][p][ty + RM_HALF];
            const Rec b0 = T.rec[1][p][tx], b1 = T.rec[1][p][tx + RM_HALF];
            accumulate(acc[0], a0, b0);
            accumulate(acc[1], a0, b1);
            accumulate(acc[2], a1, b0);
            accumulate(acc[3], a1, b1);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int li = ty + RM_HALF * (q >> 1), lj = tx + RM_HALF * (q & 1);
            const uint32_t ca = T.counted[0][li], cb = T.counted[1][lj];
            n[q] += __popc(ca & cb);
            bad[q] |= (T.broken[0][li] & cb) | (ca & T.broken[1][lj]);
        }
    }

    // ---- the epilogue: one solve per pair, the four pairs of a lane one after the other through one copy of the code
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        const int i = first_of[0] + ty + RM_HALF * (q >> 1), j = first_of[1] + tx + RM_HALF * (q & 1);
        if (i >= Ba || j >= Bb || (self && i > j)) continue;
        double s[RM_SUMS];
#pragma unroll
        for (int k = 0; k < RM_SUMS; ++k) s[k] = q == 0 ? acc[0][k] : (q == 1 ? acc[1][k] : (q == 2 ? acc[2][k] : acc[3][k]));
        const int nq = q == 0 ? n[0] : (q == 1 ? n[1] : (q == 2 ? n[2] : n[3]));
        const uint32_t broken = q == 0 ? bad[0] : (q == 1 ? bad[1] : (q == 2 ? bad[2] : bad[3]));
        float out;
        if (nq == 0 || broken) out = NAN;
        else if (self && i == j) out = 0.0f;
        else out = rmsd_from_sums(s, nq);
        const size_t at = (size_t)i * (size_t)Bb + (size_t)j;
        rmsd[at] = out;
        if (count) count[at] = nq;
        if (self && i != j) {
            const size_t mirror = (size_t)j * (size_t)Bb + (size_t)i;
            rmsd[mirror] = out;
            if (count) count[mirror] = nq;
        }
    }
}

// ---- K46 -------------------------------------------------------------------------------------------------------------------
constexpr int CL_MAX_WORDS = PS_CLUSTER_MAX_ITEMS / 32;
constexpr int CL_MAX_WAVES = 16;

__global__ __launch_bounds__(PS_WAVE) void cluster_adjacency(const float* __restrict__ D, const uint8_t* __restrict__ valid, float cutoff,
                                                             uint32_t* __restrict__ adj, int B, int W) {
    const int i = (int)blockIdx.x * PS_WAVE + (int)threadIdx.x, w = blockIdx.y;
    if (i >= B) return;
    const size_t g = blockIdx.z;
    const float* __restrict__ Dg = D + g * (size_t)B * (size_t)B;
    const uint8_t* __restrict__ vg = valid ? valid + g * (size_t)B : nullptr;
    uint32_t word = 0;
    if (!vg || vg[i]) {
        for (int bit = 0; bit < 32; ++bit) {
            const int j = w * 32 + bit;
            if (j >= B) break;
            if (j == i || (vg && !vg[j])) continue;
            const float d = j > i ? Dg[(size_t)i * (size_t)B + (size_t)j] : Dg[(size_t)j * (size_t)B + (size_t)i];
            if (d <= cutoff) word |= 1u << bit;
        }
    }
    adj[(g * (size_t)W + (size_t)w) * (size_t)B + (size_t)i] = word;
}

__global__ __launch_bounds__(1024) void cluster_rounds(const uint32_t* __restrict__ adj, const uint8_t* __restrict__ valid,
                                                       int32_t* __restrict__ label, int32_t* __restrict__ center, int32_t* __restrict__ size,
                                                       int32_t* __restrict__ n_clusters, int B, int W) {
    __shared__ int deg[PS_CLUSTER_MAX_ITEMS];        // -1: not active
    __shared__ uint32_t removed[CL_MAX_WORDS];
    __shared__ int nonzero[CL_MAX_WORDS];
    __shared__ int n_nonzero;
    __shared__ int wave_best[CL_MAX_WAVES];
    const int tid = threadIdx.x, lane = tid & (PS_WAVE - 1), wave = tid / PS_WAVE, T = blockDim.x, waves = T / PS_WAVE;
    const size_t g = blockIdx.x;
    const uint32_t* __restrict__ A = adj + g * (size_t)W * (size_t)B;       // [w][i]
    const uint8_t* __restrict__ vg = valid ? valid + g * (size_t)B : nullptr;
    int32_t* __restrict__ lab = label + g * (size_t)B;
    int32_t* __restrict__ cen = center + g * (size_t)B;
    int32_t* __restrict__ siz = size + g * (size_t)B;
    for (int i = tid; i < B; i += T) {
        lab[i] = -1, cen[i] = -1, siz[i] = 0;
        int d = -1;
        if (!vg || vg[i]) {          // the rows hold valid partners only, and all of them are active now
            d = 0;
            for (int w = 0; w < W; ++w) d += __popc(A[(size_t)w * (size_t)B + (size_t)i]);
        }
        deg[i] = d;
    }
    __syncthreads();
    int c = 0;
    for (;; ++c) {          // at most B rounds: every round removes its centre
        int key = -1;
        for (int i = tid; i < B; i += T)
            if (deg[i] >= 0) key = max(key, deg[i] * PS_CLUSTER_MAX_ITEMS + (PS_CLUSTER_MAX_ITEMS - 1 - i));
#pragma unroll
        for (int d = PS_WAVE / 2; d > 0; d >>= 1) key = max(key, __shfl_xor(key, d));
        if (lane == 0) wave_best[wave] = key;
        __syncthreads();
        int best = -1;
        for (int k = 0; k < waves; ++k) best = max(best, wave_best[k]);
        if (best < 0) break;          // the same value in every thread
        const int centre = PS_CLUSTER_MAX_ITEMS - 1 - (best & (PS_CLUSTER_MAX_ITEMS - 1)), members = (best >> 12) + 1;
        // the members: the centre's row among the active items, and the centre
        for (int w = tid; w < W; w += T) {
            uint32_t word = A[(size_t)w * (size_t)B + (size_t)centre];
            uint32_t kept = 0;
            for (uint32_t rest = word; rest; rest &= rest - 1) {
                const int bit = __ffs(rest) - 1;
                if (deg[w * 32 + bit] >= 0) kept |= 1u << bit;
            }
            if (w == (centre >> 5)) kept |= 1u << (centre & 31);
            removed[w] = kept;
            for (uint32_t rest = kept; rest; rest &= rest - 1) lab[w * 32 + __ffs(rest) - 1] = c;
        }
        if (tid == 0) cen[c] = centre, siz[c] = members;
        __syncthreads();
        if (wave == 0) {          // the words that hold a member, in order
            int base = 0;
            for (int w0 = 0; w0 < W; w0 += PS_WAVE) {
                const int w = w0 + lane;
                const bool holds = w < W && removed[w] != 0;
                const unsigned long long votes = __ballot(holds);
                if (holds) nonzero[base + __popcll(votes & ((1ull << lane) - 1ull))] = w;
                base += __popcll(votes);
            }
            if (lane == 0) n_nonzero = base;
        }
        __syncthreads();
        const int words = n_nonzero;
        for (int i = tid; i < B; i += T) {
            if (deg[i] < 0) continue;
            if ((removed[i >> 5] >> (i & 31)) & 1u) {
                deg[i] = -1;
                continue;
            }
            int lost = 0;
            for (int k = 0; k < words; ++k) {
                const int w = nonzero[k];
                lost += __popc(A[(size_t)w * (size_t)B + (size_t)i] & removed[w]);
            }
            deg[i] -= lost;
        }
        __syncthreads();
    }
    if (tid == 0) n_clusters[g] = c;
}

bool bad_cluster(int G, int B) { return G < 0 || G > 65535 || B < 1 || B > PS_CLUSTER_MAX_ITEMS; }

}  // namespace

extern "C" int ps_ensemble_api(void) { return PS_ENSEMBLE_API; }

extern "C" int ps_rmsd_matrix_f32(const float* a, const uint8_t* mask_a, const float* b, const uint8_t* mask_b, float* rmsd,
                                  int32_t* count, int Ba, int Bb, int M, void* stream) {
    if (Ba < 0 || Ba > 65535 || Bb < 0 || Bb > 65535 || M < 1 || M > PS_RMSD_MATRIX_MAX_POINTS) return (int)hipErrorInvalidValue;
    const bool self = b == nullptr;
    if (self && (Bb != Ba || mask_b)) return (int)hipErrorInvalidValue;
    if (Ba == 0 || Bb == 0) return 0;
    if (!a || !rmsd) return (int)hipErrorInvalidValue;
    const unsigned tiles_a = (unsigned)((Ba + RM_TILE - 1) / RM_TILE), tiles_b = (unsigned)((Bb + RM_TILE - 1) / RM_TILE);
    const dim3 grid = self ? dim3(tiles_a * (tiles_a + 1) / 2) : dim3(tiles_b, tiles_a);
    return ps_launch(rmsd_matrix, grid, dim3(RM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a, mask_a, self ? a : b,
                     self ? mask_a : mask_b, rmsd, count, Ba, Bb, M, self ? 1 : 0);
}

extern "C" long long ps_cluster_workspace_bytes(int G, int B) {
    if (bad_cluster(G, B)) return -1;
    return (long long)G * B * ((B + 31) / 32) * 4;
}

extern "C" int ps_cluster_f32(const float* D, const uint8_t* valid, float cutoff, void* workspace, int32_t* label, int32_t* center,
                              int32_t* size, int32_t* n_clusters, int G, int B, void* stream) {
    if (bad_cluster(G, B) || !(fabsf(cutoff) <= 3.4028234663852886e38f)) return (int)hipErrorInvalidValue;
    if (G == 0) return 0;
    if (!D || !workspace || !label || !center || !size || !n_clusters) return (int)hipErrorInvalidValue;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int W = (B + 31) / 32;
    uint32_t* adj = static_cast<uint32_t*>(workspace);
    const int rc = ps_launch(cluster_adjacency, dim3((unsigned)((B + PS_WAVE - 1) / PS_WAVE), (unsigned)W, (unsigned)G), dim3(PS_WAVE), 0, s, D,
                             valid, cutoff, adj, B, W);
    if (rc) return rc;
    const int threads = B <= 64 ? 64 : (B <= 256 ? 256 : 1024);
    return ps_launch(cluster_rounds, dim3((unsigned)G), dim3((unsigned)threads), 0, s, adj, valid, label, center, size, n_clusters, B, W);
}
