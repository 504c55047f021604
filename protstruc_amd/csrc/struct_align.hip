// K41 - K44 -- structure alignment without a given correspondence: a Needleman-Wunsch pass with TM-align's gap rule (K41),
// the alignment that alternates it with the seeded superposition search (K42) and the pick between its two starts (K43),
// and TM-align's secondary structure of a CA trace (K44).  The definitions are stated in full in
// include/protstruc_structalign.h; the build's -ffp-contract=off is part of them.  All arithmetic is double on the float32
// inputs, the chains are K39's own code (superpose_chain.hpp), nothing here uses an atomic or waits on another wave other
// than at a workgroup barrier, and every loop has a bound that is a compile-time constant or a kernel argument.
//
// ---- The DP (nw_pass), one workgroup of four waves.  A wave sweeps a strip of 64 rows, lane l owning row 64 strip + l + 1,
// along anti-diagonals: in step t of the strip lane l computes column t - l + 1.  What a cell needs from the row above --
// val[i-1][j], path[i-1][j] -- is what the lane above computed one step earlier and comes across lanes (a DPP wave shift);
// val[i-1][j-1] is what came a step before that, and val[i][j-1] is the lane's own last result: the DP front lives in
// registers.  The first lane of a strip reads the strip above's last row from LDS, where the last lane of that strip's wave
// wrote it (SA_WAVES rows of Mb + 1 doubles and path bytes: the "front").  Time is cut into supersteps of 64 steps with a
// workgroup barrier between them; in superstep T wave w works on item q = T - 2 w of its sequence of (strip, chunk of 64
// steps): strip w of round 0 from its first chunk to its last, then strip w + SA_WAVES, ...  A strip's chunk c reads columns
// 64 c + 1 .. 64 c + 64 of the row above, which that row's wave finished writing in ITS chunk c + 1, one superstep earlier at
// the latest because it runs two items ahead; a round is never shorter than 2 SA_WAVES items, so that wave 0 finds the last
// wave's row of the round before complete and that no wave overwrites a column of its row that is still to be read.  The
// score of a cell is computed where it is needed (a functor: the caller's matrix, equal labels, or the TM term of the staged
// coordinates under a transform); no score matrix of a refinement pass exists anywhere.
// A lane collects two bits per cell, path[i][j] and [v >= h], into one 64-bit word each per chunk; the trace back reads them
// and needs no value of the table.  The words live in LDS while Ma * ceil((Mb + 63) / 64) * 16 bytes fit beside the rest,
// and in the caller's workspace otherwise; the choice depends on (Ma, Mb) alone and changes no result.
//
// ---- K42, one workgroup per (pair of structures, start).  Both structures' unmasked points are compacted into LDS planes;
// start 0 is the threading (one offset per wave at a time), start 1 the DP over equal secondary-structure labels.  The
// fit-search runs its at most five chains on the four waves, each a chain of K39 over the pairs of the current map, and the
// refinement alternates DP and fit-search as the header defines, every decision taken from values all threads hold alike.
// The start's best (S, R, t, the map) goes to the workspace; K43, one wave per pair, picks between the two starts.
#include "superpose_chain.hpp"

#include "../../include/protstruc_structalign.h"

namespace {

using namespace ps_chain;

constexpr int SA_WAVES = 4;
constexpr int SA_THREADS = PS_WAVE * SA_WAVES;
constexpr int SA_LDS_MAX = 160 * 1024 - 256;
constexpr int SA_ENTRY_BYTES = 128;       // a start's result in the workspace: S, R, t, n_aligned, n_a, n_b

// ---- the layout of the dynamic LDS and of the workspace, for the host and the device alike -------------------------------------
struct Layout {
    int front_val, chain, bits, planes_a, planes_b, slot_a, slot_b, map_start, map_prev, map_cur, map_best, pair_a, pair_b,
        front_path, label_a, label_b, ints, total;
    int words;               // 64-step chunks that cover a row of the DP: path words per row
    int pairs;               // min(Ma, Mb): the most pairs a map has
    int bits_in_lds;
    long long bits_bytes;    // the path words of one DP
    long long unit_bytes;    // the workspace of one (pair, start)
};

PS_HOST_DEVICE inline int up16(int x) { return (x + 15) & ~15; }

PS_HOST_DEVICE inline Layout make_layout(int Ma, int Mb) {
    Layout L;
    L.words = (Mb + 126) >> 6;
    L.pairs = Ma < Mb ? Ma : Mb;
    L.bits_bytes = (long long)Ma * L.words * 16;
    int at = 0;
    L.front_val = at, at += up16(SA_WAVES * (Mb + 1) * 8);
    L.chain = at, at += SA_WAVES * 16 * 8;
    L.planes_a = at, at += up16(3 * Ma * 4);
    L.planes_b = at, at += up16(3 * Mb * 4);
    L.slot_a = at, at += up16(Ma * 2);
    L.slot_b = at, at += up16(Mb * 2);
    L.map_start = at, at += up16(Ma * 2);
    L.map_prev = at, at += up16(Ma * 2);
    L.map_cur = at, at += up16(Ma * 2);
    L.map_best = at, at += up16(Ma * 2);
    L.pair_a = at, at += up16(L.pairs * 2);
    L.pair_b = at, at += up16(L.pairs * 2);
    L.front_path = at, at += up16(SA_WAVES * (Mb + 1));
    L.label_a = at, at += up16(Ma);
    L.label_b = at, at += up16(Mb);
    L.ints = at, at += 64;
    L.bits = at;
    L.bits_in_lds = at + L.bits_bytes <= SA_LDS_MAX ? 1 : 0;
    L.total = L.bits_in_lds ? at + (int)L.bits_bytes : at;
    L.unit_bytes = SA_ENTRY_BYTES + (long long)((Ma * 4 + 7) & ~7) + (L.bits_in_lds ? 0 : L.bits_bytes);
    return L;
}

struct Entry {      // SA_ENTRY_BYTES at most
    double S;
    float R[9], t[3];
    int n_aligned, n_a, n_b;
};
static_assert(sizeof(Entry) <= SA_ENTRY_BYTES, "the entry outgrew its slot");

// ---- compaction ------------------------------------------------------------------------------------------------------------
// the unmasked slots of mask[M] (NULL: all), in order, into slots[]; returns their number, the same in every thread.
// M <= 4 SA_THREADS.  `totals` are SA_WAVES ints of LDS; ends with a barrier.
__device__ __forceinline__ int compact_slots(const uint8_t* __restrict__ mask, int M, int16_t* slots, int* totals) {
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int per = (M + SA_THREADS - 1) / SA_THREADS;
    const int begin = (int)threadIdx.x * per;
    int mine = 0;
    for (int q = 0; q < per; ++q) {
        const int i = begin + q;
        if (i < M && (!mask || mask[i])) ++mine;
    }
    int upto = mine;                                          // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < PS_WAVE; d <<= 1) {
        const int below = __shfl_up(upto, d);
        if (lane >= d) upto += below;
    }
    if (lane == PS_WAVE - 1) totals[wave] = upto;
    __syncthreads();
    int at = upto - mine, n = 0;
#pragma unroll
    for (int k = 0; k < SA_WAVES; ++k) {
        const int total = totals[k];
        at += k < wave ? total : 0;
        n += total;
    }
    for (int q = 0; q < per; ++q) {
        const int i = begin + q;
        if (i < M && (!mask || mask[i])) slots[at++] = (int16_t)i;
    }
    __syncthreads();
    return n;
}

// the n points at `slots` of x[M][3] into three planes of `stride` floats
__device__ __forceinline__ void stage_points(const float* __restrict__ x, const int16_t* slots, int n, float* planes, int stride) {
    for (int k = threadIdx.x; k < n; k += SA_THREADS) {
        const size_t i = (size_t)slots[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) planes[c * stride + k] = x[i * 3 + c];
    }
}

// ---- the DP ----------------------------------------------------------------------------------------------------------------
constexpr int SA_HALF = 32;         // steps whose scores are formed ahead of the steps themselves; 2 SA_HALF = a chunk

// the value of the lane above (lane 0: its own), by a data-parallel move within the wave: wave_shr:1
__device__ __forceinline__ int from_lane_above(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ double from_lane_above(double v) {
    return __hiloint2double(from_lane_above(__double2hiint(v)), from_lane_above(__double2loint(v)));
}

// the value lane `k` holds, in every lane; k is a constant
__device__ __forceinline__ double read_lane(double v, int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

struct Front {
    double* val;        // [SA_WAVES][stride]: the last row of the strip each wave is on (or was last on)
    uint8_t* path;
    int stride;         // Mb + 1
};

// One pass over n_a x n_b cells, n_a, n_b >= 1: the path words into bits[n_a][words][2] and val[n_a][n_b] into *final_val.
// Called by the whole workgroup; ends with a barrier.
template <class F>
__device__ __forceinline__ void nw_pass(const F& f, int na, int nb, double gap, const Front& fr, uint64_t* bits, int words,
                                        double* final_val) {
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int chunks = (nb + 126) >> 6;                                    // the last lane reaches column n_b in step n_b + 62
    const int per_round = chunks > 2 * SA_WAVES ? chunks : 2 * SA_WAVES;
    const int strips = (na + PS_WAVE - 1) / PS_WAVE, rounds = (strips + SA_WAVES - 1) / SA_WAVES;
    const int items = rounds * per_round, supersteps = items + 2 * (SA_WAVES - 1);
    const int above = (wave + SA_WAVES - 1) % SA_WAVES;
    if (lane == 0) fr.val[wave * fr.stride] = 0.0, fr.path[wave * fr.stride] = 0;      // column 0 of every row
    __syncthreads();
    int i = 0;
    double cur_v = 0.0, diag_v = 0.0;
    int cur_p = 0;
    typename F::Row row = {};
    for (int T = 0; T < supersteps; ++T) {
        const int q = T - 2 * wave;
        if (q >= 0 && q < items) {                  // wave-uniform
            const int round = q / per_round, c = q - round * per_round, strip = round * SA_WAVES + wave;
            if (strip < strips && c < chunks) {
                if (c == 0) {
                    i = strip * PS_WAVE + lane + 1;
                    cur_v = 0.0, cur_p = 0, diag_v = 0.0;       // val[i][0], path[i][0], val[i-1][0]
                    if (i <= na) row = f.row(i - 1);
                }
                uint64_t path_word = 0, side_word = 0;
#pragma unroll 1
                for (int half = 0; half < 2; ++half) {
                    const int j0 = c * PS_WAVE + half * SA_HALF - lane + 1;          // the lane's column in step 0 of this half
                    // what does not depend on the table first, SA_HALF steps at a time, so that it is not on the steps'
                    // critical path: the cells' scores, and the row above the strip for lane 0 -- lane k loads the column
                    // lane 0 needs in step k, which then comes from a read of that lane
                    double score[SA_HALF];
#pragma unroll
                    for (int k = 0; k < SA_HALF; ++k) {
                        const int j = j0 + k;
                        score[k] = (i <= na && j >= 1 && j <= nb) ? f.cell(row, j - 1) : 0.0;
                    }
                    const int front_j = c * PS_WAVE + half * SA_HALF + 1 + lane;
                    const bool stored = strip > 0 && lane < SA_HALF && front_j <= nb;
                    const double front_v = stored ? fr.val[above * fr.stride + front_j] : 0.0;
                    const int front_p = stored ? (int)fr.path[above * fr.stride + front_j] : 0;
                    uint32_t path_bits = 0, side_bits = 0;
#pragma unroll
                    for (int k = 0; k < SA_HALF; ++k) {
                        const int j = j0 + k;
                        double up_v = from_lane_above(cur_v);       // val[i-1][j] and path[i-1][j]: the lane above, one step ago
                        int up_p = from_lane_above(cur_p);
                        const double first_v = read_lane(front_v, k);
                        const int first_p = __builtin_amdgcn_readlane(front_p, k);
                        if (lane == 0) up_v = first_v, up_p = first_p;
                        if (i <= na && j >= 1 && j <= nb) {
                            const double d = diag_v + score[k];
                            const double h = up_v + (up_p ? gap : 0.0);
                            const double v = cur_v + (cur_p ? gap : 0.0);
                            const bool p = d >= h && d >= v, sideways = v >= h;
                            cur_v = p ? d : (sideways ? v : h);
                            cur_p = p ? 1 : 0;
                            diag_v = up_v;
                            path_bits |= p ? (1u << k) : 0u;
                            side_bits |= sideways ? (1u << k) : 0u;
                            if (lane == PS_WAVE - 1) fr.val[wave * fr.stride + j] = cur_v, fr.path[wave * fr.stride + j] = (uint8_t)cur_p;
                            if (i == na && j == nb) *final_val = cur_v;
                        }
                    }
                    path_word |= (uint64_t)path_bits << (half * SA_HALF);
                    side_word |= (uint64_t)side_bits << (half * SA_HALF);
                }
                if (i <= na) {
                    uint64_t* w = bits + ((size_t)(i - 1) * words + c) * 2;
                    w[0] = path_word, w[1] = side_word;
                }
            }
        }
        __syncthreads();
    }
}

// The trace back of a pass by one thread: the map (point of a -> point of b, or -1) and the pairs in order, which end at
// pair_a[pairs], pair_b[pairs]; returns their number.  map[] holds -1 on entry.
__device__ __forceinline__ int trace_back(const uint64_t* bits, int words, int na, int nb, int16_t* map, int16_t* pair_a,
                                          int16_t* pair_b, int pairs) {
    int i = na, j = nb, count = 0;
    for (int step = 0; step < na + nb && i > 0 && j > 0; ++step) {
        const int t = j - 1 + ((i - 1) & (PS_WAVE - 1));
        const uint64_t* w = bits + ((size_t)(i - 1) * words + (t >> 6)) * 2;
        if ((w[0] >> (t & 63)) & 1ull) {
            map[i - 1] = (int16_t)(j - 1);
            ++count;
            pair_a[pairs - count] = (int16_t)(i - 1), pair_b[pairs - count] = (int16_t)(j - 1);
            --i, --j;
        } else if ((w[1] >> (t & 63)) & 1ull) {
            --j;
        } else {
            --i;
        }
    }
    return count;
}

// ---- the score functors ------------------------------------------------------------------------------------------------------
struct MatrixScore {        // the caller's matrix at the slots of the points
    const float* score;
    const int16_t *slot_a, *slot_b;
    int Mb;
    struct Row {
        size_t first;
    };
    __device__ __forceinline__ Row row(int i) const { return Row{(size_t)slot_a[i] * (size_t)Mb}; }
    __device__ __forceinline__ double cell(const Row& r, int j) const { return (double)score[r.first + (size_t)slot_b[j]]; }
};

struct LabelScore {         // 1 where the labels are equal
    const int8_t *label_a, *label_b;
    struct Row {
        int label;
    };
    __device__ __forceinline__ Row row(int i) const { return Row{(int)label_a[i]}; }
    __device__ __forceinline__ double cell(const Row& r, int j) const { return r.label == (int)label_b[j] ? 1.0 : 0.0; }
};

struct TMScore {            // 1 / (1 + d^2 / d0^2) of T a_i against b_j, d^2 in K39's order of operations
    const float *planes_a, *planes_b;
    int Ma, Mb;
    Xform T;
    double d0sq;
    struct Row {
        double x[3];
    };
    __device__ __forceinline__ Row row(int i) const {
        const double a[3] = {(double)planes_a[i], (double)planes_a[Ma + i], (double)planes_a[2 * Ma + i]};
        Row r;
#pragma unroll
        for (int c = 0; c < 3; ++c) r.x[c] = ((T.R[c * 3] * a[0] + T.R[c * 3 + 1] * a[1]) + T.R[c * 3 + 2] * a[2]) + T.t[c];
        return r;
    }
    __device__ __forceinline__ double cell(const Row& r, int j) const {
        const double e[3] = {r.x[0] - (double)planes_b[j], r.x[1] - (double)planes_b[Mb + j], r.x[2] - (double)planes_b[2 * Mb + j]};
        return 1.0 / (1.0 + norm2(e) / d0sq);
    }
};

// ---- the clouds a chain or a fit runs over -----------------------------------------------------------------------------------
struct PairCloud {          // the pairs of a map
    const float *planes_a, *planes_b;
    int Ma, Mb;
    const int16_t *pair_a, *pair_b;
    int n, J;
    __device__ __forceinline__ void load(int k, double* a, double* b) const {
        const int i = pair_a[k], j = pair_b[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = (double)planes_a[c * Ma + i], b[c] = (double)planes_b[c * Mb + j];
    }
};

struct OffsetCloud {        // a_(i0 + k) with b_(j0 + k)
    const float *planes_a, *planes_b;
    int Ma, Mb, i0, j0;
    int n, J;
    __device__ __forceinline__ void load(int k, double* a, double* b) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = (double)planes_a[c * Ma + i0 + k], b[c] = (double)planes_b[c * Mb + j0 + k];
    }
};

// the greater S, the lower key on ties, over the waves' (S, key, R, t) in chain[SA_WAVES][16]; the same bits in every thread
__device__ __forceinline__ void pick_over_waves(const double* chain, double& S, int& key, Xform& T) {
    S = -(double)INFINITY, key = 0x7fffffff;
    int winner = 0;
#pragma unroll
    for (int w = 0; w < SA_WAVES; ++w) {
        const double Sw = chain[w * 16];
        const int kw = (int)chain[w * 16 + 1];
        if (Sw > S || (Sw == S && kw < key)) S = Sw, key = kw, winner = w;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) T.R[i] = chain[winner * 16 + 2 + i];
#pragma unroll
    for (int c = 0; c < 3; ++c) T.t[c] = chain[winner * 16 + 11 + c];
}

__device__ __forceinline__ void post_to_chain(double* chain, int wave, int lane, double S, int key, const Xform& T) {
    __syncthreads();                // the readers of an earlier round are done
    if (lane == 0) {
        chain[wave * 16] = S, chain[wave * 16 + 1] = (double)key;
#pragma unroll
        for (int i = 0; i < 9; ++i) chain[wave * 16 + 2 + i] = T.R[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) chain[wave * 16 + 11 + c] = T.t[c];
    }
    __syncthreads();
}

// fit-search over the pairs of a map (n >= 1 of them): the same (S, T) in every thread.  Whole workgroup.
__device__ __noinline__ void fit_search(const PairCloud& C, double d0, double* chain, double& S, Xform& T) {
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    SeedTable table;
    seed_table(C.n, table);
    const int n_seeds = table.count[0] + (table.n_lengths >= 2 ? table.count[1] : 0);     // at most five
    const double p2 = d0 * d0, ds = d0 < 4.5 ? 4.5 : (d0 > 8.0 ? 8.0 : d0);
    double mine = -(double)INFINITY;
    int mine_seed = 0x7fffffff;
    Xform mine_T = {};
    for (int s = wave; s < n_seeds && s < 2 * SA_WAVES; s += SA_WAVES) {
        int start, len;
        seed_fragment(table, C.n, s, start, len);
        double found;
        Xform kept;
        run_chain(C, lane, start, len, PS_SUPERPOSE_TM, p2, ds - 1.0, ds + 1.0, found, kept);
        if (found > mine) mine = found, mine_seed = s, mine_T = kept;
    }
    post_to_chain(chain, wave, lane, mine, mine_seed, mine_T);
    int seed;
    pick_over_waves(chain, S, seed, T);
}

__device__ __forceinline__ void copy_map(int16_t* to, const int16_t* from, int n) {
    for (int i = threadIdx.x; i < n; i += SA_THREADS) to[i] = from[i];
}

// TM-align's make_sec over n staged points
__device__ __forceinline__ double ca_distance(const float* p, int stride, int i, int j) {
    const double e[3] = {(double)p[i] - (double)p[j], (double)p[stride + i] - (double)p[stride + j],
                         (double)p[2 * stride + i] - (double)p[2 * stride + j]};
    return sqrt(norm2(e));
}

__device__ __forceinline__ int ca_label(const float* p, int stride, int n, int i) {
    if (i < 2 || i > n - 3) return 0;
    const double d13 = ca_distance(p, stride, i - 2, i), d14 = ca_distance(p, stride, i - 2, i + 1);
    const double d15 = ca_distance(p, stride, i - 2, i + 2), d24 = ca_distance(p, stride, i - 1, i + 1);
    const double d25 = ca_distance(p, stride, i - 1, i + 2), d35 = ca_distance(p, stride, i, i + 2);
    if (fabs(d15 - 6.37) < 2.1 && fabs(d14 - 5.18) < 2.1 && fabs(d25 - 5.18) < 2.1 && fabs(d13 - 5.45) < 2.1 &&
        fabs(d24 - 5.45) < 2.1 && fabs(d35 - 5.45) < 2.1)
        return 1;
    if (fabs(d15 - 13.0) < 1.42 && fabs(d14 - 10.4) < 1.42 && fabs(d25 - 10.4) < 1.42 && fabs(d13 - 6.1) < 1.42 &&
        fabs(d24 - 6.1) < 1.42 && fabs(d35 - 6.1) < 1.42)
        return 2;
    return d15 < 8.0 ? 3 : 0;
}

// ---- K41 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SA_THREADS) void nw_align(const float* __restrict__ score, const uint8_t* __restrict__ mask_a,
                                                       const uint8_t* __restrict__ mask_b, double gap, unsigned char* __restrict__ workspace,
                                                       int32_t* __restrict__ map, int32_t* __restrict__ n_aligned,
                                                       float* __restrict__ value, int Ma, int Mb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Layout L = make_layout(Ma, Mb);
    const size_t s = blockIdx.x;
    int16_t* slot_a = reinterpret_cast<int16_t*>(lds + L.slot_a);
    int16_t* slot_b = reinterpret_cast<int16_t*>(lds + L.slot_b);
    int16_t* map_cur = reinterpret_cast<int16_t*>(lds + L.map_cur);
    int* ints = reinterpret_cast<int*>(lds + L.ints);
    double* final_val = reinterpret_cast<double*>(lds + L.chain);
    const int na = compact_slots(mask_a ? mask_a + s * Ma : nullptr, Ma, slot_a, ints);
    const int nb = compact_slots(mask_b ? mask_b + s * Mb : nullptr, Mb, slot_b, ints);
    for (int i = threadIdx.x; i < Ma; i += SA_THREADS) map[s * Ma + i] = -1, map_cur[i] = -1;
    if (na == 0 || nb == 0) {
        if (threadIdx.x == 0) n_aligned[s] = 0, value[s] = 0.0f;
        return;
    }
    uint64_t* bits = reinterpret_cast<uint64_t*>(L.bits_in_lds ? lds + L.bits : workspace + s * 2 * (size_t)L.unit_bytes + SA_ENTRY_BYTES);
    const Front fr{reinterpret_cast<double*>(lds + L.front_val), lds + L.front_path, Mb + 1};
    const MatrixScore f{score + s * (size_t)Ma * (size_t)Mb, slot_a, slot_b, Mb};
    nw_pass(f, na, nb, gap, fr, bits, L.words, final_val);
    if (threadIdx.x == 0) {
        n_aligned[s] = trace_back(bits, L.words, na, nb, map_cur, reinterpret_cast<int16_t*>(lds + L.pair_a),
                                  reinterpret_cast<int16_t*>(lds + L.pair_b), L.pairs);
        value[s] = (float)*final_val;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < na; i += SA_THREADS)
        if (map_cur[i] >= 0) map[s * Ma + slot_a[i]] = (int32_t)slot_b[map_cur[i]];
}

// ---- K44 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SA_THREADS) void ca_secondary_structure(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                     int8_t* __restrict__ labels, int M) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const size_t s = blockIdx.x;
    float* planes = reinterpret_cast<float*>(lds);
    int16_t* slots = reinterpret_cast<int16_t*>(lds + up16(3 * M * 4));
    int* ints = reinterpret_cast<int*>(lds + up16(3 * M * 4) + up16(M * 2));
    const int n = compact_slots(mask ? mask + s * M : nullptr, M, slots, ints);
    stage_points(x + s * (size_t)M * 3, slots, n, planes, M);
    for (int i = threadIdx.x; i < M; i += SA_THREADS) labels[s * M + i] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += SA_THREADS) labels[s * M + slots[i]] = (int8_t)ca_label(planes, M, n, i);
}

// ---- K42 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SA_THREADS) void structure_align(const float* __restrict__ a, const uint8_t* __restrict__ mask_a,
                                                              const float* __restrict__ b, const uint8_t* __restrict__ mask_b,
                                                              const float* __restrict__ d0s, unsigned char* __restrict__ workspace,
                                                              int Ma, int Mb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Layout L = make_layout(Ma, Mb);
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int start = blockIdx.x;
    const size_t s = blockIdx.y;
    float* planes_a = reinterpret_cast<float*>(lds + L.planes_a);
    float* planes_b = reinterpret_cast<float*>(lds + L.planes_b);
    int16_t* slot_a = reinterpret_cast<int16_t*>(lds + L.slot_a);
    int16_t* slot_b = reinterpret_cast<int16_t*>(lds + L.slot_b);
    int16_t* map_start = reinterpret_cast<int16_t*>(lds + L.map_start);
    int16_t* map_prev = reinterpret_cast<int16_t*>(lds + L.map_prev);
    int16_t* map_cur = reinterpret_cast<int16_t*>(lds + L.map_cur);
    int16_t* map_best = reinterpret_cast<int16_t*>(lds + L.map_best);
    int16_t* pair_a = reinterpret_cast<int16_t*>(lds + L.pair_a);
    int16_t* pair_b = reinterpret_cast<int16_t*>(lds + L.pair_b);
    double* chain = reinterpret_cast<double*>(lds + L.chain);
    int* ints = reinterpret_cast<int*>(lds + L.ints);              // [0 .. 3] the compaction's totals, [4] the pairs of a trace
    double* final_val = reinterpret_cast<double*>(lds + L.ints + 32);
    unsigned char* unit = workspace + (s * 2 + start) * (size_t)L.unit_bytes;
    Entry* entry = reinterpret_cast<Entry*>(unit);
    int32_t* unit_map = reinterpret_cast<int32_t*>(unit + SA_ENTRY_BYTES + (L.bits_in_lds ? 0 : L.bits_bytes));
    uint64_t* bits = reinterpret_cast<uint64_t*>(L.bits_in_lds ? lds + L.bits : unit + SA_ENTRY_BYTES);
    const Front fr{reinterpret_cast<double*>(lds + L.front_val), lds + L.front_path, Mb + 1};

    const int na = compact_slots(mask_a ? mask_a + s * Ma : nullptr, Ma, slot_a, ints);
    const int nb = compact_slots(mask_b ? mask_b + s * Mb : nullptr, Mb, slot_b, ints);
    if (na == 0 || nb == 0) {
        if (threadIdx.x == 0) entry->S = -(double)INFINITY, entry->n_aligned = 0, entry->n_a = na, entry->n_b = nb;
        return;
    }
    stage_points(a + s * (size_t)Ma * 3, slot_a, na, planes_a, Ma);
    stage_points(b + s * (size_t)Mb * 3, slot_b, nb, planes_b, Mb);
    for (int i = threadIdx.x; i < na; i += SA_THREADS) map_start[i] = -1;
    __syncthreads();
    const double d0 = (double)d0s[s];
    int n_pairs = 0;

    if (start == 0) {
        // ---- the threading: one offset per wave at a time
        const int fewer = na < nb ? na : nb;
        const int need = fewer / 2 > (fewer < 5 ? fewer : 5) ? fewer / 2 : (fewer < 5 ? fewer : 5);
        const int k_first = -(na - need), k_last = nb - need;
        double mine = -(double)INFINITY;
        int mine_k = 0x7fffffff;
        Xform T = {};
        for (int k = k_first + wave; k <= k_last; k += SA_WAVES) {
            const int i0 = k < 0 ? -k : 0, i1 = na < nb - k ? na : nb - k;
            const OffsetCloud C{planes_a, planes_b, Ma, Mb, i0, i0 + k, i1 - i0, (i1 - i0 + PS_WAVE - 1) / PS_WAVE};
            uint32_t everyone = 0, unused;
            for (int j = 0; j < C.J; ++j) everyone |= j * PS_WAVE + lane < C.n ? (1u << j) : 0u;
            fit_selected(C, lane, everyone, T);
            double S = 0.0;
            sweep<true>(C, lane, T, PS_SUPERPOSE_TM, d0 * d0, 0.0, unused, S);
            if (S > mine) mine = S, mine_k = k;
        }
        post_to_chain(chain, wave, lane, mine, mine_k, T);
        double S;
        int k;
        pick_over_waves(chain, S, k, T);
        if (k == 0x7fffffff) k = k_first;                // no finite score (d0 is not a positive number): the caller's error
        const int i0 = k < 0 ? -k : 0, i1 = na < nb - k ? na : nb - k;
        n_pairs = i1 - i0;
        for (int i = i0 + (int)threadIdx.x; i < i1; i += SA_THREADS) {
            map_start[i] = (int16_t)(i + k);
            pair_a[L.pairs - n_pairs + (i - i0)] = (int16_t)i, pair_b[L.pairs - n_pairs + (i - i0)] = (int16_t)(i + k);
        }
        __syncthreads();
    } else {
        // ---- the DP over equal secondary-structure labels
        int8_t* label_a = reinterpret_cast<int8_t*>(lds + L.label_a);
        int8_t* label_b = reinterpret_cast<int8_t*>(lds + L.label_b);
        for (int i = threadIdx.x; i < na; i += SA_THREADS) label_a[i] = (int8_t)ca_label(planes_a, Ma, na, i);
        for (int j = threadIdx.x; j < nb; j += SA_THREADS) label_b[j] = (int8_t)ca_label(planes_b, Mb, nb, j);
        __syncthreads();
        const LabelScore f{label_a, label_b};
        nw_pass(f, na, nb, -1.0, fr, bits, L.words, final_val);
        if (threadIdx.x == 0) ints[4] = trace_back(bits, L.words, na, nb, map_start, pair_a, pair_b, L.pairs);
        __syncthreads();
        n_pairs = ints[4];
    }

    // ---- the refinement
    double best = -(double)INFINITY;
    int best_pairs = 0;
    Xform best_T = {}, T0 = {};
    if (n_pairs > 0) {
        const PairCloud P{planes_a, planes_b, Ma, Mb, pair_a + (L.pairs - n_pairs), pair_b + (L.pairs - n_pairs), n_pairs,
                          (n_pairs + PS_WAVE - 1) / PS_WAVE};
        double S;
        fit_search(P, d0, chain, S, T0);
        if (S > best) {
            best = S, best_T = T0, best_pairs = n_pairs;
            copy_map(map_best, map_start, na);
        }
        for (int round = 0; round < 2; ++round) {
            const double gap = round == 0 ? (double)(-0.6f) : 0.0;
            copy_map(map_prev, map_start, na);
            TMScore f{planes_a, planes_b, Ma, Mb, T0, d0 * d0};
            for (int it = 0; it < PS_STRUCTALIGN_MAX_ITERATIONS; ++it) {
                for (int i = threadIdx.x; i < na; i += SA_THREADS) map_cur[i] = -1;
                nw_pass(f, na, nb, gap, fr, bits, L.words, final_val);          // begins and ends with a barrier
                if (threadIdx.x == 0) ints[4] = trace_back(bits, L.words, na, nb, map_cur, pair_a, pair_b, L.pairs);
                __syncthreads();
                const int found = ints[4];
                if (found == 0) break;
                const PairCloud Q{planes_a, planes_b, Ma, Mb, pair_a + (L.pairs - found), pair_b + (L.pairs - found), found,
                                  (found + PS_WAVE - 1) / PS_WAVE};
                fit_search(Q, d0, chain, S, f.T);
                if (S > best) {
                    best = S, best_T = f.T, best_pairs = found;
                    copy_map(map_best, map_cur, na);
                }
                int differs = 0;
                for (int i = threadIdx.x; i < na; i += SA_THREADS) differs |= map_cur[i] != map_prev[i];
                if (__syncthreads_or(differs) == 0) break;
                copy_map(map_prev, map_cur, na);
                __syncthreads();
            }
            __syncthreads();
        }
    }

    // ---- the start's result
    for (int i = threadIdx.x; i < Ma; i += SA_THREADS) unit_map[i] = -1;
    __syncthreads();
    if (best > -(double)INFINITY)
        for (int i = threadIdx.x; i < na; i += SA_THREADS)
            if (map_best[i] >= 0) unit_map[slot_a[i]] = (int32_t)slot_b[map_best[i]];
    if (threadIdx.x == 0) {
        entry->S = best;
#pragma unroll
        for (int i = 0; i < 9; ++i) entry->R[i] = (float)best_T.R[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) entry->t[c] = (float)best_T.t[c];
        entry->n_aligned = best > -(double)INFINITY ? best_pairs : 0;
        entry->n_a = na, entry->n_b = nb;
    }
}

// ---- K43 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void structure_align_pick(const unsigned char* __restrict__ workspace, int n_starts,
                                                                int32_t* __restrict__ map, int32_t* __restrict__ n_aligned,
                                                                float* __restrict__ score, float* __restrict__ R, float* __restrict__ t,
                                                                int32_t* __restrict__ n_points, int32_t* __restrict__ start, int Ma,
                                                                int Mb) {
    const Layout L = make_layout(Ma, Mb);
    const int lane = threadIdx.x;
    const size_t s = blockIdx.x;
    const unsigned char* unit = workspace + s * 2 * (size_t)L.unit_bytes;
    const Entry* first = reinterpret_cast<const Entry*>(unit);
    int winner = 0;
    if (n_starts > 1 && reinterpret_cast<const Entry*>(unit + L.unit_bytes)->S > first->S) winner = 1;
    unit += (size_t)winner * (size_t)L.unit_bytes;
    const Entry* e = reinterpret_cast<const Entry*>(unit);
    const int32_t* unit_map = reinterpret_cast<const int32_t*>(unit + SA_ENTRY_BYTES + (L.bits_in_lds ? 0 : L.bits_bytes));
    const bool found = e->S > -(double)INFINITY;
    for (int i = lane; i < Ma; i += PS_WAVE) map[s * Ma + i] = found ? unit_map[i] : -1;
    if (lane < 9) R[s * 9 + lane] = found ? e->R[lane] : NAN;
    if (lane < 3) t[s * 3 + lane] = found ? e->t[lane] : NAN;
    if (lane == 0) {
        const int fewer = e->n_a < e->n_b ? e->n_a : e->n_b;
        n_aligned[s] = found ? e->n_aligned : 0;
        score[s] = found ? (float)(e->S / (double)fewer) : 0.0f;
        n_points[s * 2] = e->n_a, n_points[s * 2 + 1] = e->n_b;
        start[s] = found ? winner : 0;
    }
}

// ---- launching ---------------------------------------------------------------------------------------------------------------
// More than 64 KB of dynamic LDS has to be allowed once per kernel and per device; `done` is the kernel's own bit per device.
// Idempotent, so a race between two threads is harmless.
int allow_big_lds(const void* kernel, unsigned long long& done, hipStream_t stream) {
    int dev = 0;
    hipDevice_t of_stream;
    if (stream && hipStreamGetDevice(stream, &of_stream) == hipSuccess) dev = (int)of_stream;
    else if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorInvalidDevice;
    if (dev < 0 || dev >= 64) return (int)hipErrorInvalidDevice;
    const unsigned long long bit = 1ull << dev;
    if (__atomic_load_n(&done, __ATOMIC_ACQUIRE) & bit) return 0;
    int cur = dev;
    (void)hipGetDevice(&cur);
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return (int)hipErrorInvalidDevice;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SA_LDS_MAX);
    if (cur != dev) (void)hipSetDevice(cur);
    if (e != hipSuccess) return (int)e;
    __atomic_fetch_or(&done, bit, __ATOMIC_RELEASE);
    return 0;
}

// the workspace from its first 8-byte boundary on: the caller's pointer needs no alignment
unsigned char* aligned_workspace(void* workspace) {
    return reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 7) & ~(uintptr_t)7);
}

bool bad_shape(int B, int Ma, int Mb) {
    return B < 0 || B > 65535 || Ma < 1 || Ma > PS_STRUCTALIGN_MAX_POINTS || Mb < 1 || Mb > PS_STRUCTALIGN_MAX_POINTS;
}

}  // namespace

extern "C" int ps_structalign_api(void) { return PS_STRUCTALIGN_API; }

extern "C" long long ps_structalign_workspace_bytes(int B, int Ma, int Mb) {
    if (bad_shape(B, Ma, Mb)) return -1;
    return (long long)B * 2 * make_layout(Ma, Mb).unit_bytes + 8;       // 8: the launchers round the pointer up to 8 bytes
}

extern "C" int ps_nw_align_f32(const float* score, const uint8_t* mask_a, const uint8_t* mask_b, float gap, void* workspace,
                               int32_t* map, int32_t* n_aligned, float* value, int B, int Ma, int Mb, void* stream) {
    if (bad_shape(B, Ma, Mb) || !(gap <= 0.0f && gap > -INFINITY)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!score || !workspace || !map || !n_aligned || !value) return (int)hipErrorInvalidValue;
    static unsigned long long allowed = 0;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = allow_big_lds(reinterpret_cast<const void*>(nw_align), allowed, s);
    if (rc) return rc;
    return ps_launch(nw_align, dim3((unsigned)B), dim3(SA_THREADS), (size_t)make_layout(Ma, Mb).total, s, score, mask_a, mask_b,
                     (double)gap, aligned_workspace(workspace), map, n_aligned, value, Ma, Mb);
}

extern "C" int ps_ca_secondary_structure_f32(const float* x, const uint8_t* mask, int8_t* labels, int B, int M, void* stream) {
    if (B < 0 || B > 65535 || M < 1 || M > PS_STRUCTALIGN_MAX_POINTS) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!x || !labels) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)up16(3 * M * 4) + (size_t)up16(M * 2) + 64;
    return ps_launch(ca_secondary_structure, dim3((unsigned)B), dim3(SA_THREADS), lds, reinterpret_cast<hipStream_t>(stream), x, mask,
                     labels, M);
}

extern "C" int ps_structure_align_f32(const float* a, const uint8_t* mask_a, const float* b, const uint8_t* mask_b, const float* d0,
                                      int use_ss, void* workspace, int32_t* map, int32_t* n_aligned, float* score, float* R,
                                      float* t, int32_t* n_points, int32_t* start, int B, int Ma, int Mb, void* stream) {
    if (bad_shape(B, Ma, Mb)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!a || !b || !d0 || !workspace || !map || !n_aligned || !score || !R || !t || !n_points || !start)
        return (int)hipErrorInvalidValue;
    static unsigned long long allowed = 0;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = allow_big_lds(reinterpret_cast<const void*>(structure_align), allowed, s);
    if (rc) return rc;
    const int n_starts = use_ss ? 2 : 1;
    unsigned char* ws = aligned_workspace(workspace);
    rc = ps_launch(structure_align, dim3((unsigned)n_starts, (unsigned)B), dim3(SA_THREADS), (size_t)make_layout(Ma, Mb).total, s, a,
                   mask_a, b, mask_b, d0, ws, Ma, Mb);
    if (rc) return rc;
    return ps_launch(structure_align_pick, dim3((unsigned)B), dim3(PS_WAVE), 0, s, ws, n_starts, map, n_aligned, score, R, t, n_points,
                     start, Ma, Mb);
}
