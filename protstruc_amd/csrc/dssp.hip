// K21 / K22 -- DSSP (Kabsch & Sander 1983, with the two-best-partners rule of the DSSP programs): the backbone hydrogen
// bonds of every residue, and the secondary-structure label of every residue from them.
//
//   residue j has an amide hydrogen iff junction[j-1], complete[j] and donor[j]:   H_j = N_j + unit(C_{j-1} - O_{j-1})
//   E(i, j) = 27.888 (1/d(O_i,N_j) + 1/d(C_i,H_j) - 1/d(O_i,H_j) - 1/d(C_i,N_j))   acceptor C=O of i, donor N-H of j
//   for complete i, j with an H, i != j, j != i + 1, |CA_i - CA_j| < 9;  -9.9 if one of the four distances is below 0.5
//   every donor keeps its two lowest energies below -0.5 (ties: the lower acceptor index), every acceptor its two donors
//
// Three simplifications against the DSSP programs: energies are not rounded to 0.001, ladders are not joined across
// beta-bulges, and the label is a pure per-residue priority (H B E G I T S).
//
// The H-bond sweep (K21) is the owner sweep of violation.hip: a workgroup is four waves that share 64 OWNERS, one residue
// per lane in registers IN BOTH ROLES (N, H, CA as donor; C, O, CA as acceptor); the columns are staged through LDS in
// tiles of 256 residues, one per thread, COMPACTED while staging (an incomplete residue never reaches LDS, so NaN there
// never meets arithmetic); wave w takes the compacted items w, w + 4, ... -- each read one address for the whole wave,
// an LDS broadcast.  A wave whose 64 owners all fail the fp32 test |CA_i - CA_j|^2 < 81 for a column (one ballot, no
// square root) skips it; that leaves a few per cent of the pairs.  The survivors are evaluated in DOUBLE: the coordinates
// are fp32 values, so their differences are exact there, H is computed in double, and the decision E < -0.5 is the one a
// float64 evaluation of the definition takes.  Each lane keeps a sorted top-2 as donor and as acceptor in registers; the
// four waves' lists are merged through LDS in wave order under the same (energy, index) order.  No N x N tensor exists,
// there are no atomics and every list has one fixed order: results repeat bit for bit.
//
// The assignment (K22) is one workgroup per structure, lanes striding over residues, with the kept acceptor lists, the
// junctions and the per-residue flags in LDS: turns -> bridges -> labels, separated by barriers.  hb(i, j) is "i is in
// donor j's kept list"; the bridge partners of i are found from the lists alone -- every bridge (i, j) has j or j - 1 in
// the list of i or of i + 1, eight candidates -- so the kernel is O(N).
#include "ps_common.hpp"
#include "owner_sweep.hpp"   // WAVES, compact_slot and the barrier protocol of staging a tile

#include <math.h>

#include "../../include/protstruc_hip.h"

namespace {

constexpr int OWNERS = PS_DSSP_RESIDUE_TILE;   // owners per workgroup = lanes per wave
constexpr int THREADS = OWNERS * WAVES;        // = raw residues staged per tile
constexpr int ITEM_FLOATS = 20;                // N, CA, C, O (12), index, has_h, H as three doubles (6): five 16-byte reads
static_assert(OWNERS == PS_WAVE, "one owner per lane");

constexpr double HB_FACTOR = 27.888;      // 332 * 0.42 * 0.20 kcal/mol A
constexpr double HB_CUTOFF = -0.5;        // a hydrogen bond is an energy below this
constexpr double HB_FLOOR = -9.9;         // the energy of a pair with a distance below HB_MIN_DIST
constexpr double HB_MIN_DIST = 0.5;
constexpr float CA_CUTOFF_SQ = 81.0f;     // pairs whose CA atoms are 9 A or more apart are not evaluated

struct slots_t {
    int n, ca, c, o;
};

struct residue_t {
    f3 n, ca, c, o;
    double h[3];
    int index;
    bool has_h;
};

__device__ __forceinline__ residue_t empty_residue() {
    const f3 z = f3{0.0f, 0.0f, 0.0f};
    return residue_t{z, z, z, z, {0.0, 0.0, 0.0}, -1, false};
}

// Residue m of structure b, which is complete; its H from C and O of residue m - 1 where it has one.
__device__ __forceinline__ residue_t load_residue(const float* __restrict__ xyz, const uint8_t* __restrict__ junction,
                                                  const uint8_t* __restrict__ donor, size_t b, int N, int A, slots_t s, int m) {
    const size_t at = b * N + m;
    const float* res = xyz + at * (size_t)A * 3;
    residue_t r;
    r.n = load3(res + s.n * 3);
    r.ca = load3(res + s.ca * 3);
    r.c = load3(res + s.c * 3);
    r.o = load3(res + s.o * 3);
    r.index = m;
    r.has_h = m > 0 && junction[at - 1] != 0 && (!donor || donor[at] != 0);
    r.h[0] = r.h[1] = r.h[2] = 0.0;
    if (r.has_h) {
        const float* prev = res - (size_t)A * 3;
        const f3 c = load3(prev + s.c * 3), o = load3(prev + s.o * 3);
        const double d[3] = {(double)c.x - (double)o.x, (double)c.y - (double)o.y, (double)c.z - (double)o.z};
        const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        r.h[0] = (double)r.n.x + d[0] / len;
        r.h[1] = (double)r.n.y + d[1] / len;
        r.h[2] = (double)r.n.z + d[2] / len;
    }
    return r;
}

// Stage residues [m0, m0 + THREADS) of structure b, complete ones only, in index order; returns how many.
__device__ __forceinline__ int stage_residues(const float* __restrict__ xyz, const uint8_t* __restrict__ complete,
                                              const uint8_t* __restrict__ junction, const uint8_t* __restrict__ donor,
                                              size_t b, int N, int A, slots_t s, int m0, float* tile, int* wave_counts) {
    const int m = m0 + threadIdx.x;
    const bool valid = m < N && complete[b * N + m] != 0;
    int total;
    const int slot = compact_slot(valid, wave_counts, total);
    if (valid) {
        const residue_t r = load_residue(xyz, junction, donor, b, N, A, s, m);
        float4* o = reinterpret_cast<float4*>(tile + slot * ITEM_FLOATS);
        o[0] = make_float4(r.n.x, r.n.y, r.n.z, r.ca.x);
        o[1] = make_float4(r.ca.y, r.ca.z, r.c.x, r.c.y);
        o[2] = make_float4(r.c.z, r.o.x, r.o.y, r.o.z);
        double* h = reinterpret_cast<double*>(tile + slot * ITEM_FLOATS + 12);   // 48 bytes in: 8-byte aligned
        h[0] = r.h[0];
        h[1] = r.h[1];
        h[2] = r.h[2];
        tile[slot * ITEM_FLOATS + 18] = __int_as_float(r.index);
        tile[slot * ITEM_FLOATS + 19] = __int_as_float(r.has_h ? 1 : 0);
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ residue_t read_residue(const float* tile, int j) {
    const float4* p = reinterpret_cast<const float4*>(tile + j * ITEM_FLOATS);
    const float4 a = p[0], c = p[1], e = p[2];
    const double* h = reinterpret_cast<const double*>(tile + j * ITEM_FLOATS + 12);
    residue_t r;
    r.n = f3{a.x, a.y, a.z};
    r.ca = f3{a.w, c.x, c.y};
    r.c = f3{c.z, c.w, e.x};
    r.o = f3{e.y, e.z, e.w};
    r.h[0] = h[0];
    r.h[1] = h[1];
    r.h[2] = h[2];
    r.index = __float_as_int(tile[j * ITEM_FLOATS + 18]);
    r.has_h = __float_as_int(tile[j * ITEM_FLOATS + 19]) != 0;
    return r;
}

__device__ __forceinline__ double dist_d(double ax, double ay, double az, double bx, double by, double bz) {
    const double x = ax - bx, y = ay - by, z = az - bz;
    return sqrt((x * x + y * y) + z * z);
}

// E(acceptor, donor) in double: the C=O of `acc`, the N-H of `don`
__device__ __forceinline__ double hbond_energy(const residue_t& acc, const residue_t& don) {
    const double ox = acc.o.x, oy = acc.o.y, oz = acc.o.z, cx = acc.c.x, cy = acc.c.y, cz = acc.c.z;
    const double nx = don.n.x, ny = don.n.y, nz = don.n.z;
    const double d_on = dist_d(ox, oy, oz, nx, ny, nz), d_ch = dist_d(cx, cy, cz, don.h[0], don.h[1], don.h[2]);
    const double d_oh = dist_d(ox, oy, oz, don.h[0], don.h[1], don.h[2]), d_cn = dist_d(cx, cy, cz, nx, ny, nz);
    const double e = HB_FACTOR * (((1.0 / d_on + 1.0 / d_ch) - 1.0 / d_oh) - 1.0 / d_cn);
    const bool close = d_on < HB_MIN_DIST || d_ch < HB_MIN_DIST || d_oh < HB_MIN_DIST || d_cn < HB_MIN_DIST;
    return close ? HB_FLOOR : e;
}

// A sorted list of the two best partners: lower energy first, ties to the lower index; an empty slot is (0, -1).
struct top2_t {
    double e0, e1;
    int i0, i1;
};

__device__ __forceinline__ bool better(double e, int i, double e_kept, int i_kept) {
    return i_kept < 0 || e < e_kept || (e == e_kept && i < i_kept);
}

__device__ __forceinline__ void keep(top2_t& t, bool take, double e, int i) {
    const bool first = take && better(e, i, t.e0, t.i0);
    const bool second = take && !first && better(e, i, t.e1, t.i1);
    t.e1 = first ? t.e0 : (second ? e : t.e1);
    t.i1 = first ? t.i0 : (second ? i : t.i1);
    t.e0 = first ? e : t.e0;
    t.i0 = first ? i : t.i0;
}

// ---- K21: owner i keeps its two best acceptors (as donor) and its two best donors (as acceptor) -------------------------
__global__ __launch_bounds__(THREADS) void k_backbone_hbonds(const float* __restrict__ xyz, const uint8_t* __restrict__ complete,
                                                             const uint8_t* __restrict__ junction,
                                                             const uint8_t* __restrict__ donor, slots_t s,
                                                             int* __restrict__ acceptor_idx, float* __restrict__ acceptor_energy,
                                                             int* __restrict__ donor_idx, float* __restrict__ donor_energy,
                                                             int N, int A) {
    __shared__ __attribute__((aligned(16))) float tile[THREADS * ITEM_FLOATS];
    __shared__ double wave_e[WAVES * 4 * OWNERS];
    __shared__ int wave_i[WAVES * 4 * OWNERS];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int i = blockIdx.x * OWNERS + lane;
    const bool own = i < N && complete[b * N + i] != 0;
    // an owner that is incomplete or past the end holds zeros and takes no part: its coordinates are never read
    const residue_t me = own ? load_residue(xyz, junction, donor, b, N, A, s, i) : empty_residue();
    top2_t acc = {0.0, 0.0, -1, -1};   // as donor: the acceptors of my N-H
    top2_t don = {0.0, 0.0, -1, -1};   // as acceptor: the donors to my C=O
    for (int m0 = 0; m0 < N; m0 += THREADS) {
        const int n = stage_residues(xyz, complete, junction, donor, b, N, A, s, m0, tile, wave_counts);
        for (int j = wave; j < n; j += WAVES) {
            const residue_t o = read_residue(tile, j);
            const f3 diff = sub3(me.ca, o.ca);
            const bool near = own && o.index != i && norm_sq3(diff.x, diff.y, diff.z) < CA_CUTOFF_SQ;
            if (__ballot(near) == 0ull) continue;   // no owner of this wave comes near column j
            // my N-H to its C=O: I am not the residue after it;  its N-H to my C=O: it is not the residue after me
            const bool as_donor = near && me.has_h && i != o.index + 1;
            const bool as_acceptor = near && o.has_h && o.index != i + 1;
            const double e_d = hbond_energy(o, me), e_a = hbond_energy(me, o);
            keep(acc, as_donor && e_d < HB_CUTOFF, e_d, o.index);
            keep(don, as_acceptor && e_a < HB_CUTOFF, e_a, o.index);
        }
    }
    // the four waves' lists, merged in wave order
    const int at = wave * 4 * OWNERS + lane;
    wave_e[at] = acc.e0;
    wave_i[at] = acc.i0;
    wave_e[at + OWNERS] = acc.e1;
    wave_i[at + OWNERS] = acc.i1;
    wave_e[at + 2 * OWNERS] = don.e0;
    wave_i[at + 2 * OWNERS] = don.i0;
    wave_e[at + 3 * OWNERS] = don.e1;
    wave_i[at + 3 * OWNERS] = don.i1;
    __syncthreads();
    if (wave != 0 || i >= N) return;
    for (int w = 1; w < WAVES; ++w) {
        const int from = w * 4 * OWNERS + lane;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ia = wave_i[from + k * OWNERS], id = wave_i[from + (2 + k) * OWNERS];
            keep(acc, ia >= 0, wave_e[from + k * OWNERS], ia);
            keep(don, id >= 0, wave_e[from + (2 + k) * OWNERS], id);
        }
    }
    // one rounding to float; an empty slot is index -1 and energy 0
    const size_t out = (b * N + i) * 2;
    acceptor_idx[out] = acc.i0;
    acceptor_idx[out + 1] = acc.i1;
    acceptor_energy[out] = (float)acc.e0;
    acceptor_energy[out + 1] = (float)acc.e1;
    donor_idx[out] = don.i0;
    donor_idx[out + 1] = don.i1;
    donor_energy[out] = (float)don.e0;
    donor_energy[out + 1] = (float)don.e1;
}

// ---- K22: the labels of one structure ------------------------------------------------------------------------------------
constexpr int MAX_N = PS_DSSP_MAX_RESIDUES;
constexpr int ASSIGN_THREADS = 256;
constexpr double COS_BEND = 0.3420201433256687;   // cos(70 deg): a bend is an angle above 70 degrees

enum : int { LABEL_NONE = 0, LABEL_H = 1, LABEL_B = 2, LABEL_E = 3, LABEL_G = 4, LABEL_I = 5, LABEL_T = 6, LABEL_S = 7 };
enum : int { PARALLEL = 1, ANTIPARALLEL = 2 };

struct chain_t {
    const int* acc0;          // LDS: the kept acceptors of every donor
    const int* acc1;
    const uint8_t* junction;  // LDS: entry r = r -> r + 1 is a peptide bond; entry N - 1 is 0
    int N;
};

// junction[i .. i + k - 1] are all true
__device__ __forceinline__ bool cont(const chain_t& c, int i, int k) {
    if (i < 0 || i + k > c.N) return false;
    bool all = true;
    for (int t = 0; t < k; ++t) all = all && c.junction[i + t] != 0;
    return all;
}

// i is in donor j's kept list
__device__ __forceinline__ bool hb(const chain_t& c, int i, int j) {
    return i >= 0 && i < c.N && j >= 0 && j < c.N && (c.acc0[j] == i || c.acc1[j] == i);
}

// the types of bridge that (i, j) is: PARALLEL | ANTIPARALLEL, 0 for none
__device__ __forceinline__ int bridge(const chain_t& c, int i, int j) {
    if (i < 0 || j < 0 || i >= c.N || j >= c.N || (i > j ? i - j : j - i) < 3) return 0;
    if (!cont(c, i - 1, 2) || !cont(c, j - 1, 2)) return 0;
    const bool par = (hb(c, i - 1, j) && hb(c, j, i + 1)) || (hb(c, j - 1, i) && hb(c, i, j + 1));
    const bool anti = (hb(c, i, j) && hb(c, j, i)) || (hb(c, i - 1, j + 1) && hb(c, j - 1, i + 1));
    return (par ? PARALLEL : 0) | (anti ? ANTIPARALLEL : 0);
}

__global__ __launch_bounds__(ASSIGN_THREADS) void k_dssp_assign(const float* __restrict__ xyz,
                                                                const uint8_t* __restrict__ complete,
                                                                const uint8_t* __restrict__ junction,
                                                                const int* __restrict__ acceptor_idx, int ca_slot,
                                                                int8_t* __restrict__ codes, int N, int A) {
    __shared__ int acc0[MAX_N], acc1[MAX_N];
    __shared__ uint8_t junc[MAX_N];
    __shared__ uint8_t turns[MAX_N];    // bit n - 3: an n-turn starts here
    __shared__ uint8_t sheet[MAX_N];    // 1: in a bridge, 2: in a ladder
    const size_t b = blockIdx.x;
    const chain_t c = {acc0, acc1, junc, N};
    for (int r = threadIdx.x; r < N; r += ASSIGN_THREADS) {
        const size_t at = b * N + r;
        // an index outside [0, N) is no partner
        const int a0 = acceptor_idx[at * 2], a1 = acceptor_idx[at * 2 + 1];
        acc0[r] = a0 >= 0 && a0 < N ? a0 : -1;
        acc1[r] = a1 >= 0 && a1 < N ? a1 : -1;
        junc[r] = r < N - 1 && junction[at] != 0 ? 1 : 0;
    }
    __syncthreads();
    // turns
    for (int r = threadIdx.x; r < N; r += ASSIGN_THREADS) {
        int t = 0;
        for (int n = 3; n <= 5; ++n) t |= cont(c, r, n) && hb(c, r, r + n) ? 1 << (n - 3) : 0;
        turns[r] = (uint8_t)t;
    }
    __syncthreads();
    // bridges: every bridge (r, j) has j or j - 1 in the kept list of r or of r + 1
    for (int r = threadIdx.x; r < N; r += ASSIGN_THREADS) {
        int found = 0;
        for (int k = 0; k < 8; ++k) {
            const int row = r + (k >> 2);
            if (row >= N) continue;
            const int partner = (k & 2) ? acc1[row] : acc0[row];
            if (partner < 0) continue;
            const int j = partner + (k & 1);
            const int kind = bridge(c, r, j);
            if (!kind) continue;
            found |= 1;
            const bool par = (kind & PARALLEL) && ((bridge(c, r - 1, j - 1) | bridge(c, r + 1, j + 1)) & PARALLEL);
            const bool anti = (kind & ANTIPARALLEL) && ((bridge(c, r - 1, j + 1) | bridge(c, r + 1, j - 1)) & ANTIPARALLEL);
            found |= par || anti ? 2 : 0;
        }
        sheet[r] = (uint8_t)found;
    }
    __syncthreads();
    // labels: the first of H B E G I T S that holds
    for (int r = threadIdx.x; r < N; r += ASSIGN_THREADS) {
        const size_t at = b * N + r;
        bool helix[3] = {false, false, false}, turn = false;
        for (int n = 3; n <= 5; ++n) {
            const int bit = 1 << (n - 3);
            // residues i .. i + n - 1 of two consecutive n-turns at i - 1 and i;  residues i + 1 .. i + n - 1 of an n-turn at i
            for (int i = r - n + 1 > 0 ? r - n + 1 : 0; i <= r; ++i) {
                if (i >= 1 && (turns[i] & bit) && (turns[i - 1] & bit)) helix[n - 3] = true;
                if (i < r && (turns[i] & bit)) turn = true;
            }
        }
        bool bend = false;
        if (cont(c, r - 2, 4)) {
            const float* ca = xyz + at * (size_t)A * 3 + ca_slot * 3;
            const size_t two = (size_t)2 * A * 3;
            const double u[3] = {(double)ca[0] - (double)(ca - two)[0], (double)ca[1] - (double)(ca - two)[1],
                                 (double)ca[2] - (double)(ca - two)[2]};
            const double v[3] = {(double)(ca + two)[0] - (double)ca[0], (double)(ca + two)[1] - (double)ca[1],
                                 (double)(ca + two)[2] - (double)ca[2]};
            const double uv = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
            const double uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
            bend = uv / (sqrt(uu) * sqrt(vv)) < COS_BEND;
        }
        int label = LABEL_NONE;
        if (helix[1]) label = LABEL_H;
        else if (sheet[r] == 1) label = LABEL_B;
        else if (sheet[r] & 2) label = LABEL_E;
        else if (helix[0]) label = LABEL_G;
        else if (helix[2]) label = LABEL_I;
        else if (turn) label = LABEL_T;
        else if (bend) label = LABEL_S;
        codes[at] = (int8_t)(complete[at] != 0 ? label : LABEL_NONE);
    }
}

bool bad_slots(int A, int a, int b2, int c, int d) {
    const int s[4] = {a, b2, c, d};
    for (int k = 0; k < 4; ++k) {
        if (s[k] < 0 || s[k] >= A) return true;
        for (int l = 0; l < k; ++l)
            if (s[l] == s[k]) return true;
    }
    return false;
}

}  // namespace

extern "C" int ps_backbone_hbonds_f32(const float* xyz, const uint8_t* complete, const uint8_t* junction,
                                      const uint8_t* donor, int n_slot, int ca_slot, int c_slot, int o_slot,
                                      int32_t* acceptor_idx, float* acceptor_energy, int32_t* donor_idx,
                                      float* donor_energy, int B, int N, int A, void* stream) {
    if (!xyz || !complete || !junction || !acceptor_idx || !acceptor_energy || !donor_idx || !donor_energy || B < 0 || N < 0 ||
        A < 4 || B > 65535 || N > (1 << 24) || bad_slots(A, n_slot, ca_slot, c_slot, o_slot))
        return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0) return 0;
    return ps_launch(k_backbone_hbonds, dim3((unsigned)((N + OWNERS - 1) / OWNERS), (unsigned)B), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), xyz, complete, junction, donor,
                     slots_t{n_slot, ca_slot, c_slot, o_slot}, acceptor_idx, acceptor_energy, donor_idx, donor_energy, N, A);
}

extern "C" int ps_dssp_assign(const float* xyz, const uint8_t* complete, const uint8_t* junction, const int32_t* acceptor_idx,
                              int ca_slot, int8_t* codes, int B, int N, int A, void* stream) {
    if (!xyz || !complete || !junction || !acceptor_idx || !codes || B < 0 || N < 0 || A <= 0 || N > MAX_N ||
        (long long)B * N > (1ll << 31) || ca_slot < 0 || ca_slot >= A)
        return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0) return 0;
    return ps_launch(k_dssp_assign, dim3((unsigned)B), dim3(ASSIGN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz,
                     complete, junction, acceptor_idx, ca_slot, codes, N, A);
}
