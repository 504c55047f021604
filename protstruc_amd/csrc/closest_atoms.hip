// K31 / K32 -- the closest atoms of every residue pair, and the gradient of their distance.
//
// Inputs: xyz (B,N,A,3) fp32; atom_mask (B,N,A) uint8, NULL = every slot is present; cutoff, a float, +inf allowed.
// For structure b and residues i <= j, over every present atom a of i and present atom c of j:
//
//   X = (double)x      dx = Xjc.x - Xia.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz     in double, in this order
//
// -- K24's distance; the build's -ffp-contract=off is part of the definition.
//   * pairs whose d2 is not finite are skipped;
//   * the winner is the minimum under the order (d2, a, c) ascending: ties go to the lower a, then to the lower c;
//   * with C2 = (double)cutoff * (double)cutoff the pair counts iff d2 <= C2;
//   * dist[b,i,j] = (float)sqrt(d2)      pair[b,i,j] = a * A + c   as int16;
//   * dist = +inf and pair = -1 where no atom pair counts: a residue without a present atom, a cutoff that excludes every
//     pair, every d2 non-finite;
//   * entry (j,i) is the MIRROR of (i,j): the same dist bits and pair[b,j,i] = c * A + a, so pair[b,r,s] always reads
//     "atom of the row residue, atom of the column residue".  Both planes are exactly symmetric, and only i <= j is computed;
//   * the diagonal is not special: a residue with a present atom gets 0.0 and a0 * A + a0 for its lowest present slot;
//   * a masked slot's floats (NaN, inf, anything) never influence an output;
//   * refused with hipErrorInvalidValue before any launch: A outside 1 .. 64, N outside 1 .. 2^20, B outside 0 .. 65535,
//     a negative or NaN cutoff.  B = 0 returns 0 without touching a device.  Offsets are 64-bit.
//
// Gradient (K32): xyz gets one, and it flows to the recorded pair only.  For residue i and slot a
//
//   grad_xyz[b,i,a,:] = sum over j != i with pair[b,i,j] = a*A + c  of  ((double)g[b,i,j] + (double)g[b,j,i]) (Xia - Xjc) / sqrt(d2)
//
// over j ascending, in double, rounded to float once; d2 is recomputed from the coordinates; a term with pair outside
// [0, A*A) (one unsigned compare, before any address is formed), or with d2 equal to 0 or non-finite, contributes nothing;
// slots that win no pair get exact zeros, masked ones included.  K32 reads xyz, pair and grad_dist, and nothing else.
//
// ---- K31, the sweep.  A workgroup of WAVES waves takes one tile of TS row residues against one tile of TS column
// residues with j-tile >= i-tile (the structure on grid.y).  While staging, 2 * TS threads each take one residue of the
// two tiles: its presence word (one 64-bit mask: bit a = slot a is present), its centre (the middle of the bounding box
// of the present atoms) and its radius; the column residues' atoms go to LDS atom-major, col[xyz][c][j], so that a
// wave's read of one slot is TS consecutive words, with zeros in the absent slots (a masked float never reaches LDS).
// A wave owns one row residue at a time: the residue's presence word is wave-uniform, the loop over its atoms a is a
// scalar loop and the atom's coordinates are one scalar read; the lanes are the column residues.  Each lane keeps its
// running (d2min, a, c) in registers; the columns arrive in ascending (a, c), so "strictly less" is the tie rule, and a
// NaN or infinite d2 is never strictly less than the +inf the minimum starts from.  In the diagonal tile only the lanes
// j >= i work.
//
// A finite cutoff buys skipping.  By the triangle inequality no atom of i is within the cutoff of an atom of j when
// |ci - cj| > cutoff + Ri + Rj, with c the centres and R the radii.  The test is made in fp32 and is strictly conservative:
//   R  = sqrt(max_a fl32|x_a - c|^2) * (1 + 2^-20) + 2^-70      S = fl32(fl32(cutoff + Ri) + Rj) * (1 + 2^-20)
//   skip iff  fl32|ci - cj|^2 > fl32(S * S) * (1 + 2^-19) + 2^-100
// An fp32 squared distance carries five roundings of 2^-24 relative, its square root one more: 1 + 2^-20 = 1 + 16 * 2^-24
// covers them thrice over, so R bounds the true radius from above (the 2^-70 covers a squared radius that underflowed,
// which errs by at most 3 * 2^-149, i.e. 2^-73 in the radius), and S the true sum (two roundings).  On the left the true
// squared distance of the centres is at least the fp32 one times (1 - 6 * 2^-24) less 3 * 2^-149; on the right the product
// loses one rounding, so the factor 1 + 32 * 2^-24 leaves 25 roundings of slack and 2^-100 swallows every underflow.  A
// residue with a NaN or infinite present coordinate has R = +inf (the maximum propagates NaN), so S and the bound are +inf
// and nothing is skipped; an overflow on the left only happens where the true distance exceeds every finite bound.  A
// lane whose test says "skip" takes no part in the pair loop, and a wave whose lanes all skip drops the row's whole loop
// by one ballot.  The decision itself stays in double (d2 <= C2 on the minimum), so the skip never changes a bit.
// Whether a per-pair fp32 pre-test against the running minimum pays at cutoff = inf has not been measured; there is none.
//
// The tile's results go to LDS (dist as float, the pair as a << 8 | c) and are written twice: rows of the tile straight
// and -- off the diagonal -- transposed, the pair with a and c exchanged; the diagonal tile's lower triangle is the mirror
// of its upper one.  Sixteen lanes write one row segment: single elements up to the first 16-byte boundary of the actual
// address, 16-byte stores from there, single elements for the rest (store_run), so any element-aligned output is legal.
// A <= 32 runs with TS = 64; A <= 64 with TS = 32 (half the lanes idle), which keeps the staged columns at 24 KB.
//
// ---- K32.  A workgroup is one wave; OWN of its lanes own one residue i each and walk j ascending, in tiles of 32.  Row i
// of pair and of g and column i of g arrive through LDS: the (i-tile, j-tile) blocks of pair and g and the (j-tile, i-tile)
// block of g are read coalesced along their rows, the latter transposed in LDS (row stride 33 words: no bank conflicts).
// The A * 3 double accumulators of a lane live in LDS as acc[slot * 3 + xyz][lane] -- the slot is data-dependent --, which
// a wave reads and writes without conflicts whatever slots its lanes are at.  OWN = 64 up to A = 28 and 32 above, which
// keeps a workgroup within 64 KB.  No atomics, one fixed order: both kernels repeat bit for bit.
#include "ps_common.hpp"
#include "owner_sweep.hpp"   // WAVES

#include <math.h>

#include "../../include/protstruc_contacts.h"

namespace {

constexpr int THREADS = PS_WAVE * WAVES;
constexpr int ROW_LANES = 16;          // lanes that write one row segment of a tile
constexpr unsigned NONE = 0xFFFFu;     // the pair code of "no atom pair counts"

// Write out[0 .. total) = value(0 .. total) with `lanes` lanes (sub = this lane's index among them): single elements up
// to the first 16-byte boundary of `out`, 16 bytes per lane from there, single elements for the rest.  K24's store_span
// for any element size -- eight int16 make a 16-byte store -- and for a part of the wave.
template <typename T, typename F>
__device__ __forceinline__ void store_run(T* __restrict__ out, int total, int sub, int lanes, F value) {
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T TV __attribute__((ext_vector_type(VEC)));
    int head = (int)(((16u - (unsigned)((uintptr_t)out & 15u)) & 15u) / (unsigned)sizeof(T));
    head = head < total ? head : total;
    for (int e = sub; e < head; e += lanes) out[e] = value(e);
    const int body = (total - head) / VEC;
    for (int v = sub; v < body; v += lanes) {
        const int e = head + VEC * v;
        TV x;
#pragma unroll
        for (int q = 0; q < VEC; ++q) x[q] = value(e + q);
        *reinterpret_cast<TV*>(out + e) = x;
    }
    for (int e = head + VEC * body + sub; e < total; e += lanes) out[e] = value(e);
}

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ short pair_out(unsigned code, int A, bool exchanged) {
    const int a = (int)(code >> 8), c = (int)(code & 0xFFu);
    return code == NONE ? (short)-1 : (short)(exchanged ? c * A + a : a * A + c);
}

template <int AB, int TS>
__global__ __launch_bounds__(THREADS) void closest_atoms(const float* __restrict__ xyz, const uint8_t* __restrict__ atom_mask,
                                                         float* __restrict__ dist, int16_t* __restrict__ pair, int N, int A,
                                                         int T, float cutoff, double C2) {
    constexpr int RPW = TS / WAVES;       // row residues per wave
    constexpr int DS = TS + 1;            // row stride of the dist tile in words: a column read has no bank conflict
    constexpr int PS = TS + 2;            // row stride of the pair tile in halfwords (an odd number of words)
    static_assert(TS <= PS_WAVE && RPW % (PS_WAVE / ROW_LANES) == 0 && 2 * TS <= THREADS, "tile");
    __shared__ float col[3][AB][TS];
    __shared__ unsigned long long cmask[TS], rmask[TS];
    __shared__ float4 cball[TS], rball[TS];     // centre and radius
    __shared__ float od[TS * DS];
    __shared__ unsigned short op[TS * PS];
    const int it = blockIdx.x / T, jt = blockIdx.x - it * T;
    if (jt < it) return;
    const size_t b = blockIdx.y;
    const int i0 = it * TS, j0 = jt * TS;
    const bool diag = it == jt;
    const bool skipping = cutoff < __builtin_huge_valf();

    if (threadIdx.x < 2 * TS) {   // one residue per thread: the column tile's, then the row tile's
        const bool is_row = threadIdx.x >= TS;
        const int r = threadIdx.x - (is_row ? TS : 0);
        const int res = (is_row ? i0 : j0) + r;
        const size_t at = (b * N + (res < N ? res : 0)) * (size_t)A;
        unsigned long long present = 0ull;
        const float big = __builtin_huge_valf();
        float lox = big, loy = big, loz = big, hix = -big, hiy = -big, hiz = -big;
        for (int a = 0; a < A; ++a) {
            const bool here = res < N && (!atom_mask || atom_mask[at + a] != 0);
            f3 x = f3{0.0f, 0.0f, 0.0f};
            if (here) {
                x = load3(xyz + (at + a) * 3);
                present |= 1ull << a;
                lox = fminf(lox, x.x), loy = fminf(loy, x.y), loz = fminf(loz, x.z);
                hix = fmaxf(hix, x.x), hiy = fmaxf(hiy, x.y), hiz = fmaxf(hiz, x.z);
            }
            if (!is_row) col[0][a][r] = x.x, col[1][a][r] = x.y, col[2][a][r] = x.z;
        }
        float4 ball = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (skipping && present) {
            ball.x = 0.5f * (lox + hix), ball.y = 0.5f * (loy + hiy), ball.z = 0.5f * (loz + hiz);
            float rr = 0.0f;
            for (int a = 0; a < A; ++a) {
                if (!((present >> a) & 1ull)) continue;
                const f3 x = load3(xyz + (at + a) * 3);
                const float ex = x.x - ball.x, ey = x.y - ball.y, ez = x.z - ball.z;
                const float e2 = (ex * ex + ey * ey) + ez * ez;
                rr = (e2 > rr || e2 != e2) ? e2 : rr;      // a maximum that keeps NaN
            }
            ball.w = (rr == rr && rr < big) ? sqrtf(rr) * (1.0f + 0x1p-20f) + 0x1p-70f : big;
        }
        (is_row ? rmask : cmask)[r] = present;
        (is_row ? rball : cball)[r] = ball;
    }
    __syncthreads();

    const int lane = threadIdx.x & (PS_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / PS_WAVE));
    const int j = j0 + lane;
    const bool column = lane < TS && j < N;
    const unsigned long long my_slots = column ? cmask[lane] : 0ull;
    const float4 mine = column ? cball[lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < RPW; ++k) {
        const int r = wave * RPW + k, i = i0 + r;   // wave-uniform
        if (i >= N) break;
        const unsigned long long row_slots = uniform64(rmask[r]);
        unsigned long long slots = (diag && j < i) ? 0ull : my_slots;
        if (skipping) {
            const float4 o = rball[r];
            const float ex = mine.x - o.x, ey = mine.y - o.y, ez = mine.z - o.z;
            const float s = ((cutoff + o.w) + mine.w) * (1.0f + 0x1p-20f);
            if ((ex * ex + ey * ey) + ez * ez > (s * s) * (1.0f + 0x1p-19f) + 0x1p-100f) slots = 0ull;
        }
        double best = (double)INFINITY;
        int best_a = 0, best_c = 0;
        if (row_slots != 0ull && __ballot(slots != 0ull) != 0ull) {
            unsigned long long any = 0ull;     // the slots some lane of the wave still has
            for (int c = 0; c < A; ++c)
                if (__ballot((slots >> c) & 1ull) != 0ull) any |= 1ull << c;
            const float* __restrict__ row = xyz + (b * N + i) * (size_t)A * 3;
            for (unsigned long long ra = row_slots; ra != 0ull; ra &= ra - 1ull) {
                const int a = __builtin_ctzll(ra);
                const double xa = (double)row[3 * a], ya = (double)row[3 * a + 1], za = (double)row[3 * a + 2];
                for (unsigned long long rc = any; rc != 0ull; rc &= rc - 1ull) {
                    const int c = __builtin_ctzll(rc);
                    const double dx = (double)col[0][c][lane & (TS - 1)] - xa, dy = (double)col[1][c][lane & (TS - 1)] - ya,
                                 dz = (double)col[2][c][lane & (TS - 1)] - za;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (((slots >> c) & 1ull) && d2 < best) {
                        best = d2;
                        best_a = a;
                        best_c = c;
                    }
                }
            }
        }
        if (lane < TS) {
            const bool counts = best < (double)INFINITY && best <= C2;
            od[r * DS + lane] = counts ? (float)sqrt(best) : INFINITY;
            op[r * PS + lane] = (unsigned short)(counts ? (unsigned)(best_a << 8 | best_c) : NONE);
        }
    }
    __syncthreads();

    const int rows = N - i0 < TS ? N - i0 : TS, cols = N - j0 < TS ? N - j0 : TS;
    const int sub = lane & (ROW_LANES - 1), group = lane / ROW_LANES;
    for (int k = 0; k < RPW; k += PS_WAVE / ROW_LANES) {
        const int r = wave * RPW + k + group;
        if (r < rows) {      // row i0 + r of the outputs, columns j0 .. j0 + cols
            const size_t first = (b * N + i0 + r) * (size_t)N + j0;
            store_run(dist + first, cols, sub, ROW_LANES,
                      [&](int e) { return diag && e < r ? od[e * DS + r] : od[r * DS + e]; });
            store_run(pair + first, cols, sub, ROW_LANES, [&](int e) {
                return diag && e < r ? pair_out(op[e * PS + r], A, true) : pair_out(op[r * PS + e], A, false);
            });
        }
        if (!diag && r < cols) {   // the mirror: row j0 + r, columns i0 .. i0 + rows
            const size_t first = (b * N + j0 + r) * (size_t)N + i0;
            store_run(dist + first, rows, sub, ROW_LANES, [&](int e) { return od[e * DS + r]; });
            store_run(pair + first, rows, sub, ROW_LANES, [&](int e) { return pair_out(op[e * PS + r], A, true); });
        }
    }
}

constexpr int JT = 32;            // K32: column residues per tile
constexpr int GS = JT + 1;        // row stride of the g tiles in words
constexpr int QS = JT + 2;        // row stride of the pair tile in halfwords

__host__ __device__ constexpr size_t backward_lds_bytes(int own, int A) {
    return (size_t)A * 3 * own * sizeof(double) + (size_t)own * (2 * GS * sizeof(float) + QS * sizeof(short));
}

template <int OWN>
__global__ __launch_bounds__(PS_WAVE) void closest_atoms_backward(const float* __restrict__ xyz, const int16_t* __restrict__ pair,
                                                                  const float* __restrict__ g, float* __restrict__ grad_xyz,
                                                                  int N, int A) {
    extern __shared__ __attribute__((aligned(16))) double closest_lds[];
    double* acc = closest_lds;                                            // [slot * 3 + xyz][owner]
    float* g_row = reinterpret_cast<float*>(acc + (size_t)A * 3 * OWN);   // [owner][column]: g[b, i, j]
    float* g_col = g_row + OWN * GS;                                      // [owner][column]: g[b, j, i]
    short* p_row = reinterpret_cast<short*>(g_col + OWN * GS);            // [owner][column]: pair[b, i, j]
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x;
    const int i0 = blockIdx.x * OWN, i = i0 + lane;
    const int rows = N - i0 < OWN ? N - i0 : OWN;
    const bool owner = lane < rows;
    const unsigned AA = (unsigned)(A * A);
    const int width = A * 3;
    for (int e = lane; e < width * OWN; e += PS_WAVE) acc[e] = 0.0;
    const float* __restrict__ mine = xyz + (b * N + (owner ? i : 0)) * (size_t)width;

    for (int j0 = 0; j0 < N; j0 += JT) {
        const int cols = N - j0 < JT ? N - j0 : JT;
        __syncthreads();   // the previous tile's readers are done (and, the first time, acc is zero)
        for (int t = lane; t < OWN * JT; t += PS_WAVE) {
            const int r = t / JT, s = t % JT;              // along the rows of pair and g
            if (r < rows && s < cols) {
                const size_t at = (b * N + i0 + r) * (size_t)N + j0 + s;
                g_row[r * GS + s] = g[at];
                p_row[r * QS + s] = pair[at];
            }
            const int s2 = t / OWN, r2 = t % OWN;          // along the rows of g again: its (j-tile, i-tile) block
            if (r2 < rows && s2 < cols) g_col[r2 * GS + s2] = g[(b * N + j0 + s2) * (size_t)N + i0 + r2];
        }
        __syncthreads();
        if (!owner) continue;
        for (int s = 0; s < cols; ++s) {
            const int j = j0 + s;
            const unsigned p = (unsigned)(int)p_row[lane * QS + s];
            if (p >= AA || j == i) continue;               // "none" and every value out of range: before any address
            const unsigned a = p / (unsigned)A, c = p - a * (unsigned)A;
            const float* __restrict__ xa = mine + 3 * a;
            const float* __restrict__ xc = xyz + ((b * N + j) * (size_t)A + c) * 3;
            const double ax = (double)xa[0], ay = (double)xa[1], az = (double)xa[2];
            const double dx = (double)xc[0] - ax, dy = (double)xc[1] - ay, dz = (double)xc[2] - az;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 > 0.0 && d2 < (double)INFINITY)) continue;
            const double w = ((double)g_row[lane * GS + s] + (double)g_col[lane * GS + s]) / sqrt(d2);
            double* mine_acc = acc + (size_t)(3 * a) * OWN + lane;
            mine_acc[0] -= w * dx;                         // Xia - Xjc = -d
            mine_acc[OWN] -= w * dy;
            mine_acc[2 * OWN] -= w * dz;
        }
    }
    __syncthreads();
    // the workgroup's rows are one contiguous span of grad_xyz: element e is float e % width of its residue e / width
    store_run(grad_xyz + (b * N + i0) * (size_t)width, rows * width, lane, PS_WAVE,
              [=](int e) { return (float)acc[(e % width) * OWN + e / width]; });
}

bool bad_shape(int B, int N, int A) {
    return B < 0 || B > 65535 || N < 1 || N > PS_CLOSEST_MAX_RESIDUES || A < 1 || A > PS_CLOSEST_MAX_ATOMS;
}

}  // namespace

extern "C" int ps_contacts_api(void) { return PS_CONTACTS_API; }

extern "C" int ps_closest_atoms_f32(const float* xyz, const uint8_t* atom_mask, float* dist, int16_t* pair, int B, int N, int A,
                                    float cutoff, void* stream) {
    if (bad_shape(B, N, A) || !(cutoff >= 0.0f)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !dist || !pair) return (int)hipErrorInvalidValue;
    const double C2 = (double)cutoff * (double)cutoff;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const auto launch = [&](auto kernel, int ts) {
        const int T = (N + ts - 1) / ts;      // at most 2^15, so T * T fits grid.x
        return ps_launch(kernel, dim3((unsigned)T * (unsigned)T, (unsigned)B), dim3(THREADS), 0, s, xyz, atom_mask, dist, pair,
                         N, A, T, cutoff, C2);
    };
    if (A <= 16) return launch(closest_atoms<16, 64>, 64);
    if (A <= 32) return launch(closest_atoms<32, 64>, 64);
    return launch(closest_atoms<64, 32>, 32);
}

extern "C" int ps_closest_atoms_backward_f32(const float* xyz, const int16_t* pair, const float* grad_dist, float* grad_xyz,
                                             int B, int N, int A, void* stream) {
    if (bad_shape(B, N, A)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !pair || !grad_dist || !grad_xyz) return (int)hipErrorInvalidValue;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const auto launch = [&](auto kernel, int own) {
        return ps_launch(kernel, dim3((unsigned)((N + own - 1) / own), (unsigned)B), dim3(PS_WAVE), backward_lds_bytes(own, A),
                         s, xyz, pair, grad_dist, grad_xyz, N, A);
    };
    static_assert(backward_lds_bytes(64, 28) <= 65536 && backward_lds_bytes(32, PS_CLOSEST_MAX_ATOMS) <= 65536, "64 KB");
    if (A <= 28) return launch(closest_atoms_backward<64>, 64);
    return launch(closest_atoms_backward<32>, 32);
}
