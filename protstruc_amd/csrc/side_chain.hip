// K27 - K30 -- side-chain torsions: measure the chi angles of every residue, set them, and both gradients.
//
// The kernels know no amino acids.  A call brings two HOST tables, read and validated before it returns and handed to the
// kernel by value: chi_atoms (T,4,4), the four atom slots a, b, c, d of angle k of residue type t (all -1: no such angle),
// and, for the set step, chi_last (T,4): angle k turns the slots [d, last], -1: it is measured but never turned.
// residue_type (B,N) int32 selects the row; a value outside [0, T) is padding: no angles, and the table is not indexed.
// Angle k of a residue is DEFINED where the table has it and all four atoms are inside atom_mask (NULL = every atom).
// Coordinates under a false mask never reach arithmetic.
//
// All arithmetic is in double on the fp32 coordinates in the order written here (-ffp-contract=off is part of it), with
//   u x v = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)        u . v = (u.x*v.x + u.y*v.y) + u.z*v.z
//
// K27, ps_chi_f32:
//   b0 = a - b      b1 = c - b      b2 = d - c      n1 = b0 x b1      n2 = b2 x b1      m = n1 x n2
//   x = n1 . n2     y = (m . b1) / sqrt(b1 . b1)    chi = (float)atan2(y, x)         -- geometry.dihedral's sign, IUPAC
// exact 0 and mask 0 where the angle is undefined.
//
// K28, ps_chi_backward_f32: with p = (b0 . b1) / (b1 . b1), q = (b2 . b1) / (b1 . b1), l = sqrt(b1 . b1)
//   ga = (l / (n1 . n1)) n1      gd = -(l / (n2 . n2)) n2      gb = (p - 1) ga + q gd      gc = -(p ga) - (1 + q) gd
// each times (double)grad_chi[k]; an atom's contributions are summed in the order k = 0..3 and rounded once.  The lane
// writes its residue's whole (A,3) row: exact zeros in the slots no defined angle reads.
//
// K29, ps_chi_set_f32: for k = 0, 1, 2, 3 in this order, where angle k is defined, chi_last[t][k] >= 0 and chi_select is
// NULL or non-zero, on the residue's CURRENT coordinates (doubles between the steps):
//   delta = (double)chi[k] - phi, phi as in K27 without the rounding;  delta = (double)chi[k] if relative
//   e = c - b      u = e / sqrt(e . e)      cs = cos(delta)      sn = sin(delta)
//   for every present slot s in [d, last]:   v = p_s - c      p_s = ((c + v cs) + (u x v) sn) + u ((u . v) (1 - cs))
// rounded to fp32 once, at the store.  Every other float is the input's bit pattern (NaN of missing atoms, padding).
// How a lane does this without A*3 doubles of its own: the up to 16 table atoms of the turned angles live in registers
// and are carried through the four steps, which fixes the four rotations (c, u, cs, sn); then every covered slot is
// sent through the rotations that cover it, in the same order -- the same operations on the same values.
//
// K30, ps_chi_set_backward_f32, on the coordinates K29 wrote:
//   grad_chi[k] = sum over the present slots s in [d, last], in slot order, of (u x (p_s - c)) . g_s      u, c as above
// exact 0 where angle k was not turned.
//
// Layout.  One lane owns one residue; a workgroup is one wave and takes 64 consecutive residues.  A residue is A*3 floats
// (180 bytes at A = 15), so a lane's own row starts on no 16-byte boundary.  The two kernels that write a whole row per
// residue (K28, K29) stage the workgroup's contiguous span of the tensor through LDS: all lanes move it 16 bytes per lane
// from the first 16-byte boundary of the span's ACTUAL address (the up to three floats on either side are single
// accesses; nothing outside the span is touched); in LDS a row has an odd stride in floats (A*3, plus one where that is
// even), so the 32 lanes of a ds_read_b32 / ds_write_b32 group fall on 32 distinct banks; a lane works on its own row
// there, and the span goes back out the same way.  The two that only read a few atoms per residue and write 16 bytes (K27,
// K30) load those atoms where they lie.  Both forms of all four kernels were measured at B = 128, N = 512, A = 15
// (DESIGN.md section 4): staging won where a row is written (K29 29 against 40 us) and lost where it is not (K27 12
// against 10 us, K30 20 against 15 us).  The tables go through LDS (640 bytes), because lanes index them by their
// residue's type.  Offsets into the tensors are 64-bit.  No atomics anywhere: every result repeats bit for bit.
#include "ps_common.hpp"

#include <math.h>

#include "../../include/protstruc_hip.h"

namespace {

constexpr int THREADS = 64;
constexpr unsigned NONE = 0xFFu;            // a slot byte: no atom / never turned
constexpr unsigned NO_ANGLE = 0xFFFFFFFFu;  // the four slot bytes of an angle the type does not have

// The host tables of the call, by value in the kernel's arguments: four slot bytes a | b << 8 | c << 16 | d << 24 per
// (type, angle) and the four `last` bytes of a type in one word.
struct ChiTables {
    unsigned atoms[PS_CHI_MAX_TYPES * 4];
    unsigned last[PS_CHI_MAX_TYPES];
};

typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct d3 {
    double x, y, z;
};

__device__ __forceinline__ d3 subd(d3 a, d3 b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 addd(d3 a, d3 b) { return d3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ d3 scaled(d3 a, double s) { return d3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dotd(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ d3 crossd(d3 u, d3 v) {
    return d3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ __forceinline__ d3 loadd(const float* p) { return d3{(double)p[0], (double)p[1], (double)p[2]}; }

__device__ __forceinline__ double dihedral_d(d3 a, d3 b, d3 c, d3 d) {
    const d3 b0 = subd(a, b), b1 = subd(c, b), b2 = subd(d, c);
    const d3 n1 = crossd(b0, b1), n2 = crossd(b2, b1), m = crossd(n1, n2);
    return atan2(dotd(m, b1) / sqrt(dotd(b1, b1)), dotd(n1, n2));
}

// One turn: about the axis through c along the unit vector u by the angle whose cosine and sine are cs and sn.
struct turn_t {
    d3 c, u;
    double cs, sn;
};

__device__ __forceinline__ turn_t make_turn(d3 b, d3 c, double delta) {
    const d3 e = subd(c, b);
    const double l = sqrt(dotd(e, e));
    return turn_t{c, d3{e.x / l, e.y / l, e.z / l}, cos(delta), sin(delta)};
}

__device__ __forceinline__ d3 turned(const turn_t& t, d3 p) {
    const d3 v = subd(p, t.c);
    const double w = dotd(t.u, v) * (1.0 - t.cs);
    return addd(addd(addd(t.c, scaled(v, t.cs)), scaled(crossd(t.u, v), t.sn)), scaled(t.u, w));
}

// ---- a span of rows through LDS ------------------------------------------------------------------------------------------
// `n` floats at `g` (4-byte aligned), rows of L floats, to / from LDS rows of stride S >= L.  Element e of the span is
// lds[(e / L) * S + e % L].  All lanes of the workgroup take part.
__device__ __forceinline__ int span_head(const float* g, int n) {
    const int head = (int)((4u - (unsigned)((uintptr_t)g >> 2)) & 3u);
    return head < n ? head : n;
}

__device__ __forceinline__ void stage_in(const float* __restrict__ g, int n, int L, int S, float* lds) {
    const int t = threadIdx.x, head = span_head(g, n);
    const int body = (n - head) >> 2, tail = head + 4 * body;
    {   // at most three single floats on either side, by the first lanes
        const int e = t < head ? t : tail + (t - head);
        if (t < head || e < n) {
            const int r = e / L;
            lds[r * S + (e - r * L)] = g[e];
        }
    }
    for (int v = t; v < body; v += THREADS) {
        const int e = head + 4 * v;
        const f32x4_t x = *reinterpret_cast<const f32x4_t*>(g + e);
        int r = e / L, c = e - r * L;
        for (int i = 0; i < 4; ++i) {
            lds[r * S + c] = x[i];
            if (++c == L) {
                c = 0;
                ++r;
            }
        }
    }
}

__device__ __forceinline__ void stage_out(float* __restrict__ g, int n, int L, int S, const float* lds) {
    const int t = threadIdx.x, head = span_head(g, n);
    const int body = (n - head) >> 2, tail = head + 4 * body;
    {
        const int e = t < head ? t : tail + (t - head);
        if (t < head || e < n) {
            const int r = e / L;
            g[e] = lds[r * S + (e - r * L)];
        }
    }
    for (int v = t; v < body; v += THREADS) {
        const int e = head + 4 * v;
        f32x4_t x;
        int r = e / L, c = e - r * L;
        for (int i = 0; i < 4; ++i) {
            x[i] = lds[r * S + c];
            if (++c == L) {
                c = 0;
                ++r;
            }
        }
        *reinterpret_cast<f32x4_t*>(g + e) = x;
    }
}

// ---- what a lane knows about its residue -----------------------------------------------------------------------------------
struct residue_t {
    unsigned w[4];   // the slot bytes of the four angles, NO_ANGLE where undefined for THIS residue (table or mask)
    unsigned last;   // the four `last` bytes
};

__device__ __forceinline__ int slot_of(unsigned w, int j) { return (int)((w >> (8 * j)) & 0xFFu); }

__device__ __forceinline__ unsigned long long present_bits(const uint8_t* __restrict__ atom_mask, size_t r, int A) {
    if (!atom_mask) return ~0ull;
    unsigned long long bits = 0;
    for (int s = 0; s < A; ++s) bits |= (unsigned long long)(atom_mask[r * A + s] != 0) << s;
    return bits;
}

__device__ __forceinline__ residue_t residue_info(const int* __restrict__ residue_type, size_t r, int T,
                                                  unsigned long long bits, const unsigned* tab_atoms,
                                                  const unsigned* tab_last) {
    residue_t me;
    const int type = residue_type[r];
    const bool known = (unsigned)type < (unsigned)T;   // anything else is padding: the table is not indexed
    me.last = known ? tab_last[type] : 0xFFFFFFFFu;
    for (int k = 0; k < 4; ++k) {
        unsigned w = known ? tab_atoms[type * 4 + k] : NO_ANGLE;
        if (w != NO_ANGLE)
            for (int j = 0; j < 4; ++j)
                if (!((bits >> slot_of(w, j)) & 1ull)) w = NO_ANGLE;
        me.w[k] = w;
    }
    return me;
}

__device__ __forceinline__ void tables_to_lds(const ChiTables& tab, int T, unsigned* tab_atoms, unsigned* tab_last) {
    for (int i = threadIdx.x; i < T * 4; i += THREADS) tab_atoms[i] = tab.atoms[i];
    for (int i = threadIdx.x; i < T; i += THREADS) tab_last[i] = tab.last[i];
}

// The rows [r0, r0 + cnt) of this workgroup.
__device__ __forceinline__ int my_rows(size_t n_res, size_t& r0) {
    r0 = (size_t)blockIdx.x * THREADS;
    const size_t left = n_res - r0;
    return left < (size_t)THREADS ? (int)left : THREADS;
}

// The residue of this lane; false past the end.  The barrier orders the tables for every lane before any leaves.
__device__ __forceinline__ bool my_residue(const ChiTables& tab, int T, unsigned* tab_atoms, unsigned* tab_last, size_t n_res,
                                           size_t& r) {
    tables_to_lds(tab, T, tab_atoms, tab_last);
    __syncthreads();
    r = (size_t)blockIdx.x * THREADS + threadIdx.x;
    return r < n_res;
}

// ---- K27 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_chi(const float* __restrict__ xyz, const uint8_t* __restrict__ atom_mask,
                                                 const int* __restrict__ residue_type, const ChiTables tab, int T,
                                                 float* __restrict__ chi, uint8_t* __restrict__ chi_mask, size_t n_res,
                                                 int A) {
    __shared__ unsigned tab_atoms[PS_CHI_MAX_TYPES * 4], tab_last[PS_CHI_MAX_TYPES];
    size_t r;
    if (!my_residue(tab, T, tab_atoms, tab_last, n_res, r)) return;
    const float* row = xyz + r * (size_t)(A * 3);
    const residue_t me = residue_info(residue_type, r, T, present_bits(atom_mask, r, A), tab_atoms, tab_last);
    for (int k = 0; k < 4; ++k) {
        const unsigned w = me.w[k];
        float value = 0.0f;
        if (w != NO_ANGLE && chi)
            value = (float)dihedral_d(loadd(row + 3 * slot_of(w, 0)), loadd(row + 3 * slot_of(w, 1)),
                                      loadd(row + 3 * slot_of(w, 2)), loadd(row + 3 * slot_of(w, 3)));
        if (chi) chi[r * 4 + k] = value;
        if (chi_mask) chi_mask[r * 4 + k] = w != NO_ANGLE;
    }
}

// ---- K28 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_chi_backward(const float* __restrict__ xyz,
                                                          const uint8_t* __restrict__ atom_mask,
                                                          const int* __restrict__ residue_type, const ChiTables tab, int T,
                                                          const float* __restrict__ grad_chi, float* __restrict__ grad_xyz,
                                                          size_t n_res, int A, int S) {
    extern __shared__ float span[];
    __shared__ unsigned tab_atoms[PS_CHI_MAX_TYPES * 4], tab_last[PS_CHI_MAX_TYPES];
    const int L = A * 3, t = threadIdx.x;
    size_t r0;
    const int cnt = my_rows(n_res, r0);
    tables_to_lds(tab, T, tab_atoms, tab_last);
    stage_in(xyz + r0 * L, cnt * L, L, S, span);
    __syncthreads();
    if (t < cnt) {
        const size_t r = r0 + t;
        float* row = span + t * S;
        const residue_t me = residue_info(residue_type, r, T, present_bits(atom_mask, r, A), tab_atoms, tab_last);
        d3 G[4][4];   // the contribution of angle k to its atom j
        for (int k = 0; k < 4; ++k) {
            const unsigned w = me.w[k];
            for (int j = 0; j < 4; ++j) G[k][j] = d3{0.0, 0.0, 0.0};
            if (w == NO_ANGLE) continue;   // grad_chi is not read here
            const d3 a = loadd(row + 3 * slot_of(w, 0)), b = loadd(row + 3 * slot_of(w, 1)),
                     c = loadd(row + 3 * slot_of(w, 2)), d = loadd(row + 3 * slot_of(w, 3));
            const d3 b0 = subd(a, b), b1 = subd(c, b), b2 = subd(d, c);
            const d3 n1 = crossd(b0, b1), n2 = crossd(b2, b1);
            const double l2 = dotd(b1, b1), l = sqrt(l2);
            const double p = dotd(b0, b1) / l2, q = dotd(b2, b1) / l2;
            const d3 ga = scaled(n1, l / dotd(n1, n1)), gd = scaled(n2, -(l / dotd(n2, n2)));
            const d3 gb = addd(scaled(ga, p - 1.0), scaled(gd, q));
            const d3 pa = scaled(ga, p), qd = scaled(gd, 1.0 + q);
            const d3 gc = d3{-pa.x - qd.x, -pa.y - qd.y, -pa.z - qd.z};
            const double g = (double)grad_chi[r * 4 + k];
            G[k][0] = scaled(ga, g);
            G[k][1] = scaled(gb, g);
            G[k][2] = scaled(gc, g);
            G[k][3] = scaled(gd, g);
        }
        // every coordinate this lane needs is in registers now: its row becomes the gradient's
        for (int e = 0; e < L; ++e) row[e] = 0.0f;
        for (int k = 0; k < 4; ++k) {
            if (me.w[k] == NO_ANGLE) continue;
            for (int j = 0; j < 4; ++j) {
                const int s = slot_of(me.w[k], j);
                bool first = true;   // an earlier angle with this atom has written the sum already
                for (int k2 = 0; k2 < k; ++k2)
                    for (int j2 = 0; j2 < 4; ++j2)
                        if (me.w[k2] != NO_ANGLE && slot_of(me.w[k2], j2) == s) first = false;
                if (!first) continue;
                d3 sum = G[k][j];
                for (int k2 = k + 1; k2 < 4; ++k2)
                    for (int j2 = 0; j2 < 4; ++j2)
                        if (me.w[k2] != NO_ANGLE && slot_of(me.w[k2], j2) == s) sum = addd(sum, G[k2][j2]);
                row[3 * s] = (float)sum.x;
                row[3 * s + 1] = (float)sum.y;
                row[3 * s + 2] = (float)sum.z;
            }
        }
    }
    __syncthreads();
    stage_out(grad_xyz + r0 * L, cnt * L, L, S, span);
}

// Which angles of the residue K29 turns: defined, with a range, and selected.
__device__ __forceinline__ void turned_angles(const residue_t& me, const uint8_t* __restrict__ chi_select, size_t r,
                                              bool (&turn)[4], int (&lo)[4], int (&hi)[4]) {
    for (int k = 0; k < 4; ++k) {
        lo[k] = slot_of(me.w[k], 3);
        hi[k] = slot_of(me.last, k);
        turn[k] = me.w[k] != NO_ANGLE && (unsigned)hi[k] != NONE && (!chi_select || chi_select[r * 4 + k] != 0);
    }
}

// ---- K29 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_chi_set(const float* __restrict__ xyz, const uint8_t* __restrict__ atom_mask,
                                                     const int* __restrict__ residue_type, const ChiTables tab, int T,
                                                     const float* __restrict__ chi, const uint8_t* __restrict__ chi_select,
                                                     int relative, float* __restrict__ out, size_t n_res, int A, int S) {
    extern __shared__ float span[];
    __shared__ unsigned tab_atoms[PS_CHI_MAX_TYPES * 4], tab_last[PS_CHI_MAX_TYPES];
    const int L = A * 3, t = threadIdx.x;
    size_t r0;
    const int cnt = my_rows(n_res, r0);
    tables_to_lds(tab, T, tab_atoms, tab_last);
    stage_in(xyz + r0 * L, cnt * L, L, S, span);
    __syncthreads();
    if (t < cnt) {
        const size_t r = r0 + t;
        float* row = span + t * S;
        const unsigned long long bits = present_bits(atom_mask, r, A);
        const residue_t me = residue_info(residue_type, r, T, bits, tab_atoms, tab_last);
        bool turn[4];
        int lo[4], hi[4];
        turned_angles(me, chi_select, r, turn, lo, hi);
        if (turn[0] || turn[1] || turn[2] || turn[3]) {
            d3 P[4][4];   // the table atoms of the turned angles, carried through the steps in double
            #pragma unroll
            for (int k = 0; k < 4; ++k)
                #pragma unroll
                for (int j = 0; j < 4; ++j)
                    P[k][j] = turn[k] ? loadd(row + 3 * slot_of(me.w[k], j)) : d3{0.0, 0.0, 0.0};
            turn_t rot[4];
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                rot[k] = turn_t{d3{0.0, 0.0, 0.0}, d3{0.0, 0.0, 0.0}, 1.0, 0.0};
                if (!turn[k]) continue;   // chi is not read here
                double delta = (double)chi[r * 4 + k];
                if (!relative) delta -= dihedral_d(P[k][0], P[k][1], P[k][2], P[k][3]);
                rot[k] = make_turn(P[k][1], P[k][2], delta);
                #pragma unroll
                for (int k2 = k; k2 < 4; ++k2)
                    #pragma unroll
                    for (int j2 = 0; j2 < 4; ++j2) {
                        const int s = slot_of(me.w[k2], j2);
                        if (turn[k2] && s >= lo[k] && s <= hi[k]) P[k2][j2] = turned(rot[k], P[k2][j2]);
                    }
            }
            for (int s = 0; s < A; ++s) {
                if (!((bits >> s) & 1ull)) continue;
                bool covered = false;
                #pragma unroll
                for (int k = 0; k < 4; ++k) covered = covered || (turn[k] && s >= lo[k] && s <= hi[k]);
                if (!covered) continue;
                d3 p = loadd(row + 3 * s);
                #pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (turn[k] && s >= lo[k] && s <= hi[k]) p = turned(rot[k], p);
                row[3 * s] = (float)p.x;
                row[3 * s + 1] = (float)p.y;
                row[3 * s + 2] = (float)p.z;
            }
        }
    }
    __syncthreads();
    stage_out(out + r0 * L, cnt * L, L, S, span);
}

// ---- K30 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_chi_set_backward(const float* __restrict__ out,
                                                              const uint8_t* __restrict__ atom_mask,
                                                              const int* __restrict__ residue_type, const ChiTables tab,
                                                              int T, const uint8_t* __restrict__ chi_select,
                                                              const float* __restrict__ grad_out,
                                                              float* __restrict__ grad_chi, size_t n_res, int A) {
    __shared__ unsigned tab_atoms[PS_CHI_MAX_TYPES * 4], tab_last[PS_CHI_MAX_TYPES];
    size_t r;
    if (!my_residue(tab, T, tab_atoms, tab_last, n_res, r)) return;
    const float *row = out + r * (size_t)(A * 3), *grow = grad_out + r * (size_t)(A * 3);
    const unsigned long long bits = present_bits(atom_mask, r, A);
    const residue_t me = residue_info(residue_type, r, T, bits, tab_atoms, tab_last);
    bool turn[4];
    int lo[4], hi[4];
    turned_angles(me, chi_select, r, turn, lo, hi);
    for (int k = 0; k < 4; ++k) {
        double sum = 0.0;
        if (turn[k]) {
            const d3 b = loadd(row + 3 * slot_of(me.w[k], 1)), c = loadd(row + 3 * slot_of(me.w[k], 2));
            const d3 e = subd(c, b);
            const double l = sqrt(dotd(e, e));
            const d3 u = d3{e.x / l, e.y / l, e.z / l};
            for (int s = lo[k]; s <= hi[k]; ++s)
                if ((bits >> s) & 1ull) sum += dotd(crossd(u, subd(loadd(row + 3 * s), c)), loadd(grow + 3 * s));
        }
        grad_chi[r * 4 + k] = (float)sum;
    }
}

// ---- the host side -------------------------------------------------------------------------------------------------------
bool bad_shape(int B, int N, int A) {
    return B < 0 || N < 0 || A < 1 || A > 64 || (size_t)B * (size_t)N > ((size_t)1 << 31);
}

// Validate the tables and pack them; chi_last NULL: nothing is ever turned (K27, K28).
bool bad_tables(const int32_t* chi_atoms, const int32_t* chi_last, int T, int A, ChiTables& tab) {
    if (!chi_atoms || T < 1 || T > PS_CHI_MAX_TYPES) return true;
    for (int t = 0; t < T; ++t) {
        unsigned lasts = 0;
        for (int k = 0; k < 4; ++k) {
            const int32_t* s = chi_atoms + (t * 4 + k) * 4;
            const int32_t last = chi_last ? chi_last[t * 4 + k] : -1;
            unsigned w = NO_ANGLE;
            if (!(s[0] == -1 && s[1] == -1 && s[2] == -1 && s[3] == -1)) {
                w = 0;
                for (int j = 0; j < 4; ++j) {
                    if (s[j] < 0 || s[j] >= A) return true;
                    for (int i = 0; i < j; ++i)
                        if (s[i] == s[j]) return true;
                    w |= (unsigned)s[j] << (8 * j);
                }
            }
            if (last != -1) {
                if (w == NO_ANGLE || last < s[3] || last >= A) return true;
                for (int j = 0; j < 3; ++j)
                    if (s[j] >= s[3] && s[j] <= last) return true;
            }
            tab.atoms[t * 4 + k] = w;
            lasts |= (last == -1 ? NONE : (unsigned)last) << (8 * k);
        }
        tab.last[t] = lasts;
    }
    return false;
}

// The LDS stride of a staged row, odd, and the bytes of a workgroup's THREADS rows: 49408 at A = 64, under the 64 KB a
// workgroup may have together with the tables.
void plan(int A, int& S, size_t& lds) {
    S = (A * 3) | 1;
    lds = (size_t)THREADS * S * sizeof(float);
}

unsigned blocks(size_t n_res) { return (unsigned)((n_res + THREADS - 1) / THREADS); }

}  // namespace

extern "C" int ps_chi_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* residue_type,
                          const int32_t* chi_atoms, int T, float* chi, uint8_t* chi_mask, int B, int N, int A,
                          void* stream) {
    ChiTables tab = {};
    if (!xyz || !residue_type || (!chi && !chi_mask) || bad_shape(B, N, A) || bad_tables(chi_atoms, nullptr, T, A, tab))
        return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    return ps_launch(k_chi, dim3(blocks(n_res)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz,
                     atom_mask, residue_type, tab, T, chi, chi_mask, n_res, A);
}

extern "C" int ps_chi_backward_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* residue_type,
                                   const int32_t* chi_atoms, int T, const float* grad_chi, float* grad_xyz, int B, int N,
                                   int A, void* stream) {
    ChiTables tab = {};
    if (!xyz || !residue_type || !grad_chi || !grad_xyz || bad_shape(B, N, A) ||
        bad_tables(chi_atoms, nullptr, T, A, tab))
        return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    int S;
    size_t lds;
    plan(A, S, lds);
    return ps_launch(k_chi_backward, dim3(blocks(n_res)), dim3(THREADS), lds, reinterpret_cast<hipStream_t>(stream),
                     xyz, atom_mask, residue_type, tab, T, grad_chi, grad_xyz, n_res, A, S);
}

extern "C" int ps_chi_set_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* residue_type,
                              const int32_t* chi_atoms, const int32_t* chi_last, int T, const float* chi,
                              const uint8_t* chi_select, int relative, float* out, int B, int N, int A, void* stream) {
    ChiTables tab = {};
    if (!xyz || !residue_type || !chi_last || !chi || !out || out == xyz || bad_shape(B, N, A) ||
        bad_tables(chi_atoms, chi_last, T, A, tab))
        return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    int S;
    size_t lds;
    plan(A, S, lds);
    return ps_launch(k_chi_set, dim3(blocks(n_res)), dim3(THREADS), lds, reinterpret_cast<hipStream_t>(stream), xyz,
                     atom_mask, residue_type, tab, T, chi, chi_select, relative, out, n_res, A, S);
}

extern "C" int ps_chi_set_backward_f32(const float* out, const uint8_t* atom_mask, const int32_t* residue_type,
                                       const int32_t* chi_atoms, const int32_t* chi_last, int T,
                                       const uint8_t* chi_select, const float* grad_out, float* grad_chi, int B, int N,
                                       int A, void* stream) {
    ChiTables tab = {};
    if (!out || !residue_type || !chi_last || !grad_out || !grad_chi || bad_shape(B, N, A) ||
        bad_tables(chi_atoms, chi_last, T, A, tab))
        return (int)hipErrorInvalidValue;
    const size_t n_res = (size_t)B * N;
    if (n_res == 0) return 0;
    return ps_launch(k_chi_set_backward, dim3(blocks(n_res)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), out, atom_mask, residue_type, tab, T, chi_select, grad_out,
                     grad_chi, n_res, A);
}
