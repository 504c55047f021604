// The chain of the seeded superposition search (K39, include/protstruc_superpose.h) as one wave runs it, with the seed
// table it starts from: shared by superpose.hip (K39 itself) and struct_align.hip (K42, whose fit-search runs the same
// chains over the pairs of an alignment).  A chain sees its points through a "cloud": any type with `n` (points), `J`
// (64-point rows that cover them, at most 32) and `load(i, a, b)` giving point i of both sides as doubles.  Everything is
// double arithmetic, every product and sum rounded on its own (-ffp-contract=off), and lane-uniform: all 64 lanes hold the
// same transform and the same score bits.
#pragma once

#include "ps_common.hpp"
#include "kabsch_solve.hpp"

#include <math.h>

#include "../../include/protstruc_superpose.h"

namespace ps_chain {

constexpr int SP_MAX_LENGTHS = 10;        // n >> k reaches 4 at k = 9 for n = 2048
constexpr int SP_STRIDE_ROUNDS = 8;       // rounds of stride doubling: far more than 2048 points need

// ---- the seed table (host and device) ----------------------------------------------------------------------------------------
struct SeedTable {
    int n_lengths, total;
    int len[SP_MAX_LENGTHS], stride[SP_MAX_LENGTHS], count[SP_MAX_LENGTHS];
};

PS_HOST_DEVICE inline int seeds_of_length(int n, int len, int stride) { return 1 + (n - len + stride - 1) / stride; }

PS_HOST_DEVICE inline void seed_table(int n, SeedTable& T) {
    T.n_lengths = 0;
    T.total = 0;
#pragma unroll
    for (int k = 0; k < SP_MAX_LENGTHS; ++k) T.len[k] = 0, T.stride[k] = 1, T.count[k] = 0;
    if (n <= 0 || n > PS_SUPERPOSE_MAX_POINTS) return;
    bool done = false;
    int last = 0;
#pragma unroll
    for (int k = 0; k < SP_MAX_LENGTHS; ++k) {
        int L = n >> k;
        L = L > 4 ? L : 4;
        if (n < 4) L = n;
        if (!done && L != last) {
            const int j = T.n_lengths;
            T.len[j] = L;
            T.stride[j] = L / 2 > 1 ? L / 2 : 1;
            T.count[j] = seeds_of_length(n, L, T.stride[j]);
            T.total += T.count[j];
            T.n_lengths = j + 1;
            last = L;
        }
        done = done || L <= 4;
    }
    for (int round = 0; round < SP_STRIDE_ROUNDS; ++round)
#pragma unroll
        for (int j = SP_MAX_LENGTHS - 1; j >= 0; --j)
            if (j < T.n_lengths && T.total > PS_SUPERPOSE_MAX_SEEDS) {
                T.total -= T.count[j];
                T.stride[j] *= 2;
                T.count[j] = seeds_of_length(n, T.len[j], T.stride[j]);
                T.total += T.count[j];
            }
}

PS_HOST_DEVICE inline bool seed_fragment(const SeedTable& T, int n, int s, int& start, int& len) {
    bool found = false;
    start = 0, len = 0;
#pragma unroll
    for (int j = 0; j < SP_MAX_LENGTHS; ++j) {
        if (!found && j < T.n_lengths && s >= 0 && s < T.count[j]) {
            len = T.len[j];
            start = s == T.count[j] - 1 ? n - len : s * T.stride[j];
            found = true;
        }
        s -= T.count[j];
    }
    return found;
}

// ---- reductions ------------------------------------------------------------------------------------------------------------
// sum over the wave, the same bits in every lane: a + b and b + a are the same number, so both partners of every step agree
__device__ __forceinline__ double wave_all_sum(double v) {
#pragma unroll
    for (int o = PS_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct Xform {
    double R[9], t[3];
};

// t = cb - R ca, component by component
__device__ __forceinline__ void set_translation(Xform& T, const double* ca, const double* cb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) T.t[c] = cb[c] - ((T.R[c * 3] * ca[0] + T.R[c * 3 + 1] * ca[1]) + T.R[c * 3 + 2] * ca[2]);
}

// e = R a + t - b
__device__ __forceinline__ void residual(const Xform& T, const double* a, const double* b, double* e) {
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = (((T.R[c * 3] * a[0] + T.R[c * 3 + 1] * a[1]) + T.R[c * 3 + 2] * a[2]) + T.t[c]) - b[c];
}

__device__ __forceinline__ double norm2(const double* e) { return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]; }

// the Kabsch fit of the points whose bit is set in the lanes' words; at least one is
template <class CloudT>
__device__ __forceinline__ void fit_selected(const CloudT& C, int lane, uint32_t sel, Xform& T) {
    double s7[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < C.J; ++j)
        if ((sel >> j) & 1u) {
            double a[3], b[3];
            C.load(j * PS_WAVE + lane, a, b);
#pragma unroll
            for (int c = 0; c < 3; ++c) s7[c] += a[c], s7[3 + c] += b[c];
            s7[6] += 1.0;
        }
#pragma unroll
    for (int k = 0; k < 7; ++k) s7[k] = wave_all_sum(s7[k]);
    const double ca[3] = {s7[0] / s7[6], s7[1] / s7[6], s7[2] / s7[6]}, cb[3] = {s7[3] / s7[6], s7[4] / s7[6], s7[5] / s7[6]};
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < C.J; ++j)
        if ((sel >> j) & 1u) {
            double a[3], b[3];
            C.load(j * PS_WAVE + lane, a, b);
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] -= ca[c], b[c] -= cb[c];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) h[i * 3 + k] += a[i] * b[k];
        }
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = wave_all_sum(h[k]);
    ps_kabsch_solve(h, T.R);
    set_translation(T, ca, cb);
}

// one pass over the points under T: the lanes' selection words for d^2 < rr2, the number selected (wave-uniform) and,
// with SCORE, the objective's sum S (the same bits in every lane)
template <bool SCORE, class CloudT>
__device__ __forceinline__ int sweep(const CloudT& C, int lane, const Xform& T, int kind, double p2, double rr2, uint32_t& sel,
                                     double& S) {
    double acc = 0.0;
    uint32_t bits = 0;
    int count = 0;
    for (int j = 0; j < C.J; ++j) {
        const int i = j * PS_WAVE + lane;
        const bool ok = i < C.n;
        double d2 = (double)INFINITY;
        if (ok) {
            double a[3], b[3], e[3];
            C.load(i, a, b);
            residual(T, a, b, e);
            d2 = norm2(e);
        }
        if (SCORE) {
            const double term = kind == PS_SUPERPOSE_TM ? 1.0 / (1.0 + d2 / p2) : (d2 <= p2 ? 1.0 : 0.0);
            acc += ok ? term : 0.0;
        }
        const bool in = ok && d2 < rr2;
        bits |= in ? (1u << j) : 0u;
        count += __popcll(__ballot(in));
    }
    if (SCORE) S = wave_all_sum(acc);
    sel = bits;
    return count;
}

// One chain from the fragment [start, start + len) under one objective (kind, p2 = the squared param, the selection radii
// r1 and r): the greatest S it visits and the transform that attains it, the same bits in every lane.
template <class CloudT>
__device__ __forceinline__ void run_chain(const CloudT& C, int lane, int start, int len, int kind, double p2, double r1, double r,
                                          double& best, Xform& kept) {
    const int need = C.n < 3 ? C.n : 3;
    Xform T;
    uint32_t previous = 0, everyone = 0;
    for (int j = 0; j < C.J; ++j) {
        const int i = j * PS_WAVE + lane;
        previous |= (i >= start && i < start + len) ? (1u << j) : 0u;
        everyone |= i < C.n ? (1u << j) : 0u;
    }
    fit_selected(C, lane, previous, T);
    best = -(double)INFINITY;
    kept = T;
    for (int it = 0; it < PS_SUPERPOSE_MAX_ITERATIONS; ++it) {
        double rr = it == 0 ? r1 : r, S = 0.0, unused = 0.0;
        uint32_t sel;
        int count = sweep<true>(C, lane, T, kind, p2, rr * rr, sel, S);
        if (S > best) best = S, kept = T;
        for (int k = 0; k < PS_SUPERPOSE_MAX_DOUBLINGS; ++k) {
            if (count >= need) break;
            rr = 2.0 * rr;
            count = sweep<false>(C, lane, T, kind, p2, rr * rr, sel, unused);
        }
        if (count < need) sel = everyone;
        if (__ballot(sel != previous) == 0) break;
        previous = sel;
        fit_selected(C, lane, sel, T);
    }
}

}  // namespace ps_chain
