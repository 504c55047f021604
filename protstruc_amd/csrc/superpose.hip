// K37 - K40 -- superposition scores: the weighted Kabsch fit with its RMSD, the gradient of that RMSD, and the seeded
// search for the superposition that maximises a TM-score or a count within a cutoff (GDT).  The definitions are stated in
// full in include/protstruc_superpose.h; the build's -ffp-contract=off is part of them.  All geometry is double on the
// float32 inputs, every 3x3 solve is ps_kabsch_solve (kabsch_solve.hpp), nothing here uses an atomic, and every loop has a
// bound that is a compile-time constant or a kernel argument.
//
// ---- K37 / K38.  One workgroup of four waves per structure, as k_kabsch (align.hip): 7 weighted sums, then the 9 of the
// covariance about the centroids, by block reductions in double -- a lane's points in ascending order, an xor butterfly
// across the wave, the four waves added in wave order -- after which EVERY thread holds the same bits and runs the solve
// itself: wave-uniform control flow, no broadcast.  A third pass forms the residuals R a + t - b and their weighted mean
// square.  K38 repeats the three passes (the R of K37's float output would move every residual by 2^-25 |a|, which is
// far above the rounding its result is held to) and then writes both gradients, one lane per point.
//
// ---- K39, one chain per wave.  Grid (seed group of 4, objective, structure): a workgroup compacts its structure's
// unmasked pairs, in order, into LDS as float -- six planes ax ay az bx by bz of M floats, 24 M bytes, 48 KB at M = 2048;
// the compaction's wave totals use the first 16 bytes before the planes are filled -- and then its four waves part: wave
// w runs the chain of seed 4 * blockIdx.x + w and never meets another wave again.  Lanes stride over the points (point
// j * 64 + lane is bit j of the lane's 32-bit selection word); the 7 + 9 sums of a fit and the score are reduced by the xor
// butterfly, so all 64 lanes hold the same transform and the solve runs lane-uniformly; "the selection did not change" is
// one ballot over the lanes' words.  A chain writes (S as the two words of a double, R, t as float) to its slot of the
// workspace; seeds past the structure's count write S = -inf.
// ---- K40, one wave per (structure, objective): lanes stride over the slots keeping the greatest S (the first on ties),
// a butterfly over (S, seed) with the same order, then lanes 0 .. 11 copy the winner's R and t.
#include "superpose_chain.hpp"

namespace {

using namespace ps_chain;       // the seed table, the transform helpers and the chain: superpose_chain.hpp

constexpr int SP_WAVES = 4;
constexpr int SP_THREADS = PS_WAVE * SP_WAVES;

// the slots a structure of up to M points needs: the largest seed count of any n <= M.  Filled once, never changed after.
struct SeedSlots {
    int slots[PS_SUPERPOSE_MAX_POINTS + 1];
    SeedSlots() {
        int most = 0;
        for (int n = 0; n <= PS_SUPERPOSE_MAX_POINTS; ++n) {
            SeedTable T;
            seed_table(n, T);
            most = T.total > most ? T.total : most;
            slots[n] = most;
        }
    }
};

int seed_slots(int M) {
    static const SeedSlots table;
    return table.slots[M];
}

// ---- reductions ------------------------------------------------------------------------------------------------------------
// sums over the workgroup of four waves, the same bits in every thread; red holds NV * SP_WAVES doubles
template <int NV>
__device__ __forceinline__ void block_all_sum(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_all_sum(v[k]);
    __syncthreads();      // the readers of an earlier call are done
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) red[k * SP_WAVES + wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = ((red[k * SP_WAVES] + red[k * SP_WAVES + 1]) + red[k * SP_WAVES + 2]) + red[k * SP_WAVES + 3];
}

// ---- K37 / K38 -------------------------------------------------------------------------------------------------------------
// the weight of point k as a double: 0 under the mask (the weight is then not read) and for a weight that is not > 0
__device__ __forceinline__ double point_weight(const float* __restrict__ w, const uint8_t* __restrict__ m, size_t k) {
    if (m && !m[k]) return 0.0;
    if (!w) return 1.0;
    const float x = w[k];
    return x > 0.0f ? (double)x : 0.0;
}

// the weighted fit of one structure and its mean square residual, the same bits in every thread of the workgroup
__device__ __forceinline__ void weighted_fit(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ w,
                                             const uint8_t* __restrict__ m, int M, double* red, Xform& T, double& W, double& msd) {
    double s7[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t k = threadIdx.x; k < (size_t)M; k += SP_THREADS) {
        const double wk = point_weight(w, m, k);
        if (wk > 0.0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s7[c] += wk * (double)a[k * 3 + c], s7[3 + c] += wk * (double)b[k * 3 + c];
            s7[6] += wk;
        }
    }
    block_all_sum<7>(s7, red);
    W = s7[6];
    const double ca[3] = {s7[0] / W, s7[1] / W, s7[2] / W}, cb[3] = {s7[3] / W, s7[4] / W, s7[5] / W};
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t k = threadIdx.x; k < (size_t)M; k += SP_THREADS) {
        const double wk = point_weight(w, m, k);
        if (wk > 0.0) {
            double da[3], db[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) da[c] = (double)a[k * 3 + c] - ca[c], db[c] = (double)b[k * 3 + c] - cb[c];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) h[i * 3 + j] += wk * (da[i] * db[j]);
        }
    }
    block_all_sum<9>(h, red);
    ps_kabsch_solve(h, T.R);
    if (!(W > 0.0))      // nothing selected: H is an empty sum, but the centroids are 0 / 0
#pragma unroll
        for (int i = 0; i < 9; ++i) T.R[i] = NAN;
    set_translation(T, ca, cb);
    double sq[1] = {0};
    for (size_t k = threadIdx.x; k < (size_t)M; k += SP_THREADS) {
        const double wk = point_weight(w, m, k);
        if (wk > 0.0) {
            const double pa[3] = {(double)a[k * 3], (double)a[k * 3 + 1], (double)a[k * 3 + 2]};
            const double pb[3] = {(double)b[k * 3], (double)b[k * 3 + 1], (double)b[k * 3 + 2]};
            double e[3];
            residual(T, pa, pb, e);
            sq[0] += wk * norm2(e);
        }
    }
    block_all_sum<1>(sq, red);
    msd = sq[0] / W;
}

__global__ __launch_bounds__(SP_THREADS) void superpose(const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ weight, const uint8_t* __restrict__ mask,
                                                        float* __restrict__ R, float* __restrict__ t, float* __restrict__ rmsd,
                                                        float* __restrict__ wsum, int M, size_t b_stride) {
    __shared__ double red[9 * SP_WAVES];
    const size_t s = blockIdx.x, first = s * (size_t)M;
    Xform T;
    double W, msd;
    weighted_fit(a + first * 3, b + s * b_stride, weight ? weight + first : nullptr, mask ? mask + first : nullptr, M, red, T, W, msd);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[s * 9 + i] = (float)T.R[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[s * 3 + c] = (float)T.t[c];
    rmsd[s] = (float)sqrt(msd);
    wsum[s] = (float)W;
}

__global__ __launch_bounds__(SP_THREADS) void superpose_backward(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ weight, const uint8_t* __restrict__ mask,
                                                                 const float* __restrict__ R, const float* __restrict__ rmsd,
                                                                 const float* __restrict__ grad_rmsd, float* __restrict__ grad_a,
                                                                 float* __restrict__ grad_b, int M, size_t b_stride) {
    __shared__ double red[9 * SP_WAVES];
    const size_t s = blockIdx.x, first = s * (size_t)M;
    const float* __restrict__ pa = a + first * 3;
    const float* __restrict__ pb = b + s * b_stride;
    const float* __restrict__ w = weight ? weight + first : nullptr;
    const uint8_t* __restrict__ m = mask ? mask + first : nullptr;
    Xform T;
    double W, msd;
    weighted_fit(pa, pb, w, m, M, red, T, W, msd);
    const float given = rmsd[s];
    bool live = given > 0.0f && given < INFINITY && msd > 0.0 && msd < (double)INFINITY;
#pragma unroll
    for (int i = 0; i < 9; ++i) live = live && R[s * 9 + i] == R[s * 9 + i];
    const double g = (double)grad_rmsd[s], scale = W * sqrt(msd);
    for (size_t k = threadIdx.x; k < (size_t)M; k += SP_THREADS) {
        const double wk = point_weight(w, m, k);
        double ga[3] = {0, 0, 0}, gb[3] = {0, 0, 0};
        if (live && wk > 0.0) {
            const double xa[3] = {(double)pa[k * 3], (double)pa[k * 3 + 1], (double)pa[k * 3 + 2]};
            const double xb[3] = {(double)pb[k * 3], (double)pb[k * 3 + 1], (double)pb[k * 3 + 2]};
            double e[3];
            residual(T, xa, xb, e);
            const double coef = (g * wk) / scale;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ga[c] = coef * ((T.R[c] * e[0] + T.R[3 + c] * e[1]) + T.R[6 + c] * e[2]);
                gb[c] = -(coef * e[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            grad_a[(first + k) * 3 + c] = (float)ga[c];
            if (grad_b) grad_b[(first + k) * 3 + c] = (float)gb[c];
        }
    }
}

// ---- K39 -------------------------------------------------------------------------------------------------------------------
struct Objectives {
    int kind[PS_SUPERPOSE_MAX_OBJECTIVES];
    double p2[PS_SUPERPOSE_MAX_OBJECTIVES];        // d0 d0 or c c
    double r1[PS_SUPERPOSE_MAX_OBJECTIVES], r[PS_SUPERPOSE_MAX_OBJECTIVES];
};

struct Cloud {       // a structure's n compacted pairs in LDS: six planes of M floats
    const float* p;
    int M, n, J;     // J = the 64-point rows that cover M
    __device__ __forceinline__ void load(int i, double* a, double* b) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = (double)p[c * M + i], b[c] = (double)p[(3 + c) * M + i];
    }
};

__device__ __forceinline__ void write_entry(float* __restrict__ entry, double S, const Xform& T) {
    uint32_t* __restrict__ words = reinterpret_cast<uint32_t*>(entry);
    words[0] = (uint32_t)__double2loint(S);
    words[1] = (uint32_t)__double2hiint(S);
#pragma unroll
    for (int i = 0; i < 9; ++i) entry[2 + i] = (float)T.R[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) entry[11 + c] = (float)T.t[c];
    entry[14] = 0.0f, entry[15] = 0.0f;
}

__global__ __launch_bounds__(SP_THREADS) void superpose_chains(const float* __restrict__ a, const float* __restrict__ b,
                                                               const uint8_t* __restrict__ mask, Objectives obj,
                                                               float* __restrict__ workspace, int M, int slots) {
    extern __shared__ float planes[];
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const size_t s = blockIdx.z, first = s * (size_t)M;
    const int o = blockIdx.y;
    // ---- compaction: thread t owns the points [t * per, t * per + per)
    const int per = (M + SP_THREADS - 1) / SP_THREADS;       // <= 8
    const int begin = (int)threadIdx.x * per;
    int mine = 0;
    for (int q = 0; q < per; ++q) {
        const int i = begin + q;
        if (i < M && (!mask || mask[first + i])) ++mine;
    }
    int upto = mine;                                          // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < PS_WAVE; d <<= 1) {
        const int below = __shfl_up(upto, d);
        if (lane >= d) upto += below;
    }
    int* totals = reinterpret_cast<int*>(planes);
    if (lane == PS_WAVE - 1) totals[wave] = upto;
    __syncthreads();
    int at = upto - mine, n = 0;
#pragma unroll
    for (int k = 0; k < SP_WAVES; ++k) {
        const int total = totals[k];
        at += k < wave ? total : 0;
        n += total;
    }
    __syncthreads();                                          // the totals are read: the planes may be filled
    for (int q = 0; q < per; ++q) {
        const int i = begin + q;
        if (i < M && (!mask || mask[first + i])) {
#pragma unroll
            for (int c = 0; c < 3; ++c) planes[c * M + at] = a[(first + i) * 3 + c], planes[(3 + c) * M + at] = b[(first + i) * 3 + c];
            ++at;
        }
    }
    __syncthreads();
    // ---- from here on a wave is on its own
    const int seed = (int)blockIdx.x * SP_WAVES + wave;
    if (seed >= slots) return;
    float* __restrict__ entry = workspace + ((s * gridDim.y + o) * (size_t)slots + seed) * PS_SUPERPOSE_ENTRY_FLOATS;
    SeedTable table;
    seed_table(n, table);
    int start, len;
    Xform T;
    if (!seed_fragment(table, n, seed, start, len)) {
#pragma unroll
        for (int i = 0; i < 9; ++i) T.R[i] = 0.0;
        T.t[0] = T.t[1] = T.t[2] = 0.0;
        if (lane == 0) write_entry(entry, -(double)INFINITY, T);
        return;
    }
    const Cloud C{planes, M, n, (M + PS_WAVE - 1) / PS_WAVE};
    double best;
    Xform kept;
    run_chain(C, lane, start, len, obj.kind[o], obj.p2[o], obj.r1[o], obj.r[o], best, kept);
    if (lane == 0) write_entry(entry, best, kept);
}

// ---- K40 -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PS_WAVE) void superpose_pick(const float* __restrict__ workspace, const float* __restrict__ l_norm,
                                                          float* __restrict__ score, float* __restrict__ R, float* __restrict__ t,
                                                          int slots) {
    const int lane = threadIdx.x;
    const size_t s = blockIdx.y, at = s * gridDim.x + blockIdx.x;
    const float* __restrict__ entries = workspace + at * (size_t)slots * PS_SUPERPOSE_ENTRY_FLOATS;
    double best = -(double)INFINITY;
    int winner = 0x7fffffff;
    for (int k0 = 0; k0 < slots; k0 += PS_WAVE) {
        const int k = k0 + lane;
        if (k < slots) {
            const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(entries + (size_t)k * PS_SUPERPOSE_ENTRY_FLOATS);
            const double S = __hiloint2double((int)words[1], (int)words[0]);
            if (S > best) best = S, winner = k;
        }
    }
#pragma unroll
    for (int d = PS_WAVE / 2; d > 0; d >>= 1) {
        const double other = __shfl_xor(best, d);
        const int whose = __shfl_xor(winner, d);
        if (other > best || (other == best && whose < winner)) best = other, winner = whose;
    }
    const bool found = best > -(double)INFINITY;
    if (lane == 0) score[at] = found ? (float)(best / (double)l_norm[s]) : 0.0f;
    if (lane < 12) {
        const float v = found ? entries[(size_t)winner * PS_SUPERPOSE_ENTRY_FLOATS + 2 + lane] : NAN;
        if (lane < 9) R[at * 9 + lane] = v;
        else t[at * 3 + (lane - 9)] = v;
    }
}

bool bad_batch(int B, int M) { return B < 0 || B > 65535 || M < 1; }

bool bad_search(int B, int M, int n_obj) {
    return bad_batch(B, M) || M > PS_SUPERPOSE_MAX_POINTS || n_obj < 1 || n_obj > PS_SUPERPOSE_MAX_OBJECTIVES;
}

}  // namespace

extern "C" int ps_superpose_api(void) { return PS_SUPERPOSE_API; }

extern "C" int ps_superpose_seed_count(int n) {
    SeedTable T;
    seed_table(n, T);
    return T.total;
}

extern "C" int ps_superpose_seed(int n, int s, int* start, int* len) {
    if (!start || !len) return 1;
    SeedTable T;
    seed_table(n, T);
    return seed_fragment(T, n, s, *start, *len) ? 0 : 1;
}

extern "C" long long ps_superpose_workspace_floats(int B, int M, int n_obj) {
    if (bad_search(B, M, n_obj)) return -1;
    return (long long)B * n_obj * seed_slots(M) * PS_SUPERPOSE_ENTRY_FLOATS;
}

extern "C" int ps_superpose_f32(const float* a, const float* b, const float* weight, const uint8_t* mask, float* R, float* t,
                                float* rmsd, float* wsum, int B, int M, int b_is_shared, void* stream) {
    if (bad_batch(B, M)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!a || !b || !R || !t || !rmsd || !wsum) return (int)hipErrorInvalidValue;
    return ps_launch(superpose, dim3((unsigned)B), dim3(SP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a, b, weight, mask,
                     R, t, rmsd, wsum, M, b_is_shared ? (size_t)0 : (size_t)M * 3);
}

extern "C" int ps_superpose_backward_f32(const float* a, const float* b, const float* weight, const uint8_t* mask, const float* R,
                                         const float* t, const float* rmsd, const float* wsum, const float* grad_rmsd,
                                         float* grad_a, float* grad_b, int B, int M, int b_is_shared, void* stream) {
    if (bad_batch(B, M) || (b_is_shared && grad_b)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!a || !b || !R || !t || !rmsd || !wsum || !grad_rmsd || !grad_a || (!b_is_shared && !grad_b)) return (int)hipErrorInvalidValue;
    return ps_launch(superpose_backward, dim3((unsigned)B), dim3(SP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a, b, weight,
                     mask, R, rmsd, grad_rmsd, grad_a, grad_b, M, b_is_shared ? (size_t)0 : (size_t)M * 3);
}

extern "C" int ps_superpose_search_f32(const float* a, const float* b, const uint8_t* mask, const float* l_norm,
                                       const ps_superpose_objective* objectives, int n_obj, float* workspace, float* score,
                                       float* R, float* t, int B, int M, void* stream) {
    if (bad_search(B, M, n_obj) || !objectives) return (int)hipErrorInvalidValue;
    Objectives obj = {};
    for (int o = 0; o < n_obj; ++o) {
        const int kind = objectives[o].kind;
        const float param = objectives[o].param;
        if ((kind != PS_SUPERPOSE_TM && kind != PS_SUPERPOSE_COUNT) || !(param > 0.0f && param < INFINITY)) return (int)hipErrorInvalidValue;
        const double p = (double)param;
        obj.kind[o] = kind;
        obj.p2[o] = p * p;
        if (kind == PS_SUPERPOSE_TM) {
            const double ds = p < 4.5 ? 4.5 : (p > 8.0 ? 8.0 : p);
            obj.r1[o] = ds - 1.0, obj.r[o] = ds + 1.0;
        } else {
            obj.r1[o] = p, obj.r[o] = p;
        }
    }
    if (B == 0) return 0;
    if (!a || !b || !l_norm || !workspace || !score || !R || !t) return (int)hipErrorInvalidValue;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int slots = seed_slots(M);
    const size_t lds = (size_t)(6 * M > 4 ? 6 * M : 4) * sizeof(float);       // at least the four wave totals
    const int rc = ps_launch(superpose_chains, dim3((unsigned)((slots + SP_WAVES - 1) / SP_WAVES), (unsigned)n_obj, (unsigned)B),
                             dim3(SP_THREADS), lds, s, a, b, mask, obj, workspace, M, slots);
    if (rc) return rc;
    return ps_launch(superpose_pick, dim3((unsigned)n_obj, (unsigned)B), dim3(PS_WAVE), 0, s, workspace, l_norm, score, R, t, slots);
}
