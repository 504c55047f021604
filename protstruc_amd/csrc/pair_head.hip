// K33 - K36 -- the pair heads of a structure network: geometry to bin index, the cross-entropy of (B,N,N,C) logits against
// such bins with its gradient, and expectations under the softmax of the logits (PAE, pTM, contact probabilities).
// The definitions are stated in full in include/protstruc_pairhead.h; the build's -ffp-contract=off is part of K33's.
//
// ---- K33, geometry to bins.  One workgroup per row (b, i) -- grid (N, B) -- whose lanes are the columns j, 256 at a
// time.  Row i's point (mode 0) or its two frames (mode 1) sit at a workgroup-uniform address, so they are fetched once
// per workgroup by scalar loads and live in scalar registers; the squared breaks, (double)b * (double)b formed on the
// host -- exact: a 24-bit significand squared fits 53 bits, so "strictly increasing" survives the squaring --, travel in
// the kernel's arguments.  The bin is the plain count over the breaks (a wave-uniform loop of compares: AlphaFold's
// sum(d2 > sq_breaks), no search).  A masked row or column is computed like any other and replaced by a select at the
// end, so there is no divergent path and NaN under a mask ends in the discarded operand.
//
// ---- K34 / K35 / K36, the sweeps over the logits.  One workgroup of four waves per row (b, i) -- grid (N, B) --: a row of
// the logits is N * C contiguous floats, and the row is what K34 reduces over.  A lane owns 4 consecutive floats of one
// pair; G = C / 4 rounded up to a power of two lanes form the pair's group (16 at C = 64), so a wave covers 64 / G
// consecutive pairs with one load per lane -- 1 KB contiguous at C = 64 -- and the four waves take adjacent spans.  U = 4
// such loads per lane are issued before the first is consumed.  Lanes of a group past C, and pairs past N, hold -inf and
// load nothing.  The maximum and the sums are reduced inside the group across lanes, never through LDS memory: DPP
// quad_perm for the strides 1 and 2, row_half_mirror and row_mirror for 4 and 8 (every lane of a reduced 4- resp. 8-lane
// block holds the same value by then, so the mirror partner's value is the xor partner's), one ds_bpermute for 16.  Both
// operands of every combining step are the same two numbers in either lane and max and + commute, so all lanes of a
// group end with the same bits.  All 64 lanes stay active through the reductions: the loop bounds are wave-uniform and
// only loads and stores are predicated.
//   Two arms, one body: the FAST arm (C % 4 == 0 and the logits -- for K35 also grad_logits -- 16-byte aligned) reads and
// writes a lane's 4 floats as one 16-byte access; the GENERAL arm (any C, any float alignment) as up to four 4-byte
// accesses with the same lane-to-element map.  The arithmetic and its order are shared, so the two arms agree bit for bit.
//   Per pair in fp32: m = max_k x_k, e_k = exp2((x_k - m) * log2 e) by v_exp_f32, s = sum e_k (a lane's four as
// (e0 + e1) + (e2 + e3), then the group tree), lse = m + log2(s) * ln 2 by v_log_f32.
//   K34: the lane that holds the target's logit hands it to its group by one ds_bpermute; ce = lse - x_bin; the first lane
// of the group adds (double)ce to its accumulator where bin < C -- a select, so the logits of an uncounted pair never
// reach the sum.  A lane's pairs arrive in ascending j; the 64 accumulators are folded by an xor tree in double, the four
// waves' sums added in wave order by one thread and rounded to float once: a fixed order, no atomics.
//   K35: p_k = exp2((x_k - lse) * log2 e); the lane writes g * (p_k - [k == bin]) for its four, or four exact zeros by a
// select where bin >= C.  Every element of the row is written once.
//   K36: the lane's slice of the V tables (4 floats each) is read once per workgroup into registers; num_v = sum e_k * v_k
// is reduced like s, and the first lane of the group writes num_v / s.
#include "ps_common.hpp"

#include <math.h>

#include <type_traits>

#include "../../include/protstruc_pairhead.h"

namespace {

constexpr int PH_WAVES = 4;
constexpr int PH_THREADS = PS_WAVE * PH_WAVES;
constexpr int PH_U = 4;                       // loads per lane in flight
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

struct PairBreaks {
    double sq[PS_PAIRHEAD_MAX_BREAKS];        // (double)breaks[k] * (double)breaks[k]
};

template <int MODE>
__global__ __launch_bounds__(PH_THREADS) void pair_bins(const float* __restrict__ points, const float* __restrict__ rot,
                                                        const float* __restrict__ trans, const float* __restrict__ tpoints,
                                                        const float* __restrict__ trot, const float* __restrict__ ttrans,
                                                        const uint8_t* __restrict__ row_mask, const uint8_t* __restrict__ col_mask,
                                                        PairBreaks br, int nb, uint8_t* __restrict__ bins,
                                                        float* __restrict__ value, int N) {
    const size_t first = (size_t)blockIdx.y * N;      // the structure's first row
    const size_t ri = first + blockIdx.x;             // workgroup-uniform: what follows are scalar loads
    const bool row_ok = !row_mask || row_mask[ri] != 0;
    const float* __restrict__ origin = MODE == 0 ? points : trans;
    const double o0 = (double)origin[ri * 3], o1 = (double)origin[ri * 3 + 1], o2 = (double)origin[ri * 3 + 2];
    double R[9] = {}, S[9] = {}, t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (MODE == 1) {
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = (double)rot[ri * 9 + e], S[e] = (double)trot[ri * 9 + e];
        t0 = (double)ttrans[ri * 3], t1 = (double)ttrans[ri * 3 + 1], t2 = (double)ttrans[ri * 3 + 2];
    }
    for (int j = threadIdx.x; j < N; j += PH_THREADS) {
        const size_t cj = first + j;
        const bool ok = row_ok && (!col_mask || col_mask[cj] != 0);
        const double d0 = (double)points[cj * 3] - o0, d1 = (double)points[cj * 3 + 1] - o1, d2 = (double)points[cj * 3 + 2] - o2;
        double v2;
        if (MODE == 0) {
            v2 = (d0 * d0 + d1 * d1) + d2 * d2;
        } else {
            const double q0 = (double)tpoints[cj * 3] - t0, q1 = (double)tpoints[cj * 3 + 1] - t1, q2 = (double)tpoints[cj * 3 + 2] - t2;
            double e[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double u = (R[c] * d0 + R[3 + c] * d1) + R[6 + c] * d2;
                const double w = (S[c] * q0 + S[3 + c] * q1) + S[6 + c] * q2;
                e[c] = u - w;
            }
            v2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        }
        const bool counts = ok && v2 < (double)INFINITY;     // false for NaN
        int bin = 0;
        for (int k = 0; k < nb; ++k) bin += v2 > br.sq[k] ? 1 : 0;
        const size_t at = ri * N + j;
        bins[at] = (uint8_t)(counts ? bin : PS_PAIRHEAD_NO_TARGET);
        if (value) value[at] = counts ? (float)sqrt(v2) : INFINITY;
    }
}

// ---- the group of lanes that shares a pair ----------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

template <int G, typename Op>
__device__ __forceinline__ float group_reduce(float v, Op op) {
    if (G >= 2) v = op(v, dpp<0xB1>(v));           // quad_perm [1,0,3,2]: lane ^ 1
    if (G >= 4) v = op(v, dpp<0x4E>(v));           // quad_perm [2,3,0,1]: lane ^ 2
    if (G >= 8) v = op(v, dpp<0x141>(v));          // row_half_mirror: the other quad of the 8
    if (G >= 16) v = op(v, dpp<0x140>(v));         // row_mirror: the other 8 of the row
    if (G >= 32) v = op(v, __shfl_xor(v, 16));
    return v;
}

template <int G>
__device__ __forceinline__ float group_max(float v) {
    return group_reduce<G>(v, [](float a, float b) { return fmaxf(a, b); });
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
    return group_reduce<G>(v, [](float a, float b) { return a + b; });
}

// a lane's four floats, elements k0 .. k0 + 3 of a pair's C logits at p; -inf where there is nothing to read
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int k0, int C, bool pair_ok) {
    const float none = -__builtin_huge_valf();
    float4 x = make_float4(none, none, none, none);
    if (VEC) {
        if (pair_ok && k0 < C) x = *reinterpret_cast<const float4*>(p);      // C % 4 == 0: all four or none
    } else {
        if (pair_ok && k0 < C) x.x = p[0];
        if (pair_ok && k0 + 1 < C) x.y = p[1];
        if (pair_ok && k0 + 2 < C) x.z = p[2];
        if (pair_ok && k0 + 3 < C) x.w = p[3];
    }
    return x;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int k0, int C, bool pair_ok, float4 x) {
    if (VEC) {
        if (pair_ok && k0 < C) *reinterpret_cast<float4*>(p) = x;
    } else {
        if (pair_ok && k0 < C) p[0] = x.x;
        if (pair_ok && k0 + 1 < C) p[1] = x.y;
        if (pair_ok && k0 + 2 < C) p[2] = x.z;
        if (pair_ok && k0 + 3 < C) p[3] = x.w;
    }
}

// e = exp(x - m) for the lane's four, their sum reduced over the group
template <int G>
__device__ __forceinline__ float softmax_terms(float4 x, float m, float4& e) {
    e.x = __builtin_amdgcn_exp2f((x.x - m) * LOG2E);
    e.y = __builtin_amdgcn_exp2f((x.y - m) * LOG2E);
    e.z = __builtin_amdgcn_exp2f((x.z - m) * LOG2E);
    e.w = __builtin_amdgcn_exp2f((x.w - m) * LOG2E);
    return group_sum<G>((e.x + e.y) + (e.z + e.w));
}

__device__ __forceinline__ float max4(float4 x) { return fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w)); }

// the sweep's geometry, shared by K34 - K36: which pairs and elements a lane owns
template <int G>
struct Sweep {
    static constexpr int PPW = PS_WAVE / G;          // pairs a wave covers with one load per lane
    static constexpr int STEP = PPW * PH_WAVES;      // pairs the workgroup covers with one load per lane
    int lane, sub, k0, slot;
    __device__ __forceinline__ Sweep() {
        lane = threadIdx.x & (PS_WAVE - 1);
        sub = lane & (G - 1);
        k0 = 4 * sub;
        slot = (int)(threadIdx.x / PS_WAVE) * PPW + lane / G;
    }
};

template <int G, bool VEC>
__global__ __launch_bounds__(PH_THREADS) void binned_cross_entropy(const float* __restrict__ logits, const uint8_t* __restrict__ bins,
                                                                   float* __restrict__ row_loss, int* __restrict__ row_count,
                                                                   int N, int C) {
    __shared__ double part[PH_WAVES];
    __shared__ int part_n[PH_WAVES];
    const Sweep<G> w;
    const size_t row = (size_t)blockIdx.y * N + blockIdx.x;
    const float* __restrict__ x0 = logits + row * N * C + w.k0;
    const uint8_t* __restrict__ b0 = bins + row * N;
    double acc = 0.0;
    int n = 0;
    for (int j0 = 0; j0 < N; j0 += Sweep<G>::STEP * PH_U) {      // wave-uniform bounds
        float4 x[PH_U];
        int bin[PH_U];
#pragma unroll
        for (int u = 0; u < PH_U; ++u) {
            const int j = j0 + u * Sweep<G>::STEP + w.slot;
            const bool ok = j < N;
            x[u] = load4<VEC>(x0 + (size_t)j * C, w.k0, C, ok);
            const int label = (int)b0[ok ? j : N - 1];          // read by every lane, so that no wait sits between the loads
            bin[u] = ok ? label : PS_PAIRHEAD_NO_TARGET;
        }
#pragma unroll
        for (int u = 0; u < PH_U; ++u) {
            const float m = group_max<G>(max4(x[u]));
            float4 e;
            const float s = softmax_terms<G>(x[u], m, e);
            const float lse = m + __builtin_amdgcn_logf(s) * LN2;
            const int q = bin[u] & 3;
            const float mine = q == 0 ? x[u].x : q == 1 ? x[u].y : q == 2 ? x[u].z : x[u].w;
            const float target = __shfl(mine, (w.lane & ~(G - 1)) | ((bin[u] >> 2) & (G - 1)));
            const float ce = lse - target;
            if (bin[u] < C && w.sub == 0) {
                acc += (double)ce;
                ++n;
            }
        }
    }
#pragma unroll
    for (int stride = PS_WAVE / 2; stride >= 1; stride >>= 1) {
        acc += __shfl_xor(acc, stride);
        n += __shfl_xor(n, stride);
    }
    const int wave = (int)(threadIdx.x / PS_WAVE);
    if (w.lane == 0) part[wave] = acc, part_n[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = part[0];
        int count = part_n[0];
#pragma unroll
        for (int k = 1; k < PH_WAVES; ++k) total += part[k], count += part_n[k];
        row_loss[row] = (float)total;
        row_count[row] = count;
    }
}

template <int G, bool VEC>
__global__ __launch_bounds__(PH_THREADS) void binned_cross_entropy_backward(const float* __restrict__ logits,
                                                                            const uint8_t* __restrict__ bins,
                                                                            const float* __restrict__ grad_row,
                                                                            float* __restrict__ grad_logits, int N, int C) {
    const Sweep<G> w;
    const size_t row = (size_t)blockIdx.y * N + blockIdx.x;
    const size_t at = row * N * C + w.k0;
    const float* __restrict__ x0 = logits + at;
    float* __restrict__ g0 = grad_logits + at;
    const uint8_t* __restrict__ b0 = bins + row * N;
    const float g = grad_row[row];
    for (int j0 = 0; j0 < N; j0 += Sweep<G>::STEP * PH_U) {
        float4 x[PH_U];
        int bin[PH_U];
#pragma unroll
        for (int u = 0; u < PH_U; ++u) {
            const int j = j0 + u * Sweep<G>::STEP + w.slot;
            const bool ok = j < N;
            x[u] = load4<VEC>(x0 + (size_t)j * C, w.k0, C, ok);
            const int label = (int)b0[ok ? j : N - 1];          // read by every lane, so that no wait sits between the loads
            bin[u] = ok ? label : PS_PAIRHEAD_NO_TARGET;
        }
#pragma unroll
        for (int u = 0; u < PH_U; ++u) {
            const int j = j0 + u * Sweep<G>::STEP + w.slot;
            const float m = group_max<G>(max4(x[u]));
            float4 e;
            const float s = softmax_terms<G>(x[u], m, e);
            const float lse = m + __builtin_amdgcn_logf(s) * LN2;
            const int hit = bin[u] - w.k0;       // 0 .. 3 where the target is one of this lane's four
            float4 d;
            d.x = g * (__builtin_amdgcn_exp2f((x[u].x - lse) * LOG2E) - (hit == 0 ? 1.0f : 0.0f));
            d.y = g * (__builtin_amdgcn_exp2f((x[u].y - lse) * LOG2E) - (hit == 1 ? 1.0f : 0.0f));
            d.z = g * (__builtin_amdgcn_exp2f((x[u].z - lse) * LOG2E) - (hit == 2 ? 1.0f : 0.0f));
            d.w = g * (__builtin_amdgcn_exp2f((x[u].w - lse) * LOG2E) - (hit == 3 ? 1.0f : 0.0f));
            if (!(bin[u] < C)) d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            store4<VEC>(g0 + (size_t)j * C, w.k0, C, j < N, d);
        }
    }
}

template <int G, bool VEC>
__global__ __launch_bounds__(PH_THREADS) void binned_expectation(const float* __restrict__ logits, const float* __restrict__ values,
                                                                 float* __restrict__ out, int N, int C, int V) {
    const Sweep<G> w;
    const size_t b = blockIdx.y, B = gridDim.y;
    const size_t row = b * N + blockIdx.x;
    const float* __restrict__ x0 = logits + row * N * C + w.k0;
    float4 table[PS_PAIRHEAD_MAX_TABLES];
#pragma unroll
    for (int v = 0; v < PS_PAIRHEAD_MAX_TABLES; ++v) {
        table[v] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (v < V) {
            const float* __restrict__ t = values + (b * V + v) * C + w.k0;
            if (w.k0 < C) table[v].x = t[0];
            if (w.k0 + 1 < C) table[v].y = t[1];
            if (w.k0 + 2 < C) table[v].z = t[2];
            if (w.k0 + 3 < C) table[v].w = t[3];
        }
    }
    for (int j0 = 0; j0 < N; j0 += Sweep<G>::STEP * PH_U) {
        float4 x[PH_U];
#pragma unroll
        for (int u = 0; u < PH_U; ++u) {
            const int j = j0 + u * Sweep<G>::STEP + w.slot;
            x[u] = load4<VEC>(x0 + (size_t)j * C, w.k0, C, j < N);
        }
#pragma unroll
        for (int u = 0; u < PH_U; ++u) {
            const int j = j0 + u * Sweep<G>::STEP + w.slot;
            const float m = group_max<G>(max4(x[u]));
            float4 e;
            const float s = softmax_terms<G>(x[u], m, e);
#pragma unroll
            for (int v = 0; v < PS_PAIRHEAD_MAX_TABLES; ++v) {
                if (v < V) {     // wave-uniform
                    const float4 t = table[v];
                    const float num = group_sum<G>((e.x * t.x + e.y * t.y) + (e.z * t.z + e.w * t.w));
                    if (j < N && w.sub == 0) out[((size_t)v * B + b) * N * N + (size_t)blockIdx.x * N + j] = num / s;
                }
            }
        }
    }
}

bool bad_batch(int B, int N) { return B < 0 || B > 65535 || N < 1 || N > PS_PAIRHEAD_MAX_RESIDUES; }

bool bad_bins(int C) { return C < 2 || C > PS_PAIRHEAD_MAX_BINS; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// f(group size, 16-byte arm) as compile-time constants: the group is C / 4 rounded up to a power of two
template <typename F>
int by_group(int C, bool vec, F f) {
    const auto arm = [&](auto g) { return vec ? f(g, std::true_type{}) : f(g, std::false_type{}); };
    const int lanes = (C + 3) / 4;
    if (lanes <= 1) return arm(std::integral_constant<int, 1>{});
    if (lanes <= 2) return arm(std::integral_constant<int, 2>{});
    if (lanes <= 4) return arm(std::integral_constant<int, 4>{});
    if (lanes <= 8) return arm(std::integral_constant<int, 8>{});
    if (lanes <= 16) return arm(std::integral_constant<int, 16>{});
    return arm(std::integral_constant<int, 32>{});
}

}  // namespace

extern "C" int ps_pairhead_api(void) { return PS_PAIRHEAD_API; }

extern "C" int ps_pair_bins_f32(int mode, const float* points, const float* rot, const float* trans, const float* target_points,
                                const float* target_rot, const float* target_trans, const uint8_t* row_mask,
                                const uint8_t* col_mask, const float* breaks, int n_breaks, uint8_t* bins, float* value, int B,
                                int N, void* stream) {
    if (bad_batch(B, N) || (mode != 0 && mode != 1) || n_breaks < 1 || n_breaks > PS_PAIRHEAD_MAX_BREAKS)
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!breaks || !points || !bins) return (int)hipErrorInvalidValue;
    if (mode == 1 && (!rot || !trans || !target_points || !target_rot || !target_trans)) return (int)hipErrorInvalidValue;
    PairBreaks br = {};
    for (int k = 0; k < n_breaks; ++k) {
        const float x = breaks[k];
        if (!(x >= 0.0f && x < INFINITY) || (k > 0 && !(x > breaks[k - 1]))) return (int)hipErrorInvalidValue;
        br.sq[k] = (double)x * (double)x;
    }
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)N, (unsigned)B);
    if (mode == 0)
        return ps_launch(pair_bins<0>, grid, dim3(PH_THREADS), 0, s, points, rot, trans, target_points, target_rot, target_trans,
                         row_mask, col_mask, br, n_breaks, bins, value, N);
    return ps_launch(pair_bins<1>, grid, dim3(PH_THREADS), 0, s, points, rot, trans, target_points, target_rot, target_trans,
                     row_mask, col_mask, br, n_breaks, bins, value, N);
}

extern "C" int ps_binned_cross_entropy_f32(const float* logits, const uint8_t* bins, float* row_loss, int32_t* row_count, int B,
                                           int N, int C, void* stream) {
    if (bad_batch(B, N) || bad_bins(C)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!logits || !bins || !row_loss || !row_count) return (int)hipErrorInvalidValue;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return by_group(C, C % 4 == 0 && aligned16(logits), [&](auto g, auto vec) {
        return ps_launch(binned_cross_entropy<decltype(g)::value, decltype(vec)::value>, dim3((unsigned)N, (unsigned)B),
                         dim3(PH_THREADS), 0, s, logits, bins, row_loss, row_count, N, C);
    });
}

extern "C" int ps_binned_cross_entropy_backward_f32(const float* logits, const uint8_t* bins, const float* grad_row,
                                                    float* grad_logits, int B, int N, int C, void* stream) {
    if (bad_batch(B, N) || bad_bins(C)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!logits || !bins || !grad_row || !grad_logits) return (int)hipErrorInvalidValue;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return by_group(C, C % 4 == 0 && aligned16(logits) && aligned16(grad_logits), [&](auto g, auto vec) {
        return ps_launch(binned_cross_entropy_backward<decltype(g)::value, decltype(vec)::value>, dim3((unsigned)N, (unsigned)B),
                         dim3(PH_THREADS), 0, s, logits, bins, grad_row, grad_logits, N, C);
    });
}

extern "C" int ps_binned_expectation_f32(const float* logits, const float* values, float* out, int B, int N, int C, int V,
                                         void* stream) {
    if (bad_batch(B, N) || bad_bins(C) || V < 1 || V > PS_PAIRHEAD_MAX_TABLES) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!logits || !values || !out) return (int)hipErrorInvalidValue;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return by_group(C, C % 4 == 0 && aligned16(logits), [&](auto g, auto vec) {
        return ps_launch(binned_expectation<decltype(g)::value, decltype(vec)::value>, dim3((unsigned)N, (unsigned)B),
                         dim3(PH_THREADS), 0, s, logits, values, out, N, C, V);
    });
}
