// K55 - K59 -- message passing on graphs: segment reduce, segment gather, edge dot, segment softmax and its backward pass.
// The definitions, the order of every sum and the vocabulary (edge list, padding, grouping) are in
// include/protstruc_aggregate.h; this file is their one implementation.
//
// Every kernel is a flat grid-stride walk over items that need nothing from each other -- (segment, quad of the row) in K55,
// (edge, quad) in K56, (edge, head) in K57, (segment, head) in K58 / K59 --, so there is no LDS, no cross-lane traffic and no
// atomic, and a result depends on the lists and the data alone, never on the launch shape.  A quad is four consecutive
// floats of a row; consecutive lanes take consecutive quads, so a wave's loads of one member's row are contiguous.
//
// Addresses.  A segment's bounds are cut to the length of the list they index before the walk; a member is used as an
// address only after `member` has found it inside [0, E) and, where col is given, below row_ptr[n_rows] with col inside
// [0, M); a node index only inside [0, S).  Offsets are size_t products of widened factors.
//
// The 16-byte arm and the dword arm of K55 - K57 are one template and differ in the load and store alone.
#include "ps_common.hpp"

#include <math.h>

#include "../../include/protstruc_aggregate.h"

namespace {

constexpr int THREADS = 256;
constexpr int INFLIGHT = 4;      // members whose loads are issued before the first is used (K55)
constexpr int TREE_LEVELS = 11;  // K57: ceil(PS_AGGREGATE_MAX_ROW / 4) = 1024 = 2^10 partial sums at the most

static_assert((PS_AGGREGATE_MAX_ROW + 3) / 4 < (1 << TREE_LEVELS), "the binary counter of K57 holds every partial sum");

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// A grouping with the edge list it is checked against: by value in the kernel's arguments.
struct Grouping {
    const long long* ptr;      // [S + 1]
    const long long* perm;     // [n_perm], or NULL: the members are the positions themselves
    long long n_perm;
    const long long* row_ptr;  // [n_rows + 1], read at n_rows alone; used with col only
    const int* col;            // [E], or NULL: no member is padding
    long long E, n_rows;
    int M;
};

__device__ __forceinline__ long long clamp_ll(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the first position of the tail: positions from here on are padding
__device__ __forceinline__ long long tail_of(const Grouping& g) { return g.col ? g.row_ptr[g.n_rows] : g.E; }

// the bounds of segment s, inside the list they index
__device__ __forceinline__ void bounds_of(const Grouping& g, long long s, long long& lo, long long& hi) {
    const long long limit = g.perm ? g.n_perm : g.E;
    lo = clamp_ll(g.ptr[s], limit);
    hi = clamp_ll(g.ptr[s + 1], limit);
}

// the edge position of member t (lo <= t < hi, so perm[t] exists), or -1: skipped
__device__ __forceinline__ long long member(const Grouping& g, long long t, long long tail) {
    const long long e = g.perm ? g.perm[t] : t;
    if (e < 0 || e >= g.E) return -1;
    if (g.col && (e >= tail || (unsigned)g.col[e] >= (unsigned)g.M)) return -1;
    return e;
}

template <bool VEC>
__device__ __forceinline__ f32x4_t load_quad(const float* __restrict__ at, int mine) {
    if (VEC) return *reinterpret_cast<const f32x4_t*>(at);
    f32x4_t v = {0.0f, 0.0f, 0.0f, 0.0f};
    v[0] = at[0];
    if (mine > 1) v[1] = at[1];
    if (mine > 2) v[2] = at[2];
    if (mine > 3) v[3] = at[3];
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float* __restrict__ at, f32x4_t v, int mine) {
    if (VEC) {
        *reinterpret_cast<f32x4_t*>(at) = v;
        return;
    }
    at[0] = v[0];
    if (mine > 1) at[1] = v[1];
    if (mine > 2) at[2] = v[2];
    if (mine > 3) at[3] = v[3];
}

// the weights of a quad's four floats: one per head the quad touches (a quad lies in one head where D % 4 == 0)
__device__ __forceinline__ f32x4_t load_weights(const float* __restrict__ at, const int* hd, int mine) {
    f32x4_t w = {1.0f, 1.0f, 1.0f, 1.0f};
    w[0] = at[hd[0]];
    if (mine > 1) w[1] = hd[1] == hd[0] ? w[0] : at[hd[1]];
    if (mine > 2) w[2] = hd[2] == hd[1] ? w[1] : at[hd[2]];
    if (mine > 3) w[3] = hd[3] == hd[2] ? w[2] : at[hd[3]];
    return w;
}

// K55.  EXTREME: MAX / MIN, else SUM / MEAN.
template <bool VEC, bool EXTREME>
__global__ __launch_bounds__(THREADS) void k_segment_reduce(const float* __restrict__ values, const float* __restrict__ weight,
                                                            const Grouping g, long long S, int mode, float* __restrict__ out,
                                                            long long* __restrict__ arg, int H, int D, int L) {
    const int HD = H * D;
    const long long items = S * (long long)L;
    const long long tail = tail_of(g);
    for (long long it = (long long)blockIdx.x * THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * THREADS) {
        const long long s = it / L;
        const int c0 = 4 * (int)(it - s * L);
        const int mine = HD - c0 < 4 ? HD - c0 : 4;   // >= 1: L = ceil(HD / 4)
        int hd[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) hd[i] = (c0 + (i < mine ? i : 0)) / D;
        long long lo, hi;
        bounds_of(g, s, lo, hi);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        long long where[4] = {-1, -1, -1, -1};
        long long n = 0;
        for (long long t = lo; t < hi; t += INFLIGHT) {
            long long e[INFLIGHT];
            f32x4_t v[INFLIGHT], w[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                e[u] = t + u < hi ? member(g, t + u, tail) : -1;
                v[u] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
                w[u] = f32x4_t{1.0f, 1.0f, 1.0f, 1.0f};
                if (e[u] >= 0) {   // nothing of a skipped member is read
                    v[u] = load_quad<VEC>(values + (size_t)e[u] * (size_t)HD + (size_t)c0, mine);
                    if (!EXTREME && weight) w[u] = load_weights(weight + (size_t)e[u] * (size_t)H, hd, mine);
                }
            }
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) {
                if (e[u] < 0) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (EXTREME) {
                        if (n == 0 || (mode == PS_AGGREGATE_MAX ? v[u][i] > best[i] : v[u][i] < best[i])) {
                            best[i] = v[u][i];
                            where[i] = e[u];
                        }
                    } else {
                        acc[i] = acc[i] + (weight ? (double)w[u][i] * (double)v[u][i] : (double)v[u][i]);
                    }
                }
                ++n;
            }
        }
        f32x4_t r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (EXTREME)
                r[i] = n ? best[i] : 0.0f;
            else
                r[i] = (float)(mode == PS_AGGREGATE_MEAN && n ? acc[i] / (double)n : acc[i]);
        }
        const size_t at = (size_t)s * (size_t)HD + (size_t)c0;
        store_quad<VEC>(out + at, r, mine);
        if (EXTREME && arg) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < mine) arg[at + i] = where[i];
        }
    }
}

// K56
template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_segment_gather(const float* __restrict__ node, const float* __restrict__ weight,
                                                            const long long* __restrict__ index, long long E, long long S,
                                                            float* __restrict__ out, int H, int D, int L) {
    const int HD = H * D;
    const long long items = E * (long long)L;
    for (long long it = (long long)blockIdx.x * THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * THREADS) {
        const long long e = it / L;
        const int c0 = 4 * (int)(it - e * L);
        const int mine = HD - c0 < 4 ? HD - c0 : 4;
        const long long o = index[e];
        f32x4_t r = {0.0f, 0.0f, 0.0f, 0.0f};
        if (o >= 0 && o < S) {
            r = load_quad<VEC>(node + (size_t)o * (size_t)HD + (size_t)c0, mine);
            if (weight) {
                int hd[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) hd[i] = (c0 + (i < mine ? i : 0)) / D;
                const f32x4_t w = load_weights(weight + (size_t)e * (size_t)H, hd, mine);
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = (float)((double)w[i] * (double)r[i]);
            }
        }
        store_quad<VEC>(out + (size_t)e * (size_t)HD + (size_t)c0, r, mine);
    }
}

// The tree of the header over partial sums that arrive in order, as a binary counter: level i holds the sum of 2^i
// consecutive partial sums while bit i of `n` is set.  Pushing the k-th sum merges it (on the right) into every full level
// below the first empty one, which is the header's s_k += s_(k+stride); `finish` adds what is left, newest first, which is
// the header's steps whose right operand is the short last group.  Indices are constants after unrolling: registers.
struct Tree {
    double level[TREE_LEVELS];
    unsigned n = 0;

    __device__ __forceinline__ void push(double v) {
        bool placed = false;
#pragma unroll
        for (int i = 0; i < TREE_LEVELS; ++i) {
            if (!placed) {
                if ((n >> i) & 1u) {
                    v = level[i] + v;
                } else {
                    level[i] = v;
                    placed = true;
                }
            }
        }
        ++n;
    }

    __device__ __forceinline__ double finish() const {
        double total = 0.0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < TREE_LEVELS; ++i) {
            if ((n >> i) & 1u) {
                total = any ? level[i] + total : level[i];
                any = true;
            }
        }
        return total;
    }
};

// K57
template <bool VEC>
__global__ __launch_bounds__(THREADS) void k_edge_dot(const float* __restrict__ node, const float* __restrict__ values,
                                                      const long long* __restrict__ index, long long E, long long S,
                                                      float* __restrict__ out, int H, int D) {
    const long long items = E * (long long)H;
    const int K = (D + 3) / 4;
    for (long long it = (long long)blockIdx.x * THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * THREADS) {
        const long long e = it / H;
        const int h = (int)(it - e * H);
        const long long o = index[e];
        float r = 0.0f;
        if (o >= 0 && o < S) {
            const float* __restrict__ a = node + ((size_t)o * (size_t)H + (size_t)h) * (size_t)D;
            const float* __restrict__ b = values + (size_t)it * (size_t)D;
            Tree tree;
            for (int k = 0; k < K; ++k) {
                const int mine = D - 4 * k < 4 ? D - 4 * k : 4;
                const f32x4_t x = load_quad<VEC>(a + 4 * k, mine), y = load_quad<VEC>(b + 4 * k, mine);
                double sum = (double)x[0] * (double)y[0];
                if (mine > 1) sum = sum + (double)x[1] * (double)y[1];
                if (mine > 2) sum = sum + (double)x[2] * (double)y[2];
                if (mine > 3) sum = sum + (double)x[3] * (double)y[3];
                tree.push(sum);
            }
            r = (float)tree.finish();
        }
        out[it] = r;
    }
}

__global__ __launch_bounds__(THREADS) void k_zero(float* __restrict__ out, long long n) {
    for (long long it = (long long)blockIdx.x * THREADS + threadIdx.x; it < n; it += (long long)gridDim.x * THREADS) out[it] = 0.0f;
}

// K58
__global__ __launch_bounds__(THREADS) void k_segment_softmax(const float* __restrict__ logits, const Grouping g, long long S,
                                                             float* __restrict__ w, float* __restrict__ lse, int H) {
    const long long items = S * (long long)H;
    const long long tail = tail_of(g);
    for (long long it = (long long)blockIdx.x * THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * THREADS) {
        const long long s = it / H;
        const int h = (int)(it - s * H);
        long long lo, hi;
        bounds_of(g, s, lo, hi);
        bool any = false;
        float m = 0.0f;
        for (long long t = lo; t < hi; ++t) {
            const long long e = member(g, t, tail);
            if (e < 0) continue;
            const float x = logits[(size_t)e * (size_t)H + (size_t)h];
            if (!any || x > m) m = x;
            any = true;
        }
        const bool live = any && !(m == -INFINITY);
        double sum = 0.0;
        if (live) {
            for (long long t = lo; t < hi; ++t) {
                const long long e = member(g, t, tail);
                if (e < 0) continue;
                sum = sum + exp((double)logits[(size_t)e * (size_t)H + (size_t)h] - (double)m);
            }
        }
        for (long long t = lo; t < hi; ++t) {
            const long long e = member(g, t, tail);
            if (e < 0) continue;
            const size_t at = (size_t)e * (size_t)H + (size_t)h;
            w[at] = live ? (float)(exp((double)logits[at] - (double)m) / sum) : 0.0f;
        }
        if (lse) lse[it] = live ? (float)((double)m + log(sum)) : -INFINITY;
    }
}

// K59
__global__ __launch_bounds__(THREADS) void k_segment_softmax_backward(const float* __restrict__ w, const float* __restrict__ gw,
                                                                      const Grouping g, long long S, float* __restrict__ gx,
                                                                      int H) {
    const long long items = S * (long long)H;
    const long long tail = tail_of(g);
    for (long long it = (long long)blockIdx.x * THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * THREADS) {
        const long long s = it / H;
        const int h = (int)(it - s * H);
        long long lo, hi;
        bounds_of(g, s, lo, hi);
        double total = 0.0;
        for (long long t = lo; t < hi; ++t) {
            const long long e = member(g, t, tail);
            if (e < 0) continue;
            const size_t at = (size_t)e * (size_t)H + (size_t)h;
            total = total + (double)w[at] * (double)gw[at];
        }
        for (long long t = lo; t < hi; ++t) {
            const long long e = member(g, t, tail);
            if (e < 0) continue;
            const size_t at = (size_t)e * (size_t)H + (size_t)h;
            gx[at] = (float)((double)w[at] * ((double)gw[at] - total));
        }
    }
}

bool bad_sizes(int B, int M, int Q, long long E, long long n_perm) {
    return B < 0 || B > 65535 || M < 0 || M > (1 << 24) || Q < 0 || Q > (1 << 24) || E < 0 || n_perm < 0;
}

bool bad_row(int H, int D) {
    return H < 1 || H > PS_AGGREGATE_MAX_HEADS || D < 1 || (long long)H * D > PS_AGGREGATE_MAX_ROW;
}

bool bad_grouping(const long long* ptr, const long long* perm, long long n_perm, const long long* row_ptr, const int32_t* col) {
    return !ptr || (!perm && n_perm > 0) || (col && !row_ptr);
}

unsigned grid_for(long long items) {
    const long long blocks = (items + THREADS - 1) / THREADS;
    return (unsigned)(blocks < 65536 ? blocks : 65536);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

Grouping grouping_of(const long long* ptr, const long long* perm, long long n_perm, const long long* row_ptr, const int32_t* col,
                     long long E, int B, int Q, int M) {
    return Grouping{ptr, perm, perm ? n_perm : 0, row_ptr, col, E, (long long)B * Q, M};
}

}  // namespace

extern "C" int ps_aggregate_api(void) { return PS_AGGREGATE_API; }

extern "C" int ps_segment_reduce_f32(const float* values, const float* weight, const long long* ptr, const long long* perm,
                                     long long n_perm, const long long* row_ptr, const int32_t* col, long long E, int mode,
                                     float* out, long long* arg, int B, int Q, int M, int H, int D, void* stream) {
    if (bad_sizes(B, M, Q, E, n_perm) || bad_row(H, D) || bad_grouping(ptr, perm, n_perm, row_ptr, col) || !out ||
        (E > 0 && !values) || mode < PS_AGGREGATE_SUM || mode > PS_AGGREGATE_MIN)
        return (int)hipErrorInvalidValue;
    const bool extreme = mode == PS_AGGREGATE_MAX || mode == PS_AGGREGATE_MIN;
    if (extreme ? weight != nullptr : arg != nullptr) return (int)hipErrorInvalidValue;
    const long long S = (long long)B * (perm ? M : Q);
    if (B == 0 || S == 0) return 0;
    const int HD = H * D, L = (HD + 3) / 4;
    const bool vec = HD % 4 == 0 && aligned16(values) && aligned16(out);
    const Grouping g = grouping_of(ptr, perm, n_perm, row_ptr, col, E, B, Q, M);
    auto kernel = extreme ? (vec ? k_segment_reduce<true, true> : k_segment_reduce<false, true>)
                          : (vec ? k_segment_reduce<true, false> : k_segment_reduce<false, false>);
    return ps_launch(kernel, dim3(grid_for(S * L)), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), values, weight, g, S,
                     mode, out, arg, H, D, L);
}

extern "C" int ps_segment_gather_f32(const float* node, const float* weight, const long long* index, long long E, long long S,
                                     int H, int D, float* out, void* stream) {
    if (E < 0 || S < 0 || bad_row(H, D) || !index || !out || (S > 0 && !node)) return (int)hipErrorInvalidValue;
    if (E == 0) return 0;
    const int HD = H * D, L = (HD + 3) / 4;
    const bool vec = HD % 4 == 0 && aligned16(node) && aligned16(out);
    return ps_launch(vec ? k_segment_gather<true> : k_segment_gather<false>, dim3(grid_for(E * L)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), node, weight, index, E, S, out, H, D, L);
}

extern "C" int ps_edge_dot_f32(const float* node, const float* values, const long long* index, long long E, long long S, int H,
                               int D, float* out, void* stream) {
    if (E < 0 || S < 0 || bad_row(H, D) || !index || !out || !values || (S > 0 && !node)) return (int)hipErrorInvalidValue;
    if (E == 0) return 0;
    const bool vec = D % 4 == 0 && aligned16(node) && aligned16(values);
    return ps_launch(vec ? k_edge_dot<true> : k_edge_dot<false>, dim3(grid_for(E * H)), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), node, values, index, E, S, out, H, D);
}

extern "C" int ps_segment_softmax_f32(const float* logits, const long long* ptr, const long long* perm, long long n_perm,
                                      const long long* row_ptr, const int32_t* col, long long E, float* w, float* lse, int B,
                                      int Q, int M, int H, void* stream) {
    if (bad_sizes(B, M, Q, E, n_perm) || bad_row(H, 1) || bad_grouping(ptr, perm, n_perm, row_ptr, col) ||
        (E > 0 && (!logits || !w)))
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long S = (long long)B * (perm ? M : Q);
    if (E > 0) {
        const int rc = ps_launch(k_zero, dim3(grid_for(E * H)), dim3(THREADS), 0, st, w, E * (long long)H);
        if (rc) return rc;
    }
    if (S == 0) return 0;
    const Grouping g = grouping_of(ptr, perm, n_perm, row_ptr, col, E, B, Q, M);
    return ps_launch(k_segment_softmax, dim3(grid_for(S * H)), dim3(THREADS), 0, st, logits, g, S, w, lse, H);
}

extern "C" int ps_segment_softmax_backward_f32(const float* w, const float* grad_w, const long long* ptr, const long long* perm,
                                               long long n_perm, const long long* row_ptr, const int32_t* col, long long E,
                                               float* grad_logits, int B, int Q, int M, int H, void* stream) {
    if (bad_sizes(B, M, Q, E, n_perm) || bad_row(H, 1) || bad_grouping(ptr, perm, n_perm, row_ptr, col) ||
        (E > 0 && (!w || !grad_w || !grad_logits)))
        return (int)hipErrorInvalidValue;
    if (B == 0 || E == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long S = (long long)B * (perm ? M : Q);
    const int rc = ps_launch(k_zero, dim3(grid_for(E * H)), dim3(THREADS), 0, st, grad_logits, E * (long long)H);
    if (rc || S == 0) return rc;
    const Grouping g = grouping_of(ptr, perm, n_perm, row_ptr, col, E, B, Q, M);
    return ps_launch(k_segment_softmax_backward, dim3(grid_for(S * H)), dim3(THREADS), 0, st, w, grad_w, g, S, grad_logits, H);
}
