// K24 -- k nearest neighbours: for every query point the k nearest candidate points of the same structure, sorted.
//
//   X = (double)x      dx = Xj.x - Xq.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz     in double, in this order
//   j is a neighbour of q iff  both are in their masks, their keys differ (where keys are given), j != q in the self
//                              graph (unless include_self), d2 is finite and d2 <= C2 = (double)cutoff * (double)cutoff
//   the neighbours ordered by (d2, j) ascending -- equal distances to the lower index --, the first k kept
//   idx = j (padding -1)      dist = (float)sqrt(d2) (padding +inf)      count = how many, at most k
//
// The build's -ffp-contract=off is part of the definition: every product and sum above is rounded on its own, so a numpy
// float64 restatement gives the same bits.  A NaN or infinite coordinate makes d2 non-finite: such a point is nobody's
// neighbour and such a query has none, with no special case.
//
// The sweep is the one of violation.hip and sasa.hip: the candidates are staged through LDS in tiles of 256 raw points,
// one per thread of a four-wave workgroup, COMPACTED while staging (a masked point never reaches LDS, so NaN there never
// meets arithmetic); an item is (x, y, z, raw index) plus the key, and every column is read as an LDS broadcast.  What
// differs is who sweeps.  Each wave OWNS 64 queries of its own, one per lane, and walks ALL the staged columns: the
// lists are too large to be merged across waves (K21 merges two entries per owner; here it would be up to 64).
//
// The list of an owner is a MAX-HEAP of k entries in LDS, heap[slot][owner]: a wave's accesses to one slot fall on 64
// consecutive banks, and lanes at different slots still differ in their bank, so no access conflicts whatever the lanes'
// depths.  An entry is d2 (8 bytes) and the index (4): 12 bytes * 64 slots * 64 owners = 48 KB per wave at k = 64.  The
// kernel is a template on the bucket KB = 16, 32, 64 that holds k, and 64 / KB waves of the workgroup own queries -- four,
// two or one --, so the heaps take 48 KB in every bucket; the other waves of the workgroup only stage.  (owner_sweep.hpp
// fixes a workgroup at four waves; the 256-point tile they stage together is what keeps the barriers per column low.)
//
// The heap's root is the owner's k-th best, and its d2 is the threshold tau, kept in registers; tau = C2 until the heap
// is full.  A column is tested in fp32 first, and a wave whose 64 owners all reject it skips it by one ballot:
//   reject iff  fl32(|xj - xq|^2) > fl32(tau) * (1 + 2^-20) + 2^-126
// The fp32 squared distance carries five roundings of 2^-24 relative, the bound three (the conversion of tau, the product,
// the sum), and 1 + 2^-20 = 1 + 16 * 2^-24 covers their sum twice over; the 2^-126 covers every underflow, each of which
// errs by at most 2^-149.  An fp32 overflow gives +inf <= +inf (kept) or only happens above a finite bound.  So the test
// never drops a pair that the double test keeps.  The columns arrive in ascending index, so once the heap is full a
// candidate with d2 == tau has a higher index than the root and loses: the double test is d2 < tau then, d2 <= C2 and
// finite before.  An insert is a sift of about log2 k steps.  At the end every lane sorts its heap in place (pop the
// root to the back, k times) and pads it, and the wave writes its 64 * k outputs -- one contiguous span of global memory --
// with 16-byte stores from the first 16-byte boundary on.  No atomics, one fixed order: results repeat bit for bit.
#include "ps_common.hpp"
#include "owner_sweep.hpp"   // WAVES, compact_slot and the barrier protocol of staging a tile

#include <math.h>

#include "../../include/protstruc_hip.h"

namespace {

constexpr int THREADS = PS_WAVE * WAVES;   // = raw points staged per tile

// Stage raw points [m0, m0 + THREADS) of structure b, valid ones only, in index order; returns how many.  An item is
// (x, y, z, the raw index as bits) in `tile` and, where there are keys, the key in `keys`.
__device__ __forceinline__ int stage_points(const float* __restrict__ pts, const uint8_t* __restrict__ point_mask,
                                            const int* __restrict__ exclude, size_t b, int M, int m0, float4* tile,
                                            int* keys, int* wave_counts) {
    const int m = m0 + threadIdx.x;
    const bool valid = m < M && (!point_mask || point_mask[b * M + m] != 0);
    int total;
    const int slot = compact_slot(valid, wave_counts, total);
    if (valid) {
        const size_t at = b * M + m;
        const f3 x = load3(pts + at * 3);
        tile[slot] = make_float4(x.x, x.y, x.z, __int_as_float(m));
        if (exclude) keys[slot] = exclude[at];
    }
    __syncthreads();
    return total;
}

// (da, ja) comes before (db, jb) in the order of the result
__device__ __forceinline__ bool before(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }

// what the fp32 squared distance of a pair with d2 <= tau never exceeds (the bound of the header)
__device__ __forceinline__ float reject_above(double tau) { return (float)tau * (1.0f + 0x1p-20f) + 0x1p-126f; }

// Put (d, j) into the max-heap of `size` entries whose root is vacant: the worse child moves up while it is worse than
// the item.  hd / hj point at this owner's slot 0; consecutive slots are `stride` entries apart.
__device__ __forceinline__ void sift_down(double* hd, int* hj, int stride, int size, double d, int j) {
    int pos = 0;
    for (;;) {
        int c = 2 * pos + 1;
        if (c >= size) break;
        double cd = hd[c * stride];
        int cj = hj[c * stride];
        if (c + 1 < size) {
            const double rd = hd[(c + 1) * stride];
            const int rj = hj[(c + 1) * stride];
            if (before(cd, cj, rd, rj)) {
                ++c;
                cd = rd;
                cj = rj;
            }
        }
        if (!before(d, j, cd, cj)) break;
        hd[pos * stride] = cd;
        hj[pos * stride] = cj;
        pos = c;
    }
    hd[pos * stride] = d;
    hj[pos * stride] = j;
}

// Write out[0 .. total) = value(0 .. total) with the whole wave: single elements up to the first 16-byte boundary of
// `out`, 16 bytes per lane from there, single elements for the rest.
template <typename T, typename F>
__device__ __forceinline__ void store_span(T* __restrict__ out, int total, int lane, F value) {
    typedef T T4 __attribute__((ext_vector_type(4)));
    int head = (int)((4u - (unsigned)((uintptr_t)out >> 2)) & 3u);
    head = head < total ? head : total;
    if (lane < head) out[lane] = value(lane);
    const int body = (total - head) >> 2;
    for (int v = lane; v < body; v += PS_WAVE) {
        const int e = head + 4 * v;
        const T4 x = {value(e), value(e + 1), value(e + 2), value(e + 3)};
        *reinterpret_cast<T4*>(out + e) = x;
    }
    const int rest = head + 4 * body + lane;
    if (rest < total) out[rest] = value(rest);
}

template <int KB>
__global__ __launch_bounds__(THREADS) void k_nearest_neighbors(const float* __restrict__ pts,
                                                               const uint8_t* __restrict__ point_mask,
                                                               const float* __restrict__ qry,
                                                               const uint8_t* __restrict__ query_mask,
                                                               const int* __restrict__ exclude,
                                                               const int* __restrict__ query_exclude, int skip_self, int k,
                                                               double C2, int* __restrict__ idx, float* __restrict__ dist,
                                                               int* __restrict__ count, int M, int Q) {
    constexpr int OWNER_WAVES = PS_KNN_MAX_K / KB;     // waves of the workgroup that own queries
    constexpr int OWNERS = OWNER_WAVES * PS_WAVE;      // queries per workgroup
    static_assert(OWNER_WAVES >= 1 && OWNER_WAVES <= WAVES && KB * OWNER_WAVES == PS_KNN_MAX_K, "16, 32 or 64");
    __shared__ __attribute__((aligned(16))) float4 tile[THREADS];
    __shared__ int keys[THREADS];
    __shared__ __attribute__((aligned(16))) double heap_d[KB * OWNERS];   // [slot][owner]
    __shared__ __attribute__((aligned(16))) int heap_j[KB * OWNERS];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const bool sweeper = wave < OWNER_WAVES;           // wave-uniform
    const int q0 = blockIdx.x * OWNERS + wave * PS_WAVE, q = q0 + lane;
    const bool own = sweeper && q < Q && (!query_mask || query_mask[b * Q + q] != 0);
    double* hd = heap_d + (sweeper ? wave * PS_WAVE + lane : 0);   // dereferenced by sweepers only
    int* hj = heap_j + (sweeper ? wave * PS_WAVE + lane : 0);

    // an owner that is masked or past the end holds zeros and takes no part: its coordinates are never read
    f3 me = f3{0.0f, 0.0f, 0.0f};
    int my_key = 0;
    if (own) {
        const size_t at = b * Q + q;
        me = load3(qry + at * 3);
        my_key = exclude ? query_exclude[at] : 0;
    }
    int kept = 0;
    double tau = C2;
    float tau32 = reject_above(tau);

    for (int m0 = 0; m0 < M; m0 += THREADS) {
        const int n = stage_points(pts, point_mask, exclude, b, M, m0, tile, keys, wave_counts);
        if (!sweeper) continue;
        for (int c = 0; c < n; ++c) {
            const float4 o = tile[c];
            const int j = __float_as_int(o.w);
            const float fx = o.x - me.x, fy = o.y - me.y, fz = o.z - me.z;
            bool cand = own && !(skip_self && j == q) && (fx * fx + fy * fy) + fz * fz <= tau32;
            if (exclude) cand = cand && keys[c] != my_key;
            if (__ballot(cand) == 0ull) continue;   // no owner of this wave can take column c
            const double dx = (double)o.x - (double)me.x, dy = (double)o.y - (double)me.y, dz = (double)o.z - (double)me.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!cand) continue;
            if (kept < k) {
                if (!(d2 <= tau && d2 < (double)INFINITY)) continue;
                int pos = kept++;                  // sift up: parents that come before the item move down
                while (pos > 0) {
                    const int par = (pos - 1) >> 1;
                    const double pd = hd[par * OWNERS];
                    const int pj = hj[par * OWNERS];
                    if (!before(pd, pj, d2, j)) break;
                    hd[pos * OWNERS] = pd;
                    hj[pos * OWNERS] = pj;
                    pos = par;
                }
                hd[pos * OWNERS] = d2;
                hj[pos * OWNERS] = j;
                if (kept < k) continue;
            } else {
                if (!(d2 < tau)) continue;         // at d2 == tau the root, of a lower index, stays
                sift_down(hd, hj, OWNERS, k, d2, j);
            }
            tau = hd[0];
            tau32 = reject_above(tau);
        }
    }

    // every lane sorts its heap in place -- the root to the back, the last entry sifted in from the top -- and pads it
    if (sweeper) {
        for (int n = kept - 1; n > 0; --n) {
            const double d = hd[n * OWNERS];
            const int j = hj[n * OWNERS];
            hd[n * OWNERS] = hd[0];
            hj[n * OWNERS] = hj[0];
            sift_down(hd, hj, OWNERS, n, d, j);
        }
        for (int s = kept; s < k; ++s) {
            hd[s * OWNERS] = (double)INFINITY;
            hj[s * OWNERS] = -1;
        }
    }
    __syncthreads();
    if (!sweeper || q0 >= Q) return;
    // the wave's rows are one contiguous span of idx and of dist: element e is slot e % k of the wave's query e / k
    const int rows = Q - q0 < PS_WAVE ? Q - q0 : PS_WAVE;
    const size_t first = (b * Q + q0) * (size_t)k;
    const double* wd = heap_d + wave * PS_WAVE;
    const int* wj = heap_j + wave * PS_WAVE;
    store_span(idx + first, rows * k, lane, [=](int e) { return wj[(e % k) * OWNERS + e / k]; });
    store_span(dist + first, rows * k, lane, [=](int e) { return (float)sqrt(wd[(e % k) * OWNERS + e / k]); });
    if (q < Q) count[b * Q + q] = kept;
}

}  // namespace

extern "C" int ps_nearest_neighbors_f32(const float* points, const uint8_t* point_mask, const float* queries,
                                        const uint8_t* query_mask, const int32_t* exclude, const int32_t* query_exclude,
                                        int k, float cutoff, int include_self, int32_t* idx, float* dist, int32_t* count,
                                        int B, int M, int Q, void* stream) {
    if (!points || !idx || !dist || !count || B < 0 || M < 0 || Q < 0 || B > 65535 || M > (1 << 24) || Q > (1 << 24) ||
        k < 1 || k > PS_KNN_MAX_K || !(cutoff > 0.0f))
        return (int)hipErrorInvalidValue;
    const bool self_graph = !queries;
    if (self_graph) {   // the queries are the points, with their mask and keys
        if (Q != M || query_mask || query_exclude) return (int)hipErrorInvalidValue;
        queries = points;
        query_mask = point_mask;
        query_exclude = exclude;
    } else if (!exclude != !query_exclude) {
        return (int)hipErrorInvalidValue;
    }
    if (B == 0 || Q == 0) return 0;
    const int skip_self = self_graph && !include_self;
    const double C2 = (double)cutoff * (double)cutoff;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const auto launch = [&](auto kernel, int bucket) {
        const int owners = PS_KNN_MAX_K / bucket * PS_WAVE;
        return ps_launch(kernel, dim3((unsigned)((Q + owners - 1) / owners), (unsigned)B), dim3(THREADS), 0, s, points,
                         point_mask, queries, query_mask, exclude, query_exclude, skip_self, k, C2, idx, dist, count, M, Q);
    };
    if (k <= 16) return launch(k_nearest_neighbors<16>, 16);
    if (k <= 32) return launch(k_nearest_neighbors<32>, 32);
    return launch(k_nearest_neighbors<64>, 64);
}
