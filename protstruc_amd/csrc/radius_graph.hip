// K47 / K48 -- the radius graph: every neighbour of every query within a cutoff, as CSR lists ascending in j.
//
// The definition, the result and the argument of the box test are in include/protstruc_graph.h and radius_box.hpp; this
// file is the two kernels.
//
// K47 (k_tile_boxes): a wave per block of 64 candidate slots, a lane per slot.  min / max / count go through an xor
// butterfly; after the steps 1, 2, 4, 8 every lane holds its quarter's box, after 16 and 32 the block's.
//
// K48 (k_radius_sweep<SINK>): a workgroup is ONE wave, which owns 64 consecutive queries, one per lane.  That is the
// owner sweep of knn.hip with the four waves of a workgroup taken apart: there the waves share every staged tile, here
// which blocks are staged at all is a decision per wave -- the box of 64 consecutive queries against the box of 64
// consecutive candidates --, and a workgroup of four waves would have to stage what any of the four needs.  With one
// wave the stream compaction is one ballot (owner_sweep.hpp's compact_slot is that ballot plus the exchange between four
// waves), and the barriers around the tile cost nothing.  The wave walks the blocks in ascending order:
//   1. the block's box against the box of the wave's queries                              -> dropped for the whole wave
//   2. every lane's own query against the boxes of the four quarters (a 4-bit mask)        -> dropped if no lane keeps any
//   3. the block is staged, valid finite points only, compacted in index order (x, y, z, index; the key beside it)
//   4. quarter by quarter, skipping a quarter no lane keeps: K24's column loop -- the float32 pre-test with K24's bound at
//      tau = C2 and one ballot, then the double test of the definition -- and the sink.
// The sinks: COUNT adds one; FILL writes (j, (float)sqrt(d2)) at the lane's running position, which starts at
// row_ptr[row], and only below max_edges; STATS is COUNT plus six counters per wave.  Each lane writes along its own row
// (DESIGN.md section 4 says why not transposed).  The same source, so the same predicate: count and fill agree.
#include "ps_common.hpp"     // PS_WAVE, f3, load3, ps_launch
#include "radius_box.hpp"

#include <math.h>

#include "../../include/protstruc_graph.h"

namespace {

static_assert(PS_RADIUS_TILE == PS_WAVE && PS_RADIUS_BOX_FLOATS == 40, "a lane per slot; five boxes of eight floats");
constexpr int BOX = 8;                     // floats per box
constexpr int QUARTER = PS_RADIUS_TILE / 4;
enum { COUNT = 0, FILL = 1, STATS = 2 };

__device__ __forceinline__ float xor_min(float v, int step) { return fminf(v, __shfl_xor(v, step)); }
__device__ __forceinline__ float xor_max(float v, int step) { return fmaxf(v, __shfl_xor(v, step)); }

// lo / hi / n of the lanes whose index differs from this lane's only in the bits below `upto`, starting at bit `from`
__device__ __forceinline__ void butterfly(float (&lo)[3], float (&hi)[3], int& n, int from, int upto) {
    for (int step = from; step < upto; step <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = xor_min(lo[a], step);
            hi[a] = xor_max(hi[a], step);
        }
        n += __shfl_xor(n, step);
    }
}

__device__ __forceinline__ void store_box(float* __restrict__ out, const float (&lo)[3], const float (&hi)[3], int n) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[a] = lo[a];
        out[3 + a] = hi[a];
    }
    out[6] = (float)n;
    out[7] = 0.0f;
}

// a value every lane holds alike, as the compiler can see it: in a scalar register
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__global__ __launch_bounds__(PS_WAVE) void k_tile_boxes(const float* __restrict__ pts, const uint8_t* __restrict__ point_mask,
                                                        float* __restrict__ boxes, int M, int T) {
    const size_t b = blockIdx.y;
    const int t = blockIdx.x, lane = threadIdx.x, m = t * PS_RADIUS_TILE + lane;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int n = 0;
    if (m < M && (!point_mask || point_mask[b * M + m] != 0)) {
        const f3 x = load3(pts + (b * M + m) * 3);
        if (ps_finite3(x.x, x.y, x.z)) {
            lo[0] = hi[0] = x.x;
            lo[1] = hi[1] = x.y;
            lo[2] = hi[2] = x.z;
            n = 1;
        }
    }
    float* out = boxes + (b * T + t) * PS_RADIUS_BOX_FLOATS;
    butterfly(lo, hi, n, 1, QUARTER);
    if ((lane & (QUARTER - 1)) == 0) store_box(out + (1 + lane / QUARTER) * BOX, lo, hi, n);
    butterfly(lo, hi, n, QUARTER, PS_WAVE);
    if (lane == 0) store_box(out, lo, hi, n);
}

template <int SINK>
__global__ __launch_bounds__(PS_WAVE) void k_radius_sweep(const float* __restrict__ pts, const uint8_t* __restrict__ point_mask,
                                                          const float* __restrict__ qry, const uint8_t* __restrict__ query_mask,
                                                          const int* __restrict__ exclude, const int* __restrict__ query_exclude,
                                                          int skip_self, double C2, const float* __restrict__ boxes,
                                                          const long long* __restrict__ row_ptr, long long max_edges,
                                                          int* __restrict__ col, float* __restrict__ dist,
                                                          int* __restrict__ count, int* __restrict__ stats, int M, int Q, int T) {
    __shared__ __attribute__((aligned(16))) float4 tile[PS_RADIUS_TILE];
    __shared__ int keys[PS_RADIUS_TILE];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x, q = blockIdx.x * PS_WAVE + lane;
    const size_t row = b * Q + (q < Q ? q : 0);

    // an owner that is masked, past the end or not finite holds zeros and takes no part: its row is empty
    bool own = q < Q && (!query_mask || query_mask[row] != 0);
    f3 me = f3{0.0f, 0.0f, 0.0f};
    int my_key = 0;
    if (own) {
        me = load3(qry + row * 3);
        my_key = exclude ? query_exclude[row] : 0;
        own = ps_finite3(me.x, me.y, me.z);
    }
    float wlo[3] = {own ? me.x : INFINITY, own ? me.y : INFINITY, own ? me.z : INFINITY};
    float whi[3] = {own ? me.x : -INFINITY, own ? me.y : -INFINITY, own ? me.z : -INFINITY};
    int ignored = 0;
    butterfly(wlo, whi, ignored, 1, PS_WAVE);
#pragma unroll
    for (int a = 0; a < 3; ++a) {                       // the wave's box in scalar registers: the block test is wave-uniform
        wlo[a] = uniform(wlo[a]);
        whi[a] = uniform(whi[a]);
    }
    const int owners = __popcll(__ballot(own));
    const float mine[3] = {me.x, me.y, me.z};
    const float bound = ps_radius_reject_above(C2);

    int kept = 0;                                       // COUNT, STATS
    long long pos = SINK == FILL ? row_ptr[row] : 0;    // FILL: where this row's next edge goes
    int walked = 0, wave_dropped = 0, lane_dropped = 0, quarters = 0, quarters_skipped = 0, columns = 0;

    for (int t = 0; owners != 0 && t < T; ++t) {        // wave-uniform: `owners` is the same in every lane
        const float* bx = boxes + (b * T + t) * PS_RADIUS_BOX_FLOATS;
        if (SINK == STATS) ++walked;
        if (ps_box_dropped(wlo, whi, bx, bx + 3, (int)bx[6], bound)) {
            if (SINK == STATS) ++wave_dropped;
            continue;
        }
        unsigned live = 0;                              // the quarters this lane's own query can have a neighbour in
        if (own) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* qb = bx + (1 + k) * BOX;
                live |= ps_box_dropped(mine, mine, qb, qb + 3, (int)qb[6], bound) ? 0u : 1u << k;
            }
        }
        if (__ballot(live != 0u) == 0ull) {
            if (SINK == STATS) ++lane_dropped;
            continue;
        }

        // stage the block: valid finite points only, in index order
        const int m = t * PS_RADIUS_TILE + lane;
        bool valid = m < M && (!point_mask || point_mask[b * M + m] != 0);
        f3 x = f3{0.0f, 0.0f, 0.0f};
        if (valid) {
            x = load3(pts + (b * M + m) * 3);
            valid = ps_finite3(x.x, x.y, x.z);
        }
        const unsigned long long staged = __ballot(valid);
        const int slot = __popcll(staged & ((1ull << lane) - 1ull));
        __syncthreads();                                // the previous block's readers are done
        if (valid) {
            tile[slot] = make_float4(x.x, x.y, x.z, __int_as_float(m));
            if (exclude) keys[slot] = exclude[b * M + m];
        }
        __syncthreads();

        for (int k = 0; k < 4; ++k) {
            if (SINK == STATS) ++quarters;
            const bool in = (live >> k) & 1u;
            if (__ballot(in) == 0ull) {                 // no lane of the wave keeps this quarter
                if (SINK == STATS) ++quarters_skipped;
                continue;
            }
            const int c0 = __popcll(staged & ((1ull << (k * QUARTER)) - 1ull));
            const int c1 = k == 3 ? __popcll(staged) : __popcll(staged & ((1ull << ((k + 1) * QUARTER)) - 1ull));
            for (int c = c0; c < c1; ++c) {
                const float4 o = tile[c];
                const int j = __float_as_int(o.w);
                const float fx = o.x - me.x, fy = o.y - me.y, fz = o.z - me.z;
                bool cand = in && !(skip_self && j == q) && (fx * fx + fy * fy) + fz * fz <= bound;   // K24's pre-test
                if (exclude) cand = cand && keys[c] != my_key;
                if (__ballot(cand) == 0ull) continue;   // no owner of this wave can take column c
                if (SINK == STATS) ++columns;
                const double dx = (double)o.x - (double)me.x, dy = (double)o.y - (double)me.y, dz = (double)o.z - (double)me.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(cand && d2 <= C2 && d2 < (double)INFINITY)) continue;
                if (SINK == FILL) {
                    if (pos < max_edges) {
                        col[pos] = j;
                        dist[pos] = (float)sqrt(d2);
                    }
                    ++pos;
                } else {
                    ++kept;
                }
            }
        }
    }
    if (SINK != FILL && q < Q) count[row] = kept;
    if (SINK == STATS && lane == 0) {
        int* s = stats + (b * gridDim.x + blockIdx.x) * PS_RADIUS_STATS;
        s[0] = walked;
        s[1] = wave_dropped;
        s[2] = lane_dropped;
        s[3] = quarters;
        s[4] = quarters_skipped;
        s[5] = columns;
    }
}

constexpr int MAX_POINTS = 1 << 24;

// what the two sweeps share: the checks of the header, then the launch.  Returns the HIP error.
template <int SINK>
int sweep(const float* points, const uint8_t* point_mask, const float* queries, const uint8_t* query_mask,
          const int32_t* exclude, const int32_t* query_exclude, float cutoff, int include_self, const float* boxes,
          const long long* row_ptr, long long max_edges, int32_t* col, float* dist, int32_t* count, int32_t* stats, int B, int M,
          int Q, void* stream) {
    if (B < 0 || M < 0 || Q < 0 || B > 65535 || M > MAX_POINTS || Q > MAX_POINTS || !(cutoff > 0.0f) ||
        !(cutoff < (float)INFINITY) || max_edges < 0)
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
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (SINK == FILL) {
        if (M == 0 || max_edges == 0) return 0;
        if (!row_ptr || !col || !dist) return (int)hipErrorInvalidValue;
    } else if (!count) {
        return (int)hipErrorInvalidValue;
    }
    if (M > 0 && (!points || !boxes)) return (int)hipErrorInvalidValue;
    const int skip_self = self_graph && !include_self;
    const double C2 = (double)cutoff * (double)cutoff;
    const int T = (M + PS_RADIUS_TILE - 1) / PS_RADIUS_TILE;   // M == 0: no block is walked, every count is 0
    return ps_launch(k_radius_sweep<SINK>, dim3((unsigned)((Q + PS_WAVE - 1) / PS_WAVE), (unsigned)B), dim3(PS_WAVE), 0, s,
                     points, point_mask, queries, query_mask, exclude, query_exclude, skip_self, C2, boxes, row_ptr, max_edges,
                     col, dist, count, stats, M, Q, T);
}

}  // namespace

extern "C" int ps_graph_api(void) { return PS_GRAPH_API; }

extern "C" int ps_radius_tile_boxes_f32(const float* points, const uint8_t* point_mask, float* boxes, int B, int M,
                                        void* stream) {
    if (B < 0 || M < 0 || B > 65535 || M > MAX_POINTS) return (int)hipErrorInvalidValue;
    if (B == 0 || M == 0) return 0;
    if (!points || !boxes) return (int)hipErrorInvalidValue;
    const int T = (M + PS_RADIUS_TILE - 1) / PS_RADIUS_TILE;
    return ps_launch(k_tile_boxes, dim3((unsigned)T, (unsigned)B), dim3(PS_WAVE), 0, reinterpret_cast<hipStream_t>(stream),
                     points, point_mask, boxes, M, T);
}

extern "C" int ps_radius_count_f32(const float* points, const uint8_t* point_mask, const float* queries,
                                   const uint8_t* query_mask, const int32_t* exclude, const int32_t* query_exclude, float cutoff,
                                   int include_self, const float* boxes, int32_t* count, int32_t* stats, int B, int M, int Q,
                                   void* stream) {
    if (stats)
        return sweep<STATS>(points, point_mask, queries, query_mask, exclude, query_exclude, cutoff, include_self, boxes, nullptr,
                            0, nullptr, nullptr, count, stats, B, M, Q, stream);
    return sweep<COUNT>(points, point_mask, queries, query_mask, exclude, query_exclude, cutoff, include_self, boxes, nullptr, 0,
                        nullptr, nullptr, count, nullptr, B, M, Q, stream);
}

extern "C" int ps_radius_fill_f32(const float* points, const uint8_t* point_mask, const float* queries,
                                  const uint8_t* query_mask, const int32_t* exclude, const int32_t* query_exclude, float cutoff,
                                  int include_self, const float* boxes, const long long* row_ptr, long long max_edges,
                                  int32_t* col, float* dist, int B, int M, int Q, void* stream) {
    return sweep<FILL>(points, point_mask, queries, query_mask, exclude, query_exclude, cutoff, include_self, boxes, row_ptr,
                       max_edges, col, dist, nullptr, nullptr, B, M, Q, stream);
}
