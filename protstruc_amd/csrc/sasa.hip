// K23 -- solvent-accessible surface area by Shrake & Rupley (1973): every atom carries S test points on the sphere of
// radius R_i = radius_i + probe around it, and a test point is buried where it lies inside another atom's sphere.
//
//   p_ik = x_i + R_i u_k                                              k = 0 .. S-1, u the table of directions
//   buried(i, k) iff some j != i, both in the mask, (isolate_i == isolate_j), with |p_ik - x_j|^2 < R_j^2
//   count_i = #{k : not buried(i, k)}                                 area_i = 4 pi R_i^2 count_i / S
//
// The sweep is the one of violation.hip: a workgroup is four waves that share 64 OWNERS, one atom per lane in registers;
// the columns are staged through LDS in tiles of 256 raw points, one per thread, COMPACTED while staging (a masked point
// never reaches LDS, so NaN there never meets arithmetic); wave w takes the compacted items w, w + 4, ... -- each read one
// address for the whole wave, an LDS broadcast.  A lane drops a column where, in fp32 on the squared distance,
// |x_i - x_j|^2 > (R_i + R_j)^2 (1 + 2^-20) -- no test point of i can then lie inside j, see near() -- and a wave whose 64
// owners all drop it (one ballot) skips the column; on a protein about 40 neighbours per atom are left.
//
// What is new against the other sweeps is the work per surviving pair: not one evaluation but S of them.  The lane walks
// the directions -- staged once per workgroup in LDS as doubles, read as broadcasts -- and evaluates
//   q = R_i u_k - (x_j - x_i),   q . q < R_j^2
// in DOUBLE: the coordinates and radii are fp32 values, so x_j - x_i and R are exact there and the decision is the one a
// float64 evaluation of the definition takes unless the two sides agree to 1e-12 A^2.  |u_k| is 1 only to fp32 rounding,
// which is as large as the margins that decide real structures, so no form that assumes |R_i u_k| = R_i is used.  The
// results are ORed into a mask of 256 bits per owner, eight 32-bit registers indexed statically (a fully unrolled word
// loop under the wave-uniform guard 32 w < S); a word that is already all ones in every surviving lane is skipped.  The
// four waves' masks are ORed through LDS and counted.  No pair list, no (B,M,M) or (B,M,S) tensor, no atomics: results
// repeat bit for bit.
#include "ps_common.hpp"
#include "owner_sweep.hpp"   // WAVES, compact_slot and the barrier protocol of staging a tile

#include <math.h>

#include "../../include/protstruc_hip.h"

namespace {

constexpr int OWNERS = PS_SASA_POINT_TILE;    // owners per workgroup = lanes per wave
constexpr int THREADS = OWNERS * WAVES;       // = raw points staged per tile
constexpr int MAX_DIRS = PS_SASA_MAX_SPHERE_POINTS;
constexpr int WORDS = MAX_DIRS / 32;          // mask registers per owner
static_assert(OWNERS == PS_WAVE, "one owner per lane");
static_assert(MAX_DIRS <= THREADS, "one thread stages one direction");

// Stage raw points [m0, m0 + THREADS) of structure b, valid ones only, in index order; returns how many.  An item is
// (x, y, z, radius) in `tile` and (raw index, isolate key) in `tags`.
__device__ __forceinline__ int stage_atoms(const float* __restrict__ pts, const float* __restrict__ radius,
                                           const uint8_t* __restrict__ point_mask, const int* __restrict__ isolate,
                                           size_t b, int M, int m0, float4* tile, int2* tags, int* wave_counts) {
    const int m = m0 + threadIdx.x;
    const bool valid = m < M && (!point_mask || point_mask[b * M + m] != 0);
    int total;
    const int slot = compact_slot(valid, wave_counts, total);
    if (valid) {
        const size_t at = b * M + m;
        const f3 x = load3(pts + at * 3);
        tile[slot] = make_float4(x.x, x.y, x.z, radius[at]);
        tags[slot] = make_int2(m, isolate ? isolate[at] : 0);
    }
    __syncthreads();
    return total;
}

// Whether a test point of the owner (at `me`, reach = (radius + probe) * the longest direction, rounded up) can lie
// inside the sphere of radius rj around xj.  A buried point has |x_i - x_j| < R_i |u_k| + R_j.  Every fp32 operation
// below errs by 2^-24 relative: five on the squared distance, eight on the bound, and the bound carries 1 + 2^-20 =
// 1 + 16 * 2^-24 and `reach` another 1 + 2^-21, so a pair that buries a point always passes.
__device__ __forceinline__ bool near(f3 me, float reach, f3 xj, float rj) {
    const f3 diff = sub3(me, xj);
    const float d2 = norm_sq3(diff.x, diff.y, diff.z);
    const float sum = reach + rj;
    return d2 <= (sum * sum) * (1.0f + 0x1p-20f);
}

__global__ __launch_bounds__(THREADS) void k_solvent_accessibility(const float* __restrict__ pts,
                                                                   const float* __restrict__ radius,
                                                                   const uint8_t* __restrict__ point_mask,
                                                                   const int* __restrict__ isolate,
                                                                   const float* __restrict__ sphere, float probe,
                                                                   int* __restrict__ count, float* __restrict__ area,
                                                                   int M, int S) {
    __shared__ __attribute__((aligned(16))) float4 tile[THREADS];
    __shared__ int2 tags[THREADS];
    __shared__ __attribute__((aligned(16))) double dirs[MAX_DIRS * 4];   // (x, y, z, unused): two 16-byte broadcast reads
    __shared__ unsigned wave_masks[WAVES * WORDS * OWNERS];
    __shared__ float wave_longest[WAVES];
    __shared__ int wave_counts[WAVES];
    const size_t b = blockIdx.y;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int i = blockIdx.x * OWNERS + lane;
    const bool own = i < M && (!point_mask || point_mask[b * M + i] != 0);

    // the directions as doubles, and the longest of them rounded up to fp32: the table need not be of unit vectors
    float longest = 0.0f;
    if ((int)threadIdx.x < S) {
        const f3 u = load3(sphere + threadIdx.x * 3);
        double* d = dirs + threadIdx.x * 4;
        d[0] = (double)u.x;
        d[1] = (double)u.y;
        d[2] = (double)u.z;
        d[3] = 0.0;
        longest = (float)sqrt(((double)u.x * u.x + (double)u.y * u.y) + (double)u.z * u.z) * (1.0f + 0x1p-22f);
    }
#pragma unroll
    for (int off = PS_WAVE / 2; off > 0; off >>= 1) longest = fmaxf(longest, __shfl_xor(longest, off));
    if (lane == 0) wave_longest[wave] = longest;
    __syncthreads();
    longest = fmaxf(fmaxf(wave_longest[0], wave_longest[1]), fmaxf(wave_longest[2], wave_longest[3]));
    longest = fmaxf(longest, 1.0f) * (1.0f + 0x1p-21f);

    // an owner that is masked or past the end holds zeros and takes no part: its coordinates and radius are never read
    f3 me = f3{0.0f, 0.0f, 0.0f};
    float my_radius = 0.0f;
    int my_key = 0;
    if (own) {
        const size_t at = b * M + i;
        me = load3(pts + at * 3);
        my_radius = radius[at];
        my_key = isolate ? isolate[at] : 0;
    }
    const double Ri = (double)my_radius + (double)probe;
    const float reach = (my_radius + probe) * longest;
    unsigned buried[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) buried[w] = 0u;

    for (int m0 = 0; m0 < M; m0 += THREADS) {
        const int n = stage_atoms(pts, radius, point_mask, isolate, b, M, m0, tile, tags, wave_counts);
        for (int j = wave; j < n; j += WAVES) {
            const float4 o = tile[j];
            const int2 tag = tags[j];
            const bool inc = own && tag.x != i && tag.y == my_key && near(me, reach, f3{o.x, o.y, o.z}, o.w + probe);
            if (__ballot(inc) == 0ull) continue;   // no owner of this wave comes near column j
            const double dx = (double)o.x - (double)me.x, dy = (double)o.y - (double)me.y, dz = (double)o.z - (double)me.z;
            const double Rj = (double)o.w + (double)probe, Rj2 = Rj * Rj;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                if (32 * w < S) {   // wave-uniform
                    const int bits = S - 32 * w < 32 ? S - 32 * w : 32;
                    const unsigned full = bits == 32 ? 0xffffffffu : (1u << bits) - 1u;
                    if (__ballot(inc && buried[w] != full) == 0ull) continue;   // nothing left to bury in this word
                    unsigned word = 0u;
                    for (int t = 0; t < bits; ++t) {
                        const double2* u = reinterpret_cast<const double2*>(dirs + (32 * w + t) * 4);
                        const double2 uxy = u[0], uz = u[1];
                        const double qx = __builtin_fma(Ri, uxy.x, -dx), qy = __builtin_fma(Ri, uxy.y, -dy),
                                     qz = __builtin_fma(Ri, uz.x, -dz);
                        const double qq = __builtin_fma(qz, qz, __builtin_fma(qy, qy, qx * qx));
                        word |= qq < Rj2 ? 1u << t : 0u;
                    }
                    buried[w] |= inc ? word : 0u;
                }
            }
        }
    }
    // the four waves' masks ORed, then counted; bits at and above S are never set
#pragma unroll
    for (int w = 0; w < WORDS; ++w) wave_masks[(wave * WORDS + w) * OWNERS + lane] = buried[w];
    __syncthreads();
    if (wave != 0 || i >= M) return;
    int hidden = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        unsigned word = 0u;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) word |= wave_masks[(v * WORDS + w) * OWNERS + lane];
        hidden += __popc(word);
    }
    // a masked owner gets exact zeros by selection; the area is rounded to float once
    const int open = own ? S - hidden : 0;
    count[b * M + i] = open;
    area[b * M + i] = own ? (float)((4.0 * M_PI) * (Ri * Ri) * (double)open / (double)S) : 0.0f;
}

}  // namespace

extern "C" int ps_solvent_accessibility_f32(const float* points, const float* radius, const uint8_t* point_mask,
                                            const int32_t* isolate, const float* sphere, float probe, int32_t* count,
                                            float* area, int B, int M, int S, void* stream) {
    if (!points || !radius || !sphere || !count || !area || B < 0 || M < 0 || B > 65535 || M > (1 << 24) || S < 1 ||
        S > PS_SASA_MAX_SPHERE_POINTS || !(probe >= 0.0f) || isinf(probe))
        return (int)hipErrorInvalidValue;
    if (B == 0 || M == 0) return 0;
    return ps_launch(k_solvent_accessibility, dim3((unsigned)((M + OWNERS - 1) / OWNERS), (unsigned)B), dim3(THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), points, radius, point_mask, isolate, sphere, probe, count, area,
                     M, S);
}
