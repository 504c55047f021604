// Host-side pieces that K3 (pairwise_angles.hip) and the fused featuriser (featuriser.hip, featuriser_backward.hip) share:
// the kernels' argument and vector types, the device / CU lookup, the big-LDS attribute, the LDS budgets, the task and
// tile sizing both dispatchers use, and the launch context.
//
// Launch or record: the dispatchers either launch or only RECORD what they would launch (ps_k3_plan_f32,
// ps_featuriser_plan_f32).  Every K3 / featuriser launch goes through k3_go, so the plan a caller reads is by construction
// the dispatch a launch takes: same predicates, same grid, same LDS size (K1 has the same arrangement: k1_go).
//
// Everything here sits in the unnamed namespace: each translation unit has its own copy (the CU cache of k3_cu_count
// included: a constant of the device, not library state).
#pragma once

#include "ps_common.hpp"
#include "../../include/protstruc_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace {

struct AtomSel {
    int atom[4];
};

typedef float k3_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t k3_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t k3_u32x2 __attribute__((ext_vector_type(2)));

// The device a launch on `stream` runs on: the stream's own device; the calling thread's current device for the null stream
// (a C-ABI caller may launch on a stream of device 1 while device 0 is current: grid size and the LDS attribute are that
// device's business, not the current one's)
inline int k3_device_of(hipStream_t stream) {
    int dev = 0;
    if (stream) {
        hipDevice_t d;
        if (hipStreamGetDevice(stream, &d) == hipSuccess) return (int)d;
    }
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    return dev;
}

// CUs of that device (cached per ordinal; a constant of the device, not library state)
inline int k3_cu_count(hipStream_t stream) {
    static int cached[64] = {0};
    const int dev = k3_device_of(stream);
    if (dev < 0 || dev >= 64) return 256;
    int n = __atomic_load_n(&cached[dev], __ATOMIC_RELAXED);
    if (n <= 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        __atomic_store_n(&cached[dev], n, __ATOMIC_RELAXED);
    }
    return n;
}

// More than 64 KB of dynamic LDS has to be allowed once per kernel AND per device (function attributes belong to the module
// a device loaded; hipFuncSetAttribute acts on the CURRENT device, so the stream's device is made current around it when it
// is another one).  `done` is the kernel instantiation's own table; idempotent, so a race between two threads is harmless.
template <typename K>
inline int k3_allow_big_lds(K kernel, unsigned long long (&done)[1], hipStream_t stream) {
    const int dev = k3_device_of(stream);
    if (dev < 0 || dev >= 64) return (int)hipErrorInvalidDevice;
    const unsigned long long bit = 1ull << dev;
    if (__atomic_load_n(&done[0], __ATOMIC_ACQUIRE) & bit) return 0;
    int cur = dev;
    (void)hipGetDevice(&cur);
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return (int)hipErrorInvalidDevice;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(160 * 1024 - 256));
    if (cur != dev) (void)hipSetDevice(cur);
    if (e != hipSuccess) return (int)e;
    __atomic_fetch_or(&done[0], bit, __ATOMIC_RELEASE);
    return 0;
}

// threads of a full-width sweep workgroup: four waves per SIMD with 128 VGPRs each -- two with 256 for the faithful chains at
// four columns per lane (the library-order chains keep ~2x the values live)
constexpr int k3_sweep_threads(int NC, bool FAITHFUL) { return FAITHFUL && NC == 4 ? 512 : 1024; }
constexpr size_t K3_LDS_MAX = 160 * 1024 - 256;   // the most dynamic LDS a workgroup of the sweep kernels asks for
constexpr size_t K3_LDS_ONE_PER_CU = 80 * 1024;   // with its few static bytes on top, two such workgroups do not fit a CU
constexpr size_t K3_LDS_TWO_PER_CU = 80 * 1024 - 256;   // exactly two such workgroups fit a CU (three would need 240 KB)

// Rows per task (even, 2..8).  The 16 waves of a workgroup pull the tasks of one (structure, strip) segment at a time, and
// the pulling only evens out the SIMD arbiter's oldest-first order if a segment has several tasks per wave: a segment of
// `rows` rows gets about 64 tasks (N = 512: 8 rows per task, 256: 4, 128: 2; with one task per wave a 128-residue segment
// ended when its slowest wave did: 61 -> 5x us at 2^25 pairs, profiles/r04_k3_shapes.log).  A task costs one LDS atomic.
inline int k3_rows_per_task(int rows, int min_rows) {
    const int ch = (rows / 64) & ~1;
    return std::min(8, std::max(min_rows, ch));
}

// Tiles of two row pairs x FOUR columns (a row of the tile is one 16-byte store) save ~10 % of the instructions of the
// two-column tiles, which must not go to idle lanes: a structure's tiles fill whole tasks of 64, and the wide tiles are taken
// unless they idle > 8 % more lanes of the last task (K3, N = 36: 81 tiles in 2 tasks against 162 in 3: 113 against 105 us;
// N = 48: 144 in 3 against 288 in 5: level).  TR: the structure's tile rows.  Shared by k3_flat and k3_featurise_tiles.
inline bool k3_wide_tiles_pay(unsigned TR, int N) {
    const unsigned ft_w = TR * ((unsigned)N / 4), ft_n = TR * ((unsigned)N / 2);
    const unsigned long long lanes_w = 64ull * ((ft_w + 63) / 64) * 2, lanes_n = 64ull * ((ft_n + 63) / 64);   // in narrow-tile units
    return lanes_w * 100 <= lanes_n * 108;
}

// One-column kernels: a workgroup as wide as the chain needs (whole waves, at most 256 lanes) -- with 256 lanes for a
// 64-residue chain three of four waves computed pairs that do not exist.
inline int k3_one_column_threads(int N) { return N >= 256 ? 256 : 64 * ((N + 63) / 64); }

// ---- launch context (launch or record: see the head of this file) ----
struct K3Go {
    hipStream_t s;
    ps_k3_plan* plan;   // non-null: record only, launch nothing, make no HIP call
    int cus;            // compute units of the device the launch is for
};

struct K3Shape {        // what the plan reports besides the kernel's name and launch geometry
    int nc = 1, vec = 0, skips = 0, mask_mode = 0, wt = 0, faithful = 0, rows_per_task = 0, wgs_per_cu = 0, structs_per_segment = 0;
    unsigned n_tasks = 0, tasks_per_wg = 0;
};

template <typename... KArgs, typename... Args>
inline int k3_go(const K3Go& go, const char* family, const char* name, const K3Shape& sh, void (*kernel)(KArgs...),
                 unsigned long long (*prepared)[1], dim3 grid, dim3 block, size_t dyn, unsigned static_lds, Args&&... args) {
    if (!go.plan) {
        if (prepared)
            if (const int e = k3_allow_big_lds(kernel, *prepared, go.s)) return e;
        return ps_launch(kernel, grid, block, dyn, go.s, static_cast<Args&&>(args)...);
    }
    ps_k3_plan& pl = *go.plan;
    snprintf(pl.family, sizeof pl.family, "%s", family);
    snprintf(pl.kernel, sizeof pl.kernel, "%s", name);
    pl.n_launches = 1;
    pl.columns_per_lane = sh.nc; pl.vector_stores = sh.vec; pl.skips_dead_groups = sh.skips; pl.mask_store_mode = sh.mask_mode;
    pl.write_through = sh.wt; pl.faithful = sh.faithful; pl.rows_per_task = sh.rows_per_task; pl.workgroups_per_cu = sh.wgs_per_cu;
    pl.structures_per_segment = sh.structs_per_segment;
    pl.n_workgroups = grid.x; pl.threads_per_workgroup = (int)block.x; pl.lds_bytes = (unsigned)dyn + static_lds;
    pl.n_tasks = sh.n_tasks; pl.tasks_per_workgroup = sh.tasks_per_wg;
    return 0;
}

inline void k3_plan_reset(ps_k3_plan* plan) {
    const int sz = plan->struct_size;
    memset(plan, 0, sizeof *plan);
    plan->struct_size = sz;
    snprintf(plan->family, sizeof plan->family, "empty");
}

}  // namespace
