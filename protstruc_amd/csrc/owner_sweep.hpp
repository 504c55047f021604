// What the owner-sweep kernels -- fape.hip, lddt.hip, violation.hip, sasa.hip, dssp.hip -- share character for character:
// the number of waves of a workgroup and the stream compaction they stage their column tiles with.  Everything else of a
// sweep (the item layout, the staging function, the pair loop, the epilogue) differs per kernel and stays in its file.
//
// A workgroup is WAVES waves of PS_WAVE lanes; a tile is one raw item per thread, and only the valid items reach LDS,
// packed in index order.  compact_slot gives a thread the place of its item: a ballot and a popcount inside the wave, the
// waves' counts exchanged through WAVES ints of LDS.
//
// The barrier protocol.  compact_slot holds two __syncthreads, and the callers rely on both:
//   1. before wave_counts is written -- every reader of the PREVIOUS tile is done, both of wave_counts and of the staged
//      items, which the caller overwrites right after this call.  It is what lets a kernel loop "stage, barrier, sweep"
//      with no barrier of its own at the end of the sweep;
//   2. after it is written -- every wave sees all WAVES counts before it sums them.
// The caller stores its item at the returned slot and places ONE more barrier before anyone reads the tile.  Because of
// the barriers every thread of the workgroup must call compact_slot, the threads without a valid item (valid = false)
// included, and from uniform control flow: never under a condition that differs between threads.
#pragma once

#include "ps_common.hpp"

constexpr int WAVES = 4;

// The slot of this thread's item -- the number of valid items before it in the workgroup -- and the number of valid items
// in all (the same in every thread).  wave_counts: WAVES ints of LDS.  Two barriers; every thread of the workgroup must
// call it.
__device__ __forceinline__ int compact_slot(bool valid, int* wave_counts, int& total) {
    const unsigned long long ballot = __ballot(valid);
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    __syncthreads();   // the previous tile's readers of wave_counts and of the staged items are done
    if (lane == 0) wave_counts[wave] = __popcll(ballot);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int c = wave_counts[w];
        base += w < wave ? c : 0;
        total += c;
    }
    return base + before;
}
