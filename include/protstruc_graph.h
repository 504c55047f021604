/*
 * protstruc_graph.h -- C ABI of the radius-graph kernels (K47, K48) of libprotstruc_hip.so: every neighbour of every query
 * within a cutoff as a variable-length list in CSR form.
 *
 * These entry points are compiled into the same shared library as those of protstruc_hip.h; they are declared in a header
 * of their own, with a version number of their own, so that adding them left PS_ABI_VERSION and every declaration of the
 * other headers as they were.
 *
 * Conventions (all entry points), those of protstruc_hip.h:
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains memory;
 *   - tensors are contiguous and need only the alignment of their element; masks are one-byte booleans (0 / 1; any
 *     non-zero input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched, and an empty batch returns 0 without touching a device;
 *   - B is 0 .. 65535, M and Q are 0 .. 2^24; offsets are 64-bit throughout; no kernel uses an atomic, and repeated runs
 *     agree bit for bit.
 *
 * DEFINITION (the predicate is K24's, ps_nearest_neighbors_f32, with no k).  points is [B][M][3], the candidates; queries is
 * [B][Q][3] or NULL: the points themselves (the SELF GRAPH, Q == M, query_mask and query_exclude NULL: the points' own are
 * used).  point_mask [B][M], query_mask [B][Q] bytes or NULL (all); exclude [B][M], query_exclude [B][Q] int32 keys or
 * NULL, together or not at all.
 *     X = (double)x      dx = Xj.x - Xq.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz     in double, in this order
 *     j is a neighbour of q iff  both are in their masks, their keys differ (where keys are given), j != q in the self
 *                                graph (unless include_self), d2 is finite and d2 <= C2 = (double)cutoff * (double)cutoff
 * The library is built with -ffp-contract=off: every product and sum is rounded on its own, so a numpy float64
 * restatement gives the same bits.  cutoff is positive and finite.  A point with a NaN or infinite coordinate is nobody's
 * neighbour and, as a query, has none (its d2 would not be finite); coordinates under a mask are never read.
 *
 * RESULT.  The rows are the B * Q queries in (b, q) order.
 *     count   [B][Q] int32       the number of neighbours of each query
 *     row_ptr [B * Q + 1] int64  the exclusive prefix sum of count, row_ptr[0] = 0 -- formed BY THE CALLER between the two
 *                                sweeps (a prefix sum is no kernel of this library)
 *     col     [E] int32          the neighbours' indices into the M axis of their own structure, ASCENDING in j within a row
 *     dist    [E] float          (float)sqrt(d2), rounded once
 * In the self graph without keys (q, j) is an edge iff (j, q) is, with the same bits in dist: d2 is a sum of squares of
 * differences, and negating a difference changes no square.  Wherever a row has at most 64 entries it is the row of
 * ps_nearest_neighbors_f32 at k = 64 with the same arguments, as a set, bit for bit in dist.
 *
 * HOW.  K47 computes, once per call, the box of every block of PS_RADIUS_TILE consecutive candidate slots and of its four
 * quarters.  K48 is ONE sweep compiled twice, with a counting and with a writing sink: a wave owns 64 consecutive queries,
 * one per lane, and walks the blocks in ascending order, which is what makes a row ascending in j with no sort.  A block
 * is dropped for the whole wave by the box test below against the box of the wave's queries; in a block that survives, a
 * lane takes part in a quarter only if its own query passes the same test against that quarter's box, and a quarter no
 * lane takes part in is skipped.  What is left is decided in double, by the definition.  Both sweeps evaluate the same
 * predicate on the same inputs, so they agree; the writing sweep takes every row's position from row_ptr.
 *
 * THE BOX TEST (csrc/radius_box.hpp holds the code and the full argument).  For the box A of some queries and the box
 * B of some candidates -- lo and hi of their finite, unmasked points, exact in float32 --
 *     gap_a = max(0, A.lo[a] - B.hi[a], B.lo[a] - A.hi[a])          G = (gap_x*gap_x + gap_y*gap_y) + gap_z*gap_z      in float32
 *     B is dropped  iff  B holds no point  or  G > fl32(C2) * (1 + 2^-20) + 2^-126
 * STRICTLY CONSERVATIVE: the real squared distance of any pair (q in A, j in B) is at least the real sum of squared gaps S;
 * G carries five roundings of 2^-24 relative (the subtraction, the square, two sums; max is exact), the bound three (the
 * conversion of C2, the product, the sum), the double d2 five of 2^-53; 1 + 2^-20 = 1 + 16 * 2^-24 covers their sum
 * twice over, and 2^-126 covers every underflow (each errs by at most 2^-149).  A gap that overflows to +inf is wider
 * than any finite cutoff; a bound that overflows to +inf drops nothing.  So no block that holds a neighbour of a query
 * of the wave is ever dropped, whatever the order of the points: on shuffled input the answer is the same, only slower.
 */
#ifndef PROTSTRUC_GRAPH_H
#define PROTSTRUC_GRAPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_graph_api() returns the library's.  Launches nothing. */
#define PS_GRAPH_API 1
int ps_graph_api(void);

#define PS_RADIUS_TILE 64          /* candidate slots per block: one per lane of the wave that stages it */
#define PS_RADIUS_BOX_FLOATS 40    /* floats of `boxes` per block: five boxes of 8 -- the block's, then its four quarters' */
#define PS_RADIUS_STATS 6          /* int32 counters per wave of queries in `stats` */

/*
 * K47.  The boxes of the candidates.  boxes is [B][ceil(M / PS_RADIUS_TILE)][5][8] float, written in full: entry 0 of a block
 * is the box of its slots m with m < M, point_mask != 0 and three finite coordinates, entries 1 .. 4 those of its quarters
 * of 16 slots.  A box is lo.x lo.y lo.z hi.x hi.y hi.z n 0 with n the number of such points as a float; an empty box is
 * +inf +inf +inf -inf -inf -inf 0 0.
 *
 * Refused: B outside 0 .. 65535, M outside 0 .. 2^24; with B > 0 and M > 0 also a NULL points or boxes.
 */
int ps_radius_tile_boxes_f32(const float* points, const uint8_t* point_mask, float* boxes, int B, int M, void* stream);

/*
 * K48, counting.  count [B][Q] int32 is written in full.  boxes is what K47 wrote for the same points and point_mask.
 * stats is NULL or [B][ceil(Q / 64)][PS_RADIUS_STATS] int32, written in full, per wave of queries: blocks walked; of those
 * dropped by the wave's box test (empty blocks included); of the rest dropped because no lane's own test kept a quarter;
 * quarters of staged blocks walked; of those skipped; columns that reached the double test.  A wave with no query to serve
 * walks nothing.  (No atomics: the caller sums.)
 *
 * Refused: B outside 0 .. 65535, M or Q outside 0 .. 2^24, a cutoff that is not positive and finite, the self graph
 * (queries NULL) with Q != M or a query_mask or a query_exclude, queries with only one of exclude and query_exclude; with
 * B, M and Q > 0 also a NULL points, boxes or count.  With B or Q zero nothing is launched; with M zero count is cleared.
 */
int ps_radius_count_f32(const float* points, const uint8_t* point_mask, const float* queries, const uint8_t* query_mask,
                        const int32_t* exclude, const int32_t* query_exclude, float cutoff, int include_self,
                        const float* boxes, int32_t* count, int32_t* stats, int B, int M, int Q, void* stream);

/*
 * K48, writing.  The same arguments and the same sweep; row_ptr [B * Q + 1] int64 is the exclusive prefix sum of what the
 * counting sweep wrote.  col and dist hold max_edges entries: the entry at position p of the edge list is written iff
 * p < max_edges, so a list that is longer than the buffers is cut, never written past them (the caller sees
 * row_ptr[B * Q] > max_edges).  Entries from row_ptr[B * Q] on are not touched.
 *
 * Refused: as the counting sweep; max_edges < 0; with B, M, Q and max_edges > 0 also a NULL row_ptr, col or dist.
 */
int ps_radius_fill_f32(const float* points, const uint8_t* point_mask, const float* queries, const uint8_t* query_mask,
                       const int32_t* exclude, const int32_t* query_exclude, float cutoff, int include_self,
                       const float* boxes, const long long* row_ptr, long long max_edges, int32_t* col, float* dist,
                       int B, int M, int Q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_GRAPH_H */
