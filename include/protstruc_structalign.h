/*
 * protstruc_structalign.h -- C ABI of the structure-alignment kernels (K41 - K44) of libprotstruc_hip.so: a Needleman-Wunsch
 * pass with TM-align's gap rule, TM-align's secondary structure of a CA trace, and the alignment of two point sets of
 * different lengths WITHOUT a given correspondence, by alternating that dynamic programming with the seeded superposition
 * search of protstruc_superpose.h.
 *
 * These entry points are compiled into the same shared library as those of protstruc_hip.h and follow the same
 * conventions; they are declared in a header of their own, with a version number of their own, so that adding them
 * left PS_ABI_VERSION and every declaration of the other headers as they were.
 *
 * Conventions (all entry points), those of protstruc_superpose.h:
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains memory (the
 *     launchers that need scratch memory write it into a `workspace` the caller supplies, of
 *     ps_structalign_workspace_bytes(B, Ma, Mb) bytes, of any alignment; it needs no clearing and its contents after the
 *     call are unspecified);
 *   - tensors are contiguous and need only the alignment of their element; masks are one-byte booleans (0 / 1; any
 *     non-zero input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched, and B = 0 returns 0 without touching a device;
 *   - B is 0 .. 65535; no kernel uses an atomic, and repeated runs agree bit for bit;
 *   - all geometry is double arithmetic on the float32 inputs, every product and sum rounded on its own (no fused
 *     multiply-add); every 3x3 solve is the one of ps_kabsch_f32.
 *
 * POINTS.  a[B][Ma][3] with mask_a[B][Ma] (NULL: all) and b[B][Mb][3] with mask_b[B][Mb], Ma and Mb 1 ..
 * PS_STRUCTALIGN_MAX_POINTS.  The unmasked slots of a structure, in order, are its n_a and n_b points; "point i" below
 * counts them from 0.  Entries under a mask are never read: NaN there reaches nothing.  A MAP is int32[B][Ma]: for a slot
 * of `a` the SLOT of `b` aligned to it, or -1; strictly increasing over its entries >= 0, and -1 under mask_a.
 */
#ifndef PROTSTRUC_STRUCTALIGN_H
#define PROTSTRUC_STRUCTALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_structalign_api() returns the library's.  Launches nothing. */
#define PS_STRUCTALIGN_API 1
int ps_structalign_api(void);

#define PS_STRUCTALIGN_MAX_POINTS 1024      /* Ma and Mb: both structures' points and the DP front live in LDS */
#define PS_STRUCTALIGN_MAX_ITERATIONS 20    /* DP passes of one refinement of one start under one gap value */

/*
 * The size in bytes of the `workspace` of ps_nw_align_f32 and ps_structure_align_f32 for these B, Ma, Mb; -1 for arguments
 * the launchers refuse.  Host function; launches nothing.
 */
long long ps_structalign_workspace_bytes(int B, int Ma, int Mb);

/*
 * K41.  DEFINITION of the DP: a Needleman-Wunsch pass with TM-align's gap rule over scores S[i][j] held as double,
 * 0 <= i < n_a, 0 <= j < n_b, and a gap g <= 0.  With val[i][0] = val[0][j] = 0 and path[.][0] = path[0][.] = false, for
 * i = 1 .. n_a and j = 1 .. n_b:
 *     d = val[i-1][j-1] + S[i-1][j-1]
 *     h = val[i-1][j] + (path[i-1][j] ? g : 0)
 *     v = val[i][j-1] + (path[i][j-1] ? g : 0)
 *     if d >= h and d >= v:  path[i][j] = true,   val[i][j] = d
 *     else:                  path[i][j] = false,  val[i][j] = (v >= h ? v : h)
 * The trace starts at (i, j) = (n_a, n_b): where path[i][j] is true, points i-1 and j-1 are aligned and the trace steps to
 * (i-1, j-1); otherwise, with h and v as above, it steps to (i, j-1) if v >= h and to (i-1, j) if not.  It ends at i = 0 or
 * j = 0.  A cell is three additions and two comparisons in a fixed order: the result is defined bit for bit, ties included.
 *
 * ps_nw_align_f32 runs it on the caller's score[B][Ma][Mb] (float, widened to double; S[i][j] is the entry at the slots of
 * points i and j; entries at masked slots are never read) and writes map[B][Ma], n_aligned[B] (int32, the pairs of the map)
 * and value[B] = (float)val[n_a][n_b].  n_a = 0 or n_b = 0: a map of -1, 0 pairs, value 0.
 * Refused: Ma or Mb outside 1 .. 1024, a gap that is > 0 or not finite, a NULL among score, workspace, map, n_aligned, value.
 */
int ps_nw_align_f32(const float* score, const uint8_t* mask_a, const uint8_t* mask_b, float gap, void* workspace, int32_t* map,
                    int32_t* n_aligned, float* value, int B, int Ma, int Mb, void* stream);

/*
 * K44.  The secondary structure of a CA trace as TM-align's make_sec assigns it: labels[B][M] (int8), -1 under the mask.
 * x[B][M][3], mask[B][M] or NULL, M 1 .. PS_STRUCTALIGN_MAX_POINTS.  For point i with 2 <= i <= n - 3 (points counted
 * after masking: a masked slot does not separate its neighbours, and CHAIN BREAKS ARE NOT LOOKED AT: the five points
 * i-2 .. i+2 are taken as consecutive residues whatever lies between them) with the double distances
 *     d13 = |x(i-2) - x(i)|,    d14 = |x(i-2) - x(i+1)|,  d15 = |x(i-2) - x(i+2)|,
 *     d24 = |x(i-1) - x(i+1)|,  d25 = |x(i-1) - x(i+2)|,  d35 = |x(i) - x(i+2)|,
 * each sqrt((e0 e0 + e1 e1) + e2 e2) of the double differences e:
 *     1 (helix)   if |d15 - 6.37|, |d14 - 5.18|, |d25 - 5.18|, |d13 - 5.45|, |d24 - 5.45| and |d35 - 5.45| are all < 2.1
 *     2 (strand)  otherwise, if the same six against 13.0, 10.4, 10.4, 6.1, 6.1, 6.1 are all < 1.42
 *     3 (turn)    otherwise, if d15 < 8.0
 *     0           otherwise, and for the two points at either end (every point when n < 5)
 * Refused: M outside 1 .. 1024, a NULL among x, labels.
 */
int ps_ca_secondary_structure_f32(const float* x, const uint8_t* mask, int8_t* labels, int B, int M, void* stream);

/*
 * K42 / K43.  The alignment of a onto b (K43 picks between the two starts K42 ran).  d0[B] is given by the caller, > 0
 * and finite (anything else is the caller's error and gives unspecified results for that structure), and
 * s(d^2) = 1 / (1 + d^2 / (d0 d0)).
 *
 * DEFINITION, per pair of structures.
 *   fit-search(map).  The pairs of the map, in order, are n_p points (a_k, b_k).  K39's chain, exactly as
 *     protstruc_superpose.h defines it -- TM objective with param d0, its radii, the doubling, 20 iterations --, is run from
 *     those seeds of K39's seed table of n_p points whose length is >= max(n_p >> 1, 4): the whole set and the fragments of
 *     the second length (at most five chains); for n_p < 4 the table's single seed.  The result (S, R, t) is that of the
 *     chain with the greatest S, the lowest seed on ties.
 *   Start 0, threading.  need = max(min(n_a, n_b) / 2, min(5, n_a, n_b)), the division rounding down.  For every offset k
 *     from -(n_a - need) to n_b - need, a_i is paired with b_(i+k) over the overlap, one Kabsch fit of all those pairs is
 *     made and S_k = sum s(d^2) taken over them.  The start is the pairing of the greatest S_k, the lowest k on ties.
 *   Start 1, secondary structure (left out when use_ss = 0): the map of the DP with S[i][j] = 1.0 if the labels of K44 of
 *     point i of a and point j of b are equal, else 0.0, and g = -1.
 *   Refinement of a start m; `best` starts at -infinity and belongs to the start:
 *       (S, T0) = fit-search(m); if S > best: best = (S, m, T0)
 *       for g in ((double)(float)-0.6, 0.0):
 *           prev = m; T = T0
 *           at most PS_STRUCTALIGN_MAX_ITERATIONS times:
 *               m' = the map of the DP with S[i][j] = s(d^2(T a_i, b_j)) and gap g       (d^2 in K39's order of operations)
 *               if m' has no pair: stop
 *               (S', T) = fit-search(m'); if S' > best: best = (S', m', T)
 *               if m' == prev: stop
 *               prev = m'
 *   Result.  The best of start 0, or that of start 1 if it is strictly greater.
 * As in K39 the order of the sums over points inside a fit is left open.
 *
 * Outputs: map[B][Ma]; n_aligned[B] (int32); score[B] = (float)(S_best / min(n_a, n_b)); R[B][3][3] and t[B][3] rounded to
 * float; n_points[B][2] = (n_a, n_b) (int32); start[B] (int32) = the start that gave the best, 0 or 1.  n_a = 0 or
 * n_b = 0: a map of -1, 0 pairs, score 0, start 0 and NaN in R and t.
 *
 * This is not the TM-align program: two starts instead of five (no fragment starts), K39's search instead of TM-score's,
 * no circular permutation, and d0 is the caller's for the search and the result alike.
 *
 * Refused: Ma or Mb outside 1 .. 1024, a NULL among a, b, d0, workspace, map, n_aligned, score, R, t, n_points, start.
 */
int ps_structure_align_f32(const float* a, const uint8_t* mask_a, const float* b, const uint8_t* mask_b, const float* d0,
                           int use_ss, void* workspace, int32_t* map, int32_t* n_aligned, float* score, float* R, float* t,
                           int32_t* n_points, int32_t* start, int B, int Ma, int Mb, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_STRUCTALIGN_H */
