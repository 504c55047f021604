/*
 * protstruc_ensemble.h -- C ABI of the ensemble kernels (K45, K46) of libprotstruc_hip.so: the matrix of RMSDs after optimal
 * superposition between every member of one batch of structures and every member of another (or of the same batch), and
 * the clustering of such a matrix by the rule of Daura et al. ("gromos").
 *
 * These entry points are compiled into the same shared library as those of protstruc_hip.h and follow the same
 * conventions; they are declared in a header of their own, with a version number of their own, so that adding them
 * left PS_ABI_VERSION and every declaration of the other headers as they were.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains memory (the
 *     clustering keeps its bit matrix in a `workspace` the caller supplies);
 *   - tensors are contiguous and need only the alignment of their element; masks are one-byte booleans (0 / 1; any
 *     non-zero input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched, and an empty batch returns 0 without touching a device;
 *   - batch sizes are 0 .. 65535; offsets are 64-bit throughout; no kernel uses an atomic, and repeated runs agree bit
 *     for bit;
 *   - all geometry is double arithmetic on the float32 inputs, every product and sum rounded on its own (no fused
 *     multiply-add) EXCEPT the sums over the points of K45, where it says so; the 3x3 solve is the one of ps_kabsch_f32
 *     (one-sided Jacobi in double, a proper rotation for every covariance).
 */
#ifndef PROTSTRUC_ENSEMBLE_H
#define PROTSTRUC_ENSEMBLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_ensemble_api() returns the library's.  Launches nothing. */
#define PS_ENSEMBLE_API 1
int ps_ensemble_api(void);

#define PS_CLUSTER_MAX_ITEMS 4096        /* B of the clustering: the degrees of a matrix live in LDS */
#define PS_RMSD_MATRIX_MAX_POINTS 2147483631   /* M of K45, INT_MAX - 16: the points are walked in chunks of 16 by an int */

/*
 * K45.  The matrix of superposed RMSDs.  a is [Ba][M][3], mask_a is [Ba][M] bytes or NULL (all points); b is [Bb][M][3] and
 * mask_b [Bb][M] or NULL.  b == NULL is SELF MODE: it requires Bb == Ba and mask_b == NULL and compares a with itself.
 * Ba, Bb are 0 .. 65535 and M is 1 .. PS_RMSD_MATRIX_MAX_POINTS: the points are streamed, nothing limits M to an LDS size.  Outputs
 * rmsd[Ba][Bb] float and count[Ba][Bb] int32 (or NULL).
 *
 * DEFINITION, per pair (i, j).
 *   The points of the pair are the p with mask_a[i][p] != 0 and mask_b[j][p] != 0; n is their number.
 *   The origin o of a structure is the double value of its own lowest-index point whose own mask is non-zero (it does not
 *   depend on the partner).  x_p = a[i][p] - o_a(i) and y_p = b[j][p] - o_b(j), both in double.  Over the pair's points
 *       Sx[c] = sum x_c,  Sy[d] = sum y_d,  Sxy[c][d] = sum x_c y_d,  Qx = sum |x|^2,  Qy = sum |y|^2
 *   with |x|^2 = (x_0 x_0 + x_1 x_1) + x_2 x_2 formed per point.  The sums run over p ascending, one term after the other,
 *   and each term may enter by a fused multiply-add (this is the only place where one is used).  Then, every operation
 *   rounded on its own,
 *       H[c][d] = Sxy[c][d] - (Sx[c] Sy[d]) / n
 *       gx = Qx - ((Sx_0 Sx_0 + Sx_1 Sx_1) + Sx_2 Sx_2) / n,   gy likewise
 *       R = ps_kabsch_solve(H)                     -- the solve of K37 and ps_kabsch_f32, unchanged
 *       tr = sum over d, then c, of R[d][c] H[c][d]
 *       msd = max(0, ((gx + gy) - 2 tr) / n),      rmsd = (float)sqrt(msd),      count = n
 *   n = 0 gives rmsd NaN and count 0.  A pair with a non-finite coordinate among its points gives NaN.  Coordinates under
 *   a structure's own mask are selected away when the points are staged, never multiplied: NaN there reaches nothing; and
 *   a non-finite coordinate of one structure at a point that the partner's mask leaves out reaches nothing either (unless
 *   it is the structure's origin, which enters every x_p).
 *
 * SELF MODE.  Entries with i < j are computed with structure i in the role of a; entry (j, i) is written with the same
 * bits, in both planes.  Entry (i, i) is exactly 0 with count = the structure's own number of points, or NaN when the
 * structure counts no point or one of its counted coordinates is not finite.  Only the tiles on and above the diagonal
 * are launched.
 *
 * ACCURACY.  This is the RMSD from the five sums, E0 - 2 tr, not from a pass over the residuals: the RMSD of IDENTICAL
 * members (and of rigid copies) is NOT 0.  With E = (Qx + Qy) / n the mean square is off by at most
 *       delta = (4 (n + 8) 2^-53 + 2^-45) E
 * -- sequential summation of the sums and their centroid corrections, and the loss of the solve -- so that
 * |rmsd - exact| <= 2^-23 exact + min(sqrt(delta), delta / exact): about sqrt(delta) ~ 1e-6 A for a protein-sized member
 * compared with itself, and delta / rmsd ~ 1e-12 A from 1 A on.  Taking the origin at a point of the structure keeps E at
 * the size of the structure wherever it lies.  K37 (ps_superpose_f32) remains the tool when an RMSD near 0 matters.
 *
 * PROPERTIES.  No atomics; repeatable bit for bit; the order of every sum depends on M only, never on Ba, Bb or the
 * position of a pair in the matrix: a sub-batch gives the corresponding block of the full matrix bit for bit, and self
 * mode gives cross mode on (a, a) bit for bit at i < j.
 *
 * Refused: Ba or Bb outside 0 .. 65535, M outside 1 .. PS_RMSD_MATRIX_MAX_POINTS, self mode with Bb != Ba or with a mask_b; with Ba > 0 and Bb > 0 also a
 * NULL a or rmsd.
 */
int ps_rmsd_matrix_f32(const float* a, const uint8_t* mask_a, const float* b, const uint8_t* mask_b, float* rmsd, int32_t* count,
                       int Ba, int Bb, int M, void* stream);

/*
 * K46.  Clustering of G distance matrices by a cutoff (Daura et al. 1999, the "gromos" method).  D is [G][B][B] float, valid
 * is [G][B] bytes or NULL (all items), cutoff is passed by value; B is 1 .. PS_CLUSTER_MAX_ITEMS, G is 0 .. 65535.
 * `workspace` holds ps_cluster_workspace_bytes(G, B) bytes, 4-byte aligned; it needs no clearing and its contents after the
 * call are unspecified.
 *
 * DEFINITION, per matrix.
 *   adj(i, j) = D[min(i, j)][max(i, j)] <= cutoff for i != j: only the upper triangle of D is read, the diagonal never.
 *   A NaN entry compares false; the cutoff is finite.
 *   All valid items start active.  Until no item is active:
 *       deg(i) = the number of active j != i with adj(i, j), for every active i
 *       the centre is the active i of greatest deg, the lowest index on ties
 *       cluster c = the centre and its active neighbours; they become inactive; c increases by one
 * Outputs: label[G][B] int32, the cluster of an item, -1 where invalid; center[G][B] and size[G][B] int32 indexed by
 * cluster number, -1 and 0 from n_clusters on; n_clusters[G] int32.  Sizes are non-increasing by construction.  Everything
 * is integer work on the comparisons, so the result is defined bit for bit.  Two launches, no host read.
 *
 * Refused: B outside 1 .. 4096, G outside 0 .. 65535, a cutoff that is not finite; with G > 0 also a NULL among D, workspace,
 * label, center, size, n_clusters.
 */
int ps_cluster_f32(const float* D, const uint8_t* valid, float cutoff, void* workspace, int32_t* label, int32_t* center,
                   int32_t* size, int32_t* n_clusters, int G, int B, void* stream);

/* Host function; launches nothing.  The size of K46's workspace in bytes, G * B * ceil(B / 32) * 4; -1 for G or B that the
 * clustering refuses. */
long long ps_cluster_workspace_bytes(int G, int B);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_ENSEMBLE_H */
