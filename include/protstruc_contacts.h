/*
 * protstruc_contacts.h -- C ABI of the closest-atom residue distances (K31 / K32) of libprotstruc_hip.so.
 *
 * These entry points are compiled into the same shared library as those of protstruc_hip.h and follow the same
 * conventions; they are declared in a header of their own, with a version number of their own, so that adding them
 * left PS_ABI_VERSION and every declaration of protstruc_hip.h as they were.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains memory;
 *   - coordinates are contiguous fp32 `xyz[B][N][A][3]`; masks are contiguous one-byte booleans (0 / 1; any non-zero
 *     input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched.
 */
#ifndef PROTSTRUC_CONTACTS_H
#define PROTSTRUC_CONTACTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_contacts_api() returns the library's.  Launches nothing. */
#define PS_CONTACTS_API 1
int ps_contacts_api(void);

#define PS_CLOSEST_MAX_ATOMS 64      /* a residue's presence word is one 64-bit mask */
#define PS_CLOSEST_MAX_RESIDUES 1048576

/*
 * K31.  Closest atoms of every residue pair.  For structure b and residues i <= j, over every present atom a of i and
 * present atom c of j (atom_mask[B][N][A]; NULL = every slot is present):
 *     X = (double)x    dx = Xjc.x - Xia.x, dy, dz likewise    d2 = (dx*dx + dy*dy) + dz*dz    in double, in this order
 * (no fused multiply-add).  Pairs whose d2 is not finite are skipped; the winner is the minimum under the order
 * (d2, a, c) ascending; with C2 = (double)cutoff * (double)cutoff it counts iff d2 <= C2.  Then
 *     dist[b][i][j] = (float)sqrt(d2)      pair[b][i][j] = a * A + c
 * and dist = +inf, pair = -1 where no atom pair counts.  Entry (j, i) is the mirror of (i, j): the same dist bits and
 * pair[b][j][i] = c * A + a, so pair[b][r][s] always reads "atom of the row residue, atom of the column residue".  The
 * diagonal is not special.  A masked slot's floats never influence an output.  dist and pair need only the alignment of
 * their element type.
 * Refused: NULL xyz / dist / pair, A outside 1 .. PS_CLOSEST_MAX_ATOMS, N outside 1 .. PS_CLOSEST_MAX_RESIDUES, B outside
 * 0 .. 65535, a cutoff that is negative or NaN (+inf is allowed).  B = 0 returns 0 without touching a device.
 */
int ps_closest_atoms_f32(const float* xyz, const uint8_t* atom_mask, float* dist, int16_t* pair, int B, int N, int A,
                         float cutoff, void* stream);

/*
 * K32.  Vector-Jacobian product of K31's dist towards xyz; the gradient flows to the recorded pair only:
 *     grad_xyz[b][i][a][:] = sum over j != i with pair[b][i][j] = a * A + c  of
 *                            ((double)g[b][i][j] + (double)g[b][j][i]) * (Xia - Xjc) / sqrt(d2)
 * summed over j ascending in double and rounded to float once, with d2 recomputed from the coordinates as above.  A
 * term whose pair lies outside [0, A*A) -- the -1 of "none" included -- or whose d2 is 0 or not finite contributes
 * nothing; slots that win no pair get exact zeros.  Reads xyz, pair[B][N][N] and grad_dist[B][N][N], nothing else; no
 * atomics, deterministic.  Limits as for K31.
 */
int ps_closest_atoms_backward_f32(const float* xyz, const int16_t* pair, const float* grad_dist, float* grad_xyz, int B,
                                  int N, int A, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_CONTACTS_H */
