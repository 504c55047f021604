/*
 * protstruc_superpose.h -- C ABI of the superposition kernels (K37 - K40) of libprotstruc_hip.so: the weighted optimal
 * superposition of two point sets with its RMSD, the gradient of that RMSD, and a seeded search for the superposition
 * that maximises a TM-score or a count of points within a cutoff (GDT), up to eight such objectives in one launch.
 *
 * These entry points are compiled into the same shared library as those of protstruc_hip.h and follow the same
 * conventions; they are declared in a header of their own, with a version number of their own, so that adding them
 * left PS_ABI_VERSION and every declaration of protstruc_hip.h as they were.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller, `objectives` excepted, which is a HOST array that is read
 *     during the call and travels in the kernel's arguments; the library never allocates, frees or retains memory (the
 *     search writes its per-seed results into a `workspace` the caller supplies);
 *   - tensors are contiguous and need only the alignment of their element; masks are one-byte booleans (0 / 1; any
 *     non-zero input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched, and B = 0 returns 0 without touching a device;
 *   - B is 0 .. 65535; no kernel uses an atomic, and repeated runs agree bit for bit;
 *   - all geometry is double arithmetic on the float32 inputs, every product and sum rounded on its own (no fused
 *     multiply-add); every 3x3 solve is the one of ps_kabsch_f32 (one-sided Jacobi in double, a proper rotation for
 *     every covariance).
 */
#ifndef PROTSTRUC_SUPERPOSE_H
#define PROTSTRUC_SUPERPOSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_superpose_api() returns the library's.  Launches nothing. */
#define PS_SUPERPOSE_API 1
int ps_superpose_api(void);

#define PS_SUPERPOSE_MAX_POINTS 2048     /* M of the search: a structure's point pairs live in LDS, 24 bytes each */
#define PS_SUPERPOSE_MAX_OBJECTIVES 8
#define PS_SUPERPOSE_MAX_SEEDS 1024
#define PS_SUPERPOSE_MAX_ITERATIONS 20
#define PS_SUPERPOSE_MAX_DOUBLINGS 64
#define PS_SUPERPOSE_TM 0                /* kind: the TM-score term 1 / (1 + d^2 / d0^2), param = d0 */
#define PS_SUPERPOSE_COUNT 1             /* kind: the count [d^2 <= c^2], param = c */
#define PS_SUPERPOSE_ENTRY_FLOATS 16     /* one (S, R, t) of the workspace */

typedef struct ps_superpose_objective {
    int kind;
    float param;
} ps_superpose_objective;

/*
 * K37.  Weighted superposition with its RMSD.  a, b are [B][M][3] (b is [M][3], one target for all, with b_is_shared),
 * weight is [B][M], >= 0, or NULL for 1, mask is [B][M] bytes or NULL; M is any positive int.  Over the points i with
 * mask != 0 and w_i > 0, per structure:
 *     W = sum w_i,  ca = sum w_i a_i / W,  cb = sum w_i b_i / W,  H = sum w_i (a_i - ca)(b_i - cb)^T
 *     R = the rotation of the Kabsch fit to H,  t = cb - R ca
 *     msd = sum w_i |R a_i + t - b_i|^2 / W      -- a pass of its own over the residuals, not E0 - 2 sum sigma, so that
 *                                                   identical inputs give an RMSD at the rounding of the coordinates
 * Outputs R[B][3][3], t[B][3], rmsd[B] = (float)sqrt(msd), wsum[B] = (float)W.  W = 0 gives R, t, rmsd = NaN and wsum = 0.
 * Entries under the mask are never read, and coordinates at w = 0 are never read: NaN there reaches nothing.
 */
int ps_superpose_f32(const float* a, const float* b, const float* weight, const uint8_t* mask, float* R, float* t, float* rmsd,
                     float* wsum, int B, int M, int b_is_shared, void* stream);

/*
 * K38.  Vector-Jacobian product of K37's rmsd towards the points, with the upstream grad_rmsd[B] = g.  At the optimum the
 * derivative through R and t vanishes, so with e_i = R a_i + t - b_i
 *     grad_a[b][i] =  g w_i R^T e_i / (W rmsd),     grad_b[b][i] = -g w_i e_i / (W rmsd)
 * R, t and the weights get no gradient.  Every element of grad_a[B][M][3] and grad_b[B][M][3] is written once: exact zeros
 * under the mask, at w = 0, and for a structure whose rmsd is 0 or not finite or whose R holds a NaN.  R, t, rmsd and wsum are
 * K37's outputs for the same inputs; they decide which structures get zeros.  The residuals themselves are formed from a fit
 * that the kernel repeats in double: R rounded to float would move every e_i by 2^-25 |a_i|, far more than a rounding of
 * the result.  One lane per point, rounded to float once.  With b_is_shared the target is a constant: grad_b must be NULL
 * (a non-NULL one is refused); otherwise both gradients are required.
 */
int ps_superpose_backward_f32(const float* a, const float* b, const float* weight, const uint8_t* mask, const float* R,
                              const float* t, const float* rmsd, const float* wsum, const float* grad_rmsd, float* grad_a,
                              float* grad_b, int B, int M, int b_is_shared, void* stream);

/*
 * K39 / K40.  Seeded search for the best superposition of a[B][M][3] onto b[B][M][3] under n_obj objectives
 * (1 .. PS_SUPERPOSE_MAX_OBJECTIVES), M = 1 .. PS_SUPERPOSE_MAX_POINTS, l_norm[B] > 0.  Outputs score[B][n_obj],
 * R[B][n_obj][3][3], t[B][n_obj][3].  `workspace` holds ps_superpose_workspace_floats(B, M, n_obj) floats; it needs no
 * clearing and its contents after the call are unspecified.
 *
 * DEFINITION, per structure.
 *   Preparation.  The pairs with mask != 0 (NULL: all), in order, are the n points; they are held as float, all
 *     arithmetic is double on them.  Under a transform T = (R, t), for point i and c = 0, 1, 2:
 *         x_c = ((R_c0 a_0 + R_c1 a_1) + R_c2 a_2) + t_c,   e_c = x_c - b_c,   d_i^2 = (e_0 e_0 + e_1 e_1) + e_2 e_2
 *     The Kabsch fit of a set of points is K37's with unit weights: centroids, covariance about them, the 3x3 solve,
 *     t_c = cb_c - ((R_c0 ca_0 + R_c1 ca_1) + R_c2 ca_2).  Sums over points are taken in a fixed order that this
 *     definition leaves open (they agree with any other order to about 1e-13 of the score).
 *   Objectives.
 *     kind 0, TM:     s(d^2) = 1 / (1 + d^2 / (d0 d0)), d0 = param;  selection radii r1 = ds - 1 on the first selection of
 *                     a chain and r = ds + 1 after it, ds = min(8, max(4.5, d0))
 *     kind 1, count:  s(d^2) = [d^2 <= c c], c = param;  r1 = r = c
 *   Seeds.  Fragment lengths L_k = max(n >> k, 4) for k = 0, 1, ... until 4 is reached, a length equal to the one before
 *     it dropped; for n < 4 the only length is n.  With the stride h_k = max(L_k / 2, 1), the starts of length k are
 *     0, h_k, 2 h_k, ... below n - L_k, and then n - L_k itself: 1 + ceil((n - L_k) / h_k) seeds.  While the total exceeds
 *     PS_SUPERPOSE_MAX_SEEDS, the strides are doubled one at a time, from the shortest length to the longest and round
 *     again, the total being tested after every doubling.  Seeds are numbered by k ascending, then start ascending.
 *     n = 0 has no seed.
 *   One chain (seed s, objective o).
 *     1. T = the Kabsch fit of the fragment; the "previous selection" is the fragment.
 *     2. At most PS_SUPERPOSE_MAX_ITERATIONS times:
 *          S = sum_i s(d_i^2) under T; if S is strictly greater than the chain's best, keep (S, T);
 *          select {i : d_i^2 < r r} with r = r1 in the first iteration and r after it; while fewer than min(3, n)
 *          points are selected, r <- 2 r and select again, at most PS_SUPERPOSE_MAX_DOUBLINGS times, after which all
 *          points are selected (the doubled r is not carried to the next iteration);
 *          if the selected set equals the previous selection, stop;
 *          T = the Kabsch fit of the selected set.
 *   Result.  Per objective the chain with the greatest S, the lowest seed number on ties; score = (float)(S / l_norm),
 *     R and t rounded to float.  n = 0 gives score 0 and R, t NaN.
 *
 * This is not the search of the TM-score or LGA programs: the seed schedule is the one above, the radius is doubled where
 * those add 0.5, a count objective (GDT) is the maximum over the superpositions this search visits, and there is no sequence
 * alignment -- the correspondence is given.
 *
 * Refused: n_obj outside 1 .. 8, a kind other than 0 / 1, a param that is not finite and > 0, M outside 1 .. 2048, a NULL
 * among a, b, l_norm, objectives, workspace, score, R, t.
 */
int ps_superpose_search_f32(const float* a, const float* b, const uint8_t* mask, const float* l_norm,
                            const ps_superpose_objective* objectives, int n_obj, float* workspace, float* score, float* R,
                            float* t, int B, int M, void* stream);

/* Host functions; they launch nothing.  ps_superpose_seed_count(n): the number of seeds of n points (0 for n outside
 * 0 .. PS_SUPERPOSE_MAX_POINTS).  ps_superpose_seed(n, s, &start, &len): fragment s of n points; returns 0, or 1 when s is
 * not a seed of n.  ps_superpose_workspace_floats(B, M, n_obj): the size of the search's workspace in floats,
 * B * n_obj * PS_SUPERPOSE_ENTRY_FLOATS * max over n <= M of ps_superpose_seed_count(n); -1 for arguments the search refuses. */
int ps_superpose_seed_count(int n);
int ps_superpose_seed(int n, int s, int* start, int* len);
long long ps_superpose_workspace_floats(int B, int M, int n_obj);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_SUPERPOSE_H */
