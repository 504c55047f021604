/*
 * protstruc_pairhead.h -- C ABI of the pair-head kernels (K33 - K36) of libprotstruc_hip.so: geometry to bin index, the
 * cross-entropy of (B,N,N,C) logits against such bins with its gradient, and expectations under the softmax of the logits
 * (the distogram and predicted-aligned-error heads of a structure network).
 *
 * These entry points are compiled into the same shared library as those of protstruc_hip.h and follow the same
 * conventions; they are declared in a header of their own, with a version number of their own, so that adding them
 * left PS_ABI_VERSION and every declaration of protstruc_hip.h as they were.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller, `breaks` excepted, which is a HOST array that is read during
 *     the call and travels in the kernel's arguments; the library never allocates, frees or retains memory;
 *   - tensors are contiguous; masks are one-byte booleans (0 / 1; any non-zero input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched, and B = 0 returns 0 without touching a device;
 *   - B is 0 .. 65535 and N is 1 .. PS_PAIRHEAD_MAX_RESIDUES everywhere; every element offset is 64-bit (B * N * N * C
 *     passes 2^31 at B = 128, N = 512, C = 64).
 */
#ifndef PROTSTRUC_PAIRHEAD_H
#define PROTSTRUC_PAIRHEAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_pairhead_api() returns the library's.  Launches nothing. */
#define PS_PAIRHEAD_API 1
int ps_pairhead_api(void);

#define PS_PAIRHEAD_MAX_RESIDUES 1048576
#define PS_PAIRHEAD_MAX_BREAKS 127    /* so that every bin index and the "no target" label fit a byte */
#define PS_PAIRHEAD_MAX_BINS 128      /* C, the last axis of the logits */
#define PS_PAIRHEAD_MAX_TABLES 4      /* V, the value tables one pass of K36 serves */
#define PS_PAIRHEAD_NO_TARGET 255     /* the bin of a pair that has no target */

/*
 * K33.  Geometry to bin index.  For structure b and the pair (i, j) a squared quantity v2 is formed in double on the
 * float32 inputs, every operation rounded on its own (no fused multiply-add), X = (double)x:
 *   mode 0, distance:       d = Xj - Xi of points[B][N][3];   v2 = (dx*dx + dy*dy) + dz*dz
 *   mode 1, aligned error:  d = Xj - Ti with points[B][N][3], trans[B][N][3] and rot[B][N][3][3] (basis vectors as
 *                           columns);  u_c = (R0c*d0 + R1c*d1) + R2c*d2 for c = 0, 1, 2, i.e. u = Ri^T (xj - ti);  u* the
 *                           same from target_points, target_rot, target_trans;  e = u - u*;  v2 = (ex*ex + ey*ey) + ez*ez
 * Then
 *     bins[b][i][j]  = #{k : v2 > (double)breaks[k] * (double)breaks[k]}          (AlphaFold's sum(d2 > sq_breaks))
 *     value[b][i][j] = (float)sqrt(v2)                                            (value may be NULL: not wanted)
 * and bins = PS_PAIRHEAD_NO_TARGET, value = +inf where row_mask[b][i] * col_mask[b][j] == 0 (masks [B][N]; NULL = all; in
 * mode 1 the row mask is the frame mask and the column mask the point mask) or v2 is not finite.  Floats at masked rows
 * and columns (NaN, anything) never reach an output.  In mode 0 rot, trans and the three target pointers are ignored.
 * Refused: a mode other than 0 / 1, n_breaks outside 1 .. PS_PAIRHEAD_MAX_BREAKS, breaks that are not finite, non-negative
 * and strictly increasing, NULL breaks / points / bins, in mode 1 a NULL among the other five tensors.
 */
int ps_pair_bins_f32(int mode, const float* points, const float* rot, const float* trans, const float* target_points,
                     const float* target_rot, const float* target_trans, const uint8_t* row_mask, const uint8_t* col_mask,
                     const float* breaks, int n_breaks, uint8_t* bins, float* value, int B, int N, void* stream);

/*
 * K34.  Cross-entropy of logits[B][N][N][C] (2 <= C <= PS_PAIRHEAD_MAX_BINS) against bins[B][N][N], summed per row:
 *     row_loss[b][i]  = sum over j with bins[b][i][j] < C of  lse(x_ij) - x_ij[bins[b][i][j]]
 *     row_count[b][i] = the number of such j                                                       (int32)
 * with lse(x) = m + log(sum_k exp(x_k - m)), m = max_k x_k.  A pair's arithmetic is fp32 (hardware exp2 and log2); the sum
 * over j is accumulated in double in a fixed order and rounded to float once: no atomics, repeated runs agree bit for
 * bit.  A pair whose bin is >= C contributes nothing and its logits (NaN, anything) never reach the sum; -inf logits are
 * legal (probability 0).  logits need only the alignment of a float; a 16-byte aligned base with C % 4 == 0 is read in
 * 16-byte accesses, anything else in 4-byte ones, with the same results.
 */
int ps_binned_cross_entropy_f32(const float* logits, const uint8_t* bins, float* row_loss, int32_t* row_count, int B, int N,
                                int C, void* stream);

/*
 * K35.  Vector-Jacobian product of K34 towards the logits, with the upstream grad_row[B][N]:
 *     grad_logits[b][i][j][k] = grad_row[b][i] * (exp(x_ijk - lse(x_ij)) - [k == bins[b][i][j]])
 * and exact zeros, all C of them, where bins[b][i][j] >= C (whatever the logits hold there).  Every element of
 * grad_logits[B][N][N][C] is written exactly once, so the buffer needs no clearing.  The 16-byte arm needs both logits and
 * grad_logits 16-byte aligned; otherwise 4-byte accesses, same results.
 */
int ps_binned_cross_entropy_backward_f32(const float* logits, const uint8_t* bins, const float* grad_row, float* grad_logits,
                                         int B, int N, int C, void* stream);

/*
 * K36.  Expectations under the softmax of the logits, for V tables values[B][V][C] (1 <= V <= PS_PAIRHEAD_MAX_TABLES):
 *     out[v][b][i][j] = sum_k softmax(x_ij)_k * values[b][v][k]
 * One pass over the logits serves all V tables; out is [V][B][N][N].  fp32 throughout.
 */
int ps_binned_expectation_f32(const float* logits, const float* values, float* out, int B, int N, int C, int V, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_PAIRHEAD_H */
