/*
 * protstruc_csredge.h -- C ABI of the edge-feature kernels on CSR graphs (K49 - K51) of libprotstruc_csredge.so: what a
 * structure network computes between a radius graph (protstruc_graph.h) and its first linear layer -- the (batch, row) of
 * every edge, radial basis functions of the atom-pair distances along it, and the neighbour's frame in the source's frame.
 * They are K25 / K26 of protstruc_hip.h (edge features on padded (B, N, k) lists) on lists of any length.
 *
 * These entry points are compiled into a shared library of their own, beside libprotstruc_hip.so, and declared in a header
 * of their own with a version number of its own, so that adding them left PS_ABI_VERSION, every declaration of the other
 * headers and the other library's machine code as they were.
 *
 * Conventions (all entry points), those of protstruc_hip.h:
 *   - every pointer is a DEVICE pointer owned by the caller -- except pair_i, pair_j and centers, HOST arrays read before
 *     the call returns --; the library never allocates, frees or retains memory;
 *   - tensors are contiguous and need only the alignment of their element; masks are one-byte booleans (0 / 1; any
 *     non-zero input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched, and B == 0 or E == 0 returns 0 without touching a device;
 *   - B is 0 .. 65535, M and Q are 0 .. 2^24; offsets are 64-bit throughout; no kernel uses an atomic, and repeated runs
 *     agree bit for bit.
 *
 * THE GRAPH.  row_ptr is [n_rows + 1] int64 with n_rows = B * Q, the rows being the sources (queries) in (b, q) order; col
 * is [E] int32, indices into the M axis of the edge's own structure.  E is the LENGTH OF THE EDGE BUFFERS -- of col and of
 * every output --, not row_ptr[n_rows].  Edge position p in [0, E) belongs to row
 *     r(p) = the number of t in 1 .. n_rows with row_ptr[t] <= p
 * an upper bound over a non-decreasing array, found by bisection, so rows of length 0 are stepped over.  Position p is
 * PADDING where r(p) == n_rows (p >= row_ptr[n_rows]: the tail of a buffer longer than the list) or where col[p] is outside
 * [0, M) -- the -1 a radius graph with max_edges leaves there, or anything else.  Every output element of a padding edge is
 * written, as exact 0 (K49, which does not read col, writes -1 where r(p) == n_rows); col is not used as an address there
 * and no coordinate, frame or mask is read.  A list that was cut (row_ptr[n_rows] > E) is served for the positions that
 * exist.  A row_ptr that is not non-decreasing gives unspecified values but no access outside any buffer: the bisection
 * ends in [0, n_rows] whatever it reads, and col is range-checked.
 *
 * The library is built with -ffp-contract=off: every product and sum is rounded on its own, which is part of the
 * definitions below, so a numpy float64 restatement gives the same bits where bits are promised.
 *
 * More than 2^31 output floats cannot be tested in seconds: that the offsets are 64-bit -- size_t products whose factors
 * are widened before they are multiplied -- is established by reading, not by a test.
 */
#ifndef PROTSTRUC_CSREDGE_H
#define PROTSTRUC_CSREDGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_csredge_api() returns the library's.  Launches nothing. */
#define PS_CSREDGE_API 1
int ps_csredge_api(void);

#define PS_CSREDGE_CHUNK 64        /* consecutive edge positions a workgroup of K50 takes at a time, whatever their rows */
#define PS_CSREDGE_MAX_PAIRS 64    /* P: a chunk's PS_CSREDGE_CHUNK * P distances live in LDS (16 KB at the limit) */
#define PS_CSREDGE_MAX_RBF 64      /* R: the centres travel in the kernel's arguments */

/*
 * K49.  The (batch, row) of every edge position, with no host read: batch[p] = r(p) / Q and row[p] = r(p) % Q, both [E]
 * int32, both -1 where r(p) == n_rows.  One lane per position.
 *
 * Refused: Q outside 0 .. 2^24; n_rows negative, no multiple of Q (not 0 where Q is 0) or more than 65535 * Q; E negative;
 * a NULL row_ptr, batch or row.  E == 0 returns 0 and launches nothing.
 */
int ps_csr_edge_rows_i32(const long long* row_ptr, long long n_rows, int Q, long long E, int32_t* batch, int32_t* row,
                         void* stream);

/*
 * K50.  Radial basis functions of atom-pair distances along every edge.  The TARGETS (what col indexes) are xyz
 * [B][M][A][3] with atom_mask [B][M][A] or NULL (all); the SOURCES (the rows) are src_xyz [B][Q][As][3] with src_mask
 * [B][Q][As] or NULL.  src_xyz NULL means the sources are the targets: Q == M, As == A and src_mask NULL are required, and
 * the targets' mask is used for both.  For the edge at position p with row r(p) = b * Q + q and j = col[p], and the atom
 * pair t = (slot pair_i[t] of source q, slot pair_j[t] of target j), t < P:
 *     X = (double)x      dx = Xj.x - Xq.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz     in double, in this order
 *     dist[p][t] = d = (float)sqrt(d2)                           -- K24's, K25's and K48's distance: defined bit for bit
 *     rbf[p][t*R + c] = exp(-z*z),  z = (d - centers[c]) / sigma -- in fp32, within 1e-6 absolute of the float64 value
 * z is evaluated as K25 evaluates it: w = (d - centers[c]) * s with s = fl32(sqrt(log2 e) / sigma), computed in double and
 * rounded once on the host, and rbf = exp2(-(w*w)) by the hardware's v_exp_f32; the error analysis is K25's
 * (protstruc_hip.h).  On the same edge with the same inputs dist and rbf are the bits K25 writes.  Both are exactly 0 at
 * the padding and for a pair with an atom outside its mask; an unmasked NaN propagates.  dist is [E][P], rbf [E][P*R];
 * either may be NULL, not both.
 *
 * HOW.  A streaming-store kernel whose work is cut by edge position, not by source: chunk c is the PS_CSREDGE_CHUNK
 * positions from c * PS_CSREDGE_CHUNK on (the last one may be short), and a workgroup takes chunks blockIdx.x,
 * + gridDim.x, ...  Per chunk: (1) every position's row, one bisection per lane, and its range-checked col go to LDS;
 * (2) the chunk's 64 * P distances are computed once, in double, into LDS and written to dist from there; (3) all lanes
 * stream the chunk's 64 * P * R floats out, 16 bytes per lane per round, consecutive lanes on consecutive 16 bytes, with
 * no division inside the loop.  The output base is only 4-byte aligned and a chunk's length need not be a multiple of 4
 * floats: the up to three floats before the first 16-byte boundary of the chunk's ACTUAL address and the up to three after
 * its last whole 16 bytes are single stores; nothing outside [0, E * P * R) is touched and every float is written once.
 *
 * Refused: B outside 0 .. 65535; M or Q outside 0 .. 2^24; E negative; A or As below 1; P outside 1 ..
 * PS_CSREDGE_MAX_PAIRS; R outside 1 .. PS_CSREDGE_MAX_RBF; a pair_i outside [0, As) or a pair_j outside [0, A); a sigma that
 * is not positive and finite (or so small that s overflows); dist and rbf both NULL; src_xyz NULL with Q != M, As != A or a
 * src_mask; a NULL xyz, row_ptr, col, pair_i, pair_j or centers.
 */
int ps_csr_edge_rbf_f32(const float* xyz, const uint8_t* atom_mask, const float* src_xyz, const uint8_t* src_mask,
                        const long long* row_ptr, const int32_t* col, long long E, const int32_t* pair_i,
                        const int32_t* pair_j, int P, const float* centers, int R, float sigma, float* dist, float* rbf,
                        int B, int M, int A, int Q, int As, void* stream);

/*
 * K51.  The neighbour's frame in the source's frame along every edge.  The targets' frames are rot [B][M][3][3] (basis
 * vectors as columns), trans [B][M][3] and frame_mask [B][M] or NULL; the sources' src_rot [B][Q][3][3], src_trans [B][Q][3]
 * and src_mask [B][Q] or NULL.  src_rot and src_trans NULL together (with src_mask NULL and Q == M) mean the targets.  With
 * i the source and j = col[p] the target of the edge, K26's formulas, in double on the fp32 inputs in exactly this order,
 * each value rounded to fp32 once:
 *     v = t_j - t_i
 *     local_pos[p][c]  = (R_i[0][c]*v0 + R_i[1][c]*v1) + R_i[2][c]*v2                       = (R_i^T v)[c]
 *     rel_rot[p][a][c] = (R_i[0][a]*R_j[0][c] + R_i[1][a]*R_j[1][c]) + R_i[2][a]*R_j[2][c]  = (R_i^T R_j)[a][c]
 * bit for bit what K26 writes on the same edge.  Exactly 0 at the padding and where i or j is outside its mask.  local_pos
 * is [E][3], rel_rot [E][9]; either may be NULL, not both.  One lane per edge, r(p) found as in K49.
 *
 * Refused: B outside 0 .. 65535; M or Q outside 0 .. 2^24; E negative; local_pos and rel_rot both NULL; only one of
 * src_rot and src_trans; both NULL with Q != M or a src_mask; a NULL rot, trans, row_ptr or col.
 */
int ps_csr_edge_frames_f32(const float* rot, const float* trans, const uint8_t* frame_mask, const float* src_rot,
                           const float* src_trans, const uint8_t* src_mask, const long long* row_ptr, const int32_t* col,
                           long long E, float* local_pos, float* rel_rot, int B, int M, int Q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_CSREDGE_H */
