/*
 * protstruc_edgegrad.h -- C ABI of the backward kernels of the edge features (K52 - K54) of libprotstruc_edgegrad.so: the
 * vector-Jacobian products of K25 / K50 (radial basis functions and distances along the edges of a graph) and of K26 / K51
 * (the neighbour's frame in the source's frame), with respect to the coordinates and to the frames.  One family serves both
 * layouts: a padded (B, N, k) list is the CSR list row_ptr = arange(B * N + 1) * k, col = idx.reshape(-1).
 *
 * These entry points are compiled into a shared library of their own, beside libprotstruc_hip.so and
 * libprotstruc_csredge.so, and declared in a header of their own with a version number of its own, so that adding them left
 * every declaration of the other headers and the other libraries' machine code as they were.
 *
 * Conventions (all entry points), those of protstruc_csredge.h:
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
 *     anything is launched, and B == 0 returns 0 without touching a device; so does E == 0 in K52, whose output has E
 *     rows, while K53 and K54 then still write their zeros;
 *   - B is 0 .. 65535, M and Q are 0 .. 2^24; offsets are 64-bit throughout; no kernel uses an atomic, every output
 *     element is written, and repeated runs agree bit for bit.
 *
 * THE GRAPH is that of protstruc_csredge.h: row_ptr [n_rows + 1] int64 with n_rows = B * Q, the rows being the sources in
 * (b, q) order; col [E] int32 indexes the M axis of the edge's own structure; E is the LENGTH OF THE EDGE BUFFERS.  Edge
 * position p belongs to row r(p) = the number of t in 1 .. n_rows with row_ptr[t] <= p, found by bisection.  Position p is
 * PADDING where r(p) == n_rows or col[p] is outside [0, M): the gradient there is exactly 0, col is not used as an address,
 * and neither a coordinate, a frame, a mask nor an ELEMENT OF THE INCOMING GRADIENT is read there -- a NaN in it does not
 * reach the result.  A list that was cut (row_ptr[n_rows] > E) is served for the positions that exist.  A row_ptr that is
 * not non-decreasing gives unspecified values but no access outside any buffer.
 *
 * THE INCOMING LIST is the transpose's index: in_ptr [B * M + 1] int64 and in_edge [E_in] int64, where
 * in_edge[in_ptr[o] .. in_ptr[o + 1]) are the edge positions p with (r(p) / Q) * M + col[p] == o, ascending.  It is what lets
 * a target sum over its edges in a fixed order without atomics.  Bounds of in_ptr are cut to [0, E_in], an in_edge outside
 * [0, E) is skipped, and K54 also skips an entry that is no edge of its owner, so a wrong list gives wrong values but no
 * access outside any buffer.
 *
 * The library is built with -ffp-contract=off: every product and sum is rounded on its own, which is part of the
 * definitions below, so a numpy float64 restatement gives the same bits where bits are promised (K53, K54).
 *
 * More than 2^31 output floats cannot be tested in seconds: that the offsets are 64-bit -- size_t products whose factors
 * are widened before they are multiplied -- is established by reading, not by a test.
 */
#ifndef PROTSTRUC_EDGEGRAD_H
#define PROTSTRUC_EDGEGRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_edgegrad_api() returns the library's.  Launches nothing. */
#define PS_EDGEGRAD_API 1
int ps_edgegrad_api(void);

#define PS_EDGEGRAD_CHUNK 64        /* consecutive edge positions a workgroup of K52 takes at a time: PS_CSREDGE_CHUNK */
#define PS_EDGEGRAD_MAX_PAIRS 64    /* P: a chunk's PS_EDGEGRAD_CHUNK * P distances live in LDS (16 KB at the limit) */
#define PS_EDGEGRAD_MAX_RBF 64      /* R: the centres travel in the kernel's arguments */

/*
 * K52.  The gradient of K50 (and of K25) per edge and atom pair.  The arguments are K50's (protstruc_csredge.h), with the
 * incoming gradients g_dist [E][P] and g_rbf [E][P*R] in place of the outputs; either may be NULL (no such term), not both.
 * For the edge at position p and the pair t, d is the forward's distance -- sqrt((dx*dx + dy*dy) + dz*dz) in double on
 * X = (double)x, rounded to fp32 once -- and the Gaussian is recomputed as K25 / K50 compute it, in fp32:
 *     w_c = (d - centers[c]) * s      e_c = exp2(-(w_c*w_c))      s = fl32(sqrt(log2 e) / sigma), rounded once on the host
 *     u_c = (double)g_rbf[p][t*R + c] * (double)(e_c * w_c)      -- e_c * w_c rounded to fp32, the product by g exact
 *     S   = the sum of u_c over c, IN DOUBLE, IN THIS ORDER: fours ascending, s_k = ((u_4k + u_4k+1) + u_4k+2) + u_4k+3
 *           (the last one as far as R goes), then a tree over the K = ceil(R / 4) partial sums: for stride = 1, 2, 4, 8,
 *           s_k += s_(k+stride) for every k that is a multiple of 2 * stride with k + stride < K; S = s_0
 *     gd  = kappa * S                kappa = -2 / (sigma * sqrt(log2 e)), computed in double on the host
 *     c   = (g_dist[p][t] + gd) / d  in double, d widened        (a NULL g_dist or g_rbf leaves its term out)
 *     pair_grad[p][t][x] = f = (float)(c * (Xj.x - Xq.x)), y and z likewise: each component rounded to fp32 once
 * f is the gradient with respect to the TARGET's atom of the pair (slot pair_j[t] of col[p]); the source's atom (slot
 * pair_i[t] of the row) gets -f: K53.  f is exactly +0 at the padding, where either atom is outside its mask, and where
 * d == 0 (the self edge of a graph that includes it: the distance has no derivative there, and the gradient is DEFINED as 0,
 * not NaN); nothing is read at such a pair, the incoming gradients included.  pair_grad is [E][P][3] fp32.
 *
 * Error.  Against the same formula in exact arithmetic a term u_c carries K25's 1e-6 absolute on e_c and three fp32
 * roundings (two in w_c, one in e_c * w_c), 3 * 2^-24 < 2^-21 relative; the sum is in double and adds nothing to that:
 *     |gd - exact| <= |kappa| * sum_c |g_c| |w_c| (1e-6 + 2^-21 e_c),   and f adds 2^-23 relative for its one rounding.
 *
 * The order of S does not depend on how g_rbf is aligned: the 16-byte arm (R % 4 == 0 and g_rbf on a 16-byte boundary) and
 * the dword arm run the same lanes through the same sums and differ in the load instruction alone, so the bits agree.
 *
 * HOW.  Work is cut into chunks of PS_EDGEGRAD_CHUNK consecutive edge positions, as in K50, and a workgroup of four waves
 * takes G = min(4, max(1, 64 / P)) consecutive chunks at a time -- as many as keep their distances inside the LDS one chunk
 * has at P = 64 and their positions at one per lane --, spans blockIdx.x, + gridDim.x, ...  Per span: (1) every position's
 * row, one bisection per lane, and its range-checked col go to LDS; (2) the span's 64 * G * P distances are computed once,
 * in double, into LDS, a negative value marking a pair that gets 0; (3) K consecutive lanes take a pair, lane k its floats 4k .. 4k + 3 as one 16-byte load, so consecutive lanes
 * read consecutive 16 bytes; a wave takes 64 / K pairs a round, four rounds' loads are issued before the first is used,
 * the K partial sums meet across lanes (DPP where K is a power of two, else shuffles), and lane 0 of the pair forms f and
 * writes it.  A lane's walk over (position, pair) takes no division inside the loop.
 *
 * Refused: what K50 refuses (B outside 0 .. 65535; M or Q outside 0 .. 2^24; E negative; A or As below 1; P outside 1 ..
 * PS_EDGEGRAD_MAX_PAIRS; R outside 1 .. PS_EDGEGRAD_MAX_RBF; a pair_i outside [0, As) or a pair_j outside [0, A); a sigma
 * that is not positive and finite, or so small that s overflows; src_xyz NULL with Q != M, As != A or a src_mask; a NULL xyz,
 * row_ptr, col, pair_i, pair_j or centers); g_dist and g_rbf both NULL; a NULL pair_grad.
 */
int ps_csr_edge_rbf_backward_f32(const float* xyz, const uint8_t* atom_mask, const float* src_xyz, const uint8_t* src_mask,
                                 const long long* row_ptr, const int32_t* col, long long E, const int32_t* pair_i,
                                 const int32_t* pair_j, int P, const float* centers, int R, float sigma, const float* g_dist,
                                 const float* g_rbf, float* pair_grad, int B, int M, int A, int Q, int As, void* stream);

/*
 * K53.  The segmented sum of pair_grad [E][P][3] into grad [B][M][A][3] and, in BIPARTITE mode (grad_src not NULL), grad_src
 * [B][Q][As][3]; with grad_src NULL the sources are the targets (Q == M and As == A are required) and grad takes both sums.
 * For the owner o = (b, m) and each of its slots, an accumulator in double that starts from +0.0, in exactly this order:
 *   1. for p ascending over the owner's OUTGOING positions row_ptr[o] .. row_ptr[o + 1] (both cut to [0, E]), for t
 *      ascending: f[p][t] is SUBTRACTED from slot pair_i[t];
 *   2. then for e ascending over the owner's INCOMING list in_ptr[o] .. in_ptr[o + 1], for t ascending: f[in_edge[e]][t] is
 *      ADDED to slot pair_j[t].
 * Each accumulator is rounded to fp32 once.  In bipartite mode grad_src takes the first loop (owners (b, q), slots of As)
 * and grad the second.  A slot that no pair names and an owner without edges come out as exact +0 -- and so does an atom
 * outside its mask, because K52 wrote +0 for every pair that names it; K53 itself reads no mask and no col.
 *
 * HOW.  One lane owns one slot of one owner and keeps its three accumulators in registers; it walks the owner's positions
 * and, per position, the pairs that name its slot -- one 64-bit mask per table, made once, walked from its lowest bit --,
 * so a slot that no pair names walks nothing.  The lanes of an owner read the same rows of pair_grad at the same time.
 *
 * Refused: B outside 0 .. 65535; M or Q outside 0 .. 2^24; E or E_in negative; A or As below 1; P outside 1 ..
 * PS_EDGEGRAD_MAX_PAIRS; a pair_i outside [0, As) or a pair_j outside [0, A); grad_src NULL with Q != M or As != A; a NULL
 * row_ptr, in_ptr, pair_i, pair_j or grad; a NULL pair_grad with E > 0; a NULL in_edge with E_in > 0.
 */
int ps_csr_edge_pair_grad_sum_f32(const float* pair_grad, const long long* row_ptr, long long E, const long long* in_ptr,
                                  const long long* in_edge, long long E_in, const int32_t* pair_i, const int32_t* pair_j,
                                  int P, float* grad, float* grad_src, int B, int M, int A, int Q, int As, void* stream);

/*
 * K54.  The gradient of K51 (and of K26) with respect to the frames.  The arguments are K51's, the incoming list, and the
 * incoming gradients g_pos [E][3] and g_rot [E][9] in place of the outputs; either may be NULL, not both.  With i the source
 * and j = col[p] the target of the edge at p, v = t_j - t_i, everything in double on the fp32 inputs, R treated as nine free
 * numbers (what the backward of the frames takes), rot[.][3*r + c] = R[r][c]:
 *     the source gets   dR_i[r][c] += T,  T = v_r * g_pos[c] + ((R_j[r][0]*g_rot[c][0] + R_j[r][1]*g_rot[c][1]) + R_j[r][2]*g_rot[c][2])
 *                                         (with one of g_pos and g_rot NULL, T is the other summand alone)
 *                       dt_i[r]    -= (R_i[r][0]*g_pos[0] + R_i[r][1]*g_pos[1]) + R_i[r][2]*g_pos[2]
 *     the target gets   dR_j[r][c] += (R_i[r][0]*g_rot[0][c] + R_i[r][1]*g_rot[1][c]) + R_i[r][2]*g_rot[2][c]
 *                       dt_j[r]    += (R_i[r][0]*g_pos[0] + R_i[r][1]*g_pos[1]) + R_i[r][2]*g_pos[2]
 * An owner's twelve accumulators start from +0.0, take the terms of its outgoing positions, p ascending, then those of its
 * incoming list, e ascending, and are rounded to fp32 once: defined bit for bit.  The gradient is exactly +0 at the padding
 * and where either frame is outside its mask, and nothing is read there.  Outputs: grad_rot [B][M][9], grad_trans [B][M][3],
 * and in bipartite mode (src_rot and src_trans given) grad_src_rot [B][Q][9], grad_src_trans [B][Q][3], which take the
 * outgoing terms while grad_rot / grad_trans take the incoming ones.
 *
 * HOW.  ONE kernel that walks both lists and recomputes the terms -- no table of per-edge terms is written --, one lane per
 * owner with the accumulators in registers; the source of an incoming edge is found by the bisection r(p).
 *
 * Refused: B outside 0 .. 65535; M or Q outside 0 .. 2^24; E or E_in negative; g_pos and g_rot both NULL; only one of
 * src_rot and src_trans; both NULL with Q != M, a src_mask or a grad_src_rot / grad_src_trans; both given without
 * grad_src_rot and grad_src_trans; a NULL rot, trans, row_ptr, in_ptr, grad_rot or grad_trans; a NULL col with E > 0; a NULL
 * in_edge with E_in > 0.
 */
int ps_csr_edge_frames_backward_f32(const float* rot, const float* trans, const uint8_t* frame_mask, const float* src_rot,
                                    const float* src_trans, const uint8_t* src_mask, const long long* row_ptr,
                                    const int32_t* col, long long E, const long long* in_ptr, const long long* in_edge,
                                    long long E_in, const float* g_pos, const float* g_rot, float* grad_rot, float* grad_trans,
                                    float* grad_src_rot, float* grad_src_trans, int B, int M, int Q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_EDGEGRAD_H */
