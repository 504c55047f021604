/*
 * protstruc_aggregate.h -- C ABI of message passing on graphs (K55 - K59) of libprotstruc_aggregate.so: segment reductions of
 * per-edge rows at the sources or at the targets of an edge list, their adjoints (the gather of node rows onto the edges and
 * the per-edge dot product), and the softmax over every node's edges with its backward pass.  One family serves both
 * layouts: a padded (B, N, k) list is the CSR list row_ptr = arange(B * N + 1) * k, col = idx.reshape(-1).
 *
 * These entry points are compiled into a shared library of their own, beside libprotstruc_hip.so, libprotstruc_csredge.so
 * and libprotstruc_edgegrad.so, and declared in a header of their own with a version number of its own, so that adding them
 * left every declaration of the other headers and the other libraries' machine code as they were.
 *
 * Conventions (all entry points), those of protstruc_edgegrad.h:
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains memory;
 *   - tensors are contiguous and need only the alignment of their element;
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream): the launch goes to the caller's stream;
 *   - launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory, so they
 *     may be captured into a hipGraph;
 *   - the library holds no mutable state: every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before
 *     anything is launched, and B == 0 returns 0 without touching a device; so does E == 0 in K56 and K57, whose outputs
 *     have E rows;
 *   - B is 0 .. 65535, M and Q are 0 .. 2^24; offsets are 64-bit throughout; no kernel uses an atomic, every output
 *     element is written, and repeated runs agree bit for bit.
 *
 * THE EDGE LIST is that of protstruc_csredge.h: row_ptr [B * Q + 1] int64, the rows being the sources in (b, q) order; col [E]
 * int32 indexes the M axis of the edge's own structure; E is the LENGTH OF THE EDGE BUFFERS.  Position p is PADDING where
 * r(p) == B * Q -- the tail that max_edges leaves: p >= row_ptr[B * Q] -- or where col[p] is outside [0, M), the -1 inside the
 * rows of a padded kNN list included.  At the padding NOTHING IS READ -- no message, weight, logit or element of an
 * incoming gradient --, so a NaN there never reaches a result, and every per-edge output is exactly +0 there.
 *
 * A GROUPING is a set of S segments over edge positions, in one of two forms:
 *   - the SOURCE grouping: ptr = row_ptr and perm = NULL, S = B * Q; segment s holds the positions ptr[s] .. ptr[s + 1], both
 *     cut to [0, E];
 *   - the TARGET grouping: ptr = in_ptr [B * M + 1] and perm = in_edge [n_perm], the incoming list of protstruc_edgegrad.h
 *     (ops.csr_incoming_edges), S = B * M; segment s holds perm[t] for t in ptr[s] .. ptr[s + 1], both cut to [0, n_perm].
 * One kernel serves both: the members of a segment are perm ? perm[t] : t for t ASCENDING.  A member outside [0, E) is
 * skipped, and so is -- where col is given, and row_ptr with it -- a member at the padding.  A wrong list gives wrong values
 * but no access outside any buffer: every index a kernel uses as an address is range-checked first.
 *
 * PER-EDGE DATA are values [E][H][D] fp32 -- H heads of D floats; a plain (E, C) tensor is H = 1, D = C -- and an optional
 * weight [E][H] fp32.  Node data are [S][H][D].
 *
 * Lists are NOT SPLIT: a segment is summed by the lanes that own its row, from its first member to its last, so a launch
 * runs as long as its longest list.  The rows of a radius graph and the in-degrees of a kNN graph are tens to a few hundred
 * long, which is what this first version is for; a later split would sum fixed-size chunks and add the partial sums in chunk
 * order, so that the result still depends on the list alone.
 *
 * The library is built with -ffp-contract=off: every product and sum is rounded on its own, which is part of the
 * definitions below, so a numpy float64 restatement gives the same bits where bits are promised (K55, K56, K57, K59).
 *
 * More than 2^31 output floats cannot be tested in seconds: that the offsets are 64-bit -- size_t products whose factors
 * are widened before they are multiplied -- is established by reading, not by a test.
 */
#ifndef PROTSTRUC_AGGREGATE_H
#define PROTSTRUC_AGGREGATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header (bumped on any signature change); ps_aggregate_api() returns the library's.  Launches nothing. */
#define PS_AGGREGATE_API 1
int ps_aggregate_api(void);

#define PS_AGGREGATE_MAX_HEADS 64    /* H */
#define PS_AGGREGATE_MAX_ROW 4096    /* H * D, the floats of one row */

#define PS_AGGREGATE_SUM 0           /* the modes of K55 */
#define PS_AGGREGATE_MEAN 1
#define PS_AGGREGATE_MAX 2
#define PS_AGGREGATE_MIN 3

/*
 * K55.  Segment reduce: out [S][H][D] over the members e of every segment s of a grouping.
 *   SUM, MEAN: the accumulator is a double that starts at +0.0; the members are added in ascending order; each term is
 *     (double)weight[e][h] * (double)values[e][h][d], an exact product, or the value alone where weight is NULL; MEAN divides
 *     by the number of contributing members, in double; the result is rounded to fp32 once.  Defined bit for bit.
 *   MAX, MIN take no weight.  They start from the first contributing member and replace the best when v > best (v < best),
 *     so ties go to the lower position and a NaN never replaces anything; arg [S][H][D] int64, optional, receives the winning
 *     edge position.
 *   A segment without a contributing member gives +0, and -1 in arg.
 *
 * HOW.  A lane owns four consecutive floats of one segment's row: item i of L * S, L = ceil(H * D / 4), is quad i % L of
 * segment i / L, so consecutive lanes read consecutive 16 bytes of one member's row.  The lane walks its segment's members in
 * order, four members' loads issued before the first is used, with its accumulators in registers in double: no LDS, no
 * cross-lane traffic, no atomics.  The 16-byte arm (H * D % 4 == 0, values and out on a 16-byte boundary) and the dword arm
 * run the same lanes through the same sums and differ in the load and store instructions alone, so the bits agree.
 *
 * Refused: B outside 0 .. 65535; M or Q outside 0 .. 2^24; E or n_perm negative; H outside 1 .. PS_AGGREGATE_MAX_HEADS; D
 * below 1; H * D above PS_AGGREGATE_MAX_ROW; a mode that is none of the four; a weight with MAX or MIN; an arg with SUM or
 * MEAN; a NULL ptr or out; a NULL values with E > 0; a NULL perm with n_perm > 0; a col without row_ptr.
 */
int ps_segment_reduce_f32(const float* values, const float* weight, const long long* ptr, const long long* perm,
                          long long n_perm, const long long* row_ptr, const int32_t* col, long long E, int mode, float* out,
                          long long* arg, int B, int Q, int M, int H, int D, void* stream);

/*
 * K56.  Segment gather, the adjoint of SUM: out [E][H][D] from node [S][H][D] and index [E] int64, a flat node index.
 *     out[e][h][d] = fl32((double)weight[e][h] * (double)node[index[e]][h][d]),   or a copy where weight is NULL.
 * An index outside [0, S) gives +0 and reads nothing, the weight included: the caller marks the padding with -1.
 *
 * HOW.  Item i of L * E is quad i % L of edge i / L, as in K55; the two arms differ in the load and store alone.
 *
 * Refused: E or S negative; H outside 1 .. PS_AGGREGATE_MAX_HEADS; D below 1; H * D above PS_AGGREGATE_MAX_ROW; a NULL index
 * or out; a NULL node with S > 0.
 */
int ps_segment_gather_f32(const float* node, const float* weight, const long long* index, long long E, long long S, int H,
                          int D, float* out, void* stream);

/*
 * K57.  Edge dot, the gradient of the weight: out [E][H],
 *     out[e][h] = the sum over d of u_d = (double)node[index[e]][h][d] * (double)values[e][h][d],  exact products, summed
 *     IN DOUBLE, IN THIS ORDER: fours ascending, s_k = ((u_4k + u_4k+1) + u_4k+2) + u_4k+3 (the last one as far as D goes),
 *     then a tree over the K = ceil(D / 4) partial sums: for stride = 1, 2, 4, ..., s_k += s_(k+stride) for every k that is a
 *     multiple of 2 * stride with k + stride < K; the result is s_0, rounded to fp32 once.
 * The order depends on D alone, not on alignment or launch shape.  An index outside [0, S) gives +0 and reads nothing.
 *
 * HOW.  One lane per (e, h); the tree is kept as a binary counter of partial sums in registers.
 *
 * Refused: what K56 refuses, and a NULL values.
 */
int ps_edge_dot_f32(const float* node, const float* values, const long long* index, long long E, long long S, int H, int D,
                    float* out, void* stream);

/*
 * K58.  Segment softmax: logits [E][H] -> w [E][H] and, optionally, lse [S][H].  Per segment and head, over the members:
 *     m = the maximum (from the first member, replaced when x > m);
 *     s = the sum of exp((double)x_e - (double)m), in double, members ascending;
 *     w_e = fl32(exp((double)x_e - (double)m) / s);        lse = fl32((double)m + log(s)).
 * The exponential is evaluated in double, so the error of w is that of its one rounding and of exp's last bit.  A segment of
 * one member gives exactly 1.0; a member at -inf gives +0; a segment that is empty, or whose maximum is -inf, gives weights
 * +0 and lse = -inf; nothing is NaN unless a contributing logit is NaN or +inf.  w is +0 at every position that is in no
 * segment: the whole of w is zeroed by a first launch on the same stream.
 *
 * HOW.  One lane per (segment, head), the lanes of a segment consecutive in h; three walks over the members.
 *
 * Refused: B outside 0 .. 65535; M or Q outside 0 .. 2^24; E or n_perm negative; H outside 1 .. PS_AGGREGATE_MAX_HEADS; a
 * NULL ptr; a NULL logits or w with E > 0; a NULL perm with n_perm > 0; a col without row_ptr.
 */
int ps_segment_softmax_f32(const float* logits, const long long* ptr, const long long* perm, long long n_perm,
                           const long long* row_ptr, const int32_t* col, long long E, float* w, float* lse, int B, int Q,
                           int M, int H, void* stream);

/*
 * K59.  Softmax backward, given the saved w [E][H] and the incoming gradient grad_w [E][H]: per segment and head
 *     t = the sum of (double)w_e * (double)g_e, in double, members ascending;     gx_e = fl32((double)w_e * ((double)g_e - t)).
 * Defined bit for bit given w.  grad_logits [E][H] is +0 at the padding and at every position that is in no segment.
 *
 * Refused: what K58 refuses, with w, grad_w and grad_logits in the place of logits and w.
 */
int ps_segment_softmax_backward_f32(const float* w, const float* grad_w, const long long* ptr, const long long* perm,
                                    long long n_perm, const long long* row_ptr, const int32_t* col, long long E,
                                    float* grad_logits, int B, int Q, int M, int H, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PROTSTRUC_AGGREGATE_H */
