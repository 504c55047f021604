"""The yardstick of the backward kernels of the edge features (ps_csr_edge_rbf_backward_f32, ps_csr_edge_pair_grad_sum_f32,
ps_csr_edge_frames_backward_f32; include/protstruc_edgegrad.h) and of ``ops.csr_incoming_edges``: their definitions in numpy
float64 on the same float32 inputs the kernels get.

    incoming      the positions p that are edges, grouped by (r(p) // Q) * M + col[p], ascending in a group; the others
                  after them, ascending
    K52           d the forward's fp32 distance; w_c = (d - centers[c]) * s with the fp32 s of the host; e_c = 2^-(w_c^2);
                  gd = kappa * sum_c g_c e_c w_c; f = (g_dist + gd) * (Xj - Xq) / d -- all in float64 and NOT rounded: the
                  kernel owes it to within the bound that comes back beside it,
                      |kappa| * sum_c |g_c| |w_c| (1e-6 + 2^-21 e_c)   per (edge, pair), times |Xj - Xq| / d,
                      plus 2^-23 |f| for the rounding of f
                  (1e-6: K25's contract for a recomputed Gaussian; 2^-21: the few fp32 roundings of a term)
    K53           float64 accumulators from +0, outgoing positions ascending (subtract at pair_i), then the incoming list
                  ascending (add at pair_j), rounded to fp32 once: the kernel owes the bits
    K54           the twelve accumulators per owner in the header's order, rounded once: the kernel owes the bits

Everything is exactly 0 at the padding, outside a mask and on an edge of length 0; values there -- coordinates and incoming
gradients alike -- are replaced before any arithmetic, so NaN there cannot reach a result.
"""
from typing import NamedTuple

import numpy as np

from tests import csr_edge_ref as C

LOG2E = 1.4426950408889634


def incoming(row_ptr, col, B, Q, M):
    """(ptr (B*M+1,) int64, edge (E,) int64): counted out position by position"""
    col = np.asarray(col).astype(np.int64)
    E = col.shape[0]
    r = C.rows(row_ptr, E)
    groups = [[] for _ in range(B * M + 1)]
    for p in range(E):
        real = r[p] < B * Q and 0 <= col[p] < M
        groups[(r[p] // Q) * M + col[p] if real else B * M].append(p)
    ptr = np.zeros(B * M + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(g) for g in groups[:-1]])
    return ptr, np.asarray([p for g in groups for p in g], dtype=np.int64)


class PairGrad(NamedTuple):
    f: np.ndarray        # (E,P,3) float64: the gradient with respect to the target's atom, unrounded
    bound: np.ndarray    # (E,P,3) float64: what the kernel may be off by
    real: np.ndarray     # (E,P) bool: an edge, both atoms in their masks, d != 0


def rbf_backward(xyz, row_ptr, col, atom_mask, pair_i, pair_j, centers, sigma, src_xyz=None, src_mask=None, g_dist=None,
                 g_rbf=None, exact=False) -> PairGrad:
    """``exact``: the formula alone -- d and s are not rounded to fp32 on the way --, which is what float64 autograd of the
    composed route differentiates; otherwise d and s are the fp32 values the kernels use.  The bound of the exact form adds
    what those two roundings are worth, to first order and doubled: with u(w) = w 2^-(w^2), |u'| <= e (1 + 2 ln2 w^2), and d
    and s each off by 2^-24 relative, w moves by at most 2^-24 (s d + |w|); the division by the rounded d adds 2^-24 |f|."""
    x, centers = np.asarray(xyz), np.asarray(centers)
    assert x.dtype == np.float32 and centers.dtype == np.float32
    fwd = C.edge_rbf(x, row_ptr, col, atom_mask, pair_i, pair_j, centers, sigma, src_xyz, src_mask)
    B, M, A = x.shape[:3]
    s_xyz = x if src_xyz is None else np.asarray(src_xyz)
    ok = np.ones((B, M, A), dtype=bool) if atom_mask is None else np.asarray(atom_mask) != 0
    oks = ok if src_xyz is None else (np.ones(s_xyz.shape[:3], dtype=bool) if src_mask is None else np.asarray(src_mask) != 0)
    Q = s_xyz.shape[1]
    pi, pj = np.asarray(pair_i, dtype=np.int64), np.asarray(pair_j, dtype=np.int64)
    E, P, R = len(col), len(pi), len(centers)
    zero = np.zeros((E, P, 3))
    if not (B and M and Q and E):
        return PairGrad(zero, zero.copy(), np.zeros((E, P), bool))
    b, q, j, _ = C._edges(row_ptr, col, Q, M)
    real = fwd.real & (fwd.dist != 0)
    Xi = C._clean(s_xyz, oks, 1)[b, q][:, pi]
    Xj = C._clean(x, ok, 1)[b, j][:, pj]
    d = np.where(real, fwd.dist, np.float32(1)).astype(np.float64)               # (E,P)
    sig = np.float64(np.float32(sigma))
    s = np.float64(np.float32(np.sqrt(LOG2E) / sig))
    if exact:
        with np.errstate(invalid="ignore", over="ignore"):
            delta = Xj - Xi
            d = np.where(real, np.sqrt((delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) + delta[..., 2] * delta[..., 2]), 1.0)
        sig = np.float64(sigma)
        s = np.sqrt(LOG2E) / sig
    kappa = -2.0 / (sig * np.sqrt(LOG2E))
    gd = np.zeros((E, P))
    bound_gd = np.zeros((E, P))
    with np.errstate(invalid="ignore", over="ignore"):
        if g_rbf is not None:
            g = np.where(real[..., None], np.asarray(g_rbf, dtype=np.float32).reshape(E, P, R), np.float32(0)).astype(np.float64)
            w = (d[..., None] - centers.astype(np.float64)) * s
            e = np.exp2(-(w * w))
            gd = kappa * (g * e * w).sum(-1)
            bound_gd = abs(kappa) * (np.abs(g) * np.abs(w) * (1e-6 + 2.0 ** -21 * e)).sum(-1)
            if exact:
                moved = 2.0 ** -24 * (s * d[..., None] + np.abs(w))
                bound_gd = bound_gd + 2.0 * abs(kappa) * (np.abs(g) * e * (1.0 + 2.0 * np.log(2.0) * w * w) * moved).sum(-1)
        total = gd
        if g_dist is not None:
            total = np.where(real, np.asarray(g_dist, dtype=np.float32).reshape(E, P), np.float32(0)).astype(np.float64) + gd
        unit = (Xj - Xi) / d[..., None]
        f = np.where(real[..., None], total[..., None] * unit, 0.0)
        bound = np.where(real[..., None], bound_gd[..., None] * np.abs(unit) + (2.0 ** -22 if exact else 2.0 ** -23) * np.abs(f), 0.0)
    return PairGrad(f, bound, real)


class Summed(NamedTuple):
    grad: np.ndarray        # (B,M,A,3) float64: the accumulators, unrounded
    grad_src: np.ndarray    # (B,Q,As,3) float64, or None in the self graph
    bound: np.ndarray       # as grad: sum bound + 2^-39 sum |term| + 2^-23 |ref| + 2^-149
    bound_src: np.ndarray


def pair_grad_sum(f, row_ptr, in_ptr, in_edge, pair_i, pair_j, B, M, A, Q=None, As=None, bound=None) -> Summed:
    """K53's loops, term by term in the header's order.  ``f`` float32: ``grad.astype(float32)`` are the kernel's bits.
    ``f`` float64 with its ``bound``: the propagated bound comes back too (a double accumulator of fp32 terms is far inside
    the 2^-39 the middle term allows)."""
    f = np.asarray(f)
    E, P = f.shape[:2]
    bipartite = Q is not None
    Qs, Ass = (Q, As) if bipartite else (M, A)
    f64 = f.astype(np.float64)
    bd = np.zeros_like(f64) if bound is None else np.asarray(bound, dtype=np.float64)
    grad, mag, acc_b = np.zeros((B * M, A, 3)), np.zeros((B * M, A, 3)), np.zeros((B * M, A, 3))
    src = (np.zeros((B * Qs, Ass, 3)), np.zeros((B * Qs, Ass, 3)), np.zeros((B * Qs, Ass, 3))) if bipartite else (grad, mag, acc_b)
    for o in range(B * Qs):   # the outgoing loop: subtracted at pair_i
        for p in range(min(max(int(row_ptr[o]), 0), E), min(max(int(row_ptr[o + 1]), 0), E)):
            for t in range(P):
                src[0][o, pair_i[t]] = src[0][o, pair_i[t]] - f64[p, t]
                src[1][o, pair_i[t]] += np.abs(f64[p, t])
                src[2][o, pair_i[t]] += bd[p, t]
    for o in range(B * M):    # then the incoming loop: added at pair_j
        for e in range(min(max(int(in_ptr[o]), 0), len(in_edge)), min(max(int(in_ptr[o + 1]), 0), len(in_edge))):
            p = int(in_edge[e])
            if not 0 <= p < E:
                continue
            for t in range(P):
                grad[o, pair_j[t]] = grad[o, pair_j[t]] + f64[p, t]
                mag[o, pair_j[t]] += np.abs(f64[p, t])
                acc_b[o, pair_j[t]] += bd[p, t]

    def out(acc, shape):
        value = acc[0].reshape(shape)
        return value, (acc[2] + 2.0 ** -39 * acc[1]).reshape(shape) + 2.0 ** -23 * np.abs(value) + 2.0 ** -149
    g, gb = out((grad, mag, acc_b), (B, M, A, 3))
    if not bipartite:
        return Summed(g, None, gb, None)
    s, sb = out(src, (B, Qs, Ass, 3))
    return Summed(g, s, gb, sb)


def pair_grad_sum_any_order(f, bound, row_ptr, col, pair_i, pair_j, B, M, A, Q=None, As=None) -> Summed:
    """``pair_grad_sum`` for float64 ``f`` with its ``bound`` on graphs too large to walk term by term: numpy's scatter-add,
    whose order is not the kernel's -- in float64 that is far inside the bound that comes back"""
    f, bound = np.asarray(f, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    E, P = f.shape[:2]
    bipartite = Q is not None
    Qs, Ass = (Q, As) if bipartite else (M, A)
    b, q, j, real = C._edges(row_ptr, col, Qs, M)
    pi, pj = np.asarray(pair_i, dtype=np.int64), np.asarray(pair_j, dtype=np.int64)
    tgt = [np.zeros((B * M, A, 3)) for _ in range(3)]
    src = [np.zeros((B * Qs, Ass, 3)) for _ in range(3)] if bipartite else tgt
    rows_out, rows_in = (b * Qs + q)[real], (b * M + j)[real]
    for acc_s, acc_t, values, sign in ((src[0], tgt[0], f, -1.0), (src[1], tgt[1], np.abs(f), 1.0), (src[2], tgt[2], bound, 1.0)):
        for t in range(P):
            np.add.at(acc_s, (rows_out, pi[t]), sign * values[real, t])
            np.add.at(acc_t, (rows_in, pj[t]), values[real, t])
    assert not f[~real].any(), "pair_grad is 0 at every position that is no edge"

    def out(acc, shape):
        value = acc[0].reshape(shape)
        return value, (acc[2] + 2.0 ** -39 * acc[1]).reshape(shape) + 2.0 ** -23 * np.abs(value) + 2.0 ** -149
    g, gb = out(tgt, (B, M, A, 3))
    if not bipartite:
        return Summed(g, None, gb, None)
    sv, sb = out(src, (B, Qs, Ass, 3))
    return Summed(g, sv, gb, sb)


class FrameGrads(NamedTuple):
    rot: np.ndarray          # (B,M,3,3) float64 accumulators: .astype(float32) are the kernel's bits
    trans: np.ndarray        # (B,M,3)
    src_rot: np.ndarray      # (B,Q,3,3) / (B,Q,3), or None in the self graph
    src_trans: np.ndarray
    mag: tuple               # the sums of |term|, in the same four shapes


def _row_dot(Rm, r, g0, g1, g2):
    return (Rm[r, 0] * g0 + Rm[r, 1] * g1) + Rm[r, 2] * g2


def frames_backward(rot, trans, row_ptr, col, in_ptr, in_edge, frame_mask=None, src_rot=None, src_trans=None, src_mask=None,
                    g_pos=None, g_rot=None) -> FrameGrads:
    rot, trans = np.asarray(rot), np.asarray(trans)
    assert rot.dtype == np.float32 and trans.dtype == np.float32
    B, M = rot.shape[:2]
    ok = np.ones((B, M), dtype=bool) if frame_mask is None else np.asarray(frame_mask) != 0
    bipartite = src_rot is not None
    srot, strans = (np.asarray(src_rot), np.asarray(src_trans)) if bipartite else (rot, trans)
    oks = ok if not bipartite else (np.ones(srot.shape[:2], dtype=bool) if src_mask is None else np.asarray(src_mask) != 0)
    Q = srot.shape[1]
    col = np.asarray(col).astype(np.int64)
    E = len(col)
    Rt, Tt = rot.reshape(B * M, 3, 3).astype(np.float64), trans.reshape(B * M, 3).astype(np.float64)
    Rs, Ts = srot.reshape(B * Q, 3, 3).astype(np.float64), strans.reshape(B * Q, 3).astype(np.float64)
    okt, oks = ok.reshape(-1), oks.reshape(-1)
    gp = None if g_pos is None else np.asarray(g_pos, dtype=np.float32).reshape(E, 3).astype(np.float64)
    gr = None if g_rot is None else np.asarray(g_rot, dtype=np.float32).reshape(E, 3, 3).astype(np.float64)
    rows = C.rows(row_ptr, E)
    tR, tT = np.zeros((B * M, 3, 3)), np.zeros((B * M, 3))
    mR, mT = np.zeros((B * M, 3, 3)), np.zeros((B * M, 3))
    sR, sT, smR, smT = (np.zeros((B * Q, 3, 3)), np.zeros((B * Q, 3)), np.zeros((B * Q, 3, 3)), np.zeros((B * Q, 3))) if bipartite \
        else (tR, tT, mR, mT)
    for o in range(B * Q):      # the outgoing terms, p ascending
        if not oks[o]:
            continue
        for p in range(min(max(int(row_ptr[o]), 0), E), min(max(int(row_ptr[o + 1]), 0), E)):
            if not 0 <= col[p] < M:
                continue
            fj = (o // Q) * M + col[p]
            if not okt[fj]:
                continue
            if gp is not None:
                v = Tt[fj] - Ts[o]
                for r in range(3):
                    term = _row_dot(Rs[o], r, *gp[p])
                    sT[o, r] = sT[o, r] - term
                    smT[o, r] += abs(term)
            for r in range(3):
                for c in range(3):
                    if gr is not None:
                        term = _row_dot(Rt[fj], r, *gr[p, c])
                        if gp is not None:
                            term = v[r] * gp[p, c] + term
                    else:
                        term = v[r] * gp[p, c]
                    sR[o, r, c] = sR[o, r, c] + term
                    smR[o, r, c] += abs(term)
    for o in range(B * M):      # then the incoming terms, e ascending
        if not okt[o]:
            continue
        for e in range(min(max(int(in_ptr[o]), 0), len(in_edge)), min(max(int(in_ptr[o + 1]), 0), len(in_edge))):
            p = int(in_edge[e])
            if not 0 <= p < E:
                continue
            i = int(rows[p])
            if i >= B * Q or col[p] != o % M or i // Q != o // M or not oks[i]:
                continue
            if gp is not None:
                for r in range(3):
                    term = _row_dot(Rs[i], r, *gp[p])
                    tT[o, r] = tT[o, r] + term
                    mT[o, r] += abs(term)
            if gr is not None:
                for r in range(3):
                    for c in range(3):
                        term = _row_dot(Rs[i], r, gr[p, 0, c], gr[p, 1, c], gr[p, 2, c])
                        tR[o, r, c] = tR[o, r, c] + term
                        mR[o, r, c] += abs(term)
    shaped = (tR.reshape(B, M, 3, 3), tT.reshape(B, M, 3))
    mags = (mR.reshape(B, M, 3, 3), mT.reshape(B, M, 3))
    if not bipartite:
        return FrameGrads(*shaped, None, None, mags + (None, None))
    return FrameGrads(*shaped, sR.reshape(B, Q, 3, 3), sT.reshape(B, Q, 3), mags + (smR.reshape(B, Q, 3, 3), smT.reshape(B, Q, 3)))


def frames_bound(ref, mag):
    """what K54 may be off by from the exact sum: 2^-23 |ref| + 2^-23 sum |term| + 2^-149"""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -23 * mag + 2.0 ** -149
