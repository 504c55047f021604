"""A float64 numpy restatement of K55 - K59 (include/protstruc_aggregate.h): segment reduce, segment gather, edge dot, segment
softmax and its backward pass, with the header's vocabulary -- the edge list, the padding, the two groupings -- and explicit
ascending loops over the members (never ``np.sum``, whose order is pairwise).  A row's H * D floats are carried through a
loop together: elementwise float64 arithmetic is the same operation per float.  Where the header promises bits (K55, K56,
K57, K59) the float32 results here are those bits."""
import numpy as np

from tests.edge_grad_ref import incoming  # noqa: F401 -- the incoming list, (in_ptr, in_edge), of ops.csr_incoming_edges

MODES = ("sum", "mean", "max", "min")


def real_positions(row_ptr, col, M):
    """bool [E]: False at the padding -- from row_ptr[-1] on, and where col is outside [0, M)"""
    col = np.asarray(col)
    p = np.arange(len(col))
    return (p < int(row_ptr[-1])) & (col >= 0) & (col < M)


def edge_index(row_ptr, col, Q, M, at):
    """int64 [E]: the flat node of every edge position at its source or target, -1 at the padding"""
    col = np.asarray(col).astype(np.int64)
    E = len(col)
    r = np.searchsorted(np.asarray(row_ptr)[1:], np.arange(E), side="right")
    flat = (r // max(Q, 1)) * M + col if at == "target" else r
    return np.where(real_positions(row_ptr, col, M), flat, -1).astype(np.int64)


def grouping(row_ptr, col, B, Q, M, at):
    """(ptr, perm, S): the source grouping (row_ptr, None, B*Q) or the target grouping (in_ptr, in_edge, B*M)"""
    if at == "source":
        return np.asarray(row_ptr, dtype=np.int64), None, B * Q
    ptr, perm = incoming(row_ptr, col, B, Q, M)
    return ptr, perm, B * M


def members(ptr, perm, s, E, real):
    """the contributing members of segment s, ascending: bounds cut to the list, members outside [0, E) or at the padding
    skipped"""
    limit = E if perm is None else len(perm)
    lo, hi = (min(max(int(v), 0), limit) for v in (ptr[s], ptr[s + 1]))
    for t in range(lo, hi):
        e = t if perm is None else int(perm[t])
        if 0 <= e < E and (real is None or real[e]):
            yield e


def segment_reduce(values, ptr, perm, S, mode, weight=None, real=None, exact=False):
    """K55: (out float32 [S,H,D], arg int64 [S,H,D] or None); ``exact``: out in float64, before its one rounding"""
    values = np.asarray(values, dtype=np.float32)
    E, H, D = values.shape
    assert mode in MODES and not (mode in ("max", "min") and weight is not None)
    out = np.zeros((S, H, D), dtype=np.float64 if exact else np.float32)
    arg = np.full((S, H, D), -1, dtype=np.int64) if mode in ("max", "min") else None
    v64 = values.astype(np.float64)
    w64 = None if weight is None else np.asarray(weight, dtype=np.float32).astype(np.float64)
    for s in range(S):
        acc, n = np.zeros((H, D)), 0
        best = where = None
        for e in members(ptr, perm, s, E, real):
            if mode in ("sum", "mean"):
                acc = acc + (v64[e] if w64 is None else w64[e][:, None] * v64[e])
            elif n == 0:
                best, where = values[e].copy(), np.full((H, D), e, dtype=np.int64)
            else:
                better = values[e] > best if mode == "max" else values[e] < best
                best, where = np.where(better, values[e], best), np.where(better, e, where)
            n += 1
        if mode in ("sum", "mean"):
            out[s] = (acc / float(n) if mode == "mean" and n else acc).astype(out.dtype)
        elif n:
            out[s], arg[s] = best, where
    return out, arg


def segment_gather(node, index, weight=None, exact=False):
    """K56: float32 [E,H,D]; ``exact``: float64, before the one rounding"""
    node = np.asarray(node, dtype=np.float32)
    S, H, D = node.shape
    out = np.zeros((len(index), H, D), dtype=np.float64 if exact else np.float32)
    for e, o in enumerate(index):
        if 0 <= o < S:
            out[e] = node[o] if weight is None else \
                (np.asarray(weight[e], dtype=np.float32).astype(np.float64)[:, None] * node[o].astype(np.float64)).astype(out.dtype)
    return out


def tree_sum(u):
    """the header's order over the last axis of float64 ``u``: fours ascending, then a tree over the partial sums"""
    D = u.shape[-1]
    K = (D + 3) // 4
    s = []
    for k in range(K):
        part = u[..., 4 * k]
        for i in range(4 * k + 1, min(4 * k + 4, D)):
            part = part + u[..., i]
        s.append(part)
    stride = 1
    while stride < K:
        for k in range(0, K, 2 * stride):
            if k + stride < K:
                s[k] = s[k] + s[k + stride]
        stride *= 2
    return s[0]


def edge_dot(node, values, index, exact=False):
    """K57: float32 [E,H]; ``exact``: float64, before the one rounding"""
    node, values = np.asarray(node, dtype=np.float32), np.asarray(values, dtype=np.float32)
    S, H, D = node.shape
    out = np.zeros((len(index), H), dtype=np.float64 if exact else np.float32)
    for e, o in enumerate(index):
        if 0 <= o < S:
            out[e] = tree_sum(node[o].astype(np.float64) * values[e].astype(np.float64)).astype(out.dtype)
    return out


def segment_softmax(logits, ptr, perm, S, real=None):
    """K58: (w float64 [E,H] before its one rounding, lse float64 [S,H]); compare with K58's bound, not bit for bit"""
    logits = np.asarray(logits, dtype=np.float32)
    E, H = logits.shape
    w = np.zeros((E, H))
    lse = np.full((S, H), -np.inf)
    x64 = logits.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            mine = list(members(ptr, perm, s, E, real))
            for h in range(H):
                m = None
                for e in mine:
                    if m is None or logits[e, h] > m:
                        m = logits[e, h]
                if m is None or m == -np.inf:
                    continue
                total = 0.0
                for e in mine:
                    total = total + np.exp(x64[e, h] - np.float64(m))
                for e in mine:
                    w[e, h] = np.exp(x64[e, h] - np.float64(m)) / total
                lse[s, h] = np.float64(m) + np.log(total)
    return w, lse


def segment_softmax_backward(w, grad_w, ptr, perm, S, real=None, exact=False):
    """K59: float32 [E,H], given the saved float32 w; ``exact``: float64, before the one rounding"""
    w, grad_w = np.asarray(w, dtype=np.float32), np.asarray(grad_w, dtype=np.float32)
    E, H = w.shape
    out = np.zeros((E, H), dtype=np.float64 if exact else np.float32)
    w64, g64 = w.astype(np.float64), grad_w.astype(np.float64)
    with np.errstate(invalid="ignore"):
        for s in range(S):
            mine = list(members(ptr, perm, s, E, real))
            total = np.zeros(H)
            for e in mine:
                total = total + w64[e] * g64[e]
            for e in mine:
                out[e] = (w64[e] * (g64[e] - total)).astype(out.dtype)
    return out
