"""The yardstick of the edge-feature kernels on CSR graphs (ps_csr_edge_rows_i32, ps_csr_edge_rbf_f32,
ps_csr_edge_frames_f32; include/protstruc_csredge.h): their definitions in numpy float64, operation for operation, on the same
float32 inputs the kernels get.

    position p in [0, E) belongs to row r(p) = the number of t in 1 .. n_rows with row_ptr[t] <= p     (counted, not searched)
    padding where r(p) == n_rows or col[p] is outside [0, M); else b = r(p) // Q, q = r(p) % Q, j = col[p]
    pair t = (pair_i[t] on source q, pair_j[t] on target j)
    X = (double)x      dx = Xj.x - Xq.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz      d = (float)sqrt(d2)
    rbf[t*R + c] = exp(-z*z), z = (d - centers[c]) / sigma     in float64 on the float32 d, centers and sigma
    v = t_j - t_q;  local_pos and rel_rot as tests/edge_ref.py states them

Every numpy operation rounds on its own, as the kernels' do under -ffp-contract=off: ``dist``, ``local_pos`` and ``rel_rot``
come back rounded to float32 once and the tests demand the same bits; ``rbf`` stays in float64 and the kernel owes it to
within 1e-6 absolute.  Everything is exactly 0 at the padding and where an atom or a frame is outside its mask; values there
are replaced before any arithmetic.
"""
from typing import NamedTuple

import numpy as np


class Rbf(NamedTuple):
    dist: np.ndarray     # (E,P) float32
    rbf: np.ndarray      # (E,P*R) float64
    real: np.ndarray     # (E,P) bool: the position is an edge and both atoms are in their masks


class Frames(NamedTuple):
    local_pos: np.ndarray   # (E,3) float32
    rel_rot: np.ndarray     # (E,3,3) float32
    real: np.ndarray        # (E,) bool


def rows(row_ptr, E):
    """r(p) for p in [0, E): the definition counted out, with no search and no assumption on row_ptr"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    p = np.arange(E, dtype=np.int64)
    return (row_ptr[None, 1:] <= p[:, None]).sum(axis=1).astype(np.int64)


def edge_rows(row_ptr, Q, E):
    """(batch (E,) int32, row (E,) int32), -1 where r(p) == n_rows"""
    n_rows = len(row_ptr) - 1
    r = rows(row_ptr, E)
    tail = r == n_rows
    safe = np.where(tail, 0, r)
    Qd = max(Q, 1)
    return (np.where(tail, -1, safe // Qd).astype(np.int32), np.where(tail, -1, safe % Qd).astype(np.int32))


def _edges(row_ptr, col, Q, M):
    """(b, q, j, real) per position, the indices 0 where the position is padding"""
    col = np.asarray(col).astype(np.int64)
    E = col.shape[0]
    batch, row = edge_rows(row_ptr, Q, E)
    real = (batch >= 0) & (col >= 0) & (col < M)
    return np.where(real, batch, 0).astype(np.int64), np.where(real, row, 0).astype(np.int64), np.where(real, col, 0), real


def _clean(values, ok, tail_dims):
    """float64 copy with everything outside ``ok`` replaced by 0 before any arithmetic"""
    return np.where(ok.reshape(ok.shape + (1,) * tail_dims), values, np.float32(0)).astype(np.float64)


def edge_rbf(xyz, row_ptr, col, atom_mask, pair_i, pair_j, centers, sigma, src_xyz=None, src_mask=None) -> Rbf:
    """xyz (B,M,A,3) float32 the targets; src_xyz (B,Q,As,3) or None: the targets, with their mask"""
    x, centers = np.asarray(xyz), np.asarray(centers)
    assert x.dtype == np.float32 and centers.dtype == np.float32, "the yardstick takes the kernel's own float32 values"
    B, M, A = x.shape[:3]
    ok = np.ones((B, M, A), dtype=bool) if atom_mask is None else np.asarray(atom_mask) != 0
    if src_xyz is None:
        assert src_mask is None
        s, oks = x, ok
    else:
        s = np.asarray(src_xyz)
        assert s.dtype == np.float32
        oks = np.ones(s.shape[:3], dtype=bool) if src_mask is None else np.asarray(src_mask) != 0
    Q = s.shape[1]
    assert len(row_ptr) == B * Q + 1
    pi, pj = np.asarray(pair_i, dtype=np.int64), np.asarray(pair_j, dtype=np.int64)
    E, P, R = len(col), len(pi), len(centers)
    b, q, j, real_edge = _edges(row_ptr, col, Q, M)
    if not (B and M and Q and E):
        return Rbf(np.zeros((E, P), np.float32), np.zeros((E, P * R)), np.zeros((E, P), bool))
    X, S = _clean(x, ok, 1), _clean(s, oks, 1)
    Xi, oki = S[b, q][:, pi], oks[b, q][:, pi]                            # (E,P,3), (E,P)
    Xj, okj = X[b, j][:, pj], ok[b, j][:, pj]
    real = real_edge[:, None] & oki & okj
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (Xj[..., c] - Xi[..., c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        dist = np.where(real, np.sqrt(d2).astype(np.float32), np.float32(0))
        z = (dist.astype(np.float64)[..., None] - centers.astype(np.float64)) / np.float64(np.float32(sigma))
        rbf = np.where(real[..., None], np.exp(-(z * z)), 0.0)
    return Rbf(dist, rbf.reshape(E, P * R), real)


def edge_frames(rot, trans, row_ptr, col, frame_mask=None, src_rot=None, src_trans=None, src_mask=None) -> Frames:
    rot, trans = np.asarray(rot), np.asarray(trans)
    assert rot.dtype == np.float32 and trans.dtype == np.float32
    B, M = rot.shape[:2]
    ok = np.ones((B, M), dtype=bool) if frame_mask is None else np.asarray(frame_mask) != 0
    if src_rot is None:
        assert src_trans is None and src_mask is None
        srot, strans, oks = rot, trans, ok
    else:
        srot, strans = np.asarray(src_rot), np.asarray(src_trans)
        assert srot.dtype == np.float32 and strans.dtype == np.float32
        oks = np.ones(srot.shape[:2], dtype=bool) if src_mask is None else np.asarray(src_mask) != 0
    Q = srot.shape[1]
    assert len(row_ptr) == B * Q + 1
    E = len(col)
    b, q, j, real = _edges(row_ptr, col, Q, M)
    if not (B and M and Q and E):
        return Frames(np.zeros((E, 3), np.float32), np.zeros((E, 3, 3), np.float32), np.zeros(E, bool))
    Rt, Tt = _clean(rot, ok, 2), _clean(trans, ok, 1)
    Rs, Ts = _clean(srot, oks, 2), _clean(strans, oks, 1)
    real = real & oks[b, q] & ok[b, j]
    Ri, Rj = Rs[b, q], Rt[b, j]                                           # (E,3,3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = Tt[b, j] - Ts[b, q]
        pos = np.stack([(Ri[:, 0, c] * v[:, 0] + Ri[:, 1, c] * v[:, 1]) + Ri[:, 2, c] * v[:, 2] for c in range(3)], axis=-1)
        rel = np.stack([np.stack([(Ri[:, 0, a] * Rj[:, 0, c] + Ri[:, 1, a] * Rj[:, 1, c]) + Ri[:, 2, a] * Rj[:, 2, c]
                                  for c in range(3)], axis=-1) for a in range(3)], axis=-2)
    return Frames(np.where(real[:, None], pos.astype(np.float32), np.float32(0)),
                  np.where(real[:, None, None], rel.astype(np.float32), np.float32(0)), real)


# ---- cases -------------------------------------------------------------------------------------------------------------------
def to_csr(idx):
    """a padded (B,Q,k) list (negative: padding) as (row_ptr int64, col int32, keep (B,Q,k) bool): numpy's own
    restatement of geometry.neighbors_to_radius_graph"""
    idx = np.asarray(idx)
    keep = idx >= 0
    row_ptr = np.zeros(keep.shape[0] * keep.shape[1] + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(keep.sum(-1).reshape(-1))
    return row_ptr, idx[keep].astype(np.int32), keep


def graph_of_lengths(lengths, M, seed, E=None):
    """(row_ptr, col): rows of the given lengths with random targets in [0, M); ``E`` other than the sum cuts the buffers
    or leaves a tail of -1"""
    lengths = np.asarray(lengths, dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(row_ptr[-1])
    E = total if E is None else E
    rng = np.random.default_rng(seed)
    col = np.full(E, -1, dtype=np.int32)
    col[:min(E, total)] = rng.integers(0, max(M, 1), size=min(E, total))
    return row_ptr, col


CHUNK_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 64 * 3 + 1)


def chunk_lengths(E, n_rows):
    """Row lengths that sum to ``E`` over ``n_rows`` rows (a multiple of what the caller's B needs), shaped against the
    chunks of 64 positions: the first and the last row are empty; where E allows, a row ends exactly at position 64, a
    row spans three chunks (from inside chunk 1 to inside chunk 3), and a run of more than 40 rows of length 0 and 1
    alternates inside one chunk."""
    lengths = [0]
    left = E
    if E >= 64 * 3 + 1:
        lengths += [20] + [0, 1] * 22 + [22]      # 20 + 22 + 22 = 64: chunk 0 holds 46 rows, and a row ends on its boundary
        lengths += [10, 119]                       # the second of them runs from position 74 to 192: chunks 1, 2 and 3
        left -= 64 + 10 + 119
    elif E >= 64:
        lengths += [20] + [0, 1] * 22 + [22]
        left -= 64
    while left > 0:
        take = min(left, 1 + (left * 7) % 5)
        lengths += [take, 0]
        left -= take
    lengths += [0]
    assert len(lengths) <= n_rows, (len(lengths), n_rows)
    lengths = lengths[:-1] + [0] * (n_rows - len(lengths)) + [0]
    assert sum(lengths) == E and lengths[0] == 0 and lengths[-1] == 0
    return np.asarray(lengths, dtype=np.int64)
