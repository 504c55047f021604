"""The yardstick of the edge-feature kernels (ps_edge_rbf_f32, ps_edge_frames_f32): their definitions in numpy float64,
operation for operation, on the same float32 inputs the kernels get.

    edge (i, s), j = idx[i][s]; padding where j is outside [0, N); pair p = (pair_i[p] on i, pair_j[p] on j)
    X = (double)x      dx = Xj.x - Xi.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz      d = (float)sqrt(d2)
    rbf[p*R + c] = exp(-z*z), z = (d - centers[c]) / sigma     in float64 on the float32 d, centers and sigma
    v = t_j - t_i
    local_pos[c]  = (R_i[0][c]*v0 + R_i[1][c]*v1) + R_i[2][c]*v2
    rel_rot[a][c] = (R_i[0][a]*R_j[0][c] + R_i[1][a]*R_j[1][c]) + R_i[2][a]*R_j[2][c]

Every numpy operation rounds on its own, as the kernels' do under -ffp-contract=off, and a double square root and the
conversions to float32 are correctly rounded on both sides: ``dist``, ``local_pos`` and ``rel_rot`` come back rounded to
float32 once and the tests demand the same bits.  ``rbf`` stays in float64: the kernel owes it to within 1e-6 absolute.
Everything is exactly 0 at the padding and where an atom or a frame is outside its mask; values there are replaced
before any arithmetic.
"""
from typing import NamedTuple

import numpy as np

from tests import knn_ref


class Rbf(NamedTuple):
    dist: np.ndarray     # (B,N,k,P) float32
    rbf: np.ndarray      # (B,N,k,P*R) float64
    real: np.ndarray     # (B,N,k,P) bool: the edge is no padding and both atoms are in the mask


class Frames(NamedTuple):
    local_pos: np.ndarray   # (B,N,k,3) float32
    rel_rot: np.ndarray     # (B,N,k,3,3) float32
    real: np.ndarray        # (B,N,k) bool


def _neighbours(idx, N):
    idx = np.asarray(idx).astype(np.int64)
    real = (idx >= 0) & (idx < N)
    return np.where(real, idx, 0), real


def edge_rbf(xyz, idx, atom_mask, pair_i, pair_j, centers, sigma) -> Rbf:
    """xyz (B,N,A,3) float32; idx (B,N,k) integers; atom_mask (B,N,A) or None; centers (R,) float32; sigma a float"""
    x = np.asarray(xyz)
    centers = np.asarray(centers)
    assert x.dtype == np.float32 and centers.dtype == np.float32, "the yardstick takes the kernel's own float32 values"
    B, N, A = x.shape[:3]
    ok = np.ones((B, N, A), dtype=bool) if atom_mask is None else np.asarray(atom_mask) != 0
    X = np.where(ok[..., None], x, np.float32(0)).astype(np.float64)    # masked values are replaced before any arithmetic
    j, real_edge = _neighbours(idx, N)
    pi, pj = np.asarray(pair_i, dtype=np.int64), np.asarray(pair_j, dtype=np.int64)
    rows = np.arange(B)[:, None, None, None]
    Xi, oki = X[:, :, None, pi], ok[:, :, None, pi]                      # (B,N,1,P,3), (B,N,1,P)
    Xj, okj = X[rows, j[..., None], pj], ok[rows, j[..., None], pj]      # (B,N,k,P,3), (B,N,k,P)
    real = real_edge[..., None] & oki & okj
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (Xj[..., c] - Xi[..., c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        dist = np.where(real, np.sqrt(d2).astype(np.float32), np.float32(0))
        z = (dist.astype(np.float64)[..., None] - centers.astype(np.float64)) / np.float64(np.float32(sigma))
        rbf = np.where(real[..., None], np.exp(-(z * z)), 0.0)
    return Rbf(dist, rbf.reshape(*dist.shape[:3], -1), real)


def edge_frames(rot, trans, idx, frame_mask=None) -> Frames:
    """rot (B,N,3,3) float32, basis vectors as columns; trans (B,N,3) float32; idx (B,N,k); frame_mask (B,N) or None"""
    rot, trans = np.asarray(rot), np.asarray(trans)
    assert rot.dtype == np.float32 and trans.dtype == np.float32
    B, N = rot.shape[:2]
    ok = np.ones((B, N), dtype=bool) if frame_mask is None else np.asarray(frame_mask) != 0
    R = np.where(ok[..., None, None], rot, np.float32(0)).astype(np.float64)
    T = np.where(ok[..., None], trans, np.float32(0)).astype(np.float64)
    j, real = _neighbours(idx, N)
    rows = np.arange(B)[:, None, None]
    real = real & ok[:, :, None] & ok[rows, j]
    Ri, Rj = R[:, :, None], R[rows, j]                                    # (B,N,1,3,3), (B,N,k,3,3)
    with np.errstate(invalid="ignore", over="ignore"):
        v = T[rows, j] - T[:, :, None]                                    # (B,N,k,3)
        pos = np.stack([(Ri[..., 0, c] * v[..., 0] + Ri[..., 1, c] * v[..., 1]) + Ri[..., 2, c] * v[..., 2]
                        for c in range(3)], axis=-1)
        rel = np.stack([np.stack([(Ri[..., 0, a] * Rj[..., 0, c] + Ri[..., 1, a] * Rj[..., 1, c]) + Ri[..., 2, a] * Rj[..., 2, c]
                                  for c in range(3)], axis=-1) for a in range(3)], axis=-2)
    return Frames(np.where(real[..., None], pos.astype(np.float32), np.float32(0)),
                  np.where(real[..., None, None], rel.astype(np.float32), np.float32(0)), real)


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    xyz: np.ndarray      # (3,N,A,3) float32, NaN at masked atoms
    mask: np.ndarray     # (3,N,A) bool


def residue_case(N, A, seed, masked=0.45) -> Case:
    """``knn_ref.chain_case`` expanded to A atom slots per residue: the chain's points are the residues' centres and every
    slot lies within about 2 A of its centre.  Structure 0 has a fraction ``masked`` of its slots masked with NaN
    coordinates under the mask, structure 1 is all masked (NaN), structure 2 is complete."""
    centres = knn_ref.chain_case(N, seed, masked=0.0).x                   # structure 1 is NaN, 0 and 2 are complete
    rng = np.random.default_rng(seed + 1000)
    xyz = (centres[:, :, None, :] + rng.normal(size=(3, N, A, 3)).astype(np.float32) * np.float32(1.2)).astype(np.float32)
    mask = np.ones((3, N, A), dtype=bool)
    mask[0] = rng.random((N, A)) >= masked
    mask[1] = False
    xyz[~mask] = np.nan
    return Case(xyz, mask)


def random_frames(B, N, seed):
    """(rot (B,N,3,3), trans (B,N,3)) float32: orthonormal bases from a QR decomposition, positions of a protein's size"""
    rng = np.random.default_rng(seed)
    rot = np.linalg.qr(rng.normal(size=(B, N, 3, 3)))[0].astype(np.float32)
    return rot, (rng.normal(size=(B, N, 3)) * 15.0).astype(np.float32)


def random_graph(B, N, k, seed, padded=0.2):
    """(B,N,k) int32: random neighbours in [0, N), a fraction ``padded`` of the entries -1"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, size=(B, N, k)).astype(np.int32)
    idx[rng.random((B, N, k)) < padded] = -1
    return idx
