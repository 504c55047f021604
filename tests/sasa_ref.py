"""The yardstick of the solvent-accessibility kernel: Shrake & Rupley's definition in numpy float64, on the same float32
inputs the kernel gets.

    R_i = (double)r_i + (double)probe          p_ik = x_i + R_i u_k
    buried(i, k) iff some j != i, both in the mask, (isolate_i == isolate_j), |p_ik - x_j|^2 < R_j^2
    count_i = #{k : not buried}                area_i = 4 pi R_i^2 count_i / S

Every atom loops over its candidate neighbours j -- those with |x_i - x_j| < R_i max|u| + R_j + 0.01, found from the dense
float64 distance matrix -- and all S directions.  A pair left out cannot bury a point: its test points are further than
R_j + 0.01 from x_j, more than 0.02 A^2 on the squared scale.  ``margin`` is the smallest | |p_ik - x_j|^2 - R_j^2 | over
every evaluated triple; the kernel's double evaluation errs below 1e-12 A^2 for coordinates under 1000 A, so with
``margin >= 1e-10`` equal counts are owed, not lucky.
"""
from typing import NamedTuple

import numpy as np

from tests import dssp_ref

SLACK = 0.01                                   # A: how much further than touching a candidate neighbour may be
RADII = {"N": 1.55, "CA": 1.7, "C": 1.7, "O": 1.52}


class Sasa(NamedTuple):
    count: np.ndarray     # (M,) int32
    area: np.ndarray      # (M,) float64, A^2
    buried: np.ndarray    # (M,S) bool; all False at masked points
    margin: float         # A^2; inf if no triple was evaluated


def sphere_points(n):
    """the golden spiral in float64, rounded to float32 once: (n,3)"""
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1).astype(np.float32)


def sasa(x, r, mask=None, isolate=None, probe=1.4, sphere=None, n_points=96) -> Sasa:
    """One structure: x (M,3) float32, r (M,) float32, mask (M,) bool or None, isolate (M,) integers or None, sphere (S,3)
    float32 or None (= ``sphere_points(n_points)``).  Masked coordinates and radii are never read."""
    x, r = np.asarray(x), np.asarray(r)
    assert x.dtype == np.float32 and r.dtype == np.float32, "the yardstick takes the kernel's own float32 values"
    u = sphere_points(n_points) if sphere is None else np.asarray(sphere)
    assert u.dtype == np.float32
    u = u.astype(np.float64)
    M, S = x.shape[0], u.shape[0]
    mask = np.ones(M, dtype=bool) if mask is None else np.asarray(mask) != 0
    count, area, buried, margin = np.zeros(M, dtype=np.int32), np.zeros(M), np.zeros((M, S), dtype=bool), np.inf
    valid = np.flatnonzero(mask)
    if valid.size == 0:
        return Sasa(count, area, buried, margin)
    xv = x[valid].astype(np.float64)
    R = r[valid].astype(np.float64) + np.float64(np.float32(probe))
    key = None if isolate is None else np.asarray(isolate)[valid]
    dist = np.sqrt(((xv[:, None, :] - xv[None, :, :]) ** 2).sum(-1))
    reach = R * np.sqrt((u * u).sum(-1)).max()
    for a, i in enumerate(valid):
        cand = dist[a] < reach[a] + R + SLACK
        cand[a] = False                                           # j != i, by index: a coincident atom is a neighbour
        if key is not None:
            cand &= key == key[a]
        p = xv[a] + R[a] * u                                      # (S,3)
        d2 = ((p[:, None, :] - xv[cand][None, :, :]) ** 2).sum(-1)   # (S, neighbours)
        gap = d2 - (R[cand] ** 2)[None, :]
        if gap.size:
            margin = min(margin, float(np.abs(gap).min()))
        buried[i] = (gap < 0).any(-1)
        count[i] = S - int(buried[i].sum())
        area[i] = 4.0 * np.pi * R[a] * R[a] * count[i] / S
    return Sasa(count, area, buried, margin)


def batch(x, r, mask=None, isolate=None, **kw):
    """[Sasa] per structure of (B,M,3), (B,M), ..."""
    return [sasa(x[b], r[b], None if mask is None else mask[b], None if isolate is None else isolate[b], **kw)
            for b in range(x.shape[0])]


# ---- synthetic structures -------------------------------------------------------------------------------------------------
def self_avoiding_walk(L, rng, step=3.8, clearance=4.0):
    """(L,3) a CA trace with ``step`` between neighbours that comes no closer than ``clearance`` to any earlier CA but
    its predecessor: packed like a chain, never overlapping like a Gaussian cloud"""
    ca = np.zeros((L, 3))
    for k in range(1, L):
        for _ in range(10000):
            d = rng.normal(size=3)
            cand = ca[k - 1] + step * d / np.linalg.norm(d)
            if k < 2 or np.sqrt(((ca[:k - 1] - cand) ** 2).sum(-1)).min() >= clearance:
                break
        else:
            raise RuntimeError("the walk is stuck; take another seed")
        ca[k] = cand
    return ca


def chain_atoms(M, rng):
    """(M,3) float64 and (M,) float32: the first M of the N, CA, C, O atoms placed around a self-avoiding 3.8 A walk
    (``dssp_ref.backbone_on_trace``), moved off the origin, with their radii"""
    L = max((M + 3) // 4, 1)
    atoms = dssp_ref.backbone_on_trace(self_avoiding_walk(L, rng, clearance=4.5)).reshape(-1, 3)[:M]
    radii = np.tile(np.array([RADII[a] for a in ("N", "CA", "C", "O")], dtype=np.float32), L)[:M]
    return atoms + rng.normal(size=3) * 5.0, radii


class Case(NamedTuple):
    x: np.ndarray          # (B,M,3) float32, NaN at masked points
    r: np.ndarray          # (B,M) float32, NaN at some masked points
    mask: np.ndarray       # (B,M) bool
    isolate: object        # (B,M) int32 or None


def synthetic_case(M, seed, B=3, masked=0.1, keys=0) -> Case:
    """B structures of M points: structure 1 is all padding (NaN, masked); a fraction ``masked`` of the points of structure
    0 is masked with NaN coordinates (every other one also a NaN radius); ``keys`` > 0 deals the points of every structure
    into that many ``isolate`` classes in runs of random length."""
    rng = np.random.default_rng(seed)
    x = np.full((B, M, 3), np.nan, dtype=np.float32)
    r = np.full((B, M), np.nan, dtype=np.float32)
    mask = np.zeros((B, M), dtype=bool)
    for b in range(B):
        if b == 1:
            continue
        atoms, radii = chain_atoms(M, rng)
        ok = rng.random(M) >= masked if b == 0 and M > 2 else np.ones(M, dtype=bool)
        mask[b] = ok
        x[b] = np.where(ok[:, None], atoms.astype(np.float32), np.nan)
        nan_radius = ~ok & (np.arange(M) % 2 == 0)
        r[b] = np.where(nan_radius, np.nan, radii)
    isolate = None
    if keys:
        isolate = np.zeros((B, M), dtype=np.int32)
        for b in range(B):
            cuts = np.sort(rng.choice(np.arange(1, M), size=min(2 * keys, M - 1), replace=False))
            isolate[b] = (np.searchsorted(cuts, np.arange(M), side="right") % keys).astype(np.int32)
    return Case(x, r, mask, isolate)


def case_reference(case: Case, **kw):
    return batch(case.x, case.r, case.mask, case.isolate, **kw)


def edge_pairs(factors=(1.0 - 1e-6, 1.0 + 1e-6, 0.999), ks=(0, 7, 50, 95), n_points=96, probe=1.4):
    """Pairs at the edge of the kernel's fp32 pre-test, (B,2,3) / (B,2): atom 0 at the origin with radius 1.7, atom 1
    with radius 1.52 at distance ``factor (R_0 + R_1)`` along direction k of the table, so that test point k of atom 0
    lies ``(factor - 1)(R_0 + R_1)`` (and the rounding of |u_k|) outside the other's sphere or inside it."""
    u = sphere_points(n_points).astype(np.float64)
    r = np.array([1.7, 1.52], dtype=np.float32)
    R = r.astype(np.float64) + np.float64(np.float32(probe))
    x = np.zeros((len(factors) * len(ks), 2, 3), dtype=np.float32)
    for a, f in enumerate(factors):
        for c, k in enumerate(ks):
            x[a * len(ks) + c, 1] = (f * (R[0] + R[1]) * u[k] / np.linalg.norm(u[k])).astype(np.float32)
    return x, np.broadcast_to(r, (x.shape[0], 2)).copy()
