"""The yardstick of the radius graph (include/protstruc_graph.h): its definition in numpy float64, operation for operation,
on the same float32 inputs the kernels get -- brute force over all pairs.

    X = (double)x      dx = Xj.x - Xq.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz
    j is a neighbour of q iff both are in their masks, their keys differ (where keys are given), j != q in the self graph
    (unless include_self), d2 is finite and d2 <= C2 = (double)cutoff * (double)cutoff
    count (Q,)   row_ptr = the exclusive prefix sum of count   col = the neighbours, ascending in j   dist = (float)sqrt(d2)

Every numpy operation rounds on its own, as the kernel's do under -ffp-contract=off, and a double square root and its
conversion to float32 are correctly rounded on both sides: the tests demand EQUAL count, row_ptr and col and bitwise equal
dist.  Also here: a float32 restatement of the box test (csrc/radius_box.hpp), the case families of
tests/test_gpu_radius.py, and the conditions that keep those cases from passing vacuously (``assert_family``).
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from tests import knn_ref

TILE = 64
CHUNK = 1024


class Radius(NamedTuple):
    count: np.ndarray      # (B,Q) int32 -- (Q,) from ``radius``
    row_ptr: np.ndarray    # (B*Q+1,) int64
    col: np.ndarray        # (E,) int32
    dist: np.ndarray       # (E,) float32


def near_matrix(points, cutoff, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None,
                include_self=False):
    """(near (Q,M) bool, d2 (Q,M) float64) of one structure: the predicate of the definition, pair by pair.  Masked
    coordinates are replaced before any arithmetic."""
    x = np.asarray(points)
    assert x.dtype == np.float32, "the yardstick takes the kernel's own float32 values"
    M = x.shape[0]
    ok_j = np.ones(M, dtype=bool) if mask is None else np.asarray(mask) != 0
    self_graph = queries is None
    if self_graph:
        assert query_mask is None and query_exclude is None
        y, ok_q, query_exclude = x, ok_j, exclude
    else:
        y = np.asarray(queries)
        assert y.dtype == np.float32
        ok_q = np.ones(y.shape[0], dtype=bool) if query_mask is None else np.asarray(query_mask) != 0
        assert (exclude is None) == (query_exclude is None)
    assert np.isfinite(cutoff) and cutoff > 0
    X = np.where(ok_j[:, None], x, np.float32(0)).astype(np.float64)
    Y = np.where(ok_q[:, None], y, np.float32(0)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (X[None, :, c] - Y[:, None, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        C2 = np.float64(np.float32(cutoff)) * np.float64(np.float32(cutoff))
        near = (ok_q[:, None] & ok_j[None, :]) & np.isfinite(d2) & (d2 <= C2)
    if exclude is not None:
        near &= np.asarray(query_exclude)[:, None] != np.asarray(exclude)[None, :]
    if self_graph and not include_self:
        near[np.arange(M), np.arange(M)] = False
    return near, d2


def radius(points, cutoff, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None,
           include_self=False) -> Radius:
    """One structure: points (M,3) float32, mask (M,) or None; queries (Q,3) float32 or None = the points themselves;
    exclude (M,) / query_exclude (Q,) integers or None.  Brute force over every pair of a query and a candidate that are in
    their masks (a pair with a masked member is no edge, whatever lies under the mask), CHUNK queries at a time."""
    x = np.asarray(points)
    self_graph = queries is None
    y = x if self_graph else np.asarray(queries)
    M, Q = x.shape[0], y.shape[0]
    ok_j = np.ones(M, dtype=bool) if mask is None else np.asarray(mask) != 0
    ok_q = ok_j if self_graph else np.ones(Q, dtype=bool) if query_mask is None else np.asarray(query_mask) != 0
    if self_graph:
        assert query_mask is None and query_exclude is None
        query_exclude = exclude
    jj, qq = np.flatnonzero(ok_j), np.flatnonzero(ok_q)
    keys = {} if exclude is None else dict(exclude=np.asarray(exclude)[jj])
    count = np.zeros(Q, dtype=np.int32)
    cols, dists = [np.zeros(0, dtype=np.int32)], [np.zeros(0, dtype=np.float32)]
    for r0 in range(0, qq.size, CHUNK):
        rows = qq[r0:r0 + CHUNK]
        if exclude is not None:
            keys["query_exclude"] = np.asarray(query_exclude)[rows]
        near, d2 = near_matrix(x[jj], cutoff, None, y[rows], None, **keys)
        if self_graph and not include_self:
            near &= rows[:, None] != jj[None, :]
        r, c = np.nonzero(near)                                        # row-major: rows ascending, j ascending within a row
        count[rows] = near.sum(axis=1)
        cols.append(jj[c].astype(np.int32))
        dists.append(np.sqrt(d2[r, c]).astype(np.float32))
    row_ptr = np.concatenate([[0], np.cumsum(count, dtype=np.int64)]).astype(np.int64)
    return Radius(count, row_ptr, np.concatenate(cols), np.concatenate(dists))


def batch(points, cutoff, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None, **kw) -> Radius:
    """The graph of (B,M,3), (B,M), ...: the structures' rows one after the other, in (b, q) order."""
    pick = lambda t, b: None if t is None else t[b]   # noqa: E731
    each = [radius(points[b], cutoff, pick(mask, b), pick(queries, b), pick(query_mask, b), pick(exclude, b),
                   pick(query_exclude, b), **kw) for b in range(points.shape[0])]
    Q = points.shape[1] if queries is None else queries.shape[1]
    count = np.stack([r.count for r in each]) if each else np.zeros((0, Q), dtype=np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(count.reshape(-1), dtype=np.int64)]).astype(np.int64)
    col = np.concatenate([r.col for r in each] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    dist = np.concatenate([r.dist for r in each] + [np.zeros(0, dtype=np.float32)]).astype(np.float32)
    return Radius(count, row_ptr, col, dist)


def rows_of(ref: Radius):
    """[(col, dist)] per row"""
    return [(ref.col[a:b], ref.dist[a:b]) for a, b in zip(ref.row_ptr[:-1], ref.row_ptr[1:])]


# ---- the box test, restated in float32 -------------------------------------------------------------------------------------------
def reject_above(cutoff):
    """fl32(C2) * (1 + 2^-20) + 2^-126, every operation in float32"""
    with np.errstate(over="ignore", under="ignore"):
        C2 = np.float64(np.float32(cutoff)) * np.float64(np.float32(cutoff))
        return np.float32(np.float32(C2) * np.float32(1.0 + 2.0 ** -20)) + np.float32(2.0 ** -126)


def box(points, mask=None):
    """(lo (3,), hi (3,), n) of the finite, unmasked points of (m,3) float32; the empty box is +inf, -inf, 0"""
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x).all(axis=1)
    if mask is not None:
        ok &= np.asarray(mask).reshape(-1) != 0
    if not ok.any():
        return np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32), 0
    return x[ok].min(axis=0), x[ok].max(axis=0), int(ok.sum())


def gap2(a, b):
    """G of two non-empty boxes, in float32"""
    with np.errstate(over="ignore", under="ignore"):
        g = np.maximum(np.float32(0), np.maximum(a[0] - b[1], b[0] - a[1])).astype(np.float32)
        sq = (g * g).astype(np.float32)
        return np.float32(np.float32(sq[0] + sq[1]) + sq[2])


def dropped(a, b, cutoff) -> bool:
    """whether the candidates' box ``b`` is dropped for the queries' box ``a`` (both non-empty or b empty)"""
    return b[2] == 0 or bool(gap2(a, b) > reject_above(cutoff))


def block_decisions(points, cutoff, mask=None, queries=None, query_mask=None):
    """One structure: (dropped (W,T) bool, holds (W,T) bool) over the waves of 64 queries and the blocks of 64 candidates --
    what the wave-level test decides, and whether the pair of blocks holds a pair within the cutoff (keys and the self
    pair ignored: the box test does not know them)."""
    x = np.asarray(points)
    y, qm = (x, mask) if queries is None else (np.asarray(queries), query_mask)
    near, _ = near_matrix(x, cutoff, mask, None if queries is None else y, None if queries is None else qm, include_self=True)
    W, T = -(-y.shape[0] // TILE), -(-x.shape[0] // TILE)
    drop, holds = np.zeros((W, T), dtype=bool), np.zeros((W, T), dtype=bool)
    for w in range(W):
        a = box(y[w * TILE:(w + 1) * TILE], None if qm is None else qm[w * TILE:(w + 1) * TILE])
        for t in range(T):
            b = box(x[t * TILE:(t + 1) * TILE], None if mask is None else mask[t * TILE:(t + 1) * TILE])
            drop[w, t] = a[2] == 0 or dropped(a, b, cutoff)
            holds[w, t] = near[w * TILE:(w + 1) * TILE, t * TILE:(t + 1) * TILE].any()
    return drop, holds


# ---- the case families ---------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 257, 1000)      # the lane end, the block boundary, two and three blocks, many
CUTOFFS = (4.0, 12.0)
CROSS_Q = (1, 65, 130)
LATTICE_N, LATTICE_CUTOFF = 8, 3.0                        # C2 = 9 = 3^2 + 0 + 0 = 2^2 + 2^2 + 1: attained


class Case(NamedTuple):
    x: np.ndarray                      # (B,M,3) float32
    mask: Optional[np.ndarray]         # (B,M) bool or None
    key: Optional[np.ndarray] = None   # (B,M) int32: the exclusion key the family is also run with


@functools.lru_cache(maxsize=None)
def chain(M) -> Case:
    """knn_ref.chain_case: structure 0 with 45 % of the slots masked over NaN, structure 1 all padding, structure 2 complete;
    the key is the index // 4 (a "residue" of four atoms)"""
    c = knn_ref.chain_case(M, seed=11)
    return Case(c.x, c.mask, np.broadcast_to(np.arange(M, dtype=np.int32) // 4, (3, M)).copy())


@functools.lru_cache(maxsize=None)
def permuted(M=1000) -> Case:
    """the complete chain of ``chain(M)`` and a copy with its points in random order: no block of the copy is coherent"""
    x = chain(M).x[2]
    perm = np.random.default_rng(5).permutation(M)
    return Case(np.stack([x, x[perm]]), None)


@functools.lru_cache(maxsize=None)
def clusters(M=384) -> Case:
    """two compact clusters of M / 2 points (three blocks each), 1000 A apart on x; 10 % masked over NaN"""
    rng = np.random.default_rng(6)
    x = (rng.normal(size=(1, M, 3)) * 4.0).astype(np.float32)
    x[0, M // 2:, 0] += np.float32(1000.0)
    mask = rng.random((1, M)) >= 0.1
    x[~mask] = np.nan
    return Case(x, mask)


@functools.lru_cache(maxsize=None)
def lattice() -> Case:
    """the integer lattice {0 .. 7}^3, x slowest: block t is the plane x = t, every d2 is a small integer"""
    return Case(knn_ref.lattice(LATTICE_N)[None], None)


def trap(c) -> Case:
    """block 0 is 64 copies of the origin, block 1 is 64 copies of (c, 0, 0)"""
    x = np.zeros((1, 2 * TILE, 3), dtype=np.float32)
    x[0, TILE:, 0] = np.float32(c)
    return Case(x, None)


def assert_family(name, cases_and_cutoffs, may_drop=True):
    """The conditions of a synthetic family, over its (Case, cutoff) members together: some row has more than 64
    neighbours; the wave-level test drops some pair of blocks and keeps some (``may_drop`` False: it drops none, and says
    so); and -- always -- no pair of blocks that holds a neighbour pair is dropped."""
    most, n_dropped, n_kept = 0, 0, 0
    for case, cutoff in cases_and_cutoffs:
        for b in range(case.x.shape[0]):
            mask = None if case.mask is None else case.mask[b]
            near, _ = near_matrix(case.x[b], cutoff, mask)
            most = max(most, int(near.sum(axis=1).max(initial=0)))
            drop, holds = block_decisions(case.x[b], cutoff, mask)
            assert not (drop & holds).any(), f"{name}: a block pair with a neighbour pair is dropped"
            nonempty = np.array([box(case.x[b][t * TILE:(t + 1) * TILE], None if mask is None else mask[t * TILE:(t + 1) * TILE])[2] > 0
                                 for t in range(drop.shape[1])])
            n_dropped += int(drop[nonempty][:, nonempty].sum())
            n_kept += int((~drop[nonempty][:, nonempty]).sum())
    assert most > 64, f"{name}: no row has more than 64 neighbours (the longest has {most})"
    assert n_kept > 0, f"{name}: every pair of blocks is dropped"
    assert (n_dropped > 0) == may_drop, f"{name}: {n_dropped} pairs of non-empty blocks are dropped"
    return most, n_dropped, n_kept
