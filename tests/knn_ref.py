"""The yardstick of the nearest-neighbour kernel: its definition in numpy float64, operation for operation, on the same
float32 inputs the kernel gets.

    X = (double)x      dx = Xj.x - Xq.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz
    j is a neighbour of q iff both are in their masks, their keys differ (where keys are given), j != q in the self graph
    (unless include_self), d2 is finite and d2 <= C2 = (double)cutoff * (double)cutoff
    the neighbours in the order of (d2, j), the first k kept;  idx = j (padding -1), dist = (float)sqrt(d2) (padding +inf)

Every numpy operation rounds on its own, as the kernel's do under -ffp-contract=off, and a double square root and its
conversion to float32 are correctly rounded on both sides: the tests demand EQUAL indices and counts and bitwise equal
distances.  Also here: the case builders -- the compact random chain of ``sasa_ref`` and the integer lattice, whose many
exactly equal distances exercise the rule "equal distances go to the lower index".
"""
from typing import NamedTuple

import numpy as np

from tests import sasa_ref


class Knn(NamedTuple):
    idx: np.ndarray      # (Q,k) int32, -1 at the padding
    dist: np.ndarray     # (Q,k) float32, +inf at the padding
    count: np.ndarray    # (Q,) int32
    d2: np.ndarray       # (Q,M) float64: the squared distances, NaN where either point is masked


def knn(points, k, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None, cutoff=np.inf,
        include_self=False) -> Knn:
    """One structure: points (M,3) float32, mask (M,) or None; queries (Q,3) float32 or None = the points themselves (then
    query_mask and query_exclude are the points'); exclude (M,) / query_exclude (Q,) integers or None.  Masked coordinates
    are never read."""
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
    Q = y.shape[0]
    X = np.where(ok_j[:, None], x, np.float32(0)).astype(np.float64)     # masked values are replaced before any arithmetic
    Y = np.where(ok_q[:, None], y, np.float32(0)).astype(np.float64)
    pair = ok_q[:, None] & ok_j[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (X[None, :, c] - Y[:, None, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
    C2 = np.float64(np.float32(cutoff)) * np.float64(np.float32(cutoff))
    with np.errstate(invalid="ignore"):
        near = pair & np.isfinite(d2) & (d2 <= C2)
    if exclude is not None:
        near &= np.asarray(query_exclude)[:, None] != np.asarray(exclude)[None, :]
    if self_graph and not include_self:
        near[np.arange(M), np.arange(M)] = False
    idx = np.full((Q, k), -1, dtype=np.int32)
    dist = np.full((Q, k), np.inf, dtype=np.float32)
    count = np.zeros(Q, dtype=np.int32)
    for q in range(Q):
        cand = np.flatnonzero(near[q])                                    # ascending j
        best = cand[np.argsort(d2[q, cand], kind="stable")][:k]           # stable: equal d2 keep the lower j first
        count[q] = best.size
        idx[q, :best.size] = best
        dist[q, :best.size] = np.sqrt(d2[q, best]).astype(np.float32)
    return Knn(idx, dist, count, np.where(pair, d2, np.nan))


def batch(points, k, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None, **kw):
    """[Knn] per structure of (B,M,3), (B,M), ..."""
    pick = lambda t, b: None if t is None else t[b]   # noqa: E731
    return [knn(points[b], k, pick(mask, b), pick(queries, b), pick(query_mask, b), pick(exclude, b),
                pick(query_exclude, b), **kw) for b in range(points.shape[0])]


def first(ref: Knn, k) -> Knn:
    """The result for a smaller ``k`` from one for a larger: the lists are sorted, so it is their first k entries."""
    assert k <= ref.idx.shape[1]
    return Knn(ref.idx[:, :k], ref.dist[:, :k], np.minimum(ref.count, k).astype(np.int32), ref.d2)


def boundary_ties(ref: Knn, k) -> int:
    """How many rows of a self graph WITHOUT its own point have, among all their candidates, an exact tie across the k
    boundary: the k-th and the (k+1)-th nearest at equal d2, so that only the index decides who is kept."""
    rows = 0
    for q in range(ref.d2.shape[0]):
        d = np.sort(np.delete(ref.d2[q], q))
        d = d[np.isfinite(d)]
        rows += int(d.size > k and d[k - 1] == d[k])
    return rows


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    x: np.ndarray        # (3,M,3) float32
    mask: np.ndarray     # (3,M) bool


def chain_case(M, seed, masked=0.45) -> Case:
    """Three structures of M points on compact random chains (``sasa_ref.chain_atoms``): in structure 0 a fraction
    ``masked`` of the points is masked with NaN coordinates under the mask, structure 1 is all padding (masked, NaN),
    structure 2 is complete."""
    rng = np.random.default_rng(seed)
    x = np.full((3, M, 3), np.nan, dtype=np.float32)
    mask = np.zeros((3, M), dtype=bool)
    for b in (0, 2):
        atoms, _ = sasa_ref.chain_atoms(M, rng)
        ok = rng.random(M) >= masked if b == 0 and M > 2 else np.ones(M, dtype=bool)
        mask[b] = ok
        x[b] = np.where(ok[:, None], atoms.astype(np.float32), np.nan)
    return Case(x, mask)


def cloud(M, seed, spread=12.0):
    """(M,3) float32: a Gaussian cloud, for queries and for atoms around residues"""
    return (np.random.default_rng(seed).normal(size=(M, 3)) * spread).astype(np.float32)


def lattice(n=6):
    """(n^3, 3) float32: the integer lattice {0 .. n-1}^3, x slowest.  Every squared distance is a small integer, exact
    in any precision, so equal distances are exactly equal."""
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
