"""Float64 numpy restatements for the ensemble kernels (K45, K46; include/protstruc_ensemble.h), and the inputs that the
host tests and the GPU tests share.  Not a test module.

``pairwise_rmsd`` is the yardstick of K45 and does NOT use the header's formula: centroids, an SVD Kabsch fit with the
determinant fix, and then a pass of its own over the residuals ``R x - y``.  ``formula`` is the header's formula, evaluated
in float64 with the sums taken one point after the other, forwards or backwards: tests/test_ensemble_host.py holds it to
``bound`` against the yardstick on every input the GPU tests use, so that those inputs are shown to lie inside the bound by
arithmetic alone.  ``cluster_plain`` is the clustering rule written the plain way from the active set and ``D``;
``cluster`` keeps the degrees up to date instead of counting them again every round (the same results, checked on the
host), which is what makes B = 4096 singletons affordable."""
import functools
from typing import NamedTuple

import numpy as np


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- K45: the yardstick ----------------------------------------------------------------------------------------------------------
def _masks(a, b, mask_a, mask_b):
    """(b, mask_a (Ba,M), mask_b (Bb,M)) with a shared (M,) mask spread over its batch and None as all-true"""
    b = a if b is None else b
    mask_b = mask_a if (mask_b is None and b is a) else mask_b
    out = []
    for x, m in ((a, mask_a), (b, mask_b)):
        m = np.ones(x.shape[:2], dtype=bool) if m is None else np.asarray(m) != 0
        out.append(np.broadcast_to(m, x.shape[:2]))
    return b, out[0], out[1]


def pairwise_rmsd(a, b=None, mask_a=None, mask_b=None):
    """(rmsd (Ba,Bb) float64, count (Ba,Bb) int64): per pair over the points both masks count -- centroids, the SVD Kabsch fit
    with the determinant fix, a pass over the residuals.  NaN where no point is common or a common coordinate is not finite.
    ``b`` None compares ``a`` with itself (every entry computed like any other: the diagonal is the rounding of a fit)."""
    b, ma, mb = _masks(a, b, mask_a, mask_b)
    W = ma[:, None, :] & mb[None, :, :]                                   # (Ba,Bb,M)
    n = W.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        X = np.where(W[..., None], a.astype(np.float64)[:, None], 0.0)   # (Ba,Bb,M,3)
        Y = np.where(W[..., None], b.astype(np.float64)[None, :], 0.0)
        broken = ~(np.isfinite(X).all((-1, -2)) & np.isfinite(Y).all((-1, -2)))
        X, Y = np.nan_to_num(X, posinf=0.0, neginf=0.0), np.nan_to_num(Y, posinf=0.0, neginf=0.0)
        nn = np.maximum(n, 1)[..., None, None]
        Xc = np.where(W[..., None], X - X.sum(2, keepdims=True) / nn, 0.0)
        Yc = np.where(W[..., None], Y - Y.sum(2, keepdims=True) / nn, 0.0)
        H = np.einsum("ijpc,ijpd->ijcd", Xc, Yc)
        U, _, Vt = np.linalg.svd(H)
        V = np.swapaxes(Vt, -1, -2)
        d = np.sign(np.linalg.det(V @ np.swapaxes(U, -1, -2)))
        d[d == 0] = 1.0
        V = V.copy()
        V[..., :, 2] *= d[..., None]
        R = V @ np.swapaxes(U, -1, -2)                                    # R x ~ y
        E = np.einsum("ijdc,ijpc->ijpd", R, Xc) - Yc
        rmsd = np.sqrt((E ** 2).sum((-1, -2)) / n)
    rmsd[(n == 0) | broken] = np.nan
    return rmsd, n.astype(np.int64)


# ---- K45: the header's formula ---------------------------------------------------------------------------------------------------
class Formula(NamedTuple):
    rmsd: np.ndarray     # (Ba,Bb) float64
    n: np.ndarray        # (Ba,Bb)
    E: np.ndarray        # (Ba,Bb): (Qx + Qy) / n about the origins of the header


def origins(x, m):
    """(B,3) float64: every structure's own lowest-index counted point (0 where it counts none)"""
    first = np.argmax(m, axis=1)
    o = x.astype(np.float64)[np.arange(x.shape[0]), first]
    return np.where(m.any(1)[:, None], o, 0.0)


def formula(a, b=None, mask_a=None, mask_b=None, reverse=False) -> Formula:
    """The formula of include/protstruc_ensemble.h in float64, the sums taken one point after the other (``reverse``: from
    the last point to the first); the trace of the solve is ``s0 + s1 + sign(det H) s2`` from numpy's singular values."""
    b, ma, mb = _masks(a, b, mask_a, mask_b)
    Ba, Bb, M = a.shape[0], b.shape[0], a.shape[1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = np.where(ma[..., None], a.astype(np.float64) - origins(a, ma)[:, None], 0.0)
        y = np.where(mb[..., None], b.astype(np.float64) - origins(b, mb)[:, None], 0.0)
        qx, qy = (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2], (y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1]) + y[..., 2] * y[..., 2]
        Sxy, Sx, Sy = np.zeros((Ba, Bb, 3, 3)), np.zeros((Ba, Bb, 3)), np.zeros((Ba, Bb, 3))
        Qx, Qy, n = np.zeros((Ba, Bb)), np.zeros((Ba, Bb)), np.zeros((Ba, Bb))
        for p in (range(M - 1, -1, -1) if reverse else range(M)):
            w = (ma[:, None, p] & mb[None, :, p]).astype(np.float64)
            xp, yp = x[:, None, p, :], y[None, :, p, :]
            Sxy += w[..., None, None] * (xp[..., :, None] * yp[..., None, :])
            Sx += w[..., None] * xp
            Sy += w[..., None] * yp
            Qx += w * qx[:, None, p]
            Qy += w * qy[None, :, p]
            n += w
        H = Sxy - (Sx[..., :, None] * Sy[..., None, :]) / n[..., None, None]
        gx = Qx - ((Sx[..., 0] * Sx[..., 0] + Sx[..., 1] * Sx[..., 1]) + Sx[..., 2] * Sx[..., 2]) / n
        gy = Qy - ((Sy[..., 0] * Sy[..., 0] + Sy[..., 1] * Sy[..., 1]) + Sy[..., 2] * Sy[..., 2]) / n
        ok = np.isfinite(H).all((-1, -2)) & (n > 0)
        s = np.linalg.svd(np.where(ok[..., None, None], H, 0.0), compute_uv=False)
        sign = np.where(np.linalg.det(np.where(ok[..., None, None], H, 0.0)) < 0, -1.0, 1.0)
        tr = s[..., 0] + s[..., 1] + sign * s[..., 2]
        rmsd = np.sqrt(np.maximum(0.0, ((gx + gy) - 2.0 * tr) / n))
        rmsd[~ok] = np.nan
        return Formula(rmsd, n.astype(np.int64), (Qx + Qy) / n)


def bound(ref, n, E):
    """the bound of the header, elementwise: 2^-23 ref + min(sqrt(delta), delta / ref), delta = (4 (n + 8) 2^-53 + 2^-45) E"""
    delta = (4.0 * (n + 8.0) * 2.0 ** -53 + 2.0 ** -45) * E
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 ** -23 * ref + np.minimum(np.sqrt(delta), np.where(ref > 0, delta / ref, np.inf))


def fraction_of_bound(error, limit):
    """error / limit elementwise; where the bound is 0 (one point: both sides are exactly 0) 0 for no error, else inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(limit > 0, error / limit, np.where(error == 0, 0.0, np.inf))


# ---- K45: the inputs -------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1, 1), (2, 3, 2), (3, 2, 3), (15, 17, 4), (16, 16, 63), (17, 33, 64), (33, 15, 65), (65, 2, 130), (3, 65, 257),
          (16, 1, 257), (65, 65, 3), (33, 33, 130))            # (Ba, Bb, M)
MASK_KINDS = ("none", "shared", "own")
FAMILIES = ("copy", "noise 1e-3", "noise 0.5", "noise 5", "mirror", "collinear", "noise 0.5 again")
OFFSET_SHAPES = ((15, 17, 4), (17, 33, 64), (3, 65, 257))      # everything moved by 1000 A in these


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def members(base, B, rng, first=0):
    """(B,M,3) float32: member k is the family FAMILIES[(first + k) % 7] of ``base`` under a random rigid motion"""
    M = base.shape[0]
    out = np.empty((B, M, 3))
    for k in range(B):
        kind = (first + k) % len(FAMILIES)
        pts = base.copy()
        if kind in (1, 2, 3, 6):
            pts = pts + rng.normal(scale=(1e-3, 0.5, 5.0, 0.5)[(1, 2, 3, 6).index(kind)], size=pts.shape)
        elif kind == 4:
            pts = pts * np.array([-1.0, 1.0, 1.0])
        elif kind == 5:
            pts = np.outer(np.linspace(-1.0, 1.0, M) * 3.8 * M / 2 + rng.normal(scale=0.1, size=M), rng.normal(size=3))
        out[k] = pts @ rotation(rng).T + rng.uniform(-20.0, 20.0, 3)
    return out


@functools.lru_cache(maxsize=None)
def rmsd_case(Ba, Bb, M, mask_kind):
    """(a (Ba,M,3), b (Bb,M,3), mask_a, mask_b) float32 / bool: the members of one cloud of M points the size of a protein
    of M residues, in the seven families; ``mask_kind`` "none", "shared" -- one (M,) mask for both sides -- or "own" --
    per-structure masks that leave out 45 % of the points, NaN in their place, with (where the batch is large enough) one
    structure of a that counts nothing and structures of b that count two points and one point"""
    rng = np.random.default_rng(100000 * Ba + 1000 * Bb + M + 7 * MASK_KINDS.index(mask_kind))
    base = rng.normal(size=(M, 3)) * 2.2 * max(M, 2) ** (1.0 / 3.0) + rng.uniform(-30, 30, 3)
    shift = 1000.0 if (Ba, Bb, M) in OFFSET_SHAPES else 0.0
    a, b = f32(members(base, Ba, rng) + shift), f32(members(base, Bb, rng, first=2) + shift)
    if mask_kind == "none":
        return a, b, None, None
    if mask_kind == "shared":
        m = rng.random(M) < 0.7
        m[rng.integers(M)] = True
        return a, b, m, m
    ma, mb = rng.random((Ba, M)) < 0.55, rng.random((Bb, M)) < 0.55
    ma[np.arange(Ba), rng.integers(M, size=Ba)] = True
    mb[np.arange(Bb), rng.integers(M, size=Bb)] = True
    if Ba >= 3:
        ma[1] = False
    if Bb >= 5 and M >= 3:
        mb[2], mb[3] = False, False
        mb[2, [0, M - 1]] = True
        mb[3, M // 2] = True
    a, b = a.copy(), b.copy()
    a[~ma], b[~mb] = np.nan, np.nan
    return a, b, ma, mb


def all_rmsd_cases():
    return [(Ba, Bb, M, kind) for Ba, Bb, M in SHAPES for kind in MASK_KINDS]


def contract_case(variant):
    """the inputs of the launch-contract cases, two seeded variants: a (5,37,3), b (4,37,3) and their own masks"""
    rng = np.random.default_rng(900 + "AB".index(variant))
    base = rng.normal(size=(37, 3)) * 7.0
    a, b = f32(members(base, 5, rng, first=1)), f32(members(base, 4, rng, first=2))
    ma, mb = rng.random((5, 37)) < 0.8, rng.random((4, 37)) < 0.8
    return a, b, ma, mb


def limit_case():
    """the three structures that the batch-limit tests repeat: a (3,4,3), b (3,4,3); and three of M = 3 for self mode"""
    rng = np.random.default_rng(77)
    base = rng.normal(size=(4, 3)) * 4.0
    return f32(members(base, 3, rng, first=1)), f32(members(base, 3, rng, first=2)), f32(members(base[:3], 3, rng, first=1))


# ---- K46 -------------------------------------------------------------------------------------------------------------------------
class Clusters(NamedTuple):
    label: np.ndarray        # (B,) int32, -1 where invalid
    center: np.ndarray       # (B,) int32 by cluster number, -1 past the last
    size: np.ndarray         # (B,) int32, 0 past the last
    n_clusters: int


def adjacency(D, cutoff):
    with np.errstate(invalid="ignore"):
        upper = np.triu(D <= np.float32(cutoff), 1)
    return upper | upper.T


def cluster_plain(D, cutoff, valid=None) -> Clusters:
    """one matrix (B,B), the plain way: the degrees are counted again from the active set in every round"""
    B = D.shape[0]
    adj = adjacency(D, cutoff)
    active = np.ones(B, dtype=bool) if valid is None else np.asarray(valid) != 0
    label, center, size = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.zeros(B, np.int32)
    c = 0
    while active.any():
        deg = (adj & active[None, :]).sum(1)
        deg[~active] = -1
        centre = int(np.argmax(deg))                 # the first of the greatest: the lowest index on ties
        chosen = active & adj[centre]
        chosen[centre] = True
        label[chosen], center[c], size[c] = c, centre, chosen.sum()
        active = active & ~chosen
        c += 1
    return Clusters(label, center, size, c)


def cluster(D, cutoff, valid=None) -> Clusters:
    """the same rule with the degrees kept up to date: every removed member lowers its neighbours' degrees by one"""
    B = D.shape[0]
    adj = adjacency(D, cutoff)
    active = np.ones(B, dtype=bool) if valid is None else (np.asarray(valid) != 0).copy()
    deg = (adj & active[None, :]).sum(1).astype(np.int64)
    deg[~active] = -1
    label, center, size = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.zeros(B, np.int32)
    c = 0
    while True:
        centre = int(np.argmax(deg))
        if deg[centre] < 0:
            break
        chosen = np.flatnonzero(active & adj[centre])
        chosen = np.union1d(chosen, [centre])
        label[chosen], center[c], size[c] = c, centre, chosen.size
        active[chosen] = False
        deg -= adj[:, chosen].sum(1)
        deg[~active] = -1
        c += 1
    return Clusters(label, center, size, c)


def lattice_distances(B, rng):
    """(B,B) float32: the distances between B points of an integer lattice in the plane, in a random order -- 3-4-5 and its
    like make many of them exactly integers, and whole rows have the same degree"""
    side = int(np.ceil(np.sqrt(B)))
    pts = np.stack(np.divmod(np.arange(side * side), side), 1)[rng.permutation(side * side)[:B]].astype(np.int32)
    dx, dy = pts[:, None, 0] - pts[None, :, 0], pts[:, None, 1] - pts[None, :, 1]
    return f32(np.sqrt((dx * dx + dy * dy).astype(np.float64)))


CLUSTER_FAMILIES = ("lattice", "one cluster", "singletons", "path", "invalid", "nan", "asymmetric")
CLUSTER_SIZES = (1, 2, 63, 64, 65, 1000, 4096)
LARGE_FAMILIES = CLUSTER_FAMILIES + ("mixed",)      # B = 1000 and 4096: every family, and lattice + invalid + nan + asymmetric in one


@functools.lru_cache(maxsize=4)
def cluster_case(family, B, G=3):
    """(D (G,B,B) float32, cutoff, valid (G,B) bool or None)"""
    rng = np.random.default_rng(1000 * B + len(family) + 31 * ord(family[0]))
    valid = None
    if family == "one cluster":
        return f32(rng.random((G, B, B))), 2.0, None
    if family == "singletons":
        return f32(1.0 + rng.random((G, B, B))), 0.5, None
    if family == "path":
        idx = np.arange(B, dtype=np.float64)
        D = f32(np.abs(idx[:, None] - idx[None, :]))
        return np.stack([D, D * 0.5, D * 2.0][:G] + [D] * max(0, G - 3)), 1.0, None      # paths, pairs of steps, nothing
    D = np.stack([lattice_distances(B, rng) for _ in range(G)])
    if family in ("invalid", "mixed"):
        valid = rng.random((G, B)) < 0.7
        D = np.where(valid[:, :, None] & valid[:, None, :], D, np.float32(np.nan))
    if family in ("nan", "mixed"):
        D = np.where(rng.random(D.shape) < 0.1, np.float32(np.nan), D)
    if family in ("asymmetric", "mixed"):
        lower = np.tril(np.ones((B, B), dtype=bool), 0)           # the diagonal too: it is never read
        D = np.where(lower[None], f32(rng.random(D.shape) * 10.0), D)
    return f32(D), 5.0, valid


def cluster_all(D, cutoff, valid=None, rule=cluster):
    """the four outputs of K46 for (G,B,B): label, center, size (G,B) int32 and n_clusters (G,) int32"""
    per = [rule(D[g], cutoff, None if valid is None else valid[g]) for g in range(D.shape[0])]
    B = D.shape[1]
    return (np.stack([p.label for p in per]).reshape(-1, B), np.stack([p.center for p in per]).reshape(-1, B),
            np.stack([p.size for p in per]).reshape(-1, B), np.array([p.n_clusters for p in per], np.int32))


# ---- StructureBatch: twelve members of one PDB file ------------------------------------------------------------------------------
def ensemble_of(xyz, atom_mask, seed=5):
    """(xyz (12,N,A,3) float32, atom_mask (12,N,A) bool, family (12,)): three families of four -- each family its own smooth
    3 A deformation of the structure, its members 0.3 A of noise apart --, every member under a random rigid motion, a
    tenth of the present atoms removed (NaN in their place)"""
    rng = np.random.default_rng(seed)
    N, A = atom_mask.shape
    x0 = np.nan_to_num(xyz.astype(np.float64))
    out, masks, family = [], [], []
    for f in range(3):
        # a deformation that varies slowly along the chain, 3 A in size
        phase, direction = rng.uniform(0, 2 * np.pi, 3), rng.normal(size=(3, 3))
        wave = sum(np.sin(2 * np.pi * (k + 1) * np.arange(N) / N + phase[k])[:, None] * direction[k] for k in range(3))
        wave *= 3.0 / np.sqrt((wave ** 2).sum(-1).mean())
        for _ in range(4):
            pts = x0 + wave[:, None, :] + rng.normal(scale=0.3 / np.sqrt(3.0), size=x0.shape)
            pts = pts @ rotation(rng).T + rng.uniform(-30, 30, 3)
            keep = atom_mask & (rng.random((N, A)) >= 0.1)
            pts[~keep] = np.nan
            out.append(f32(pts)), masks.append(keep), family.append(f)
    order = rng.permutation(12)
    return np.stack(out)[order], np.stack(masks)[order], np.array(family)[order]
