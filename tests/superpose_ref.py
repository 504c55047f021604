"""Yardstick of the superposition kernels (csrc/superpose.hip, K37 - K40): a float64 numpy restatement of the definitions
of include/protstruc_superpose.h -- the weighted fit with its RMSD, the seed table, the seeded search under TM and count
objectives, ``tm_d0`` -- and the builders of the cases the tests use.  Inputs are float32 values widened to float64;
nothing here imports the package under test.  The 3x3 solve is numpy's SVD (as tests/align_ref.py), not the kernels' Jacobi.

The definition leaves the order of the sums over points open.  ``search(..., reverse=True)`` takes them over the points in
descending order; a case whose scores or winning seeds depend on that is on a knife edge and is not used
(tests/test_superpose_host.py holds every search case of the GPU tests to that)."""
from collections import namedtuple

import numpy as np

from tests import align_ref

TM, COUNT = 0, 1
MAX_POINTS, MAX_SEEDS, MAX_ITERATIONS, MAX_DOUBLINGS, MAX_OBJECTIVES = 2048, 1024, 20, 64, 8
SIX = ((TM, None), (COUNT, 0.5), (COUNT, 1.0), (COUNT, 2.0), (COUNT, 4.0), (COUNT, 8.0))   # None: tm_d0 of l_norm
SEARCH_SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 130, 257)

Fit = namedtuple("Fit", "R t rmsd wsum")
Search = namedtuple("Search", "score R t seed S")


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def tm_d0(length):
    """d0 of the TM-score for a target of ``length`` residues: 1.24 cbrt(L - 15) - 1.8 above 21 residues, else 0.5; never
    below 0.5."""
    length = float(length)
    return max(0.5, 1.24 * np.cbrt(length - 15.0) - 1.8) if length > 21 else 0.5


def six_objectives(l_norm):
    """the six objectives of ``superposition_scores`` for one normalisation length, params as the float32 the launch gets"""
    return [(kind, float(np.float32(tm_d0(l_norm) if param is None else param))) for kind, param in SIX]


# ---- the seed table -----------------------------------------------------------------------------------------------------------
def seed_table(n):
    """[(start, length)] of the seeds of n points, in seed order."""
    if n <= 0:
        return []
    lengths = []
    if n < 4:
        lengths = [n]
    else:
        k = 0
        while True:
            L = max(n >> k, 4)
            if not lengths or L != lengths[-1]:
                lengths.append(L)
            if L == 4:
                break
            k += 1
    strides = [max(L // 2, 1) for L in lengths]

    def starts(L, h):
        return list(range(0, n - L, h)) + [n - L]

    def total():
        return sum(len(starts(L, h)) for L, h in zip(lengths, strides))

    while total() > MAX_SEEDS:
        for j in reversed(range(len(lengths))):
            strides[j] *= 2
            if total() <= MAX_SEEDS:
                break
    return [(s, L) for L, h in zip(lengths, strides) for s in starts(L, h)]


# ---- fits ---------------------------------------------------------------------------------------------------------------------
def _total(x, reverse=False):
    """the sum over axis 0, over the points ascending or descending"""
    return np.add.reduce(x[::-1] if reverse else x, axis=0)


def _solve(H):
    U, s, Vt = np.linalg.svd(H)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    return V @ np.diag([1.0, 1.0, d]) @ U.T


def fit(a, b, w=None, reverse=False):
    """(R, t) of the weighted Kabsch fit of a (n,3) onto b (n,3), float64; unit weights where ``w`` is None"""
    w = np.ones(a.shape[0]) if w is None else w
    W = _total(w, reverse)
    ca, cb = _total(w[:, None] * a, reverse) / W, _total(w[:, None] * b, reverse) / W
    H = _total(w[:, None, None] * ((a - ca)[:, :, None] * (b - cb)[:, None, :]), reverse)
    R = _solve(H)
    return R, cb - R @ ca


def dist2(R, t, a, b):
    """d_i^2 in the header's order of operations"""
    x = ((R[None, :, 0] * a[:, 0:1] + R[None, :, 1] * a[:, 1:2]) + R[None, :, 2] * a[:, 2:3]) + t[None, :]
    e = x - b
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def superpose(a, b, weight=None, mask=None):
    """Fit(R, t, rmsd, wsum) of K37 for one structure: a, b (M,3), weight (M,) or None, mask (M,) or None.  No point with
    a positive weight: R, t, rmsd NaN and wsum 0."""
    a, b = align_ref.f64(a).reshape(-1, 3), align_ref.f64(b).reshape(-1, 3)
    w = np.ones(a.shape[0]) if weight is None else align_ref.f64(weight).reshape(-1).copy()
    w[~(w > 0)] = 0.0
    if mask is not None:
        w[np.asarray(mask).reshape(-1) == 0] = 0.0
    keep = w > 0
    if not keep.any():
        return Fit(np.full((3, 3), np.nan), np.full(3, np.nan), np.nan, 0.0)
    a, b, w = a[keep], b[keep], w[keep]
    R, t = fit(a, b, w)
    return Fit(R, t, float(np.sqrt((w * dist2(R, t, a, b)).sum() / w.sum())), float(w.sum()))


def superpose_grad(a, b, weight=None, mask=None, g=1.0):
    """(grad_a, grad_b, terms) of K38 for one structure from the closed form at the float64 fit; ``terms`` is, per element
    of grad_a, the sum of the absolute values of the terms of its residual, scaled like the gradient: what a relative
    error of the double arithmetic multiplies."""
    a64, b64 = align_ref.f64(a).reshape(-1, 3), align_ref.f64(b).reshape(-1, 3)
    f = superpose(a, b, weight, mask)
    w = np.ones(a64.shape[0]) if weight is None else align_ref.f64(weight).reshape(-1).copy()
    w[~(w > 0)] = 0.0
    if mask is not None:
        w[np.asarray(mask).reshape(-1) == 0] = 0.0
    ga, gb, terms = np.zeros_like(a64), np.zeros_like(a64), np.zeros_like(a64)
    keep = w > 0
    if not keep.any() or not f.rmsd > 0:
        return ga, gb, terms
    e = a64[keep] @ f.R.T + f.t - b64[keep]
    size = np.abs(a64[keep]) @ np.abs(f.R).T + np.abs(f.t) + np.abs(b64[keep])
    coef = (g * w[keep] / (f.wsum * f.rmsd))[:, None]
    ga[keep], gb[keep] = coef * (e @ f.R), -coef * e
    terms[keep] = np.abs(coef) * (size @ np.abs(f.R))
    return ga, gb, terms


# ---- the search ---------------------------------------------------------------------------------------------------------------
def _objective(kind, param):
    p = float(np.float32(param))
    if kind == TM:
        ds = min(8.0, max(4.5, p))
        return p * p, ds - 1.0, ds + 1.0
    return p * p, p, p


def terms(kind, p2, d2):
    return 1.0 / (1.0 + d2 / p2) if kind == TM else (d2 <= p2).astype(np.float64)


def chain(a, b, start, length, kind, param, reverse=False):
    """(S, R, t) of one chain over the n compacted points a, b (n,3) float64"""
    n = a.shape[0]
    p2, r1, r = _objective(kind, param)
    need = min(3, n)
    previous = np.zeros(n, dtype=bool)
    previous[start:start + length] = True
    R, t = fit(a[previous], b[previous], None, reverse)
    best = (-np.inf, R, t)
    for it in range(MAX_ITERATIONS):
        d2 = dist2(R, t, a, b)
        S = float(_total(terms(kind, p2, d2), reverse))
        if S > best[0]:
            best = (S, R, t)
        rr = r1 if it == 0 else r
        sel = d2 < rr * rr
        for _ in range(MAX_DOUBLINGS):
            if sel.sum() >= need:
                break
            rr = 2.0 * rr
            sel = d2 < rr * rr
        if sel.sum() < need:
            sel = np.ones(n, dtype=bool)
        if np.array_equal(sel, previous):
            break
        previous = sel
        R, t = fit(a[sel], b[sel], None, reverse)
    return best


def search(a, b, mask, l_norm, objectives, reverse=False):
    """Search(score, R, t, seed, S) of K39 / K40 for one structure: a, b (M,3), mask (M,) or None, objectives a list of
    (kind, param); score (n_obj,) float64 -- S / l_norm, not yet rounded to float --, R (n_obj,3,3), t (n_obj,3), the
    winning seed and its S per objective."""
    a, b = align_ref.f64(a).reshape(-1, 3), align_ref.f64(b).reshape(-1, 3)
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        a, b = a[keep], b[keep]
    n_obj = len(objectives)
    out = Search(np.zeros(n_obj), np.full((n_obj, 3, 3), np.nan), np.full((n_obj, 3), np.nan), np.full(n_obj, -1), np.zeros(n_obj))
    seeds = seed_table(a.shape[0])
    for o, (kind, param) in enumerate(objectives):
        best = -np.inf
        for s, (start, length) in enumerate(seeds):
            S, R, t = chain(a, b, start, length, kind, param, reverse)
            if S > best:
                best = S
                out.R[o], out.t[o], out.seed[o], out.S[o] = R, t, s, S
        if seeds:
            out.score[o] = best / float(l_norm)
    return out


def score_at(R, t, a, b, mask, l_norm, kind, param):
    """the objective's score under a given transform: what the returned (R, t) must reproduce"""
    a, b = align_ref.f64(a).reshape(-1, 3), align_ref.f64(b).reshape(-1, 3)
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        a, b = a[keep], b[keep]
    p2 = _objective(kind, param)[0]
    return float(terms(kind, p2, dist2(align_ref.f64(R), align_ref.f64(t), a, b)).sum() / float(l_norm))


def gdt_from(scores, cutoffs, wanted):
    """the mean of the count scores of ``wanted`` cutoffs out of the ``scores`` of ``cutoffs``"""
    return float(np.mean([scores[list(cutoffs).index(c)] for c in wanted]))


# ---- case builders ------------------------------------------------------------------------------------------------------------
def model_and_target(n, seed):
    """A compact cloud a (n,3) and a target b: a moved rigidly, every point displaced by noise whose size runs from 0.2 A
    to 6 A along the chain, so that every cutoff from 0.5 A to 8 A and the TM term tell some points from others."""
    rng = np.random.default_rng(seed)
    a = 2.5 * max(n, 1) ** (1 / 3) * rng.standard_normal((n, 3))
    sigma = np.geomspace(0.2, 6.0, max(n, 1))[rng.permutation(n)] if n else np.zeros(0)
    b = a @ align_ref.rotation(rng).T + rng.uniform(-10, 10, 3) + sigma[:, None] * rng.standard_normal((n, 3))
    return f32(a), f32(b)


def scatter(a, b, masked=0.45, seed=0):
    """(a (M,3), b (M,3), mask (M,)): the n pairs in order among M = round(n / (1 - masked)) slots, the others masked
    and NaN in both arrays"""
    n = a.shape[0]
    M = max(int(round(n / (1.0 - masked))), n, 1)
    rng = np.random.default_rng(seed + 7919)
    mask = np.zeros(M, dtype=bool)
    mask[np.sort(rng.choice(M, n, replace=False))] = True
    A, Bt = np.full((M, 3), np.nan, np.float32), np.full((M, 3), np.nan, np.float32)
    A[mask], Bt[mask] = a, b
    return A, Bt, mask


def search_case(n, seed=0):
    """(a, b, mask, l_norm, objectives) of the search case with n points after masking"""
    a, b, mask = scatter(*model_and_target(n, 300 + 17 * n + seed), seed=n + seed)
    l_norm = float(max(n, 1))
    return a, b, mask, l_norm, six_objectives(l_norm)


def two_domains(n=130, first=78, angle=40.0, noise=0.05, seed=5):
    """A chain of n points whose first ``first`` points are moved by one rigid motion and the rest by another, ``angle``
    degrees away, plus ``noise`` A on every point: (a, b) float32"""
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.standard_normal((n, 3)) * 2.2, axis=0)
    Q = align_ref.rotation(rng)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    th = np.deg2rad(angle)
    Q2 = (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)) @ Q
    b = np.concatenate([a[:first] @ Q.T + np.array([3.0, -2.0, 5.0]), a[first:] @ Q2.T + np.array([-4.0, 6.0, 1.0])])
    return f32(a), f32(b + noise * rng.standard_normal((n, 3)))


def perturbed_model(xyz, atom_mask, seed, sigma=0.5, removed=0.1, ca=1):
    """(model xyz float32, model atom mask) of a target (N,A,3) / (N,A): every coordinate moved by ``sigma`` A of noise and
    the CA of a tenth of the residues that have one taken out of the model's mask"""
    rng = np.random.default_rng(seed)
    xyz, atom_mask = np.asarray(xyz, dtype=np.float32), np.asarray(atom_mask).astype(bool).copy()
    model = f32(xyz + sigma * rng.standard_normal(xyz.shape))
    have = np.flatnonzero(atom_mask[:, ca])
    atom_mask[rng.choice(have, int(round(removed * have.size)), replace=False), ca] = False
    return model, atom_mask


def structure_case(xyz, atom_mask, seed, ca=1):
    """the search case of a StructureBatch method: the model of ``perturbed_model`` against the target, CA atoms, the pairs
    those present in both, l_norm the target's CA count: (a, b, mask, l_norm, objectives)"""
    model, model_mask = perturbed_model(xyz, atom_mask, seed)
    target_mask = np.asarray(atom_mask).astype(bool)
    l_norm = float(target_mask[:, ca].sum())
    return model[:, ca], f32(np.asarray(xyz)[:, ca]), model_mask[:, ca] & target_mask[:, ca], l_norm, six_objectives(l_norm)


CONTRACT_M = 35


def contract_case(variant, structure):
    """structure 0 / 1 of variant "A" / "B" of the launch-contract case: 19 points among CONTRACT_M slots"""
    a, b, mask = scatter(*model_and_target(19, 900 + 10 * "AB".index(variant) + structure), seed=40 + structure)
    assert a.shape[0] == CONTRACT_M
    return a, b, mask, 19.0, six_objectives(19.0)


def batch_limit_case(structure):
    """one of the three structures of the batch-limit case: M = 5, the second with one point masked over NaN"""
    a, b = model_and_target(5, 950 + structure)
    mask = np.ones(5, dtype=bool)
    if structure == 1:
        mask[2] = False
        a[2], b[2] = np.nan, np.nan
    return a, b, mask, 5.0, six_objectives(5.0)


def search_cases():
    """name -> (a (M,3), b (M,3), mask (M,) or None, l_norm, objectives): every search case the GPU tests run, the ones made
    from PDB files excepted (the test files build those with ``structure_case``)"""
    cases = {f"n={n}": search_case(n) for n in SEARCH_SIZES}
    a, b = two_domains()
    cases["two domains"] = (a, b, None, 130.0, six_objectives(130.0))
    a, _ = model_and_target(40, 77)
    cases["identical"] = (a, a.copy(), None, 40.0, six_objectives(40.0))
    a, b, mask, _, _ = search_case(65, seed=1)
    cases["l_norm above n"] = (a, b, mask, 100.0, six_objectives(100.0))
    wide = scatter(*model_and_target(50, 78), masked=1.0 - 50 / 2048.0, seed=3)
    assert wide[0].shape[0] == MAX_POINTS
    cases["M=2048"] = (*wide, 50.0, six_objectives(50.0))
    for v in "AB":
        for s in (0, 1):
            cases[f"contract {v}{s}"] = contract_case(v, s)
    for s in range(3):
        cases[f"batch limit {s}"] = batch_limit_case(s)
    return cases
