"""Yardstick of the structure-alignment kernels (csrc/struct_align.hip, K41 - K44): a float64 numpy restatement of the
definitions of include/protstruc_structalign.h -- the Needleman-Wunsch pass with TM-align's gap rule and its trace back,
TM-align's secondary structure of a CA trace, the threading start, the fit-search and the refinement that alternates
them -- and the builders of the cases the tests use.  Fits, chains, the seed table, ``dist2`` and ``tm_d0`` are those of
tests/superpose_ref.py; nothing here imports the package under test (the PDB files are read by a reader of its own).

The definition leaves the order of the sums over points open.  ``align(..., reverse=True)`` takes them over the points in
descending order; a case whose map, winning start or score depends on that is on a knife edge and is not used
(tests/test_structalign_host.py holds every alignment case of the GPU tests to that)."""
import functools
import os
from collections import namedtuple

import numpy as np

from tests import align_ref
from tests import superpose_ref as S

MAX_POINTS, MAX_ITERATIONS = 1024, 20
GAPS = (float(np.float32(-0.6)), 0.0)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Pass = namedtuple("Pass", "map n_aligned value")
Result = namedtuple("Result", "map n_aligned S score R t start n_a n_b passes")


# ---- the DP -------------------------------------------------------------------------------------------------------------------
def _tables(score, gap):
    """(val, path) of the recurrence, filled one anti-diagonal at a time: each cell's three additions and two comparisons
    are those of the definition"""
    na, nb = score.shape
    val, path = np.zeros((na + 1, nb + 1)), np.zeros((na + 1, nb + 1), dtype=bool)
    for s in range(2, na + nb + 1):
        i = np.arange(max(1, s - nb), min(na, s - 1) + 1)
        j = s - i
        d = val[i - 1, j - 1] + score[i - 1, j - 1]
        h = val[i - 1, j] + np.where(path[i - 1, j], gap, 0.0)
        v = val[i, j - 1] + np.where(path[i, j - 1], gap, 0.0)
        p = (d >= h) & (d >= v)
        val[i, j] = np.where(p, d, np.where(v >= h, v, h))
        path[i, j] = p
    return val, path


def _tables_cell_by_cell(score, gap):
    """the same tables by the plain double loop of the definition (the check of ``_tables``)"""
    na, nb = score.shape
    val, path = np.zeros((na + 1, nb + 1)), np.zeros((na + 1, nb + 1), dtype=bool)
    for i in range(1, na + 1):
        for j in range(1, nb + 1):
            d = val[i - 1, j - 1] + score[i - 1, j - 1]
            h = val[i - 1, j] + (gap if path[i - 1, j] else 0.0)
            v = val[i, j - 1] + (gap if path[i, j - 1] else 0.0)
            if d >= h and d >= v:
                path[i, j], val[i, j] = True, d
            else:
                path[i, j], val[i, j] = False, (v if v >= h else h)
    return val, path


def nw(score, gap, tables=_tables):
    """Pass(map (n_a,) of points of b or -1, n_aligned, value) of one DP over score (n_a, n_b) float64"""
    score = np.asarray(score, dtype=np.float64)
    na, nb = score.shape
    out = np.full(na, -1, dtype=np.int64)
    if na == 0 or nb == 0:
        return Pass(out, 0, 0.0)
    gap = float(gap)
    val, path = tables(score, gap)
    i, j = na, nb
    while i > 0 and j > 0:
        if path[i, j]:
            out[i - 1] = j - 1
            i, j = i - 1, j - 1
        else:
            h = val[i - 1, j] + (gap if path[i - 1, j] else 0.0)
            v = val[i, j - 1] + (gap if path[i, j - 1] else 0.0)
            if v >= h:
                j -= 1
            else:
                i -= 1
    return Pass(out, int((out >= 0).sum()), float(val[na, nb]))


def nw_slots(score, gap, mask_a=None, mask_b=None):
    """``nw`` on a (Ma, Mb) matrix with masks: Pass with the map over the Ma slots holding slots of b"""
    score = np.asarray(score)
    Ma, Mb = score.shape
    ia = np.arange(Ma) if mask_a is None else np.flatnonzero(np.asarray(mask_a) != 0)
    ib = np.arange(Mb) if mask_b is None else np.flatnonzero(np.asarray(mask_b) != 0)
    got = nw(score[np.ix_(ia, ib)].astype(np.float64), gap)
    out = np.full(Ma, -1, dtype=np.int64)
    hit = got.map >= 0
    out[ia[hit]] = ib[got.map[hit]]
    return Pass(out, got.n_aligned, got.value)


def path_value(score, gap, pairs):
    """what the gap rule pays for an alignment given as increasing (i, j) pairs: the scores of the pairs, plus the gap for
    every pair that is not directly followed by the pair (i + 1, j + 1) unless it is the last cell of the table"""
    na, nb = score.shape
    total = 0.0
    for k, (i, j) in enumerate(pairs):
        total += score[i, j]
        follows = pairs[k + 1] if k + 1 < len(pairs) else (na, nb)
        if follows != (i + 1, j + 1):
            total += gap
    return total


def all_alignments(na, nb):
    """every strictly increasing partial matching of range(na) with range(nb), as lists of pairs"""
    def extend(i0, j0):
        yield []
        for i in range(i0, na):
            for j in range(j0, nb):
                for rest in extend(i + 1, j + 1):
                    yield [(i, j)] + rest
    return list(extend(0, 0))


# ---- the secondary structure --------------------------------------------------------------------------------------------------
def _dist(x, i, j):
    e = x[i] - x[j]
    return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def secondary_structure(x, mask=None):
    """labels (M,) int8 of a CA trace x (M,3): -1 under the mask"""
    x = align_ref.f64(x).reshape(-1, 3)
    M = x.shape[0]
    slots = np.arange(M) if mask is None else np.flatnonzero(np.asarray(mask) != 0)
    p, n = x[slots], slots.size
    out = np.full(M, -1, dtype=np.int8)
    for i in range(n):
        label = 0
        if 2 <= i <= n - 3:
            d13, d14, d15 = _dist(p, i - 2, i), _dist(p, i - 2, i + 1), _dist(p, i - 2, i + 2)
            d24, d25, d35 = _dist(p, i - 1, i + 1), _dist(p, i - 1, i + 2), _dist(p, i, i + 2)
            six = np.array([d15, d14, d25, d13, d24, d35])
            if (np.abs(six - np.array([6.37, 5.18, 5.18, 5.45, 5.45, 5.45])) < 2.1).all():
                label = 1
            elif (np.abs(six - np.array([13.0, 10.4, 10.4, 6.1, 6.1, 6.1])) < 1.42).all():
                label = 2
            elif d15 < 8.0:
                label = 3
        out[slots[i]] = label
    return out


# ---- the alignment ------------------------------------------------------------------------------------------------------------
def tm_terms(d2, d0):
    return 1.0 / (1.0 + d2 / (d0 * d0))


def fit_search(a, b, m, d0, reverse=False):
    """(S, R, t) of the fit-search over the pairs of map m (points of b per point of a, -1 for none); at least one pair"""
    idx = np.flatnonzero(m >= 0)
    A, Bm = a[idx], b[m[idx]]
    n = idx.size
    seeds = S.seed_table(n)
    if n >= 4:
        seeds = [(s, L) for s, L in seeds if L >= max(n >> 1, 4)]
    best = (-np.inf, None, None)
    for start, length in seeds:
        found = S.chain(A, Bm, start, length, S.TM, d0, reverse)
        if found[0] > best[0]:
            best = found
    return best


def threading(a, b, d0, reverse=False):
    """(map, S_k, k) of the best gapless threading"""
    na, nb = a.shape[0], b.shape[0]
    need = max(min(na, nb) // 2, min(5, na, nb))
    best, best_k = -np.inf, None
    for k in range(-(na - need), nb - need + 1):
        i0, i1 = max(0, -k), min(na, nb - k)
        A, Bm = a[i0:i1], b[i0 + k:i1 + k]
        R, t = S.fit(A, Bm, None, reverse)
        Sk = float(S._total(tm_terms(S.dist2(R, t, A, Bm), d0), reverse))
        if Sk > best:
            best, best_k = Sk, k
    m = np.full(na, -1, dtype=np.int64)
    i0, i1 = max(0, -best_k), min(na, nb - best_k)
    m[i0:i1] = np.arange(i0, i1) + best_k
    return m, best, best_k


def tm_matrix(R, t, a, b, d0):
    """s(d^2(T a_i, b_j)) for every i, j, d^2 in K39's order of operations"""
    x = ((R[None, :, 0] * a[:, 0:1] + R[None, :, 1] * a[:, 1:2]) + R[None, :, 2] * a[:, 2:3]) + t[None, :]
    e = x[:, None, :] - b[None, :, :]
    return tm_terms((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], d0)


def refine(a, b, m, d0, reverse=False):
    """(S, map, R, t, DP passes) of the refinement of start m"""
    Sm, R0, t0 = fit_search(a, b, m, d0, reverse)
    best, passes = (-np.inf, None, None, None), 0
    if Sm > best[0]:
        best = (Sm, m, R0, t0)
    for gap in GAPS:
        prev, R, t = m, R0, t0
        for _ in range(MAX_ITERATIONS):
            new = nw(tm_matrix(R, t, a, b, d0), gap).map
            passes += 1
            if not (new >= 0).any():
                break
            Sn, R, t = fit_search(a, b, new, d0, reverse)
            if Sn > best[0]:
                best = (Sn, new, R, t)
            if np.array_equal(new, prev):
                break
            prev = new
    return best + (passes,)


def align(a, b, mask_a=None, mask_b=None, d0=None, use_ss=True, reverse=False, starts=(0, 1)):
    """Result of the alignment of a (Ma,3) onto b (Mb,3) float32: the map over the Ma slots (slots of b), S and score =
    S / min(n_a, n_b) in float64 (not yet rounded to float).  ``d0`` None: float32(tm_d0(min(n_a, n_b))).  ``starts``
    restricts the starts that are tried (the tests compare the threading start alone)."""
    a, b = align_ref.f64(a).reshape(-1, 3), align_ref.f64(b).reshape(-1, 3)
    Ma, Mb = a.shape[0], b.shape[0]
    ia = np.arange(Ma) if mask_a is None else np.flatnonzero(np.asarray(mask_a) != 0)
    ib = np.arange(Mb) if mask_b is None else np.flatnonzero(np.asarray(mask_b) != 0)
    na, nb = ia.size, ib.size
    out = np.full(Ma, -1, dtype=np.int64)
    if na == 0 or nb == 0:
        return Result(out, 0, 0.0, 0.0, np.full((3, 3), np.nan), np.full(3, np.nan), 0, na, nb, 0)
    pa, pb = a[ia], b[ib]
    d0 = float(np.float32(S.tm_d0(min(na, nb)) if d0 is None else d0))
    best, winner, passes = (-np.inf, None, None, None), 0, 0
    for start in starts:
        if start == 0:
            m = threading(pa, pb, d0, reverse)[0]
        elif use_ss:
            la, lb = secondary_structure(pa), secondary_structure(pb)
            m = nw((la[:, None] == lb[None, :]).astype(np.float64), -1.0).map
            passes += 1
        else:
            continue
        found = refine(pa, pb, m, d0, reverse)
        passes += found[4]
        if found[0] > best[0]:
            best, winner = found[:4], start
    hit = best[1] >= 0
    out[ia[hit]] = ib[best[1][hit]]
    return Result(out, int(hit.sum()), best[0], best[0] / min(na, nb), best[2], best[3], winner, na, nb, passes)


def score_of(R, t, a, b, m, d0, n_norm):
    """sum of the TM terms over the pairs of the slot map m under (R, t), per n_norm: what the returned transform must
    reproduce"""
    a, b = align_ref.f64(a).reshape(-1, 3), align_ref.f64(b).reshape(-1, 3)
    idx = np.flatnonzero(np.asarray(m) >= 0)
    if idx.size == 0:
        return 0.0
    d2 = S.dist2(align_ref.f64(R), align_ref.f64(t), a[idx], b[np.asarray(m)[idx]])
    return float(tm_terms(d2, float(np.float32(d0))).sum() / n_norm)


# ---- case builders ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ca_trace(name, chain):
    """(CA coordinates (n,3) float32, residue names) of one chain of tests/golden/<name>.pdb, every ATOM record named CA"""
    xyz, names = [], []
    with open(os.path.join(GOLDEN_DIR, name + ".pdb")) as f:
        for line in f:
            if line.startswith("ATOM") and line[12:16] == " CA " and line[21] == chain and line[16] in " A":
                xyz.append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
                names.append(line[17:20])
    return S.f32(np.array(xyz)), tuple(names)


def cut_1rex(seed=3, noise=0.8):
    """1REX against itself with residues 0-11 and 60-68 cut out, moved rigidly, ``noise`` A on every coordinate:
    (a (130,3), b (109,3), the known map (130,))"""
    a = ca_trace("1REX", "A")[0]
    keep = np.ones(a.shape[0], dtype=bool)
    keep[0:12], keep[60:69] = False, False
    rng = np.random.default_rng(seed)
    b = a[keep].astype(np.float64) @ align_ref.rotation(rng).T + rng.uniform(-30, 30, 3) + noise * rng.standard_normal((int(keep.sum()), 3))
    known = np.full(a.shape[0], -1, dtype=np.int64)
    known[keep] = np.arange(int(keep.sum()))
    return a, S.f32(b), known


def scatter(x, masked=0.45, seed=0, M=None):
    """(X (M,3), mask (M,)): the n points in order among M = round(n / (1 - masked)) slots, the others masked and NaN"""
    n = x.shape[0]
    M = max(int(round(n / (1.0 - masked))), n, 1) if M is None else M
    rng = np.random.default_rng(seed + 104729)
    mask = np.zeros(M, dtype=bool)
    mask[np.sort(rng.choice(M, n, replace=False))] = True
    X = np.full((M, 3), np.nan, np.float32)
    X[mask] = x
    return X, mask


def helix(n, seed=0, noise=0.1):
    """an ideal alpha-helical CA trace with a little noise"""
    k = np.arange(n)
    rng = np.random.default_rng(seed)
    x = np.stack([2.3 * np.cos(np.deg2rad(100.0) * k), 2.3 * np.sin(np.deg2rad(100.0) * k), 1.5 * k], axis=1)
    return S.f32(x + noise * rng.standard_normal((n, 3)))


def strand(n, seed=0, noise=0.1):
    """an ideal extended CA trace with a little noise"""
    k = np.arange(n)
    rng = np.random.default_rng(seed)
    x = np.stack([3.3 * k, 0.9 * (k % 2), np.zeros(n)], axis=1)
    return S.f32(x + noise * rng.standard_normal((n, 3)))


def small_pair(na, nb, seed=0):
    """na points of a 40-point chain's middle, moved and jittered, against the chain (or the other way round): (a, b)"""
    rng = np.random.default_rng(1000 + 41 * na + nb + seed)
    long = np.cumsum(rng.standard_normal((40, 3)) * 2.2, axis=0)
    n = min(na, nb)
    short = long[17:17 + n] @ align_ref.rotation(rng).T + rng.uniform(-10, 10, 3) + 0.3 * rng.standard_normal((n, 3))
    return (S.f32(short), S.f32(long)) if na <= nb else (S.f32(long), S.f32(short))


Case = namedtuple("Case", "a b mask_a mask_b d0 use_ss")


def _case(a, b, mask_a=None, mask_b=None, d0=None, use_ss=True):
    na = a.shape[0] if mask_a is None else int(mask_a.sum())
    nb = b.shape[0] if mask_b is None else int(mask_b.sum())
    d0 = float(np.float32(S.tm_d0(max(min(na, nb), 1)) if d0 is None else d0))
    return Case(a, b, mask_a, mask_b, d0, use_ss)


@functools.lru_cache(maxsize=None)
def alignment_cases():
    """name -> Case: every alignment case the GPU tests run"""
    h1, l1 = ca_trace("1a3r_HL", "H")[0], ca_trace("1a3r_HL", "L")[0]
    h5, l5 = ca_trace("5cjx_HL", "H")[0], ca_trace("5cjx_HL", "L")[0]
    cases = {"1a3r H on L": _case(h1, l1), "5cjx H on L": _case(h5, l5), "5cjx H on 1a3r H": _case(h5, h1),
             "V on C": _case(l1, h5[-107:]), "V on C, no ss": _case(l1, h5[-107:], use_ss=False)}
    a, b, _ = cut_1rex()
    cases["cut 1REX"] = _case(a, b)
    cases["itself"] = _case(l1, l1.copy())
    for n in range(6):
        cases[f"{n} on 40"] = _case(*small_pair(n, 40)) if n else _case(np.zeros((1, 3), np.float32), small_pair(1, 40)[1],
                                                                           np.zeros(1, dtype=bool))
        cases[f"40 on {n}"] = _case(*small_pair(40, n)) if n else _case(small_pair(40, 1)[0], np.zeros((1, 3), np.float32), None,
                                                                           np.zeros(1, dtype=bool))
    for k, (na, nb) in enumerate(PADDED):
        cases[f"padded {k}"] = padded_case(k)
    rng = np.random.default_rng(8)
    chain = np.cumsum(rng.standard_normal((70, 3)) * 2.2, axis=0)
    moved = chain[6:66] @ align_ref.rotation(rng).T + rng.uniform(-10, 10, 3) + 0.4 * rng.standard_normal((60, 3))
    (A, ma), (Bt, mb) = scatter(S.f32(moved), seed=1, M=MAX_POINTS), scatter(S.f32(chain), seed=2, M=MAX_POINTS)
    cases["M=1024"] = _case(A, Bt, ma, mb)
    return cases


PADDED = ((31, 57), (48, 20), (57, 55))       # (n_a, n_b) of the padded batch; its arrays are PADDED_M slots long
PADDED_M = (104, 104)


def padded_case(k):
    """structure k of the padded batch: chains of unequal lengths scattered among 45 % masked slots over NaN"""
    na, nb = PADDED[k]
    rng = np.random.default_rng(500 + k)
    chain = np.cumsum(rng.standard_normal((max(na, nb) + 8, 3)) * 2.2, axis=0)
    a = chain[3:3 + na] @ align_ref.rotation(rng).T + rng.uniform(-10, 10, 3) + 0.5 * rng.standard_normal((na, 3))
    b = chain[5:5 + nb] + 0.5 * rng.standard_normal((nb, 3))
    (A, ma), (Bt, mb) = scatter(S.f32(a), seed=10 + k, M=PADDED_M[0]), scatter(S.f32(b), seed=20 + k, M=PADDED_M[1])
    return _case(A, Bt, ma, mb)


@functools.lru_cache(maxsize=None)
def restated(name, reverse=False):
    """the restatement of an alignment case, once"""
    c = alignment_cases()[name]
    return align(c.a, c.b, c.mask_a, c.mask_b, c.d0, c.use_ss, reverse)


# ---- DP cases -----------------------------------------------------------------------------------------------------------------
DP_SHAPES = ((1, 1), (1, 7), (2, 3), (63, 64), (64, 65), (65, 63), (130, 257), (257, 130), (1024, 3), (3, 1024))
DP_GAPS = (0.0, -0.6, -1.0)
DP_FAMILIES = ("eighths", "zeros", "diagonal")


def dp_scores(family, na, nb, seed=0):
    """(na, nb) float32 scores: multiples of 1/8 in [0, 1] (ties everywhere), all zeros (pure tie-breaking), or a sharp
    diagonal with an offset block"""
    rng = np.random.default_rng(7000 + 13 * na + nb + seed)
    if family == "eighths":
        return (rng.integers(0, 9, (na, nb)) / 8.0).astype(np.float32)
    if family == "zeros":
        return np.zeros((na, nb), np.float32)
    i, j = np.arange(na)[:, None], np.arange(nb)[None, :]
    shift = np.where(i < na // 2, 0, max(1, nb // 5))
    return (np.exp(-0.5 * (j - (i + shift)) ** 2) + 0.01 * rng.random((na, nb))).astype(np.float32)


def dp_scatter(score, seed=0, masked=0.45):
    """(score (Ma, Mb) with NaN at masked slots, mask_a, mask_b) with the given scores at the unmasked slots"""
    na, nb = score.shape
    _, ma = scatter(np.zeros((na, 3), np.float32), masked, seed)
    _, mb = scatter(np.zeros((nb, 3), np.float32), masked, seed + 1)
    full = np.full((ma.size, mb.size), np.nan, np.float32)
    full[np.ix_(np.flatnonzero(ma), np.flatnonzero(mb))] = score
    return full, ma, mb
