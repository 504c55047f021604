"""float64 model of metric SMACOF (sklearn 1.7's smacof / _smacof_single) and of the finishing step of
geometry.initialize_backbone_with_mds (reference geometry.py:350-410): the yardsticks of tests/test_gpu_mds.py.

smacof64 follows the equations of include/protstruc_hip.h (ps_smacof_f32): distances by direct differences, the Guttman
transform, sigma and S over the full matrix, the stop rule (sigma_t - sigma_{t+1}) / (S_{t+1} / 2) < eps for t >= 1.
"""
import numpy as np

# reference constants/ideal.py
AB, NAB, BANC = 1.522, 1.927, -2.143
CO, ACO, NACO = 1.231, 2.108, -3.142


def pdist64(X):
    diff = X[:, None, :] - X[None, :, :]
    return np.sqrt((diff * diff).sum(-1))


def smacof_single64(delta, X0, max_iter=300, eps=1e-6, history=False):
    """One start: (X, stress, n_iter) or, with ``history``, also the list of sigma_1 .. sigma_T."""
    delta = np.asarray(delta, dtype=np.float64)
    X = np.asarray(X0, dtype=np.float64).copy()
    n = X.shape[0]
    d = pdist64(X)
    old = None
    sigmas = []
    for it in range(max_iter):
        dt = np.where(d == 0, 1e-5, d)   # (errstate below: a one-node or collapsed S = 0 gives 0 / 0 in the stop rule)
        ratio = delta / dt
        X = (ratio.sum(1)[:, None] * X - ratio @ X) / n
        d = pdist64(X)
        stress = ((d - delta) ** 2).sum() / 2
        sigmas.append(stress)
        with np.errstate(divide="ignore", invalid="ignore"):
            stop = old is not None and (old - stress) / ((d ** 2).sum() / 2) < eps
        if stop:
            break
        old = stress
    out = (X, stress, it + 1)
    return out + (sigmas,) if history else out


def smacof64(delta, starts, max_iter=300, eps=1e-6):
    """K starts (K, n, 3): the best (X, stress, n_iter, index), smallest stress, lowest index on ties."""
    best = None
    for k, X0 in enumerate(starts):
        X, s, it = smacof_single64(delta, X0, max_iter, eps)
        if best is None or s < best[1]:
            best = (X, s, it, k)
    return best


def random_starts(K, n, random_state):
    """sklearn's draws for K starts of n nodes: random_state.uniform(size=3 n) per start, in order."""
    return np.stack([random_state.uniform(size=3 * n).reshape(n, 3) for _ in range(K)])


def node_matrix(dist_mat):
    """(3, 3, L, L) -> the (3 L, 3 L) matrix of nodes g L + i (the reference's transpose(0, 2, 1, 3))."""
    L = dist_mat.shape[-1]
    return np.asarray(dist_mat, dtype=np.float64).transpose(0, 2, 1, 3).reshape(3 * L, 3 * L)


def dihedral64(a, b, c, d):
    b0, b1, b2 = a - b, c - b, d - c
    b1n = b1 / np.linalg.norm(b1, axis=-1, keepdims=True)
    v = b0 - (b0 * b1n).sum(-1, keepdims=True) * b1n
    w = b2 - (b2 * b1n).sum(-1, keepdims=True) * b1n
    x = (v * w).sum(-1)
    y = (np.cross(b1n, v) * w).sum(-1)
    return np.arctan2(y, x)


def place4_64(a, b, c, length, planar, dihedral):
    bc = b - c
    bc = bc / np.linalg.norm(bc, axis=-1, keepdims=True)
    nv = np.cross(b - a, bc)
    nv = nv / np.linalg.norm(nv, axis=-1, keepdims=True)
    m = np.cross(nv, bc)
    return c + length * np.cos(planar) * bc + length * np.sin(planar) * np.cos(dihedral) * m \
        - length * np.sin(planar) * np.sin(dihedral) * nv


def mean_phi64(coords):
    n, ca, c = coords
    return dihedral64(c[:-1], n[1:], ca[1:], c[1:]).mean() if coords.shape[1] > 1 else np.nan


def fix_chirality64(coords, mirror=True):
    """(3, L, 3) -> mirrored (z negated) iff the mean phi is positive (never with mirror=False)."""
    coords = np.asarray(coords, dtype=np.float64)
    if mirror and mean_phi64(coords) > 0:
        return coords * np.array([1.0, 1.0, -1.0])
    return coords


def finish64(coords, mirror=True):
    """(3, L, 3) N / CA / C -> (5, L, 3) N, CA, C, O, CB (reference geometry.py:365-386 after fix_chirality)."""
    x = fix_chirality64(coords, mirror)
    n, ca, c = x
    cb = place4_64(c, n, ca, AB, NAB, BANC)
    o = place4_64(np.roll(n, -1, axis=0), ca, c, CO, ACO, NACO)
    return np.concatenate([x, o[None], cb[None]], 0)


def kabsch_rmsd64(P, Q, proper=True):
    """RMSD of P onto Q (n, 3) after the best rotation (proper = det +1 only) and translation."""
    P = np.asarray(P, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    p, q = P - P.mean(0), Q - Q.mean(0)
    U, S, Vt = np.linalg.svd(p.T @ q)
    dsign = np.sign(np.linalg.det(U @ Vt)) if proper else 1.0
    Dm = np.diag([1.0, 1.0, dsign])
    R = U @ Dm @ Vt
    return float(np.sqrt((((p @ R) - q) ** 2).sum(1).mean()))
