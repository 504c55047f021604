"""Host models of the distance-matrix reconstruction behind geometry.reconstruct_backbone_distmat_from_interresidue_geometry
(reference geometry.py:229-347), for the tests.

* ``init64``: steps 1-6 (placements, distances, categorical entries) in float64 numpy -- the yardstick of K8;
* ``fw_sequential``: step 7, the reference's loop D[r][c] = min(D[r][c], D[k][r] + D[k][c]), one pivot at a time, in
  float32 torch (on whatever device the tensor lives: the additions and minima are exact IEEE float32 either way);
* ``fw_blocked``: the same update in pivot blocks (panel snapshots + a min-plus product), float32 numpy -- the scheme
  of K9, which must equal ``fw_sequential`` bit for bit;
* ``finish``: steps 8-9 in float32 torch;
* ``geometry_of``: d_cb / omega (trRosetta) / theta / phi of given N, CA, CB coordinates in float64.
Node (g, i) = g L + i of a (B, G, G, L, L) tensor; ``to_nodes`` / ``from_nodes`` convert to and from (B, n, n).
"""
import numpy as np
import torch

from tests import nerf_ref as R

MASK = 12345679.0
FLT_MAX = float(np.finfo(np.float32).max)
# reference constants/ideal.py
NA, AC, C_N, NC, BA, AB, BAN, ANC, NAB, BANC = 1.458, 1.523, 1.329, 2.460, 1.522, 1.522, 1.927, 0.615, 1.927, -2.143
DIAG = np.array([[0.0, NA, NC], [NA, 0.0, AC], [NC, AC, 0.0]])   # ideal.as_dict["ab"] for a, b in N, CA, C


def ideal_local_frame():
    """N, CA, C, CB of the reference's ideal_local_frame() (geometry.py:171-188) in float64: N at the origin, CA on +z."""
    n = np.zeros(3)
    ca = np.array([0.0, 0.0, NA])
    cb = np.array([0.0, AB * np.sin(NAB), NA - AB * np.cos(NAB)])
    c = R.place_fourth_atom(cb, ca, n, NC, ANC, BANC)
    return np.array([n, ca, c, cb])


def place_pairs(d_cb, omega, theta, phi):
    """Residue j's N, CA, C in residue i's ideal frame for every pair: (4, B, L, L, 3) float64 of (N, CA, C, CB)."""
    d_cb, omega, theta, phi = (np.asarray(t, dtype=np.float64)[..., None] for t in (d_cb, omega, theta, phi))
    x = ideal_local_frame()
    phi_t, theta_t = np.swapaxes(phi, -2, -3), np.swapaxes(theta, -2, -3)
    shape = d_cb.shape[:-1] + (3,)
    N, CA, CB = (np.broadcast_to(x[k], shape) for k in (0, 1, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        y_cb = R.place_fourth_atom(N, CA, CB, d_cb, phi, theta)
        y_ca = R.place_fourth_atom(CA, CB, y_cb, BA, phi_t, omega)
        y_n = R.place_fourth_atom(CB, y_cb, y_ca, NA, BAN, theta_t)
        y_c = R.place_fourth_atom(y_cb, y_ca, y_n, NC, ANC, BANC)
    return np.stack([y_n, y_ca, y_c, y_cb])


def break_matrix(chain_breaks, B, L):
    out = np.zeros((B, L), dtype=bool)
    if chain_breaks is not None:
        out[:] = np.asarray(chain_breaks, dtype=bool).reshape(B, L)
    return out


def init64(d_cb, omega, theta, phi, mask=None, chain_breaks=None, lengths=None):
    """Steps 1-6 in float64: (B, L, L) inputs -> (B, 3, 3, L, L).  Returns (values, categorical) where ``categorical``
    marks the entries that do not come from a placement (diagonal, bonds, breaks, mask, padding)."""
    B, L = np.asarray(d_cb).shape[:2]
    y = place_pairs(d_cb, omega, theta, phi)[:3]                       # (3, B, L, L, 3)
    x = ideal_local_frame()[:3]
    D = np.linalg.norm(x[:, None, None, None, None, :] - y[None], axis=-1)   # (a, b, B, L, L)
    D = np.ascontiguousarray(D.transpose(2, 0, 1, 3, 4))
    cat = np.zeros(D.shape, dtype=bool)
    ar = np.arange(L)
    D[:, :, :, ar, ar] = DIAG[None, :, :, None]
    cat[:, :, :, ar, ar] = True
    brk = break_matrix(chain_breaks, B, L)
    i = np.arange(L - 1)
    for b in range(B):
        v = np.where(brk[b, :L - 1], MASK, C_N)
        D[b, 2, 0, i, i + 1] = v
        D[b, 0, 2, i + 1, i] = v
        cat[b, 2, 0, i, i + 1] = cat[b, 0, 2, i + 1, i] = True
    if mask is not None:
        off = ~np.asarray(mask, dtype=bool)
        D[np.broadcast_to(off[:, None, None], D.shape)] = MASK
        cat |= np.broadcast_to(off[:, None, None], D.shape)
    nan = np.isnan(D)
    cat |= nan | np.isinf(D)
    D = np.nan_to_num(D, nan=MASK, posinf=FLT_MAX, neginf=-FLT_MAX)
    if lengths is not None:
        for b, n in enumerate(lengths):
            n = int(n)
            pad = np.zeros((L, L), dtype=bool)
            pad[n:, :] = pad[:, n:] = True
            D[b][:, :, pad] = MASK
            for a in range(3):
                D[b, a, a, ar[n:], ar[n:]] = 0.0
            cat[b][:, :, pad] = True
    return D, cat


def to_nodes(D):
    """(B, G, G, L, L) -> (B, G L, G L) with node (g, i) = g L + i."""
    B, G, _, L, _ = D.shape
    if isinstance(D, torch.Tensor):
        return D.permute(0, 1, 3, 2, 4).reshape(B, G * L, G * L)
    return D.transpose(0, 1, 3, 2, 4).reshape(B, G * L, G * L)


def from_nodes(M, G):
    B, n, _ = M.shape
    L = n // G
    if isinstance(M, torch.Tensor):
        return M.reshape(B, G, L, G, L).permute(0, 1, 3, 2, 4).contiguous()
    return np.ascontiguousarray(M.reshape(B, G, L, G, L).transpose(0, 1, 3, 2, 4))


def fw_sequential(M):
    """The reference's Floyd-Warshall loop (geometry.py:327-330) on a float32 (B, n, n) tensor: for each k in order,
    M = min(M, M[k][r] + M[k][c]).  Returns a new tensor."""
    M = M.clone()
    for k in range(M.shape[-1]):
        d = M[:, k, :]
        M = torch.minimum(M, d[:, None, :] + d[:, :, None])
    return M


def fw_blocked(M, b):
    """K9's scheme in float32 numpy on (B, n, n): per pivot block, the block's rows evolve step by step with snapshots
    P[k] (row k as step k reads it); every other row takes min(M[r][c], min_k P[k][r] + P[k][c])."""
    M = np.array(M, dtype=np.float32, copy=True)
    n = M.shape[-1]
    for k0 in range(0, n, b):
        K = np.arange(k0, min(n, k0 + b))
        panel = M[:, K, :].copy()
        P = np.empty_like(panel)
        for t in range(len(K)):
            P[:, t] = panel[:, t]
            cand = panel[:, t, K][:, :, None] + panel[:, t][:, None, :]   # (B, |K|, n): P[k][k'] + P[k][c]
            others = np.arange(len(K)) != t
            panel[:, others] = np.minimum(panel[:, others], cand[:, others])
        rest = np.setdiff1d(np.arange(n), K)
        best = M[:, rest, :]
        for t in range(len(K)):
            best = np.minimum(best, P[:, t, rest][:, :, None] + P[:, t][:, None, :])
        M[:, rest, :] = best
        M[:, K, :] = panel
    return M


def finish(D, chain_breaks=None, lengths=None):
    """Steps 8-9 on a float32 (B, 3, 3, L, L) tensor: (D + D^T) / 2 over the nodes, the bonds again (none across a
    chain break), NaN for residues at or beyond ``lengths``.  Returns a new tensor."""
    B, _, _, L, _ = D.shape
    M = to_nodes(D)
    M = (M + M.transpose(1, 2)) / 2.0
    D = from_nodes(M, 3)
    ar = torch.arange(L, device=D.device)
    D[:, 0, 1, ar, ar] = NA
    D[:, 1, 0, ar, ar] = NA
    D[:, 1, 2, ar, ar] = AC
    D[:, 2, 1, ar, ar] = AC
    brk = torch.as_tensor(break_matrix(None if chain_breaks is None else np.asarray(chain_breaks), B, L), device=D.device)
    for b in range(B):
        i = torch.nonzero(~brk[b, :L - 1]).flatten()
        D[b, 2, 0, i, i + 1] = C_N
        D[b, 0, 2, i + 1, i] = C_N
    if lengths is not None:
        for b, n in enumerate(lengths):
            n = int(n)
            D[b, :, :, n:, :] = float("nan")
            D[b, :, :, :, n:] = float("nan")
    return D


def geometry_of(n, ca, cb):
    """trRosetta geometry of coordinates (B, L, 3) each, float64: d_cb, omega = dihedral(CA_i, CB_i, CB_j, CA_j),
    theta = dihedral(N_i, CA_i, CB_i, CB_j), phi = angle(CA_i, CB_i, CB_j)."""
    n, ca, cb = (np.asarray(t, dtype=np.float64) for t in (n, ca, cb))
    I = lambda t: t[:, :, None, :]   # noqa: E731  residue i
    J = lambda t: t[:, None, :, :]   # noqa: E731  residue j
    L = n.shape[1]
    full = lambda t: np.broadcast_to(t, (n.shape[0], L, L, 3))   # noqa: E731
    d_cb = np.linalg.norm(I(cb) - J(cb), axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        omega = R.dihedral(full(I(ca)), full(I(cb)), full(J(cb)), full(J(ca)))
        theta = R.dihedral(full(I(n)), full(I(ca)), full(I(cb)), full(J(cb)))
        phi = R.angle(full(I(ca)), full(I(cb)), full(J(cb)))
    return d_cb, omega, theta, phi


def random_rotations(rng, k):
    q = rng.normal(size=(k, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def rigid_ideal_residues(rng, B, L, spread=12.0):
    """B structures of L rigid copies of ideal_local_frame() in random poses: (N, CA, C, CB) each (B, L, 3), float64."""
    x = ideal_local_frame()
    Rm = random_rotations(rng, B * L).reshape(B, L, 3, 3)
    t = rng.uniform(-spread, spread, size=(B, L, 3))
    atoms = np.einsum("blij,aj->abli", Rm, x) + t[None]
    return atoms[0], atoms[1], atoms[2], atoms[3]


def true_distmat(n, ca, c):
    """|atom a of residue i - atom b of residue j| for a, b in N, CA, C: (B, 3, 3, L, L) float64."""
    X = np.stack([n, ca, c], axis=1)   # (B, 3, L, 3)
    return np.linalg.norm(X[:, :, None, :, None, :] - X[:, None, :, None, :, :], axis=-1)


def random_graph(rng, B, n, mask_frac=0.3, nonzero_diag=False):
    """Random asymmetric non-negative float32 (B, n, n) with ~mask_frac MASK entries and a zero (or small) diagonal."""
    M = rng.uniform(0.0, 20.0, size=(B, n, n)).astype(np.float32)
    M[rng.random(size=M.shape) < mask_frac] = MASK
    d = np.arange(n)
    M[:, d, d] = rng.uniform(0.0, 0.5, size=(B, n)).astype(np.float32) if nonzero_diag else 0.0
    return M
