"""Yardstick of the alignment and rigid-body kernels (csrc/align.hip, csrc/rigid.hip: ps_kabsch_f32,
ps_min_dist_to_points_f32, ps_rigid_f32, ps_center_of_mass_f32, ps_frames_to_backbone_f32): plain float64 numpy
restatements of the reference's formulas, and the builders of the cases the tests use.  Inputs are float32 values widened
to float64; nothing here imports the package under test.

    Kabsch     ca, cb = centroids over the selected atoms,  H = sum (a - ca)(b - cb)^T = U S V^T,
               d = sign det(V U^T),  R = V diag(1, 1, d) U^T,  t = cb - R ca
    unique     the optimal rotation is unique iff s1 + d s2 > 0; the tests compare R elementwise only where
               s1 + d s2 > UNIQUE * s0 and hold every other case to the properties (orthonormal, det 1, optimal RMSD)
    DELTA      2^-22 (3 max_k |a_k| + |t|): twice the displacement of an atom when a perfect (R, t) is rounded to float32
               (each R_ij moves by at most 2^-25, so a row of R a by sqrt(3) 2^-25 |a| and the vector by 3 2^-25 |a|; t_i by
               2^-25 |t_i|); the RMSD over atoms moved by at most DELTA grows by at most DELTA
"""
from collections import namedtuple

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
UNIQUE = 1e-3
ORTHO_BOUND = 8 * U32     # max |R R^T - I| of a rotation whose rows are unit vectors rounded to float32
DET_BOUND = 16 * U32
R_TOL = 5e-6              # elementwise |R - R64| where the rotation is unique (tests/test_gpu_parity.py)
TOPK_GAP = 1e-3           # every top-k case keeps its k-th and (k+1)-th distance further apart than this
CA = 1

Kabsch = namedtuple("Kabsch", "R t s d rmsd")


def f64(x):
    """numpy float64 of a tensor or array (float32 values are widened exactly)."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def _selected(a, b, mask):
    a, b = f64(a).reshape(-1, 3), f64(b).reshape(-1, 3)
    if mask is None:
        return a, b
    m = np.asarray(mask.detach().cpu().numpy() if hasattr(mask, "detach") else mask).reshape(-1) != 0
    return a[m], b[m]


def kabsch64(a, b, mask=None):
    """Kabsch(R, t, s, d, rmsd) of point sets (n,3) over the atoms of ``mask`` (all if None).  No selected atom: every
    field is NaN (the reference's 0 / 0).  One atom, or coincident atoms: H = 0, whose SVD is U = V = I, so R = I."""
    a, b = _selected(a, b, mask)
    if a.shape[0] == 0:
        nan = np.full(3, np.nan)
        return Kabsch(np.full((3, 3), np.nan), nan, nan, np.nan, np.nan)
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    U, s, Vt = np.linalg.svd(H)
    V = Vt.T
    d = float(np.sign(np.linalg.det(V @ U.T)))
    R = V @ np.diag([1.0, 1.0, d]) @ U.T
    t = cb - R @ ca
    return Kabsch(R, t, s, d, rmsd64(R, t, a, b))


def rmsd64(R, t, a, b, mask=None):
    """sqrt(mean |R a + t - b|^2) over the selected atoms, for any R (3,3) and t (3,)."""
    a, b = _selected(a, b, mask)
    diff = a @ f64(R).T + f64(t) - b
    return float(np.sqrt((diff ** 2).sum(-1).mean()))


def delta(a, t, mask=None):
    """DELTA of the module docstring for the selected atoms of ``a`` and a translation ``t``."""
    a, _ = _selected(a, a, mask)
    return 2.0 ** -22 * (3 * float(np.sqrt((a ** 2).sum(-1)).max()) + float(np.linalg.norm(f64(t))))


def is_unique(k):
    return bool(k.s[1] + k.d * k.s[2] > UNIQUE * k.s[0])


def rotation_errors(R):
    """(max |R R^T - I|, |det R - 1|) of a (3,3), evaluated in float64."""
    R = f64(R)
    return float(np.abs(R @ R.T - np.eye(3)).max()), float(abs(np.linalg.det(R) - 1.0))


# ---- rigid-body ops ---------------------------------------------------------------------------------------------------
def _rigid_operands(xyz, R, t, transpose):
    x = f64(xyz)
    B, N, A = x.shape[:3]
    if R is None:
        M = np.broadcast_to(np.eye(3), (B, N, A, 3, 3))
    else:
        M = f64(R)
        M = {2: M[None, None, None], 3: M[:, None, None], 4: M[:, :, None]}[M.ndim]
        if transpose:
            M = np.swapaxes(M, -1, -2)
        M = np.broadcast_to(M, (B, N, A, 3, 3))
    if t is None:
        v = np.zeros((B, N, A, 3))
    else:
        v = f64(t)
        if v.shape == (3,) or v.shape == (1, 3):
            v = v.reshape(1, 1, 1, 3)
        elif v.shape == (B, 3) or v.shape == (B, 1, 3):
            v = v.reshape(B, 1, 1, 3)
        elif v.shape == (B, N, 3):
            v = v[:, :, None]
        else:
            assert v.shape == (B, N, A, 3), v.shape
        v = np.broadcast_to(v, (B, N, A, 3))
    return x, M, v


def rigid64(xyz, R=None, t=None, transpose=False):
    """(R x + t or R^T x + t, scale) for xyz (B,N,A,3) and every form ops.rigid accepts: R None | (3,3) | (B,3,3) |
    (B,N,3,3); t None | (3,) | (1,3) | (B,3) | (B,1,3) | (B,N,3) | (B,N,A,3).  ``scale_i = sum_j |R_ij x_j| + |t_i|``: three
    float32 products, three sums and the translation add keep the error of component i below 4 * 2^-24 * scale_i."""
    x, M, v = _rigid_operands(xyz, R, t, transpose)
    if R is None:             # no product: a NaN component stays in its own component
        return x + v, np.abs(x) + np.abs(v)
    terms = M * x[..., None, :]
    return terms.sum(-1) + v, np.abs(terms).sum(-1) + np.abs(v)


def center_of_mass64(xyz, atom=CA):
    """(B,3) per-component mean of slot ``atom`` over the residues whose component is not NaN; NaN where none is."""
    p = f64(xyz)[:, :, atom]
    ok = ~np.isnan(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, p, 0.0).sum(1) / ok.sum(1)


def frames_to_backbone64(rot, trans, ideal, n_slots):
    """(xyz (B,N,n_slots,3), scale): rot @ ideal[a] + trans in the first len(ideal) slots, exact zeros after."""
    rot, trans, ideal = f64(rot), f64(trans), f64(ideal)
    B, N = rot.shape[:2]
    terms = rot[:, :, None] * ideal[None, None, :, None, :]
    xyz = np.zeros((B, N, n_slots, 3))
    scale = np.zeros((B, N, n_slots, 3))
    xyz[:, :, :ideal.shape[0]] = terms.sum(-1) + trans[:, :, None]
    scale[:, :, :ideal.shape[0]] = np.abs(terms).sum(-1) + np.abs(trans[:, :, None])
    return xyz, scale


def min_dist64(xyz_one, query, atom=CA):
    """(N,) distance of slot ``atom`` of every residue of one structure (N,A,3) to its nearest query point; a NaN query
    point turns every entry NaN and a NaN atom its own entry (numpy's min propagates NaN as torch's does)."""
    p, q = f64(xyz_one)[:, atom], f64(query).reshape(-1, 3)
    return np.sqrt(((p[:, None] - q[None]) ** 2).sum(-1)).min(-1)


def topk_mask64(xyz_one, residue_mask, query, k, mask=None, atom=CA):
    """(mask (N,) of the min(k, valid) valid residues nearest to a query point, gap between the last distance taken and
    the first one left out -- inf when nothing is left out).  Invalid residues sit at 1e9 as in the reference."""
    dist = min_dist64(xyz_one, query, atom)
    valid = np.asarray(residue_mask).reshape(-1) != 0
    if mask is not None:
        valid = valid & (np.asarray(mask).reshape(-1) != 0)
    dist = np.where(valid, dist, 1e9)
    k = min(int(k), int(valid.sum()))
    order = np.argsort(dist, kind="stable")
    out = np.zeros(dist.shape[0], dtype=bool)
    out[order[:k]] = True
    gap = float(dist[order[k]] - dist[order[k - 1]]) if 0 < k < dist.shape[0] else float("inf")
    return out, gap


# ---- case builders ------------------------------------------------------------------------------------------------------
def rotation(rng, proper=True):
    """A random orthogonal 3x3 (float64) with det +1, or -1 for ``proper=False``."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) < 0) == proper:
        q[:, 0] = -q[:, 0]
    return q


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def cloud(n, seed=0, noise=0.5, proper=True, scale=10.0):
    """A generic pair: a = scale * randn, b = Q a + shift + noise * randn with Q a rotation (a reflection for
    ``proper=False``: the mirror-image target)."""
    rng = np.random.default_rng(seed)
    a = scale * rng.standard_normal((n, 3))
    b = a @ rotation(rng, proper).T + rng.uniform(-20, 20, 3) + noise * rng.standard_normal((n, 3))
    return _f32(a), _f32(b)


def planar(n=40, seed=1):
    """Source exactly in the plane z = 0; target the rotated plane with in-plane noise: H has rank 2."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([8 * rng.standard_normal((n, 2)), np.zeros((n, 1))], 1)
    noisy = a + np.concatenate([0.3 * rng.standard_normal((n, 2)), np.zeros((n, 1))], 1)
    return _f32(a), _f32(noisy @ rotation(rng).T + rng.uniform(-5, 5, 3))


def collinear(n=30):
    """Both sets EXACTLY collinear in float32 (every coordinate a small dyadic rational): H has rank 1.  The spacings
    differ by multiples of 1/1024, so the optimal RMSD is not zero."""
    k = np.arange(n, dtype=np.float64)
    e = ((k * 7) % 5 - 2) / 1024.0
    a = np.stack([k, 2 * k, -k], 1) * 0.5 + np.array([3.0, -1.0, 2.0])
    b = (k + e)[:, None] * np.array([0.75, 0.0, 1.0]) * 1.5 + np.array([-4.0, 6.0, 0.5])
    assert (_f32(a) == a).all() and (_f32(b) == b).all()
    return _f32(a), _f32(b)


def line_plus_noise(sigma, n=30, seed=2):
    """Points along a 30 A line plus isotropic noise ``sigma`` on both sets (1e-6 is below float32's resolution of the
    larger coordinates: what is left of it is whatever survives the rounding of the inputs)."""
    rng = np.random.default_rng(seed)
    line = np.linspace(-15, 15, n)[:, None] * np.array([[0.6, -0.48, 0.64]])
    a = line + sigma * rng.standard_normal((n, 3))
    b = line @ rotation(rng).T + np.array([2.0, -3.0, 1.0]) + sigma * rng.standard_normal((n, 3))
    return _f32(a), _f32(b)


def coincident(n=5):
    """All atoms of the source at one point and all atoms of the target at another: H = 0 exactly."""
    return _f32(np.tile([1.25, -7.5, 3.0625], (n, 1))), _f32(np.tile([-2.5, 0.75, 11.0], (n, 1)))


def octahedron(seed=3):
    """Six points on the axes: three equal singular values, yet one optimal rotation."""
    rng = np.random.default_rng(seed)
    a = 4.0 * np.concatenate([np.eye(3), -np.eye(3)])
    return _f32(a), _f32(a @ rotation(rng).T + np.array([1.0, 2.0, -3.0]))


def far(offset, n=360, seed=0):
    """The generic cloud with both centroids moved ``offset`` A from the origin (the inputs are the rounded values)."""
    a, b = cloud(n, seed)
    shift = offset * np.array([0.6, -0.64, 0.48])
    return _f32(a + shift), _f32(b + shift[[2, 0, 1]])


def first_atoms(n_sel, seed=4):
    """The first ``n_sel`` atoms of a generic cloud (1, 2, 3 and 4 selected atoms)."""
    a, b = cloud(8, seed, noise=0.3)
    return a[:n_sel].copy(), b[:n_sel].copy()


def kabsch_cases():
    """name -> (a (n,3) float32, b (n,3) float32): every degenerate and generic selection the Kabsch tests use."""
    cases = {"generic 360": cloud(360), "mirror-image target": cloud(360, seed=5, proper=False), "planar": planar(),
             "collinear": collinear(), "coincident": coincident(), "octahedron": octahedron(),
             "far 1e3": far(1e3), "far 1e4": far(1e4)}
    a, _ = cloud(50, seed=6)
    cases["identical"] = (a, a.copy())
    for sigma in (1e-2, 1e-4, 1e-6):
        cases[f"line + {sigma:g}"] = line_plus_noise(sigma)
    for n_sel in (1, 2, 3, 4):
        cases[f"{n_sel} atoms"] = first_atoms(n_sel)
    return cases


ATOM_COUNTS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1005)
N_TOTAL = 1005            # 67 residues x 15 slots


def selection(n_sel, layout, B=3, seed=10):
    """(src (B,n,3), dst (B,n,3), mask (B,n)) with ``n_sel`` selected atoms per structure.  ``dense``: n = n_sel, all
    selected.  ``scattered``: n = N_TOTAL with the selection spread over the whole range (another one per structure) and
    every slot outside it NaN in source and target.  ``tail``: the same with every selected index past 256."""
    rng = np.random.default_rng(seed + n_sel)
    n = n_sel if layout == "dense" else N_TOTAL
    src, dst, mask = np.empty((B, n, 3), np.float32), np.empty((B, n, 3), np.float32), np.zeros((B, n), bool)
    for s in range(B):
        a, b = cloud(n, seed=seed + 100 * n_sel + s)
        lo = 257 if layout == "tail" else 0
        idx = np.arange(n) if layout == "dense" else lo + rng.choice(n - lo, n_sel, replace=False)
        mask[s, idx] = True
        src[s], dst[s] = a, b
    src[~mask], dst[~mask] = np.nan, np.nan
    return src, dst, mask


def topk_case(N, n_query, seed=20):
    """(xyz (N,3,3) float32, residue_mask (N,), user mask (N,), query (n_query,3)): CA atoms 3 randn * N^(1/3) so that the
    spacing of the sorted distances does not shrink with N; a fifth of the residues invalid, a quarter masked by the user."""
    rng = np.random.default_rng(seed + N + 1000 * n_query)
    xyz = _f32(3.0 * max(N, 1) ** (1 / 3) * rng.standard_normal((N, 3, 3)))
    residue_mask = rng.random(N) > 0.2
    residue_mask[0] = True
    user = rng.random(N) > 0.25
    user[0] = True
    return xyz, residue_mask, user, _f32(10.0 * rng.standard_normal((n_query, 3)))


def _batch(pairs, masks=None):
    """Stack (a, b) pairs of one size into (src (B,n,3), dst (B,n,3), mask (B,n)); masked-out slots become NaN."""
    src, dst = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    mask = np.ones(src.shape[:2], bool) if masks is None else np.stack(masks)
    src, dst = src.copy(), dst.copy()
    src[~mask], dst[~mask] = np.nan, np.nan
    return src, dst, mask


def mixed_batch(n=30):
    """A generic structure, a 2-atom selection, a collinear one and an empty mask in one batch of n atoms each."""
    generic, line = cloud(n, seed=30), collinear(n)
    two = np.zeros(n, bool)
    two[[4, 21]] = True
    return _batch([generic, cloud(n, seed=31), line, cloud(n, seed=32)],
                  [np.ones(n, bool), two, np.ones(n, bool), np.zeros(n, bool)])


def sharing_batch(B, shared_target, shared_mask, n=130, n_sel=65, seed=40):
    """B structures of n atoms with n_sel selected; one target and / or one mask for all when asked.  Under a shared mask
    with per-structure targets every array keeps NaN outside the selection; a shared target is finite only where a mask
    selects it."""
    rng = np.random.default_rng(seed + B)
    pairs = [cloud(n, seed=seed + 10 * B + s) for s in range(B)]
    masks = []
    for s in range(B):
        m = np.zeros(n, bool)
        m[rng.choice(n, n_sel, replace=False)] = True
        masks.append(m)
    if shared_mask:
        masks = [masks[0]] * B
    src, dst, mask = _batch(pairs, masks)
    if shared_target:
        dst = cloud(n, seed=seed + 7)[1][None].copy()
        dst[0, ~np.any(mask, 0)] = np.nan
    if shared_mask:
        mask = mask[:1]
    return src, dst, mask


def kabsch_batches():
    """name -> (src (B,n,3), dst (B|1,n,3), mask (B|1,n)): every batch the GPU tests hand to ops.kabsch.  The host tests
    assert the conditions of the comparisons on the same batches."""
    out = {}
    for name, (a, b) in kabsch_cases().items():
        out[name] = _batch([(a, b)])
    for n_sel in ATOM_COUNTS:
        out[f"dense {n_sel}"] = selection(n_sel, "dense")
        if n_sel < N_TOTAL:
            out[f"scattered {n_sel} of {N_TOTAL}"] = selection(n_sel, "scattered")
    for n_sel in (1, 2, 65, 300):
        out[f"tail {n_sel} past index 256"] = selection(n_sel, "tail")
    for B in (1, 3, 5):
        for shared_target in (False, True):
            for shared_mask in (False, True):
                out[f"B={B} target {'shared' if shared_target else 'own'} mask {'shared' if shared_mask else 'own'}"] = \
                    sharing_batch(B, shared_target, shared_mask)
    out["mixed"] = mixed_batch()
    out["empty mask"] = _batch([cloud(70, seed=50)] * 3, [np.zeros(70, bool)] * 3)
    return out


def structures(batch):
    """The (a (n,3), b (n,3), mask (n,)) of every structure of a batch of ``kabsch_batches``."""
    src, dst, mask = batch
    return [(src[s], dst[s if dst.shape[0] > 1 else 0], mask[s if mask.shape[0] > 1 else 0]) for s in range(src.shape[0])]


def topk_cases():
    """Dicts (xyz, residue_mask, user, query, k, use_user, label): N in {1, 255, 256, 257} with 1, 7 and 300 query points;
    k below, equal to and above the number of valid residues, with and without a user mask.  A k below the count is
    moved up to the next k whose gap between the k-th and (k+1)-th float64 distance exceeds 2 TOPK_GAP."""
    cases = []
    for N, n_query in ((1, 1), (1, 7), (255, 7), (256, 1), (256, 300), (257, 7), (257, 300)):
        xyz, residue_mask, user, query = topk_case(N, n_query)
        for use_user in (False, True):
            valid = int((residue_mask & user).sum() if use_user else residue_mask.sum())
            ks = {valid, valid + 5}
            if valid > 2:
                k = valid // 3
                while topk_mask64(xyz, residue_mask, query, k, user if use_user else None)[1] <= 2 * TOPK_GAP:
                    k += 1
                ks.add(k)
            for k in sorted(ks):
                cases.append(dict(xyz=xyz, residue_mask=residue_mask, user=user if use_user else None, query=query, k=k,
                                  label=f"N={N} queries={n_query} k={k} of {valid} valid{' user mask' if use_user else ''}"))
    return cases
