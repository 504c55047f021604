"""GPU tests of the MDS step: K10 (ops.smacof), K11 (ops.mds_backbone_finish), geometry.initialize_backbone_with_mds
and geometry.fix_chirality.

Yardsticks: the float64 model of tests/mds_ref.py, run from the same float32 starts.  Bounds, with the value measured
on the MI355X:
  * fixed start, eps = 0, max_iter <= 50: max |X - X64| / max |X64| <= X_REL (measured 1.8e-7) and
    |sigma - sigma64| / sigma64 <= S_REL (measured 6.6e-8);
  * sigma does not grow from one pass to the next by more than MONO_REL, relative (measured: it never grows);
  * golden g16 from its own starts: |result - reference| <= G16_A (measured 1.6e-5 A), after undoing the reference's
    unconditional mirror where ours does not mirror; O / CB placed from the golden's N / CA / C: <= PLACE_A (2.4e-6 A);
  * 15c8_HL, exact distances, random_state = 0: proper-rotation RMSD <= RMSD_EXACT_A (measured 0.109 A; sklearn 0.109 A);
  * 15c8_HL end to end (trRosetta geometry with ideal CB -> reconstruct -> MDS): proper RMSD <= RMSD_E2E_A (measured
    0.130 A), stress <= STRESS_E2E x the model's from the same starts (measured 1.00001 x).
"""
import os

import numpy as np
import pytest
import torch

from tests import distmat_ref as DM
from tests import mds_ref as M
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

X_REL = 7e-7
S_REL = 2.5e-7
MONO_REL = 1e-7
G16_A = 6e-5
PLACE_A = 1e-5
RMSD_EXACT_A = 0.25
RMSD_E2E_A = 4.5
STRESS_E2E = 1.001

LS = [1, 2, 5, 31, 64, 100, 229, 257, 512]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


def bits_equal(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    if a.shape != b.shape or not torch.equal(a.isnan(), b.isnan()):
        return False
    if a.dtype == torch.float64:
        return torch.equal(a.nan_to_num(0.0).view(torch.int64), b.nan_to_num(0.0).view(torch.int64))
    if a.dtype == torch.float32:
        return torch.equal(a.nan_to_num(0.0).view(torch.int32), b.nan_to_num(0.0).view(torch.int32))
    return torch.equal(a, b)


def structure_matrix(seed, G, L):
    """Exact distances of a structure: G = 1 a random point cloud (L points), G = 3 rigid ideal residues (N, CA, C).
    Returns (D (G, G, L, L) float32 in the node layout, points (G L, 3) float64)."""
    rng = np.random.default_rng(seed)
    if G == 1:
        P = rng.normal(scale=2.0 + L ** (1 / 3), size=(L, 3))
        return M.pdist64(P).astype(np.float32)[None, None], P
    n, ca, c, _ = DM.rigid_ideal_residues(rng, 1, L, spread=4.0 + 2.0 * L ** (1 / 3))
    P = np.concatenate([n[0], ca[0], c[0]], 0)
    return M.pdist64(P).reshape(3, L, 3, L).transpose(0, 2, 1, 3).astype(np.float32), P


def noisy(D, G, amp, seed):
    """D plus symmetric uniform noise in [0, amp) off the diagonal (in the node layout)."""
    L = D.shape[-1]
    A = M.node_matrix(D) if G == 3 else D[0, 0].astype(np.float64)
    E = np.triu(np.random.default_rng(seed).uniform(0, amp, size=A.shape), 1)
    A = (A + E + E.T).astype(np.float32)
    return A.reshape(G, L, G, L).transpose(0, 2, 1, 3).copy()


def starts_for(seed, K, n):
    return np.random.RandomState(seed).uniform(size=(K, n, 3)).astype(np.float32)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, D, G, starts, max_iter, eps, lengths=None):
    """ops.smacof on (B, G, G, L, L) numpy D and (B, K, G L, 3) numpy starts -> numpy X, stress, n_iter."""
    X, s, it = ops.smacof(cuda(D), G, init=cuda(starts), max_iter=max_iter, eps=eps,
                          lengths=None if lengths is None else cuda(np.asarray(lengths, dtype=np.int32)))
    return X.cpu().numpy(), s.cpu().numpy(), it.cpu().numpy()


# ---- 1. from a given start, eps = 0: X and sigma against the model -------------------------------------------------
@pytest.mark.parametrize("G,L", [(1, 50), (3, 24)])
@pytest.mark.parametrize("max_iter", [1, 2, 10, 50])
def test_fixed_start_matches_model(ops, G, L, max_iter):
    D, _ = structure_matrix(11 + G, G, L)
    D = noisy(D, G, 0.3, 5)
    x0 = starts_for(3, 1, G * L)
    X, s, it = run(ops, D[None], G, x0[None], max_iter, 0.0)
    Xm, sm, im = M.smacof_single64(M.node_matrix(D) if G == 3 else D[0, 0].astype(np.float64), x0[0].astype(np.float64),
                                   max_iter, 0.0)
    assert it[0] == im == max_iter
    xerr = np.abs(X[0] - Xm).max() / np.abs(Xm).max()
    serr = abs(s[0] - sm) / sm
    print(f"G={G} L={L} max_iter={max_iter}: X rel {xerr:.2e}, sigma rel {serr:.2e}")
    assert xerr <= X_REL and serr <= S_REL


def test_stress_does_not_increase(ops):
    D, _ = structure_matrix(4, 3, 40)
    x0 = starts_for(8, 1, 120)
    prev = None
    worst = 0.0
    for m in range(1, 31):
        _, s, _ = run(ops, D[None], 3, x0[None], m, 0.0)
        if prev is not None:
            worst = max(worst, (s[0] - prev) / prev)
        prev = s[0]
    print(f"largest relative growth of sigma between passes: {worst:.2e}")
    assert worst <= MONO_REL


# ---- 2. n_iter equals the model's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("L", LS)
def test_n_iter_matches_model(ops, G, L):
    D, _ = structure_matrix(100 + L, G, L)
    x0 = starts_for(L, 1, G * L)
    X, s, it = run(ops, D[None], G, x0[None], 300, 1e-5)
    Dm = M.node_matrix(D) if G == 3 else D[0, 0].astype(np.float64)
    Xm, sm, im = M.smacof_single64(Dm, x0[0].astype(np.float64), 300, 1e-5)
    print(f"G={G} L={L}: n_iter gpu {it[0]} model {im}; stress gpu {s[0]:.6g} model {sm:.6g}")
    assert it[0] == im


def test_ragged_and_empty_batches(ops):
    G, L = 3, 20
    lengths = [20, 13, 0, 1, 7]
    D = np.full((len(lengths), G, G, L, L), np.nan, dtype=np.float32)
    starts = np.full((len(lengths), 2, G * L, 3), np.nan, dtype=np.float32)
    for b, ln in enumerate(lengths):
        if ln:
            Db, _ = structure_matrix(200 + b, G, ln)
            D[b, :, :, :ln, :ln] = Db
            s0 = starts_for(b, 2, G * ln).reshape(2, G, ln, 3)
            starts[b].reshape(2, G, L, 3)[:, :, :ln] = s0
    X, s, it = run(ops, D, G, starts, 300, 1e-5, lengths)
    for b, ln in enumerate(lengths):
        Xb = X[b].reshape(G, L, 3)
        assert np.isnan(Xb[:, ln:]).all()
        if ln == 0:
            assert it[b] == 0 and s[b] == 0.0
            continue
        Dm = M.node_matrix(D[b, :, :, :ln, :ln])
        s0 = starts[b].reshape(2, G, L, 3)[:, :, :ln].reshape(2, G * ln, 3).astype(np.float64)
        _, sm, im, _ = M.smacof64(Dm, s0, 300, 1e-5)
        assert it[b] == im and np.isfinite(Xb[:, :ln]).all()
    Xe, se, ie = ops.smacof(torch.zeros(0, 3, 3, 4, 4, device="cuda"), 3, random_state=0)
    assert Xe.shape == (0, 12, 3) and se.shape == (0,) and ie.shape == (0,)
    Xz, sz, iz = ops.smacof(torch.zeros(2, 0, 0, device="cuda"), random_state=0)
    assert Xz.shape == (2, 0, 3) and (iz.cpu() == 0).all() and (sz.cpu() == 0).all()


# ---- 3. start independence --------------------------------------------------------------------------------------------
def test_best_start_equals_its_own_single_run(ops):
    G, L = 3, 30
    D, P = structure_matrix(31, G, L)
    D = noisy(D, G, 0.4, 6)   # not Euclidean: the starts end at different stresses
    starts = starts_for(17, 4, G * L)
    X4, s4, i4 = run(ops, D[None], G, starts[None], 200, 1e-6)
    singles = [run(ops, D[None], G, starts[k][None, None], 200, 1e-6) for k in range(4)]
    stresses = [r[1][0] for r in singles]
    best = min(range(4), key=lambda k: (stresses[k], k))
    assert bits_equal(X4, singles[best][0]) and bits_equal(s4, singles[best][1]) and i4[0] == singles[best][2][0]
    # the truth as one of the starts always wins
    D, P = structure_matrix(32, G, L)
    starts[2] = P.astype(np.float32)
    X4, s4, _ = run(ops, D[None], G, starts[None], 200, 1e-6)
    Xt, st, _ = run(ops, D[None], G, starts[2][None, None], 200, 1e-6)
    assert bits_equal(X4, Xt) and bits_equal(s4, st)


# ---- 4. padding and NaN ---------------------------------------------------------------------------------------------
def test_ragged_batch_equals_cropped_runs_and_nan_is_contained(ops):
    G, L = 3, 40
    lengths = [40, 33, 9]
    D = np.zeros((3, G, G, L, L), dtype=np.float32)
    starts = np.zeros((3, 3, G * L, 3), dtype=np.float32)
    rng = np.random.default_rng(3)
    D[...] = rng.uniform(0, 50, size=D.shape)   # padding garbage: never read
    crops = []
    for b, ln in enumerate(lengths):
        Db, _ = structure_matrix(300 + b, G, ln)
        D[b, :, :, :ln, :ln] = Db
        s0 = starts_for(40 + b, 3, G * ln)
        starts[b].reshape(3, G, L, 3)[:, :, :ln] = s0.reshape(3, G, ln, 3)
        crops.append((Db, s0))
    X, s, it = run(ops, D, G, starts, 150, 1e-6, lengths)
    for b, ln in enumerate(lengths):
        Xc, sc, ic = run(ops, crops[b][0][None], G, crops[b][1][None], 150, 1e-6)
        assert bits_equal(X[b].reshape(G, L, 3)[:, :ln], Xc[0].reshape(G, ln, 3))
        assert bits_equal(s[b], sc[0]) and it[b] == ic[0]
    D2 = D.copy()
    D2[1, 0, 1, 3, 5] = np.nan
    X2, s2, it2 = run(ops, D2, G, starts, 150, 1e-6, lengths)
    assert np.isnan(s2[1])
    for b in (0, 2):
        assert bits_equal(X2[b], X[b]) and bits_equal(s2[b], s[b]) and it2[b] == it[b]


# ---- 5. determinism and graph capture ---------------------------------------------------------------------------------
def test_deterministic_and_graph_capture(ops):
    G, L, B = 3, 64, 4
    D = np.stack([structure_matrix(400 + b, G, L)[0] for b in range(B)])
    starts = np.stack([starts_for(50 + b, 4, G * L) for b in range(B)])
    Dd, sd = cuda(D), cuda(starts)
    a = ops.smacof(Dd, G, init=sd, max_iter=120, eps=1e-6)
    b = ops.smacof(Dd, G, init=sd, max_iter=120, eps=1e-6)
    assert all(bits_equal(x, y) for x, y in zip(a, b))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.smacof(Dd, G, init=sd, max_iter=120, eps=1e-6)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.smacof(Dd, G, init=sd, max_iter=120, eps=1e-6)
    g.replay()
    torch.cuda.synchronize()
    assert all(bits_equal(x, y) for x, y in zip(out, a))


# ---- 6. / 7. 15c8_HL ------------------------------------------------------------------------------------------------------
def backbone_15c8():
    from protstruc_amd import StructureBatch
    sb = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "15c8_HL.pdb"))
    xyz = sb.get_xyz()[0].double().cpu().numpy()
    chain = sb.get_chain_idx()[0].cpu().numpy()
    return np.stack([xyz[:, 0], xyz[:, 1], xyz[:, 2]]), chain   # (3, L, 3)


def test_15c8_exact_distances_right_hand(ops):
    from protstruc_amd import geometry as G
    true, _ = backbone_15c8()
    L = true.shape[1]
    dist = DM.true_distmat(true[0][None], true[1][None], true[2][None])[0]
    out = G.initialize_backbone_with_mds(dist, random_state=0)
    assert out.shape == (5, L, 3) and isinstance(out, np.ndarray)
    rmsd = M.kabsch_rmsd64(out[:3].reshape(-1, 3), true.reshape(-1, 3), proper=True)
    print(f"15c8_HL exact distances: proper RMSD {rmsd:.4f} A")
    assert rmsd <= RMSD_EXACT_A
    assert M.mean_phi64(out[:3].astype(np.float64)) < 0


def test_15c8_end_to_end(ops):
    from protstruc_amd import StructureBatch
    from protstruc_amd import geometry as G
    true, chain = backbone_15c8()
    L = true.shape[1]
    cb = M.place4_64(true[2], true[0], true[1], M.AB, M.NAB, M.BANC)   # ideal CB, glycines included
    xyz = np.zeros((1, L, 15, 3), dtype=np.float32)
    amask = np.zeros((1, L, 15), dtype=bool)
    for slot, atom in ((0, true[0]), (1, true[1]), (2, true[2]), (4, cb)):
        xyz[0, :, slot] = atom
        amask[0, :, slot] = True
    sb = StructureBatch.from_xyz(xyz, amask, device="cuda")
    dist, _ = sb.pairwise_distance_matrix()
    d_cb = dist[:, :, :, 4, 4].contiguous()
    omega = sb.pairwise_dihedrals(["CA", "CB"], ["CB", "CA"])
    theta = sb.pairwise_dihedrals(["N", "CA", "CB"], ["CB"])
    phi = sb.pairwise_planar_angles(["CA", "CB"], ["CB"])
    ends = np.nonzero(chain[:-1] != chain[1:])[0]
    dm = G.reconstruct_backbone_distmat_from_interresidue_geometry(d_cb[0], omega[0], theta[0], phi[0],
                                                                    chain_breaks=[int(e) for e in ends])
    out = G.initialize_backbone_with_mds(dm, random_state=0)
    assert out.shape == (5, L, 3) and torch.is_tensor(out)
    rmsd = M.kabsch_rmsd64(out[:3].cpu().numpy().reshape(-1, 3), true.reshape(-1, 3), proper=True)
    X, s, it = ops.smacof(dm[None], 3, random_state=0, max_iter=500)
    starts = ops.smacof_random_starts(1, 4, 3, L, None, 0)[0].astype(np.float32).astype(np.float64)
    _, sm, im, _ = M.smacof64(M.node_matrix(dm.cpu().numpy()), starts, 500, 1e-6)
    print(f"15c8_HL end to end: proper RMSD {rmsd:.3f} A; stress gpu {s.item():.6g} model {sm:.6g} "
          f"(n_iter {it.item()} / {im})")
    assert rmsd <= RMSD_E2E_A
    assert s.item() <= STRESS_E2E * sm


# ---- 8. golden g16 ----------------------------------------------------------------------------------------------------
def test_golden_placement(ops):
    g = np.load(os.path.join(GOLDEN_DIR, "g16_mds.npz"))
    ref = g["coords"]
    out = ops.mds_backbone_finish(cuda(ref[:3].astype(np.float32))[None], mirror=False)[0].cpu().numpy()
    err = np.abs(out[3:] - ref[3:]).max()
    print(f"g16 O / CB from the golden's N / CA / C: {err:.2e} A")
    assert np.array_equal(out[:3], ref[:3].astype(np.float32))
    assert err <= PLACE_A


def test_golden_full_function(ops):
    from protstruc_amd import geometry as G
    g = np.load(os.path.join(GOLDEN_DIR, "g16_mds.npz"))
    L = g["dist_mat"].shape[-1]
    out = G.initialize_backbone_with_mds(g["dist_mat"], init=g["starts"])
    assert out.shape == (5, L, 3)
    ref_bb = g["coords"][:3]
    ours_mirrored = M.mean_phi64(ref_bb * np.array([1.0, 1.0, -1.0])) > 0   # the hand SMACOF itself produced
    want = M.finish64(ref_bb if ours_mirrored else ref_bb * np.array([1.0, 1.0, -1.0]), mirror=False)
    err = np.abs(out - want).max()
    print(f"g16 full function (mirrored: {ours_mirrored}): {err:.2e} A")
    assert err <= G16_A


# ---- 9. fix_chirality -------------------------------------------------------------------------------------------------
def test_fix_chirality(ops):
    from protstruc_amd import geometry as G
    true, _ = backbone_15c8()
    x = true.astype(np.float32)
    assert M.mean_phi64(true) < 0
    out = G.fix_chirality(x)
    assert np.array_equal(out.view(np.int32), x.view(np.int32))
    mirror = x * np.array([1, 1, -1], dtype=np.float32)
    back = G.fix_chirality(torch.from_numpy(mirror).cuda()).cpu().numpy()
    assert np.array_equal(back.view(np.int32), x.view(np.int32))
    # batched, ragged, NaN contained to its structure
    L = x.shape[1]
    batch = np.stack([x, mirror, x]).copy()
    batch[2, 1, 5, 0] = np.nan
    outb = G.fix_chirality(batch, lengths=[L, L, L])
    assert np.array_equal(outb[0], x) and np.array_equal(outb[1], x) and np.isnan(outb[2]).all()
    outr = G.fix_chirality(batch[:2], lengths=[L, 10])
    assert np.isnan(outr[1][:, 10:]).all()
    assert np.array_equal(outr[1][:, :10], G.fix_chirality(mirror[:, :10]))
