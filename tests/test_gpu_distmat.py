"""GPU tests of the backbone distance-matrix reconstruction: K8 (ops.backbone_distmat_init), K9 (ops.floyd_warshall_),
the finishing step and geometry.reconstruct_backbone_distmat_from_interresidue_geometry.

Yardsticks (tests/distmat_ref.py): the sequential float32 Floyd-Warshall loop and the float32 finishing step, which K9
and the whole function must equal bit for bit; the float64 model of steps 1-6 for K8, and the whole float64 pipeline
end to end.  Measured bounds, with e = |gpu - fp64| / (d_cb + 4 A) for K8 and
e = |gpu - fp64| / (value + 4 A) end to end:
  * K8 distances: e <= K8_REL;  end to end: e <= E2E_REL;
  * round trip of rigid ideal residues through the package's own featurisers: |K8 - true| <= ROUND_TRIP_A;
  * 15c8_HL, pairs of non-glycine residues: |result - true| <= PDB_A.
"""
import os

import numpy as np
import pytest
import torch

from tests import distmat_ref as M
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

LS = [1, 2, 5, 31, 64, 100, 229, 257, 512]
K8_REL = 5e-6
E2E_REL = 4e-6
ROUND_TRIP_A = 1e-4
PDB_A = 1.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


def bits_equal(a, b):
    """Equal bit for bit, NaN included (any NaN matches any NaN)."""
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    if a.shape != b.shape or not torch.equal(a.isnan(), b.isnan()):
        return False
    return torch.equal(a.nan_to_num(0.0).view(torch.int32), b.nan_to_num(0.0).view(torch.int32))


def make_inputs(rng, B, L, nan_frac=0.02, mask_frac=0.1, break_frac=0.05):
    """trRosetta geometry (float32) of B structures of L rigid ideal residues, with some NaN d_cb, a random pair mask
    and random chain breaks.  Returns (inputs dict of numpy, (n, ca, c) float64)."""
    n, ca, c, cb = M.rigid_ideal_residues(rng, B, L, spread=4.0 + 2.0 * L ** (1 / 3))
    d_cb, omega, theta, phi = (t.astype(np.float32) for t in M.geometry_of(n, ca, cb))
    d_cb[rng.random(d_cb.shape) < nan_frac] = np.nan
    mask = rng.random((B, L, L)) >= mask_frac
    breaks = rng.random((B, L)) < break_frac
    return dict(d_cb=d_cb, omega=omega, theta=theta, phi=phi, mask=mask, chain_breaks=breaks), (n, ca, c)


def cuda(inp):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if v is not None else None) for k, v in inp.items()}


def relative_errors(got, want, scale):
    return np.abs(got.astype(np.float64) - want) / (scale + 4.0)


# ---- 1. K9 against the sequential float32 loop, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("L", LS)
def test_floyd_warshall_bit_for_bit(ops, L, G):
    rng = np.random.default_rng(1000 * G + L)
    n = G * L
    nodes = np.concatenate([M.random_graph(rng, 2, n), M.random_graph(rng, 1, n, nonzero_diag=True)])
    want = M.fw_sequential(torch.from_numpy(nodes).cuda())
    D = torch.from_numpy(nodes).cuda()
    if G > 1:
        D = M.from_nodes(D, G)
    got = ops.floyd_warshall_(D, G=G)
    assert got is D
    if G > 1:
        got = M.to_nodes(got)
    assert bits_equal(got, want), f"L={L} G={G}: {(got != want).sum().item()} entries differ"


@pytest.mark.parametrize("B, L, G", [(64, 256, 3), (160, 200, 1)])
def test_floyd_warshall_bit_for_bit_beyond_residency(ops, B, L, G):
    """Batches whose panel grid (one 1024-thread workgroup per 64 columns and structure) cannot be resident at once, so
    the workgroups of one launch run in rounds: the diagonal block every panel workgroup reads must stay unchanged
    however late a workgroup starts."""
    rng = np.random.default_rng(B + L + G)
    n = G * L
    nodes = M.random_graph(rng, B, n)
    nodes[: B // 2] = M.random_graph(rng, B // 2, n, nonzero_diag=True)
    D = torch.from_numpy(nodes).cuda()
    want = M.fw_sequential(D)
    if G > 1:
        D = M.from_nodes(D, G)
    got = ops.floyd_warshall_(D, G=G)
    if G > 1:
        got = M.to_nodes(got)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        f"B={B} L={L} G={G}: {(got != want).sum().item()} entries differ"


# ---- 2. the whole function against the float32 model of steps 7-9 applied to the GPU's own K8 output ----------------
@pytest.mark.parametrize("L", LS)
def test_function_equals_model_of_steps_7_to_9(ops, L):
    from protstruc_amd import geometry as G
    rng = np.random.default_rng(L)
    inp, _ = make_inputs(rng, 3, L)
    lengths = np.array([L, max(L - 3, 0), L // 2], dtype=np.int32)
    t = cuda(inp)
    lt = torch.from_numpy(lengths).cuda()
    init = ops.backbone_distmat_init(t["d_cb"], t["omega"], t["theta"], t["phi"], t["mask"], t["chain_breaks"], lt)
    want = M.finish(M.from_nodes(M.fw_sequential(M.to_nodes(init)), 3), inp["chain_breaks"], lengths)
    got = G.reconstruct_backbone_distmat_from_interresidue_geometry(t["d_cb"], t["omega"], t["theta"], t["phi"],
                                                                     mask=t["mask"], chain_breaks=t["chain_breaks"],
                                                                     lengths=lt)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape == (3, 3, 3, L, L)
    assert bits_equal(got, want)


# ---- 3. K8 against the float64 model ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS)
def test_init_against_float64_model(ops, L):
    rng = np.random.default_rng(10 + L)
    inp, _ = make_inputs(rng, 3, L)
    lengths = np.array([L, max(L - 1, 0), (2 * L) // 3], dtype=np.int32)
    t = cuda(inp)
    got = ops.backbone_distmat_init(t["d_cb"], t["omega"], t["theta"], t["phi"], t["mask"], t["chain_breaks"],
                                    torch.from_numpy(lengths).cuda()).cpu().numpy()
    want, cat = M.init64(*(inp[k].astype(np.float64) for k in ("d_cb", "omega", "theta", "phi")), inp["mask"],
                         inp["chain_breaks"], lengths)
    assert np.array_equal(got[cat].view(np.int32), want[cat].astype(np.float32).view(np.int32)), "categorical entries"
    if (~cat).any():
        scale = np.broadcast_to(np.nan_to_num(inp["d_cb"], nan=0.0)[:, None, None], got.shape)[~cat]
        e = relative_errors(got[~cat], want[~cat], scale)
        assert e.max() <= K8_REL, f"L={L}: K8 relative error {e.max():.3e} > {K8_REL:.1e}"


# ---- 4. end to end against the float64 pipeline ------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64, 229])
def test_end_to_end_against_float64_pipeline(ops, L):
    from protstruc_amd import geometry as G
    rng = np.random.default_rng(20 + L)
    inp, _ = make_inputs(rng, 2, L, mask_frac=0.3)
    got = G.reconstruct_backbone_distmat_from_interresidue_geometry(**inp)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (2, 3, 3, L, L)
    init, _ = M.init64(*(inp[k].astype(np.float64) for k in ("d_cb", "omega", "theta", "phi")), inp["mask"],
                       inp["chain_breaks"])
    want = M.from_nodes(M.fw_sequential(M.to_nodes(torch.from_numpy(init).cuda())), 3)
    want = M.finish(want, inp["chain_breaks"]).cpu().numpy()
    assert np.isfinite(got).all()
    e = relative_errors(got, want, want)
    assert e.max() <= E2E_REL, f"L={L}: end-to-end relative error {e.max():.3e} > {E2E_REL:.1e}"


# ---- 5. round trip through the package's own featurisers ----------------------------------------------------------
def featurise(sb):
    """trRosetta d_cb, omega, theta, phi of a StructureBatch, (B, L, L) each."""
    dist, _ = sb.pairwise_distance_matrix()
    d_cb = dist[:, :, :, 4, 4].contiguous()
    omega = sb.pairwise_dihedrals(["CA", "CB"], ["CB", "CA"])
    theta = sb.pairwise_dihedrals(["N", "CA", "CB"], ["CB"])
    phi = sb.pairwise_planar_angles(["CA", "CB"], ["CB"])
    return d_cb, omega, theta, phi


@pytest.mark.parametrize("L", [12, 64, 229])
def test_round_trip_rigid_ideal_residues(ops, L):
    from protstruc_amd import StructureBatch
    rng = np.random.default_rng(30 + L)
    n, ca, c, cb = M.rigid_ideal_residues(rng, 2, L, spread=4.0 + 2.0 * L ** (1 / 3))
    xyz = np.zeros((2, L, 15, 3), dtype=np.float32)
    amask = np.zeros((2, L, 15), dtype=bool)
    for slot, atom in ((0, n), (1, ca), (2, c), (4, cb)):
        xyz[:, :, slot] = atom
        amask[:, :, slot] = True
    sb = StructureBatch.from_xyz(xyz, amask, device="cuda")
    d_cb, omega, theta, phi = featurise(sb)
    got = ops.backbone_distmat_init(d_cb, omega, theta, phi).cpu().numpy()
    true = M.true_distmat(xyz[:, :, 0].astype(np.float64), xyz[:, :, 1].astype(np.float64),
                          xyz[:, :, 2].astype(np.float64))
    _, cat = M.init64(*(t.double().cpu().numpy() for t in (d_cb, omega, theta, phi)))
    err = np.abs(got - true)[~cat]
    assert err.max() <= ROUND_TRIP_A, f"L={L}: round trip off by {err.max():.3e} A > {ROUND_TRIP_A:.1e}"


def test_pdb_15c8_sanity(ops):
    from protstruc_amd import StructureBatch
    from protstruc_amd import geometry as G
    sb = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "15c8_HL.pdb"))
    chain = sb.get_chain_idx()[0].cpu().numpy()
    L = chain.shape[0]
    ends = np.nonzero(chain[:-1] != chain[1:])[0]
    assert len(ends) == 1   # the heavy chain's last residue
    d_cb, omega, theta, phi = featurise(sb)
    got = G.reconstruct_backbone_distmat_from_interresidue_geometry(d_cb[0], omega[0], theta[0], phi[0],
                                                                     chain_breaks=[int(ends[0])]).cpu().numpy()
    assert got.shape == (3, 3, L, L) and np.isfinite(got).all()
    xyz = sb.get_xyz()[0].double().cpu().numpy()
    am = sb.get_atom_mask()[0].bool().cpu().numpy()
    has = am[:, [0, 1, 2, 4]].all(-1)   # N, CA, C and CB: not a glycine, nothing missing
    true = M.true_distmat(xyz[None, :, 0], xyz[None, :, 1], xyz[None, :, 2])[0]
    sel = np.broadcast_to((has[:, None] & has[None, :] & ~np.eye(L, dtype=bool))[None, None], got.shape)
    err = np.abs(got - true)[sel]
    assert err.max() <= PDB_A, f"15c8_HL: max |result - true| = {err.max():.3f} A > {PDB_A}"
    # the break: no peptide bond between the chains, a bond everywhere else
    i = int(ends[0])
    assert got[2, 0, i, i + 1] != np.float32(1.329) and got[2, 0, i - 1, i] == np.float32(1.329)


# ---- 6. padding, determinism, graph capture, empty inputs ---------------------------------------------------------
def test_padded_batch_equals_truncated_structures(ops):
    from protstruc_amd import geometry as G
    rng = np.random.default_rng(7)
    Lmax, lengths = 100, [100, 64, 31, 5, 1, 0]
    B = len(lengths)
    inp, _ = make_inputs(rng, B, Lmax)
    for b, n in enumerate(lengths):   # garbage beyond each length
        for k in ("d_cb", "omega", "theta", "phi"):
            inp[k][b, n:, :] = rng.normal(size=inp[k][b, n:, :].shape) * 100
            inp[k][b, :, n:] = np.nan
    t = cuda(inp)
    got = G.reconstruct_backbone_distmat_from_interresidue_geometry(
        t["d_cb"], t["omega"], t["theta"], t["phi"], mask=t["mask"], chain_breaks=t["chain_breaks"],
        lengths=torch.tensor(lengths, device="cuda")).cpu()
    for b, n in enumerate(lengths):
        one = G.reconstruct_backbone_distmat_from_interresidue_geometry(
            *(t[k][b, :n, :n] for k in ("d_cb", "omega", "theta", "phi")), mask=t["mask"][b, :n, :n],
            chain_breaks=t["chain_breaks"][b, :n]).cpu()
        assert bits_equal(got[b, :, :, :n, :n], one), f"structure {b} (length {n})"
        assert got[b, :, :, n:, :].isnan().all() and got[b, :, :, :, n:].isnan().all()


def test_deterministic(ops):
    from protstruc_amd import geometry as G
    inp, _ = make_inputs(np.random.default_rng(8), 4, 257)
    t = cuda(inp)
    runs = [G.reconstruct_backbone_distmat_from_interresidue_geometry(**t) for _ in range(3)]
    for r in runs[1:]:
        assert bits_equal(r, runs[0])


def test_graph_capture(ops):
    from protstruc_amd import geometry as G
    inp, _ = make_inputs(np.random.default_rng(9), 3, 100)
    t = cuda(inp)
    lengths = torch.tensor([100, 70, 33], device="cuda")
    f = G.reconstruct_backbone_distmat_from_interresidue_geometry
    f(**t, lengths=lengths)   # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = f(**t, lengths=lengths)
    t["d_cb"].mul_(1.25)
    t["omega"].add_(0.1)
    g.replay()
    torch.cuda.synchronize()
    assert bits_equal(captured, f(**t, lengths=lengths))


@pytest.mark.parametrize("B,L", [(0, 5), (3, 0), (0, 0)])
def test_empty(ops, B, L):
    from protstruc_amd import geometry as G
    z = torch.zeros(B, L, L, device="cuda")
    out = G.reconstruct_backbone_distmat_from_interresidue_geometry(z, z, z, z)
    assert out.shape == (B, 3, 3, L, L)
    assert ops.floyd_warshall_(torch.zeros(B, L, L, device="cuda")).shape == (B, L, L)
    one = G.reconstruct_backbone_distmat_from_interresidue_geometry(np.zeros((L, L)), np.zeros((L, L)),
                                                                     np.zeros((L, L)), np.zeros((L, L)))
    assert isinstance(one, np.ndarray) and one.shape == (3, 3, L, L)


def test_unbatched_numpy_signature(ops):
    """The reference's call: (L, L) numpy in, (3, 3, L, L) numpy out; a list of chain-break indices."""
    from protstruc_amd import geometry as G
    inp, _ = make_inputs(np.random.default_rng(11), 1, 40)
    one = {k: v[0] for k, v in inp.items() if k != "chain_breaks"}
    brk = [int(i) for i in np.nonzero(inp["chain_breaks"][0])[0]]
    got = G.reconstruct_backbone_distmat_from_interresidue_geometry(**one, chain_breaks=brk)
    want = G.reconstruct_backbone_distmat_from_interresidue_geometry(**cuda(inp))[0].cpu().numpy()
    assert isinstance(got, np.ndarray) and got.shape == (3, 3, 40, 40)
    assert bits_equal(torch.from_numpy(got), torch.from_numpy(want))
