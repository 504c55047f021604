"""Host-side tests of the distance-matrix reconstruction (no GPU): the float64 model of tests/distmat_ref.py against true
geometry, the Floyd-Warshall models against scipy and against each other (bit for bit), and the argument errors raised
before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import distmat_ref as M


@pytest.mark.parametrize("L, seed", [(12, 0), (33, 1), (64, 2)])
def test_float64_model_round_trips_rigid_ideal_residues(L, seed):
    """Placements from the trRosetta geometry of rigid ideal residues recover every off-diagonal N / CA / C distance."""
    rng = np.random.default_rng(seed)
    n, ca, c, cb = M.rigid_ideal_residues(rng, 2, L)
    d_cb, omega, theta, phi = M.geometry_of(n, ca, cb)
    D, cat = M.init64(d_cb, omega, theta, phi)
    true = M.true_distmat(n, ca, c)
    off = ~np.eye(L, dtype=bool)
    err = np.abs(D - true)[:, :, :, off]
    assert not cat[:, :, :, off].all()
    assert err[~cat[:, :, :, off]].max() <= 1e-9


def test_float64_model_needs_the_trrosetta_omega():
    """With dihedral(CA_i, CB_i, CA_j, CB_j) -- the featuriser's omega -- in place of the trRosetta one, the placements
    are wrong by up to Angstroms (why the public function documents the convention)."""
    rng = np.random.default_rng(3)
    n, ca, c, cb = M.rigid_ideal_residues(rng, 1, 16)
    d_cb, _, theta, phi = M.geometry_of(n, ca, cb)
    L = n.shape[1]
    I = lambda t: np.broadcast_to(t[:, :, None, :], (1, L, L, 3))   # noqa: E731
    J = lambda t: np.broadcast_to(t[:, None, :, :], (1, L, L, 3))   # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        omega_featuriser = M.R.dihedral(I(ca), I(cb), J(ca), J(cb))
    D, cat = M.init64(d_cb, omega_featuriser, theta, phi)
    err = np.abs(D - M.true_distmat(n, ca, c))[~cat]
    assert err.max() > 0.1


@pytest.mark.parametrize("n, seed", [(5, 0), (40, 1), (97, 2)])
def test_sequential_fw_matches_scipy_on_symmetric_graphs(n, seed):
    from scipy.sparse.csgraph import floyd_warshall

    rng = np.random.default_rng(seed)
    G = M.random_graph(rng, 1, n)[0]
    G = np.minimum(G, G.T)
    ours = M.fw_sequential(torch.from_numpy(G[None]))[0].numpy()
    ref = floyd_warshall(G.astype(np.float64), directed=True)
    np.testing.assert_allclose(ours, ref, rtol=2e-6, atol=0)


@pytest.mark.parametrize("b", [3, 8, 16, 64])
@pytest.mark.parametrize("n, seed", [(7, 0), (50, 1), (150, 2)])
def test_blocked_fw_equals_sequential_bit_for_bit(n, seed, b):
    rng = np.random.default_rng(seed)
    G = np.concatenate([M.random_graph(rng, 1, n), M.random_graph(rng, 1, n, nonzero_diag=True)])
    seq = M.fw_sequential(torch.from_numpy(G)).numpy()
    blk = M.fw_blocked(G, b)
    assert np.array_equal(seq.view(np.int32), blk.view(np.int32))


def test_reconstruct_argument_errors_are_raised_before_any_launch():
    from protstruc_amd import geometry as G

    f = G.reconstruct_backbone_distmat_from_interresidue_geometry
    a = np.zeros((2, 5, 5), dtype=np.float32)
    with pytest.raises(ValueError, match="omega"):
        f(a, a[:1], a, a)
    with pytest.raises(ValueError, match="d_cb"):
        f(a[:, :, :4], a[:, :, :4], a[:, :, :4], a[:, :, :4])
    with pytest.raises(ValueError, match="mask"):
        f(a, a, a, a, mask=np.ones((2, 4, 4), dtype=bool))
    with pytest.raises(ValueError, match="outside"):
        f(a, a, a, a, chain_breaks=[5])
    with pytest.raises(ValueError, match="structures"):
        f(a, a, a, a, chain_breaks=[[1], [2], [3]])
    with pytest.raises(ValueError, match="shape"):
        f(a, a, a, a, chain_breaks=np.zeros((2, 4), dtype=bool))
    with pytest.raises(ValueError, match="lengths"):
        f(a, a, a, a, lengths=[5, 6])
    with pytest.raises(ValueError, match="lengths"):
        f(a, a, a, a, lengths=[5])


def test_ops_argument_errors_are_raised_before_any_launch():
    from protstruc_amd import ops

    a = torch.zeros(2, 5, 5)
    with pytest.raises(ValueError, match="phi"):
        ops.backbone_distmat_init(a, a, a, a[:, :4])
    with pytest.raises(ValueError, match="chain_breaks"):
        ops.backbone_distmat_init(a, a, a, a, chain_breaks=torch.zeros(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="lengths"):
        ops.backbone_distmat_init(a, a, a, a, lengths=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="D must have shape"):
        ops.floyd_warshall_(torch.zeros(2, 3, 3, 5, 5), G=1)
    with pytest.raises(ValueError, match="D must have shape"):
        ops.floyd_warshall_(torch.zeros(2, 5, 5), G=3)
    with pytest.raises(ValueError, match="G must be"):
        ops.floyd_warshall_(torch.zeros(2, 5, 5), G=0)
    with pytest.raises(ValueError, match="D must have shape"):
        ops.backbone_distmat_finish_(torch.zeros(2, 1, 1, 5, 5))
    with pytest.raises(RuntimeError, match="HIP-only"):   # CPU tensors: refused, never computed on the host
        ops.floyd_warshall_(torch.zeros(2, 5, 5))


def test_c_abi_argument_errors_return_before_any_launch():
    """Every check of the three entry points runs on the host and returns hipErrorInvalidValue (1) without touching the
    device: the pointers below are never dereferenced."""
    from protstruc_amd import _lib

    lib = _lib.load()
    fake = ctypes.c_void_p(256)   # a 16-byte aligned non-NULL address that is never read
    assert lib.ps_floyd_warshall_workspace_bytes(2, 3, 10) == 2 * 64 * (30 + 64) * 4
    assert lib.ps_floyd_warshall_workspace_bytes(1, 0, 10) == -1
    assert lib.ps_floyd_warshall_f32(None, 1, 1, 8, fake, 1 << 20, None) == 1
    assert lib.ps_floyd_warshall_f32(fake, 1, 0, 8, fake, 1 << 20, None) == 1
    assert lib.ps_floyd_warshall_f32(fake, 1, 1, 8, None, 1 << 20, None) == 1
    assert lib.ps_floyd_warshall_f32(fake, 1, 1, 8, fake, lib.ps_floyd_warshall_workspace_bytes(1, 1, 8) - 4, None) == 1
    assert lib.ps_floyd_warshall_f32(fake, 1, 1, 50000, fake, 1 << 40, None) == 1   # (G L)^2 >= 2^31
    assert lib.ps_floyd_warshall_f32(fake, 0, 1, 8, None, 0, None) == 0             # nothing to do
    assert lib.ps_backbone_distmat_init_f32(fake, fake, fake, None, None, None, None, fake, 1, 8, None) == 1
    assert lib.ps_backbone_distmat_init_f32(fake, fake, fake, fake, None, None, None, fake, 65536, 8, None) == 1
    assert lib.ps_backbone_distmat_init_f32(fake, fake, fake, fake, None, None, None, ctypes.c_void_p(258), 1, 8,
                                            None) == 1
    assert lib.ps_backbone_distmat_init_f32(fake, fake, fake, fake, None, None, None, fake, 1, 0, None) == 0
    assert lib.ps_backbone_distmat_finish_f32(None, None, None, 1, 8, None) == 1
    assert lib.ps_backbone_distmat_finish_f32(fake, None, None, 1, -1, None) == 1
    assert lib.ps_backbone_distmat_finish_f32(fake, None, None, 0, 8, None) == 0
