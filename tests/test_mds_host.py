"""CPU tests of the MDS step (geometry.initialize_backbone_with_mds): the float64 model (tests/mds_ref.py) against
sklearn, the host-side start draws, the golden g16 against the model, and argument errors -- no GPU needed."""
import os

import numpy as np
import pytest
import torch

from tests import mds_ref as M
from tests.conftest import GOLDEN_DIR


def cloud_matrix(seed, n, scale=4.0):
    rng = np.random.default_rng(seed)
    P = rng.normal(scale=scale, size=(n, 3))
    return M.pdist64(P)


@pytest.mark.parametrize("seed,n,K,max_iter,eps", [(0, 30, 1, 300, 1e-6), (1, 45, 4, 300, 1e-6), (2, 12, 3, 5, 1e-6),
                                                    (3, 60, 2, 300, 1e-3), (4, 20, 1, 1, 0.0)])
def test_model_equals_sklearn(seed, n, K, max_iter, eps):
    sk = pytest.importorskip("sklearn.manifold")
    from protstruc_amd import ops
    D = cloud_matrix(seed, n)
    D = D + np.random.default_rng(seed + 100).uniform(0, 0.5, size=D.shape) * (1 - np.eye(n))
    D = (D + D.T) / 2   # not exactly Euclidean: a stress that does not go to 0
    X, s, it = sk.smacof(D, n_components=3, n_init=K, max_iter=max_iter, eps=eps, random_state=seed, return_n_iter=True)
    starts = ops.smacof_random_starts(1, K, 1, n, None, seed)[0]
    Xm, sm, im, _ = M.smacof64(D, starts, max_iter, eps)
    assert im == it
    assert abs(sm - s) <= 1e-9 * max(s, 1.0)
    np.testing.assert_allclose(Xm, X, atol=1e-8)


@pytest.mark.parametrize("kind", ["int", "RandomState", "global"])
def test_start_draws_equal_sklearn(kind):
    sk = pytest.importorskip("sklearn.manifold")
    from protstruc_amd import ops
    n, K = 18, 3
    D = cloud_matrix(9, n)
    seed = 1234

    def rs():
        if kind == "int":
            return seed
        if kind == "RandomState":
            return np.random.RandomState(seed)
        np.random.seed(seed)
        return None

    X, s, it = sk.smacof(D, n_components=3, n_init=K, max_iter=300, random_state=rs(), return_n_iter=True)
    starts = ops.smacof_random_starts(1, K, 1, n, None, rs())[0]
    Xm, sm, im, _ = M.smacof64(D, starts, 300, 1e-6)
    assert im == it
    np.testing.assert_allclose(Xm, X, atol=1e-8)
    # structure by structure, start by start, n = G lengths[b] draws each
    B, G, L, lengths = 3, 3, 5, [5, 2, 0]
    got = ops.smacof_random_starts(B, 2, G, L, lengths, np.random.RandomState(7))
    r = np.random.RandomState(7)
    for b in range(B):
        for k in range(2):
            want = r.uniform(size=3 * G * lengths[b]).reshape(G, lengths[b], 3)
            assert np.array_equal(got[b, k].reshape(G, L, 3)[:, :lengths[b]], want)
            assert not got[b, k].reshape(G, L, 3)[:, lengths[b]:].any()


def test_golden_g16_is_the_model_with_an_unconditional_mirror():
    g = np.load(os.path.join(GOLDEN_DIR, "g16_mds.npz"))
    D = M.node_matrix(g["dist_mat"])
    X, s, it, k = M.smacof64(D, g["starts"], 500, 1e-6)
    L = g["dist_mat"].shape[-1]
    coords = X.reshape(3, L, 3) * np.array([1.0, 1.0, -1.0])   # the reference mirrors whatever the hand
    want = M.finish64(coords, mirror=False)
    np.testing.assert_allclose(want, g["coords"], atol=1e-6)
    # and the result is the backbone up to a rigid motion and the hand (0.60 A: this seed's best start ends in a
    # shallow local minimum of the 48-node stress)
    assert M.kabsch_rmsd64(coords.reshape(-1, 3), g["true_backbone"].reshape(-1, 3), proper=False) < 1.0


def test_finish_model_mirrors_iff_mean_phi_positive():
    g = np.load(os.path.join(GOLDEN_DIR, "g16_mds.npz"))
    true = g["true_backbone"]
    assert M.mean_phi64(true) < 0   # a protein
    assert np.array_equal(M.fix_chirality64(true), true)
    mirrored = true * np.array([1.0, 1.0, -1.0])
    assert np.array_equal(M.fix_chirality64(mirrored), true)
    assert np.array_equal(M.fix_chirality64(mirrored, mirror=False), mirrored)


# ---- argument errors: raised on the host before anything is launched -----------------------------------------------
def test_smacof_argument_errors():
    from protstruc_amd import ops
    D = torch.zeros(2, 5, 5)
    D3 = torch.zeros(2, 3, 3, 4, 4)
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(torch.zeros(2, 5, 6))
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(torch.zeros(5, 5))
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D3, G=1)
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D3, G=2)
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, n_init=0)
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, max_iter=0)
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, eps=-1e-9)
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, eps=float("nan"))
    with pytest.raises(ValueError):   # wrong node count
        ops.check_smacof_shapes(D, init=torch.zeros(2, 4, 6, 3))
    with pytest.raises(ValueError):   # wrong batch
        ops.check_smacof_shapes(D, init=torch.zeros(1, 4, 5, 3))
    with pytest.raises(ValueError):   # K disagrees with n_init
        ops.check_smacof_shapes(D, n_init=2, init=torch.zeros(2, 4, 5, 3))
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, init=torch.zeros(2, 0, 5, 3))
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, lengths=np.array([5, 6]))
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, lengths=np.array([-1, 2]))
    with pytest.raises(ValueError):
        ops.check_smacof_shapes(D, lengths=np.array([1, 2, 3]))
    assert ops.check_smacof_shapes(D3, G=3, init=torch.zeros(2, 7, 12, 3)) == (2, 4, 7)
    assert ops.check_smacof_shapes(D) == (2, 5, 4)
    # the public entry points refuse before touching a device
    with pytest.raises(ValueError):
        ops.smacof(D, n_init=0)
    with pytest.raises(ValueError):
        ops.smacof(D, lengths=[5, 9])
    with pytest.raises(ValueError):
        ops.smacof(D, init=torch.zeros(2, 1, 5, 3), random_state=0)


def test_cpu_tensors_are_refused():
    from protstruc_amd import ops
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.smacof(torch.zeros(1, 5, 5), random_state=0)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.smacof(torch.zeros(1, 5, 5), init=torch.zeros(1, 2, 5, 3))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.mds_backbone_finish(torch.zeros(1, 3, 4, 3))


def test_geometry_argument_errors():
    from protstruc_amd import geometry as G
    with pytest.raises(TypeError):
        G.initialize_backbone_with_mds([[0.0]])
    with pytest.raises(ValueError):
        G.initialize_backbone_with_mds(np.zeros((3, 3, 4, 5)))
    with pytest.raises(ValueError):
        G.initialize_backbone_with_mds(np.zeros((2, 3, 4, 4)))
    with pytest.raises(ValueError):
        G.initialize_backbone_with_mds(np.zeros((2, 3, 3, 4, 4)), lengths=[4, 5])
    with pytest.raises(ValueError):
        G.fix_chirality(np.zeros((4, 6, 3)))
    with pytest.raises(ValueError):
        G.fix_chirality(np.zeros((2, 3, 6, 3)), lengths=[1])
    with pytest.raises(ValueError):
        from protstruc_amd import ops
        ops.check_backbone_coords_shape(torch.zeros(2, 5, 6, 3), 3)
