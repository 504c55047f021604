"""Host side of StructureBatch.from_backbone_dihedrals (no GPU): the float64 builder of tests/nerf_ref.py against the
reference's own place_fourth_atom (golden G15), its conventions, and argument validation before any launch."""
import math

import numpy as np
import pytest
import torch

from tests import nerf_ref as R
from tests.conftest import load_golden


def test_fp64_place_fourth_atom_reproduces_the_reference():
    g = {k: v.numpy() for k, v in load_golden("g15_place_fourth_atom").items()}
    x = R.place_fourth_atom(g["a"], g["b"], g["c"], g["length"], g["planar"], g["dihedral"])
    np.testing.assert_allclose(x, g["x"], rtol=0, atol=1e-9)
    xs = R.place_fourth_atom(g["a"], g["b"], g["c"], g["s_length"], g["s_planar"], g["s_dihedral"])
    np.testing.assert_allclose(xs, g["x_scalar"], rtol=0, atol=1e-9)


def test_fp64_place_fourth_atom_conventions():
    """dihedral(a, b, c, X) = dihedral and angle(X, c, b) = planar, |X - c| = length."""
    g = {k: v.numpy().astype(np.float64) for k, v in load_golden("g15_place_fourth_atom").items()}
    a, b, c = g["a"], g["b"], g["c"]
    x = R.place_fourth_atom(a, b, c, g["length"], g["planar"], g["dihedral"])
    assert np.abs(R.angle_diff(R.dihedral(a, b, c, x), g["dihedral"][:, 0])).max() < 1e-9
    assert np.abs(R.angle(x, c, b) - g["planar"][:, 0]).max() < 1e-9
    assert np.abs(np.linalg.norm(x - c, axis=-1) - g["length"][:, 0]).max() < 1e-9


def test_fp64_builder_inverts_its_angles():
    """The float64 walk reproduces every used dihedral, bond angle and bond length it was given; segments start at
    chain changes and after masked residues, whose rows are zero."""
    B, N = 2, 40
    dih = R.chain_family("random", B, N, seed=3)
    chain = np.zeros((B, N), dtype=np.float32)
    chain[0, 25:] = 1
    rmask = np.ones((B, N), dtype=bool)
    rmask[1, 10] = False
    rmask[1, 35:] = False
    xyz, mask = R.build(dih, chain, rmask, include_cb=True)
    used = R.used_angles(B, N, chain, rmask)
    n, ca, c = xyz[:, :, 0], xyz[:, :, 1], xyz[:, :, 2]
    phi = R.dihedral(c[:, :-1], n[:, 1:], ca[:, 1:], c[:, 1:])
    psi = R.dihedral(n[:, :-1], ca[:, :-1], c[:, :-1], n[:, 1:])
    omega = R.dihedral(ca[:, :-1], c[:, :-1], n[:, 1:], ca[:, 1:])
    assert R.angle_diff(phi, dih[:, 1:, 0])[used[:, 1:, 0]].max() < 1e-9
    assert R.angle_diff(psi, dih[:, :-1, 1])[used[:, :-1, 1]].max() < 1e-9
    assert R.angle_diff(omega, dih[:, :-1, 2])[used[:, :-1, 2]].max() < 1e-9
    assert not used[0, 25, 0] and not used[0, 24, 1] and not used[1, 11, 0] and not used[1, 9, 1]
    start = R.segment_starts(B, N, chain, rmask)
    for b, i in zip(*np.nonzero(start & rmask)):   # each segment starts at the ideal position
        np.testing.assert_allclose(ca[b, i], 0.0, atol=1e-12)
        assert c[b, i, 1] == 0 and c[b, i, 2] == 0 and c[b, i, 0] > 0 and n[b, i, 1] > 0 and n[b, i, 2] == 0
    assert (xyz[~rmask] == 0).all() and (mask[~rmask] == 0).all()
    assert (mask[rmask][:, [0, 1, 2, 4]] == 1).all() and (mask[rmask][:, [3] + list(range(5, 15))] == 0).all()


def test_ideal_constants():
    from protstruc_amd import geometry as G
    assert (G.IDEAL_NA, G.IDEAL_AC, G.IDEAL_C_N, G.IDEAL_NAC) == (1.458, 1.523, 1.329, 1.937)
    assert G.IDEAL_CACN == math.radians(116.2) and G.IDEAL_CNCA == math.radians(121.7)
    assert R.IDEAL_LENGTHS == (G.IDEAL_NA, G.IDEAL_AC, G.IDEAL_C_N)
    assert R.IDEAL_ANGLES == (G.IDEAL_NAC, G.IDEAL_CACN, G.IDEAL_CNCA)


@pytest.mark.parametrize("kwargs", [
    dict(dihedrals=np.zeros((2, 5))),                                          # no angle axis
    dict(dihedrals=np.zeros((2, 5, 2))),                                       # two angles
    dict(dihedrals=np.zeros((5, 3))),                                          # no batch axis
    dict(dihedrals=np.zeros((2, 5, 3)), chain_idx=np.zeros((2, 4)), chain_ids=[["A"], ["A"]]),
    dict(dihedrals=np.zeros((2, 5, 3)), residue_mask=np.ones((1, 5), dtype=bool)),
    dict(dihedrals=np.zeros((2, 5, 3)), bond_angles=np.zeros((2, 5))),
    dict(dihedrals=np.zeros((2, 5, 3)), bond_lengths=np.zeros((2, 6, 3))),
    dict(dihedrals=np.zeros((2, 5, 3)), chain_idx=np.zeros((2, 5))),           # chain_idx without chain_ids
    dict(dihedrals=np.zeros((2, 5, 3)), chain_ids=[["A"], ["A"]]),             # chain_ids without chain_idx
])
def test_from_backbone_dihedrals_validates_before_launch(kwargs):
    """Shape errors and the chain_idx / chain_ids rule raise ValueError on the host, before any device work (this
    machine may have no GPU at all)."""
    from protstruc_amd import StructureBatch
    with pytest.raises(ValueError):
        StructureBatch.from_backbone_dihedrals(**kwargs)


def test_op_validates_shapes_before_device_checks():
    from protstruc_amd import ops
    with pytest.raises(ValueError, match="dihedrals"):
        ops.backbone_from_dihedrals(torch.zeros(2, 5, 4))
    with pytest.raises(ValueError, match="bond_lengths"):
        ops.backbone_from_dihedrals(torch.zeros(2, 5, 3), bond_lengths=torch.zeros(2, 5, 2))
    with pytest.raises(ValueError, match="n_slots"):
        ops.backbone_from_dihedrals(torch.zeros(2, 5, 3), include_cb=True, n_slots=4)


def test_from_dihedrals_is_still_the_reference_stub():
    from protstruc_amd import StructureBatch
    with pytest.raises(NotImplementedError, match="TODO"):
        StructureBatch.from_dihedrals(np.zeros((1, 4, 3)))
