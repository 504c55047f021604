"""Closest-atom residue distances without a GPU: the float64 restatement tests/closest_ref.py against an independent brute
force, its tie and mirror rules by hand, the entry points of include/protstruc_contacts.h,
the argument checks of the launchers and of the shell, and the contact maps, interface residues and Fnat of a complex in
numpy -- the values tests/test_gpu_closest.py holds StructureBatch to."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import closest_ref as R
from tests.c_headers import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


# ---- the restatement against a brute force ---------------------------------------------------------------------------------------
def random_case(seed, B=2, N=9, A=5):
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(size=(B, N, A, 3)) * 4.0).astype(np.float32)
    mask = rng.random((B, N, A)) >= 0.3
    mask[0, 2] = False                      # a residue without atoms
    xyz[~mask] = np.nan
    return xyz, mask


def brute_d2(x64, mask):
    """(B,N,N,A,A) float64 squared distances, +inf where either atom is masked: torch, on the gathered tensor"""
    X = torch.where(mask[..., None], x64, torch.zeros_like(x64))
    d = X[:, None, :, None, :, :] - X[:, :, None, :, None, :]        # [b, i, j, a, c]: atom c of j minus atom a of i
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    both = mask[:, :, None, :, None] & mask[:, None, :, None, :]
    return torch.where(both, d2, torch.full_like(d2, math.inf))


@pytest.mark.parametrize("cutoff", (math.inf, 6.0))
def test_restatement_against_a_brute_force(cutoff):
    xyz, mask = random_case(1)
    B, N, A = mask.shape
    dist, pair = R.forward(xyz, mask, cutoff)
    d2 = brute_d2(torch.from_numpy(xyz).double(), torch.from_numpy(mask)).reshape(B, N, N, A * A)
    low, at = d2.min(dim=-1)
    counts = torch.isfinite(low) & (low <= float(np.float32(cutoff)) ** 2)
    want = torch.where(counts, low.sqrt(), torch.full_like(low, math.inf)).float().numpy()
    assert np.array_equal(dist.view(np.int32), want.view(np.int32)), "dist differs in its bits"
    off = ~np.eye(N, dtype=bool)[None] & np.ones((B, 1, 1), dtype=bool)     # the diagonal is all ties: checked below
    ties = (d2 == low[..., None]).sum(-1).numpy()
    assert (ties[off & np.isfinite(low.numpy())] == 1).all(), "the random case is meant to have no ties off the diagonal"
    assert np.array_equal(pair[off], torch.where(counts, at, torch.full_like(at, -1)).numpy().astype(np.int16)[off])
    lowest = np.where(mask.any(-1), mask.argmax(-1), -1)
    diagonal = pair[:, np.arange(N), np.arange(N)]
    assert np.array_equal(diagonal, np.where(lowest >= 0, lowest * A + lowest, -1))
    assert np.array_equal(dist[:, np.arange(N), np.arange(N)], np.where(lowest >= 0, 0.0, np.inf).astype(np.float32))
    assert (pair[0, 2] == -1).all() and (pair[0, :, 2] == -1).all() and np.isinf(dist[0, 2]).all()
    # exactly symmetric, the pair with its atoms exchanged
    assert np.array_equal(dist, dist.transpose(0, 2, 1))
    swapped = np.where(pair >= 0, (pair % A) * A + pair // A, -1)
    assert np.array_equal(pair, swapped.transpose(0, 2, 1))


def test_restatement_gradient_against_autograd():
    xyz, mask = random_case(2)
    B, N, A = mask.shape
    rng = np.random.default_rng(3)
    g = rng.normal(size=(B, N, N)).astype(np.float32)
    dist, pair = R.forward(xyz, mask, 7.0)
    grad, S = R.backward(xyz, pair, g)
    x64 = torch.from_numpy(np.nan_to_num(xyz)).double().requires_grad_(True)
    low = brute_d2(x64, torch.from_numpy(mask)).reshape(B, N, N, A * A).amin(dim=-1)
    use = torch.from_numpy(np.isfinite(dist) & ~np.eye(N, dtype=bool)[None])
    d = torch.where(use, low, torch.ones_like(low)).sqrt()
    (torch.where(use, d, torch.zeros_like(d)) * torch.from_numpy(g).double()).sum().backward()
    want = x64.grad.numpy()
    assert np.abs(want).max() > 0.5 and np.abs(grad - want).max() <= 1e-9
    assert (grad[~mask] == 0).all() and (S >= np.abs(grad) - 1e-12).all()
    # out-of-range pairs are "none"
    wild = pair.astype(np.int64)
    wild[0, 0, 1], wild[0, 1, 0] = A * A, -7
    g2, _ = R.backward(xyz, wild, g)
    none = pair.copy()
    none[0, 0, 1] = none[0, 1, 0] = -1
    assert np.array_equal(g2, R.backward(xyz, none, g)[0])


def test_ties_and_mirror_by_hand():
    """Two residues of three slots on a lattice.  Residue 0: slots 0, 1 at (0,0,0), (0,0,1); slot 2 masked, at (2,0,0) --
    it would win.  Residue 1: slots 0, 1, 2 at (3,0,1), (3,0,0), (3,0,1).  d2 = 9 three times over: (a,c) = (0,1), (1,0),
    (1,2); the order (d2, a, c) picks (0,1).  The mirror entry reads (1,0) -- residue 1's slot first -- although a sweep
    from residue 1's side would have found its slot 0 first, (0,1)."""
    xyz = np.array([[[[0, 0, 0], [0, 0, 1], [2, 0, 0]], [[3, 0, 1], [3, 0, 0], [3, 0, 1]]]], dtype=np.float32)
    mask = np.array([[[1, 1, 0], [1, 1, 1]]], dtype=bool)
    dist, pair = R.forward(xyz, mask)
    assert dist.tolist() == [[[0.0, 3.0], [3.0, 0.0]]]
    assert pair.tolist() == [[[0 * 3 + 0, 0 * 3 + 1], [1 * 3 + 0, 0 * 3 + 0]]]
    for cutoff, counts in ((3.0, True), (np.nextafter(np.float32(3.0), np.float32(0)), False), (0.0, False)):
        dist, pair = R.forward(xyz, mask, cutoff)
        assert (dist[0, 0, 1] == 3.0) == counts and (pair[0, 0, 1] == 1) == counts and pair[0, 1, 0] == (3 if counts else -1)
        assert dist[0, 0, 0] == 0.0 and pair[0, 1, 1] == 0, "the diagonal counts at any cutoff"
    # the gradient goes to the recorded atoms only: slot 0 of residue 0 is pulled along -x by g[0,1] + g[1,0]
    g = np.array([[[9.0, 2.0], [0.5, 9.0]]], dtype=np.float32)
    grad, S = R.backward(xyz, R.forward(xyz, mask)[1], g)
    assert grad[0, 0].tolist() == [[-2.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert grad[0, 1].tolist() == [[0.0, 0.0, 0.0], [2.5, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert S[0, 0, 0].tolist() == [2.5, 0.0, 0.0]


def test_lattice_case_has_the_boundary_on_both_sides():
    xyz, mask = R.lattice_case()
    free = R.forward(xyz, mask)[0]
    dist, pair = R.forward(xyz, mask, 5.0)
    assert (free == np.float32(5.0)).sum() >= 20 and (free == np.float32(np.sqrt(26.0))).sum() >= 20
    assert np.array_equal(np.isfinite(dist), free <= 5.0) and ((pair >= 0) == np.isfinite(dist)).all()


# ---- the header (tests/test_api_families.py holds it to the binding and the library) ------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from protstruc_amd import _lib, build
    build.build(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_the_entry_points_of_the_header():
    from protstruc_amd import build
    assert declared_symbols("protstruc_contacts.h") == ["ps_closest_atoms_backward_f32", "ps_closest_atoms_f32", "ps_contacts_api"]
    assert "closest_atoms.hip" in {os.path.basename(d) for d in build._deps()}


def test_arguments_are_checked_before_any_launch(lib):
    """hipErrorInvalidValue (1) without touching a device; B = 0 returns 0 (the pointers are never dereferenced)."""
    fake = ctypes.c_void_p(0x1000)
    inf = math.inf

    def forward(xyz=fake, B=1, N=4, A=15, cutoff=inf):
        return lib.ps_closest_atoms_f32(xyz, None, fake, fake, B, N, A, cutoff, None)

    def backward(xyz=fake, B=1, N=4, A=15):
        return lib.ps_closest_atoms_backward_f32(xyz, fake, fake, fake, B, N, A, None)

    assert forward(B=0) == 0 and backward(B=0) == 0 and forward(B=0, cutoff=0.0) == 0
    for bad in (dict(xyz=None), dict(A=0), dict(A=65), dict(B=65536), dict(B=-1), dict(N=0), dict(cutoff=-1.0),
                dict(cutoff=math.nan), dict(cutoff=-inf), dict(B=0, A=65), dict(B=0, cutoff=math.nan)):
        assert forward(**bad) == 1, bad
    for bad in (dict(xyz=None), dict(A=0), dict(A=65), dict(B=65536), dict(N=0)):
        assert backward(**bad) == 1, bad
    assert lib.ps_closest_atoms_f32(fake, None, None, fake, 1, 4, 15, inf, None) == 1
    assert lib.ps_closest_atoms_f32(fake, None, fake, None, 1, 4, 15, inf, None) == 1
    assert lib.ps_closest_atoms_backward_f32(fake, None, fake, fake, 1, 4, 15, None) == 1


def test_shape_checks_of_the_shell():
    from protstruc_amd import ops
    check = ops.check_closest_atoms_shapes
    xyz, mask = torch.zeros(2, 5, 4, 3), torch.ones(2, 5, 4, dtype=torch.bool)
    pair, g = torch.zeros(2, 5, 5, dtype=torch.int16), torch.zeros(2, 5, 5)
    check(xyz, mask, 5.0), check(xyz, None, math.inf), check(xyz.double(), mask.float(), 0.0, pair.long(), g.double())
    for bad in (dict(xyz=torch.zeros(2, 5, 4)), dict(xyz=torch.zeros(2, 5, 4, 2)), dict(xyz=torch.zeros(2, 5, 4, 3, dtype=torch.int32)),
                dict(xyz=torch.zeros(2, 5, 65, 3), atom_mask=None), dict(xyz=torch.zeros(2, 5, 0, 3), atom_mask=None),
                dict(xyz=torch.zeros(2, 0, 4, 3), atom_mask=None), dict(atom_mask=mask[:, :4]), dict(atom_mask=mask[..., :3]),
                dict(cutoff=-1.0), dict(cutoff=math.nan), dict(cutoff=-math.inf), dict(pair=pair[:, :4]), dict(pair=g),
                dict(grad_dist=g[:, :, :4]), dict(grad_dist=pair)):
        with pytest.raises(ValueError):
            check(**{**dict(xyz=xyz, atom_mask=mask, cutoff=5.0), **bad})
    for call in (lambda: ops.closest_atoms(xyz), lambda: ops.closest_atoms_backward(xyz, pair, g)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- a complex: contact map, interface, Fnat ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def complex_1a3r():
    """(xyz (N,A,3), present (N,A), chain (N,)) of tests/golden/1a3r_HL.pdb and the yardstick's dist at 5 A and without a cutoff"""
    from protstruc_amd import StructureBatch
    batch = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "1a3r_HL.pdb"), device="cpu")
    xyz, present = batch.get_xyz().numpy(), batch._present_atoms().numpy()
    chain = batch._chain_keys().numpy()[0]
    at5 = R.forward(xyz, present, 5.0)[0][0]
    free = R.forward(xyz, present)[0][0]
    return xyz, present, chain, at5, free


def test_contacts_interface_and_fnat_of_a_complex():
    xyz, present, chain, at5, free = complex_1a3r()
    N = chain.shape[0]
    assert set(chain.tolist()) == {0, 1} and present.any(-1).all()
    assert np.array_equal(np.isfinite(at5), free <= np.float32(5.0)) and np.array_equal(at5[np.isfinite(at5)], free[np.isfinite(at5)])
    contact = R.contacts(at5, chain)
    assert not contact.diagonal().any() and np.array_equal(contact, contact.T)
    bonded = np.flatnonzero(chain[:-1] == chain[1:])
    assert contact[bonded, bonded + 1].all(), "covalently bonded neighbours touch"
    assert not R.contacts(at5, chain, min_separation=2)[bonded, bonded + 1].any()
    assert 3 * N < contact.sum() // 2 < 12 * N, "a globular protein: a handful of contacts per residue"
    across = R.contacts(at5, chain, other_chains_only=True)
    assert np.array_equal(across, contact & (chain[:, None] != chain[None, :]))
    face = R.interface(at5, chain)
    assert 10 <= face.sum() <= 120 and face[chain == 0].any() and face[chain == 1].any()
    assert R.fnat(at5, at5, chain) == (np.float32(1.0), int(across.sum()) // 2)
    moved = xyz.copy()
    moved[0, chain == 1] += np.array([30.0, 0.0, 0.0], dtype=np.float32)      # one chain translated by 30 A
    gone, n = R.fnat(R.forward(moved, present, 5.0)[0][0], at5, chain)
    assert gone == 0.0 and n == int(across.sum()) // 2 > 0
    one_chain = np.zeros_like(chain)
    assert np.isnan(R.fnat(at5, at5, one_chain)[0]) and R.fnat(at5, at5, one_chain)[1] == 0


def test_structure_batch_refuses_another_layout():
    from protstruc_amd import StructureBatch
    xyz = torch.zeros(1, 6, 4, 3)
    chain = torch.tensor([[0.0, 0, 0, 1, 1, 1]])
    batch = StructureBatch(xyz, chain_idx=chain, chain_ids=[["A", "B"]], device="cpu")
    other = StructureBatch(xyz, chain_idx=torch.tensor([[0.0, 0, 1, 1, 1, 1]]), chain_ids=[["A", "B"]], device="cpu")
    with pytest.raises(ValueError, match="chain layout"):
        batch.fraction_native_contacts(other)
    with pytest.raises(ValueError, match="shape"):
        batch.fraction_native_contacts(StructureBatch(xyz[:, :5], device="cpu"))
    with pytest.raises(ValueError, match="min_separation"):
        batch.residue_contacts(min_separation=-1)
