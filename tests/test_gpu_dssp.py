"""GPU tests of DSSP (ps_backbone_hbonds_f32, ps_dssp_assign; ops.backbone_hbonds, ops.dssp_assign;
geometry.backbone_hbonds, geometry.dssp; StructureBatch.backbone_hbonds, .secondary_structure).

Yardstick: tests/dssp_ref.py, the definition in float64 with dense N x N loops, on the same float32 coordinates.  The
kernel's partner indices and the labels must EQUAL the yardstick's; its energies, one rounding of a double to float32,
must lie within rtol 2^-23.  Equality is owed, not lucky: every case first asserts, from the yardstick, that no evaluated
energy lies within 1e-6 kcal/mol of the -0.5 threshold and no CA pair within 1e-4 A of the 9 A cutoff -- the kernel's
double evaluation of fp32 coordinates and its fp32 squared-distance test err by orders of magnitude less -- and the seeds
of the synthetic cases were picked so that this holds (the four PDB files have margins of 2.1e-4 kcal/mol and 9e-4 A).

No consecutive 5-turns exist in the four PDB files, so the label I cannot occur there under the definition (the other
seven labels do); the synthetic chains carry an ideal pi-helix, and all eight labels occur over the whole set.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dssp_ref as R
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

RTOL = 2.0 ** -23
PDB_FILES = ("1REX", "4EOT", "1ad0_DC", "5cjx_HL")
# name -> arguments of R.synthetic_case: the lane end (1, 2, 5), the 64-owner boundary (63, 64, 65), the 256-residue staging
# boundary (257, 300: two tiles, the second with holes), each with a structure that is all padding and masked residues
SYNTHETIC = {f"n{N}": dict(N=N, seed={257: 6, 300: 6}.get(N, 1)) for N in (1, 2, 5, 63, 64, 65, 257, 300)}
SYNTHETIC["helix_break"] = dict(N=65, seed=1, helix_break=True)
SYNTHETIC["donor_mask"] = dict(N=65, seed=1, with_donor=True)
SLOTS_CASE = dict(N=63, seed=1, A=6, slots=(4, 2, 0, 5))


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib
    _lib.load()
    return protstruc_amd


def assert_margins(refs, what):
    energy = min(bonds.energy_margin for bonds, _ in refs)
    ca = min(bonds.ca_margin for bonds, _ in refs)
    print(f"{what}: smallest |E + 0.5| = {energy:.3g} kcal/mol, smallest | |CA - CA| - 9 | = {ca:.3g} A")
    assert energy >= 1e-6 and ca >= 1e-4, (what, energy, ca)


def assert_hbonds_equal(got, refs, what):
    """the kernel's four (B,N,2) tensors against the yardstick's lists, structure by structure"""
    for b, (bonds, _) in enumerate(refs):
        for name in ("acceptor", "donor"):
            idx = getattr(got, name + "_idx")[b].cpu().numpy()
            energy = getattr(got, name + "_energy")[b].cpu().numpy()
            want_idx, want_e = getattr(bonds, name + "_idx"), getattr(bonds, name + "_energy")
            n = want_idx.shape[0]                       # a single structure may be shorter than its padded batch
            assert idx.dtype == np.int32 and energy.dtype == np.float32
            assert np.array_equal(idx[:n], want_idx), (what, b, name)
            err = np.abs(energy[:n].astype(np.float64) - want_e)
            assert (err <= RTOL * np.abs(want_e)).all(), (what, b, name, float(err.max()))
            assert (idx[n:] == -1).all() and (energy[n:] == 0).all(), (what, b, name)


def assert_codes_equal(codes, refs, what):
    assert codes.dtype == torch.int8
    got = codes.cpu().numpy()
    for b, (_, want) in enumerate(refs):
        n = want.shape[0]
        assert np.array_equal(got[b, :n], want), (what, b, R.strings(got[b, :n]), R.strings(want))
        assert (got[b, n:] == 0).all(), (what, b)


# ---- real structures -------------------------------------------------------------------------------------------------------
def pdb_path(name):
    return os.path.join(GOLDEN_DIR, name + ".pdb")


@functools.lru_cache(maxsize=None)
def pdb_reference():
    """The yardstick on the four files, from the batch's own tensors on the host (computed once, never modified)."""
    from protstruc_amd import StructureBatch
    batch = StructureBatch.from_pdb([pdb_path(name) for name in PDB_FILES], device="cpu")
    refs = []
    for b in range(len(PDB_FILES)):
        seq = "".join(batch.get_seq()[b][c] for c in batch.get_chain_ids()[b])
        n = len(seq)
        complete, junction, donor = R.structure_inputs(batch.get_atom_mask()[b, :n].numpy(), batch.chain_idx[b, :n].numpy(), seq)
        refs.append(R.dssp(batch.get_xyz()[b, :n, :4].numpy(), complete, junction, donor))
    return refs


def test_real_structures_in_one_batch_and_one_by_one(pkg):
    refs = pdb_reference()
    assert_margins(refs, "four PDB files")
    batch = pkg.StructureBatch.from_pdb([pdb_path(name) for name in PDB_FILES])
    assert batch.get_max_n_residues() == 448 and max(len(ids) for ids in batch.get_chain_ids()) == 2
    assert "X" in "".join(batch.get_seq()[3].values()) and "P" in "".join(batch.get_seq()[3].values())   # UNK gaps, prolines
    codes = batch.secondary_structure()
    bonds = batch.backbone_hbonds()
    assert_codes_equal(codes, refs, "batch")
    assert_hbonds_equal(bonds, refs, "batch")
    labels = "".join(R.strings(want) for _, want in refs)
    assert set(labels) == set(R.CODES) - {"I"}                 # no two consecutive 5-turns in these files: no I
    strings = batch.secondary_structure(as_strings=True)
    assert strings == [R.strings(want) for _, want in refs]
    reduced = batch.secondary_structure(reduced=True)
    for b, (_, want) in enumerate(refs):
        assert np.array_equal(reduced[b, :len(want)].cpu().numpy(), R.reduce_codes(want))
    assert batch.secondary_structure(reduced=True, as_strings=True) == [R.strings(R.reduce_codes(want), "CHE") for _, want in refs]
    # one by one: the same bits as in the batch
    for b, name in enumerate(PDB_FILES):
        single = pkg.StructureBatch.from_pdb(pdb_path(name))
        n = single.get_max_n_residues()
        assert torch.equal(single.secondary_structure()[0], codes[b, :n]), name
        for one, many in zip(single.backbone_hbonds(), bonds):
            assert torch.equal(one[0], many[b, :n]), name


# ---- synthetic chains --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic_reference(name):
    case = R.synthetic_case(**(SLOTS_CASE if name == "slots" else SYNTHETIC[name]))
    return case, R.case_reference(case)


def gpu_inputs(case):
    donor = None if case.donor is None else torch.from_numpy(case.donor).cuda()
    return (torch.from_numpy(case.xyz).cuda(), torch.from_numpy(case.complete).cuda(), torch.from_numpy(case.junction).cuda(),
            donor)


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_synthetic_chains_equal_the_yardstick(pkg, name):
    case, refs = synthetic_reference(name)
    assert_margins(refs, name)
    assert not case.complete[1].any() and np.isnan(case.xyz[1]).all()          # one structure is all padding
    if case.xyz.shape[1] > 5:
        assert not case.complete[0].all() and case.complete[0].any()           # some residues are masked
    xyz, complete, junction, donor = gpu_inputs(case)
    bonds = pkg.geometry.backbone_hbonds(xyz, complete, junction, donor)
    codes = pkg.geometry.dssp(xyz, complete, junction, donor)
    assert_hbonds_equal(bonds, refs, name)
    assert_codes_equal(codes, refs, name)
    assert (codes[1] == 0).all() and (bonds.acceptor_idx[1] == -1).all() and (bonds.donor_energy[1] == 0).all()
    # a second launch on the same input: the same bits
    again = pkg.geometry.backbone_hbonds(xyz, complete, junction, donor)
    for first, second in zip(bonds, again):
        assert torch.equal(first, second)
    assert torch.equal(codes, pkg.geometry.dssp(xyz, complete, junction, donor))
    reduced = pkg.geometry.dssp(xyz, complete, junction, donor, reduced=True)
    assert np.array_equal(reduced.cpu().numpy(), np.stack([R.reduce_codes(want) for _, want in refs]))


def test_the_cases_reach_what_they_are_for():
    """From the yardstick alone: the chain break changes the helix, the donor mask removes bonds, and every label occurs."""
    plain = synthetic_reference("n65")[1]
    broken = synthetic_reference("helix_break")[1]
    count_h = lambda refs: sum(R.strings(want).count("H") for _, want in refs)  # noqa: E731
    assert count_h(plain) > count_h(broken) > 0
    masked_case, masked = synthetic_reference("donor_mask")
    lost = [(b, j) for b in (0, 2) for j in range(65) if not masked_case.donor[b, j] and plain[b][0].acceptor_idx[j, 0] >= 0]
    assert lost and all(masked[b][0].acceptor_idx[j, 0] == -1 for b, j in lost)
    labels = "".join(R.strings(want) for name in SYNTHETIC for _, want in synthetic_reference(name)[1])
    assert set(labels) | set("".join(R.strings(want) for _, want in pdb_reference())) == set(R.CODES)
    assert "I" in labels and "G" in labels and "E" in labels and "H" in labels


def test_atom_slots_other_than_the_default(pkg):
    case, refs = synthetic_reference("slots")
    assert_margins(refs, "slots")
    xyz, complete, junction, _ = gpu_inputs(case)
    n, ca, c, o = case.slots
    bonds = pkg.geometry.backbone_hbonds(xyz, complete, junction, None, n, ca, c, o)
    assert_hbonds_equal(bonds, refs, "slots")
    assert_codes_equal(pkg.ops.dssp_assign(xyz, complete, junction, bonds.acceptor_idx, ca_slot=ca), refs, "slots")
    # the same chains in the default slots: the same bits
    default = xyz[:, :, [n, ca, c, o]].contiguous()
    for moved, plain in zip(bonds, pkg.geometry.backbone_hbonds(default, complete, junction)):
        assert torch.equal(moved, plain)


def test_longer_chains_than_the_assignment_takes_are_an_argument_error(pkg):
    xyz = torch.zeros(1, 2049, 4, 3, device="cuda")
    ones = torch.ones(1, 2049, dtype=torch.bool, device="cuda")
    bonds = pkg.ops.backbone_hbonds(xyz, ones, ones)                            # the sweep takes any length
    assert bonds[0].shape == (1, 2049, 2)
    with pytest.raises(ValueError, match="2048"):
        pkg.ops.dssp_assign(xyz, ones, ones, bonds[0])
    empty = pkg.geometry.dssp(xyz[:, :0], ones[:, :0], ones[:, :0])
    assert empty.shape == (1, 0) and empty.dtype == torch.int8
