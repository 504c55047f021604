"""Host-side checks of DSSP: the yardstick itself (tests/dssp_ref.py) on hand-computed energies and against the HELIX and
SHEET records of four PDB files, the C ABI's surface, the argument validation of ``ops.backbone_hbonds`` /
``ops.dssp_assign`` and the signatures of the layers above.  No GPU needed."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import dssp_ref as R
from tests.conftest import GOLDEN_DIR

PDB_FILES = ("1REX", "4EOT", "1ad0_DC", "5cjx_HL")


def collinear_pair(d_oh=2.0):
    """C=O...H-N on the x axis: C-O 1.2, O...H ``d_oh``, H-N 1.0 -- as (O, C, N, H)"""
    C, O = np.array([0.0, 0.0, 0.0]), np.array([1.2, 0.0, 0.0])
    H = O + [d_oh, 0.0, 0.0]
    return O, C, H + [1.0, 0.0, 0.0], H


def test_yardstick_energy_on_a_hand_computed_pair():
    """d(O,H) = 2.0, C-O = 1.2, N-H = 1.0 on a line: d(O,N) = 3.0, d(C,H) = 3.2, d(C,N) = 4.2, so
    E = 27.888 (1/3 + 1/3.2 - 1/2 - 1/4.2) = -2.5730..."""
    want = 27.888 * (1 / 3 + 1 / 3.2 - 1 / 2 - 1 / 4.2)
    assert abs(want - (-2.573)) < 5e-4
    assert abs(R.pair_energy(*collinear_pair()) - want) < 1e-9
    # the 0.5 A floor: O...H at 0.4 gives -9.9 whatever the formula says, at 0.6 the formula again
    assert R.pair_energy(*collinear_pair(0.4)) == -9.9
    O, C, N, H = collinear_pair(0.6)
    assert abs(R.pair_energy(O, C, N, H) - 27.888 * (1 / 1.6 + 1 / 1.8 - 1 / 0.6 - 1 / 2.8)) < 1e-9


def pair_structure():
    """Three residues: 0 -> 1 is a peptide bond, residue 2 is an acceptor alone whose C=O faces the N-H of residue 1 as in
    ``collinear_pair``.  H_1 = N_1 + unit(C_0 - O_0) lies on the x axis by the choice of C_0 - O_0 = (-1.2, 0, 0)."""
    O, C, N, H = collinear_pair()
    xyz = np.zeros((3, 4, 3))
    xyz[2, 2], xyz[2, 3], xyz[2, 1] = C, O, C + [0.0, 1.5, 0.0]
    xyz[1, 0], xyz[1, 1], xyz[1, 2], xyz[1, 3] = N, N + [1.0, 1.0, 0.0], N + [2.4, 1.0, 0.0], N + [2.4, 2.2, 0.0]
    xyz[0, 3], xyz[0, 2], xyz[0, 1], xyz[0, 0] = N + [1.2, -1.3, 0.0], N + [0.0, -1.3, 0.0], N + [-0.5, -2.7, 0.0], N + [0.5, -3.8, 0.0]
    return xyz, np.ones(3, dtype=bool), np.array([True, False, False])


def test_yardstick_lists_on_the_hand_computed_pair():
    xyz, complete, junction = pair_structure()
    want = 27.888 * (1 / 3 + 1 / 3.2 - 1 / 2 - 1 / 4.2)
    bonds = R.hbonds(xyz, complete, junction)
    assert abs(bonds.energy[2, 1] - want) < 1e-9                       # acceptor 2, donor 1
    assert np.isnan(bonds.energy[0, 1]) and np.isnan(bonds.energy[1, 1])   # j = i + 1 and i = j are not evaluated
    assert np.isnan(bonds.energy[:, 0]).all() and np.isnan(bonds.energy[:, 2]).all()   # no H without a junction before
    assert bonds.acceptor_idx.tolist() == [[-1, -1], [2, -1], [-1, -1]]
    assert bonds.donor_idx.tolist() == [[-1, -1], [-1, -1], [1, -1]]
    assert abs(bonds.acceptor_energy[1, 0] - want) < 1e-9 and bonds.acceptor_energy[1, 1] == 0.0
    assert abs(bonds.energy_margin - abs(want + 0.5)) < 1e-9
    # a proline at the donor, an incomplete acceptor, a CA beyond 9 A: no bond
    assert (R.hbonds(xyz, complete, junction, donor=np.array([True, False, True])).acceptor_idx == -1).all()
    assert (R.hbonds(xyz, np.array([True, True, False]), junction).acceptor_idx == -1).all()
    far = xyz.copy()
    far[2, 1] = far[1, 1] + [0.0, 9.5, 0.0]
    assert (R.hbonds(far, complete, junction).acceptor_idx == -1).all()
    assert abs(R.hbonds(far, complete, junction).ca_margin - 0.5) < 1e-9


def test_yardstick_keeps_the_two_best_and_breaks_ties_by_index():
    """Four acceptors around one donor, mirror images of each other about the donor's N-H axis: equal energies pairwise."""
    O, C, N, H = collinear_pair()
    xyz, complete, junction = pair_structure()
    xyz = np.concatenate([xyz[:2]] + [xyz[2:3]] * 4)
    for k, (y, z) in enumerate(((0.6, 0.0), (-0.6, 0.0), (0.0, 0.9), (0.0, -0.9))):
        xyz[2 + k, 2], xyz[2 + k, 3] = C + [0.0, y, z], O + [0.0, y, z]
        xyz[2 + k, 1] = C + [0.0, y, z] + [-1.0, 1.0 if k % 2 else -1.0, 0.0]
    complete, junction = np.ones(6, dtype=bool), np.array([True] + [False] * 5)
    bonds = R.hbonds(xyz, complete, junction)
    e = bonds.energy[2:, 1]
    assert e[0] == e[1] and e[2] == e[3] and e[0] < e[2] < -0.5          # exact ties, by symmetry
    assert bonds.acceptor_idx[1].tolist() == [2, 3]                      # the two best; the tie goes to the lower index
    assert bonds.acceptor_energy[1].tolist() == [e[0], e[1]]
    swapped = xyz[[0, 1, 4, 5, 2, 3]]
    assert R.hbonds(swapped, complete, junction).acceptor_idx[1].tolist() == [4, 5]
    # the acceptor side: one C=O, its two best donors
    assert bonds.donor_idx[2].tolist() == [1, -1]


def test_yardstick_labels_an_ideal_helix_and_a_hairpin():
    helix = R.ideal_helix(12)
    complete = np.ones(12, dtype=bool)
    bonds, codes = R.dssp(helix, complete, R.chain_junctions(complete))
    assert R.strings(codes) == "-HHHHHHHHHH-"
    assert [int(bonds.acceptor_idx[j, 0]) for j in range(4, 12)] == list(range(8))
    _, broken = R.dssp(helix, complete, R.chain_junctions(complete, breaks=(5,)))
    assert R.strings(broken) == "-HHHH--HHHH-"                          # no turn spans the break: two helices of four
    pin = R.hairpin(7)
    complete = np.ones(14, dtype=bool)
    _, codes = R.dssp(pin, complete, R.chain_junctions(complete, breaks=(6,)))
    assert R.strings(codes).count("E") >= 8 and set(R.strings(codes)) <= set("-ES")
    assert R.strings(R.reduce_codes(codes), "CHE").count("E") == R.strings(codes).count("E")


def pdb_case(name):
    """One PDB file through the package's reader (host-side plumbing): xyz (N,4,3), complete, junction, donor, and the
    residue's index by (chain, number)."""
    from protstruc_amd.pdb import PDB
    path = os.path.join(GOLDEN_DIR, name + ".pdb")
    p = PDB.read_pdb(path)
    complete, junction, donor = R.structure_inputs(p.atom_xyz_mask.numpy(), np.array(p.chain_idx), p.get_seq())
    index = {(c, n): k for k, (c, n) in enumerate(zip(p.chain_of, p.number_of))}
    return path, p.atom_xyz.numpy()[:, :4], complete, junction, donor, index


@pytest.fixture(scope="module")
def pdb_labels():
    out = {}
    for name in PDB_FILES:
        path, xyz, complete, junction, donor, index = pdb_case(name)
        bonds, codes = R.dssp(xyz, complete, junction, donor)
        helices, strands = R.pdb_records(path)
        out[name] = (R.strings(codes), helices, strands, index, bonds)
    return out


@pytest.mark.parametrize("name", PDB_FILES)
def test_every_h_of_the_yardstick_lies_inside_a_helix_record(pdb_labels, name):
    labels, helices, _, index, bonds = pdb_labels[name]
    inside = {index[(chain, n)] for _, chain, first, last in helices for n in range(first, last + 1) if (chain, n) in index}
    assert labels.count("H") > 0
    assert [k for k, s in enumerate(labels) if s == "H" and k not in inside] == []
    print(name, "H", labels.count("H"), "E", labels.count("E"), "margins", bonds.energy_margin, bonds.ca_margin)


def test_the_records_of_1rex_are_found(pdb_labels):
    """Every residue of a class-1 HELIX record is H, G, I or T (40 residues), every residue of a SHEET record is E (8)."""
    labels, helices, strands, index, _ = pdb_labels["1REX"]
    alpha = [index[(chain, n)] for cls, chain, first, last in helices if cls == 1 for n in range(first, last + 1)]
    sheet = [index[(chain, n)] for chain, first, last in strands for n in range(first, last + 1)]
    assert len(alpha) == 40 and len(sheet) == 8
    assert [k for k in alpha if labels[k] not in "HGIT"] == []
    assert [k for k in sheet if labels[k] != "E"] == []


def test_codes_are_the_yardsticks():
    """(declared, exported, bound: tests/test_capi_symbols.py)"""
    from protstruc_amd import geometry
    assert geometry.DSSP_CODES == R.CODES == "-HBEGITS"


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 and N = 0 launch nothing."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)

    def hbonds(xyz=fake, complete=fake, junction=fake, donor=None, slots=(0, 1, 2, 3), out=(fake,) * 4, B=1, N=8, A=4):
        return lib.ps_backbone_hbonds_f32(xyz, complete, junction, donor, *slots, *out, B, N, A, None)

    def assign(xyz=fake, complete=fake, junction=fake, acc=fake, ca=1, codes=fake, B=1, N=8, A=4):
        return lib.ps_dssp_assign(xyz, complete, junction, acc, ca, codes, B, N, A, None)

    for call in (hbonds, assign):
        assert call(B=0) == 0 and call(N=0) == 0
        assert call(xyz=None) == 1 and call(complete=None) == 1 and call(junction=None) == 1
        assert call(B=-1) == 1 and call(N=-1) == 1 and call(A=0) == 1
    assert hbonds(B=65536) == 1 and hbonds(N=2 ** 24 + 1) == 1 and hbonds(A=3) == 1
    for k in range(4):
        assert hbonds(out=tuple(None if m == k else fake for m in range(4))) == 1
    for slots in ((0, 1, 2, 4), (-1, 1, 2, 3), (0, 1, 1, 3), (0, 1, 2, 0)):
        assert hbonds(slots=slots) == 1
    assert hbonds(B=0, slots=(3, 2, 1, 0), A=15) == 0
    assert assign(acc=None) == 1 and assign(codes=None) == 1
    assert assign(N=2049) == 1 and assign(B=0, N=2048) == 0            # the chain limit of the LDS-resident lists
    assert assign(ca=4) == 1 and assign(ca=-1) == 1
    assert assign(B=2 ** 21, N=2048) == 1                               # B * N beyond 2^31


def dssp_args(B=2, N=9, A=4):
    g = torch.Generator().manual_seed(1)
    complete = torch.ones(B, N, dtype=torch.bool)
    junction = torch.ones(B, N, dtype=torch.bool)
    junction[:, -1] = False
    return [torch.randn(B, N, A, 3, generator=g), complete, junction]


def test_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_dssp_shapes
    xyz, complete, junction = dssp_args()
    acc = torch.full((2, 9, 2), -1, dtype=torch.int32)
    check(xyz, complete, junction)
    check(xyz, complete, junction, complete)
    check(xyz, complete, junction, acceptor_idx=acc)
    check(xyz, complete.to(torch.uint8), junction.float())                # any mask dtype: reduced to its truth value
    for bad in (xyz[0], xyz[..., :2], xyz.long(), xyz[:, :, :3]):
        with pytest.raises(ValueError):
            check(bad, complete, junction)
    with pytest.raises(ValueError):
        check(xyz, complete[:, :8], junction)
    with pytest.raises(ValueError):
        check(xyz, complete, junction[:1])
    with pytest.raises(ValueError):
        check(xyz, None, junction)
    with pytest.raises(ValueError):
        check(xyz, complete, None)
    with pytest.raises(ValueError):
        check(xyz, complete, junction, complete[:, :8])
    for slots in ((0, 1, 2, 4), (0, 0, 2, 3), (-1, 1, 2, 3)):
        with pytest.raises(ValueError):
            check(xyz, complete, junction, None, *slots)
    for bad in (acc[:, :, :1], acc.float(), acc[:1]):
        with pytest.raises(ValueError):
            check(xyz, complete, junction, acceptor_idx=bad)
    with pytest.raises(ValueError):
        check(xyz, complete, junction, ca_slot=4, acceptor_idx=acc)
    long_xyz = torch.zeros(1, 2049, 4, 3)
    ones = torch.ones(1, 2049, dtype=torch.bool)
    check(long_xyz, ones, ones)                                           # the sweep takes any length
    with pytest.raises(ValueError, match="2048"):
        check(long_xyz, ones, ones, acceptor_idx=torch.zeros(1, 2049, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        check(xyz, complete.to("meta"), junction)                         # device disagreement


def test_ops_validate_first_then_refuse_cpu_tensors():
    from protstruc_amd import geometry, ops
    xyz, complete, junction = dssp_args()
    acc = torch.full((2, 9, 2), -1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.backbone_hbonds(xyz, complete[:, :8], junction)
    with pytest.raises(ValueError):
        ops.dssp_assign(xyz, complete, junction, acc.float())
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.backbone_hbonds(xyz, complete, junction)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.dssp_assign(xyz, complete, junction, acc)
    with pytest.raises(RuntimeError, match="HIP-only"):
        geometry.dssp(xyz, complete, junction)


def test_signatures_of_the_layers_above():
    from protstruc_amd import StructureBatch, geometry, ops
    p = inspect.signature(geometry.backbone_hbonds).parameters
    assert list(p) == ["xyz", "complete", "junction", "donor", "n", "ca", "c", "o"]
    assert [p[k].default for k in ("donor", "n", "ca", "c", "o")] == [None, 0, 1, 2, 3]
    assert geometry.BackboneHBonds._fields == ("acceptor_idx", "acceptor_energy", "donor_idx", "donor_energy")
    p = inspect.signature(geometry.dssp).parameters
    assert list(p) == ["xyz", "complete", "junction", "donor", "reduced"]
    assert (p["donor"].default, p["reduced"].default) == (None, False)
    p = inspect.signature(geometry.dssp_strings).parameters
    assert list(p)[:2] == ["codes", "lengths"] and p["lengths"].default is None
    assert all(p[k].default is not inspect.Parameter.empty for k in list(p)[2:])
    assert list(inspect.signature(StructureBatch.backbone_hbonds).parameters) == ["self"]
    p = inspect.signature(StructureBatch.secondary_structure).parameters
    assert list(p) == ["self", "reduced", "as_strings"] and (p["reduced"].default, p["as_strings"].default) == (False, False)
    p = inspect.signature(ops.backbone_hbonds).parameters
    assert list(p) == ["xyz", "complete", "junction", "donor", "n_slot", "ca_slot", "c_slot", "o_slot"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("n_slot", "ca_slot", "c_slot", "o_slot"))
    assert list(inspect.signature(ops.dssp_assign).parameters) == ["xyz", "complete", "junction", "acceptor_idx", "ca_slot"]


def test_strings_and_the_reduced_alphabet():
    from protstruc_amd import geometry
    codes = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7], [1, 1, 0, 0, 0, 0, 0, 0]], dtype=torch.int8)
    assert geometry.dssp_strings(codes) == ["-HBEGITS", "HH------"]
    assert geometry.dssp_strings(codes, [8, 2]) == ["-HBEGITS", "HH"]
    assert geometry.dssp_strings(codes, torch.tensor([3, 0])) == ["-HB", ""]
    reduced = torch.from_numpy(R.reduce_codes(codes.numpy()))
    assert geometry.dssp_strings(reduced, reduced=True) == ["CHEEHHCC", "HHCCCCCC"]
    with pytest.raises(ValueError):
        geometry.dssp_strings(codes, [8])


def test_structure_batch_builds_complete_junction_and_donor(monkeypatch):
    """The masks the methods hand to ``geometry.dssp`` are the ones the definition asks for (host-only: the geometry
    function is replaced by a recorder), on a file with UNK gap residues, two chains and prolines."""
    from protstruc_amd import StructureBatch, geometry
    seen = {}

    def fake_dssp(xyz, complete, junction, donor=None, reduced=False):
        seen.update(complete=complete, junction=junction, donor=donor, reduced=reduced)
        return torch.zeros(complete.shape, dtype=torch.int8)

    monkeypatch.setattr(geometry, "dssp", fake_dssp)
    batch = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "5cjx_HL.pdb"), device="cpu")
    out = batch.secondary_structure(reduced=True, as_strings=True)
    assert out == ["C" * 448] and seen["reduced"] is True
    seq = "".join(batch.get_seq()[0][c] for c in batch.get_chain_ids()[0])
    complete, junction, donor = R.structure_inputs(batch.get_atom_mask()[0].numpy(), batch.chain_idx[0].numpy(), seq)
    assert int((~complete).sum()) == 7 and "P" in seq and len(batch.get_chain_ids()[0]) == 2
    assert np.array_equal(seen["complete"][0].numpy(), complete)
    assert np.array_equal(seen["junction"][0].numpy(), junction)
    assert np.array_equal(seen["donor"][0].numpy(), donor)


def test_the_timing_tool_composes_the_same_definition():
    """tools/dssp_time.py's composed-torch evaluation (dense energies, topk, shifted boolean maps; float32), run on the CPU
    here, labels a synthetic case as the yardstick does: what the tool times is the definition, not something cheaper."""
    from tools import dssp_time
    case = R.synthetic_case(65, 1)
    refs = R.case_reference(case)
    assert min(bonds.energy_margin for bonds, _ in refs) > 1e-3           # float32 against float64: far from the threshold
    codes = dssp_time.composed(torch.from_numpy(case.xyz), torch.from_numpy(case.complete), torch.from_numpy(case.junction))
    assert codes.dtype == torch.int8
    for b, (_, want) in enumerate(refs):
        assert R.strings(codes[b].numpy()) == R.strings(want)
    assert (dssp_time.B, dssp_time.N) == (128, 512) and set(dssp_time.STEPS) == set(dssp_time.STEP_TIMEOUT_S) == {"events", "torch"}
