"""Host-side checks of the side-chain torsions: the yardstick itself (tests/chi_ref.py) on hand cases and on the golden PDB
files, the three tables of ``general``, the analytic gradients against torch-float64 autograd, the C ABI's surface and
its argument validation, the argument validation of the four ``ops``, ``geometry.set_side_chain_torsions``' refusal of a
differentiable ``xyz``, what ``StructureBatch`` hands to the geometry layer, and the composed route of the timing tool.
No GPU needed."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import chi_ref as R
from tests.c_headers import parameters

SYMBOLS = ("ps_chi_f32", "ps_chi_backward_f32", "ps_chi_set_f32", "ps_chi_set_backward_f32")
PDB_COUNTS = {"1REX": (105, 77, 30, 19), "4EOT": (146, 88, 44, 22), "5cjx_HL": (342, 197, 50, 17),
              "15c8_HL": (190, 121, 41, 16), "6dc4": (370, 227, 78, 37), "4uuj": (443, 274, 86, 41)}
ONE_ANGLE = np.array([[[0, 1, 2, 3], [-1] * 4, [-1] * 4, [-1] * 4]])          # one residue type whose chi1 is slots 0 1 2 3


def circular(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def clean(case):
    return np.where(case.mask[..., None], case.xyz, 0).astype(np.float64)


# ---- hand cases -----------------------------------------------------------------------------------------------------------
def four_atoms(degrees):
    """a, b, c on a right-angled path in the xy plane and d turned by ``degrees`` about b -> c, counted as IUPAC does:
    clockwise looking from b to c is positive"""
    t = np.radians(degrees)
    return np.array([[[[1, 0, 0], [0, 0, 0], [0, 1, 0], [np.cos(t), 1, -np.sin(t)]]]], dtype=np.float32)


@pytest.mark.parametrize("degrees", [60.0, -60.0, 180.0])
def test_a_known_dihedral_has_its_sign(degrees):
    chi, defined = R.measure(four_atoms(degrees), np.zeros((1, 1), dtype=np.int32), None, ONE_ANGLE)
    assert defined.tolist() == [[[True, False, False, False]]]
    assert circular(chi[0, 0, 0], np.radians(degrees)) < 1e-7               # the float32 rounding of the corner d
    assert (chi[0, 0, 1:] == 0).all()
    if degrees != 180.0:
        assert np.sign(chi[0, 0, 0]) == np.sign(degrees)


def test_setting_180_degrees_on_a_cis_arrangement_mirrors_d_through_the_axis():
    xyz = four_atoms(0.0)                                                    # planar cis: d = (1, 1, 0)
    last = np.array([[3, -1, -1, -1]])
    t = R.set_chi(xyz, np.full((1, 1, 4), np.pi), np.zeros((1, 1), dtype=np.int32), None, ONE_ANGLE, last)
    assert t.moved.tolist() == [[[False, False, False, True]]] and t.turned.tolist() == [[[True, False, False, False]]]
    assert np.abs(t.out[0, 0, 3] - [-1.0, 1.0, 0.0]).max() < 1e-15           # through the axis x = 0, z = 0
    assert (t.out[0, 0, :3] == xyz[0, 0, :3]).all()
    rel = R.set_chi(xyz, np.full((1, 1, 4), np.pi / 2), np.zeros((1, 1), dtype=np.int32), None, ONE_ANGLE, last, relative=True)
    assert np.abs(rel.out[0, 0, 3] - [0.0, 1.0, -1.0]).max() < 1e-15         # +90 degrees: clockwise seen from b to c


# ---- the tables -------------------------------------------------------------------------------------------------------------
CHAINS = {"ARG": "CG CD NE CZ", "LYS": "CG CD CE NZ", "MET": "CG SD CE", "GLN": "CG CD OE1", "GLU": "CG CD OE1",
          "ASN": "CG OD1", "ASP": "CG OD1", "HIS": "CG ND1", "LEU": "CG CD1", "PHE": "CG CD1", "TRP": "CG CD1",
          "TYR": "CG CD1", "ILE": "CG1 CD1", "PRO": "CG CD", "CYS": "SG", "SER": "OG", "THR": "OG1", "VAL": "CG1",
          "ALA": "", "GLY": "", "UNK": ""}


def test_chi_atom_table_names_the_stated_atoms():
    from protstruc_amd import general, pdb
    table = general.chi_atom_table()
    assert table.shape == (21, 4, 4) and table.dtype == torch.int32
    for three, chain in CHAINS.items():
        row = table[pdb.ONE_TO_INDEX[pdb.THREE_TO_ONE[three]]]
        names = ["N", "CA", "CB"] + chain.split()
        n_angles = len(chain.split())
        for k in range(4):
            if k < n_angles:
                assert row[k].tolist() == [pdb.ATOM_SLOT[three][a] for a in names[k:k + 4]], (three, k)
            else:
                assert row[k].tolist() == [-1] * 4, (three, k)
    # ARG and LYS 4; MET, GLN and GLU 3; ...: 18 types have a chi1 (every type but ALA, GLY and X, as the table of chains
    # says -- the "19" of the issue's summary counts glycine), 14 a chi2, 5 a chi3, 2 a chi4
    assert (table[:, :, 0] >= 0).sum(0).tolist() == [18, 14, 5, 2]


def test_chi_last_table_follows_the_rule():
    from protstruc_amd import general, pdb
    atoms, last = general.chi_atom_table(), general.chi_last_table()
    assert last.shape == (21, 4) and last.dtype == torch.int32
    row = lambda three: pdb.ONE_TO_INDEX[pdb.THREE_TO_ONE[three]]   # noqa: E731
    assert last[row("ILE")].tolist() == [7, 7, -1, -1] and atoms[row("ILE"), 1].tolist() == [1, 4, 5, 7]
    assert last[row("PRO")].tolist() == [-1] * 4 and (atoms[row("PRO"), :2] >= 0).all()
    assert last.max() == 13 and last[row("TRP")].tolist() == [13, 13, -1, -1]        # no range reaches OXT in slot 14
    for three in CHAINS:
        side_chain_end = max(s for name, s in pdb.ATOM_SLOT.get(three, {"CB": 4}).items() if name != "OXT")
        for k in range(4):
            has = atoms[row(three), k, 0] >= 0
            want = side_chain_end if has and three != "PRO" else -1
            assert last[row(three), k] == want, (three, k)
            if want >= 0:     # the library's rule: last in [d, A), none of a, b, c inside [d, last]
                a, b, c, d = atoms[row(three), k].tolist()
                assert d <= want and not any(d <= s <= want for s in (a, b, c))


def test_chi_pi_periodic_table():
    from protstruc_amd import general, pdb
    table = general.chi_pi_periodic_table()
    assert table.shape == (21, 4) and table.dtype == torch.bool and table.sum() == 4
    for three, k in (("ASP", 1), ("GLU", 2), ("PHE", 1), ("TYR", 1)):
        assert table[pdb.ONE_TO_INDEX[pdb.THREE_TO_ONE[three]], k]


# ---- the yardstick on data ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pdb_cases():
    return {name: R.pdb_case([name + ".pdb"]) for name in PDB_COUNTS}


@pytest.mark.parametrize("name", sorted(PDB_COUNTS))
def test_the_yardstick_on_a_pdb_file(pdb_cases, name):
    case = pdb_cases[name]
    atoms, last = R.tables()
    chi, defined = R.measure(case.xyz, case.types, case.mask, atoms)
    assert tuple(defined.sum((0, 1)).tolist()) == PDB_COUNTS[name]
    assert (chi[~defined] == 0).all() and np.isfinite(chi).all()
    X = clean(case)
    rng = np.random.default_rng(7)
    want = rng.uniform(-np.pi, np.pi, size=chi.shape)
    want[~defined] = np.nan                                                  # never read
    t = R.set_chi(case.xyz, want, case.types, case.mask, atoms, last)
    assert (t.turned == (defined & (last[np.clip(case.types, 0, 20)] >= 0))).all()
    out = np.where(t.moved[..., None], t.out, X)
    again, _ = R.measure(out, case.types, case.mask, atoms)
    assert circular(again, want)[t.turned].max() <= 1e-12
    assert (again[defined & ~t.turned] == chi[defined & ~t.turned]).all()    # proline is measured, never turned
    # no intra-residue distance that was below 1.95 A changes
    before = np.linalg.norm(X[:, :, :, None] - X[:, :, None, :], axis=-1)
    after = np.linalg.norm(out[:, :, :, None] - out[:, :, None, :], axis=-1)
    bonded = case.mask[:, :, :, None] & case.mask[:, :, None, :] & (before < 1.95)
    assert np.abs(after - before)[bonded].max() <= 1e-12
    # the measured angles put back give the input
    same = R.set_chi(case.xyz, chi, case.types, case.mask, atoms, last)
    assert np.abs(same.out - X)[same.moved].max() <= 1e-12
    # relative with delta = absolute with phi + delta
    delta = rng.uniform(-np.pi, np.pi, size=chi.shape)
    rel = R.set_chi(case.xyz, delta, case.types, case.mask, atoms, last, relative=True)
    absolute = R.set_chi(case.xyz, chi + delta, case.types, case.mask, atoms, last)
    assert (rel.moved == absolute.moved).all() and np.abs(rel.out - absolute.out)[rel.moved].max() <= 1e-12


def test_synthetic_case():
    case = R.synthetic_case(3, 40, 15, seed=3)
    assert case.xyz.shape == (3, 40, 15, 3) and case.xyz.dtype == np.float32 and case.types.dtype == np.int32
    assert case.types.min() == -1 and case.types.max() == 22 and (case.types == 20).any()
    assert np.isnan(case.xyz[~case.mask]).all() and not np.isnan(case.xyz[case.mask]).any()
    assert 0.3 < 1 - case.mask[0].mean() < 0.6 and case.mask[1].all() and not case.mask[2].any()
    steps = np.linalg.norm(np.diff(case.xyz[1].astype(np.float64), axis=1), axis=-1)
    assert steps.min() > 0.99 and steps.max() < 2.01
    _, defined = R.measure(case.xyz, case.types, case.mask, R.tables()[0])
    assert defined[1].sum() > 20 and not defined[2].any() and not defined[(case.types < 0) | (case.types >= 20)].any()


# ---- gradients of the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["synthetic", "1REX"])
def test_analytic_gradients_match_autograd(pdb_cases, which):
    case = R.synthetic_case(2, 9, 15, seed=1) if which == "synthetic" else pdb_cases["1REX"]
    atoms, last = R.tables()
    rng = np.random.default_rng(2)
    g_chi = rng.normal(size=case.types.shape + (4,))
    X = torch.from_numpy(clean(case))
    # measure
    analytic = R.measure_backward(case.xyz, case.types, case.mask, atoms, g_chi)
    leaf = X.clone().requires_grad_()
    chi_t = R.measure_torch(leaf, case.types, case.mask, atoms)
    assert np.abs(chi_t.detach().numpy() - R.measure(case.xyz, case.types, case.mask, atoms)[0]).max() < 1e-12
    (chi_t * torch.from_numpy(g_chi)).sum().backward()
    assert np.abs(analytic).max() > 0
    assert np.abs(analytic - leaf.grad.numpy()).max() <= 1e-9 * np.abs(analytic).max()
    # set, both modes, with and without a selection
    g_out = np.where(case.mask[..., None], rng.normal(size=case.xyz.shape), 0.0)
    select = rng.random(g_chi.shape) < 0.6
    for relative in (False, True):
        for sel in (None, select):
            want = rng.uniform(-np.pi, np.pi, size=g_chi.shape)
            t = R.set_chi(case.xyz, want, case.types, case.mask, atoms, last, sel, relative)
            out = np.where(t.moved[..., None], t.out, X.numpy())
            analytic = R.set_chi_backward(out, g_out, case.types, case.mask, atoms, last, sel)
            angles = torch.from_numpy(want).requires_grad_()
            out_t = R.set_torch(X, angles, case.types, case.mask, atoms, last, sel, relative)
            assert np.abs(out_t.detach().numpy() - out).max() < 1e-12
            (out_t * torch.from_numpy(g_out)).sum().backward()
            assert t.turned.any() and (analytic[~t.turned] == 0).all()
            assert np.abs(analytic - angles.grad.numpy()).max() <= 1e-9 * np.abs(analytic).max(), (relative, sel is None)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_parameter_names_of_the_entry_points():
    """(declared, exported, bound, and the parameter counts: tests/test_capi_symbols.py)"""
    names = lambda symbol: [p.split()[-1].lstrip("*") for p in parameters("protstruc_hip.h", symbol)]       # noqa: E731
    assert names("ps_chi_f32") == ["xyz", "atom_mask", "residue_type", "chi_atoms", "T", "chi", "chi_mask", "B", "N", "A", "stream"]
    assert names("ps_chi_set_f32") == ["xyz", "atom_mask", "residue_type", "chi_atoms", "chi_last", "T", "chi", "chi_select",
                                       "relative", "out", "B", "N", "A", "stream"]


def ints(values):
    flat = np.asarray(values).astype(np.int64).ravel().tolist()
    return (ctypes.c_int * len(flat))(*flat)


def entries(lib, fake):
    """name -> (call(**overrides) with B = 0, the names of its required pointers, whether it takes chi_last)"""
    def chi(xyz=fake, mask=None, types=fake, atoms=None, last=None, T=1, chi=fake, chi_mask=fake, B=0, N=8, A=15):
        return lib.ps_chi_f32(xyz, mask, types, atoms, T, chi, chi_mask, B, N, A, None)

    def chi_backward(xyz=fake, mask=None, types=fake, atoms=None, last=None, T=1, grad_chi=fake, grad_xyz=fake, B=0, N=8, A=15):
        return lib.ps_chi_backward_f32(xyz, mask, types, atoms, T, grad_chi, grad_xyz, B, N, A, None)

    def chi_set(xyz=fake, mask=None, types=fake, atoms=None, last=None, T=1, chi=fake, select=None, relative=0,
                out=ctypes.c_void_p(0x2000), B=0, N=8, A=15):
        return lib.ps_chi_set_f32(xyz, mask, types, atoms, last, T, chi, select, relative, out, B, N, A, None)

    def chi_set_backward(out=fake, mask=None, types=fake, atoms=None, last=None, T=1, select=None, grad_out=fake,
                         grad_chi=fake, B=0, N=8, A=15):
        return lib.ps_chi_set_backward_f32(out, mask, types, atoms, last, T, select, grad_out, grad_chi, B, N, A, None)

    return {"ps_chi_f32": (chi, ("xyz", "types", "atoms"), False),
            "ps_chi_backward_f32": (chi_backward, ("xyz", "types", "atoms", "grad_chi", "grad_xyz"), False),
            "ps_chi_set_f32": (chi_set, ("xyz", "types", "atoms", "last", "chi", "out"), True),
            "ps_chi_set_backward_f32": (chi_set_backward, ("out", "types", "atoms", "last", "grad_out", "grad_chi"), True)}


@pytest.mark.parametrize("symbol", sorted(SYMBOLS))
def test_entry_refuses_bad_arguments_before_any_launch(symbol):
    """hipErrorInvalidValue (1) without touching a device: B = 0 launches nothing, so the device pointers are never
    dereferenced; the tables are host arrays and are read and validated in every call."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    call, required, takes_last = entries(lib, fake)[symbol]
    one_atoms, one_last = [[0, 1, 2, 3], [1, 2, 3, 4], [-1] * 4, [-1] * 4], [5, 5, -1, -1]
    good = dict(atoms=ints(one_atoms), last=ints(one_last))

    def with_tables(atoms=one_atoms, last=one_last, **kw):
        return call(atoms=ints(atoms), last=ints(last), **kw)

    assert call(**good) == 0 and call(mask=fake, **good) == 0 and call(B=4, N=0, **good) == 0
    for name in required:
        assert call(**{**good, name: None}) == 1, name
    if symbol == "ps_chi_f32":
        assert call(chi=None, **good) == 0 and call(chi_mask=None, **good) == 0
        assert call(chi=None, chi_mask=None, **good) == 1                    # both outputs null
    if symbol == "ps_chi_set_f32":
        assert call(select=fake, relative=1, **good) == 0
        assert call(out=fake, **good) == 1                                   # out may not alias xyz
    for T in (0, 33, -1):
        assert call(T=T, atoms=ints(np.full((33, 4, 4), -1)), last=ints(np.full((33, 4), -1))) == 1, T
    assert call(T=32, atoms=ints(np.full((32, 4, 4), -1)), last=ints(np.full((32, 4), -1))) == 0
    for A in (0, 65, -1):
        assert call(A=A, **good) == 1, A
    assert call(A=64, **good) == 0 and call(A=6, **good) == 0
    assert call(A=4, **good) == 1                                            # a slot equal to A
    assert with_tables(atoms=[[0, 1, 2, 15]] + one_atoms[1:]) == 1 and with_tables(atoms=[[0, 1, 2, 14]] + one_atoms[1:], last=[14, 5, -1, -1]) == 0
    assert with_tables(atoms=[[0, 1, 2, -1]] + one_atoms[1:]) == 1           # three slots and one -1
    assert with_tables(atoms=[[0, 1, 1, 3]] + one_atoms[1:]) == 1            # two equal slots
    assert with_tables(atoms=[[-2] * 4] + one_atoms[1:], last=[-1, 5, -1, -1]) == 1
    if takes_last:
        assert with_tables(last=[2, 5, -1, -1]) == 1                         # last < d
        assert with_tables(last=[5, 5, 3, -1]) == 1                          # a range without an angle
        assert with_tables(last=[15, 5, -1, -1]) == 1 and with_tables(last=[14, 5, -1, -1]) == 0
        assert with_tables(atoms=[[4, 1, 2, 3]] + one_atoms[1:]) == 1        # a inside [d, last]
        assert with_tables(atoms=[[4, 1, 2, 3]] + one_atoms[1:], last=[3, 5, -1, -1]) == 0
        assert with_tables(last=[-2, 5, -1, -1]) == 1
    assert call(B=-1, **good) == 1 and call(N=-1, **good) == 1
    assert call(B=2 ** 16, N=2 ** 15 + 1, **good) == 1 and call(B=0, N=2 ** 31 - 1, **good) == 0             # B * N <= 2^31
    # the project's own tables: fine at A = 15 and at A = 14 -- TRP's CH2 sits in slot 13 --; at A = 13 that row, and
    # only that row, is refused (the issue names A = 14 for this; TRP's fourteen heavy atoms end in slot 13)
    atoms, last = R.tables()
    own = dict(T=21, atoms=ints(atoms), last=ints(last))
    assert call(A=15, **own) == 0 and call(A=14, **own) == 0
    trp = 18
    if takes_last:
        assert call(A=13, **own) == 1
        blank = last.copy()
        blank[trp] = -1
        assert call(A=13, T=21, atoms=ints(atoms), last=ints(blank)) == 0


# ---- ops and geometry -----------------------------------------------------------------------------------------------------
def chi_args(B=2, N=6, A=15):
    return torch.zeros(B, N, A, 3), torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N, 4)


def test_chi_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import general, ops
    xyz, types, chi = chi_args()
    atoms = general.chi_atom_table()
    check = ops.check_chi_shapes
    check(xyz, types, chi_atoms=atoms)
    check(xyz, types, torch.ones(2, 6, 15, dtype=torch.bool), atoms, chi)
    check(xyz.double(), types.int(), chi_atoms=atoms.numpy())
    bad = [dict(xyz=xyz[0]), dict(xyz=torch.zeros(2, 6, 15, 2)), dict(xyz=xyz.long()),                  # rank, last, dtype
           dict(xyz=torch.zeros(2, 6, 65, 3)), dict(xyz=torch.zeros(2, 6, 6, 3)),                       # A; slot 7 at A = 6
           dict(residue_type=types[:1]), dict(residue_type=types[:, :5]), dict(residue_type=types.float()),
           dict(residue_type=types[0]), dict(atom_mask=torch.ones(2, 6, 14)), dict(atom_mask=torch.ones(2, 5, 15)),
           dict(chi_atoms=None), dict(chi_atoms=atoms[0]), dict(chi_atoms=atoms[:, :, :3]), dict(chi_atoms=atoms.float()),
           dict(chi_atoms=atoms.repeat(2, 1, 1)), dict(chi_atoms=atoms[:0]), dict(chi_atoms=atoms.clamp(min=0)),
           dict(grad_chi=chi[:1]), dict(grad_chi=chi[..., :3]), dict(grad_chi=chi.long()), dict(grad_chi=chi[:, :5]),
           dict(want_chi=False, want_mask=False)]
    for kw in bad:
        args = dict(xyz=xyz, residue_type=types, atom_mask=None, chi_atoms=atoms, grad_chi=None)
        args.update(kw)
        with pytest.raises(ValueError):
            check(**args)
            pytest.fail(f"accepted {sorted(kw)}")
    with pytest.raises(ValueError, match="lives on"):
        check(xyz, types.to("meta"), chi_atoms=atoms)


def test_chi_set_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import general, ops
    xyz, types, chi = chi_args()
    atoms, last = general.chi_atom_table(), general.chi_last_table()
    check = ops.check_chi_set_shapes
    check(xyz, chi, types, chi_atoms=atoms, chi_last=last)
    check(xyz, None, types, torch.ones(2, 6, 15), torch.ones(2, 6, 4, dtype=torch.bool), atoms, last, xyz)
    wrong_last = last.clone()
    wrong_last[14, 0] = 4                                                    # ARG chi1: last below d = 5
    inside = last.clone()
    inside[0, 0] = 5                                                         # ALA has no chi1 to give a range to
    bad = [dict(xyz=xyz[0]), dict(xyz=xyz.long()), dict(xyz=torch.zeros(2, 6, 65, 3)),
           dict(xyz=torch.zeros(2, 6, 13, 3), atom_mask=None),                                          # TRP's range at A = 13
           dict(chi=chi[:1]), dict(chi=chi[..., :3]), dict(chi=chi.long()), dict(chi=chi[:, :5]), dict(chi=chi[0]),
           dict(residue_type=types[:, :5]), dict(residue_type=types.bool()),
           dict(atom_mask=torch.ones(2, 6, 14)), dict(chi_select=torch.ones(2, 6, 3)), dict(chi_select=torch.ones(1, 6, 4)),
           dict(chi_atoms=None), dict(chi_last=None), dict(chi_last=last[:20]), dict(chi_last=last[:, :3]),
           dict(chi_last=last.float()), dict(chi_last=wrong_last), dict(chi_last=inside), dict(chi_last=last.clamp(min=14)),
           dict(grad_out=xyz[:1]), dict(grad_out=xyz.long()), dict(grad_out=xyz[..., :2])]
    for kw in bad:
        args = dict(xyz=xyz, chi=chi, residue_type=types, atom_mask=None, chi_select=None, chi_atoms=atoms, chi_last=last,
                    grad_out=None)
        args.update(kw)
        with pytest.raises(ValueError):
            check(**args)
            pytest.fail(f"accepted {sorted(kw)}")
    with pytest.raises(ValueError, match="lives on"):
        check(xyz, chi.to("meta"), types, chi_atoms=atoms, chi_last=last)


def test_ops_validate_first_then_refuse_cpu_tensors(monkeypatch):
    from protstruc_amd import _lib, general, ops

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_load)
    xyz, types, chi = chi_args()
    tables = dict(chi_atoms=general.chi_atom_table(), chi_last=general.chi_last_table())
    one = dict(chi_atoms=tables["chi_atoms"])
    with pytest.raises(ValueError):
        ops.chi(xyz, types[:, :5], **one)
    with pytest.raises(ValueError):
        ops.chi_backward(xyz, types, chi[..., :3], **one)
    with pytest.raises(ValueError):
        ops.chi_set(xyz, chi, types, chi_atoms=tables["chi_atoms"], chi_last=tables["chi_last"][:5])
    with pytest.raises(ValueError):
        ops.chi_set_backward(xyz, xyz[:1], types, **tables)
    with pytest.raises(TypeError):
        ops.chi(xyz, types, None, tables["chi_atoms"])                      # the tables go by keyword
    with pytest.raises(TypeError):
        ops.chi_set(xyz, chi, types, None, None, tables["chi_atoms"], tables["chi_last"])
    for run in (lambda: ops.chi(xyz, types, **one), lambda: ops.chi_backward(xyz, types, chi, **one),
                lambda: ops.chi_set(xyz, chi, types, **tables), lambda: ops.chi_set_backward(xyz, xyz, types, **tables)):
        with pytest.raises(RuntimeError, match="HIP-only"):
            run()


def test_set_side_chain_torsions_refuses_an_xyz_that_requires_grad():
    from protstruc_amd import geometry
    xyz, types, chi = chi_args()
    with pytest.raises(ValueError, match="constant"):
        geometry.set_side_chain_torsions(xyz.requires_grad_(), chi, types)
    with pytest.raises(ValueError):                                          # validation comes first
        geometry.set_side_chain_torsions(xyz.detach(), chi[..., :3], types)
    with pytest.raises(RuntimeError, match="HIP-only"):
        geometry.set_side_chain_torsions(xyz.detach(), chi.requires_grad_(), types)
    with pytest.raises(RuntimeError, match="HIP-only"):
        geometry.side_chain_torsions(xyz.detach().requires_grad_(), types)


def sig(fn):
    """names and defaults, as tests/test_api_surface.py spells them"""
    return "(" + ", ".join(p.name if p.default is inspect._empty else f"{p.name}={p.default!r}"
                           for p in inspect.signature(fn).parameters.values()) + ")"


def test_signatures_of_the_three_layers():
    from protstruc_amd import StructureBatch, geometry, ops
    kinds = lambda fn: [p.name for p in inspect.signature(fn).parameters.values() if p.kind is p.KEYWORD_ONLY]   # noqa: E731
    assert sig(ops.chi) == "(xyz, residue_type, atom_mask=None, chi_atoms, want_chi=True, want_mask=True)"
    assert sig(ops.chi_backward) == "(xyz, residue_type, grad_chi, atom_mask=None, chi_atoms)"
    assert sig(ops.chi_set) == "(xyz, chi, residue_type, atom_mask=None, chi_select=None, chi_atoms, chi_last, relative=False)"
    assert sig(ops.chi_set_backward) == "(out, grad_out, residue_type, atom_mask=None, chi_select=None, chi_atoms, chi_last)"
    assert kinds(ops.chi) == ["chi_atoms", "want_chi", "want_mask"] and kinds(ops.chi_backward) == ["chi_atoms"]
    assert kinds(ops.chi_set) == ["chi_atoms", "chi_last", "relative"] and kinds(ops.chi_set_backward) == ["chi_atoms", "chi_last"]
    assert sig(ops.check_chi_shapes) == ("(xyz, residue_type, atom_mask=None, chi_atoms=None, grad_chi=None, want_chi=True, "
                                         "want_mask=True)")
    assert sig(ops.check_chi_set_shapes) == ("(xyz, chi, residue_type, atom_mask=None, chi_select=None, chi_atoms=None, "
                                             "chi_last=None, grad_out=None)")
    assert sig(geometry.side_chain_torsions) == "(xyz, residue_type, atom_mask=None, chi_atoms=None)"
    assert sig(geometry.set_side_chain_torsions) == ("(xyz, chi, residue_type, atom_mask=None, chi_select=None, "
                                                     "relative=False, chi_atoms=None, chi_last=None)")
    assert geometry.SideChainTorsions._fields == ("chi", "mask")
    assert sig(StructureBatch.side_chain_torsions) == "(self)"
    assert sig(StructureBatch.chi_pi_periodic) == "(self)"
    assert sig(StructureBatch.with_side_chain_torsions) == "(self, chi, chi_select=None, relative=False)"
    for fn in (geometry.side_chain_torsions, geometry.set_side_chain_torsions):
        assert "ifferentiable" in fn.__doc__
    assert "atan2" in geometry.side_chain_torsions.__doc__ and "xyz.detach()" in geometry.set_side_chain_torsions.__doc__


# ---- StructureBatch -----------------------------------------------------------------------------------------------------------
def small_batch(with_seq=True):
    from protstruc_amd import StructureBatch
    rng = np.random.default_rng(0)
    xyz = torch.from_numpy(rng.normal(size=(2, 5, 15, 3)).astype(np.float32))
    mask = torch.from_numpy(rng.random((2, 5, 15)) < 0.8)
    mask[1, 4] = False                                                       # a padded residue
    mask[0, 2, 1] = False                                                    # a residue without CA: outside the residue mask?
    chain_idx = torch.zeros(2, 5)
    chain_idx[1, 4] = float("nan")
    if not with_seq:
        return StructureBatch(xyz, mask, device="cpu")
    return StructureBatch(xyz, mask, chain_idx, [["A"], ["A"]], [{"A": "RKDWP"}, {"A": "GAFY"}], torch.arange(5).repeat(2, 1),
                          device="cpu")


def test_structure_batch_hands_over_types_and_masks(monkeypatch):
    from protstruc_amd import geometry, pdb
    sb = small_batch()
    seen = {}

    def measure(xyz, residue_type, atom_mask=None, chi_atoms=None):
        seen["measure"] = (xyz, residue_type, atom_mask, chi_atoms)
        return geometry.SideChainTorsions(torch.zeros(2, 5, 4), torch.zeros(2, 5, 4, dtype=torch.bool))

    def turn(xyz, chi, residue_type, atom_mask=None, chi_select=None, relative=False, chi_atoms=None, chi_last=None):
        seen["set"] = (xyz, chi, residue_type, atom_mask, chi_select, relative, chi_atoms, chi_last)
        return xyz + 1.0

    monkeypatch.setattr(geometry, "side_chain_torsions", measure)
    monkeypatch.setattr(geometry, "set_side_chain_torsions", turn)
    present = sb.get_atom_mask() & sb.residue_mask[:, :, None]
    types = sb.get_seq_idx().to(torch.int32)
    assert types[0].tolist() == [pdb.ONE_TO_INDEX[c] for c in "RKDWP"] and types[1, 4] == pdb.ONE_TO_INDEX["X"]

    result = sb.side_chain_torsions()
    assert isinstance(result, geometry.SideChainTorsions)
    xyz, residue_type, atom_mask, chi_atoms = seen["measure"]
    assert xyz.data_ptr() == sb.get_xyz().data_ptr() and xyz.shape == (2, 5, 15, 3)          # zero-copy
    assert residue_type.dtype == torch.int32 and torch.equal(residue_type, types)
    assert atom_mask.dtype == torch.bool and torch.equal(atom_mask, present) and chi_atoms is None

    chi, select = torch.full((2, 5, 4), 0.5), torch.ones(2, 5, 4, dtype=torch.bool)
    before = sb.get_xyz().clone()
    new = sb.with_side_chain_torsions(chi, select, relative=True)
    xyz, got_chi, residue_type, atom_mask, chi_select, relative, chi_atoms, chi_last = seen["set"]
    assert xyz.data_ptr() == sb.get_xyz().data_ptr() and torch.equal(got_chi, chi) and torch.equal(chi_select, select)
    assert torch.equal(residue_type, types) and residue_type.dtype == torch.int32 and torch.equal(atom_mask, present)
    assert relative is True and chi_atoms is None and chi_last is None
    assert torch.equal(sb.get_xyz(), before) and torch.equal(new.get_xyz(), before + 1.0)    # the original is untouched
    assert new is not sb and new.get_seq() is sb.get_seq() and new.get_chain_ids() is sb.get_chain_ids()
    assert torch.equal(new.get_atom_mask(), sb.get_atom_mask()) and torch.equal(new.residue_mask, sb.residue_mask)
    assert torch.equal(new.chain_idx.nan_to_num(-1), sb.chain_idx.nan_to_num(-1)) and new.residue_idx is sb.residue_idx
    sb.with_side_chain_torsions(chi.numpy())
    assert seen["set"][4] is None and seen["set"][5] is False and isinstance(seen["set"][1], torch.Tensor)

    periodic = sb.chi_pi_periodic()
    assert periodic.shape == (2, 5, 4) and periodic.dtype == torch.bool
    assert periodic[0, 2].tolist() == [False, True, False, False] and periodic[1, 2].tolist() == [False, True, False, False]
    assert periodic.sum() == 3                                               # D of the first, F and Y of the second


def test_structure_batch_without_a_sequence_raises():
    sb = small_batch(with_seq=False)
    for run in (sb.side_chain_torsions, sb.chi_pi_periodic, lambda: sb.with_side_chain_torsions(torch.zeros(2, 5, 4))):
        with pytest.raises(ValueError, match="sequence"):
            run()


# ---- the timing tool ----------------------------------------------------------------------------------------------------------
def test_the_timing_tool_composes_the_same_definition():
    from tools import chi_time
    assert (chi_time.B, chi_time.N, chi_time.A, chi_time.MASKED) == (128, 512, 15, 0.10)
    assert tuple(chi_time.STEPS) == ("events", "torch") and set(chi_time.STEP_TIMEOUT_S) == {"events", "torch"}
    case = R.synthetic_case(3, 33, 15, seed=5)
    atoms, last = R.tables()
    xyz, mask, types = torch.from_numpy(case.xyz), torch.from_numpy(case.mask), torch.from_numpy(case.types)
    chi, defined = chi_time.composed_measure(xyz, mask, types, torch.from_numpy(atoms))
    ref, ref_defined = R.measure(case.xyz, case.types, case.mask, atoms)
    assert chi.dtype == torch.float32 and (defined.numpy() == ref_defined).all() and ref_defined.sum() > 30
    assert circular(chi.numpy(), ref).max() <= 1e-4 and (chi.numpy()[~ref_defined] == 0).all()
    want = np.random.default_rng(6).uniform(-np.pi, np.pi, size=ref.shape).astype(np.float32)
    out = chi_time.composed_set(xyz, torch.from_numpy(want), mask, types, torch.from_numpy(atoms), torch.from_numpy(last))
    t = R.set_chi(case.xyz, want, case.types, case.mask, atoms, last)
    expected = np.where(t.moved[..., None], t.out, clean(case))
    assert out.dtype == torch.float32 and t.moved.sum() > 30
    assert np.abs(out.numpy() - expected).max() <= 1e-4
    # the tool's own inputs: every one of the 20 types, a tenth of the atoms masked with NaN under the mask
    x, m, ty, c = chi_time.inputs(2)
    assert x.shape == (2, 512, 15, 3) and x.dtype == np.float32 and ty.dtype == np.int32 and c.shape == (2, 512, 4)
    assert sorted(set(ty.ravel().tolist())) == list(range(20)) and 0.08 < 1 - m.mean() < 0.12
    assert np.isnan(x[~m]).all() and not np.isnan(x[m]).any()
