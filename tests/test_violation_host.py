"""Host-side checks of the structural-violation terms: the yardstick itself (tests/violation_ref.py) and the conditions
its cases must meet, the C ABI's surface, the argument validation of ``ops.clash`` / ``ops.peptide_bond`` and their
backwards, the radius table and the link / junction construction of ``StructureBatch``.  No GPU needed."""
import ctypes
import inspect

import pytest
import torch

from tests import violation_ref as R


def two_points(distance=2.0, **kw):
    x = torch.tensor([[[0.0, 0, 0], [distance, 0, 0]]], dtype=torch.float64)
    return R.clash(x, torch.full((1, 2), 1.7, dtype=torch.float64), **kw)


def test_yardstick_on_hand_computed_examples():
    """Two carbons at 2.0 A: s = 3.4 - 1.5 = 1.9 < 2.0, no clash; at 1.5 A: v = 0.4 in both owners' sums.  With
    tolerance 0 at 2.0 A: v = 3.4 - 2.0 = 1.4 each, so E pooled over both owners is 2 (3.4 - 0 - 2.0)."""
    E, n = two_points(2.0)
    assert float(E.sum()) == 0 and float(n.sum()) == 0
    E, n = two_points(1.5)
    assert torch.allclose(E, torch.full((1, 2), 0.4, dtype=torch.float64), atol=1e-9) and torch.equal(n, torch.ones(1, 2, dtype=torch.float64))
    E, n = two_points(2.0, tolerance=0.0)
    assert abs(float(E.sum()) - 2 * (3.4 - 0.0 - 2.0)) < 1e-9
    # the issue's example, E = 2 (3.4 - 1.5 - 2.0) pooled, is negative before the max: no clash
    assert 2 * (3.4 - 1.5 - 2.0) < 0 and float(two_points(2.0)[0].sum()) == 0
    for kw in (dict(groups=torch.tensor([[7, 7]])), dict(link=torch.tensor([[3, 3]])), dict(point_mask=torch.tensor([[1, 0]]))):
        E, n = two_points(1.5, **kw)
        assert float(E.sum()) == 0 and float(n.sum()) == 0, kw
    E, n = two_points(1.5, groups=torch.tensor([[7, 8]]), link=torch.tensor([[-1, -1]]))   # -1 links nothing
    assert float(n.sum()) == 2
    E, n = two_points(1.5, link=torch.tensor([[3, 4]]))
    assert float(n.sum()) == 2


def test_bond_yardstick_on_a_hand_computed_example():
    """C at the origin, N' at 1.625 on x: l = 1.625, viol_0 = |1.625 - 1.329| - 12 * 0.014 = 0.128; proline: |1.625 - 1.341| -
    12 * 0.016 = 0.092.  CA at (-1, 1, 0): cos(CA-C-N') = -1/sqrt 2, |.-(-0.4473)| - 12 * 0.0311 < 0: no violation."""
    xyz = torch.zeros(1, 2, 3, 3, dtype=torch.float64)
    xyz[0, 0, 1] = torch.tensor([-1.0, 1.0, 0.0])          # CA
    xyz[0, 1, 0] = torch.tensor([1.625, 0.0, 0.0])           # N'
    xyz[0, 1, 1] = torch.tensor([2.375, 1.25, 0.0])           # CA'
    viol = R.peptide_bond(xyz, eps=0.0)
    assert viol.shape == (1, 2, 3) and (viol[0, 1] == 0).all()
    assert abs(float(viol[0, 0, 0]) - (abs(1.625 - 1.329) - 12 * 0.014)) < 1e-12 and float(viol[0, 0, 1]) == 0
    cn = float((torch.tensor([-1.0, 0.0], dtype=torch.float64) * torch.tensor([0.75, 1.25], dtype=torch.float64) / (0.75 ** 2 + 1.25 ** 2) ** 0.5).sum())
    assert abs(float(viol[0, 0, 2]) - max(0.0, abs(cn + 0.5203) - 12 * 0.0353)) < 1e-12
    pro = R.peptide_bond(xyz, next_is_proline=torch.tensor([[1, 0]]), eps=0.0)
    assert abs(float(pro[0, 0, 0]) - (abs(1.625 - 1.341) - 12 * 0.016)) < 1e-12
    assert (R.peptide_bond(xyz, junction_mask=torch.tensor([[0, 1]])) == 0).all()
    assert abs(float(R.peptide_bond(xyz, eps=0.0, tau=0.0)[0, 0, 0]) - (1.625 - 1.329)) < 1e-12


def test_yardstick_gradients_pass_finite_differences():
    case = R.random_case(2, 9, "p60", groups=2, link=True, seed=7)
    x = torch.where(case.valid()[..., None], case.points, torch.zeros_like(case.points)).double().requires_grad_(True)
    w = torch.where(case.valid(), case.grad_E, torch.zeros_like(case.grad_E)).double()
    assert torch.autograd.gradcheck(lambda p: (R.clash(p, case.radius.double(), **case.kwargs())[0] * w).sum(), (x,),
                                    eps=1e-6, atol=1e-7, rtol=1e-5)
    g = R.gradient(case)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0 and (g[~case.valid()] == 0).all()
    bond = R.bond_case(N=6, keep=0.8, seed=9)
    xb = torch.nan_to_num(bond.xyz[:, :, :3]).double().requires_grad_(True)
    wb = torch.where(bond.valid()[..., None], bond.grad_viol, torch.zeros_like(bond.grad_viol)).double()
    assert torch.autograd.gradcheck(lambda p: (R.peptide_bond(p, **bond.kwargs()) * wb).sum(), (xb,), eps=1e-6, atol=1e-7,
                                    rtol=1e-5)
    gb = R.bond_gradient(bond)
    assert torch.isfinite(gb).all() and float(gb.abs().max()) > 0 and (gb[:, :, 3:] == 0).all()


@pytest.mark.parametrize("name", list(R.accuracy_cases()))
def test_clash_cases_meet_their_input_conditions(name):
    """Asserted in float64: a case with M >= 63 has more than 25 % of its valid points in a clash (measured 75-100 %), and
    at most 2 % of the points are open (measured at most 0.6 %)."""
    kw = R.accuracy_cases()[name]
    assert kw["B"] == 3
    case = R.random_case(**kw)
    valid = case.valid()
    if case.point_mask is not None:
        assert case.points[~valid].isnan().all() and case.radius[~valid].isnan().all()
    E, n = R.forward(case)
    n_lo, n_hi, open_ = R.brackets(case)
    assert torch.isfinite(E).all() and (n_lo <= n).all() and (n <= n_hi).all()
    assert (E[~valid] == 0).all() and (n[~valid] == 0).all()
    if case.M >= 63:
        assert float(((E > 0) & valid).sum()) > 0.25 * float(valid.sum())
        steps = (case.points[0, 1:] - case.points[0, :-1])[valid[0, 1:] & valid[0, :-1]].norm(dim=-1)
        assert torch.allclose(steps, torch.full_like(steps, 1.5), atol=1e-4)
    assert float((open_ & valid).sum()) <= 0.02 * max(float(valid.sum()), 1)
    if name == "M=130 structure masked":
        assert not valid[-1].any()
    if case.link is not None:       # the link takes pairs away: the last point of a group touches the first of the next
        assert float(R.clash(case.points.double(), case.radius.double(), **{**case.kwargs(), "link": None})[1].sum()) > float(n.sum())


@pytest.mark.parametrize("name", list(R.bond_cases()))
def test_bond_cases_meet_their_input_conditions(name):
    """Asserted in float64: every full-length case has more than 10 % of its valid junctions non-zero in each of the three
    terms (measured at 0.3 A: 68 %, 31-36 % and 26-28 %); the chain break is no junction."""
    case = R.bond_case(**R.bond_cases()[name])
    assert case.B == 3
    viol, valid = R.bond_forward(case), case.valid()
    assert torch.isfinite(viol).all() and (viol[~valid] == 0).all()
    if case.N == 229:
        for t in range(3):
            assert float(((viol[..., t] > 0) & valid).sum()) > 0.10 * float(valid.sum()), t
        chain = R.pdb_batch().chain_idx[0]
        brk = int((chain[1:] != chain[:-1]).nonzero()[0])
        assert not valid[:, brk].any() and case.xyz.isnan().any()
    if name == "N=229 p80":
        gone = case.xyz[:, :, 1].isnan().any(-1)
        assert 0.1 < float(gone.float().mean()) < 0.3 and not valid[gone].any()
    if name == "N=229":
        assert case.next_is_proline.any()


def test_source_is_built_and_the_constants_are_the_yardsticks():
    """(declared, exported, bound: tests/test_capi_symbols.py)"""
    from protstruc_amd import build, ops
    assert any(src.endswith("violation.hip") for src in build.sources())
    assert any(dep.endswith("violation.hip") for dep in build._deps())        # the source hash covers the new file
    assert ops.VDW_RADII == {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8} and ops.CLASH_TOLERANCE == 1.5
    assert ops.PEPTIDE_BOND == R.BOND


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; empty problems launch nothing (no pointer is dereferenced but
    the host array of constants)."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    nan, inf = float("nan"), float("inf")

    def forward(pts=fake, radius=fake, tolerance=1.5, eps=1e-10, E=fake, n=fake, B=1, M=8):
        return lib.ps_clash_f32(pts, radius, None, None, None, tolerance, eps, E, n, B, M, None)

    def backward(pts=fake, radius=fake, tolerance=1.5, eps=1e-10, w=fake, out=fake, B=1, M=8):
        return lib.ps_clash_backward_f32(pts, radius, None, None, None, tolerance, eps, w, out, B, M, None)

    for call in (forward, backward):
        assert call(B=0) == 0 and call(M=0) == 0
        assert call(pts=None) == 1 and call(radius=None) == 1
        assert call(tolerance=nan) == 1 and call(tolerance=inf) == 1 and call(tolerance=-inf) == 1
        assert call(eps=-1.0) == 1 and call(eps=nan) == 1 and call(eps=inf) == 1
        assert call(B=65536) == 1 and call(B=-1) == 1 and call(M=-1) == 1 and call(M=2 ** 30 + 1) == 1
    assert forward(E=None) == 1 and forward(n=None) == 1
    assert backward(w=None) == 1 and backward(out=None) == 1

    good = (ctypes.c_float * 12)(1.329, 0.014, 1.341, 0.016, -0.4473, 0.0311, -0.5203, 0.0353, 12.0, 1e-10, 0, 0)

    def constants(index, value):
        k = (ctypes.c_float * 12)(*good)
        k[index] = value
        return k

    def bond(xyz=fake, slots=(0, 1, 2), k=good, viol=fake, B=1, N=8, A=15):
        return lib.ps_peptide_bond_f32(xyz, None, None, *slots, k, viol, B, N, A, None)

    def bond_backward(xyz=fake, slots=(0, 1, 2), k=good, viol=fake, out=fake, B=1, N=8, A=15):
        return lib.ps_peptide_bond_backward_f32(xyz, None, None, *slots, k, viol, out, B, N, A, None)

    for call in (bond, bond_backward):
        assert call(B=0) == 0 and call(N=0) == 0
        assert call(xyz=None) == 1 and call(k=None) == 1 and call(viol=None) == 1
        assert call(B=-1) == 1 and call(N=-1) == 1 and call(A=0) == 1 and call(B=65536, N=65536) == 1
        assert call(slots=(0, 1, 15)) == 1 and call(slots=(-1, 1, 2)) == 1 and call(slots=(0, 0, 2)) == 1 and call(slots=(0, 1, 1)) == 1
        assert call(k=constants(0, nan)) == 1 and call(k=constants(4, inf)) == 1
        for index in (1, 3, 5, 7, 8, 9):
            assert call(k=constants(index, -1.0)) == 1, index
    assert bond_backward(out=None) == 1


def clash_args(B=2, M=9):
    g = torch.Generator().manual_seed(1)
    return [torch.randn(B, M, 3, generator=g), torch.full((B, M), 1.7)]


def test_clash_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_clash_shapes
    a = clash_args()
    pm, gr = torch.ones(2, 9, dtype=torch.bool), torch.arange(9).expand(2, 9)
    check(*a)
    check(*a, pm, gr, gr, 0.0, 0.0, torch.ones(2, 9))
    check(*a, tolerance=-1.0)
    bad = [(a[0][:, :-1], a[1]), (a[0].long(), a[1]), (a[0][0], a[1]), (a[0].reshape(2, 9, 3, 1), a[1]), (a[0][..., :2], a[1]),
           (a[0], a[1][:, :-1]), (a[0], a[1].long()), (a[0], a[1][..., None])]
    for args in bad:
        with pytest.raises(ValueError):
            check(*args)
    for kw in (dict(point_mask=pm[:, :8]), dict(groups=gr[:1]), dict(groups=gr.float()), dict(groups=pm), dict(link=gr[:, :8]),
               dict(link=gr.float()), dict(link=pm), dict(tolerance=float("nan")), dict(tolerance=float("inf")),
               dict(eps=-1e-9), dict(eps=float("inf")), dict(eps=float("nan")), dict(grad_E=torch.ones(2, 8)),
               dict(grad_E=torch.ones(2, 9, dtype=torch.long)), dict(point_mask=pm.to("meta")), dict(link=gr.to("meta"))):
        with pytest.raises(ValueError):
            check(*a, **kw)


def test_peptide_bond_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_peptide_bond_shapes
    xyz, jm = torch.randn(2, 7, 5, 3), torch.ones(2, 7, dtype=torch.bool)
    check(xyz)
    check(xyz, jm, jm, 0, 1, 2, 0.0, torch.ones(2, 7, 3), tau=3.0, l0=1.33)
    for bad in (xyz[0], xyz[..., :2], xyz.long(), xyz[..., None]):
        with pytest.raises(ValueError):
            check(bad)
    for kw in (dict(junction_mask=jm[:, :6]), dict(next_is_proline=jm[:1]), dict(n_slot=5), dict(c_slot=-1), dict(ca_slot=0),
               dict(c_slot=1), dict(eps=-1.0), dict(eps=float("nan")), dict(tau=-1.0), dict(sigma_l=-0.1), dict(l0=float("inf")),
               dict(cos_cacn=float("nan")), dict(stiffness=1.0), dict(grad_viol=torch.ones(2, 7)),
               dict(grad_viol=torch.ones(2, 7, 3, dtype=torch.long)), dict(junction_mask=jm.to("meta"))):
        with pytest.raises(ValueError):
            check(xyz, **kw)


def test_ops_validate_first_then_refuse_cpu_tensors():
    from protstruc_amd import ops
    a = clash_args()
    xyz = torch.randn(2, 7, 5, 3)
    with pytest.raises(ValueError):
        ops.clash(*a, eps=-1.0)
    with pytest.raises(ValueError):
        ops.clash_backward(*a, torch.ones(2, 8))
    with pytest.raises(ValueError):
        ops.peptide_bond(xyz, tau=-1.0)
    with pytest.raises(ValueError):
        ops.peptide_bond_backward(xyz, torch.ones(2, 7))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.clash(*a)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.clash_backward(*a, torch.ones(2, 9))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.peptide_bond(xyz)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.peptide_bond_backward(xyz, torch.ones(2, 7, 3))


def test_signatures_of_the_layers_above():
    from protstruc_amd import StructureBatch, geometry, ops
    p = inspect.signature(geometry.steric_clash).parameters
    assert list(p) == ["points", "radius", "point_mask", "groups", "link", "tolerance", "eps", "reduction"]
    assert (p["point_mask"].default, p["groups"].default, p["link"].default, p["tolerance"].default, p["eps"].default,
            p["reduction"].default) == (None, None, None, 1.5, 1e-10, "point")
    p = inspect.signature(geometry.peptide_bond_violations).parameters
    assert list(p)[:3] == ["xyz", "junction_mask", "next_is_proline"] and p["constants"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(StructureBatch.steric_clashes).parameters
    assert list(p) == ["self", "atoms", "tolerance", "radii", "per_residue"]
    assert (p["atoms"].default, p["tolerance"].default, p["radii"].default, p["per_residue"].default) == ("all", 1.5, None, True)
    p = inspect.signature(StructureBatch.structural_violation_loss).parameters
    assert list(p) == ["self", "tolerance", "tau"] and (p["tolerance"].default, p["tau"].default) == (1.5, 12.0)
    assert hasattr(StructureBatch, "peptide_bond_violations")
    for name in ("clash", "clash_backward", "peptide_bond", "peptide_bond_backward", "check_clash_shapes", "check_peptide_bond_shapes"):
        assert callable(getattr(ops, name))
    with pytest.raises(ValueError):
        geometry.steric_clash(*clash_args(), reduction="mean")


def test_autograd_wrappers_hand_the_upstream_gradient_to_the_backward_ops(monkeypatch):
    """Host-only: the four ops are replaced by CPU stand-ins (the restatement; recorders)."""
    from protstruc_amd import geometry, ops
    x, r = clash_args()
    x = (2 * x).requires_grad_()
    seen = []
    monkeypatch.setattr(ops, "clash", lambda p, rad, pm, gr, lk, *, tolerance, eps: R.clash(p.detach(), rad, pm, gr, lk, tolerance, eps))

    def clash_backward(p, rad, grad_E, pm, gr, lk, *, tolerance, eps):
        ops.check_clash_shapes(p, rad, pm, gr, lk, tolerance, eps, grad_E)
        seen.append(grad_E.clone())
        return torch.ones_like(p)

    monkeypatch.setattr(ops, "clash_backward", clash_backward)
    pm = torch.ones(2, 9, dtype=torch.bool)
    pm[0, :3] = False
    E, n = geometry.steric_clash(x, r, pm, reduction="none")
    assert E.grad_fn is not None and n.grad_fn is None and not n.requires_grad
    want = R.clash(x.detach(), r, pm)[0]
    assert torch.equal(geometry.steric_clash(x, r, pm), want)
    assert torch.allclose(geometry.steric_clash(x, r, pm, reduction="structure"), want.sum(-1) / torch.tensor([6.0, 9.0]))
    assert torch.allclose(geometry.steric_clash(x, r, reduction="structure"), R.clash(x.detach(), r)[0].sum(-1) / 9)
    (3.0 * E).sum().backward()
    assert len(seen) == 1 and torch.equal(seen[0], torch.full((2, 9), 3.0)) and torch.equal(x.grad, torch.ones_like(x))

    xyz = torch.randn(2, 7, 5, 3).requires_grad_()
    got = {}
    monkeypatch.setattr(ops, "peptide_bond", lambda p, jm, pro, **kw: (got.update(forward=kw), torch.ones(2, 7, 3))[1])
    monkeypatch.setattr(ops, "peptide_bond_backward", lambda p, g, jm, pro, **kw: (got.update(backward=kw, grad=g.clone()), torch.ones_like(p))[1])
    viol = geometry.peptide_bond_violations(xyz, tau=3.0)
    (2.0 * viol).sum().backward()
    assert got["forward"] == got["backward"] == dict(n_slot=0, ca_slot=1, c_slot=2, eps=1e-10, tau=3.0)
    assert torch.equal(got["grad"], torch.full((2, 7, 3), 2.0)) and torch.equal(xyz.grad, torch.ones_like(xyz))


def test_radius_table():
    from protstruc_amd.general import vdw_radius_table
    from protstruc_amd.pdb import ONE_TO_INDEX
    table = vdw_radius_table()
    assert table.shape == (21, 15) and table.dtype == torch.float32
    f = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    assert (table[:, 14] == f(1.52)).all()                                  # OXT in every type
    assert (table[:, 0] == f(1.55)).all() and (table[:, 1] == f(1.7)).all() and (table[:, 2] == f(1.7)).all() and (table[:, 3] == f(1.52)).all()
    assert table[ONE_TO_INDEX["G"], 4] == 0 and (table[ONE_TO_INDEX["G"], 4:14] == 0).all()   # glycine has no CB
    assert table[ONE_TO_INDEX["C"], 5] == f(1.8) and table[ONE_TO_INDEX["M"], 6] == f(1.8)    # SG, SD
    assert (table[ONE_TO_INDEX["W"], :14] > 0).all()                        # tryptophan fills every slot
    assert table[ONE_TO_INDEX["K"], 8] == f(1.55) and table[ONE_TO_INDEX["S"], 5] == f(1.52)   # NZ, OG
    x = table[ONE_TO_INDEX["X"]]
    assert (x[:5] > 0).all() and (x[5:14] == 0).all() and x[14] == f(1.52)


def test_links_and_junctions_on_a_two_chain_toy_batch():
    """Residues 0-2 are chain 0, residues 3-4 chain 1, residue 5 is padding; residue 1 lacks its C; CYS at 0 and 3."""
    from protstruc_amd.structure_batch import clash_links, valid_junctions
    A = 6
    present = torch.ones(1, 6, A, dtype=torch.bool)
    present[0, 1, 2] = False
    present[0, 5] = False
    chain = torch.tensor([[0.0, 0, 0, 1, 1, float("nan")]])
    j = valid_junctions(present, chain)
    assert j.tolist() == [[True, False, False, True, False, False]]          # 1 lacks C; 2 -> 3 changes chain; 4 -> padding
    assert valid_junctions(present, chain, torch.tensor([[0.0, 1, 2, 3, 5, float("nan")]])).tolist() == [[True, False, False, False, False, False]]
    assert valid_junctions(present[:, :1], chain[:, :1]).tolist() == [[False]]
    link = clash_links(j, A, torch.tensor([[True, False, False, True, False, False]])).reshape(1, 6, A)
    want = torch.full((1, 6, A), -1, dtype=torch.int32)
    want[0, 0, 2] = want[0, 1, 0] = 0
    want[0, 3, 2] = want[0, 4, 0] = 3
    want[0, 0, 5] = want[0, 3, 5] = 6
    assert link.dtype == torch.int32 and torch.equal(link, want)
    assert (clash_links(j, A).reshape(1, 6, A)[:, :, 5] == -1).all()


def test_structure_batch_refuses_side_chains_without_a_sequence():
    from protstruc_amd import StructureBatch
    sb = StructureBatch.from_xyz(torch.randn(1, 4, 15, 3), device="cpu")
    with pytest.raises(ValueError, match="radii"):
        sb.steric_clashes()
    with pytest.raises(ValueError):
        sb.steric_clashes(atoms=("N", "CA"), radii=torch.ones(1, 4, 14))
    with pytest.raises(RuntimeError, match="HIP-only"):
        sb.steric_clashes(atoms=("N", "CA", "C", "O", "CB"))
