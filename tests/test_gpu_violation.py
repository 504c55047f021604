"""GPU tests of the structural-violation terms (ps_clash_f32, ps_clash_backward_f32, ps_peptide_bond_f32,
ps_peptide_bond_backward_f32; ops.clash, ops.peptide_bond and their backwards; geometry.steric_clash,
geometry.peptide_bond_violations; StructureBatch.steric_clashes, .peptide_bond_violations, .structural_violation_loss).

Yardstick: the float64 evaluation of the torch restatement in tests/violation_ref.py.

E, viol and the gradients use the error measure and the margin of tests/test_gpu_fape.py and tests/test_gpu_lddt.py: with
e(row) = the row's largest error divided by the row's largest float64 |value| and E = the worst row,
E_kernel <= 4 E_f32, where E_f32 is the SAME restatement run in float32 on the CPU; a row whose float64 value is
identically zero must be exactly zero.  Rows are points (clash) or residues (bond, end to end).  The clash energy is
continuous, so every point counts for it; the count n must lie in the float64 bracket in which every pair within 1e-4 of
s = d is counted out and in (equality wherever the bracket is closed); the points that own such a pair, and the residues
of a junction within 1e-4 of a kink, are left out of the GRADIENT's error, for the kernel and the float32 restatement
alike, because the gradient jumps there.
"""
import functools

import pytest
import torch

from tests import violation_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 4.0
CASES = R.accuracy_cases()
BOND_CASES = R.bond_cases()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


@functools.lru_cache(maxsize=None)
def reference(name):
    """The clash case and its CPU references, computed once and shared (never modified) by the tests that need them."""
    case = R.random_case(**CASES[name])
    n_lo, n_hi, open_ = R.brackets(case)
    return {"case": case, "n_lo": n_lo, "n_hi": n_hi, "open": open_,
            "E64": R.forward(case)[0], "E32": R.forward(case, torch.float32)[0],
            "grad64": R.gradient(case), "grad32": R.gradient(case, torch.float32)}


@functools.lru_cache(maxsize=None)
def bond_reference(name):
    case = R.bond_case(**BOND_CASES[name])
    return {"case": case, "open": R.bond_open(case),
            "viol64": R.bond_forward(case), "viol32": R.bond_forward(case, torch.float32),
            "grad64": R.bond_gradient(case), "grad32": R.bond_gradient(case, torch.float32)}


def cuda(t):
    return None if t is None else t.cuda()


def gpu_args(case):
    return [case.points.cuda(), case.radius.cuda()], dict(point_mask=cuda(case.point_mask), groups=cuda(case.groups),
                                                          link=cuda(case.link), tolerance=case.tolerance, eps=case.eps)


def bond_args(case):
    return case.xyz.cuda(), dict(junction_mask=cuda(case.junction_mask), next_is_proline=cuda(case.next_is_proline))


def closed(t, open_):
    """t with the open rows zeroed (a zero row against a zero row has e = 0)."""
    keep = ~open_
    return torch.where(keep.reshape(keep.shape + (1,) * (t.dim() - keep.dim())), t.detach().cpu().double(), 0.0)


def check_rows(name, what, got, want, f32, open_=None, floor=0.0):
    if open_ is None:
        open_ = torch.zeros(want.shape[:2], dtype=torch.bool)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.isfinite(got).all(), (name, what)
    e_kernel, e_f32 = R.worst_error(closed(got, open_), closed(want, open_)), R.worst_error(closed(f32, open_), closed(want, open_))
    print(f"{name} {what}: E_kernel = {e_kernel:.3e}  E_f32 = {e_f32:.3e}  ratio = {e_kernel / e_f32 if e_f32 else float('nan'):.2f}")
    assert e_kernel <= MARGIN * max(e_f32, floor), f"{name} {what}: E_kernel {e_kernel:.3e} > {MARGIN} x E_f32 {e_f32:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_clash_forward_accuracy(ops, name):
    ref = reference(name)
    case = ref["case"]
    args, kw = gpu_args(case)
    E, n = ops.clash(*args, **kw)
    assert E.shape == (case.B, case.M) and E.dtype == torch.float32 and n.shape == E.shape and n.dtype == torch.float32
    check_rows(name, "E", E.cpu(), ref["E64"], ref["E32"])
    n = n.cpu().double()
    print(f"{name} n: {int((ref['open'] & case.valid()).sum())} open points of {int(case.valid().sum())}")
    assert ((ref["n_lo"] <= n) & (n <= ref["n_hi"])).all(), f"{name}: n outside its bracket"   # equality where lo == hi
    assert (E.cpu()[~case.valid()] == 0).all() and (n[~case.valid()] == 0).all()
    assert (E.cpu()[n == 0] == 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_clash_backward_accuracy(ops, name):
    ref = reference(name)
    case = ref["case"]
    args, kw = gpu_args(case)
    got = ops.clash_backward(*args, case.grad_E.cuda(), **kw)
    check_rows(name, "grad_points", got.cpu(), ref["grad64"], ref["grad32"], ref["open"])
    assert (got.cpu()[~case.valid()] == 0).all()
    if case.point_mask is not None:                                      # NaN upstream at a masked point never arrives either
        dirty = torch.where(case.point_mask, case.grad_E, torch.full_like(case.grad_E, float("nan")))
        assert torch.equal(ops.clash_backward(*args, dirty.cuda(), **kw), got)


@pytest.mark.parametrize("name", list(BOND_CASES))
def test_peptide_bond_accuracy(ops, name):
    ref = bond_reference(name)
    case = ref["case"]
    xyz, kw = bond_args(case)
    viol = ops.peptide_bond(xyz, **kw)
    check_rows(name, "viol", viol.cpu(), ref["viol64"], ref["viol32"])
    assert (viol.cpu()[~case.valid()] == 0).all()
    grad = ops.peptide_bond_backward(xyz, case.grad_viol.cuda(), **kw)
    print(f"{name}: {int(ref['open'].sum())} open residues of {case.B * case.N}")
    check_rows(name, "grad_xyz", grad.cpu(), ref["grad64"], ref["grad32"], ref["open"])
    assert (grad[:, :, 3:] == 0).all()
    # NaN upstream at an invalid junction never arrives, and neither does NaN at the atoms no valid junction reads
    dirty = torch.where(case.valid()[..., None], case.grad_viol, torch.full_like(case.grad_viol, float("nan")))
    assert torch.equal(ops.peptide_bond_backward(xyz, dirty.cuda(), **kw), grad)
    unread = (ref["grad64"] == 0).all(-1) & ~case.xyz.isnan().any(-1)
    assert (grad.cpu()[unread] == 0).all()


def test_deterministic(ops):
    case = reference("M=600 p60")["case"]
    args, kw = gpu_args(case)
    w = case.grad_E.cuda()
    assert all(torch.equal(a, b) for a, b in zip(ops.clash(*args, **kw), ops.clash(*args, **kw)))
    assert torch.equal(ops.clash_backward(*args, w, **kw), ops.clash_backward(*args, w, **kw))
    bond = bond_reference("N=229 p80")["case"]
    xyz, kw = bond_args(bond)
    g = bond.grad_viol.cuda()
    assert torch.equal(ops.peptide_bond(xyz, **kw), ops.peptide_bond(xyz, **kw))
    assert torch.equal(ops.peptide_bond_backward(xyz, g, **kw), ops.peptide_bond_backward(xyz, g, **kw))


def test_finite_difference_step_of_one_point(ops):
    """L = sum w E through the forward kernel at x -+ h e_k for one point of the smooth interior (none of its pairs within
    0.05 of s = d, so none crosses the kink during the step of h = 2^-8) against K18.  Error budget of the central
    difference: the E that change are rounded to float32 (half an ulp of a value below 16, 2^-21) and weighted by |w|, over
    2 h; the truncation h^2 / 6 |L'''| stays below 1e-4."""
    ref = reference("M=257")
    case = ref["case"]
    margin, allowed = R.pair_terms(case.points.double(), case.radius.double(), **case.kwargs())
    near = (allowed & (margin.abs() < 0.05)).any(-1)
    E64 = ref["E64"]
    b = 1
    i = int(((E64[b] > 0.5) & ~near[b]).nonzero()[0])
    args, kw = gpu_args(case)
    w = case.grad_E.double()
    grad = ops.clash_backward(*args, case.grad_E.cuda(), **kw).cpu().double()
    h = 2.0 ** -8
    assert float(E64.max()) < 16
    for k in range(3):
        sides = []
        for sign in (1.0, -1.0):
            x = case.points.clone()
            x[b, i, k] += sign * h
            sides.append(ops.clash(x.cuda(), args[1], **kw)[0].cpu().double())
        changed = sides[0] != sides[1]
        fd = float(((sides[0] - sides[1]) * w).sum()) / (2 * h)
        budget = float((changed * w.abs()).sum()) * 2.0 ** -21 * 2 / (2 * h) + 1e-4
        print(f"finite difference, component {k}: kernel {float(grad[b, i, k]):.6f}  difference {fd:.6f}  budget {budget:.2e}")
        assert int(changed.sum()) >= 2 and abs(fd - float(grad[b, i, k])) <= budget
    assert float(grad[b, i].abs().max()) > 0.1


def test_zero_cases_are_exactly_zero(ops):
    """Points 5 A apart on a grid do not clash; the file's own coordinates with tau = 1000 violate nothing."""
    grid = torch.stack(torch.meshgrid(*(torch.arange(5.0),) * 3, indexing="ij"), -1).reshape(1, 125, 3).mul(5.0).cuda()
    radius = torch.full((1, 125), 1.8, device="cuda")
    E, n = ops.clash(grid, radius)
    assert (E == 0).all() and (n == 0).all()
    assert (ops.clash_backward(grid, radius, torch.ones(1, 125, device="cuda")) == 0).all()
    case = R.bond_case(noise=0.0, seed=1)
    xyz, kw = bond_args(case)
    assert (ops.peptide_bond(xyz, tau=1000.0, **kw) == 0).all()
    assert (ops.peptide_bond_backward(xyz, case.grad_viol.cuda(), tau=1000.0, **kw) == 0).all()
    real = ops.peptide_bond(xyz, **kw)                                   # a crystal structure keeps to 12 sigma almost everywhere
    assert float((real > 0).any(-1).float().mean()) < 0.05


def test_empty_inputs_launch_nothing(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for B, M in ((0, 5), (2, 0)):
        E, n = ops.clash(z(B, M, 3), z(B, M))
        assert E.shape == (B, M) and n.shape == (B, M)
        assert ops.clash_backward(z(B, M, 3), z(B, M), z(B, M)).shape == (B, M, 3)
        assert ops.peptide_bond(z(B, M, 4, 3)).shape == (B, M, 3)
        assert ops.peptide_bond_backward(z(B, M, 4, 3), z(B, M, 3)).shape == (B, M, 4, 3)


def pdb_copies(B=2, N=130, noise=0.3, seed=31):
    """The first N residues of 15c8_HL (chain break included) with all atoms, B noisy copies, as the arguments of
    StructureBatch (on the CPU): NaN at missing atoms."""
    sb = R.pdb_batch()
    g = torch.Generator().manual_seed(seed)
    xyz = sb.xyz[:, :N].expand(B, -1, -1, -1) + noise * torch.randn(B, N, 15, 3, generator=g)
    assert int(sb.chain_idx[0, :N].max()) == 1 and xyz.isnan().any()
    seq = {c: s[:max(0, N - sum(len(sb.seq[0][p]) for p in sb.chain_ids[0][:k]))] for k, (c, s) in
           enumerate((c, sb.seq[0][c]) for c in sb.chain_ids[0])}
    return dict(xyz=xyz.contiguous(), atom_mask=sb.atom_mask[:, :N].expand(B, -1, -1).contiguous(),
                chain_idx=sb.chain_idx[:, :N].expand(B, -1).contiguous(), chain_ids=[sb.chain_ids[0]] * B, seq=[seq] * B)


def test_end_to_end_structural_violation_loss(ops):
    """xyz.requires_grad_() -> structural_violation_loss().sum().backward() against the float64 restatement built from
    the package's own radius table, junctions and links (checked on the host); rows of the gradient are residues."""
    from protstruc_amd import StructureBatch
    from protstruc_amd.general import vdw_radius_table
    from protstruc_amd.pdb import ONE_TO_INDEX
    from protstruc_amd.structure_batch import clash_links, valid_junctions
    parts = pdb_copies()
    B, N, A = parts["xyz"].shape[:3]
    host = StructureBatch(**parts, device="cpu")
    seq_idx = host.get_seq_idx()
    present = host.atom_mask != 0
    junctions = valid_junctions(present, host.chain_idx)
    radius = vdw_radius_table()[seq_idx]
    takes_part = (present & (radius > 0)).reshape(B, N * A)
    groups = torch.arange(N, dtype=torch.int32).repeat_interleave(A).expand(B, N * A)
    link = clash_links(junctions, A, seq_idx == ONE_TO_INDEX["C"])
    pro = torch.roll(seq_idx == ONE_TO_INDEX["P"], -1, dims=1)
    assert int(junctions.sum()) == B * (N - 2) and int(seq_idx.eq(ONE_TO_INDEX["X"]).sum()) == 0

    def restated(dtype):
        x = parts["xyz"].detach().clone().to(dtype).requires_grad_(True)   # a copy: .to() of the same dtype is the tensor itself
        E, _ = R.clash(x.reshape(B, N * A, 3), radius.reshape(B, N * A).to(dtype), takes_part, groups, link)
        viol = R.peptide_bond(x, junctions, pro)
        loss = viol.sum(dim=(1, 2)) / junctions.sum(-1).clamp(min=1) + E.sum(-1) / takes_part.sum(-1).clamp(min=1)
        (g,) = torch.autograd.grad(loss.sum(), x)
        return loss.detach(), g

    want_loss, want = restated(torch.float64)
    f32_loss, f32 = restated(torch.float32)
    clash_case = R.Case(parts["xyz"].reshape(B, N * A, 3), radius.reshape(B, N * A), takes_part, groups, link, None)
    open_ = R.brackets(clash_case)[2].reshape(B, N, A).any(-1) | R.bond_open(R.BondCase(parts["xyz"], junctions, pro, None))
    print(f"end to end: {int(open_.sum())} open residues of {B * N}")
    assert float(open_.sum()) <= 0.02 * B * N

    x = parts["xyz"].detach().cuda().requires_grad_()
    sb = StructureBatch(**{**parts, "xyz": x}, device="cuda")
    loss = sb.structural_violation_loss()
    assert loss.shape == (B,) and loss.grad_fn is not None
    loss.sum().backward()
    # the loss is two float32 reductions, two divisions and an addition past the kernels' outputs: the float32 restatement may
    # happen to land closer to float64 than eight roundings
    check_rows("end to end", "loss", loss.detach().cpu()[:, None], want_loss[:, None], f32_loss[:, None], floor=8 * 2.0 ** -24)
    check_rows("end to end", "grad_xyz", x.grad.cpu(), want, f32, open_)
    assert (x.grad.cpu()[~present] == 0).all() and float(x.grad.abs().max()) > 0
    per_residue = sb.steric_clashes()
    assert per_residue.shape == (B, N) and float(per_residue.sum()) > 0
    assert torch.allclose(per_residue.sum(-1) / takes_part.sum(-1).cuda(), sb.steric_clashes(per_residue=False))
    assert sb.peptide_bond_violations().shape == (B, N, 3)


def test_end_to_end_from_dihedrals(ops):
    """dihedrals -> from_backbone_dihedrals(include_cb=True) -> steric_clashes(backbone + CB) -> backward()."""
    from protstruc_amd import StructureBatch
    g = torch.Generator().manual_seed(5)
    dihedrals = (3.0 * torch.randn(2, 40, 3, generator=g)).cuda().requires_grad_()
    sb = StructureBatch.from_backbone_dihedrals(dihedrals, include_cb=True)
    energy = sb.steric_clashes(atoms=("N", "CA", "C", "O", "CB"))
    assert energy.shape == (2, 40) and energy.grad_fn is not None
    (energy.sum() + sb.structural_violation_loss().sum()).backward()
    assert dihedrals.grad.shape == (2, 40, 3) and torch.isfinite(dihedrals.grad).all()
    print(f"from dihedrals: clash energy {float(energy.sum()):.3f}, |grad| max {float(dihedrals.grad.abs().max()):.3e}")


def test_nothing_of_size_m_squared_is_allocated(ops):
    """B = 1, M = 4096: the rise of the allocator's peak across geometry.steric_clash and backward() stays below
    M * M * 4 bytes (64 MiB), the size of one float32 pair tensor."""
    from protstruc_amd import geometry
    M = 4096
    g = torch.Generator().manual_seed(9)
    x = R.random_walk(1, M, g).cuda().requires_grad_()
    radius = torch.full((1, M), 1.7, device="cuda")
    groups = (torch.arange(M, device="cuda", dtype=torch.int32) // 4).expand(1, M)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    energy = geometry.steric_clash(x, radius, groups=groups, reduction="structure")
    energy.sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes")
    assert rise < M * M * 4
    assert float(energy.detach()) > 0 and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
