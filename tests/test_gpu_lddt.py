"""GPU tests of lDDT (ps_lddt_f32, ps_lddt_backward_f32; ops.lddt, ops.lddt_backward; geometry.lddt; StructureBatch.lddt).

Yardstick: the float64 evaluation of the torch restatement in tests/lddt_ref.py.

The HARD forward is bracketed, not toleranced: equality with float64 is undecidable at a step.  tests/lddt_ref.brackets
counts, in float64, every term within 1e-4 of the cutoff or of a threshold out (lo) and in (hi); the kernel must lie in
[lo, hi] at every point -- exact equality wherever lo == hi -- and at most OPEN_CAP of a case's unmasked points may have
lo != hi, so the brackets cannot hide a kernel error (the float64 reference gives 0-2.1 % on these cases).

The SMOOTH forward and the gradient use the error measure and the margin of tests/test_gpu_fape.py: with e(row) = the
row's largest error divided by the row's largest float64 |value| and E = the worst row, E_kernel <= 4 max(E_f32, 2^-24)
for S (rows are points) and E_kernel <= 4 E_f32 for the gradient (rows are points, or residues end to end), where E_f32
is the SAME restatement run in float32 on the CPU; a row whose float64 value is identically zero must be exactly zero.
Points whose float32 result is not a rounding of the float64 one are left out of E, for the kernel and for the float32
restatement alike, and count against the same cap: a point with a target pair within 1e-4 of the cutoff (the pair is in
or out as a whole), and, for the gradient, a point with a counted pair whose |d - d'| is below 1e-4 (the gradient of
|d - d'| jumps from -e'(0) to +e'(0) there; 0-1.5 % of the points).  n is exact wherever its bracket is closed and inside
the bracket elsewhere.
"""
import functools
import os

import pytest
import torch

from tests import lddt_ref as R
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

MARGIN = 4.0
OPEN_CAP = 0.10
CASES = R.accuracy_cases()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case and its CPU references, computed once and shared (never modified) by the tests that need them."""
    case = R.random_case(**CASES[name])
    hard_open, smooth_open, grad_open = R.open_points(case)
    (s_lo, s_hi), (n_lo, n_hi), _ = R.brackets(case)
    return {"case": case, "s_lo": s_lo, "s_hi": s_hi, "n_lo": n_lo, "n_hi": n_hi,
            "hard_open": hard_open, "smooth_open": smooth_open, "grad_open": grad_open,
            "S64": R.forward(case, True)[0], "S32": R.forward(case, True, torch.float32)[0],
            "grad64": R.gradient(case), "grad32": R.gradient(case, torch.float32)}


def cuda(t):
    return None if t is None else t.cuda()


def gpu_args(case):
    return [case.points.cuda(), case.target.cuda()], dict(point_mask=cuda(case.point_mask), groups=cuda(case.groups),
                                                          cutoff=case.cutoff, thresholds=case.thresholds, eps=case.eps)


def check_cap(name, what, open_, case):
    valid = case.valid()
    frac = float((open_ & valid).sum()) / max(int(valid.sum()), 1)
    print(f"{name} {what}: {100 * frac:.2f} % of the unmasked points are open")
    assert frac <= OPEN_CAP, f"{name} {what}: {frac:.3f} of the points are undecidable in float32"


def check_count(name, n, ref):
    n = n.cpu().double()
    assert ((ref["n_lo"] <= n) & (n <= ref["n_hi"])).all(), f"{name}: n outside its bracket"   # equality where lo == hi
    assert (n[~ref["case"].valid()] == 0).all()


def closed(t, open_):
    """t with the open points' rows zeroed (a zero row against a zero row has e = 0)."""
    keep = ~open_
    return torch.where(keep.reshape(keep.shape + (1,) * (t.dim() - keep.dim())), t.detach().cpu().double(), 0.0)


def check_rows(name, what, got, want, f32, open_, floor=0.0):
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.isfinite(got).all(), (name, what)
    e_kernel, e_f32 = R.worst_error(closed(got, open_), closed(want, open_)), R.worst_error(closed(f32, open_), closed(want, open_))
    print(f"{name} {what}: E_kernel = {e_kernel:.3e}  E_f32 = {e_f32:.3e}  ratio = {e_kernel / e_f32 if e_f32 else float('nan'):.2f}")
    assert e_kernel <= MARGIN * max(e_f32, floor), f"{name} {what}: E_kernel {e_kernel:.3e} > {MARGIN} x E_f32 {e_f32:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_hard_forward_lies_in_the_float64_bracket(ops, name):
    ref = reference(name)
    case = ref["case"]
    args, kw = gpu_args(case)
    S, n = ops.lddt(*args, **kw)
    assert S.shape == (case.B, case.M) and S.dtype == torch.float32 and n.shape == S.shape and n.dtype == torch.float32
    check_cap(name, "hard", ref["hard_open"], case)
    check_count(name, n, ref)
    T = torch.tensor(float(len(case.thresholds)), dtype=torch.float32)
    lo, hi = (ref["s_lo"].float() / T), (ref["s_hi"].float() / T)      # the float32 quotient of two small integers, as the kernel's
    S = S.cpu()
    assert ((lo <= S) & (S <= hi)).all(), f"{name}: S outside its bracket at {int(((S < lo) | (S > hi)).sum())} points"
    assert (S[~case.valid()] == 0).all()
    assert (S[n.cpu() == 0] == 0).all()                                 # no pair: 0, not 1 or NaN


@pytest.mark.parametrize("name", list(CASES))
def test_smooth_forward_accuracy(ops, name):
    ref = reference(name)
    case = ref["case"]
    args, kw = gpu_args(case)
    S, n = ops.lddt(*args, smooth=True, **kw)
    check_cap(name, "smooth", ref["smooth_open"], case)
    check_count(name, n, ref)
    check_rows(name, "S", S.cpu(), ref["S64"], ref["S32"], ref["smooth_open"], floor=2.0 ** -24)
    assert (S.cpu()[~case.valid()] == 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_backward_accuracy(ops, name):
    ref = reference(name)
    case = ref["case"]
    args, kw = gpu_args(case)
    w = case.grad_S.cuda()
    got = ops.lddt_backward(*args, w, **kw)
    check_cap(name, "gradient", ref["grad_open"], case)
    check_rows(name, "grad_points", got.cpu(), ref["grad64"], ref["grad32"], ref["grad_open"])
    assert (got.cpu()[~case.valid()] == 0).all()
    if case.point_mask is not None:                                      # NaN upstream at a masked point never arrives either
        dirty = torch.where(case.point_mask, case.grad_S, torch.full_like(case.grad_S, float("nan")))
        assert torch.equal(ops.lddt_backward(*args, dirty.cuda(), **kw), got)


def test_prediction_equal_to_target(ops):
    case = reference("M=600 p60")["case"]
    t = case.target.cuda()
    kw = gpu_args(case)[1]
    S, n = ops.lddt(t, t, **kw)
    assert torch.equal(S, n) and float(n.max()) > 10
    grad = ops.lddt_backward(t, t, case.grad_S.cuda(), **kw)
    assert (grad == 0).all()
    from protstruc_amd import geometry
    assert (geometry.lddt(t, t, kw["point_mask"])[kw["point_mask"] & (n > 0)] == 1).all()
    assert (geometry.lddt(t, t, kw["point_mask"], reduction="structure") == 1).all()


def test_deterministic(ops):
    case = reference("M=600 p60")["case"]
    args, kw = gpu_args(case)
    w = case.grad_S.cuda()
    for smooth in (False, True):
        assert all(torch.equal(a, b) for a, b in zip(ops.lddt(*args, smooth=smooth, **kw), ops.lddt(*args, smooth=smooth, **kw)))
    assert torch.equal(ops.lddt_backward(*args, w, **kw), ops.lddt_backward(*args, w, **kw))


def test_rigid_motion_of_the_prediction(ops):
    name = "M=257"
    ref = reference(name)
    case = ref["case"]
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4)))
    moved = (case.points.double() @ q.T + torch.tensor([3.0, -7.0, 11.0], dtype=torch.float64)).float()
    args, kw = gpu_args(case)
    S0, n0 = ops.lddt(*args, smooth=True, **kw)
    S, n = ops.lddt(moved.cuda(), args[1], smooth=True, **kw)
    assert torch.equal(n, n0)
    S32 = R.forward(case, True, torch.float32, points=moved)[0]
    check_rows(name, "S of the moved prediction", S.cpu(), ref["S64"], S32, ref["smooth_open"], floor=2.0 ** -24)


def test_empty_inputs_launch_nothing(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for B, M in ((0, 5), (2, 0)):
        S, n = ops.lddt(z(B, M, 3), z(B, M, 3))
        assert S.shape == (B, M) and n.shape == (B, M)
        assert ops.lddt_backward(z(B, M, 3), z(B, M, 3), z(B, M)).shape == (B, M, 3)


def residue_case():
    """A batch of 3 x 40 residues x 5 atom slots from the 600-point walk's generator: atoms present with p = 0.85, NaN at
    the missing ones."""
    B, N, A = 3, 40, 5
    case = R.random_case(B, N * A, "none", groups=A, noise=0.3, seed=211)
    g = torch.Generator().manual_seed(212)
    atom_mask = torch.rand(B, N, A, generator=g) < 0.85
    nan = float("nan")
    xyz = torch.where(atom_mask[..., None], case.points.reshape(B, N, A, 3), nan)
    target = torch.where(atom_mask[..., None], case.target.reshape(B, N, A, 3), nan)
    return R.Case(xyz.reshape(B, N * A, 3), target.reshape(B, N * A, 3), atom_mask.reshape(B, N * A), case.groups,
                  case.thresholds, case.grad_S), atom_mask, (B, N, A)


def test_end_to_end_gradient_reaches_the_coordinates(ops):
    """xyz.requires_grad_() -> StructureBatch.lddt(target, atoms="all", smooth=True, per_residue=True).sum().backward()
    against the float64 gradient of the restatement; rows are residues."""
    from protstruc_amd import StructureBatch
    case, atom_mask, (B, N, A) = residue_case()

    def restated(dtype):
        x = case.points.detach().to(dtype).requires_grad_(True)
        S, n = R.lddt(x, case.target.to(dtype), smooth=True, **case.kwargs())
        per_residue = S.reshape(B, N, A).sum(-1) / n.reshape(B, N, A).sum(-1).clamp(min=1)
        (g,) = torch.autograd.grad(per_residue.sum(), x)
        return per_residue.detach(), g.reshape(B, N, A, 3)

    want_score, want = restated(torch.float64)
    f32_score, f32 = restated(torch.float32)
    _, at_cutoff, grad_open = R.open_points(case)
    open_residues = grad_open.reshape(B, N, A).any(-1)
    frac = float(open_residues.sum()) / (B * N)
    print(f"end to end: {100 * frac:.2f} % of the residues are open")
    assert frac <= OPEN_CAP

    x = case.points.reshape(B, N, A, 3).cuda().requires_grad_()
    sb = StructureBatch.from_xyz(x, atom_mask, device="cuda")
    tb = StructureBatch.from_xyz(case.target.reshape(B, N, A, 3), atom_mask, device="cuda")
    out = sb.lddt(tb, atoms="all", smooth=True, per_residue=True)
    assert out.shape == (B, N) and out.grad_fn is not None
    out.sum().backward()
    check_rows("end to end", "score per residue", out.detach().cpu(), want_score, f32_score, at_cutoff.reshape(B, N, A).any(-1),
               floor=2.0 ** -24)
    check_rows("end to end", "grad_xyz", x.grad.cpu(), want, f32, open_residues)
    assert (x.grad.cpu()[~atom_mask] == 0).all()

    hard = sb.lddt(tb, atoms="all", smooth=False)
    assert hard.grad_fn is None and not hard.requires_grad and hard.shape == (B, N)
    whole = sb.lddt(tb, atoms="all", per_residue=False)
    assert whole.shape == (B,) and whole.grad_fn is None and ((whole > 0.3) & (whole <= 1)).all()


def test_structure_batch(ops):
    """15c8_HL.pdb (NaN coordinates of missing atoms) against a perturbed copy: the method equals the geometry call on the
    hand-built views, for CA alone, for three atoms and for every slot; against itself every residue with a partner
    scores exactly 1; a single-structure target serves a batch."""
    from protstruc_amd import StructureBatch, geometry
    from protstruc_amd.general import ATOM
    sb = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "15c8_HL.pdb"))
    B, N, A = sb.xyz.shape[:3]
    assert sb.xyz.isnan().any()
    g = torch.Generator().manual_seed(15)
    moved = sb.xyz + 0.7 * torch.randn(B, N, A, 3, generator=g).cuda()
    other = StructureBatch.from_xyz(moved, sb.atom_mask, device="cuda")
    am = (sb.atom_mask != 0) & sb.residue_mask[:, :, None]
    ca = int(ATOM["CA"])
    got = other.lddt(sb)
    S, n = geometry.lddt(moved[:, :, ca], sb.xyz[:, :, ca], am[:, :, ca], reduction="none")
    assert got.shape == (B, N) and torch.isfinite(got).all() and torch.equal(got, S / n.clamp(min=1))
    assert 0.2 < float(got[am[:, :, ca]].mean()) < 0.95
    assert torch.equal(other.lddt(sb, per_residue=False), S.sum(-1) / n.sum(-1).clamp(min=1))
    groups = torch.arange(N, device="cuda", dtype=torch.int32).repeat_interleave(A).expand(B, N * A)
    backbone = torch.zeros(A, dtype=torch.bool, device="cuda")
    backbone[[int(ATOM[a]) for a in ("N", "CA", "C")]] = True
    for atoms, pm in (("all", am), (("N", "CA", "C"), am & backbone)):
        got = other.lddt(sb, atoms=atoms)
        S, n = geometry.lddt(moved.reshape(B, -1, 3), sb.xyz.reshape(B, -1, 3), pm.reshape(B, -1), groups, reduction="none")
        S, n = S.reshape(B, N, A).sum(-1), n.reshape(B, N, A).sum(-1)
        assert torch.isfinite(got).all() and torch.equal(got, S / n.clamp(min=1))
        itself = sb.lddt(sb, atoms=atoms)
        assert torch.equal(itself, (n > 0).float())
    x = torch.cat([moved, sb.xyz]).requires_grad_()
    both = StructureBatch.from_xyz(x, torch.cat([sb.atom_mask, sb.atom_mask]), device="cuda")
    score = both.lddt(sb, smooth=True, per_residue=False)
    assert score.shape == (2,) and score[0] == other.lddt(sb, smooth=True, per_residue=False)[0] and score[1] > score[0]
    (1 - score).sum().backward()
    assert torch.isfinite(x.grad).all() and (x.grad[~torch.cat([am, am])] == 0).all() and float(x.grad[0].abs().max()) > 0
    assert (x.grad[:, :, [s for s in range(A) if s != ca]] == 0).all() and (x.grad[1] == 0).all()


def test_nothing_of_size_m_squared_is_allocated(ops):
    """B = 1, M = 4096: the rise of the allocator's peak across geometry.lddt(..., smooth=True) and backward() stays
    below M * M bytes (16 MiB), less than the smallest pair tensor a composed version could build."""
    from protstruc_amd import geometry
    M = 4096
    g = torch.Generator().manual_seed(9)
    target = R.random_walk(1, M, g).cuda()
    x = (target + 0.3 * torch.randn(1, M, 3, generator=g).cuda()).requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    score = geometry.lddt(x, target, smooth=True, reduction="structure")
    (1 - score).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes")
    assert rise < M * M
    assert 0.5 < float(score.detach()) < 1 and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
