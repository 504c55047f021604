"""Host-side checks of the frame-aligned point error: the yardstick itself (tests/fape_ref.py), the C ABI's surface and the
argument validation of ``ops.fape`` / ``ops.fape_backward`` / ``ops.frames_backward``.  No GPU needed."""
import ctypes

import pytest
import torch

from oracle import protstruc_oracle as O
from tests import fape_ref as R
from tests.conftest import load_golden


@pytest.mark.parametrize("regime", ["clamped", "unclamped", "frames_from_xyz"])
def test_float64_gradient_agrees_with_central_differences(regime):
    """<gradient, v> against (L(x + h v) - L(x - h v)) / (2 h) in float64 along 8 random directions, with the step and the
    tolerance argued in tests/test_irg_backward_host.py: h = 1e-5 puts truncation (h^2 |L'''| / 6) and rounding
    (1.1e-16 |L| / h) both near 1e-10 |L'| for terms of order one, four orders below the 1e-6 asserted relative to
    sum |gradient_k v_k| (the directional derivative itself is a sum of random signs and no scale for its own error).
    The clamp is no obstacle: it sits in a gap of the distances at least 4e-4 wide (tests/fape_ref.pick_clamp), forty
    times what a step of 1e-5 along a unit-scale direction moves a distance, so no pair crosses it."""
    case = R.random_case(17, 2, 24, 4, "both")
    clamp = float("inf") if regime == "unclamped" else None
    h = 1e-5
    gen = torch.Generator().manual_seed(5)
    g64 = case.grad_loss.double()
    if regime == "frames_from_xyz":
        grads = [R.gradient_xyz(case)]
        x0 = [case.xyz.double()]

        def value(xs):
            moved = R.Case(xs[0], case.target_xyz, case.frame_mask, case.point_mask, case.atom_mask, case.clamp, case.grad_loss)
            x = moved.xyz
            bb = x[:, :, list(R.SLOTS[:3])]
            rot, trans = R.frames_from_xyz(bb, 0, 1, 2, 1)
            t = case.target_xyz.double()
            trot, ttrans = R.frames_from_xyz(t, *R.SLOTS)
            l, _ = R.fape(rot, trans, x.reshape(case.B, -1, 3), trot, ttrans, t.reshape(case.B, -1, 3), **case.kwargs(torch.float64))
            return float((l * g64).sum())
    else:
        grads = list(R.gradient(case, clamp=clamp))
        ops = case.operands(torch.float64)
        x0 = ops[:3]

        def value(xs):
            kw = case.kwargs(torch.float64)
            if clamp is not None:
                kw["clamp"] = clamp
            l, _ = R.fape(*xs, *ops[3:], **kw)
            return float((l * g64).sum())

    assert all(torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    for _ in range(8):
        vs = [torch.randn(x.shape, generator=gen, dtype=torch.float64) for x in x0]
        fd = (value([x + h * v for x, v in zip(x0, vs)]) - value([x - h * v for x, v in zip(x0, vs)])) / (2 * h)
        an = sum(float((g * v).sum()) for g, v in zip(grads, vs))
        scale = sum(float((g * v).abs().sum()) for g, v in zip(grads, vs))
        print(f"{regime}: analytic {an:.12e} finite difference {fd:.12e} relative {abs(an - fd) / scale:.2e}")
        assert abs(an - fd) <= 1e-6 * scale


def test_clamp_passes_gradient_only_below_it_and_masked_entries_get_zeros():
    case = R.random_case(19, 2, 12, 4, "both")
    g_rot, g_trans, g_pts = R.gradient(case)
    assert (g_rot[~case.frame_mask] == 0).all() and (g_trans[~case.frame_mask] == 0).all()
    assert (g_pts[~case.point_mask] == 0).all()
    assert (g_rot[-1] == 0).all() and (g_pts[-1] == 0).all()       # the structure with every frame masked
    l, count = R.loss(case)
    assert float(l[-1]) == 0 and float(count[-1]) == 0
    tiny = [g.abs().max() for g in R.gradient(case, clamp=1e-3)]   # below every distance (sqrt(eps) = 1e-2): no pair passes
    assert all(float(t) == 0 for t in tiny)


def test_restated_frames_equal_the_oracle():
    g = load_golden("g5_frames")
    xyz = g["xyz"]
    for slots in ((0, 1, 2), (2, 1, 0), (4, 1, 3)):
        rot, trans = R.frames_from_xyz(xyz, *slots, 1)
        want = O.backbone_orientations(xyz, *slots)
        assert float((rot - want).abs().max()) <= 1e-5
        assert torch.equal(trans, xyz[:, :, 1])


def test_case_generator_covers_both_sides_of_the_clamp():
    case = R.random_case(23, 2, 33, 4, "none")
    d, _ = R.distances(*case.operands(torch.float64))
    assert float(d.min()) < 2.0 and float(d.max()) > 40.0
    below = (d < case.clamp.double()[:, None, None]).double().mean()
    assert 0.3 < float(below) < 0.6
    assert ((case.clamp > 8) & (case.clamp < 12)).all()


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 launches nothing (the pointers are never dereferenced)."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    six = [fake] * 6
    fwd, bwd, frames = lib.ps_fape_f32, lib.ps_fape_backward_f32, lib.ps_frames_backward_f32
    assert fwd(*six, None, None, fake, 10.0, 1e-4, fake, fake, fake, 0, 4, 12, None) == 0
    assert fwd(None, *six[1:], None, None, fake, 10.0, 1e-4, fake, fake, fake, 1, 4, 12, None) == 1
    assert fwd(*six, None, None, None, 10.0, 1e-4, fake, fake, fake, 1, 4, 12, None) == 1      # no clamp
    assert fwd(*six, None, None, fake, 0.0, 1e-4, fake, fake, fake, 1, 4, 12, None) == 1       # scale
    assert fwd(*six, None, None, fake, 10.0, -1.0, fake, fake, fake, 1, 4, 12, None) == 1      # eps
    assert fwd(*six, None, None, fake, 10.0, 1e-4, fake, fake, None, 1, 4, 12, None) == 1      # no scratch
    assert fwd(*six, None, None, fake, 10.0, 1e-4, fake, fake, fake, 65536, 4, 12, None) == 1
    assert bwd(*six, None, None, fake, 10.0, 1e-4, fake, fake, fake, fake, 0, 4, 12, None) == 0
    assert bwd(*six, None, None, fake, 10.0, 1e-4, fake, None, None, None, 1, 4, 12, None) == 1   # no output at all
    assert bwd(*six, None, None, fake, 10.0, 1e-4, None, fake, fake, fake, 1, 4, 12, None) == 1   # no upstream
    assert bwd(*six, None, None, fake, float("nan"), 1e-4, fake, fake, fake, fake, 1, 4, 12, None) == 1
    assert frames(fake, fake, fake, None, fake, 0, 4, 15, 0, 1, 2, 1, None) == 0
    assert frames(fake, None, None, None, fake, 1, 4, 15, 0, 1, 2, 1, None) == 1               # no upstream
    assert frames(fake, fake, fake, None, None, 1, 4, 15, 0, 1, 2, 1, None) == 1               # no output
    assert frames(fake, fake, None, None, fake, 1, 4, 15, 0, 1, 15, 1, None) == 1              # slot outside A
    assert frames(fake, None, fake, None, fake, 1, 4, 15, 0, 1, 2, -1, None) == 1


def fape_args(B=2, N=6, M=9):
    g = torch.Generator().manual_seed(1)
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return [mk(B, N, 3, 3), mk(B, N, 3), mk(B, M, 3), mk(B, N, 3, 3), mk(B, N, 3), mk(B, M, 3)]


def test_fape_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_fape_shapes
    a = fape_args()
    fm, pm = torch.ones(2, 6, dtype=torch.bool), torch.ones(2, 9)
    check(*a)
    check(*a, fm, pm, torch.tensor([10.0, float("inf")]), 10.0, 0.0, torch.ones(2))
    check(*a, clamp=float("inf"))
    for k in range(6):                                                   # each operand with a wrong shape, then a wrong dtype
        bad = list(a)
        bad[k] = a[k][:, :-1]
        with pytest.raises(ValueError):
            check(*bad)
        bad[k] = a[k].long()
        with pytest.raises(ValueError):
            check(*bad)
    with pytest.raises(ValueError):
        check(a[0][0], *a[1:])                                           # rank
    with pytest.raises(ValueError):
        check(a[0].reshape(2, 6, 9), *a[1:])
    with pytest.raises(ValueError):
        check(*a, fm[:, :5])
    with pytest.raises(ValueError):
        check(*a, fm, pm[:1])
    with pytest.raises(ValueError):
        check(*a, fm, fm)                                                # a point mask with the frames' shape
    for clamp in (0.0, -1.0, float("nan"), torch.tensor([10.0, 0.0]), torch.tensor([10.0]), torch.tensor([10, 10])):
        with pytest.raises(ValueError):
            check(*a, clamp=clamp)
    for scale in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            check(*a, scale=scale)
    for eps in (-1e-9, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            check(*a, eps=eps)
    with pytest.raises(ValueError):
        check(*a, grad_loss=torch.ones(3))
    with pytest.raises(ValueError):
        check(*a, grad_loss=torch.ones(2, dtype=torch.long))
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            check(*a, fm.cuda())                                         # device disagreement


def test_frames_backward_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_frames_backward_shapes
    xyz, g_rot, g_trans = torch.randn(2, 6, 5, 3), torch.randn(2, 6, 3, 3), torch.randn(2, 6, 3)
    check(xyz, 0, 1, 2, 1, g_rot, g_trans, torch.ones(2, 6, dtype=torch.bool), torch.empty(2, 6, 5, 3))
    check(xyz, 0, 1, 2, 1, g_rot)
    check(xyz, 0, 1, 2, 4, None, g_trans)
    check(xyz, 9, 9, 9, 1, None, g_trans)                                # slots that are not read are not checked
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 2, 1)                                           # no upstream gradient at all
    with pytest.raises(ValueError):
        check(xyz[0], 0, 1, 2, 1, g_rot)
    with pytest.raises(ValueError):
        check(xyz.long(), 0, 1, 2, 1, g_rot)
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 2, 1, g_rot[:, :5])
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 2, 1, g_rot.reshape(2, 6, 9))
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 2, 1, None, g_trans[:1])
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 5, 1, g_rot)                                    # slot outside [0, A)
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 2, -1, None, g_trans)
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 2, 1, g_rot, residue_mask=torch.ones(2, 5))
    with pytest.raises(ValueError):
        check(xyz, 0, 1, 2, 1, g_rot, out=torch.empty(2, 6, 5, 3, dtype=torch.float64))


def test_ops_validate_first_then_refuse_cpu_tensors():
    from protstruc_amd import ops
    a = fape_args()
    with pytest.raises(ValueError):
        ops.fape(*a, clamp=-1.0)
    with pytest.raises(ValueError):
        ops.fape_backward(*a, torch.ones(3))
    with pytest.raises(ValueError):
        ops.frames_backward(torch.randn(1, 4, 5, 3), 0, 1, 2, 1)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.fape(*a)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.fape_backward(*a, torch.ones(2))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.frames_backward(torch.randn(1, 4, 5, 3), 0, 1, 2, 1, grad_rot=torch.randn(1, 4, 3, 3))


@pytest.mark.parametrize("needs", [(True, True, True), (False, False, True), (True, False, False), (False, True, True)])
def test_autograd_wrapper_asks_only_for_the_gradients_autograd_needs(monkeypatch, needs):
    """geometry.frame_aligned_point_error hands ``ctx.needs_input_grad`` to the backward op as want_rot / want_trans /
    want_points.  Host-only: both ops are replaced by CPU stand-ins (the restatement; a recorder)."""
    from protstruc_amd import geometry, ops
    a = fape_args()
    seen = []

    def fake_forward(*args, clamp, scale, eps):
        return R.fape(*[t.detach() if isinstance(t, torch.Tensor) else t for t in args], clamp=clamp, scale=scale, eps=eps)

    def fake_backward(*args, clamp, scale, eps, want_rot, want_trans, want_points):
        ops.check_fape_shapes(*args[:6], args[7], args[8], clamp, scale, eps, args[6])
        seen.append((want_rot, want_trans, want_points))
        rot, trans, pts = args[:3]
        return (torch.ones_like(rot) if want_rot else None, torch.ones_like(trans) if want_trans else None,
                torch.ones_like(pts) if want_points else None)

    monkeypatch.setattr(ops, "fape", fake_forward)
    monkeypatch.setattr(ops, "fape_backward", fake_backward)
    leaves = [t.clone().requires_grad_(n) for t, n in zip(a[:3], needs)]
    target = [t.clone().requires_grad_(True) for t in a[3:]]           # the target side is used detached
    loss = geometry.frame_aligned_point_error(*leaves, *target, clamp=torch.tensor([9.0, float("inf")]))
    assert loss.shape == (2,) and loss.requires_grad
    loss.sum().backward()
    assert seen == [needs]
    for t, n in zip(leaves, needs):
        assert (t.grad is not None) == n
    assert all(t.grad is None for t in target)
