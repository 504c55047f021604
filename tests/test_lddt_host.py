"""Host-side checks of lDDT: the yardstick itself (tests/lddt_ref.py), the C ABI's surface, the argument validation of
``ops.lddt`` / ``ops.lddt_backward`` and the signatures of the layers above.  No GPU needed."""
import ctypes
import inspect

import pytest
import torch

from tests import lddt_ref as R


def test_yardstick_on_a_hand_computed_example():
    """Four points on a line at 0, 10, 20, 34 (target) and 0, 10.7, 23, 34 (prediction), cutoff 15, thresholds 0.5 1 2 4.
    Target distances under 15: (0,1) = 10, (1,2) = 10, (2,3) = 14.  Predicted: 10.7, 12.3, 11 -> delta 0.7, 2.3, 3.
    Thresholds passed: 0.7 -> 3 of 4, 2.3 -> 1, 3 -> 1.  So S = (3/4, 3/4 + 1/4, 1/4 + 1/4, 1/4), n = (1, 2, 2, 1)."""
    t = torch.tensor([[[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0], [34.0, 0, 0]]], dtype=torch.float64)
    x = torch.tensor([[[0.0, 0, 0], [10.7, 0, 0], [23.0, 0, 0], [34.0, 0, 0]]], dtype=torch.float64)
    S, n = R.lddt(x, t)
    assert torch.equal(n, torch.tensor([[1.0, 2, 2, 1]], dtype=torch.float64))
    assert torch.allclose(S, torch.tensor([[0.75, 1.0, 0.5, 0.25]], dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.allclose(R.score(S, n), torch.tensor([[0.75, 0.5, 0.25, 0.25]], dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.allclose(R.score(S, n, "structure"), torch.tensor([2.5 / 6], dtype=torch.float64), rtol=0, atol=1e-12)
    # a mask drops a point and its pairs; groups drop the pairs inside a group
    S, n = R.lddt(x, t, point_mask=torch.tensor([[1, 0, 1, 1]]))
    assert torch.equal(n, torch.tensor([[0.0, 0, 1, 1]], dtype=torch.float64))
    assert torch.allclose(S, torch.tensor([[0.0, 0.0, 0.25, 0.25]], dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.equal(R.score(S, n)[0, :2], torch.zeros(2, dtype=torch.float64))     # no pair: 0, not 1 or NaN
    S, n = R.lddt(x, t, groups=torch.tensor([[0, 0, 1, 1]]))
    assert torch.equal(n, torch.tensor([[0.0, 1, 1, 0]], dtype=torch.float64))
    # smooth: the same pairs, sigmoid(thr - delta) in place of the step
    S, n = R.lddt(x, t, smooth=True)
    sig = lambda d: sum(1 / (1 + torch.exp(torch.tensor(d - thr, dtype=torch.float64))) for thr in R.THRESHOLDS) / 4  # noqa: E731
    want = torch.stack([sig(0.7), sig(0.7) + sig(2.3), sig(2.3) + sig(3.0), sig(3.0)])[None]
    assert torch.allclose(S, want, rtol=0, atol=1e-9) and torch.equal(n, torch.tensor([[1.0, 2, 2, 1]], dtype=torch.float64))


def test_yardstick_gradient_passes_gradcheck():
    case = R.random_case(2, 9, "p60", groups=2, noise=1.5, seed=7)
    x = torch.where(case.valid()[..., None], case.points, torch.zeros_like(case.points)).double().requires_grad_(True)
    w = case.grad_S.double()

    def f(p):
        S, _ = R.lddt(p, case.target.double(), smooth=True, **case.kwargs())
        return (S * w).sum()

    assert torch.autograd.gradcheck(f, (x,), eps=1e-6, atol=1e-7, rtol=1e-5)
    g = R.gradient(case)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0 and (g[~case.valid()] == 0).all()


def test_case_generator_and_brackets():
    case = R.random_case(3, 70, "structure", noise=0.3, seed=3)
    assert case.points.isnan().any() and case.target.isnan().any() and not case.valid()[-1].any()
    steps = (case.target[0, 1:] - case.target[0, :-1])[case.valid()[0, 1:] & case.valid()[0, :-1]].norm(dim=-1)
    assert torch.allclose(steps, torch.full_like(steps, 3.8), atol=1e-4)
    (s_lo, s_hi), (n_lo, n_hi), _ = R.brackets(case)
    S, n = R.forward(case, smooth=False)
    T = len(case.thresholds)
    assert (s_lo <= T * S + 1e-9).all() and (T * S <= s_hi + 1e-9).all() and (n_lo <= n).all() and (n <= n_hi).all()
    assert (S[-1] == 0).all() and (n[-1] == 0).all()
    for name, kw in R.accuracy_cases().items():
        assert kw["B"] == 3, name


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 and M = 0 launch nothing (no pointer is dereferenced
    but the host array of thresholds)."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    thr = (ctypes.c_float * 4)(0.5, 1.0, 2.0, 4.0)
    fwd, bwd = lib.ps_lddt_f32, lib.ps_lddt_backward_f32

    def forward(pts=fake, tgt=fake, cutoff=15.0, thresholds=thr, T=4, eps=1e-10, S=fake, n=fake, B=1, M=8):
        return fwd(pts, tgt, None, None, cutoff, thresholds, T, 0, eps, S, n, B, M, None)

    def backward(pts=fake, tgt=fake, cutoff=15.0, thresholds=thr, T=4, eps=1e-10, w=fake, out=fake, B=1, M=8):
        return bwd(pts, tgt, None, None, cutoff, thresholds, T, eps, w, out, B, M, None)

    for call in (forward, backward):
        assert call(B=0) == 0 and call(M=0) == 0
        assert call(pts=None) == 1 and call(tgt=None) == 1 and call(thresholds=None) == 1
        assert call(T=0) == 1 and call(T=9) == 1
        assert call(cutoff=0.0) == 1 and call(cutoff=-1.0) == 1 and call(cutoff=float("nan")) == 1 and call(cutoff=float("inf")) == 1
        assert call(eps=-1.0) == 1 and call(eps=float("nan")) == 1
        assert call(B=65536) == 1 and call(B=-1) == 1 and call(M=-1) == 1 and call(M=2 ** 30 + 1) == 1
        assert call(thresholds=(ctypes.c_float * 4)(0.5, 2.0, 1.0, 4.0)) == 1      # unsorted
        assert call(thresholds=(ctypes.c_float * 4)(0.5, 1.0, 1.0, 4.0)) == 1      # repeated
        assert call(thresholds=(ctypes.c_float * 4)(0.0, 1.0, 2.0, 4.0)) == 1      # not positive
        assert call(thresholds=(ctypes.c_float * 4)(0.5, 1.0, 2.0, 65.0)) == 1     # beyond PS_LDDT_MAX_THRESHOLD
        assert call(thresholds=(ctypes.c_float * 4)(0.5, 1.0, 2.0, float("nan"))) == 1
    assert forward(S=None) == 1 and forward(n=None) == 1
    assert backward(w=None) == 1 and backward(out=None) == 1


def lddt_args(B=2, M=9):
    g = torch.Generator().manual_seed(1)
    return [torch.randn(B, M, 3, generator=g), torch.randn(B, M, 3, generator=g)]


def test_lddt_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_lddt_shapes
    a = lddt_args()
    pm, gr = torch.ones(2, 9, dtype=torch.bool), torch.arange(9).expand(2, 9)
    check(*a)
    check(*a, pm, gr, 12.0, (1.0,), 0.0, torch.ones(2, 9))
    check(*a, thresholds=(0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0))
    for k in range(2):                                                   # each operand with a wrong shape, then a wrong dtype
        bad = list(a)
        bad[k] = a[k][:, :-1]
        with pytest.raises(ValueError):
            check(*bad)
        bad[k] = a[k].long()
        with pytest.raises(ValueError):
            check(*bad)
    with pytest.raises(ValueError):
        check(a[0][0], a[1][0])                                          # rank
    with pytest.raises(ValueError):
        check(a[0].reshape(2, 9, 3, 1), a[1].reshape(2, 9, 3, 1))
    with pytest.raises(ValueError):
        check(a[0][..., :2], a[1][..., :2])
    with pytest.raises(ValueError):
        check(*a, pm[:, :8])
    with pytest.raises(ValueError):
        check(*a, pm, gr[:1])
    with pytest.raises(ValueError):
        check(*a, pm, gr.float())                                        # groups are integers
    with pytest.raises(ValueError):
        check(*a, pm, pm)
    for thresholds in ((), tuple(0.5 * k for k in range(1, 10)), (1.0, 0.5), (0.5, 0.5), (0.0, 1.0), (-1.0,), (1.0, 65.0),
                       (float("nan"),)):
        with pytest.raises(ValueError):
            check(*a, thresholds=thresholds)
    for cutoff in (0.0, -3.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            check(*a, cutoff=cutoff)
    for eps in (-1e-9, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            check(*a, eps=eps)
    with pytest.raises(ValueError):
        check(*a, grad_S=torch.ones(2, 8))
    with pytest.raises(ValueError):
        check(*a, grad_S=torch.ones(2, 9, dtype=torch.long))
    with pytest.raises(ValueError):
        check(*a, pm.to("meta"))                                         # device disagreement


def test_ops_validate_first_then_refuse_cpu_tensors():
    from protstruc_amd import ops
    a = lddt_args()
    with pytest.raises(ValueError):
        ops.lddt(*a, cutoff=-1.0)
    with pytest.raises(ValueError):
        ops.lddt_backward(*a, torch.ones(2, 8))
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.lddt(*a)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.lddt_backward(*a, torch.ones(2, 9))


def test_signatures_of_the_layers_above():
    from protstruc_amd import StructureBatch, geometry, ops
    p = inspect.signature(geometry.lddt).parameters
    assert list(p) == ["points", "target_points", "point_mask", "groups", "cutoff", "thresholds", "smooth", "reduction", "eps"]
    assert (p["point_mask"].default, p["groups"].default, p["cutoff"].default, tuple(p["thresholds"].default),
            p["smooth"].default, p["reduction"].default, p["eps"].default) == (None, None, 15.0, (0.5, 1.0, 2.0, 4.0), False,
                                                                               "point", 1e-10)
    p = inspect.signature(StructureBatch.lddt).parameters
    assert list(p) == ["self", "target", "atoms", "cutoff", "per_residue", "smooth"]
    assert (tuple(p["atoms"].default), p["cutoff"].default, p["per_residue"].default, p["smooth"].default) == (("CA",), 15.0, True, False)
    p = inspect.signature(ops.lddt).parameters
    assert list(p) == ["points", "target_points", "point_mask", "groups", "cutoff", "thresholds", "smooth", "eps"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("cutoff", "thresholds", "smooth", "eps"))
    assert "grad_S" in inspect.signature(ops.lddt_backward).parameters
    with pytest.raises(ValueError):
        geometry.lddt(*lddt_args(), reduction="mean")


@pytest.mark.parametrize("smooth", [False, True])
def test_autograd_wrapper_differentiates_the_smooth_form_only(monkeypatch, smooth):
    """geometry.lddt: S carries a grad_fn iff ``smooth``, n never; the backward op receives dL/dS.  Host-only: both ops are
    replaced by CPU stand-ins (the restatement; a recorder)."""
    from protstruc_amd import geometry, ops
    x, t = lddt_args()
    seen = []

    def fake_forward(points, target, point_mask, groups, *, cutoff, thresholds, smooth, eps):
        return R.lddt(points.detach(), target, point_mask, groups, cutoff, thresholds, smooth, eps)

    def fake_backward(points, target, grad_S, point_mask, groups, *, cutoff, thresholds, eps):
        ops.check_lddt_shapes(points, target, point_mask, groups, cutoff, thresholds, eps, grad_S)
        seen.append(grad_S.clone())
        return torch.ones_like(points)

    monkeypatch.setattr(ops, "lddt", fake_forward)
    monkeypatch.setattr(ops, "lddt_backward", fake_backward)
    x = (4 * x).requires_grad_()
    target = (4 * t).requires_grad_()                                    # the target is used detached
    S, n = geometry.lddt(x, target, smooth=smooth, reduction="none")
    assert n.grad_fn is None and not n.requires_grad
    for reduction, shape in (("point", (2, 9)), ("structure", (2,))):
        out = geometry.lddt(x, target, smooth=smooth, reduction=reduction)
        assert out.shape == shape and (out.grad_fn is not None) == smooth
        assert torch.allclose(out, R.score(*R.lddt(x.detach(), target.detach(), smooth=smooth), reduction))
    if smooth:
        (3.0 * S).sum().backward()
        assert len(seen) == 1 and torch.equal(seen[0], torch.full((2, 9), 3.0))
        assert torch.equal(x.grad, torch.ones_like(x)) and target.grad is None
    else:
        assert S.grad_fn is None and not S.requires_grad
