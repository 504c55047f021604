"""Host-side checks of the backbone builder's backward pass: the yardstick itself (tests/nerf_grad_ref.py), the closed form
the kernel evaluates, the C ABI's surface and the argument validation of ``ops.backbone_from_dihedrals_backward``.  No GPU
needed."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nerf_grad_ref as R
from tests import nerf_ref

SYMBOL = "ps_backbone_from_dihedrals_backward_f32"
# every option of the GPU test's accuracy cases, at the two lengths where the float64 walk costs a second
HOST_CASES = [c for c in R.accuracy_cases() if c["N"] in (5, 64, 229)]


def _np(t):
    return None if t is None else t.numpy()


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c["name"])
def test_restatement_equals_the_numpy_walk(case):
    """The torch restatement places every atom where nerf_ref.build does (both float64, another order of operations)."""
    c = R.make_case(case)
    got = R.coordinates(c["dihedrals"], c["chain_idx"], c["residue_mask"], c["bond_angles"], c["bond_lengths"],
                        c["include_cb"], c["n_slots"])
    want, _ = nerf_ref.build(_np(c["dihedrals"]), _np(c["chain_idx"]), _np(c["residue_mask"]), _np(c["bond_angles"]),
                             _np(c["bond_lengths"]), c["include_cb"], c["n_slots"])
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - torch.from_numpy(want)).abs().max()) <= 1e-9


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c["name"])
def test_torque_form_equals_autograd_in_float64(case):
    """The force / torque projections of include/protstruc_hip.h, evaluated in float64 from the coordinates alone, are the
    autograd gradient of the sequential walk: all nine parameter kinds, signs included, to 1e-10 of each kind's largest
    entry per structure; the entries the builder never reads are exact zeros in both."""
    c = R.make_case(case)
    want = R.case_gradients(c, torch.float64)
    xyz = R.coordinates(c["dihedrals"], c["chain_idx"], c["residue_mask"], c["bond_angles"], c["bond_lengths"],
                        c["include_cb"], c["n_slots"])
    got = R.torque_gradient(xyz, c["grad_xyz"], c["chain_idx"], c["residue_mask"], c["include_cb"])
    E = R.worst_error(got, want)
    print(f"{case['name']}: E(torque form, float64) = {E:.2e}")
    assert E <= 1e-10
    B, N = case["B"], case["N"]
    unused = torch.from_numpy(~nerf_ref.used_angles(B, N, _np(c["chain_idx"]), _np(c["residue_mask"])))
    assert unused.any()
    assert (want[0][unused] == 0).all() and (got[0][unused] == 0).all()
    assert (want[0][~unused] != 0).all(), "a used angle with an identically zero gradient: the case is degenerate"
    if c["residue_mask"] is not None:
        dead = ~c["residue_mask"]
        for k in range(3):
            assert (got[k][dead][:, 0] == 0).all() and (want[k][dead][:, 0] == 0).all()   # the residue's own parameters


def test_float32_figures_of_the_yardstick():
    """E_f32 (float32 autograd of the walk) and the float32 torque form on float32-rounded exact coordinates, printed: the
    figures the GPU test measures the kernel against.  The bounds are sanity checks of the yardstick (a wrong sign or a
    missing term gives order one), not rounding budgets."""
    case = next(c for c in R.accuracy_cases() if c["name"] == "strand N=229 perturbed")
    c = R.make_case(case)
    want = R.case_gradients(c, torch.float64)
    f32 = R.case_gradients(c, torch.float32)
    xyz = R.coordinates(c["dihedrals"], None, None, c["bond_angles"], c["bond_lengths"], False, 15).float()
    tq = R.torque_gradient(xyz, c["grad_xyz"], dtype=torch.float32)
    e_f32, e_tq = R.worst_error(f32, want), R.worst_error(tq, want)
    print(f"{case['name']}: E_f32 = {e_f32:.2e}  E(torque form, float32) = {e_tq:.2e}")
    assert e_f32 < 1e-1 and e_tq < 1e-2


def test_error_measure_demands_exact_zeros():
    want = torch.zeros(2, 4, 3, dtype=torch.float64)
    want[1, 2, 0] = 2.0
    got = want.clone().float()
    assert R.worst_error((got,), (want,)) == 0.0
    got[1, 0, 1] = 1e-3
    assert R.worst_error((got,), (want,)) == pytest.approx(5e-4)
    got[0, 0, 0] = 1e-30
    assert R.worst_error((got,), (want,)) == float("inf")
    got[0, 0, 0] = float("nan")
    assert R.worst_error((got,), (want,)) == float("inf")


def test_accuracy_cases_cover_what_they_must():
    cases = R.accuracy_cases()
    plain = {(c["family"], c["N"]) for c in cases if c["name"].endswith("plain")}
    assert plain == {(f, n) for f in R.FAMILIES for n in R.LENGTHS}
    assert R.LENGTHS == (5, 64, 229, 512, 1024, 1025, 2048)
    for N in (64, 229):
        here = [c for c in cases if c["N"] == N]
        assert any(c["include_cb"] for c in here) and any(c["perturbed"] for c in here)
        assert any(c["chains"] for c in here) and any(c["A"] == 7 for c in here)
    for N in (1025, 2048):
        assert any(c["chains"] and c["N"] == N for c in cases)
    assert all(c["B"] >= 2 for c in cases)
    chain, mask = R.chains_and_masks(3, 64)
    assert [len(set(row)) for row in chain] == [2, 3, 2]
    for b in range(3):
        gone = np.flatnonzero(~mask[b])
        assert gone[0] == 0 and len(gone) == 4
        end = np.flatnonzero(np.diff(chain[b]))[0]
        assert end in gone                                  # the last residue of the first chain
        assert gone[3] == gone[2] + 1                       # two adjacent


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 or N = 0 launches nothing (the pointers are never
    dereferenced)."""
    from protstruc_amd import _lib
    fn = getattr(_lib.load(), SYMBOL)
    fake = ctypes.c_void_p(0x1000)
    assert fn(None, fake, None, None, fake, None, None, 0, 1, 4, 15, None) == 1      # no coordinates
    assert fn(fake, None, None, None, fake, None, None, 0, 1, 4, 15, None) == 1      # no upstream gradient
    assert fn(fake, fake, None, None, None, fake, fake, 0, 1, 4, 15, None) == 1      # no grad_dihedrals
    assert fn(fake, fake, None, None, fake, None, None, 0, 1, 4, 2, None) == 1       # A < 3
    assert fn(fake, fake, None, None, fake, None, None, 1, 1, 4, 4, None) == 1       # CB needs A >= 5
    assert fn(fake, fake, None, None, fake, None, None, 0, -1, 4, 15, None) == 1
    assert fn(fake, fake, None, None, fake, None, None, 0, 1, -4, 15, None) == 1
    assert fn(fake, fake, None, None, fake, None, None, 1, 0, 4, 15, None) == 0
    assert fn(fake, fake, None, None, fake, fake, fake, 1, 3, 0, 15, None) == 0


def test_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_backbone_from_dihedrals_backward_shapes
    xyz, g = torch.zeros(2, 6, 15, 3), torch.zeros(2, 6, 15, 3)
    chain, mask = torch.zeros(2, 6), torch.ones(2, 6, dtype=torch.bool)
    out = tuple(torch.empty(2, 6, 3) for _ in range(3))
    check(xyz, g)
    check(xyz, g.double(), chain, mask, include_cb=True, want_bond_angles=True, want_bond_lengths=True, out=out)
    check(xyz[:, :, :3], g[:, :, :3])
    check(xyz, g, out=(out[0], None, None))
    with pytest.raises(ValueError):
        check(xyz[0], g[0])                                            # rank 3
    with pytest.raises(ValueError):
        check(xyz[..., :2], g[..., :2])                                # trailing axis
    with pytest.raises(ValueError):
        check(xyz, g[:, :5])                                           # a gradient of another shape
    with pytest.raises(ValueError):
        check(xyz, g.long())
    with pytest.raises(ValueError):
        check(xyz[:, :, :4], g[:, :, :4], include_cb=True)             # no CB slot
    with pytest.raises(ValueError):
        check(xyz[:, :, :2], g[:, :, :2])
    with pytest.raises(ValueError):
        check(xyz, g, chain[:, :5])
    with pytest.raises(ValueError):
        check(xyz, g, None, mask[:1])
    with pytest.raises(ValueError):
        check(xyz, g, out=out[0])                                      # not a triple
    with pytest.raises(ValueError):
        check(xyz, g, out=out)                                         # bond outputs given but not wanted
    with pytest.raises(ValueError):
        check(xyz, g, want_bond_angles=True, out=(out[0], out[1].double(), None))
    with pytest.raises(ValueError):
        check(xyz, g, out=(torch.empty(2, 5, 3), None, None))


def test_op_validates_first_then_refuses_cpu_tensors():
    from protstruc_amd import ops
    xyz, g = torch.zeros(1, 4, 15, 3), torch.zeros(1, 4, 15, 3)
    with pytest.raises(ValueError):
        ops.backbone_from_dihedrals_backward(xyz, g[:, :3])
    with pytest.raises(ValueError):
        ops.backbone_from_dihedrals_backward(xyz[:, :, :4], g[:, :, :4], include_cb=True)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.backbone_from_dihedrals_backward(xyz, g)


def test_public_surface():
    from protstruc_amd import geometry, ops
    assert callable(geometry.backbone_from_dihedrals)
    assert callable(ops.backbone_from_dihedrals_backward)
    assert callable(ops.check_backbone_from_dihedrals_backward_shapes)


def _stand_ins(monkeypatch, seen):
    """Both ops replaced by CPU stand-ins: the float32 restatement forwards, the float32 torque form (and a recorder of
    what was asked for) backwards."""
    from protstruc_amd import ops

    def fake_forward(dih, chain=None, rmask=None, ang=None, lens=None, include_cb=False, n_slots=15):
        ops.check_backbone_from_dihedrals_shapes(dih, chain, rmask, ang, lens)
        xyz = R.coordinates(dih, chain, rmask, ang, lens, include_cb, n_slots, dtype=torch.float32)
        return xyz, R.read_entries(dih.shape[0], dih.shape[1], n_slots, rmask, include_cb).float()

    def fake_backward(xyz, g, chain=None, rmask=None, *, include_cb=False, want_bond_angles=False, want_bond_lengths=False,
                      out=None):
        ops.check_backbone_from_dihedrals_backward_shapes(xyz, g, chain, rmask, include_cb, want_bond_angles,
                                                          want_bond_lengths, out)
        seen.append((want_bond_angles, want_bond_lengths))
        d, a, l = R.torque_gradient(xyz, g, chain, rmask, include_cb, dtype=torch.float32)
        return d, a if want_bond_angles else None, l if want_bond_lengths else None

    monkeypatch.setattr(ops, "backbone_from_dihedrals", fake_forward)
    monkeypatch.setattr(ops, "backbone_from_dihedrals_backward", fake_backward)


@pytest.mark.parametrize("needs", [(True, False, False), (True, True, False), (False, False, True), (True, True, True)])
def test_autograd_wrapper_asks_only_for_the_gradients_that_are_needed(monkeypatch, needs):
    """geometry.backbone_from_dihedrals hands the backward op want_bond_* = whether that input requires grad, and returns a
    gradient to exactly the inputs that require one.  Host-only (stand-ins for both ops)."""
    from protstruc_amd import geometry
    seen = []
    _stand_ins(monkeypatch, seen)
    c = R.make_case(dict(family="random", B=2, N=12, A=15, include_cb=True, perturbed=True, chains=True, seed=5, name="x"))
    inputs = [c["dihedrals"].clone(), c["bond_angles"].clone(), c["bond_lengths"].clone()]
    for t, need in zip(inputs, needs):
        t.requires_grad_(need)
    xyz, atom_mask = geometry.backbone_from_dihedrals(inputs[0], c["chain_idx"], c["residue_mask"], inputs[1], inputs[2],
                                                      include_cb=True, n_slots=15)
    assert xyz.grad_fn is not None and not atom_mask.requires_grad
    (c["grad_xyz"] * xyz).sum().backward()
    assert seen == [(needs[1], needs[2])]
    want = R.case_gradients(c, torch.float64)
    for t, need, w in zip(inputs, needs, want):
        assert (t.grad is not None) == need
        if need:
            assert t.grad.dtype == t.dtype and R.worst_error((t.grad,), (w,)) < 1e-4


def test_segment_rules_changed_in_place_before_backward_is_an_error(monkeypatch):
    from protstruc_amd import geometry
    _stand_ins(monkeypatch, [])
    c = R.make_case(dict(family="helix", B=1, N=8, A=15, include_cb=False, perturbed=False, chains=True, seed=6, name="x"))
    for which in ("chain_idx", "residue_mask"):
        dih = c["dihedrals"].clone().requires_grad_()
        rules = {"chain_idx": c["chain_idx"].clone(), "residue_mask": c["residue_mask"].clone()}
        xyz, _ = geometry.backbone_from_dihedrals(dih, rules["chain_idx"], rules["residue_mask"])
        rules[which].fill_(1)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            xyz.sum().backward()
