"""Host-side checks of the featuriser's backward pass: the yardstick itself (tests/irg_grad_ref.py), the C ABI's surface and
the argument validation of ``ops.inter_residue_geometry_backward``.  No GPU needed."""
import ctypes

import pytest
import torch

from oracle import protstruc_oracle as O
from tests import irg_grad_ref as R
from tests.conftest import load_golden

SYMBOL = "ps_inter_residue_geometry_backward_f32"


def random_case(seed, B, N, A=15):
    return R.random_case(seed, B, N, A, "bool")


def test_restatement_forward_equals_the_oracle_at_active_entries():
    """In float32 the restatement's six planes equal oracle.inter_residue_geometry on the golden inputs within the
    project's 1e-5 gate at every active entry (inactive entries hold the stand-in's value and are not compared)."""
    g = load_golden("g8_inter_residue_geometry")
    want = O.inter_residue_geometry(g["xyz"], g["atom_mask"])
    got, active = R.planes(g["xyz"], g["atom_mask"])
    for plane in R.PLANES:
        a = active[plane]
        assert a.any(), plane
        assert got[plane].dtype == torch.float32
        d = (got[plane] - want[plane])[a].abs()
        # omega / theta live on a circle: -pi and pi are the same angle
        if plane in ("omega", "theta"):
            d = torch.minimum(d, (2 * torch.pi - d).abs())
        assert not d.isnan().any(), plane
        assert float(d.max()) <= 1e-5, (plane, float(d.max()))


@pytest.mark.parametrize("case", ["golden", "randn"])
def test_float64_gradient_agrees_with_central_differences(case):
    """<gradient, v> against (L(x + h v) - L(x - h v)) / (2 h) in float64 along 8 random directions.
    Step and tolerance: with coordinates and directions of unit scale, the central difference has a truncation error of
    h^2 |L'''| / 6 and a rounding error of eps |L| / h (eps = 1.1e-16).  L is a sum of ~6 B N^2 terms of order one with
    derivatives of order one per unit step away from degenerate pairs, so h = 1e-5 puts both near 1e-10 |L'| -- four
    orders below the 1e-6 relative tolerance asserted, which leaves room for the pairs close to a degenerate geometry
    (third derivatives grow like the inverse cube of the distance to it).  "Relative" is relative to sum |gradient_k v_k|,
    the size of the terms the directional derivative adds up: the derivative itself is a sum of random signs that can
    cancel to any value, so it is no scale for its own error."""
    if case == "golden":
        g = load_golden("g8_inter_residue_geometry")
        xyz, mask = g["xyz"], g["atom_mask"]
        gen = torch.Generator().manual_seed(11)
        grads = {k: torch.randn(xyz.shape[0], xyz.shape[1], xyz.shape[1], generator=gen) for k in R.PLANES}
    else:
        xyz, mask, grads = random_case(5, 2, 24)
    x = xyz.double()
    clean = x.nan_to_num(0.0)     # a direction may not move NaN coordinates; they belong to absent atoms only
    grad = R.gradient(xyz, mask, grads)
    assert torch.isfinite(grad).all()
    unused = [s for s in range(x.shape[2]) if s not in R.USED_SLOTS]
    assert (grad[:, :, unused] == 0).all()
    h = 1e-5
    gen = torch.Generator().manual_seed(3)
    gd = {k: v.double() for k, v in grads.items()}
    for _ in range(8):
        v = torch.randn(x.shape, generator=gen, dtype=torch.float64)
        v = torch.where(x.isnan(), torch.zeros_like(v), v)
        up = R.weighted_sum(torch.where(x.isnan(), x, clean + h * v), mask, gd)
        down = R.weighted_sum(torch.where(x.isnan(), x, clean - h * v), mask, gd)
        fd = float(up - down) / (2 * h)
        an, scale = float((grad * v).sum()), float((grad * v).abs().sum())
        print(f"{case}: analytic {an:.12e} finite difference {fd:.12e} relative {abs(an - fd) / scale:.2e}")
        assert abs(an - fd) <= 1e-6 * scale


def test_float32_autograd_of_the_restatement_is_close_to_float64():
    """The figure the GPU test measures the kernel against, E_f32 (about 2e-5 on input of this kind), printed.  The bound
    is a sanity check of the yardstick and not a rounding budget: float32's 6e-8 amplified by the conditioning of the
    worst pair of 2 x 64^2 random ones stays orders below 1e-3; a wrong sign or a missing term does not."""
    xyz, mask, grads = random_case(7, 2, 64)
    want = R.gradient(xyz, mask, grads)
    got = R.gradient(xyz, mask, grads, dtype=torch.float32)
    assert torch.isfinite(got).all()
    E = R.worst_error(got, want)
    print(f"E_f32 = {E:.3e}")
    assert E < 1e-3


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 or N = 0 launches nothing (the pointers are never
    dereferenced)."""
    from protstruc_amd import _lib
    fn = getattr(_lib.load(), SYMBOL)
    fake = ctypes.c_void_p(0x1000)
    none6 = [None] * 6
    assert fn(None, None, *none6, fake, 1, 4, 15, None) == 1           # no coordinates
    assert fn(fake, None, *none6, None, 1, 4, 15, None) == 1           # no output
    assert fn(fake, None, *none6, fake, 1, 4, 4, None) == 1            # A < 5
    assert fn(fake, None, *none6, fake, -1, 4, 15, None) == 1
    assert fn(fake, None, *none6, fake, 1, 2049, 15, None) == 1        # beyond the staged length
    assert fn(fake, None, *none6, fake, 0, 4, 15, None) == 0
    assert fn(fake, None, *none6, fake, 3, 0, 15, None) == 0


def test_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_inter_residue_geometry_backward_shapes
    xyz, mask, grads = random_case(1, 2, 6)
    check(xyz, grads, mask)
    check(xyz, {}, None)
    check(xyz, {"phi": grads["phi"], "d_no": None})
    with pytest.raises(ValueError):
        check(xyz[0], grads)                                           # rank 3
    with pytest.raises(ValueError):
        check(xyz[..., :2], grads)                                     # trailing axis
    with pytest.raises(ValueError):
        check(xyz, {"omega": grads["omega"][:, :5]})                   # a gradient of another shape
    with pytest.raises(ValueError):
        check(xyz, {"omega": grads["omega"][0]})
    with pytest.raises(ValueError):
        check(xyz, grads, mask[:, :, :5])
    with pytest.raises(ValueError):
        check(xyz, grads, out=torch.empty(2, 6, 15, 3, dtype=torch.float64))
    with pytest.raises(KeyError):
        check(xyz, {"d_ca_mask": grads["d_ca"]})
    with pytest.raises(KeyError):
        check(xyz, {"psi": grads["d_ca"]})
    with pytest.raises(IndexError):
        check(xyz[:, :, :4], grads)                                    # A < 5, as the forward raises
    with pytest.raises(ValueError):
        check(torch.zeros(1, 2049, 5, 3), {})


def test_op_validates_first_then_refuses_cpu_tensors():
    from protstruc_amd import ops
    xyz, mask, grads = random_case(2, 1, 4)
    with pytest.raises(IndexError):
        ops.inter_residue_geometry_backward(xyz[:, :, :4], grads)
    with pytest.raises(KeyError):
        ops.inter_residue_geometry_backward(xyz, {"nope": grads["phi"]})
    with pytest.raises(ValueError):
        ops.inter_residue_geometry_backward(xyz, {"phi": grads["phi"][:, :3]})
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.inter_residue_geometry_backward(xyz, grads, mask)


def test_public_surface():
    from protstruc_amd import geometry, ops
    assert callable(geometry.inter_residue_geometry)
    assert callable(ops.inter_residue_geometry_backward)
    assert ops.IRG_GRAD_KEYS == R.PLANES


@pytest.mark.parametrize("used", [("d_cb",), ("d_ca", "phi"), R.PLANES])
def test_autograd_wrapper_passes_unused_planes_as_absent(monkeypatch, used):
    """geometry.inter_residue_geometry hands the backward op exactly the planes the loss used: the others arrive absent,
    not as zero tensors.  Host-only: both ops are replaced by CPU stand-ins (the restatement's planes; a recorder)."""
    from protstruc_amd import geometry, ops
    xyz, mask, grads = random_case(9, 2, 6)
    seen = []

    def fake_forward(x, m=None):
        vals, active = R.planes(x.detach(), m)
        return {**vals, "d_ca_mask": active["d_ca"], "d_cb_mask": active["d_cb"], "d_no_mask": active["d_no"]}

    def fake_backward(x, g, m=None, **kw):
        ops.check_inter_residue_geometry_backward_shapes(x, g, m)
        seen.append({k for k, v in g.items() if v is not None})
        with torch.enable_grad():    # a backward pass runs with grad mode off; the stand-in differentiates the restatement
            return R.gradient(x, m, {k: v for k, v in g.items() if v is not None}, dtype=torch.float32)

    monkeypatch.setattr(ops, "inter_residue_geometry", fake_forward)
    monkeypatch.setattr(ops, "inter_residue_geometry_backward", fake_backward)
    x = xyz.clone().requires_grad_()
    geo = geometry.inter_residue_geometry(x, mask)
    assert list(geo) == list(R.PLANES) + ["d_ca_mask", "d_cb_mask", "d_no_mask"]
    assert all(geo[k].requires_grad for k in R.PLANES) and not any(geo[k].requires_grad for k in list(geo)[6:])
    sum((grads[k] * geo[k]).sum() for k in used).backward()
    assert seen == [set(used)]
    assert x.grad.shape == xyz.shape and torch.isfinite(x.grad).all()
