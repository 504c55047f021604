"""GPU tests of the featuriser's backward pass (ps_inter_residue_geometry_backward_f32, ops.inter_residue_geometry_backward,
geometry.inter_residue_geometry, StructureBatch.inter_residue_geometry on coordinates that require grad).

Yardstick: the float64 autograd gradient of the torch restatement in tests/irg_grad_ref.py.  With e(r) = the largest error
over residue r's entries divided by the residue's largest |gradient| and E = max_r e(r), the kernel has to stay within
four times the error of the SAME restatement evaluated by autograd in float32 on the CPU: E_kernel <= 4 E_f32 per case
(the kernel adds up to 2 N terms in another order and takes reciprocals from v_rcp_f32 / v_rsq_f32 where autograd
divides; anything much beyond a small multiple of a float32 reference hides a cancellation or a bug).  No residue is left
out, and a residue whose float64 gradient is identically zero must be exactly zero in the kernel's output.
"""
import os

import pytest
import torch

from tests import irg_grad_ref as R
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

MARGIN = 4.0
SHAPES, MASKS, random_case = R.SHAPES, R.MASKS, R.random_case


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


def to_gpu(xyz, mask, grads):
    return xyz.cuda(), None if mask is None else mask.cuda(), {k: v.cuda() for k, v in grads.items()}


def check_accuracy(ops, name, xyz, mask, grads):
    """E_kernel <= MARGIN * E_f32, every residue counted; exact zeros where the float64 gradient is identically zero and in
    every slot the featuriser does not read."""
    want = R.gradient(xyz, mask, grads)
    f32 = R.gradient(xyz, mask, grads, dtype=torch.float32)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    got = ops.inter_residue_geometry_backward(xg, gg, mg).cpu()
    assert got.shape == xyz.shape and got.dtype == torch.float32
    assert torch.isfinite(want).all() and torch.isfinite(f32).all()
    e_kernel, e_f32 = R.worst_error(got, want), R.worst_error(f32, want)
    print(f"{name}: E_kernel = {e_kernel:.3e}  E_f32 = {e_f32:.3e}  ratio = {e_kernel / e_f32 if e_f32 else float('nan'):.2f}")
    assert torch.isfinite(got).all(), name
    unused = [s for s in range(xyz.shape[2]) if s not in R.USED_SLOTS]
    assert (got[:, :, unused] == 0).all(), "slots the featuriser does not read must be exact zeros"
    dead = (want.reshape(*want.shape[:2], -1) == 0).all(-1)
    assert (got[dead] == 0).all(), "a residue with an identically zero gradient must be exactly zero"
    assert e_kernel <= MARGIN * e_f32, f"{name}: E_kernel {e_kernel:.3e} > {MARGIN} x E_f32 {e_f32:.3e}"
    return e_kernel, e_f32


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_randn(ops, shape, mask_kind):
    B, N, A = shape
    xyz, mask, grads = random_case(1000 + 7 * N + B, B, N, A, mask_kind)
    check_accuracy(ops, f"randn {shape} mask={mask_kind}", xyz, mask, grads)


def pdb_case():
    xyz, mask, grads = R.pdb_case(os.path.join(GOLDEN_DIR, "15c8_HL.pdb"))
    assert xyz.isnan().any(), "from_pdb stores NaN for missing atoms: the case is meant to carry them"
    return xyz, mask, grads


def test_accuracy_15c8_with_nan_coordinates(ops):
    xyz, mask, grads = pdb_case()
    assert xyz.shape[1] == 229
    check_accuracy(ops, "15c8_HL", xyz, mask, grads)


def test_nan_hygiene(ops):
    """NaN upstream values at every inactive entry and NaN coordinates at every masked atom: finite, and bit for bit the
    result of the clean run."""
    xyz, mask, grads = random_case(31, 2, 70, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    clean = ops.inter_residue_geometry_backward(xg, gg, mg)
    active = R.active_entries(2, 70, mask)
    dirty_grads = {k: torch.where(active[k], v, torch.full_like(v, float("nan"))) for k, v in grads.items()}
    dirty_xyz = torch.where(mask[..., None], xyz, torch.full_like(xyz, float("nan")))
    assert dirty_xyz.isnan().any() and all(v.isnan().any() for v in dirty_grads.values())
    xg, mg, gg = to_gpu(dirty_xyz, mask, dirty_grads)
    dirty = ops.inter_residue_geometry_backward(xg, gg, mg)
    assert torch.isfinite(dirty).all()
    assert torch.equal(dirty, clean)


def test_partial_upstreams(ops):
    """Each plane alone (the other five absent) equals the full call with zeros for the others; the six single-plane
    results add up to the full call within the accuracy bound."""
    xyz, mask, grads = random_case(77, 2, 45, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    full = ops.inter_residue_geometry_backward(xg, gg, mg)
    total = torch.zeros_like(full, dtype=torch.float64)
    for k in R.PLANES:
        alone = ops.inter_residue_geometry_backward(xg, {k: gg[k]}, mg)
        also_none = ops.inter_residue_geometry_backward(xg, {**{p: None for p in R.PLANES}, k: gg[k]}, mg)
        zeros = ops.inter_residue_geometry_backward(xg, {p: (gg[p] if p == k else torch.zeros_like(gg[p])) for p in R.PLANES}, mg)
        assert torch.equal(alone, zeros), k
        assert torch.equal(alone, also_none), k
        total += alone.double()
    want = R.gradient(xyz, mask, grads)
    f32 = R.gradient(xyz, mask, grads, dtype=torch.float32)
    e_sum, e_f32 = R.worst_error(total.cpu(), want), R.worst_error(f32, want)
    print(f"sum of single planes: E = {e_sum:.3e}  E_f32 = {e_f32:.3e}")
    assert e_sum <= MARGIN * e_f32
    nothing = ops.inter_residue_geometry_backward(xg, {}, mg)
    assert (nothing == 0).all()


def test_non_contiguous_and_non_fp32_upstreams(ops):
    xyz, mask, grads = random_case(78, 2, 37, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    full = ops.inter_residue_geometry_backward(xg, gg, mg)
    odd = dict(gg)
    odd["omega"] = gg["omega"].transpose(1, 2).contiguous().transpose(1, 2)     # same values, strided
    odd["d_cb"] = gg["d_cb"].double()
    assert not odd["omega"].is_contiguous()
    assert torch.equal(ops.inter_residue_geometry_backward(xg, odd, mg), full)


def test_deterministic(ops):
    xyz, mask, grads = random_case(5, 3, 200, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    a = ops.inter_residue_geometry_backward(xg, gg, mg)
    b = ops.inter_residue_geometry_backward(xg, gg, mg)
    assert torch.equal(a, b)


def test_independent_of_the_forward_arithmetic_modes(ops):
    xyz, mask, grads = random_case(6, 2, 50, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    base = ops.inter_residue_geometry_backward(xg, gg, mg)
    with ops.exact_sqrt(), ops.exact_angles():
        assert torch.equal(ops.inter_residue_geometry_backward(xg, gg, mg), base)


@pytest.mark.parametrize("shape", [(2, 33, 15), (1, 64, 7), (3, 5, 5)], ids=lambda s: "x".join(map(str, s)))
def test_inside_sentinels(ops, shape):
    """grad_xyz carved out of a larger buffer of sentinels: nothing outside it is written, and every element inside is --
    the slots the featuriser does not read hold exact zeros, not left-over sentinels."""
    B, N, A = shape
    xyz, mask, grads = random_case(90 + N, B, N, A)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    n, pad = B * N * A * 3, 1024
    buf = torch.full((n + 2 * pad,), -777.25, device="cuda")
    out = buf[pad:pad + n].view(B, N, A, 3)
    res = ops.inter_residue_geometry_backward(xg, gg, mg, out=out)
    assert res.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert (buf[:pad] == -777.25).all() and (buf[pad + n:] == -777.25).all()
    assert (out != -777.25).all()
    unused = [s for s in range(A) if s not in R.USED_SLOTS]
    assert (out[:, :, unused] == 0).all()
    assert torch.equal(out, ops.inter_residue_geometry_backward(xg, gg, mg))


def test_long_chain_takes_the_large_lds_launch(ops):
    """N = 2048 is the longest chain the kernel stages (more than 64 KB of dynamic LDS): a distance-only gradient against
    the closed form evaluated by torch on the GPU in float64."""
    g = torch.Generator().manual_seed(2048)
    xyz = torch.randn(1, 2048, 5, 3, generator=g).cuda()
    w = torch.randn(1, 2048, 2048, generator=g).cuda()
    got = ops.inter_residue_geometry_backward(xyz, {"d_ca": w})
    x = xyz.double().requires_grad_(True)
    ca = x[:, :, 1]
    d = (ca[:, :, None] - ca[:, None, :] + torch.eye(2048, device="cuda", dtype=torch.float64)[None, :, :, None]).norm(dim=-1)
    off = ~torch.eye(2048, dtype=torch.bool, device="cuda")[None]
    (want,) = torch.autograd.grad((torch.where(off, w.double(), 0.0) * d).sum(), x)
    # one float32 rounding per term (6e-8 of its size) over 2 x 2047 unit-vector terms of random sign and weight
    E = R.worst_error(got, want)
    print(f"N = 2048 d_ca only: E = {E:.3e}")
    assert E <= 1e-5
    with pytest.raises(ValueError):
        ops.inter_residue_geometry_backward(torch.zeros(1, 2049, 5, 3, device="cuda"), {})


def test_empty_batches(ops):
    for B, N in ((0, 4), (2, 0)):
        out = ops.inter_residue_geometry_backward(torch.zeros(B, N, 15, 3, device="cuda"), {"phi": torch.zeros(B, N, N, device="cuda")})
        assert out.shape == (B, N, 15, 3)


def test_autograd_end_to_end(ops):
    from protstruc_amd import StructureBatch, geometry
    xyz, mask, grads = random_case(41, 2, 60, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    x = xg.clone().requires_grad_()
    sb = StructureBatch.from_xyz(x, mg)
    geo = sb.inter_residue_geometry()
    assert list(geo) == ["d_ca", "d_ca_mask", "d_cb", "d_cb_mask", "d_no", "d_no_mask", "omega", "theta", "phi"]
    plain = ops.inter_residue_geometry(xg, mg)
    for k in R.PLANES:
        assert geo[k].grad_fn is not None and geo[k].requires_grad
        assert torch.equal(geo[k].detach().nan_to_num(9.0), plain[k].nan_to_num(9.0))       # phi's diagonal is NaN
    for k in ("d_ca_mask", "d_cb_mask", "d_no_mask"):
        assert not geo[k].requires_grad and torch.equal(geo[k], plain[k])
    active = {k: v.cuda() for k, v in R.active_entries(2, 60, mask).items()}
    # a weighted sum over the entries that have a derivative (the diagonal of phi is the forward's 0 / 0 NaN)
    loss = sum((torch.where(active[k], gg[k] * geo[k], 0.0)).sum() for k in R.PLANES)
    loss.backward()
    upstream = {k: torch.where(active[k], gg[k], 0.0) for k in R.PLANES}
    assert torch.equal(x.grad, ops.inter_residue_geometry_backward(xg, upstream, mg))

    # a loss on two planes only gives the gradient of those two planes
    x2 = xg.clone().requires_grad_()
    geo2 = geometry.inter_residue_geometry(x2, mg)
    assert list(geo2) == list(plain)
    (gg["d_cb"] * geo2["d_cb"] + gg["d_no"] * geo2["d_no"]).sum().backward()
    assert torch.equal(x2.grad, ops.inter_residue_geometry_backward(xg, {"d_cb": gg["d_cb"], "d_no": gg["d_no"]}, mg))


@pytest.mark.parametrize("used", [("d_cb",), ("d_cb", "d_no"), ("omega", "theta", "phi"), R.PLANES])
def test_unused_planes_reach_the_op_as_absent(ops, monkeypatch, used):
    """Backward is the new op with the upstream gradients of the planes the loss does not use ABSENT -- not materialised
    as (B,N,N) zeros, which would cost an allocation and a fill per plane and every block of the kernel."""
    from protstruc_amd import StructureBatch
    xyz, mask, grads = random_case(43, 2, 20, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    seen = []
    real = ops.inter_residue_geometry_backward

    def spy(xyz_, grads_, atom_mask_=None, **kw):
        seen.append({k for k, v in grads_.items() if v is not None})
        return real(xyz_, grads_, atom_mask_, **kw)

    monkeypatch.setattr(ops, "inter_residue_geometry_backward", spy)
    x = xg.clone().requires_grad_()
    geo = StructureBatch.from_xyz(x, mg).inter_residue_geometry()
    active = {k: v.cuda() for k, v in R.active_entries(2, 20, mask).items()}
    sum(torch.where(active[k], gg[k] * geo[k], 0.0).sum() for k in used).backward()
    assert seen == [set(used)]
    assert torch.equal(x.grad, real(xg, {k: torch.where(active[k], gg[k], 0.0) for k in used}, mg))


def test_mask_changed_in_place_before_backward_is_an_error(ops):
    from protstruc_amd import geometry
    xyz, mask, grads = random_case(44, 1, 12, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    geo = geometry.inter_residue_geometry(xg.requires_grad_(), mg)
    mg.fill_(True)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (gg["d_ca"] * geo["d_ca"]).sum().backward()


def test_no_grad_paths_are_the_plain_featuriser(ops):
    from protstruc_amd import StructureBatch
    xyz, mask, _ = random_case(42, 2, 40, 15, "float")
    xg, mg = xyz.cuda(), mask.cuda()
    plain = StructureBatch.from_xyz(xg, mg).inter_residue_geometry()
    x = xg.clone().requires_grad_()
    with torch.no_grad():
        quiet = StructureBatch.from_xyz(x, mg).inter_residue_geometry()
    raw = ops.inter_residue_geometry(xg, mg)
    for geo in (plain, quiet):
        assert list(geo) == list(plain)
        for k, v in geo.items():
            assert v.grad_fn is None and not v.requires_grad
            if k.endswith("_mask"):
                assert v.dtype == mg.dtype and torch.equal(v, raw[k].to(mg.dtype))
            else:
                assert torch.equal(v.nan_to_num(9.0), raw[k].nan_to_num(9.0))
    tracked = StructureBatch.from_xyz(x, mg).inter_residue_geometry()
    for k in ("d_ca_mask", "d_cb_mask", "d_no_mask"):
        assert not tracked[k].requires_grad and tracked[k].dtype == mg.dtype


def test_inside_a_captured_graph(ops):
    """The op captured in torch.cuda.graph and replayed twice gives the eager result (no allocation, synchronisation or
    host read on the launch path)."""
    xyz, mask, grads = random_case(4244, 3, 131, 15)
    xg, mg, gg = to_gpu(xyz, mask, grads)
    out = torch.empty_like(xg)
    ops.inter_residue_geometry_backward(xg, gg, mg, out=out)            # eager first: loads the code object
    eager = out.clone()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ops.inter_residue_geometry_backward(xg, gg, mg, out=out)
    for _ in range(2):
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
