"""GPU tests of the backbone builder's backward pass (ps_backbone_from_dihedrals_backward_f32,
ops.backbone_from_dihedrals_backward, geometry.backbone_from_dihedrals, StructureBatch.from_backbone_dihedrals on angles
that require grad).

Yardstick: tests/nerf_grad_ref.py -- the sequential builder restated in torch and differentiated by autograd in float64
("want").  Per structure and per output kind (dihedrals, bond angles, bond lengths) e = max |got - want| / max |want|,
E = the largest e of the case; a kind whose ``want`` is identically zero for a structure must be exactly zero.  The
kernel has to stay within MARGIN = 4 times the error of the SAME restatement differentiated by autograd in float32 on the
CPU: E_kernel <= 4 E_f32, the margin of the featuriser's backward test (tests/test_gpu_irg_backward.py).  The kernel
reads K7's float32 coordinates and sums forces and torques in a tree, where float32 autograd carries the rounding of 3 N
dependent placements, so it is expected well below 1 x (tests/test_nerf_backward_host.py prints the float32 figures of the
closed form on the CPU).  No case and no structure is left out.
"""
import numpy as np
import pytest
import torch

from tests import irg_grad_ref as IR
from tests import nerf_grad_ref as R
from tests import nerf_ref

pytestmark = pytest.mark.gpu

MARGIN = 4.0
CASES = R.accuracy_cases()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


def cuda(t):
    return None if t is None else t.cuda()


def forward(ops, c, **over):
    a = {**c, **over}
    return ops.backbone_from_dihedrals(cuda(a["dihedrals"]), cuda(a["chain_idx"]), cuda(a["residue_mask"]),
                                       cuda(a["bond_angles"]), cuda(a["bond_lengths"]), include_cb=a["include_cb"],
                                       n_slots=a["n_slots"])


def backward(ops, c, xyz, grad_xyz=None, both=True, **kw):
    g = c["grad_xyz"] if grad_xyz is None else grad_xyz
    return ops.backbone_from_dihedrals_backward(xyz, cuda(g), cuda(c["chain_idx"]), cuda(c["residue_mask"]),
                                                include_cb=c["include_cb"], want_bond_angles=both, want_bond_lengths=both, **kw)


def small_case(N, seed, B=3, A=15, include_cb=True, perturbed=True, chains=True, family="random"):
    return R.make_case(dict(family=family, B=B, N=N, A=A, include_cb=include_cb, perturbed=perturbed, chains=chains,
                            seed=seed, name="small"))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_accuracy(ops, case):
    c = R.make_case(case)
    want = R.case_gradients(c, torch.float64)
    f32 = R.case_gradients(c, torch.float32)
    xyz, _ = forward(ops, c)
    got = [g.cpu() for g in backward(ops, c, xyz)]
    for g in got:
        assert g.shape == (case["B"], case["N"], 3) and g.dtype == torch.float32
    assert all(torch.isfinite(w).all() for w in want) and all(torch.isfinite(w).all() for w in f32)
    e_kernel, e_f32 = R.worst_error(got, want), R.worst_error(f32, want)
    print(f"{case['name']}: E_kernel = {e_kernel:.3e}  E_f32 = {e_f32:.3e}  ratio = {e_kernel / e_f32 if e_f32 else float('nan'):.3f}")
    unused = torch.from_numpy(~nerf_ref.used_angles(case["B"], case["N"], None if c["chain_idx"] is None else c["chain_idx"].numpy(),
                                                    None if c["residue_mask"] is None else c["residue_mask"].numpy()))
    assert (got[0][unused] == 0).all(), "angles the builder never reads must get exact zeros"
    for g, w in zip(got, want):
        assert (g[w == 0] == 0).all(), "an entry with an identically zero gradient must be exactly zero"
    assert e_kernel <= MARGIN * e_f32, f"{case['name']}: E_kernel {e_kernel:.3e} > {MARGIN} x E_f32 {e_f32:.3e}"


def test_nan_hygiene_and_exact_zeros(ops):
    """NaN in every unused dihedral entry, in grad_xyz at masked rows and unread slots, and in the xyz slots the builder
    leaves alone: bit for bit the clean result, with exact zeros at every unused entry."""
    for include_cb in (True, False):
        c = small_case(70, 31, include_cb=include_cb)
        B, N, A = 3, 70, 15
        xyz, _ = forward(ops, c)
        clean = backward(ops, c, xyz)
        chain, rmask = c["chain_idx"].numpy(), c["residue_mask"].numpy()
        unused = torch.from_numpy(nerf_ref.unused_angles(B, N, chain, rmask))
        dirty_dih = torch.where(unused, torch.tensor(float("nan")), c["dihedrals"])
        read = R.read_entries(B, N, A, c["residue_mask"], include_cb)
        dirty_g = torch.where(read[..., None], c["grad_xyz"], torch.tensor(float("nan")))
        dirty_xyz, _ = forward(ops, c, dihedrals=dirty_dih)
        assert torch.equal(dirty_xyz, xyz)
        left_alone = torch.ones(A, dtype=torch.bool)
        left_alone[[0, 1, 2] + ([4] if include_cb else [])] = False
        dirty_xyz[:, :, left_alone.cuda()] = float("nan")
        assert dirty_dih.isnan().any() and dirty_g.isnan().any() and dirty_xyz.isnan().any()
        dirty = backward(ops, c, dirty_xyz, dirty_g)
        for d, cl in zip(dirty, clean):
            assert torch.isfinite(d).all() and torch.equal(d, cl)
        not_used = torch.from_numpy(~nerf_ref.used_angles(B, N, chain, rmask)).cuda()
        assert (clean[0][not_used] == 0).all()
        dead = ~c["residue_mask"].cuda()
        assert (clean[1][dead][:, 0] == 0).all() and (clean[2][dead][:, :2] == 0).all()


def test_bond_outputs_absent_equals_present(ops):
    c = small_case(133, 32)
    xyz, _ = forward(ops, c)
    d3, a3, l3 = backward(ops, c, xyz)
    d1, a1, l1 = backward(ops, c, xyz, both=False)
    assert a1 is None and l1 is None and torch.equal(d1, d3)
    d2, a2, l2 = ops.backbone_from_dihedrals_backward(xyz, c["grad_xyz"].cuda(), c["chain_idx"].cuda(), c["residue_mask"].cuda(),
                                                      include_cb=True, want_bond_lengths=True)
    assert a2 is None and torch.equal(d2, d3) and torch.equal(l2, l3)


def test_deterministic(ops):
    c = small_case(1300, 33, B=2)
    xyz, _ = forward(ops, c)
    first, second = backward(ops, c, xyz), backward(ops, c, xyz)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2, 33, 15), (1, 600, 7), (3, 5, 5), (2, 1, 15), (2, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_inside_sentinels(ops, shape):
    """The three outputs carved out of larger buffers of sentinels: nothing outside them is written, every element
    inside is."""
    B, N, A = shape
    c = small_case(N, 90 + N, B=B, A=A, include_cb=A >= 5, chains=N >= 33)
    xyz, _ = forward(ops, c)
    n, pad = B * N * 3, 512
    bufs = [torch.full((n + 2 * pad,), -777.25, device="cuda") for _ in range(3)]
    outs = tuple(b[pad:pad + n].view(B, N, 3) for b in bufs)
    res = backward(ops, c, xyz, out=outs)
    torch.cuda.synchronize()
    plain = backward(ops, c, xyz)
    for r, o, b, p in zip(res, outs, bufs, plain):
        assert r.data_ptr() == o.data_ptr()
        assert (b[:pad] == -777.25).all() and (b[pad + n:] == -777.25).all()
        assert (o != -777.25).all() and torch.equal(o, p)


@pytest.mark.parametrize("N", [1, 2])
def test_shortest_chains(ops, N):
    """N = 1: only the first residue's own bond parameters move anything; N = 2: one junction.  Against float64 autograd,
    over 256 structures: a chain this short has a handful of roundings per entry, at the float32 floor for the kernel and
    for float32 autograd alike, so over a few structures the ratio of the two maxima is the luck of single roundings."""
    c = small_case(N, 50 + N, B=256, chains=False)
    want = R.case_gradients(c, torch.float64)
    f32 = R.case_gradients(c, torch.float32)
    xyz, _ = forward(ops, c)
    got = [g.cpu() for g in backward(ops, c, xyz)]
    if N == 1:
        assert (got[0] == 0).all() and (want[0] == 0).all()
    for g, w in zip(got, want):
        assert (g[w == 0] == 0).all()
    e_kernel, e_f32 = R.worst_error(got, want), R.worst_error(f32, want)
    print(f"N = {N}: E_kernel = {e_kernel:.3e}  E_f32 = {e_f32:.3e}")
    assert e_kernel <= MARGIN * e_f32


def test_empty_batches(ops):
    for B, N in ((0, 4), (2, 0)):
        z = torch.zeros(B, N, 15, 3, device="cuda")
        d, a, l = ops.backbone_from_dihedrals_backward(z, z, include_cb=True, want_bond_angles=True, want_bond_lengths=True)
        assert d.shape == a.shape == l.shape == (B, N, 3)


def test_non_contiguous_and_float64_upstream(ops):
    c = small_case(47, 34)
    xyz, _ = forward(ops, c)
    base = backward(ops, c, xyz)
    g = c["grad_xyz"].cuda()
    strided = g.transpose(1, 2).contiguous().transpose(1, 2)
    assert not strided.is_contiguous()
    for odd in (strided, g.double()):
        for a, b in zip(backward(ops, c, xyz, odd), base):
            assert torch.equal(a, b)


def test_inside_a_captured_graph(ops):
    """The op captured in torch.cuda.graph and replayed twice gives the eager result (no allocation, synchronisation or
    host read on the launch path)."""
    c = small_case(700, 35)
    xyz, _ = forward(ops, c)
    g, chain, rmask = c["grad_xyz"].cuda(), c["chain_idx"].cuda(), c["residue_mask"].cuda()
    outs = tuple(torch.empty(3, 700, 3, device="cuda") for _ in range(3))

    def run():
        ops.backbone_from_dihedrals_backward(xyz, g, chain, rmask, include_cb=True, want_bond_angles=True,
                                             want_bond_lengths=True, out=outs)

    run()                                                             # eager first: loads the code object
    eager = [o.clone() for o in outs]
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run()
    for _ in range(2):
        for o in outs:
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)


# ---- autograd ----

def test_backward_is_the_op(ops):
    from protstruc_amd import geometry
    c = small_case(90, 36)
    dih, ang, lens = (cuda(c[k]).requires_grad_() for k in ("dihedrals", "bond_angles", "bond_lengths"))
    chain, rmask, g = c["chain_idx"].cuda(), c["residue_mask"].cuda(), c["grad_xyz"].cuda()
    xyz, atom_mask = geometry.backbone_from_dihedrals(dih, chain, rmask, ang, lens, include_cb=True, n_slots=15)
    px, pm = forward(ops, c)
    assert xyz.grad_fn is not None and torch.equal(xyz.detach(), px)
    assert not atom_mask.requires_grad and torch.equal(atom_mask, pm)
    (g * xyz).sum().backward()
    direct = backward(ops, c, px)
    for t, d in zip((dih, ang, lens), direct):
        assert torch.equal(t.grad, d)


@pytest.mark.parametrize("needs", [(True, False, False), (True, False, True), (False, True, False), (True, True, True)])
def test_unneeded_bond_gradients_reach_the_op_as_absent(ops, monkeypatch, needs):
    """Backward is the new op with the bond outputs nobody needs ABSENT: their arithmetic and stores are skipped."""
    from protstruc_amd import geometry
    c = small_case(40, 37)
    seen = []
    real = ops.backbone_from_dihedrals_backward

    def spy(*args, **kw):
        seen.append((kw.get("want_bond_angles", False), kw.get("want_bond_lengths", False)))
        out = real(*args, **kw)
        assert (out[1] is not None, out[2] is not None) == seen[-1]
        return out

    monkeypatch.setattr(ops, "backbone_from_dihedrals_backward", spy)
    inputs = [cuda(c[k]).requires_grad_(need) for k, need in zip(("dihedrals", "bond_angles", "bond_lengths"), needs)]
    xyz, _ = geometry.backbone_from_dihedrals(inputs[0], c["chain_idx"].cuda(), c["residue_mask"].cuda(), inputs[1], inputs[2],
                                              include_cb=True)
    (c["grad_xyz"].cuda() * xyz).sum().backward()
    assert seen == [(needs[1], needs[2])]
    direct = backward(ops, c, xyz.detach())
    for t, need, d in zip(inputs, needs, direct):
        assert (t.grad is not None) == need
        if need:
            assert torch.equal(t.grad, d)


def test_segment_rules_changed_in_place_before_backward_is_an_error(ops):
    from protstruc_amd import geometry
    c = small_case(12, 38, B=1)
    chain, rmask = c["chain_idx"].cuda(), c["residue_mask"].cuda()
    xyz, _ = geometry.backbone_from_dihedrals(c["dihedrals"].cuda().requires_grad_(), chain, rmask)
    rmask.fill_(True)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        xyz.sum().backward()


def test_no_grad_paths_are_the_plain_builder(ops):
    from protstruc_amd import StructureBatch
    c = small_case(40, 39, B=2, chains=False)
    plain_xyz, plain_mask = ops.backbone_from_dihedrals(c["dihedrals"].cuda(), None, None, c["bond_angles"].cuda(),
                                                        c["bond_lengths"].cuda(), include_cb=True, n_slots=15)
    kw = dict(bond_angles=c["bond_angles"].cuda(), bond_lengths=c["bond_lengths"].cuda(), include_cb=True)
    no_input_needs_grad = StructureBatch.from_backbone_dihedrals(c["dihedrals"].cuda(), **kw)
    d = c["dihedrals"].cuda().requires_grad_()
    with torch.no_grad():
        quiet = StructureBatch.from_backbone_dihedrals(d, **kw)
    for sb in (no_input_needs_grad, quiet):
        assert sb.get_xyz().grad_fn is None and not sb.get_xyz().requires_grad
        assert torch.equal(sb.get_xyz(), plain_xyz) and torch.equal(sb.atom_mask, plain_mask)
    tracked = StructureBatch.from_backbone_dihedrals(d, **kw)
    assert tracked.get_xyz().grad_fn is not None and torch.equal(tracked.get_xyz().detach(), plain_xyz)
    assert not tracked.atom_mask.requires_grad and torch.equal(tracked.atom_mask, plain_mask)
    # the bond parameters alone requiring grad take the differentiable path as well
    ang = c["bond_angles"].cuda().requires_grad_()
    sb = StructureBatch.from_backbone_dihedrals(c["dihedrals"].cuda(), bond_angles=ang, bond_lengths=kw["bond_lengths"], include_cb=True)
    sb.get_xyz()[:, :, :3].sum().backward()
    assert ang.grad is not None and d.grad is None


E2E_PLANES = ("d_cb", "omega", "theta", "phi")


def e2e_host_loss(dih, weights, dtype):
    """The end-to-end loss by the host restatements in ``dtype``: sequential walk -> the featuriser's planes -> weighted sum
    over the active entries of d_cb, omega, theta, phi.  ``dih`` (B, N, 3) of ``dtype``; differentiable."""
    B, N = dih.shape[:2]
    ang, lens = (t.to(dtype) for t in R.geometry_or_default(B, N))
    xyz = R.build(dih, None, None, ang, lens, True, 15)
    return IR.weighted_sum(xyz, R.read_entries(B, N, 15, None, True), {k: v.to(dtype) for k, v in weights.items()})


def test_end_to_end_through_the_featuriser(ops):
    """dihedrals -> from_backbone_dihedrals(include_cb=True) -> inter_residue_geometry() -> loss -> backward(): the two
    backward ops composed by hand bit for bit, and the directional derivative along three seeded directions against a
    central difference of the same loss in float64 on the host.
    Step: h = 1e-6 puts the truncation error (h^2 times a third derivative) and the rounding error (1e-16 |L| / h) of
    the float64 central difference many orders below float32 rounding.  Tolerance: MARGIN times the largest disagreement
    the float32 CPU autograd of the same restatements shows against the same central differences (both relative to
    sum |g_k v_k|, the size of the terms the directional derivative adds up)."""
    from protstruc_amd import StructureBatch
    B, N = 2, 60
    dih = torch.from_numpy(nerf_ref.chain_family("helix", B, N, 4100))
    gen = torch.Generator().manual_seed(4101)
    weights = {k: torch.randn(B, N, N, generator=gen) for k in E2E_PLANES}
    d = dih.cuda().requires_grad_()
    sb = StructureBatch.from_backbone_dihedrals(d, include_cb=True)
    assert sb.get_xyz().grad_fn is not None
    geo = sb.inter_residue_geometry()
    active = {k: v.cuda() for k, v in IR.active_entries(B, N, R.read_entries(B, N, 15, None, True)).items()}
    assert all(active[k].sum() == B * N * (N - 1) for k in E2E_PLANES)
    loss = sum(torch.where(active[k], weights[k].cuda() * geo[k], 0.0).sum() for k in E2E_PLANES)
    loss.backward()
    xyz, atom_mask = ops.backbone_from_dihedrals(dih.cuda(), include_cb=True, n_slots=15)
    upstream = {k: torch.where(active[k], weights[k].cuda(), 0.0) for k in E2E_PLANES}
    grad_xyz = ops.inter_residue_geometry_backward(xyz, upstream, atom_mask)
    by_hand = ops.backbone_from_dihedrals_backward(xyz, grad_xyz, include_cb=True)[0]
    assert torch.equal(d.grad, by_hand)

    got = d.grad.cpu().double()
    d32 = dih.clone().requires_grad_()
    (f32,) = torch.autograd.grad(e2e_host_loss(d32, weights, torch.float32), d32)
    f32 = f32.double()
    d64 = dih.double()
    h, err_gpu, err_f32 = 1e-6, 0.0, 0.0
    gen = torch.Generator().manual_seed(4102)
    with torch.no_grad():
        for _ in range(3):
            v = torch.randn(B, N, 3, generator=gen, dtype=torch.float64)
            fd = float(e2e_host_loss(d64 + h * v, weights, torch.float64) - e2e_host_loss(d64 - h * v, weights, torch.float64)) / (2 * h)
            for name, grad in (("gpu", got), ("f32", f32)):
                rel = abs(float((grad * v).sum()) - fd) / float((grad * v).abs().sum())
                print(f"direction: central difference {fd:.9e}  {name} {float((grad * v).sum()):.9e}  relative {rel:.2e}")
                if name == "gpu":
                    err_gpu = max(err_gpu, rel)
                else:
                    err_f32 = max(err_f32, rel)
    print(f"end to end: GPU {err_gpu:.3e}  float32 CPU autograd {err_f32:.3e}  (tolerance {MARGIN} x the latter)")
    assert err_gpu <= MARGIN * err_f32


def descent_loss(geo, target):
    return sum(((geo[k] - target[k]) ** 2).sum() for k in ("d_ca", "d_cb")) / geo["d_ca"].numel()


def test_descent_in_torsion_space(ops):
    """Target geometry from a helix, start 0.2 rad away, 20 plain gradient steps.  The step is small enough that the float64
    host restatement's loss falls at every step (asserted: that validates the step, not the kernel); of the GPU only
    that the loss after the last step is below the first."""
    from protstruc_amd import StructureBatch
    B, N, STEP, STEPS = 2, 60, 2e-4, 20
    target_dih = torch.from_numpy(nerf_ref.chain_family("helix", B, N, 4200))
    rng = np.random.default_rng(4201)
    start = target_dih + torch.from_numpy(rng.choice([-0.2, 0.2], size=(B, N, 3)).astype(np.float32))

    def host_geo(dih):
        ang, lens = (t.double() for t in R.geometry_or_default(B, N))
        xyz = R.build(dih, None, None, ang, lens, True, 15)
        return {"d_ca": IR._distance(xyz[:, :, None, 1], xyz[:, None, :, 1] + torch.eye(N, dtype=torch.float64)[None, :, :, None]),
                "d_cb": IR._distance(xyz[:, :, None, 4], xyz[:, None, :, 4] + torch.eye(N, dtype=torch.float64)[None, :, :, None])}

    with torch.no_grad():
        host_target = host_geo(target_dih.double())
    x, host_losses = start.double(), []
    for _ in range(STEPS + 1):
        x = x.detach().requires_grad_()
        loss = descent_loss(host_geo(x), host_target)
        host_losses.append(float(loss.detach()))
        (g,) = torch.autograd.grad(loss, x)
        x = x - STEP * g
    assert all(b < a for a, b in zip(host_losses, host_losses[1:])), host_losses

    with torch.no_grad():
        target = StructureBatch.from_backbone_dihedrals(target_dih.cuda(), include_cb=True).inter_residue_geometry()
    d, gpu_losses = start.cuda(), []
    for _ in range(STEPS + 1):
        d = d.detach().requires_grad_()
        loss = descent_loss(StructureBatch.from_backbone_dihedrals(d, include_cb=True).inter_residue_geometry(), target)
        gpu_losses.append(float(loss))
        loss.backward()
        d = d - STEP * d.grad
    print(f"descent: host {host_losses[0]:.4f} -> {host_losses[-1]:.4f}, GPU {gpu_losses[0]:.4f} -> {gpu_losses[-1]:.4f}")
    assert gpu_losses[-1] < gpu_losses[0]
