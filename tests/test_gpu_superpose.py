"""The superposition kernels on the GPU (K37 - K40) against tests/superpose_ref.py, the float64 restatement of
include/protstruc_superpose.h: the weighted fit and its RMSD, the gradient against torch-float64 autograd of an SVD Kabsch
RMSD, the seeded search against the restated search on cases that tests/test_superpose_host.py has shown to be off every
knife edge, the StructureBatch methods on two PDB files; and, since include/protstruc_superpose.h is not in the case table
of tests/launch_cases.py, this file also holds the three launchers to the launch contract: the caller's stream, capture,
four threads, the batch limit.

The search cases "n = ..." count the points AFTER masking; with 45 % of the slots masked over NaN the arrays are M = n / 0.55
long (467 at n = 257).  Masked slots cost a chain nothing."""
import functools
import os
import threading

import numpy as np
import pytest
import torch

from tests import align_ref
from tests import superpose_ref as R
from tests.launch_cases import Case, on_device
from tests.test_gpu_closest import carve
from tests.test_gpu_launch_contract import (SENTINEL, SLEEP_CYCLES, assert_all_same, assert_batch_of_65535_repeats_the_three,
                                            raw, same, side_stream_beside_the_default_stream)
from tests.test_superpose_host import PDB_CASES, pdb_case, svd_rmsd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
# the worst |rmsd - restatement| measured on an MI355X over the identical-cloud cases of test_tau_on_identical_clouds (a = b:
# both sides return the rounding noise of their own 3x3 solve; b a rigid motion of a: the rounding of b's coordinates) and
# TAU = 4 x that: the absolute term of the RMSD bound, which covers the rounding of R a + t - b where the RMSD is near 0
MEASURED_IDENTICAL_ERROR = 3.0e-14      # 2.966e-14, at "rigid motion, n = 4"
TAU = 4 * MEASURED_IDENTICAL_ERROR
SCORE_TOL = 1e-6


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---- K37 -------------------------------------------------------------------------------------------------------------------------
def fit_batch(n_sel, weighted, scattered, B=3, seed=0):
    """(a (B,M,3), b (B,M,3), weight (B,M) or None, mask (B,M) or None): n_sel counted points per structure; ``scattered``
    puts them among 45 % masked slots that hold NaN; ``weighted`` gives random weights, a fifth of them 0 over NaN
    coordinates (but never all)"""
    rng = np.random.default_rng(1000 * n_sel + 10 * seed + weighted + 2 * scattered)
    a, b, w, m = [], [], [], []
    for s in range(B):
        pa, pb = align_ref.cloud(n_sel, seed=seed + 100 * n_sel + s)
        mask = np.ones(n_sel, dtype=bool)
        if scattered:
            pa, pb, mask = R.scatter(pa, pb, seed=seed + s)
        weight = rng.uniform(0.25, 4.0, pa.shape[0]).astype(np.float32)
        dropped = rng.random(pa.shape[0]) < 0.2
        dropped[np.flatnonzero(mask)[0]] = False
        weight[dropped] = 0.0
        if weighted:
            pa, pb = pa.copy(), pb.copy()
            pa[dropped], pb[dropped] = np.nan, np.nan
        a.append(pa), b.append(pb), w.append(weight), m.append(mask)
    return np.stack(a), np.stack(b), np.stack(w) if weighted else None, np.stack(m) if scattered else None


def assert_fit(got, a, b, w, m, what):
    Rg, tg, rmsd, wsum = (host(t).astype(np.float64) for t in got)
    worst = 0.0
    for s in range(a.shape[0]):
        ref = R.superpose(a[s], b[s if b.shape[0] > 1 else 0], None if w is None else w[s], None if m is None else m[s])
        assert abs(wsum[s] - ref.wsum) <= 2.0 ** -23 * ref.wsum, (what, s)
        err = abs(rmsd[s] - ref.rmsd)
        assert err <= 2.0 ** -23 * ref.rmsd + TAU, f"{what}, structure {s}: rmsd {rmsd[s]!r} for {ref.rmsd!r}"
        worst = max(worst, err / (2.0 ** -23 * ref.rmsd + TAU))
        ortho, det = align_ref.rotation_errors(Rg[s])
        assert ortho <= align_ref.ORTHO_BOUND and det <= align_ref.DET_BOUND, (what, s, ortho, det)
        keep = np.ones(a.shape[1], dtype=bool) if m is None else m[s].copy()
        if w is not None:
            keep &= w[s] > 0
        if keep.sum() >= 4:      # generic clouds of four and more points: the rotation is unique
            assert np.abs(Rg[s] - ref.R).max() <= align_ref.R_TOL, (what, s)
            assert np.abs(tg[s] - ref.t).max() <= 2.0 ** -23 * max(1.0, float(np.abs(ref.t).max())) + 1e-9, (what, s)
    return worst


@pytest.mark.parametrize("n_sel", align_ref.ATOM_COUNTS)
def test_fit_against_the_yardstick(pkg, n_sel):
    ops = pkg.ops
    for weighted in (False, True):
        for scattered in (False, True):
            a, b, w, m = fit_batch(n_sel, weighted, scattered)
            what = f"n = {n_sel}, weights {weighted}, scattered {scattered}"
            worst = assert_fit(ops.superpose(dev(a), dev(b), dev(w), dev(m)), a, b, w, m, what)
            shared = np.nan_to_num(b[:1])       # one target for all: finite wherever any structure counts it
            assert_fit(ops.superpose(dev(a), dev(shared), dev(w), dev(m)), a, shared, w, m, what + ", shared target")
            print(f"{what}: worst rmsd error {worst:.3f} of its bound")


def test_fit_without_a_counted_point_is_nan(pkg):
    a, b = (np.stack(x) for x in zip(*[align_ref.cloud(9, seed=s) for s in range(3)]))
    w = np.ones((3, 9), np.float32)
    m = np.ones((3, 9), bool)
    w[0] = 0.0
    m[1] = False
    a[1], b[1] = np.nan, np.nan
    Rg, tg, rmsd, wsum = (host(t) for t in pkg.ops.superpose(dev(a), dev(b), dev(w), dev(m)))
    for s in (0, 1):
        assert np.isnan(Rg[s]).all() and np.isnan(tg[s]).all() and np.isnan(rmsd[s]) and wsum[s] == 0.0, s
    assert np.isfinite(Rg[2]).all() and np.isfinite(rmsd[2]) and wsum[2] == 9.0


def identical_clouds():
    """name -> (a, b): a = b, and b a rigid motion of a rounded to float32, at several sizes"""
    out = {}
    for n in (1, 2, 3, 4, 50, 257, 1005):
        a, _ = align_ref.cloud(n, seed=60 + n)
        out[f"a = b, n = {n}"] = (a, a.copy())
        rng = np.random.default_rng(61 + n)
        out[f"rigid motion, n = {n}"] = (a, R.f32(a @ align_ref.rotation(rng).T + rng.uniform(-20, 20, 3)))
    return out


def test_tau_on_identical_clouds(pkg):
    """the measurement TAU is made from: every figure printed, the worst held to TAU"""
    worst = 0.0
    for name, (a, b) in identical_clouds().items():
        rmsd = float(host(pkg.ops.superpose(dev(a[None]), dev(b[None]))[2])[0])
        ref = R.superpose(a, b).rmsd
        err = abs(rmsd - ref)
        print(f"{name}: rmsd {rmsd:.3e}, restatement {ref:.3e}, absolute error {err:.3e}")
        worst = max(worst, err)
        assert rmsd <= 5e-6, name        # the rounding of the coordinates, not sqrt(eps)
    print(f"worst {worst:.3e}; TAU = {TAU:.3e}")
    assert worst <= TAU


# ---- K38 -------------------------------------------------------------------------------------------------------------------------
def autograd_reference(a, b, w, m):
    """(grad_a, grad_b) float64 of sum_s g_s rmsd_s by torch-float64 autograd of the SVD Kabsch RMSD, per structure over its
    counted points; zeros elsewhere"""
    ga, gb = np.zeros(a.shape), np.zeros(a.shape)
    for s in range(a.shape[0]):
        keep = np.ones(a.shape[1], dtype=bool) if m is None else m[s].copy()
        weight = np.ones(a.shape[1]) if w is None else w[s].astype(np.float64)
        keep &= weight > 0
        x = torch.from_numpy(a[s][keep]).double().requires_grad_(True)
        y = torch.from_numpy(b[s][keep]).double().requires_grad_(True)
        svd_rmsd(x, y, torch.from_numpy(weight[keep])).backward()
        ga[s][keep], gb[s][keep] = x.grad.numpy(), y.grad.numpy()
    return ga, gb


@pytest.mark.parametrize("n_sel", (8, 64, 65, 257, 1005))
def test_gradient_against_float64_autograd(pkg, n_sel):
    """|grad - ref| <= 2^-22 |ref| + 2^-39 sum|term| + 2^-149 per float, for grad_a and grad_b; exact zeros under the mask
    and at w = 0"""
    ops = pkg.ops
    for weighted, scattered in ((False, False), (True, True)):
        a, b, w, m = fit_batch(n_sel, weighted, scattered, seed=3)
        g = np.array([1.0, -0.5, 2.25], np.float32)
        fit = ops.superpose(dev(a), dev(b), dev(w), dev(m))
        grad_a, grad_b = (host(t).astype(np.float64) for t in ops.superpose_backward(dev(a), dev(b), dev(w), dev(m), *fit, dev(g)))
        want_a, want_b = autograd_reference(a, b, w, m)
        worst = 0.0
        for s in range(3):
            _, _, terms = R.superpose_grad(a[s], b[s], None if w is None else w[s], None if m is None else m[s], float(g[s]))
            for got, want in ((grad_a[s], g[s] * want_a[s]), (grad_b[s], g[s] * want_b[s])):
                bound = 2.0 ** -22 * np.abs(want) + 2.0 ** -39 * terms + 2.0 ** -149
                assert (np.abs(got - want) <= bound).all(), (n_sel, weighted, s, float((np.abs(got - want) / bound).max()))
                worst = max(worst, float((np.abs(got - want) / bound).max()))
                assert (got[terms == 0] == 0).all() and np.isfinite(got).all()
        assert np.abs(grad_a).max() > 1e-4
        print(f"n = {n_sel}, weights {weighted}: worst gradient error {worst:.3f} of its bound")
    shared = ops.superpose_backward(dev(a), dev(np.nan_to_num(b[:1])), dev(w), dev(m),
                                    *ops.superpose(dev(a), dev(np.nan_to_num(b[:1])), dev(w), dev(m)), dev(g))
    assert shared[1] is None and np.isfinite(host(shared[0])).all()


def test_gradient_at_zero_rmsd_is_zero(pkg):
    ops = pkg.ops
    a, b = align_ref.cloud(6, seed=70)
    one = np.zeros((3, 6), bool)
    one[:, 2] = True                                        # one counted point: rmsd = 0 exactly
    fit = ops.superpose(dev(np.stack([a] * 3)), dev(np.stack([b] * 3)), None, dev(one))
    assert (host(fit[2]) == 0).all()
    grads = ops.superpose_backward(dev(np.stack([a] * 3)), dev(np.stack([b] * 3)), None, dev(one), *fit, torch.ones(3, device="cuda"))
    assert all((host(x) == 0).all() for x in grads)
    a3 = np.stack([a, a, a])
    fit = ops.superpose(dev(a3), dev(a3.copy()))            # identical clouds: rmsd at rounding noise, whatever it is nothing is non-finite
    grads = ops.superpose_backward(dev(a3), dev(a3.copy()), None, None, *fit, torch.ones(3, device="cuda"))
    assert all(np.isfinite(host(x)).all() for x in grads) and (host(fit[2]) <= TAU).all()
    nan_fit = [torch.full_like(t, float("nan")) for t in fit]
    grads = ops.superpose_backward(dev(a3), dev(np.stack([b] * 3)), None, None, *nan_fit, torch.ones(3, device="cuda"))
    assert all((host(x) == 0).all() for x in grads)


def test_autograd_reaches_the_dihedrals(pkg):
    """geometry.superposition_rmsd as an autograd function: backward() through the backbone builder to the dihedrals, and
    a central difference in the float32 function agrees with the analytic derivative along a random direction"""
    geometry = pkg.geometry
    B, N = 2, 24
    gen = torch.Generator().manual_seed(5)
    dihedrals = (torch.rand(B, N, 3, generator=gen) * 2 - 1).cuda().requires_grad_(True)
    target = geometry.backbone_from_dihedrals((torch.rand(B, N, 3, generator=gen) * 2 - 1).cuda())[0][:, :, 1].detach()
    xyz, _ = geometry.backbone_from_dihedrals(dihedrals)
    out = geometry.superposition_rmsd(xyz[:, :, 1], target)
    assert out.rmsd.requires_grad and not out.rot.requires_grad and not out.trans.requires_grad
    out.rmsd.sum().backward()
    grad = dihedrals.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 1e-3
    # the points themselves: a central difference of the float32 op along a direction, against grad . direction
    a = (5.0 * torch.randn(B, 40, 3, generator=gen)).cuda().requires_grad_(True)
    b = (a.detach() + torch.randn(B, 40, 3, generator=gen).cuda()).requires_grad_(True)
    weight = torch.rand(B, 40, generator=gen).cuda() + 0.5
    geometry.superposition_rmsd(a, b, weight).rmsd.sum().backward()
    direction = torch.randn(B, 40, 3, generator=gen).cuda()
    h = 1e-2
    with torch.no_grad():
        up = geometry.superposition_rmsd(a + h * direction, b, weight).rmsd.double().sum()
        down = geometry.superposition_rmsd(a - h * direction, b, weight).rmsd.double().sum()
        analytic = float((a.grad.double() * direction.double()).sum())
    assert abs(float(up - down) / (2 * h) - analytic) <= 1e-3 * max(1.0, abs(analytic)), (float(up - down) / (2 * h), analytic)
    assert b.grad is not None and float((a.grad + b.grad @ out_rot(geometry, a, b, weight)).abs().max()) < 1e-5


def out_rot(geometry, a, b, weight):
    """grad_a = -R^T grad_b: (B,M,3) @ (B,3,3) with grad_b as row vectors gives grad_b R"""
    with torch.no_grad():
        return geometry.superposition_rmsd(a, b, weight).rot


# ---- K39 / K40 -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement of a search case, once"""
    a, b, mask, l_norm, obj = all_cases()[name]
    return R.search(a, b, mask, l_norm, obj)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = R.search_cases()
    for name, seed in PDB_CASES:
        cases[name] = pdb_case(name, seed)
    return cases


def run_search(pkg, case):
    a, b, mask, l_norm, obj = case
    out = pkg.ops.superpose_search(dev(a[None]), dev(b[None]), None if mask is None else dev(mask[None]),
                                   torch.tensor([l_norm], device="cuda"), obj)
    return tuple(host(t)[0] for t in out)


def assert_search(got, case, want, what):
    a, b, mask, l_norm, obj = case
    score, Rg, tg = got
    assert score.dtype == np.float32 and score.shape == (len(obj),)
    n = a.shape[0] if mask is None else int(mask.sum())
    if n == 0:
        assert (score == 0).all() and np.isnan(Rg).all() and np.isnan(tg).all(), what
        return
    assert np.abs(score.astype(np.float64) - want.score).max() <= SCORE_TOL, (what, score, want.score)
    for o, (kind, param) in enumerate(obj):
        again = R.score_at(Rg[o], tg[o], a, b, mask, l_norm, kind, param)
        assert abs(again - float(score[o])) <= SCORE_TOL, f"{what}, objective {o}: the returned transform scores {again}, the score is {score[o]}"
        ortho, det = align_ref.rotation_errors(Rg[o])
        assert ortho <= align_ref.ORTHO_BOUND and det <= align_ref.DET_BOUND, (what, o, ortho, det)


@pytest.mark.parametrize("n", R.SEARCH_SIZES)
def test_search_against_the_restatement(pkg, n):
    name = f"n={n}"
    assert_search(run_search(pkg, all_cases()[name]), all_cases()[name], restated(name), name)


def test_search_of_a_batch_is_the_search_of_its_structures(pkg):
    """B = 4 structures of one M with different n: every structure's results are those of its own launch, bit for bit"""
    names = ("contract A0", "contract A1", "contract B0", "contract B1")
    cases = [all_cases()[k] for k in names]
    a, b, mask = (np.stack([c[i] for c in cases]) for i in range(3))
    mask[3, np.flatnonzero(mask[3])[:7]] = False          # 12 points left in the last one
    obj = cases[0][4]
    score, Rg, tg = pkg.ops.superpose_search(dev(a), dev(b), dev(mask), torch.full((4,), 19.0, device="cuda"), obj)
    for s in range(4):
        case = (a[s], b[s], mask[s], 19.0, obj)
        alone = run_search(pkg, case)
        assert all(np.array_equal(host(x)[s].view(np.int32), y.view(np.int32)) for x, y in zip((score, Rg, tg), alone)), s
        if s < 3:
            assert_search(alone, case, restated(names[s]), names[s])


def test_the_search_searches(pkg):
    """Two domains, 40 degrees apart: the TM-score reaches the first domain's own fit and the 1 A fraction is the first
    domain, both strictly above what the all-points fit gives"""
    case = all_cases()["two domains"]
    a, b, _, l_norm, obj = case
    score = run_search(pkg, case)[0].astype(np.float64)
    assert_search(run_search(pkg, case), case, restated("two domains"), "two domains")
    A, Bt = align_ref.f64(a), align_ref.f64(b)
    R1, t1 = R.fit(A[:78], Bt[:78])
    domain = float((1.0 / (1.0 + R.dist2(R1, t1, A[:78], Bt[:78]) / obj[0][1] ** 2)).sum() / 130.0)
    Rall, tall = R.fit(A, Bt)
    tm_all, one_all = (R.score_at(Rall, tall, a, b, None, l_norm, *obj[o]) for o in (0, 2))
    assert score[0] >= domain - SCORE_TOL and score[2] >= 78 / 130 - SCORE_TOL
    assert score[0] > tm_all and score[2] > one_all
    for name, case in all_cases().items():
        if name.startswith("n=") and name not in ("n=0", "n=257"):
            a, b, mask, l_norm, obj = case
            Rall, tall = R.fit(align_ref.f64(a)[mask], align_ref.f64(b)[mask])
            got = run_search(pkg, case)[0]
            assert got[0] >= R.score_at(Rall, tall, a, b, mask, l_norm, *obj[0]) - SCORE_TOL, name


def test_edges(pkg):
    geometry, ops = pkg.geometry, pkg.ops
    a, b, _, l_norm, obj = all_cases()["identical"]
    score = run_search(pkg, all_cases()["identical"])[0]
    assert (score == np.float32(1.0)).all(), score
    scores = geometry.superposition_scores(dev(a[None]), dev(b[None]))
    assert float(scores.tm) == 1.0 and float(scores.gdt_ts) == 1.0 and float(scores.gdt_ha) == 1.0
    assert float(geometry.superposition_rmsd(dev(a[None]), dev(b[None])).rmsd) <= TAU
    # an explicit l_norm above n scales the score
    case = all_cases()["l_norm above n"]
    got = run_search(pkg, case)
    assert_search(got, case, restated("l_norm above n"), "l_norm above n")
    own = run_search(pkg, (*case[:3], 65.0, case[4]))[0].astype(np.float64)
    assert np.abs(got[0] - own * 0.65).max() <= 2e-7 and got[0][5] < 0.66
    # the largest M, once
    case = all_cases()["M=2048"]
    assert case[0].shape[0] == ops.SUPERPOSE_MAX_POINTS
    assert_search(run_search(pkg, case), case, restated("M=2048"), "M = 2048")
    with pytest.raises(ValueError, match="points per structure"):
        ops.superpose_search(torch.zeros(1, 2049, 3, device="cuda"), torch.zeros(1, 2049, 3, device="cuda"), None,
                             torch.ones(1, device="cuda"), obj)


def test_geometry_functions_agree_with_one_search(pkg):
    geometry = pkg.geometry
    names = ("n=63", "n=64")
    M = 120
    a, b, mask = (np.zeros((2, M, 3), np.float32), np.zeros((2, M, 3), np.float32), np.zeros((2, M), bool))
    for s, name in enumerate(names):
        ca, cb, cm = all_cases()[name][:3]
        a[s, :ca.shape[0]], b[s, :ca.shape[0]], mask[s, :ca.shape[0]] = ca, cb, cm
    a[~mask], b[~mask] = np.nan, np.nan
    A, Bt, Mk = dev(a), dev(b), dev(mask)
    scores = geometry.superposition_scores(A, Bt, Mk)               # l_norm 63 and 64: two d0, two launches behind one call
    tm = geometry.tm_score(A, Bt, Mk)
    assert same(tm.score, scores.tm) and same(geometry.gdt_ts(A, Bt, Mk), scores.gdt_ts) and same(geometry.gdt_ha(A, Bt, Mk), scores.gdt_ha)
    for s, name in enumerate(names):
        want = restated(name).score
        assert abs(float(scores.tm[s]) - want[0]) <= SCORE_TOL and abs(float(scores.gdt_ts[s]) - want[2:6].mean()) <= SCORE_TOL
        assert abs(float(scores.gdt_ha[s]) - want[1:5].mean()) <= SCORE_TOL
        case = all_cases()[name]
        again = R.score_at(host(tm.rot)[s], host(tm.trans)[s], a[s], b[s], mask[s], case[3], *case[4][0])
        assert abs(again - float(tm.score[s])) <= SCORE_TOL
    fixed = geometry.tm_score(A, Bt, Mk, l_norm=100.0, d0=3.0)
    for s in range(2):
        want = R.search(a[s], b[s], mask[s], 100.0, [(R.TM, 3.0)]).score[0]
        assert abs(float(fixed.score[s]) - want) <= SCORE_TOL


# ---- alignment and sentinels ---------------------------------------------------------------------------------------------------
def intact(buf, start, n_bytes):
    return bool((buf[:start] == SENTINEL).all()) and bool((buf[start + n_bytes:] == SENTINEL).all())


def carved(t, off, dtype=torch.float32):
    """a copy of tensor ``t`` ``off`` bytes past a 16-byte boundary"""
    _, view, _ = carve(t.numel() * t.element_size(), off, dtype)
    view.copy_(t.reshape(-1).view(dtype) if t.dtype != dtype else t.reshape(-1))
    return view


@pytest.mark.parametrize("off,mask_off", ((4, 1), (8, 6), (12, 15), (0, 0)))
def test_sentinels_and_alignment(pkg, off, mask_off):
    """every tensor ``off`` bytes past a 16-byte boundary (the mask ``mask_off``), the outputs and the workspace inside
    sentinels: the results of the aligned run through ``ops``, bit for bit, and no sentinel byte changes"""
    from protstruc_amd import _lib
    lib, ops = _lib.load(), pkg.ops
    stream = torch.cuda.current_stream().cuda_stream
    B = 2
    a, b, w, m = fit_batch(63, True, True, B=B, seed=9)
    M = a.shape[1]
    A, Bt, W, Mk = dev(a), dev(b), dev(w), dev(m)
    want = ops.superpose(A, Bt, W, Mk)
    am, bm, wm, mm = carved(A, off), carved(Bt, off), carved(W, off), carved(Mk, mask_off, torch.bool)
    outs = [carve(n * 4, off, torch.float32) for n in (B * 9, B * 3, B, B)]
    assert lib.ps_superpose_f32(am.data_ptr(), bm.data_ptr(), wm.data_ptr(), mm.data_ptr(), *[o[1].data_ptr() for o in outs], B, M, 0,
                                stream) == 0
    torch.cuda.synchronize()
    for (buf, view, start), w_, n in zip(outs, want, (B * 9, B * 3, B, B)):
        assert same(view.reshape(w_.shape), w_) and intact(buf, start, n * 4)
    g = torch.tensor([1.0, -2.0], device="cuda")
    want_grads = ops.superpose_backward(A, Bt, W, Mk, *want, g)
    grads = [carve(B * M * 12, off, torch.float32) for _ in range(2)]
    assert lib.ps_superpose_backward_f32(am.data_ptr(), bm.data_ptr(), wm.data_ptr(), mm.data_ptr(), *[o[1].data_ptr() for o in outs],
                                         carved(g, off).data_ptr(), grads[0][1].data_ptr(), grads[1][1].data_ptr(), B, M, 0, stream) == 0
    torch.cuda.synchronize()
    for (buf, view, start), w_ in zip(grads, want_grads):
        assert same(view.reshape(B, M, 3), w_) and intact(buf, start, B * M * 12)
    # the search
    obj = R.six_objectives(63.0)
    l_norm = torch.full((B,), 63.0, device="cuda")
    want = ops.superpose_search(A, Bt, Mk, l_norm, obj)
    table = (_lib.SuperposeObjective * 6)(*[_lib.SuperposeObjective(k, p) for k, p in obj])
    floats = lib.ps_superpose_workspace_floats(B, M, 6)
    ws = carve(floats * 4, off, torch.float32)
    outs = [carve(n * 4, off, torch.float32) for n in (B * 6, B * 6 * 9, B * 6 * 3)]
    assert lib.ps_superpose_search_f32(am.data_ptr(), bm.data_ptr(), mm.data_ptr(), carved(l_norm, off).data_ptr(), table, 6,
                                       ws[1].data_ptr(), *[o[1].data_ptr() for o in outs], B, M, stream) == 0
    torch.cuda.synchronize()
    for (buf, view, start), w_, n in zip(outs, want, (B * 6, B * 6 * 9, B * 6 * 3)):
        assert same(view.reshape(w_.shape), w_) and intact(buf, start, n * 4)
    assert intact(ws[0], ws[2], floats * 4)


# ---- repeatability -------------------------------------------------------------------------------------------------------------
def test_repeatability(pkg):
    ops = pkg.ops
    a, b, w, m = fit_batch(257, True, True, seed=11)
    A, Bt, W, Mk = dev(a), dev(b), dev(w), dev(m)
    g = torch.tensor([1.0, 2.0, 3.0], device="cuda")
    l_norm = torch.full((3,), 257.0, device="cuda")
    obj = R.six_objectives(257.0)
    fit = ops.superpose(A, Bt, W, Mk)
    grads = ops.superpose_backward(A, Bt, W, Mk, *fit, g)
    found = ops.superpose_search(A, Bt, Mk, l_norm, obj)
    for _ in range(2):
        assert_all_same(ops.superpose(A, Bt, W, Mk), fit, "superpose")
        assert_all_same(ops.superpose_backward(A, Bt, W, Mk, *fit, g), grads, "superpose_backward")
        assert_all_same(ops.superpose_search(A, Bt, Mk, l_norm, obj), found, "superpose_search")


# ---- StructureBatch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", PDB_CASES)
def test_structure_batch_methods(pkg, name, seed):
    from protstruc_amd import StructureBatch
    target = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, name + ".pdb"))
    xyz, atom_mask = host(target.get_xyz())[0], host(target.get_atom_mask())[0]
    model_xyz, model_mask = R.perturbed_model(xyz, atom_mask, seed)
    model = StructureBatch(torch.from_numpy(model_xyz[None]), torch.from_numpy(model_mask[None]), target.chain_idx, target.get_chain_ids())
    case = all_cases()[name]
    a, b, mask, l_norm, obj = case
    assert l_norm == atom_mask[:, 1].sum() and mask.sum() == round(0.9 * l_norm) and np.array_equal(a[mask], model_xyz[:, 1][mask])
    want = restated(name)
    scores = model.superposition_scores(target)
    tm = model.tm_score(target)
    assert abs(float(scores.tm) - want.score[0]) <= SCORE_TOL and same(tm.score, scores.tm)
    assert abs(float(scores.gdt_ts) - want.score[2:6].mean()) <= SCORE_TOL and same(model.gdt_ts(target), scores.gdt_ts)
    assert abs(float(scores.gdt_ha) - want.score[1:5].mean()) <= SCORE_TOL and same(model.gdt_ha(target), scores.gdt_ha)
    assert float(scores.tm) < 0.9 * 1.0 + 1e-6, "a tenth of the CA atoms is missing from the model: the target's length normalises"
    again = R.score_at(host(tm.rot)[0], host(tm.trans)[0], a, b, mask, l_norm, *obj[0])
    assert abs(again - float(tm.score)) <= SCORE_TOL
    # the RMSD: superimposed against the yardstick, as it lies against plain numpy
    fit = model.rmsd(target)
    ref = R.superpose(a, b, None, mask)
    assert abs(float(fit.rmsd) - ref.rmsd) <= 2.0 ** -23 * ref.rmsd + TAU and np.abs(host(fit.rot)[0] - ref.R).max() <= align_ref.R_TOL
    diff = a[mask].astype(np.float64) - b[mask].astype(np.float64)
    plain = np.sqrt((diff ** 2).sum(-1).mean())
    assert abs(float(model.rmsd(target, superimpose=False)) - plain) <= 2.0 ** -22 * plain
    backbone = model.rmsd(target, atoms=("N", "CA", "C"))
    keep = (model_mask & atom_mask)[:, :3]
    ref = R.superpose(model_xyz[:, :3].reshape(-1, 3), xyz[:, :3].reshape(-1, 3), None, keep.reshape(-1))
    assert abs(float(backbone.rmsd) - ref.rmsd) <= 2.0 ** -23 * ref.rmsd + TAU


# ---- the launch contract -------------------------------------------------------------------------------------------------------
# Two seeded variants that differ in every output; float64 strided points and a float mask, so that the shell's conversions
# are on the launch path that is checked (as the cases of tests/launch_cases.py).
CONTRACT_OBJECTIVES = tuple(R.six_objectives(19.0))


def _contract_inputs(v):
    cases = [R.contract_case(v, s) for s in (0, 1)]
    a, b, mask = (np.stack([c[i] for c in cases]) for i in range(3))
    rng = np.random.default_rng(60 + "AB".index(v))
    t = torch.from_numpy
    return dict(a=t(np.nan_to_num(a)).double(), b=t(np.nan_to_num(b)), weight=t(rng.uniform(0.5, 2.0, mask.shape).astype(np.float32)),
                mask=t(mask).float(), grad_rmsd=t(rng.normal(size=2).astype(np.float32)), l_norm=torch.full((2,), 19.0))


def _ops():
    from protstruc_amd import ops
    return ops


def _run_backward(i):
    fit = _ops().superpose(i["a"], i["b"], i["weight"], i["mask"])
    return _ops().superpose_backward(i["a"], i["b"], i["weight"], i["mask"], *fit, i["grad_rmsd"])


CONTRACT = (
    Case("superpose", ("ps_superpose_f32",), _contract_inputs,
         lambda i: _ops().superpose(i["a"], i["b"], i["weight"], i["mask"]), strided=("a",)),
    Case("superpose_backward", ("ps_superpose_backward_f32",), _contract_inputs, _run_backward, strided=("a",)),
    Case("superpose_search", ("ps_superpose_search_f32",), _contract_inputs,
         lambda i: _ops().superpose_search(i["a"], i["b"], i["mask"], i["l_norm"], CONTRACT_OBJECTIVES), strided=("a",)),
)
BY_NAME = {case.name: case for case in CONTRACT}
NAMES = list(BY_NAME)
HOST_FUNCTIONS = {"ps_superpose_api", "ps_superpose_seed", "ps_superpose_seed_count", "ps_superpose_workspace_floats"}


@functools.lru_cache(maxsize=None)
def inputs(name, variant):
    return on_device(BY_NAME[name], variant)


@functools.lru_cache(maxsize=None)
def eager(name, variant):
    """the case run eagerly on the default stream, once: the reference of every contract test (never modified)"""
    outs = tuple(BY_NAME[name].run(inputs(name, variant)))
    torch.cuda.synchronize()
    return outs


def assert_variants_differ(name):
    for k, (a, b) in enumerate(zip(eager(name, "A"), eager(name, "B"))):
        if name == "superpose_search" and k == 0:
            continue      # the scores are fractions of 19: some objectives may tie between the variants; R and t tell them apart
        assert a.shape == b.shape and a.dtype == b.dtype and not same(a, b), (name, k)


def test_contract_cases_cover_the_header_and_meet_the_yardstick(pkg):
    from protstruc_amd import _lib
    assert sorted(s for case in CONTRACT for s in case.symbols) == sorted(set(_lib.SUPERPOSE_SIGNATURES) - HOST_FUNCTIONS)
    for name in NAMES:
        assert_variants_differ(name)
    for v in "AB":
        i = {k: t.numpy() for k, t in _contract_inputs(v).items()}
        a32 = i["a"].astype(np.float32)
        assert_fit(eager("superpose", v), a32, i["b"], i["weight"], i["mask"] != 0, f"contract {v}")
        score, Rg, tg = (host(t) for t in eager("superpose_search", v))
        for s in (0, 1):
            case = R.contract_case(v, s)
            assert_search((score[s], Rg[s], tg[s]), case, restated(f"contract {v}{s}"), f"contract {v}{s}")


@pytest.mark.parametrize("name", NAMES)
def test_launches_on_the_callers_stream(pkg, name):
    """As tests/test_gpu_launch_contract.py: on a side stream, a sleep, the copies of variant B over variant A, the op; a
    clone on the default stream meanwhile still sees variant A."""
    case = BY_NAME[name]
    assert_variants_differ(name)
    want_a, want_b = eager(name, "A"), eager(name, "B")
    a, b = inputs(name, "A"), inputs(name, "B")
    live = on_device(case, "A")
    first = next(iter(live))
    side = side_stream_beside_the_default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        for k in live:
            live[k].copy_(b[k])
    control = live[first].clone()                           # the default stream: runs while the side stream sleeps
    with torch.cuda.stream(side):
        outs = tuple(case.run(live))
    torch.cuda.synchronize()
    if not same(control, a[first]):
        pytest.fail(f"{name}: inconclusive -- the control clone did not see variant A")
    assert_all_same(outs, want_b, f"{name} on a side stream")
    assert any(not same(o, w) for o, w in zip(outs, want_a)), f"{name}: computed from the inputs as they were before the side stream's copies"


@pytest.mark.parametrize("name", NAMES)
def test_inside_a_captured_graph(pkg, name):
    """captured on variant A after one eager call, replayed twice on variant B over overwritten outputs"""
    case = BY_NAME[name]
    assert_variants_differ(name)
    want_b, b = eager(name, "B"), inputs(name, "B")
    live = on_device(case, "A")
    case.run(live)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = tuple(case.run(live))
    torch.cuda.synchronize()
    for k in live:
        live[k].copy_(b[k])
    for replay in range(2):
        for o in outs:
            raw(o).fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert_all_same(outs, want_b, f"{name}, replay {replay + 1}")


def test_four_threads_on_four_streams(pkg):
    rounds, n_threads = 3, 4
    want = {(name, v): eager(name, v) for name in NAMES for v in "AB"}
    mine = [{name: on_device(BY_NAME[name], "AB"[t % 2]) for name in NAMES} for t in range(n_threads)]
    streams = [torch.cuda.Stream() for _ in range(n_threads)]
    torch.cuda.synchronize()
    gate = threading.Barrier(n_threads)
    failures = []

    def work(t):
        try:
            variant = "AB"[t % 2]
            order = NAMES[t % len(NAMES):] + NAMES[:t % len(NAMES)]
            gate.wait(timeout=60)
            with torch.cuda.stream(streams[t]):
                for r in range(rounds):
                    results = [(name, tuple(BY_NAME[name].run(mine[t][name]))) for name in order]
                    streams[t].synchronize()
                    for name, outs in results:
                        for k, (o, w) in enumerate(zip(outs, want[name, variant])):
                            if not same(o, w):
                                failures.append(f"thread {t}, round {r}, {name}: output {k} differs from the serial result")
        except Exception as exc:  # noqa: BLE001 -- reported by the main thread
            failures.append(f"thread {t}: {type(exc).__name__}: {exc}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not failures, failures[:10]


def test_batch_limit(pkg):
    """B = 65535 at M = 5 (the search) and M = 4 (the fit and its gradient): structure b is structure b % 3, and the results
    are those of the three, bit for bit"""
    ops = pkg.ops
    cases = [R.batch_limit_case(s) for s in range(3)]
    a, b, mask = (np.stack([c[i] for c in cases]) for i in range(3))
    obj = cases[0][4]
    tensors = dict(a=dev(a), b=dev(b), mask=dev(mask), l_norm=torch.full((3,), 5.0, device="cuda"))
    run = functools.partial(ops.superpose_search, objectives=obj)
    small = run(**tensors)
    for s in range(3):
        assert_search(tuple(host(t)[s] for t in small), cases[s], restated(f"batch limit {s}"), f"batch limit {s}")
    assert_batch_of_65535_repeats_the_three(run, tensors, small, "superpose_search")
    a, b, w, m = fit_batch(4, True, False, seed=13)
    tensors = dict(a=dev(a), b=dev(b), weight=dev(w))
    small = ops.superpose(**tensors)
    assert_fit(small, a, b, w, None, "M = 4")
    assert_batch_of_65535_repeats_the_three(ops.superpose, tensors, small, "superpose")

    def backward(a, b, weight, grad_rmsd):
        return ops.superpose_backward(a, b, weight, None, *ops.superpose(a, b, weight), grad_rmsd)

    tensors["grad_rmsd"] = torch.tensor([1.0, -1.5, 0.5], device="cuda")
    assert_batch_of_65535_repeats_the_three(backward, tensors, backward(**tensors), "superpose_backward")
