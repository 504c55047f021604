"""The pair heads without a GPU: the C header include/protstruc_pairhead.h against the binding and the library, the argument
checks of the four launchers and of the shell, and the yardstick tests/pairhead_ref.py itself -- its bins against torch
float64, its cross-entropy and gradient against torch's, its pTM against a line-by-line restatement of the formula."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import pairhead_ref as R
from tests.c_headers import declared_symbols

LAUNCHERS = ["ps_binned_cross_entropy_backward_f32", "ps_binned_cross_entropy_f32", "ps_binned_expectation_f32",
             "ps_pair_bins_f32"]


# ---- the header (tests/test_api_families.py holds it to the binding and the library) ------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from protstruc_amd import _lib, build
    build.build(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_the_entry_points_of_the_header():
    from protstruc_amd import build, ops
    assert declared_symbols("protstruc_pairhead.h") == sorted(LAUNCHERS + ["ps_pairhead_api"])
    assert "pair_head.hip" in {os.path.basename(d) for d in build._deps()}
    assert R.NO_TARGET == ops.PAIRHEAD_NO_TARGET


def floats(*values):
    return (ctypes.c_float * len(values))(*values)


def test_arguments_are_checked_before_any_launch(lib):
    """hipErrorInvalidValue (1) without touching a device; B = 0 returns 0 (the device pointers are never dereferenced)."""
    fake = ctypes.c_void_p(0x1000)
    good = floats(2.0, 4.0, 8.0)

    def bins(mode=0, points=fake, frames=fake, breaks=good, n_breaks=3, out=fake, B=1, N=4):
        return lib.ps_pair_bins_f32(mode, points, frames, frames, frames, frames, frames, None, None, breaks, n_breaks, out, None,
                                    B, N, None)

    def ce(logits=fake, labels=fake, loss=fake, count=fake, B=1, N=4, C=64):
        return lib.ps_binned_cross_entropy_f32(logits, labels, loss, count, B, N, C, None)

    def back(logits=fake, labels=fake, grad_row=fake, out=fake, B=1, N=4, C=64):
        return lib.ps_binned_cross_entropy_backward_f32(logits, labels, grad_row, out, B, N, C, None)

    def expect(logits=fake, values=fake, out=fake, B=1, N=4, C=64, V=1):
        return lib.ps_binned_expectation_f32(logits, values, out, B, N, C, V, None)

    assert bins(B=0) == 0 and bins(mode=1, B=0) == 0 and ce(B=0) == 0 and back(B=0) == 0 and expect(B=0) == 0
    for bad in (dict(points=None), dict(out=None), dict(breaks=None), dict(mode=1, frames=None), dict(mode=2), dict(mode=-1),
                dict(n_breaks=0), dict(breaks=floats(*range(1, 129)), n_breaks=128), dict(breaks=floats(2.0, 8.0, 4.0)),
                dict(breaks=floats(2.0, 2.0, 4.0)), dict(breaks=floats(-1.0, 2.0, 4.0)), dict(breaks=floats(1.0, math.nan, 4.0)),
                dict(breaks=floats(1.0, 2.0, math.inf)), dict(B=65536), dict(B=-1), dict(N=0), dict(N=2 ** 20 + 1),
                dict(B=0, n_breaks=0), dict(B=0, mode=2)):
        assert bins(**bad) == 1, bad
    assert bins(breaks=floats(*range(127)), n_breaks=127, B=0) == 0 and bins(breaks=floats(0.0), n_breaks=1, B=0) == 0
    for call in (ce, back, expect):
        for bad in (dict(logits=None), dict(C=1), dict(C=129), dict(B=65536), dict(B=-1), dict(N=0), dict(B=0, C=1)):
            assert call(**bad) == 1, (call.__name__, bad)
    for bad in (dict(labels=None), dict(loss=None), dict(count=None)):
        assert ce(**bad) == 1, bad
    for bad in (dict(labels=None), dict(grad_row=None), dict(out=None)):
        assert back(**bad) == 1, bad
    for bad in (dict(values=None), dict(out=None), dict(V=0), dict(V=5), dict(B=0, V=5)):
        assert expect(**bad) == 1, bad


def test_shape_checks_of_the_shell():
    from protstruc_amd import ops
    B, N, C = 2, 5, 8
    points, mask = torch.zeros(B, N, 3), torch.ones(B, N, dtype=torch.bool)
    rot, breaks = torch.zeros(B, N, 3, 3), [1.0, 2.0, 3.0]
    check = ops.check_pair_bins_shapes
    check(points, breaks, mask, mask.float())
    check(points.double(), torch.tensor(breaks), None, None, rot, points, rot.double(), points, points)
    base = dict(points=points, breaks=breaks, row_mask=mask, col_mask=mask)
    for bad, message in ((dict(points=torch.zeros(B, N)), "points must have shape"), (dict(points=torch.zeros(B, N, 2)), "points must have shape"),
                         (dict(points=torch.zeros(B, N, 3, dtype=torch.int32)), "floating-point"),
                         (dict(points=torch.zeros(B, 0, 3), row_mask=None, col_mask=None), "residues per structure"),
                         (dict(row_mask=mask[:, :4]), "row_mask must have shape"), (dict(col_mask=mask[:1]), "col_mask must have shape"),
                         (dict(breaks=[]), "breaks, got 0"), (dict(breaks=list(range(128))), "breaks, got 128"),
                         (dict(breaks=[1.0, 1.0]), "strictly increasing"), (dict(breaks=[-1.0, 1.0]), "strictly increasing"),
                         (dict(breaks=[1.0, math.nan]), "strictly increasing"), (dict(breaks=[[1.0, 2.0]]), "one-dimensional"),
                         (dict(rot=rot[:, :4], trans=points, target_rot=rot, target_trans=points, target_points=points), "rot must have shape"),
                         (dict(rot=rot, trans=points[:, :4], target_rot=rot, target_trans=points, target_points=points), "trans must have shape"),
                         (dict(rot=rot, trans=points, target_rot=rot, target_trans=points, target_points=points.long()), "floating-point")):
        with pytest.raises(ValueError, match=message):
            check(**{**base, **bad})
    logits, labels = torch.zeros(B, N, N, C), torch.zeros(B, N, N, dtype=torch.uint8)
    check = ops.check_binned_shapes
    check(logits, labels, torch.zeros(B, N), torch.zeros(B, 4, C))
    check(logits.double(), labels.long(), torch.zeros(B, N).double(), torch.zeros(B, 1, C).double())
    for bad, message in ((dict(logits=torch.zeros(B, N, C)), "logits must have shape"), (dict(logits=torch.zeros(B, N, 4, C)), "logits must have shape"),
                         (dict(logits=torch.zeros(B, N, N, C, dtype=torch.int64)), "floating-point"),
                         (dict(logits=torch.zeros(B, N, N, 1)), "bins, got 1"), (dict(logits=torch.zeros(B, N, N, 129)), "bins, got 129"),
                         (dict(bins=labels[:, :4]), "bins must have shape"), (dict(bins=labels.float()), "integer tensor"),
                         (dict(grad_row=torch.zeros(B, N, 1)), "grad_row must have shape"), (dict(grad_row=torch.zeros(B, N).long()), "floating-point"),
                         (dict(values=torch.zeros(B, C)), "values must have shape"), (dict(values=torch.zeros(B, 1, C + 1)), "values must have shape"),
                         (dict(values=torch.zeros(B, 0, C)), "value tables, got 0"), (dict(values=torch.zeros(B, 5, C)), "value tables, got 5"),
                         (dict(values=torch.zeros(B, 1, C).long()), "floating-point")):
        with pytest.raises(ValueError, match=message):
            check(**{**dict(logits=logits), **bad})
    for call in (lambda: ops.pair_bins_distance(points, breaks), lambda: ops.pair_bins_aligned_error(rot, points, points, rot, points, points, breaks),
                 lambda: ops.binned_cross_entropy(logits, labels), lambda: ops.binned_cross_entropy_backward(logits, labels, torch.zeros(B, N)),
                 lambda: ops.binned_expectation(logits, torch.zeros(B, 1, C))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_breaks_and_centres_of_the_shell_are_the_yardsticks():
    from protstruc_amd import geometry
    for n_bins in (64, 37, 3):
        assert np.array_equal(geometry.distogram_breaks(n_bins=n_bins).numpy(), R.distogram_breaks(n_bins=n_bins))
        assert np.array_equal(geometry.aligned_error_breaks(n_bins=n_bins).numpy(), R.aligned_error_breaks(n_bins=n_bins))
        assert np.array_equal(geometry.aligned_error_bin_centers(25.0, n_bins).numpy(), R.aligned_error_bin_centers(25.0, n_bins))
    breaks, centers = geometry.distogram_breaks().numpy(), geometry.aligned_error_bin_centers().numpy()
    assert breaks.dtype == np.float32 and breaks.shape == (63,) and breaks[0] == 2.3125 and breaks[-1] == 21.6875
    assert centers.shape == (64,) and centers[0] == 0.25 and centers[-1] == 31.75 and np.allclose(np.diff(centers), 0.5)
    with pytest.raises(ValueError, match="bins"):
        geometry.distogram_breaks(n_bins=1)
    with pytest.raises(ValueError, match="bins"):
        geometry.aligned_error_breaks(n_bins=129)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def test_yardstick_bins_against_torch_float64():
    B, N = 2, 23
    bb = R.backbone_case(B, N, seed=1)
    points = bb[:, :, 1].copy()
    row, col = R.masks(B, N, seed=2)
    points[~(row | col)] = np.nan
    breaks = R.distogram_breaks()
    bins, value = R.bins_distance(points, breaks, row, col)
    x = torch.from_numpy(np.nan_to_num(points)).double()
    d = x[:, None, :, :] - x[:, :, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    want = (d2[..., None] > torch.from_numpy(breaks).double() ** 2).sum(-1)
    ok = torch.from_numpy(row[:, :, None] & col[:, None, :])
    assert np.array_equal(bins, torch.where(ok, want, torch.full_like(want, 255)).numpy().astype(np.uint8))
    assert np.array_equal(value.view(np.int32), torch.where(ok, d2.sqrt(), torch.full_like(d2, math.inf)).float().numpy().view(np.int32))
    assert len(np.unique(bins)) > 20 and (bins == 255).mean() > 0.3 and np.isinf(value[bins == 255]).all()
    # the aligned error against einsum, to rounding: the stated order differs from einsum's in the last bits only
    rot = np.linalg.qr(np.random.default_rng(3).normal(size=(B, N, 3, 3)))[0].astype(np.float32)
    trot = np.linalg.qr(np.random.default_rng(4).normal(size=(B, N, 3, 3)))[0].astype(np.float32)
    target = (np.nan_to_num(points) + np.random.default_rng(5).normal(size=points.shape)).astype(np.float32)
    clean = np.nan_to_num(points)
    v2 = R.aligned_v2(rot, clean, clean, trot, target, target)
    local = np.einsum("bikc,bijk->bijc", rot.astype(np.float64), clean[:, None, :, :].astype(np.float64) - clean[:, :, None, :])
    tlocal = np.einsum("bikc,bijk->bijc", trot.astype(np.float64), target[:, None, :, :].astype(np.float64) - target[:, :, None, :])
    assert np.allclose(v2, ((local - tlocal) ** 2).sum(-1), rtol=1e-12, atol=1e-12) and v2.max() > 1.0
    assert (v2[:, np.arange(N), np.arange(N)] == 0).all(), "a frame sees its own origin at the origin in both structures"
    bins, value = R.bins_aligned_error(rot, clean, clean, trot, target, target, R.aligned_error_breaks(), row, col)
    assert np.array_equal(bins == 255, ~ok.numpy()) and np.array_equal(bins[ok.numpy()], (v2[..., None] > R.sq_breaks(R.aligned_error_breaks())).sum(-1)[ok.numpy()])


def test_yardstick_lattice_sits_on_the_breaks():
    points = R.lattice_points(1, 40, seed=6)
    breaks = np.arange(1, 12, dtype=np.float32)
    v2 = R.distance_v2(points)
    on_a_break = np.isin(v2, R.sq_breaks(breaks))
    assert on_a_break.sum() >= 20
    bins, value = R.bins_distance(points, breaks)
    assert np.array_equal(bins[on_a_break], np.sqrt(v2[on_a_break]).astype(np.uint8) - 1), "a distance equal to a break is not beyond it"
    rot, trans = R.lattice_frames(1, 40, seed=7)
    trot, ttrans = R.lattice_frames(1, 40, seed=8)
    v2 = R.aligned_v2(rot, trans, points, trot, ttrans, R.lattice_points(1, 40, seed=9))
    assert (v2 == np.round(v2)).all() and np.isin(v2, R.sq_breaks(np.arange(1, 30, dtype=np.float32))).sum() >= 20


@pytest.mark.parametrize("family", R.LOGIT_FAMILIES)
def test_yardstick_cross_entropy_against_torch(family):
    import torch.nn.functional as F
    B, N, C = 2, 7, 37
    x, bins = R.logits_case(family, B, N, C, seed=11)
    ref = R.CrossEntropy(x, bins)
    g = np.random.default_rng(12).normal(size=(B, N)).astype(np.float32)
    logits = torch.from_numpy(np.nan_to_num(x, nan=0.0, neginf=-np.inf)).double().requires_grad_(True)
    labels = torch.from_numpy(np.where(bins < C, bins.astype(np.int64), -100))
    ce = F.cross_entropy(logits.reshape(-1, C), labels.reshape(-1), ignore_index=-100, reduction="none").reshape(B, N, N)
    scale = max(1.0, float(np.abs(ref.ce).max()))
    assert np.abs(ce.detach().numpy() - ref.ce).max() <= 1e-12 * scale
    assert np.abs(ce.sum(-1).detach().numpy() - ref.row_loss).max() <= 1e-12 * scale * N
    assert np.array_equal(ref.row_count, (bins < C).sum(-1)) and (bins == 255).any()
    (ce.sum(-1) * torch.from_numpy(g).double()).sum().backward()
    grad = ref.backward(g)
    assert np.abs(logits.grad.numpy() - grad).max() <= 1e-12 * max(1.0, float(np.abs(g).max()))
    assert (grad[bins == 255] == 0).all() and np.isfinite(grad).all() and np.isfinite(ref.row_loss).all()
    assert (ref.row_bound() > 0).all() and (ref.pair_bound()[bins == 255] == 0).all()


def test_yardstick_expectations_and_ptm():
    B, N, C = 2, 11, 64
    x, _ = R.logits_case("normal", B, N, C, seed=13)
    x = (3.0 * x).astype(np.float32)
    values = np.random.default_rng(14).normal(size=(B, 3, C)).astype(np.float32)
    p = torch.softmax(torch.from_numpy(x).double(), dim=-1)
    assert np.abs(R.expectation(x, values) - torch.einsum("bijk,bvk->vbij", p, torch.from_numpy(values).double()).numpy()).max() <= 1e-12
    assert np.abs(R.predicted_aligned_error(x) - (p * torch.from_numpy(R.aligned_error_bin_centers())).sum(-1).numpy()).max() <= 1e-11
    contact = R.contact_probability(x, 8.0)
    edges = R.distogram_breaks()
    assert np.abs(contact - p[..., :C - 1][..., edges <= 8.0].sum(-1).numpy()).max() <= 1e-12 and 0 < contact.min() < contact.max() < 1
    assert (edges <= 8.0).sum() == 19 and np.abs(R.contact_probability(x, 100.0) - (1 - p[..., -1].numpy())).max() <= 1e-12
    # pTM, line by line: two chains, the second structure with padding
    mask = np.ones((B, N), dtype=bool)
    mask[1, 8:] = False
    chain = np.array([[0] * 5 + [1] * 6, [0] * 4 + [1] * 4 + [-1] * 3])
    centers = R.aligned_error_bin_centers()
    for interface in (False, True):
        got = R.predicted_tm_score(x, mask, chain, interface)
        for b in range(B):
            n = int(mask[b].sum())
            d0 = 1.24 * (max(n, 19) - 15) ** (1.0 / 3) - 1.8
            best = 0.0
            for i in range(N):
                if not mask[b, i]:
                    continue
                total, weight = 0.0, 0.0
                for j in range(N):
                    if not mask[b, j] or (interface and chain[b, i] == chain[b, j]):
                        continue
                    total += sum(float(p[b, i, j, k]) / (1.0 + (centers[k] / d0) ** 2) for k in range(C))
                    weight += 1.0
                best = max(best, total / (1e-8 + weight))
            assert abs(got[b] - best) <= 1e-12 and 0.0 < got[b] < 1.0, (interface, b)
    assert (R.predicted_tm_score(x, mask, chain, True) != R.predicted_tm_score(x, mask, chain, False)).all()
    assert abs(1.24 * (19 - 15) ** (1.0 / 3) - 1.8 - 0.16838) < 1e-4       # d0 of every structure up to 19 residues
