"""The pair-head kernels on the GPU (K33 - K36) against tests/pairhead_ref.py, the float64 restatement of their definitions.
Bins and ``value`` are tested for EQUALITY -- every bin, the bits of ``value`` --; the cross-entropy, its gradient and the
expectations against the derived bounds stated at ``assert_sweeps_within_the_bounds``; and, since
include/protstruc_pairhead.h is not in the case table of tests/launch_cases.py, this file also holds the four launchers to
the launch contract: the caller's stream, capture, four threads, the batch limit."""
import ctypes
import functools
import math
import os
import threading

import numpy as np
import pytest
import torch

from tests import pairhead_ref as R
from tests.launch_cases import Case, on_device
from tests.test_gpu_closest import carve
from tests.test_gpu_launch_contract import (SENTINEL, SLEEP_CYCLES, assert_all_same, assert_batch_of_65535_repeats_the_three,
                                            raw, same, side_stream_beside_the_default_stream)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
BIN_SIZES = (1, 2, 3, 5, 63, 64, 65, 130)
CLASSES = (2, 3, 37, 60, 64, 65, 128)
SWEEP_SIZES = (1, 3, 5, 17, 67)
PDB_FILES = ("1a3r_HL", "1REX", "15c8_HL", "1a6v_HL")


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def assert_bins_equal(got, want, what):
    bins, value = host(got[0]), host(got[1])
    assert bins.dtype == np.uint8 and value.dtype == np.float32 and bins.shape == want[0].shape == value.shape, what
    wrong = np.flatnonzero(bins.ravel() != want[0].ravel())
    assert wrong.size == 0, (f"{what}: {wrong.size} bins differ, the first at {np.unravel_index(wrong[0], bins.shape)}: "
                             f"{bins.ravel()[wrong[0]]} for {want[0].ravel()[wrong[0]]}")
    wrong = np.flatnonzero(value.view(np.int32).ravel() != want[1].view(np.int32).ravel())
    assert wrong.size == 0, (f"{what}: {wrong.size} values differ in their bits, the first at {np.unravel_index(wrong[0], value.shape)}: "
                             f"{value.ravel()[wrong[0]]!r} for {want[1].ravel()[wrong[0]]!r}")


# ---- K33 -----------------------------------------------------------------------------------------------------------------------
def frames_of(pkg, backbone):
    """(rot, trans) float32 numpy of the N / CA / C backbone (B,N,3,3): the library's own frames, origin at CA"""
    rot, trans = pkg.ops.frames(dev(backbone), 0, 1, 2, 1)
    return host(rot), host(trans)


@functools.lru_cache(maxsize=None)
def chain_pair(N):
    """a synthetic chain and a target 2 A away from it, (B,N,3,3) float32 each"""
    backbone = R.backbone_case(2, N, seed=100 + N)
    noise = np.random.default_rng(200 + N).normal(size=backbone.shape) * 2.0
    return backbone, (backbone + noise).astype(np.float32)


@pytest.mark.parametrize("N", BIN_SIZES)
def test_bins_distance(pkg, N):
    points = chain_pair(N)[0][:, :, 1].copy()
    row, col = R.masks(2, N, seed=300 + N)
    assert N < 5 or not np.array_equal(row, col)
    points[~(row | col)] = np.nan                       # a point that is in neither mask holds NaN
    breaks = R.distogram_breaks()
    want = R.bins_distance(points, breaks, row, col)
    got = pkg.ops.pair_bins_distance(dev(points), breaks, dev(row), dev(col), return_value=True)
    assert_bins_equal(got, want, f"distance, N={N}")
    assert same(pkg.ops.pair_bins_distance(dev(points), torch.from_numpy(breaks), dev(row).float(), dev(col)), got[0])
    if N >= 63:
        assert len(np.unique(want[0])) > 30 and 0.5 < (want[0] == 255).mean() < 0.9
    clean = np.nan_to_num(points)
    assert_bins_equal(pkg.ops.pair_bins_distance(dev(clean), breaks, return_value=True), R.bins_distance(clean, breaks), f"no masks, N={N}")


@pytest.mark.parametrize("N", BIN_SIZES)
def test_bins_aligned_error(pkg, N):
    backbone, target = chain_pair(N)
    rot, trans = frames_of(pkg, backbone)
    trot, ttrans = frames_of(pkg, target)
    assert np.abs(np.einsum("bnij,bnik->bnjk", rot.astype(np.float64), rot.astype(np.float64)) - np.eye(3)).max() < 1e-5
    points, tpoints = backbone[:, :, 1].copy(), target[:, :, 1].copy()
    frame, point = R.masks(2, N, seed=400 + N)
    for a in (rot, trans, trot, ttrans):
        a[~frame] = np.nan                               # frames are rows only, points columns only: NaN under either mask
    points[~point], tpoints[~point] = np.nan, np.nan
    breaks = R.aligned_error_breaks()
    want = R.bins_aligned_error(rot, trans, points, trot, ttrans, tpoints, breaks, frame, point)
    tensors = [dev(a) for a in (rot, trans, points, trot, ttrans, tpoints)]
    got = pkg.ops.pair_bins_aligned_error(*tensors, breaks, dev(frame), dev(point), return_value=True)
    assert_bins_equal(got, want, f"aligned error, N={N}")
    assert same(pkg.ops.pair_bins_aligned_error(*tensors, breaks, dev(frame), dev(point)), got[0])
    assert same(pkg.geometry.aligned_error(*tensors, dev(frame), dev(point)), got[1])
    if N >= 63:
        assert len(np.unique(want[0])) > 10 and 0.5 < (want[0] == 255).mean() < 0.9


def test_bins_on_a_lattice_full_of_values_on_a_break(pkg):
    N = 70
    points, tpoints = R.lattice_points(2, N, seed=6), R.lattice_points(2, N, seed=9)
    breaks = np.arange(1, 31, dtype=np.float32)
    v2 = R.distance_v2(points)
    assert np.isin(v2, R.sq_breaks(breaks)).sum() >= 20
    row, col = R.masks(2, N, seed=10, keep=0.8)
    assert_bins_equal(pkg.ops.pair_bins_distance(dev(points), breaks, dev(row), dev(col), return_value=True),
                      R.bins_distance(points, breaks, row, col), "lattice, distance")
    rot, trans = R.lattice_frames(2, N, seed=7)
    trot, ttrans = R.lattice_frames(2, N, seed=8)
    v2 = R.aligned_v2(rot, trans, points, trot, ttrans, tpoints)
    counted = row[:, :, None] & col[:, None, :]
    assert (np.isin(v2, R.sq_breaks(breaks)) & counted).sum() >= 20
    got = pkg.ops.pair_bins_aligned_error(*[dev(a) for a in (rot, trans, points, trot, ttrans, tpoints)], breaks, dev(row), dev(col),
                                          return_value=True)
    assert_bins_equal(got, R.bins_aligned_error(rot, trans, points, trot, ttrans, tpoints, breaks, row, col), "lattice, aligned error")
    # a single break, and 127 of them
    for table in (np.array([5.0], dtype=np.float32), np.arange(127, dtype=np.float32) * 0.25):
        assert_bins_equal(pkg.ops.pair_bins_distance(dev(points), table, return_value=True), R.bins_distance(points, table),
                          f"{table.size} breaks")


@functools.lru_cache(maxsize=None)
def pdb_batch():
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, name + ".pdb") for name in PDB_FILES])


def moved_copy(batch, seed, sigma=0.5):
    from protstruc_amd import StructureBatch
    g = torch.Generator().manual_seed(seed)
    noise = (torch.randn(batch.get_xyz().shape, generator=g) * sigma).to(batch.get_xyz().device)
    return StructureBatch(batch.get_xyz() + noise, batch.get_atom_mask(), batch.chain_idx, batch.get_chain_ids())


def pseudo_beta(batch):
    """numpy restatement: CB (slot 4) where present, else CA (slot 1), and the mask to match"""
    xyz, present = host(batch.get_xyz()), host(batch._present_atoms())
    return np.where(present[:, :, 4, None], xyz[:, :, 4], xyz[:, :, 1]), present[:, :, 4] | present[:, :, 1]


def aligned_error_yardstick(pkg, batch, target, breaks):
    """(bins, value) of the yardstick from the library's frames of both batches, and the masks of the FAPE rule"""
    xyz, txyz = batch.get_xyz(), target.get_xyz()
    present = host(batch.get_atom_mask() != 0) & host(target.get_atom_mask() != 0)
    rot, trans = (host(t) for t in pkg.ops.frames(xyz, 0, 1, 2, 1))
    trot, ttrans = (host(t) for t in pkg.ops.frames(txyz, 0, 1, 2, 1))
    frame = present[:, :, 0] & present[:, :, 1] & present[:, :, 2]
    return R.bins_aligned_error(rot, trans, host(xyz)[:, :, 1], trot, ttrans, host(txyz)[:, :, 1], breaks, frame, present[:, :, 1])


def test_bins_of_the_pdb_files(pkg):
    batch = pdb_batch()
    assert batch.get_xyz().isnan().any() and not bool(batch.residue_mask.all()), "a padded batch that carries NaN for missing atoms"
    points, mask = pseudo_beta(batch)
    got_points, got_mask = batch._pseudo_beta()
    assert np.array_equal(host(got_mask), mask) and np.array_equal(host(got_points)[mask], points[mask])
    breaks = R.distogram_breaks()
    assert_bins_equal(pkg.ops.pair_bins_distance(got_points, breaks, got_mask, got_mask, return_value=True),
                      R.bins_distance(points, breaks, mask, mask), "PDB, distogram")
    target = moved_copy(batch, seed=3)
    want = aligned_error_yardstick(pkg, batch, target, R.aligned_error_breaks())
    got = batch.aligned_error(target)
    assert same(got, dev(want[1])), "PDB, the aligned-error matrix"
    assert 0.02 < np.isinf(want[1]).mean() < 0.9 and len(np.unique(want[0])) > 30, "the case is meant to fill many bins"


# ---- K34 / K35 / K36 -----------------------------------------------------------------------------------------------------------
def tables(C, n_residues, B=2, V=4, seed=0):
    """(B,V,C) float32: bin centres up to 31.75, the TM kernel of a structure of ``n_residues``, a 0/1 indicator, and random
    numbers; structure 1's are half of structure 0's, so that a launch that reads the wrong structure's table fails"""
    centers = np.linspace(0.25, 31.75, C)
    d0 = 1.24 * (max(n_residues, 19) - 15) ** (1.0 / 3.0) - 1.8
    one = np.stack([centers, 1.0 / (1.0 + (centers / d0) ** 2), (np.arange(C) < max(1, C // 3)).astype(np.float64),
                    np.random.default_rng(seed).normal(size=C)])[:V]
    return np.stack([one * 0.5 ** b for b in range(B)]).astype(np.float32)


WORST = {"K34": 0.0, "K35": 0.0, "K36": 0.0}


def assert_sweeps_within_the_bounds(pkg, x, bins, what, tables_=(1, 2, 4), seed=0):
    """K34, K35 and K36 on the logits ``x`` (B,N,N,C) and the labels ``bins`` against the yardstick.  With E the per-pair
    bound 2^-22 (2 + ln C + |lse| + |ce|) + C 2^-24 -- twice the sum of: 1 ulp each for v_exp_f32 and v_log_f32, the
    rounding of the exponentials' arguments (sum_k p_k (m - x_k) <= ln C), up to C - 1 float additions, and the two final
    roundings of lse and ce --
      K34  |row_loss - ref| <= sum over the counted j of E + 2^-24 |ref|, row_count equal
      K35  |grad - ref| <= |grad_row| (p E + 2^-22) per element; bitwise +0.0 where the label is >= C
      K36  |out - ref| <= max_k |v_k| (2^-22 (2 + ln C) + C 2^-23)"""
    B, N, _, C = x.shape
    ref = R.CrossEntropy(x, bins)
    xd, bd = dev(x), dev(bins)
    row_loss, row_count = pkg.ops.binned_cross_entropy(xd, bd)
    assert row_loss.dtype == torch.float32 and row_count.dtype == torch.int32 and tuple(row_loss.shape) == (B, N)
    assert np.array_equal(host(row_count), ref.row_count), f"{what}: row_count"
    err, bound = np.abs(host(row_loss).astype(np.float64) - ref.row_loss), ref.row_bound()
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    WORST["K34"] = max(WORST["K34"], ratio)
    print(f"{what}: K34 max |row_loss - ref| = {err.max():.3e}, worst ratio to the bound {ratio:.3f}")
    assert np.isfinite(host(row_loss)).all() and (err <= bound).all(), f"{what}: K34"

    g = np.random.default_rng(seed + 1).normal(size=(B, N)).astype(np.float32)
    grad = host(pkg.ops.binned_cross_entropy_backward(xd, bd, dev(g)))
    assert grad.shape == x.shape and grad.dtype == np.float32
    assert (grad.view(np.int32)[~ref.counted] == 0).all(), f"{what}: K35 does not write +0.0 under a label >= C"
    want = ref.backward(g)
    bound = np.abs(g.astype(np.float64))[:, :, None, None] * (ref.p * ref.pair_bound()[..., None] + 2.0 ** -22)
    err = np.abs(grad.astype(np.float64) - want)
    ratio = float((err[ref.counted] / bound[ref.counted]).max()) if ref.counted.any() else 0.0
    WORST["K35"] = max(WORST["K35"], ratio)
    print(f"{what}: K35 max |grad - ref| = {err.max():.3e}, worst ratio to the bound {ratio:.3f}")
    assert np.isfinite(grad).all() and (err[ref.counted] <= bound[ref.counted]).all(), f"{what}: K35"

    legal = np.isfinite(x).any(-1) & ~np.isnan(x).any(-1)          # a pair of NaN logits has no softmax
    for V in tables_:
        values = tables(C, N, B, V, seed)
        out = host(pkg.ops.binned_expectation(xd, dev(values)))
        assert out.shape == (V, B, N, N) and out.dtype == np.float32
        with np.errstate(invalid="ignore"):
            want = R.expectation(np.where(legal[..., None], x, 0.0), values)
        err = np.abs(out.astype(np.float64) - want)[:, legal]
        bound = np.broadcast_to(R.expectation_bound(values, C), want.shape)[:, legal]
        ratio = float((err / bound).max())
        WORST["K36"] = max(WORST["K36"], ratio)
        print(f"{what}: K36 V={V} max |out - ref| = {err.max():.3e}, worst ratio to the bound {ratio:.3f}")
        assert (err <= bound).all(), f"{what}: K36, V={V}"
    return row_loss, grad


@pytest.mark.parametrize("family", R.LOGIT_FAMILIES)
@pytest.mark.parametrize("C", CLASSES)
def test_sweeps_against_the_yardstick(pkg, C, family):
    for N in SWEEP_SIZES:
        x, bins = R.logits_case(family, 2, N, C, seed=1000 * C + N)
        assert family != "nan_under_no_target" or N < 17 or np.isnan(x).any()
        assert_sweeps_within_the_bounds(pkg, x, bins, f"{family}, C={C}, N={N}", seed=C + N)
    print(f"worst ratios so far: {WORST}")


def test_wider_labels_are_mapped_so_that_nothing_wraps(pkg):
    N, C = 17, 37
    x, bins = R.logits_case("normal", 2, N, C, seed=5)
    wild = bins.astype(np.int64)
    wild[bins == 255] = np.random.default_rng(6).choice([-1, -256 + 3, 256, 256 + 5, C, 2 ** 40, 255], size=int((bins == 255).sum()))
    xd = dev(x)
    want = pkg.ops.binned_cross_entropy(xd, dev(bins))
    got = pkg.ops.binned_cross_entropy(xd, dev(wild))
    assert same(got[0], want[0]) and same(got[1], want[1])
    g = torch.randn(2, N, device="cuda")
    assert same(pkg.ops.binned_cross_entropy_backward(xd, dev(wild), g), pkg.ops.binned_cross_entropy_backward(xd, dev(bins), g))
    assert same(pkg.ops.binned_cross_entropy(xd.double(), dev(bins).int())[0], want[0])


def test_autograd_through_binned_cross_entropy(pkg):
    N, C = 17, 64
    x, bins = R.logits_case("normal", 2, N, C, seed=7)
    bins[1] = 255                                          # a structure without a labelled pair: loss 0, zero gradients
    ref = R.CrossEntropy(x, bins)
    logits = dev(x).requires_grad_(True)
    loss = pkg.geometry.binned_cross_entropy(logits, dev(bins), eps=1e-6)
    assert tuple(loss.shape) == (2,) and loss.dtype == torch.float32 and float(loss[1].detach()) == 0.0
    want = ref.row_loss.sum(-1) / (1e-6 + ref.row_count.sum(-1))
    assert abs(float(loss[0].detach()) - want[0]) <= ref.row_bound()[0].sum() / ref.row_count[0].sum() + 2.0 ** -23 * want[0]
    weights = torch.tensor([0.7, 1.3], device="cuda")
    (loss * weights).sum().backward()
    grad_row = (weights[:, None].double() / (1e-6 + dev(ref.row_count).sum(1, keepdim=True).double())).float().expand(2, N)
    assert same(logits.grad, pkg.ops.binned_cross_entropy_backward(logits.detach(), dev(bins), grad_row))
    assert bool((logits.grad[1] == 0).all()) and float(logits.grad[0].abs().max()) > 0
    # float64 logits get a float64 gradient of the same values
    logits64 = dev(x).double().requires_grad_(True)
    (pkg.geometry.binned_cross_entropy(logits64, dev(bins)) * weights).sum().backward()
    assert logits64.grad.dtype == torch.float64 and torch.equal(logits64.grad.float(), logits.grad)


# ---- what is read out of the logits --------------------------------------------------------------------------------------------
def test_readouts_against_the_yardstick(pkg):
    """pTM, ipTM, PAE and contact probability at C = 64 with padding rows masked.  K36's bound with max |v| = 1 (TM kernel,
    indicator) or 31.75 (centres); pTM adds 2^-23 for the float32 table and the final rounding -- an average of terms does
    not amplify their absolute error."""
    B, N, C = 2, 67, 64
    x = (3.0 * R.logits_case("normal", B, N, C, seed=21)[0]).astype(np.float32)
    mask = np.ones((B, N), dtype=bool)
    mask[1, 40:] = False
    x[1, 40:], x[1, :, 40:] = np.nan, np.nan               # the padding's logits are not read into any result
    chain = np.array([[0] * 30 + [1] * 37, [0] * 25 + [1] * 15 + [-1] * 27])
    unit = 2.0 ** -22 * (2.0 + math.log(C)) + C * 2.0 ** -23
    xd = dev(np.nan_to_num(x))
    clean = np.nan_to_num(x)
    for interface in (False, True):
        got = host(pkg.geometry.predicted_tm_score(dev(x), dev(mask), dev(chain), interface)).astype(np.float64)
        want = R.predicted_tm_score(clean, mask, chain, interface)
        print(f"pTM interface={interface}: {got} for {want}")
        assert got.shape == (B,) and (np.abs(got - want) <= unit + 2.0 ** -23).all() and (want > 0.01).all()
    assert not np.allclose(R.predicted_tm_score(clean, mask, chain, True), R.predicted_tm_score(clean, mask, chain, False))
    pae = host(pkg.geometry.predicted_aligned_error(xd)).astype(np.float64)
    assert pae.shape == (B, N, N) and (np.abs(pae - R.predicted_aligned_error(clean)) <= 31.75 * unit).all()
    assert same(pkg.geometry.predicted_aligned_error(xd, max_bin=31.0), pkg.ops.binned_expectation(
        xd, pkg.geometry.aligned_error_bin_centers().float().cuda().expand(B, 1, C))[0])
    for cutoff in (8.0, 12.0):
        contact = host(pkg.geometry.contact_probability(xd, cutoff)).astype(np.float64)
        assert (np.abs(contact - R.contact_probability(clean, cutoff)) <= unit).all() and 0.0 < contact.min() < contact.max() < 1.0
    with pytest.raises(ValueError, match="breaks"):
        pkg.geometry.contact_probability(xd, 8.0, breaks=[1.0, 2.0])
    with pytest.raises(ValueError, match="chain_idx"):
        pkg.geometry.predicted_tm_score(xd, dev(mask), None, True)


# ---- alignment and sentinels ---------------------------------------------------------------------------------------------------
def intact(buf, start, n_bytes):
    return bool((buf[:start] == SENTINEL).all()) and bool((buf[start + n_bytes:] == SENTINEL).all())


@pytest.mark.parametrize("C", (64, 37))
@pytest.mark.parametrize("off,bins_off", ((0, 1), (4, 6), (8, 11), (12, 15), (4, 8), (0, 0)))
def test_sentinels_and_alignment(pkg, C, off, bins_off):
    """logits, grad_logits, row_loss, row_count, value and out ``off`` bytes past a 16-byte boundary and the bins ``bins_off``
    bytes, inside sentinels: the results are those of the aligned run through ``ops``, bit for bit, and no sentinel byte
    changes.  At C = 64 the aligned run takes the 16-byte arm and every off != 0 the 4-byte arm."""
    from protstruc_amd import _lib
    lib = _lib.load()
    B, N, V = 2, 17, 2
    stream = torch.cuda.current_stream().cuda_stream
    x, labels = R.logits_case("normal", B, N, C, seed=31 + C)
    points = chain_pair(N)[0][:, :, 1]
    breaks = R.distogram_breaks(n_bins=C)
    table = (ctypes_floats(breaks), len(breaks))
    want_bins, want_value = pkg.ops.pair_bins_distance(dev(points), breaks, return_value=True)
    # K33 into misaligned outputs
    bbuf, b, bstart = carve(B * N * N, bins_off, torch.uint8)
    vbuf, v, vstart = carve(B * N * N * 4, off, torch.float32)
    _, p, _ = carve(points.nbytes, off, torch.float32)
    p.copy_(dev(points).reshape(-1))
    assert lib.ps_pair_bins_f32(0, p.data_ptr(), None, None, None, None, None, None, None, table[0], table[1], b.data_ptr(),
                                v.data_ptr(), B, N, stream) == 0
    torch.cuda.synchronize()
    assert same(b.reshape(B, N, N), want_bins) and same(v.reshape(B, N, N), want_value)
    assert intact(bbuf, bstart, B * N * N) and intact(vbuf, vstart, B * N * N * 4)
    # the labels of the sweeps, misaligned as well
    b.copy_(dev(labels).reshape(-1))
    _, xm, _ = carve(x.nbytes, off, torch.float32)
    xm.copy_(dev(x).reshape(-1))
    want_loss, want_count = pkg.ops.binned_cross_entropy(dev(x), dev(labels))
    lbuf, loss, lstart = carve(B * N * 4, off, torch.float32)
    cbuf, count, cstart = carve(B * N * 4, off, torch.int32)
    assert lib.ps_binned_cross_entropy_f32(xm.data_ptr(), b.data_ptr(), loss.data_ptr(), count.data_ptr(), B, N, C, stream) == 0
    torch.cuda.synchronize()
    assert same(loss.reshape(B, N), want_loss) and same(count.reshape(B, N), want_count)
    assert intact(lbuf, lstart, B * N * 4) and intact(cbuf, cstart, B * N * 4)
    g = torch.randn(B, N, device="cuda")
    gbuf, grad, gstart = carve(x.nbytes, off, torch.float32)
    assert lib.ps_binned_cross_entropy_backward_f32(xm.data_ptr(), b.data_ptr(), g.data_ptr(), grad.data_ptr(), B, N, C, stream) == 0
    torch.cuda.synchronize()
    assert same(grad.reshape(B, N, N, C), pkg.ops.binned_cross_entropy_backward(dev(x), dev(labels), g))
    assert intact(gbuf, gstart, x.nbytes)
    # logits aligned, the gradient not: the 4-byte arm again
    if off:
        gbuf, grad, gstart = carve(x.nbytes, off, torch.float32)
        xa = dev(x)
        assert lib.ps_binned_cross_entropy_backward_f32(xa.data_ptr(), b.data_ptr(), g.data_ptr(), grad.data_ptr(), B, N, C, stream) == 0
        torch.cuda.synchronize()
        assert same(grad.reshape(B, N, N, C), pkg.ops.binned_cross_entropy_backward(xa, dev(labels), g)) and intact(gbuf, gstart, x.nbytes)
    values = dev(tables(C, N, B, V))
    obuf, out, ostart = carve(V * B * N * N * 4, off, torch.float32)
    assert lib.ps_binned_expectation_f32(xm.data_ptr(), values.data_ptr(), out.data_ptr(), B, N, C, V, stream) == 0
    torch.cuda.synchronize()
    assert same(out.reshape(V, B, N, N), pkg.ops.binned_expectation(dev(x), values)) and intact(obuf, ostart, V * B * N * N * 4)


def ctypes_floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


# ---- beyond 2^31 floats ----------------------------------------------------------------------------------------------------------
def test_offsets_past_two_to_the_31(pkg):
    """B = 128, N = 512, C = 64: 2^31 floats of logits, made on the device; one launch each of K34, K35 and K36; the first
    row and the last two rows of the last structure -- whose offsets lie past 2^31 elements -- against the yardstick"""
    B, N, C, V = 128, 512, 64, 2
    g = torch.Generator(device="cuda").manual_seed(41)
    logits = torch.randn(B, N, N, C, device="cuda", generator=g)
    assert logits.numel() >= 2 ** 31
    labels = torch.randint(0, C, (B, N, N), device="cuda", generator=g, dtype=torch.uint8)
    labels[torch.rand(B, N, N, device="cuda", generator=g) < 0.1] = 255
    grad_row = torch.randn(B, N, device="cuda", generator=g)
    values = dev(tables(C, N, 1, V)).expand(B, V, C).contiguous()
    row_loss, row_count = pkg.ops.binned_cross_entropy(logits, labels)
    grad = pkg.ops.binned_cross_entropy_backward(logits, labels, grad_row)
    out = pkg.ops.binned_expectation(logits, values)
    torch.cuda.synchronize()
    for b, rows in ((0, slice(0, 1)), (B - 1, slice(N - 2, N))):
        x = host(logits[b, rows])[None]
        ref = R.CrossEntropy(x, host(labels[b, rows])[None])
        assert np.array_equal(host(row_count[b, rows]), ref.row_count[0])
        assert (np.abs(host(row_loss[b, rows]).astype(np.float64) - ref.row_loss[0]) <= ref.row_bound()[0]).all(), f"K34, structure {b}"
        gr = host(grad_row[b, rows])[None]
        got = host(grad[b, rows]).astype(np.float64)
        bound = np.abs(gr.astype(np.float64))[:, :, None, None] * (ref.p * ref.pair_bound()[..., None] + 2.0 ** -22)
        assert (got[~ref.counted[0]] == 0).all() and (np.abs(got - ref.backward(gr)[0]) <= bound[0]).all(), f"K35, structure {b}"
        want = R.expectation(x, host(values[:1]))[:, 0]
        assert (np.abs(host(out[:, b, rows]).astype(np.float64) - want) <= R.expectation_bound(host(values[:1]), C)[:, 0]).all(), f"K36, structure {b}"
    del logits, grad, out, labels, row_loss, row_count, grad_row, values
    torch.cuda.empty_cache()


# ---- repeatability -------------------------------------------------------------------------------------------------------------
def test_repeatability(pkg):
    N, C = 67, 64
    x, bins = R.logits_case("spread", 2, N, C, seed=51)
    xd, bd, g = dev(x), dev(bins), torch.randn(2, N, device="cuda")
    first = pkg.ops.binned_cross_entropy(xd, bd)
    grad = pkg.ops.binned_cross_entropy_backward(xd, bd, g)
    for _ in range(2):
        again = pkg.ops.binned_cross_entropy(xd, bd)
        assert same(again[0], first[0]) and same(again[1], first[1])
        assert same(pkg.ops.binned_cross_entropy_backward(xd, bd, g), grad)


# ---- StructureBatch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("1REX", "1a3r_HL"))
def test_structure_batch_methods(pkg, name):
    from protstruc_amd import StructureBatch
    batch = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, name + ".pdb"))
    B, N, C = 1, batch.get_xyz().shape[1], 64
    assert len(batch.get_chain_ids()[0]) == (2 if name == "1a3r_HL" else 1)
    g = torch.Generator().manual_seed(61)
    x = (2.0 * torch.randn(B, N, N, C, generator=g)).numpy()
    # the distogram loss and its gradient
    points, mask = pseudo_beta(batch)
    bins = R.bins_distance(points, R.distogram_breaks(), mask, mask)[0]
    ref = R.CrossEntropy(x, bins)
    count = ref.row_count.sum()
    want = ref.row_loss.sum() / (1e-6 + count)
    logits = dev(x).requires_grad_(True)
    loss = batch.distogram_loss(logits)
    assert tuple(loss.shape) == (1,) and count > N
    assert abs(float(loss.detach()) - want) <= ref.row_bound().sum() / count + 2.0 ** -23 * want, (float(loss.detach()), want)
    loss.sum().backward()
    grad_row = np.full((B, N), 1.0 / (1e-6 + count)).astype(np.float32)
    bound = np.abs(grad_row.astype(np.float64))[:, :, None, None] * (ref.p * ref.pair_bound()[..., None] + 2.0 ** -22)
    got = host(logits.grad).astype(np.float64)
    assert (np.abs(got - ref.backward(grad_row)) <= bound).all() and (got[~ref.counted] == 0).all() and np.abs(got).max() > 0
    # the aligned error against a moved copy, and its loss
    target = moved_copy(batch, seed=62)
    ae_bins, ae = aligned_error_yardstick(pkg, batch, target, R.aligned_error_breaks())
    assert same(batch.aligned_error(target), dev(ae)) and np.isfinite(ae).mean() > 0.5
    ref = R.CrossEntropy(x, ae_bins)
    count = ref.row_count.sum()
    want = ref.row_loss.sum() / (1e-8 + count)
    loss = batch.aligned_error_loss(dev(x), target)
    assert abs(float(loss) - want) <= ref.row_bound().sum() / count + 2.0 ** -23 * want, (float(loss), want)
    # what is read out of a PAE head
    unit = 2.0 ** -22 * (2.0 + math.log(C)) + C * 2.0 ** -23
    mask, chain = host(batch.residue_mask), host(batch._chain_keys())
    for interface in (False, True):
        got = float(batch.predicted_tm_score(dev(x), interface))
        want = float(R.predicted_tm_score(x, mask, chain, interface)[0])
        assert abs(got - want) <= unit + 2.0 ** -23 and (want > 0.0) == (not interface or name == "1a3r_HL"), (interface, got, want)
    pae = host(batch.predicted_aligned_error(dev(x))).astype(np.float64)
    inside = mask[:, :, None] & mask[:, None, :]
    assert (np.abs(pae - R.predicted_aligned_error(x))[inside] <= 31.75 * unit).all() and np.isinf(pae[~inside]).all()


# ---- the launch contract -------------------------------------------------------------------------------------------------------
# Two seeded variants that differ in every output; float64 strided points and logits, float masks and int64 labels, so that
# the shell's conversions are on the launch path that is checked (as the cases of tests/launch_cases.py).
CONTRACT_N, CONTRACT_C = 19, 64
CONTRACT_BREAKS = tuple(float(v) for v in R.aligned_error_breaks())


def _bins_inputs(v):
    s = {"A": 0, "B": 1}[v]
    bb = R.backbone_case(2, CONTRACT_N, seed=70 + s)
    tb = (bb + np.random.default_rng(72 + s).normal(size=bb.shape)).astype(np.float32)
    rot, trot = (np.linalg.qr(np.random.default_rng(k + s).normal(size=(2, CONTRACT_N, 3, 3)))[0].astype(np.float32) for k in (74, 76))
    frame, point = R.masks(2, CONTRACT_N, seed=78 + s, keep=0.8)
    t = torch.from_numpy
    return dict(points=t(bb[:, :, 1].copy()).double(), rot=t(rot), trans=t(bb[:, :, 0].copy()), target_rot=t(trot),
                target_trans=t(tb[:, :, 0].copy()), target_points=t(tb[:, :, 1].copy()), frame_mask=t(frame).float(), point_mask=t(point))


def _sweep_inputs(v):
    s = {"A": 0, "B": 1}[v]
    x, bins = R.logits_case("normal", 2, CONTRACT_N, CONTRACT_C, seed=80 + s)
    g = np.random.default_rng(82 + s).normal(size=(2, CONTRACT_N)).astype(np.float32)
    return dict(logits=torch.from_numpy(x).double(), bins=torch.from_numpy(bins).long(), grad_row=torch.from_numpy(g),
                values=torch.from_numpy(tables(CONTRACT_C, CONTRACT_N, 2, 3, seed=84 + s)))


def _ops():
    from protstruc_amd import ops
    return ops


CONTRACT = (
    Case("pair_bins", ("ps_pair_bins_f32",), _bins_inputs,
         lambda i: _ops().pair_bins_aligned_error(i["rot"], i["trans"], i["points"], i["target_rot"], i["target_trans"],
                                                  i["target_points"], CONTRACT_BREAKS, i["frame_mask"], i["point_mask"],
                                                  return_value=True), strided=("points",)),
    Case("binned_cross_entropy", ("ps_binned_cross_entropy_f32",), _sweep_inputs,
         lambda i: _ops().binned_cross_entropy(i["logits"], i["bins"]), strided=("logits",)),
    Case("binned_cross_entropy_backward", ("ps_binned_cross_entropy_backward_f32",), _sweep_inputs,
         lambda i: (_ops().binned_cross_entropy_backward(i["logits"], i["bins"], i["grad_row"]),), strided=("logits",)),
    Case("binned_expectation", ("ps_binned_expectation_f32",), _sweep_inputs,
         lambda i: (_ops().binned_expectation(i["logits"], i["values"]),), strided=("logits",)),
)
BY_NAME = {case.name: case for case in CONTRACT}
NAMES = list(BY_NAME)


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
        assert a.shape == b.shape and a.dtype == b.dtype and not same(a, b), (name, k)


def test_contract_cases_cover_the_header_and_meet_the_yardstick(pkg):
    from protstruc_amd import _lib
    assert sorted(s for case in CONTRACT for s in case.symbols) == sorted(set(_lib.PAIRHEAD_SIGNATURES) - {"ps_pairhead_api"})
    for name in NAMES:
        assert_variants_differ(name)
    for v in "AB":
        i = {k: t.numpy() for k, t in _bins_inputs(v).items()}
        want = R.bins_aligned_error(i["rot"], i["trans"], i["points"].astype(np.float32), i["target_rot"], i["target_trans"],
                                    i["target_points"], CONTRACT_BREAKS, i["frame_mask"], i["point_mask"])
        assert_bins_equal(eager("pair_bins", v), want, f"pair_bins {v}")
        i = _sweep_inputs(v)
        ref = R.CrossEntropy(i["logits"].numpy().astype(np.float32), i["bins"].numpy())
        loss, count = eager("binned_cross_entropy", v)
        assert np.array_equal(host(count), ref.row_count) and (np.abs(host(loss) - ref.row_loss) <= ref.row_bound()).all()


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
    for k, (o, w) in enumerate(zip(outs, want_a)):
        assert not same(o, w), f"{name}: output {k} was computed from the inputs as they were before the side stream's copies"


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
            order = NAMES[t:] + NAMES[:t]
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
    """B = 65535 at N = 2: structure b is structure b % 3, and the results are those of the three, bit for bit"""
    ops = pkg.ops
    N, C = 2, 64
    bb = R.backbone_case(3, N, seed=90)
    tb = (bb + np.random.default_rng(91).normal(size=bb.shape)).astype(np.float32)
    frame = np.ones((3, N), dtype=bool)
    frame[1, 0] = False
    bb[1, 0] = np.nan                                      # one frame missing, with NaN under the mask
    tensors = dict(zip(("rot", "trans"), pkg.ops.frames(dev(bb), 0, 1, 2, 1)))
    tensors.update(zip(("target_rot", "target_trans"), pkg.ops.frames(dev(tb), 0, 1, 2, 1)))
    tensors.update(points=dev(np.nan_to_num(bb[:, :, 1])), target_points=dev(tb[:, :, 1]), frame_mask=dev(frame))
    run = functools.partial(ops.pair_bins_aligned_error, breaks=CONTRACT_BREAKS, return_value=True)
    small = run(**tensors)
    want = R.bins_aligned_error(*[host(tensors[k]) for k in ("rot", "trans", "points", "target_rot", "target_trans", "target_points")],
                                CONTRACT_BREAKS, frame)
    assert_bins_equal(small, want, "N = 2")
    assert len({tuple(want[1][b].ravel()) for b in range(3)}) == 3
    assert_batch_of_65535_repeats_the_three(run, tensors, small, "pair_bins_aligned_error")
    run = functools.partial(ops.pair_bins_distance, breaks=R.distogram_breaks(), return_value=True)
    tensors = dict(points=dev(3.0 * tb[:, :, 1]), row_mask=dev(frame))
    assert_batch_of_65535_repeats_the_three(run, tensors, run(**tensors), "pair_bins_distance")
    x, bins = R.logits_case("normal", 3, N, C, seed=92)
    g = np.random.default_rng(93).normal(size=(3, N)).astype(np.float32)
    tensors = dict(logits=dev(x), bins=dev(bins))
    assert_batch_of_65535_repeats_the_three(ops.binned_cross_entropy, tensors, ops.binned_cross_entropy(**tensors), "binned_cross_entropy")
    tensors["grad_row"] = dev(g)
    assert_batch_of_65535_repeats_the_three(ops.binned_cross_entropy_backward, tensors, ops.binned_cross_entropy_backward(**tensors),
                                            "binned_cross_entropy_backward")
    tensors = dict(logits=dev(x), values=dev(tables(C, N, 3, 4)))

    def structure_first(**t):
        return ops.binned_expectation(**t).transpose(0, 1)           # (B,V,N,N): the batch axis in front, as the helper tiles it

    assert_batch_of_65535_repeats_the_three(structure_first, tensors, structure_first(**tensors), "binned_expectation")
