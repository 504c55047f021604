"""The ensemble kernels without a GPU: the C header include/protstruc_ensemble.h against the binding and the cross-compiled
library, the argument checks of the launchers and of the shell, the two restatements of tests/ensemble_ref.py against each
other and against brute force, and the bound of K45: on every input the GPU tests use, the header's formula evaluated in
float64, forwards and backwards, stays inside the bound against the yardstick -- so those inputs are shown to lie inside it
by arithmetic alone."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import ensemble_ref as R
from tests.c_headers import declared_symbols, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "protstruc_ensemble.h"
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
LAUNCHERS = ["ps_cluster_f32", "ps_rmsd_matrix_f32"]
HOST_FUNCTIONS = ["ps_cluster_workspace_bytes", "ps_ensemble_api"]
PDB_NAME = "1REX"      # tests/test_gpu_ensemble.py uses the same file


@pytest.fixture(scope="module")
def lib():
    from protstruc_amd import _lib, build
    build.build(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def pdb_ensemble():
    """(xyz (12,N,A,3), atom_mask (12,N,A), family (12,)) of the StructureBatch tests"""
    from protstruc_amd import pdb
    xyz, mask = pdb.read_batch([os.path.join(GOLDEN_DIR, PDB_NAME + ".pdb")])[:2]
    return R.ensemble_of(xyz[0].numpy(), mask[0].numpy().astype(bool))


# ---- the header (tests/test_api_families.py holds it to the binding and the library) ------------------------------------------
def test_the_entry_points_and_the_caveat_of_the_header():
    from protstruc_amd import build
    assert declared_symbols(HEADER) == sorted(LAUNCHERS + HOST_FUNCTIONS)
    assert {"ensemble.hip", "kabsch_solve.hpp"} <= {os.path.basename(d) for d in build._deps()}
    text = header_text(HEADER)
    assert "NOT 0" in text and "ps_superpose_f32" in text, "the header states that identical members do not give an RMSD of 0"


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_any_launch(lib):
    """hipErrorInvalidValue (1) without touching a device; an empty batch returns 0 (the pointers are never dereferenced)."""
    fake = ctypes.c_void_p(0x1000)

    def matrix(a=fake, ma=None, b=fake, mb=None, rmsd=fake, count=fake, Ba=2, Bb=3, M=4):
        return lib.ps_rmsd_matrix_f32(a, ma, b, mb, rmsd, count, Ba, Bb, M, None)

    def cluster(D=fake, valid=None, cutoff=1.0, ws=fake, label=fake, center=fake, size=fake, n=fake, G=1, B=4):
        return lib.ps_cluster_f32(D, valid, cutoff, ws, label, center, size, n, G, B, None)

    assert matrix(Ba=0) == 0 and matrix(Bb=0) == 0 and matrix(Ba=0, Bb=0, b=None) == 0 and matrix(Ba=0, Bb=0, count=None) == 0
    assert cluster(G=0) == 0
    assert matrix(Ba=0, M=2 ** 31 - 17) == 0 and matrix(M=2 ** 31 - 16) == 1 and matrix(Ba=0, M=2 ** 31 - 1) == 1
    for bad in (dict(a=None), dict(rmsd=None), dict(Ba=-1), dict(Ba=65536), dict(Bb=-1), dict(Bb=65536), dict(M=0), dict(M=-2),
                dict(Ba=0, M=0), dict(b=None), dict(b=None, Ba=3, Bb=3, mb=fake), dict(b=None, Ba=0, Bb=3)):
        assert matrix(**bad) == 1, bad          # b = None with Bb != Ba, or with a mask_b, is no self mode
    for bad in (dict(D=None), dict(ws=None), dict(label=None), dict(center=None), dict(size=None), dict(n=None), dict(B=0),
                dict(B=4097), dict(G=-1), dict(G=65536), dict(cutoff=math.nan), dict(cutoff=math.inf), dict(cutoff=-math.inf),
                dict(G=0, B=4097), dict(G=0, cutoff=math.nan)):
        assert cluster(**bad) == 1, bad
    assert lib.ps_cluster_workspace_bytes(3, 4096) == 3 * 4096 * 128 * 4 and lib.ps_cluster_workspace_bytes(65535, 2) == 65535 * 2 * 4
    assert lib.ps_cluster_workspace_bytes(0, 5) == 0 and lib.ps_cluster_workspace_bytes(1, 33) == 33 * 2 * 4
    assert lib.ps_cluster_workspace_bytes(1, 4097) == -1 and lib.ps_cluster_workspace_bytes(1, 0) == -1
    assert lib.ps_cluster_workspace_bytes(65536, 2) == -1 and lib.ps_cluster_workspace_bytes(-1, 2) == -1


def test_shape_checks_of_the_shell():
    from protstruc_amd import StructureBatch, geometry, ops
    a, b = torch.zeros(3, 7, 3), torch.zeros(2, 7, 3)
    check = ops.check_rmsd_matrix_shapes
    assert check(a, b.double(), torch.ones(3, 7), torch.ones(2, 7, dtype=torch.bool)) == (3, 2, 7)
    assert check(a) == (3, 3, 7) and check(a, None, torch.ones(3, 7)) == (3, 3, 7)
    for bad, message in ((dict(a=torch.zeros(3, 7)), "a must have shape"), (dict(a=torch.zeros(3, 7, 2)), "a must have shape"),
                         (dict(a=torch.zeros(3, 7, 3, 1)), "a must have shape"), (dict(a=a.long()), "floating-point"),
                         (dict(a=torch.zeros(3, 0, 3)), "points per structure"), (dict(b=torch.zeros(2, 7)), "b must have shape"),
                         (dict(b=torch.zeros(2, 6, 3)), "b must have shape"), (dict(b=b.long()), "floating-point"),
                         (dict(b=None, mask_b=torch.ones(3, 7)), "mask_b needs a b"), (dict(mask_a=torch.ones(2, 7)), "mask_a must have shape"),
                         (dict(mask_b=torch.ones(3, 7)), "mask_b must have shape"), (dict(mask_a=torch.ones(7)), "mask_a must have shape")):
        with pytest.raises(ValueError, match=message):
            check(**{**dict(a=a, b=b), **bad})
    with pytest.raises(ValueError, match="at most 65535"):
        check(torch.zeros(65536, 1, 3))
    D = torch.zeros(2, 5, 5)
    assert ops.check_cluster_shapes(D, 1.5, torch.ones(2, 5)) == (2, 5) and ops.check_cluster_shapes(D.double(), 0) == (2, 5)
    for bad, message in ((dict(D=torch.zeros(5, 5)), "D must have shape"), (dict(D=torch.zeros(2, 5, 4)), "D must have shape"),
                         (dict(D=D.long()), "floating-point"), (dict(D=torch.zeros(1, 4097, 4097, dtype=torch.float16)), "items per matrix"),
                         (dict(D=torch.zeros(1, 0, 0)), "items per matrix"), (dict(cutoff=math.nan), "cutoff must be finite"),
                         (dict(cutoff=math.inf), "cutoff must be finite"), (dict(valid=torch.ones(2, 4)), "valid must have shape"),
                         (dict(valid=torch.ones(5)), "valid must have shape")):
        with pytest.raises(ValueError, match=message):
            ops.check_cluster_shapes(**{**dict(D=D, cutoff=1.0), **bad})
    # the geometry layer: a shared (M,) mask, a single matrix, and its own refusals
    with pytest.raises(ValueError, match="mask_a must have shape"):
        geometry.pairwise_rmsd(a, b, torch.ones(6))
    with pytest.raises(ValueError, match="D must have shape"):
        geometry.cluster_by_cutoff(torch.zeros(5), 1.0)
    for call in (lambda: ops.rmsd_matrix(a, b), lambda: ops.cluster(D, 1.0), lambda: geometry.pairwise_rmsd(a),
                 lambda: geometry.cluster_by_cutoff(D[0], 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert callable(StructureBatch.rmsd_matrix) and callable(StructureBatch.cluster)
    assert geometry.PairwiseRMSD._fields == ("rmsd", "count") and geometry.Clusters._fields == ("label", "center", "size", "n_clusters")


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def one_pair(x, y):
    """the RMSD of two (n,3) float64 clouds after the optimal superposition, from a search-free closed form that shares
    nothing with the yardstick: Horn's quaternion method, the largest eigenvalue of the 4x4 key matrix"""
    xc, yc = x - x.mean(0), y - y.mean(0)
    S = xc.T @ yc
    K = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])
    lam = np.linalg.eigvalsh(K)[-1]
    return math.sqrt(max(0.0, ((xc ** 2).sum() + (yc ** 2).sum() - 2.0 * lam) / x.shape[0]))


@pytest.mark.parametrize("case", [(15, 17, 4, "own"), (3, 65, 257, "none"), (33, 15, 65, "shared"), (2, 3, 2, "none")])
def test_yardstick_against_brute_force(case):
    a, b, ma, mb = R.rmsd_case(*case)
    rmsd, count = R.pairwise_rmsd(a, b, ma, mb)
    _, MA, MB = R._masks(a, b, ma, mb)
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            sel = MA[i] & MB[j]
            assert count[i, j] == sel.sum()
            if not sel.any():
                assert np.isnan(rmsd[i, j])
                continue
            want = one_pair(a[i][sel].astype(np.float64), b[j][sel].astype(np.float64))
            # the eigenvalue form is E0 - 2 lambda itself: it is only good to sqrt(eps E0) near 0
            scale = float(np.abs(a[i][sel].astype(np.float64) - a[i][sel][0]).max()) + 1.0
            assert abs(rmsd[i, j] - want) <= 1e-9 * scale + min(1e-6 * scale, 1e-12 * scale * scale / max(want, 1e-300)), (i, j, rmsd[i, j], want)


def test_yardstick_known_answers():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(1, 40, 3)) * 10
    moved = x @ R.rotation(rng).T + np.array([5.0, -3.0, 2.0])
    rmsd, count = R.pairwise_rmsd(x, moved)
    assert rmsd[0, 0] < 1e-12 and count[0, 0] == 40
    mirrored = x * np.array([-1.0, 1.0, 1.0])
    assert R.pairwise_rmsd(x, mirrored)[0][0, 0] > 1.0, "a mirror image is not a rotation"
    both = np.concatenate([x, moved + rng.normal(scale=0.5, size=x.shape)])
    self_rmsd, _ = R.pairwise_rmsd(both)
    assert self_rmsd.shape == (2, 2) and abs(self_rmsd[0, 1] - self_rmsd[1, 0]) < 1e-12 and 0.5 < self_rmsd[0, 1] < 1.0
    nothing = np.zeros((1, 40), bool)
    assert np.isnan(R.pairwise_rmsd(x, moved, nothing, None)[0]).all()
    x[0, 3, 1] = np.inf
    assert np.isnan(R.pairwise_rmsd(x, moved)[0]).all()
    keep = np.ones((1, 40), bool)
    keep[0, 3] = False
    assert np.isfinite(R.pairwise_rmsd(x, moved, keep, None)[0]).all()


def test_clustering_known_answers():
    # five points on a line at 0, 1, 2, 10, 11 with cutoff 1: item 1 has two neighbours
    pos = np.array([0.0, 1.0, 2.0, 10.0, 11.0])
    D = R.f32(np.abs(pos[:, None] - pos[None, :]))
    for rule in (R.cluster_plain, R.cluster):
        got = rule(D, 1.0)
        assert got.label.tolist() == [0, 0, 0, 1, 1] and got.center.tolist() == [1, 3, -1, -1, -1]
        assert got.size.tolist() == [3, 2, 0, 0, 0] and got.n_clusters == 2
        got = rule(D, 1.0, np.array([1, 0, 1, 1, 1], bool))
        assert got.label.tolist() == [1, -1, 2, 0, 0] and got.center.tolist() == [3, 0, 2, -1, -1] and got.size.tolist() == [2, 1, 1, 0, 0]
        lower = D.copy()
        lower[np.tril_indices(5, -1)] = 0.0             # a lower triangle that says "everything is close": never read
        assert rule(lower, 1.0).label.tolist() == [0, 0, 0, 1, 1]
        nan = D.copy()
        nan[0, 1] = np.nan
        assert rule(nan, 1.0).label.tolist() == [2, 0, 0, 1, 1]


@pytest.mark.parametrize("family", R.CLUSTER_FAMILIES + ("mixed",))
def test_the_two_clustering_restatements_agree(family):
    for B in (1, 2, 63, 64, 65, 200):
        D, cutoff, valid = R.cluster_case(family, B)
        fast, plain = R.cluster_all(D, cutoff, valid), R.cluster_all(D, cutoff, valid, rule=R.cluster_plain)
        assert all(np.array_equal(x, y) for x, y in zip(fast, plain)), (family, B)
        label, center, size, n = fast
        for g in range(D.shape[0]):
            k = int(n[g])
            ok = np.ones(B, bool) if valid is None else valid[g]
            assert (np.diff(size[g][:k]) <= 0).all() and size[g][:k].sum() == ok.sum() and (label[g][~ok] == -1).all()
            assert (label[g][center[g][:k]] == np.arange(k)).all() and (np.bincount(label[g][ok], minlength=k)[:k] == size[g][:k]).all()
    D, cutoff, _ = R.cluster_case("lattice", 200)
    assert (D == np.float32(cutoff)).sum() > 100, "many entries lie exactly at the cutoff"


# ---- the bound -------------------------------------------------------------------------------------------------------------------
def assert_inside_the_bound(a, b, ma, mb, what):
    """the header's formula in float64, both summation orders, against the yardstick: inside the bound; the same counts and
    the same NaN; returns the worst fraction of the bound"""
    ref, n = R.pairwise_rmsd(a, b, ma, mb)
    worst = 0.0
    for reverse in (False, True):
        f = R.formula(a, b, ma, mb, reverse=reverse)
        assert np.array_equal(f.n, n) and np.array_equal(np.isnan(f.rmsd), np.isnan(ref)), what
        ok = ~np.isnan(ref)
        if ok.any():
            fraction = R.fraction_of_bound(np.abs(f.rmsd - ref)[ok], R.bound(ref, n, f.E)[ok])
            assert (fraction <= 1.0).all(), (what, reverse, float(fraction.max()))
            worst = max(worst, float(fraction.max()))
    return worst


@pytest.mark.parametrize("shape", R.SHAPES)
def test_every_gpu_input_lies_inside_the_bound(shape):
    for kind in R.MASK_KINDS:
        a, b, ma, mb = R.rmsd_case(*shape, kind)
        worst = max(assert_inside_the_bound(a, b, ma, mb, (shape, kind, "cross")),
                    assert_inside_the_bound(a, None, ma, None, (shape, kind, "self")),
                    assert_inside_the_bound(a, a, ma, ma, (shape, kind, "a against a")))
        print(f"{shape}, masks {kind}: the float64 formula uses {worst:.3f} of the bound")


def test_the_other_gpu_inputs_lie_inside_the_bound():
    for v in "AB":
        a, b, ma, mb = R.contract_case(v)
        assert_inside_the_bound(a, b, ma, mb, f"contract {v}")
        assert_inside_the_bound(a, None, ma, None, f"contract {v}, self")
    a, b, a3 = R.limit_case()
    assert_inside_the_bound(a, b, None, None, "batch limit")
    assert_inside_the_bound(a3, None, None, None, "batch limit, self")
    xyz, atom_mask, family = pdb_ensemble()
    B, N, A = atom_mask.shape
    ca = assert_inside_the_bound(xyz[:, :, 1], None, atom_mask[:, :, 1], None, "the PDB ensemble, CA")
    every = assert_inside_the_bound(xyz.reshape(B, N * A, 3), None, atom_mask.reshape(B, N * A), None, "the PDB ensemble, all atoms")
    print(f"the PDB ensemble: {ca:.3f} (CA) and {every:.3f} (all atoms) of the bound")
    # and it is the ensemble the clustering test needs: three families of four, far apart at 1.5 A
    rmsd, _ = R.pairwise_rmsd(xyz[:, :, 1], None, atom_mask[:, :, 1], None)
    same = family[:, None] == family[None, :]
    assert rmsd[same].max() < 1.0 and rmsd[~same].min() > 2.5, (rmsd[same].max(), rmsd[~same].min())
    assert sorted(np.bincount(family).tolist()) == [4, 4, 4]
