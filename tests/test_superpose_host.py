"""The superposition scores without a GPU: the C header include/protstruc_superpose.h against the binding and the library,
the seed table of the library against its restatement for every n, the argument checks of the launchers and of the shell,
the yardstick tests/superpose_ref.py against known answers, and the knife-edge guard: every search case the GPU tests
run gives the same scores and the same winning seeds whichever way the sums over points are taken."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import align_ref
from tests import superpose_ref as R
from tests.c_headers import declared_symbols, header_text, macros

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "protstruc_superpose.h"
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
LAUNCHERS = ["ps_superpose_backward_f32", "ps_superpose_f32", "ps_superpose_search_f32"]
HOST_FUNCTIONS = ["ps_superpose_api", "ps_superpose_seed", "ps_superpose_seed_count", "ps_superpose_workspace_floats"]
PDB_CASES = (("1REX", 11), ("1a3r_HL", 12))     # file, seed of the perturbed model: tests/test_gpu_superpose.py uses the same


@pytest.fixture(scope="module")
def lib():
    from protstruc_amd import _lib, build
    build.build(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def pdb_case(name, seed):
    """the search case of the StructureBatch methods on a PDB file (a, b, mask, l_norm, objectives)"""
    from protstruc_amd import pdb
    xyz, mask = pdb.read_batch([os.path.join(GOLDEN_DIR, name + ".pdb")])[:2]
    return R.structure_case(xyz[0].numpy(), mask[0].numpy(), seed)


# ---- the header (tests/test_api_families.py holds it to the binding and the library) ------------------------------------------
def test_the_entry_points_and_constants_of_the_header():
    from protstruc_amd import _lib, build
    assert declared_symbols(HEADER) == sorted(LAUNCHERS + HOST_FUNCTIONS)
    assert {"superpose.hip", "kabsch_solve.hpp"} <= {os.path.basename(d) for d in build._deps()}
    defined = macros(HEADER)
    for macro, value in (("MAX_POINTS", R.MAX_POINTS), ("MAX_SEEDS", R.MAX_SEEDS), ("MAX_ITERATIONS", R.MAX_ITERATIONS),
                         ("MAX_DOUBLINGS", R.MAX_DOUBLINGS), ("MAX_OBJECTIVES", R.MAX_OBJECTIVES), ("TM", R.TM), ("COUNT", R.COUNT)):
        assert defined["PS_SUPERPOSE_" + macro] == value, macro
    body = re.search(r"typedef struct ps_superpose_objective \{(.*?)\} ps_superpose_objective;", header_text(HEADER), flags=re.S).group(1)
    assert re.findall(r"(int|float)\s+(\w+)\s*;", body) == [("int", "kind"), ("float", "param")]
    assert [f for f, _ in _lib.SuperposeObjective._fields_] == ["kind", "param"] and ctypes.sizeof(_lib.SuperposeObjective) == 8


# ---- the seed table --------------------------------------------------------------------------------------------------------------
def test_seed_table_of_the_library_is_the_restatement(lib):
    start, length = ctypes.c_int(), ctypes.c_int()
    at, ln = ctypes.byref(start), ctypes.byref(length)      # every pointer parameter is bound as c_void_p: by reference, spelled out
    most = 0
    for n in range(R.MAX_POINTS + 1):
        want = R.seed_table(n)
        assert lib.ps_superpose_seed_count(n) == len(want) <= R.MAX_SEEDS, n
        most = max(most, len(want))
        if n:
            assert want[0] == (0, n) and want[-1][0] + want[-1][1] == n, f"n = {n}: the first fragment is everything, the last ends at n"
            assert all(0 <= s and s + L <= n and L >= min(n, 4) for s, L in want) and len(set(want)) == len(want), n
        for s, frag in enumerate(want):
            assert lib.ps_superpose_seed(n, s, at, ln) == 0 and (start.value, length.value) == frag, (n, s)
        assert lib.ps_superpose_seed(n, len(want), at, ln) == 1 and lib.ps_superpose_seed(n, -1, at, ln) == 1, n
        assert lib.ps_superpose_workspace_floats(3, max(n, 1), 2) == 3 * 2 * 16 * most or n == 0, n
    assert lib.ps_superpose_seed_count(-1) == 0 and lib.ps_superpose_seed_count(R.MAX_POINTS + 1) == 0
    assert R.seed_table(5) == [(0, 5), (0, 4), (1, 4)] and R.seed_table(3) == [(0, 3)] and R.seed_table(0) == []
    assert R.seed_table(16) == [(0, 16), (0, 8), (4, 8), (8, 8)] + [(s, 4) for s in range(0, 12, 2)] + [(12, 4)]
    assert len(R.seed_table(2048)) == 1024 and 400 < len(R.seed_table(512)) < 600


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def objectives(*pairs):
    from protstruc_amd import _lib
    return (_lib.SuperposeObjective * len(pairs))(*[_lib.SuperposeObjective(k, p) for k, p in pairs])


def test_arguments_are_checked_before_any_launch(lib):
    """hipErrorInvalidValue (1) without touching a device; B = 0 returns 0 (the device pointers are never dereferenced)."""
    fake = ctypes.c_void_p(0x1000)
    good = objectives((0, 3.5), (1, 1.0))

    def fit(a=fake, b=fake, R_=fake, t=fake, rmsd=fake, wsum=fake, B=1, M=4, shared=0):
        return lib.ps_superpose_f32(a, b, None, None, R_, t, rmsd, wsum, B, M, shared, None)

    def back(a=fake, b=fake, R_=fake, t=fake, rmsd=fake, wsum=fake, g=fake, ga=fake, gb=fake, B=1, M=4, shared=0):
        return lib.ps_superpose_backward_f32(a, b, None, None, R_, t, rmsd, wsum, g, ga, gb, B, M, shared, None)

    def search(a=fake, b=fake, l_norm=fake, obj=good, n_obj=2, ws=fake, score=fake, R_=fake, t=fake, B=1, M=4):
        return lib.ps_superpose_search_f32(a, b, None, l_norm, obj, n_obj, ws, score, R_, t, B, M, None)

    assert fit(B=0) == 0 and back(B=0) == 0 and back(B=0, shared=1, gb=None) == 0 and search(B=0) == 0
    for bad in (dict(a=None), dict(b=None), dict(R_=None), dict(t=None), dict(rmsd=None), dict(wsum=None), dict(B=-1), dict(B=65536),
                dict(M=0), dict(M=-3), dict(B=0, M=0)):
        assert fit(**bad) == 1, bad
        assert back(**bad) == 1, bad
    for bad in (dict(g=None), dict(ga=None), dict(gb=None), dict(shared=1), dict(B=0, shared=1)):
        assert back(**bad) == 1, bad          # a shared target is a constant: its gradient buffer is refused
    for bad in (dict(a=None), dict(b=None), dict(l_norm=None), dict(ws=None), dict(score=None), dict(R_=None), dict(t=None),
                dict(obj=None), dict(n_obj=0), dict(n_obj=9), dict(M=0), dict(M=2049), dict(B=65536), dict(B=-1),
                dict(obj=objectives((2, 1.0), (1, 1.0))), dict(obj=objectives((-1, 1.0), (1, 1.0))),
                dict(obj=objectives((0, 0.0), (1, 1.0))), dict(obj=objectives((0, 1.0), (1, -1.0))),
                dict(obj=objectives((0, math.nan), (1, 1.0))), dict(obj=objectives((0, 1.0), (1, math.inf))),
                dict(B=0, n_obj=9), dict(B=0, M=2049), dict(B=0, obj=objectives((2, 1.0), (1, 1.0)))):
        assert search(**bad) == 1, bad
    assert search(B=0, M=2048, n_obj=8, obj=objectives(*[(k % 2, 1.0 + k) for k in range(8)])) == 0
    assert lib.ps_superpose_workspace_floats(1, 2049, 1) == -1 and lib.ps_superpose_workspace_floats(1, 4, 9) == -1
    assert lib.ps_superpose_workspace_floats(0, 4, 1) == 0 and lib.ps_superpose_workspace_floats(65535, 5, 6) == 65535 * 6 * 3 * 16


def test_shape_checks_of_the_shell():
    from protstruc_amd import geometry, ops
    B, M = 2, 7
    a, mask = torch.zeros(B, M, 3), torch.ones(B, M, dtype=torch.bool)
    check = ops.check_superpose_shapes
    assert check(a, a.double(), torch.ones(B, M), mask.float(), torch.ones(B), torch.ones(B)) == (B, M, False)
    assert check(a, a[:1]) == (B, M, True)
    for bad, message in ((dict(a=torch.zeros(B, M)), "a must have shape"), (dict(a=torch.zeros(B, M, 2)), "a must have shape"),
                         (dict(a=a.long()), "floating-point"), (dict(b=a[:, :4]), "b must have shape"), (dict(b=a.long()), "floating-point"),
                         (dict(a=torch.zeros(B, 0, 3), b=torch.zeros(B, 0, 3)), "points per structure"),
                         (dict(weight=torch.ones(B, M - 1)), "weight must have shape"), (dict(weight=torch.ones(B, M).long()), "floating-point"),
                         (dict(mask=mask[:1]), "mask must have shape"), (dict(grad_rmsd=torch.ones(B, 1)), "grad_rmsd must have shape"),
                         (dict(l_norm=torch.ones(B + 1)), "l_norm must have shape"),
                         (dict(a=torch.zeros(B, 2049, 3), b=torch.zeros(B, 2049, 3), max_points=2048), "points per structure")):
        with pytest.raises(ValueError, match=message):
            check(**{**dict(a=a, b=a), **bad})
    for bad, message in (([], "objectives, got 0"), ([(0, 1.0)] * 9, "objectives, got 9"), ([(2, 1.0)], "kind"), ([(0, 0.0)], "positive"),
                         ([(1, math.nan)], "positive")):
        with pytest.raises(ValueError, match=message):
            ops._check_objectives(bad)
    for call in (lambda: ops.superpose(a, a), lambda: ops.superpose_search(a, a, mask, torch.ones(B), [(0, 1.0)]),
                 lambda: geometry.superposition_rmsd(a, a), lambda: geometry.tm_score(a, a, d0=2.0), lambda: geometry.gdt_ts(a, a)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_tm_d0_of_the_shell_is_the_yardsticks():
    from protstruc_amd import geometry
    for L in (1, 15, 19, 21, 22, 23, 50, 100, 130, 232, 500, 2048):
        assert geometry.tm_d0(L) == R.tm_d0(L), L
        assert abs(float(geometry.tm_d0(torch.tensor([float(L)]))[0]) - R.tm_d0(L)) <= 1e-12, L
    assert geometry.GDT_TS_CUTOFFS == (1.0, 2.0, 4.0, 8.0) and geometry.GDT_HA_CUTOFFS == (0.5, 1.0, 2.0, 4.0)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def test_yardstick_known_answers():
    assert all(R.tm_d0(L) == 0.5 for L in (0, 1, 15, 21)) and abs(R.tm_d0(22) - 0.5720) < 1e-4
    assert abs(R.tm_d0(100) - (1.24 * 85.0 ** (1.0 / 3.0) - 1.8)) < 1e-12 and abs(R.tm_d0(100) - 3.6520) < 1e-3
    assert R.tm_d0(23) == max(0.5, 1.24 * 2.0 - 1.8) and R.tm_d0(30) > 0.5
    a, _ = R.model_and_target(40, 77)
    same = R.search(a, a.copy(), None, 40.0, R.six_objectives(40.0))
    assert (same.score == 1.0).all() and (same.seed == 0).all(), "identical clouds: TM = 1 and every GDT fraction = 1, at seed 0"
    moved = R.f32(a @ align_ref.rotation(np.random.default_rng(1)).T + np.array([3.0, -4.0, 5.0]))
    rigid = R.search(a, moved, None, 40.0, R.six_objectives(40.0))
    assert (rigid.score[1:] == 1.0).all() and 1.0 - 1e-9 < rigid.score[0] <= 1.0
    # the RMSD is align_ref's at align_ref's transform
    for n, seed in ((1, 0), (2, 1), (3, 2), (50, 3), (257, 4)):
        a, b = align_ref.cloud(n, seed=seed)
        k, f = align_ref.kabsch64(a, b), R.superpose(a, b)
        assert abs(f.rmsd - k.rmsd) <= 1e-12 * max(1.0, k.rmsd) and abs(f.rmsd - align_ref.rmsd64(k.R, k.t, a, b)) <= 1e-12 * max(1.0, k.rmsd)
        if align_ref.is_unique(k):
            assert np.abs(f.R - k.R).max() <= 1e-12 and np.abs(f.t - k.t).max() <= 1e-10
    # weights: a weight of 2 is the point twice, a weight of 0 is the point left out
    a, b = align_ref.cloud(20, seed=5)
    w = np.ones(20)
    w[3], w[7] = 2.0, 0.0
    twice = R.superpose(np.concatenate([a[:7], a[8:], a[3:4]]), np.concatenate([b[:7], b[8:], b[3:4]]))
    f = R.superpose(a, b, w)
    assert abs(f.rmsd - twice.rmsd) <= 1e-12 and np.abs(f.R - twice.R).max() <= 1e-12 and f.wsum == 20.0
    empty = R.superpose(a, b, np.zeros(20))
    assert np.isnan(empty.rmsd) and np.isnan(empty.R).all() and empty.wsum == 0.0


def test_yardstick_gradient_against_torch_autograd():
    a, b = align_ref.cloud(30, seed=6)
    w = np.random.default_rng(7).uniform(0.5, 2.0, 30)
    w[[2, 11]] = 0.0
    x, y = torch.from_numpy(a).double().requires_grad_(True), torch.from_numpy(b).double().requires_grad_(True)
    svd_rmsd(x, y, torch.from_numpy(w)).backward()
    ga, gb, terms = R.superpose_grad(a, b, w)
    assert np.abs(x.grad.numpy() - ga).max() <= 1e-12 and np.abs(y.grad.numpy() - gb).max() <= 1e-12
    assert (ga[[2, 11]] == 0).all() and (terms >= np.abs(ga)).all() and np.abs(ga).max() > 1e-3


def svd_rmsd(x, y, w):
    """the RMSD after the weighted SVD Kabsch fit as a differentiable torch float64 function (n,3), (n,3), (n,)"""
    W = w.sum()
    cx, cy = (w[:, None] * x).sum(0) / W, (w[:, None] * y).sum(0) / W
    H = ((x - cx) * w[:, None]).T @ (y - cy)
    U, _, Vt = torch.linalg.svd(H)
    d = torch.sign(torch.linalg.det(Vt.T @ U.T))
    Rm = Vt.T @ torch.diag(torch.stack([torch.ones_like(d), torch.ones_like(d), d])) @ U.T
    e = (x - cx) @ Rm.T - (y - cy)
    return ((w * (e ** 2).sum(-1)).sum() / W).sqrt()


def test_two_domains_case_is_what_the_gpu_test_needs():
    """the search finds domain 1: TM above the sum over domain 1 at its own fit, the 1 A fraction 78 / 130, both strictly
    above the all-points fit; and TM is never below the all-points fit"""
    a, b = R.two_domains()
    obj = R.six_objectives(130.0)
    got = R.search(a, b, None, 130.0, obj)
    A, Bt = align_ref.f64(a), align_ref.f64(b)
    R1, t1 = R.fit(A[:78], Bt[:78])
    d0sq = obj[0][1] ** 2
    domain = float((1.0 / (1.0 + R.dist2(R1, t1, A[:78], Bt[:78]) / d0sq)).sum() / 130.0)
    Rall, tall = R.fit(A, Bt)
    assert got.score[0] >= domain - 1e-6 and got.score[2] >= 78 / 130 - 1e-6
    assert got.score[0] > R.score_at(Rall, tall, a, b, None, 130.0, *obj[0]) + 0.05
    assert got.score[2] > R.score_at(Rall, tall, a, b, None, 130.0, *obj[2]) + 0.05


# ---- the knife-edge guard --------------------------------------------------------------------------------------------------------
def all_search_cases():
    cases = R.search_cases()
    for name, seed in PDB_CASES:
        cases[name] = pdb_case(name, seed)
    return cases


@pytest.mark.parametrize("name", list(R.search_cases()) + [name for name, _ in PDB_CASES])
def test_no_search_case_is_on_a_knife_edge(name):
    """Forwards and reversed sums agree in every score to 1e-9 and in the winning seed; and the winner's transform rounded to
    float32, as the kernel returns it, reproduces every score to 1e-7 -- no point sits on a cutoff closer than that rounding
    moves it.  A case that fails is replaced, never tolerated."""
    a, b, mask, l_norm, obj = all_search_cases()[name]
    forwards, backwards = R.search(a, b, mask, l_norm, obj), R.search(a, b, mask, l_norm, obj, reverse=True)
    assert np.abs(forwards.score - backwards.score).max() <= 1e-9, (forwards.score, backwards.score)
    assert np.array_equal(forwards.seed, backwards.seed), (forwards.seed, backwards.seed)
    if (forwards.seed >= 0).all():
        for o, (kind, param) in enumerate(obj):
            rounded = R.score_at(R.f32(forwards.R[o]), R.f32(forwards.t[o]), a, b, mask, l_norm, kind, param)
            assert abs(rounded - forwards.score[o]) <= 1e-7, (o, rounded, forwards.score[o])
