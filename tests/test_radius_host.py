"""The radius graph without a GPU: the yardstick (tests/radius_ref.py) held to K24's, the box test the kernels run
(csrc/radius_box.hpp, compiled for the host) held to "never drops a block that holds a neighbour pair" on adversarial
blocks, the conditions that keep the GPU cases of tests/test_gpu_radius.py from passing vacuously, every refusal of
``ops.check_radius_graph_shapes`` with its message, and the radius graph's own entry points, arguments and sources (what
every family shares is in tests/test_api_families.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from protstruc_amd import _lib, build, ops
from tests import knn_ref, radius_ref as R
from tests.c_headers import macros

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "protstruc_graph.h"


# ---- the restatement against K24's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", R.CUTOFFS)
@pytest.mark.parametrize("M", (65, 257, 1000))
def test_rows_of_at_most_64_are_the_rows_of_k24(M, cutoff):
    """wherever a row has <= 64 entries it is knn_ref's row at k = 64 with the same arguments, as a set, with the same bits
    in dist -- with and without keys, with and without the point itself"""
    case = R.chain(M)
    short = 0
    for kw in ({}, {"exclude": case.key}, {"include_self": True}):
        ref = R.batch(case.x, cutoff, case.mask, **kw)
        knn = knn_ref.batch(case.x, 64, case.mask, cutoff=cutoff, **kw)
        rows = R.rows_of(ref)
        assert len(rows) == 3 * M
        for b in range(3):
            for q in range(M):
                col, dist = rows[b * M + q]
                assert np.array_equal(col, np.sort(col)) and len(col) == ref.count[b, q]
                if len(col) > 64:
                    assert knn[b].count[q] == 64
                    continue
                short += 1
                n = knn[b].count[q]
                order = np.argsort(knn[b].idx[q, :n], kind="stable")
                assert n == len(col) and np.array_equal(knn[b].idx[q, :n][order], col)
                assert np.array_equal(knn[b].dist[q, :n][order].view(np.int32), dist.view(np.int32))
    assert short > M


# ---- the conservative test: the kernel's own code on the host --------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_program(tmp_path_factory):
    compiler = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert compiler is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("radius_box") / "radius_box_host")
    subprocess.run([compiler, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "protstruc_amd", "csrc"),
                    os.path.join(ROOT, "tools", "radius_box_host.cpp"), "-o", exe], check=True)
    return exe


def run_boxes(exe, cases):
    """[(cutoff, A (nA,3) float32, B (nB,3) float32)] -> [(dropped, G bits, bound bits, A.n, B.n)] from the host program"""
    lines = []
    for cutoff, a, b in cases:
        words = [int(np.float32(cutoff).view(np.uint32)), len(a), len(b)]
        words += [int(v) for v in np.asarray(a, np.float32).reshape(-1).view(np.uint32)]
        words += [int(v) for v in np.asarray(b, np.float32).reshape(-1).view(np.uint32)]
        lines.append(" ".join(map(str, words)))
    done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = [tuple(int(w) for w in line.split()) for line in done.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def step(v, ulps):
    """the float32 ``ulps`` representable values above (below, if negative) ``v``"""
    v = np.float32(v)
    for _ in range(abs(ulps)):
        v = np.nextafter(v, np.float32(np.inf if ulps > 0 else -np.inf))
    return v


def adversarial_cases():
    """Pairs of blocks whose boxes are a cutoff apart exactly, 1 and 2 ulps more and less -- inside the margin of the test --
    and 64 and 1024 ulps more and less -- outside it, so that blocks are dropped too --: along one axis (a point of
    each block faces the other, so the closest pair is as far apart as the boxes) and along the diagonal; coordinates of
    the size of 1, near 1e4, near 1e-20 and subnormal; blocks of 1, 5 and 64 points."""
    rng = np.random.default_rng(17)
    cases = []
    for scale, origin in ((1.0, 0.0), (1.0, 1.0e4), (1.0e-20, 0.0), (1.0e-20, 3.0e-20), (1.0e-41, 0.0), (1.0e-39, 5.0e-39)):
        for n in (1, 5, 64):
            for kind in ("axis", "diagonal"):
                for ulps in (-1024, -64, -2, -1, 0, 1, 2, 64, 1024):
                    cutoff = np.float32(scale * rng.uniform(2.0, 12.0))
                    if not cutoff > 0:
                        continue
                    a = (origin + scale * rng.uniform(-20.0, 0.0, size=(n, 3))).astype(np.float32)
                    b = (origin + scale * rng.uniform(-20.0, 0.0, size=(n, 3))).astype(np.float32)
                    a[0] = a.max(axis=0)                                          # a corner point: hi of A
                    g = cutoff if kind == "axis" else np.float32(np.float64(cutoff) / np.sqrt(3.0))
                    shift = np.array([g, 0, 0] if kind == "axis" else [g, g, g], dtype=np.float32)
                    b = (b - b.min(axis=0) + a[0]).astype(np.float32)             # lo of B at hi of A ...
                    b = (b + shift).astype(np.float32)                            # ... and then the gap
                    b[0] = b.min(axis=0)                                          # the corner point facing a[0]
                    b[0, 0] = step(b[0, 0], ulps)
                    if ulps < 0:
                        b[:, 0] = np.maximum(b[:, 0], b[0, 0])
                    cases.append((cutoff, a, b))
    # the gap is the cutoff EXACTLY, in exactly representable numbers
    for cutoff, lo in ((3.0, 0.0), (0.5, 1024.0), (4.0, 16384.0), (2.0 ** -70, 2.0 ** -60), (2.0 ** -140, 0.0)):
        for ulps in (0, 1, -1):
            a = np.array([[lo, 1.0, 2.0]], dtype=np.float32)
            b = np.array([[step(np.float32(lo) + np.float32(cutoff), ulps), 1.0, 2.0]], dtype=np.float32)
            cases.append((np.float32(cutoff), a, b))
    return cases


def test_the_box_test_never_drops_a_neighbour_pair(box_program):
    cases = adversarial_cases()
    got = run_boxes(box_program, cases)
    n_dropped = n_kept_with_pair = exact = 0
    for (cutoff, a, b), (drop, G_bits, bound_bits, an, bn) in zip(cases, got):
        near, d2 = R.near_matrix(b, float(cutoff), queries=a)
        box_a, box_b = R.box(a), R.box(b)
        assert (an, bn) == (box_a[2], box_b[2]) == (len(a), len(b))
        # the program is the restatement, bit for bit
        assert bound_bits == int(R.reject_above(cutoff).view(np.uint32)) and G_bits == int(R.gap2(box_a, box_b).view(np.uint32))
        assert bool(drop) == R.dropped(box_a, box_b, cutoff)
        assert not (drop and near.any()), (float(cutoff), a[0], b[0], float(d2.min()))
        n_dropped += drop
        n_kept_with_pair += bool(near.any())
        C2 = np.float64(cutoff) * np.float64(cutoff)
        exact += int((d2 == C2).any())
    assert n_dropped > 20 and n_kept_with_pair > 20, (n_dropped, n_kept_with_pair)      # both outcomes are exercised
    assert exact >= 5, "no case has a pair exactly at the cutoff"


def test_pairs_exactly_at_the_cutoff_are_kept_and_the_next_float_decides_in_double(box_program):
    """the smallest trap of the GPU tests: 64 copies of the origin against 64 copies of (c, 0, 0)"""
    for cutoff in (3.0, 4.1, 7.3e-21, 1.0e4):
        c = np.float32(cutoff)
        at = R.trap(c)
        beyond = R.trap(np.nextafter(c, np.float32(np.inf)))
        (drop_at, *_), (drop_beyond, *_) = run_boxes(box_program, [(c, at.x[0, :64], at.x[0, 64:]), (c, beyond.x[0, :64], beyond.x[0, 64:])])
        # a point's 63 copies in its own block are always neighbours; the 64 of the other block are at d2 == C2 exactly
        assert not drop_at and R.radius(at.x[0], float(c)).count.tolist() == [127] * 128
        # whatever the box test says one float further (it may keep the block), the double test drops the pairs
        assert drop_beyond in (0, 1) and R.radius(beyond.x[0], float(c)).count.tolist() == [63] * 128


def test_empty_blocks_are_always_dropped(box_program):
    nan = np.full((3, 3), np.nan, dtype=np.float32)
    inf = np.array([[np.inf, 0, 0], [0, -np.inf, 0]], dtype=np.float32)
    point = np.zeros((1, 3), dtype=np.float32)
    none = np.zeros((0, 3), dtype=np.float32)
    got = run_boxes(box_program, [(np.float32(1e30), point, none), (np.float32(1e30), point, nan), (np.float32(1e30), point, inf),
                                  (np.float32(3e38), point, none), (np.float32(1e30), point, point)])
    assert [g[0] for g in got] == [1, 1, 1, 1, 0] and [g[4] for g in got] == [0, 0, 0, 0, 1]
    # a box takes the finite points of a block and leaves the others out
    mixed = np.concatenate([nan, np.array([[1, 2, 3], [-1, 5, 0]], dtype=np.float32), inf])
    (drop, _, _, _, n), = run_boxes(box_program, [(np.float32(2.0), point, mixed)])
    assert (drop, n) == (0, 2)


# ---- the conditions on the GPU cases -----------------------------------------------------------------------------------------------
def test_the_chain_family_is_not_vacuous():
    most, n_dropped, n_kept = R.assert_family("chains", [(R.chain(M), c) for M in R.SIZES for c in R.CUTOFFS])
    print("chains: longest row", most, "block pairs dropped", n_dropped, "kept", n_kept)
    for M in R.SIZES:
        case = R.chain(M)
        assert not case.mask[1].any() and np.isnan(case.x[1]).all() and case.mask[2].all()
        if M > 8:
            assert 0.3 < 1.0 - case.mask[0].mean() < 0.6 and np.isnan(case.x[0][~case.mask[0]]).all()


def test_the_permuted_family_drops_nothing():
    case = R.permuted()
    most, n_dropped, _ = R.assert_family("permuted", [(Case1(case, 1), 12.0)], may_drop=False)
    assert most > 64 and n_dropped == 0
    R.assert_family("the chain it permutes", [(Case1(case, 0), 12.0)])


def Case1(case, b):
    return R.Case(case.x[b:b + 1], None if case.mask is None else case.mask[b:b + 1])


def test_the_cluster_family_drops_nearly_everything():
    case = R.clusters()
    R.assert_family("clusters", [(case, 12.0)])
    drop, holds = R.block_decisions(case.x[0], 12.0, case.mask[0])
    # three blocks per cluster: every pair of blocks across the two clusters is dropped, and only those
    assert drop.shape == (6, 6) and drop[:3, 3:].all() and drop[3:, :3].all() and drop.mean() == 0.5 and not (drop & holds).any()


def test_the_lattice_family_has_pairs_exactly_at_the_cutoff():
    case = R.lattice()
    R.assert_family("lattice", [(case, R.LATTICE_CUTOFF)])
    near, d2 = R.near_matrix(case.x[0], R.LATTICE_CUTOFF)
    C2 = np.float64(np.float32(R.LATTICE_CUTOFF)) ** 2
    assert C2 == 9.0 and int(((d2 == C2) & near).sum()) >= 100
    drop, holds = R.block_decisions(case.x[0], R.LATTICE_CUTOFF)
    # block t is the plane x = t: planes three apart are kept (they hold the pairs at exactly the cutoff), four apart dropped
    assert all(not drop[t, t + 3] and holds[t, t + 3] and drop[t, t + 4] for t in range(4))


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_check_radius_graph_shapes():
    x, q = torch.zeros(2, 5, 3), torch.zeros(2, 4, 3)
    m, k = torch.ones(2, 5, dtype=torch.bool), torch.zeros(2, 5, dtype=torch.int32)
    qm, qk = torch.ones(2, 4, dtype=torch.bool), torch.zeros(2, 4, dtype=torch.int32)
    check = ops.check_radius_graph_shapes
    assert check(x, 4.0, m, exclude=k) == (2, 5, 5) and check(x, 4.0, m, q, qm, k, qk, max_edges=0) == (2, 5, 4)
    refusals = [
        (dict(points=torch.zeros(2, 5)), "points must have shape (batch, points, 3), got (2, 5)"),
        (dict(points=torch.zeros(65536, 1, 3)), "at most 65535 structures per call, got 65536"),
        (dict(points=torch.zeros(2, 5, 3, dtype=torch.int32)), "points must be a floating-point tensor, got torch.int32"),
        (dict(cutoff=0.0), "cutoff must be positive and finite, got 0.0"),
        (dict(cutoff=-1.0), "cutoff must be positive and finite, got -1.0"),
        (dict(cutoff=float("inf")), "cutoff must be positive and finite, got inf"),
        (dict(cutoff=float("nan")), "cutoff must be positive and finite, got nan"),
        (dict(max_edges=-1), "max_edges must be None or a non-negative integer, got -1"),
        (dict(max_edges=2.0), "max_edges must be None or a non-negative integer, got 2.0"),
        (dict(max_edges=True), "max_edges must be None or a non-negative integer, got True"),
        (dict(point_mask=torch.ones(2, 4)), "point_mask must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
        (dict(exclude=torch.zeros(2, 6, dtype=torch.int32)), "exclude must have shape (2, 5) to match points (2, 5, 3), got (2, 6)"),
        (dict(exclude=torch.zeros(2, 5)), "exclude must be an integer tensor, got torch.float32"),
        (dict(query_mask=qm), "query_mask needs queries: in the self graph the points' own mask and keys are used"),
        (dict(query_exclude=qk), "query_exclude needs queries: in the self graph the points' own mask and keys are used"),
        (dict(queries=torch.zeros(3, 4, 3)), "queries must have shape (2, queries, 3) to match points (2, 5, 3), got (3, 4, 3)"),
        (dict(queries=torch.zeros(2, 4, 3, dtype=torch.int64)), "queries must be a floating-point tensor, got torch.int64"),
        (dict(queries=q, query_mask=torch.ones(2, 5)), "query_mask must have shape (2, 4) to match queries (2, 4, 3), got (2, 5)"),
        (dict(queries=q, exclude=k, query_exclude=torch.zeros(2, 4)), "query_exclude must be an integer tensor, got torch.float32"),
        (dict(queries=q, exclude=k), "exclude and query_exclude come together: a candidate is skipped where the two keys are equal"),
        (dict(queries=q, query_exclude=qk), "exclude and query_exclude come together: a candidate is skipped where the two keys are equal"),
        (dict(queries=q, include_self=True), "include_self applies to the self graph only (queries=None)"),
    ]
    for changes, message in refusals:
        args = dict(points=x, cutoff=4.0)
        args.update(changes)
        with pytest.raises(ValueError) as info:
            check(**args)
        assert str(info.value) == message, changes
    with pytest.raises(ValueError, match=r"at most 2\^24 points per structure, got 16777217"):
        check(torch.zeros(1, 2 ** 24 + 1, 3, device="meta"), 4.0)
    with pytest.raises(ValueError, match=r"at most 2\^24 queries per structure, got 16777217"):
        check(torch.zeros(1, 2, 3, device="meta"), 4.0, queries=torch.zeros(1, 2 ** 24 + 1, 3, device="meta"))
    with pytest.raises(ValueError, match="`point_mask` lives on meta, the coordinates on cpu"):
        check(x, 4.0, torch.ones(2, 5, device="meta"))
    # K24's words wherever the rule is K24's
    for changes, message in refusals[10:]:
        args = dict(points=x, k=3)
        args.update(changes)
        with pytest.raises(ValueError) as info:
            ops.check_knn_shapes(**args)
        assert str(info.value) == message


def test_the_public_functions_have_the_signatures_of_the_issue():
    import inspect

    from protstruc_amd import StructureBatch, geometry
    want = "(points, cutoff, point_mask=None, *, queries=None, query_mask=None, exclude=None, query_exclude=None, include_self=False, max_edges=None)"
    assert str(inspect.signature(geometry.radius_graph)).split(" ->")[0] == want
    assert list(inspect.signature(ops.radius_graph).parameters)[:9] == list(inspect.signature(geometry.radius_graph).parameters)
    assert geometry.RadiusGraph._fields == ("row_ptr", "col", "dist", "count")
    defaults = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][1:]   # noqa: E731
    assert defaults(StructureBatch.radius_graph) == [("cutoff", 10.0), ("atom", "CA"), ("include_self", False),
                                                     ("other_chains_only", False), ("max_edges", None)]
    assert defaults(StructureBatch.atom_radius_graph) == [("cutoff", 5.0), ("atoms", "all"), ("exclude_same_residue", True),
                                                          ("max_edges", None)]
    assert ops.RADIUS_TILE == macros(HEADER)["PS_RADIUS_TILE"] == R.TILE == 64


# ---- the radius graph's own entry points and sources (what every family shares: tests/test_api_families.py) -------------------------
def test_the_entry_points_and_their_arguments():
    assert sorted(_lib.GRAPH_SIGNATURES) == ["ps_graph_api", "ps_radius_count_f32", "ps_radius_fill_f32",
                                             "ps_radius_tile_boxes_f32"]
    for name in ("ps_radius_tile_boxes_f32", "ps_radius_count_f32", "ps_radius_fill_f32"):
        restype, argtypes = _lib.GRAPH_SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p                # the HIP error; the stream last
    assert _lib.GRAPH_SIGNATURES["ps_radius_fill_f32"][1][9:11] == [ctypes.c_void_p, ctypes.c_longlong]   # row_ptr, max_edges
    assert _lib.GRAPH_SIGNATURES["ps_radius_count_f32"][1][6] is ctypes.c_float


def test_the_library_exports_every_table_and_is_built_from_the_radius_sources():
    build.build(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    tables = ["SIGNATURES"] + [family.signatures for family in _lib.FAMILIES]
    nm = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert set(re.findall(r"\b(ps_[a-z0-9_]+)$", nm, flags=re.M)) == set().union(*(getattr(_lib, t) for t in tables))
    assert all(os.path.dirname(s) == build.CSRC for s in build.sources())
    names = {os.path.basename(d) for d in build._deps()}
    assert {"radius_graph.hip", "radius_box.hpp", "ps_common.hpp", "owner_sweep.hpp", HEADER} <= names
