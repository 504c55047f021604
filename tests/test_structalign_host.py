"""Structure alignment without a GPU: the C header include/protstruc_structalign.h against the binding and the library, the
argument checks of the launchers and of the shell, the yardstick tests/structalign_ref.py against brute force and known
answers, and the knife-edge guard: every alignment case the GPU tests run gives the same map, the same winning start and
the same score whichever way the sums over points are taken."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from tests import structalign_ref as A
from tests.c_headers import declared_symbols, macros

HEADER = "protstruc_structalign.h"
LAUNCHERS = ["ps_ca_secondary_structure_f32", "ps_nw_align_f32", "ps_structure_align_f32"]
HOST_FUNCTIONS = ["ps_structalign_api", "ps_structalign_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    from protstruc_amd import _lib, build
    build.build(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ---- the header (tests/test_api_families.py holds it to the binding and the library) ------------------------------------------
def test_the_entry_points_and_constants_of_the_header(lib):
    from protstruc_amd import build
    assert declared_symbols(HEADER) == sorted(LAUNCHERS + HOST_FUNCTIONS)
    assert lib.ps_superpose_api() == 1, "the alignment is built on this version of the superposition search"
    assert {"protstruc_superpose.h", "struct_align.hip", "superpose.hip", "superpose_chain.hpp"} <= {os.path.basename(d) for d in build._deps()}
    assert macros(HEADER)["PS_STRUCTALIGN_MAX_POINTS"] == A.MAX_POINTS and macros(HEADER)["PS_STRUCTALIGN_MAX_ITERATIONS"] == A.MAX_ITERATIONS


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_any_launch(lib):
    """hipErrorInvalidValue (1) without touching a device; B = 0 returns 0 (the device pointers are never dereferenced)."""
    fake = ctypes.c_void_p(0x1000)

    def dp(score=fake, gap=-0.6, ws=fake, out=fake, n=fake, value=fake, B=1, Ma=4, Mb=5):
        return lib.ps_nw_align_f32(score, None, None, gap, ws, out, n, value, B, Ma, Mb, None)

    def labels(x=fake, out=fake, B=1, M=4):
        return lib.ps_ca_secondary_structure_f32(x, None, out, B, M, None)

    def align(a=fake, b=fake, d0=fake, ws=fake, out=fake, n=fake, score=fake, R=fake, t=fake, pts=fake, start=fake, B=1, Ma=4, Mb=5):
        return lib.ps_structure_align_f32(a, None, b, None, d0, 1, ws, out, n, score, R, t, pts, start, B, Ma, Mb, None)

    assert dp(B=0) == 0 and labels(B=0) == 0 and align(B=0) == 0 and dp(B=0, gap=0.0) == 0
    shapes = (dict(Ma=0), dict(Mb=0), dict(Ma=1025), dict(Mb=1025), dict(B=-1), dict(B=65536), dict(B=0, Ma=1025), dict(B=0, Mb=0))
    for bad in shapes + (dict(score=None), dict(ws=None), dict(out=None), dict(n=None), dict(value=None), dict(gap=0.5),
                         dict(gap=math.nan), dict(gap=-math.inf), dict(B=0, gap=1e-3)):
        assert dp(**bad) == 1, bad
    for bad in shapes + (dict(a=None), dict(b=None), dict(d0=None), dict(ws=None), dict(out=None), dict(n=None), dict(score=None),
                         dict(R=None), dict(t=None), dict(pts=None), dict(start=None)):
        assert align(**bad) == 1, bad
    for bad in (dict(x=None), dict(out=None), dict(M=0), dict(M=1025), dict(B=65536), dict(B=-1)):
        assert labels(**bad) == 1, bad
    size = lib.ps_structalign_workspace_bytes
    assert size(1, 1025, 4) == -1 and size(1, 4, 0) == -1 and size(65536, 4, 4) == -1 and size(0, 4, 4) == 8
    assert size(2, 128, 128) == 2 * size(1, 128, 128) - 8
    # the path words leave LDS for the workspace somewhere between 512 and 1024 points: the size jumps by what they take
    small, large = size(1, 512, 512), size(1, 1024, 1024)
    assert small < 2 * (128 + 4 * 512) + 64 and large >= 2 * 1024 * 17 * 16


def test_shape_checks_of_the_shell():
    from protstruc_amd import geometry, ops
    B, Ma, Mb = 2, 7, 9
    a, b = torch.zeros(B, Ma, 3), torch.zeros(B, Mb, 3)
    ma, mb = torch.ones(B, Ma, dtype=torch.bool), torch.ones(B, Mb)
    check = ops.check_structalign_shapes
    assert check(a, b.double(), ma, mb, torch.ones(B)) == (B, Ma, Mb)
    for bad, message in ((dict(a=torch.zeros(B, Ma)), "a must have shape"), (dict(b=torch.zeros(B, Mb, 2)), "b must have shape"),
                         (dict(a=a.long()), "floating-point"), (dict(b=torch.zeros(B + 1, Mb, 3)), "batch size"),
                         (dict(a=torch.zeros(B, 0, 3)), "points per structure"), (dict(b=torch.zeros(B, 1025, 3)), "points per structure"),
                         (dict(mask_a=ma[:, :3]), "mask_a must have shape"), (dict(mask_b=mb[:1]), "mask_b must have shape"),
                         (dict(d0=torch.ones(B + 1)), "d0 must have shape"), (dict(d0=torch.ones(B).long()), "floating-point")):
        with pytest.raises(ValueError, match=message):
            check(**{**dict(a=a, b=b), **bad})
    score = torch.zeros(B, Ma, Mb)
    for call, message in ((lambda: ops.nw_align(score, 0.5), "gap"), (lambda: ops.nw_align(score, math.nan), "gap"),
                          (lambda: ops.nw_align(score[0], 0.0), "score must have shape"),
                          (lambda: ops.nw_align(score.long(), 0.0), "floating-point"),
                          (lambda: ops.nw_align(torch.zeros(B, 1025, 3), 0.0), "rows and columns"),
                          (lambda: ops.nw_align(score, 0.0, ma[:1]), "mask_a must have shape"),
                          (lambda: ops.ca_secondary_structure(torch.zeros(B, 2000, 3)), "points per structure"),
                          (lambda: ops.ca_secondary_structure(a, ma[:, :3]), "mask must have shape"),
                          (lambda: geometry.structure_alignment(a, b, d0=0.0), "positive"),
                          (lambda: geometry.structure_alignment(a, b, d0=math.inf), "positive")):
        with pytest.raises(ValueError, match=message):
            call()
    for call in (lambda: ops.nw_align(score, -0.6), lambda: ops.ca_secondary_structure(a), lambda: geometry.structure_alignment(a, b, d0=2.0),
                 lambda: ops.structure_align(a, b, ma, mb, torch.ones(B))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def test_the_dp_of_the_yardstick_against_brute_force():
    """On every matrix of up to 5 x 5 multiples of 1/8 (sums are exact): the table filled by anti-diagonals is the table of
    the definition's double loop; the value is what the gap rule pays for the traced alignment; with g = 0 it is the
    maximum over ALL alignments.  With g < 0 the recurrence keeps one state per cell, where an exact maximisation of the
    gap rule would need two (a cell reached diagonally and the same cell reached by a gap): its value never exceeds the
    brute-force maximum and falls short of it on a few matrices (10 of 150 here), which is TM-align's behaviour and part
    of the definition."""
    short = 0
    for na, nb in itertools.product(range(1, 6), repeat=2):
        every = A.all_alignments(na, nb)
        for gap in (0.0, -0.5, -1.0):
            for seed in range(3):
                score = A.dp_scores("eighths", na, nb, seed).astype(np.float64)
                got = A.nw(score, gap)
                by_cell = A.nw(score, gap, A._tables_cell_by_cell)
                assert np.array_equal(got.map, by_cell.map) and got.value == by_cell.value
                pairs = [(i, int(j)) for i, j in enumerate(got.map) if j >= 0]
                assert pairs == sorted(pairs) and len({j for _, j in pairs}) == len(pairs)
                assert A.path_value(score, gap, pairs) == got.value, (na, nb, gap, seed)
                best = max(A.path_value(score, gap, p) for p in every)
                assert got.value <= best and (gap < 0 or got.value == best), (na, nb, gap, seed)
                short += got.value < best
    print(f"the recurrence falls short of the brute-force maximum on {short} of 150 matrices with g < 0")
    for shape in ((63, 64), (130, 257)):
        for family in A.DP_FAMILIES:
            score = A.dp_scores(family, *shape).astype(np.float64)
            fast, slow = A.nw(score, -0.6), A.nw(score, -0.6, A._tables_cell_by_cell)
            assert np.array_equal(fast.map, slow.map) and fast.value == slow.value, (shape, family)
    zeros = A.nw(np.zeros((3, 5)), -1.0)          # pure tie-breaking: d >= h and d >= v takes the diagonal from the corner
    assert list(zeros.map) == [2, 3, 4] and zeros.value == 0.0
    empty = A.nw(np.zeros((0, 4)), 0.0)
    assert empty.n_aligned == 0 and empty.value == 0.0 and empty.map.size == 0


def test_secondary_structure_of_ideal_traces():
    assert list(A.secondary_structure(A.helix(12))) == [0, 0] + [1] * 8 + [0, 0]
    assert list(A.secondary_structure(A.strand(12))) == [0, 0] + [2] * 8 + [0, 0]
    assert list(A.secondary_structure(A.helix(4))) == [0] * 4
    x, mask = A.scatter(A.helix(9), seed=4)
    labels = A.secondary_structure(x, mask)
    assert (labels[~mask] == -1).all() and list(labels[mask]) == [0, 0, 1, 1, 1, 1, 1, 0, 0]
    for name, chain in (("1a3r_HL", "L"), ("1REX", "A")):
        found = np.bincount(A.secondary_structure(A.ca_trace(name, chain)[0]), minlength=4)
        assert found.sum() == A.ca_trace(name, chain)[0].shape[0] and (found[2 if name == "1a3r_HL" else 1] > 20), (name, found)


def test_cut_1rex_recovers_the_known_map():
    a, b, known = A.cut_1rex()
    got = A.restated("cut 1REX")
    assert (known >= 0).sum() == 109 and not ((got.map >= 0) & (got.map != known)).any(), "a wrong pair"
    assert (got.map == known)[known >= 0].sum() >= 105 and got.score > 0.8
    print(f"cut 1REX: {int((got.map == known)[known >= 0].sum())} of 109 pairs recovered, none wrong, score {got.score:.4f}")


def test_the_secondary_structure_start_rescues_v_on_c():
    """1a3r chain L (a V and a C domain) against the C-terminal domain of 5cjx chain H: the threading start alone ends on
    a poor alignment, the secondary-structure start finds the domain.  Measured: 0.3193 without, 0.5281 with (+0.2088)."""
    with_ss, without = A.restated("V on C"), A.restated("V on C, no ss")
    print(f"V on C: {without.score:.4f} without the secondary-structure start, {with_ss.score:.4f} with it "
          f"(+{with_ss.score - without.score:.4f})")
    assert with_ss.start == 1 and without.start == 0
    assert with_ss.score > without.score + 0.1


def test_known_answers_of_the_alignment():
    same = A.restated("itself")
    assert list(same.map) == list(range(115)) and abs(same.score - 1.0) <= 1e-12 and same.start == 0
    for n in range(6):
        for name in (f"{n} on 40", f"40 on {n}"):
            got = A.restated(name)
            assert got.n_aligned == n and min(got.n_a, got.n_b) == n, name
            if n >= 4:        # enough points to tell where in the chain they came from (its points 17 ..)
                hit = got.map[got.map >= 0]
                assert (np.diff(hit) == 1).all() and (hit[0] == 17 or np.flatnonzero(got.map >= 0)[0] == 17), name
            elif n == 0:
                assert got.score == 0.0 and np.isnan(got.R).all()


# ---- the knife-edge guard --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.alignment_cases()))
def test_no_alignment_case_is_on_a_knife_edge(name):
    """Forwards and reversed sums give the same map and the same winning start, and S within 1e-12; the threading start
    alone too, since the GPU tests compare against it.  A case that fails is replaced, never tolerated."""
    c = A.alignment_cases()[name]
    forwards, backwards = A.restated(name), A.restated(name, reverse=True)
    assert np.array_equal(forwards.map, backwards.map) and forwards.start == backwards.start
    assert abs(forwards.S - backwards.S) <= 1e-12, (forwards.S, backwards.S)
    assert forwards.passes == backwards.passes
    one = [A.align(c.a, c.b, c.mask_a, c.mask_b, c.d0, c.use_ss, reverse, starts=(0,)) for reverse in (False, True)]
    assert np.array_equal(one[0].map, one[1].map) and abs(one[0].S - one[1].S) <= 1e-12 and forwards.S >= one[0].S
    # the map lands on unmasked slots and is strictly increasing
    hit = forwards.map[forwards.map >= 0]
    assert (np.diff(hit) > 0).all() and forwards.n_aligned == hit.size
    if c.mask_a is not None:
        assert (forwards.map[~c.mask_a] == -1).all()
    if c.mask_b is not None:
        assert c.mask_b[hit].all()
