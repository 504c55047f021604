"""The structure-alignment kernels on the GPU (K41 - K44) against tests/structalign_ref.py, the float64 restatement of
include/protstruc_structalign.h: the DP and the labels for equality, the alignment for the same map, the same winning start
and the score on cases that tests/test_structalign_host.py has shown to be off every knife edge; properties that need no
restatement; and, since include/protstruc_structalign.h is not in the case table of tests/launch_cases.py, this file also
holds the three launchers to the launch contract: the caller's stream, capture, four threads, the batch limit."""
import functools
import os
import threading

import numpy as np
import pytest
import torch

from tests import align_ref
from tests import structalign_ref as A
from tests.launch_cases import Case, on_device
from tests.test_gpu_closest import carve
from tests.test_gpu_launch_contract import (SENTINEL, SLEEP_CYCLES, assert_all_same, assert_batch_of_65535_repeats_the_three,
                                            raw, same, side_stream_beside_the_default_stream)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
SCORE_TOL = 1e-6          # what tests/test_gpu_superpose.py holds search scores and score_at to


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


# ---- K41 -------------------------------------------------------------------------------------------------------------------------
def assert_dp(pkg, scores, gap, masks, what):
    """one launch over the batch ``scores`` (B,Ma,Mb): map, n_aligned and the bits of value are the restatement's"""
    mask_a = None if masks is None else np.stack([m[0] for m in masks])
    mask_b = None if masks is None else np.stack([m[1] for m in masks])
    got_map, got_n, got_value = (host(t) for t in pkg.ops.nw_align(dev(scores), gap, dev(mask_a), dev(mask_b)))
    assert got_map.dtype == np.int32 and got_n.dtype == np.int32 and got_value.dtype == np.float32
    for s in range(scores.shape[0]):
        want = A.nw_slots(scores[s], float(np.float32(gap)), None if masks is None else masks[s][0], None if masks is None else masks[s][1])
        assert np.array_equal(got_map[s], want.map), f"{what}, structure {s}: the map differs"
        assert got_n[s] == want.n_aligned, (what, s)
        assert got_value[s].view(np.int32) == np.float32(want.value).view(np.int32), (what, s, got_value[s], want.value)


@pytest.mark.parametrize("shape", A.DP_SHAPES)
def test_dp_against_the_restatement(pkg, shape):
    na, nb = shape
    families = [A.dp_scores(f, na, nb) for f in A.DP_FAMILIES]
    for gap in A.DP_GAPS:
        assert_dp(pkg, np.stack(families), gap, None, f"{shape}, gap {gap}")
    if round(max(na, nb) / 0.55) <= A.MAX_POINTS:          # 45 % of both sides masked over NaN scores
        scattered = [A.dp_scatter(f, seed=k) for k, f in enumerate(families)]
        Ma, Mb = max(s[0].shape[0] for s in scattered), max(s[0].shape[1] for s in scattered)
        scores, masks = np.full((3, Ma, Mb), np.nan, np.float32), []
        for k, (full, ma, mb) in enumerate(scattered):
            scores[k, :full.shape[0], :full.shape[1]] = full
            masks.append((np.pad(ma, (0, Ma - ma.size)), np.pad(mb, (0, Mb - mb.size))))
        for gap in A.DP_GAPS:
            assert_dp(pkg, scores, gap, masks, f"{shape} among masked slots, gap {gap}")


def test_dp_at_the_largest_size_and_in_a_mixed_batch(pkg):
    big = A.dp_scores("eighths", 1024, 1024)[None]
    assert_dp(pkg, big, -0.6, None, "1024 x 1024")
    # 560 x 5 and 5 x 560 points among 1018 slots, the rest masked over NaN
    for na, nb in ((560, 5), (5, 560)):
        full, ma, mb = A.dp_scatter(A.dp_scores("diagonal", na, nb), seed=3)
        assert max(full.shape) == 1018
        assert_dp(pkg, full[None], -1.0, [(ma, mb)], f"{na} x {nb} among masked slots")
    # a batch that mixes sizes: (130, 100), (63, 64) and (1, 7) points among 140 x 140 slots, and a structure without points
    M = 140
    scores, masks = np.full((4, M, M), np.nan, np.float32), []
    for k, (na, nb) in enumerate(((130, 100), (63, 64), (1, 7), (0, 9))):
        ma, mb = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
        rng = np.random.default_rng(90 + k)
        ma[np.sort(rng.choice(M, na, replace=False))] = True
        mb[np.sort(rng.choice(M, nb, replace=False))] = True
        scores[k][np.ix_(np.flatnonzero(ma), np.flatnonzero(mb))] = A.dp_scores("eighths", na, nb, seed=k)
        masks.append((ma, mb))
    for gap in A.DP_GAPS:
        assert_dp(pkg, scores, gap, masks, f"mixed batch, gap {gap}")


# ---- K44 -------------------------------------------------------------------------------------------------------------------------
def test_labels_against_the_restatement(pkg):
    ops = pkg.ops
    traces = [A.helix(30, 1), A.strand(30, 2), np.concatenate([A.helix(14, 3), A.strand(12, 4) + 20.0, A.helix(9, 5) - 15.0]),
              A.helix(4, 6), A.helix(5, 7), A.strand(1, 8)]
    traces += [A.ca_trace(name, chain)[0] for name, chain in (("1a3r_HL", "H"), ("1a3r_HL", "L"), ("5cjx_HL", "H"), ("1REX", "A"),
                                                                    ("15c8_HL", "H"))]
    M = max(t.shape[0] for t in traces)
    x, mask = np.full((len(traces), M, 3), np.nan, np.float32), np.zeros((len(traces), M), dtype=bool)
    for k, t in enumerate(traces):
        x[k, :t.shape[0]], mask[k, :t.shape[0]] = t, True
    got = host(ops.ca_secondary_structure(dev(x), dev(mask)))
    assert got.dtype == np.int8
    for k in range(len(traces)):
        assert np.array_equal(got[k], A.secondary_structure(x[k], mask[k])), k
    assert (got[0][2:28] == 1).all() and (got[1][2:28] == 2).all() and (got[3][:4] == 0).all() and (got[~mask] == -1).all()
    # scattered among masked slots over NaN, and without a mask
    scattered = [A.scatter(t, seed=k) for k, t in enumerate(traces[:3])]
    Ms = max(s[0].shape[0] for s in scattered)
    xs, ms = np.full((3, Ms, 3), np.nan, np.float32), np.zeros((3, Ms), dtype=bool)
    for k, (X, m) in enumerate(scattered):
        xs[k, :X.shape[0]], ms[k, :X.shape[0]] = X, m
    got = host(ops.ca_secondary_structure(dev(xs), dev(ms)))
    for k in range(3):
        assert np.array_equal(got[k], A.secondary_structure(xs[k], ms[k])), k
    whole = A.ca_trace("5cjx_HL", "L")[0]
    assert np.array_equal(host(ops.ca_secondary_structure(dev(whole[None])))[0], A.secondary_structure(whole))


# ---- K42 / K43 -------------------------------------------------------------------------------------------------------------------
FIELDS = ("map", "n_aligned", "score", "R", "t", "n_points", "start")


def run_align(pkg, c):
    out = pkg.ops.structure_align(dev(c.a[None]), dev(c.b[None]), None if c.mask_a is None else dev(c.mask_a[None]),
                                  None if c.mask_b is None else dev(c.mask_b[None]), torch.tensor([c.d0], device="cuda"), c.use_ss)
    return dict(zip(FIELDS, (host(t)[0] for t in out)))


def assert_alignment(got, c, want, what):
    assert got["map"].dtype == np.int32 and got["score"].dtype == np.float32
    assert tuple(got["n_points"]) == (want.n_a, want.n_b), what
    assert np.array_equal(got["map"], want.map), f"{what}: the map differs at {np.flatnonzero(got['map'] != want.map)[:8]}"
    assert got["n_aligned"] == want.n_aligned and got["start"] == want.start, (what, got["n_aligned"], got["start"], want.start)
    if min(want.n_a, want.n_b) == 0:
        assert got["score"] == 0 and np.isnan(got["R"]).all() and np.isnan(got["t"]).all() and (got["map"] == -1).all(), what
        return
    print(f"{what}: search score {float(got['score']):.7f}, restatement {want.score:.7f}")
    assert abs(float(got["score"]) - want.score) <= SCORE_TOL, (what, got["score"], want.score)
    # properties that need no restatement
    hit = got["map"][got["map"] >= 0]
    assert (np.diff(hit) > 0).all() and hit.size == got["n_aligned"]
    if c.mask_a is not None:
        assert (got["map"][~c.mask_a] == -1).all()
    if c.mask_b is not None:
        assert c.mask_b[hit].all()
    again = A.score_of(got["R"], got["t"], c.a, c.b, got["map"], c.d0, min(want.n_a, want.n_b))
    assert abs(again - float(got["score"])) <= SCORE_TOL, f"{what}: the returned transform scores {again}, the score is {got['score']}"
    ortho, det = align_ref.rotation_errors(got["R"].astype(np.float64))
    assert ortho <= align_ref.ORTHO_BOUND and det <= align_ref.DET_BOUND, (what, ortho, det)


@pytest.mark.parametrize("name", list(A.alignment_cases()))
def test_alignment_against_the_restatement(pkg, name):
    c = A.alignment_cases()[name]
    got = run_align(pkg, c)
    assert_alignment(got, c, A.restated(name), name)
    if c.use_ss and name in ("1a3r H on L", "V on C", "cut 1REX", "padded 1"):       # never below the threading start alone
        alone = run_align(pkg, c._replace(use_ss=False))
        assert alone["start"] == 0 and got["score"] >= alone["score"], (name, got["score"], alone["score"])
    if name == "itself":
        assert abs(float(got["score"]) - 1.0) <= SCORE_TOL and list(got["map"]) == list(range(c.a.shape[0]))
    if name == "M=1024":
        from protstruc_amd import _lib
        size = _lib.load().ps_structalign_workspace_bytes
        assert c.a.shape[0] == pkg.ops.STRUCTALIGN_MAX_POINTS and size(1, 1024, 1024) > 2 * 1024 * 17 * 16 > 64 * size(1, 128, 128), \
            "the path words of this shape are meant to live in the workspace"


def test_padded_batch_is_the_alignment_of_its_structures(pkg):
    """three pairs of unequal lengths in one launch, 45 % of the slots masked over NaN, each with its own d0: every
    structure's results are those of its own launch, bit for bit"""
    cases = [A.alignment_cases()[f"padded {k}"] for k in range(3)]
    stack = lambda i: np.stack([c[i] for c in cases])       # noqa: E731
    out = pkg.ops.structure_align(dev(stack(0)), dev(stack(1)), dev(stack(2)), dev(stack(3)),
                                  torch.tensor([c.d0 for c in cases], device="cuda"))
    for k, c in enumerate(cases):
        alone = run_align(pkg, c)
        for field, t in zip(FIELDS, out):
            assert np.array_equal(host(t)[k].view(np.int32), alone[field].view(np.int32)), (k, field)
        assert_alignment(alone, c, A.restated(f"padded {k}"), f"padded {k}")


def test_geometry_function(pkg):
    """the default d0 is tm_d0(min(n_a, n_b)) evaluated on the device; tm_a, tm_b and rmsd are those of the aligned pairs"""
    geometry = pkg.geometry
    c = A.alignment_cases()["padded 0"]
    want = A.restated("padded 0")
    got = geometry.structure_alignment(dev(c.a[None]), dev(c.b[None]), dev(c.mask_a[None]), dev(c.mask_b[None]))
    assert np.array_equal(host(got.map)[0], want.map) and int(got.start) == want.start and int(got.n_aligned) == want.n_aligned
    assert abs(float(got.search_score) - want.score) <= SCORE_TOL
    paired = got.map >= 0
    partner = torch.where(paired[:, :, None], dev(c.b[None])[:, got.map.clamp(min=0).long()[0]], torch.zeros((), device="cuda"))
    tm_b = geometry.tm_score(dev(c.a[None]), partner, paired, float(want.n_b))
    assert same(got.tm_b, tm_b.score) and same(got.rot, tm_b.rot) and 0 < float(got.tm_a) <= 1 and 0 < float(got.tm_b) <= 1
    assert 0 < float(got.rmsd) < 5
    fixed = geometry.structure_alignment(dev(c.a[None]), dev(c.b[None]), dev(c.mask_a[None]), dev(c.mask_b[None]), d0=c.d0)
    assert np.array_equal(host(fixed.map), host(got.map))
    empty = geometry.structure_alignment(dev(c.a[None]), dev(c.b[None]), dev(np.zeros_like(c.mask_a)[None]), dev(c.mask_b[None]))
    assert (host(empty.map) == -1).all() and float(empty.search_score) == 0 and float(empty.tm_b) == 0 and int(empty.n_aligned) == 0


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
    """every input ``off`` bytes past a 16-byte boundary (the masks ``mask_off``), the outputs and the workspace inside
    sentinels: the results of the aligned run through ``ops``, bit for bit, and no sentinel byte changes"""
    from protstruc_amd import _lib
    lib, ops = _lib.load(), pkg.ops
    stream = torch.cuda.current_stream().cuda_stream
    cases = [A.alignment_cases()[f"padded {k}"] for k in range(3)]
    stack = lambda i: dev(np.stack([c[i] for c in cases]))       # noqa: E731
    a, b, ma, mb = stack(0), stack(1), stack(2), stack(3)
    d0 = torch.tensor([c.d0 for c in cases], device="cuda")
    B, Ma, Mb = 3, a.shape[1], b.shape[1]
    want = ops.structure_align(a, b, ma, mb, d0)
    sizes = (B * Ma * 4, B * 4, B * 4, B * 36, B * 12, B * 8, B * 4)
    dtypes = (torch.int32, torch.int32, torch.float32, torch.float32, torch.float32, torch.int32, torch.int32)
    outs = [carve(n, off, dt) for n, dt in zip(sizes, dtypes)]
    n_ws = lib.ps_structalign_workspace_bytes(B, Ma, Mb)
    ws = carve(n_ws, mask_off, torch.uint8)
    ins = (carved(a, off), carved(ma, mask_off, torch.bool), carved(b, off), carved(mb, mask_off, torch.bool), carved(d0, off))
    assert lib.ps_structure_align_f32(*[t.data_ptr() for t in ins], 1, ws[1].data_ptr(), *[o[1].data_ptr() for o in outs], B, Ma, Mb,
                                      stream) == 0
    torch.cuda.synchronize()
    for (buf, view, start), w, n in zip(outs, want, sizes):
        assert same(view.reshape(w.shape), w) and intact(buf, start, n)
    assert intact(ws[0], ws[2], n_ws)
    # the DP and the labels
    score = dev(np.stack([A.dp_scores("eighths", Ma, Mb, seed=k) for k in range(B)]))
    want = ops.nw_align(score, -0.6, ma, mb)
    outs = [carve(n, off, dt) for n, dt in zip((B * Ma * 4, B * 4, B * 4), (torch.int32, torch.int32, torch.float32))]
    ws = carve(n_ws, mask_off, torch.uint8)
    assert lib.ps_nw_align_f32(carved(score, off).data_ptr(), ins[1].data_ptr(), ins[3].data_ptr(), -0.6, ws[1].data_ptr(),
                               *[o[1].data_ptr() for o in outs], B, Ma, Mb, stream) == 0
    torch.cuda.synchronize()
    for (buf, view, start), w, n in zip(outs, want, (B * Ma * 4, B * 4, B * 4)):
        assert same(view.reshape(w.shape), w) and intact(buf, start, n)
    assert intact(ws[0], ws[2], n_ws)
    want = ops.ca_secondary_structure(a, ma)
    buf, view, start = carve(B * Ma, mask_off, torch.int8)
    assert lib.ps_ca_secondary_structure_f32(ins[0].data_ptr(), ins[1].data_ptr(), view.data_ptr(), B, Ma, stream) == 0
    torch.cuda.synchronize()
    assert same(view.reshape(B, Ma), want) and intact(buf, start, B * Ma)


def test_repeatability(pkg):
    c = A.alignment_cases()["5cjx H on L"]
    args = (dev(c.a[None]), dev(c.b[None]), None, None, torch.tensor([c.d0], device="cuda"))
    first = pkg.ops.structure_align(*args)
    assert_all_same(pkg.ops.structure_align(*args), first, "structure_align")
    score = dev(A.dp_scores("eighths", 257, 130)[None])
    first = pkg.ops.nw_align(score, -0.6)
    assert_all_same(pkg.ops.nw_align(score, -0.6), first, "nw_align")


# ---- StructureBatch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", (("1a3r_HL", "5cjx_HL"), ("1REX", "1a3r_HL")))
def test_structure_batch_method(pkg, names):
    from protstruc_amd import StructureBatch
    mine, target = (StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, n + ".pdb")) for n in names)
    got = mine.structural_alignment(target)
    want = pkg.geometry.structure_alignment(mine.get_xyz()[:, :, 1], target.get_xyz()[:, :, 1], mine.get_atom_mask()[:, :, 1] != 0,
                                            target.get_atom_mask()[:, :, 1] != 0)
    assert_all_same(tuple(got[:9]), tuple(want), "structural_alignment")
    assert got.map.shape == (1, mine.get_max_n_residues()) and int(got.n_aligned) > 50
    sequences = ["".join(sb.get_seq()[0][c] for c in sb.get_chain_ids()[0]) for sb in (mine, target)]
    pairs = [(i, int(j)) for i, j in enumerate(host(got.map)[0]) if j >= 0]
    identical = sum(sequences[0][i] == sequences[1][j] for i, j in pairs)
    assert abs(float(got.identity) - identical / len(pairs)) <= 1e-6 and 0 < float(got.identity) < 1
    alone = mine.structural_alignment(target, use_secondary_structure=False)
    assert float(got.search_score) >= float(alone.search_score) and int(alone.start) == 0


# ---- the launch contract -------------------------------------------------------------------------------------------------------
# Two seeded variants that differ in the outputs that can differ; float64 strided points and scores and a float mask, so
# that the shell's conversions are on the launch path that is checked (as the cases of tests/launch_cases.py).
CONTRACT_M = (35, 47)


def _contract_inputs(v):
    k = "AB".index(v)
    a, b, ma, mb = [], [], [], []
    for s in (0, 1):
        rng = np.random.default_rng(300 + 10 * k + s)
        chain = np.cumsum(rng.standard_normal((26, 3)) * 2.2, axis=0)
        first = 2 + 3 * k + s
        short = chain[first:first + 19] @ align_ref.rotation(rng).T + rng.uniform(-10, 10, 3) + 0.4 * rng.standard_normal((19, 3))
        (A_, m_a), (B_, m_b) = A.scatter(A.S.f32(short), seed=40 + s, M=CONTRACT_M[0]), A.scatter(A.S.f32(chain), seed=50 + s, M=CONTRACT_M[1])
        a.append(np.nan_to_num(A_)), b.append(np.nan_to_num(B_)), ma.append(m_a), mb.append(m_b)
    rng = np.random.default_rng(70 + k)
    t = torch.from_numpy
    return dict(a=t(np.stack(a)).double(), b=t(np.stack(b)), mask_a=t(np.stack(ma)).float(), mask_b=t(np.stack(mb)),
                d0=torch.full((2,), 2.0), score=t(rng.integers(0, 9, (2,) + CONTRACT_M) / 8.0))


def _ops():
    from protstruc_amd import ops
    return ops


CONTRACT = (
    Case("nw_align", ("ps_nw_align_f32",), _contract_inputs,
         lambda i: _ops().nw_align(i["score"], -0.6, i["mask_a"], i["mask_b"]), strided=("score",)),
    Case("ca_secondary_structure", ("ps_ca_secondary_structure_f32",), _contract_inputs,
         lambda i: (_ops().ca_secondary_structure(i["a"], i["mask_a"]),), strided=("a",)),
    Case("structure_align", ("ps_structure_align_f32",), _contract_inputs,
         lambda i: _ops().structure_align(i["a"], i["b"], i["mask_a"], i["mask_b"], i["d0"]), strided=("a",)),
)
BY_NAME = {case.name: case for case in CONTRACT}
NAMES = list(BY_NAME)
HOST_FUNCTIONS = {"ps_structalign_api", "ps_structalign_workspace_bytes"}
MAY_TIE = {"nw_align": (1,), "ca_secondary_structure": (), "structure_align": (1, 5, 6)}      # counts and the start


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
        assert a.shape == b.shape and a.dtype == b.dtype, (name, k)
        assert k in MAY_TIE[name] or not same(a, b), (name, k)


def test_contract_cases_cover_the_header_and_meet_the_yardstick(pkg):
    from protstruc_amd import _lib
    assert sorted(s for case in CONTRACT for s in case.symbols) == sorted(set(_lib.STRUCTALIGN_SIGNATURES) - HOST_FUNCTIONS)
    for name in NAMES:
        assert_variants_differ(name)
    for v in "AB":
        i = {k: t.numpy() for k, t in _contract_inputs(v).items()}
        out = [host(t) for t in eager("structure_align", v)]
        got_dp = [host(t) for t in eager("nw_align", v)]
        labels = host(eager("ca_secondary_structure", v)[0])
        for s in (0, 1):
            ma, mb = i["mask_a"][s] != 0, i["mask_b"][s]
            c = A.Case(i["a"][s].astype(np.float32), i["b"][s], ma, mb, 2.0, True)
            want = A.align(c.a, c.b, ma, mb, 2.0)
            backwards = A.align(c.a, c.b, ma, mb, 2.0, reverse=True)
            assert np.array_equal(want.map, backwards.map) and want.start == backwards.start and abs(want.S - backwards.S) <= 1e-12
            assert_alignment(dict(zip(FIELDS, (o[s] for o in out))), c, want, f"contract {v}{s}")
            dp = A.nw_slots(i["score"][s].astype(np.float32), float(np.float32(-0.6)), ma, mb)
            assert np.array_equal(got_dp[0][s], dp.map) and got_dp[2][s] == np.float32(dp.value)
            assert np.array_equal(labels[s], A.secondary_structure(c.a, ma))


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
    """B = 65535 at Ma = Mb = 5: structure b is structure b % 3, and the results are those of the three, bit for bit"""
    ops = pkg.ops
    pairs = [A.small_pair(5, 40, seed=s) for s in range(3)]
    a = np.stack([p[0] for p in pairs])
    b = np.stack([p[1][15:20] for p in pairs])
    mask_a = np.ones((3, 5), dtype=bool)
    mask_a[1, 2] = False
    a[1, 2] = np.nan
    tensors = dict(a=dev(a), b=dev(b), mask_a=dev(mask_a), mask_b=dev(np.ones((3, 5), dtype=bool)), d0=torch.full((3,), 1.5, device="cuda"))
    small = ops.structure_align(**tensors)
    for s in range(3):
        c = A.Case(a[s], b[s], mask_a[s], None, 1.5, True)
        assert_alignment(dict(zip(FIELDS, (host(t)[s] for t in small))), c, A.align(a[s], b[s], mask_a[s], None, 1.5), f"batch limit {s}")
    assert_batch_of_65535_repeats_the_three(ops.structure_align, tensors, small, "structure_align")
    tensors = dict(score=dev(np.stack([A.dp_scores("eighths", 5, 5, seed=s) for s in range(3)])), mask_a=dev(mask_a))
    run = lambda score, mask_a: ops.nw_align(score, -0.6, mask_a)       # noqa: E731
    assert_batch_of_65535_repeats_the_three(run, tensors, run(**tensors), "nw_align")
    tensors = dict(points=dev(a), mask=dev(mask_a))
    assert_batch_of_65535_repeats_the_three(ops.ca_secondary_structure, tensors, ops.ca_secondary_structure(**tensors), "ca_secondary_structure")
