"""Message passing on graphs (K55 - K59) without a GPU: the restatement (tests/aggregate_ref.py) and every backward formula
held to torch float64 autograd of the composed route -- ``index_add``, a per-segment ``log_softmax``, gathers --, the header,
the binding table and the cross-compiled library held to each other, every refusal of the five entry points (nothing is
launched: no device is needed to be refused) and the argument checks of ``ops`` and ``geometry``."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from protstruc_amd import _aggregate, _csredge, _edgegrad, _lib, build, geometry, ops
from tests import aggregate_ref as A
from tests.c_headers import INCLUDE, declared_symbols, header_text, macros

HEADER = "protstruc_aggregate.h"
ENTRY_POINTS = ["ps_edge_dot_f32", "ps_segment_gather_f32", "ps_segment_reduce_f32", "ps_segment_softmax_backward_f32",
                "ps_segment_softmax_f32"]
INVALID = 1          # hipErrorInvalidValue
FAKE = 0x1000        # a device pointer that is not NULL; a refused call never uses it
TOL = 1e-9           # the project's figure for a restatement against float64 autograd


@pytest.fixture(scope="module")
def lib():
    build.build_aggregate(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _aggregate.load()


# ---- 1. the restatement against float64 autograd of the composed route ---------------------------------------------------------------
def graph_cases():
    """(name, B, Q, M, row_ptr, col): empty rows, padding inside rows, a max_edges tail, a cut list, a bipartite graph"""
    rng = np.random.default_rng(17)
    cases = []
    B, M = 2, 7
    lengths = [0, 3, 0, 0, 5, 2, 1, 4, 0, 6, 0, 0, 2, 0]
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = rng.integers(0, M, size=int(row_ptr[-1]) + 3).astype(np.int32)
    col[3:8] = [2, 2, 5, 2, 5]            # row 4 names point 2 three times
    col[-3:] = -1                          # the tail a max_edges graph leaves
    col[9], col[12] = M + 3, -1            # padding inside rows: a column out of range, the -1 of a padded list
    cases.append(("self", B, M, M, row_ptr, col))
    lengths = [5, 5, 0, 5, 1, 0, 0, 6, 2, 0, 3, 3, 0, 4]
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cases.append(("cut", B, M, M, row_ptr, rng.integers(0, M, size=int(row_ptr[-1]) - 9).astype(np.int32)))
    Q = 3
    lengths = [4, 0, 9, 0, 0, 7]
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = rng.integers(0, M, size=int(row_ptr[-1])).astype(np.int32)
    col[4:8] = [6, 6, 0, 6]
    cases.append(("bipartite", B, Q, M, row_ptr, col))
    return cases


CASES = pytest.mark.parametrize("case", graph_cases(), ids=lambda c: c[0])
ENDS = pytest.mark.parametrize("at", ("source", "target"))


def relative(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)


def setup(case, at, H=3, D=5, seed=3):
    name, B, Q, M, row_ptr, col = case
    rng = np.random.default_rng(seed)
    E = len(col)
    real = A.real_positions(row_ptr, col, M)
    index = A.edge_index(row_ptr, col, Q, M, at)
    ptr, perm, S = A.grouping(row_ptr, col, B, Q, M, at)
    values = rng.standard_normal((E, H, D)).astype(np.float32)
    weight = rng.standard_normal((E, H)).astype(np.float32)
    assert (index[real] >= 0).all() and (index[~real] == -1).all() and index.max() < S
    return rng, E, S, real, index, ptr, perm, values, weight


def planted(x, real):
    """a copy of ``x`` with NaN at the padding"""
    x = x.copy()
    x[~real] = np.nan
    return x


@CASES
@ENDS
@pytest.mark.parametrize("mode", ("sum", "mean"))
def test_the_sum_and_its_backward_formulas_are_float64_autograd_of_index_add(case, at, mode):
    rng, E, S, real, index, ptr, perm, values, weight = setup(case, at)
    H, D = values.shape[1:]
    out, _ = A.segment_reduce(planted(values, real), ptr, perm, S, mode, planted(weight, real), real, exact=True)
    assert np.isfinite(out).all(), "NaN at the padding does not surface"
    tv = torch.from_numpy(values.astype(np.float64)).requires_grad_()
    tw = torch.from_numpy(weight.astype(np.float64)).requires_grad_()
    keep = torch.from_numpy(index[real])
    n = torch.zeros(S, dtype=torch.float64).index_add(0, keep, torch.ones(len(keep), dtype=torch.float64))
    want = torch.zeros(S, H, D, dtype=torch.float64).index_add(0, keep, (tw[:, :, None] * tv)[torch.from_numpy(real)])
    if mode == "mean":
        want = want / n.clamp(min=1)[:, None, None]
    assert relative(out, want.detach().numpy()) <= TOL
    empty = (n == 0).numpy()
    assert (out[empty] == 0).all() and not np.signbit(out[empty]).any()
    g = rng.standard_normal((S, H, D)).astype(np.float32)
    (want * torch.from_numpy(g).double()).sum().backward()
    # the formulas of the backward pass: K56 over the same grouping with the weight (and the 1/n of MEAN), K57 for the weight
    gn = g if mode == "sum" else (g / np.maximum(n.numpy(), 1)[:, None, None]).astype(np.float32)
    grad_values = A.segment_gather(gn, index, planted(weight, real), exact=True)
    grad_weight = A.edge_dot(gn, planted(values, real), index, exact=True)
    tol = TOL if mode == "sum" else 3e-7      # MEAN's g / n is rounded to float32 before the kernels see it: 2^-24, and slack
    assert relative(grad_values, tv.grad.numpy()) <= tol and relative(grad_weight, tw.grad.numpy()) <= tol
    assert (grad_values[~real] == 0).all() and (grad_weight[~real] == 0).all()


@CASES
@ENDS
@pytest.mark.parametrize("mode", ("max", "min"))
def test_max_and_min_are_scatter_reduce_with_ties_to_the_lower_position(case, at, mode):
    rng, E, S, real, index, ptr, perm, values, _ = setup(case, at)
    values = np.round(values * 2).astype(np.float32) / 2          # coarse values: ties happen
    out, arg = A.segment_reduce(planted(values, real), ptr, perm, S, mode, None, real)
    H, D = values.shape[1:]
    keep = torch.from_numpy(index[real])[:, None, None].expand(-1, H, D)
    want = torch.zeros(S, H, D, dtype=torch.float64).scatter_reduce(0, keep, torch.from_numpy(values[real]).double(),
                                                                    "amax" if mode == "max" else "amin", include_self=False)
    assert np.array_equal(out.astype(np.float64), want.numpy())
    for s in range(S):
        mine = [e for e in range(E) if index[e] == s]
        if not mine:
            assert (arg[s] == -1).all() and (out[s] == 0).all()
            continue
        for h in range(H):
            for d in range(D):
                assert arg[s, h, d] == min(e for e in mine if values[e, h, d] == out[s, h, d])


@CASES
@ENDS
def test_the_gather_and_its_backward_formulas_are_float64_autograd_of_indexing(case, at):
    rng, E, S, real, index, ptr, perm, values, weight = setup(case, at)
    H, D = values.shape[1:]
    node = rng.standard_normal((S, H, D)).astype(np.float32)
    out = A.segment_gather(node, index, planted(weight, real), exact=True)
    tn = torch.from_numpy(node.astype(np.float64)).requires_grad_()
    tw = torch.from_numpy(weight.astype(np.float64)).requires_grad_()
    treal = torch.from_numpy(real)
    want = torch.where(treal[:, None, None], tw[:, :, None] * tn[torch.from_numpy(index).clamp(min=0)], torch.zeros((), dtype=torch.float64))
    assert relative(out, want.detach().numpy()) <= TOL and (out[~real] == 0).all() and not np.signbit(out[~real]).any()
    assert np.array_equal(A.segment_gather(node, index), np.where(real[:, None, None], node[np.maximum(index, 0)], 0))
    g = rng.standard_normal((E, H, D)).astype(np.float32)
    (want * torch.from_numpy(g).double()).sum().backward()
    # K55 SUM at the same end of the edges, with the weight; K57 for the weight; NaN in the incoming gradient at the padding
    grad_node, _ = A.segment_reduce(planted(g, real), ptr, perm, S, "sum", planted(weight, real), real, exact=True)
    grad_weight = A.edge_dot(node, planted(g, real), index, exact=True)
    assert relative(grad_node, tn.grad.numpy()) <= TOL and relative(grad_weight, tw.grad.numpy()) <= TOL


def test_the_edge_dot_sums_in_the_order_of_the_header():
    """fours ascending, then a tree: at D = 11 that is (s0 + s1) + s2 with s2 of three terms, not a running sum"""
    u = np.asarray([2.0 ** 53, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0 ** -30, 5.0, 7.0])
    s0, s1, s2 = ((u[0] + u[1]) + u[2]) + u[3], ((u[4] + u[5]) + u[6]) + u[7], (u[8] + u[9]) + u[10]
    assert s0 == 2.0 ** 53 and s1 == 4.0, "the ones are lost one at a time and kept four at a time"
    running = 0.0
    for term in u:
        running = running + term
    assert A.tree_sum(u) == (s0 + s1) + s2 and A.tree_sum(u) != running
    for D in (1, 3, 4, 5, 16, 17, 23, 64, 260):
        v = np.arange(1.0, D + 1)
        assert A.tree_sum(v) == D * (D + 1) / 2
    K = 7                                            # ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + s6)
    p = np.asarray([2.0 ** (-9 * k) for k in range(K)] * 1)
    quads = np.repeat(p, 4) / 4
    assert A.tree_sum(quads) == ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + p[6])


@CASES
@ENDS
def test_the_softmax_and_its_backward_are_float64_autograd_of_a_per_segment_log_softmax(case, at):
    rng, E, S, real, index, ptr, perm, _, _ = setup(case, at, H=2)
    H = 2
    logits = (rng.standard_normal((E, H)) * 3).astype(np.float32)
    logits[np.flatnonzero(real)[0], 0] = -np.inf                   # one member at -inf
    w, lse = A.segment_softmax(planted(logits, real), ptr, perm, S, real)
    assert np.isfinite(w).all() and (w[~real] == 0).all()
    tx = torch.from_numpy(logits.astype(np.float64)).requires_grad_()
    want = torch.zeros(E, H, dtype=torch.float64)
    want_lse = np.full((S, H), -np.inf)
    for s in range(S):
        mine = torch.from_numpy(np.flatnonzero(index == s))
        if len(mine):
            want = want.index_add(0, mine, torch.log_softmax(tx[mine], 0).exp())
            want_lse[s] = torch.logsumexp(tx[mine], 0).detach().numpy()
    assert relative(w, want.detach().numpy()) <= TOL
    both = np.isfinite(want_lse)
    assert np.array_equal(both, np.isfinite(lse)) and relative(lse[both], want_lse[both]) <= TOL
    sums = np.zeros((S, H))
    np.add.at(sums, index[real], w[real])
    assert np.allclose(sums[both], 1.0, atol=1e-12, rtol=0)
    g = rng.standard_normal((E, H)).astype(np.float32)
    (want * torch.from_numpy(g).double()).sum().backward()
    w32 = w.astype(np.float32)
    gx = A.segment_softmax_backward(planted(w32, real), planted(g, real), ptr, perm, S, real)
    # K59 starts from the float32 w: its distance from autograd is w's one rounding, 2^-24 relative, times the terms summed
    assert np.isfinite(gx).all() and (gx[~real] == 0).all() and relative(gx, tx.grad.numpy()) <= 1e-6
    # ... and from the same formula on the same float32 w, nothing but the order of the sum
    exact = A.segment_softmax_backward(w32, g, ptr, perm, S, real, exact=True)
    t64 = np.zeros((S, H))
    np.add.at(t64, index[real], (w32.astype(np.float64) * g)[real])
    assert relative(exact, np.where(real[:, None], w32.astype(np.float64) * (g - t64[np.maximum(index, 0)]), 0)) <= TOL


def test_the_softmax_edge_cases():
    ptr = np.asarray([0, 1, 1, 4, 6, 9], dtype=np.int64)          # one member; empty; normal; all -inf; one at 1e4
    x = np.asarray([[3.5], [0.0], [1.0], [-np.inf], [-np.inf], [-np.inf], [1e4], [0.0], [-1e4]], dtype=np.float32)
    w, lse = A.segment_softmax(x, ptr, None, 5)
    assert w[0, 0] == 1.0 and lse[0, 0] == 3.5
    assert lse[1, 0] == -np.inf
    assert w[3, 0] == 0 and not np.signbit(w[3, 0]) and abs(w[1:3].sum() - 1) < 1e-15
    assert (w[4:6] == 0).all() and lse[3, 0] == -np.inf
    assert w[6, 0] == 1.0 and (w[7:, 0] == 0).all() and lse[4, 0] == 1e4 and np.isfinite(w).all()


def test_a_wrong_list_is_cut_and_skipped_not_followed():
    values = np.ones((4, 1, 1), np.float32)
    out, _ = A.segment_reduce(values, np.asarray([-5, 2, 99]), None, 2, "sum")
    assert out.reshape(-1).tolist() == [2.0, 2.0]
    out, _ = A.segment_reduce(values, np.asarray([0, 3, 7]), np.asarray([0, -1, 9, 3, 3]), 2, "sum")
    assert out.reshape(-1).tolist() == [1.0, 2.0]


# ---- 2. the header, the table, the library ---------------------------------------------------------------------------------------------
def test_header_is_c99():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(INCLUDE, HEADER)], check=True)


def test_header_binding_and_library_agree(lib):
    declared = declared_symbols(HEADER)
    assert declared == sorted(_aggregate.AGGREGATE_SIGNATURES) == sorted(ENTRY_POINTS + ["ps_aggregate_api"])
    nm = subprocess.run(["nm", "-D", "--defined-only", build.AGGREGATE_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)$", nm, flags=re.M))) == declared
    for table in ["SIGNATURES"] + [family.signatures for family in _lib.FAMILIES]:
        assert not set(declared) & set(getattr(_lib, table)), table
    assert not set(declared) & set(_csredge.CSREDGE_SIGNATURES) and not set(declared) & set(_edgegrad.EDGEGRAD_SIGNATURES)
    api = macros(HEADER)["PS_AGGREGATE_API"]
    assert lib.ps_aggregate_api() == api == _aggregate.EXPECTED_AGGREGATE_API == 1
    for name in ENTRY_POINTS:
        restype, argtypes = _aggregate.AGGREGATE_SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p                # the HIP error; the stream last
    assert _aggregate.AGGREGATE_SIGNATURES["ps_segment_reduce_f32"][1][7] is ctypes.c_longlong           # E
    assert _aggregate.AGGREGATE_SIGNATURES["ps_segment_gather_f32"][1][3:5] == [ctypes.c_longlong] * 2   # E, S
    # K59 takes K58's grouping, with the saved weights and the incoming gradient in the place of the logits
    forward, backward = (_aggregate.AGGREGATE_SIGNATURES[n][1] for n in ("ps_segment_softmax_f32", "ps_segment_softmax_backward_f32"))
    assert forward[1:7] == backward[2:8] and len(forward) == len(backward)


def test_the_names_follow_the_family_rule_and_the_conventions_are_those_of_the_edge_gradients():
    stem = "aggregate"
    assert HEADER == f"protstruc_{stem}.h" and f"ps_{stem}_api" in _aggregate.AGGREGATE_SIGNATURES
    assert isinstance(getattr(_aggregate, f"EXPECTED_{stem.upper()}_API"), int)
    assert "#define PS_AGGREGATE_API 1" in header_text(HEADER)
    assert stem not in "".join(family.header for family in _lib.FAMILIES) and len(_lib.FAMILIES) == 6
    ours, theirs = header_text(HEADER), header_text("protstruc_edgegrad.h")
    for sentence in ("every pointer is a DEVICE pointer owned by the caller",
                     "the library never allocates, frees or retains memory",
                     "tensors are contiguous and need only the alignment of their element",
                     "`stream` is a `hipStream_t` passed as `void*` (NULL = the default stream)",
                     "launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory",
                     "may be captured into a hipGraph",
                     "the library holds no mutable state",
                     "the return value is a `hipError_t` as int (0 = success); argument errors return hipErrorInvalidValue (1) before",
                     "B == 0 returns 0 without touching a device",
                     "offsets are 64-bit throughout; no kernel uses an atomic, every output",
                     "element is written, and repeated runs agree bit for bit",
                     "is established by reading, not by a test",
                     "The library is built with -ffp-contract=off"):
        assert sentence in ours and sentence in theirs, sentence
    # the header says which design each kernel is, fixes the order of every sum, and says that lists are not split
    for sentence in ("A lane owns four consecutive floats of one segment's row", "four members' loads issued before the first is used",
                     "fours ascending", "then a tree over the K = ceil(D / 4) partial sums", "One lane per (segment, head)",
                     "Lists are NOT SPLIT", "add the partial sums in chunk\n * order", "ties go to the lower position",
                     "every index a kernel uses as an address is range-checked first"):
        assert sentence in ours, sentence


def test_the_limits_are_macros_and_ops_mirrors_them():
    m = macros(HEADER)
    assert m["PS_AGGREGATE_MAX_HEADS"] == ops.AGGREGATE_MAX_HEADS >= 8 and m["PS_AGGREGATE_MAX_ROW"] == ops.AGGREGATE_MAX_ROW >= 4096
    assert [m["PS_AGGREGATE_" + mode.upper()] for mode in ops.AGGREGATE_MODES] == [0, 1, 2, 3] and A.MODES == ops.AGGREGATE_MODES
    text = open(ops.__file__).read()
    for name in ("AGGREGATE_MAX_HEADS", "AGGREGATE_MAX_ROW"):
        assert re.search(rf"^{name} = \d+  # PS_{name}", text, flags=re.M), "the comment form the mirrored-constant test reads"


MAIN_LIBRARY_DIGEST = "067f9c134d294534ce1d488d885b63a3fc84b67e711c8e50814285fba3c6f5e9"


def test_the_library_is_a_target_of_its_own_and_the_main_library_is_what_it_was():
    target = build._aggregate_library()
    names = [os.path.basename(d) for d in target.inputs]
    assert "segment_ops.hip" in names and "ps_common.hpp" in names and HEADER in names
    assert all(os.path.dirname(s) == build.AGGREGATE_SRC_DIR for s in build.aggregate_sources()) and build.aggregate_sources()
    for others in (build.sources(), build.csredge_sources(), build.edgegrad_sources()):
        assert not set(build.aggregate_sources()) & set(others)
    assert HEADER not in {os.path.basename(d) for d in build._deps()}
    assert build.source_hash() == MAIN_LIBRARY_DIGEST, "the main library's digest is the parent commit's"
    for other in (build._csredge_library(), build._edgegrad_library()):
        assert HEADER not in {os.path.basename(d) for d in other.inputs}
    cmd = target.command("out.so")
    assert cmd == [build.HIPCC] + build.FLAGS + ["-I" + build.CSRC, "-o", "out.so"] + build.aggregate_sources()
    assert not build.aggregate_is_stale()
    assert os.path.basename(build.AGGREGATE_LIB_PATH) == "libprotstruc_aggregate.so"


def test_the_entry_point_and_the_command_line_build_and_load_the_library(lib, monkeypatch):
    """what they do, not how they spell it: build() builds this library and loads it; the command line names it as built"""
    import __graft_entry__
    seen = []
    build_aggregate, load = build.build_aggregate, _aggregate.load
    monkeypatch.setattr(build, "build_aggregate", lambda *a, **kw: (seen.append("build"), build_aggregate(*a, **kw))[1])
    monkeypatch.setattr(_aggregate, "load", lambda: (seen.append("load"), load())[1])
    __graft_entry__.build()
    assert seen == ["build", "load"]
    out = subprocess.run([sys.executable, "-m", "protstruc_amd.build"], check=True, capture_output=True, text=True,
                         cwd=os.path.dirname(build.HERE)).stdout
    assert os.path.abspath(build.AGGREGATE_LIB_PATH) in [os.path.abspath(line) for line in out.splitlines()]


def test_a_library_with_another_version_is_refused(lib, monkeypatch):
    bound = _aggregate.EXPECTED_AGGREGATE_API
    monkeypatch.setattr(_aggregate, "_lib", None)
    monkeypatch.setattr(_aggregate, "EXPECTED_AGGREGATE_API", bound + 1)
    with pytest.raises(_lib.HipLibraryError) as info:
        _aggregate.load()
    assert str(info.value) == (f"{_aggregate.LIB_PATH} has aggregate API version {bound}, this package binds version {bound + 1}: "
                               "rebuild with `python -m protstruc_amd.build --force`")


def test_a_missing_or_stale_library_is_refused_in_the_words_of_the_edge_gradients(lib, monkeypatch, tmp_path):
    def refusals(module, stem, stale):
        said = []
        gone = str(tmp_path / f"libprotstruc_{stem}.so")
        monkeypatch.setattr(module, "_lib", None)
        monkeypatch.setattr(module, "LIB_PATH", gone)
        with pytest.raises(_lib.HipLibraryError) as info:
            module.load()
        said.append(str(info.value).replace(gone, "LIB"))
        monkeypatch.undo()
        monkeypatch.setattr(module, "_lib", None)
        monkeypatch.setattr(build, stale, lambda path=None: True)
        monkeypatch.setattr(build, "HIPCC", "/nonexistent/hipcc")
        with pytest.raises(_lib.HipLibraryError) as info:
            module.load()
        said.append(str(info.value).replace(module.LIB_PATH, "LIB").replace(stem, "STEM"))
        monkeypatch.undo()
        return said
    ours = refusals(_aggregate, "aggregate", "aggregate_is_stale")
    assert ours == refusals(_edgegrad, "edgegrad", "edgegrad_is_stale")
    assert ours[0] == ("LIB is missing: build it with `python -m protstruc_amd.build` (hipcc --offload-arch=gfx950). "
                       "protstruc_amd has no CPU fallback.")
    assert ours[1].startswith("LIB is older than its sources (csrc_STEM/*.hip, csrc/*.hpp, include/protstruc_STEM.h)")


# ---- 3. every refusal of the five entry points -------------------------------------------------------------------------------------------
def reduce_args(**changes):
    a = dict(values=FAKE, weight=None, ptr=FAKE, perm=None, n_perm=0, row_ptr=FAKE, col=FAKE, E=0, mode=0, out=FAKE, arg=None,
             B=0, Q=7, M=7, H=2, D=8)
    a.update(changes)
    return [a[k] for k in ("values", "weight", "ptr", "perm", "n_perm", "row_ptr", "col", "E", "mode", "out", "arg", "B", "Q", "M",
                           "H", "D")] + [None]


def gather_args(**changes):
    a = dict(node=FAKE, weight=None, index=FAKE, E=0, S=14, H=2, D=8, out=FAKE)
    a.update(changes)
    return [a[k] for k in ("node", "weight", "index", "E", "S", "H", "D", "out")] + [None]


def dot_args(**changes):
    a = dict(node=FAKE, values=FAKE, index=FAKE, E=0, S=14, H=2, D=8, out=FAKE)
    a.update(changes)
    return [a[k] for k in ("node", "values", "index", "E", "S", "H", "D", "out")] + [None]


def softmax_args(**changes):
    a = dict(logits=FAKE, ptr=FAKE, perm=None, n_perm=0, row_ptr=FAKE, col=FAKE, E=0, w=FAKE, lse=None, B=0, Q=7, M=7, H=2)
    a.update(changes)
    return [a[k] for k in ("logits", "ptr", "perm", "n_perm", "row_ptr", "col", "E", "w", "lse", "B", "Q", "M", "H")] + [None]


def softmax_backward_args(**changes):
    a = dict(w=FAKE, grad_w=FAKE, ptr=FAKE, perm=None, n_perm=0, row_ptr=FAKE, col=FAKE, E=0, grad_logits=FAKE, B=0, Q=7, M=7, H=2)
    a.update(changes)
    return [a[k] for k in ("w", "grad_w", "ptr", "perm", "n_perm", "row_ptr", "col", "E", "grad_logits", "B", "Q", "M", "H")] + [None]


BIG = 2 ** 24 + 1
GROUPING_REFUSALS = [dict(B=-1), dict(B=65536), dict(M=-1), dict(M=BIG), dict(Q=-1), dict(Q=BIG), dict(E=-1), dict(n_perm=-1),
                     dict(H=0), dict(H=65), dict(ptr=None), dict(n_perm=5), dict(row_ptr=None)]      # a col without row_ptr
REDUCE_REFUSALS = GROUPING_REFUSALS + [dict(D=0), dict(H=64, D=65), dict(H=1, D=4097), dict(mode=-1), dict(mode=4),
                                       dict(mode=2, weight=FAKE), dict(mode=3, weight=FAKE), dict(mode=0, arg=FAKE),
                                       dict(mode=1, arg=FAKE), dict(out=None), dict(E=5, values=None)]
ROW_REFUSALS = [dict(E=-1), dict(S=-1), dict(H=0), dict(H=65), dict(D=0), dict(H=64, D=65), dict(H=1, D=4097), dict(index=None),
                dict(out=None), dict(node=None)]
SOFTMAX_REFUSALS = GROUPING_REFUSALS + [dict(E=5, logits=None), dict(E=5, w=None)]
SOFTMAX_BACKWARD_REFUSALS = GROUPING_REFUSALS + [dict(E=5, w=None), dict(E=5, grad_w=None), dict(E=5, grad_logits=None)]


def test_the_base_arguments_are_accepted_and_an_empty_call_launches_nothing(lib):
    """B == 0 (E == 0 in K56 and K57) returns 0 after every check and before any launch: what each refusal below changes is
    the reason"""
    assert lib.ps_segment_reduce_f32(*reduce_args()) == 0 and lib.ps_segment_reduce_f32(*reduce_args(E=5)) == 0
    assert lib.ps_segment_reduce_f32(*reduce_args(weight=FAKE, mode=1)) == 0
    assert lib.ps_segment_reduce_f32(*reduce_args(arg=FAKE, mode=2, perm=FAKE, n_perm=9, E=9)) == 0
    assert lib.ps_segment_reduce_f32(*reduce_args(row_ptr=None, col=None, H=64, D=64)) == 0
    assert lib.ps_segment_reduce_f32(*reduce_args(B=3, Q=0, E=5)) == 0, "no segments: nothing to write"
    assert lib.ps_segment_gather_f32(*gather_args()) == 0 and lib.ps_segment_gather_f32(*gather_args(weight=FAKE, S=0, node=None)) == 0
    assert lib.ps_edge_dot_f32(*dot_args()) == 0 and lib.ps_edge_dot_f32(*dot_args(S=0, node=None, H=1, D=4096)) == 0
    assert lib.ps_segment_softmax_f32(*softmax_args()) == 0 and lib.ps_segment_softmax_f32(*softmax_args(E=5, lse=FAKE)) == 0
    assert lib.ps_segment_softmax_f32(*softmax_args(perm=FAKE, n_perm=5, E=5, row_ptr=None, col=None)) == 0
    assert lib.ps_segment_softmax_backward_f32(*softmax_backward_args()) == 0
    assert lib.ps_segment_softmax_backward_f32(*softmax_backward_args(E=5, perm=FAKE, n_perm=5)) == 0
    assert lib.ps_segment_softmax_backward_f32(*softmax_backward_args(B=2, E=0, w=None, grad_w=None, grad_logits=None)) == 0


@pytest.mark.parametrize("B", (0, 2))
def test_every_refusal_returns_invalid_value(lib, B):
    """with B = 2 and edges a call that was NOT refused would launch on pointers that are no memory: the refusal comes first"""
    live = dict(B=B, E=100) if B else {}
    for changes in REDUCE_REFUSALS:
        assert lib.ps_segment_reduce_f32(*reduce_args(**{**live, **changes})) == INVALID, changes
    for changes in ROW_REFUSALS:
        assert lib.ps_segment_gather_f32(*gather_args(**{"E": 100 if B else 0, **changes})) == INVALID, changes
        assert lib.ps_edge_dot_f32(*dot_args(**{"E": 100 if B else 0, **changes})) == INVALID, changes
    assert lib.ps_edge_dot_f32(*dot_args(E=100 if B else 0, values=None)) == INVALID
    for changes in SOFTMAX_REFUSALS:
        assert lib.ps_segment_softmax_f32(*softmax_args(**{**live, **changes})) == INVALID, changes
    for changes in SOFTMAX_BACKWARD_REFUSALS:
        assert lib.ps_segment_softmax_backward_f32(*softmax_backward_args(**{**live, **changes})) == INVALID, changes


# ---- 4. the argument checks of ops and geometry -----------------------------------------------------------------------------------------
def operands():
    row_ptr = torch.arange(15, dtype=torch.int64) * 2
    col = torch.zeros(28, dtype=torch.int32)
    return torch.zeros(28, 2, 8), row_ptr, col, dict(B=2, Q=7, M=7)


def test_ops_refuses_wrong_shapes_dtypes_devices_and_a_weight_with_max():
    values, row_ptr, col, dims = operands()
    check = ops.check_segment_reduce_shapes
    assert check(values, row_ptr, None, torch.zeros(28, 2), row_ptr, col, **dims) == (28, 2, 8, 14)
    in_ptr, in_edge = ops.csr_incoming_edges(row_ptr, col, 2, 7, 7)
    assert check(values, in_ptr, in_edge, **dims, reduce="max", return_arg=True) == (28, 2, 8, 14)
    with pytest.raises(ValueError, match="reduce='max' takes no weight"):
        check(values, row_ptr, weight=torch.zeros(28, 2), **dims, reduce="max")
    with pytest.raises(ValueError, match="reduce='mean' has no arg"):
        check(values, row_ptr, **dims, reduce="mean", return_arg=True)
    with pytest.raises(ValueError, match="reduce must be one of sum, mean, max, min"):
        check(values, row_ptr, **dims, reduce="prod")
    with pytest.raises(ValueError, match=r"values must have shape \(rows, heads, floats\)"):
        check(values.reshape(28, 16), row_ptr, **dims)
    with pytest.raises(ValueError, match="values must be a floating-point tensor"):
        check(values.int(), row_ptr, **dims)
    with pytest.raises(ValueError, match="1 .. 64 heads in values"):
        check(torch.zeros(28, 65, 1), row_ptr, **dims)
    with pytest.raises(ValueError, match="a row of values holds 1 .. 4096 floats"):
        check(torch.zeros(28, 64, 65), row_ptr, **dims)
    with pytest.raises(ValueError, match=r"weight must have shape \(28, 2\)"):
        check(values, row_ptr, weight=torch.zeros(28), **dims)
    with pytest.raises(ValueError, match=r"ptr must be an int64 tensor of shape \(15,\)"):
        check(values, row_ptr[:-1], **dims)
    with pytest.raises(ValueError, match=r"ptr must be an int64 tensor of shape \(15,\)"):
        check(values, row_ptr.int(), **dims)
    with pytest.raises(ValueError, match="perm must be an int64 tensor"):
        check(values, in_ptr, in_edge.int(), **dims)
    with pytest.raises(ValueError, match="row_ptr and col come together"):
        check(values, row_ptr, col=col, **dims)
    with pytest.raises(ValueError, match=r"col must have shape \(28,\)"):
        check(values, row_ptr, row_ptr=row_ptr, col=col[:-1], **dims)
    with pytest.raises(ValueError, match="at most 65535 structures"):
        check(values, row_ptr, B=65536, Q=7, M=7)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.segment_reduce(values, row_ptr, **dims)

    node, index = torch.zeros(14, 2, 8), torch.zeros(28, dtype=torch.int64)
    assert ops.check_segment_gather_shapes(node, index, torch.zeros(28, 2)) == (28, 14, 2, 8)
    with pytest.raises(ValueError, match=r"index must be an int64 tensor of shape \(edges,\)"):
        ops.check_segment_gather_shapes(node, index.int())
    with pytest.raises(ValueError, match=r"weight must have shape \(28, 2\)"):
        ops.check_segment_gather_shapes(node, index, torch.zeros(28, 3))
    assert ops.check_edge_dot_shapes(node, values, index) == (28, 14, 2, 8)
    with pytest.raises(ValueError, match=r"values must be a floating-point tensor of shape \(28, 2, 8\)"):
        ops.check_edge_dot_shapes(node, values[:, :1], index)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.segment_gather(node, index)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.edge_dot(node, values, index)

    logits = torch.zeros(28, 2)
    assert ops.check_segment_softmax_shapes(logits, row_ptr, None, row_ptr, col, **dims) == (28, 2, 14)
    with pytest.raises(ValueError, match=r"logits must be a floating-point tensor of shape \(edges, heads\)"):
        ops.check_segment_softmax_shapes(logits.reshape(-1), row_ptr, **dims)
    with pytest.raises(ValueError, match="1 .. 64 heads in logits"):
        ops.check_segment_softmax_shapes(torch.zeros(28, 65), row_ptr, **dims)
    assert ops.check_segment_softmax_backward_shapes(logits, logits, in_ptr, in_edge, **dims) == (28, 2, 14)
    with pytest.raises(ValueError, match=r"grad_w must be a floating-point tensor of shape \(28, 2\)"):
        ops.check_segment_softmax_backward_shapes(logits, logits[:, :1], row_ptr, **dims)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.segment_softmax(logits, row_ptr, **dims)


def test_geometry_refuses_what_does_not_fit_the_graph():
    _, row_ptr, col, _ = operands()
    graph = geometry.RadiusGraph(row_ptr, col, None, torch.full((2, 7), 2, dtype=torch.int32))
    idx = torch.zeros(2, 7, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"messages must have shape \(28,\) \+ \(C,\) or \(H, D\)"):
        geometry.edge_aggregate(torch.zeros(27, 4), graph)
    with pytest.raises(ValueError, match=r"messages must have shape \(28,\) \+ \(C,\) or \(H, D\)"):
        geometry.edge_aggregate(torch.zeros(28), graph)
    with pytest.raises(ValueError, match=r"messages must have shape \(2, 7, 4\) \+"):
        geometry.edge_aggregate(torch.zeros(2, 7, 5, 3), idx)
    with pytest.raises(ValueError, match="messages must be a floating-point tensor"):
        geometry.edge_aggregate(torch.zeros(28, 4, dtype=torch.int64), graph)
    with pytest.raises(ValueError, match="reduce='min' takes no weight"):
        geometry.edge_aggregate(torch.zeros(28, 4), graph, reduce="min", weight=torch.zeros(28))
    with pytest.raises(ValueError, match="reduce='sum' has no arg"):
        geometry.edge_aggregate(torch.zeros(28, 4), graph, return_arg=True)
    with pytest.raises(ValueError, match="weight must hold one number per edge or per head"):
        geometry.edge_aggregate(torch.zeros(28, 2, 4), graph, weight=torch.zeros(28, 3))
    with pytest.raises(ValueError, match="at must be 'source' or 'target'"):
        geometry.edge_aggregate(torch.zeros(28, 4), graph, at="both")
    with pytest.raises(ValueError, match="n_targets must be a non-negative integer"):
        geometry.edge_aggregate(torch.zeros(28, 4), graph, at="target", n_targets=-1)
    with pytest.raises(TypeError, match="graph must be a geometry.RadiusGraph, a geometry.Neighbors or"):
        geometry.edge_aggregate(torch.zeros(28, 4), (row_ptr, col))
    with pytest.raises(ValueError, match="a padded neighbour list must be an integer tensor"):
        geometry.edge_softmax(torch.zeros(2, 7, 4), idx.float())
    with pytest.raises(ValueError, match=r"logits must have shape \(28,\) \+ \(\) or \(H,\)"):
        geometry.edge_softmax(torch.zeros(28, 2, 2), graph)
    with pytest.raises(ValueError, match=r"values must be a floating-point tensor of shape \(2, M, C\)"):
        geometry.edge_gather(torch.zeros(3, 7, 4), graph)
    with pytest.raises(ValueError, match=r"values must be a floating-point tensor of shape \(2, 7, C\)"):
        geometry.edge_gather(torch.zeros(2, 8, 4), graph, at="source")
    with pytest.raises(ValueError, match=r"logits must have shape \(28,\)"):
        geometry.edge_attention(torch.zeros(27), torch.zeros(28, 4), graph)
    for function in (geometry.edge_aggregate, geometry.edge_gather, geometry.edge_softmax, geometry.edge_attention):
        assert "Differentiable with respect to" in function.__doc__ and "torch.cuda.graph" in function.__doc__
    assert "COMPOSED" in geometry.edge_attention.__doc__ and "gather_neighbors" in geometry.edge_gather.__doc__
