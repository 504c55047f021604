"""The backward kernels of the edge features (K52 - K54) without a GPU: the restatement's gradients held to torch float64
autograd of the composed route, ``ops.csr_incoming_edges`` on CPU tensors held to its restatement, the header, the binding
table and the cross-compiled library held to each other, every refusal of the three entry points (nothing is launched: no
device is needed to be refused) and the argument checks of ``ops``."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from protstruc_amd import _csredge, _edgegrad, _lib, build, geometry, ops
from tests import csr_edge_ref as C, edge_grad_ref as G
from tests.c_headers import INCLUDE, declared_symbols, header_text, macros

HEADER = "protstruc_edgegrad.h"
ENTRY_POINTS = ["ps_csr_edge_frames_backward_f32", "ps_csr_edge_pair_grad_sum_f32", "ps_csr_edge_rbf_backward_f32"]
INVALID = 1          # hipErrorInvalidValue
FAKE = 0x1000        # a device pointer that is not NULL; a refused call never uses it


@pytest.fixture(scope="module")
def lib():
    build.build_edgegrad(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _edgegrad.load()


# ---- 1. the restatement against float64 autograd of the composed route ---------------------------------------------------------------
def graph_cases():
    """(name, B, M, A, Q, As, row_ptr, col): self and bipartite graphs with rows of length 0, duplicate columns in a row, a
    tail of -1 and a column out of range"""
    rng = np.random.default_rng(11)
    cases = []
    B, M, A = 2, 7, 4
    lengths = [0, 3, 0, 0, 5, 2, 1, 4, 0, 6, 0, 0, 2, 0]
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = rng.integers(0, M, size=int(row_ptr[-1]) + 3).astype(np.int32)
    col[3:8] = [2, 2, 5, 2, 5]            # row 4 names residue 2 three times
    col[-3:] = -1                          # the tail a max_edges graph leaves
    col[9] = M + 3                         # a column out of range inside a row
    cases.append(("self", B, M, A, None, None, row_ptr, col))
    Q, As = 3, 2
    lengths = [4, 0, 9, 0, 0, 7]
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = rng.integers(0, M, size=int(row_ptr[-1])).astype(np.int32)
    col[4:8] = [6, 6, 0, 6]
    cases.append(("bipartite", B, M, A, Q, As, row_ptr, col))
    return cases


def composed_distance_loss(x, s, row_ptr, col, ok, oks, pi, pj, centers, sigma, g_dist, g_rbf, Q, M, keep_zero_lengths):
    """sum(g_dist * d) + sum(g_rbf * exp(-((d - mu) / sigma)^2)) over the real pairs, by gather + sqrt-of-squares + exp in
    torch float64.  With ``keep_zero_lengths`` a pair of length 0 stays in the loss, as a plain composed route has it."""
    b, q, j, real_edge = (torch.from_numpy(np.asarray(a)) for a in C._edges(row_ptr, col, Q, M))
    Xi, Xj = s[b, q][:, pi], x[b, j][:, pj]                                         # (E,P,3)
    real = real_edge[:, None] & oks[b, q][:, pi] & ok[b, j][:, pj]
    diff = torch.where(real[..., None], Xj - Xi, torch.ones_like(Xi))
    if not keep_zero_lengths:
        zero = (diff == 0).all(-1)
        real = real & ~zero
        diff = torch.where(zero[..., None], torch.ones_like(diff), diff)
    d = torch.sqrt((diff * diff).sum(-1))
    rbf = torch.exp(-(((d[..., None] - centers) / sigma) ** 2))
    E, P = d.shape
    loss = (torch.where(real, d, torch.zeros_like(d)) * g_dist).sum()
    return loss + (torch.where(real[..., None], rbf, torch.zeros_like(rbf)) * g_rbf.reshape(E, P, -1)).sum()


def relative(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize("case", graph_cases(), ids=lambda c: c[0])
def test_the_distance_restatement_is_float64_autograd_of_the_composed_route(case):
    name, B, M, A, Q, As, row_ptr, col = case
    rng = np.random.default_rng(5)
    bipartite = Q is not None
    Qs, Ass = (Q, As) if bipartite else (M, A)
    x = (rng.standard_normal((B, M, A, 3)) * 3).astype(np.float32)
    s = (rng.standard_normal((B, Qs, Ass, 3)) * 3).astype(np.float32) if bipartite else None
    ok = rng.random((B, M, A)) > 0.25
    oks = rng.random((B, Qs, Ass)) > 0.25 if bipartite else None
    x[~ok] = np.nan                                                                 # masked atoms over NaN
    pair_i, pair_j = [0, Ass - 1, 1, 0], [A - 1, 0, 2, 0]
    centers = np.linspace(1.0, 9.0, 5).astype(np.float32)
    sigma = 1.75
    E, P, R = len(col), len(pair_i), len(centers)
    g_dist = rng.standard_normal((E, P)).astype(np.float32)
    g_rbf = rng.standard_normal((E, P * R)).astype(np.float32)

    pg = G.rbf_backward(x, row_ptr, col, ok, pair_i, pair_j, centers, sigma, s, oks, g_dist, g_rbf, exact=True)
    in_ptr, in_edge = G.incoming(row_ptr, col, B, Qs, M)
    got = G.pair_grad_sum(pg.f, row_ptr, in_ptr, in_edge, pair_i, pair_j, B, M, A, Q, As)

    tx = torch.from_numpy(np.nan_to_num(x).astype(np.float64)).requires_grad_()
    ts = torch.from_numpy(s.astype(np.float64)).requires_grad_() if bipartite else tx
    loss = composed_distance_loss(tx, ts, row_ptr, col, torch.from_numpy(ok), torch.from_numpy(oks if bipartite else ok),
                                  pair_i, pair_j, torch.from_numpy(centers.astype(np.float64)), sigma, torch.from_numpy(g_dist).double(),
                                  torch.from_numpy(g_rbf).double(), Qs, M, keep_zero_lengths=False)
    loss.backward()
    assert np.isfinite(got.grad).all() and (got.grad[~ok] == 0).all()
    assert relative(got.grad, tx.grad.numpy()) <= 1e-9
    if bipartite:
        assert (got.grad_src[~oks] == 0).all()
        assert relative(got.grad_src, ts.grad.numpy()) <= 1e-9
    assert pg.real.any() and not pg.real.all() and (pg.f[~pg.real] == 0).all()


def test_a_self_edge_of_length_zero_is_zero_in_the_definition_and_nan_in_plain_autograd():
    B, M, A = 1, 4, 2
    rng = np.random.default_rng(2)
    x = rng.standard_normal((B, M, A, 3)).astype(np.float32)
    row_ptr = np.asarray([0, 2, 4, 6, 8], dtype=np.int64)                          # an include_self graph: i, then a neighbour
    col = np.asarray([0, 1, 1, 2, 2, 3, 3, 0], dtype=np.int32)
    pair_i, pair_j = [0, 1, 0], [0, 1, 1]                                           # the first two pairs have length 0 on a self edge
    centers = np.asarray([0.0, 1.0, 2.0], dtype=np.float32)
    sigma, E, P, R = 0.8, 8, 3, 3
    g_dist, g_rbf = np.ones((E, P), np.float32), rng.standard_normal((E, P * R)).astype(np.float32)
    ok = np.ones((B, M, A), bool)
    pg = G.rbf_backward(x, row_ptr, col, None, pair_i, pair_j, centers, sigma, g_dist=g_dist, g_rbf=g_rbf, exact=True)
    assert not pg.real[0::2, :2].any() and pg.real[0::2, 2].all() and pg.real[1::2].all()
    assert (pg.f[0::2, :2] == 0).all() and np.isfinite(pg.f).all()
    in_ptr, in_edge = G.incoming(row_ptr, col, B, M, M)
    got = G.pair_grad_sum(pg.f, row_ptr, in_ptr, in_edge, pair_i, pair_j, B, M, A)

    def autograd(keep_zero_lengths):
        tx = torch.from_numpy(x.astype(np.float64)).requires_grad_()
        composed_distance_loss(tx, tx, row_ptr, col, torch.from_numpy(ok), torch.from_numpy(ok), pair_i, pair_j,
                               torch.from_numpy(centers.astype(np.float64)), sigma, torch.from_numpy(g_dist).double(),
                               torch.from_numpy(g_rbf).double(), M, M, keep_zero_lengths).backward()
        return tx.grad.numpy()
    assert np.isnan(autograd(True)).all(), "plain autograd: 0 * inf at sqrt(0) reaches every atom, each being on a self edge"
    assert relative(got.grad, autograd(False)) <= 1e-9


@pytest.mark.parametrize("case", graph_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize("which", ("both", "pos", "rot"))
def test_the_frames_restatement_is_float64_autograd_of_the_composed_route(case, which):
    name, B, M, _, Q, _, row_ptr, col = case
    rng = np.random.default_rng(8)
    bipartite = Q is not None
    Qs = Q if bipartite else M
    rot, trans = rng.standard_normal((B, M, 3, 3)).astype(np.float32), rng.standard_normal((B, M, 3)).astype(np.float32)
    ok = rng.random((B, M)) > 0.3
    rot[~ok] = np.nan
    srot = rng.standard_normal((B, Qs, 3, 3)).astype(np.float32) if bipartite else None
    strans = rng.standard_normal((B, Qs, 3)).astype(np.float32) if bipartite else None
    oks = rng.random((B, Qs)) > 0.3 if bipartite else None
    E = len(col)
    g_pos = rng.standard_normal((E, 3)).astype(np.float32) if which != "rot" else None
    g_rot = rng.standard_normal((E, 3, 3)).astype(np.float32) if which != "pos" else None
    in_ptr, in_edge = G.incoming(row_ptr, col, B, Qs, M)
    got = G.frames_backward(rot, trans, row_ptr, col, in_ptr, in_edge, ok, srot, strans, oks, g_pos, g_rot)

    tR = torch.from_numpy(np.nan_to_num(rot).astype(np.float64)).requires_grad_()
    tT = torch.from_numpy(trans.astype(np.float64)).requires_grad_()
    sR = torch.from_numpy(srot.astype(np.float64)).requires_grad_() if bipartite else tR
    sT = torch.from_numpy(strans.astype(np.float64)).requires_grad_() if bipartite else tT
    b, q, j, real = (torch.from_numpy(np.asarray(a)) for a in C._edges(row_ptr, col, Qs, M))
    real = real & torch.from_numpy(oks if bipartite else ok)[b, q] & torch.from_numpy(ok)[b, j]
    Ri, Rj, v = sR[b, q], tR[b, j], tT[b, j] - sT[b, q]
    pos = torch.einsum("erc,er->ec", Ri, v)                                         # R_i^T (t_j - t_i)
    rel = torch.einsum("era,erc->eac", Ri, Rj)                                      # R_i^T R_j
    loss = 0
    if g_pos is not None:
        loss = loss + (torch.where(real[:, None], pos, torch.zeros_like(pos)) * torch.from_numpy(g_pos).double()).sum()
    if g_rot is not None:
        loss = loss + (torch.where(real[:, None, None], rel, torch.zeros_like(rel)) * torch.from_numpy(g_rot).double()).sum()
    loss.backward()

    def close(ours, theirs):   # a tensor the loss does not depend on has no grad: the restatement's zeros
        want = np.zeros(ours.shape) if theirs.grad is None else theirs.grad.numpy()
        return np.isfinite(ours).all() and ((ours == 0).all() if not want.any() else relative(ours, want) <= 1e-9)
    assert close(got.rot, tR) and (got.rot[~ok] == 0).all() and close(got.trans, tT)
    assert got.rot.any() == (not (bipartite and which == "pos")) and got.trans.any() == (which != "rot")
    if bipartite:
        assert close(got.src_rot, sR) and (got.src_rot[~oks] == 0).all() and close(got.src_trans, sT) and got.src_rot.any()


def test_the_sum_restatement_keeps_exact_zeros_and_rounds_once():
    B, M, A, P = 1, 3, 4, 3
    row_ptr = np.asarray([0, 2, 2, 3], dtype=np.int64)
    col = np.asarray([1, 1, 0], dtype=np.int32)
    f = np.zeros((3, P, 3), np.float32)
    f[0, 0], f[1, 0], f[2, 2] = (1.0, 2.0 ** -30, -0.0), (2.0 ** -30, 1.0, 0.0), (3.0, 0.0, 0.0)
    in_ptr, in_edge = G.incoming(row_ptr, col, B, M, M)
    out = G.pair_grad_sum(f, row_ptr, in_ptr, in_edge, [0, 1, 0], [2, 2, 2], B, M, A)
    assert out.grad[0, 0, 0, 0] == -(1.0 + 2.0 ** -30) and np.float32(out.grad[0, 0, 0, 0]) == np.float32(-1.0)   # held in double
    assert not np.signbit(out.grad[0, :, 3]).any() and (out.grad[0, :, 3] == 0).all()                 # a slot no pair names: +0
    assert (out.grad[0, 1, 2] == [1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, 0.0]).all() and not np.signbit(out.grad[0, 1, 2, 2])
    assert (out.grad[0, 2, 0] == [-3.0, 0.0, 0.0]).all() and (out.grad[0, 0, 2] == [3.0, 0.0, 0.0]).all()


# ---- 2. the incoming list ------------------------------------------------------------------------------------------------------------
def incoming_cases():
    rng = np.random.default_rng(4)
    cases = [("empty", 2, 3, 4, np.zeros(7, dtype=np.int64), np.zeros(0, dtype=np.int32)),
             ("no rows", 0, 3, 4, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)),
             ("no targets", 2, 2, 0, np.asarray([0, 1, 2, 2, 3], dtype=np.int64), np.asarray([0, -1, 0], dtype=np.int32))]
    row_ptr, col = C.graph_of_lengths([0, 4, 0, 2, 7, 0], 5, seed=1, E=13 + 4)         # a max_edges tail of -1
    cases.append(("tail", 2, 3, 5, row_ptr, col))
    row_ptr, col = C.graph_of_lengths([3, 0, 5, 1, 0, 6], 4, seed=2)
    col[[1, 7]] = [4, -7]                                                              # columns out of range inside rows
    cases.append(("out of range", 3, 2, 4, row_ptr, col))
    row_ptr, col = C.graph_of_lengths([5, 5, 0, 5], 6, seed=3, E=8)                    # a cut list: row_ptr[-1] = 15 > E = 8
    cases.append(("cut", 1, 4, 6, row_ptr, col))
    row_ptr, col = C.graph_of_lengths(rng.integers(0, 5, size=12), 3, seed=5)
    cases.append(("bipartite", 4, 3, 3, row_ptr, col.astype(np.int64)))
    return cases


@pytest.mark.parametrize("case", incoming_cases(), ids=lambda c: c[0])
def test_csr_incoming_edges_on_cpu_tensors_is_the_restatement(case):
    name, B, Q, M, row_ptr, col = case
    ptr, edge = ops.csr_incoming_edges(torch.from_numpy(row_ptr), torch.from_numpy(col), B, Q, M)
    want_ptr, want_edge = G.incoming(row_ptr, col, B, Q, M)
    assert ptr.dtype == edge.dtype == torch.int64 and tuple(ptr.shape) == (B * M + 1,) and tuple(edge.shape) == (len(col),)
    assert np.array_equal(ptr.numpy(), want_ptr) and np.array_equal(edge.numpy(), want_edge)
    # every group is ascending and holds exactly the edges of its target; the padding comes after ptr[-1]
    r = C.rows(row_ptr, len(col))
    for o in range(B * M):
        group = want_edge[want_ptr[o]:want_ptr[o + 1]]
        assert (np.diff(group) > 0).all() and (col[group] == o % M).all() and (r[group] // Q == o // M).all()
    rest = want_edge[want_ptr[-1]:]
    assert all(r[p] == B * Q or not 0 <= col[p] < M for p in rest) and sorted(want_edge) == list(range(len(col)))


def test_radius_graph_incoming_takes_arrays_and_cpu_tensors():
    row_ptr, col = C.graph_of_lengths([2, 0, 3, 1], 4, seed=9, E=8)
    count = np.diff(row_ptr).reshape(2, 2).astype(np.int32)
    graph = geometry.RadiusGraph(row_ptr, col, None, count)
    out = geometry.radius_graph_incoming(graph, 4)
    want = G.incoming(row_ptr, col, 2, 2, 4)
    assert isinstance(out, geometry.IncomingEdges) and isinstance(out.ptr, np.ndarray)
    assert np.array_equal(out.ptr, want[0]) and np.array_equal(out.edge, want[1])
    tensors = geometry.RadiusGraph(torch.from_numpy(row_ptr), torch.from_numpy(col), None, torch.from_numpy(count))
    out = geometry.radius_graph_incoming(tensors, 4)
    assert isinstance(out.ptr, torch.Tensor) and np.array_equal(out.edge.numpy(), want[1])
    with pytest.raises(TypeError, match="graph must be a geometry.RadiusGraph"):
        geometry.radius_graph_incoming((row_ptr, col), 4)
    with pytest.raises(ValueError, match="M must be a non-negative integer"):
        geometry.radius_graph_incoming(graph, -1)
    with pytest.raises(ValueError, match=r"row_ptr must have shape \(7,\)"):
        ops.csr_incoming_edges(torch.from_numpy(row_ptr), torch.from_numpy(col), 2, 3, 4)


# ---- 3. the header, the table, the library ---------------------------------------------------------------------------------------------
def test_header_is_c99():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(INCLUDE, HEADER)], check=True)


def test_header_binding_and_library_agree(lib):
    declared = declared_symbols(HEADER)
    assert declared == sorted(_edgegrad.EDGEGRAD_SIGNATURES) == sorted(ENTRY_POINTS + ["ps_edgegrad_api"])
    nm = subprocess.run(["nm", "-D", "--defined-only", build.EDGEGRAD_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)$", nm, flags=re.M))) == declared
    for table in ["SIGNATURES"] + [family.signatures for family in _lib.FAMILIES]:
        assert not set(declared) & set(getattr(_lib, table)), table
    assert not set(declared) & set(_csredge.CSREDGE_SIGNATURES)
    api = macros(HEADER)["PS_EDGEGRAD_API"]
    assert lib.ps_edgegrad_api() == api == _edgegrad.EXPECTED_EDGEGRAD_API == 1
    for name in ENTRY_POINTS:
        restype, argtypes = _edgegrad.EDGEGRAD_SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p                # the HIP error; the stream last
    assert _edgegrad.EDGEGRAD_SIGNATURES["ps_csr_edge_rbf_backward_f32"][1][6] is ctypes.c_longlong          # E
    assert _edgegrad.EDGEGRAD_SIGNATURES["ps_csr_edge_pair_grad_sum_f32"][1][2] is ctypes.c_longlong
    assert _edgegrad.EDGEGRAD_SIGNATURES["ps_csr_edge_frames_backward_f32"][1][8] is ctypes.c_longlong
    # K52 takes K50's arguments with the incoming gradients and pair_grad in place of the two outputs
    forward = _csredge.CSREDGE_SIGNATURES["ps_csr_edge_rbf_f32"][1]
    assert _edgegrad.EDGEGRAD_SIGNATURES["ps_csr_edge_rbf_backward_f32"][1] == forward[:15] + [ctypes.c_void_p] + forward[15:]


def test_the_names_follow_the_family_rule_and_the_conventions_are_those_of_the_forward_header():
    stem = "edgegrad"
    assert HEADER == f"protstruc_{stem}.h" and f"ps_{stem}_api" in _edgegrad.EDGEGRAD_SIGNATURES
    assert isinstance(getattr(_edgegrad, f"EXPECTED_{stem.upper()}_API"), int)
    assert "#define PS_EDGEGRAD_API 1" in header_text(HEADER)
    assert "edgegrad" not in {family.header for family in _lib.FAMILIES} and len(_lib.FAMILIES) == 6
    ours, theirs = header_text(HEADER), header_text("protstruc_csredge.h")
    for sentence in ("tensors are contiguous and need only the alignment of their element",
                     "`stream` is a `hipStream_t` passed as `void*` (NULL = the default stream)",
                     "launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory",
                     "the library holds no mutable state", "no kernel uses an atomic"):
        assert sentence in ours and sentence in theirs, sentence
    assert "-ffp-contract=off" in ours and "by reading" in ours
    # the header says which design each kernel is, and fixes the order of every sum
    for sentence in ("fours ascending", "then a tree over the K = ceil(R / 4) partial sums", "One lane owns one slot of one owner",
                     "ONE kernel that walks both lists and recomputes the terms", "p ascending, then those of its\n * incoming list"):
        assert sentence in ours, sentence


def test_the_limits_are_macros_of_the_forward_kernels():
    m, forward = macros(HEADER), macros("protstruc_csredge.h")
    assert (m["PS_EDGEGRAD_CHUNK"], m["PS_EDGEGRAD_MAX_PAIRS"], m["PS_EDGEGRAD_MAX_RBF"]) == \
        (forward["PS_CSREDGE_CHUNK"], forward["PS_CSREDGE_MAX_PAIRS"], forward["PS_CSREDGE_MAX_RBF"]) == (64, 64, 64)


def test_the_library_is_a_target_of_its_own():
    target = build._edgegrad_library()
    names = [os.path.basename(d) for d in target.inputs]
    assert "edge_features_backward.hip" in names and "ps_common.hpp" in names and HEADER in names
    assert all(os.path.dirname(s) == build.EDGEGRAD_SRC_DIR for s in build.edgegrad_sources()) and build.edgegrad_sources()
    assert not set(build.edgegrad_sources()) & set(build.sources())
    assert not set(build.edgegrad_sources()) & set(build.csredge_sources())
    assert HEADER not in {os.path.basename(d) for d in build._deps()}, "the main library's digest is as it was"
    assert HEADER not in {os.path.basename(d) for d in build._csredge_library().inputs}
    cmd = target.command("out.so")
    assert cmd[1:1 + len(build.FLAGS)] == build.FLAGS and "-I" + build.CSRC in cmd
    assert not build.edgegrad_is_stale()
    assert os.path.basename(build.EDGEGRAD_LIB_PATH) == "libprotstruc_edgegrad.so"


def test_the_entry_point_and_the_command_line_build_and_load_the_library(lib, monkeypatch):
    """what they do, not how they spell it: build() builds this library and loads it; the command line names it as built"""
    import __graft_entry__
    seen = []
    build_edgegrad, load = build.build_edgegrad, _edgegrad.load
    monkeypatch.setattr(build, "build_edgegrad", lambda *a, **kw: (seen.append("build"), build_edgegrad(*a, **kw))[1])
    monkeypatch.setattr(_edgegrad, "load", lambda: (seen.append("load"), load())[1])
    __graft_entry__.build()
    assert seen == ["build", "load"]
    out = subprocess.run([sys.executable, "-m", "protstruc_amd.build"], check=True, capture_output=True, text=True,
                         cwd=os.path.dirname(build.HERE)).stdout
    assert os.path.abspath(build.EDGEGRAD_LIB_PATH) in [os.path.abspath(line) for line in out.splitlines()]


def test_a_library_with_another_version_is_refused(lib, monkeypatch):
    bound = _edgegrad.EXPECTED_EDGEGRAD_API
    monkeypatch.setattr(_edgegrad, "_lib", None)
    monkeypatch.setattr(_edgegrad, "EXPECTED_EDGEGRAD_API", bound + 1)
    with pytest.raises(_lib.HipLibraryError) as info:
        _edgegrad.load()
    assert str(info.value) == (f"{_edgegrad.LIB_PATH} has edge-grad API version {bound}, this package binds version {bound + 1}: "
                               "rebuild with `python -m protstruc_amd.build --force`")


def test_a_missing_or_stale_library_is_refused(lib, monkeypatch, tmp_path):
    gone = str(tmp_path / "libprotstruc_edgegrad.so")
    monkeypatch.setattr(_edgegrad, "_lib", None)
    monkeypatch.setattr(_edgegrad, "LIB_PATH", gone)
    with pytest.raises(_lib.HipLibraryError) as info:
        _edgegrad.load()
    assert str(info.value) == (f"{gone} is missing: build it with `python -m protstruc_amd.build` "
                               "(hipcc --offload-arch=gfx950). protstruc_amd has no CPU fallback.")
    monkeypatch.undo()
    monkeypatch.setattr(_edgegrad, "_lib", None)
    monkeypatch.setattr(build, "edgegrad_is_stale", lambda path=None: True)
    monkeypatch.setattr(build, "HIPCC", "/nonexistent/hipcc")
    with pytest.raises(_lib.HipLibraryError) as info:
        _edgegrad.load()
    assert str(info.value).startswith(f"{_edgegrad.LIB_PATH} is older than its sources (csrc_edgegrad/*.hip, csrc/*.hpp, "
                                      "include/protstruc_edgegrad.h)")


# ---- every refusal of the three entry points ----------------------------------------------------------------------------------------------
def ints(*values):
    return (ctypes.c_int * len(values))(*values)


def floats(*values):
    return (ctypes.c_float * len(values))(*values)


def rbf_args(**changes):
    a = dict(xyz=FAKE, atom_mask=None, src_xyz=None, src_mask=None, row_ptr=FAKE, col=FAKE, E=0, pair_i=ints(0, 4), pair_j=ints(1, 2),
             P=2, centers=floats(2.0, 4.0, 6.0), R=3, sigma=1.25, g_dist=FAKE, g_rbf=FAKE, pair_grad=FAKE, B=2, M=7, A=5, Q=7, As=5)
    a.update(changes)
    return [a[k] for k in ("xyz", "atom_mask", "src_xyz", "src_mask", "row_ptr", "col", "E", "pair_i", "pair_j", "P", "centers",
                           "R", "sigma", "g_dist", "g_rbf", "pair_grad", "B", "M", "A", "Q", "As")] + [None]


def sum_args(**changes):
    a = dict(pair_grad=FAKE, row_ptr=FAKE, E=0, in_ptr=FAKE, in_edge=FAKE, E_in=0, pair_i=ints(0, 4), pair_j=ints(1, 2), P=2,
             grad=FAKE, grad_src=None, B=0, M=7, A=5, Q=7, As=5)
    a.update(changes)
    return [a[k] for k in ("pair_grad", "row_ptr", "E", "in_ptr", "in_edge", "E_in", "pair_i", "pair_j", "P", "grad", "grad_src",
                           "B", "M", "A", "Q", "As")] + [None]


def frames_args(**changes):
    a = dict(rot=FAKE, trans=FAKE, frame_mask=None, src_rot=None, src_trans=None, src_mask=None, row_ptr=FAKE, col=FAKE, E=0,
             in_ptr=FAKE, in_edge=FAKE, E_in=0, g_pos=FAKE, g_rot=FAKE, grad_rot=FAKE, grad_trans=FAKE, grad_src_rot=None,
             grad_src_trans=None, B=0, M=7, Q=7)
    a.update(changes)
    return [a[k] for k in ("rot", "trans", "frame_mask", "src_rot", "src_trans", "src_mask", "row_ptr", "col", "E", "in_ptr",
                           "in_edge", "E_in", "g_pos", "g_rot", "grad_rot", "grad_trans", "grad_src_rot", "grad_src_trans", "B", "M",
                           "Q")] + [None]


BIG = 2 ** 24 + 1
RBF_REFUSALS = [dict(B=-1), dict(B=65536), dict(M=-1), dict(M=BIG), dict(Q=-1, src_xyz=FAKE), dict(Q=BIG, src_xyz=FAKE), dict(E=-1),
                dict(A=0), dict(As=0, src_xyz=FAKE), dict(P=0), dict(P=65), dict(R=0), dict(R=65),
                dict(pair_i=ints(0, 5)), dict(pair_i=ints(-1, 0)), dict(pair_j=ints(1, 5)), dict(pair_j=ints(1, -2)),
                dict(pair_i=ints(0, 4), src_xyz=FAKE, As=4), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(sigma=float("inf")), dict(sigma=1e-39), dict(g_dist=None, g_rbf=None), dict(pair_grad=None),
                dict(Q=8), dict(As=6), dict(src_mask=FAKE),                             # src_xyz NULL: the sources are the targets
                dict(xyz=None), dict(row_ptr=None), dict(col=None), dict(pair_i=None), dict(pair_j=None), dict(centers=None)]
SUM_REFUSALS = [dict(B=-1), dict(B=65536), dict(M=-1), dict(M=BIG), dict(Q=-1, grad_src=FAKE), dict(Q=BIG, grad_src=FAKE),
                dict(E=-1), dict(E_in=-1), dict(A=0), dict(As=0, grad_src=FAKE), dict(P=0), dict(P=65),
                dict(pair_i=ints(0, 5)), dict(pair_i=ints(-1, 0)), dict(pair_j=ints(1, 5)), dict(pair_j=ints(1, -2)),
                dict(pair_i=ints(0, 4), grad_src=FAKE, As=4), dict(Q=8), dict(As=6),  # grad_src NULL: the sources are the targets
                dict(row_ptr=None), dict(in_ptr=None), dict(pair_i=None), dict(pair_j=None), dict(grad=None),
                dict(E=5, pair_grad=None), dict(E_in=5, in_edge=None)]
FRAMES_REFUSALS = [dict(B=-1), dict(B=65536), dict(M=-1), dict(M=BIG), dict(E=-1), dict(E_in=-1), dict(g_pos=None, g_rot=None),
                   dict(src_rot=FAKE), dict(src_trans=FAKE), dict(Q=8), dict(src_mask=FAKE), dict(grad_src_rot=FAKE),
                   dict(grad_src_trans=FAKE), dict(src_rot=FAKE, src_trans=FAKE),            # bipartite without its outputs
                   dict(src_rot=FAKE, src_trans=FAKE, grad_src_rot=FAKE),
                   dict(src_rot=FAKE, src_trans=FAKE, grad_src_rot=FAKE, grad_src_trans=FAKE, Q=-1),
                   dict(src_rot=FAKE, src_trans=FAKE, grad_src_rot=FAKE, grad_src_trans=FAKE, Q=BIG),
                   dict(rot=None), dict(trans=None), dict(row_ptr=None), dict(in_ptr=None), dict(grad_rot=None), dict(grad_trans=None),
                   dict(E=5, col=None), dict(E_in=5, in_edge=None)]


def test_the_base_arguments_are_accepted_and_an_empty_call_launches_nothing(lib):
    """B == 0 (and E == 0 in K52) returns 0 after every check and before any launch: what each refusal below changes is the
    reason"""
    assert lib.ps_csr_edge_rbf_backward_f32(*rbf_args()) == 0 and lib.ps_csr_edge_rbf_backward_f32(*rbf_args(B=0, E=5)) == 0
    assert lib.ps_csr_edge_rbf_backward_f32(*rbf_args(g_dist=None)) == 0 and lib.ps_csr_edge_rbf_backward_f32(*rbf_args(g_rbf=None)) == 0
    assert lib.ps_csr_edge_rbf_backward_f32(*rbf_args(src_xyz=FAKE, src_mask=FAKE, Q=3, As=9, pair_i=ints(8, 4))) == 0
    assert lib.ps_csr_edge_rbf_backward_f32(*rbf_args(P=64, pair_i=ints(*[0] * 64), pair_j=ints(*[1] * 64), R=64,
                                                      centers=floats(*range(64)))) == 0
    assert lib.ps_csr_edge_pair_grad_sum_f32(*sum_args()) == 0 and lib.ps_csr_edge_pair_grad_sum_f32(*sum_args(E=5, E_in=5)) == 0
    assert lib.ps_csr_edge_pair_grad_sum_f32(*sum_args(grad_src=FAKE, Q=3, As=9, pair_i=ints(8, 4))) == 0
    assert lib.ps_csr_edge_pair_grad_sum_f32(*sum_args(pair_grad=None, in_edge=None)) == 0
    assert lib.ps_csr_edge_frames_backward_f32(*frames_args()) == 0 and lib.ps_csr_edge_frames_backward_f32(*frames_args(E=5, E_in=5)) == 0
    assert lib.ps_csr_edge_frames_backward_f32(*frames_args(g_pos=None)) == 0 and lib.ps_csr_edge_frames_backward_f32(*frames_args(g_rot=None)) == 0
    assert lib.ps_csr_edge_frames_backward_f32(*frames_args(src_rot=FAKE, src_trans=FAKE, src_mask=FAKE, grad_src_rot=FAKE,
                                                            grad_src_trans=FAKE, Q=3)) == 0


@pytest.mark.parametrize("B", (0, 2))
def test_every_refusal_returns_invalid_value(lib, B):
    """with B = 2 and edges a call that was NOT refused would launch on pointers that are no memory: the refusal comes first"""
    live = dict(B=B, E=100, E_in=100) if B else {}
    for changes in RBF_REFUSALS:
        assert lib.ps_csr_edge_rbf_backward_f32(*rbf_args(**{"E": 100 if B else 0, **changes})) == INVALID, changes
    for changes in SUM_REFUSALS:
        assert lib.ps_csr_edge_pair_grad_sum_f32(*sum_args(**{**live, **changes})) == INVALID, changes
    for changes in FRAMES_REFUSALS:
        assert lib.ps_csr_edge_frames_backward_f32(*frames_args(**{**live, **changes})) == INVALID, changes


# ---- the argument checks of ops -----------------------------------------------------------------------------------------------------------
def rbf_operands():
    xyz = torch.zeros(2, 7, 5, 3)
    row_ptr = torch.arange(15, dtype=torch.int64) * 2
    col = torch.zeros(28, dtype=torch.int32)
    tables = dict(pair_i=[0, 4], pair_j=[1, 2], centers=[2.0, 4.0, 6.0], sigma=1.25)
    return xyz, row_ptr, col, tables


def test_ops_refuses_wrong_gradients_and_lists():
    xyz, row_ptr, col, tables = rbf_operands()
    check = ops.check_csr_edge_rbf_backward_shapes
    assert check(xyz, row_ptr, col, grad_rbf=torch.zeros(28, 6), **tables) == (2, 7, 5, 7, 5, 28)
    with pytest.raises(ValueError, match="nothing to compute: grad_dist and grad_rbf are both None"):
        check(xyz, row_ptr, col, **tables)
    with pytest.raises(ValueError, match=r"grad_rbf must have shape \(28, 6\)"):
        check(xyz, row_ptr, col, grad_rbf=torch.zeros(28, 5), **tables)
    with pytest.raises(ValueError, match=r"grad_dist must have shape \(28, 2\)"):
        check(xyz, row_ptr, col, grad_dist=torch.zeros(28, 3), **tables)
    with pytest.raises(ValueError, match="grad_dist must be a floating-point tensor"):
        check(xyz, row_ptr, col, grad_dist=torch.zeros(28, 2, dtype=torch.int32), **tables)
    with pytest.raises(ValueError, match=r"row_ptr must have shape \(15,\)"):
        check(xyz, row_ptr[:-1], col, grad_dist=torch.zeros(28, 2), **tables)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.csr_edge_rbf_backward(xyz, row_ptr, col, grad_dist=torch.zeros(28, 2), **tables)

    in_ptr, in_edge = ops.csr_incoming_edges(row_ptr, col, 2, 7, 7)
    sums = ops.check_csr_edge_pair_grad_sum_shapes
    pairs = dict(pair_i=[0, 4], pair_j=[1, 2])
    assert sums(torch.zeros(28, 2, 3), row_ptr, in_ptr, in_edge, B=2, M=7, A=5, **pairs) == (7, 5, 28)
    with pytest.raises(ValueError, match=r"pair_grad must be a floating-point tensor of shape \(edges, 2, 3\)"):
        sums(torch.zeros(28, 3, 3), row_ptr, in_ptr, in_edge, B=2, M=7, A=5, **pairs)
    with pytest.raises(ValueError, match="Q and As come together"):
        sums(torch.zeros(28, 2, 3), row_ptr, in_ptr, in_edge, B=2, M=7, A=5, Q=7, **pairs)
    with pytest.raises(ValueError, match=r"in_ptr must be an int64 tensor of shape \(15,\)"):
        sums(torch.zeros(28, 2, 3), row_ptr, in_ptr[:-1], in_edge, B=2, M=7, A=5, **pairs)
    with pytest.raises(ValueError, match="in_edge must be an int64 tensor"):
        sums(torch.zeros(28, 2, 3), row_ptr, in_ptr, in_edge.int(), B=2, M=7, A=5, **pairs)
    with pytest.raises(ValueError, match=r"row_ptr must be an integer tensor of shape \(7,\)"):
        sums(torch.zeros(28, 2, 3), row_ptr, in_ptr, in_edge, B=2, M=7, A=5, Q=3, As=5, **pairs)
    with pytest.raises(ValueError, match=r"atom slot 4 outside \[0, 4\)"):
        sums(torch.zeros(28, 2, 3), row_ptr, in_ptr, in_edge, B=2, M=7, A=5, Q=7, As=4, **pairs)

    rot, trans = torch.zeros(2, 7, 3, 3), torch.zeros(2, 7, 3)
    frames = ops.check_csr_edge_frames_backward_shapes
    assert frames(rot, trans, row_ptr, col, in_ptr, in_edge, grad_pos=torch.zeros(28, 3)) == (2, 7, 7, 28)
    with pytest.raises(ValueError, match="nothing to compute: grad_pos and grad_rot are both None"):
        frames(rot, trans, row_ptr, col, in_ptr, in_edge)
    with pytest.raises(ValueError, match=r"grad_rot must have shape \(28, 3, 3\)"):
        frames(rot, trans, row_ptr, col, in_ptr, in_edge, grad_rot=torch.zeros(28, 9))
    with pytest.raises(ValueError, match=r"in_ptr must be an int64 tensor of shape \(15,\)"):
        frames(rot, trans, row_ptr, col, in_ptr.int(), in_edge, grad_pos=torch.zeros(28, 3))


def test_without_grad_the_public_functions_take_the_forward_path_alone():
    """numpy inputs and tensors that do not require grad never reach the autograd functions; what decides is one predicate"""
    x = torch.zeros(1, 2, 3, 3)
    assert not geometry._wants_grad(x, None, np.zeros(3)) and geometry._wants_grad(x.clone().requires_grad_())
    with torch.no_grad():
        assert not geometry._wants_grad(x.clone().requires_grad_())
    assert not geometry._wants_grad(torch.zeros(3, dtype=torch.int64))
    for doc in (geometry.edge_distance_features, geometry.edge_frame_features, geometry.radius_edge_distance_features,
                geometry.radius_edge_frame_features):
        assert "Differentiable with respect to" in doc.__doc__ and "no backward kernel exists" not in doc.__doc__
