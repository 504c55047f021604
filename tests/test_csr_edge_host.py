"""The edge features on CSR graphs (K49 - K51) without a GPU: the header, the binding table and the cross-compiled library
held to each other, the loader's refusals, every refusal of the three entry points (nothing is launched: no device is
needed to be refused), the restatement's r(p) held to numpy's search and its features held to tests/edge_ref.py on the same
edges, ``geometry.neighbors_to_radius_graph``, and the argument checks of ``ops`` with their messages."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from protstruc_amd import _csredge, _lib, build, geometry, ops
from tests import csr_edge_ref as C, edge_ref as E
from tests.c_headers import INCLUDE, declared_symbols, header_text, macros

HEADER = "protstruc_csredge.h"
ENTRY_POINTS = ["ps_csr_edge_frames_f32", "ps_csr_edge_rbf_f32", "ps_csr_edge_rows_i32"]
INVALID = 1          # hipErrorInvalidValue
FAKE = 0x1000        # a device pointer that is not NULL; a refused call never uses it


@pytest.fixture(scope="module")
def lib():
    build.build_csredge(force=False, verbose=False)      # hipcc cross-compiles gfx950 without a GPU
    return _csredge.load()


# ---- the header, the table, the library ----------------------------------------------------------------------------------------
def test_header_is_c99():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(INCLUDE, HEADER)], check=True)


def test_header_binding_and_library_agree(lib):
    declared = declared_symbols(HEADER)
    assert declared == sorted(_csredge.CSREDGE_SIGNATURES) == sorted(ENTRY_POINTS + ["ps_csredge_api"])
    nm = subprocess.run(["nm", "-D", "--defined-only", build.CSREDGE_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)$", nm, flags=re.M))) == declared
    for table in ["SIGNATURES"] + [family.signatures for family in _lib.FAMILIES]:
        assert not set(declared) & set(getattr(_lib, table)), table
    api = macros(HEADER)["PS_CSREDGE_API"]
    assert lib.ps_csredge_api() == api == _csredge.EXPECTED_CSREDGE_API
    for name in ENTRY_POINTS:
        restype, argtypes = _csredge.CSREDGE_SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p                # the HIP error; the stream last
    assert _csredge.CSREDGE_SIGNATURES["ps_csr_edge_rows_i32"][1][:4] == [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                                                           ctypes.c_longlong]
    assert _csredge.CSREDGE_SIGNATURES["ps_csr_edge_rbf_f32"][1][6] is ctypes.c_longlong  # E
    assert _csredge.CSREDGE_SIGNATURES["ps_csr_edge_frames_f32"][1][8] is ctypes.c_longlong


def test_the_names_follow_the_family_rule():
    """ps_<stem>_api, protstruc_<stem>.h, EXPECTED_<STEM>_API: what one line of _lib.FAMILIES would name"""
    stem = "csredge"
    assert HEADER == f"protstruc_{stem}.h" and f"ps_{stem}_api" in _csredge.CSREDGE_SIGNATURES
    assert isinstance(getattr(_csredge, f"EXPECTED_{stem.upper()}_API"), int)
    assert "#define PS_CSREDGE_API 1" in header_text(HEADER)
    # the conventions paragraph of protstruc_graph.h
    ours, theirs = header_text(HEADER), header_text("protstruc_graph.h")
    for sentence in ("tensors are contiguous and need only the alignment of their element",
                     "`stream` is a `hipStream_t` passed as `void*` (NULL = the default stream)",
                     "launches are asynchronous, perform no allocation, no synchronisation and no host read of device memory",
                     "the library holds no mutable state", "no kernel uses an atomic"):
        assert sentence in ours and sentence in theirs, sentence
    assert "-ffp-contract=off" in ours and "by reading" in ours


def test_the_limits_are_macros_and_ops_mirrors_them():
    m = macros(HEADER)
    assert (m["PS_CSREDGE_CHUNK"], m["PS_CSREDGE_MAX_PAIRS"], m["PS_CSREDGE_MAX_RBF"]) == (64, 64, 64)
    assert (ops.CSREDGE_CHUNK, ops.CSREDGE_MAX_PAIRS, ops.CSREDGE_MAX_RBF) == (64, 64, 64)
    assert m["PS_CSREDGE_MAX_PAIRS"] == macros("protstruc_hip.h")["PS_EDGE_MAX_PAIRS"]
    assert m["PS_CSREDGE_MAX_RBF"] == macros("protstruc_hip.h")["PS_EDGE_MAX_RBF"]


def test_the_library_is_a_target_of_its_own():
    target = build._csredge_library()
    names = [os.path.basename(d) for d in target.inputs]
    assert "csr_edge_features.hip" in names and "ps_common.hpp" in names and HEADER in names
    assert all(os.path.dirname(s) == build.CSREDGE_SRC_DIR for s in build.csredge_sources())
    assert not set(build.csredge_sources()) & set(build.sources())
    assert HEADER not in {os.path.basename(d) for d in build._deps()}, "the main library's digest is as it was"
    cmd = target.command("out.so")
    assert cmd[1:1 + len(build.FLAGS)] == build.FLAGS and "-I" + build.CSRC in cmd
    assert not build.csredge_is_stale()
    assert os.path.basename(build.CSREDGE_LIB_PATH) == "libprotstruc_csredge.so"


# ---- the loader's refusals, in the words of _lib.load() --------------------------------------------------------------------------
def test_a_library_with_another_version_is_refused(lib, monkeypatch):
    bound = _csredge.EXPECTED_CSREDGE_API
    monkeypatch.setattr(_csredge, "_lib", None)
    monkeypatch.setattr(_csredge, "EXPECTED_CSREDGE_API", bound + 1)
    with pytest.raises(_lib.HipLibraryError) as info:
        _csredge.load()
    assert str(info.value) == (f"{_csredge.LIB_PATH} has csr-edge API version {bound}, this package binds version {bound + 1}: "
                               "rebuild with `python -m protstruc_amd.build --force`")


def test_a_missing_library_is_refused(lib, monkeypatch, tmp_path):
    gone = str(tmp_path / "libprotstruc_csredge.so")
    monkeypatch.setattr(_csredge, "_lib", None)
    monkeypatch.setattr(_csredge, "LIB_PATH", gone)
    with pytest.raises(_lib.HipLibraryError) as info:
        _csredge.load()
    assert str(info.value) == (f"{gone} is missing: build it with `python -m protstruc_amd.build` "
                               "(hipcc --offload-arch=gfx950). protstruc_amd has no CPU fallback.")


def test_a_stale_library_is_refused_where_it_cannot_be_rebuilt(lib, monkeypatch):
    monkeypatch.setattr(_csredge, "_lib", None)
    monkeypatch.setattr(build, "csredge_is_stale", lambda path=None: True)
    monkeypatch.setattr(build, "HIPCC", "/nonexistent/hipcc")
    with pytest.raises(_lib.HipLibraryError) as info:
        _csredge.load()
    assert str(info.value).startswith(f"{_csredge.LIB_PATH} is older than its sources (csrc_csredge/*.hip, csrc/*.hpp, "
                                      "include/protstruc_csredge.h)")
    assert "run `python -m protstruc_amd.build --force` where hipcc is available" in str(info.value)


def test_a_library_without_the_version_symbol_is_refused(lib, monkeypatch):
    monkeypatch.setattr(_csredge, "_lib", None)
    build.build(force=False, verbose=False)
    monkeypatch.setattr(_csredge, "LIB_PATH", build.LIB_PATH)      # a library of this package, but not this one
    with pytest.raises(_lib.HipLibraryError, match="does not export ps_csredge_api: not a protstruc_amd library"):
        _csredge.load()


# ---- every refusal of the three entry points --------------------------------------------------------------------------------------
def ints(*values):
    return (ctypes.c_int * len(values))(*values)


def floats(*values):
    return (ctypes.c_float * len(values))(*values)


def rows_args(**changes):
    a = dict(row_ptr=FAKE, n_rows=6, Q=3, E=0, batch=FAKE, row=FAKE)
    a.update(changes)
    return [a[k] for k in ("row_ptr", "n_rows", "Q", "E", "batch", "row")] + [None]


def rbf_args(**changes):
    a = dict(xyz=FAKE, atom_mask=None, src_xyz=None, src_mask=None, row_ptr=FAKE, col=FAKE, E=0, pair_i=ints(0, 4), pair_j=ints(1, 2),
             P=2, centers=floats(2.0, 4.0, 6.0), R=3, sigma=1.25, dist=FAKE, rbf=FAKE, B=2, M=7, A=5, Q=7, As=5)
    a.update(changes)
    return [a[k] for k in ("xyz", "atom_mask", "src_xyz", "src_mask", "row_ptr", "col", "E", "pair_i", "pair_j", "P", "centers",
                           "R", "sigma", "dist", "rbf", "B", "M", "A", "Q", "As")] + [None]


def frames_args(**changes):
    a = dict(rot=FAKE, trans=FAKE, frame_mask=None, src_rot=None, src_trans=None, src_mask=None, row_ptr=FAKE, col=FAKE, E=0,
             local_pos=FAKE, rel_rot=FAKE, B=2, M=7, Q=7)
    a.update(changes)
    return [a[k] for k in ("rot", "trans", "frame_mask", "src_rot", "src_trans", "src_mask", "row_ptr", "col", "E", "local_pos",
                           "rel_rot", "B", "M", "Q")] + [None]


BIG = 2 ** 24 + 1
ROWS_REFUSALS = [dict(n_rows=-1), dict(n_rows=7), dict(Q=-1), dict(Q=BIG, n_rows=BIG), dict(Q=0, n_rows=6), dict(E=-1),
                 dict(n_rows=65536 * 3), dict(row_ptr=None), dict(batch=None), dict(row=None)]
RBF_REFUSALS = [dict(B=-1), dict(B=65536), dict(M=-1), dict(M=BIG), dict(Q=-1, src_xyz=FAKE), dict(Q=BIG, src_xyz=FAKE), dict(E=-1),
                dict(A=0), dict(As=0, src_xyz=FAKE), dict(P=0), dict(P=65), dict(R=0), dict(R=65),
                dict(pair_i=ints(0, 5)), dict(pair_i=ints(-1, 0)), dict(pair_j=ints(1, 5)), dict(pair_j=ints(1, -2)),
                dict(pair_i=ints(0, 4), src_xyz=FAKE, As=4), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(sigma=float("inf")), dict(sigma=1e-39), dict(dist=None, rbf=None),
                dict(Q=8), dict(As=6), dict(src_mask=FAKE),                             # src_xyz NULL: the sources are the targets
                dict(xyz=None), dict(row_ptr=None), dict(col=None), dict(pair_i=None), dict(pair_j=None), dict(centers=None)]
FRAMES_REFUSALS = [dict(B=-1), dict(B=65536), dict(M=-1), dict(M=BIG), dict(Q=-1, src_rot=FAKE, src_trans=FAKE),
                   dict(Q=BIG, src_rot=FAKE, src_trans=FAKE), dict(E=-1), dict(local_pos=None, rel_rot=None),
                   dict(src_rot=FAKE), dict(src_trans=FAKE), dict(Q=8), dict(src_mask=FAKE),
                   dict(rot=None), dict(trans=None), dict(row_ptr=None), dict(col=None)]


def test_the_base_arguments_are_accepted_and_an_empty_call_launches_nothing(lib):
    """E == 0 and B == 0 return 0 after every check and before any launch: what each refusal below changes is the reason"""
    assert lib.ps_csr_edge_rows_i32(*rows_args()) == 0
    assert lib.ps_csr_edge_rbf_f32(*rbf_args()) == 0 and lib.ps_csr_edge_frames_f32(*frames_args()) == 0
    assert lib.ps_csr_edge_rbf_f32(*rbf_args(B=0, E=5)) == 0 and lib.ps_csr_edge_frames_f32(*frames_args(B=0, E=5)) == 0
    assert lib.ps_csr_edge_rows_i32(*rows_args(Q=0, n_rows=0)) == 0
    # each output alone, a bipartite call and the limits of the tables are fine too
    assert lib.ps_csr_edge_rbf_f32(*rbf_args(dist=None)) == 0 and lib.ps_csr_edge_rbf_f32(*rbf_args(rbf=None)) == 0
    assert lib.ps_csr_edge_rbf_f32(*rbf_args(src_xyz=FAKE, src_mask=FAKE, Q=3, As=9, pair_i=ints(8, 4))) == 0
    assert lib.ps_csr_edge_rbf_f32(*rbf_args(P=64, pair_i=ints(*[0] * 64), pair_j=ints(*[1] * 64), R=64,
                                             centers=floats(*range(64)))) == 0
    assert lib.ps_csr_edge_frames_f32(*frames_args(src_rot=FAKE, src_trans=FAKE, src_mask=FAKE, Q=3)) == 0
    assert lib.ps_csr_edge_frames_f32(*frames_args(local_pos=None)) == 0 and lib.ps_csr_edge_frames_f32(*frames_args(rel_rot=None)) == 0


@pytest.mark.parametrize("E", (0, 100))
def test_every_refusal_returns_invalid_value(lib, E):
    """with E = 100 a call that was NOT refused would launch on pointers that are no memory: the refusal comes first"""
    for changes in ROWS_REFUSALS:
        assert lib.ps_csr_edge_rows_i32(*rows_args(**{"E": E, **changes})) == INVALID, changes
    for changes in RBF_REFUSALS:
        assert lib.ps_csr_edge_rbf_f32(*rbf_args(**{"E": E, **changes})) == INVALID, changes
    for changes in FRAMES_REFUSALS:
        assert lib.ps_csr_edge_frames_f32(*frames_args(**{"E": E, **changes})) == INVALID, changes


def test_null_device_pointers_are_refused(lib):
    null = dict(xyz=None, row_ptr=None, col=None, dist=None, rbf=None)
    assert lib.ps_csr_edge_rbf_f32(*rbf_args(E=100, **null)) == INVALID
    assert lib.ps_csr_edge_rows_i32(*rows_args(E=100, row_ptr=None, batch=None, row=None)) == INVALID
    assert lib.ps_csr_edge_frames_f32(*frames_args(E=100, rot=None, trans=None, row_ptr=None, col=None, local_pos=None,
                                                   rel_rot=None)) == INVALID


# ---- r(p) -----------------------------------------------------------------------------------------------------------------------------
def row_ptr_cases():
    rng = np.random.default_rng(3)
    cases = []
    for lengths in ([0, 0, 0, 5, 1, 0, 0, 0, 0, 70, 3, 0, 0],            # empty runs at the start, in the middle, at the end
                    [0] * 50 + [1] + [0] * 50, [3], [0], [], [0, 0, 0], [64, 64], [1] * 130,
                    list(rng.integers(0, 4, size=200)), list(C.chunk_lengths(193, 120)), list(C.chunk_lengths(64, 60))):
        row_ptr = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)
        total = int(row_ptr[-1])
        for E in sorted({0, max(total - 3, 0), total, total + 5, total // 2}):   # row_ptr[-1] above, equal to and below E
            cases.append((row_ptr, E))
    return cases


def test_rows_of_the_restatement_are_numpys_upper_bound():
    seen = set()
    for row_ptr, E in row_ptr_cases():
        r = C.rows(row_ptr, E)
        want = np.searchsorted(row_ptr[1:], np.arange(E), side="right")
        assert np.array_equal(r, want), (row_ptr, E)
        n_rows = len(row_ptr) - 1
        assert ((0 <= r) & (r <= n_rows)).all()
        inside = r < n_rows
        assert (row_ptr[r[inside]] <= np.arange(E)[inside]).all() and (np.arange(E)[inside] < row_ptr[r[inside] + 1]).all()
        assert (np.arange(E)[~inside] >= row_ptr[-1]).all()
        seen.add(int(np.sign(int(row_ptr[-1]) - E)))
        for Q in (q for q in (1, 2, 3, 5) if n_rows % q == 0):
            batch, row = C.edge_rows(row_ptr, Q, E)
            assert batch.dtype == row.dtype == np.int32
            assert np.array_equal(batch[inside] * Q + row[inside], r[inside]) and (row[inside] < Q).all()
            assert (batch[~inside] == -1).all() and (row[~inside] == -1).all()
    assert seen == {-1, 0, 1}


def test_chunk_lengths_hold_what_the_gpu_cases_need():
    for E in C.CHUNK_EDGES:
        lengths = C.chunk_lengths(E, 150)
        row_ptr = np.concatenate([[0], np.cumsum(lengths)])
        assert len(lengths) == 150 and row_ptr[-1] == E and lengths[0] == 0 and lengths[-1] == 0
        if E >= 64:
            assert 64 in row_ptr[1:-1], "a row ends exactly on a chunk boundary"
            starts_in_chunk_0 = ((row_ptr[:-1] < 64) & (lengths <= 1)).sum()
            assert starts_in_chunk_0 > 40, "a chunk holds more than 40 rows of length 0 and 1"
        if E >= 193:
            assert any(row_ptr[r] // 64 + 2 <= (row_ptr[r + 1] - 1) // 64 for r in range(150) if lengths[r]), "a row spans three chunks"


# ---- the restatement against tests/edge_ref.py on the same edges ---------------------------------------------------------------------
@pytest.mark.parametrize("N,k", ((1, 1), (7, 3), (65, 7)))
def test_the_restatement_is_edge_refs_on_the_same_edges(N, k):
    case = E.residue_case(N, 5, seed=3)
    idx = E.random_graph(3, N, k, seed=N + k)
    pairs = [(0, 1), (4, 4), (2, 0)]
    centers, sigma = geometry.rbf_centers(5, 0.0, 8.0)
    row_ptr, col, keep = C.to_csr(idx)
    padded = E.edge_rbf(case.xyz, idx, case.mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    flat = C.edge_rbf(case.xyz, row_ptr, col, case.mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    assert np.array_equal(flat.dist.view(np.int32), padded.dist[keep].view(np.int32))
    assert np.array_equal(flat.rbf, padded.rbf[keep]) and np.array_equal(flat.real, padded.real[keep])
    rot, trans = E.random_frames(3, N, seed=N)
    mask = np.random.default_rng(N).random((3, N)) >= 0.3
    rot[~mask], trans[~mask] = np.nan, np.nan
    pf, ff = E.edge_frames(rot, trans, idx, mask), C.edge_frames(rot, trans, row_ptr, col, mask)
    assert np.array_equal(ff.local_pos.view(np.int32), pf.local_pos[keep].view(np.int32))
    assert np.array_equal(ff.rel_rot.view(np.int32), pf.rel_rot[keep].view(np.int32)) and np.array_equal(ff.real, pf.real[keep])
    # the tail of a longer buffer and a col outside the range are exact zeros
    longer = np.concatenate([col, np.array([0, 2 ** 31 - 1, -7], dtype=np.int32)])
    tail = C.edge_rbf(case.xyz, row_ptr, longer, case.mask, [0], [1], centers, sigma)
    assert not tail.real[len(col):].any() and not tail.dist[len(col):].any() and not tail.rbf[len(col):].any()


# ---- neighbors_to_radius_graph ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k", ((1, 1, 1), (3, 7, 3), (2, 65, 30)))
def test_neighbors_to_radius_graph_round_trips(B, N, k):
    idx = E.random_graph(B, N, k, seed=B + N + k)
    row_ptr, col, keep = C.to_csr(idx)
    dist = np.random.default_rng(1).random((B, N, k)).astype(np.float32)
    for make in (np.asarray, torch.from_numpy):
        g = geometry.neighbors_to_radius_graph(make(idx))
        assert isinstance(g, geometry.RadiusGraph) and g.dist is None
        assert isinstance(g.col, np.ndarray if make is np.asarray else torch.Tensor)
        got = [np.asarray(t) for t in (g.row_ptr, g.col, g.count)]
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
        assert np.array_equal(got[0], row_ptr) and np.array_equal(got[1], col) and np.array_equal(got[2], keep.sum(-1))
        # back to the padded form: row r holds its entries in their order
        back = np.full((B * N, k), -1, dtype=np.int32)
        for r in range(B * N):
            back[r, :got[0][r + 1] - got[0][r]] = got[1][got[0][r]:got[0][r + 1]]
        assert np.array_equal(np.sort(back, axis=1), np.sort(idx.reshape(B * N, k), axis=1))
        g = geometry.neighbors_to_radius_graph(geometry.Neighbors(make(idx), make(dist), make(keep.sum(-1).astype(np.int32))))
        assert np.array_equal(np.asarray(g.dist), dist[keep]) and np.array_equal(np.asarray(g.col), col)
    with pytest.raises(ValueError, match=r"idx must be an integer tensor of shape \(B, Q, k\)"):
        geometry.neighbors_to_radius_graph(torch.zeros(2, 3))
    with pytest.raises(ValueError, match=r"idx must be an integer tensor of shape \(B, Q, k\)"):
        geometry.neighbors_to_radius_graph(torch.zeros(2, 3, 4))


# ---- the argument checks of ops --------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_shape_checks():
    B, M, A, Q, As, n = 2, 5, 5, 3, 4, 9
    f = torch.zeros
    xyz, src = f(B, M, A, 3), f(B, Q, As, 3)
    rp_self, rp_src, col = f(B * M + 1, dtype=torch.int64), f(B * Q + 1, dtype=torch.int64), f(n, dtype=torch.int32)
    kw = dict(pair_i=(0, 1), pair_j=(1, 0), centers=(2.0, 4.0), sigma=1.0)
    rbf = ops.check_csr_edge_rbf_shapes
    assert rbf(xyz, rp_self, col, **kw) == (B, M, A, M, A, n)
    assert rbf(xyz, rp_src, col, src_xyz=src, src_mask=f(B, Q, As), **{**kw, "pair_i": (3, 0)}) == (B, M, A, Q, As, n)
    refusals = [
        ((f(B, M, A), rp_self, col), {}, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
        ((f(65536, 1, 1, 3, device="meta"), rp_self, col), {}, "at most 65535 structures per call, got 65536"),
        ((xyz, rp_src, col), {}, "row_ptr must have shape (11,) to match the 2 x 5 sources of xyz (2, 5, 5, 3), got (7,)"),
        ((xyz, rp_self, col), {"src_xyz": src},
         "row_ptr must have shape (7,) to match the 2 x 3 sources of src_xyz (2, 3, 4, 3), got (11,)"),
        ((xyz, rp_self.float(), col), {}, "row_ptr must be an integer tensor, got torch.float32"),
        ((xyz, rp_self, f(n, 2, dtype=torch.int32)), {}, "col must have shape (edges,), got (9, 2)"),
        ((xyz, rp_self, f(n)), {}, "col must be an integer tensor, got torch.float32"),
        ((xyz, rp_self, col, f(B, M, 4)), {}, "atom_mask must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
        ((xyz, rp_self, col), {"src_mask": f(B, M, A)}, "src_mask needs src_xyz: where the sources are the targets, atom_mask is used"),
        ((xyz, rp_src, col), {"src_xyz": f(3, Q, As, 3)},
         "src_xyz must have shape (2, queries, atoms, 3) to match xyz (2, 5, 5, 3), got (3, 3, 4, 3)"),
        ((xyz, rp_src, col), {"src_xyz": src.long()}, "src_xyz must be a floating-point tensor, got torch.int64"),
        ((xyz, rp_src, col), {"src_xyz": src, "src_mask": f(B, Q, 5)},
         "src_mask must have shape (2, 3, 4) to match src_xyz (2, 3, 4, 3), got (2, 3, 5)"),
        ((xyz, rp_src, col), {"src_xyz": src, "pair_i": (4, 0)}, "atom slot 4 outside [0, 4)"),
        ((xyz, rp_self, col), {"pair_j": (1, 5)}, "atom slot 5 outside [0, 5)"),
        ((xyz, rp_self, col), {"pair_j": (1,)}, "pair_i and pair_j must be equally long, 1 .. 64 atom slots each, got 2 and 1"),
        ((xyz, rp_self, col), {"pair_i": 1}, "pair_i and pair_j must be sequences of atom slots"),
        ((xyz, rp_self, col), {"centers": ()}, "centers must hold 1 .. 64 values, got 0"),
        ((xyz, rp_self, col), {"centers": np.arange(65.0)}, "centers must hold 1 .. 64 values, got 65"),
        ((xyz, rp_self, col), {"sigma": 0}, "sigma must be positive and finite, got 0"),
        ((xyz, rp_self, col), {"want_dist": False, "want_rbf": False}, "nothing to compute: want_dist and want_rbf are both False"),
        ((xyz, rp_self, f(n, dtype=torch.int32, device="meta")), {}, "`col` lives on meta, the coordinates on cpu"),
    ]
    for args, changes, message in refusals:
        with pytest.raises(ValueError) as info:
            rbf(*args, **{**kw, **changes})
        assert str(info.value) == message, message
    rot, trans = f(B, M, 3, 3), f(B, M, 3)
    frames = ops.check_csr_edge_frames_shapes
    assert frames(rot, trans, rp_self, col, f(B, M)) == (B, M, M, n)
    assert frames(rot, trans, rp_src, col, src_rot=f(B, Q, 3, 3), src_trans=f(B, Q, 3), src_mask=f(B, Q)) == (B, M, Q, n)
    refusals = [
        ((f(B, M, 3), trans, rp_self, col), {}, "rot must have shape (batch, frames, 3, 3), got (2, 5, 3)"),
        ((rot, f(B, M, 2), rp_self, col), {}, "trans must have shape (2, 5, 3) to match rot (2, 5, 3, 3), got (2, 5, 2)"),
        ((rot, trans, rp_self, col, f(B, 4)), {}, "frame_mask must have shape (2, 5) to match rot (2, 5, 3, 3), got (2, 4)"),
        ((rot, trans, rp_src, col), {}, "row_ptr must have shape (11,) to match the 2 x 5 sources of rot (2, 5, 3, 3), got (7,)"),
        ((rot, trans, rp_src, col), {"src_rot": f(B, Q, 3, 3)}, "src_rot and src_trans come together: the sources' frames"),
        ((rot, trans, rp_self, col), {"src_mask": f(B, M)},
         "src_mask needs src_rot and src_trans: where the sources are the targets, frame_mask is used"),
        ((rot, trans, rp_src, col), {"src_rot": f(B, Q, 3), "src_trans": f(B, Q, 3)},
         "src_rot must have shape (2, queries, 3, 3) to match rot (2, 5, 3, 3), got (2, 3, 3)"),
        ((rot, trans, rp_src, col), {"src_rot": f(B, Q, 3, 3), "src_trans": f(B, Q, 2)},
         "src_trans must have shape (2, 3, 3) to match src_rot (2, 3, 3, 3), got (2, 3, 2)"),
        ((rot, trans, rp_self, col), {"want_pos": False, "want_rot": False}, "nothing to compute: want_pos and want_rot are both False"),
    ]
    for args, changes, message in refusals:
        with pytest.raises(ValueError) as info:
            frames(*args, **changes)
        assert str(info.value) == message, message
    rows = ops.check_csr_edge_rows_shapes
    assert rows(rp_self, M, n) == B and rows(f(1, dtype=torch.int64), 0, 4) == 0
    for args, message in (((rp_self, 3, n), "row_ptr holds 10 rows, no multiple of Q = 3"),
                          ((rp_self, -1, n), "Q must be a non-negative integer, got -1"),
                          ((rp_self, M, 2.0), "E must be a non-negative integer, got 2.0"),
                          ((rp_self, 0, n), "row_ptr holds 10 rows, no multiple of Q = 0"),
                          ((rp_self.float(), M, n), "row_ptr must be an integer tensor, got torch.float32"),
                          ((f(2, 3, dtype=torch.int64), M, n), "row_ptr must have shape (rows + 1,), got (2, 3)"),
                          ((f(65536 + 1, dtype=torch.int64, device="meta"), 1, n), "at most 65535 structures per call, got 65536")):
        with pytest.raises(ValueError) as info:
            rows(*args)
        assert str(info.value) == message, message


def test_cpu_tensors_are_refused_by_the_launchers():
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.csr_edge_rows(torch.zeros(3, dtype=torch.int64), 1, 4)


def test_the_public_functions_have_the_signatures_of_the_issue():
    from protstruc_amd import StructureBatch
    from protstruc_amd.structure_batch import AtomEdgeFeatures, RadiusEdgeFeatures
    sig = lambda fn: str(inspect.signature(fn)).split(" ->")[0]   # noqa: E731
    assert sig(geometry.radius_edge_rows) == "(graph)"
    assert sig(geometry.radius_edge_distance_features) == (
        "(xyz, graph, atom_mask=None, pairs=" + repr(geometry.BACKBONE_PAIRS) + ", centers=None, sigma=None, return_dist=False, "
        "source_xyz=None, source_mask=None)")
    assert sig(geometry.radius_edge_frame_features) == (
        "(rot, trans, graph, frame_mask=None, source_rot=None, source_trans=None, source_mask=None)")
    assert sig(geometry.neighbors_to_radius_graph) == "(neighbors_or_idx)"
    assert RadiusEdgeFeatures._fields == ("batch", "row", "col", "mask", "rbf", "offset", "local_pos", "rel_rot")
    assert AtomEdgeFeatures._fields == ("batch", "atom", "col", "mask", "rbf")
    assert list(inspect.signature(StructureBatch.atom_edge_features).parameters) == ["self", "graph", "n_rbf", "d_min", "d_max"]
    for fn in (geometry.radius_edge_rows, geometry.radius_edge_distance_features, geometry.radius_edge_frame_features,
               geometry.neighbors_to_radius_graph):
        assert "Not differentiable" in fn.__doc__
    assert "radius_edge_rows" in geometry.radius_graph_edges.__doc__
    with pytest.raises(TypeError, match="graph must be a geometry.RadiusGraph"):
        geometry.radius_edge_rows((torch.zeros(3), torch.zeros(2)))
