"""GPU tests of the edge features on CSR graphs (ps_csr_edge_rows_i32, ps_csr_edge_rbf_f32, ps_csr_edge_frames_f32;
ops.csr_edge_*; geometry.radius_edge_*; StructureBatch.edge_features(graph=RadiusGraph), .atom_edge_features).

Yardstick: tests/csr_edge_ref.py, the definitions in float64 in the kernels' own order of operations on the same float32
inputs.  ``dist``, ``local_pos`` and ``rel_rot`` must be BITWISE equal to it, every ``batch`` / ``row`` equal, ``rbf`` within
1e-6 absolute on every element (the bound K25's header derives and K25's tests use), the zeros at the padding exact.  On a
padded graph turned into CSR, all four must be BITWISE what K25 / K26 write for the same edges.  include/protstruc_csredge.h
is not in the case table of tests/launch_cases.py, so this file also holds the launchers to the launch contract: the
caller's stream, capture (from radius_graph(max_edges=n) through edge_features), four threads, the batch limit.

Offsets past 2^31 output floats cannot be tested in seconds: that they are 64-bit is established by reading the kernels."""
import ctypes
import functools
import os
import threading

import numpy as np
import pytest
import torch

from tests import csr_edge_ref as C, edge_ref as E
from tests.conftest import GOLDEN_DIR
from tests.test_gpu_edge import RBF_TOL, bits, carve, dev, sentinels_intact, tables
from tests.test_gpu_launch_contract import (SENTINEL, SLEEP_CYCLES, assert_all_same, raw, same,
                                            side_stream_beside_the_default_stream)

pytestmark = pytest.mark.gpu

PDB_FILES = ("1REX", "4EOT", "1ad0_DC", "5cjx_HL")     # those of tests/test_gpu_radius.py


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _csredge, _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    _csredge.load()
    return protstruc_amd


def split(pairs):
    return [p[0] for p in pairs], [p[1] for p in pairs]


def graph(pkg, row_ptr, col, B, Q):
    """a RadiusGraph of device tensors from numpy lists (dist is not used by the edge kernels)"""
    count = np.diff(row_ptr).reshape(B, Q).astype(np.int32)
    return pkg.geometry.RadiusGraph(dev(row_ptr), dev(col), None, dev(count))


def assert_rbf(got, ref, what):
    """(dist, rbf) tensors against a csr_edge_ref.Rbf"""
    dist, rbf = (t.cpu().numpy() for t in got)
    assert dist.dtype == np.float32 and rbf.dtype == np.float32
    assert dist.shape == ref.dist.shape and rbf.shape == ref.rbf.shape, (what, dist.shape, ref.dist.shape)
    wrong = np.flatnonzero(dist.view(np.int32).ravel() != ref.dist.view(np.int32).ravel())
    assert wrong.size == 0, (what, f"{wrong.size} dist differ in their bits, the first at {wrong[0]}")
    R = rbf.shape[-1] // max(dist.shape[-1], 1)
    real = np.repeat(ref.real, R, axis=-1)
    assert not dist[~ref.real].view(np.int32).any() and not rbf[~real].view(np.int32).any(), (what, "zeros are not exact")
    worst = float(np.abs(rbf.astype(np.float64) - ref.rbf).max()) if rbf.size else 0.0
    print(f"{what}: max |rbf - float64| = {worst:.3e}")
    assert worst <= RBF_TOL, (what, worst)


def assert_frames(got, ref, what):
    pos, rel = (t.cpu().numpy() for t in got)
    assert pos.dtype == np.float32 and rel.dtype == np.float32
    assert pos.shape == ref.local_pos.shape and rel.shape == ref.rel_rot.shape, what
    assert np.array_equal(pos.view(np.int32), ref.local_pos.view(np.int32)), (what, "local_pos differs in its bits")
    assert np.array_equal(rel.view(np.int32), ref.rel_rot.view(np.int32)), (what, "rel_rot differs in its bits")
    assert not pos[~ref.real].view(np.int32).any() and not rel[~ref.real].view(np.int32).any(), (what, "zeros are not exact")


def assert_rows(got, row_ptr, Q, E_, what):
    batch, row = (t.cpu().numpy() for t in got)
    want = C.edge_rows(row_ptr, Q, E_)
    assert batch.dtype == np.int32 and row.dtype == np.int32
    assert np.array_equal(batch, want[0]) and np.array_equal(row, want[1]), what


@functools.lru_cache(maxsize=None)
def residues(N, A):
    return E.residue_case(N, A, seed=11)


@functools.lru_cache(maxsize=None)
def frames_case(N):
    """(rot, trans, mask): 3 structures, 30 % of structure 0 and all of structure 1 masked over NaN, structure 2 complete"""
    rot, trans = E.random_frames(3, N, seed=N)
    mask = np.random.default_rng(N).random((3, N)) >= 0.3
    mask[1], mask[2] = False, True
    rot[~mask], trans[~mask] = np.nan, np.nan
    return rot, trans, mask


# ---- against K25 / K26 on the very same edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 7, 30))
@pytest.mark.parametrize("N", (1, 63, 64, 65, 130))
def test_bitwise_what_k25_and_k26_write_on_the_same_edges(pkg, N, k):
    geometry = pkg.geometry
    case = residues(N, 5)
    if N > 8:
        assert 0.3 < 1.0 - case.mask[0].mean() < 0.6 and np.isnan(case.xyz[0][~case.mask[0]]).all()
    idx = E.random_graph(3, N, k, seed=N + k)                              # 20 % padding
    g = geometry.neighbors_to_radius_graph(dev(idx))
    row_ptr, col, keep = C.to_csr(idx)
    assert np.array_equal(g.row_ptr.cpu().numpy(), row_ptr) and np.array_equal(g.col.cpu().numpy(), col)
    keep_t = dev(keep)
    assert_rows(geometry.radius_edge_rows(g), row_ptr, N, len(col), f"N={N} k={k}")
    for P, R in ((1, 1), (3, 5), (25, 16)):
        pairs, centers, sigma = tables(5, P, R)
        rbf25, dist25 = geometry.edge_distance_features(dev(case.xyz), dev(idx), dev(case.mask), pairs=pairs, centers=centers,
                                                        sigma=sigma, return_dist=True)
        rbf, dist = geometry.radius_edge_distance_features(dev(case.xyz), g, dev(case.mask), pairs=pairs, centers=centers,
                                                           sigma=sigma, return_dist=True)
        assert tuple(rbf.shape) == (len(col), P * R) and tuple(dist.shape) == (len(col), P) and not rbf.requires_grad
        assert torch.equal(bits(dist), bits(dist25[keep_t])), f"N={N} k={k} P={P} R={R}: dist is not K25's"
        assert torch.equal(bits(rbf), bits(rbf25[keep_t])), f"N={N} k={k} P={P} R={R}: rbf is not K25's"
        ref = C.edge_rbf(case.xyz, row_ptr, col, case.mask, *split(pairs), centers, sigma)
        assert_rbf((dist, rbf), ref, f"N={N} k={k} P={P} R={R}")
        if N > 8 and k > 1:
            assert ref.real.any() and not ref.real.all()
    rot, trans, mask = frames_case(N)
    k26 = geometry.edge_frame_features(dev(rot), dev(trans), dev(idx), dev(mask))
    got = geometry.radius_edge_frame_features(dev(rot), dev(trans), g, dev(mask))
    assert isinstance(got, geometry.EdgeFrames) and tuple(got.local_pos.shape) == (len(col), 3)
    assert tuple(got.rel_rot.shape) == (len(col), 3, 3)
    assert torch.equal(bits(got.local_pos), bits(k26.local_pos[keep_t])) and torch.equal(bits(got.rel_rot), bits(k26.rel_rot[keep_t]))
    assert_frames(got, C.edge_frames(rot, trans, row_ptr, col, mask), f"N={N} k={k} frames")


# ---- chunk edges, row widths that are no multiple of 4 floats, misaligned outputs ----------------------------------------------------
def addressable(col):
    """an empty tensor has no device pointer, and a NULL col is refused: E = 0 is called with one entry that is never read"""
    return col if col.numel() else torch.full((1,), -1, dtype=torch.int32, device=col.device)


def at(buf, front):
    """the address ``front`` floats into a sentinel buffer (an empty view of it may report no address at all)"""
    return buf.data_ptr() + 4 * front


def raw_rbf(pkg, xyz, row_ptr, col, mask, pairs, centers, sigma, front, src=None, src_mask=None, want_dist=True, want_rbf=True):
    """the C ABI into outputs ``front`` floats (4 * front bytes) past a 16-byte boundary inside sentinel-filled buffers"""
    lib = pkg._csredge.load()
    B, M, A = xyz.shape[:3]
    Q, As = (M, A) if src is None else src.shape[1:3]
    n, P, R = col.shape[0], len(pairs), len(centers)
    bufs, (dist, rbf), back = carve(((n, P), (n, P * R)), front)
    u8 = lambda t: None if t is None else t.to(torch.uint8).contiguous()                 # noqa: E731
    keep = [xyz.float().contiguous(), u8(mask), None if src is None else src.float().contiguous(), u8(src_mask),
            row_ptr.to(torch.int64).contiguous(), addressable(col.to(torch.int32).contiguous())]
    ptr = lambda t: None if t is None else t.data_ptr()                                  # noqa: E731
    ints = ctypes.c_int * P
    rc = lib.ps_csr_edge_rbf_f32(*(ptr(t) for t in keep), n, ints(*(p[0] for p in pairs)), ints(*(p[1] for p in pairs)), P,
                                 (ctypes.c_float * R)(*np.asarray(centers, np.float32).tolist()), R, float(sigma),
                                 at(bufs[0], front) if want_dist else None, at(bufs[1], front) if want_rbf else None, B, M, A, Q, As,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    sentinels_intact(bufs, front, back)
    for wanted, out in ((want_dist, dist), (want_rbf, rbf)):
        if not wanted:
            assert (out == 777.0).all(), "an output that was not asked for was written"
    return (dist.reshape(n, P) if want_dist else None), (rbf.reshape(n, P * R) if want_rbf else None)


def raw_frames(pkg, rot, trans, row_ptr, col, mask, front):
    lib = pkg._csredge.load()
    B, M = rot.shape[:2]
    n = col.shape[0]
    bufs, (pos, rel), back = carve(((n, 3), (n, 3, 3)), front)
    keep = [rot.float().contiguous(), trans.float().contiguous(), None if mask is None else mask.to(torch.uint8).contiguous(),
            row_ptr.to(torch.int64).contiguous(), addressable(col.to(torch.int32).contiguous())]
    rc = lib.ps_csr_edge_frames_f32(keep[0].data_ptr(), keep[1].data_ptr(), None if keep[2] is None else keep[2].data_ptr(),
                                    None, None, None, keep[3].data_ptr(), keep[4].data_ptr(), n, at(bufs[0], front), at(bufs[1], front),
                                    B, M, M, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    sentinels_intact(bufs, front, back)
    return pos.reshape(n, 3), rel.reshape(n, 3, 3)


def raw_rows(pkg, row_ptr, Q, n, front):
    lib = pkg._csredge.load()
    bufs, (batch, row), back = carve(((n,), (n,)), front)
    outs = [b.view(torch.int32)[front:front + n] for b in bufs]
    rp = row_ptr.to(torch.int64).contiguous()
    rc = lib.ps_csr_edge_rows_i32(rp.data_ptr(), rp.shape[0] - 1, Q, n, at(bufs[0], front), at(bufs[1], front),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    sentinels_intact(bufs, front, back)
    return outs


M_CHUNK = 50          # residues per structure of the chunk cases: 3 * 50 = 150 rows


@functools.lru_cache(maxsize=None)
def chunk_inputs():
    """three structures that all hold real atoms: residue_case's partly masked one, its complete one, the partly masked one"""
    case = residues(M_CHUNK, 5)
    pick = [0, 2, 0]
    return case.xyz[pick].copy(), case.mask[pick].copy()


@pytest.mark.parametrize("n_edges", C.CHUNK_EDGES)
def test_chunk_edges_row_widths_and_misaligned_outputs(pkg, n_edges):
    """E around one, two and three chunks with rows that end on a chunk boundary, span three chunks, and crowd 46 to a
    chunk; P * R in {1, 3, 5, 15, 17}, so chunks of 64 * P * R floats start at every alignment; outputs 4, 8 and 12 bytes
    off a 16-byte boundary inside sentinels"""
    xyz, mask = chunk_inputs()
    lengths = C.chunk_lengths(n_edges, 3 * M_CHUNK)
    row_ptr, col = C.graph_of_lengths(lengths, M_CHUNK, seed=n_edges)
    g = graph(pkg, row_ptr, col, 3, M_CHUNK)
    assert_rows(pkg.geometry.radius_edge_rows(g), row_ptr, M_CHUNK, n_edges, f"E={n_edges}")
    for front, (P, R) in zip((1, 2, 3, 1, 2), ((1, 1), (3, 1), (1, 5), (3, 5), (1, 17))):
        pairs, centers, sigma = tables(5, P, R, seed=front)
        if R == 17:
            centers, sigma = pkg.geometry.rbf_centers(17, 0.0, 16.0)
        ref = C.edge_rbf(xyz, row_ptr, col, mask, *split(pairs), centers, sigma)
        rbf, dist = pkg.geometry.radius_edge_distance_features(dev(xyz), g, dev(mask), pairs=pairs, centers=centers, sigma=sigma,
                                                               return_dist=True)
        assert_rbf((dist, rbf), ref, f"E={n_edges} P={P} R={R}")
        for off in ((front, front % 3 + 1) if n_edges else (front,)):
            rd, rr = raw_rbf(pkg, dev(xyz), dev(row_ptr), dev(col), dev(mask), pairs, centers, sigma, off)
            assert (rd.data_ptr() % 16, rr.data_ptr() % 16) == (4 * off, 4 * off) or not n_edges
            assert torch.equal(bits(rd), bits(dist)) and torch.equal(bits(rr), bits(rbf)), f"E={n_edges} P={P} R={R} off={off}"
        if n_edges > 64:
            assert ref.real.any() and not ref.real.all()
    # each output alone, inside sentinels
    pairs, centers, sigma = tables(5, 3, 5)
    both = pkg.ops.csr_edge_rbf(dev(xyz), g.row_ptr, g.col, dev(mask), pair_i=split(pairs)[0], pair_j=split(pairs)[1],
                                centers=centers, sigma=sigma)
    only = raw_rbf(pkg, dev(xyz), dev(row_ptr), dev(col), dev(mask), pairs, centers, sigma, 3, want_rbf=False)
    assert only[1] is None and torch.equal(bits(only[0]), bits(both[0]))
    only = raw_rbf(pkg, dev(xyz), dev(row_ptr), dev(col), dev(mask), pairs, centers, sigma, 1, want_dist=False)
    assert only[0] is None and torch.equal(bits(only[1]), bits(both[1]))
    # K49 and K51 inside sentinels too
    rot, trans, fmask = (t[[0, 2, 0]] for t in frames_case(M_CHUNK))
    fr = pkg.geometry.radius_edge_frame_features(dev(rot), dev(trans), g, dev(fmask))
    assert_frames(fr, C.edge_frames(rot, trans, row_ptr, col, fmask), f"E={n_edges} frames")
    rp, rl = raw_frames(pkg, dev(rot), dev(trans), dev(row_ptr), dev(col), dev(fmask), 2)
    assert torch.equal(bits(rp), bits(fr.local_pos)) and torch.equal(bits(rl), bits(fr.rel_rot))
    rb, rw = raw_rows(pkg, dev(row_ptr), M_CHUNK, n_edges, 1)
    assert_rows((rb, rw), row_ptr, M_CHUNK, n_edges, f"E={n_edges} raw")


def test_the_limits_of_the_tables(pkg):
    """P = R = 64: a full chunk is 64 * 64 * 64 floats, 16 KB of distances in LDS"""
    xyz, mask = chunk_inputs()
    row_ptr, col = C.graph_of_lengths(C.chunk_lengths(129, 3 * M_CHUNK), M_CHUNK, seed=5)
    pairs, centers, sigma = tables(5, 64, 64)
    ref = C.edge_rbf(xyz, row_ptr, col, mask, *split(pairs), centers, sigma)
    rbf, dist = pkg.geometry.radius_edge_distance_features(dev(xyz), graph(pkg, row_ptr, col, 3, M_CHUNK), dev(mask), pairs=pairs,
                                                           centers=centers, sigma=sigma, return_dist=True)
    assert_rbf((dist, rbf), ref, "P=64 R=64")


def test_more_chunks_than_workgroups(pkg):
    """K50 caps its grid at 8192 workgroups: 8192 * 64 + 70 edges give the first two a second chunk; K49 / K51 run a capped
    grid of 65536 workgroups of 256 lanes and are covered at this size by their one-lane-per-edge loop"""
    B, M = 2, 300
    rng = np.random.default_rng(8)
    n_edges = 8192 * 64 + 70
    lengths = rng.multinomial(n_edges, np.full(B * M, 1.0 / (B * M)))
    row_ptr, col = C.graph_of_lengths(lengths, M, seed=9)
    xyz = (rng.normal(size=(B, M, 2, 3)) * 6.0).astype(np.float32)
    mask = rng.random((B, M, 2)) >= 0.25
    xyz[~mask] = np.nan
    centers, sigma = pkg.geometry.rbf_centers(3, 0.0, 12.0)
    pairs = [(0, 1)]
    g = graph(pkg, row_ptr, col, B, M)
    rbf, dist = pkg.geometry.radius_edge_distance_features(dev(xyz), g, dev(mask), pairs=pairs, centers=centers, sigma=sigma,
                                                           return_dist=True)
    assert_rbf((dist, rbf), C.edge_rbf(xyz, row_ptr, col, mask, [0], [1], centers, sigma), "8192 * 64 + 70 edges")
    batch, row = pkg.geometry.radius_edge_rows(g)
    r = np.searchsorted(row_ptr[1:], np.arange(n_edges), side="right")
    assert np.array_equal(batch.cpu().numpy(), r // M) and np.array_equal(row.cpu().numpy(), r % M)


# ---- cut and tailed graphs -----------------------------------------------------------------------------------------------------------
def test_cut_and_tailed_graphs(pkg):
    """graphs of radius_graph(max_edges=n): n below row_ptr[-1] (served for the positions that exist), n above (the tail is
    exact 0 / -1), and the tail of col overwritten with 2^31 - 1 and with -7.  Residue 0 of every structure is NaN, NOT
    masked for the edge kernels and left out of the graph: a tail entry used as an address, or clamped to 0, reads it"""
    geometry = pkg.geometry
    case = residues(130, 5)
    xyz, mask = case.xyz.copy(), case.mask.copy()
    xyz[:, 0], mask[:, 0] = np.nan, True
    in_graph = mask[:, :, 1].copy()
    in_graph[:, 0] = False
    full = geometry.radius_graph(dev(np.nan_to_num(xyz[:, :, 1])), 9.0, dev(in_graph))
    total = int(full.row_ptr[-1])
    assert total > 500 and not bool((full.col == 0).any())
    rot, trans, fmask = frames_case(130)
    rot, trans, fmask = rot.copy(), trans.copy(), fmask.copy()
    rot[:, 0], trans[:, 0], fmask[:, 0] = np.nan, np.nan, True
    pairs, centers, sigma = tables(5, 3, 5)
    for n in (total - 77, total - 1, total, total + 1, total + 200):
        g = geometry.radius_graph(dev(np.nan_to_num(xyz[:, :, 1])), 9.0, dev(in_graph), max_edges=n)
        row_ptr = g.row_ptr.cpu().numpy()
        assert int(row_ptr[-1]) == total and g.col.shape[0] == n
        for fill in (None, 2 ** 31 - 1, -7):
            col = g.col.clone()
            if fill is not None:
                if n <= total:
                    continue
                col[total:] = fill
            gg = geometry.RadiusGraph(g.row_ptr, col, g.dist, g.count)
            what = f"max_edges={n} (row_ptr[-1]={total}), tail {fill}"
            assert_rows(geometry.radius_edge_rows(gg), row_ptr, 130, n, what)
            ref = C.edge_rbf(xyz, row_ptr, col.cpu().numpy(), mask, *split(pairs), centers, sigma)
            rbf, dist = geometry.radius_edge_distance_features(dev(xyz), gg, dev(mask), pairs=pairs, centers=centers, sigma=sigma,
                                                               return_dist=True)
            assert_rbf((dist, rbf), ref, what)
            assert not ref.real[total:].any() and ref.real[:min(n, total)].any()
            fr = geometry.radius_edge_frame_features(dev(rot), dev(trans), gg, dev(fmask))
            assert_frames(fr, C.edge_frames(rot, trans, row_ptr, col.cpu().numpy(), fmask), what)
            assert bool(torch.isfinite(rbf).all()) and bool(torch.isfinite(fr.rel_rot).all())
    # an unmasked NaN on a real edge does propagate
    points = np.nan_to_num(xyz[:, :, 1])
    points[:, 0] = points[:, 1] + np.float32(1.0)                         # residue 0 into the graph, next to residue 1
    g = geometry.radius_graph(dev(points), 9.0, dev(mask[:, :, 1]))
    hit = (g.col == 0) & (geometry.radius_edge_rows(g)[0] == 2)
    assert bool(hit.any())
    dist = pkg.ops.csr_edge_rbf(dev(xyz), g.row_ptr, g.col, dev(mask), pair_i=[1], pair_j=[1], centers=[4.0], sigma=2.0)[0]
    assert bool(torch.isnan(dist[hit]).all()) and bool(torch.isfinite(dist).any())


# ---- bipartite -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,M", ((1, 64), (65, 64), (1, 130), (65, 130)))
def test_bipartite_graphs(pkg, Q, M):
    geometry = pkg.geometry
    targets, sources = residues(M, 5), E.residue_case(Q, 3, seed=40 + Q)
    # the queries are slot 0 of the sources; every source is moved onto a residue of the targets' chain so that rows are not empty
    anchor = np.nan_to_num(targets.xyz[:, np.arange(Q) % M, :1])          # (3,Q,1,3)
    src_xyz = (np.nan_to_num(sources.xyz) - np.nan_to_num(sources.xyz[:, :, :1]) + anchor).astype(np.float32)
    src_xyz[~sources.mask] = np.nan
    g = geometry.radius_graph(dev(np.nan_to_num(targets.xyz[:, :, 0])), 10.0, dev(targets.mask[:, :, 0]),
                              queries=dev(np.nan_to_num(src_xyz[:, :, 0])), query_mask=dev(sources.mask[:, :, 0]))
    row_ptr, col = g.row_ptr.cpu().numpy(), g.col.cpu().numpy()
    assert tuple(g.count.shape) == (3, Q) and len(col) > 0
    what = f"Q={Q} M={M}"
    assert_rows(geometry.radius_edge_rows(g), row_ptr, Q, len(col), what)
    pairs = [(0, 0), (2, 4), (1, 3)]                                       # source slots in [0, 3), target slots in [0, 5)
    centers, sigma = geometry.rbf_centers(5, 0.0, 12.0)
    ref = C.edge_rbf(targets.xyz, row_ptr, col, targets.mask, *split(pairs), centers, sigma, src_xyz, sources.mask)
    rbf, dist = geometry.radius_edge_distance_features(dev(targets.xyz), g, dev(targets.mask), pairs=pairs, centers=centers,
                                                       sigma=sigma, return_dist=True, source_xyz=dev(src_xyz),
                                                       source_mask=dev(sources.mask))
    assert_rbf((dist, rbf), ref, what)
    assert ref.real.any()
    # the graph's own distance is the (0, 0) pair's wherever both atoms are in the mask
    d00 = dist[:, 0].cpu().numpy()
    assert np.array_equal(d00[ref.real[:, 0]].view(np.int32), g.dist.cpu().numpy()[ref.real[:, 0]].view(np.int32))
    rot, trans, fmask = frames_case(M)
    srot, strans, smask = frames_case(Q + 200)
    srot, strans, smask = srot[:, :Q], strans[:, :Q], smask[:, :Q]
    fr = geometry.radius_edge_frame_features(dev(rot), dev(trans), g, dev(fmask), source_rot=dev(srot), source_trans=dev(strans),
                                             source_mask=dev(smask))
    assert_frames(fr, C.edge_frames(rot, trans, row_ptr, col, fmask, srot, strans, smask), what)
    # without masks
    fr = geometry.radius_edge_frame_features(dev(rot[2:]), dev(trans[2:]), geometry.RadiusGraph(
        g.row_ptr[2 * Q:] - g.row_ptr[2 * Q], g.col[int(g.row_ptr[2 * Q]):], None, g.count[2:]), source_rot=dev(srot[2:]),
        source_trans=dev(strans[2:]))
    sub = (row_ptr[2 * Q:] - row_ptr[2 * Q], col[row_ptr[2 * Q]:])
    assert_frames(fr, C.edge_frames(rot[2:], trans[2:], *sub, None, srot[2:], strans[2:]), what + ", no masks")
    # sources omitted: the rows no longer match the targets
    with pytest.raises(ValueError, match="row_ptr must have shape"):
        geometry.radius_edge_distance_features(dev(targets.xyz), g, dev(targets.mask))
    with pytest.raises(ValueError, match="row_ptr must have shape"):
        geometry.radius_edge_frame_features(dev(rot), dev(trans), g)
    rc = pkg._csredge.load().ps_csr_edge_rbf_f32(dist.data_ptr(), None, None, None, g.row_ptr.data_ptr(), g.col.data_ptr(), len(col),
                                                 (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0), 1, (ctypes.c_float * 1)(1.0), 1, 1.0,
                                                 dist.data_ptr(), None, 3, M, 5, Q, 5, None)
    assert rc == 1, "src_xyz NULL with Q != M is refused before anything is launched"


def test_empty_inputs_launch_nothing(pkg, monkeypatch):
    ops = pkg.ops

    def no_launch(*args):
        raise AssertionError("an empty call launched a kernel")

    monkeypatch.setattr(ops, "_launch_csredge", no_launch)
    for B, M, n in ((0, 5, 0), (2, 0, 0), (2, 5, 0), (0, 5, 4), (2, 0, 4)):
        rp = torch.zeros(B * M + 1, dtype=torch.int64, device="cuda")
        col = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        dist, rbf = ops.csr_edge_rbf(torch.zeros(B, M, 5, 3, device="cuda"), rp, col, pair_i=[0, 1], pair_j=[1, 0],
                                     centers=[1.0, 2.0, 3.0], sigma=1.0)
        assert tuple(dist.shape) == (n, 2) and tuple(rbf.shape) == (n, 6) and not dist.any() and not rbf.any()
        pos, rel = ops.csr_edge_frames(torch.zeros(B, M, 3, 3, device="cuda"), torch.zeros(B, M, 3, device="cuda"), rp, col)
        assert tuple(pos.shape) == (n, 3) and tuple(rel.shape) == (n, 3, 3) and not pos.any() and not rel.any()
    assert all(t.numel() == 0 for t in ops.csr_edge_rows(torch.zeros(11, dtype=torch.int64, device="cuda"), 5, 0))
    monkeypatch.undo()
    # a tail with no row at all: every position is padding
    batch, row = ops.csr_edge_rows(torch.zeros(1, dtype=torch.int64, device="cuda"), 0, 5)
    assert bool((batch == -1).all()) and bool((row == -1).all()) and batch.shape[0] == 5


def test_arrays_come_back_as_arrays_and_cpu_tensors_on_the_cpu(pkg):
    geometry = pkg.geometry
    case = residues(65, 5)
    idx = E.random_graph(3, 65, 4, seed=2)
    g = geometry.neighbors_to_radius_graph(idx)
    assert all(isinstance(t, np.ndarray) for t in (g.row_ptr, g.col, g.count))
    rbf = geometry.radius_edge_distance_features(case.xyz, g, case.mask)
    rows = geometry.radius_edge_rows(g)
    fr = geometry.radius_edge_frame_features(*frames_case(65)[:2], g, frames_case(65)[2])
    assert isinstance(rbf, np.ndarray) and rbf.shape == (len(g.col), 400) and all(isinstance(t, np.ndarray) for t in rows + tuple(fr))
    gt = geometry.neighbors_to_radius_graph(torch.from_numpy(idx))
    out = geometry.radius_edge_distance_features(torch.from_numpy(case.xyz), gt, torch.from_numpy(case.mask))
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and np.array_equal(out.numpy().view(np.int32), rbf.view(np.int32))


# ---- StructureBatch on the PDB files ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pdb_batch():
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, name + ".pdb") for name in PDB_FILES])


def padded_from_csr(g, B, N):
    """(idx (B,N,kmax) int32 with -1 at the padding, keep (B,N,kmax) bool) of a self graph of tensors"""
    count = g.count.long()
    kmax = int(count.max())
    keep = torch.arange(kmax, device=count.device)[None, None, :] < count[:, :, None]
    idx = torch.full((B, N, kmax), -1, dtype=torch.int32, device=count.device)
    idx[keep] = g.col[:int(g.row_ptr[-1])]
    return idx, keep


def test_pdb_edge_features_on_a_radius_graph(pkg):
    from protstruc_amd.structure_batch import RadiusEdgeFeatures
    geometry = pkg.geometry
    batch = pdb_batch()
    B, N = batch.get_xyz().shape[:2]
    g = batch.radius_graph(10.0)
    n = g.col.shape[0]
    ef = batch.edge_features(graph=g)
    assert isinstance(ef, RadiusEdgeFeatures) and tuple(ef.rbf.shape) == (n, 400) and not ef.rbf.requires_grad
    row_ptr, col = g.row_ptr.cpu().numpy(), g.col.cpu().numpy()
    assert int(g.count.max()) > 20 and n == int(row_ptr[-1])
    assert_rows((ef.batch, ef.row), row_ptr, N, n, "PDB batch")
    assert torch.equal(ef.col, g.col) and ef.col.dtype == torch.int32 and torch.equal(ef.mask, ef.batch >= 0) and bool(ef.mask.all())
    centers, sigma = geometry.rbf_centers()
    pairs = [(a, b) for a in range(5) for b in range(5)]
    xyz, present = batch.get_xyz().cpu().numpy(), batch._present_atoms().cpu().numpy()
    ref = C.edge_rbf(xyz, row_ptr, col, present, *split(pairs), centers, sigma)
    rbf = ef.rbf.cpu().numpy()
    assert not rbf[~np.repeat(ref.real, 16, axis=-1)].view(np.int32).any()
    worst = float(np.abs(rbf - ref.rbf).max())
    print(f"edge_features(graph=radius_graph(10.0)): max |rbf - float64| = {worst:.3e}")
    assert worst <= RBF_TOL
    rot, trans = batch.backbone_orientations_and_translations()
    frame_mask = batch._present_atoms()[:, :, :3].all(-1)
    assert_frames((ef.local_pos, ef.rel_rot), C.edge_frames(rot.cpu().numpy(), trans.cpu().numpy(), row_ptr, col,
                                                            frame_mask.cpu().numpy()), "PDB batch, frames")
    # |local_pos| is the graph's own CA-CA distance wherever the source has its frame
    has = frame_mask[ef.batch.long(), ef.row.long()] & frame_mask[ef.batch.long(), ef.col.long()]
    assert float((ef.local_pos.norm(dim=-1) - g.dist)[has].abs().max()) < 1e-4
    # the offsets: what the padded route gives on the same edges
    idx, keep = padded_from_csr(g, B, N)
    assert ef.offset.dtype == torch.int64 and torch.equal(ef.offset, batch._edge_offsets(idx, 32)[keep])
    assert int(ef.offset.max()) == 65 and bool(((ef.offset == 31) | (ef.offset == 33)).any())
    # and so are the features: K25 / K26 on the padded form where it fits K25's limit
    if idx.shape[2] <= 64:
        k25 = batch.edge_features(idx)
        assert torch.equal(bits(ef.rbf), bits(k25.rbf[keep])) and torch.equal(bits(ef.rel_rot), bits(k25.rel_rot[keep]))
    # other settings, no frames
    ef2 = batch.edge_features(graph=g, atoms=("CA", "CB", "N"), n_rbf=8, d_min=0.0, d_max=16.0, frames=False, max_offset=4)
    assert ef2.local_pos is None and ef2.rel_rot is None and tuple(ef2.rbf.shape) == (n, 72) and int(ef2.offset.max()) == 9
    centers, sigma = geometry.rbf_centers(8, 0.0, 16.0)
    ref2 = C.edge_rbf(xyz, row_ptr, col, present, *split([(a, b) for a in (1, 4, 0) for b in (1, 4, 0)]), centers, sigma)
    assert float(np.abs(ef2.rbf.cpu().numpy() - ref2.rbf).max()) <= RBF_TOL


def test_pdb_atom_edge_features(pkg):
    from protstruc_amd.structure_batch import AtomEdgeFeatures
    batch = pdb_batch()
    B, N, A = batch.get_xyz().shape[:3]
    g = batch.atom_radius_graph(5.0)
    n = g.col.shape[0]
    ef = batch.atom_edge_features(g, n_rbf=16, d_min=0.0, d_max=8.0)
    assert isinstance(ef, AtomEdgeFeatures) and tuple(ef.rbf.shape) == (n, 16) and n > 10000
    row_ptr = g.row_ptr.cpu().numpy()
    r = np.searchsorted(row_ptr[1:], np.arange(n), side="right")
    assert np.array_equal(ef.batch.cpu().numpy(), r // (N * A)) and np.array_equal(ef.atom.cpu().numpy(), r % (N * A))
    assert torch.equal(ef.col, g.col) and bool(ef.mask.all())
    centers, sigma = pkg.geometry.rbf_centers(16, 0.0, 8.0)
    z = (g.dist.cpu().numpy().astype(np.float64)[:, None] - centers.astype(np.float64)) / np.float64(np.float32(sigma))
    worst = float(np.abs(ef.rbf.cpu().numpy() - np.exp(-(z * z))).max())
    print(f"atom_edge_features(atom_radius_graph(5.0)): max |rbf - float64 of graph.dist| = {worst:.3e}")
    assert worst <= RBF_TOL
    assert float(ef.rbf.max()) > 0.9
    with pytest.raises(ValueError, match="graph must be a geometry.RadiusGraph over the"):
        batch.atom_edge_features(batch.radius_graph(10.0))


def test_the_padded_route_is_what_it_was(pkg):
    """edge_features() with no graph, with Neighbors and with a tensor: torch.equal to geometry's padded functions called
    directly, as before the radius-graph route existed"""
    geometry = pkg.geometry
    batch = pdb_batch()
    B, N = batch.get_xyz().shape[:2]
    present = batch._present_atoms()
    centers, sigma = geometry.rbf_centers()
    pairs = [(a, b) for a in range(5) for b in range(5)]
    rot, trans = batch.backbone_orientations_and_translations()
    nb = batch.knn_graph(30)
    mine = torch.from_numpy(E.random_graph(B, N, 5, seed=3)).long()
    mine[:, ::7, 2] = N + 5
    for given, idx in ((None, nb.idx), (nb, nb.idx), (mine, None)):
        ef = batch.edge_features() if given is None else batch.edge_features(given)
        if idx is None:
            idx = torch.where((mine >= 0) & (mine < N), mine, torch.full_like(mine, -1)).to(torch.int32).cuda()
        assert type(ef).__name__ == "EdgeFeatures" and torch.equal(ef.idx, idx) and torch.equal(ef.mask, idx >= 0)
        want = geometry.edge_distance_features(batch.get_xyz(), idx, present, pairs=pairs, centers=centers, sigma=sigma)
        assert torch.equal(bits(ef.rbf), bits(want))
        pos, rel = geometry.edge_frame_features(rot, trans, idx, present[:, :, :3].all(-1))
        assert torch.equal(bits(ef.local_pos), bits(pos)) and torch.equal(bits(ef.rel_rot), bits(rel))
        assert torch.equal(ef.offset, batch._edge_offsets(idx, 32))


# ---- repeatability ---------------------------------------------------------------------------------------------------------------------
def test_repeatability(pkg):
    batch = pdb_batch()
    g = batch.radius_graph(8.0)
    first = batch.edge_features(graph=g)
    for _ in range(2):
        again = batch.edge_features(graph=g)
        for a, b in zip(first, again):
            assert same(a, b)


# ---- the launch contract -----------------------------------------------------------------------------------------------------------------
# Two seeded variants with the same masks and other coordinates: radius_graph(max_edges=n) -> edge_features reaches K49, K50
# and K51, makes no host read, and every output differs between the variants.
CONTRACT_EDGES = 1500
SYMBOLS = ("ps_csr_edge_rows_i32", "ps_csr_edge_rbf_f32", "ps_csr_edge_frames_f32")


def _contract_inputs(v):
    case = E.residue_case(37, 5, seed=60)
    other = E.residue_case(37, 5, seed=61)
    xyz = np.nan_to_num(case.xyz if v == "A" else other.xyz)
    return dict(xyz=torch.from_numpy(xyz), atom_mask=torch.from_numpy(case.mask))


def _contract_batch(inputs):
    from protstruc_amd import StructureBatch
    return StructureBatch.from_xyz(inputs["xyz"].cuda().clone(), inputs["atom_mask"].cuda())


def _contract_run(batch):
    g = batch.radius_graph(9.0, max_edges=CONTRACT_EDGES)
    ef = batch.edge_features(graph=g)
    return (g.row_ptr, g.col, ef.batch, ef.row, ef.mask, ef.rbf, ef.offset, ef.local_pos, ef.rel_rot)


@functools.lru_cache(maxsize=None)
def contract_eager(v):
    outs = _contract_run(_contract_batch(_contract_inputs(v)))
    torch.cuda.synchronize()
    return outs


def test_contract_case_reaches_the_three_symbols_and_meets_the_yardstick(pkg, monkeypatch):
    seen = []
    launch = pkg.ops._launch_csredge
    monkeypatch.setattr(pkg.ops, "_launch_csredge", lambda name, *args: (seen.append(name), launch(name, *args))[1])
    outs = _contract_run(_contract_batch(_contract_inputs("A")))
    torch.cuda.synchronize()
    assert tuple(seen) == SYMBOLS
    assert_all_same(outs, contract_eager("A"), "a second eager call")
    a, b = contract_eager("A"), contract_eager("B")
    total = int(a[0][-1])
    assert 200 < total < CONTRACT_EDGES and int(b[0][-1]) < CONTRACT_EDGES, "the buffers leave a tail and cut nothing"
    for k in (0, 1, 2, 3, 5, 6, 7, 8):
        assert not same(a[k], b[k]), f"output {k} is the same for both variants"
    i = _contract_inputs("A")
    xyz, mask = i["xyz"].numpy(), i["atom_mask"].numpy()
    row_ptr, col = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert_rows((a[2], a[3]), row_ptr, 37, CONTRACT_EDGES, "contract A")
    centers, sigma = pkg.geometry.rbf_centers()
    ref = C.edge_rbf(xyz, row_ptr, col, mask, *split([(p, q) for p in range(5) for q in range(5)]), centers, sigma)
    assert float(np.abs(a[5].cpu().numpy() - ref.rbf).max()) <= RBF_TOL and not bool(a[5][total:].any())
    assert not bool(a[7][total:].any()) and not bool(a[8][total:].any()) and not bool(a[6][total:].any())
    assert bool((a[2][total:] == -1).all()) and bool((a[1][total:] == -1).all())


def test_launches_on_the_callers_stream(pkg):
    """As tests/test_gpu_launch_contract.py: on a side stream, a sleep, the copy of variant B over variant A, the calls; a
    clone on the default stream meanwhile still sees variant A."""
    want_a, want_b = contract_eager("A"), contract_eager("B")
    a, b = _contract_inputs("A"), _contract_inputs("B")
    batch = _contract_batch(a)
    new = b["xyz"].cuda()
    side = side_stream_beside_the_default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        batch.xyz.copy_(new)
    control = batch.xyz.clone()                              # the default stream: runs while the side stream sleeps
    with torch.cuda.stream(side):
        outs = _contract_run(batch)
    torch.cuda.synchronize()
    if not same(control, a["xyz"].cuda()):
        pytest.fail("inconclusive -- the control clone did not see variant A")
    assert_all_same(outs, want_b, "on a side stream")
    for k in (0, 1, 5, 7, 8):
        assert not same(outs[k], want_a[k]), f"output {k} was computed from the inputs as they were before the side stream's copy"


def test_inside_a_captured_graph(pkg):
    """radius_graph(max_edges=n) -> edge_features captured on variant A after one eager call, on one stream, and replayed
    twice on variant B over overwritten outputs: no host read anywhere on the route"""
    want_b, b = contract_eager("B"), _contract_inputs("B")
    batch = _contract_batch(_contract_inputs("A"))
    _contract_run(batch)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(captured, stream=side):
            outs = _contract_run(batch)
    torch.cuda.synchronize()
    batch.xyz.copy_(b["xyz"].cuda())
    for replay in range(2):
        for o in outs:
            raw(o).fill_(SENTINEL)
        captured.replay()
        torch.cuda.synchronize()
        assert_all_same(outs, want_b, f"replay {replay + 1}")


def test_four_threads_on_four_streams(pkg):
    rounds, n_threads = 3, 4
    want = {v: contract_eager(v) for v in "AB"}
    mine = [_contract_batch(_contract_inputs("AB"[t % 2])) for t in range(n_threads)]
    streams = [torch.cuda.Stream() for _ in range(n_threads)]
    torch.cuda.synchronize()
    gate = threading.Barrier(n_threads)
    failures = []

    def work(t):
        try:
            gate.wait(timeout=60)
            with torch.cuda.stream(streams[t]):
                for r in range(rounds):
                    outs = _contract_run(mine[t])
                    streams[t].synchronize()
                    for k, (o, w) in enumerate(zip(outs, want["AB"[t % 2]])):
                        if not same(o, w):
                            failures.append(f"thread {t}, round {r}: output {k} differs from the serial result")
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
    """B = 65535 with Q = 1 against M = 3 targets: structure b is structure b % 3, one source each with its own row, and the
    results are those of the three, bit for bit"""
    geometry = pkg.geometry
    B = 65535
    rng = np.random.default_rng(14)
    xyz = (rng.normal(size=(3, 3, 2, 3)) * 4.0).astype(np.float32)
    src = (rng.normal(size=(3, 1, 2, 3)) * 4.0).astype(np.float32)
    rot, trans = E.random_frames(3, 3, seed=15)
    srot, strans = E.random_frames(3, 1, seed=16)
    lengths3 = np.array([2, 0, 3])                                        # per structure: its one row
    cols3 = [np.array([2, 0]), np.array([], dtype=np.int64), np.array([0, 1, 2])]
    pick = np.arange(B) % 3
    lengths = lengths3[pick]
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate([cols3[p] for p in pick]).astype(np.int32)
    small_rp = np.concatenate([[0], np.cumsum(lengths3)]).astype(np.int64)
    small_col = np.concatenate(cols3).astype(np.int32)
    centers, sigma = geometry.rbf_centers(4, 0.0, 12.0)
    pairs = [(0, 1), (1, 1)]
    ref = C.edge_rbf(xyz, small_rp, small_col, None, *split(pairs), centers, sigma, src)
    gs = graph(pkg, small_rp, small_col, 3, 1)
    small = geometry.radius_edge_distance_features(dev(xyz), gs, pairs=pairs, centers=centers, sigma=sigma, return_dist=True,
                                                   source_xyz=dev(src))
    assert_rbf((small[1], small[0]), ref, "B = 3, Q = 1")
    small_fr = geometry.radius_edge_frame_features(dev(rot), dev(trans), gs, source_rot=dev(srot), source_trans=dev(strans))
    assert_frames(small_fr, C.edge_frames(rot, trans, small_rp, small_col, None, srot, strans), "B = 3, Q = 1")
    tile = lambda a: dev(a)[torch.from_numpy(pick).cuda()]               # noqa: E731
    g = graph(pkg, row_ptr, col, B, 1)
    rbf, dist = geometry.radius_edge_distance_features(tile(xyz), g, pairs=pairs, centers=centers, sigma=sigma, return_dist=True,
                                                       source_xyz=tile(src))
    fr = geometry.radius_edge_frame_features(tile(rot), tile(trans), g, source_rot=tile(srot), source_trans=tile(strans))
    batch, row = geometry.radius_edge_rows(g)
    torch.cuda.synchronize()
    n = len(col)
    assert n == 5 * (B // 3) and tuple(rbf.shape) == (n, 8)
    assert np.array_equal(batch.cpu().numpy(), np.repeat(np.arange(B), lengths)) and not bool(row.any())
    for got, three in ((rbf, small[0]), (dist, small[1]), (fr.local_pos, small_fr.local_pos), (fr.rel_rot, small_fr.rel_rot)):
        assert same(got, three.repeat(B // 3, *([1] * (three.ndim - 1)))), "B = 65535 is not the B = 3 result repeated"
