"""GPU tests of the backward kernels of the edge features (ps_csr_edge_rbf_backward_f32, ps_csr_edge_pair_grad_sum_f32,
ps_csr_edge_frames_backward_f32; ops.csr_edge_rbf_backward, .csr_edge_pair_grad_sum, .csr_edge_frames_backward,
.csr_incoming_edges) and of the autograd functions behind geometry.edge_distance_features, .edge_frame_features,
.radius_edge_distance_features, .radius_edge_frame_features, StructureBatch.edge_features and .atom_edge_features.

Yardstick: tests/edge_grad_ref.py.  K53 and K54 owe its BITS (double accumulators in a fixed order, rounded once).  K52 owes
its float64 value within the bound that the restatement returns beside it, element by element,
    |kappa| sum_c |g_c| |w_c| (1e-6 + 2^-21 e_c) |Xj - Xq| / d + 2^-23 |f|,
propagated through the sum as  sum bound + 2^-39 sum |term| + 2^-23 |ref| + 2^-149;  K54 also
    |got - ref| <= 2^-23 |ref| + 2^-23 sum |term| + 2^-149.
Every test prints the worst ratio of error to bound it met; a ratio above 1 is a bug in the kernel or in the derivation.
The zeros -- padding, masks, an edge of length 0 -- are exact, over NaN in the coordinates AND in the incoming gradients.

include/protstruc_edgegrad.h is not in the case table of tests/launch_cases.py, so this file also holds the new symbols to
the launch contract: the caller's stream, capture (the backward pass behind radius_graph(max_edges=n)), four threads, the
batch limit.  Offsets past 2^31 floats cannot be tested in seconds: that they are 64-bit is established by reading."""
import ctypes
import functools
import os
import threading

import numpy as np
import pytest
import torch

from tests import csr_edge_ref as C, edge_grad_ref as G, edge_ref as E
from tests.conftest import GOLDEN_DIR
from tests.test_gpu_edge import bits, carve, dev, sentinels_intact, tables
from tests.test_gpu_launch_contract import (SENTINEL, SLEEP_CYCLES, assert_all_same, raw, same,
                                            side_stream_beside_the_default_stream)

pytestmark = pytest.mark.gpu

CHUNK_EDGES = (0, 1, 63, 64, 65, 129, 255, 256, 257)     # around one and two chunks of 64, and around the 128 and 256 K52 takes at a time
M_CHUNK = 50          # residues per structure of the chunk cases: 3 * 50 = 150 rows, owners on both sides of lanes 64 and 128


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _csredge, _edgegrad, _lib, geometry, ops  # noqa: F401 -- reached through the package
    _lib.load()
    _csredge.load()
    _edgegrad.load()
    return protstruc_amd


def split(pairs):
    return [p[0] for p in pairs], [p[1] for p in pairs]


def graph(pkg, row_ptr, col, B, Q):
    count = np.diff(row_ptr).reshape(B, Q).astype(np.int32)
    return pkg.geometry.RadiusGraph(dev(row_ptr), dev(col), None, dev(count))


def ratio(got, ref, bound, what):
    """the worst |got - ref| / bound; exact zeros of the reference must be exact zeros"""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    worst = float((np.abs(got - ref) / bound).max()) if got.size else 0.0
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (what, worst)
    return worst


def mixed(rng, shape):
    """float32 values over six decades, so that the order of a sum shows in its bits"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, size=shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def chunk_inputs():
    """three structures of 50 residues with 5 slots: 45 % of the slots of structures 0 and 2 masked over NaN, structure 1
    complete"""
    case = E.residue_case(M_CHUNK, 5, seed=11)
    pick = [0, 2, 0]
    return case.xyz[pick].copy(), case.mask[pick].copy()


@functools.lru_cache(maxsize=None)
def chunk_graph(n_edges):
    """(row_ptr, col) of tests/csr_edge_ref.py's chunk cases with, where there is room, a -1 and a column out of range inside
    rows"""
    row_ptr, col = C.graph_of_lengths(C.chunk_lengths(n_edges, 3 * M_CHUNK), M_CHUNK, seed=n_edges)
    if n_edges > 8:
        col[5], col[n_edges - 2] = -1, M_CHUNK + 1
    return row_ptr, col


@functools.lru_cache(maxsize=None)
def frames_case(N, B=3):
    """(rot, trans, mask): 30 % of the frames masked over NaN"""
    rot, trans = E.random_frames(B, N, seed=N)
    mask = np.random.default_rng(N).random((B, N)) >= 0.3
    if N > 1:
        mask[0, 0], mask[0, 1 % N] = True, False
    rot[~mask], trans[~mask] = np.nan, np.nan
    return rot, trans, mask


# ---- 1. there is a gradient --------------------------------------------------------------------------------------------------------
def test_edge_distance_features_has_a_gradient(pkg):
    """fails where the feature is missing: the outputs of the four functions carried no graph"""
    geometry = pkg.geometry
    case = E.residue_case(33, 5, seed=7)
    idx = dev(E.random_graph(3, 33, 6, seed=80)).long()
    mask = dev(case.mask)
    x = dev(case.xyz).requires_grad_()
    rbf = geometry.edge_distance_features(x, idx, mask)
    assert rbf.requires_grad and rbf.grad_fn is not None
    rbf.sum().backward()                                              # hands in a gradient of stride 0
    g = x.grad.cpu().numpy()
    assert g.shape == case.xyz.shape and np.isfinite(g).all() and np.abs(g[2]).max() > 1e-3
    assert not g[~case.mask].view(np.int32).any(), "an atom outside the mask takes an exact +0"
    # the bits of the forward are those of the route without a graph, which is still there
    plain = geometry.edge_distance_features(x.detach(), idx, mask)
    assert not plain.requires_grad and torch.equal(bits(plain), bits(rbf.detach()))
    with torch.no_grad():
        assert not geometry.edge_distance_features(x, idx, mask).requires_grad
    assert isinstance(geometry.edge_distance_features(np.nan_to_num(case.xyz), idx.cpu().numpy(), case.mask), np.ndarray)
    # frames, both layouts, and the flat functions
    rot, trans, fmask = frames_case(33)
    r, t = dev(np.nan_to_num(rot)).requires_grad_(), dev(np.nan_to_num(trans)).requires_grad_()
    fr = geometry.edge_frame_features(r, t, idx, dev(fmask))
    assert fr.local_pos.requires_grad and fr.rel_rot.requires_grad
    (fr.local_pos.sum() + fr.rel_rot.sum()).backward()
    assert tuple(r.grad.shape) == (3, 33, 3, 3) and tuple(t.grad.shape) == (3, 33, 3) and float(r.grad.abs().max()) > 0
    assert not bool(r.grad[~dev(fmask)].any()) and not bool(t.grad[~dev(fmask)].any())
    assert not geometry.edge_frame_features(r.detach(), t.detach(), idx, dev(fmask)).local_pos.requires_grad
    gr = geometry.neighbors_to_radius_graph(idx)
    x2 = dev(case.xyz).requires_grad_()
    rbf2, dist2 = geometry.radius_edge_distance_features(x2, gr, mask, return_dist=True)
    assert rbf2.requires_grad and dist2.requires_grad
    dist2.sum().backward()                                            # grad_rbf is None: K52 takes a NULL for it
    assert np.isfinite(x2.grad.cpu().numpy()).all() and float(x2.grad[2].abs().max()) > 1e-3
    # only the trans of a frame pair requires grad
    t2 = dev(np.nan_to_num(trans)).requires_grad_()
    geometry.radius_edge_frame_features(r.detach(), t2, gr, dev(fmask)).local_pos.sum().backward()
    assert float(t2.grad.abs().max()) > 0
    # a CPU tensor that requires grad gets its gradient on the CPU
    xc = torch.from_numpy(case.xyz).requires_grad_()
    out = geometry.edge_distance_features(xc, idx.cpu(), torch.from_numpy(case.mask))
    assert out.device.type == "cpu" and out.requires_grad
    out.sum().backward()
    assert xc.grad.device.type == "cpu" and torch.equal(bits(xc.grad), bits(x.grad.cpu()))


# ---- 2. K53 and K54: the bits ------------------------------------------------------------------------------------------------------
PAIRS_BY_SLOTS = {1: ([0, 0, 0], [0, 0, 0]),                                   # one slot, named by every pair
                  5: ([0, 0, 2, 4, 0, 2, 2], [1, 1, 1, 4, 0, 0, 4]),           # slot 3 never named, slot 0 and 2 several times
                  15: ([13, 0, 13, 7, 7, 7, 1, 0, 13], [2, 2, 9, 9, 2, 11, 11, 0, 13])}   # slot 14 never named


def raw_sum(pkg, f, row_ptr, in_ptr, in_edge, pair_i, pair_j, B, M, A, front, Q=None, As=None):
    """the C ABI into outputs ``front`` floats past a 16-byte boundary inside sentinel-filled buffers"""
    lib = pkg._edgegrad.load()
    bip = Q is not None
    Qs, Ass = (Q, As) if bip else (M, A)
    shapes = ((B, M, A, 3),) + (((B, Qs, Ass, 3),) if bip else ())
    bufs, outs, back = carve(shapes, front)
    P, n = len(pair_i), f.shape[0]
    keep = [f.contiguous(), row_ptr.contiguous(), in_ptr.contiguous(), in_edge.contiguous()]
    ints = ctypes.c_int * P
    rc = lib.ps_csr_edge_pair_grad_sum_f32(keep[0].data_ptr() if n else None, keep[1].data_ptr(), n, keep[2].data_ptr(),
                                           keep[3].data_ptr() if n else None, keep[3].shape[0], ints(*pair_i), ints(*pair_j), P,
                                           bufs[0].data_ptr() + 4 * front, bufs[1].data_ptr() + 4 * front if bip else None, B, M, A,
                                           Qs, Ass, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    sentinels_intact(bufs, front, back)
    return [o.reshape(s) for o, s in zip(outs, shapes)]


@pytest.mark.parametrize("A", (1, 5, 15))
@pytest.mark.parametrize("n_edges", CHUNK_EDGES)
def test_pair_grad_sum_bits(pkg, n_edges, A):
    ops = pkg.ops
    B, M = 3, M_CHUNK
    row_ptr, col = chunk_graph(n_edges)
    pair_i, pair_j = PAIRS_BY_SLOTS[A]
    f = mixed(np.random.default_rng(n_edges + A), (n_edges, len(pair_i), 3))
    in_ptr, in_edge = ops.csr_incoming_edges(dev(row_ptr), dev(col), B, M, M)
    want_ptr, want_edge = G.incoming(row_ptr, col, B, M, M)
    assert np.array_equal(in_ptr.cpu().numpy(), want_ptr) and np.array_equal(in_edge.cpu().numpy(), want_edge)
    want = G.pair_grad_sum(f, row_ptr, want_ptr, want_edge, pair_i, pair_j, B, M, A).grad.astype(np.float32)
    got = ops.csr_edge_pair_grad_sum(dev(f), dev(row_ptr), in_ptr, in_edge, pair_i=pair_i, pair_j=pair_j, B=B, M=M, A=A)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), f"E={n_edges} A={A}: the bits differ"
    unnamed = [a for a in range(A) if a not in pair_i and a not in pair_j]
    assert not got[:, :, unnamed].cpu().numpy().view(np.int32).any(), "a slot no pair names is an exact +0"
    assert (len(unnamed) > 0) == (A > 1)
    for front in (1, 2, 3):
        (inside,) = raw_sum(pkg, dev(f), dev(row_ptr), in_ptr, in_edge, pair_i, pair_j, B, M, A, front)
        assert torch.equal(bits(inside), bits(got)), f"E={n_edges} A={A}: {4 * front} bytes off a 16-byte boundary"


def bipartite_graph(Q, M, B=2, n_edges=129, seed=0):
    rng = np.random.default_rng(1000 * Q + M + seed)
    lengths = rng.multinomial(n_edges, np.ones(B * Q) / (B * Q))
    if B * Q > 4:
        lengths[-1] += lengths[1]
        lengths[1] = 0
    row_ptr, col = C.graph_of_lengths(lengths, M, seed=Q + M)
    col[7], col[40] = -1, M                                              # padding inside rows
    col[60:64] = col[60]                                                 # a row (or two) names one target several times
    return row_ptr, col


@pytest.mark.parametrize("Q,M", ((1, 64), (65, 130)))
def test_bipartite_sums_bits(pkg, Q, M):
    ops = pkg.ops
    B, A, As = 2, 5, 3
    row_ptr, col = bipartite_graph(Q, M)
    pair_i, pair_j = [2, 0, 2, 2], [1, 4, 4, 0]                           # slot 1 of the sources, 2 and 3 of the targets unnamed
    f = mixed(np.random.default_rng(Q), (len(col), 4, 3))
    in_ptr, in_edge = ops.csr_incoming_edges(dev(row_ptr), dev(col), B, Q, M)
    want_ptr, want_edge = G.incoming(row_ptr, col, B, Q, M)
    assert np.array_equal(in_ptr.cpu().numpy(), want_ptr) and np.array_equal(in_edge.cpu().numpy(), want_edge)
    want = G.pair_grad_sum(f, row_ptr, want_ptr, want_edge, pair_i, pair_j, B, M, A, Q, As)
    grad, grad_src = ops.csr_edge_pair_grad_sum(dev(f), dev(row_ptr), in_ptr, in_edge, pair_i=pair_i, pair_j=pair_j, B=B, M=M, A=A,
                                                Q=Q, As=As)
    assert np.array_equal(grad.cpu().numpy().view(np.int32), want.grad.astype(np.float32).view(np.int32))
    assert np.array_equal(grad_src.cpu().numpy().view(np.int32), want.grad_src.astype(np.float32).view(np.int32))
    inside = raw_sum(pkg, dev(f), dev(row_ptr), in_ptr, in_edge, pair_i, pair_j, B, M, A, 3, Q, As)
    assert torch.equal(bits(inside[0]), bits(grad)) and torch.equal(bits(inside[1]), bits(grad_src))
    # K54 on the same graph: sources and targets with frames of their own
    rot, trans, fmask = frames_case(M, B)
    srot, strans, smask = frames_case(Q + 200, B)
    srot, strans, smask = srot[:, :Q], strans[:, :Q], smask[:, :Q]
    rng = np.random.default_rng(M)
    g_pos, g_rot = mixed(rng, (len(col), 3)), mixed(rng, (len(col), 3, 3))
    ref = G.frames_backward(rot, trans, row_ptr, col, want_ptr, want_edge, fmask, srot, strans, smask, g_pos, g_rot)
    got = ops.csr_edge_frames_backward(dev(rot), dev(trans), dev(row_ptr), dev(col), in_ptr, in_edge, dev(fmask), src_rot=dev(srot),
                                       src_trans=dev(strans), src_mask=dev(smask), grad_pos=dev(g_pos), grad_rot=dev(g_rot))
    for name, out, want64 in zip(("rot", "trans", "src_rot", "src_trans"), got, ref[:4]):
        assert np.array_equal(out.cpu().numpy().view(np.int32), want64.astype(np.float32).view(np.int32)), f"Q={Q} M={M} {name}"
    assert float(got[2].abs().max()) > 0 and not bool(got[2][~dev(smask)].any()) and not bool(got[0][~dev(fmask)].any())


def raw_frames_backward(pkg, rot, trans, mask, row_ptr, col, in_ptr, in_edge, g_pos, g_rot, front):
    lib = pkg._edgegrad.load()
    B, M = rot.shape[:2]
    bufs, outs, back = carve(((B, M, 3, 3), (B, M, 3)), front)
    keep = [rot.contiguous(), trans.contiguous(), mask.to(torch.uint8).contiguous(), row_ptr.contiguous(), col.contiguous(),
            in_ptr.contiguous(), in_edge.contiguous(), g_pos.contiguous(), g_rot.contiguous()]
    p = [t.data_ptr() for t in keep]
    rc = lib.ps_csr_edge_frames_backward_f32(p[0], p[1], p[2], None, None, None, p[3], p[4], col.shape[0], p[5], p[6], in_edge.shape[0],
                                             p[7], p[8], bufs[0].data_ptr() + 4 * front, bufs[1].data_ptr() + 4 * front, None, None,
                                             B, M, M, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    sentinels_intact(bufs, front, back)
    return outs[0].reshape(B, M, 3, 3), outs[1].reshape(B, M, 3)


@pytest.mark.parametrize("N", (1, 63, 65, 130))
def test_frames_backward_bits_and_bound(pkg, N):
    """the self graph: every owner sums its outgoing terms, then its incoming ones, into the same accumulators"""
    ops = pkg.ops
    B = 3
    rot, trans, fmask = frames_case(N)
    idx = E.random_graph(B, N, 7, seed=N)
    idx[2, :, 0] = np.arange(N)                                            # self edges: i == j sums both terms into one owner
    row_ptr, col, _ = C.to_csr(idx)
    col = np.concatenate([col, np.full(3, -1, np.int32)])                  # the tail of a max_edges graph
    n = len(col)
    rng = np.random.default_rng(N)
    g_pos, g_rot = mixed(rng, (n, 3)), mixed(rng, (n, 3, 3))
    real = C.edge_frames(np.nan_to_num(rot), np.nan_to_num(trans), row_ptr, col, fmask).real
    g_pos[~real], g_rot[~real] = np.nan, np.nan                            # nothing is read at the padding and under the mask
    in_ptr, in_edge = ops.csr_incoming_edges(dev(row_ptr), dev(col), B, N, N)
    want_ptr, want_edge = G.incoming(row_ptr, col, B, N, N)
    worst = 0.0
    for which in ("both", "pos", "rot"):
        gp, gr = (g_pos if which != "rot" else None), (g_rot if which != "pos" else None)
        ref = G.frames_backward(rot, trans, row_ptr, col, want_ptr, want_edge, fmask, g_pos=gp, g_rot=gr)
        got = ops.csr_edge_frames_backward(dev(rot), dev(trans), dev(row_ptr), dev(col), in_ptr, in_edge, dev(fmask),
                                           grad_pos=dev(gp), grad_rot=dev(gr))
        assert len(got) == 2
        for name, out, want64, mag in zip(("rot", "trans"), got, ref[:2], ref.mag[:2]):
            assert np.array_equal(out.cpu().numpy().view(np.int32), want64.astype(np.float32).view(np.int32)), f"N={N} {which} {name}"
            worst = max(worst, ratio(out, want64, G.frames_bound(want64, mag), f"K54 N={N} {which} {name}"))
        assert not got[0].cpu().numpy()[~fmask].view(np.int32).any() and not got[1].cpu().numpy()[~fmask].view(np.int32).any()
    both = ops.csr_edge_frames_backward(dev(rot), dev(trans), dev(row_ptr), dev(col), in_ptr, in_edge, dev(fmask), grad_pos=dev(g_pos),
                                        grad_rot=dev(g_rot))
    for front in (1, 2, 3):
        inside = raw_frames_backward(pkg, dev(rot), dev(trans), dev(fmask), dev(row_ptr), dev(col), in_ptr, in_edge, dev(g_pos),
                                     dev(g_rot), front)
        assert torch.equal(bits(inside[0]), bits(both[0])) and torch.equal(bits(inside[1]), bits(both[1]))
    print(f"K54 N={N}: worst error / bound over the cases = {worst:.3f}")


# ---- 3. K52 within the derived bound -------------------------------------------------------------------------------------------------
def shifted(t, off):
    """the same values ``off`` floats past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    return view


@pytest.mark.parametrize("P,R", ((1, 1), (3, 5), (25, 16), (64, 64), (2, 12), (3, 20), (5, 32)))
def test_rbf_backward_within_the_derived_bound(pkg, P, R):
    """(2, 12) and (3, 20): three and five lanes to a pair, where the partial sums meet by shuffles and a wave has idle lanes;
    (5, 32): eight lanes to a pair, the one shape whose last step across lanes is row_half_mirror"""
    ops = pkg.ops
    xyz, mask = chunk_inputs()
    pairs, centers, sigma = tables(5, P, R, seed=R)
    if R in (12, 20, 32):
        centers, sigma = pkg.geometry.rbf_centers(R, 0.0, 12.0)
    pair_i, pair_j = split(pairs)
    kw = dict(pair_i=pair_i, pair_j=pair_j, centers=centers, sigma=sigma)
    worst = 0.0
    for n_edges in CHUNK_EDGES:
        row_ptr, col = chunk_graph(n_edges)
        rng = np.random.default_rng(n_edges + P)
        g_dist = rng.standard_normal((n_edges, P)).astype(np.float32)
        g_rbf = rng.standard_normal((n_edges, P * R)).astype(np.float32)
        real = C.edge_rbf(xyz, row_ptr, col, mask, pair_i, pair_j, centers, sigma).real
        g_dist[~real] = np.nan                                            # nothing is read at the padding and under the mask
        g_rbf.reshape(n_edges, P, R)[~real] = np.nan
        for which in ("both", "rbf", "dist"):
            gd, gr = (g_dist if which != "rbf" else None), (g_rbf if which != "dist" else None)
            ref = G.rbf_backward(xyz, row_ptr, col, mask, pair_i, pair_j, centers, sigma, g_dist=gd, g_rbf=gr)
            got = ops.csr_edge_rbf_backward(dev(xyz), dev(row_ptr), dev(col), dev(mask), grad_dist=dev(gd), grad_rbf=dev(gr), **kw)
            assert tuple(got.shape) == (n_edges, P, 3) and got.dtype == torch.float32
            assert not got.cpu().numpy()[~ref.real].view(np.int32).any(), f"E={n_edges} {which}: the zeros are not exact +0"
            if n_edges:
                live = ref.real
                worst = max(worst, ratio(got.cpu().numpy()[live], ref.f[live], ref.bound[live] + 2.0 ** -149,
                                         f"K52 P={P} R={R} E={n_edges} {which}"))
            if gr is not None and n_edges:
                for off in (1, 2, 3):                                     # the dword arm: the same sums, the same bits
                    moved = ops.csr_edge_rbf_backward(dev(xyz), dev(row_ptr), dev(col), dev(mask), grad_dist=dev(gd),
                                                      grad_rbf=shifted(dev(gr), off), **kw)
                    assert torch.equal(bits(moved), bits(got)), f"P={P} R={R} E={n_edges} {which}: g_rbf {4 * off} bytes off"
        if n_edges > 64:
            assert real.any() and not real.all()
    print(f"K52 P={P} R={R}: worst error / bound over the cases = {worst:.3f}")


def test_a_workgroup_that_takes_more_than_one_span(pkg):
    """K52 launches at most 8192 workgroups, and a workgroup walks spans blockIdx.x, + gridDim.x, ...: with P = 1 a span is 256
    positions, so 2.2 M edges are 8594 spans and the first 402 workgroups take a second one over the LDS tables of their first.
    Eight long rows with every kind of position in them; held to the restatement within the bound, and bit for bit to the
    same list run in two pieces that each fit one pass of the grid"""
    ops = pkg.ops
    B, M, A, n_edges, tail = 2, 4, 2, 2_200_000, 1000
    assert -(-n_edges // 256) > 8192
    rng = np.random.default_rng(52)
    xyz = (rng.standard_normal((B, M, A, 3)) * 3.0).astype(np.float32)
    mask = np.ones((B, M, A), dtype=bool)
    mask[0, 1, 0], mask[1, 2, 1] = False, False
    xyz[~mask] = np.nan
    lengths = rng.multinomial(n_edges - tail, np.ones(B * M) / (B * M))
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = rng.integers(0, M, size=n_edges).astype(np.int32)
    col[rng.random(n_edges) < 0.05] = -1
    col[rng.random(n_edges) < 0.02] = M + 2
    col[n_edges - tail:] = -1
    pair_i, pair_j = [0], [1]
    centers, sigma = pkg.geometry.rbf_centers(4, 0.0, 9.0)
    kw = dict(pair_i=pair_i, pair_j=pair_j, centers=centers, sigma=sigma)
    g_dist = rng.standard_normal((n_edges, 1)).astype(np.float32)
    g_rbf = rng.standard_normal((n_edges, 4)).astype(np.float32)
    ref = G.rbf_backward(xyz, row_ptr, col, mask, pair_i, pair_j, centers, sigma, g_dist=g_dist, g_rbf=g_rbf)
    g_dist[~ref.real] = np.nan
    g_rbf.reshape(n_edges, 1, 4)[~ref.real] = np.nan
    x, m, gd, gr = dev(xyz), dev(mask), dev(g_dist), dev(g_rbf)
    got = ops.csr_edge_rbf_backward(x, dev(row_ptr), dev(col), m, grad_dist=gd, grad_rbf=gr, **kw)
    host = got.cpu().numpy()
    assert not host[~ref.real].view(np.int32).any() and 0.5 < ref.real.mean() < 0.95
    ratio(host[ref.real], ref.f[ref.real], ref.bound[ref.real] + 2.0 ** -149, "K52 over 8594 spans")
    cut = 1_000_003                                                        # no multiple of a span: the pieces' spans lie elsewhere
    pieces = []
    for a, b in ((0, cut), (cut, n_edges)):
        assert -(-(b - a) // 256) <= 8192
        piece_ptr = np.clip(row_ptr - a, 0, b - a)
        pieces.append(ops.csr_edge_rbf_backward(x, dev(piece_ptr), dev(col[a:b]), m, grad_dist=gd[a:b], grad_rbf=gr[a:b], **kw))
    assert torch.equal(bits(torch.cat(pieces)), bits(got)), "a second span of a workgroup differs from the same edges in a first"


def test_an_edge_of_length_zero_gets_a_finite_zero(pkg):
    """an include_self graph: pairs (a, a) on the self edge have d = 0; the gradient there is defined as 0, nothing of the
    incoming gradient is read, and the other pairs of the same edge are as the bound says"""
    geometry, ops = pkg.geometry, pkg.ops
    xyz, mask = chunk_inputs()
    xyz, mask = np.nan_to_num(xyz[1:2]), mask[1:2]                         # the complete structure
    pts = dev(xyz[:, :, 1])
    g = geometry.radius_graph(pts, 6.0, include_self=True)
    row_ptr, col = g.row_ptr.cpu().numpy(), g.col.cpu().numpy()
    pair_i, pair_j = [0, 1, 1, 4], [0, 1, 2, 4]
    centers, sigma = geometry.rbf_centers(16, 0.0, 8.0)
    n, P, R = len(col), 4, 16
    rng = np.random.default_rng(0)
    g_dist, g_rbf = rng.standard_normal((n, P)).astype(np.float32), rng.standard_normal((n, P * R)).astype(np.float32)
    ref = G.rbf_backward(xyz, row_ptr, col, None, pair_i, pair_j, centers, sigma, g_dist=g_dist, g_rbf=g_rbf)
    zero_length = ~ref.real
    assert zero_length.sum() == 3 * M_CHUNK and not zero_length[:, 2].any()
    g_dist[zero_length] = np.nan
    g_rbf.reshape(n, P, R)[zero_length] = np.nan
    got = ops.csr_edge_rbf_backward(dev(xyz), g.row_ptr, g.col, None, pair_i=pair_i, pair_j=pair_j, centers=centers, sigma=sigma,
                                    grad_dist=dev(g_dist), grad_rbf=dev(g_rbf)).cpu().numpy()
    assert np.isfinite(got).all() and not got[zero_length].view(np.int32).any()
    ratio(got[ref.real], ref.f[ref.real], ref.bound[ref.real], "K52 on an include_self graph")
    # and through autograd: finite where plain torch gives NaN
    x = dev(xyz).requires_grad_()
    rbf, dist = geometry.radius_edge_distance_features(x, g, pairs=list(zip(pair_i, pair_j)), centers=centers, sigma=sigma,
                                                       return_dist=True)
    (rbf.sum() + dist.sum()).backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


# ---- 5. the two layouts agree ------------------------------------------------------------------------------------------------------
def both_layouts(pkg, xyz, mask, idx, rot, trans, fmask, w_rbf, w_dist, w_pos, w_rot):
    geometry = pkg.geometry
    out = []
    for layout in ("padded", "csr"):
        x, r, t = dev(xyz).requires_grad_(), dev(rot).requires_grad_(), dev(trans).requires_grad_()
        if layout == "padded":
            rbf, dist = geometry.edge_distance_features(x, dev(idx), dev(mask), return_dist=True)
            fr = geometry.edge_frame_features(r, t, dev(idx), dev(fmask))
            keep = dev(idx >= 0)
            terms = (rbf[keep], dist[keep], fr.local_pos[keep], fr.rel_rot[keep])
        else:
            g = geometry.neighbors_to_radius_graph(dev(idx))
            rbf, dist = geometry.radius_edge_distance_features(x, g, dev(mask), return_dist=True)
            fr = geometry.radius_edge_frame_features(r, t, g, dev(fmask))
            terms = (rbf, dist, fr.local_pos, fr.rel_rot)
        sum(((a * dev(w)).sum() for a, w in zip(terms, (w_rbf, w_dist, w_pos, w_rot)))).backward()
        out.append((x.grad, r.grad, t.grad))
    return out


@pytest.mark.parametrize("padded", (False, True))
def test_the_padded_gradient_is_the_csr_gradient(pkg, padded):
    """without padding the two lists are the same list, and the gradients agree bit for bit; with padding the padded list
    has positions the CSR list lacks, all of them exact zeros, and the issue's bound is what is owed"""
    N, k = 65, 7
    case = E.residue_case(N, 5, seed=3)
    rot, trans, fmask = frames_case(N)
    idx = E.random_graph(3, N, k, seed=5, padded=0.3 if padded else 0.0)
    n = int((idx >= 0).sum())
    rng = np.random.default_rng(9)
    w = [rng.standard_normal(s).astype(np.float32) for s in ((n, 400), (n, 25), (n, 3), (n, 3, 3))]
    (xp, rp, tp), (xc, rc, tc) = both_layouts(pkg, case.xyz, case.mask, idx, np.nan_to_num(rot), np.nan_to_num(trans), fmask, *w)
    equal = all(torch.equal(bits(a), bits(b)) for a, b in ((xp, xc), (rp, rc), (tp, tc)))
    print(f"padded={padded}: the gradients of the two layouts are {'bitwise equal' if equal else 'not bitwise equal'}")
    if not padded:
        assert equal
    # within the bound either way: the CSR gradient against the restatement
    row_ptr, col, _ = C.to_csr(idx)
    centers, sigma = pkg.geometry.rbf_centers()
    pair_i, pair_j = split(list(pkg.geometry.BACKBONE_PAIRS))
    pg = G.rbf_backward(case.xyz, row_ptr, col, case.mask, pair_i, pair_j, centers, sigma, g_dist=w[1], g_rbf=w[0])
    ref = G.pair_grad_sum_any_order(pg.f, pg.bound, row_ptr, col, pair_i, pair_j, 3, N, 5)
    for name, got in (("padded", xp), ("csr", xc)):
        ratio(got, ref.grad, ref.bound, f"layouts, padding={padded}, {name} xyz.grad")
    in_ptr, in_edge = G.incoming(row_ptr, col, 3, N, N)
    fr = G.frames_backward(np.nan_to_num(rot), np.nan_to_num(trans), row_ptr, col, in_ptr, in_edge, fmask, g_pos=w[2], g_rot=w[3])
    for name, got, want, mag in (("rot", rp, fr.rot, fr.mag[0]), ("trans", tp, fr.trans, fr.mag[1])):
        ratio(got, want, G.frames_bound(want, mag), f"layouts, padding={padded}, padded {name}.grad")
    assert torch.equal(bits(rc), bits(dev(fr.rot.astype(np.float32)))) and torch.equal(bits(tc), bits(dev(fr.trans.astype(np.float32))))


# ---- 6. end to end on a PDB file ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pdb_batch():
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, "1a3r_HL.pdb")])


def composed_rbf_gradient(xyz, present, row_ptr, col, pair_i, pair_j, centers, sigma, w_rbf, Q, M):
    """float64 autograd of the composed route: gather, sqrt of the sum of squares, exp"""
    x = torch.from_numpy(np.nan_to_num(xyz).astype(np.float64)).requires_grad_()
    b, q, j, real_edge = (torch.from_numpy(np.asarray(a)) for a in C._edges(row_ptr, col, Q, M))
    ok = torch.from_numpy(present)
    real = real_edge[:, None] & ok[b, q][:, pair_i] & ok[b, j][:, pair_j]
    diff = torch.where(real[..., None], x[b, j][:, pair_j] - x[b, q][:, pair_i], torch.ones(3, dtype=torch.float64))
    d = torch.sqrt((diff * diff).sum(-1))
    rbf = torch.exp(-(((d[..., None] - torch.from_numpy(centers.astype(np.float64))) / sigma) ** 2))
    n, P = d.shape
    (torch.where(real[..., None], rbf, torch.zeros_like(rbf)) * torch.from_numpy(w_rbf).double().reshape(n, P, -1)).sum().backward()
    return x.grad.numpy()


def test_pdb_edge_features_flow_back_to_the_coordinates(pkg):
    """batch.edge_features(graph=batch.radius_graph(10.0)) with coordinates that require grad: ``rbf`` reaches them through
    K52 / K53 and ``local_pos`` through K54 and then the frames' own backward kernel.  Held in three steps, each to float64
    autograd of the composed route: the distance part within the propagated bound (the restatement's exact form, which the
    CPU tests hold to autograd at 1e-9, is autograd's value here too); the frame gradients K54 hands to the frames' backward
    kernel within K54's bound; and the coordinates' gradient as, bit for bit, the sum of the distance part and of what
    ``ops.frames_backward`` makes of K54's output.  That kernel is held to float64 autograd of the Gram-Schmidt frames, for
    arbitrary upstream gradients, by tests/test_gpu_fape.py::test_frames_backward_alone (and through a loss by
    ::test_end_to_end_gradient_reaches_the_coordinates there), against a float32 composition as its yardstick: it has no analytic bound that
    could be propagated here, which is why the frame part is not compared with autograd a second time."""
    geometry, ops = pkg.geometry, pkg.ops
    batch = pdb_batch()
    B, N, A = batch.xyz.shape[:3]
    g = batch.radius_graph(10.0)
    n = g.col.shape[0]
    rng = np.random.default_rng(1)
    w_rbf, w_pos = rng.standard_normal((n, 400)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    batch.xyz.requires_grad_()
    try:
        ef = batch.edge_features(graph=g)
        assert ef.rbf.requires_grad and ef.local_pos.requires_grad and ef.rel_rot.requires_grad and not ef.offset.is_floating_point()
        ((ef.rbf * dev(w_rbf)).sum() + (ef.local_pos * dev(w_pos)).sum()).backward()
        total = batch.xyz.grad.clone()
    finally:
        batch.xyz.grad = None
        batch.xyz.requires_grad_(False)
    plain = batch.edge_features(graph=g)
    assert not plain.rbf.requires_grad and torch.equal(bits(plain.rbf), bits(ef.rbf.detach()))
    assert torch.equal(bits(plain.local_pos), bits(ef.local_pos.detach()))
    xyz, present = batch.xyz.cpu().numpy(), batch._present_atoms().cpu().numpy()
    row_ptr, col = g.row_ptr.cpu().numpy(), g.col.cpu().numpy()
    centers, sigma = geometry.rbf_centers()
    pair_i, pair_j = split([(a, b) for a in range(5) for b in range(5)])
    # the distance part
    pg = G.rbf_backward(xyz, row_ptr, col, present, pair_i, pair_j, centers, sigma, g_rbf=w_rbf, exact=True)
    ref = G.pair_grad_sum_any_order(pg.f, pg.bound, row_ptr, col, pair_i, pair_j, B, N, A)
    auto = composed_rbf_gradient(xyz, present, row_ptr, col, pair_i, pair_j, centers, sigma, w_rbf, N, N)
    assert np.abs(ref.grad - auto).max() <= 1e-9 * np.abs(auto).max()
    in_ptr, in_edge = ops.csr_incoming_edges(g.row_ptr, g.col, B, N, N)
    pair_grad = ops.csr_edge_rbf_backward(batch.xyz, g.row_ptr, g.col, batch._present_atoms(), pair_i=pair_i, pair_j=pair_j,
                                          centers=centers, sigma=sigma, grad_rbf=dev(w_rbf))
    part_rbf = ops.csr_edge_pair_grad_sum(pair_grad, g.row_ptr, in_ptr, in_edge, pair_i=pair_i, pair_j=pair_j, B=B, M=N, A=A)
    ratio(part_rbf, auto, ref.bound, "1a3r_HL, radius 10: the distance part of xyz.grad against float64 autograd")
    # the frame part
    frame_mask = batch._present_atoms()[:, :, :3].all(-1)
    rot, trans = ops.frames(batch.xyz, 0, 1, 2, 1)
    d_rot, d_trans = ops.csr_edge_frames_backward(rot, trans, g.row_ptr, g.col, in_ptr, in_edge, frame_mask, grad_pos=dev(w_pos))
    r64, t64 = rot.cpu().double().requires_grad_(), trans.cpu().double().requires_grad_()
    b, q, j, real = (torch.from_numpy(np.asarray(a)) for a in C._edges(row_ptr, col, N, N))
    fm = frame_mask.cpu()
    real = real & fm[b, q] & fm[b, j]
    pos = torch.einsum("erc,er->ec", r64[b, q], t64[b, j] - t64[b, q])
    (torch.where(real[:, None], pos, torch.zeros_like(pos)) * torch.from_numpy(w_pos).double()).sum().backward()
    fr = G.frames_backward(rot.cpu().numpy(), trans.cpu().numpy(), row_ptr, col, in_ptr.cpu().numpy(), in_edge.cpu().numpy(),
                           fm.numpy(), g_pos=w_pos)
    ratio(d_rot, r64.grad.numpy(), G.frames_bound(r64.grad.numpy(), fr.mag[0]), "1a3r_HL: K54 rot against float64 autograd")
    ratio(d_trans, t64.grad.numpy(), G.frames_bound(t64.grad.numpy(), fr.mag[1]), "1a3r_HL: K54 trans against float64 autograd")
    part_frames = ops.frames_backward(batch.xyz, 0, 1, 2, 1, grad_rot=d_rot, grad_trans=d_trans, residue_mask=frame_mask)
    assert torch.equal(bits(total), bits(part_rbf + part_frames)), "xyz.grad is the sum of its two parts, bit for bit"
    assert bool(torch.isfinite(total).all()) and float(part_frames.abs().max()) > 0


def test_pdb_knn_edge_features_flow_back_like_the_same_list_in_csr_form(pkg):
    """StructureBatch.edge_features on the padded kNN graph with coordinates that require grad: the gradient is, bit for bit,
    that of the same list handed over as a RadiusGraph"""
    geometry = pkg.geometry
    batch = pdb_batch()
    nb = batch.knn_graph(9, cutoff=7.0)                                   # a cutoff: some rows are padded
    assert bool((nb.idx < 0).any()) and bool((nb.idx >= 0).any())
    grads = []
    for g in (nb, geometry.neighbors_to_radius_graph(nb)):
        batch.xyz.requires_grad_()
        try:
            ef = batch.edge_features(graph=g)
            assert ef.rbf.requires_grad and ef.local_pos.requires_grad and not ef.mask.requires_grad
            (ef.rbf.sum() + 0.5 * ef.local_pos.sum() + 0.25 * ef.rel_rot.sum()).backward()
            grads.append(batch.xyz.grad.clone())
        finally:
            batch.xyz.grad = None
            batch.xyz.requires_grad_(False)
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().max()) > 0
    assert torch.equal(bits(grads[0]), bits(grads[1]))


def test_pdb_atom_edge_features_flow_back_to_the_coordinates(pkg):
    geometry = pkg.geometry
    batch = pdb_batch()
    B, N, A = batch.xyz.shape[:3]
    g = batch.atom_radius_graph(4.0)
    n = g.col.shape[0]
    w = np.random.default_rng(2).standard_normal((n, 16)).astype(np.float32)
    batch.xyz.requires_grad_()
    try:
        ef = batch.atom_edge_features(g)
        assert ef.rbf.requires_grad and not ef.mask.requires_grad
        (ef.rbf * dev(w)).sum().backward()
        total = batch.xyz.grad.clone()
    finally:
        batch.xyz.grad = None
        batch.xyz.requires_grad_(False)
    assert not batch.atom_edge_features(g).rbf.requires_grad
    xyz = batch.xyz.cpu().numpy().reshape(B, N * A, 1, 3)
    present = batch._present_atoms().cpu().numpy().reshape(B, N * A, 1)
    row_ptr, col = g.row_ptr.cpu().numpy(), g.col.cpu().numpy()
    centers, sigma = geometry.rbf_centers(16, 0.0, 8.0)
    pg = G.rbf_backward(xyz, row_ptr, col, present, [0], [0], centers, sigma, g_rbf=w, exact=True)
    ref = G.pair_grad_sum_any_order(pg.f, pg.bound, row_ptr, col, [0], [0], B, N * A, 1)
    auto = composed_rbf_gradient(xyz, present, row_ptr, col, [0], [0], centers, sigma, w, N * A, N * A)
    assert np.abs(ref.grad - auto).max() <= 1e-9 * np.abs(auto).max()
    ratio(total.reshape(B, N * A, 1, 3), auto, ref.bound, "1a3r_HL, atom graph 4 A: xyz.grad against float64 autograd")


# ---- 7 and 8. repeatability and the launch contract ---------------------------------------------------------------------------------------
# Two seeded variants with the same masks and other coordinates: radius_graph(max_edges=n) -> edge_features -> a weighted sum
# -> the gradient of the coordinates reaches K52, K53 and K54 and makes no host read.
CONTRACT_EDGES = 1500
SYMBOLS = ("ps_csr_edge_frames_backward_f32", "ps_csr_edge_pair_grad_sum_f32", "ps_csr_edge_rbf_backward_f32")


def _contract_inputs(v):
    case = E.residue_case(37, 5, seed=60)
    other = E.residue_case(37, 5, seed=61)
    xyz = np.nan_to_num(case.xyz if v == "A" else other.xyz)
    return dict(xyz=torch.from_numpy(xyz), atom_mask=torch.from_numpy(case.mask))


@functools.lru_cache(maxsize=None)
def _contract_weights():
    g = torch.Generator().manual_seed(5)
    return tuple(torch.randn(CONTRACT_EDGES, *tail, generator=g).cuda() for tail in ((400,), (3,), (3, 3)))


def _contract_batch(inputs):
    from protstruc_amd import StructureBatch
    batch = StructureBatch.from_xyz(inputs["xyz"].cuda().clone(), inputs["atom_mask"].cuda())
    batch.xyz.requires_grad_()
    return batch


def _contract_run(batch):
    w_rbf, w_pos, w_rot = _contract_weights()
    g = batch.radius_graph(9.0, max_edges=CONTRACT_EDGES)
    ef = batch.edge_features(graph=g)
    loss = (ef.rbf * w_rbf).sum() + (ef.local_pos * w_pos).sum() + (ef.rel_rot * w_rot).sum()
    (grad,) = torch.autograd.grad(loss, batch.xyz)
    in_ptr, in_edge = pkg_geometry().radius_graph_incoming(g, batch.xyz.shape[1])
    return (grad, in_ptr, in_edge)


def pkg_geometry():
    from protstruc_amd import geometry
    return geometry


@functools.lru_cache(maxsize=None)
def contract_eager(v):
    outs = _contract_run(_contract_batch(_contract_inputs(v)))
    torch.cuda.synchronize()
    return outs


def test_contract_case_reaches_the_three_symbols_and_repeats_bit_for_bit(pkg, monkeypatch):
    seen = []
    launch = pkg.ops._launch_edgegrad
    monkeypatch.setattr(pkg.ops, "_launch_edgegrad", lambda name, *args: (seen.append(name), launch(name, *args))[1])
    outs = _contract_run(_contract_batch(_contract_inputs("A")))
    torch.cuda.synchronize()
    assert tuple(sorted(seen)) == SYMBOLS
    a, b = contract_eager("A"), contract_eager("B")
    for again in (outs, _contract_run(_contract_batch(_contract_inputs("A")))):
        assert_all_same(again, a, "a second run")                      # repeatability: bit for bit
    for k in range(3):
        assert not same(a[k], b[k]), f"output {k} is the same for both variants"
    assert bool(torch.isfinite(a[0]).all()) and float(a[0].abs().max()) > 0
    assert 200 < int(a[1][-1]) < CONTRACT_EDGES, "the buffers leave a tail and cut nothing"


def test_launches_on_the_callers_stream(pkg):
    want_a, want_b = contract_eager("A"), contract_eager("B")
    a, b = _contract_inputs("A"), _contract_inputs("B")
    batch = _contract_batch(a)
    new = b["xyz"].cuda()
    side = side_stream_beside_the_default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side), torch.no_grad():
        torch.cuda._sleep(SLEEP_CYCLES)
        batch.xyz.copy_(new)
    control = batch.xyz.detach().clone()                              # the default stream: runs while the side stream sleeps
    with torch.cuda.stream(side):
        outs = _contract_run(batch)
    torch.cuda.synchronize()
    if not same(control, a["xyz"].cuda()):
        pytest.fail("inconclusive -- the control clone did not see variant A")
    assert_all_same(outs, want_b, "on a side stream")
    assert not same(outs[0], want_a[0]), "the gradient was computed from the inputs as they were before the side stream's copy"


def test_the_backward_pass_inside_a_captured_graph(pkg):
    """radius_graph(max_edges=n) -> edge_features -> the gradient, captured on variant A after one eager call and replayed
    twice on variant B over overwritten outputs: no host read anywhere on the route, the incoming lists included"""
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
    with torch.no_grad():
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
    """B = 65535 with Q = 1 against M = 3 targets: structure b is structure b % 3, and every gradient is that of the three,
    bit for bit"""
    geometry = pkg.geometry
    B = 65535
    rng = np.random.default_rng(14)
    xyz = (rng.normal(size=(3, 3, 2, 3)) * 4.0).astype(np.float32)
    src = (rng.normal(size=(3, 1, 2, 3)) * 4.0).astype(np.float32)
    rot, trans = E.random_frames(3, 3, seed=15)
    srot, strans = E.random_frames(3, 1, seed=16)
    lengths3 = np.array([2, 0, 3])
    cols3 = [np.array([2, 0]), np.array([], dtype=np.int64), np.array([0, 1, 2])]
    pick = np.arange(B) % 3
    centers, sigma = geometry.rbf_centers(4, 0.0, 12.0)
    pairs = [(0, 1), (1, 1)]
    weights = [rng.standard_normal((5,) + tail).astype(np.float32) for tail in ((8,), (2,), (3,), (3, 3))]

    def gradients(reps):
        pk = np.arange(reps) % 3
        row_ptr = np.concatenate([[0], np.cumsum(lengths3[pk])]).astype(np.int64)
        col = np.concatenate([cols3[p] for p in pk]).astype(np.int32)
        g = graph(pkg, row_ptr, col, reps, 1)
        tile = lambda a: dev(a)[torch.from_numpy(pk).cuda()].clone().requires_grad_()          # noqa: E731
        leaves = [tile(a) for a in (xyz, src, rot, trans, srot, strans)]
        rbf, dist = geometry.radius_edge_distance_features(leaves[0], g, pairs=pairs, centers=centers, sigma=sigma, return_dist=True,
                                                           source_xyz=leaves[1])
        fr = geometry.radius_edge_frame_features(leaves[2], leaves[3], g, source_rot=leaves[4], source_trans=leaves[5])
        w = [dev(a).repeat(reps // 3, *([1] * (a.ndim - 1))) for a in weights]
        sum((o * v).sum() for o, v in zip((rbf, dist, fr.local_pos, fr.rel_rot), w)).backward()
        torch.cuda.synchronize()
        return [leaf.grad for leaf in leaves]
    small, big = gradients(3), gradients(B)
    for name, three, got in zip(("xyz", "source_xyz", "rot", "trans", "source_rot", "source_trans"), small, big):
        assert float(three.abs().max()) > 0 and got.shape[0] == B
        assert same(got, three.repeat(B // 3, *([1] * (three.ndim - 1)))), f"{name}.grad at B = 65535 is not the B = 3 result repeated"
