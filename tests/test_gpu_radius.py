"""GPU tests of the radius graph (ps_radius_tile_boxes_f32, ps_radius_count_f32, ps_radius_fill_f32; ops.radius_graph;
geometry.radius_graph, .radius_graph_edges; StructureBatch.radius_graph, .atom_radius_graph).

Yardstick: tests/radius_ref.py, the definition in float64 in the kernels' own order of operations on the same float32
inputs.  The criterion is EQUALITY throughout: ``count``, ``row_ptr`` and every ``col`` equal the yardstick's, ``dist`` is
bitwise equal (compared as int32).  Every case runs twice -- through the public function and through the C ABI into
``col`` / ``dist`` carved out of sentinel-filled buffers at a start that is no 16-byte boundary -- and the two results
must agree bit for bit, which is also the determinism check; no sentinel may change.  tests/test_radius_host.py holds the
conditions that keep the families here from passing vacuously.
"""
import functools
import os
import threading

import numpy as np
import pytest
import torch

from tests import radius_ref as R
from tests.conftest import GOLDEN_DIR
from tests.launch_cases import Case, on_device
from tests.test_gpu_launch_contract import (MAX_BATCH, SENTINEL, SLEEP_CYCLES, assert_all_same, raw, same,
                                            side_stream_beside_the_default_stream, tile)

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000
PDB_FILES = ("1REX", "4EOT", "1ad0_DC", "5cjx_HL")


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, build, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    build.build(force=False)
    _lib.load()
    return protstruc_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def in_sentinels(pkg, x, cutoff, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None,
                 include_self=False, capacity=None):
    """The three launches through the C ABI, with col and dist carved out of buffers of sentinels 4 to 12 bytes past a
    16-byte boundary: (row_ptr, col, dist, count), after checking that nothing around them was written.  ``capacity`` None:
    exactly the number of edges; otherwise entries past the edges keep the sentinel."""
    lib = pkg._lib.load()
    B, M = x.shape[:2]
    Q = M if queries is None else queries.shape[1]
    u8 = lambda t: None if t is None else t.to(torch.uint8).contiguous()       # noqa: E731
    i32 = lambda t: None if t is None else t.to(torch.int32).contiguous()      # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()                         # noqa: E731
    keep = [x.float().contiguous(), u8(mask), None if queries is None else queries.float().contiguous(), u8(query_mask),
            i32(exclude), i32(query_exclude)]
    stream = torch.cuda.current_stream().cuda_stream
    boxes = torch.empty(B, -(-M // 64), 40, device="cuda")
    count = torch.full((B * Q + 2,), 777, dtype=torch.int32, device="cuda")
    assert lib.ps_radius_tile_boxes_f32(ptr(keep[0]), ptr(keep[1]), ptr(boxes), B, M, stream) == 0
    args = [ptr(t) for t in keep] + [float(cutoff), int(include_self), ptr(boxes)]
    assert lib.ps_radius_count_f32(*args, ptr(count[1:]), None, B, M, Q, stream) == 0
    assert count[0] == 777 and count[-1] == 777
    count = count[1:-1].reshape(B, Q)
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)])
    n = int(row_ptr[-1]) if capacity is None else capacity
    front, back = 1 + (M + n) % 3, 9
    bufs = [torch.full((front + n + back,), 777, dtype=dt, device="cuda") for dt in (torch.int32, torch.float32)]
    col, dist = (buf[front:front + n] for buf in bufs)
    assert n == 0 or col.data_ptr() % 16 in (4, 8, 12)
    assert lib.ps_radius_fill_f32(*args, ptr(row_ptr), n, ptr(col) if n else None, ptr(dist) if n else None, B, M, Q, stream) == 0
    torch.cuda.synchronize()
    for buf in bufs:
        assert (buf[:front] == 777).all() and (buf[front + n:] == 777).all(), "a sentinel around an output changed"
    return row_ptr, col, dist, count


def run(pkg, x, cutoff, mask=None, **kw):
    """numpy in; the public function and the C ABI inside sentinels, bitwise equal; the public function's result"""
    args = {name: dev(t) if isinstance(t, np.ndarray) else t for name, t in kw.items()}
    got = pkg.geometry.radius_graph(dev(x), cutoff, dev(mask), **args)
    assert isinstance(got, pkg.geometry.RadiusGraph)
    assert not any(t.requires_grad for t in got) and all(t.is_cuda for t in got)
    again = in_sentinels(pkg, dev(x), cutoff, dev(mask), **args)
    for a, b in zip(got, again):
        assert a.shape == b.shape and a.dtype == b.dtype and same(a, b), "two launches differ"
    return got


def assert_equal_to_yardstick(got, ref, what):
    row_ptr, col, dist, count = (t.cpu().numpy() for t in got)
    assert (row_ptr.dtype, col.dtype, dist.dtype, count.dtype) == (np.int64, np.int32, np.float32, np.int32)
    assert count.shape == ref.count.shape and np.array_equal(count, ref.count), (what, np.argwhere(count != ref.count)[:8])
    assert np.array_equal(row_ptr, ref.row_ptr), what
    assert col.shape == ref.col.shape and np.array_equal(col, ref.col), (what, np.flatnonzero(col != ref.col)[:8])
    assert np.array_equal(dist.view(np.int32), ref.dist.view(np.int32)), what


# ---- synthetic chains --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", R.CUTOFFS)
@pytest.mark.parametrize("M", R.SIZES)
def test_chains_equal_the_yardstick(pkg, M, cutoff):
    case = R.chain(M)
    longest = 0
    for keys in (None, case.key):
        for include_self in (False, True):
            ref = R.batch(case.x, cutoff, case.mask, exclude=keys, include_self=include_self)
            got = run(pkg, case.x, cutoff, case.mask, exclude=keys, include_self=include_self)
            assert_equal_to_yardstick(got, ref, f"M = {M}, cutoff = {cutoff}, keys = {keys is not None}, self = {include_self}")
            assert not got.count[1].any() and not got.count[0][~dev(case.mask)[0]].any()      # masked queries: empty rows
            longest = max(longest, int(got.count.max()))
    if M == 1000 and cutoff == 12.0:
        assert longest > 64                                                                  # no cap
    # without a mask the NaN points are nobody's neighbours and have none: the same lists, with no special case
    bare = run(pkg, case.x, cutoff)
    assert_equal_to_yardstick(bare, R.batch(case.x, cutoff), f"M = {M}, no mask")


@pytest.mark.parametrize("Q", R.CROSS_Q)
def test_cross_queries_with_masks_and_keys(pkg, Q):
    case = R.chain(257)
    rng = np.random.default_rng(Q)
    centre = np.nanmean(case.x[2], axis=0)
    queries = (centre + rng.normal(size=(3, Q, 3)) * 10.0).astype(np.float32)
    query_mask = rng.random((3, Q)) > 0.25 if Q > 1 else np.ones((3, 1), dtype=bool)
    queries[0][~query_mask[0]] = np.nan                                                  # NaN under the query mask
    query_key = rng.integers(0, 60, size=(3, Q)).astype(np.int32)
    for cutoff in R.CUTOFFS:
        for keys in ({}, dict(exclude=case.key, query_exclude=query_key)):
            ref = R.batch(case.x, cutoff, case.mask, queries, query_mask, **keys)
            got = run(pkg, case.x, cutoff, case.mask, queries=queries, query_mask=query_mask, **keys)
            assert tuple(got.count.shape) == (3, Q) and got.row_ptr.shape == (3 * Q + 1,)
            assert_equal_to_yardstick(got, ref, f"Q = {Q}, cutoff = {cutoff}, keys = {bool(keys)}")
    if Q > 1:
        assert int(R.batch(case.x, 12.0, case.mask, queries, query_mask).count.max()) > 64                # no cap here either


def test_unmasked_nan_and_infinite_points(pkg):
    x = R.chain(129).x[2:].copy()
    x[0, 5] = np.nan
    x[0, 9, 1] = np.inf
    x[0, 70, 2] = -np.inf
    ref = R.batch(x, 12.0)
    assert not ref.count[0, [5, 9, 70]].any() and not np.isin(ref.col, (5, 9, 70)).any() and ref.count[0, 0] > 0
    assert_equal_to_yardstick(run(pkg, x, 12.0), ref, "NaN and inf")


# ---- no block coherent; nearly every block dropped; pairs exactly at the cutoff ---------------------------------------------------------
def test_a_permuted_chain(pkg):
    case = R.permuted()
    ref = R.batch(case.x, 12.0)
    assert ref.count.max() > 64
    got = run(pkg, case.x, 12.0)
    assert_equal_to_yardstick(got, ref, "permuted")
    assert int(got.row_ptr[-1]) == 2 * int(got.count[0].sum())          # the same graph under another numbering
    stats = pkg.ops.radius_graph(dev(case.x), 12.0, return_stats=True)[4].sum(dim=1).cpu().numpy()
    assert stats[0, 1] > 0 and stats[1, 1] == 0, stats                   # the chain drops blocks, its permuted copy none


def test_two_clusters_far_apart(pkg):
    case = R.clusters()
    got = run(pkg, case.x, 12.0, case.mask)
    assert_equal_to_yardstick(got, R.batch(case.x, 12.0, case.mask), "clusters")
    M = case.x.shape[1]
    col, row_ptr = got.col.cpu().numpy(), got.row_ptr.cpu().numpy()
    assert (col[:row_ptr[M // 2]] < M // 2).all() and (col[row_ptr[M // 2]:] >= M // 2).all()
    stats = pkg.ops.radius_graph(dev(case.x), 12.0, dev(case.mask), return_stats=True)[4].sum(dim=(0, 1)).cpu().numpy()
    assert stats[0] == 36 and stats[1] == 18, stats                      # 6 waves x 6 blocks, every cross pair dropped


@pytest.mark.parametrize("reverse", (False, True))
def test_lattice_pairs_exactly_at_the_cutoff_are_kept(pkg, reverse):
    x = R.lattice().x[:, ::-1].copy() if reverse else R.lattice().x
    ref = R.batch(x, R.LATTICE_CUTOFF)
    at = (ref.dist == np.float32(R.LATTICE_CUTOFF)).sum()
    assert at >= 100 and ref.count.max() > 64
    assert_equal_to_yardstick(run(pkg, x, R.LATTICE_CUTOFF), ref, f"lattice, reverse = {reverse}")
    keyed = np.broadcast_to(np.arange(x.shape[1], dtype=np.int32) // 8, x.shape[:2]).copy()
    assert_equal_to_yardstick(run(pkg, x, R.LATTICE_CUTOFF, exclude=keyed), R.batch(x, R.LATTICE_CUTOFF, exclude=keyed), "lattice, keys")


@pytest.mark.parametrize("cutoff", (3.0, 4.1, 7.3e-21, 1.0e4))
def test_the_smallest_trap(pkg, cutoff):
    """64 copies of the origin, then 64 copies of (c, 0, 0): with c = cutoff the 64 x 64 pairs across are kept, with the
    next float above they are not"""
    c = np.float32(cutoff)
    at, beyond = R.trap(c), R.trap(np.nextafter(c, np.float32(np.inf)))
    got = run(pkg, at.x, float(c))
    assert_equal_to_yardstick(got, R.batch(at.x, float(c)), "c = cutoff")
    assert (got.count == 127).all() and int((got.dist == float(c)).sum()) == 2 * 64 * 64
    got = run(pkg, beyond.x, float(c))
    assert_equal_to_yardstick(got, R.batch(beyond.x, float(c)), "c = the next float")
    assert (got.count == 63).all() and not got.dist.any()


# ---- the PDB files ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pdb_batch():
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, name + ".pdb") for name in PDB_FILES])


def assert_symmetric(got, M):
    """(q, j) is an edge iff (j, q) is, with the same bits in dist: the edge list sorted by (b, j, q) is itself"""
    b, i, j = (t.cpu().numpy() for t in _edges(got))
    d = got.dist.cpu().numpy().view(np.int32)
    there = np.lexsort((j, i, b))
    back = np.lexsort((i, j, b))
    assert np.array_equal(there, np.arange(len(b)))                      # rows in (b, q) order, ascending j within
    assert np.array_equal(i[there], j[back]) and np.array_equal(j[there], i[back]) and np.array_equal(d[there], d[back])
    assert (j < M).all() and (j >= 0).all()


def _edges(got):
    from protstruc_amd import geometry
    return geometry.radius_graph_edges(got)


def assert_short_rows_are_k24(got, knn):
    """rows with <= 64 entries against the live nearest_neighbors(k = 64) at the same cutoff: the same set, the same bits"""
    count = got.count.reshape(-1)
    short = count <= 64
    assert bool(short.any()) and torch.equal(knn.count.reshape(-1)[short], count[short])
    assert (knn.count.reshape(-1)[~short] == 64).all()
    rows = torch.repeat_interleave(torch.arange(count.numel(), device="cuda"), count.long())
    keep = short[rows]
    idx, dist = knn.idx.reshape(-1, 64), knn.dist.reshape(-1, 64)
    order = torch.argsort(torch.where(idx >= 0, idx, torch.full_like(idx, 2 ** 30)), dim=1, stable=True)   # ascending j, padding last
    idx, dist = torch.gather(idx, 1, order), torch.gather(dist, 1, order)
    real = (idx >= 0) & short[:, None]
    assert torch.equal(idx[real], got.col[keep]) and torch.equal(dist[real].view(torch.int32), got.dist[keep].view(torch.int32))


def test_pdb_residue_graphs(pkg):
    batch = pdb_batch()
    ca = batch.get_xyz()[:, :, 1].contiguous()
    present = batch._present_atoms()[:, :, 1]
    got = batch.radius_graph(cutoff=10.0)
    assert isinstance(got, pkg.geometry.RadiusGraph) and tuple(got.count.shape) == tuple(ca.shape[:2])
    assert_equal_to_yardstick(got, R.batch(ca.cpu().numpy(), 10.0, present.cpu().numpy()), "radius_graph")
    assert_symmetric(got, ca.shape[1])
    assert_short_rows_are_k24(got, batch.knn_graph(k=64, cutoff=10.0))
    for b in range(4):                                                                   # padded residues: nothing
        assert not got.count[b][~batch.residue_mask[b]].any()
    key = batch._chain_keys()
    other = batch.radius_graph(cutoff=12.0, other_chains_only=True, include_self=True)
    assert_equal_to_yardstick(other, R.batch(ca.cpu().numpy(), 12.0, present.cpu().numpy(), exclude=key.cpu().numpy(),
                                             include_self=True), "other_chains_only")
    b, i, j = _edges(other)
    assert (key[b, i] != key[b, j]).all() and len(b) > 0
    assert_short_rows_are_k24(other, batch.knn_graph(k=64, cutoff=12.0, other_chains_only=True, include_self=True))


def test_pdb_atom_graph(pkg):
    batch = pdb_batch()
    B, N, A = batch.get_xyz().shape[:3]
    x = batch.get_xyz().reshape(B, N * A, 3)
    present = batch._present_atoms().reshape(B, N * A)
    key = torch.arange(N, dtype=torch.int32, device="cuda").repeat_interleave(A).expand(B, N * A)
    got = batch.atom_radius_graph(cutoff=5.0)
    ref = R.batch(x.cpu().numpy(), 5.0, present.cpu().numpy(), exclude=key.cpu().numpy())
    assert_equal_to_yardstick(got, ref, "atom_radius_graph")
    wide = batch.atom_radius_graph(cutoff=9.0)                                           # an atom has hundreds of neighbours
    assert_equal_to_yardstick(wide, R.batch(x.cpu().numpy(), 9.0, present.cpu().numpy(), exclude=key.cpu().numpy()), "9 A")
    assert int(got.count.max()) <= 64 < int(wide.count.max())
    assert_short_rows_are_k24(wide, batch.atom_knn_graph(k=64, cutoff=9.0))
    assert_symmetric(got, N * A)                        # the residue key is symmetric too
    b, i, j = _edges(got)
    assert (i // A != j // A).all()
    assert_short_rows_are_k24(got, batch.atom_knn_graph(k=64, cutoff=5.0))
    backbone = batch.atom_radius_graph(cutoff=4.0, atoms=("N", "CA", "C", "O"), exclude_same_residue=False)
    chosen = torch.zeros(A, dtype=torch.bool, device="cuda")
    chosen[:4] = True
    picked = (batch._present_atoms() & chosen).reshape(B, N * A)
    assert_equal_to_yardstick(backbone, R.batch(x.cpu().numpy(), 4.0, picked.cpu().numpy()), "backbone atoms")


# ---- max_edges -------------------------------------------------------------------------------------------------------------------
def test_max_edges(pkg):
    case = R.chain(257)
    ref = R.batch(case.x, 12.0, case.mask)
    E = int(ref.row_ptr[-1])
    assert E > 1000
    x, mask = dev(case.x), dev(case.mask)
    for capacity in (E + 37, E, E - 501, 0):
        n = min(E, capacity)
        got = pkg.geometry.radius_graph(x, 12.0, mask, max_edges=capacity)
        row_ptr, col, dist, count = (t.cpu().numpy() for t in got)
        assert col.shape == dist.shape == (capacity,)
        assert np.array_equal(row_ptr, ref.row_ptr) and np.array_equal(count, ref.count)            # exact whatever the capacity
        assert np.array_equal(col[:n], ref.col[:n]) and np.array_equal(dist[:n].view(np.int32), ref.dist[:n].view(np.int32))
        assert (col[n:] == -1).all() and (dist[n:].view(np.int32) == INF_BITS).all()
        # the C ABI inside sentinels: the prefix is written, nothing past the edges or past the capacity
        raw_ptr, raw_col, raw_dist, raw_count = in_sentinels(pkg, x, 12.0, mask, capacity=capacity)
        assert np.array_equal(raw_ptr.cpu().numpy(), ref.row_ptr) and np.array_equal(raw_count.cpu().numpy(), ref.count)
        assert np.array_equal(raw_col.cpu().numpy()[:n], ref.col[:n]) and (raw_col[n:] == 777).all() and (raw_dist[n:] == 777).all()
        assert np.array_equal(raw_dist.cpu().numpy()[:n].view(np.int32), ref.dist[:n].view(np.int32))
    with pytest.raises(ValueError, match="max_edges was too small"):
        pkg.geometry.radius_graph_edges(pkg.geometry.radius_graph(x, 12.0, mask, max_edges=E - 1))


# ---- the layers above ------------------------------------------------------------------------------------------------------------
def test_edges_are_the_triples_and_carry_gradients(pkg):
    """Distances recomputed from the triples equal ``dist`` to float32 rounding (a difference of two coordinates below 64 A
    and a norm below 16 A: under 5e-6 A), and the gradient reaches the coordinates."""
    case = R.chain(129)
    x = torch.nan_to_num(dev(case.x)).requires_grad_(True)
    mask = dev(case.mask)
    g = pkg.geometry.radius_graph(x, 8.0, mask)
    b, i, j = pkg.geometry.radius_graph_edges(g)
    assert all(t.dtype == torch.int64 and t.shape == g.col.shape for t in (b, i, j)) and len(b) > 100
    count = torch.zeros(3 * 129, dtype=torch.int64, device="cuda").index_add_(0, b * 129 + i, torch.ones_like(b))
    assert torch.equal(count.reshape(3, 129), g.count.long()) and torch.equal(j, g.col.long())
    edge = (x[b, i] - x[b, j]).norm(dim=-1)
    assert float((edge.detach() - g.dist).abs().max()) <= 1e-5
    edge.sum().backward()
    assert torch.isfinite(x.grad).all() and bool(x.grad[0][mask[0]].any()) and not x.grad[1].any()


def test_ops_with_nothing_to_do_launch_nothing(pkg, monkeypatch):
    ops = pkg.ops

    def no_launch(*args):
        raise AssertionError("an empty call launched a kernel")

    monkeypatch.setattr(ops, "_launch", no_launch)
    for B, M, Q in ((0, 5, None), (2, 0, None), (2, 0, 5), (2, 5, 0), (0, 0, 0)):
        x = torch.zeros(B, M, 3, device="cuda")
        queries = None if Q is None else torch.zeros(B, Q, 3, device="cuda")
        rows = M if Q is None else Q
        for capacity in (None, 7):
            row_ptr, col, dist, count = ops.radius_graph(x, 4.0, queries=queries, max_edges=capacity)
            assert tuple(row_ptr.shape) == (B * rows + 1,) and tuple(count.shape) == (B, rows) and not row_ptr.any()
            assert (row_ptr.dtype, col.dtype, dist.dtype, count.dtype) == (torch.int64, torch.int32, torch.float32, torch.int32)
            assert col.shape == dist.shape == (capacity or 0,) and (col == -1).all() and (dist.view(torch.int32) == INF_BITS).all()
            assert col.is_cuda and not count.any()


def test_geometry_takes_cpu_tensors_and_arrays(pkg):
    case = R.chain(65)
    ref = R.batch(case.x, 12.0, case.mask)
    got = pkg.geometry.radius_graph(torch.from_numpy(case.x), 12.0, torch.from_numpy(case.mask))
    assert all(isinstance(t, torch.Tensor) and t.device.type == "cpu" for t in got)
    assert_equal_to_yardstick(got, ref, "CPU tensors")
    arrays = pkg.geometry.radius_graph(case.x, 12.0, case.mask)
    assert all(isinstance(t, np.ndarray) for t in arrays) and np.array_equal(arrays.col, ref.col)
    strided = torch.full((3, 65, 2, 5), 99.0, device="cuda", dtype=torch.float64)
    strided[:, :, 1, 1:4] = dev(case.x)
    assert_equal_to_yardstick(pkg.geometry.radius_graph(strided[:, :, 1, 1:4], 12.0, dev(case.mask).float()), ref, "strided float64")


# ---- the launch contract -----------------------------------------------------------------------------------------------------------
CONTRACT_EDGES = 2500


def _contract_inputs(v):
    M, Q, seed = 70, 40, "AB".index(v)
    c = R.knn_ref.chain_case(M, seed=21 + seed)
    rng = np.random.default_rng(30 + seed)
    queries = np.stack([np.nanmean(c.x[2], axis=0) + R.knn_ref.cloud(Q, seed=31 + 3 * seed + b, spread=6.0) for b in range(3)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))                               # noqa: E731
    return dict(points=t(c.x).double(), point_mask=t(c.mask).float(), queries=t(queries.astype(np.float32)),
                query_mask=t(rng.random((3, Q)) < 0.8), exclude=t(np.broadcast_to(np.arange(M) // 4, (3, M))).long(),
                query_exclude=t(rng.integers(0, 10, (3, Q))))


def _ops():
    from protstruc_amd import ops
    return ops


CONTRACT = (
    Case("radius_graph", ("ps_radius_tile_boxes_f32", "ps_radius_count_f32", "ps_radius_fill_f32"), _contract_inputs,
         lambda i: _ops().radius_graph(i["points"], 9.0, i["point_mask"], exclude=i["exclude"], max_edges=CONTRACT_EDGES),
         strided=("points",)),
    Case("radius_graph_cross", ("ps_radius_tile_boxes_f32", "ps_radius_count_f32", "ps_radius_fill_f32"), _contract_inputs,
         lambda i: _ops().radius_graph(i["points"], 9.0, i["point_mask"], queries=i["queries"], query_mask=i["query_mask"],
                                       exclude=i["exclude"], query_exclude=i["query_exclude"], max_edges=CONTRACT_EDGES),
         strided=("points",)),
)
BY_NAME = {case.name: case for case in CONTRACT}
NAMES = list(BY_NAME)


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
        assert a.shape == b.shape and a.dtype == b.dtype and not same(a, b), (name, k)


def test_contract_cases_cover_the_header_and_meet_the_yardstick(pkg):
    assert sorted({s for case in CONTRACT for s in case.symbols}) == sorted(set(pkg._lib.GRAPH_SIGNATURES) - {"ps_graph_api"})
    for name in NAMES:
        assert_variants_differ(name)
    for v in "AB":
        i = {k: t.numpy() for k, t in _contract_inputs(v).items()}
        x, mask = i["points"].astype(np.float32), i["point_mask"] != 0
        for name, ref in (("radius_graph", R.batch(x, 9.0, mask, exclude=i["exclude"])),
                          ("radius_graph_cross", R.batch(x, 9.0, mask, i["queries"], i["query_mask"], i["exclude"], i["query_exclude"]))):
            E = int(ref.row_ptr[-1])
            assert 100 < E < CONTRACT_EDGES
            row_ptr, col, dist, count = eager(name, v)
            assert_equal_to_yardstick((row_ptr, col[:E], dist[:E], count), ref, f"contract {name} {v}")
            assert (col[E:] == -1).all() and (dist[E:].view(torch.int32) == INF_BITS).all()


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
    """the ``max_edges`` form makes no host read: captured on variant A after one eager call, replayed twice on variant B
    over overwritten outputs"""
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
    """B = 65535 at M = 2: structure b is structure b % 3 of three -- a pair within the cutoff, a pair beyond it, a pair with
    one point masked -- and the lists are those of the three, repeated"""
    x = torch.tensor([[[0.0, 0, 0], [3.0, 0, 0]], [[0.0, 0, 0], [3.5, 0, 0]], [[1.0, 1, 1], [float("nan"), 0, 0]]], device="cuda")
    mask = torch.tensor([[True, True], [True, True], [True, False]], device="cuda")
    small = pkg.ops.radius_graph(x, 3.0, mask, include_self=True)
    assert_equal_to_yardstick(small, R.batch(x.cpu().numpy(), 3.0, mask.cpu().numpy(), include_self=True), "M = 2")
    assert small[3].tolist() == [[2, 2], [1, 1], [1, 0]] and small[1].tolist() == [0, 1, 0, 1, 0, 1, 0]
    big = pkg.ops.radius_graph(tile(x), 3.0, tile(mask), include_self=True)
    torch.cuda.synchronize()
    times = MAX_BATCH // 3
    assert big[3].shape == (MAX_BATCH, 2) and same(big[3], tile(small[3]))
    assert same(big[1], small[1].repeat(times)) and same(big[2], small[2].repeat(times))
    starts = torch.arange(times, device="cuda")[:, None] * small[0][-1]                  # three structures hold small[0][-1] edges
    assert same(big[0], torch.cat([small[0][:1], (small[0][1:][None, :] + starts).reshape(-1)]))
    with pytest.raises(ValueError, match="at most 65535 structures per call, got 65536"):
        pkg.ops.radius_graph(torch.zeros(65536, 2, 3, device="cuda"), 3.0)
