"""Host-side checks of the nearest-neighbour graphs: the yardstick itself (tests/knn_ref.py) on hand-computed cases and on
the integer lattice, the C ABI's surface, the argument validation of ``ops.nearest_neighbors``, the signatures of the
layers above, what ``StructureBatch`` hands to the geometry layer, ``geometry.gather_neighbors``, and the composed route of
the timing tool.  No GPU needed."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import knn_ref as R
from tests.conftest import GOLDEN_DIR

INF = np.float32(np.inf)


def f32(*rows):
    return np.array(rows, dtype=np.float32)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def test_three_collinear_points():
    x = f32([0, 0, 0], [1, 0, 0], [3, 0, 0])
    ref = R.knn(x, 2)
    assert ref.idx.tolist() == [[1, 2], [0, 2], [1, 0]]
    assert ref.dist.tolist() == [[1.0, 3.0], [1.0, 2.0], [2.0, 3.0]] and ref.count.tolist() == [2, 2, 2]
    assert ref.idx.dtype == np.int32 and ref.dist.dtype == np.float32 and ref.count.dtype == np.int32
    first = R.knn(x, 1)
    assert first.idx.tolist() == [[1], [0], [1]] and R.first(ref, 1).idx.tolist() == first.idx.tolist()


def test_a_duplicate_pair_orders_by_index():
    x = f32([5, 5, 5], [0, 0, 0], [5, 5, 5], [5, 5, 6])
    ref = R.knn(x, 3)
    assert ref.idx[3].tolist() == [0, 2, 1] and ref.dist[3].tolist()[:2] == [1.0, 1.0]     # equal distances: the lower index
    assert ref.idx[0].tolist() == [2, 3, 1] and ref.dist[0, 0] == 0.0                       # distance 0 is a neighbour
    assert ref.idx[2].tolist() == [0, 3, 1]
    assert R.knn(x, 1).idx[:, 0].tolist() == [2, 0, 0, 0]


def test_masked_and_unmasked_nan():
    x = f32([0, 0, 0], [np.nan, np.nan, np.nan], [2, 0, 0], [0, 1, 0])
    masked = R.knn(x, 3, mask=np.array([1, 0, 1, 1], dtype=bool))
    assert masked.idx.tolist() == [[3, 2, -1], [-1, -1, -1], [0, 3, -1], [0, 2, -1]]
    assert masked.count.tolist() == [2, 0, 2, 2] and (masked.dist[1] == INF).all() and masked.dist[0, 2] == INF
    # unmasked, the NaN point is nobody's neighbour and has none: the same lists
    bare = R.knn(x, 3)
    assert bare.idx.tolist() == masked.idx.tolist() and bare.count.tolist() == masked.count.tolist()
    assert np.array_equal(bare.dist.view(np.int32), masked.dist.view(np.int32))
    inf = R.knn(f32([0, 0, 0], [np.inf, 0, 0], [1, 0, 0]), 2)
    assert inf.idx.tolist() == [[2, -1], [-1, -1], [0, -1]]


def test_keys_cutoff_padding_and_self():
    x = f32([0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3])
    keyed = R.knn(x, 2, exclude=np.array([7, 7, 8, 9]))
    assert keyed.idx.tolist() == [[2, 3], [2, 3], [0, 1], [0, 1]]                           # 0 and 1 share a key
    cut = R.knn(x, 3, cutoff=2.0)                                                           # exactly at a distance: inclusive
    assert cut.idx[0].tolist() == [1, 2, -1] and cut.dist[0].tolist()[:2] == [1.0, 2.0] and cut.count.tolist() == [2, 1, 1, 0]
    assert R.knn(x, 3, cutoff=np.nextafter(np.float32(2.0), np.float32(0.0))).count.tolist() == [1, 1, 0, 0]
    wide = R.knn(x, 6)                                                                      # k above the candidates: padded
    assert wide.count.tolist() == [3, 3, 3, 3] and (wide.idx[:, 3:] == -1).all() and (wide.dist[:, 3:] == INF).all()
    own = R.knn(x, 2, include_self=True)
    assert own.idx[:, 0].tolist() == [0, 1, 2, 3] and not own.dist[:, 0].any() and own.idx[:, 1].tolist() == [1, 0, 0, 0]
    # cross queries: keys on both sides, a masked query
    cross = R.knn(x, 2, queries=f32([0, 0, 0.5], [9, 9, 9]), query_mask=np.array([True, False]),
                  exclude=np.array([0, 1, 2, 3]), query_exclude=np.array([0, 0]))
    assert cross.idx.tolist() == [[1, 2], [-1, -1]] and cross.count.tolist() == [2, 0]


def test_the_order_of_operations_is_the_stated_one():
    """d2 = (dx*dx + dy*dy) + dz*dz in double, each operation rounded on its own, and one rounding to float32"""
    x = f32([0, 0, 0], [0.1, 0.7, 1.3])
    X = x.astype(np.float64)
    dx, dy, dz = X[1] - X[0]
    assert R.knn(x, 1).d2[0, 1] == (dx * dx + dy * dy) + dz * dz
    assert R.knn(x, 1).dist[0, 0] == np.float32(np.sqrt((dx * dx + dy * dy) + dz * dz))


def test_lattice_has_ties_across_the_k_boundary():
    """What makes the GPU test on the lattice a test of the tie rule: 208 of its 216 rows have the 7th and 8th nearest at
    exactly equal distance, 192 the 27th and 28th."""
    x = R.lattice()
    assert x.shape == (216, 3) and x.dtype == np.float32 and x[1].tolist() == [0, 0, 1] and x[36].tolist() == [1, 0, 0]
    assert R.boundary_ties(R.knn(x, 7), 7) == 208
    assert R.boundary_ties(R.knn(x, 27), 27) == 192
    corner = R.knn(x, 7).idx[0].tolist()
    assert corner[:3] == [1, 6, 36] and corner[3:6] == [7, 37, 42] and corner[6] == 43   # d2 = 1, 1, 1, 2, 2, 2, 3


def test_chain_case():
    case = R.chain_case(257, seed=7)
    assert case.x.shape == (3, 257, 3) and case.x.dtype == np.float32
    assert 0.35 < 1.0 - case.mask[0].mean() < 0.55 and np.isnan(case.x[0][~case.mask[0]]).all()
    assert not np.isnan(case.x[0][case.mask[0]]).any()
    assert not case.mask[1].any() and np.isnan(case.x[1]).all() and case.mask[2].all() and not np.isnan(case.x[2]).any()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 and Q = 0 launch nothing."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)

    def call(points=fake, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None, k=8, cutoff=math.inf,
             include_self=0, idx=fake, dist=fake, count=fake, B=0, M=8, Q=8):
        return lib.ps_nearest_neighbors_f32(points, mask, queries, query_mask, exclude, query_exclude, k, cutoff, include_self,
                                            idx, dist, count, B, M, Q, None)

    assert call() == 0 and call(mask=fake, exclude=fake, include_self=1) == 0 and call(B=1, M=0, Q=0) == 0
    assert call(queries=fake, Q=3) == 0 and call(queries=fake, query_mask=fake, exclude=fake, query_exclude=fake, Q=3) == 0
    assert call(queries=fake, B=4, Q=0) == 0
    for k in (0, 65, -1):
        assert call(k=k) == 1, k
    assert call(k=1) == 0 and call(k=64) == 0
    for cutoff in (math.nan, 0.0, -1.0, -math.inf):
        assert call(cutoff=cutoff) == 1, cutoff
    assert call(cutoff=1e-30) == 0 and call(cutoff=3.0e38) == 0
    for name in ("points", "idx", "dist", "count"):
        assert call(**{name: None}) == 1, name
    assert call(B=-1) == 1 and call(M=-1, Q=-1) == 1 and call(B=65536) == 1 and call(B=65535, M=0, Q=0) == 0
    assert call(M=2 ** 24 + 1, Q=2 ** 24 + 1) == 1 and call(M=2 ** 24, Q=2 ** 24) == 0
    assert call(queries=fake, Q=2 ** 24 + 1) == 1 and call(queries=fake, Q=-1) == 1
    # the self graph has the points' own count, mask and keys; cross queries take both keys or neither
    assert call(Q=3) == 1 and call(query_mask=fake) == 1 and call(query_exclude=fake) == 1
    assert call(queries=fake, exclude=fake) == 1 and call(queries=fake, query_exclude=fake) == 1


# ---- ops -------------------------------------------------------------------------------------------------------------------
def knn_args(B=2, M=9, Q=4):
    g = torch.Generator().manual_seed(1)
    return torch.randn(B, M, 3, generator=g), torch.randn(B, Q, 3, generator=g)


def test_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_knn_shapes
    x, y = knn_args()
    mask, key = torch.ones(2, 9, dtype=torch.bool), torch.zeros(2, 9, dtype=torch.int32)
    qmask, qkey = torch.ones(2, 4, dtype=torch.bool), torch.zeros(2, 4, dtype=torch.int64)
    check(x, 1)
    check(x, 64, mask, None, None, key, None, 8.0, True)
    check(x.double(), np.int64(5), mask.float(), exclude=key.long(), cutoff=math.inf)
    check(x, 3, mask.to(torch.uint8), y, qmask, key, qkey, 1e-3)
    check(x, 3, queries=y.double())
    check(x, 3, queries=y[:, :0])
    for bad in (x[0], x[..., :2], x.long(), x[:, :, None]):
        with pytest.raises(ValueError):
            check(bad, 3)
    for bad in (0, 65, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="k must"):
            check(x, bad)
    for bad in (0.0, -1.0, -math.inf, math.nan):
        with pytest.raises(ValueError, match="cutoff"):
            check(x, 3, cutoff=bad)
    for bad in (mask[:, :8], mask[:1]):
        with pytest.raises(ValueError):
            check(x, 3, bad)
    for bad in (key[:, :8], key.float(), key.bool()):
        with pytest.raises(ValueError):
            check(x, 3, exclude=bad)
    for bad in (y[0], y[:1], y[..., :2], y.long()):
        with pytest.raises(ValueError, match="queries"):
            check(x, 3, queries=bad)
    for bad in (qmask[:, :3], mask):
        with pytest.raises(ValueError):
            check(x, 3, queries=y, query_mask=bad)
    for bad in (qkey[:, :3], qkey.float(), key):
        with pytest.raises(ValueError):
            check(x, 3, queries=y, exclude=key, query_exclude=bad)
    with pytest.raises(ValueError, match="come together"):
        check(x, 3, queries=y, exclude=key)
    with pytest.raises(ValueError, match="come together"):
        check(x, 3, queries=y, query_exclude=qkey)
    with pytest.raises(ValueError, match="needs queries"):
        check(x, 3, query_mask=mask)
    with pytest.raises(ValueError, match="needs queries"):
        check(x, 3, exclude=key, query_exclude=key)
    with pytest.raises(ValueError, match="include_self"):
        check(x, 3, queries=y, include_self=True)
    for name, moved in (("point_mask", mask), ("queries", y), ("query_mask", qmask), ("exclude", key), ("query_exclude", qkey)):
        kw = dict(point_mask=mask, queries=y, query_mask=qmask, exclude=key, query_exclude=qkey)
        kw[name] = moved.to("meta")
        with pytest.raises(ValueError):                                   # device disagreement
            check(x, 3, **kw)
    with pytest.raises(ValueError, match="65535"):
        check(torch.zeros(65536, 0, 3), 3)
    with pytest.raises(ValueError, match="2\\^24"):
        check(torch.zeros(1, 2 ** 24 + 1, 3, device="meta"), 3)
    with pytest.raises(ValueError, match="2\\^24"):
        check(torch.zeros(1, 4, 3, device="meta"), 3, queries=torch.zeros(1, 2 ** 24 + 1, 3, device="meta"))


def test_ops_validate_first_then_refuse_cpu_tensors():
    from protstruc_amd import ops
    x, y = knn_args()
    with pytest.raises(ValueError):
        ops.nearest_neighbors(x, 0)
    with pytest.raises(ValueError):
        ops.nearest_neighbors(x, 3, torch.ones(2, 8))
    with pytest.raises(ValueError):
        ops.nearest_neighbors(x, 3, cutoff=0.0)
    with pytest.raises(TypeError):
        ops.nearest_neighbors(x, 3, None, y)                              # everything past point_mask goes by keyword
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.nearest_neighbors(x, 3)


def test_signatures_of_the_three_layers():
    from protstruc_amd import StructureBatch, geometry, ops
    names = ["points", "k", "point_mask", "queries", "query_mask", "exclude", "query_exclude", "cutoff", "include_self"]
    for fn in (ops.nearest_neighbors, geometry.nearest_neighbors):
        p = inspect.signature(fn).parameters
        assert list(p) == names
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[3:])
        assert [p[k].default for k in names[2:]] == [None, None, None, None, None, math.inf, False]
        assert p["k"].default is inspect.Parameter.empty
    p = inspect.signature(ops.check_knn_shapes).parameters
    assert list(p) == names and [p[k].default for k in names[2:]] == [None, None, None, None, None, math.inf, False]
    assert geometry.Neighbors._fields == ("idx", "dist", "count")
    doc = geometry.nearest_neighbors.__doc__
    assert "not differentiable" in doc.lower() and "gather_neighbors" in doc
    p = inspect.signature(geometry.gather_neighbors).parameters
    assert list(p) == ["values", "idx", "fill"] and p["fill"].default == 0
    p = inspect.signature(StructureBatch.knn_graph).parameters
    assert list(p) == ["self", "k", "atom", "cutoff", "include_self", "other_chains_only"]
    assert [p[k].default for k in list(p)[1:]] == [30, "CA", None, False, False]
    p = inspect.signature(StructureBatch.atom_knn_graph).parameters
    assert list(p) == ["self", "k", "atoms", "cutoff", "exclude_same_residue"]
    assert [p[k].default for k in list(p)[1:]] == [32, "all", None, True]
    doc = StructureBatch.atom_knn_graph.__doc__
    assert "idx // A" in doc and "idx % A" in doc
    assert list(inspect.signature(StructureBatch.get_topk_nearest_residue_mask).parameters)[:3] == ["self", "query_xyz", "k"]


# ---- StructureBatch ----------------------------------------------------------------------------------------------------------
def test_structure_batch_hands_over_masks_keys_and_views(monkeypatch):
    """What ``knn_graph`` and ``atom_knn_graph`` hand to ``geometry.nearest_neighbors`` (host-only: the function is a
    recorder), on a file with two chains and UNK gap residues, batched with a shorter file so that there is padding."""
    from protstruc_amd import StructureBatch, geometry
    calls = []

    def recorder(points, k, point_mask=None, *, queries=None, query_mask=None, exclude=None, query_exclude=None,
                 cutoff=math.inf, include_self=False):
        calls.append(dict(points=points, k=k, point_mask=point_mask, queries=queries, query_mask=query_mask, exclude=exclude,
                          query_exclude=query_exclude, cutoff=cutoff, include_self=include_self))
        B, M = points.shape[:2]
        return geometry.Neighbors(torch.full((B, M, k), -1, dtype=torch.int32), torch.full((B, M, k), math.inf),
                                  torch.zeros(B, M, dtype=torch.int32))

    monkeypatch.setattr(geometry, "nearest_neighbors", recorder)
    batch = StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, "5cjx_HL.pdb"), os.path.join(GOLDEN_DIR, "1REX.pdb")],
                                    device="cpu")
    xyz = batch.get_xyz()
    B, N, A = xyz.shape[:3]
    assert (B, N, A) == (2, 448, 15) and not batch.residue_mask[1].all()
    present = batch.get_atom_mask() & batch.residue_mask[:, :, None]

    out = batch.knn_graph()
    assert isinstance(out, geometry.Neighbors) and tuple(out.idx.shape) == (B, N, 30)
    call = calls[-1]
    assert torch.equal(torch.nan_to_num(call["points"]), torch.nan_to_num(xyz[:, :, 1])) and tuple(call["points"].shape) == (B, N, 3)
    assert call["points"].data_ptr() == xyz[:, :, 1].data_ptr()                              # a strided view, no gather
    assert torch.equal(call["point_mask"], present[:, :, 1])
    assert (call["k"], call["cutoff"], call["include_self"]) == (30, math.inf, False)
    assert all(call[name] is None for name in ("queries", "query_mask", "exclude", "query_exclude"))

    batch.knn_graph(k=48, atom="CB", cutoff=10.0, include_self=True, other_chains_only=True)
    call = calls[-1]
    assert call["points"].data_ptr() == xyz[:, :, 4].data_ptr() and torch.equal(call["point_mask"], present[:, :, 4])
    assert not torch.equal(present[:, :, 4], present[:, :, 1])                               # glycines have no CB
    assert (call["k"], call["cutoff"], call["include_self"]) == (48, 10.0, True)
    key = call["exclude"]
    assert key.dtype == torch.int32 and tuple(key.shape) == (B, N)
    assert set(key[0].unique().tolist()) == {0, 1} and set(key[1].unique().tolist()) == {-1, 0}   # the padding's NaN is -1
    assert torch.equal(key[batch.residue_mask].double(), batch.chain_idx[batch.residue_mask].double())
    assert call["query_exclude"] is None and call["queries"] is None
    with pytest.raises(ValueError):
        batch.knn_graph(atom="XX")

    out = batch.atom_knn_graph()
    assert tuple(out.idx.shape) == (B, N * A, 32)
    call = calls[-1]
    assert call["points"].data_ptr() == xyz.data_ptr() and tuple(call["points"].shape) == (B, N * A, 3)   # a view
    assert torch.equal(call["point_mask"], present.reshape(B, N * A))
    assert torch.equal(call["exclude"], torch.arange(N, dtype=torch.int32).repeat_interleave(A).expand(B, N * A))
    assert (call["k"], call["cutoff"], call["include_self"]) == (32, math.inf, False)

    batch.atom_knn_graph(k=8, atoms=("CA", "CB"), cutoff=6.0, exclude_same_residue=False)
    call = calls[-1]
    chosen = torch.zeros(A, dtype=torch.bool)
    chosen[[1, 4]] = True
    assert torch.equal(call["point_mask"], (present & chosen).reshape(B, N * A))
    assert call["exclude"] is None and (call["k"], call["cutoff"]) == (8, 6.0)
    # neither a sequence nor radii are needed
    StructureBatch.from_xyz(xyz, device="cpu").atom_knn_graph(k=4)
    assert calls[-1]["point_mask"].all() and tuple(calls[-1]["points"].shape) == (B, N * A, 3)


# ---- gather_neighbors --------------------------------------------------------------------------------------------------------
def test_gather_neighbors_values_fill_and_gradient():
    from protstruc_amd import geometry
    g = torch.Generator().manual_seed(2)
    values = torch.randn(2, 5, 3, generator=g, dtype=torch.float64)
    idx = torch.tensor([[[1, 4, -1], [0, -1, -1], [2, 2, 3], [-1, -1, -1]],
                        [[4, 3, 2], [1, 0, -1], [0, 0, 0], [3, -1, -1]]], dtype=torch.int32)
    out = geometry.gather_neighbors(values, idx)
    assert tuple(out.shape) == (2, 4, 3, 3) and out.dtype == torch.float64
    for b in range(2):
        for q in range(4):
            for s in range(3):
                j = int(idx[b, q, s])
                assert torch.equal(out[b, q, s], values[b, j] if j >= 0 else torch.zeros(3, dtype=torch.float64))
    filled = geometry.gather_neighbors(values, idx, fill=-7.5)
    assert (filled[idx < 0] == -7.5).all() and torch.equal(filled[idx >= 0], out[idx >= 0])
    # any trailing shape, none included; int64 indices
    scalars = geometry.gather_neighbors(values[..., 0], idx.long(), fill=9.0)
    assert tuple(scalars.shape) == (2, 4, 3) and torch.equal(scalars, filled[..., 0].masked_fill(idx < 0, 9.0))
    wide = geometry.gather_neighbors(values[:, :, None, :].expand(2, 5, 2, 3), idx)
    assert tuple(wide.shape) == (2, 4, 3, 2, 3) and torch.equal(wide[:, :, :, 1], out)
    labels = geometry.gather_neighbors(torch.arange(10).reshape(2, 5), idx, fill=-1)
    assert labels.dtype == torch.int64 and labels[0, 0].tolist() == [1, 4, -1] and labels[1, 0].tolist() == [9, 8, 7]
    empty = geometry.gather_neighbors(values[:, :0], torch.full((2, 4, 3), -1, dtype=torch.int32), fill=2.0)
    assert tuple(empty.shape) == (2, 4, 3, 3) and (empty == 2.0).all()
    with pytest.raises(ValueError):
        geometry.gather_neighbors(values, idx[0])
    with pytest.raises(ValueError):
        geometry.gather_neighbors(values[:1], idx)
    v = values.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: geometry.gather_neighbors(t, idx), (v,))
    geometry.gather_neighbors(v, idx).sum().backward()
    counts = torch.zeros(2, 5, dtype=torch.float64)
    for b in range(2):
        for j in idx[b][idx[b] >= 0].tolist():
            counts[b, j] += 1
    assert torch.equal(v.grad, counts[:, :, None].expand(2, 5, 3))                         # the padding takes no gradient


# ---- the timing tool -------------------------------------------------------------------------------------------------------
def test_the_timing_tool_composes_the_same_definition():
    """tools/knn_time.py's composed route (cdist, masking, topk; float32), run on the CPU here, finds the yardstick's
    neighbours in every row whose distances -- the first one dropped included -- lie at least 1e-3 A apart, which float32
    (cdist through a matrix product errs by about 1e-4 A at these coordinates) cannot reorder: what the tool times is
    the definition, not something cheaper."""
    from tools import knn_time
    case = R.chain_case(65, seed=11)
    key = np.broadcast_to(np.arange(65, dtype=np.int32) // 4, (3, 65)).copy()
    for k, keys in ((16, None), (63, key)):
        wider = R.batch(case.x, k + 1, case.mask, exclude=keys)
        refs = [R.first(ref, k) for ref in wider]
        idx, dist, count = knn_time.composed(torch.from_numpy(case.x), k, torch.from_numpy(case.mask),
                                             None if keys is None else torch.from_numpy(keys))
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and count.dtype == torch.int32
        settled = 0
        for b, (ref, wide) in enumerate(zip(refs, wider)):
            assert np.array_equal(count[b].numpy(), ref.count), b
            for q in range(65):
                d = wide.dist[q, :wide.count[q]].astype(np.float64)
                if d.size > 1 and np.diff(d).min() < 1e-3:
                    continue
                settled += int(d.size > 0)
                assert np.array_equal(idx[b, q].numpy(), ref.idx[q]), (b, q)
                inside = np.arange(k) < ref.count[q]
                assert np.allclose(dist[b, q].numpy()[inside], ref.dist[q][inside], rtol=0, atol=1e-3)
        assert settled >= 50, settled
    assert (knn_time.B, knn_time.N, knn_time.A) == (128, 512, 15)
    assert knn_time.SHAPES == {"residues_k48": 48, "residues_k30": 30, "atoms_k64": 64}
    assert set(knn_time.STEPS) == set(knn_time.STEP_TIMEOUT_S) == {"events", "torch"}
