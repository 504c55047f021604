"""GPU tests of the nearest-neighbour kernel (ps_nearest_neighbors_f32; ops.nearest_neighbors;
geometry.nearest_neighbors, .gather_neighbors; StructureBatch.knn_graph, .atom_knn_graph).

Yardstick: tests/knn_ref.py, the definition in float64 in the kernel's own order of operations on the same float32 inputs.
The criterion is EQUALITY throughout: ``idx`` and ``count`` equal the yardstick's, ``dist`` is bitwise equal (compared as
int32), the padding is exactly -1 / +inf.  Every case runs twice -- through the public function and through the C ABI
into outputs carved out of sentinel-filled buffers at a start that is no 16-byte boundary -- and the two results must agree
bit for bit, which is also the determinism check; no sentinel may change.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import knn_ref as R
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000
PDB_FILES = ("1REX", "4EOT", "1ad0_DC", "5cjx_HL")
# the lane end (1, 2), the 64-owner boundary (63, 64, 65), the 256-item staging boundary (255, 256, 257: two tiles; 513:
# three)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)
KS = (1, 2, 16, 17, 32, 33, 48, 64)          # each bucket's edge: 16 | 17, 32 | 33, and the cap
PAIRS = sorted({(257, k) for k in KS} | {(M, 17) for M in SIZES}
               | {(1, 1), (2, 2), (63, 64), (64, 1), (65, 32), (255, 33), (256, 16), (513, 48), (513, 64)})


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def in_sentinels(pkg, x, k, mask=None, queries=None, query_mask=None, exclude=None, query_exclude=None, cutoff=math.inf,
                 include_self=False):
    """One call through the C ABI with idx, dist and count carved out of buffers of sentinels, 4 to 16 bytes past a
    16-byte boundary: (idx, dist, count), after checking that nothing around them was written."""
    lib = pkg._lib.load()
    B, M = x.shape[:2]
    Q = M if queries is None else queries.shape[1]
    front, back = 1 + (M + k) % 4, 9
    bufs = [torch.full((front + n + back,), 777, dtype=dt, device="cuda")
            for n, dt in ((B * Q * k, torch.int32), (B * Q * k, torch.float32), (B * Q, torch.int32))]
    outs = [buf[front:buf.numel() - back] for buf in bufs]
    u8 = lambda t: None if t is None else t.to(torch.uint8).contiguous()       # noqa: E731
    i32 = lambda t: None if t is None else t.to(torch.int32).contiguous()      # noqa: E731
    keep = [x.float().contiguous(), u8(mask), None if queries is None else queries.float().contiguous(), u8(query_mask),
            i32(exclude), i32(query_exclude)]
    ptr = lambda t: None if t is None else t.data_ptr()                         # noqa: E731
    rc = lib.ps_nearest_neighbors_f32(*(ptr(t) for t in keep), k, float(cutoff), int(include_self),
                                      *(ptr(t) for t in outs), B, M, Q, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for buf in bufs:
        assert (buf[:front] == 777).all() and (buf[buf.numel() - back:] == 777).all(), "a sentinel around an output changed"
    return outs[0].reshape(B, Q, k), outs[1].reshape(B, Q, k), outs[2].reshape(B, Q)


def run(pkg, x, k, mask=None, **kw):
    """numpy in; the public function and the C ABI inside sentinels, bitwise equal; the public function's result"""
    args = {name: dev(t) if isinstance(t, np.ndarray) else t for name, t in kw.items()}
    got = pkg.geometry.nearest_neighbors(dev(x), k, dev(mask), **args)
    assert isinstance(got, pkg.geometry.Neighbors)
    assert not any(t.requires_grad for t in got) and all(t.is_cuda for t in got)
    raw = in_sentinels(pkg, dev(x), k, dev(mask), **args)
    for a, b in zip(got, raw):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two launches differ"
    return got


def assert_equal_to_yardstick(got, refs, what):
    """(idx, dist, count) against the yardstick's, structure by structure: equal, bitwise, with exact padding"""
    idx, dist, count = (t.cpu().numpy() for t in got)
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and count.dtype == np.int32
    k = idx.shape[2]
    for b, ref in enumerate(refs):
        assert ref.idx.shape == idx[b].shape, (what, b)
        assert np.array_equal(count[b], ref.count), (what, b, np.flatnonzero(count[b] != ref.count)[:8])
        rows = np.flatnonzero((idx[b] != ref.idx).any(-1))
        assert rows.size == 0, (what, b, rows[:8], idx[b][rows[:1]], ref.idx[rows[:1]])
        assert np.array_equal(dist[b].view(np.int32), ref.dist.view(np.int32)), (what, b)
        pad = np.arange(k)[None, :] >= count[b][:, None]
        assert (idx[b][pad] == -1).all() and (dist[b][pad].view(np.int32) == INF_BITS).all(), (what, b)
        assert (idx[b][~pad] >= 0).all() and np.isfinite(dist[b][~pad]).all(), (what, b)


@functools.lru_cache(maxsize=None)
def chain(M):
    """the three-structure chain case of M points and its yardstick at k = 64, which holds every smaller k"""
    case = R.chain_case(M, seed=7)
    return case, R.batch(case.x, 64, case.mask)


# ---- synthetic chains --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,k", PAIRS)
def test_chains_equal_the_yardstick(pkg, M, k):
    case, refs64 = chain(M)
    refs = [R.first(ref, k) for ref in refs64]
    assert not case.mask[1].any() and np.isnan(case.x[1]).all() and case.mask[2].all()
    if M > 8:
        assert 0.3 < 1.0 - case.mask[0].mean() < 0.6 and np.isnan(case.x[0][~case.mask[0]]).all()
    got = run(pkg, case.x, k, case.mask)
    assert_equal_to_yardstick(got, refs, f"M = {M}, k = {k}")
    assert not got.count[1].any() and not got.count[0][~dev(case.mask)[0]].any()      # masked queries: no neighbours
    if k >= M:
        assert (got.count[2] == M - 1).all()                                             # k >= the candidates: padded
    # without a mask the NaN points are nobody's neighbours and have none: the same lists, with no special case
    bare = run(pkg, case.x, k)
    assert_equal_to_yardstick(bare, R.batch(case.x, k), f"M = {M}, k = {k}, no mask")
    assert torch.equal(bare.idx, got.idx) and torch.equal(bare.count, got.count)


# ---- ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (7, 27))
@pytest.mark.parametrize("reverse", (False, True))
def test_lattice_ties_go_to_the_lower_index(pkg, k, reverse):
    """The 6 x 6 x 6 integer lattice: most rows have exactly equal distances across the k boundary (asserted in
    test_knn_host.py), so only the index decides; with the points in reverse order "the lower index" is not "the first
    met in space"."""
    x = R.lattice()[::-1].copy() if reverse else R.lattice()
    ref = R.knn(x, k)
    assert R.boundary_ties(ref, k) == {7: 208, 27: 192}[k]
    assert_equal_to_yardstick(run(pkg, x[None], k), [ref], f"lattice k = {k} reverse = {reverse}")


def test_coincident_points_order_by_index(pkg):
    x = np.full((1, 216, 3), 1.5, dtype=np.float32)
    got = run(pkg, x, 5)
    assert_equal_to_yardstick(got, R.batch(x, 5), "coincident")
    want = np.array([[j for j in range(6) if j != q][:5] for q in range(216)], dtype=np.int32)
    assert np.array_equal(got.idx[0].cpu().numpy(), want) and not got.dist.any() and (got.count == 5).all()


# ---- cutoff, keys, include_self ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff,k", ((6.0, 17), (10.0, 64)))
def test_cutoff(pkg, cutoff, k):
    case, _ = chain(257)
    refs = R.batch(case.x, k, case.mask, cutoff=cutoff)
    counts = refs[2].count
    assert counts.min() < k and counts.max() == k and len(np.unique(counts)) > 10     # rows below k and full rows
    got = run(pkg, case.x, k, case.mask, cutoff=cutoff)
    assert_equal_to_yardstick(got, refs, f"cutoff {cutoff}")
    assert float(got.dist[torch.isfinite(got.dist)].max()) <= cutoff


def test_residue_keys_on_an_atom_cloud(pkg):
    """20 residues of 15 atoms: with the residue index as the key no atom finds an atom of its own residue"""
    centres = R.cloud(20, seed=1, spread=6.0)
    x = (np.repeat(centres, 15, axis=0) + R.cloud(300, seed=2, spread=1.2))[None]
    key = (np.arange(300, dtype=np.int32) // 15)[None]
    mask = (np.random.default_rng(3).random((1, 300)) > 0.2)
    refs = R.batch(x, 32, mask, exclude=key)
    assert (R.batch(x, 32, mask)[0].idx != refs[0].idx).any()                            # the key changes the answer
    got = run(pkg, x, 32, mask, exclude=key)
    assert_equal_to_yardstick(got, refs, "residue keys")
    idx = got.idx[0].cpu().numpy()
    assert (idx[idx >= 0] // 15 != np.broadcast_to(np.arange(300)[:, None] // 15, idx.shape)[idx >= 0]).all()
    # int64 keys are converted
    again = pkg.geometry.nearest_neighbors(dev(x), 32, dev(mask), exclude=dev(key).long())
    assert torch.equal(again.idx, got.idx)


def test_chain_keys_leave_the_other_chain_only(pkg):
    case, _ = chain(257)
    key = np.broadcast_to((np.arange(257) >= 120).astype(np.int32), (3, 257)).copy()
    refs = R.batch(case.x, 33, case.mask, exclude=key)
    got = run(pkg, case.x, 33, case.mask, exclude=key)
    assert_equal_to_yardstick(got, refs, "chain keys")
    idx = got.idx[2].cpu().numpy()
    assert (idx[:120] >= 120).all() and (idx[120:] < 120).all()


def test_include_self(pkg):
    case, _ = chain(65)
    refs = R.batch(case.x, 16, case.mask, include_self=True)
    got = run(pkg, case.x, 16, case.mask, include_self=True)
    assert_equal_to_yardstick(got, refs, "include_self")
    ok = dev(case.mask)
    own = torch.arange(65, device="cuda", dtype=torch.int32).expand(3, 65)
    assert torch.equal(got.idx[:, :, 0][ok], own[ok]) and not got.dist[:, :, 0][ok].any()
    without = run(pkg, case.x, 16, case.mask)
    assert torch.equal(without.idx[:, :, :15][ok], got.idx[:, :, 1:][ok])


# ---- cross queries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", (1, 65, 300))
def test_cross_queries_with_masks_and_keys(pkg, Q):
    case, _ = chain(257)
    rng = np.random.default_rng(Q)
    centre = np.nanmean(case.x[2], axis=0)
    queries = (centre + rng.normal(size=(3, Q, 3)) * 10.0).astype(np.float32)
    query_mask = rng.random((3, Q)) > 0.25 if Q > 1 else np.ones((3, 1), dtype=bool)
    queries[0][~query_mask[0]] = np.nan                                                  # NaN under the query mask
    key = np.broadcast_to(np.arange(257, dtype=np.int32) // 15, (3, 257)).copy()
    query_key = rng.integers(0, 18, size=(3, Q)).astype(np.int32)
    for k, keys in ((17, {}), (48, dict(exclude=key, query_exclude=query_key))):
        refs = R.batch(case.x, k, case.mask, queries, query_mask, **keys)
        got = run(pkg, case.x, k, case.mask, queries=queries, query_mask=query_mask, **keys)
        assert tuple(got.idx.shape) == (3, Q, k)
        assert_equal_to_yardstick(got, refs, f"Q = {Q}, k = {k}")
    bare = run(pkg, case.x[2:], 17, queries=queries[2:])                                  # no mask on either side
    assert_equal_to_yardstick(bare, R.batch(case.x[2:], 17, queries=queries[2:]), f"Q = {Q}, no masks")


# ---- layout, special values ------------------------------------------------------------------------------------------------------
def test_strided_points(pkg):
    case, refs64 = chain(257)
    big = torch.full((3, 257, 2, 5), 99.0, device="cuda")
    big[:, :, 1, 1:4] = dev(case.x)
    view = big[:, :, 1, 1:4]
    assert not view.is_contiguous()
    got = pkg.geometry.nearest_neighbors(view, 17, dev(case.mask))
    assert_equal_to_yardstick(got, [R.first(ref, 17) for ref in refs64], "strided")
    # float64 coordinates are rounded to float32 first, as everywhere in this package
    wide = pkg.geometry.nearest_neighbors(dev(case.x).double(), 17, dev(case.mask))
    assert torch.equal(wide.idx, got.idx) and torch.equal(wide.dist.view(torch.int32), got.dist.view(torch.int32))


def test_unmasked_nan_and_infinite_points(pkg):
    x = chain(65)[0].x[2:].copy()
    x[0, 5] = np.nan
    x[0, 9, 1] = np.inf
    x[0, 40, 2] = -np.inf
    refs = R.batch(x, 16)
    assert not refs[0].count[[5, 9, 40]].any() and not np.isin(refs[0].idx, (5, 9, 40)).any() and refs[0].count[0] == 16
    assert_equal_to_yardstick(run(pkg, x, 16), refs, "NaN and inf")
    assert_equal_to_yardstick(run(pkg, x, 64, cutoff=9.0), R.batch(x, 64, cutoff=9.0), "NaN and inf, cutoff")


# ---- the PDB files ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pdb_batch():
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, name + ".pdb") for name in PDB_FILES])


def assert_within_cdist(got, x, mask, key=None, tol=1e-5):
    """The second witness: the returned distances against the k smallest of ``torch.cdist`` in float64 on the GPU, which
    does not depend on any index."""
    d = torch.cdist(x.double(), x.double())
    ok = mask[:, :, None] & mask[:, None, :] & ~torch.eye(x.shape[1], dtype=torch.bool, device=x.device)
    if key is not None:
        ok &= key[:, :, None] != key[:, None, :]
    d = torch.where(ok, d, torch.full_like(d, math.inf))
    k = got.idx.shape[2]
    want = torch.topk(d, min(k, d.shape[2]), dim=2, largest=False).values
    if want.shape[2] < k:
        want = torch.nn.functional.pad(want, (0, k - want.shape[2]), value=math.inf)
    assert torch.equal(torch.isfinite(want), got.idx >= 0)
    real = got.idx >= 0
    assert float((got.dist.double() - want)[real].abs().max()) <= tol


@pytest.mark.parametrize("k", (30, 48))
def test_pdb_residue_graphs(pkg, k):
    batch = pdb_batch()
    ca = batch.get_xyz()[:, :, 1].contiguous()
    present = batch._present_atoms()[:, :, 1]
    got = batch.knn_graph(k=k)
    refs = R.batch(ca.cpu().numpy(), k, present.cpu().numpy())
    assert_equal_to_yardstick(got, refs, f"knn_graph k = {k}")
    assert tuple(got.idx.shape) == (4, ca.shape[1], k) and int(got.count.max()) == k
    assert_within_cdist(got, ca, present)
    for b in range(4):                                                                   # padded residues: nothing
        assert not got.count[b][~batch.residue_mask[b]].any()


def test_pdb_interface_graphs(pkg):
    batch = pdb_batch()
    ca = batch.get_xyz()[:, :, 1].contiguous()
    present = batch._present_atoms()[:, :, 1]
    key = torch.nan_to_num(batch.chain_idx.float(), nan=-1.0).to(torch.int32)
    got = batch.knn_graph(k=30, other_chains_only=True, cutoff=12.0)
    refs = R.batch(ca.cpu().numpy(), 30, present.cpu().numpy(), exclude=key.cpu().numpy(), cutoff=12.0)
    assert_equal_to_yardstick(got, refs, "other_chains_only")
    two_chains = [b for b in range(4) if len(batch.get_chain_ids()[b]) == 2]
    assert len(two_chains) >= 2
    for b in range(4):
        assert bool(got.count[b].any()) == (b in two_chains)                             # one chain: no interface
    free = batch.knn_graph(k=30, other_chains_only=True)
    assert_equal_to_yardstick(free, R.batch(ca.cpu().numpy(), 30, present.cpu().numpy(), exclude=key.cpu().numpy()),
                              "other_chains_only, no cutoff")
    assert_within_cdist(free, ca, present, key)


def test_pdb_atom_graph(pkg):
    from protstruc_amd import StructureBatch
    batch = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "1REX.pdb"))
    B, N, A = batch.get_xyz().shape[:3]
    x = batch.get_xyz().reshape(B, N * A, 3)
    present = batch._present_atoms().reshape(B, N * A)
    key = torch.arange(N, dtype=torch.int32, device="cuda").repeat_interleave(A).expand(B, N * A)
    got = batch.atom_knn_graph(k=64)
    refs = R.batch(x.cpu().numpy(), 64, present.cpu().numpy(), exclude=key.cpu().numpy())
    assert_equal_to_yardstick(got, refs, "atom_knn_graph")
    idx = got.idx[0]
    own = torch.arange(N * A, device="cuda")[:, None].expand_as(idx) // A
    assert (idx[idx >= 0] // A != own[idx >= 0]).all()
    assert_within_cdist(got, x, present, key)
    backbone = batch.atom_knn_graph(k=8, atoms=("N", "CA", "C", "O"), cutoff=5.0, exclude_same_residue=False)
    chosen = torch.zeros(A, dtype=torch.bool, device="cuda")
    chosen[:4] = True
    picked = (batch._present_atoms() & chosen).reshape(B, N * A)
    assert_equal_to_yardstick(backbone, R.batch(x.cpu().numpy(), 8, picked.cpu().numpy(), cutoff=5.0), "backbone atoms")


# ---- the layers above ------------------------------------------------------------------------------------------------------------
def test_ops_with_nothing_to_do_launch_nothing(pkg, monkeypatch):
    ops = pkg.ops

    def no_launch(*args):
        raise AssertionError("an empty call launched a kernel")

    monkeypatch.setattr(ops, "_launch", no_launch)
    for B, M, Q in ((0, 5, None), (2, 0, None), (2, 0, 5), (2, 5, 0), (0, 0, 0)):
        x = torch.zeros(B, M, 3, device="cuda")
        queries = None if Q is None else torch.zeros(B, Q, 3, device="cuda")
        idx, dist, count = ops.nearest_neighbors(x, 7, queries=queries)
        rows = M if Q is None else Q
        assert tuple(idx.shape) == tuple(dist.shape) == (B, rows, 7) and tuple(count.shape) == (B, rows)
        assert (idx.dtype, dist.dtype, count.dtype) == (torch.int32, torch.float32, torch.int32) and idx.is_cuda
        assert (idx == -1).all() and (dist.view(torch.int32) == INF_BITS).all() and not count.any()


def test_geometry_takes_cpu_tensors_and_arrays(pkg):
    case, refs64 = chain(65)
    refs = [R.first(ref, 16) for ref in refs64]
    got = pkg.geometry.nearest_neighbors(torch.from_numpy(case.x), 16, torch.from_numpy(case.mask))
    assert all(isinstance(t, torch.Tensor) and t.device.type == "cpu" for t in got)
    assert_equal_to_yardstick(got, refs, "CPU tensors")
    arrays = pkg.geometry.nearest_neighbors(case.x, 16, case.mask)
    assert all(isinstance(t, np.ndarray) for t in arrays)
    assert np.array_equal(arrays.idx, got.idx.numpy()) and np.array_equal(arrays.count, got.count.numpy())
    x = torch.from_numpy(case.x).cuda().requires_grad_(True)
    assert not any(t.requires_grad for t in pkg.geometry.nearest_neighbors(x, 16, dev(case.mask)))


def test_edges_rebuilt_by_gather_are_the_distances(pkg):
    """The recipe of the docstring: differentiable edge lengths from the indices equal ``dist`` to float32 rounding (a
    difference of two coordinates below 64 A and a norm below 32 A: under 5e-6 A), and the gradient reaches the
    coordinates."""
    case, _ = chain(65)
    x = torch.nan_to_num(dev(case.x[2:])).requires_grad_(True)
    nb = pkg.geometry.nearest_neighbors(x, 16, cutoff=4.0)
    assert 0 < int(nb.count.min()) < 16                                                  # real edges and padding
    xj = pkg.geometry.gather_neighbors(x, nb.idx)
    edge = (xj - x[:, :, None]).norm(dim=-1).masked_fill(nb.idx < 0, 0.0)
    real = nb.idx >= 0
    assert float((edge.detach() - nb.dist)[real].abs().max()) <= 1e-5 and not edge[~real].any()
    edge.sum().backward()
    assert torch.isfinite(x.grad).all() and bool(x.grad.any())
