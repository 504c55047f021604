"""GPU tests of the edge-feature kernels (ps_edge_rbf_f32, ps_edge_frames_f32; ops.edge_rbf, ops.edge_frames;
geometry.edge_distance_features, .edge_frame_features; StructureBatch.edge_features).

Yardstick: tests/edge_ref.py, the definitions in float64 in the kernels' own order of operations on the same float32 inputs.
``dist``, ``local_pos`` and ``rel_rot`` must be BITWISE equal to it (compared as int32); ``rbf`` must lie within 1e-6 absolute
on every element -- the contract of include/protstruc_hip.h, above the 2e-7 the kernel's arithmetic owes by analysis --;
the zeros at the padding and at masked pairs must be exact.  Every case runs twice -- through the public function and through
the C ABI into outputs carved out of sentinel-filled buffers 4 to 12 bytes past a 16-byte boundary -- and the two results
must agree bit for bit, which is also the determinism check; no sentinel may change.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import edge_ref as E
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

RBF_TOL = 1e-6
PDB_FILES = ("1REX", "4EOT", "1ad0_DC", "5cjx_HL")
# (N, k, A, P, R): N at the lane end (1, 2), around a wave (63, 64, 65) and over one workgroup's 256 threads (257); k at both
# ends, a small odd one and the consumers' 30 and 48; rows of k*P*R floats that are no multiple of 4 (15 = 3 * 5, k odd) and
# that are (112 = 7 * 16), so that with the output 4 to 12 bytes off a 16-byte boundary the single floats before and after
# the 16-byte stores are exercised at every length; (64, 64) is the limit of both tables, (1, 1) a row of k floats
CASES = ((1, 1, 5, 1, 1), (2, 3, 5, 3, 5), (2, 1, 15, 7, 16), (63, 64, 5, 3, 5), (64, 1, 15, 25, 16), (65, 48, 5, 25, 16),
         (65, 3, 15, 7, 16), (257, 1, 5, 3, 5), (257, 3, 15, 3, 5), (257, 30, 5, 25, 16), (257, 48, 15, 25, 16),
         (257, 64, 5, 7, 16), (63, 30, 15, 1, 1), (9, 64, 15, 64, 64), (5, 3, 5, 64, 64))


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def tables(A, P, R, seed=0):
    """(pairs [(slot_i, slot_j)] * P, centers (R,) float32, sigma)"""
    from protstruc_amd import geometry
    if P == 25:
        pairs = list(geometry.BACKBONE_PAIRS)
    else:
        rng = np.random.default_rng(100 * P + A + seed)
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, A, size=(P, 2))]
    if R == 16:
        centers, sigma = geometry.rbf_centers()                      # 2 .. 22 A, sigma 1.25
    elif R == 64:
        centers, sigma = geometry.rbf_centers(64, 0.0, 32.0)         # sigma 0.5
    elif R > 1:
        centers, sigma = geometry.rbf_centers(R, 0.0, 8.0)           # R = 5: sigma 1.6
    else:
        centers, sigma = np.array([4.0], np.float32), 2.0
    return pairs, centers, sigma


def carve(shapes, front):
    """buffers of sentinels with the outputs ``front`` floats past their (at least 256-byte aligned) start"""
    back = 9
    bufs = [torch.full((front + int(np.prod(s)) + back,), 777.0, dtype=torch.float32, device="cuda") for s in shapes]
    assert all(b.data_ptr() % 16 == 0 for b in bufs) and 1 <= front <= 3
    return bufs, [b[front:b.numel() - back] for b in bufs], back


def sentinels_intact(bufs, front, back):
    for buf in bufs:
        assert (buf[:front] == 777.0).all() and (buf[buf.numel() - back:] == 777.0).all(), "a sentinel around an output changed"


def rbf_in_sentinels(pkg, xyz, idx, mask, pairs, centers, sigma, want_dist=True, want_rbf=True):
    import ctypes
    lib = pkg._lib.load()
    B, N, A = xyz.shape[:3]
    k, P, R = idx.shape[2], len(pairs), len(centers)
    front = 1 + (N + k) % 3
    bufs, (dist, rbf), back = carve(((B, N, k, P), (B, N, k, P * R)), front)
    keep = [xyz.float().contiguous(), None if mask is None else mask.to(torch.uint8).contiguous(), idx.to(torch.int32).contiguous()]
    ints = ctypes.c_int * P
    rc = lib.ps_edge_rbf_f32(keep[0].data_ptr(), None if keep[1] is None else keep[1].data_ptr(), keep[2].data_ptr(),
                             ints(*(p[0] for p in pairs)), ints(*(p[1] for p in pairs)), P,
                             (ctypes.c_float * R)(*np.asarray(centers, np.float32).tolist()), R, float(sigma),
                             dist.data_ptr() if want_dist else None, rbf.data_ptr() if want_rbf else None, B, N, A, k,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    sentinels_intact(bufs, front, back)
    for wanted, out in ((want_dist, dist), (want_rbf, rbf)):
        if not wanted:
            assert (out == 777.0).all(), "an output that was not asked for was written"
    return (dist.reshape(B, N, k, P) if want_dist else None), (rbf.reshape(B, N, k, P * R) if want_rbf else None)


def run_rbf(pkg, xyz, idx, mask, pairs, centers, sigma):
    """numpy in; the public function and the C ABI inside sentinels, bitwise equal; (dist, rbf) of the public function"""
    rbf, dist = pkg.geometry.edge_distance_features(dev(xyz), dev(idx), dev(mask), pairs=pairs, centers=centers, sigma=sigma,
                                                    return_dist=True)
    assert rbf.is_cuda and dist.is_cuda and not rbf.requires_grad and not dist.requires_grad
    raw_dist, raw_rbf = rbf_in_sentinels(pkg, dev(xyz), dev(idx), dev(mask), pairs, centers, sigma)
    assert dist.shape == raw_dist.shape and rbf.shape == raw_rbf.shape
    assert torch.equal(bits(dist), bits(raw_dist)) and torch.equal(bits(rbf), bits(raw_rbf)), "two launches differ"
    return dist, rbf


def assert_rbf_meets_the_yardstick(got, ref, what):
    dist, rbf = (t.cpu().numpy() for t in got)
    assert dist.dtype == np.float32 and rbf.dtype == np.float32
    assert dist.shape == ref.dist.shape and rbf.shape == ref.rbf.shape, what
    assert np.array_equal(dist.view(np.int32), ref.dist.view(np.int32)), (what, "dist differs in its bits")
    R = rbf.shape[-1] // dist.shape[-1]
    real = np.repeat(ref.real, R, axis=-1)
    assert not dist[~ref.real].view(np.int32).any() and not rbf[~real].view(np.int32).any(), (what, "zeros are not exact")
    worst = float(np.abs(rbf.astype(np.float64) - ref.rbf).max()) if rbf.size else 0.0
    print(f"{what}: max |rbf - float64| = {worst:.3e}")
    assert worst <= RBF_TOL, (what, worst)


@functools.lru_cache(maxsize=None)
def residues(N, A):
    return E.residue_case(N, A, seed=7)


def graph_of(pkg, case, k, cutoff=float("inf")):
    """the neighbour lists of slot 0, from the kernel under its own test (tests/test_gpu_knn.py): masked residues and
    residues with fewer than k neighbours are padded"""
    return pkg.geometry.nearest_neighbors(dev(case.xyz[:, :, 0]), k, dev(case.mask[:, :, 0]), cutoff=cutoff).idx.cpu().numpy()


# ---- synthetic chains --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k,A,P,R", CASES)
def test_rbf_on_chains_meets_the_yardstick(pkg, N, k, A, P, R):
    case = residues(N, A)
    assert not case.mask[1].any() and np.isnan(case.xyz[1]).all() and case.mask[2].all()
    if N > 8:
        assert 0.3 < 1.0 - case.mask[0].mean() < 0.6 and np.isnan(case.xyz[0][~case.mask[0]]).all()
    pairs, centers, sigma = tables(A, P, R)
    idx = graph_of(pkg, case, k)
    assert (idx[1] == -1).all() and (N == 1 or (idx[2] >= 0).any())
    ref = E.edge_rbf(case.xyz, idx, case.mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    got = run_rbf(pkg, case.xyz, idx, case.mask, pairs, centers, sigma)
    assert_rbf_meets_the_yardstick(got, ref, f"N={N} k={k} A={A} P={P} R={R}")
    if N > 8:
        assert ref.real[0].any() and not ref.real[0].all() and ref.real[2][idx[2] >= 0].all() and float(got[1].max()) > 0.5


def test_rbf_on_graphs_with_a_cutoff(pkg):
    """graphs of nearest_neighbors with a cutoff: many rows are partly or wholly padded"""
    case = residues(257, 5)
    pairs, centers, sigma = tables(5, 25, 16)
    for cutoff, k in ((3.0, 30), (6.0, 48)):
        idx = graph_of(pkg, case, k, cutoff)
        counts = (idx[2] >= 0).sum(-1)
        assert counts.min() < k and counts.max() > 0 and len(np.unique(counts)) > 3
        ref = E.edge_rbf(case.xyz, idx, case.mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
        assert_rbf_meets_the_yardstick(run_rbf(pkg, case.xyz, idx, case.mask, pairs, centers, sigma), ref, f"cutoff {cutoff}")


def test_any_index_outside_the_range_is_padding(pkg):
    """-1, -7, N and N + 5 among valid entries, and int64 values that would wrap into the range as int32"""
    case = residues(65, 15)
    N = 65
    idx = E.random_graph(3, N, 6, seed=4, padded=0.0)
    idx[:, ::2, 1], idx[:, 1::3, 2], idx[:, ::5, 4], idx[:, 3::4, 0] = -1, -7, N, N + 5
    idx[:, 7, 5] = 2 ** 31 - 1
    idx[:, 8, 5] = -2 ** 31
    pairs, centers, sigma = tables(15, 7, 16)
    ref = E.edge_rbf(case.xyz, idx, case.mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    assert not ref.real[:, ::2, 1].any() and not ref.real[:, ::5, 4].any() and ref.real[2, :, 3].all()
    got = run_rbf(pkg, case.xyz, idx, case.mask, pairs, centers, sigma)
    assert_rbf_meets_the_yardstick(got, ref, "hand-made idx")
    wide = idx.astype(np.int64)
    wide[:, 9, 5] = 2 ** 32 + 3                                                     # 3 as int32: still padding
    wide[:, 10, 5] = -2 ** 32 + 3
    ref64 = E.edge_rbf(case.xyz, wide, case.mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    assert not ref64.real[:, 9, 5].any() and not ref64.real[:, 10, 5].any()
    rbf, dist = pkg.geometry.edge_distance_features(dev(case.xyz), dev(wide), dev(case.mask), pairs=pairs, centers=centers,
                                                    sigma=sigma, return_dist=True)
    assert_rbf_meets_the_yardstick((dist, rbf), ref64, "int64 idx")


def test_each_rbf_output_alone(pkg):
    case = residues(65, 5)
    pairs, centers, sigma = tables(5, 3, 5)
    idx = graph_of(pkg, case, 3)
    both = run_rbf(pkg, case.xyz, idx, case.mask, pairs, centers, sigma)
    kw = dict(pair_i=[p[0] for p in pairs], pair_j=[p[1] for p in pairs], centers=centers, sigma=sigma)
    dist, none = pkg.ops.edge_rbf(dev(case.xyz), dev(idx), dev(case.mask), want_rbf=False, **kw)
    assert none is None and torch.equal(bits(dist), bits(both[0]))
    none, rbf = pkg.ops.edge_rbf(dev(case.xyz), dev(idx), dev(case.mask), want_dist=False, **kw)
    assert none is None and torch.equal(bits(rbf), bits(both[1]))
    raw = rbf_in_sentinels(pkg, dev(case.xyz), dev(idx), dev(case.mask), pairs, centers, sigma, want_rbf=False)
    assert raw[1] is None and torch.equal(bits(raw[0]), bits(both[0]))
    raw = rbf_in_sentinels(pkg, dev(case.xyz), dev(idx), dev(case.mask), pairs, centers, sigma, want_dist=False)
    assert raw[0] is None and torch.equal(bits(raw[1]), bits(both[1]))
    # the default of geometry: rbf alone, ProteinMPNN's pairs and centres; no mask: every atom
    full = case.xyz[2:]
    only = pkg.geometry.edge_distance_features(dev(full), dev(idx[2:]))
    assert tuple(only.shape) == (1, 65, 3, 400)
    pairs, centers, sigma = tables(5, 25, 16)
    ref = E.edge_rbf(full, idx[2:], None, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    assert float(np.abs(only.cpu().numpy() - ref.rbf).max()) <= RBF_TOL


def test_unmasked_nan_propagates_and_arrays_come_back_as_arrays(pkg):
    case = residues(65, 5)
    xyz = case.xyz[2:].copy()
    xyz[0, 5, 1] = np.nan
    pairs, centers, sigma = tables(5, 25, 16)
    idx = E.random_graph(1, 65, 3, seed=9)
    idx[0, 0, 0], idx[0, 5, 0] = 5, 6
    ref = E.edge_rbf(xyz, idx, None, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    assert np.isnan(ref.dist).any() and np.isnan(ref.dist[0, 0, 0]).sum() == 5 and np.isnan(ref.dist[0, 5, 0]).sum() == 5
    rbf, dist = pkg.geometry.edge_distance_features(xyz, idx, pairs=pairs, centers=centers, sigma=sigma, return_dist=True)
    assert isinstance(rbf, np.ndarray) and isinstance(dist, np.ndarray)
    assert np.array_equal(np.isnan(dist), np.isnan(ref.dist)) and np.array_equal(np.isnan(rbf), np.isnan(ref.rbf))
    fine = ~np.isnan(ref.dist)
    assert np.array_equal(dist[fine].view(np.int32), ref.dist[fine].view(np.int32))
    assert np.nanmax(np.abs(rbf - ref.rbf)) <= RBF_TOL
    # CPU tensors come back on the CPU
    out = pkg.geometry.edge_distance_features(torch.from_numpy(case.xyz), torch.from_numpy(idx).expand(3, 65, 3),
                                              torch.from_numpy(case.mask))
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and tuple(out.shape) == (3, 65, 3, 400)


# ---- frames ------------------------------------------------------------------------------------------------------------------
def frames_in_sentinels(pkg, rot, trans, idx, mask, want_pos=True, want_rot=True):
    lib = pkg._lib.load()
    B, N, k = idx.shape
    front = 1 + (N + k) % 3
    bufs, (pos, rel), back = carve(((B, N, k, 3), (B, N, k, 3, 3)), front)
    keep = [rot.float().contiguous(), trans.float().contiguous(), None if mask is None else mask.to(torch.uint8).contiguous(),
            idx.to(torch.int32).contiguous()]
    rc = lib.ps_edge_frames_f32(keep[0].data_ptr(), keep[1].data_ptr(), None if keep[2] is None else keep[2].data_ptr(),
                                keep[3].data_ptr(), pos.data_ptr() if want_pos else None, rel.data_ptr() if want_rot else None,
                                B, N, k, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    sentinels_intact(bufs, front, back)
    for wanted, out in ((want_pos, pos), (want_rot, rel)):
        if not wanted:
            assert (out == 777.0).all(), "an output that was not asked for was written"
    return (pos.reshape(B, N, k, 3) if want_pos else None), (rel.reshape(B, N, k, 3, 3) if want_rot else None)


def assert_frames_equal_the_yardstick(got, ref, what):
    pos, rel = (t.cpu().numpy() for t in got)
    assert pos.dtype == np.float32 and rel.dtype == np.float32
    assert pos.shape == ref.local_pos.shape and rel.shape == ref.rel_rot.shape, what
    assert np.array_equal(pos.view(np.int32), ref.local_pos.view(np.int32)), (what, "local_pos differs in its bits")
    assert np.array_equal(rel.view(np.int32), ref.rel_rot.view(np.int32)), (what, "rel_rot differs in its bits")
    assert not pos[~ref.real].view(np.int32).any() and not rel[~ref.real].view(np.int32).any(), (what, "zeros are not exact")


@pytest.mark.parametrize("N,k", ((1, 1), (2, 3), (63, 64), (64, 1), (65, 48), (257, 3), (257, 30), (257, 64)))
def test_frames_equal_the_yardstick(pkg, N, k):
    rot, trans = E.random_frames(3, N, seed=N + k)
    mask = np.random.default_rng(N).random((3, N)) >= 0.3
    mask[1], mask[2] = False, True
    rot[~mask], trans[~mask] = np.nan, np.nan                                        # NaN under the mask
    idx = E.random_graph(3, N, k, seed=k)
    idx[:, ::3, 0] = N + 5
    ref = E.edge_frames(rot, trans, idx, mask)
    assert not ref.real[1].any() and (N == 1 or ref.real[2].any())
    got = pkg.geometry.edge_frame_features(dev(rot), dev(trans), dev(idx), dev(mask))
    assert isinstance(got, pkg.geometry.EdgeFrames) and all(t.is_cuda and not t.requires_grad for t in got)
    raw = frames_in_sentinels(pkg, dev(rot), dev(trans), dev(idx), dev(mask))
    for a, b in zip(got, raw):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b)), "two launches differ"
    assert_frames_equal_the_yardstick(got, ref, f"N={N} k={k}")
    if N >= 63:
        # the complete structure without a mask: the same values, and rel_rot is a rotation
        bare = pkg.geometry.edge_frame_features(dev(rot[2:]), dev(trans[2:]), dev(idx[2:]))
        assert_frames_equal_the_yardstick(bare, E.edge_frames(rot[2:], trans[2:], idx[2:]), f"N={N} k={k}, no mask")
        rr = bare.rel_rot[bare.rel_rot.abs().sum((-1, -2)) > 0].double()
        assert float((rr @ rr.transpose(-1, -2) - torch.eye(3, device="cuda", dtype=torch.float64)).abs().max()) < 1e-5


def test_each_frame_output_alone(pkg):
    rot, trans = E.random_frames(2, 65, seed=1)
    idx = E.random_graph(2, 65, 5, seed=2)
    both = pkg.ops.edge_frames(dev(rot), dev(trans), dev(idx))
    pos, none = pkg.ops.edge_frames(dev(rot), dev(trans), dev(idx), want_rot=False)
    assert none is None and torch.equal(bits(pos), bits(both[0]))
    none, rel = pkg.ops.edge_frames(dev(rot), dev(trans), dev(idx), want_pos=False)
    assert none is None and torch.equal(bits(rel), bits(both[1]))
    raw = frames_in_sentinels(pkg, dev(rot), dev(trans), dev(idx), None, want_rot=False)
    assert raw[1] is None and torch.equal(bits(raw[0]), bits(both[0]))
    raw = frames_in_sentinels(pkg, dev(rot), dev(trans), dev(idx), None, want_pos=False)
    assert raw[0] is None and torch.equal(bits(raw[1]), bits(both[1]))
    arrays = pkg.geometry.edge_frame_features(rot, trans, idx)
    assert all(isinstance(t, np.ndarray) for t in arrays) and np.array_equal(arrays.local_pos, both[0].cpu().numpy())


def test_ops_with_nothing_to_do_launch_nothing(pkg, monkeypatch):
    ops = pkg.ops

    def no_launch(*args):
        raise AssertionError("an empty call launched a kernel")

    monkeypatch.setattr(ops, "_launch", no_launch)
    for B, N in ((0, 5), (2, 0), (0, 0)):
        idx = torch.zeros(B, N, 4, dtype=torch.int32, device="cuda")
        dist, rbf = ops.edge_rbf(torch.zeros(B, N, 5, 3, device="cuda"), idx, pair_i=[0, 1], pair_j=[1, 0], centers=[1.0, 2.0, 3.0],
                                 sigma=1.0)
        assert tuple(dist.shape) == (B, N, 4, 2) and tuple(rbf.shape) == (B, N, 4, 6) and dist.is_cuda
        pos, rel = ops.edge_frames(torch.zeros(B, N, 3, 3, device="cuda"), torch.zeros(B, N, 3, device="cuda"), idx)
        assert tuple(pos.shape) == (B, N, 4, 3) and tuple(rel.shape) == (B, N, 4, 3, 3)


# ---- the PDB files ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pdb_batch():
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, name + ".pdb") for name in PDB_FILES])


def pdb_reference(batch, idx, slots, n_rbf=16, d_min=2.0, d_max=22.0):
    from protstruc_amd import geometry
    centers, sigma = geometry.rbf_centers(n_rbf, d_min, d_max)
    pairs = [(a, b) for a in slots for b in slots]
    return E.edge_rbf(batch.get_xyz().cpu().numpy(), idx.cpu().numpy(), batch._present_atoms().cpu().numpy(),
                      [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)


def assert_pdb_rbf(ef, ref, what):
    rbf = ef.rbf.cpu().numpy()
    real = np.repeat(ref.real, rbf.shape[-1] // ref.real.shape[-1], axis=-1)
    assert rbf.shape == ref.rbf.shape and not rbf[~real].view(np.int32).any(), what
    worst = float(np.abs(rbf - ref.rbf).max())
    print(f"{what}: max |rbf - float64| = {worst:.3e}")
    assert worst <= RBF_TOL, (what, worst)


def test_pdb_edge_features(pkg):
    batch = pdb_batch()
    B, N = batch.get_xyz().shape[:2]
    ef = batch.edge_features()
    graph = batch.knn_graph(30)
    assert torch.equal(ef.idx, graph.idx) and ef.idx.dtype == torch.int32 and torch.equal(ef.mask, graph.idx >= 0)
    assert tuple(ef.rbf.shape) == (B, N, 30, 400) and not ef.rbf.requires_grad
    assert_pdb_rbf(ef, pdb_reference(batch, ef.idx, range(5)), "edge_features()")
    # every pair of a real edge between residues with all five atoms has its nearest centre above exp(-0.29) (centres 1.33 A
    # apart, sigma 1.25: z <= 0.534) while the distance is within 2 .. 22 A; the CA-CA pair of the nearest neighbour is
    peak = ef.rbf.reshape(B, N, 30, 25, 16)[:, :, 0, 6].max(-1).values
    assert float(peak[ef.mask[:, :, 0]].min()) > 0.74
    # the frames: bitwise the yardstick's on the frames the batch itself computes
    rot, trans = batch.backbone_orientations_and_translations()
    frame_mask = batch._present_atoms()[:, :, :3].all(-1)
    ref = E.edge_frames(rot.cpu().numpy(), trans.cpu().numpy(), ef.idx.cpu().numpy(), frame_mask.cpu().numpy())
    assert_frames_equal_the_yardstick((ef.local_pos, ef.rel_rot), ref, "edge_features() frames")
    assert ref.real.any() and torch.isfinite(ef.local_pos).all() and torch.isfinite(ef.rel_rot).all()
    # |local_pos| of the nearest neighbour is its CA-CA distance
    d = ef.local_pos[:, :, 0].norm(dim=-1)
    ok = dev(ref.real[:, :, 0])
    assert float((d - graph.dist[:, :, 0])[ok].abs().max()) < 1e-4
    # the offsets: 0 at the padding, 65 across chains, and -1 / +1 along a chain
    assert ef.offset.dtype == torch.int64 and not ef.offset[~ef.mask].any() and int(ef.offset.max()) == 65
    chain = batch._chain_keys()
    other = pkg.geometry.gather_neighbors(chain, ef.idx, fill=-2) != chain[:, :, None]
    assert torch.equal(ef.offset == 65, other & ef.mask)
    assert bool(((ef.offset == 31) | (ef.offset == 33))[ef.mask].any())


def test_pdb_edge_features_without_frames_and_on_a_users_graph(pkg):
    batch = pdb_batch()
    B, N = batch.get_xyz().shape[:2]
    ef = batch.edge_features(k=48, atoms=("CA", "CB", "N"), n_rbf=8, d_min=0.0, d_max=16.0, frames=False, max_offset=4)
    assert ef.local_pos is None and ef.rel_rot is None and tuple(ef.rbf.shape) == (B, N, 48, 9 * 8)
    assert torch.equal(ef.idx, batch.knn_graph(48).idx) and int(ef.offset.max()) == 9
    assert_pdb_rbf(ef, pdb_reference(batch, ef.idx, (1, 4, 0), 8, 0.0, 16.0), "frames=False")
    # a user's graph: the interface graph as Neighbors, and a bare tensor with values outside the range
    iface = batch.knn_graph(k=30, other_chains_only=True, cutoff=12.0)
    ef = batch.edge_features(iface)
    assert torch.equal(ef.idx, iface.idx) and bool(((ef.offset == 65) == ef.mask).all())
    assert_pdb_rbf(ef, pdb_reference(batch, ef.idx, range(5)), "interface graph")
    mine = torch.from_numpy(E.random_graph(B, N, 5, seed=3)).long()
    mine[:, ::7, 2] = N + 5
    mine[:, 1::7, 3] = -7
    ef = batch.edge_features(mine, frames=True)
    assert ef.idx.is_cuda and int(ef.idx.min()) == -1 and int(ef.idx.max()) < N and not ef.mask[:, ::7, 2].any()
    assert_pdb_rbf(ef, pdb_reference(batch, ef.idx, range(5)), "a bare tensor")
    rot, trans = batch.backbone_orientations_and_translations()
    ref = E.edge_frames(rot.cpu().numpy(), trans.cpu().numpy(), ef.idx.cpu().numpy(),
                        batch._present_atoms()[:, :, :3].all(-1).cpu().numpy())
    assert_frames_equal_the_yardstick((ef.local_pos, ef.rel_rot), ref, "a bare tensor, frames")


# ---- second trips of the two grid-capped kernels ---------------------------------------------------------------------------------
def prefix_graph(B, N, k, seed):
    """(B,N,k) int32 from numpy alone, not from the kNN kernel: every row a random number (0 .. k) of random neighbours
    followed by -1, a tenth of the rows wholly padded -- consecutive residues of one workgroup use different amounts of
    what the workgroup keeps between them"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, size=(B, N, k)).astype(np.int32)
    count = rng.integers(0, k + 1, size=(B, N))
    count[rng.random((B, N)) < 0.1] = 0
    idx[np.arange(k)[None, None, :] >= count[..., None]] = -1
    return idx


# k_edge_rbf runs min(N, 1024) workgroups that walk residues i, i + 1024, ...: at N = 1025 workgroup 0 alone takes a second
# residue, at N = 2050 workgroups 0 and 1 take three and the others two; rows of 45 floats (no multiple of 4) and of 1904
@pytest.mark.parametrize("N", (1025, 2050))
@pytest.mark.parametrize("k,A,P,R", ((3, 5, 3, 5), (17, 15, 7, 16)))
def test_rbf_workgroups_that_take_more_than_one_residue(pkg, N, k, A, P, R):
    rng = np.random.default_rng(1000 * k + N)
    xyz = (rng.normal(size=(2, N, A, 3)) * 8.0).astype(np.float32)
    mask = rng.random((2, N, A)) >= 1.0 / 3.0
    xyz[~mask] = np.nan                                                              # NaN under the mask
    idx = prefix_graph(2, N, k, seed=k + N)
    assert k * P * R in (45, 1904) and (idx[:, :1024] >= 0).any() and (idx[:, 1024:] >= 0).any()
    assert ((idx >= 0).sum(-1) == 0).any() and ((idx >= 0).sum(-1) == k).any()
    pairs, centers, sigma = tables(A, P, R)
    ref = E.edge_rbf(xyz, idx, mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    assert ref.real[:, :1024].any() and ref.real[:, 1024:].any() and not ref.real[:, 1024:].all()
    got = run_rbf(pkg, xyz, idx, mask, pairs, centers, sigma)
    assert_rbf_meets_the_yardstick(got, ref, f"N={N} k={k} A={A} P={P} R={R}")
    # dist alone: the workgroup skips the rbf row of every residue it takes
    kw = dict(pair_i=[p[0] for p in pairs], pair_j=[p[1] for p in pairs], centers=centers, sigma=sigma)
    dist, none = pkg.ops.edge_rbf(dev(xyz), dev(idx), dev(mask), want_rbf=False, **kw)
    assert none is None and torch.equal(bits(dist), bits(got[0]))
    raw = rbf_in_sentinels(pkg, dev(xyz), dev(idx), dev(mask), pairs, centers, sigma, want_rbf=False)
    assert raw[1] is None and torch.equal(bits(raw[0]), bits(got[0]))


def test_frames_grid_that_takes_a_second_trip(pkg):
    """k_edge_frames caps its grid at 4096 workgroups of 256 lanes, 1 048 576 edges of a structure per trip: N = 16500,
    k = 64 are 1 056 000, so the first 29 workgroups take a second trip"""
    B, N, k = 2, 16500, 64
    assert N * k - 4096 * 256 == 7424
    rot, trans = E.random_frames(B, N, seed=5)
    mask = np.random.default_rng(6).random((B, N)) >= 0.3
    rot[~mask], trans[~mask] = np.nan, np.nan                                        # NaN under the mask
    idx = prefix_graph(B, N, k, seed=7)
    ref = E.edge_frames(rot, trans, idx, mask)
    last = ref.real.reshape(B, N * k)[:, 4096 * 256:]
    assert last.any() and not last.all()
    got = pkg.geometry.edge_frame_features(dev(rot), dev(trans), dev(idx), dev(mask))
    raw = frames_in_sentinels(pkg, dev(rot), dev(trans), dev(idx), dev(mask))
    for a, b in zip(got, raw):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b)), "two launches differ"
    assert_frames_equal_the_yardstick(got, ref, f"N={N} k={k}")
