"""Host-side checks of the edge features: the yardstick itself (tests/edge_ref.py) on hand-computed cases, the C ABI's
surface and its argument validation, the argument validation of ``ops.edge_rbf`` and ``ops.edge_frames``,
``geometry.rbf_centers``, what ``StructureBatch.edge_features`` hands to the geometry layer, its sequence offsets, and the
composed route of the timing tool.  No GPU needed."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import edge_ref as E
from tests.conftest import GOLDEN_DIR


def f32(*rows):
    return np.array(rows, dtype=np.float32)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def test_a_3_4_5_triangle():
    """three residues of two atoms: slot 0 at the corners of a 3-4-5 triangle, slot 1 one unit above"""
    corners = f32([0, 0, 0], [3, 0, 0], [3, 4, 0])
    xyz = np.stack([corners, corners + f32([0, 0, 1])], axis=1)[None]           # (1,3,2,3)
    idx = np.array([[[1, 2], [2, 0], [0, 1]]], dtype=np.int32)
    centers = f32(3.0, 4.0, 5.0, 0.0).reshape(-1)
    ref = E.edge_rbf(xyz, idx, None, [0, 0], [0, 1], centers, 2.0)
    assert ref.dist.dtype == np.float32 and ref.rbf.dtype == np.float64
    assert ref.dist.shape == (1, 3, 2, 2) and ref.rbf.shape == (1, 3, 2, 8)
    assert ref.dist[0, :, :, 0].tolist() == [[3.0, 5.0], [4.0, 3.0], [5.0, 4.0]]
    assert ref.dist[0, 0, 0, 1] == np.float32(math.sqrt(10.0)) and ref.dist[0, 0, 1, 1] == np.float32(math.sqrt(26.0))
    # a centre exactly at d gives 1.0; the others are the Gaussian of the gap over sigma
    assert ref.rbf[0, 0, 0, 0] == 1.0 and ref.rbf[0, 0, 1, 2] == 1.0
    assert np.allclose(ref.rbf[0, 0, 0, :4], [1.0, math.exp(-0.25), math.exp(-1.0), math.exp(-2.25)], rtol=1e-15, atol=0)
    assert np.allclose(ref.rbf[0, 0, 1, :4], [math.exp(-1.0), math.exp(-0.25), 1.0, math.exp(-6.25)], rtol=1e-15, atol=0)
    z = (np.float64(np.float32(math.sqrt(10.0))) - 3.0) / 2.0
    assert math.isclose(ref.rbf[0, 0, 0, 4], math.exp(-z * z), rel_tol=1e-15)                              # element [p * R + c]
    assert ref.real.all()


def test_the_order_of_operations_is_the_stated_one():
    xyz = f32([0.1, 0.7, 1.3], [0.25, -2.0, 9.5]).reshape(1, 2, 1, 3)
    X = xyz.astype(np.float64)
    dx, dy, dz = X[0, 1, 0] - X[0, 0, 0]
    ref = E.edge_rbf(xyz, np.array([[[1], [0]]]), None, [0], [0], f32(2.0, 22.0).reshape(-1), np.float32(1.25))
    d = np.float32(np.sqrt((dx * dx + dy * dy) + dz * dz))
    assert ref.dist[0, 0, 0, 0] == d == ref.dist[0, 1, 0, 0]
    z = (np.float64(d) - 22.0) / 1.25
    assert math.isclose(ref.rbf[0, 0, 0, 1], math.exp(-(z * z)), rel_tol=1e-15)


def test_padding_and_masked_pairs_give_exact_zeros():
    xyz = np.arange(2 * 4 * 2 * 3, dtype=np.float32).reshape(2, 4, 2, 3)
    mask = np.ones((2, 4, 2), dtype=bool)
    mask[0, 1, 1] = False
    xyz[0, 1, 1] = np.nan                                                        # NaN under the mask
    idx = np.array([[[1, -1, 4], [0, 2, -7], [1, 3, 9], [3, 3, 3]]] * 2, dtype=np.int32)
    ref = E.edge_rbf(xyz, idx, mask, [0, 1, 0], [0, 1, 1], f32(1.0, 30.0).reshape(-1), 3.0)
    assert not np.isnan(ref.dist).any() and not np.isnan(ref.rbf).any()
    pad = ~((idx >= 0) & (idx < 4))                                              # -1, 4, -7, 9: anything outside [0, N)
    assert not ref.real[pad].any()
    assert not ref.dist[pad].any() and not ref.rbf[pad].any()
    # structure 0: pairs that touch atom (1, 1) -- as the source's slot 1 in row 1, as the neighbour's slot 1 in row 0
    assert not ref.dist[0, 1, :, 1].any() and not ref.rbf[0, 1, :, 2:4].any()
    assert ref.dist[0, 0, 0].tolist()[1:] == [0.0, 0.0] and ref.dist[0, 0, 0, 0] > 0 and not ref.rbf[0, 0, 0, 2:].any()
    assert ref.real[1][~pad[1]].all() and (ref.rbf[1][~pad[1]] > 0).any()
    # a residue is its own neighbour at distance 0: a real value, not a zero of the padding
    assert ref.dist[1, 3, 0].tolist() == [0.0, 0.0, float(np.float32(math.sqrt(27.0)))]
    assert ref.real[1, 3, 0].all() and math.isclose(ref.rbf[1, 3, 0, 0], math.exp(-1.0 / 9.0), rel_tol=1e-15)
    # an unmasked NaN propagates
    assert np.isnan(E.edge_rbf(xyz, idx, None, [1], [1], f32(1.0).reshape(-1), 3.0).dist[0, 1, 0, 0])


def test_identity_and_equal_frames():
    rot, trans = E.random_frames(1, 5, seed=3)
    idx = np.array([[[1, 2], [0, -1], [2, 4], [9, 0], [3, 3]]], dtype=np.int32)
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (1, 5, 3, 3))
    ref = E.edge_frames(eye, trans, idx)
    assert ref.local_pos.dtype == np.float32 and ref.rel_rot.dtype == np.float32
    assert ref.local_pos.shape == (1, 5, 2, 3) and ref.rel_rot.shape == (1, 5, 2, 3, 3)
    want = (trans[0, 1].astype(np.float64) - trans[0, 0].astype(np.float64)).astype(np.float32)
    assert np.array_equal(ref.local_pos[0, 0, 0], want)                          # the identity frame: t_j - t_i
    assert np.array_equal(ref.rel_rot[0, 0, 0], np.eye(3, dtype=np.float32))
    assert not ref.local_pos[0, 1, 1].any() and not ref.rel_rot[0, 3, 0].any() and not ref.real[0, 1, 1]
    # equal frames: rel_rot is the identity to the rounding of a float32 basis, and exactly so for a signed permutation
    same = np.broadcast_to(rot[0, 0], (1, 5, 3, 3)).copy()
    assert np.abs(E.edge_frames(same, trans, idx).rel_rot[0, 0, 0] - np.eye(3)).max() < 1e-6
    perm = np.broadcast_to(f32([0, -1, 0], [0, 0, 1], [-1, 0, 0]), (1, 5, 3, 3)).copy()
    ref = E.edge_frames(perm, trans, idx)
    assert np.array_equal(ref.rel_rot[0, 2, 1], np.eye(3, dtype=np.float32))
    v = trans[0, 4].astype(np.float64) - trans[0, 2].astype(np.float64)
    assert np.array_equal(ref.local_pos[0, 2, 1], np.array([-v[2], -v[0], v[1]]).astype(np.float32))   # R^T v: the columns
    # the frame mask: a masked source or neighbour gives zeros, and its NaN is never read
    rot[0, 1], trans[0, 1] = np.nan, np.nan
    ref = E.edge_frames(rot, trans, idx, np.array([[1, 0, 1, 1, 1]], dtype=bool))
    assert not np.isnan(ref.local_pos).any() and not np.isnan(ref.rel_rot).any()
    assert not ref.real[0, 0, 0] and not ref.real[0, 1].any() and ref.real[0, 0, 1] and ref.real[0, 2].all()
    assert not ref.rel_rot[0, 0, 0].any() and ref.rel_rot[0, 0, 1].any()


def test_residue_case():
    case = E.residue_case(65, 5, seed=7)
    assert case.xyz.shape == (3, 65, 5, 3) and case.xyz.dtype == np.float32 and case.mask.shape == (3, 65, 5)
    assert 0.35 < 1.0 - case.mask[0].mean() < 0.55 and np.isnan(case.xyz[0][~case.mask[0]]).all()
    assert not np.isnan(case.xyz[0][case.mask[0]]).any()
    assert not case.mask[1].any() and np.isnan(case.xyz[1]).all() and case.mask[2].all() and not np.isnan(case.xyz[2]).any()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_rbf_entry_refuses_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 and N = 0 launch nothing.  The pair tables and the
    centres are host arrays and are read in every call."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)           # noqa: E731
    floats = lambda *v: (ctypes.c_float * len(v))(*v)       # noqa: E731
    tables = dict(pair_i=ints(*range(64)), pair_j=ints(2, 1, 0, *range(3, 64)), centers=floats(*range(64)))

    def call(xyz=fake, mask=None, idx=fake, pair_i=tables["pair_i"], pair_j=tables["pair_j"], P=3, centers=tables["centers"],
             R=5, sigma=1.25, dist=fake, rbf=fake, B=0, N=8, A=64, k=8):
        return lib.ps_edge_rbf_f32(xyz, mask, idx, pair_i, pair_j, P, centers, R, sigma, dist, rbf, B, N, A, k, None)

    assert call() == 0 and call(mask=fake) == 0 and call(B=4, N=0) == 0 and call(B=0, N=0) == 0
    assert call(dist=None) == 0 and call(rbf=None) == 0
    assert call(dist=None, rbf=None) == 1                                     # both outputs null
    for name in ("xyz", "idx", "pair_i", "pair_j", "centers"):
        assert call(**{name: None}) == 1, name
    for k in (0, 65, -1):
        assert call(k=k) == 1, k
    for P in (0, 65, -1):
        assert call(P=P) == 1, P
    for R in (0, 65, -1):
        assert call(R=R) == 1, R
    assert call(k=1, P=1, R=1) == 0 and call(k=64, P=64, R=64) == 0
    # a slot below 0 or not below A, in either table, within the first P entries only
    assert call(A=3) == 0 and call(A=2) == 1 and call(A=0) == 1
    assert call(pair_i=ints(0, -1, 0)) == 1 and call(pair_j=ints(0, 0, 64)) == 1 and call(pair_j=ints(0, 0, 63)) == 0
    assert call(pair_i=ints(0, 0, 0, -1)) == 0 and call(P=64, A=63) == 1
    for sigma in (0.0, -1.25, math.nan, -math.inf, math.inf):
        assert call(sigma=sigma) == 1, sigma
    assert call(sigma=1e-30) == 0 and call(sigma=1e30) == 0
    assert call(B=-1) == 1 and call(N=-1) == 1 and call(B=65536) == 1 and call(B=65535, N=0) == 0
    assert call(N=2 ** 24 + 1) == 1 and call(N=2 ** 24) == 0


def test_frames_entry_refuses_bad_arguments_before_any_launch():
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)

    def call(rot=fake, trans=fake, mask=None, idx=fake, pos=fake, rel=fake, B=0, N=8, k=8):
        return lib.ps_edge_frames_f32(rot, trans, mask, idx, pos, rel, B, N, k, None)

    assert call() == 0 and call(mask=fake) == 0 and call(B=4, N=0) == 0 and call(pos=None) == 0 and call(rel=None) == 0
    assert call(pos=None, rel=None) == 1
    for name in ("rot", "trans", "idx"):
        assert call(**{name: None}) == 1, name
    for k in (0, 65, -1):
        assert call(k=k) == 1, k
    assert call(k=1) == 0 and call(k=64) == 0
    assert call(B=-1) == 1 and call(N=-1) == 1 and call(B=65536) == 1 and call(N=2 ** 24 + 1) == 1 and call(N=2 ** 24) == 0


# ---- ops -------------------------------------------------------------------------------------------------------------------
def rbf_args(B=2, N=6, A=5, k=3):
    g = torch.Generator().manual_seed(1)
    return torch.randn(B, N, A, 3, generator=g), torch.randint(-1, N, (B, N, k), generator=g, dtype=torch.int32)


def test_rbf_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    xyz, idx = rbf_args()
    mask = torch.ones(2, 6, 5, dtype=torch.bool)
    good = dict(pair_i=[0, 1, 4], pair_j=[1, 1, 0], centers=[2.0, 3.0], sigma=1.25)
    check = lambda x=xyz, i=idx, m=None, **kw: ops.check_edge_rbf_shapes(x, i, m, **{**good, **kw})   # noqa: E731
    check()
    check(xyz.double(), idx.long(), mask.float(), centers=np.linspace(0, 1, 64), pair_i=(0,) * 64, pair_j=[4] * 64)
    check(m=mask.to(torch.uint8), centers=torch.tensor([1.0]), want_dist=False)
    check(i=idx[:, :, :1], want_rbf=False)
    for bad in (xyz[0], xyz[..., :2], xyz.long(), xyz[:, :, :, None]):
        with pytest.raises(ValueError, match="xyz"):
            check(bad)
    for bad in (idx[0], idx[:1], idx[:, :5], idx[..., None], idx[:, :, :0], idx.repeat(1, 1, 22)):
        with pytest.raises(ValueError, match="idx"):
            check(i=bad)
    for bad in (idx.float(), idx.bool()):
        with pytest.raises(ValueError, match="integer"):
            check(i=bad)
    for bad in (mask[:, :, :4], mask[:1], mask[..., None]):
        with pytest.raises(ValueError, match="atom_mask"):
            check(m=bad)
    for bad in (dict(pair_i=[0, 1]), dict(pair_i=[], pair_j=[]), dict(pair_i=[0] * 65, pair_j=[0] * 65), dict(pair_i=3)):
        with pytest.raises(ValueError, match="pair_i and pair_j"):
            check(**bad)
    for bad in (dict(pair_i=[0, 1, 5]), dict(pair_j=[-1, 0, 0])):
        with pytest.raises(ValueError, match="atom slot"):
            check(**bad)
    for bad in ([], [0.0] * 65, [[1.0, 2.0]], "abc"):
        with pytest.raises(ValueError, match="centers"):
            check(centers=bad)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="sigma"):
            check(sigma=bad)
    with pytest.raises(ValueError, match="nothing to compute"):
        check(want_dist=False, want_rbf=False)
    with pytest.raises(ValueError):                                           # device disagreement
        check(i=idx.to("meta"))
    with pytest.raises(ValueError):
        check(m=mask.to("meta"))
    with pytest.raises(ValueError, match="65535"):
        ops.check_edge_rbf_shapes(torch.zeros(65536, 0, 5, 3), torch.zeros(65536, 0, 3, dtype=torch.int32), **good)
    with pytest.raises(ValueError, match="2\\^24"):
        ops.check_edge_rbf_shapes(torch.zeros(1, 2 ** 24 + 1, 5, 3, device="meta"),
                                  torch.zeros(1, 2 ** 24 + 1, 3, dtype=torch.int32, device="meta"), **good)


def test_frames_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    rot, trans, idx = torch.zeros(2, 6, 3, 3), torch.zeros(2, 6, 3), rbf_args()[1]
    mask = torch.ones(2, 6, dtype=torch.bool)
    check = ops.check_edge_frames_shapes
    check(rot, trans, idx)
    check(rot.double(), trans.double(), idx.long(), mask.float(), False, True)
    check(rot, trans, idx, mask, True, False)
    for bad in (rot[0], rot[..., :2], rot.reshape(2, 6, 9), rot.long()):
        with pytest.raises(ValueError, match="rot"):
            check(bad, trans, idx)
    for bad in (trans[0], trans[:1], trans[:, :5], trans[..., :2], trans.long()):
        with pytest.raises(ValueError, match="trans"):
            check(rot, bad, idx)
    for bad in (idx[0], idx[:, :5], idx[:, :, :0], idx.repeat(1, 1, 22), idx.float()):
        with pytest.raises(ValueError, match="idx"):
            check(rot, trans, bad)
    for bad in (mask[:, :5], mask[:1], mask[..., None]):
        with pytest.raises(ValueError, match="frame_mask"):
            check(rot, trans, idx, bad)
    with pytest.raises(ValueError, match="nothing to compute"):
        check(rot, trans, idx, None, False, False)
    for moved in (dict(trans=trans.to("meta")), dict(idx=idx.to("meta")), dict(frame_mask=mask.to("meta"))):
        kw = dict(trans=trans, idx=idx, frame_mask=mask)
        kw.update(moved)
        with pytest.raises(ValueError):
            check(rot, **kw)


def test_ops_validate_first_then_refuse_cpu_tensors(monkeypatch):
    from protstruc_amd import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_load)
    xyz, idx = rbf_args()
    good = dict(pair_i=[0], pair_j=[1], centers=[2.0], sigma=1.0)
    with pytest.raises(ValueError):
        ops.edge_rbf(xyz, idx[:, :5], **good)
    with pytest.raises(ValueError):
        ops.edge_rbf(xyz, idx, **{**good, "sigma": 0.0})
    with pytest.raises(ValueError):
        ops.edge_rbf(xyz, idx, **{**good, "pair_j": [5]})
    with pytest.raises(TypeError):
        ops.edge_rbf(xyz, idx, None, [0], [1], [2.0], 1.0)                    # the tables go by keyword
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.edge_rbf(xyz, idx, **good)
    rot, trans = torch.zeros(2, 6, 3, 3), torch.zeros(2, 6, 3)
    with pytest.raises(ValueError):
        ops.edge_frames(rot, trans[:, :5], idx)
    with pytest.raises(ValueError):
        ops.edge_frames(rot, trans, idx, want_pos=False, want_rot=False)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.edge_frames(rot, trans, idx)


def test_signatures_of_the_three_layers():
    from protstruc_amd import StructureBatch, geometry, ops
    from protstruc_amd.structure_batch import EdgeFeatures
    p = inspect.signature(ops.edge_rbf).parameters
    assert list(p) == ["xyz", "idx", "atom_mask", "pair_i", "pair_j", "centers", "sigma", "want_dist", "want_rbf"]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[3:])
    assert all(p[n].default is inspect.Parameter.empty for n in ("pair_i", "pair_j", "centers", "sigma"))
    assert (p["atom_mask"].default, p["want_dist"].default, p["want_rbf"].default) == (None, True, True)
    p = inspect.signature(ops.edge_frames).parameters
    assert list(p) == ["rot", "trans", "idx", "frame_mask", "want_pos", "want_rot"]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("want_pos", "want_rot"))
    assert (p["frame_mask"].default, p["want_pos"].default, p["want_rot"].default) == (None, True, True)
    p = inspect.signature(geometry.rbf_centers).parameters
    assert [(n, p[n].default) for n in p] == [("n_rbf", 16), ("d_min", 2.0), ("d_max", 22.0)]
    p = inspect.signature(geometry.edge_distance_features).parameters
    assert list(p) == ["xyz", "idx", "atom_mask", "pairs", "centers", "sigma", "return_dist"]
    assert (p["atom_mask"].default, p["centers"].default, p["sigma"].default, p["return_dist"].default) == (None, None, None, False)
    assert list(p["pairs"].default) == [(a, b) for a in range(5) for b in range(5)]
    p = inspect.signature(geometry.edge_frame_features).parameters
    assert list(p) == ["rot", "trans", "idx", "frame_mask"] and p["frame_mask"].default is None
    for fn in (geometry.edge_distance_features, geometry.edge_frame_features):
        assert "not differentiable" in fn.__doc__.lower() and "gather_neighbors" in fn.__doc__
    p = inspect.signature(StructureBatch.edge_features).parameters
    assert list(p) == ["self", "graph", "k", "atoms", "n_rbf", "d_min", "d_max", "frames", "max_offset"]
    assert [p[n].default for n in list(p)[1:]] == [None, 30, ("N", "CA", "C", "O", "CB"), 16, 2.0, 22.0, True, 32]
    assert EdgeFeatures._fields == ("idx", "mask", "rbf", "offset", "local_pos", "rel_rot")


def test_rbf_centers():
    from protstruc_amd import geometry
    centers, sigma = geometry.rbf_centers()
    assert isinstance(centers, np.ndarray) and centers.dtype == np.float32 and centers.shape == (16,)
    assert np.array_equal(centers, np.linspace(2.0, 22.0, 16).astype(np.float32)) and sigma == 1.25
    assert centers[0] == 2.0 and centers[-1] == 22.0
    centers, sigma = geometry.rbf_centers(64, 0.0, 32.0)
    assert np.array_equal(centers, np.linspace(0.0, 32.0, 64).astype(np.float32)) and sigma == 0.5
    assert geometry.rbf_centers(1, 3.0, 4.0)[0].tolist() == [3.0]
    for bad in (dict(n_rbf=0), dict(n_rbf=65), dict(n_rbf=2.0), dict(n_rbf=True), dict(d_min=5.0, d_max=5.0),
                dict(d_min=math.nan)):
        with pytest.raises(ValueError):
            geometry.rbf_centers(**bad)
    with pytest.raises(ValueError, match="come together"):
        geometry.edge_distance_features(np.zeros((1, 2, 5, 3), np.float32), np.zeros((1, 2, 1), np.int32), sigma=1.0)


# ---- StructureBatch ----------------------------------------------------------------------------------------------------------
def test_structure_batch_hands_over_pairs_masks_and_frames(monkeypatch):
    """What ``edge_features`` hands to the geometry layer (host-only: the three functions are recorders), on a file with
    two chains batched with a shorter file so that there is padding."""
    from protstruc_amd import StructureBatch, geometry
    from protstruc_amd.structure_batch import EdgeFeatures
    calls = {}
    batch = StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, "5cjx_HL.pdb"), os.path.join(GOLDEN_DIR, "1REX.pdb")],
                                    device="cpu")
    B, N, A = batch.get_xyz().shape[:3]
    g = torch.Generator().manual_seed(5)
    graph = torch.randint(-1, N, (B, N, 30), generator=g, dtype=torch.int32)

    def knn(points, k, point_mask=None, **kw):
        calls["knn"] = dict(points=points, k=k, point_mask=point_mask, **kw)
        return geometry.Neighbors(graph[:, :, :k].clone(), torch.zeros(B, N, k), torch.zeros(B, N, dtype=torch.int32))

    def distance(xyz, idx, atom_mask=None, pairs=None, centers=None, sigma=None, return_dist=False):
        calls["rbf"] = dict(xyz=xyz, idx=idx, atom_mask=atom_mask, pairs=pairs, centers=centers, sigma=sigma,
                            return_dist=return_dist)
        return torch.zeros(*idx.shape, len(pairs) * len(centers))

    def frame(rot, trans, idx, frame_mask=None):
        calls["frames"] = dict(rot=rot, trans=trans, idx=idx, frame_mask=frame_mask)
        return geometry.EdgeFrames(torch.zeros(*idx.shape, 3), torch.zeros(*idx.shape, 3, 3))

    monkeypatch.setattr(geometry, "nearest_neighbors", knn)
    monkeypatch.setattr(geometry, "edge_distance_features", distance)
    monkeypatch.setattr(geometry, "edge_frame_features", frame)
    monkeypatch.setattr(StructureBatch, "backbone_orientations_and_translations",
                        lambda self: (torch.full((B, N, 3, 3), 7.0), self.xyz[:, :, 1]))
    present = batch.get_atom_mask() & batch.residue_mask[:, :, None]

    out = batch.edge_features()
    assert isinstance(out, EdgeFeatures)
    assert calls["knn"]["k"] == 30 and torch.equal(out.idx, graph) and out.idx.dtype == torch.int32
    assert torch.equal(out.mask, graph >= 0) and out.mask.dtype == torch.bool
    call = calls["rbf"]
    assert call["pairs"] == [(a, b) for a in range(5) for b in range(5)] and len(call["pairs"]) == 25   # p = 5 a + b
    assert call["xyz"].data_ptr() == batch.get_xyz().data_ptr() and torch.equal(call["idx"], graph)
    assert torch.equal(call["atom_mask"], present) and not call["return_dist"]
    assert np.array_equal(call["centers"], np.linspace(2.0, 22.0, 16).astype(np.float32)) and call["sigma"] == 1.25
    assert tuple(out.rbf.shape) == (B, N, 30, 400)
    call = calls["frames"]
    assert torch.equal(call["frame_mask"], present[:, :, :3].all(-1)) and torch.equal(call["idx"], graph)
    assert float(call["rot"][0, 0, 0, 0]) == 7.0 and call["trans"].data_ptr() == batch.get_xyz()[:, :, 1].data_ptr()
    assert tuple(out.local_pos.shape) == (B, N, 30, 3) and tuple(out.rel_rot.shape) == (B, N, 30, 3, 3)
    assert out.offset.dtype == torch.int64 and tuple(out.offset.shape) == (B, N, 30)

    # atoms in the caller's order, other centres, no frames, k
    calls.clear()
    out = batch.edge_features(k=48 - 30, atoms=("CB", "CA", "N"), n_rbf=8, d_min=0.0, d_max=16.0, frames=False)
    assert calls["knn"]["k"] == 18 and "frames" not in calls and out.local_pos is None and out.rel_rot is None
    assert calls["rbf"]["pairs"] == [(4, 4), (4, 1), (4, 0), (1, 4), (1, 1), (1, 0), (0, 4), (0, 1), (0, 0)]
    assert np.array_equal(calls["rbf"]["centers"], np.linspace(0.0, 16.0, 8).astype(np.float32)) and calls["rbf"]["sigma"] == 2.0

    # a user's graph, as Neighbors or as a bare tensor of any integer type: anything outside [0, N) becomes -1
    calls.clear()
    mine = graph[:, :, :4].long().clone()
    mine[0, 0] = torch.tensor([-7, N, N + 5, 3])
    want = mine.clone()
    want[0, 0, :3] = -1
    for given in (mine, geometry.Neighbors(mine, None, None), mine.numpy()):
        out = batch.edge_features(given, frames=False)
        assert "knn" not in calls and out.idx.dtype == torch.int32 and torch.equal(out.idx, want.to(torch.int32))
        assert torch.equal(calls["rbf"]["idx"], out.idx) and torch.equal(out.mask, want >= 0)
        assert out.offset[0, 0].tolist()[:3] == [0, 0, 0]
    for bad in (dict(atoms=("XX",)), dict(atoms=()), dict(max_offset=-1), dict(max_offset=1.5)):
        with pytest.raises(ValueError):
            batch.edge_features(mine, frames=False, **bad)


def test_offsets_on_two_chains_with_a_numbering_gap():
    """offset = clip(r_i - r_j + 32, 0, 64) within a chain, 65 across chains, 0 at the padding, in CPU torch"""
    from protstruc_amd import StructureBatch
    N = 8
    xyz = torch.zeros(2, N, 5, 3)
    chain_idx = torch.tensor([[0, 0, 0, 0, 1, 1, 1, float("nan")], [0.0] * N])
    numbering = torch.tensor([[1, 2, 3, 50, 7, 8, 9, float("nan")], [float(v) for v in range(10, 10 + N)]])
    mask = torch.ones(2, N, 5, dtype=torch.bool)
    mask[0, 7] = False
    batch = StructureBatch(xyz, mask, chain_idx, [["A", "B"], ["A"]], None, numbering, device="cpu")
    idx = torch.tensor([[[1, 3, 4, -1]] * N, [[0, 7, -1, 2]] * N], dtype=torch.int32)
    idx[0, 3] = torch.tensor([0, 2, 3, 5])
    idx[0, 5] = torch.tensor([4, 6, 0, 3])
    off = batch._edge_offsets(idx, 32)
    assert off.dtype == torch.int64 and tuple(off.shape) == (2, N, 4)
    assert off[0, 0].tolist() == [32 + 1 - 2, 0, 65, 0]            # 1 - 50 = -49 clips to 0; another chain; the padding
    assert off[0, 2].tolist() == [32 + 3 - 2, 0, 65, 0]
    assert off[0, 3].tolist() == [64, 64, 32, 65]                  # 50 - 1 = 49 and 50 - 3 = 47 clip to 64; itself: 32
    assert off[0, 5].tolist() == [32 + 1, 32 - 1, 65, 65]          # within chain B; chain A twice
    assert off[0, 7].tolist() == [65, 65, 65, 0]                   # a padded residue belongs to no chain
    assert off[1, 0].tolist() == [32, 32 - 7, 0, 32 - 2] and off[1, 7].tolist() == [32 + 7, 32, 0, 32 + 5]
    assert batch._edge_offsets(idx, 2)[1, 0].tolist() == [2, 0, 0, 0] and batch._edge_offsets(idx, 2)[0, 0, 2] == 5
    assert batch._edge_offsets(idx, 0)[0, 5].tolist() == [0, 0, 1, 1]
    # without a numbering the position along N counts: the gap is gone
    bare = StructureBatch(xyz, mask, chain_idx, [["A", "B"], ["A"]], device="cpu")
    assert bare._edge_offsets(idx, 32)[0, 0].tolist() == [31, 29, 65, 0]
    assert bare._edge_offsets(idx, 32)[0, 3].tolist() == [35, 33, 32, 65]


# ---- the timing tool -------------------------------------------------------------------------------------------------------
def test_the_timing_tool_composes_the_same_definition():
    """tools/edge_time.py's composed float32 route (``gather_neighbors``, norm, broadcast exp), run on the CPU here, is the
    yardstick's definition: distances within 1e-4 A (float32 differences of coordinates below 64 A), rbf within 1e-4 (the
    slope of exp(-z^2) in d is below 0.86 / sigma), exact zeros at the padding and the masked pairs."""
    from tools import edge_time
    from protstruc_amd import geometry
    case = E.residue_case(33, 5, seed=11)
    idx = E.random_graph(3, 33, 6, seed=12)
    centers, sigma = geometry.rbf_centers()
    pairs = list(geometry.BACKBONE_PAIRS)
    ref = E.edge_rbf(case.xyz, idx, case.mask, [p[0] for p in pairs], [p[1] for p in pairs], centers, sigma)
    rbf = edge_time.composed(torch.from_numpy(case.xyz), torch.from_numpy(idx), torch.from_numpy(case.mask),
                             torch.tensor(pairs), torch.from_numpy(centers), sigma)
    assert rbf.dtype == torch.float32 and tuple(rbf.shape) == (3, 33, 6, 400)
    assert not rbf.numpy()[~np.repeat(ref.real, 16, axis=-1)].any() and ref.real.any() and not ref.real.all()
    assert np.abs(rbf.numpy() - ref.rbf).max() < 1e-4
    assert (edge_time.B, edge_time.N, edge_time.P, edge_time.R) == (128, 512, 25, 16)
    assert edge_time.SHAPES == {"k48": 48, "k30": 30}
    assert set(edge_time.STEPS) == set(edge_time.STEP_TIMEOUT_S) == {"events", "torch"}
