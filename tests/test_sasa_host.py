"""Host-side checks of solvent accessibility: the yardstick itself (tests/sasa_ref.py) on hand-computed cases and on
human lysozyme, the table of directions, the C ABI's surface, the argument validation of ``ops.solvent_accessibility``, the
signatures of the layers above, the table of maximum accessibilities, and what ``StructureBatch`` hands to the geometry
layer.  No GPU needed."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import sasa_ref as R
from tests.conftest import GOLDEN_DIR

MAX_ACCESSIBILITY = dict(A=129, R=274, N=195, D=193, C=167, E=223, Q=225, G=104, H=224, I=197,
                         L=201, K=236, M=224, F=240, P=159, S=155, T=172, W=285, Y=263, V=174)


def f32(*rows):
    return np.array(rows, dtype=np.float32)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 100))
def test_one_atom_is_fully_exposed(S):
    got = R.sasa(f32([1.0, -2.0, 3.0]), f32(1.7), probe=1.4, n_points=S)
    Rd = float(np.float32(1.7)) + float(np.float32(1.4))
    assert got.count.tolist() == [S] and got.margin == math.inf and not got.buried.any()
    assert abs(got.area[0] - 4 * math.pi * Rd * Rd) < 1e-12


def test_a_hand_computed_pair_on_the_z_axis():
    """r = probe = 1.5, so R = 3 exactly; 3 A apart on z.  Test point k of the lower atom is at 3 u_k, and inside the upper
    sphere iff |3 u_k - (0,0,3)|^2 = 18 - 18 z_k < 9, i.e. z_k > 0.5: with z_k = 1 - (2k+1)/100 that is k <= 24, and by
    symmetry the upper atom loses the 25 points with z_k < -0.5.  75 of 100 points of a sphere of radius 3: 27 pi A^2."""
    got = R.sasa(f32([0, 0, 0], [0, 0, 3]), f32(1.5, 1.5), probe=1.5, n_points=100)
    assert got.count.tolist() == [75, 75]
    assert np.flatnonzero(got.buried[0]).tolist() == list(range(25))
    assert np.flatnonzero(got.buried[1]).tolist() == list(range(75, 100))
    assert np.allclose(got.area, 27 * math.pi, rtol=0, atol=1e-12) and abs(27 * math.pi - 84.8230) < 1e-4
    assert abs(got.margin - 0.18) < 1e-6                  # the closest point to a surface is k = 24: 18 z - 9 = 0.18


def test_yardstick_edge_cases():
    x, r = f32([0, 0, 0], [0, 0, 3]), f32(1.5, 1.5)
    masked = R.sasa(x, r, mask=np.array([True, False]), probe=1.5, n_points=100)
    assert masked.count.tolist() == [100, 0] and masked.area[1] == 0.0          # a masked neighbour buries nothing
    apart = R.sasa(x, r, isolate=np.array([0, 1]), probe=1.5, n_points=100)
    assert apart.count.tolist() == [100, 100]                                   # nor does one with another key
    together = R.sasa(x, r, isolate=np.array([4, 4]), probe=1.5, n_points=100)
    assert together.count.tolist() == [75, 75]
    x3, r3 = f32([0, 0, 0], [np.nan] * 3, [0, 0, 3]), f32(1.5, np.nan, 1.5)
    nan = R.sasa(x3, r3, mask=np.array([True, False, True]), probe=1.5, n_points=100)
    assert nan.count.tolist() == [75, 0, 75] and np.isfinite(nan.area).all() and math.isfinite(nan.margin)
    # two atoms at one place bury each other whole; which is "the other" is decided by index, not by distance
    twice = R.sasa(f32([1, 1, 1], [1, 1, 1]), f32(1.5, 1.6), probe=1.4, n_points=50)
    assert twice.count.tolist() == [0, 50]


# ---- the table of directions -----------------------------------------------------------------------------------------------
def test_sphere_points():
    from protstruc_amd import geometry
    for n in (1, 2, 96, 100, 256):
        u = geometry.sphere_points(n)
        assert tuple(u.shape) == (n, 3) and u.dtype == torch.float32 and u.device.type == "cpu"
        assert np.array_equal(u.numpy(), R.sphere_points(n))
        length = np.sqrt((u.numpy().astype(np.float64) ** 2).sum(-1))
        assert np.abs(length - 1.0).max() <= 2.0 ** -22
        assert (np.diff(u[:, 2].numpy()) < 0).all()
    # n = 1: z = 0, rho = 1, phi = 0
    assert geometry.sphere_points(1).tolist() == [[1.0, 0.0, 0.0]]
    k = 37
    z = 1 - (2 * k + 1) / 96
    phi = k * math.pi * (3 - math.sqrt(5))
    want = np.array([math.sqrt(1 - z * z) * math.cos(phi), math.sqrt(1 - z * z) * math.sin(phi), z]).astype(np.float32)
    assert np.array_equal(geometry.sphere_points(96)[k].numpy(), want)
    with pytest.raises(ValueError):
        geometry.sphere_points(0)


def test_n_points_outside_the_mask_registers_is_refused():
    from protstruc_amd import geometry
    x, r = torch.zeros(1, 4, 3), torch.ones(1, 4)
    for n in (0, -1, 257, 1000):
        with pytest.raises(ValueError, match="n_points"):
            geometry.solvent_accessibility(x, r, n_points=n)
    with pytest.raises(RuntimeError, match="HIP-only"):          # 1 and 256 pass the checks and reach the device test
        geometry.solvent_accessibility(x, r, n_points=256)
    with pytest.raises(RuntimeError, match="HIP-only"):
        geometry.solvent_accessibility(x, r, n_points=1)


# ---- human lysozyme --------------------------------------------------------------------------------------------------------
def test_lysozyme_through_the_reader(monkeypatch):
    """1REX, every atom slot, S = 96, from the tensors ``StructureBatch.solvent_accessibility`` hands on (host-only: the
    geometry function is replaced by the yardstick).  Total area in 6400 .. 7100 A^2 -- a loose plausibility band around
    the 6.6e3 .. 7e3 of the literature, not a measurement -- and every residue's relative accessibility in [0, 1.5]."""
    from protstruc_amd import StructureBatch, geometry
    seen = {}

    def by_yardstick(points, radius, point_mask=None, isolate=None, probe=1.4, n_points=96, sphere=None):
        refs = R.batch(points.numpy(), radius.numpy(), point_mask.numpy(), None if isolate is None else isolate.numpy(),
                       probe=probe, n_points=n_points)
        seen["margin"] = min(ref.margin for ref in refs)
        return geometry.SolventAccessibility(torch.from_numpy(np.stack([ref.count for ref in refs])),
                                             torch.from_numpy(np.stack([ref.area for ref in refs]).astype(np.float32)))

    monkeypatch.setattr(geometry, "solvent_accessibility", by_yardstick)
    batch = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "1REX.pdb"), device="cpu")
    area = batch.solvent_accessibility()
    assert tuple(area.shape) == (1, 130) and area.dtype == torch.float32
    total = float(area.double().sum())
    print("1REX: total accessible area", total, "A^2, margin", seen["margin"])
    assert 6400.0 <= total <= 7100.0
    assert seen["margin"] >= 1e-10
    relative = batch.solvent_accessibility(relative=True)
    assert not torch.isnan(relative).any() and float(relative.min()) >= 0.0 and float(relative.max()) <= 1.5
    assert float(relative.max()) > 0.5 and float((relative < 0.05).float().mean()) > 0.1     # exposed and buried residues
    per_atom = batch.solvent_accessibility(per_residue=False)
    assert tuple(per_atom.shape) == (1, 130, 15) and torch.equal(per_atom.sum(-1, dtype=torch.float64).float(), area)
    assert torch.equal(batch.interface_area(), torch.zeros(1, 130))                            # one chain


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_bad_arguments_before_any_launch():
    """hipErrorInvalidValue (1) without touching a device; B = 0 and M = 0 launch nothing."""
    from protstruc_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)

    def call(points=fake, radius=fake, mask=None, isolate=None, sphere=fake, probe=1.4, count=fake, area=fake, B=0, M=8, S=96):
        return lib.ps_solvent_accessibility_f32(points, radius, mask, isolate, sphere, probe, count, area, B, M, S, None)

    assert call() == 0 and call(B=1, M=0) == 0 and call(mask=fake, isolate=fake) == 0
    for name in ("points", "radius", "sphere", "count", "area"):
        assert call(**{name: None}) == 1, name
    assert call(B=-1) == 1 and call(M=-1) == 1 and call(B=65536, M=0) == 1 and call(B=65535, M=0) == 0
    assert call(M=2 ** 24 + 1) == 1 and call(M=2 ** 24) == 0
    assert call(S=0) == 1 and call(S=-3) == 1 and call(S=1) == 0
    assert call(S=256) == 0 and call(S=257) == 1
    for probe in (-0.5, math.inf, -math.inf, math.nan):
        assert call(probe=probe) == 1, probe
    assert call(probe=0.0) == 0


# ---- ops -------------------------------------------------------------------------------------------------------------------
def sasa_args(B=2, M=9):
    g = torch.Generator().manual_seed(1)
    return torch.randn(B, M, 3, generator=g), torch.full((B, M), 1.7)


def test_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import geometry, ops
    check = ops.check_sasa_shapes
    x, r = sasa_args()
    mask, key, sphere = torch.ones(2, 9, dtype=torch.bool), torch.zeros(2, 9, dtype=torch.int32), geometry.sphere_points(96)
    check(x, r)
    check(x, r, mask, key, sphere, 1.4)
    check(x, r, mask.to(torch.uint8), key.long(), sphere, 0.0)
    check(x, r, mask.float())                                             # any mask dtype: reduced to its truth value
    check(x.double(), r.double())
    check(x, r, sphere=geometry.sphere_points(1))
    check(x, r, sphere=geometry.sphere_points(256))
    for bad in (x[0], x[..., :2], x.long(), x[:, :, None]):
        with pytest.raises(ValueError):
            check(bad, r)
    for bad in (r[:, :8], r[:1], r.long(), r[:, :, None]):
        with pytest.raises(ValueError):
            check(x, bad)
    for bad in (mask[:, :8], mask[:1]):
        with pytest.raises(ValueError):
            check(x, r, bad)
    for bad in (key[:, :8], key.float(), key.bool()):
        with pytest.raises(ValueError):
            check(x, r, None, bad)
    for bad in (sphere.double(), sphere[:, :2], sphere[0], sphere[:0], geometry.sphere_points(257), sphere.numpy(), sphere.long()):
        with pytest.raises(ValueError):
            check(x, r, sphere=bad)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="probe"):
            check(x, r, probe=bad)
    for name, moved in (("radius", r), ("point_mask", mask), ("isolate", key), ("sphere", sphere)):
        kw = dict(radius=r, point_mask=mask, isolate=key, sphere=sphere)
        kw[name] = moved.to("meta")
        with pytest.raises(ValueError):                                   # device disagreement
            check(x, kw["radius"], kw["point_mask"], kw["isolate"], kw["sphere"])
    with pytest.raises(ValueError, match="65535"):
        check(torch.zeros(65536, 0, 3), torch.zeros(65536, 0))
    with pytest.raises(ValueError, match="2\\^24"):
        check(torch.zeros(1, 2 ** 24 + 1, 3, device="meta"), torch.zeros(1, 2 ** 24 + 1, device="meta"))


def test_ops_validate_first_then_refuse_cpu_tensors():
    from protstruc_amd import geometry, ops
    x, r = sasa_args()
    sphere = geometry.sphere_points(96)
    with pytest.raises(ValueError):
        ops.solvent_accessibility(x, r[:, :8], sphere=sphere)
    with pytest.raises(ValueError):
        ops.solvent_accessibility(x, r, sphere=geometry.sphere_points(257))
    with pytest.raises(ValueError):
        ops.solvent_accessibility(x, r, sphere=None)
    with pytest.raises(ValueError):
        ops.solvent_accessibility(x, r, sphere=sphere, probe=-1.0)
    with pytest.raises(TypeError):
        ops.solvent_accessibility(x, r)                                   # sphere is required, by keyword
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.solvent_accessibility(x, r, sphere=sphere)
    with pytest.raises(RuntimeError, match="HIP-only"):
        geometry.solvent_accessibility(x, r)
    with pytest.raises(ValueError):
        geometry.solvent_accessibility(x, r[:, :8])


def test_signatures_of_the_three_layers():
    from protstruc_amd import StructureBatch, geometry, ops
    p = inspect.signature(ops.solvent_accessibility).parameters
    assert list(p) == ["points", "radius", "point_mask", "isolate", "sphere", "probe"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("sphere", "probe"))
    assert (p["point_mask"].default, p["isolate"].default, p["probe"].default) == (None, None, 1.4)
    assert p["sphere"].default is inspect.Parameter.empty
    p = inspect.signature(ops.check_sasa_shapes).parameters
    assert list(p) == ["points", "radius", "point_mask", "isolate", "sphere", "probe"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, 1.4]
    p = inspect.signature(geometry.solvent_accessibility).parameters
    assert list(p) == ["points", "radius", "point_mask", "isolate", "probe", "n_points", "sphere"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, 1.4, 96, None]
    assert geometry.SolventAccessibility._fields == ("count", "area")
    assert list(inspect.signature(geometry.sphere_points).parameters) == ["n"]
    assert "not differentiable" in geometry.solvent_accessibility.__doc__.lower()
    p = inspect.signature(StructureBatch.solvent_accessibility).parameters
    assert list(p) == ["self", "atoms", "probe", "n_points", "radii", "per_residue", "relative", "per_chain"]
    assert [p[k].default for k in list(p)[1:]] == ["all", 1.4, 96, None, True, False, False]
    assert list(inspect.signature(StructureBatch.interface_area).parameters) == ["self"]


def test_max_accessibility_table():
    from protstruc_amd.general import max_accessibility_table
    from protstruc_amd.pdb import ONE_TO_INDEX
    table = max_accessibility_table()
    assert tuple(table.shape) == (21,) and table.dtype == torch.float32
    assert len(MAX_ACCESSIBILITY) == 20 and set(MAX_ACCESSIBILITY) | {"X"} == set(ONE_TO_INDEX)
    for one, value in MAX_ACCESSIBILITY.items():
        assert float(table[ONE_TO_INDEX[one]]) == float(value), one
    assert math.isnan(float(table[ONE_TO_INDEX["X"]]))
    assert float(table[ONE_TO_INDEX["G"]]) == float(table[:20].min()) and float(table[ONE_TO_INDEX["W"]]) == float(table[:20].max())


# ---- StructureBatch ----------------------------------------------------------------------------------------------------------
def test_structure_batch_hands_over_the_points_of_steric_clashes(monkeypatch):
    """The points, radii and mask ``solvent_accessibility`` hands to the geometry layer are those ``steric_clashes``
    hands to ``geometry.steric_clash`` -- rebuilt here by hand, as the method built them before the two shared a helper --
    and ``per_chain`` adds the chain index repeated per atom (host-only: both geometry functions are recorders), on a
    file with two chains and UNK gap residues."""
    from protstruc_amd import StructureBatch, geometry
    from protstruc_amd.general import max_accessibility_table, vdw_radius_table
    from protstruc_amd.structure_batch import clash_links
    sasa_calls, clash_calls = [], []

    def fake_sasa(points, radius, point_mask=None, isolate=None, probe=1.4, n_points=96, sphere=None):
        sasa_calls.append(dict(points=points, radius=radius, point_mask=point_mask, isolate=isolate, probe=probe,
                               n_points=n_points, sphere=sphere))
        area = torch.arange(radius.numel(), dtype=torch.float32).reshape(radius.shape) * (2.0 if isolate is not None else 1.0)
        return geometry.SolventAccessibility(torch.zeros(radius.shape, dtype=torch.int32), area)

    def fake_clash(points, radius, point_mask=None, groups=None, link=None, tolerance=1.5, eps=1e-10, reduction="point"):
        clash_calls.append(dict(points=points, radius=radius, point_mask=point_mask, groups=groups, link=link,
                                tolerance=tolerance, reduction=reduction))
        return torch.zeros(radius.shape), torch.zeros(radius.shape)

    monkeypatch.setattr(geometry, "solvent_accessibility", fake_sasa)
    monkeypatch.setattr(geometry, "steric_clash", fake_clash)
    batch = StructureBatch.from_pdb(os.path.join(GOLDEN_DIR, "5cjx_HL.pdb"), device="cpu")
    B, N, A = batch.get_xyz().shape[:3]
    assert (B, N, A) == (1, 448, 15) and len(batch.get_chain_ids()[0]) == 2

    # by hand: the radii from the sequence, the mask = present, with a radius
    seq_idx = batch.get_seq_idx()
    radius = vdw_radius_table()[seq_idx].reshape(B, N * A)
    present = (batch.get_atom_mask() & batch.residue_mask[:, :, None]).reshape(B, N * A)
    takes_part = present & (radius > 0)
    assert 0 < int(takes_part.sum()) < int(present.sum()) or int(takes_part.sum()) == int(present.sum())

    out = batch.solvent_accessibility(probe=1.2, n_points=64)
    call = sasa_calls[-1]
    assert call["points"].data_ptr() == batch.get_xyz().data_ptr() and tuple(call["points"].shape) == (B, N * A, 3)   # a view
    assert torch.equal(call["radius"], radius) and torch.equal(call["point_mask"], takes_part)
    assert call["isolate"] is None and (call["probe"], call["n_points"], call["sphere"]) == (1.2, 64, None)
    want = torch.arange(N * A, dtype=torch.float32).reshape(B, N, A)
    assert torch.equal(out, want.sum(-1))
    assert torch.equal(batch.solvent_accessibility(per_residue=False), want)

    batch.solvent_accessibility(per_chain=True)
    chain = batch.chain_idx
    key = sasa_calls[-1]["isolate"]
    assert key.dtype == torch.int32 and tuple(key.shape) == (B, N * A)
    assert torch.equal(key.reshape(B, N, A)[:, :, 0].double(), chain.double()) and (key.reshape(B, N, A) == key.reshape(B, N, A)[:, :, :1]).all()
    assert set(key.unique().tolist()) == {0, 1}

    assert torch.equal(batch.interface_area(), want.sum(-1))          # 2 x - x of the recorder
    assert [c["isolate"] is not None for c in sasa_calls[-2:]] == [True, False]

    # a selection of atoms and radii of the caller's own
    own = torch.full((B, N, A), 2.0)
    batch.solvent_accessibility(atoms=("CA", "CB"), radii=own)
    chosen = torch.zeros(A, dtype=torch.bool)
    chosen[[1, 4]] = True
    assert torch.equal(sasa_calls[-1]["point_mask"], (present.reshape(B, N, A) & chosen).reshape(B, N * A))
    assert torch.equal(sasa_calls[-1]["radius"], own.reshape(B, N * A))

    relative = batch.solvent_accessibility(relative=True)
    table = max_accessibility_table()[seq_idx]
    assert torch.equal(torch.isnan(relative), torch.isnan(table) | ~batch.residue_mask)
    assert int(torch.isnan(relative).sum()) == 7                         # the UNK gap residues of this file
    ok = ~torch.isnan(relative)
    assert torch.equal(relative[ok], (want.sum(-1).double() / table.double()).float()[ok])   # divided in double, rounded once
    with pytest.raises(ValueError):
        batch.solvent_accessibility(relative=True, per_residue=False)
    no_seq = StructureBatch.from_xyz(batch.get_xyz()[:, :, :5], device="cpu")
    with pytest.raises(ValueError):
        no_seq.solvent_accessibility(relative=True)
    with pytest.raises(ValueError, match="radii"):
        StructureBatch.from_xyz(batch.get_xyz(), device="cpu").solvent_accessibility()
    no_seq.solvent_accessibility()                                       # N, CA, C, O, CB: the elements are known
    assert float(sasa_calls[-1]["radius"].max()) == pytest.approx(1.7) and sasa_calls[-1]["isolate"] is None

    # steric_clashes: what it received before the refactor
    batch.steric_clashes(tolerance=1.3)
    call = clash_calls[-1]
    assert call["points"].data_ptr() == batch.get_xyz().data_ptr()
    assert torch.equal(call["radius"], radius) and torch.equal(call["point_mask"], takes_part)
    assert torch.equal(call["groups"], torch.arange(N, dtype=torch.int32).repeat_interleave(A).expand(B, N * A))
    assert torch.equal(call["link"], clash_links(batch._valid_junctions(), A, seq_idx == 1))
    assert (call["tolerance"], call["reduction"]) == (1.3, "none")


# ---- the timing tool -------------------------------------------------------------------------------------------------------
def test_the_timing_tool_composes_the_same_definition():
    """tools/sasa_time.py's composed-torch evaluation (cdist neighbours, a dense point-to-neighbour test; float32), run on
    the CPU here, counts as the yardstick does on a case whose margin is above float32's reach: what the tool times is the
    definition, not something cheaper."""
    from tools import sasa_time
    case = R.synthetic_case(65, 11)
    refs = R.case_reference(case)
    margin = min(ref.margin for ref in refs)
    print("margin", margin)
    assert margin >= 1e-4                                                 # float32 against float64
    sphere = torch.from_numpy(R.sphere_points(96))
    count, area = sasa_time.composed(torch.from_numpy(case.x), torch.from_numpy(case.r), torch.from_numpy(case.mask), sphere)
    assert count.dtype == torch.int32 and area.dtype == torch.float32
    for b, ref in enumerate(refs):
        assert np.array_equal(count[b].numpy(), ref.count), b
        assert np.allclose(area[b].numpy(), ref.area, rtol=1e-6, atol=0)
    keyed = R.synthetic_case(65, 11, keys=2)
    count, _ = sasa_time.composed(torch.from_numpy(keyed.x), torch.from_numpy(keyed.r), torch.from_numpy(keyed.mask), sphere,
                                  isolate=torch.from_numpy(keyed.isolate))
    keyed_refs = R.case_reference(keyed)
    assert min(ref.margin for ref in keyed_refs) >= 1e-4
    assert all(np.array_equal(count[b].numpy(), ref.count) for b, ref in enumerate(keyed_refs))
    assert (sasa_time.B, sasa_time.N, sasa_time.A, sasa_time.S) == (128, 512, 15, 96)
    assert set(sasa_time.STEPS) == set(sasa_time.STEP_TIMEOUT_S) == {"events", "torch"}
