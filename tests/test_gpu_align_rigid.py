"""GPU tests of the alignment and rigid-body kernels (csrc/align.hip, csrc/rigid.hip) behind ops.kabsch, geometry.kabsch,
StructureBatch.align, ops.rigid (translate / rotate / center_at / get_local_xyz), ops.center_of_mass,
ops.frames_to_backbone and ops.min_dist_to_points (get_topk_nearest_residue_mask).

Yardstick: tests/align_ref.py, float64 numpy on the same float32 inputs.  Every element of every case is compared.

Kabsch, for every structure with at least one selected atom, R and t read back as float32 and evaluated in float64:
    max |R R^T - I| <= 8 * 2^-24        (the rows are unit vectors rounded to float32)
    |det R - 1|     <= 16 * 2^-24
    rmsd(R, t)      <= rmsd_opt + DELTA,  DELTA = 2^-22 (3 max_k |a_k| + |t|): twice the displacement caused by rounding a
                       perfect R and t to float32 (align_ref's docstring); tests/test_align_host.py asserts that the float64
                       SVD solution rounded to float32 stays inside DELTA / 2 on every case
    max |R - R64|   <= 5e-6             where the rotation is unique (s1 + d s2 > 1e-3 s0, asserted there for those cases)
One selected atom or coincident atoms: R is exactly the identity and t = b - a to one float32 ulp.  No selected atom:
R and t are NaN.

Measured on an MI355X, max |R R^T - I| and rmsd / optimum in A -- with the former solve (eigenvectors of H^T H) and with
the present one (one-sided Jacobi on H, csrc/kabsch_solve.hpp):
    generic 360 atoms          5.0e-8   0.875697 / 0.875697          unchanged (max |R - R64| = 2.2e-8)
    mirror-image target        3.8e-8   18.23672 / 18.23672          unchanged
    planar, 3 atoms, 4 atoms   <= 5.1e-8, optimal                    unchanged
    line + 1e-2 A              3.0e-8   optimal                  ->  6.2e-8, optimal
    line + 1e-4 A              3.2e-6   2.2939e-4 / 2.2516e-4    ->  3.9e-8   2.25167e-4 / 2.25159e-4
    line + 1e-6 A              3.7e-2   0.386 / 2.2e-6           ->  4.1e-8   2.27e-6 / 2.22e-6
    exactly collinear, 30      NaN                               ->  3.1e-8   5.628457 / 5.628457
    2 atoms                    0.96     12.8 / 0.0176            ->  3.3e-8   0.01757806 / 0.01757784
    1 atom, coincident atoms   NaN                               ->  exactly I, t = b - a
    align() over 2 anchors     0.98; pairwise distances off by up to 43 A  ->  4.6e-8; by 2.8e-6 A
rigid: largest error 2.64 x 2^-24 of the scale (bound 4); center_of_mass: at most 0.9 x 2^-24 |mean| (bound 2).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import protstruc_oracle as O
from tests import align_ref as A

pytestmark = pytest.mark.gpu

BATCHES = A.kabsch_batches()
U = A.U32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


def gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """The float64 fits of a batch's structures, computed once and shared (never modified)."""
    return [A.kabsch64(a, b, m) for a, b, m in A.structures(BATCHES[name])]


def as_residues(x):
    """(B, n, ...) -> (B, N, 15, ...) when n is a multiple of 15, else (B, n, 1, ...)."""
    B, n = x.shape[:2]
    return x.reshape((B, n // 15, 15) + x.shape[2:]) if n % 15 == 0 else x.reshape((B, n, 1) + x.shape[2:])


def run_kabsch(ops, batch):
    src, dst, mask = batch
    R, t = ops.kabsch(gpu(as_residues(src)), gpu(as_residues(dst)), gpu(as_residues(mask)))
    torch.cuda.synchronize()
    assert R.dtype == torch.float32 and t.dtype == torch.float32
    assert R.shape == (src.shape[0], 3, 3) and t.shape == (src.shape[0], 3)
    return R.cpu().numpy(), t.cpu().numpy()


def check_structure(label, R, t, a, b, m, k):
    n_sel = int(m.sum())
    if n_sel == 0:
        assert np.isnan(R).all() and np.isnan(t).all(), f"{label}: no selected atom gives NaN"
        return
    ortho, det = A.rotation_errors(R)
    rmsd, bound = A.rmsd64(R, t, a, b, m), A.delta(a, t, m)
    unique = A.is_unique(k)
    print(f"{label}: selected {n_sel}  max|RR^T-I| = {ortho:.2e}  |det-1| = {det:.2e}  rmsd = {rmsd:.6e}  optimum = "
          f"{k.rmsd:.6e}  DELTA = {bound:.2e}  max|R-R64| = {np.abs(R - k.R).max():.2e}{'' if unique else ' (not unique)'}")
    assert np.isfinite(R).all() and np.isfinite(t).all(), label
    assert ortho <= A.ORTHO_BOUND, f"{label}: max|RR^T - I| = {ortho:.3e}"
    assert det <= A.DET_BOUND, f"{label}: |det R - 1| = {det:.3e}"
    assert rmsd <= k.rmsd + bound, f"{label}: rmsd {rmsd:.6e} against the optimum {k.rmsd:.6e} + {bound:.2e}"
    if unique:
        assert np.abs(R - k.R).max() <= A.R_TOL, f"{label}: max|R - R64| = {np.abs(R - k.R).max():.3e}"
    if (k.s == 0).all():
        assert (R == np.eye(3, dtype=np.float32)).all(), f"{label}: H = 0 gives exactly the identity"
        assert (np.abs(t - k.t) <= 2 * U * np.abs(k.t)).all(), f"{label}: t = b - a to one ulp"


@pytest.mark.parametrize("name", list(BATCHES))
def test_kabsch(ops, name):
    """Every batch of align_ref.kabsch_batches: the degenerate and generic builders, 1 ... 1005 selected atoms dense and
    scattered in 1005 NaN-filled slots, selections past index 256, B in {1, 3, 5} with own and shared targets and masks,
    the mixed batch and the empty mask."""
    R, t = run_kabsch(ops, BATCHES[name])
    for s, ((a, b, m), k) in enumerate(zip(A.structures(BATCHES[name]), yardstick(name))):
        check_structure(f"{name} [{s}]", R[s], t[s], a, b, m, k)


def test_kabsch_structures_of_a_batch_do_not_see_each_other(ops):
    """The mixed batch (generic, two atoms, collinear, empty mask): every result equals, bit for bit, the one obtained
    alone; so do the results under a shared target and a shared mask."""
    for name in ("mixed", "B=3 target shared mask shared", "B=5 target own mask own"):
        src, dst, mask = BATCHES[name]
        R, t = run_kabsch(ops, BATCHES[name])
        for s in range(src.shape[0]):
            one = (src[s:s + 1], dst[s:s + 1] if dst.shape[0] > 1 else dst, mask[s:s + 1] if mask.shape[0] > 1 else mask)
            R1, t1 = run_kabsch(ops, one)
            assert np.array_equal(R1[0], R[s], equal_nan=True) and np.array_equal(t1[0], t[s], equal_nan=True), (name, s)


def test_kabsch_no_atoms_and_no_structures(ops):
    R, t = ops.kabsch(torch.zeros(3, 0, 15, 3).cuda(), torch.zeros(1, 0, 15, 3).cuda(), torch.zeros(3, 0, 15, dtype=torch.bool).cuda())
    assert R.shape == (3, 3, 3) and t.shape == (3, 3) and R.isnan().all() and t.isnan().all()
    R, t = ops.kabsch(torch.zeros(0, 4, 15, 3).cuda(), torch.zeros(0, 4, 15, 3).cuda(), torch.zeros(0, 4, 15, dtype=torch.bool).cuda())
    assert R.shape == (0, 3, 3) and t.shape == (0, 3)
    torch.cuda.synchronize()


def test_kabsch_wrappers_take_float64_and_strided_inputs(ops):
    """Float64 tensors, tensors with a stride in the last axis, a float mask and numpy arrays give the float32 contiguous
    call's result bit for bit, through ops.kabsch and geometry.kabsch."""
    from protstruc_amd import geometry
    for name in ("B=3 target shared mask own", "mirror-image target"):
        src, dst, mask = BATCHES[name]
        R, t = run_kabsch(ops, (src, dst, mask))
        wide = lambda x: torch.from_numpy(np.repeat(x.astype(np.float64), 2, axis=-1)).cuda()[..., ::2]  # noqa: E731
        s64, d64 = wide(src), wide(dst)
        assert s64.dtype == torch.float64 and not s64.is_contiguous()
        fmask = torch.from_numpy(np.repeat(mask.astype(np.float32) * 3.0, 2, axis=-1)).cuda()[..., ::2]
        R2, t2 = ops.kabsch(s64[:, :, None], d64[:, :, None], fmask)
        assert np.array_equal(R2.cpu().numpy(), R) and np.array_equal(t2.cpu().numpy(), t), name
    a, b = A.kabsch_cases()["generic 360"]
    k = A.kabsch64(a, b)
    R, t = geometry.kabsch(a.astype(np.float64), b.astype(np.float64))
    assert isinstance(R, np.ndarray) and R.shape == (3, 3) and t.shape == (3,)
    check_structure("geometry.kabsch numpy float64", R.astype(np.float32), t.astype(np.float32), a, b, np.ones(360, bool), k)
    Rt, tt = geometry.kabsch(torch.from_numpy(np.repeat(a, 2, axis=0)).cuda()[::2], torch.from_numpy(b).double())
    assert Rt.is_cuda and np.array_equal(Rt.cpu().numpy(), R) and np.array_equal(tt.cpu().numpy(), t)
    for name in ("2 atoms", "1 atoms", "collinear"):
        a, b = A.kabsch_cases()[name]
        R, t = geometry.kabsch(a, b)
        check_structure(f"geometry.kabsch {name}", R, t, a, b, np.ones(len(a), bool), A.kabsch64(a, b))


def pair_distances(x):
    x = A.f64(x).reshape(-1, 3)
    return np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))


@pytest.mark.parametrize("selection", ["2 atoms", "collinear"])
def test_align_end_to_end_on_degenerate_selections(selection):
    """StructureBatch.align over two anchors, and over 30 collinear atoms, of a 20-residue structure: the moved anchors lie
    within DELTA of the optimal RMSD and the structure keeps its shape (every pairwise distance to 1e-4 A).  The check the
    closed form from the eigenvectors of H^T H failed: it collapsed the structure."""
    from protstruc_amd import StructureBatch
    a, b = A.cloud(60, seed=60, noise=0.2)
    mask = np.zeros(60, bool)
    if selection == "2 atoms":
        mask[[7, 40]] = True
    else:
        a[:30], b[:30] = A.collinear(30)
        mask[:30] = True
    k = A.kabsch64(a, b, mask)
    assert not A.is_unique(k)
    sb = StructureBatch.from_xyz(torch.from_numpy(a).reshape(1, 20, 3, 3), device="cuda")
    target = StructureBatch.from_xyz(torch.from_numpy(b).reshape(1, 20, 3, 3), device="cuda")
    R = sb.align(target, atom_mask=torch.from_numpy(mask).reshape(1, 20, 3).cuda())
    moved = sb.get_xyz().cpu().numpy().reshape(60, 3)
    ortho, det = A.rotation_errors(R[0].cpu().numpy())
    rmsd = A.rmsd64(np.eye(3), np.zeros(3), moved, b, mask)
    R64 = A.f64(R[0])
    bound = A.delta(a, A.f64(b)[mask].mean(0) - R64 @ A.f64(a)[mask].mean(0), mask)
    drift = np.abs(pair_distances(moved) - pair_distances(a)).max()
    print(f"align over {selection}: max|RR^T-I| = {ortho:.2e}  rmsd of the moved anchors = {rmsd:.6e}  optimum = {k.rmsd:.6e}"
          f"  DELTA = {bound:.2e}  largest change of a pairwise distance = {drift:.2e} A")
    assert ortho <= A.ORTHO_BOUND and det <= A.DET_BOUND
    assert rmsd <= k.rmsd + bound
    assert drift <= 1e-4


# ---- ops.rigid ----------------------------------------------------------------------------------------------------------
def check_rigid(label, got, x, R, t, transpose):
    want, scale = A.rigid64(x, R, t, transpose)
    got = A.f64(got)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label}: NaN positions"
    err = np.nan_to_num(np.abs(got - want) - 4 * U * scale, nan=-1.0)
    assert (err <= 0).all(), f"{label}: {np.nanmax(np.abs(got - want) / scale):.3e} of the scale (bound {4 * U:.3e})"
    return float(np.nanmax(np.abs(got - want) / np.where(scale > 0, scale, np.nan))) if np.isfinite(want).any() else 0.0


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 3), (3, 17, 15), (1, 86, 3)])
def test_rigid_every_arm(ops, shape):
    """Every r_mode x t_mode x transpose, in place and out of place, elementwise within 4 * 2^-24 (sum_j |R_ij x_j| + |t_i|);
    the matrices are not symmetric, so a swapped transpose fails; NaN atoms and NaN components stay where they are."""
    B, N, A_ = shape
    rng = np.random.default_rng(sum(shape))
    x = (12 * rng.standard_normal((B, N, A_, 3))).astype(np.float32)
    if N * A_ > 4:
        flat = x.reshape(B, N * A_, 3)
        flat[0, 1] = np.nan                                  # a whole atom
        flat[-1, 3, 1] = np.nan                              # one component
        flat[0, -1, 2] = np.nan                              # the last atom of a structure (index 257 of 258)
        if N * A_ > 256:
            flat[0, 255] = np.nan
    rots = {"none": None, "(3,3)": rng.standard_normal((3, 3)), "(B,3,3)": rng.standard_normal((B, 3, 3)),
            "(B,N,3,3)": rng.standard_normal((B, N, 3, 3))}
    trs = {"none": None, "(3,)": (3,), "(1,3)": (1, 3), "(B,3)": (B, 3), "(B,1,3)": (B, 1, 3), "(B,N,3)": (B, N, 3),
           "(B,N,A,3)": (B, N, A_, 3)}
    xg = gpu(x)
    worst = 0.0
    for rn, R in rots.items():
        R = None if R is None else R.astype(np.float32)
        if R is not None:
            assert np.abs(R - np.swapaxes(R, -1, -2)).max() > 0.1
        for tn, ts in trs.items():
            t = None if ts is None else (30 * rng.standard_normal(ts)).astype(np.float32)
            for transpose in (False, True):
                label = f"{shape} R {rn} t {tn} transpose {transpose}"
                Rg, tg = None if R is None else gpu(R), None if t is None else gpu(t)
                out = ops.rigid(xg, Rg, tg, transpose=transpose)
                assert out.data_ptr() != xg.data_ptr() and np.array_equal(xg.cpu().numpy(), x, equal_nan=True)
                worst = max(worst, check_rigid(label, out.cpu().numpy(), x, R, t, transpose))
                own = xg.clone()
                same = ops.rigid(own, Rg, tg, transpose=transpose, inplace=True)
                assert same.data_ptr() == own.data_ptr() and torch.equal(same.nan_to_num(7e7), out.nan_to_num(7e7)), label
    print(f"rigid {shape}: largest error = {worst / U:.2f} x 2^-24 of the scale (bound 4)")


def test_structure_batch_rigid_methods():
    """translate, rotate, center_at and get_local_xyz against the yardstick applied to the same operands."""
    from protstruc_amd import StructureBatch
    rng = np.random.default_rng(70)
    x = (9 * rng.standard_normal((3, 17, 15, 3))).astype(np.float32)
    sb = StructureBatch.from_xyz(torch.from_numpy(x), device="cuda")
    rot = sb.backbone_orientations()
    ca = x[:, :, A.CA]
    check_rigid("get_local_xyz", sb.get_local_xyz().cpu().numpy(), x, rot.cpu().numpy(), -ca, True)
    t = (5 * rng.standard_normal((3, 17, 3))).astype(np.float32)
    sb.translate(torch.from_numpy(t))
    check_rigid("translate", sb.get_xyz().cpu().numpy(), x, None, t, False)
    x1 = sb.get_xyz().cpu().numpy()
    R = rng.standard_normal((3, 3, 3)).astype(np.float32)
    sb.rotate(torch.from_numpy(R))
    check_rigid("rotate", sb.get_xyz().cpu().numpy(), x1, R, None, False)
    x2 = sb.get_xyz().cpu().numpy()
    com = sb.center_of_mass().cpu().numpy()
    center = np.array([[1.0, -2.0, 3.0]], dtype=np.float32)
    sb.center_at(torch.from_numpy(center))
    check_rigid("center_at", sb.get_xyz().cpu().numpy(), x2, None, (center - com).astype(np.float32), False)


# ---- ops.center_of_mass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_center_of_mass(ops, N):
    """Per-component nanmean of the first and the last slot: NaN in single components, a structure whose slot is all NaN,
    a centroid near 1e4 A.  The kernel accumulates in double and rounds once: |error| <= 2^-23 |mean|."""
    rng = np.random.default_rng(80 + N)
    x = (10 * rng.standard_normal((4, N, 5, 3))).astype(np.float32)
    for atom in (0, 4):
        x[1, rng.integers(0, N, max(1, N // 4)), atom, rng.integers(0, 3, max(1, N // 4))] = np.nan
        x[2, :, atom] = np.nan
        x[3, :, atom] += np.array([9000.0, -7000.0, 10000.0], dtype=np.float32)
    for atom in (0, 4):
        got = ops.center_of_mass(gpu(x), atom).cpu().numpy()
        want = A.center_of_mass64(x, atom)
        assert got.dtype == np.float32 and got.shape == (4, 3)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[2]).all() and not np.isnan(got[[0, 3]]).any()
        err = np.nan_to_num(np.abs(got - want) / np.abs(want))
        print(f"center_of_mass N={N} slot {atom}: largest error = {err.max() / U:.2f} x 2^-24 |mean| (bound 2)")
        assert (err <= 2 * U).all()
    assert ops.center_of_mass(torch.zeros(2, 0, 5, 3).cuda(), 1).isnan().all()


# ---- ops.frames_to_backbone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ideal,n_slots", [(3, 3), (3, 4), (3, 5), (3, 15), (4, 4), (4, 5), (4, 15)])
def test_frames_to_backbone(ops, n_ideal, n_slots):
    rng = np.random.default_rng(90)
    rot = np.stack([A.rotation(rng) for _ in range(2 * 37)]).reshape(2, 37, 3, 3).astype(np.float32)
    trans = (25 * rng.standard_normal((2, 37, 3))).astype(np.float32)
    ideal = O.ideal_backbone(n_ideal == 4).numpy()
    got = ops.frames_to_backbone(gpu(rot), gpu(trans), gpu(ideal), n_slots).cpu().numpy()
    want, scale = A.frames_to_backbone64(rot, trans, ideal, n_slots)
    assert got.shape == (2, 37, n_slots, 3) and got.dtype == np.float32
    assert (got[:, :, n_ideal:] == 0).all() and not np.signbit(got[:, :, n_ideal:]).any(), "padded slots are exactly +0.0"
    assert (np.abs(got - want) <= 4 * U * scale).all()
    if n_slots == 15:
        from protstruc_amd import StructureBatch
        sb = StructureBatch.from_backbone_orientations_translations(torch.from_numpy(rot), torch.from_numpy(trans),
                                                                    include_cb=n_ideal == 4, device="cuda")
        assert (np.abs(sb.get_xyz().cpu().numpy() - want) <= 4 * U * scale + 1e-6).all()   # its own ideal coordinates
        assert sb.get_atom_mask().sum().item() == 2 * 37 * n_ideal


# ---- ops.min_dist_to_points, get_topk_nearest_residue_mask ---------------------------------------------------------------
@pytest.mark.parametrize("N,n_query", [(1, 1), (1, 300), (255, 7), (256, 1), (256, 300), (257, 7), (257, 300)])
def test_min_dist_to_points(ops, N, n_query):
    """|d - d64| <= 8 * 2^-24 d for each of the three slots; a NaN query point turns every output NaN, a NaN atom only its
    own residue; zero query points are refused before any launch."""
    xyz, _, _, query = A.topk_case(N, n_query)
    for atom in (0, 1, 2):
        got = ops.min_dist_to_points(gpu(xyz), gpu(query), atom).cpu().numpy()
        want = A.min_dist64(xyz, query, atom)
        assert got.dtype == np.float32 and got.shape == (N,)
        assert (np.abs(got - want) <= 8 * U * want).all(), np.abs(got / want - 1).max()
    poisoned = query.copy()
    poisoned[n_query // 2, 1] = np.nan
    assert np.isnan(ops.min_dist_to_points(gpu(xyz), gpu(poisoned)).cpu().numpy()).all()
    hole = xyz.copy()
    hole[N // 2, A.CA, 0] = np.nan
    got, want = ops.min_dist_to_points(gpu(hole), gpu(query)).cpu().numpy(), A.min_dist64(hole, query)
    assert np.array_equal(np.isnan(got), np.arange(N) == N // 2) and np.array_equal(np.isnan(got), np.isnan(want))
    assert (np.nan_to_num(np.abs(got - want) - 8 * U * want, nan=-1.0) <= 0).all()
    with pytest.raises(ValueError, match="no point"):
        ops.min_dist_to_points(gpu(xyz), gpu(query[:0]))


def test_topk_nearest_residue_mask():
    """Equal to the float64 selection for k below, equal to and above the number of valid residues, with and without a
    user mask; tests/test_align_host.py asserts that every case keeps 1e-3 A between the last distance taken and the
    first one left out, so no comparison depends on a tie."""
    from protstruc_amd import StructureBatch
    cases = A.topk_cases()
    for c in cases:
        N = c["xyz"].shape[0]
        atom_mask = torch.from_numpy(c["residue_mask"])[None, :, None].expand(1, N, 3)
        sb = StructureBatch.from_xyz(torch.from_numpy(c["xyz"])[None], atom_mask, device="cuda")
        got = sb.get_topk_nearest_residue_mask(torch.from_numpy(c["query"]), k=c["k"],
                                               mask=None if c["user"] is None else torch.from_numpy(c["user"]))
        want, gap = A.topk_mask64(c["xyz"], c["residue_mask"], c["query"], c["k"], c["user"])
        assert gap > A.TOPK_GAP
        assert got.shape == (1, N) and got.dtype == torch.bool and np.array_equal(got[0].cpu().numpy(), want), c["label"]
    print(f"top-k: {len(cases)} cases equal to the float64 selection")
