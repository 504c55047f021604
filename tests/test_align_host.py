"""Host-side checks of the alignment and rigid-body ops: the yardstick itself (tests/align_ref.py) against the goldens, the
oracle and hand-computed examples; the conditions the GPU comparisons of tests/test_gpu_align_rigid.py rely on, asserted
from the yardstick alone; the argument validation of ops.kabsch / rigid / min_dist_to_points / center_of_mass before any
launch; and the kernel's 3x3 solve (csrc/kabsch_solve.hpp), compiled into a stand-alone host program and held to the
float64 SVD on every case builder.  No GPU needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import protstruc_oracle as O
from tests import align_ref as A
from tests.conftest import ROOT, load_golden

BATCHES = A.kabsch_batches()


def test_yardstick_matches_the_golden_and_the_oracle():
    g = load_golden("g12_align_topk")
    a, b = g["xyz"][0].reshape(-1, 3), g["target_xyz"][0].reshape(-1, 3)
    k = A.kabsch64(a, b)
    assert np.abs(k.R - A.f64(g["kabsch_R"])).max() <= 2e-6 and np.abs(k.t - A.f64(g["kabsch_t"])).max() <= 2e-5
    gen = torch.Generator().manual_seed(3)
    for n in (3, 4, 57):
        a = torch.randn(n, 3, generator=gen, dtype=torch.float64) * 7
        b = torch.randn(n, 3, generator=gen, dtype=torch.float64) * 7 + 3
        r, t = O.kabsch(a, b)
        k = A.kabsch64(a, b)
        assert np.abs(k.R - r.numpy()).max() <= 1e-12 and np.abs(k.t - t.numpy()).max() <= 1e-11
    xyz = torch.randn(3, 9, 5, 3, generator=gen, dtype=torch.float64)
    xyz[0, 2, 1, 1] = float("nan")
    xyz[1, :, 1] = float("nan")
    com, want = A.center_of_mass64(xyz), O.center_of_mass(xyz).numpy()
    assert np.array_equal(np.isnan(com), np.isnan(want)) and np.isnan(com[1]).all() and not np.isnan(com[0]).any()
    assert np.nanmax(np.abs(com - want)) <= 1e-14
    rot = torch.linalg.qr(torch.randn(2, 6, 3, 3, generator=gen, dtype=torch.float64)).Q
    trans = torch.randn(2, 6, 3, generator=gen, dtype=torch.float64) * 20
    for cb in (False, True):
        want, _ = O.frames_to_backbone(rot.float(), trans.float(), include_cb=cb, n_slots=6)
        got, scale = A.frames_to_backbone64(rot.float(), trans.float(), O.ideal_backbone(cb), 6)
        assert got.shape == (2, 6, 6, 3) and (got[:, :, 3 + cb:] == 0).all() and (scale[:, :, 3 + cb:] == 0).all()
        assert (np.abs(got - want.numpy()) <= 4 * A.U32 * scale).all()
    for case in A.topk_cases():
        want = O.topk_nearest_residue_mask(torch.from_numpy(case["xyz"]).double(), torch.from_numpy(case["residue_mask"]),
                                           torch.from_numpy(case["query"]).double(), case["k"],
                                           None if case["user"] is None else torch.from_numpy(case["user"]))
        got, _ = A.topk_mask64(case["xyz"], case["residue_mask"], case["query"], case["k"], case["user"])
        assert np.array_equal(got, want[0].numpy()), case["label"]


def test_yardstick_on_hand_computed_examples():
    """A quarter turn about z, a pure translation, and two points: the best fit puts the segments' midpoints and
    directions on each other, leaving each end half the difference of the lengths away."""
    a = np.array([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0], [1.0, 1.0, 1.0]])
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    k = A.kabsch64(a, a @ turn.T + np.array([5.0, -2.0, 0.5]))
    assert np.abs(k.R - turn).max() <= 1e-15 and np.abs(k.t - [5.0, -2.0, 0.5]).max() <= 1e-14 and k.rmsd <= 1e-14 and k.d == 1
    k = A.kabsch64(a, a + np.array([1.0, 2.0, 3.0]))
    assert np.abs(k.R - np.eye(3)).max() <= 1e-15 and np.abs(k.t - [1.0, 2.0, 3.0]).max() <= 1e-14
    a2, b2 = np.array([[0.0, 0, 0], [3.0, 4.0, 0]]), np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 8.5]])
    k = A.kabsch64(a2, b2)
    assert abs(k.rmsd - abs(5.0 - 7.5) / 2) <= 1e-14 and A.rotation_errors(k.R)[0] <= 1e-14 and not A.is_unique(k)
    k = A.kabsch64(a, a * np.array([-1.0, 1.0, 1.0]))            # a mirror image: d = -1, still a proper rotation
    assert k.d == -1 and A.rotation_errors(k.R)[1] <= 1e-14
    one = A.kabsch64(a[:1], a[:1] + 2.0)
    assert (one.R == np.eye(3)).all() and (one.t == 2.0).all() and one.rmsd == 0
    none = A.kabsch64(a, a, np.zeros(4, bool))
    assert np.isnan(none.R).all() and np.isnan(none.t).all()
    assert A.rmsd64(np.eye(3), np.zeros(3), a, a + 1.0, [1, 0, 0, 1]) == pytest.approx(3 ** 0.5)
    x = np.arange(24.0).reshape(1, 2, 4, 3)
    y, scale = A.rigid64(x, turn, np.array([[1.0, 0, 0]]), transpose=True)
    assert np.array_equal(y, x @ turn + [1.0, 0, 0]) and np.array_equal(scale, np.abs(x) @ np.abs(turn) + [1.0, 0, 0])
    assert A.min_dist64(x[0], np.array([[4.0, 4.0, 5.0], [100.0, 0, 0]]))[0] == 1.0 and A.min_dist64(x[0], x[0, 1, 1])[1] == 0


@pytest.mark.parametrize("name", list(BATCHES))
def test_kabsch_cases_meet_the_conditions_of_their_comparisons(name):
    """From the yardstick alone: the float64 solution rounded to float32 meets the three property bounds with room to
    spare; the masked-out slots hold NaN; a degenerate case has H = 0 exactly."""
    src, dst, mask = BATCHES[name]
    assert src.dtype == np.float32 and dst.dtype == np.float32 and mask.dtype == bool
    assert src.shape[0] in (1, 3, 4, 5) and src.size <= 5 * 67 * 15 * 3
    for a, b, m in A.structures(BATCHES[name]):
        assert np.isnan(a[~m]).all() and not np.isnan(a[m]).any() and not np.isnan(b[m]).any()
        k = A.kabsch64(a, b, m)
        if m.sum() == 0:
            assert np.isnan(k.R).all()
            continue
        R32, t32 = k.R.astype(np.float32), k.t.astype(np.float32)
        ortho, det = A.rotation_errors(R32)
        assert ortho <= A.ORTHO_BOUND / 2 and det <= A.DET_BOUND / 2
        assert A.rmsd64(R32, t32, a, b, m) <= k.rmsd + A.delta(a, t32, m) / 2
        if m.sum() == 1 or name == "coincident":
            assert (k.s == 0).all() and (k.R == np.eye(3)).all()
        if name in ("generic 360", "mirror-image target", "planar", "octahedron", "far 1e3", "far 1e4", "identical",
                    "3 atoms", "4 atoms") or (name.startswith(("dense", "scattered", "tail", "B=")) and m.sum() >= 3):
            assert A.is_unique(k), (name, k.s, k.d)
        if name in ("collinear", "2 atoms", "line + 1e-06", "line + 0.0001", "line + 0.01", "coincident", "1 atoms"):
            assert not A.is_unique(k)
    if name == "mirror-image target":
        assert k.d == -1
    if name == "octahedron":
        assert k.s[2] > 0.999 * k.s[0]
    if name.startswith("tail"):
        assert not mask[:, :257].any()
    if name == "mixed":
        assert [int(m.sum()) for _, _, m in A.structures(BATCHES[name])] == [30, 2, 30, 0]


def test_topk_cases_keep_their_gap():
    cases = A.topk_cases()
    assert {c["xyz"].shape[0] for c in cases} == {1, 255, 256, 257}
    assert {c["query"].shape[0] for c in cases} == {1, 7, 300}
    relation = set()
    for c in cases:
        valid = c["residue_mask"] if c["user"] is None else c["residue_mask"] & c["user"]
        relation.add(np.sign(c["k"] - int(valid.sum())))
        got, gap = A.topk_mask64(c["xyz"], c["residue_mask"], c["query"], c["k"], c["user"])
        assert gap > A.TOPK_GAP, c["label"]
        assert got.sum() == min(c["k"], valid.sum()) and not got[~valid].any()
    assert relation == {-1, 0, 1}


def test_gpu_tests_compare_every_element():
    """The GPU tests exclude nothing from a comparison: no fraction of permitted outliers, no skip, no expected failure."""
    text = open(os.path.join(ROOT, "tests", "test_gpu_align_rigid.py")).read()
    for word in ("bad_frac", "frac_bad", "skip", "xfail", "quantile", "percentile", "median"):
        assert word not in text, word


# ---- argument validation ------------------------------------------------------------------------------------------------
def test_kabsch_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_kabsch_shapes
    src, m = torch.zeros(4, 6, 5, 3), torch.ones(4, 6, 5, dtype=torch.bool)
    assert check(src, src, m) == (4, 30, False, False)
    assert check(src, src[:1], m[0]) == (4, 30, True, True)
    assert check(src[:1], src[:1], m[:1]) == (1, 30, False, False)
    assert check(src.reshape(4, 30, 3), src.reshape(4, 30, 1, 3), m.reshape(-1)) == (4, 30, False, False)
    assert check(src[:, :0], src[:1, :0], m[:, :0])[:2] == (4, 0)
    for args in ((src[..., :2], src, m), (src, src[..., :2], m), (src[0, 0, 0], src, m), (src, src[:, :5], m),
                 (src, src[:2], m), (src, src[:0], m), (src, src, m[:2]), (src, src, m[:, :5]), (src, src, m[:, :, :4]),
                 (src, src, m[:0]), (src[:, :0], src[:, :0], m)):
        with pytest.raises(ValueError):
            check(*args)
    with pytest.raises(ValueError):
        ops.kabsch(src, src[:3], m)                     # validated first, then the CPU tensors are refused
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.kabsch(src, src, m)


def test_min_dist_shape_checker_raises_for_each_malformed_argument():
    from protstruc_amd import ops
    check = ops.check_min_dist_shapes
    xyz, q = torch.zeros(6, 5, 3), torch.zeros(7, 3)
    assert check(xyz, q) == (6, 5, 7) and check(xyz, q[0], 4) == (6, 5, 1) and check(xyz, q.reshape(7, 1, 3), 0) == (6, 5, 7)
    for args in ((xyz[None], q), (xyz[..., :2], q), (xyz, q[:, :2]), (xyz, q[:0]), (xyz, torch.zeros(())), (xyz, q, 5),
                 (xyz, q, -1), (xyz[:, :0], q, 0)):
        with pytest.raises(ValueError):
            check(*args)
    with pytest.raises(ValueError, match="no point"):
        ops.min_dist_to_points(xyz, q[:0])
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.min_dist_to_points(xyz, q)


def test_rigid_and_center_of_mass_validate_before_any_launch():
    from protstruc_amd import ops
    xyz = torch.zeros(2, 5, 4, 3)
    eye = torch.eye(3)
    assert ops.check_rigid_shapes(xyz) == (0, 0)
    assert ops.check_rigid_shapes(xyz, eye, torch.zeros(3)) == (1, 1)
    assert ops.check_rigid_shapes(xyz, eye.expand(2, 3, 3), torch.zeros(1, 3)) == (2, 1)
    assert ops.check_rigid_shapes(xyz, eye.expand(2, 5, 3, 3), torch.zeros(2, 3)) == (3, 2)
    assert [ops.check_rigid_shapes(xyz, None, torch.zeros(*s))[1] for s in ((2, 1, 3), (2, 5, 3), (2, 5, 4, 3))] == [2, 3, 4]
    for R, t in ((torch.zeros(3, 2), None), (eye.expand(3, 3, 3), None), (eye.expand(2, 4, 3, 3), None), (eye[0], None),
                 (eye.expand(1, 2, 5, 3, 3), None), (None, torch.zeros(2)), (None, torch.zeros(3, 3)),
                 (None, torch.zeros(2, 4, 3)), (None, torch.zeros(2, 5, 3, 3)), (None, torch.zeros(2, 5, 4, 2))):
        with pytest.raises(ValueError):
            ops.rigid(xyz, R, t)
    with pytest.raises(ValueError):
        ops.rigid(xyz[0], eye)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.rigid(xyz, eye)
    for atom in (-1, 4):
        with pytest.raises(ValueError):
            ops.center_of_mass(xyz, atom)
    with pytest.raises(ValueError):
        ops.center_of_mass(xyz[0])
    with pytest.raises(RuntimeError, match="HIP-only"):
        ops.center_of_mass(xyz, 3)


# ---- the kernel's 3x3 solve on the host ---------------------------------------------------------------------------------
def covariance(a, b, m):
    a, b = A.f64(a)[m], A.f64(b)[m]
    return (a - a.mean(0)).T @ (b - b.mean(0))


def test_the_kernels_solve_on_the_host_matches_the_float64_svd(tmp_path):
    """csrc/kabsch_solve.hpp, the function the kernel calls, in a plain C++ program: on the covariance of every structure
    of every batch, R held in double is a proper rotation to 1e-14 (measured: 1.1e-15), reaches the optimal RMSD within
    DELTA and equals the float64 SVD's rotation where that is unique; H = 0 gives the identity, a NaN covariance NaN."""
    compiler = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "kabsch_solve_host")
    subprocess.run([compiler, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "protstruc_amd", "csrc"),
                    os.path.join(ROOT, "tools", "kabsch_solve_host.cpp"), "-o", exe], check=True)
    todo = [(name, a, b, m) for name in BATCHES for a, b, m in A.structures(BATCHES[name]) if m.any()]
    Hs = [covariance(a, b, m) for _, a, b, m in todo]
    extra = [np.zeros((3, 3)), np.full((3, 3), np.nan), Hs[0] * 1e-150, Hs[0] * 1e120, np.diag([2.0, 0, 0]),
             np.diag([0, 0, -3.0]), np.diag([1.0, 1.0, -1.0])]
    text = "".join(" ".join(repr(float(x)) for x in H.reshape(-1)) + "\n" for H in Hs + extra)
    done = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
    Rs = np.array([[float(x) for x in line.split()] for line in done.stdout.splitlines()]).reshape(-1, 3, 3)
    assert Rs.shape[0] == len(Hs) + len(extra)
    worst = 0.0
    for (name, a, b, m), R in zip(todo, Rs):
        k = A.kabsch64(a, b, m)
        ortho, det = A.rotation_errors(R)
        worst = max(worst, ortho)
        assert ortho <= 1e-14 and det <= 1e-14, (name, ortho, det)
        t = A.f64(b)[m].mean(0) - R @ A.f64(a)[m].mean(0)
        assert A.rmsd64(R, t, a, b, m) <= k.rmsd + A.delta(a, t, m), name
        if A.is_unique(k):
            assert np.abs(R - k.R).max() <= 1e-9, (name, np.abs(R - k.R).max())
        if (k.s == 0).all():
            assert (R == np.eye(3)).all(), name
    print(f"largest max|R R^T - I| of the host solve over {len(todo)} covariances: {worst:.2e}")
    tail = Rs[len(Hs):]
    assert (tail[0] == np.eye(3)).all() and np.isnan(tail[1]).all()
    assert np.abs(tail[2] - Rs[0]).max() <= 1e-14 and np.abs(tail[3] - Rs[0]).max() <= 1e-14      # R ignores the scale of H
    for R, H in zip(tail[4:], extra[4:]):
        ortho, det = A.rotation_errors(R)
        assert ortho <= 1e-15 and det <= 1e-15
        U, s, Vt = np.linalg.svd(H)
        best = s[0] + s[1] + np.sign(np.linalg.det(Vt.T @ U.T)) * s[2]
        assert abs(np.trace(R @ H) - best) <= 1e-15 * s[0]                                        # the optimum: max tr(R H)
