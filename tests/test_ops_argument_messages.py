"""The argument checks of the shell, pinned word for word: one table of (callable, args, kwargs, exception type, exact
message), compared with ``==``.  Every row has one fault in otherwise valid arguments at the smallest shapes (B = 2,
N or M = 5, A = 5); the size limits are reached with ``meta`` tensors, which have a shape and no memory.  A second table
holds one valid call per ``check_*`` function and what it returns.  The expected texts were recorded from the code before
the checks were rewritten over shared helpers.  No GPU and no built library needed.

Covered: the public ``check_*`` functions of ``ops``, ``check_lengths``, ``_peptide_bond_constants`` and the helpers they
raise through (``_check_atom_slots``, ``_check_float_tensor``, ``_check_out`` without a device, ``_same_device`` -- a
``meta`` tensor is "another device" to it), and the ``reduction`` check of ``geometry.lddt`` / ``geometry.steric_clash``,
which raises before any launch.  Those functions held 112 ``raise`` statements when the texts were recorded (105 in the
19 ``check_*`` functions and ``_peptide_bond_constants``, 5 in the four helpers, 2 in ``geometry``); the table has 186
rows: at least one per statement, and several where one statement serves a loop of names, has two ways to fail, or sits
in a helper that more than one checker calls.

The K24-K46 families were added to the table later, again from the code as it stood before their checks moved onto the
helpers: the 14 ``check_*`` functions of k-NN, the edge features, chi, the closest atoms, the pair head, superposition,
structure alignment and the ensemble, the checks of ``nw_align`` and ``ca_secondary_structure`` -- reached through the
wrappers themselves, where they come before the device is asked for -- and the helpers ``_check_breaks``,
``_check_objectives``, ``_check_neighbor_idx``, ``_host_f32``, ``_host_i32_table``, ``_chi_tables`` and
``_check_residue_type``.  Those held 79 ``raise`` statements (``_pair_batch`` and ``_chi_dims`` included) and take 260
rows, which brings the table to 446 rows and the valid calls to 47; ``test_host_tables_normalise`` holds what the
host-table helpers return.  The checks of the two wrappers have since become ``check_nw_align_shapes`` and
``check_ca_secondary_structure_shapes``, which added their two valid calls and no row.

Left out, because they need a CUDA tensor: ``_require_device``, the device half of ``_check_rng_state`` (its other
two ``raise`` statements belong to no ``check_*`` function) and ``_check_out`` with a device.
"""
import numpy as np
import pytest
import torch

from protstruc_amd import geometry, ops

B, N, A, M = 2, 5, 5, 5


def f(*shape):
    return torch.zeros(*shape)


def meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def i64(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


def b8(*shape):
    return torch.ones(*shape, dtype=torch.bool)


XYZ = f(B, N, A, 3)
XYZ_INT = i64(B, N, A, 3)
PTS = f(B, M, 3)
RAD = f(B, M)
ROT, TRANS = f(B, N, 3, 3), f(B, N, 3)
PLANE = f(B, N, N)
DIH = f(B, N, 3)
SPHERE = f(4, 3)
FAPE = (ROT, TRANS, PTS, ROT, TRANS, PTS)
DSSP = (XYZ, b8(B, N), b8(B, N))
E = ValueError

irg = ops.check_inter_residue_geometry_backward_shapes
nerf = ops.check_backbone_from_dihedrals_shapes
nerf_bw = ops.check_backbone_from_dihedrals_backward_shapes
distmat = ops.check_distmat_shapes
fw = ops.check_floyd_warshall_shape
smacof = ops.check_smacof_shapes
frames_bw = ops.check_frames_backward_shapes
fape = ops.check_fape_shapes
lddt = ops.check_lddt_shapes
clash = ops.check_clash_shapes
bond = ops.check_peptide_bond_shapes
dssp = ops.check_dssp_shapes
sasa = ops.check_sasa_shapes
rigid = ops.check_rigid_shapes
kabsch = ops.check_kabsch_shapes
min_dist = ops.check_min_dist_shapes
knn = ops.check_knn_shapes
closest = ops.check_closest_atoms_shapes
pair_bins = ops.check_pair_bins_shapes
binned = ops.check_binned_shapes
superpose = ops.check_superpose_shapes
structalign = ops.check_structalign_shapes
rmsd_matrix = ops.check_rmsd_matrix_shapes
cluster = ops.check_cluster_shapes
edge_rbf = ops.check_edge_rbf_shapes
edge_frames = ops.check_edge_frames_shapes
chi = ops.check_chi_shapes
chi_set = ops.check_chi_set_shapes

Q = 4                                   # queries, columns and the points of a second structure: another number than M
QRY = f(B, Q, 3)
KEYS = dict(exclude=i64(B, M), query_exclude=i64(B, Q))
BREAKS = (2.0, 4.0, 8.0)
PAIR_FRAMES = (ROT, TRANS, ROT, TRANS, PTS)   # rot, trans, target_rot, target_trans, target_points of check_pair_bins_shapes
LOGITS = f(B, N, N, 4)
SCORE = f(B, M, Q)
IDX = i64(B, N, 3)
RBF = dict(pair_i=(1, 4), pair_j=(1, 0), centers=(2.0, 4.0, 6.0))
LIKE = "xyz (2, 5, 5, 3)"
RT = i64(B, N)
CHI = f(B, N, 4)
NO_ANGLE = [-1, -1, -1, -1]


def chi_atoms(first=(0, 1, 2, 3), second=NO_ANGLE):
    """(2, 4, 4): type 0 has its first two angles, type 1 none"""
    return np.array([[first, second, NO_ANGLE, NO_ANGLE], [NO_ANGLE] * 4], dtype=np.int64)


def chi_last(first=4, other=-1, types=2):
    """(types, 4): -1 except angle 0 of type 0 and angle 0 of type 1"""
    table = np.full((types, 4), -1, dtype=np.int64)
    table[0, 0], table[1, 0] = first, other
    return table


ATOMS, LAST = chi_atoms(), chi_last()
CHI_REQUIRED = "chi_atoms is required (general.chi_atom_table())"
CHI_SET_REQUIRED = "chi_atoms and chi_last are required (general.chi_atom_table(), general.chi_last_table())"
TOGETHER = "exclude and query_exclude come together: a candidate is skipped where the two keys are equal"

FAULTS = [
    # ---- check_inter_residue_geometry_backward_shapes
    (irg, (XYZ, {"d_xx": PLANE}), {}, KeyError,
     "\"'d_xx' is not a differentiable plane of inter_residue_geometry (known: d_ca, d_cb, d_no, omega, theta, phi)\""),
    (irg, (f(B, N, A), {}), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (irg, (f(B, N, A, 4), {}), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5, 4)"),
    (irg, (XYZ_INT, {}), {}, E, "xyz must be a floating-point tensor, got torch.int64"),
    (irg, (f(B, N, 4, 3), {}), {}, IndexError, "inter_residue_geometry needs the N, CA, C, O, CB atom slots"),
    (irg, (meta(1, 2049, A, 3), {}), {}, E, "inter_residue_geometry_backward takes at most 2048 residues, got 2049"),
    (irg, (XYZ, {}, f(B, N, 4)), {}, E,
     "atom_mask must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (irg, (XYZ, {"d_ca": f(B, N, 4)}), {}, E,
     "grads['d_ca'] must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (irg, (XYZ, {"phi": i64(B, N, N)}), {}, E, "grads['phi'] must be a floating-point tensor, got torch.int64"),
    (irg, (XYZ, {}), {"out": f(B, N, A, 2)}, E, "out must be a contiguous float32 tensor of shape (2, 5, 5, 3)"),
    (irg, (XYZ, {}), {"out": XYZ.double()}, E, "out must be a contiguous float32 tensor of shape (2, 5, 5, 3)"),
    # ---- check_backbone_from_dihedrals_shapes
    (nerf, (f(B, N, 2),), {}, E, "dihedrals must have shape (batch, residues, 3) [phi, psi, omega], got (2, 5, 2)"),
    (nerf, (DIH, f(B, 4)), {}, E, "chain_idx must have shape (2, 5) to match dihedrals (2, 5, 3), got (2, 4)"),
    (nerf, (DIH,), {"residue_mask": f(B, 4)}, E,
     "residue_mask must have shape (2, 5) to match dihedrals (2, 5, 3), got (2, 4)"),
    (nerf, (DIH,), {"bond_angles": f(B, N)}, E,
     "bond_angles must have shape (2, 5, 3) to match dihedrals (2, 5, 3), got (2, 5)"),
    (nerf, (DIH,), {"bond_lengths": f(B, N)}, E,
     "bond_lengths must have shape (2, 5, 3) to match dihedrals (2, 5, 3), got (2, 5)"),
    # ---- check_backbone_from_dihedrals_backward_shapes
    (nerf_bw, (f(B, N, A), f(B, N, A)), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (nerf_bw, (XYZ, f(B, N, 4, 3)), {}, E, "grad_xyz must have shape (2, 5, 5, 3) to match xyz, got (2, 5, 4, 3)"),
    (nerf_bw, (XYZ_INT, XYZ), {}, E, "xyz must be a floating-point tensor, got torch.int64"),
    (nerf_bw, (XYZ, XYZ_INT), {}, E, "grad_xyz must be a floating-point tensor, got torch.int64"),
    (nerf_bw, (f(B, N, 2, 3), f(B, N, 2, 3)), {}, E, "2 atom slots leave no room for N, CA, C"),
    (nerf_bw, (f(B, N, 4, 3), f(B, N, 4, 3)), {"include_cb": True}, E, "4 atom slots leave no room for N, CA, C and CB"),
    (nerf_bw, (XYZ, XYZ, f(B, 4)), {}, E, "chain_idx must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (nerf_bw, (XYZ, XYZ, None, f(B, 4)), {}, E,
     "residue_mask must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (nerf_bw, (XYZ, XYZ), {"out": (DIH, None)}, E,
     "out must be a (grad_dihedrals, grad_bond_angles, grad_bond_lengths) triple (None where not wanted)"),
    (nerf_bw, (XYZ, XYZ), {"out": (DIH, DIH, None)}, E, "out[1] is given but that gradient is not wanted"),
    (nerf_bw, (XYZ, XYZ), {"out": (f(B, N, 2), None, None)}, E,
     "out[0] must be a contiguous float32 tensor of shape (2, 5, 3)"),
    # ---- check_distmat_shapes / check_distmat_size
    (distmat, (f(B, N, 4), f(B, N, 4), f(B, N, 4), f(B, N, 4)), {}, E, "d_cb must have shape (batch, L, L), got (2, 5, 4)"),
    (distmat, (PLANE, f(B, N, 4), PLANE, PLANE), {}, E,
     "omega must have shape (2, 5, 5) to match d_cb (2, 5, 5), got (2, 5, 4)"),
    (distmat, (PLANE, PLANE, PLANE, PLANE), {"chain_breaks": f(B, 4)}, E,
     "chain_breaks must have shape (2, 5) to match d_cb (2, 5, 5), got (2, 4)"),
    (distmat, (PLANE, PLANE, PLANE, PLANE), {"lengths": f(3)}, E,
     "lengths must have shape (2,) to match d_cb (2, 5, 5), got (3,)"),
    (ops.check_distmat_size, (65536, 5), {}, E, "at most 65535 structures per call, got 65536"),
    (distmat, (meta(1, 15447, 15447),) * 4, {}, E, "L = 15447 is too long (9 L^2 must stay below 2^31)"),
    # ---- check_floyd_warshall_shape
    (fw, (PLANE, 0), {}, E, "G must be >= 1, got 0"),
    (fw, (f(B, N, 4),), {}, E, "D must have shape (batch, 1, 1, L, L) or (batch, L, L), got (2, 5, 4)"),
    (fw, (PLANE, 3), {}, E, "D must have shape (batch, 3, 3, L, L), got (2, 5, 5)"),
    (fw, (meta(65536, 2, 2),), {}, E, "at most 65535 structures per call, got 65536"),
    (fw, (meta(1, 46341, 46341),), {}, E, "46341 nodes are too many ((G L)^2 must stay below 2^31)"),
    # ---- check_lengths
    (ops.check_lengths, ([1, 2, 3], B, N), {}, E, "lengths must have shape (2,), got (3,)"),
    (ops.check_lengths, (i64(3), B, N), {}, E, "lengths must have shape (2,), got (3,)"),
    (ops.check_lengths, ([1, 6], B, N), {}, E, "lengths must lie in 0 .. 5, got [1, 6]"),
    (ops.check_lengths, ([-1, 5], B, N), {}, E, "lengths must lie in 0 .. 5, got [-1, 5]"),
    # ---- check_smacof_shapes
    (smacof, (PLANE,), {"max_iter": 0}, E, "max_iter must be an integer >= 1, got 0"),
    (smacof, (PLANE,), {"max_iter": True}, E, "max_iter must be an integer >= 1, got True"),
    (smacof, (PLANE,), {"eps": -1.0}, E, "eps must be >= 0, got -1.0"),
    (smacof, (PLANE,), {"eps": float("nan")}, E, "eps must be >= 0, got nan"),
    (smacof, (PLANE,), {"n_init": 0}, E, "n_init must be an integer >= 1, got 0"),
    (smacof, (PLANE,), {"init": f(B, 1, 4, 3)}, E, "init must have shape (2, n_init, 5, 3), got (2, 1, 4, 3)"),
    (smacof, (PLANE,), {"init": f(B, 2, N, 3), "n_init": 3}, E, "init holds 2 starts, n_init = 3"),
    (smacof, (PLANE,), {"init": f(B, 0, N, 3)}, E, "init must hold at least one start"),
    (smacof, (PLANE,), {"lengths": [1, 2, 3]}, E, "lengths must have shape (2,), got (3,)"),
    (smacof, (PLANE,), {"n_init": 65536}, E, "2 x 65536 starts of 5 nodes are too many for one call"),
    # ---- check_backbone_coords_shape
    (ops.check_backbone_coords_shape, (f(B, 5, N, 3),), {}, E,
     "coordinates must have shape (batch, 3, L, 3), got (2, 5, 5, 3)"),
    (ops.check_backbone_coords_shape, (meta(65536, 3, N, 3),), {}, E, "at most 65535 structures per call, got 65536"),
    # ---- check_frames_backward_shapes
    (frames_bw, (f(B, N, A), 0, 1, 2), {"grad_trans": TRANS}, E,
     "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (frames_bw, (XYZ_INT, 0, 1, 2), {"grad_trans": TRANS}, E, "xyz must be a floating-point tensor, got torch.int64"),
    (frames_bw, (XYZ, 0, 1, 2), {}, E, "at least one of grad_rot and grad_trans is required"),
    (frames_bw, (XYZ, 0, 1, 2), {"grad_rot": f(B, N, 3)}, E,
     "grad_rot must have shape (2, 5, 3, 3) to match xyz (2, 5, 5, 3), got (2, 5, 3)"),
    (frames_bw, (XYZ, 0, 1, 2), {"grad_rot": i64(B, N, 3, 3)}, E,
     "grad_rot must be a floating-point tensor, got torch.int64"),
    (frames_bw, (XYZ, 0, 1, 5), {"grad_rot": ROT}, E, "atom slot 5 outside [0, 5)"),
    (frames_bw, (XYZ, 0, 1, 2), {"grad_trans": f(B, N, 2)}, E,
     "grad_trans must have shape (2, 5, 3) to match xyz (2, 5, 5, 3), got (2, 5, 2)"),
    (frames_bw, (XYZ, 0, 1, 2, -1), {"grad_trans": TRANS}, E, "atom slot -1 outside [0, 5)"),
    (frames_bw, (XYZ, 0, 1, 2), {"grad_trans": TRANS, "residue_mask": f(B, 4)}, E,
     "residue_mask must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (frames_bw, (XYZ, 0, 1, 2), {"grad_trans": TRANS, "out": f(B, N, A, 2)}, E,
     "out must be a contiguous float32 tensor of shape (2, 5, 5, 3)"),
    # ---- check_fape_shapes
    (fape, (f(B, N, 3, 2),) + FAPE[1:], {}, E, "rot must have shape (batch, frames, 3, 3), got (2, 5, 3, 2)"),
    (fape, (ROT, TRANS, f(3, M, 3), ROT, TRANS, PTS), {}, E, "points must have shape (2, points, 3), got (3, 5, 3)"),
    (fape, (meta(65536, 1, 3, 3), TRANS, meta(65536, M, 3), ROT, TRANS, PTS), {}, E,
     "at most 65535 structures per call, got 65536"),
    (fape, (meta(B, 2 ** 30 + 1, 3, 3),) + FAPE[1:], {}, E,
     "at most 2^30 frames and points per structure, got 1073741825 and 5"),
    (fape, (ROT, TRANS, meta(B, 2 ** 30 + 1, 3), ROT, TRANS, PTS), {}, E,
     "at most 2^30 frames and points per structure, got 5 and 1073741825"),
    (fape, (ROT, f(B, N, 2)) + FAPE[2:], {}, E,
     "trans must have shape (2, 5, 3) to match rot (2, 5, 3, 3) and points (2, 5, 3), got (2, 5, 2)"),
    (fape, FAPE[:5] + (f(B, 4, 3),), {}, E,
     "target_points must have shape (2, 5, 3) to match rot (2, 5, 3, 3) and points (2, 5, 3), got (2, 4, 3)"),
    (fape, FAPE[:3] + (i64(B, N, 3, 3),) + FAPE[4:], {}, E, "target_rot must be a floating-point tensor, got torch.int64"),
    (fape, FAPE + (f(B, 4),), {}, E, "frame_mask must have shape (2, 5), got (2, 4)"),
    (fape, FAPE + (None, f(B, 4)), {}, E, "point_mask must have shape (2, 5), got (2, 4)"),
    (fape, FAPE, {"clamp": f(3)}, E, "clamp must have shape (2,) to match rot (2, 5, 3, 3), got (3,)"),
    (fape, FAPE, {"clamp": i64(B)}, E, "clamp must be a floating-point tensor, got torch.int64"),
    (fape, FAPE, {"clamp": f(B)}, E, "clamp must be positive (inf = unclamped)"),
    (fape, FAPE, {"clamp": 0.0}, E, "clamp must be positive (inf = unclamped), got 0.0"),
    (fape, FAPE, {"scale": 0}, E, "scale must be positive and finite, got 0"),
    (fape, FAPE, {"scale": float("inf")}, E, "scale must be positive and finite, got inf"),
    (fape, FAPE, {"eps": -1e-4}, E, "eps must be non-negative and finite, got -0.0001"),
    (fape, FAPE, {"eps": float("inf")}, E, "eps must be non-negative and finite, got inf"),
    (fape, FAPE, {"grad_loss": f(3)}, E, "grad_loss must have shape (2,) to match rot (2, 5, 3, 3), got (3,)"),
    (fape, FAPE[:5] + (meta(B, M, 3),), {}, E, "`target_points` lives on meta, the coordinates on cpu"),
    # ---- check_lddt_shapes
    (lddt, (f(B, M), f(B, M)), {}, E, "points must have shape (batch, points, 3), got (2, 5)"),
    (lddt, (meta(65536, M, 3),) * 2, {}, E, "at most 65535 structures per call, got 65536"),
    (lddt, (meta(B, 2 ** 30 + 1, 3),) * 2, {}, E, "at most 2^30 points per structure, got 1073741825"),
    (lddt, (i64(B, M, 3), PTS), {}, E, "points must be a floating-point tensor, got torch.int64"),
    (lddt, (PTS, f(B, 4, 3)), {}, E, "target_points must have shape (2, 5, 3) to match points (2, 5, 3), got (2, 4, 3)"),
    (lddt, (PTS, PTS, f(B, 4)), {}, E, "point_mask must have shape (2, 5), got (2, 4)"),
    (lddt, (PTS, PTS, None, i64(B, 4)), {}, E, "groups must have shape (2, 5), got (2, 4)"),
    (lddt, (PTS, PTS, None, f(B, M)), {}, E, "groups must be an integer tensor, got torch.float32"),
    (lddt, (PTS, PTS, None, b8(B, M)), {}, E, "groups must be an integer tensor, got torch.bool"),
    (lddt, (PTS, PTS), {"cutoff": 0.0}, E, "cutoff must be positive and finite, got 0.0"),
    (lddt, (PTS, PTS), {"cutoff": float("inf")}, E, "cutoff must be positive and finite, got inf"),
    (lddt, (PTS, PTS), {"cutoff": float("nan")}, E, "cutoff must be positive and finite, got nan"),
    (lddt, (PTS, PTS), {"thresholds": ()}, E, "between 1 and 8 thresholds, got 0"),
    (lddt, (PTS, PTS), {"thresholds": (1.0, 1.0)}, E,
     "thresholds must be strictly increasing and in (0, 64.0], got (1.0, 1.0)"),
    (lddt, (PTS, PTS), {"thresholds": (1.0, 65.0)}, E,
     "thresholds must be strictly increasing and in (0, 64.0], got (1.0, 65.0)"),
    (lddt, (PTS, PTS), {"eps": -1.0}, E, "eps must be non-negative and finite, got -1.0"),
    (lddt, (PTS, PTS), {"eps": float("nan")}, E, "eps must be non-negative and finite, got nan"),
    (lddt, (PTS, PTS), {"grad_S": f(B, 4)}, E, "grad_S must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (lddt, (PTS, PTS), {"grad_S": i64(B, M)}, E, "grad_S must be a floating-point tensor, got torch.int64"),
    (lddt, (PTS, PTS, meta(B, M)), {}, E, "`point_mask` lives on meta, the coordinates on cpu"),
    # ---- check_clash_shapes
    (clash, (f(B, M, 2), RAD), {}, E, "points must have shape (batch, points, 3), got (2, 5, 2)"),
    (clash, (meta(65536, M, 3), meta(65536, M)), {}, E, "at most 65535 structures per call, got 65536"),
    (clash, (meta(B, 2 ** 30 + 1, 3), meta(B, 2 ** 30 + 1)), {}, E, "at most 2^30 points per structure, got 1073741825"),
    (clash, (PTS.to(torch.int32), RAD), {}, E, "points must be a floating-point tensor, got torch.int32"),
    (clash, (PTS, f(B, 4)), {}, E, "radius must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (clash, (PTS, i64(B, M)), {}, E, "radius must be a floating-point tensor, got torch.int64"),
    (clash, (PTS, RAD, f(B, 4)), {}, E, "point_mask must have shape (2, 5), got (2, 4)"),
    (clash, (PTS, RAD, None, i64(B, 4)), {}, E, "groups must have shape (2, 5), got (2, 4)"),
    (clash, (PTS, RAD, None, None, i64(B, 4)), {}, E, "link must have shape (2, 5), got (2, 4)"),
    (clash, (PTS, RAD, None, f(B, M)), {}, E, "groups must be an integer tensor, got torch.float32"),
    (clash, (PTS, RAD, None, None, b8(B, M)), {}, E, "link must be an integer tensor, got torch.bool"),
    (clash, (PTS, RAD), {"tolerance": float("inf")}, E, "tolerance must be finite, got inf"),
    (clash, (PTS, RAD), {"tolerance": float("nan")}, E, "tolerance must be finite, got nan"),
    (clash, (PTS, RAD), {"eps": -1.0}, E, "eps must be non-negative and finite, got -1.0"),
    (clash, (PTS, RAD), {"grad_E": f(B, 4)}, E, "grad_E must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (clash, (PTS, meta(B, M)), {}, E, "`radius` lives on meta, the coordinates on cpu"),
    # ---- _peptide_bond_constants
    (ops._peptide_bond_constants, (1e-10, {"sigma": 1.0, "l1": 2.0}), {}, E,
     "unknown peptide-bond constants ['l1', 'sigma']; the names are ['cos_cacn', 'cos_cnca', 'l0', 'l0_pro', 'sigma_cacn', "
     "'sigma_cnca', 'sigma_l', 'sigma_l_pro', 'tau']"),
    (ops._peptide_bond_constants, (1e-10, {"l0": float("nan")}), {}, E, "l0 must be finite, got nan"),
    (ops._peptide_bond_constants, (float("inf"), {}), {}, E, "eps must be finite, got inf"),
    (ops._peptide_bond_constants, (1e-10, {"sigma_l": -1.0}), {}, E, "sigma_l must be non-negative, got -1.0"),
    (ops._peptide_bond_constants, (1e-10, {"tau": -1.0}), {}, E, "tau must be non-negative, got -1.0"),
    (ops._peptide_bond_constants, (-1.0, {}), {}, E, "eps must be non-negative, got -1.0"),
    # ---- check_peptide_bond_shapes
    (bond, (f(B, N, A),), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (bond, (XYZ_INT,), {}, E, "xyz must be a floating-point tensor, got torch.int64"),
    (bond, (meta(B, 2 ** 30 + 1, A, 3),), {}, E, "at most 2^31 residues per call, got 2147483650"),
    (bond, (XYZ,), {"c_slot": 5}, E, "atom slot 5 outside [0, 5)"),
    (bond, (XYZ,), {"ca_slot": 0}, E, "the N, CA and C slots must differ, got (0, 0, 2)"),
    (bond, (XYZ, f(B, 4)), {}, E, "junction_mask must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (bond, (XYZ, None, f(B, 4)), {}, E, "next_is_proline must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (bond, (XYZ,), {"eps": -1.0}, E, "eps must be non-negative, got -1.0"),
    (bond, (XYZ,), {"l2": 1.0}, E,
     "unknown peptide-bond constants ['l2']; the names are ['cos_cacn', 'cos_cnca', 'l0', 'l0_pro', 'sigma_cacn', "
     "'sigma_cnca', 'sigma_l', 'sigma_l_pro', 'tau']"),
    (bond, (XYZ,), {"grad_viol": f(B, N, 2)}, E,
     "grad_viol must have shape (2, 5, 3) to match xyz (2, 5, 5, 3), got (2, 5, 2)"),
    (bond, (XYZ, meta(B, N)), {}, E, "`junction_mask` lives on meta, the coordinates on cpu"),
    # ---- check_dssp_shapes
    (dssp, (f(B, N, A),) + DSSP[1:], {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (dssp, (XYZ_INT,) + DSSP[1:], {}, E, "xyz must be a floating-point tensor, got torch.int64"),
    (dssp, (meta(65536, N, A, 3),) + DSSP[1:], {}, E, "at most 65535 structures per call, got 65536"),
    (dssp, (meta(B, 2 ** 24 + 1, A, 3),) + DSSP[1:], {}, E, "at most 2^24 residues per structure, got 16777217"),
    (dssp, (f(B, N, 3, 3),) + DSSP[1:], {}, E, "xyz needs slots for N, CA, C and O, got 3 atoms per residue"),
    (dssp, DSSP, {"o_slot": 5}, E, "atom slot 5 outside [0, 5)"),
    (dssp, DSSP, {"o_slot": 2}, E, "the N, CA, C and O slots must differ, got (0, 1, 2, 2)"),
    (dssp, DSSP, {"ca_slot": 7, "acceptor_idx": i64(B, N, 2)}, E, "atom slot 7 outside [0, 5)"),
    (dssp, (XYZ, None, DSSP[2]), {}, E, "complete is required"),
    (dssp, (XYZ, DSSP[1], None), {}, E, "junction is required"),
    (dssp, (XYZ, b8(B, 4), DSSP[2]), {}, E, "complete must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (dssp, (XYZ, DSSP[1], b8(B, 4)), {}, E, "junction must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (dssp, DSSP + (b8(B, 4),), {}, E, "donor must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (dssp, (meta(1, 2049, A, 3), meta(1, 2049), meta(1, 2049)), {"acceptor_idx": meta(1, 2049, 2, dtype=torch.int64)}, E,
     "at most 2048 residues per structure, got 2049"),
    (dssp, DSSP, {"acceptor_idx": i64(B, N, 3)}, E,
     "acceptor_idx must be an integer tensor of shape (2, 5, 2), got torch.int64 (2, 5, 3)"),
    (dssp, DSSP, {"acceptor_idx": f(B, N, 2)}, E,
     "acceptor_idx must be an integer tensor of shape (2, 5, 2), got torch.float32 (2, 5, 2)"),
    (dssp, (XYZ, DSSP[1], meta(B, N)), {}, E, "`junction` lives on meta, the coordinates on cpu"),
    # ---- check_sasa_shapes
    (sasa, (f(B, M, 3, 1), RAD), {}, E, "points must have shape (batch, points, 3), got (2, 5, 3, 1)"),
    (sasa, (meta(65536, M, 3), meta(65536, M)), {}, E, "at most 65535 structures per call, got 65536"),
    (sasa, (meta(B, 2 ** 24 + 1, 3), meta(B, 2 ** 24 + 1)), {}, E, "at most 2^24 points per structure, got 16777217"),
    (sasa, (i64(B, M, 3), RAD), {}, E, "points must be a floating-point tensor, got torch.int64"),
    (sasa, (PTS, f(B, 4)), {}, E, "radius must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (sasa, (PTS, RAD, f(B, 4)), {}, E, "point_mask must have shape (2, 5), got (2, 4)"),
    (sasa, (PTS, RAD, None, i64(B, 4)), {}, E, "isolate must have shape (2, 5), got (2, 4)"),
    (sasa, (PTS, RAD, None, f(B, M)), {}, E, "isolate must be an integer tensor, got torch.float32"),
    (sasa, (PTS, RAD), {"sphere": f(4, 3).double()}, E,
     "sphere must be a float32 tensor of shape (S, 3), got torch.float64 (4, 3)"),
    (sasa, (PTS, RAD), {"sphere": f(4, 2)}, E, "sphere must be a float32 tensor of shape (S, 3), got torch.float32 (4, 2)"),
    (sasa, (PTS, RAD), {"sphere": [[0.0, 0.0, 1.0]]}, E, "sphere must be a float32 tensor of shape (S, 3), got list ()"),
    (sasa, (PTS, RAD), {"sphere": f(0, 3)}, E, "sphere must have between 1 and 256 directions, got 0"),
    (sasa, (PTS, RAD), {"sphere": f(257, 3)}, E, "sphere must have between 1 and 256 directions, got 257"),
    (sasa, (PTS, RAD), {"probe": -0.1}, E, "probe must be non-negative and finite, got -0.1"),
    (sasa, (PTS, RAD), {"probe": float("inf")}, E, "probe must be non-negative and finite, got inf"),
    (sasa, (PTS, RAD), {"sphere": meta(4, 3)}, E, "`sphere` lives on meta, the coordinates on cpu"),
    # ---- check_rigid_shapes
    (rigid, (f(B, N, A),), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (rigid, (XYZ, f(3)), {}, E, "rotation must be (3,3), (2,3,3) or (2,5,3,3), got (3,)"),
    (rigid, (XYZ, f(3, 3, 3)), {}, E, "rotation must be (3,3), (2,3,3) or (2,5,3,3), got (3, 3, 3)"),
    (rigid, (XYZ, None, f(4, 3)), {}, E, "translation shape (4, 3) does not broadcast against xyz (2, 5, 5, 3)"),
    # ---- check_kabsch_shapes
    (kabsch, (f(B), XYZ, b8(B, N, A)), {}, E, "source xyz must have shape (batch, ..., 3), got (2,)"),
    (kabsch, (XYZ, f(B, N, A, 2), b8(B, N, A)), {}, E, "target xyz must have shape (batch, ..., 3), got (2, 5, 5, 2)"),
    (kabsch, (XYZ, f(B, N, 4, 3), b8(B, N, A)), {}, E,
     "source and target must have the same number of atoms per structure, got (2, 5, 5, 3) and (2, 5, 4, 3)"),
    (kabsch, (XYZ, f(3, N, A, 3), b8(B, N, A)), {}, E,
     "the target must have the batch size of the source (2) or 1, got 3"),
    (kabsch, (XYZ, XYZ, b8(3, N, A)), {}, E, "atom_mask must have the batch size of the source (2) or 1, got 3"),
    (kabsch, (XYZ, XYZ, b8(B, N, 4)), {}, E,
     "atom_mask must have 25 entries per structure, got (2, 5, 4) against source (2, 5, 5, 3)"),
    # ---- check_min_dist_shapes
    (min_dist, (XYZ, PTS), {}, E, "xyz must be one structure of shape (residues, atoms, 3), got (2, 5, 5, 3)"),
    (min_dist, (f(N, A, 3), f(M, 2)), {}, E, "query_xyz must have shape (..., 3), got (5, 2)"),
    (min_dist, (f(N, A, 3), f(0, 3)), {}, E, "query_xyz holds no point: the nearest of no points is undefined"),
    (min_dist, (f(N, A, 3), PTS, 5), {}, E, "atom slot 5 outside [0, 5)"),
    # ---- geometry: the reduction is checked before anything is launched
    (geometry.lddt, (PTS, PTS), {"reduction": "mean"}, E, "reduction must be 'point', 'structure' or 'none', got 'mean'"),
    (geometry.steric_clash, (PTS, RAD), {"reduction": None}, E,
     "reduction must be 'point', 'structure' or 'none', got None"),
    # ---- check_knn_shapes
    (knn, (f(B, M), 3), {}, E, "points must have shape (batch, points, 3), got (2, 5)"),
    (knn, (meta(65536, M, 3), 3), {}, E, "at most 65535 structures per call, got 65536"),
    (knn, (meta(B, 2 ** 24 + 1, 3), 3), {}, E, "at most 2^24 points per structure, got 16777217"),
    (knn, (i64(B, M, 3), 3), {}, E, "points must be a floating-point tensor, got torch.int64"),
    (knn, (PTS, 0), {}, E, "k must be an integer in 1 .. 64, got 0"),
    (knn, (PTS, 65), {}, E, "k must be an integer in 1 .. 64, got 65"),
    (knn, (PTS, True), {}, E, "k must be an integer in 1 .. 64, got True"),
    (knn, (PTS, 3.0), {}, E, "k must be an integer in 1 .. 64, got 3.0"),
    (knn, (PTS, 3), {"cutoff": 0.0}, E, "cutoff must be positive and finite, got 0.0"),
    (knn, (PTS, 3), {"cutoff": float("nan")}, E, "cutoff must be positive and finite, got nan"),
    (knn, (PTS, 3, f(B, 4)), {}, E, "point_mask must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (knn, (PTS, 3), {"exclude": i64(B, 4)}, E, "exclude must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (knn, (PTS, 3), {"exclude": f(B, M)}, E, "exclude must be an integer tensor, got torch.float32"),
    (knn, (PTS, 3), {"query_mask": b8(B, M)}, E,
     "query_mask needs queries: in the self graph the points' own mask and keys are used"),
    (knn, (PTS, 3), {"query_exclude": i64(B, M)}, E,
     "query_exclude needs queries: in the self graph the points' own mask and keys are used"),
    (knn, (PTS, 3), {"queries": f(B, Q)}, E, "queries must have shape (2, queries, 3) to match points (2, 5, 3), got (2, 4)"),
    (knn, (PTS, 3), {"queries": f(B, Q, 2)}, E,
     "queries must have shape (2, queries, 3) to match points (2, 5, 3), got (2, 4, 2)"),
    (knn, (PTS, 3), {"queries": f(3, Q, 3)}, E,
     "queries must have shape (2, queries, 3) to match points (2, 5, 3), got (3, 4, 3)"),
    (knn, (PTS, 3), {"queries": i64(B, Q, 3)}, E, "queries must be a floating-point tensor, got torch.int64"),
    (knn, (PTS, 3), {"queries": meta(B, 2 ** 24 + 1, 3)}, E, "at most 2^24 queries per structure, got 16777217"),
    (knn, (PTS, 3), {"queries": QRY, "query_mask": b8(B, M)}, E,
     "query_mask must have shape (2, 4) to match queries (2, 4, 3), got (2, 5)"),
    (knn, (PTS, 3), {"queries": QRY, "exclude": i64(B, M), "query_exclude": i64(B, M)}, E,
     "query_exclude must have shape (2, 4) to match queries (2, 4, 3), got (2, 5)"),
    (knn, (PTS, 3), {"queries": QRY, "exclude": i64(B, M), "query_exclude": f(B, Q)}, E,
     "query_exclude must be an integer tensor, got torch.float32"),
    (knn, (PTS, 3), {"queries": QRY, "exclude": i64(B, M)}, E, TOGETHER),
    (knn, (PTS, 3), {"queries": QRY, "query_exclude": i64(B, Q)}, E, TOGETHER),
    (knn, (PTS, 3), {"queries": QRY, "include_self": True}, E, "include_self applies to the self graph only (queries=None)"),
    (knn, (PTS, 3, meta(B, M)), {}, E, "`point_mask` lives on meta, the coordinates on cpu"),
    (knn, (PTS, 3), {"queries": meta(B, Q, 3)}, E, "`queries` lives on meta, the coordinates on cpu"),
    # ---- check_closest_atoms_shapes
    (closest, (f(B, N, A),), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (closest, (XYZ_INT,), {}, E, "xyz must be a floating-point tensor, got torch.int64"),
    (closest, (meta(65536, N, A, 3),), {}, E, "at most 65535 structures per call, got 65536"),
    (closest, (f(B, 0, A, 3),), {}, E, "1 .. 2^20 residues per structure, got 0"),
    (closest, (meta(B, 2 ** 20 + 1, A, 3),), {}, E, "1 .. 2^20 residues per structure, got 1048577"),
    (closest, (f(B, N, 0, 3),), {}, E, "1 .. 64 atom slots per residue, got 0"),
    (closest, (f(B, N, 65, 3),), {}, E, "1 .. 64 atom slots per residue, got 65"),
    (closest, (XYZ, f(B, N, 4)), {}, E, "atom_mask must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (closest, (XYZ, None, -1.0), {}, E, "cutoff must be non-negative and finite, got -1.0"),
    (closest, (XYZ, None, float("nan")), {}, E, "cutoff must be non-negative and finite, got nan"),
    (closest, (XYZ, None, float("-inf")), {}, E, "cutoff must be non-negative and finite, got -inf"),
    (closest, (XYZ,), {"pair": i64(B, N, 4)}, E, "pair must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (closest, (XYZ,), {"pair": PLANE}, E, "pair must be an integer tensor, got torch.float32"),
    (closest, (XYZ,), {"grad_dist": f(B, N, 4)}, E,
     "grad_dist must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (closest, (XYZ,), {"grad_dist": i64(B, N, N)}, E, "grad_dist must be a floating-point tensor, got torch.int64"),
    (closest, (XYZ, meta(B, N, A)), {}, E, "`atom_mask` lives on meta, the coordinates on cpu"),
    # ---- _check_breaks
    (ops._check_breaks, ("abc",), {}, E, "breaks must be a sequence of numbers"),
    (ops._check_breaks, ([[2.0, 4.0]],), {}, E, "breaks must be one-dimensional, got shape (1, 2)"),
    (ops._check_breaks, ((),), {}, E, "1 .. 127 breaks, got 0"),
    (ops._check_breaks, (np.arange(128.0),), {}, E, "1 .. 127 breaks, got 128"),
    (ops._check_breaks, ((2.0, float("inf")),), {}, E, "breaks must be finite, non-negative and strictly increasing"),
    (ops._check_breaks, ((2.0, float("nan")),), {}, E, "breaks must be finite, non-negative and strictly increasing"),
    (ops._check_breaks, ((-1.0, 2.0),), {}, E, "breaks must be finite, non-negative and strictly increasing"),
    (ops._check_breaks, ((2.0, 2.0),), {}, E, "breaks must be finite, non-negative and strictly increasing"),
    # ---- check_pair_bins_shapes
    (pair_bins, (f(B, N), BREAKS), {}, E, "points must have shape (batch, residues, 3), got (2, 5)"),
    (pair_bins, (f(B, N, 2), BREAKS), {}, E, "points must have shape (batch, residues, 3), got (2, 5, 2)"),
    (pair_bins, (i64(B, N, 3), BREAKS), {}, E, "points must be a floating-point tensor, got torch.int64"),
    (pair_bins, (meta(65536, N, 3), BREAKS), {}, E, "at most 65535 structures per call, got 65536"),
    (pair_bins, (f(B, 0, 3), BREAKS), {}, E, "1 .. 2^20 residues per structure, got 0"),
    (pair_bins, (meta(B, 2 ** 20 + 1, 3), BREAKS), {}, E, "1 .. 2^20 residues per structure, got 1048577"),
    (pair_bins, (PTS, ()), {}, E, "1 .. 127 breaks, got 0"),
    (pair_bins, (PTS, (4.0, 2.0)), {}, E, "breaks must be finite, non-negative and strictly increasing"),
    (pair_bins, (PTS, BREAKS, f(B, 4)), {}, E, "row_mask must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (pair_bins, (PTS, BREAKS, None, f(B, 4)), {}, E, "col_mask must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (pair_bins, (PTS, BREAKS, None, None, f(B, N, 3)) + PAIR_FRAMES[1:], {}, E,
     "rot must have shape (2, 5, 3, 3) to match points (2, 5, 3), got (2, 5, 3)"),
    (pair_bins, (PTS, BREAKS, None, None, ROT, f(B, N, 2)) + PAIR_FRAMES[2:], {}, E,
     "trans must have shape (2, 5, 3) to match points (2, 5, 3), got (2, 5, 2)"),
    (pair_bins, (PTS, BREAKS, None, None, ROT, TRANS, i64(B, N, 3, 3)) + PAIR_FRAMES[3:], {}, E,
     "target_rot must be a floating-point tensor, got torch.int64"),
    (pair_bins, (PTS, BREAKS, None, None, ROT, TRANS, ROT, f(B, 4, 3), PTS), {}, E,
     "target_trans must have shape (2, 5, 3) to match points (2, 5, 3), got (2, 4, 3)"),
    (pair_bins, (PTS, BREAKS, None, None, ROT, TRANS, ROT, TRANS, f(B, N)), {}, E,
     "target_points must have shape (2, 5, 3) to match points (2, 5, 3), got (2, 5)"),
    (pair_bins, (PTS, BREAKS, None, meta(B, N)), {}, E, "`col_mask` lives on meta, the coordinates on cpu"),
    (pair_bins, (PTS, BREAKS, None, None, ROT, TRANS, ROT, TRANS, meta(B, N, 3)), {}, E,
     "`target_points` lives on meta, the coordinates on cpu"),
    # ---- check_binned_shapes
    (binned, (f(B, N, N),), {}, E, "logits must have shape (batch, residues, residues, bins), got (2, 5, 5)"),
    (binned, (f(B, N, 4, 4),), {}, E, "logits must have shape (batch, residues, residues, bins), got (2, 5, 4, 4)"),
    (binned, (i64(B, N, N, 4),), {}, E, "logits must be a floating-point tensor, got torch.int64"),
    (binned, (meta(65536, 1, 1, 4),), {}, E, "at most 65535 structures per call, got 65536"),
    (binned, (f(B, 0, 0, 4),), {}, E, "1 .. 2^20 residues per structure, got 0"),
    (binned, (meta(1, 2 ** 20 + 1, 2 ** 20 + 1, 4),), {}, E, "1 .. 2^20 residues per structure, got 1048577"),
    (binned, (f(B, N, N, 1),), {}, E, "2 .. 128 bins, got 1"),
    (binned, (f(B, N, N, 129),), {}, E, "2 .. 128 bins, got 129"),
    (binned, (LOGITS, i64(B, N, 4)), {}, E, "bins must have shape (2, 5, 5) to match logits (2, 5, 5, 4), got (2, 5, 4)"),
    (binned, (LOGITS, PLANE), {}, E, "bins must be an integer tensor, got torch.float32"),
    (binned, (LOGITS, None, f(B, 4)), {}, E, "grad_row must have shape (2, 5) to match logits (2, 5, 5, 4), got (2, 4)"),
    (binned, (LOGITS, None, i64(B, N)), {}, E, "grad_row must be a floating-point tensor, got torch.int64"),
    (binned, (LOGITS,), {"values": f(B, 4)}, E, "values must have shape (2, tables, 4) to match logits (2, 5, 5, 4), got (2, 4)"),
    (binned, (LOGITS,), {"values": f(3, 2, 4)}, E,
     "values must have shape (2, tables, 4) to match logits (2, 5, 5, 4), got (3, 2, 4)"),
    (binned, (LOGITS,), {"values": f(B, 2, 3)}, E,
     "values must have shape (2, tables, 4) to match logits (2, 5, 5, 4), got (2, 2, 3)"),
    (binned, (LOGITS,), {"values": f(B, 0, 4)}, E, "1 .. 4 value tables, got 0"),
    (binned, (LOGITS,), {"values": f(B, 5, 4)}, E, "1 .. 4 value tables, got 5"),
    (binned, (LOGITS,), {"values": i64(B, 2, 4)}, E, "values must be a floating-point tensor, got torch.int64"),
    (binned, (LOGITS, meta(B, N, N, dtype=torch.int64)), {}, E, "`bins` lives on meta, the coordinates on cpu"),
    # ---- check_superpose_shapes
    (superpose, (f(B, M), PTS), {}, E, "a must have shape (batch, points, 3), got (2, 5)"),
    (superpose, (f(B, M, 2), PTS), {}, E, "a must have shape (batch, points, 3), got (2, 5, 2)"),
    (superpose, (i64(B, M, 3), PTS), {}, E, "a must be a floating-point tensor, got torch.int64"),
    (superpose, (meta(65536, 1, 3),) * 2, {}, E, "at most 65535 structures per call, got 65536"),
    (superpose, (f(B, 0, 3),) * 2, {}, E, "1 .. any number of points per structure, got 0"),
    (superpose, (f(B, 0, 3),) * 2, {"max_points": 2048}, E, "1 .. 2048 points per structure, got 0"),
    (superpose, (f(B, 2049, 3),) * 2, {"max_points": 2048}, E, "1 .. 2048 points per structure, got 2049"),
    (superpose, (PTS, f(B, 4, 3)), {}, E, "b must have shape (2, 5, 3) or (1, 5, 3) to match a, got (2, 4, 3)"),
    (superpose, (PTS, f(3, M, 3)), {}, E, "b must have shape (2, 5, 3) or (1, 5, 3) to match a, got (3, 5, 3)"),
    (superpose, (PTS, i64(B, M, 3)), {}, E, "b must be a floating-point tensor, got torch.int64"),
    (superpose, (PTS, PTS, f(B, 4)), {}, E, "weight must have shape (2, 5) to match a (2, 5, 3), got (2, 4)"),
    (superpose, (PTS, PTS, i64(B, M)), {}, E, "weight must be a floating-point tensor, got torch.int64"),
    (superpose, (PTS, PTS, None, f(B, 4)), {}, E, "mask must have shape (2, 5) to match a (2, 5, 3), got (2, 4)"),
    (superpose, (PTS, PTS), {"grad_rmsd": f(3)}, E, "grad_rmsd must have shape (2,) to match a (2, 5, 3), got (3,)"),
    (superpose, (PTS, PTS), {"grad_rmsd": i64(B)}, E, "grad_rmsd must be a floating-point tensor, got torch.int64"),
    (superpose, (PTS, PTS), {"l_norm": f(B, 1)}, E, "l_norm must have shape (2,) to match a (2, 5, 3), got (2, 1)"),
    (superpose, (PTS, PTS), {"l_norm": i64(B)}, E, "l_norm must be a floating-point tensor, got torch.int64"),
    (superpose, (PTS, meta(B, M, 3)), {}, E, "`b` lives on meta, the coordinates on cpu"),
    # ---- _check_objectives
    (ops._check_objectives, ([],), {}, E, "1 .. 8 objectives, got 0"),
    (ops._check_objectives, ([(0, 1.0)] * 9,), {}, E, "1 .. 8 objectives, got 9"),
    (ops._check_objectives, ([(0, 1.0), (2, 1.0)],), {}, E,
     "an objective's kind is SUPERPOSE_TM (0) or SUPERPOSE_COUNT (1), got 2"),
    (ops._check_objectives, ([(0, 0.0)],), {}, E, "an objective's param must be positive and finite, got 0.0"),
    (ops._check_objectives, ([(1, float("inf"))],), {}, E, "an objective's param must be positive and finite, got inf"),
    # ---- check_structalign_shapes
    (structalign, (f(B, M), QRY), {}, E, "a must have shape (batch, points, 3), got (2, 5)"),
    (structalign, (PTS, f(B, Q, 2)), {}, E, "b must have shape (batch, points, 3), got (2, 4, 2)"),
    (structalign, (i64(B, M, 3), QRY), {}, E, "a must be a floating-point tensor, got torch.int64"),
    (structalign, (PTS, i64(B, Q, 3)), {}, E, "b must be a floating-point tensor, got torch.int64"),
    (structalign, (f(B, 0, 3), QRY), {}, E, "1 .. 1024 points per structure, got 0 in a"),
    (structalign, (PTS, f(B, 1025, 3)), {}, E, "1 .. 1024 points per structure, got 1025 in b"),
    (structalign, (meta(65536, 1, 3),) * 2, {}, E, "at most 65535 structures per call, got 65536"),
    (structalign, (PTS, f(3, Q, 3)), {}, E, "b must have the batch size of a, 2, got 3"),
    (structalign, (PTS, QRY, f(B, Q)), {}, E, "mask_a must have shape (2, 5) to match a (2, 5, 3), got (2, 4)"),
    (structalign, (PTS, QRY, None, f(B, M)), {}, E, "mask_b must have shape (2, 4) to match b (2, 4, 3), got (2, 5)"),
    (structalign, (PTS, QRY), {"d0": f(3)}, E, "d0 must have shape (2,) to match a (2, 5, 3), got (3,)"),
    (structalign, (PTS, QRY), {"d0": i64(B)}, E, "d0 must be a floating-point tensor, got torch.int64"),
    (structalign, (PTS, QRY, None, meta(B, Q)), {}, E, "`mask_b` lives on meta, the coordinates on cpu"),
    # ---- nw_align: its checks come before the device is asked for
    (ops.nw_align, (f(2, 5), 0.0), {}, E, "score must have shape (batch, rows, columns), got (2, 5)"),
    (ops.nw_align, (i64(B, M, Q), 0.0), {}, E, "score must be a floating-point tensor, got torch.int64"),
    (ops.nw_align, (meta(65536, 1, 1), 0.0), {}, E, "at most 65535 structures per call, got 65536"),
    (ops.nw_align, (f(B, 0, Q), 0.0), {}, E, "1 .. 1024 rows and columns, got 0 x 4"),
    (ops.nw_align, (f(B, M, 1025), 0.0), {}, E, "1 .. 1024 rows and columns, got 5 x 1025"),
    (ops.nw_align, (SCORE, 1.0), {}, E, "gap must be <= 0 and finite, got 1.0"),
    (ops.nw_align, (SCORE, float("-inf")), {}, E, "gap must be <= 0 and finite, got -inf"),
    (ops.nw_align, (SCORE, float("nan")), {}, E, "gap must be <= 0 and finite, got nan"),
    (ops.nw_align, (SCORE, -0.6, f(B, Q)), {}, E, "mask_a must have shape (2, 5) to match score (2, 5, 4), got (2, 4)"),
    (ops.nw_align, (SCORE, -0.6, None, f(B, M)), {}, E, "mask_b must have shape (2, 4) to match score (2, 5, 4), got (2, 5)"),
    (ops.nw_align, (SCORE, -0.6, meta(B, M)), {}, E, "`mask_a` lives on meta, the coordinates on cpu"),
    # ---- ca_secondary_structure: likewise
    (ops.ca_secondary_structure, (f(B, M),), {}, E, "points must have shape (batch, points, 3), got (2, 5)"),
    (ops.ca_secondary_structure, (meta(65536, M, 3),), {}, E, "at most 65535 structures per call, got 65536"),
    (ops.ca_secondary_structure, (f(B, 1025, 3),), {}, E, "at most 2^10 points per structure, got 1025"),
    (ops.ca_secondary_structure, (i64(B, M, 3),), {}, E, "points must be a floating-point tensor, got torch.int64"),
    (ops.ca_secondary_structure, (f(B, 0, 3),), {}, E, "1 .. 1024 points per structure, got 0"),
    (ops.ca_secondary_structure, (PTS, f(B, 4)), {}, E, "mask must have shape (2, 5) to match points (2, 5, 3), got (2, 4)"),
    (ops.ca_secondary_structure, (PTS, meta(B, M)), {}, E, "`mask` lives on meta, the coordinates on cpu"),
    # ---- check_rmsd_matrix_shapes
    (rmsd_matrix, (f(B, M),), {}, E, "a must have shape (batch, points, 3), got (2, 5)"),
    (rmsd_matrix, (f(B, M, 2),), {}, E, "a must have shape (batch, points, 3), got (2, 5, 2)"),
    (rmsd_matrix, (i64(B, M, 3),), {}, E, "a must be a floating-point tensor, got torch.int64"),
    (rmsd_matrix, (f(3, 0, 3),), {}, E, "1 .. 2147483631 points per structure, got 0"),
    (rmsd_matrix, (meta(B, 2 ** 31 - 16, 3),), {}, E, "1 .. 2147483631 points per structure, got 2147483632"),
    (rmsd_matrix, (PTS, None, None, b8(B, M)), {}, E, "mask_b needs a b: in self mode (b None) mask_a serves both sides"),
    (rmsd_matrix, (PTS, f(3, M)), {}, E, "b must have shape (batch, 5, 3) to match a (2, 5, 3), got (3, 5)"),
    (rmsd_matrix, (PTS, f(3, Q, 3)), {}, E, "b must have shape (batch, 5, 3) to match a (2, 5, 3), got (3, 4, 3)"),
    (rmsd_matrix, (PTS, i64(3, M, 3)), {}, E, "b must be a floating-point tensor, got torch.int64"),
    (rmsd_matrix, (meta(65536, 1, 3),), {}, E, "at most 65535 structures per call, got 65536"),
    (rmsd_matrix, (f(B, 1, 3), meta(65537, 1, 3)), {}, E, "at most 65535 structures per call, got 65537"),
    (rmsd_matrix, (PTS, None, f(B, 4)), {}, E, "mask_a must have shape (2, 5) to match a (2, 5, 3), got (2, 4)"),
    (rmsd_matrix, (PTS, f(3, M, 3), None, f(B, M)), {}, E, "mask_b must have shape (3, 5) to match b (3, 5, 3), got (2, 5)"),
    (rmsd_matrix, (PTS, meta(3, M, 3)), {}, E, "`b` lives on meta, the coordinates on cpu"),
    # ---- check_cluster_shapes
    (cluster, (f(B, N), 1.0), {}, E, "D must have shape (matrices, items, items), got (2, 5)"),
    (cluster, (f(B, N, 4), 1.0), {}, E, "D must have shape (matrices, items, items), got (2, 5, 4)"),
    (cluster, (i64(B, N, N), 1.0), {}, E, "D must be a floating-point tensor, got torch.int64"),
    (cluster, (meta(65536, 2, 2), 1.0), {}, E, "at most 65535 matrices per call, got 65536"),
    (cluster, (f(B, 0, 0), 1.0), {}, E, "1 .. 4096 items per matrix, got 0"),
    (cluster, (meta(1, 4097, 4097), 1.0), {}, E, "1 .. 4096 items per matrix, got 4097"),
    (cluster, (PLANE, float("nan")), {}, E, "cutoff must be finite, got nan"),
    (cluster, (PLANE, float("inf")), {}, E, "cutoff must be finite, got inf"),
    (cluster, (PLANE, 1.0, f(B, 4)), {}, E, "valid must have shape (2, 5) to match D (2, 5, 5), got (2, 4)"),
    (cluster, (PLANE, 1.0, meta(B, N)), {}, E, "`valid` lives on meta, the coordinates on cpu"),
    # ---- _check_neighbor_idx
    (ops._check_neighbor_idx, (i64(B, N), B, N, LIKE), {}, E, "idx must have shape (2, 5, k) to match xyz (2, 5, 5, 3), got (2, 5)"),
    (ops._check_neighbor_idx, (i64(B, 4, 3), B, N, LIKE), {}, E,
     "idx must have shape (2, 5, k) to match xyz (2, 5, 5, 3), got (2, 4, 3)"),
    (ops._check_neighbor_idx, (f(B, N, 3), B, N, LIKE), {}, E, "idx must be an integer tensor, got torch.float32"),
    (ops._check_neighbor_idx, (b8(B, N, 3), B, N, LIKE), {}, E, "idx must be an integer tensor, got torch.bool"),
    (ops._check_neighbor_idx, (i64(B, N, 0), B, N, LIKE), {}, E, "idx must hold 1 .. 64 neighbours per residue, got 0"),
    (ops._check_neighbor_idx, (i64(B, N, 65), B, N, LIKE), {}, E, "idx must hold 1 .. 64 neighbours per residue, got 65"),
    # ---- _host_f32
    (ops._host_f32, ("abc", "centers"), {}, E, "centers must be a sequence of numbers"),
    (ops._host_f32, (object(), "centers"), {}, E, "centers must be a sequence of numbers"),
    (ops._host_f32, ([[1.0]], "centers"), {}, E, "centers must be one-dimensional, got shape (1, 1)"),
    (ops._host_f32, (f(2, 2), "centers"), {}, E, "centers must be one-dimensional, got shape (2, 2)"),
    (ops._host_f32, (1.0, "centers"), {}, E, "centers must be one-dimensional, got shape ()"),
    # ---- check_edge_rbf_shapes
    (edge_rbf, (f(B, N, A), IDX), RBF, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (edge_rbf, (XYZ_INT, IDX), RBF, E, "xyz must be a floating-point tensor, got torch.int64"),
    (edge_rbf, (meta(65536, N, A, 3), IDX), RBF, E, "at most 65535 structures per call, got 65536"),
    (edge_rbf, (meta(B, 2 ** 24 + 1, A, 3), IDX), RBF, E, "at most 2^24 residues per structure, got 16777217"),
    (edge_rbf, (XYZ, i64(B, 4, 3)), RBF, E, "idx must have shape (2, 5, k) to match xyz (2, 5, 5, 3), got (2, 4, 3)"),
    (edge_rbf, (XYZ, f(B, N, 3)), RBF, E, "idx must be an integer tensor, got torch.float32"),
    (edge_rbf, (XYZ, IDX, f(B, N, 4)), RBF, E, "atom_mask must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (edge_rbf, (XYZ, IDX), {**RBF, "pair_i": 1}, E, "pair_i and pair_j must be sequences of atom slots"),
    (edge_rbf, (XYZ, IDX), {**RBF, "pair_j": (1, "CA")}, E, "pair_i and pair_j must be sequences of atom slots"),
    (edge_rbf, (XYZ, IDX), {**RBF, "pair_j": (1,)}, E,
     "pair_i and pair_j must be equally long, 1 .. 64 atom slots each, got 2 and 1"),
    (edge_rbf, (XYZ, IDX), {**RBF, "pair_i": (), "pair_j": ()}, E,
     "pair_i and pair_j must be equally long, 1 .. 64 atom slots each, got 0 and 0"),
    (edge_rbf, (XYZ, IDX), {**RBF, "pair_i": (1,) * 65, "pair_j": (1,) * 65}, E,
     "pair_i and pair_j must be equally long, 1 .. 64 atom slots each, got 65 and 65"),
    (edge_rbf, (XYZ, IDX), {**RBF, "pair_j": (1, 5)}, E, "atom slot 5 outside [0, 5)"),
    (edge_rbf, (XYZ, IDX), {**RBF, "pair_i": (-1, 4)}, E, "atom slot -1 outside [0, 5)"),
    (edge_rbf, (XYZ, IDX), {**RBF, "centers": ()}, E, "centers must hold 1 .. 64 values, got 0"),
    (edge_rbf, (XYZ, IDX), {**RBF, "centers": np.arange(65.0)}, E, "centers must hold 1 .. 64 values, got 65"),
    (edge_rbf, (XYZ, IDX), {**RBF, "centers": [[2.0, 4.0]]}, E, "centers must be one-dimensional, got shape (1, 2)"),
    (edge_rbf, (XYZ, IDX), {**RBF, "sigma": 0}, E, "sigma must be positive and finite, got 0"),
    (edge_rbf, (XYZ, IDX), {**RBF, "sigma": float("inf")}, E, "sigma must be positive and finite, got inf"),
    (edge_rbf, (XYZ, IDX), {**RBF, "want_dist": False, "want_rbf": False}, E,
     "nothing to compute: want_dist and want_rbf are both False"),
    (edge_rbf, (XYZ, meta(B, N, 3, dtype=torch.int64)), RBF, E, "`idx` lives on meta, the coordinates on cpu"),
    # ---- check_edge_frames_shapes
    (edge_frames, (f(B, N, 3, 2), TRANS, IDX), {}, E, "rot must have shape (batch, frames, 3, 3), got (2, 5, 3, 2)"),
    (edge_frames, (f(B, N, 3), TRANS, IDX), {}, E, "rot must have shape (batch, frames, 3, 3), got (2, 5, 3)"),
    (edge_frames, (meta(65536, 1, 3, 3), TRANS, IDX), {}, E, "at most 65535 structures per call, got 65536"),
    (edge_frames, (meta(B, 2 ** 24 + 1, 3, 3), TRANS, IDX), {}, E, "at most 2^24 frames per structure, got 16777217"),
    (edge_frames, (i64(B, N, 3, 3), TRANS, IDX), {}, E, "rot must be a floating-point tensor, got torch.int64"),
    (edge_frames, (ROT, f(B, N, 2), IDX), {}, E, "trans must have shape (2, 5, 3) to match rot (2, 5, 3, 3), got (2, 5, 2)"),
    (edge_frames, (ROT, i64(B, N, 3), IDX), {}, E, "trans must be a floating-point tensor, got torch.int64"),
    (edge_frames, (ROT, TRANS, i64(B, N)), {}, E, "idx must have shape (2, 5, k) to match rot (2, 5, 3, 3), got (2, 5)"),
    (edge_frames, (ROT, TRANS, i64(B, N, 65)), {}, E, "idx must hold 1 .. 64 neighbours per residue, got 65"),
    (edge_frames, (ROT, TRANS, IDX, f(B, 4)), {}, E, "frame_mask must have shape (2, 5) to match rot (2, 5, 3, 3), got (2, 4)"),
    (edge_frames, (ROT, TRANS, IDX), {"want_pos": False, "want_rot": False}, E,
     "nothing to compute: want_pos and want_rot are both False"),
    (edge_frames, (ROT, meta(B, N, 3), IDX), {}, E, "`trans` lives on meta, the coordinates on cpu"),
    # ---- _host_i32_table
    (ops._host_i32_table, ([[0, 1, 2, 3], [0, 1]], (4,), "chi_last"), {}, E,
     "chi_last must be an integer array of shape (types, 4)"),
    (ops._host_i32_table, (np.zeros((2, 3), np.int64), (4,), "chi_last"), {}, E,
     "chi_last must be an integer array of shape (types, 4), got int64 (2, 3)"),
    (ops._host_i32_table, (np.zeros(4, np.int64), (4,), "chi_last"), {}, E,
     "chi_last must be an integer array of shape (types, 4), got int64 (4,)"),
    (ops._host_i32_table, (np.zeros((2, 4)), (4,), "chi_last"), {}, E,
     "chi_last must be an integer array of shape (types, 4), got float64 (2, 4)"),
    (ops._host_i32_table, (f(2, 4, 4), (4, 4), "chi_atoms"), {}, E,
     "chi_atoms must be an integer array of shape (types, 4, 4), got float32 (2, 4, 4)"),
    (ops._host_i32_table, (np.zeros((2, 4), np.int32), (4, 4), "chi_atoms"), {}, E,
     "chi_atoms must be an integer array of shape (types, 4, 4), got int32 (2, 4)"),
    (ops._host_i32_table, (np.zeros((0, 4), np.int64), (4,), "chi_last"), {}, E, "chi_last must hold 1 .. 32 residue types, got 0"),
    (ops._host_i32_table, (np.zeros((33, 4, 4), np.int64), (4, 4), "chi_atoms"), {}, E,
     "chi_atoms must hold 1 .. 32 residue types, got 33"),
    # ---- _chi_tables
    (ops._chi_tables, (None, None, A, False), {}, E, CHI_REQUIRED),
    (ops._chi_tables, (None, LAST, A, True), {}, E, CHI_SET_REQUIRED),
    (ops._chi_tables, (ATOMS, None, A, True), {}, E, CHI_SET_REQUIRED),
    (ops._chi_tables, (chi_atoms((0, 1, 2, 5)), None, A, False), {}, E,
     "chi_atoms[0][0] = [0, 1, 2, 5] must be all -1 or four distinct atom slots in [0, 5)"),
    (ops._chi_tables, (chi_atoms(second=(1, 2, 2, 4)), None, A, False), {}, E,
     "chi_atoms[0][1] = [1, 2, 2, 4] must be all -1 or four distinct atom slots in [0, 5)"),
    (ops._chi_tables, (chi_atoms((0, 1, 2, -1)), None, A, False), {}, E,
     "chi_atoms[0][0] = [0, 1, 2, -1] must be all -1 or four distinct atom slots in [0, 5)"),
    (ops._chi_tables, (ATOMS, chi_last(types=3), A, True), {}, E, "chi_last must hold the 2 residue types of chi_atoms, got 3"),
    (ops._chi_tables, (ATOMS, chi_last(2), A, True), {}, E,
     "chi_last[0][0] = 2 must be -1, or in [d, 5) with none of a, b, c of chi_atoms[0][0] = [0, 1, 2, 3] inside [d, last]"),
    (ops._chi_tables, (ATOMS, chi_last(5), A, True), {}, E,
     "chi_last[0][0] = 5 must be -1, or in [d, 5) with none of a, b, c of chi_atoms[0][0] = [0, 1, 2, 3] inside [d, last]"),
    (ops._chi_tables, (ATOMS, chi_last(4, 4), A, True), {}, E,
     "chi_last[1][0] = 4 must be -1, or in [d, 5) with none of a, b, c of chi_atoms[1][0] = [-1, -1, -1, -1] inside [d, last]"),
    (ops._chi_tables, (chi_atoms((4, 1, 2, 3)), LAST, A, True), {}, E,
     "chi_last[0][0] = 4 must be -1, or in [d, 5) with none of a, b, c of chi_atoms[0][0] = [4, 1, 2, 3] inside [d, last]"),
    # ---- _check_residue_type
    (ops._check_residue_type, (i64(B, 4), B, N, LIKE), {}, E,
     "residue_type must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (ops._check_residue_type, (f(B, N), B, N, LIKE), {}, E, "residue_type must be an integer tensor, got torch.float32"),
    (ops._check_residue_type, (b8(B, N), B, N, LIKE), {}, E, "residue_type must be an integer tensor, got torch.bool"),
    # ---- check_chi_shapes
    (chi, (f(B, N, A), RT, None, ATOMS), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (chi, (XYZ_INT, RT, None, ATOMS), {}, E, "xyz must be a floating-point tensor, got torch.int64"),
    (chi, (meta(2 ** 16 + 1, 2 ** 15, A, 3), RT, None, ATOMS), {}, E, "at most 2^31 residues per call, got 2147516416"),
    (chi, (f(B, N, 0, 3), RT, None, ATOMS), {}, E, "1 .. 64 atom slots per residue, got 0"),
    (chi, (f(B, N, 65, 3), RT, None, ATOMS), {}, E, "1 .. 64 atom slots per residue, got 65"),
    (chi, (XYZ, i64(B, 4), None, ATOMS), {}, E, "residue_type must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (chi, (XYZ, f(B, N), None, ATOMS), {}, E, "residue_type must be an integer tensor, got torch.float32"),
    (chi, (XYZ, RT, f(B, N, 4), ATOMS), {}, E, "atom_mask must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (chi, (XYZ, RT), {}, E, CHI_REQUIRED),
    (chi, (XYZ, RT, None, chi_atoms((0, 1, 2, 5))), {}, E,
     "chi_atoms[0][0] = [0, 1, 2, 5] must be all -1 or four distinct atom slots in [0, 5)"),
    (chi, (XYZ, RT, None, np.zeros((2, 4), np.int64)), {}, E,
     "chi_atoms must be an integer array of shape (types, 4, 4), got int64 (2, 4)"),
    (chi, (XYZ, RT, None, ATOMS, f(B, N, 3)), {}, E, "grad_chi must have shape (2, 5, 4) to match xyz (2, 5, 5, 3), got (2, 5, 3)"),
    (chi, (XYZ, RT, None, ATOMS, i64(B, N, 4)), {}, E, "grad_chi must be a floating-point tensor, got torch.int64"),
    (chi, (XYZ, RT, None, ATOMS), {"want_chi": False, "want_mask": False}, E,
     "nothing to compute: want_chi and want_mask are both False"),
    (chi, (XYZ, meta(B, N, dtype=torch.int64), None, ATOMS), {}, E, "`residue_type` lives on meta, the coordinates on cpu"),
    # ---- check_chi_set_shapes
    (chi_set, (f(B, N, A), CHI, RT, None, None, ATOMS, LAST), {}, E, "xyz must have shape (batch, residues, atoms, 3), got (2, 5, 5)"),
    (chi_set, (meta(2 ** 16 + 1, 2 ** 15, A, 3), CHI, RT, None, None, ATOMS, LAST), {}, E,
     "at most 2^31 residues per call, got 2147516416"),
    (chi_set, (f(B, N, 65, 3), CHI, RT, None, None, ATOMS, LAST), {}, E, "1 .. 64 atom slots per residue, got 65"),
    (chi_set, (XYZ, f(B, N, 3), RT, None, None, ATOMS, LAST), {}, E,
     "chi must have shape (2, 5, 4) to match xyz (2, 5, 5, 3), got (2, 5, 3)"),
    (chi_set, (XYZ, i64(B, N, 4), RT, None, None, ATOMS, LAST), {}, E, "chi must be a floating-point tensor, got torch.int64"),
    (chi_set, (XYZ, CHI, i64(B, 4), None, None, ATOMS, LAST), {}, E,
     "residue_type must have shape (2, 5) to match xyz (2, 5, 5, 3), got (2, 4)"),
    (chi_set, (XYZ, CHI, RT, f(B, N, 4), None, ATOMS, LAST), {}, E,
     "atom_mask must have shape (2, 5, 5) to match xyz (2, 5, 5, 3), got (2, 5, 4)"),
    (chi_set, (XYZ, CHI, RT, None, f(B, N, 3), ATOMS, LAST), {}, E,
     "chi_select must have shape (2, 5, 4) to match xyz (2, 5, 5, 3), got (2, 5, 3)"),
    (chi_set, (XYZ, CHI, RT, None, None, ATOMS), {}, E, CHI_SET_REQUIRED),
    (chi_set, (XYZ, CHI, RT, None, None, ATOMS, chi_last(2)), {}, E,
     "chi_last[0][0] = 2 must be -1, or in [d, 5) with none of a, b, c of chi_atoms[0][0] = [0, 1, 2, 3] inside [d, last]"),
    (chi_set, (XYZ, None, RT, None, None, ATOMS, LAST, f(B, N, A, 2)), {}, E,
     "grad_out must have shape (2, 5, 5, 3) to match xyz (2, 5, 5, 3), got (2, 5, 5, 2)"),
    (chi_set, (XYZ, None, RT, None, None, ATOMS, LAST, XYZ_INT), {}, E, "grad_out must be a floating-point tensor, got torch.int64"),
    (chi_set, (XYZ, CHI, RT, None, meta(B, N, 4), ATOMS, LAST), {}, E, "`chi_select` lives on meta, the coordinates on cpu"),
]

VALID = [
    (irg, (XYZ, {"d_ca": PLANE, "phi": None}, b8(B, N, A)), {"out": f(B, N, A, 3)}, None),
    (nerf, (DIH, f(B, N), b8(B, N), DIH, DIH), {}, None),
    (nerf_bw, (XYZ, XYZ, f(B, N), b8(B, N)), {"include_cb": True, "want_bond_angles": True, "out": (DIH, DIH, None)}, None),
    (distmat, (PLANE, PLANE, PLANE, PLANE, b8(B, N, N), b8(B, N), i64(B)), {}, None),
    (ops.check_distmat_size, (65535, 15446), {}, None),
    (fw, (PLANE,), {}, (B, N)),
    (fw, (f(B, 3, 3, N, N), 3), {}, (B, N)),
    (smacof, (PLANE,), {}, (B, N, 4)),
    (smacof, (f(B, 3, 3, N, N), 3), {"init": f(B, 2, 3 * N, 3), "lengths": [5, 3]}, (B, N, 2)),
    (ops.check_backbone_coords_shape, (f(B, 3, N, 3),), {}, (B, N)),
    (frames_bw, (XYZ, 0, 1, 2), {"grad_rot": ROT, "grad_trans": TRANS, "residue_mask": b8(B, N), "out": f(B, N, A, 3)}, None),
    (fape, FAPE + (b8(B, N), b8(B, M)), {"clamp": torch.full((B,), 10.0), "grad_loss": f(B)}, None),
    (fape, FAPE, {"clamp": float("inf")}, None),
    (lddt, (PTS, PTS, b8(B, M), i64(B, M)), {"grad_S": f(B, M)}, None),
    (clash, (PTS, RAD, b8(B, M), i64(B, M), i64(B, M)), {"grad_E": f(B, M)}, None),
    (bond, (XYZ, b8(B, N), b8(B, N)), {"grad_viol": f(B, N, 3), "tau": 10.0}, None),
    (dssp, DSSP + (b8(B, N),), {}, None),
    (dssp, DSSP, {"acceptor_idx": i64(B, N, 2)}, None),
    (sasa, (PTS, RAD, b8(B, M), i64(B, M), SPHERE, 0.0), {}, None),
    (rigid, (XYZ,), {}, (0, 0)),
    (rigid, (XYZ, f(3, 3), f(3)), {}, (1, 1)),
    (rigid, (XYZ, f(B, 3, 3), f(B, 1, 3)), {}, (2, 2)),
    (rigid, (XYZ, f(B, N, 3, 3), f(B, N, 3)), {}, (3, 3)),
    (rigid, (XYZ, None, XYZ), {}, (0, 4)),
    (kabsch, (XYZ, XYZ, b8(B, N, A)), {}, (B, N * A, False, False)),
    (kabsch, (XYZ, f(1, N, A, 3), b8(N, A)), {}, (B, N * A, True, True)),
    (min_dist, (f(N, A, 3), PTS), {}, (N, A, B * M)),
    (knn, (PTS, 64, b8(B, M)), {"exclude": i64(B, M), "include_self": True}, None),
    (knn, (PTS, 3, b8(B, M)), {"queries": QRY, "query_mask": b8(B, Q), "cutoff": 8.0, **KEYS}, None),
    (closest, (XYZ, b8(B, N, A), 5.0, i64(B, N, N), PLANE), {}, None),
    (closest, (XYZ, None, 0.0), {}, None),
    (pair_bins, (PTS, BREAKS), {}, None),
    (pair_bins, (PTS, BREAKS, b8(B, N), b8(B, N)) + PAIR_FRAMES, {}, None),
    (binned, (LOGITS, i64(B, N, N), f(B, N), f(B, 2, 4)), {}, None),
    (superpose, (PTS, PTS, RAD, b8(B, M), f(B), f(B), 2048), {}, (B, M, False)),
    (superpose, (PTS, f(1, M, 3)), {}, (B, M, True)),
    (structalign, (PTS, QRY, b8(B, M), b8(B, Q), f(B)), {}, (B, M, Q)),
    (rmsd_matrix, (PTS, f(3, M, 3), b8(B, M), b8(3, M)), {}, (B, 3, M)),
    (rmsd_matrix, (PTS, None, b8(B, M)), {}, (B, B, M)),
    (cluster, (PLANE, 1.5, b8(B, N)), {}, (B, N)),
    (ops._check_neighbor_idx, (IDX, B, N, LIKE), {}, 3),
    (edge_rbf, (XYZ, IDX, b8(B, N, A)), {**RBF, "sigma": 1.5, "want_dist": False}, None),
    (edge_frames, (ROT, TRANS, IDX, b8(B, N)), {"want_rot": False}, None),
    (ops._check_residue_type, (RT, B, N, LIKE), {}, None),
    (chi, (XYZ, RT, b8(B, N, A), ATOMS, CHI), {"want_mask": False}, None),
    (chi_set, (XYZ, CHI, RT, b8(B, N, A), b8(B, N, 4), ATOMS, LAST), {}, None),
    (chi_set, (XYZ, None, RT, None, None, ATOMS, LAST, XYZ), {}, None),
    (ops.check_nw_align_shapes, (SCORE, -0.6, b8(B, M), b8(B, Q)), {}, (B, M, Q)),
    (ops.check_ca_secondary_structure_shapes, (PTS, b8(B, M)), {}, (B, M)),
]


@pytest.mark.parametrize("fn, args, kwargs, exc, message", FAULTS, ids=[f"{k}-{r[0].__name__}" for k, r in enumerate(FAULTS)])
def test_fault_message(fn, args, kwargs, exc, message):
    with pytest.raises(Exception) as info:
        fn(*args, **kwargs)
    print(f"{type(info.value).__name__}: {info.value}")
    assert type(info.value) is exc and str(info.value) == message


@pytest.mark.parametrize("fn, args, kwargs, want", VALID, ids=[f"{k}-{r[0].__name__}" for k, r in enumerate(VALID)])
def test_valid_arguments(fn, args, kwargs, want):
    assert fn(*args, **kwargs) == want


def test_check_lengths_normalises():
    assert ops.check_lengths(None, B, N) is None
    t = i64(B)
    assert ops.check_lengths(t, B, N) is t
    got = ops.check_lengths([5, 0], B, N)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [5, 0]
    assert ops.check_lengths(3, 1, N).tolist() == [3]


def test_host_tables_normalise():
    """what the helpers that take a host table hand to the launchers"""
    breaks = ops._check_breaks(torch.tensor(BREAKS, dtype=torch.float64))
    assert breaks.dtype == np.float32 and breaks.flags.c_contiguous and breaks.tolist() == [2.0, 4.0, 8.0]
    centers = ops._host_f32(range(3), "centers")
    assert centers.dtype == np.float32 and centers.tolist() == [0.0, 1.0, 2.0]
    table = ops._check_objectives([(ops.SUPERPOSE_TM, 2), (ops.SUPERPOSE_COUNT, 4.5)])
    assert [(o.kind, o.param) for o in table] == [(0, 2.0), (1, 4.5)]
    wide = ops._host_i32_table(torch.tensor([[-7, 0, 2 ** 40, 3]]), (4,), "chi_last")
    assert wide.dtype == np.int32 and wide.flags.c_contiguous and wide.tolist() == [[-2, 0, 2 ** 31 - 1, 3]]
    atoms, last = ops._chi_tables(ATOMS, LAST, A, True)
    assert atoms.dtype == last.dtype == np.int32 and atoms.tolist() == ATOMS.tolist() and last.tolist() == LAST.tolist()
    atoms, last = ops._chi_tables(ATOMS.tolist(), LAST, A, False)
    assert atoms.tolist() == ATOMS.tolist() and last is None


def test_peptide_bond_constants_in_abi_order():
    k = ops._peptide_bond_constants(1e-10, {"tau": 10.0})
    assert k == [1.329, 0.014, 1.341, 0.016, -0.4473, 0.0311, -0.5203, 0.0353, 10.0, 1e-10, 0.0, 0.0]
