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


def test_peptide_bond_constants_in_abi_order():
    k = ops._peptide_bond_constants(1e-10, {"tau": 10.0})
    assert k == [1.329, 0.014, 1.341, 0.016, -0.4473, 0.0311, -0.5203, 0.0353, 10.0, 1e-10, 0.0, 0.0]
