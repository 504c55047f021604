"""Free-function geometry API of the reference (``protstruc.geometry``), on the GPU.

``angle``, ``dihedral``, ``gram_schmidt`` and ``place_fourth_atom`` evaluate in the same HIP device
functions the batch kernels use (csrc/ps_common.hpp) through a point-wise
launcher; ``dot`` / ``norm`` / ``unit`` are single broadcasting tensor ops.
``reconstruct_backbone_distmat_from_interresidue_geometry`` runs the distance-matrix kernels (csrc/distmat.hip);
``initialize_backbone_with_mds`` and ``fix_chirality`` the SMACOF and finishing kernels (csrc/mds.hip).
``inter_residue_geometry`` is the fused featuriser as a differentiable function of the coordinates (its backward pass is
one HIP kernel, ``ops.inter_residue_geometry_backward``); ``backbone_from_dihedrals`` is the backbone builder as a
differentiable function of the dihedrals, bond angles and bond lengths (``ops.backbone_from_dihedrals_backward``);
``frame_aligned_point_error`` is the fused FAPE loss (``ops.fape`` / ``ops.fape_backward``) and ``backbone_frames`` the
per-residue frames as a differentiable function of the coordinates (``ops.frames_backward``); ``lddt`` is the fused lDDT,
hard (the metric) and smooth (differentiable; ``ops.lddt`` / ``ops.lddt_backward``); ``steric_clash`` and
``peptide_bond_violations`` are the structural-violation terms (``ops.clash`` / ``ops.peptide_bond`` and their backwards);
``backbone_hbonds`` and ``dssp`` are the DSSP hydrogen bonds and secondary-structure labels (``ops.backbone_hbonds`` /
``ops.dssp_assign``); ``solvent_accessibility`` is Shrake and Rupley's surface area (``ops.solvent_accessibility``);
``nearest_neighbors`` is the k-nearest-neighbour graph (``ops.nearest_neighbors``) and ``gather_neighbors`` the gather
that turns its indices into edge features; ``radius_graph`` is every neighbour within a cutoff as CSR lists
(``ops.radius_graph``) and ``radius_graph_edges`` their (batch, row, col) triples; ``edge_distance_features`` and ``edge_frame_features`` are the fused edge
features of a structure network on such a graph (``ops.edge_rbf`` / ``ops.edge_frames``), differentiable in the
coordinates and the frames (``ops.csr_edge_rbf_backward``, ``.csr_edge_pair_grad_sum``, ``.csr_edge_frames_backward``), and
``radius_graph_incoming`` groups a graph's edges by their target; ``edge_aggregate``, ``edge_gather``, ``edge_softmax`` and
``edge_attention`` are message passing on such a graph -- segment sums, gathers and the softmax over every node's edges, with
their gradients, in a fixed order and without atomics (``ops.segment_reduce``, ``.segment_gather``, ``.edge_dot``,
``.segment_softmax``, ``.segment_softmax_backward``); ``side_chain_torsions``
measures chi1 .. chi4, differentiably in the coordinates, and ``set_side_chain_torsions`` turns the side chains to given
angles, differentiably in the angles (``ops.chi`` / ``ops.chi_set`` and their backwards); ``superposition_rmsd`` is the
RMSD after optimal superposition, differentiable in both point sets (``ops.superpose`` / ``ops.superpose_backward``), and
``tm_score``, ``gdt`` and ``superposition_scores`` are maxima over superpositions by a seeded search (``ops.superpose_search``).
``structure_alignment`` aligns two structures of different lengths without a given correspondence (``ops.structure_align``:
dynamic programming alternated with that search), with ``needleman_wunsch`` and ``ca_secondary_structure`` as its parts.
Type polymorphism follows the reference's ``with_tensor`` decorator
(decorator.py:5-53): numpy arrays in -> numpy arrays out (float64 is computed in
float32, as there), any tensor in -> tensor out.  Tensors must live on (or are
moved to) the GPU; there is no CPU evaluation path.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import ops


# ideal backbone geometry (reference constants/ideal.py:2-36): bond lengths in Angstrom, angles in radians
IDEAL_NA, IDEAL_AC, IDEAL_NAC = 1.458, 1.523, 1.937
# the peptide bond, for StructureBatch.from_backbone_dihedrals: |C-N| from the reference (ideal.C_N); the two angles
# around it, which the reference has no constant for, from Engh & Huber (CA-C-N 116.2 deg, C-N-CA 121.7 deg).
# The builder kernel (csrc/nerf.hip) rounds the same doubles to float32.
IDEAL_C_N = 1.329
IDEAL_CACN, IDEAL_CNCA = math.radians(116.2), math.radians(121.7)
# the placeholder of unknown distances in reconstruct_backbone_distmat_from_interresidue_geometry (reference
# geometry.py:21); exact in float32
MASK = 12345679


def ideal_backbone_coordinates(size, include_cb: bool = False) -> torch.Tensor:
    """Ideal N, CA, C (and CB) coordinates with CA at the origin and CA->C along +x, expanded to
    ``(*size, 3 or 4, 3)`` (reference geometry.py:191-226).  Returned on the CPU like the reference."""
    import math

    ca = torch.zeros(3)
    c = torch.tensor([IDEAL_AC, 0.0, 0.0])
    n = torch.tensor([IDEAL_NA * math.cos(IDEAL_NAC), IDEAL_NA * math.sin(IDEAL_NAC), 0.0])
    atoms = [n, ca, c]
    if include_cb:
        b_, c_ = ca - n, c - ca
        a_ = torch.linalg.cross(b_, c_)
        atoms.append(-0.58273431 * a_ + 0.56802827 * b_ - 0.54067466 * c_ + ca)  # tetrahedral CB placement
    return torch.stack(atoms).expand(*size, -1, -1)


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("protstruc_amd.geometry is HIP-only (no CPU fallback): no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _prep(args):
    """with_tensor semantics: convert ndarrays, remember whether any input was already a tensor."""
    found_tensor = any(isinstance(a, torch.Tensor) for a in args)
    dev = next((a.device for a in args if isinstance(a, torch.Tensor) and a.is_cuda), None) or _device()
    out = []
    for a in args:
        if isinstance(a, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(a))
            a = t.float() if t.dtype in (torch.float32, torch.float64) else t
        out.append(a.to(dev))
    return out, found_tensor


def _finish(t, found_tensor):
    return t if found_tensor else t.cpu().numpy()


def dot(x, y):
    """(x*y).sum(-1, keepdim=True)  (reference geometry.py:24-26)."""
    (x, y), ft = _prep([x, y])
    return _finish((x * y).sum(dim=-1, keepdim=True), ft)


def norm(x):
    """x.norm(dim=-1, keepdim=True)  (reference geometry.py:29-31)."""
    (x,), ft = _prep([x])
    return _finish(x.norm(dim=-1, keepdim=True), ft)


def unit(x):
    """x / |x|  (reference geometry.py:34-36)."""
    (x,), ft = _prep([x])
    return _finish(x / x.norm(dim=-1, keepdim=True), ft)


def angle(a, b, c, to_degree: bool = False):
    """Planar angle a-b-c in [0, pi] (reference geometry.py:39-71); acos without clamp, as in the reference."""
    (a, b, c), ft = _prep([a, b, c])
    out = ops.pointwise(0, a, b, c)
    return _finish(torch.rad2deg(out) if to_degree else out, ft)


def dihedral(a, b, c, d, to_degree: bool = False):
    """Dihedral angle of a-b-c-d in [-pi, pi] (reference geometry.py:74-124)."""
    (a, b, c, d), ft = _prep([a, b, c, d])
    out = ops.pointwise(1, a, b, c, d)
    return _finish(torch.rad2deg(out) if to_degree else out, ft)


def gram_schmidt(a, b, c):
    """Orthonormal basis of the plane through (c-b) and (a-b), basis vectors as columns (reference geometry.py:413-439)."""
    (a, b, c), ft = _prep([a, b, c])
    return _finish(ops.pointwise(2, a, b, c), ft)


def place_fourth_atom(a, b, c, length, planar, dihedral):
    """The atom X with |X - c| = ``length``, angle(X, c, b) = ``planar`` and dihedral(a, b, c, X) = ``dihedral``
    (reference geometry.py:127-168).  ``a``, ``b``, ``c`` are (n,3) points, the three parameters (n,1) or anything that
    broadcasts as a trailing size-1 axis against them (scalars included).  Evaluated by the same device function as
    StructureBatch.from_backbone_dihedrals (ps_pointwise_f32 mode 3)."""
    params = [np.asarray(p, dtype=np.float32) if isinstance(p, (int, float)) else p for p in (length, planar, dihedral)]
    (a, b, c, length, planar, dihedral), ft = _prep([a, b, c] + params)
    length, planar, dihedral = (p.reshape(1) if p.ndim == 0 else p for p in (length, planar, dihedral))
    if any(p.shape[-1] != 1 for p in (length, planar, dihedral)):
        raise ValueError("length, planar and dihedral must have a trailing axis of size 1, e.g. (n, 1)")
    full = torch.broadcast_shapes(a.shape, b.shape, c.shape, length.shape, planar.shape, dihedral.shape)
    if full[-1] != 3:
        raise ValueError("points must have a trailing axis of size 3")
    lead = tuple(full[:-1]) + (1,)
    d = torch.cat([p.float().expand(lead) for p in (length, planar, dihedral)], dim=-1)
    return _finish(ops.pointwise(3, a, b, c, d), ft)


def kabsch(a, b):
    """Rotation (3,3) and translation (3,) minimising the RMSD of ``R a + t`` against ``b`` for point sets
    (n,3) (reference geometry.py:442-480); evaluated by the batched Kabsch kernel with a batch of one.

    R is always a proper rotation (det +1), also for a mirror-image target.  Two points or collinear points leave a
    family of optimal rotations and R is one member of it; one point, or coincident points, give R = I and t = b - a;
    no point gives NaN (``ops.kabsch``)."""
    (a, b), ft = _prep([a, b])
    mask = torch.ones(1, a.shape[0], dtype=torch.bool, device=a.device)
    R, t = ops.kabsch(a.reshape(1, -1, 1, 3).contiguous(), b.reshape(1, -1, 1, 3).contiguous(), mask)
    return _finish(R[0], ft), _finish(t[0], ft)


_IRG_MASK_KEYS = ("d_ca_mask", "d_cb_mask", "d_no_mask")


class _InterResidueGeometry(torch.autograd.Function):
    """ops.inter_residue_geometry with ops.inter_residue_geometry_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, xyz, atom_mask):
        g = ops.inter_residue_geometry(xyz, atom_mask)
        masks = tuple(g[k] for k in _IRG_MASK_KEYS)
        ctx.mark_non_differentiable(*masks)
        # a plane the loss does not use arrives in backward() as None, not as a (B,N,N) tensor of zeros autograd would
        # otherwise allocate and fill: the kernel skips the arithmetic of an absent plane
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xyz, atom_mask)   # saved tensors: an in-place change before backward() is an error, not a wrong gradient
        return tuple(g[k] for k in ops.IRG_GRAD_KEYS) + masks

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_outputs):
        xyz, atom_mask = ctx.saved_tensors
        grads = {k: g for k, g in zip(ops.IRG_GRAD_KEYS, grad_outputs) if g is not None}
        grad_xyz = ops.inter_residue_geometry_backward(xyz, grads, atom_mask)
        return grad_xyz.to(xyz.dtype), None


def inter_residue_geometry(xyz, atom_mask=None):
    """The fused featuriser, differentiable with respect to ``xyz`` (B,N,A,3): the dict of ``ops.inter_residue_geometry``,
    in its key order -- d_ca, d_cb, d_no, omega, theta, phi (B,N,N) fp32, then the three bool mask planes; every value
    bit for bit what that call returns -- with the six float planes attached to the autograd graph.  Their backward pass
    is one launch of the HIP kernel behind ``ops.inter_residue_geometry_backward``, which receives only the planes the
    loss used (the others are absent, and their arithmetic is skipped): entries that read an atom absent from
    ``atom_mask`` and the diagonals of every plane but d_no pass no gradient (NaN coordinates of missing atoms never
    reach ``xyz.grad``).  The mask planes are not differentiable and ``atom_mask`` gets no gradient; no double backward."""
    out = _InterResidueGeometry.apply(xyz, atom_mask)
    return dict(zip(ops.IRG_GRAD_KEYS + _IRG_MASK_KEYS, out))   # the order ops.inter_residue_geometry builds its dict in


class _BackboneFromDihedrals(torch.autograd.Function):
    """ops.backbone_from_dihedrals with ops.backbone_from_dihedrals_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, dihedrals, chain_idx, residue_mask, bond_angles, bond_lengths, include_cb, n_slots):
        xyz, atom_mask = ops.backbone_from_dihedrals(dihedrals, chain_idx, residue_mask, bond_angles, bond_lengths,
                                                     include_cb=include_cb, n_slots=n_slots)
        ctx.mark_non_differentiable(atom_mask)
        ctx.include_cb = bool(include_cb)
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (dihedrals, bond_angles, bond_lengths))
        # the backward pass reads the coordinates and the segment rules, not the angles; saved tensors: an in-place change
        # of chain_idx / residue_mask before backward() is an error, not a wrong gradient
        ctx.save_for_backward(xyz, chain_idx, residue_mask)
        return xyz, atom_mask

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_xyz, _grad_atom_mask):
        xyz, chain_idx, residue_mask = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[3], ctx.needs_input_grad[4])
        grads = ops.backbone_from_dihedrals_backward(xyz, grad_xyz, chain_idx, residue_mask, include_cb=ctx.include_cb,
                                                     want_bond_angles=need[1], want_bond_lengths=need[2])
        g_dih, g_ang, g_len = (g.to(dt) if wanted else None for g, dt, wanted in zip(grads, ctx.dtypes, need))
        return g_dih, None, None, g_ang, g_len, None, None


def backbone_from_dihedrals(dihedrals, chain_idx=None, residue_mask=None, bond_angles=None, bond_lengths=None,
                            include_cb=False, n_slots=15):
    """The backbone builder as a differentiable function: ``(xyz (B,N,n_slots,3), atom_mask (B,N,n_slots))``, bit for
    bit what ``ops.backbone_from_dihedrals`` returns, with ``xyz`` attached to the autograd graph.  Gradients flow to
    ``dihedrals`` (B,N,3) and to ``bond_angles`` / ``bond_lengths`` (B,N,3) where given, each only if it requires grad;
    the backward pass is one launch of the HIP kernel behind ``ops.backbone_from_dihedrals_backward`` (the bond gradients
    that nobody needs reach it as absent and are not computed).  Angles the builder never reads (phi at a segment's
    first residue, psi / omega at its last, everything that only moves masked residues) get exact zeros.  ``atom_mask``
    is not differentiable; ``chain_idx`` / ``residue_mask`` get no gradient; no double backward."""
    return _BackboneFromDihedrals.apply(dihedrals, chain_idx, residue_mask, bond_angles, bond_lengths, include_cb, n_slots)


def _slot(atom) -> int:
    """An atom slot from its name ("CA"; KeyError on an unknown one, as StructureBatch raises) or its index."""
    from .general import ATOM
    return int(ATOM[atom]) if isinstance(atom, str) else int(atom)


class _BackboneFrames(torch.autograd.Function):
    """ops.frames (K4) with ops.frames_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, xyz, residue_mask, a1, a2, a3, t_atom):
        # t_atom None: the rotation alone (no translation is computed or written; that output is None)
        rot, trans = ops.frames(xyz, a1, a2, a3, 0 if t_atom is None else t_atom, want_trans=t_atom is not None)
        ctx.slots = (a1, a2, a3, 0 if t_atom is None else t_atom)
        ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None: its arithmetic is skipped
        ctx.save_for_backward(xyz, residue_mask)
        return rot, trans

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rot, grad_trans):
        xyz, residue_mask = ctx.saved_tensors
        if grad_rot is None and grad_trans is None:
            return (None,) * 6
        grad_xyz = ops.frames_backward(xyz, *ctx.slots, grad_rot=grad_rot, grad_trans=grad_trans, residue_mask=residue_mask)
        return grad_xyz.to(xyz.dtype), None, None, None, None, None


def backbone_frames(xyz, a1="N", a2="CA", a3="C", atom="CA", residue_mask=None):
    """Per-residue frames as a differentiable function of the coordinates: ``(rot (B,N,3,3), trans (B,N,3))``, bit for
    bit what ``ops.frames`` (K4) returns -- the Gram-Schmidt basis of (a3 - a2, a1 - a2) as the columns of ``rot`` and the
    position of ``atom`` -- attached to the autograd graph.  The backward pass is one launch of the HIP kernel behind
    ``ops.frames_backward``; an output the loss does not use costs nothing there.  Atoms are names ("CA") or slot indices;
    ``atom=None`` computes the rotation alone and returns ``(rot, None)``.
    Residues absent from ``residue_mask`` (B,N) get an exactly zero gradient whatever their coordinates hold (NaN of
    missing atoms included); their frames are still computed and are the caller's to mask.  No double backward."""
    return _BackboneFrames.apply(xyz, residue_mask, _slot(a1), _slot(a2), _slot(a3), None if atom is None else _slot(atom))


class _FrameAlignedPointError(torch.autograd.Function):
    """ops.fape with ops.fape_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, rot, trans, points, target_rot, target_trans, target_points, frame_mask, point_mask, clamp, scale, eps):
        loss, _ = ops.fape(rot, trans, points, target_rot, target_trans, target_points, frame_mask, point_mask,
                           clamp=clamp, scale=scale, eps=eps)
        ctx.scalars = (None if isinstance(clamp, torch.Tensor) else clamp, scale, eps)
        ctx.dtypes = (rot.dtype, trans.dtype, points.dtype)
        # nothing of the forward's arithmetic is kept: the backward kernel recomputes the pairs from the inputs
        ctx.save_for_backward(rot, trans, points, target_rot, target_trans, target_points, frame_mask, point_mask,
                              clamp if isinstance(clamp, torch.Tensor) else None)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        *operands, frame_mask, point_mask, clamp_t = ctx.saved_tensors
        clamp, scale, eps = ctx.scalars
        need = ctx.needs_input_grad[:3]
        grads = ops.fape_backward(*operands, grad_loss, frame_mask, point_mask, clamp=clamp_t if clamp is None else clamp,
                                  scale=scale, eps=eps, want_rot=need[0], want_trans=need[1], want_points=need[2])
        return tuple(g.to(dt) if wanted else None for g, dt, wanted in zip(grads, ctx.dtypes, need)) + (None,) * 8


def frame_aligned_point_error(rot, trans, points, target_rot, target_trans, target_points, frame_mask=None,
                              point_mask=None, *, clamp=10.0, scale=10.0, eps=1e-4):
    """Frame-aligned point error (AlphaFold 2 suppl. alg. 28) per structure, ``(B,)`` fp32, differentiable with respect to
    ``rot`` (B,N,3,3; basis vectors as columns), ``trans`` (B,N,3) and ``points`` (B,M,3):
    the mean over valid (frame, point) pairs of ``min(sqrt(|R_i^T (x_j - t_i) - R'_i^T (x'_j - t'_i)|^2 + eps), clamp) / scale``.
    ``frame_mask`` (B,N) and ``point_mask`` (B,M) select the pairs (None = all); ``clamp`` is a float or a (B,) tensor
    and ``inf`` means unclamped, so a per-sample mixture of clamped and unclamped structures is one call.  Forward and
    backward are one fused HIP kernel each (``ops.fape``, ``ops.fape_backward``): no (B,N,M) tensor is ever built, and only
    the gradients autograd asks for are computed.  A pair passes gradient iff its distance is below the clamp; a structure
    without a valid pair has loss 0 and zero gradients; masked frames and points get exact zeros, and NaN there (missing
    atoms) never reaches the loss or a gradient.  The target side is a constant; no double backward."""
    detach = [t.detach() for t in (target_rot, target_trans, target_points)]
    return _FrameAlignedPointError.apply(rot, trans, points, *detach, frame_mask, point_mask, clamp, scale, eps)


class _LDDT(torch.autograd.Function):
    """ops.lddt with ops.lddt_backward as the vector-Jacobian product of its smooth form."""

    @staticmethod
    def forward(ctx, points, target_points, point_mask, groups, cutoff, thresholds, smooth, eps):
        S, n = ops.lddt(points, target_points, point_mask, groups, cutoff=cutoff, thresholds=thresholds, smooth=smooth,
                        eps=eps)
        ctx.scalars = (cutoff, thresholds, eps)
        ctx.dtype = points.dtype
        if smooth:
            # nothing of the forward's arithmetic is kept: the backward kernel recomputes the pairs from the inputs
            ctx.save_for_backward(points, target_points, point_mask, groups)
            ctx.mark_non_differentiable(n)
        else:
            ctx.mark_non_differentiable(S, n)   # a step function of the coordinates: a metric, not a loss
        return S, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_S, _grad_n):
        points, target_points, point_mask, groups = ctx.saved_tensors
        cutoff, thresholds, eps = ctx.scalars
        grad = ops.lddt_backward(points, target_points, grad_S, point_mask, groups, cutoff=cutoff, thresholds=thresholds,
                                 eps=eps)
        return (grad.to(ctx.dtype),) + (None,) * 7


def _check_reduction(reduction) -> None:
    if reduction not in ("point", "structure", "none"):
        raise ValueError(f"reduction must be 'point', 'structure' or 'none', got {reduction!r}")


def lddt(points, target_points, point_mask=None, groups=None, cutoff=15.0, thresholds=ops.LDDT_THRESHOLDS, smooth=False,
         reduction="point", eps=1e-10):
    """lDDT (local distance difference test) of ``points`` (B,M,3) against ``target_points``: for every point the mean,
    over the points within ``cutoff`` of it ON THE TARGET (itself, points outside ``point_mask`` (B,M) and, where
    ``groups`` (B,M; integers) are given, points of its own group excluded), of the fraction of ``thresholds`` under which
    the pair's distance stays preserved.  ``reduction="point"`` returns ``S / max(n, 1)`` per point, (B,M);
    ``"structure"`` returns ``sum S / max(sum n, 1)``, (B,), the score over all pairs; ``"none"`` returns the kernel's
    ``(S, n)``.  A point (a structure) without a counted pair scores 0, never 1 or NaN.

    ``smooth=False`` is the METRIC: a step function of the coordinates, so the result carries no ``grad_fn`` even when
    the inputs require grad; per residue it is the training target of a confidence (pLDDT) head (AlphaFold 2 suppl.
    1.9.6).  ``smooth=True`` replaces every step by ``sigmoid(threshold - |d - d'|)`` (AlphaFold 3 suppl. alg. 27) and is
    differentiable with respect to ``points``: ``1 - lddt(..., smooth=True, reduction="structure")`` is a loss.

    Forward and backward are one fused HIP kernel each (``ops.lddt``, ``ops.lddt_backward``): nothing of size M^2 is ever
    built; the reductions are ordinary torch on (B,M) tensors.  Masked points get exact zeros (score and gradient), and NaN
    there (missing atoms) never reaches a result.  The target is a constant; no double backward."""
    _check_reduction(reduction)
    S, n = _LDDT.apply(points, target_points.detach(), point_mask, groups, float(cutoff),
                       tuple(float(t) for t in thresholds), bool(smooth), float(eps))
    if reduction == "none":
        return S, n
    if reduction == "point":
        return S / n.clamp(min=1)
    return S.sum(-1) / n.sum(-1).clamp(min=1)


class _StericClash(torch.autograd.Function):
    """ops.clash with ops.clash_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, points, radius, point_mask, groups, link, tolerance, eps):
        E, n = ops.clash(points, radius, point_mask, groups, link, tolerance=tolerance, eps=eps)
        # nothing of the forward's arithmetic is kept: the backward kernel recomputes the pairs from the inputs
        ctx.save_for_backward(points, radius, point_mask, groups, link)
        ctx.scalars = (tolerance, eps)
        ctx.dtype = points.dtype
        ctx.mark_non_differentiable(n)
        return E, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_E, _grad_n):
        points, radius, point_mask, groups, link = ctx.saved_tensors
        tolerance, eps = ctx.scalars
        grad = ops.clash_backward(points, radius, grad_E, point_mask, groups, link, tolerance=tolerance, eps=eps)
        return (grad.to(ctx.dtype),) + (None,) * 6


def steric_clash(points, radius, point_mask=None, groups=None, link=None, tolerance=ops.CLASH_TOLERANCE, eps=1e-10,
                 reduction="point"):
    """Steric clash energy of ``points`` (B,M,3) with van der Waals ``radius`` (B,M) (AlphaFold 2 suppl. 1.9.11, eq. 46):
    for every point the sum, over the other points (points outside ``point_mask`` (B,M), points of its own group where
    ``groups`` (B,M; integers) are given, and points that carry the same non-negative ``link`` (B,M; integers: a covalent
    bond between two groups) excluded), of ``max(0, radius_i + radius_j - tolerance - |x_i - x_j|)``.  Every clashing pair
    appears in both points' sums.  ``reduction="point"`` returns ``E`` (B,M); ``"structure"`` returns
    ``sum_i E_i / max(number of valid points, 1)``, (B,); ``"none"`` returns the kernel's ``(E, n)`` with ``n`` the number
    of points each point overlaps.

    Differentiable with respect to ``points`` (the radii are constants).  Forward and backward are one fused HIP kernel
    each (``ops.clash``, ``ops.clash_backward``): nothing of size M^2 is ever built.  Masked points get exact zeros
    (energy and gradient), and NaN there (missing atoms) never reaches a result.  No double backward."""
    _check_reduction(reduction)
    E, n = _StericClash.apply(points, radius.detach(), point_mask, groups, link, float(tolerance), float(eps))
    if reduction == "none":
        return E, n
    if reduction == "point":
        return E
    B, M = E.shape
    valid = (point_mask != 0).sum(-1) if point_mask is not None else torch.full((B,), M, device=E.device)
    return E.sum(-1) / valid.clamp(min=1).to(E.dtype)


class _PeptideBond(torch.autograd.Function):
    """ops.peptide_bond with ops.peptide_bond_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, xyz, junction_mask, next_is_proline, slots, eps, constants):
        n_slot, ca_slot, c_slot = slots
        ctx.kwargs = dict(n_slot=n_slot, ca_slot=ca_slot, c_slot=c_slot, eps=eps, **dict(constants))
        ctx.save_for_backward(xyz, junction_mask, next_is_proline)
        ctx.dtype = xyz.dtype
        return ops.peptide_bond(xyz, junction_mask, next_is_proline, **ctx.kwargs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_viol):
        xyz, junction_mask, next_is_proline = ctx.saved_tensors
        grad = ops.peptide_bond_backward(xyz, grad_viol, junction_mask, next_is_proline, **ctx.kwargs)
        return (grad.to(ctx.dtype),) + (None,) * 5


def peptide_bond_violations(xyz, junction_mask=None, next_is_proline=None, n_slot=0, ca_slot=1, c_slot=2, eps=1e-10,
                            **constants):
    """Peptide-bond violations of ``xyz`` (B,N,A,3) at every junction r -> r+1 (AlphaFold 2 suppl. 1.9.11, eq. 44-45),
    (B,N,3): how far the bond length |C - N'|, the cosine of the angle CA-C-N' and the cosine of the angle C-N'-CA' lie
    outside ``tau`` standard deviations around their ideal values -- ``max(0, |value - ideal| - tau * sigma)`` each, with
    the constants of ``ops.PEPTIDE_BOND`` (``tau=12.0``; any of them may be overridden by keyword).  ``junction_mask``
    (B,N): entry r is the junction from residue r to residue r+1 (None = all; entry N-1 is ignored); ``next_is_proline``
    (B,N): residue r+1 is a proline.  Invalid junctions and row N-1 are exact zeros, value and gradient, whatever NaN sits
    there.  Differentiable with respect to ``xyz``; one HIP kernel forwards (``ops.peptide_bond``) and one backwards
    (``ops.peptide_bond_backward``).  No double backward."""
    ops.check_peptide_bond_shapes(xyz, junction_mask, next_is_proline, n_slot, ca_slot, c_slot, eps, **constants)
    return _PeptideBond.apply(xyz, junction_mask, next_is_proline, (int(n_slot), int(ca_slot), int(c_slot)), float(eps),
                              tuple(sorted((k, float(v)) for k, v in constants.items())))


DSSP_CODES = "-HBEGITS"
DSSP_REDUCED_CODES = "CHE"
# the reduced class of every code of DSSP_CODES (- -> C, H G I -> H, B E -> E), two bits per code
_DSSP_REDUCED_PACKED = sum(cls << (2 * code) for code, cls in enumerate((0, 1, 2, 2, 1, 1, 0, 0)))


class BackboneHBonds(NamedTuple):
    """The two best hydrogen-bond partners of every residue (``backbone_hbonds``), each (B,N,2); -1 / 0 where empty."""
    acceptor_idx: torch.Tensor      # int32: the residues whose C=O accepts this residue's N-H
    acceptor_energy: torch.Tensor   # fp32, kcal/mol
    donor_idx: torch.Tensor         # int32: the residues whose N-H donate to this residue's C=O
    donor_energy: torch.Tensor


def backbone_hbonds(xyz, complete, junction, donor=None, n=0, ca=1, c=2, o=3) -> BackboneHBonds:
    """The backbone hydrogen bonds of ``xyz`` (B,N,A,3) by the Kabsch-Sander energy of DSSP, with the two-best-partners
    rule of the DSSP programs: for the C=O of residue i and the N-H of residue j, H placed 1 A from N along the previous
    residue's O -> C, ``E = 27.888 (1/d(O,N) + 1/d(C,H) - 1/d(O,H) - 1/d(C,N))`` kcal/mol (-9.9 where a distance is below
    0.5 A); a hydrogen bond is E < -0.5, and every N-H and every C=O keeps its two best.  ``complete`` (B,N): the residue
    has N, CA, C and O and is in the residue mask; ``junction`` (B,N): r -> r+1 is a peptide bond between two complete
    residues (``structure_batch.valid_junctions`` ANDed with ``complete`` of both); ``donor`` (B,N): False for proline
    (None = every residue donates); ``n``, ``ca``, ``c``, ``o``: the atoms' slots.  Energies are not rounded to 0.001 as
    the DSSP programs do.  One HIP kernel (``ops.backbone_hbonds``); no (B,N,N) tensor is built; not differentiable."""
    return BackboneHBonds(*ops.backbone_hbonds(xyz, complete, junction, donor, n_slot=n, ca_slot=ca, c_slot=c, o_slot=o))


def dssp(xyz, complete, junction, donor=None, reduced=False):
    """DSSP secondary structure of ``xyz`` (B,N,A,3; N, CA, C, O in slots 0-3), (B,N) int8 indices into ``DSSP_CODES`` =
    "-HBEGITS" -- or, ``reduced=True``, into ``DSSP_REDUCED_CODES`` = "CHE" (H, G, I -> H; E, B -> E; everything else ->
    C).  Kabsch & Sander 1983 on the hydrogen bonds of ``backbone_hbonds`` (same ``complete``, ``junction``, ``donor``):
    n-turns, the helices G / H / I from two consecutive turns, T, bridges and ladders (B / E) and the bend S.  Three
    simplifications against the DSSP programs: energies are not rounded to 0.001, ladders are not joined across
    beta-bulges, and the label is a pure per-residue priority H, B, E, G, I, T, S.  Incomplete and padded residues are 0.
    Two HIP kernels (``ops.backbone_hbonds``, ``ops.dssp_assign``); at most ``ops.DSSP_MAX_RESIDUES`` residues per
    structure; not differentiable."""
    acceptor_idx = ops.backbone_hbonds(xyz, complete, junction, donor)[0]
    codes = ops.dssp_assign(xyz, complete, junction, acceptor_idx)
    if reduced:
        # arithmetic on the device, not a table built on the host: a host tensor would be copied on every call, which
        # synchronises and cannot be captured in a graph.  Two bits per code, code c at bits 2c
        codes = ((_DSSP_REDUCED_PACKED >> (codes.to(torch.int32) * 2)) & 3).to(torch.int8)
    return codes


def dssp_strings(codes, lengths=None, reduced=False):
    """The codes of ``dssp`` (B,N) as a list of B ``str`` over ``DSSP_CODES`` (``reduced=True``: over
    ``DSSP_REDUCED_CODES``), each cut to its entry of ``lengths`` where given."""
    alphabet = DSSP_REDUCED_CODES if reduced else DSSP_CODES
    rows = torch.as_tensor(codes).cpu().tolist()
    if lengths is None:
        lengths = [len(row) for row in rows]
    else:
        lengths = [int(n) for n in torch.as_tensor(lengths).cpu().tolist()]
        if len(lengths) != len(rows):
            raise ValueError(f"lengths must have one entry per structure, got {len(lengths)} for {len(rows)}")
    return ["".join(alphabet[k] for k in row[:n]) for row, n in zip(rows, lengths)]


class SolventAccessibility(NamedTuple):
    """Shrake-Rupley accessibility of every point (``solvent_accessibility``), each (B,M); zeros at masked points."""
    count: torch.Tensor   # int32: the test points of the atom that no other atom buries
    area: torch.Tensor    # fp32, A^2: 4 pi (radius + probe)^2 count / S


def sphere_points(n):
    """``n`` directions spread over the unit sphere by the golden spiral, an (n,3) float32 CPU tensor: for k = 0 .. n-1
    ``z = 1 - (2k+1)/n``, ``rho = sqrt(1 - z^2)``, ``phi = k pi (3 - sqrt 5)``, ``u_k = (rho cos phi, rho sin phi, z)``,
    evaluated in float64 and rounded to float32 once -- so ``|u_k|`` is 1 to float32 rounding only, and everything that
    uses the table takes it as it is."""
    n = int(n)
    if n < 1:
        raise ValueError(f"a sphere needs at least one point, got {n}")
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    rho = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return torch.from_numpy(np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1).astype(np.float32))


_SPHERES = {}   # (n, device) -> the table on that device


def _sphere_on(n: int, device) -> torch.Tensor:
    key = (n, torch.device(device))
    table = _SPHERES.get(key)
    if table is None:
        table = _SPHERES[key] = sphere_points(n).to(device)
    return table


def solvent_accessibility(points, radius, point_mask=None, isolate=None, probe=1.4, n_points=96, sphere=None) -> SolventAccessibility:
    """Solvent-accessible surface area of ``points`` (B,M,3) with van der Waals ``radius`` (B,M) by Shrake & Rupley (1973):
    every atom carries ``n_points`` test points on the sphere of radius ``radius + probe`` around it -- the golden spiral
    of ``sphere_points``, or the rows of ``sphere`` (S,3; float32 unit vectors) where given -- and a test point is buried
    where it lies inside that sphere of another atom.  Returns ``(count, area)``, each (B,M): the test points left open
    (int32) and ``4 pi (radius + probe)^2 count / S`` in A^2.  Points outside ``point_mask`` (B,M) neither occlude nor are
    measured (zeros; NaN there never reaches a result); with ``isolate`` (B,M; integers) two points see each other only
    where their keys are equal, which measures every chain, or every residue, alone.  Atoms of one residue occlude each
    other.  At most ``ops.SASA_MAX_SPHERE_POINTS`` test points per atom.  One HIP kernel (``ops.solvent_accessibility``)
    that decides in double on the float32 inputs; no (B,M,M) or (B,M,S) tensor is built.  Not differentiable: the
    result is a count."""
    if sphere is None:
        n = int(n_points)
        if not 1 <= n <= ops.SASA_MAX_SPHERE_POINTS:
            raise ValueError(f"n_points must lie in 1 .. {ops.SASA_MAX_SPHERE_POINTS}, got {n_points}")
        ops.check_sasa_shapes(points, radius, point_mask, isolate, None, probe)
        sphere = _sphere_on(n, points.device)
    return SolventAccessibility(*ops.solvent_accessibility(points.detach(), radius.detach(), point_mask, isolate, sphere=sphere,
                                                           probe=float(probe)))


def _marshal(named):
    """What the functions over neighbour lists share: numpy or tensors in (``named``: (name, value) pairs, None left out,
    the first one deciding the device the results come back on) -> ``(prepared, finish)``, the dict of prepared tensors
    by name and the function that takes a tuple of result tensors (or None) back out the same way.  The edge functions
    pass the dict on as ``**prepared``, so their names are the parameter names of ``ops.edge_rbf`` / ``ops.edge_frames``."""
    given = [(name, t) for name, t in named if t is not None]
    for name, t in given:
        if not isinstance(t, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{name} must be a tensor or an ndarray")
    home = named[0][1].device if isinstance(named[0][1], torch.Tensor) else None
    prepped, ft = _prep([t.detach() if isinstance(t, torch.Tensor) else t for _, t in given])

    def finish(out):
        return tuple(None if t is None else _finish(t if home is None else t.to(home), ft) for t in out)
    return dict(zip((name for name, _ in given), prepped)), finish


class Neighbors(NamedTuple):
    """The k nearest neighbours of every query (``nearest_neighbors``), nearest first."""
    idx: torch.Tensor     # (B,Q,k) int32: indices into the points' M axis; -1 where a query has fewer than k neighbours
    dist: torch.Tensor    # (B,Q,k) fp32: the distances, ascending; +inf at the padding
    count: torch.Tensor   # (B,Q) int32: the number of real neighbours, at most k


def nearest_neighbors(points, k, point_mask=None, *, queries=None, query_mask=None, exclude=None, query_exclude=None,
                      cutoff=float("inf"), include_self=False) -> Neighbors:
    """The ``k`` nearest ``points`` (B,M,3) of every query, sorted by distance: ``Neighbors(idx, dist, count)`` with
    ``idx`` and ``dist`` (B,Q,k) and ``count`` (B,Q).  The queries are ``queries`` (B,Q,3) or, None, the points themselves
    (the neighbour graph of the points, Q = M; a point is not its own neighbour unless ``include_self``).  Points outside
    ``point_mask`` (B,M) are no candidates and queries outside ``query_mask`` (B,Q; in the self graph ``point_mask``) get
    no neighbours; NaN there never reaches a result.  ``exclude`` (B,M) and ``query_exclude`` (B,Q; in the self graph
    ``exclude``) are integer keys: a candidate with the query's key is skipped -- the residue index leaves out an atom's
    own residue, the chain index leaves only the other chains.  ``cutoff`` drops candidates further away (inclusive).
    Distances are compared in double on the float32 coordinates and ties go to the lower index, so the result is defined
    bit for bit; a query with fewer than ``k`` neighbours is padded with index -1 and distance +inf, and ``count`` says
    how many are real.  ``k <= ops.KNN_MAX_K``.  One HIP kernel (``ops.nearest_neighbors``); no (B,Q,M) tensor is built.
    numpy in -> numpy out; tensors come back on the device of ``points``, CPU tensors included.

    Not differentiable -- the selection is discrete -- and the outputs carry no graph.  Edge lengths that are
    differentiable with respect to the coordinates are rebuilt from the indices::

        nb = nearest_neighbors(x, 30, mask)
        xj = gather_neighbors(x, nb.idx)                        # (B,M,k,3), zeros at the padding
        edge = (xj - x[:, :, None]).norm(dim=-1)                # (B,M,k), equal to nb.dist up to float32 rounding
        edge = edge.masked_fill(nb.idx < 0, 0.0)                # the padding takes no gradient
    """
    args, finish = _marshal((("points", points), ("point_mask", point_mask), ("queries", queries), ("query_mask", query_mask),
                             ("exclude", exclude), ("query_exclude", query_exclude)))
    out = ops.nearest_neighbors(args.pop("points"), k, args.pop("point_mask", None), cutoff=cutoff, include_self=include_self,
                                **args)
    return Neighbors(*finish(out))


def gather_neighbors(values, idx, fill=0):
    """``values`` (B,M,...) at the neighbours ``idx`` (B,Q,k) of ``nearest_neighbors``: (B,Q,k,...), with ``fill`` where
    ``idx`` is -1 (the padding).  Plain torch, on any device; differentiable with respect to ``values`` (the padding takes
    no gradient)."""
    if idx.ndim != 3 or values.ndim < 2 or values.shape[0] != idx.shape[0]:
        raise ValueError(f"values must be (B, M, ...) and idx (B, Q, k), got {tuple(values.shape)} and {tuple(idx.shape)}")
    B, Q, k = idx.shape
    if values.shape[1] == 0:   # no candidates: everything is padding
        return values.new_full((B, Q, k, *values.shape[2:]), fill)
    real = idx >= 0
    at = idx.clamp(min=0).long().reshape(B, Q * k, *([1] * (values.ndim - 2))).expand(B, Q * k, *values.shape[2:])
    out = torch.gather(values, 1, at).reshape(B, Q, k, *values.shape[2:])
    return torch.where(real.reshape(B, Q, k, *([1] * (values.ndim - 2))), out, torch.full_like(out, fill))


class RadiusGraph(NamedTuple):
    """Every neighbour of every query within a cutoff (``radius_graph``), in CSR form: row ``r = b * Q + q`` is
    ``col[row_ptr[r]:row_ptr[r + 1]]``."""
    row_ptr: torch.Tensor   # (B*Q+1,) int64: the exclusive prefix sum of count; row_ptr[-1] is the number of edges E
    col: torch.Tensor       # (E,) int32: the neighbours' indices into the M axis of their own structure, ascending in a row
    dist: torch.Tensor      # (E,) fp32: the distances
    count: torch.Tensor     # (B,Q) int32: the number of neighbours of each query


def radius_graph(points, cutoff, point_mask=None, *, queries=None, query_mask=None, exclude=None, query_exclude=None,
                 include_self=False, max_edges=None) -> RadiusGraph:
    """Every one of the ``points`` (B,M,3) within ``cutoff`` of every query: ``RadiusGraph(row_ptr, col, dist, count)``, lists
    of any length in CSR form.  The arguments are those of ``nearest_neighbors`` -- ``queries`` (B,Q,3) or, None, the points
    themselves (a point is not its own neighbour unless ``include_self``); masks; the integer keys ``exclude`` /
    ``query_exclude`` that skip a candidate with the query's key -- and so is the predicate: distances compared in double
    on the float32 coordinates, ``<=`` at the cutoff, so the result is defined bit for bit and, in the self graph without
    keys, symmetric.  There is no ``k`` and no cap.  The rows are the B*Q queries in (b, q) order; within a row ``col`` is
    ascending.  ``cutoff`` is positive and finite.  HIP kernels (``ops.radius_graph``): blocks of 64 consecutive points
    whose bounding box is further than the cutoff from the box of 64 consecutive queries are never looked at, which is
    what chain-ordered input gives; shuffled input gives the same answer, slower.  No (B,Q,M) tensor is built.

    With ``max_edges=None`` the number of edges is read from the device once (not capturable by ``torch.cuda.graph``);
    with ``max_edges=n`` nothing is read: ``col`` and ``dist`` have n entries, edges from position n on are not written
    while ``row_ptr`` and ``count`` stay exact -- test ``row_ptr[-1] <= n`` --, and entries past ``row_ptr[-1]`` are -1 /
    +inf.  numpy in -> numpy out; tensors come back on the device of ``points``, CPU tensors included.

    Unlike ``torch_cluster.radius_graph``: no ``max_num_neighbors`` (nothing is ever cut silently); ``col`` indexes each
    structure's own M axis and comes with ``row_ptr``, not as a flat ``edge_index`` over a concatenated batch
    (``radius_graph_edges`` gives the triples); rows are ascending in j; a pair exactly at the cutoff IS an edge.

    Not differentiable -- the list is discrete -- and the outputs carry no graph; ``radius_graph_edges`` is the route to
    distances that are differentiable with respect to the coordinates."""
    args, finish = _marshal((("points", points), ("point_mask", point_mask), ("queries", queries), ("query_mask", query_mask),
                             ("exclude", exclude), ("query_exclude", query_exclude)))
    out = ops.radius_graph(args.pop("points"), cutoff, args.pop("point_mask", None), include_self=include_self,
                           max_edges=max_edges, **args)
    return RadiusGraph(*finish(out))


def radius_graph_edges(graph):
    """``(batch, row, col)``, each (E,) int64, one entry per edge of a ``RadiusGraph`` of tensors: the structure, the query
    and the neighbour -- the form ``index_add`` / scatter layers take.  Plain torch (``repeat_interleave`` over
    ``count``), on the graph's device.  It is also the differentiable route to the distances, which the list is not::

        g = radius_graph(x, 10.0, mask)
        b, i, j = radius_graph_edges(g)
        edge = (x[b, i] - x[b, j]).norm(dim=-1)      # (E,), equal to g.dist up to float32 rounding; grads reach x

    For a graph made with ``max_edges`` below ``row_ptr[-1]`` the triples past the buffers have no ``col``: refused.
    This function reads ``row_ptr[-1]`` on the host; ``radius_edge_rows`` gives ``batch`` and ``row`` for every position
    of ``col`` without a host read and is the route that runs inside a captured graph."""
    row_ptr, col, count = graph.row_ptr, graph.col, graph.count
    B, Q = count.shape
    edges = int(row_ptr[-1])
    if edges > col.shape[0]:
        raise ValueError(f"the graph has {edges} edges but col holds {col.shape[0]}: max_edges was too small")
    row = torch.repeat_interleave(torch.arange(B * Q, device=count.device), count.reshape(-1).long(), output_size=edges)
    return row // max(Q, 1), row % max(Q, 1), col[:edges].long()


BACKBONE_PAIRS = tuple((a, b) for a in range(5) for b in range(5))   # all ordered pairs of N, CA, C, O, CB: ProteinMPNN's 25


def rbf_centers(n_rbf: int = 16, d_min: float = 2.0, d_max: float = 22.0):
    """``(centers, sigma)`` of ``n_rbf`` Gaussians spread evenly over [d_min, d_max]: ``centers`` is a float32 array of
    shape (n_rbf,) on the host -- the kernel takes it as an argument --, the linspace computed in double and rounded once,
    and ``sigma = (d_max - d_min) / n_rbf``, a float
    -- ProteinMPNN's choice (16 centres from 2 to 22 A, sigma 1.25)."""
    if isinstance(n_rbf, bool) or not isinstance(n_rbf, (int, np.integer)) or not 1 <= n_rbf <= ops.EDGE_MAX_RBF:
        raise ValueError(f"n_rbf must be an integer in 1 .. {ops.EDGE_MAX_RBF}, got {n_rbf!r}")
    if not float(d_max) > float(d_min):
        raise ValueError(f"d_max must be above d_min, got {d_min} and {d_max}")
    centers = np.linspace(float(d_min), float(d_max), int(n_rbf), dtype=np.float64).astype(np.float32)
    return centers, (float(d_max) - float(d_min)) / int(n_rbf)


def _wants_grad(*tensors) -> bool:
    """whether a graph is to be built: grad mode is on and one of ``tensors`` is a floating tensor that requires grad"""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.is_floating_point() and t.requires_grad
                                           for t in tensors)


def _attached(prepared: dict, **given) -> dict:
    """``prepared`` (the detached tensors of ``_marshal``, on the kernels' device) with those of ``given`` that require grad
    put back attached to their graph"""
    for name, t in given.items():
        if isinstance(t, torch.Tensor) and t.is_floating_point() and t.requires_grad:
            prepared[name] = t.to(prepared[name].device)
    return prepared


def _csr_lists(first, col, B: int, N: int):
    """``(row_ptr, col)`` of the edge lists a function was called with: CSR lists ``(row_ptr, col)`` as they are, a padded
    (B,N,k) list ``(idx, None)`` as the CSR lists it is -- ``arange(B*N + 1) * k`` and the flattened indices"""
    if col is not None:
        return first, col
    idx = ops._idx32(first, N)
    return torch.arange(B * N + 1, dtype=torch.int64, device=idx.device) * idx.shape[2], idx.reshape(-1)


def _flat_grad(g, E: int):
    """an incoming gradient as a contiguous (E, ...) tensor; ``x.sum().backward()`` hands in one of stride 0"""
    return None if g is None else g.contiguous().reshape(E, -1)


class _EdgeDistanceFeatures(torch.autograd.Function):
    """ops.edge_rbf (K25) or ops.csr_edge_rbf (K50) with K52 and K53 as their vector-Jacobian product.  The lists are
    ``(idx, None)`` or ``(row_ptr, col)``; ``tables`` the keywords pair_i, pair_j, centers and sigma.  Lists and masks are
    saved like the coordinates, so that changing one in place before the backward pass is noticed."""

    @staticmethod
    def forward(ctx, xyz, src_xyz, first, col, atom_mask, src_mask, tables, want_dist):
        if col is None:
            dist, rbf = ops.edge_rbf(xyz, first, atom_mask, want_dist=want_dist, **tables)
        else:
            dist, rbf = ops.csr_edge_rbf(xyz, first, col, atom_mask, src_xyz=src_xyz, src_mask=src_mask, want_dist=want_dist,
                                         **tables)
        ctx.tables = tables
        ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None: K52 takes a NULL for it
        ctx.save_for_backward(xyz, src_xyz, first, col, atom_mask, src_mask)
        return rbf, dist

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rbf, grad_dist):
        xyz, src_xyz, first, col, atom_mask, src_mask = ctx.saved_tensors
        if grad_rbf is None and grad_dist is None:
            return (None,) * 8
        B, M, A = xyz.shape[:3]
        row_ptr, col = _csr_lists(first, col, B, M)
        E = col.shape[0]
        pair_grad = ops.csr_edge_rbf_backward(xyz, row_ptr, col, atom_mask, src_xyz=src_xyz, src_mask=src_mask,
                                              grad_dist=_flat_grad(grad_dist, E), grad_rbf=_flat_grad(grad_rbf, E), **ctx.tables)
        Q, As = (None, None) if src_xyz is None else src_xyz.shape[1:3]
        in_ptr, in_edge = ops.csr_incoming_edges(row_ptr, col, B, M if Q is None else Q, M)
        out = ops.csr_edge_pair_grad_sum(pair_grad, row_ptr, in_ptr, in_edge, pair_i=ctx.tables["pair_i"],
                                         pair_j=ctx.tables["pair_j"], B=B, M=M, A=A, Q=Q, As=As)
        grad, grad_src = (out, None) if src_xyz is None else out
        return (grad.to(xyz.dtype) if ctx.needs_input_grad[0] else None,
                grad_src.to(src_xyz.dtype) if src_xyz is not None and ctx.needs_input_grad[1] else None) + (None,) * 6


class _EdgeFrameFeatures(torch.autograd.Function):
    """ops.edge_frames (K26) or ops.csr_edge_frames (K51) with K54 as their vector-Jacobian product; the lists as above."""

    @staticmethod
    def forward(ctx, rot, trans, src_rot, src_trans, first, col, frame_mask, src_mask):
        if col is None:
            pos, rel = ops.edge_frames(rot, trans, first, frame_mask)
        else:
            pos, rel = ops.csr_edge_frames(rot, trans, first, col, frame_mask, src_rot=src_rot, src_trans=src_trans,
                                           src_mask=src_mask)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(rot, trans, src_rot, src_trans, first, col, frame_mask, src_mask)
        return pos, rel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_pos, grad_rot):
        rot, trans, src_rot, src_trans, first, col, frame_mask, src_mask = ctx.saved_tensors
        if grad_pos is None and grad_rot is None:
            return (None,) * 8
        B, M = rot.shape[:2]
        row_ptr, col = _csr_lists(first, col, B, M)
        E = col.shape[0]
        in_ptr, in_edge = ops.csr_incoming_edges(row_ptr, col, B, M if src_rot is None else src_rot.shape[1], M)
        out = ops.csr_edge_frames_backward(rot, trans, row_ptr, col, in_ptr, in_edge, frame_mask, src_rot=src_rot,
                                           src_trans=src_trans, src_mask=src_mask, grad_pos=_flat_grad(grad_pos, E),
                                           grad_rot=None if grad_rot is None else grad_rot.contiguous().reshape(E, 3, 3))
        out = tuple(out) + (None, None) * (src_rot is None)
        inputs = (rot, trans, src_rot, src_trans)
        return tuple(g.to(x.dtype) if x is not None and ctx.needs_input_grad[n] else None
                     for n, (g, x) in enumerate(zip(out, inputs))) + (None,) * 4


def edge_distance_features(xyz, idx, atom_mask=None, pairs=BACKBONE_PAIRS, centers=None, sigma=None, return_dist=False):
    """Radial basis functions of the atom-pair distances along the edges of a neighbour graph: ``rbf`` (B,N,k,P*R) fp32
    or, with ``return_dist``, ``(rbf, dist)`` with ``dist`` (B,N,k,P).  ``xyz`` is (B,N,A,3); ``idx`` (B,N,k) are the
    neighbour lists of ``nearest_neighbors`` on the residues (``Neighbors.idx``; any entry outside [0, N), the -1 of the
    padding included, is padding); ``pairs`` are (slot on the source residue, slot on the neighbour) -- by default all 25
    ordered pairs of the first five slots, N, CA, C, O, CB --; ``centers`` (R,) and ``sigma`` default to ``rbf_centers()``
    (16 centres over 2 .. 22 A, sigma 1.25), and one given without the other is refused.
    ``rbf[..., p*R + c] = exp(-((dist_p - centers[c]) / sigma)^2)`` with ``dist`` the distance computed in double on the
    float32 coordinates and rounded once.  Both are exactly 0 at the padding and where either atom is outside
    ``atom_mask`` (B,N,A), and NaN there never reaches the result.  One HIP kernel (``ops.edge_rbf``): the gathered
    (B,N,k,A,3) coordinates and the broadcast (B,N,k,P,R) intermediates of the composed route are never built.
    numpy in -> numpy out; tensors come back on the device of ``xyz``, CPU tensors included.

    Differentiable with respect to ``xyz``: where it is a tensor that requires grad (and grad mode is on) the outputs carry
    a graph whose backward pass is HIP too -- ``ops.csr_edge_rbf_backward`` (K52) on the list as CSR lists, the incoming
    lists of ``ops.csr_incoming_edges`` and ``ops.csr_edge_pair_grad_sum`` (K53): no atomics, bit-for-bit repeatable, exactly
    0 at the padding, under the mask and on a self edge of length 0.  Not differentiable with respect to ``centers``,
    ``sigma`` or the list, and not twice: for a second derivative the composed route -- ``gather_neighbors`` and plain torch
    -- is still the one.  numpy inputs and inputs that do not require grad take the forward kernel alone, and their
    outputs carry no graph."""
    if (centers is None) != (sigma is None):
        raise ValueError("centers and sigma come together (rbf_centers() returns both)")
    if centers is None:
        centers, sigma = rbf_centers()
    pairs = [tuple(p) for p in pairs]
    if any(len(p) != 2 for p in pairs):
        raise ValueError("pairs must be (slot on the source residue, slot on the neighbour) pairs")
    args, finish = _marshal((("xyz", xyz), ("idx", idx), ("atom_mask", atom_mask)))
    tables = dict(pair_i=[p[0] for p in pairs], pair_j=[p[1] for p in pairs], centers=centers, sigma=sigma)
    if _wants_grad(xyz):
        args = _attached(args, xyz=xyz)
        rbf, dist = finish(_EdgeDistanceFeatures.apply(args["xyz"], None, args["idx"], None, args.get("atom_mask"), None, tables,
                                                       bool(return_dist)))
    else:
        dist, rbf = finish(ops.edge_rbf(**args, **tables, want_dist=bool(return_dist)))
    return (rbf, dist) if return_dist else rbf


class EdgeFrames(NamedTuple):
    """The neighbours' frames in the source residues' frames (``edge_frame_features``)."""
    local_pos: torch.Tensor   # (B,N,k,3) fp32: R_i^T (t_j - t_i)
    rel_rot: torch.Tensor     # (B,N,k,3,3) fp32: R_i^T R_j


def edge_frame_features(rot, trans, idx, frame_mask=None) -> EdgeFrames:
    """Every neighbour's position and orientation in the source residue's frame (Ingraham et al. 2019; GVP, PiFold,
    Chroma): ``EdgeFrames(local_pos (B,N,k,3) = R_i^T (t_j - t_i), rel_rot (B,N,k,3,3) = R_i^T R_j)``.  ``rot`` (B,N,3,3)
    has the basis vectors as columns and ``trans`` is (B,N,3), as ``backbone_frames`` returns them; ``idx`` (B,N,k) are
    the neighbour lists of ``nearest_neighbors`` (any entry outside [0, N) is padding).  Evaluated in double on the
    float32 inputs in a fixed order and rounded once, so defined bit for bit; exactly 0 at the padding and where i or j
    is outside ``frame_mask`` (B,N), and NaN there never reaches the result.  One HIP kernel (``ops.edge_frames``).
    numpy in -> numpy out; tensors come back on the device of ``rot``, CPU tensors included.

    Differentiable with respect to ``rot`` and ``trans``: where one of them is a tensor that requires grad (and grad mode
    is on) the outputs carry a graph whose backward pass is one HIP kernel, ``ops.csr_edge_frames_backward`` (K54), on the
    list as CSR lists -- ``rot`` as nine free numbers per frame, which is what the backward pass of ``backbone_frames``
    takes; no atomics, defined bit for bit, exactly 0 at the padding and under the mask.  Not differentiable twice (for a
    second derivative ``gather_neighbors`` and plain torch are still the route), nor with respect to the list; where
    neither input requires grad the outputs carry no graph."""
    args, finish = _marshal((("rot", rot), ("trans", trans), ("idx", idx), ("frame_mask", frame_mask)))
    if _wants_grad(rot, trans):
        args = _attached(args, rot=rot, trans=trans)
        return EdgeFrames(*finish(_EdgeFrameFeatures.apply(args["rot"], args["trans"], None, None, args["idx"], None,
                                                           args.get("frame_mask"), None)))
    return EdgeFrames(*finish(ops.edge_frames(**args)))


# ---- the same edge features on the CSR lists of radius_graph -----------------------------------------------------------------
def _graph_queries(graph) -> int:
    """Q of a ``RadiusGraph``: the queries per structure, from ``count`` (B,Q)"""
    if not isinstance(graph, RadiusGraph):
        raise TypeError("graph must be a geometry.RadiusGraph (radius_graph, neighbors_to_radius_graph)")
    if graph.count.ndim != 2:
        raise ValueError(f"graph.count must have shape (batch, queries), got {tuple(graph.count.shape)}")
    return int(graph.count.shape[1])


def radius_edge_rows(graph):
    """``(batch, row)``, each (E,) int32, of every edge position of a ``RadiusGraph``, E being ``graph.col.shape[0]``: the
    structure and the query the entry ``col[p]`` belongs to, both -1 from position ``row_ptr[-1]`` on (the tail that
    ``max_edges`` leaves).  With ``col`` these are the triples of ``radius_graph_edges``, found on the device (one HIP
    kernel, ``ops.csr_edge_rows``) with no host read, so this runs inside ``torch.cuda.graph`` behind
    ``radius_graph(..., max_edges=n)``.  numpy in -> numpy out; tensors come back on the device of ``graph.row_ptr``.

    Not differentiable (indices)."""
    Q = _graph_queries(graph)
    args, finish = _marshal((("row_ptr", graph.row_ptr), ("col", graph.col)))
    return finish(ops.csr_edge_rows(args["row_ptr"], Q, int(args["col"].shape[0])))


def radius_edge_distance_features(xyz, graph, atom_mask=None, pairs=BACKBONE_PAIRS, centers=None, sigma=None, return_dist=False,
                                  source_xyz=None, source_mask=None):
    """``edge_distance_features`` along the edges of a ``RadiusGraph``: ``rbf`` (E, P*R) fp32 or, with ``return_dist``,
    ``(rbf, dist)`` with ``dist`` (E, P), one row per entry of ``graph.col`` -- flat over the batch, lists of any length, no
    padding to a ``k``.  ``xyz`` (B,M,A,3) are the residues ``col`` indexes (``atom_mask`` (B,M,A)); the sources, the rows
    of the graph, are ``source_xyz`` (B,Q,As,3) with ``source_mask`` (B,Q,As) where the graph was made with ``queries``, and
    the same residues otherwise.  ``pairs`` are (slot on the source, slot on the neighbour); ``centers`` / ``sigma`` default
    to ``rbf_centers()``.  The values are ``edge_distance_features``' on the same edges, bit for bit; exactly 0 where
    either atom is outside its mask and on every position that is no edge -- from ``row_ptr[-1]`` on, and wherever ``col``
    is outside [0, M) -- and NaN there never reaches the result.  One HIP kernel (``ops.csr_edge_rbf``) that cuts its work
    by edge position, so load balance does not depend on row lengths; nothing gathered or broadcast is built; no host
    read.  For an atom graph pass the zero-copy view ``xyz.reshape(B, N*A, 1, 3)`` with ``pairs=((0, 0),)``.
    numpy in -> numpy out; tensors come back on the device of ``xyz``, CPU tensors included.

    Differentiable with respect to ``xyz`` and ``source_xyz``, like ``edge_distance_features`` and by the same kernels (K52,
    K53): where one of them requires grad the outputs carry a graph; the graph itself, ``centers`` and ``sigma`` take no
    gradient.  The backward pass makes no host read either, so it runs inside ``torch.cuda.graph`` behind a ``max_edges``
    graph.  Not differentiable with respect to anything else, and where neither requires grad the outputs carry no graph."""
    if (centers is None) != (sigma is None):
        raise ValueError("centers and sigma come together (rbf_centers() returns both)")
    if centers is None:
        centers, sigma = rbf_centers()
    pairs = [tuple(p) for p in pairs]
    if any(len(p) != 2 for p in pairs):
        raise ValueError("pairs must be (slot on the source residue, slot on the neighbour) pairs")
    _graph_queries(graph)
    args, finish = _marshal((("xyz", xyz), ("row_ptr", graph.row_ptr), ("col", graph.col), ("atom_mask", atom_mask),
                             ("src_xyz", source_xyz), ("src_mask", source_mask)))
    tables = dict(pair_i=[p[0] for p in pairs], pair_j=[p[1] for p in pairs], centers=centers, sigma=sigma)
    if _wants_grad(xyz, source_xyz):
        args = _attached(args, xyz=xyz, src_xyz=source_xyz)
        rbf, dist = finish(_EdgeDistanceFeatures.apply(args["xyz"], args.get("src_xyz"), args["row_ptr"], args["col"],
                                                       args.get("atom_mask"), args.get("src_mask"), tables, bool(return_dist)))
    else:
        dist, rbf = finish(ops.csr_edge_rbf(**args, **tables, want_dist=bool(return_dist)))
    return (rbf, dist) if return_dist else rbf


def radius_edge_frame_features(rot, trans, graph, frame_mask=None, source_rot=None, source_trans=None,
                               source_mask=None) -> EdgeFrames:
    """``edge_frame_features`` along the edges of a ``RadiusGraph``: ``EdgeFrames(local_pos (E,3) = R_i^T (t_j - t_i), rel_rot
    (E,3,3) = R_i^T R_j)``, one row per entry of ``graph.col``; i is the edge's source -- a frame of ``source_rot`` (B,Q,3,3),
    ``source_trans`` (B,Q,3), ``source_mask`` (B,Q) where given, else of ``rot`` / ``trans`` / ``frame_mask`` like the
    neighbour j.  ``edge_frame_features``' values on the same edges, bit for bit; exactly 0 where either frame is outside
    its mask and on every position that is no edge.  One HIP kernel (``ops.csr_edge_frames``); no host read.
    numpy in -> numpy out; tensors come back on the device of ``rot``, CPU tensors included.

    Differentiable with respect to ``rot``, ``trans``, ``source_rot`` and ``source_trans``, like ``edge_frame_features`` and by
    the same kernel (K54), with no host read.  Not differentiable with respect to the graph, and where none of the four
    requires grad the outputs carry no graph."""
    _graph_queries(graph)
    args, finish = _marshal((("rot", rot), ("trans", trans), ("row_ptr", graph.row_ptr), ("col", graph.col),
                             ("frame_mask", frame_mask), ("src_rot", source_rot), ("src_trans", source_trans),
                             ("src_mask", source_mask)))
    if _wants_grad(rot, trans, source_rot, source_trans):
        args = _attached(args, rot=rot, trans=trans, src_rot=source_rot, src_trans=source_trans)
        return EdgeFrames(*finish(_EdgeFrameFeatures.apply(args["rot"], args["trans"], args.get("src_rot"), args.get("src_trans"),
                                                           args["row_ptr"], args["col"], args.get("frame_mask"),
                                                           args.get("src_mask"))))
    return EdgeFrames(*finish(ops.csr_edge_frames(**args)))


class IncomingEdges(NamedTuple):
    """The edges of a ``RadiusGraph`` grouped by their target (``radius_graph_incoming``): target ``o = b * n_targets + j``
    receives the edge positions ``edge[ptr[o]:ptr[o + 1]]``."""
    ptr: torch.Tensor    # (B*n_targets+1,) int64; ptr[-1] is the number of real edges
    edge: torch.Tensor   # (E,) int64: positions into graph.col, ascending within a group; from ptr[-1] on, the padding


def radius_graph_incoming(graph, n_targets) -> IncomingEdges:
    """The edges of a ``RadiusGraph`` by the point they arrive at: ``IncomingEdges(ptr (B*n_targets+1,) int64, edge (E,)
    int64)``, E being ``graph.col.shape[0]``.  ``edge[ptr[o]:ptr[o + 1]]`` are the positions p into ``graph.col`` with
    ``col[p] == j`` in structure b, ``o = b * n_targets + j``, ascending.  Positions that are no edge -- from ``row_ptr[-1]``
    on, and wherever ``col`` is outside [0, n_targets) -- are left out of every group: they fill ``edge`` from ``ptr[-1]`` on,
    so the shapes do not depend on the data.  ``n_targets`` is M, the length of the axis ``col`` indexes.  With it a layer
    aggregates messages at the targets in a fixed order -- ``segment_reduce`` over ``messages[edge]``, or a loop -- where
    ``index_add`` uses atomics; it is what the backward pass of the edge features sums by.  Plain torch
    (``ops.csr_incoming_edges``: a stable sort and two ``searchsorted``) on the graph's own device, CPU included; no host
    read, so it runs inside ``torch.cuda.graph`` behind ``radius_graph(max_edges=n)``.  numpy in -> numpy out."""
    Q = _graph_queries(graph)
    arrays = isinstance(graph.row_ptr, np.ndarray)
    row_ptr, col = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t for t in (graph.row_ptr, graph.col))
    out = ops.csr_incoming_edges(row_ptr, col, int(graph.count.shape[0]), Q, n_targets)
    return IncomingEdges(*(t.numpy() if arrays else t for t in out))


def neighbors_to_radius_graph(neighbors_or_idx) -> RadiusGraph:
    """A padded neighbour list -- ``Neighbors`` or its ``idx`` (B,Q,k) -- as CSR lists with the padding dropped:
    ``RadiusGraph(row_ptr (B*Q+1,) int64, col (E,) int32, dist (E,) or None, count (B,Q) int32)``.  Every negative entry is
    padding; the others keep their order within the row (nearest first for ``nearest_neighbors``, not ascending in j).
    ``dist`` is ``Neighbors.dist`` at the entries kept, or None for a bare index tensor.  Gives a kNN graph the flat edge
    list the ``radius_edge_*`` functions take.  Plain torch on the list's own device (mask, ``cumsum``,
    ``masked_select``: the number of edges is read from the device); numpy in -> numpy out.  Not differentiable."""
    idx, dist = (neighbors_or_idx.idx, neighbors_or_idx.dist) if isinstance(neighbors_or_idx, Neighbors) else (neighbors_or_idx, None)
    arrays = isinstance(idx, np.ndarray)
    idx = torch.from_numpy(np.ascontiguousarray(idx)) if arrays else idx
    if not isinstance(idx, torch.Tensor):
        raise TypeError("idx must be a tensor or an ndarray")
    if idx.ndim != 3 or idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool:
        raise ValueError(f"idx must be an integer tensor of shape (B, Q, k), got {idx.dtype} {tuple(idx.shape)}")
    B, Q, _ = idx.shape
    real = idx >= 0
    count = real.sum(-1, dtype=torch.int32)
    row_ptr = torch.zeros(B * Q + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(count.reshape(-1), 0, dtype=torch.int64, out=row_ptr[1:])
    col = torch.masked_select(idx, real).to(torch.int32)
    if dist is not None:
        dist = torch.from_numpy(np.ascontiguousarray(dist)) if isinstance(dist, np.ndarray) else dist
        if tuple(dist.shape) != tuple(idx.shape):
            raise ValueError(f"dist must have shape {tuple(idx.shape)} to match idx, got {tuple(dist.shape)}")
        dist = torch.masked_select(dist.detach().to(idx.device), real)
    out = (row_ptr, col, dist, count)
    return RadiusGraph(*(t if t is None or not arrays else t.numpy() for t in out))


# ---- message passing on a graph: segment sums, gathers, the edge softmax (K55 - K59) --------------------------------------------
class _EdgeLists(NamedTuple):
    """The edge list a message-passing function was called with, on the kernels' device, as CSR lists"""
    row_ptr: torch.Tensor   # (B*Q+1,) int64
    col: torch.Tensor       # (E,) int32
    B: int
    Q: int
    M: int

    def grouping(self, at):
        """``(ptr, perm)`` of the segments ``at`` the sources (the rows themselves) or the targets (the incoming list)"""
        if at == "source":
            return self.row_ptr, None
        return ops.csr_incoming_edges(self.row_ptr, self.col, self.B, self.Q, self.M)

    def index(self, at):
        """(E,) int64: the flat node every edge position has ``at`` its source or target, -1 at the padding; no host read"""
        E = self.col.shape[0]
        batch, row = ops.csr_edge_rows(self.row_ptr, self.Q, E)
        target = self.col.long()
        real = (batch >= 0) & (target >= 0) & (target < self.M)
        flat = batch.long() * self.M + target if at == "target" else batch.long() * self.Q + row.long()
        return torch.where(real, flat, torch.full_like(flat, -1))

    def nodes(self, at) -> int:
        return self.M if at == "target" else self.Q


def _message_graph(graph):
    """``(first, col, B, Q, edge_shape)`` of a ``RadiusGraph`` -- its CSR lists, edge axis (E,) -- or of a padded list, a
    ``Neighbors`` or a bare (B,Q,k) index tensor -- ``(idx, None)``, edge axis (B,Q,k)"""
    if isinstance(graph, RadiusGraph):
        Q = _graph_queries(graph)
        if graph.col.ndim != 1:
            raise ValueError(f"graph.col must have shape (edges,), got {tuple(graph.col.shape)}")
        return graph.row_ptr, graph.col, int(graph.count.shape[0]), Q, (int(graph.col.shape[0]),)
    idx = graph.idx if isinstance(graph, Neighbors) else graph
    if not isinstance(idx, (torch.Tensor, np.ndarray)):
        raise TypeError("graph must be a geometry.RadiusGraph, a geometry.Neighbors or a (B, Q, k) index tensor")
    integer = np.issubdtype(idx.dtype, np.integer) if isinstance(idx, np.ndarray) else ops._is_integer_tensor(idx)
    if idx.ndim != 3 or not integer:
        raise ValueError(f"a padded neighbour list must be an integer tensor of shape (B, Q, k), got {idx.dtype} {tuple(idx.shape)}")
    return idx, None, int(idx.shape[0]), int(idx.shape[1]), tuple(int(n) for n in idx.shape)


def _check_at(at, n_targets, Q: int) -> int:
    """M, the number of targets per structure: ``n_targets`` or, None, Q; ValueError for an ``at`` that is neither end"""
    if at not in ("source", "target"):
        raise ValueError(f"at must be 'source' or 'target', got {at!r}")
    if n_targets is None:
        return Q
    if isinstance(n_targets, bool) or not isinstance(n_targets, (int, np.integer)) or n_targets < 0:
        raise ValueError(f"n_targets must be a non-negative integer, got {n_targets!r}")
    return int(n_targets)


def _edge_tail(t, edge_shape, name: str, what: str, most: int) -> tuple:
    """the axes of the per-edge tensor ``t`` after its edge axis ``edge_shape``: 0 .. ``most`` of them; ValueError otherwise"""
    if not isinstance(t, (torch.Tensor, np.ndarray)):
        raise TypeError(f"{name} must be a tensor or an ndarray")
    shape, n = tuple(t.shape), len(edge_shape)
    floating = np.issubdtype(t.dtype, np.floating) if isinstance(t, np.ndarray) else t.dtype.is_floating_point
    if shape[:n] != tuple(edge_shape) or not (len(shape) - n <= most) or (most == 2 and len(shape) == n):
        raise ValueError(f"{name} must have shape {tuple(edge_shape)} + {what} to match the graph, got {shape}")
    if not floating:
        raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")
    return shape[n:]


def _edge_weight(weight, E: int, H: int):
    """a weight (edges,) or (edges, H) as (E, H): one number per edge serves every head"""
    if weight is None:
        return None
    weight = weight.reshape(E, H if weight.numel() == E * H else 1)   # named sizes: E may be 0
    return weight.expand(E, H) if weight.shape[1] == 1 and H > 1 else weight


def _edge_setup(named, floats, parsed, at, n_targets):
    """What the four functions share: the lists of the graph ``parsed`` by ``_message_graph`` and the named operands on the
    kernels' device (those of ``floats`` that require grad attached), ``finish`` and whether a graph is to be built.  A
    padded (B,Q,k) list is the CSR list ``arange(B*Q + 1) * k`` -- its rows are the Q queries -- with the indices held to
    [0, M), the targets, which a bipartite list has another number of."""
    first, col, B, Q, edge_shape = parsed
    M = _check_at(at, n_targets, Q)
    args, finish = _marshal(tuple(named) + (("first", first), ("col", col)))
    wants = _wants_grad(*floats.values())
    if wants:
        args = _attached(args, **floats)
    if col is not None and tuple(first.shape) != (B * Q + 1,):
        raise ValueError(f"graph.row_ptr must have shape ({B * Q + 1},) to match count {(B, Q)}, got {tuple(first.shape)}")
    first, col = args.pop("first"), args.pop("col", None)
    if col is None:
        col = ops._idx32(first, M).reshape(-1)
        first = torch.arange(B * Q + 1, dtype=torch.int64, device=col.device) * edge_shape[2]
    return args, finish, _EdgeLists(first.to(torch.int64), col, B, Q, M), wants


class _EdgeAggregate(torch.autograd.Function):
    """ops.segment_reduce (K55) with K56 and K57 as its vector-Jacobian product (sum, mean) or a scatter to ``arg`` (max, min)"""

    @staticmethod
    def forward(ctx, messages, weight, row_ptr, col, ptr, perm, dims, at, reduce, return_arg):
        lists = _EdgeLists(row_ptr, col, *dims)
        extreme = reduce in ("max", "min")
        out = ops.segment_reduce(messages, ptr, perm, B=lists.B, Q=lists.Q, M=lists.M, reduce=reduce, weight=weight,
                                 row_ptr=row_ptr, col=col, return_arg=extreme)
        out, arg = out if extreme else (out, None)
        n = None
        if reduce == "mean":   # the 1/n of the backward pass: n is the sum of ones over the same grouping, taken once, here
            ones = torch.ones(messages.shape[0], 1, 1, dtype=torch.float32, device=messages.device)
            n = ops.segment_reduce(ones, ptr, perm, B=lists.B, Q=lists.Q, M=lists.M, row_ptr=row_ptr, col=col).clamp_(min=1.0)
        ctx.dims, ctx.at, ctx.reduce = dims, at, reduce
        ctx.save_for_backward(messages, weight, row_ptr, col, arg, n)
        if return_arg:
            ctx.mark_non_differentiable(arg)
            return out, arg
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_arg=None):
        messages, weight, row_ptr, col, arg, n = ctx.saved_tensors
        lists = _EdgeLists(row_ptr, col, *ctx.dims)
        E, H, D = messages.shape
        g = grad_out.contiguous().float()
        if ctx.reduce in ("max", "min"):   # the destinations are unique: a plain scatter, deterministic
            place = torch.arange(H * D, device=g.device).reshape(1, H, D)
            dest = torch.where(arg >= 0, arg * (H * D) + place, torch.full_like(arg, E * H * D))
            grad = torch.zeros(E * H * D + 1, dtype=g.dtype, device=g.device).scatter_(0, dest.reshape(-1), g.reshape(-1))
            return (grad[:-1].reshape(E, H, D).to(messages.dtype),) + (None,) * 9
        if ctx.reduce == "mean":
            g = g / n
        index = lists.index(ctx.at)
        grad_messages = ops.segment_gather(g, index, weight).to(messages.dtype) if ctx.needs_input_grad[0] else None
        grad_weight = None
        if weight is not None and ctx.needs_input_grad[1]:
            grad_weight = ops.edge_dot(g, messages, index).to(weight.dtype)
        return (grad_messages, grad_weight) + (None,) * 8


class _EdgeGather(torch.autograd.Function):
    """ops.segment_gather (K56) with K55 (the sum at the same end of the edges) and K57 as its vector-Jacobian product"""

    @staticmethod
    def forward(ctx, values, weight, row_ptr, col, dims, at):
        lists = _EdgeLists(row_ptr, col, *dims)
        index = lists.index(at)
        ctx.dims, ctx.at = dims, at
        ctx.save_for_backward(values, weight, row_ptr, col, index)
        return ops.segment_gather(values, index, weight)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        values, weight, row_ptr, col, index = ctx.saved_tensors
        lists = _EdgeLists(row_ptr, col, *ctx.dims)
        g = grad_out.contiguous().float()
        grad_values = grad_weight = None
        if ctx.needs_input_grad[0]:
            ptr, perm = lists.grouping(ctx.at)
            grad_values = ops.segment_reduce(g, ptr, perm, B=lists.B, Q=lists.Q, M=lists.M, weight=weight, row_ptr=row_ptr,
                                             col=col).to(values.dtype)
        if weight is not None and ctx.needs_input_grad[1]:
            grad_weight = ops.edge_dot(values, g, index).to(weight.dtype)
        return (grad_values, grad_weight) + (None,) * 4


class _EdgeSoftmax(torch.autograd.Function):
    """ops.segment_softmax (K58) with ops.segment_softmax_backward (K59) as its vector-Jacobian product"""

    @staticmethod
    def forward(ctx, logits, row_ptr, col, ptr, perm, dims, return_lse):
        lists = _EdgeLists(row_ptr, col, *dims)
        out = ops.segment_softmax(logits, ptr, perm, B=lists.B, Q=lists.Q, M=lists.M, row_ptr=row_ptr, col=col,
                                  return_lse=return_lse)
        w, lse = out if return_lse else (out, None)
        ctx.dims = dims
        ctx.save_for_backward(w, row_ptr, col, ptr, perm)
        if return_lse:
            ctx.mark_non_differentiable(lse)
            return w, lse
        return w

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_w, _grad_lse=None):
        w, row_ptr, col, ptr, perm = ctx.saved_tensors
        B, Q, M = ctx.dims
        gx = ops.segment_softmax_backward(w, grad_w.contiguous(), ptr, perm, B=B, Q=Q, M=M, row_ptr=row_ptr, col=col)
        return (gx.to(grad_w.dtype),) + (None,) * 6


def _run_aggregate(m3, w2, lists, ptr, perm, at, reduce="sum", return_arg=False):
    """K55 on prepared operands -- with its graph where ``m3`` (E,H,D) or ``w2`` (E,H) requires grad, alone otherwise"""
    if _wants_grad(m3, w2):
        return _EdgeAggregate.apply(m3, w2, lists.row_ptr, lists.col, ptr, perm, (lists.B, lists.Q, lists.M), at, reduce,
                                    bool(return_arg))
    return ops.segment_reduce(m3, ptr, perm, B=lists.B, Q=lists.Q, M=lists.M, reduce=reduce, weight=w2, row_ptr=lists.row_ptr,
                              col=lists.col, return_arg=bool(return_arg))


def _run_softmax(x2, lists, ptr, perm, return_lse=False):
    """K58 on prepared logits (E,H) -- with its graph where they require grad, alone otherwise"""
    if _wants_grad(x2):
        return _EdgeSoftmax.apply(x2, lists.row_ptr, lists.col, ptr, perm, (lists.B, lists.Q, lists.M), bool(return_lse))
    return ops.segment_softmax(x2, ptr, perm, B=lists.B, Q=lists.Q, M=lists.M, row_ptr=lists.row_ptr, col=lists.col,
                               return_lse=bool(return_lse))


def _weight_tail_fits(wtail, tail) -> bool:
    return wtail in ((), (1,), (tail[0],) if len(tail) == 2 else (1,))


def edge_aggregate(messages, graph, *, at="source", n_targets=None, reduce="sum", weight=None, return_arg=False):
    """The sum, mean, max or min (``reduce``) of per-edge ``messages`` at every node of a graph: (B, Q, ...) at the sources of
    the edges -- the rows of the graph -- or, with ``at="target"``, (B, n_targets, ...) at the points ``col`` names
    (``n_targets`` defaults to Q and is required for a bipartite graph).  ``graph`` is a ``RadiusGraph``, with ``messages``
    (E, C) or (E, H, D), one row per entry of ``graph.col``, or a padded list -- a ``Neighbors`` or its ``idx`` (B,Q,k) --,
    with ``messages`` (B, Q, k, C) or (B, Q, k, H, D).  ``weight`` -- (E,) or (E, H); (B,Q,k) or (B,Q,k,H) -- multiplies every
    message per head before the sum (sum and mean only; no (E,H,D) product is built).  With ``return_arg`` (max, min) the
    result is ``(out, arg)``, ``arg`` int64 the winning edge position (flat over (B,Q,k) for a padded list), -1 at a node
    without edges.  Nothing is read at the padding -- from ``row_ptr[-1]`` on, and wherever ``col`` is outside [0, n_targets),
    the -1 of a padded list included --, so NaN there never reaches a result.  One HIP kernel (``ops.segment_reduce``, K55):
    every node sums its own edges in ascending order, in double from +0, and rounds once -- no atomics, defined bit for
    bit; the targets' lists come from ``ops.csr_incoming_edges``; a node without edges gets exactly +0.  Lists are not
    split, so the time is that of the longest list.  No host read: it runs inside ``torch.cuda.graph`` behind
    ``radius_graph(max_edges=n)``.  numpy in -> numpy out; tensors come back on the device of ``messages``.

    Differentiable with respect to ``messages`` and ``weight`` (not twice, and not with respect to the graph): the backward
    pass of sum and mean is ``ops.segment_gather`` (K56) and ``ops.edge_dot`` (K57); that of max and min a scatter to ``arg``,
    whose destinations are unique.  Where neither requires grad the forward kernel runs alone."""
    if reduce not in ops.AGGREGATE_MODES:
        raise ValueError(f"reduce must be one of {', '.join(ops.AGGREGATE_MODES)}, got {reduce!r}")
    if reduce in ("max", "min") and weight is not None:
        raise ValueError(f"reduce={reduce!r} takes no weight")
    if return_arg and reduce in ("sum", "mean"):
        raise ValueError(f"reduce={reduce!r} has no arg: return_arg goes with max and min")
    parsed = _message_graph(graph)
    edge_shape = parsed[4]
    tail = _edge_tail(messages, edge_shape, "messages", "(C,) or (H, D)", 2)
    if weight is not None:
        wtail = _edge_tail(weight, edge_shape, "weight", "() or (H,)", 1)
        if not _weight_tail_fits(wtail, tail):
            raise ValueError(f"weight must hold one number per edge or per head, got {wtail} for messages {tail}")
    args, finish, lists, _ = _edge_setup((("messages", messages), ("weight", weight)), dict(messages=messages, weight=weight),
                                         parsed, at, n_targets)
    E = lists.col.shape[0]
    H, D = tail if len(tail) == 2 else (1, tail[0])
    m3 = args["messages"].reshape(E, H, D)
    w2 = _edge_weight(args.get("weight"), E, H)
    out = _run_aggregate(m3, w2, lists, *lists.grouping(at), at, reduce, return_arg)
    shape = (lists.B, lists.nodes(at)) + tuple(tail)
    if return_arg:
        return finish((out[0].reshape(shape), out[1].reshape(shape)))
    return finish((out.reshape(shape),))[0]


def edge_gather(values, graph, *, at="target", n_targets=None, weight=None):
    """A node's features on every edge of a graph: ``values`` (B, M, ...) of the edges' targets -- ``values[b, col[p]]`` -- or,
    with ``at="source"``, (B, Q, ...) of their sources, as (E, ...) for a ``RadiusGraph`` and (B, Q, k, ...) for a padded list
    (``Neighbors`` or ``idx``); ``...`` is (C,) or (H, D), and M is read off ``values`` (``n_targets`` where ``at="source"`` and
    the graph is bipartite).  ``weight`` -- one number per edge, or per edge and head -- multiplies the row, rounded once.  The
    result is exactly 0 at the padding, and nothing is read there.  The CSR counterpart of ``gather_neighbors``, which stays
    as it is.  One HIP kernel (``ops.segment_gather``, K56) behind ``ops.csr_edge_rows``; no host read, so it runs inside
    ``torch.cuda.graph``.  numpy in -> numpy out; tensors come back on the device of ``values``.

    Differentiable with respect to ``values`` and ``weight`` (not twice, and not with respect to the graph): the gradient
    of ``values`` is the sum of the incoming rows at the same end of the edges (``ops.segment_reduce``, K55: fixed order, no
    atomics), that of ``weight`` ``ops.edge_dot`` (K57)."""
    parsed = _message_graph(graph)
    _, _, B, Q, edge_shape = parsed
    if not isinstance(values, (torch.Tensor, np.ndarray)):
        raise TypeError("values must be a tensor or an ndarray")
    if at not in ("source", "target"):
        raise ValueError(f"at must be 'source' or 'target', got {at!r}")
    shape = tuple(values.shape)
    floating = np.issubdtype(values.dtype, np.floating) if isinstance(values, np.ndarray) else values.dtype.is_floating_point
    if len(shape) not in (3, 4) or shape[0] != B or (at == "source" and shape[1] != Q) or not floating:
        raise ValueError(f"values must be a floating-point tensor of shape ({B}, {'M' if at == 'target' else Q}, C) or "
                         f"(.., H, D) to match the graph, got {values.dtype} {shape}")
    if at == "target":
        n_targets = shape[1]
    tail = shape[2:]
    if weight is not None:
        wtail = _edge_tail(weight, edge_shape, "weight", "() or (H,)", 1)
        if not _weight_tail_fits(wtail, tail):
            raise ValueError(f"weight must hold one number per edge or per head, got {wtail} for values {tail}")
    args, finish, lists, wants = _edge_setup((("values", values), ("weight", weight)), dict(values=values, weight=weight),
                                             parsed, at, n_targets)
    E = lists.col.shape[0]
    H, D = tail if len(tail) == 2 else (1, tail[0])
    v3 = args["values"].reshape(B * lists.nodes(at), H, D)
    w2 = _edge_weight(args.get("weight"), E, H)
    if wants:
        out = _EdgeGather.apply(v3, w2, lists.row_ptr, lists.col, (lists.B, lists.Q, lists.M), at)
    else:
        out = ops.segment_gather(v3, lists.index(at), w2)
    return finish((out.reshape(tuple(edge_shape) + tuple(tail)),))[0]


def edge_softmax(logits, graph, *, at="source", n_targets=None, return_lse=False):
    """The softmax of attention ``logits`` over the edges of every node of a graph -- over every row (``at="source"``) or over
    the edges that arrive at every target (``at="target"``; ``n_targets`` as in ``edge_aggregate``): the weights, of the
    shape of ``logits`` -- (E,) or (E, H) for a ``RadiusGraph``, (B,Q,k) or (B,Q,k,H) for a padded list, each head on its own
    -- or, with ``return_lse``, ``(w, lse)`` with ``lse`` (B, nodes) or (B, nodes, H), the logarithm of every node's sum.  One
    HIP kernel (``ops.segment_softmax``, K58): the maximum is subtracted, the exponentials are evaluated and summed in
    double in ascending order and each weight is rounded once; no temporaries, no atomics, repeatable bit for bit.  A node
    with one edge gives exactly 1; a logit of -inf gives 0; a node without edges, or with -inf on all of them, gives zeros
    and ``lse`` -inf; the weights are exactly 0 at the padding and nothing is read there.  No host read, so it runs inside
    ``torch.cuda.graph``.  numpy in -> numpy out; tensors come back on the device of ``logits``.

    Differentiable with respect to ``logits`` (``ops.segment_softmax_backward``, K59; not twice); ``lse`` carries no graph."""
    parsed = _message_graph(graph)
    edge_shape = parsed[4]
    tail = _edge_tail(logits, edge_shape, "logits", "() or (H,)", 1)
    args, finish, lists, _ = _edge_setup((("logits", logits),), dict(logits=logits), parsed, at, n_targets)
    E = lists.col.shape[0]
    x2 = args["logits"].reshape(E, tail[0] if tail else 1)
    out = _run_softmax(x2, lists, *lists.grouping(at), return_lse)
    if return_lse:
        return finish((out[0].reshape(tuple(edge_shape) + tail), out[1].reshape((lists.B, lists.nodes(at)) + tail)))
    return finish((out.reshape(tuple(edge_shape) + tail),))[0]


def edge_attention(logits, values, graph, *, at="source", n_targets=None):
    """One attention step over a graph: every node's softmax-weighted sum of the ``values`` on its edges,
    ``edge_aggregate(values, graph, weight=edge_softmax(logits, graph))`` -- (B, nodes, C) or (B, nodes, H, D) from ``logits``
    (E,) or (E, H) and ``values`` (E, C) or (E, H, D) (for a padded list the edge axis is (B,Q,k)).  It is COMPOSED of the two
    functions, on one set of lists (at the targets the incoming list is built once): two HIP kernels forwards (K58, K55),
    K56, K57 and K59 backwards, and no (E,H,D) product of weights and values is built; a single fused kernel is not part of
    this version.  Differentiable with respect to ``logits`` and
    ``values``; everything ``edge_softmax`` and ``edge_aggregate`` say about order, padding and running inside
    ``torch.cuda.graph`` holds::

        g = radius_graph(x, 10.0, mask, max_edges=n)
        rbf = radius_edge_distance_features(xyz, g)                    # (E, P*R)
        out = edge_attention(rbf @ w_logit, (rbf @ w_value).reshape(-1, H, D), g)   # (B, N, H, D); backward() reaches the weights and xyz
    """
    parsed = _message_graph(graph)
    edge_shape = parsed[4]
    ltail = _edge_tail(logits, edge_shape, "logits", "() or (H,)", 1)
    tail = _edge_tail(values, edge_shape, "values", "(C,) or (H, D)", 2)
    if not _weight_tail_fits(ltail, tail):
        raise ValueError(f"logits must hold one number per edge or per head, got {ltail} for values {tail}")
    args, finish, lists, _ = _edge_setup((("logits", logits), ("values", values)), dict(logits=logits, values=values), parsed, at,
                                         n_targets)
    E = lists.col.shape[0]
    H, D = tail if len(tail) == 2 else (1, tail[0])
    ptr, perm = lists.grouping(at)
    w = _edge_weight(_run_softmax(args["logits"].reshape(E, ltail[0] if ltail else 1), lists, ptr, perm), E, H)
    out = _run_aggregate(args["values"].reshape(E, H, D), w, lists, ptr, perm, at)
    return finish((out.reshape((lists.B, lists.nodes(at)) + tuple(tail)),))[0]


class SideChainTorsions(NamedTuple):
    """The side-chain torsions chi1 .. chi4 of every residue (``side_chain_torsions``)."""
    chi: torch.Tensor    # (B,N,4) fp32, radians in [-pi, pi]; exactly 0 where undefined
    mask: torch.Tensor   # (B,N,4) bool: the residue type has the angle and its four atoms are present


class _SideChainTorsions(torch.autograd.Function):
    """ops.chi with ops.chi_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, xyz, residue_type, atom_mask, chi_atoms):
        ctx.chi_atoms = chi_atoms
        ctx.save_for_backward(xyz, residue_type, atom_mask)
        ctx.dtype = xyz.dtype
        chi, mask = ops.chi(xyz, residue_type, atom_mask, chi_atoms=chi_atoms)
        ctx.mark_non_differentiable(mask)
        return chi, mask

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_chi, _grad_mask):
        xyz, residue_type, atom_mask = ctx.saved_tensors
        grad = ops.chi_backward(xyz, residue_type, grad_chi, atom_mask, chi_atoms=ctx.chi_atoms)
        return grad.to(ctx.dtype), None, None, None


def side_chain_torsions(xyz, residue_type, atom_mask=None, chi_atoms=None) -> SideChainTorsions:
    """The side-chain torsions chi1 .. chi4 of ``xyz`` (B,N,A,3): ``SideChainTorsions(chi (B,N,4) fp32, mask (B,N,4)
    bool)``.  ``residue_type`` (B,N) integers selects each residue's row of ``chi_atoms`` (T,4,4), the atom slots a, b,
    c, d of every angle (None: ``general.chi_atom_table()``, indexed by ``pdb.ONE_TO_INDEX``); a type outside [0, T) is
    padding.  An angle is defined where the table has it and its four atoms are in ``atom_mask`` (B,N,A; None = all):
    ``chi = atan2((m . b1) / |b1|, n1 . n2)`` with ``b0 = a - b, b1 = c - b, b2 = d - c, n1 = b0 x b1, n2 = b2 x b1, m = n1 x
    n2`` -- the sign of ``dihedral`` and of IUPAC --, evaluated in double on the float32 coordinates and rounded once.
    Undefined angles are exactly 0 with mask False, value and gradient, whatever NaN sits under the mask.
    Differentiable with respect to ``xyz`` (nothing else); one HIP kernel forwards (``ops.chi``) and one backwards
    (``ops.chi_backward``, deterministic).  No double backward.  Tensors on the GPU."""
    if chi_atoms is None:
        from .general import chi_atom_table
        chi_atoms = chi_atom_table()
    ops.check_chi_shapes(xyz, residue_type, atom_mask, chi_atoms)
    return SideChainTorsions(*_SideChainTorsions.apply(xyz, residue_type, atom_mask, chi_atoms))


class _SetSideChainTorsions(torch.autograd.Function):
    """ops.chi_set with ops.chi_set_backward as its vector-Jacobian product towards the angles."""

    @staticmethod
    def forward(ctx, xyz, chi, residue_type, atom_mask, chi_select, relative, chi_atoms, chi_last):
        out = ops.chi_set(xyz, chi, residue_type, atom_mask, chi_select, chi_atoms=chi_atoms, chi_last=chi_last,
                          relative=relative)
        ctx.tables = dict(chi_atoms=chi_atoms, chi_last=chi_last)
        ctx.save_for_backward(out, residue_type, atom_mask, chi_select)
        ctx.dtype = chi.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        out, residue_type, atom_mask, chi_select = ctx.saved_tensors
        grad = ops.chi_set_backward(out, grad_out, residue_type, atom_mask, chi_select, **ctx.tables)
        return None, grad.to(ctx.dtype), None, None, None, None, None, None


def set_side_chain_torsions(xyz, chi, residue_type, atom_mask=None, chi_select=None, relative=False, chi_atoms=None,
                            chi_last=None):
    """``xyz`` (B,N,A,3) with the side chains turned to the angles ``chi`` (B,N,4), or by them with ``relative``: a new
    (B,N,A,3) fp32 tensor.  ``chi_atoms`` (T,4,4) names the four atoms of every angle and ``chi_last`` (T,4) the last atom
    slot it moves (None: ``general.chi_atom_table()`` and ``general.chi_last_table()``); ``residue_type`` (B,N) selects
    the rows, a type outside [0, T) is padding.  For k = 0..3 in this order, where the angle is defined
    (``side_chain_torsions``), ``chi_last`` is not -1 (proline's angles are measured but never turned: that would open
    the ring) and ``chi_select`` (B,N,4; None = all) is true, the present atoms from the angle's fourth atom through
    ``chi_last`` are rotated about its b -> c axis by ``chi[k]`` minus the angle measured on the current coordinates (by
    ``chi[k]`` with ``relative``), in double, rounded once.  Every other float is the input's own -- missing atoms' NaN,
    the padding --, and ``chi`` may hold anything, NaN included, where it is not used.

    Differentiable with respect to ``chi``: ``grad_chi[k] = sum_s (u_k x (p_s - c_k)) . grad_s`` over the atoms angle k
    moved, which is the whole derivative in both modes (``ops.chi_set_backward``, one HIP kernel, deterministic; exactly
    0 at angles that were not turned).  NOT differentiable with respect to ``xyz``, which is a constant of this
    function: an ``xyz`` that requires grad raises ValueError rather than lose its gradient silently -- pass
    ``xyz.detach()``.  No double backward.  Tensors on the GPU."""
    if chi_atoms is None:
        from .general import chi_atom_table
        chi_atoms = chi_atom_table()
    if chi_last is None:
        from .general import chi_last_table
        chi_last = chi_last_table()
    ops.check_chi_set_shapes(xyz, chi, residue_type, atom_mask, chi_select, chi_atoms, chi_last)
    if isinstance(xyz, torch.Tensor) and xyz.requires_grad:
        raise ValueError("set_side_chain_torsions: xyz is a constant here and gets no gradient, but it requires grad; "
                         "pass xyz.detach() (only chi is differentiable)")
    return _SetSideChainTorsions.apply(xyz, chi, residue_type, atom_mask, chi_select, bool(relative), chi_atoms, chi_last)


class ClosestAtoms(NamedTuple):
    """How close every pair of residues comes, and between which atoms (``closest_atom_distances``)."""
    dist: torch.Tensor     # (B,N,N) fp32: the smallest distance between an atom of i and an atom of j; +inf where none
    atom_i: torch.Tensor   # (B,N,N) int16: the slot of the row residue's atom; -1 where none
    atom_j: torch.Tensor   # (B,N,N) int16: the slot of the column residue's atom; -1 where none


class _ClosestAtoms(torch.autograd.Function):
    """ops.closest_atoms with ops.closest_atoms_backward as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, xyz, atom_mask, cutoff):
        dist, pair = ops.closest_atoms(xyz, atom_mask, cutoff)
        ctx.save_for_backward(xyz, pair)
        ctx.dtype = xyz.dtype
        ctx.mark_non_differentiable(pair)
        return dist, pair

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dist, _grad_pair):
        xyz, pair = ctx.saved_tensors
        return ops.closest_atoms_backward(xyz, pair, grad_dist).to(ctx.dtype), None, None


def closest_atom_distances(xyz, atom_mask=None, cutoff=float("inf")) -> ClosestAtoms:
    """The smallest distance between any atom of residue i and any atom of residue j of ``xyz`` (B,N,A,3), with the atom
    pair that attains it: ``ClosestAtoms(dist (B,N,N) fp32, atom_i (B,N,N) int16, atom_j (B,N,N) int16)`` -- what contact
    maps, interface residues and the fraction of native contacts are defined by.  Only atoms in ``atom_mask`` (B,N,A; None =
    all) take part, and NaN under the mask never reaches a result.  Squared distances are compared in double on the
    float32 coordinates; among equal ones the lower slot of the earlier residue wins, then the lower slot of the later
    one, so the result is defined bit for bit and exactly symmetric: ``dist[b,j,i] = dist[b,i,j]``, ``atom_i[b,j,i] =
    atom_j[b,i,j]``.  ``atom_i`` is always a slot of the row residue and ``atom_j`` one of the column residue.  Where no
    atom pair counts -- a residue without atoms, or nothing within ``cutoff`` (inclusive) -- ``dist`` is +inf and both
    slots are -1.  On the diagonal ``dist`` is 0 and both slots are the residue's lowest present one.  A finite ``cutoff``
    lets the kernel skip residue pairs that are far apart.  One HIP kernel (``ops.closest_atoms``); the (B,N,N,A,A) tensor
    of ``pairwise_distance_matrix`` is never built.

    Differentiable with respect to ``xyz`` (a second HIP kernel, ``ops.closest_atoms_backward``, deterministic): the
    gradient of ``dist[b,i,j]`` flows to its two recorded atoms only, as for ``amin``; entries that are +inf, and pairs
    at distance 0 -- the diagonal --, pass none, so masking with ``torch.where(dist.isfinite(), ...)`` downstream is safe.
    No double backward.  Tensors on the GPU."""
    ops.check_closest_atoms_shapes(xyz, atom_mask, cutoff)
    A = xyz.shape[2]
    dist, pair = _ClosestAtoms.apply(xyz, atom_mask, float(cutoff))
    none = pair < 0
    atom_i = torch.div(pair, A, rounding_mode="floor").masked_fill(none, -1)
    atom_j = torch.remainder(pair, A).masked_fill(none, -1)
    return ClosestAtoms(dist, atom_i, atom_j)


# ---- the pair heads: distogram, predicted aligned error, pTM (K33 - K36) -----------------------------------------------------
def _linspace_breaks(first: float, last: float, n_bins: int, what: str) -> torch.Tensor:
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 2 <= n_bins <= ops.PAIRHEAD_MAX_BINS:
        raise ValueError(f"{what}: 2 .. {ops.PAIRHEAD_MAX_BINS} bins, got {n_bins!r}")
    return torch.from_numpy(np.linspace(float(first), float(last), int(n_bins) - 1, dtype=np.float64).astype(np.float32))


def distogram_breaks(first: float = 2.3125, last: float = 21.6875, n_bins: int = 64) -> torch.Tensor:
    """The ``n_bins - 1`` bin edges of a distogram head, ``linspace(first, last, n_bins - 1)`` as float32 on the host
    (AlphaFold 2's defaults): bin 0 is everything up to ``first``, the last bin everything beyond ``last``."""
    return _linspace_breaks(first, last, n_bins, "distogram_breaks")


def aligned_error_breaks(max_bin: float = 31.0, n_bins: int = 64) -> torch.Tensor:
    """The ``n_bins - 1`` bin edges of a predicted-aligned-error head, ``linspace(0, max_bin, n_bins - 1)`` as float32 on the
    host (AlphaFold 2's defaults)."""
    return _linspace_breaks(0.0, max_bin, n_bins, "aligned_error_breaks")


def aligned_error_bin_centers(max_bin: float = 31.0, n_bins: int = 64) -> torch.Tensor:
    """The ``n_bins`` bin centres that go with ``aligned_error_breaks``: every break plus half a step, and the last of these
    plus a whole step for the open last bin (AlphaFold 2's ``_calculate_bin_centers``); float64 on the host."""
    breaks = aligned_error_breaks(max_bin, n_bins).double()
    step = breaks[1] - breaks[0] if breaks.numel() > 1 else breaks[0]
    centers = breaks + step / 2
    return torch.cat([centers, centers[-1:] + step])


class _BinnedCrossEntropy(torch.autograd.Function):
    """ops.binned_cross_entropy (K34) with ops.binned_cross_entropy_backward (K35) as its vector-Jacobian product."""

    @staticmethod
    def forward(ctx, logits, bins):
        row_loss, row_count = ops.binned_cross_entropy(logits, bins)
        # nothing of the forward's arithmetic is kept: the backward kernel recomputes the softmax from the logits
        ctx.save_for_backward(logits, bins)
        ctx.dtype = logits.dtype
        ctx.mark_non_differentiable(row_count)
        return row_loss, row_count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_row, _grad_count):
        logits, bins = ctx.saved_tensors
        return ops.binned_cross_entropy_backward(logits, bins, grad_row).to(ctx.dtype), None


def binned_cross_entropy(logits, bins, eps: float = 1e-6) -> torch.Tensor:
    """Mean cross-entropy of ``logits`` (B,N,N,C) against the labels ``bins`` (B,N,N) per structure, ``(B,)`` fp32: the sum
    of ``lse(x_ij) - x_ij[bins_ij]`` over the pairs whose label is in ``[0, C)`` divided by ``eps`` plus their number.  A
    label outside the range -- the 255 of ``ops.pair_bins_*`` -- is "no target": the pair counts nowhere and its logits,
    NaN included, never reach the loss or a gradient.  Differentiable with respect to ``logits`` only; forward and
    backward are one pass over the logits each (``ops.binned_cross_entropy``, ``ops.binned_cross_entropy_backward``) and
    neither builds a log-softmax or softmax tensor.  A structure without a labelled pair has loss 0 and zero gradients.
    No double backward."""
    ops._check_scalar(eps, "eps", "non-negative")
    row_loss, row_count = _BinnedCrossEntropy.apply(logits, bins.detach())
    return (row_loss.double().sum(dim=1) / (float(eps) + row_count.sum(dim=1).double())).float()


def distogram_loss(logits, points, point_mask=None, breaks=None, eps: float = 1e-6) -> torch.Tensor:
    """AlphaFold 2's distogram loss per structure, ``(B,)``: ``binned_cross_entropy`` of ``logits`` (B,N,N,C) against the
    bins of the distances between ``points`` (B,N,3) -- pseudo-beta atoms, usually -- over the pairs both of whose points
    are in ``point_mask`` (B,N; None = all), the diagonal included.  ``breaks``: ``C - 1`` bin edges, default
    ``distogram_breaks(n_bins=C)``.  The bins are piecewise constant in the coordinates, so ``points`` is used detached and
    the gradient flows to ``logits`` only.  Two fused passes (``ops.pair_bins_distance``, K34); the only (B,N,N) tensor is
    the byte per pair that holds the bin."""
    C = logits.shape[-1]
    table = distogram_breaks(n_bins=C) if breaks is None else breaks
    bins = ops.pair_bins_distance(points.detach(), table, point_mask, point_mask)
    return binned_cross_entropy(logits, bins, eps)


def aligned_error(rot, trans, points, target_rot, target_trans, target_points, frame_mask=None, point_mask=None) -> torch.Tensor:
    """The aligned-error matrix between a prediction and a target, ``(B,N,N)`` fp32: ``e[b,i,j] = |R_i^T (x_j - t_i) - R*_i^T
    (x*_j - t*_i)|``, the error of point j seen from frame i -- what FAPE averages and a PAE head is trained on.  ``rot``
    (B,N,3,3) has the basis vectors as columns; ``points`` (B,N,3).  +inf where frame i is not in ``frame_mask`` or point j
    not in ``point_mask`` (B,N; None = all).  Computed in double on the float32 inputs and rounded once; not differentiable
    (every input is used detached)."""
    operands = [t.detach() for t in (rot, trans, points, target_rot, target_trans, target_points)]
    return ops.pair_bins_aligned_error(*operands, aligned_error_breaks(), frame_mask, point_mask, return_value=True)[1]


def aligned_error_loss(logits, rot, trans, points, target_rot, target_trans, target_points, frame_mask=None, point_mask=None,
                       breaks=None, eps: float = 1e-8) -> torch.Tensor:
    """AlphaFold 2's predicted-aligned-error loss per structure, ``(B,)``: ``binned_cross_entropy`` of ``logits`` (B,N,N,C)
    against the bins of ``aligned_error`` over the pairs (frame i in ``frame_mask``, point j in ``point_mask``).
    ``breaks``: ``C - 1`` bin edges, default ``aligned_error_breaks(n_bins=C)``.  The bins are piecewise constant in the
    geometry, so all six geometry inputs are used detached and the gradient flows to ``logits`` only."""
    C = logits.shape[-1]
    table = aligned_error_breaks(n_bins=C) if breaks is None else breaks
    operands = [t.detach() for t in (rot, trans, points, target_rot, target_trans, target_points)]
    bins = ops.pair_bins_aligned_error(*operands, table, frame_mask, point_mask)
    return binned_cross_entropy(logits, bins, eps)


def predicted_aligned_error(logits, max_bin: float = 31.0) -> torch.Tensor:
    """The expected aligned error under a PAE head's ``logits`` (B,N,N,C), ``(B,N,N)`` fp32: ``sum_k softmax(x_ij)_k c_k`` with
    the bin centres ``aligned_error_bin_centers(max_bin, C)``.  One pass (``ops.binned_expectation``); not differentiable."""
    B, C = logits.shape[0], logits.shape[-1]
    centers = aligned_error_bin_centers(max_bin, C).to(device=logits.device, dtype=torch.float32)
    return ops.binned_expectation(logits.detach(), centers.expand(B, 1, C))[0]


def contact_probability(logits, cutoff: float = 8.0, breaks=None) -> torch.Tensor:
    """The probability a distogram head's ``logits`` (B,N,N,C) give to a distance of at most ``cutoff``, ``(B,N,N)`` fp32:
    the softmax mass of the bins whose upper edge is ``<= cutoff`` (the open last bin has none).  ``breaks``: the ``C - 1``
    edges, default ``distogram_breaks(n_bins=C)``.  One pass (``ops.binned_expectation``); not differentiable."""
    B, C = logits.shape[0], logits.shape[-1]
    table = ops._check_breaks(distogram_breaks(n_bins=C) if breaks is None else breaks)
    if table.size != C - 1:
        raise ValueError(f"{C - 1} breaks for logits of {C} bins, got {table.size}")
    ops._check_scalar(cutoff, "cutoff", "non-negative")
    inside = np.zeros(C, dtype=np.float32)
    inside[:C - 1] = table <= np.float32(cutoff)
    return ops.binned_expectation(logits.detach(), torch.from_numpy(inside).to(logits.device).expand(B, 1, C))[0]


def predicted_tm_score(logits, residue_mask, chain_idx=None, interface: bool = False, max_bin: float = 31.0) -> torch.Tensor:
    """AlphaFold's predicted TM-score (pTM; ipTM with ``interface``) per structure, ``(B,)`` fp32, from a PAE head's
    ``logits`` (B,N,N,C), exactly its formula: with ``n`` the residues in ``residue_mask`` (B,N), ``d0 = 1.24 (max(n, 19) -
    15)^(1/3) - 1.8`` per structure; the term of a pair is ``sum_k softmax(x_ij)_k / (1 + (c_k / d0)^2)`` over the bin
    centres ``c_k`` (one pass over the logits, ``ops.binned_expectation``); the pair mask ``pm`` is ``mask_i mask_j``, times
    ``chain_i != chain_j`` (``chain_idx`` (B,N)) with ``interface``; per row ``sum_j term pm / (1e-8 + sum_j pm)``, times
    ``mask_i``; the result is the maximum over ``i``.  The (B,N,N) tail is plain torch in float64.  Not differentiable."""
    ops.check_binned_shapes(logits)
    B, N, _, C = logits.shape
    ops._check_optional(residue_mask, (B, N), "residue_mask", "logits", tuple(logits.shape))
    if interface and chain_idx is None:
        raise ValueError("interface=True needs chain_idx")
    ops._check_optional(chain_idx, (B, N), "chain_idx", "logits", tuple(logits.shape))
    mask = (residue_mask.to(logits.device) != 0).double()
    n = mask.sum(dim=1).clamp(min=19.0)
    d0 = 1.24 * (n - 15.0) ** (1.0 / 3.0) - 1.8
    centers = aligned_error_bin_centers(max_bin, C).to(logits.device)
    kernel = 1.0 / (1.0 + (centers[None, :] / d0[:, None]) ** 2)                     # (B,C) float64
    term = ops.binned_expectation(logits.detach(), kernel.float()[:, None, :])[0].double()
    pair = mask[:, :, None] * mask[:, None, :]
    if interface:
        chain = torch.nan_to_num(chain_idx.to(logits.device).double(), nan=-1.0)
        pair = pair * (chain[:, :, None] != chain[:, None, :])
    term = torch.where(pair > 0, term, torch.zeros_like(term))       # whatever the logits of the padding hold stays out
    per_row = term.sum(dim=-1) / (1e-8 + pair.sum(dim=-1))
    return (per_row * mask).amax(dim=1).float()


# ---- superposition scores: aligned RMSD, TM-score, GDT (K37 - K40) -------------------------------------------------------------
class SuperpositionRMSD(NamedTuple):
    """The RMSD after optimal superposition with the transform that attains it (``superposition_rmsd``)."""
    rmsd: torch.Tensor     # (B,) fp32; NaN where no point counts
    rot: torch.Tensor      # (B,3,3) fp32: a proper rotation
    trans: torch.Tensor    # (B,3) fp32: R a + t lies on b


class SuperpositionScore(NamedTuple):
    """A score maximised over superpositions with the transform that attains it (``tm_score``)."""
    score: torch.Tensor    # (B,) fp32
    rot: torch.Tensor      # (B,3,3) fp32
    trans: torch.Tensor    # (B,3) fp32


class SuperpositionScores(NamedTuple):
    """TM-score, GDT-TS and GDT-HA of one search (``superposition_scores``), each (B,) fp32."""
    tm: torch.Tensor
    gdt_ts: torch.Tensor
    gdt_ha: torch.Tensor


GDT_TS_CUTOFFS = (1.0, 2.0, 4.0, 8.0)
GDT_HA_CUTOFFS = (0.5, 1.0, 2.0, 4.0)


class _SuperpositionRMSD(torch.autograd.Function):
    """ops.superpose with ops.superpose_backward as the vector-Jacobian product of its rmsd."""

    @staticmethod
    def forward(ctx, a, b, weight, mask):
        R, t, rmsd, wsum = ops.superpose(a, b, weight, mask)
        ctx.save_for_backward(a, b, weight, mask, R, t, rmsd, wsum)
        ctx.dtypes = (a.dtype, b.dtype)
        ctx.mark_non_differentiable(R, t)
        return rmsd, R, t

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rmsd, _grad_rot, _grad_trans):
        a, b, weight, mask, R, t, rmsd, wsum = ctx.saved_tensors
        grad_a, grad_b = ops.superpose_backward(a, b, weight, mask, R, t, rmsd, wsum, grad_rmsd)
        if grad_b is None and ctx.needs_input_grad[1]:
            raise RuntimeError("superposition_rmsd: a target shared by the batch, b (1,M,3), is a constant and gets no gradient")
        return (grad_a.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None,
                grad_b.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None, None, None)


def superposition_rmsd(a, b, weight=None, mask=None) -> SuperpositionRMSD:
    """The RMSD of ``a`` (B,M,3) against ``b`` (B,M,3), or (1,M,3) as one target for all, after the optimal weighted
    superposition: ``SuperpositionRMSD(rmsd (B,), rot (B,3,3), trans (B,3))`` with ``rmsd = sqrt(sum w |rot a + trans - b|^2 /
    sum w)`` over the points in ``mask`` (B,M; None = all) with ``weight`` (B,M; None = 1) above 0.  The fit and the residuals
    are double arithmetic on the float32 inputs (one HIP kernel, ``ops.superpose``): identical structures give an RMSD at
    the rounding of the coordinates, and NaN under the mask reaches nothing.  No counted point: NaN.

    Differentiable in ``a`` and ``b`` through ``rmsd`` only (a second kernel, ``ops.superpose_backward``): at the optimum the
    derivative through the transform vanishes, so the gradient is the one of the residuals at a fixed transform.  ``rot``,
    ``trans`` and ``weight`` get no gradient; a structure with ``rmsd = 0`` passes none (the gradient of a norm at 0), nor does
    one without points.  No double backward.  Tensors on the GPU."""
    ops.check_superpose_shapes(a, b, weight, mask)
    weight = None if weight is None else weight.detach()
    return SuperpositionRMSD(*_SuperpositionRMSD.apply(a, b, weight, mask))


def tm_d0(length):
    """The distance scale of the TM-score for a target of ``length`` residues: ``1.24 cbrt(L - 15) - 1.8`` for L > 21, else
    0.5, and never below 0.5.  A number gives a float, a tensor a float64 tensor."""
    if isinstance(length, torch.Tensor):
        L = length.double()
        return torch.where(L > 21, (1.24 * torch.sign(L - 15.0) * (L - 15.0).abs() ** (1.0 / 3.0) - 1.8).clamp(min=0.5),
                           torch.full_like(L, 0.5))
    L = float(length)
    return max(0.5, float(1.24 * np.cbrt(L - 15.0) - 1.8)) if L > 21 else 0.5


def _search_operands(a, b, mask, l_norm):
    B, M, _ = ops.check_superpose_shapes(a, b, None, mask, None, None, ops.SUPERPOSE_MAX_POINTS)
    a, b = a.detach(), b.detach()
    if l_norm is None:      # the number of points that count, and 1 for a structure without any (its score is 0 anyway)
        l_norm = (torch.full((B,), float(M), device=a.device) if mask is None
                  else (mask.to(a.device) != 0).sum(dim=1).clamp(min=1).float())
    else:
        l_norm = torch.as_tensor(l_norm, dtype=torch.float32, device=a.device).expand(B).contiguous()
    return a, b, mask, l_norm


def _search(a, b, mask, l_norm, d0, cutoffs, with_tm):
    """One launch of ``ops.superpose_search`` with the objectives (TM at d0 if ``with_tm``, then a count per cutoff) where one
    d0 serves the batch -- it is given, or every structure's ``tm_d0(l_norm)`` is the same --, else one launch per distinct
    d0 over the structures that share it.  The default d0 is read from ``l_norm`` on the host."""
    counts = [(ops.SUPERPOSE_COUNT, float(c)) for c in cutoffs]
    if not with_tm:
        return ops.superpose_search(a, b, mask, l_norm, counts)
    B = a.shape[0]
    scales = [float(d0)] * B if d0 is not None else [tm_d0(x) for x in l_norm.tolist()]
    distinct = sorted(set(scales))
    if len(distinct) <= 1:
        return ops.superpose_search(a, b, mask, l_norm, [(ops.SUPERPOSE_TM, distinct[0] if distinct else 1.0)] + counts)
    n_obj = 1 + len(counts)
    score = torch.empty(B, n_obj, dtype=torch.float32, device=a.device)
    rot = torch.empty(B, n_obj, 3, 3, dtype=torch.float32, device=a.device)
    trans = torch.empty(B, n_obj, 3, dtype=torch.float32, device=a.device)
    for value in distinct:
        idx = torch.tensor([k for k, x in enumerate(scales) if x == value], device=a.device)
        part = ops.superpose_search(a[idx], b[idx] if b.shape[0] == B else b, None if mask is None else mask[idx], l_norm[idx],
                                    [(ops.SUPERPOSE_TM, value)] + counts)
        score[idx], rot[idx], trans[idx] = part
    return score, rot, trans


def tm_score(a, b, mask=None, l_norm=None, d0=None) -> SuperpositionScore:
    """The TM-score of the model ``a`` (B,M,3) against the target ``b`` (B,M,3) with the residue correspondence given:
    ``SuperpositionScore(score (B,), rot (B,3,3), trans (B,3))``, ``score = max over superpositions of sum_i 1 / (1 + d_i^2 /
    d0^2) / l_norm`` over the points in ``mask`` (B,M; None = all).  ``l_norm`` (B,) or a number defaults to the number of
    points that count; ``d0`` defaults to ``tm_d0(l_norm)`` per structure, which is read on the host (pass ``d0`` to keep the
    call free of a synchronisation).  The maximum is taken by the library's seeded search (``ops.superpose_search``,
    include/protstruc_superpose.h), one wave per seed: it is not the TM-score program's search -- another seed schedule,
    the selection radius doubled where that adds 0.5 -- and there is no sequence alignment: for two structures whose
    correspondence is not known (other lengths, insertions, another chain) use ``structure_alignment``.  Deterministic; not
    differentiable."""
    a, b, mask, l_norm = _search_operands(a, b, mask, l_norm)
    score, rot, trans = _search(a, b, mask, l_norm, d0, (), True)
    return SuperpositionScore(*(x[:, 0].clone(memory_format=torch.contiguous_format) for x in (score, rot, trans)))


def gdt(a, b, mask=None, l_norm=None, cutoffs=GDT_TS_CUTOFFS) -> torch.Tensor:
    """The global distance test of ``a`` (B,M,3) against ``b`` (B,M,3), (B,) fp32: the mean over ``cutoffs`` of the largest
    fraction of points (of ``l_norm``, default the points in ``mask``) within the cutoff of their partner under one
    superposition -- the maximum over the superpositions the library's seeded search visits (``tm_score``), one launch with
    one objective per cutoff.  Not LGA's search; no sequence alignment (``structure_alignment`` finds a correspondence where
    none is given).  Not differentiable."""
    a, b, mask, l_norm = _search_operands(a, b, mask, l_norm)
    return _search(a, b, mask, l_norm, None, cutoffs, False)[0].mean(dim=1)


def gdt_ts(a, b, mask=None, l_norm=None) -> torch.Tensor:
    """GDT-TS: ``gdt`` with the cutoffs 1, 2, 4 and 8 A."""
    return gdt(a, b, mask, l_norm, GDT_TS_CUTOFFS)


def gdt_ha(a, b, mask=None, l_norm=None) -> torch.Tensor:
    """GDT-HA: ``gdt`` with the cutoffs 0.5, 1, 2 and 4 A."""
    return gdt(a, b, mask, l_norm, GDT_HA_CUTOFFS)


def superposition_scores(a, b, mask=None, l_norm=None) -> SuperpositionScores:
    """``SuperpositionScores(tm, gdt_ts, gdt_ha)`` of ``a`` (B,M,3) against ``b`` (B,M,3), each (B,), from a single launch of
    six objectives -- TM at ``tm_d0(l_norm)`` and the counts within 0.5, 1, 2, 4 and 8 A -- where one d0 serves the batch
    (``tm_score``); the same numbers as ``tm_score``, ``gdt_ts`` and ``gdt_ha`` give one by one."""
    a, b, mask, l_norm = _search_operands(a, b, mask, l_norm)
    score = _search(a, b, mask, l_norm, None, (0.5, 1.0, 2.0, 4.0, 8.0), True)[0]
    return SuperpositionScores(score[:, 0].clone(memory_format=torch.contiguous_format), score[:, 2:6].mean(dim=1), score[:, 1:5].mean(dim=1))


# ---- structure alignment without a given correspondence (K41 - K44) ---------------------------------------------------------------
class Alignment(NamedTuple):
    """The alignment of one Needleman-Wunsch pass (``needleman_wunsch``)."""
    map: torch.Tensor          # (B,Ma) int32: the column slot aligned to a row slot, or -1; strictly increasing
    n_aligned: torch.Tensor    # (B,) int32
    value: torch.Tensor        # (B,) fp32: the corner value of the DP table


class StructureAlignment(NamedTuple):
    """The alignment of two structures of different lengths (``structure_alignment``)."""
    map: torch.Tensor            # (B,Ma) int32: the slot of b aligned to a slot of a, or -1; strictly increasing
    n_aligned: torch.Tensor      # (B,) int32
    tm_a: torch.Tensor           # (B,) fp32: the TM-score of the aligned pairs normalised by the length of a
    tm_b: torch.Tensor           # (B,) fp32: ... by the length of b
    rmsd: torch.Tensor           # (B,) fp32: the RMSD of the aligned pairs after their own optimal superposition
    rot: torch.Tensor            # (B,3,3) fp32: the transform of tm_b, rot a + trans lies on b
    trans: torch.Tensor          # (B,3) fp32
    search_score: torch.Tensor   # (B,) fp32: what the alignment maximised, at the search's d0, per min(n_a, n_b)
    start: torch.Tensor          # (B,) int32: the start that gave the alignment, 0 threading, 1 secondary structure


def needleman_wunsch(score, gap, mask_a=None, mask_b=None) -> Alignment:
    """One Needleman-Wunsch pass with TM-align's gap rule over ``score`` (B,Ma,Mb): ``Alignment(map (B,Ma) int32, n_aligned
    (B,), value (B,))`` (one HIP kernel, ``ops.nw_align``; the recurrence and its ties are defined bit for bit in
    include/protstruc_structalign.h).  ``gap <= 0`` is charged for leaving an aligned pair; ``mask_a`` (B,Ma) and ``mask_b``
    (B,Mb) select the rows and columns (None = all).  Not differentiable."""
    return Alignment(*ops.nw_align(score.detach(), gap, mask_a, mask_b))


def ca_secondary_structure(points, mask=None) -> torch.Tensor:
    """TM-align's secondary structure of CA traces ``points`` (B,M,3), (B,M) int8: 1 helix, 2 strand, 3 turn, 0 otherwise, -1
    under ``mask`` (``ops.ca_secondary_structure``).  Chain breaks are not looked at."""
    return ops.ca_secondary_structure(points.detach(), mask)


def structure_alignment(a, b, mask_a=None, mask_b=None, d0=None, use_secondary_structure=True) -> StructureAlignment:
    """Align ``a`` (B,Ma,3) onto ``b`` (B,Mb,3) -- CA traces of different lengths -- WITHOUT a given correspondence, in the
    manner of TM-align: ``StructureAlignment(map, n_aligned, tm_a, tm_b, rmsd, rot, trans, search_score, start)``.  The points
    are the slots with ``mask_a`` (B,Ma) / ``mask_b`` (B,Mb) set (None = all); ``map`` (B,Ma) holds for a slot of ``a`` the
    slot of ``b`` aligned to it, or -1.  Two starts -- the best gapless threading, and a Needleman-Wunsch alignment of the
    secondary structure (left out with ``use_secondary_structure=False``) -- are each refined by alternating a
    Needleman-Wunsch pass over the TM terms ``1 / (1 + d^2 / d0^2)`` under the current transform with the seeded
    superposition search over the aligned pairs (``ops.structure_align``, HIP kernels; include/protstruc_structalign.h is
    the definition).  ``d0`` (a number or (B,)) is the scale of that search and defaults to ``tm_d0(min(n_a, n_b))``, which is
    evaluated on the device: the alignment itself reads nothing on the host, and ``search_score`` is its best sum per
    ``min(n_a, n_b)``.

    ``tm_a`` and ``tm_b`` are ``tm_score`` of the aligned pairs normalised by ``n_a`` and by ``n_b`` (its default d0 is read on
    the host: these two calls synchronise), ``rot`` / ``trans`` are those of ``tm_b``, and ``rmsd`` is ``superposition_rmsd`` of the
    aligned pairs.  A pair with an empty side gives a map of -1, scores 0 and NaN elsewhere.  Not TM-align itself: two
    starts instead of five, this library's search instead of TM-score's, no circular permutation.  Deterministic; not
    differentiable."""
    B, Ma, Mb = ops.check_structalign_shapes(a, b, mask_a, mask_b)
    a, b = a.detach(), b.detach()
    dev = a.device
    n_a = torch.full((B,), Ma, device=dev) if mask_a is None else (mask_a.to(dev) != 0).sum(dim=1)
    n_b = torch.full((B,), Mb, device=dev) if mask_b is None else (mask_b.to(dev) != 0).sum(dim=1)
    if d0 is None:
        scale = tm_d0(torch.minimum(n_a, n_b)).float()
    else:
        if not isinstance(d0, torch.Tensor):
            ops._check_scalar(d0, "d0", "positive")
        scale = torch.as_tensor(d0, dtype=torch.float32, device=dev).expand(B).contiguous()
    found, n_aligned, score, _, _, _, start = ops.structure_align(a, b, mask_a, mask_b, scale, use_secondary_structure)
    paired = found >= 0
    partner = b[torch.arange(B, device=dev)[:, None], found.clamp(min=0).long()]       # (B,Ma,3): b through the map
    partner = torch.where(paired[:, :, None], partner, torch.zeros((), dtype=b.dtype, device=dev))
    tm_b = tm_score(a, partner, paired, n_b.clamp(min=1).float())
    tm_a = tm_score(a, partner, paired, n_a.clamp(min=1).float())
    rmsd = superposition_rmsd(a, partner, None, paired).rmsd
    return StructureAlignment(found, n_aligned, tm_a.score, tm_b.score, rmsd, tm_b.rot, tm_b.trans, score, start)


# ---- ensembles: all-against-all superposed RMSD and clustering by a cutoff (K45, K46) ---------------------------------------------
class PairwiseRMSD(NamedTuple):
    """The matrix of RMSDs after optimal superposition between the members of two batches (``pairwise_rmsd``)."""
    rmsd: torch.Tensor     # (Ba,Bb) fp32; NaN where a pair has no point in common
    count: torch.Tensor    # (Ba,Bb) int32: the number of points the pair has in common


class Clusters(NamedTuple):
    """The clusters of a distance matrix (``cluster_by_cutoff``), the largest first."""
    label: torch.Tensor        # (G,B) int32: the cluster of an item, -1 where it is not valid
    center: torch.Tensor       # (G,B) int32: the centre of cluster c at [.., c]; -1 from n_clusters on
    size: torch.Tensor         # (G,B) int32: the size of cluster c, never increasing; 0 from n_clusters on
    n_clusters: torch.Tensor   # (G,) int32


def _batch_mask(mask, B: int, M: int):
    """a mask (B,M), or (M,) shared by the batch, as (B,M)"""
    if mask is not None and mask.ndim == 1 and tuple(mask.shape) == (M,):
        return mask.expand(B, M)
    return mask


def pairwise_rmsd(a, b=None, mask_a=None, mask_b=None) -> PairwiseRMSD:
    """The RMSD after optimal superposition of every member of ``a`` (Ba,M,3) against every member of ``b`` (Bb,M,3):
    ``PairwiseRMSD(rmsd (Ba,Bb) fp32, count (Ba,Bb) int32)``.  ``b`` None compares ``a`` with itself: a symmetric matrix with
    an exactly zero diagonal, half the work.  The points of a pair are those that both ``mask_a`` and ``mask_b`` count --
    each (B,M), or (M,) shared by its batch, None = all; in the self comparison ``mask_a`` serves both sides --, ``count``
    says how many; a pair without any is NaN, and NaN under a structure's own mask reaches nothing.  One tiled HIP kernel in
    double (``ops.rmsd_matrix``): the five sums of a pair over the common points, then the 3x3 solve of ``kabsch``; no
    broadcast of the coordinates over the pairs, no batched SVD.  The RMSD of identical members is about 1e-6 A, not 0
    (include/protstruc_ensemble.h gives the bound): ``superposition_rmsd`` remains the tool when that matters, and the one
    that returns rotations -- against a chosen medoid, say.

    Not differentiable: the outputs carry no graph, and inputs that require grad are detached."""
    a = a.detach()
    b = None if b is None else b.detach()
    if a.ndim == 3:
        mask_a = _batch_mask(mask_a, a.shape[0], a.shape[1])
        if b is not None and b.ndim == 3:
            mask_b = _batch_mask(mask_b, b.shape[0], b.shape[1])
    return PairwiseRMSD(*ops.rmsd_matrix(a, b, mask_a, mask_b, return_count=True))


def cluster_by_cutoff(D, cutoff, valid=None) -> Clusters:
    """Cluster the items of a distance matrix ``D`` (B,B), or of G matrices (G,B,B), by the rule of Daura et al. (GROMACS'
    ``cluster -method gromos``): ``Clusters(label, center, size, n_clusters)``.  Items are neighbours where ``D <= cutoff``
    (the upper triangle decides; NaN is no neighbour).  Among the items still unassigned -- at first those of ``valid``
    ((B,) / (G,B), None = all) -- the one with the most unassigned neighbours, the lowest index on ties, becomes the centre
    of the next cluster and is taken out with its neighbours, until none is left.  ``label`` (.., B) holds every item's
    cluster, -1 where it is not valid; ``center`` and ``size`` (.., B) are indexed by cluster number, padded with -1 and 0;
    ``n_clusters`` is () / (G,).  The largest cluster is cluster 0, its centre ``center[..., 0]`` -- the medoid by this rule.
    HIP kernels (``ops.cluster``), integer work defined bit for bit, no host read: usable inside a captured graph.
    ``B <= ops.CLUSTER_MAX_ITEMS``.  Not differentiable."""
    D = D.detach()
    single = D.ndim == 2
    if single:
        D = D[None]
        valid = None if valid is None else valid[None]
    out = ops.cluster(D, cutoff, valid)
    return Clusters(*(t[0] for t in out)) if single else Clusters(*out)


def _chain_break_matrix(chain_breaks, B: int, L: int, batched: bool):
    """chain_breaks as a (B, L) bool array / tensor ("the chain ends after residue i"), or None.  Accepts a list of
    residue indices (every structure), a list of B such lists, or a (B, L) ((L,) unbatched) boolean array / tensor."""
    if chain_breaks is None:
        return None
    if isinstance(chain_breaks, (torch.Tensor, np.ndarray)):
        want = (B, L) if batched else (L,)
        if tuple(chain_breaks.shape) != want:
            raise ValueError(f"a chain_breaks array must have shape {want}, got {tuple(chain_breaks.shape)}")
        return chain_breaks.reshape(B, L) if isinstance(chain_breaks, torch.Tensor) else np.asarray(chain_breaks).reshape(B, L)
    items = list(chain_breaks)
    per_structure = len(items) > 0 and all(isinstance(x, (list, tuple, np.ndarray)) for x in items)
    if per_structure and len(items) != B:
        raise ValueError(f"chain_breaks holds {len(items)} lists for {B} structures")
    lists = items if per_structure else [items] * B
    out = np.zeros((B, L), dtype=bool)
    for b, idx in enumerate(lists):
        for i in idx:
            if isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)):
                raise ValueError(f"chain_breaks entries must be residue indices (int), got {i!r}")
            if not 0 <= int(i) < L:
                raise ValueError(f"chain break after residue {int(i)} is outside 0 .. {L - 1}")
            out[b, int(i)] = True
    return out


def reconstruct_backbone_distmat_from_interresidue_geometry(d_cb, omega, theta, phi, mask=None, chain_breaks=None,
                                                            lengths=None):
    """The N / CA / C distance matrix implied by trRosetta inter-residue geometry (reference geometry.py:229-347).

    ``d_cb`` (CB-CB distance), ``omega``, ``theta`` and ``phi`` are (L, L) -> (3, 3, L, L), or (B, L, L) ->
    (B, 3, 3, L, L); plane [a, b] holds |atom a of residue i - atom b of residue j| for atoms N, CA, C.
    ``omega`` is the trRosetta dihedral (CA_i, CB_i, CB_j, CA_j) -- ``StructureBatch.pairwise_dihedrals(["CA", "CB"],
    ["CB", "CA"])``, not ``inter_residue_geometry()["omega"]`` (which is dihedral(CA_i, CB_i, CA_j, CB_j), following the
    reference's featuriser): the placement of CA_j below is only consistent with the former.  ``theta[i, j]`` =
    dihedral(N_i, CA_i, CB_i, CB_j), ``phi[i, j]`` = angle(CA_i, CB_i, CB_j).

    Residue j's atoms are placed in residue i's ideal frame (``place_fourth_atom`` four times), the diagonal and the
    bonds take ideal values, ``chain_breaks`` (a list of residue indices i -- the chain ends after i -- for every
    structure, a list of B such lists, or a (B, L) boolean array) remove the peptide bond, ``mask`` (pair mask, (L, L)
    or (B, L, L)) False and NaN entries become ``MASK``, and the Floyd-Warshall pass of the reference replaces them by
    shortest-path distances over the 3 L atoms; the result is symmetrised and the bonds are set again.  Unlike the
    reference, that last step does not put a peptide bond back across a chain break.  ``lengths`` (B,) pads a ragged
    batch: residues at or beyond a structure's length do not take part, and their entries are NaN.

    numpy in -> numpy out, tensor in -> tensor out (on the GPU); evaluated in float32 by the K8 / K9 kernels."""
    for name, t in (("d_cb", d_cb), ("omega", omega), ("theta", theta), ("phi", phi)):
        if not isinstance(t, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{name} must be a tensor or an ndarray")
    shape = tuple(d_cb.shape)
    if len(shape) not in (2, 3) or shape[-1] != shape[-2]:
        raise ValueError(f"d_cb must have shape (L, L) or (B, L, L), got {shape}")
    for name, t in (("omega", omega), ("theta", theta), ("phi", phi)):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have the shape of d_cb {shape}, got {tuple(t.shape)}")
    batched = len(shape) == 3
    B, L = (shape[0] if batched else 1), shape[-1]
    if mask is not None and tuple(mask.shape) != shape:
        raise ValueError(f"mask must have the shape of d_cb {shape}, got {tuple(mask.shape)}")
    breaks = _chain_break_matrix(chain_breaks, B, L, batched)
    lengths = ops.check_lengths(lengths, B, L)
    if isinstance(lengths, np.ndarray):
        lengths = lengths.astype(np.int32)
    ops.check_distmat_size(B, L)

    args = [d_cb, omega, theta, phi] + [t for t in (mask, breaks, lengths) if t is not None]
    prepped, ft = _prep(args)
    d_cb, omega, theta, phi = (t.reshape(B, L, L) for t in prepped[:4])
    rest = iter(prepped[4:])
    mask = None if mask is None else next(rest).reshape(B, L, L)
    breaks = None if breaks is None else next(rest).reshape(B, L)
    lengths = None if lengths is None else next(rest)
    out = ops.backbone_distmat_init(d_cb, omega, theta, phi, mask, breaks, lengths)
    ops.floyd_warshall_(out, G=3)
    ops.backbone_distmat_finish_(out, breaks, lengths)
    return _finish(out if batched else out[0], ft)


def _lengths_array(lengths, B: int, L: int):
    """``lengths`` on the host, as a checked int64 ndarray (None stays None)."""
    return ops.check_lengths(lengths.cpu().numpy() if isinstance(lengths, torch.Tensor) else lengths, B, L)


def initialize_backbone_with_mds(dist_mat, max_iter: int = 500, *, n_init: int = 4, eps: float = 1e-6,
                                 random_state=None, init=None, lengths=None):
    """Backbone coordinates from an N / CA / C distance matrix by metric MDS (reference geometry.py:350-386).

    ``dist_mat`` (3, 3, L, L) -> (5, L, 3), or (B, 3, 3, L, L) -> (B, 5, L, 3), atoms N, CA, C, O, CB.  SMACOF as
    sklearn 1.7's ``MDS(3, max_iter=max_iter, dissimilarity="precomputed")`` runs it (``n_init`` = 4 random starts,
    ``eps`` = 1e-6) over the 3 L atoms; the starts are sklearn's draws from ``random_state`` (None: numpy's global
    state, as in the reference, so ``np.random.seed(s)`` before the call reproduces its starts).  ``init`` ((K, 3 L, 3)
    or (B, K, 3 L, 3), node g L + i = atom g of residue i) gives K explicit starts instead -- an extension: sklearn runs
    a single start when given one.  The best start is mirrored (z negated) iff its mean backbone phi is positive -- the
    reference's documented intent; its code mirrors unconditionally, which returns the wrong hand about half the time
    -- and CB and O are placed at ideal geometry; O of the last residue is placed from N of the first residue (the
    reference's np.roll).  ``lengths`` (B,) pads a ragged batch: residues at or beyond a structure's length do not take
    part and come back NaN.  A NaN distance inside a structure makes that structure's result all NaN.

    numpy in -> numpy out, tensor in -> tensor out (on the GPU); float32 coordinates, float64 stress sums."""
    if not isinstance(dist_mat, (torch.Tensor, np.ndarray)):
        raise TypeError("dist_mat must be a tensor or an ndarray")
    shape = tuple(dist_mat.shape)
    if len(shape) not in (4, 5) or shape[-4:-2] != (3, 3) or shape[-1] != shape[-2]:
        raise ValueError(f"dist_mat must have shape (3, 3, L, L) or (B, 3, 3, L, L), got {shape}")
    batched = len(shape) == 5
    B, L = (shape[0] if batched else 1), shape[-1]
    lens = _lengths_array(lengths, B, L)
    args = [dist_mat] + ([init] if init is not None else [])
    prepped, ft = _prep(args)
    D = prepped[0].reshape(B, 3, 3, L, L)
    x0 = None
    if init is not None:
        x0 = prepped[1]
        if not batched:
            x0 = x0.unsqueeze(0)
    lens_t = None if lens is None else torch.from_numpy(lens.astype(np.int32)).to(D.device)
    X, _, _ = ops.smacof(D, 3, n_init=None if init is not None else n_init, max_iter=max_iter, eps=eps, init=x0,
                         random_state=random_state, lengths=lens)
    out = ops.mds_backbone_finish(X.reshape(B, 3, L, 3), lens_t, mirror=True, place_o_cb=True)
    return _finish(out if batched else out[0], ft)


def fix_chirality(coords, lengths=None):
    """N / CA / C coordinates (3, L, 3) or (B, 3, L, 3), mirrored (z negated) iff the mean of the backbone phi
    dihedrals (C_{i-1}, N_i, CA_i, C_i), i = 1 .. L-1, is positive (reference geometry.py:389-410, as its docstring and
    commented-out test intend; its code mirrors unconditionally).  Evaluated by the same kernel as
    ``initialize_backbone_with_mds``; an unmirrored structure comes back bit for bit.  numpy in -> numpy out."""
    if not isinstance(coords, (torch.Tensor, np.ndarray)):
        raise TypeError("coords must be a tensor or an ndarray")
    shape = tuple(coords.shape)
    if len(shape) not in (3, 4) or shape[-3] != 3 or shape[-1] != 3:
        raise ValueError(f"coords must have shape (3, L, 3) or (B, 3, L, 3), got {shape}")
    batched = len(shape) == 4
    B, L = (shape[0] if batched else 1), shape[-2]
    lens = _lengths_array(lengths, B, L)
    (x,), ft = _prep([coords])
    lens_t = None if lens is None else torch.from_numpy(lens.astype(np.int32)).to(x.device)
    out = ops.mds_backbone_finish(x.reshape(B, 3, L, 3), lens_t, mirror=True, place_o_cb=False)
    return _finish(out if batched else out[0], ft)
