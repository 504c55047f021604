"""Yardstick of the frame-aligned point error kernels (ps_fape_f32, ps_fape_backward_f32, ps_frames_backward_f32): a plain
torch restatement of the definition, dtype-generic, whose gradients come from ``torch.autograd.grad``.

    u_ij = R_i^T (x_j - t_i)    u'_ij = R'_i^T (x'_j - t'_i)    d_ij = sqrt(|u_ij - u'_ij|^2 + eps)
    loss_b = (1 / scale) * sum_ij f_i p_j min(d_ij, clamp_b) / max(sum_ij f_i p_j, 1)

The masks are applied by ``torch.where`` ON THE INPUTS: a masked frame is replaced by the identity at the origin and a
masked point by the origin before anything is evaluated, so autograd never sees a NaN that sits at a masked entry and the
entry's contribution to every gradient is an exact zero.  The frames of ``frames_from_xyz`` restate the reference's
``gram_schmidt`` (v1 = c - b, e1 = v1 / |v1|, u2 = v2 - (e1 . v2) e1, e2 = u2 / |u2|, e3 = e1 x e2; basis vectors as the
COLUMNS of the 3x3) with differentiable torch ops.

The case generator draws target coordinates 8 randn and predictions target + 4 randn (d spans 0.01-80 A, 40-45 % of the
pairs under 10 A) and sets each structure's clamp in the middle of the widest gap between consecutive float64 distances
in [8, 12] A, asserting that half that gap is at least 10 times the largest float32 error of a distance in the window:
no pair changes side of the clamp through rounding, so the float64 gradient is the yardstick for every pair.
"""
import math
from fractions import Fraction

import numpy as np
import torch

from tests.irg_grad_ref import worst_error  # noqa: F401  (the project's error measure: worst row error / the row's largest |gradient|)

SLOTS = (0, 1, 2, 1)     # a1, a2, a3, t_atom: N, CA, C with the origin at CA
CLAMP_WINDOW = (8.0, 12.0)
GAP_FACTOR = 10.0


def frames_from_xyz(xyz, a1=0, a2=1, a3=2, t_atom=1):
    """(rot (B,N,3,3) with columns e1, e2, e3, trans (B,N,3)) of coordinates (B,N,A,3); differentiable."""
    a, b, c = xyz[:, :, a1], xyz[:, :, a2], xyz[:, :, a3]
    v1 = c - b
    e1 = v1 / torch.linalg.vector_norm(v1, dim=-1, keepdim=True)
    v2 = a - b
    u2 = v2 - (e1 * v2).sum(-1, keepdim=True) * e1
    e2 = u2 / torch.linalg.vector_norm(u2, dim=-1, keepdim=True)
    e3 = torch.linalg.cross(e1, e2, dim=-1)
    return torch.stack([e1, e2, e3], dim=-1), xyz[:, :, t_atom]


def _clean(rot, trans, pts, frame_mask, point_mask):
    if frame_mask is not None:
        f = frame_mask != 0
        rot = torch.where(f[..., None, None], rot, torch.eye(3, dtype=rot.dtype, device=rot.device).expand_as(rot))
        trans = torch.where(f[..., None], trans, torch.zeros_like(trans))
    if point_mask is not None:
        pts = torch.where((point_mask != 0)[..., None], pts, torch.zeros_like(pts))
    return rot, trans, pts


def distances(rot, trans, pts, target_rot, target_trans, target_pts, frame_mask=None, point_mask=None, eps=1e-4):
    """(d (B,N,M), weight (B,N,M) = f_i p_j in d's dtype); masked entries hold the stand-in's value."""
    rot, trans, pts = _clean(rot, trans, pts, frame_mask, point_mask)
    target_rot, target_trans, target_pts = _clean(target_rot, target_trans, target_pts, frame_mask, point_mask)
    u = torch.einsum("bnac,bnma->bnmc", rot, pts[:, None, :, :] - trans[:, :, None, :])
    v = torch.einsum("bnac,bnma->bnmc", target_rot, target_pts[:, None, :, :] - target_trans[:, :, None, :])
    d = torch.sqrt(((u - v) ** 2).sum(-1) + eps)
    B, N, M = d.shape
    f = torch.ones(B, N, dtype=torch.bool, device=d.device) if frame_mask is None else frame_mask != 0
    p = torch.ones(B, M, dtype=torch.bool, device=d.device) if point_mask is None else point_mask != 0
    return d, (f[:, :, None] & p[:, None, :]).to(d.dtype)


def fape(rot, trans, pts, target_rot, target_trans, target_pts, frame_mask=None, point_mask=None, clamp=10.0, scale=10.0,
         eps=1e-4):
    """(loss (B,), count (B,)) in rot's dtype.  ``clamp``: a float or a (B,) tensor, inf = unclamped."""
    d, w = distances(rot, trans, pts, target_rot, target_trans, target_pts, frame_mask, point_mask, eps)
    cl = torch.as_tensor(clamp, dtype=d.dtype, device=d.device).expand(d.shape[0])
    l = torch.minimum(d, cl[:, None, None])
    count = w.sum((1, 2))
    return (w * l).sum((1, 2)) / count.clamp(min=1) / scale, count


class Case:
    """One accuracy case on the CPU in float32: coordinates of both sides, masks, the clamp and an upstream gradient."""

    def __init__(self, xyz, target_xyz, frame_mask, point_mask, atom_mask, clamp, grad_loss, scale=10.0, eps=1e-4):
        self.xyz, self.target_xyz = xyz, target_xyz
        self.frame_mask, self.point_mask, self.atom_mask = frame_mask, point_mask, atom_mask
        self.clamp, self.grad_loss, self.scale, self.eps = clamp, grad_loss, scale, eps
        self.B, self.N, self.A = xyz.shape[:3]

    def operands(self, dtype=torch.float32):
        """rot, trans, points of both sides in ``dtype``: frames in float32 (what a float32 caller holds), then cast."""
        rot, trans = frames_from_xyz(self.xyz, *SLOTS)
        trot, ttrans = frames_from_xyz(self.target_xyz, *SLOTS)
        pts, tpts = self.xyz.reshape(self.B, -1, 3), self.target_xyz.reshape(self.B, -1, 3)
        return [t.detach().to(dtype) for t in (rot, trans, pts, trot, ttrans, tpts)]

    def kwargs(self, dtype=torch.float32):
        return dict(frame_mask=self.frame_mask, point_mask=self.point_mask, clamp=self.clamp.to(dtype), scale=self.scale,
                    eps=self.eps)


def loss(case, dtype=torch.float64, clamp=None):
    kw = case.kwargs(dtype)
    if clamp is not None:
        kw["clamp"] = clamp
    return fape(*case.operands(dtype), **kw)


def gradient(case, dtype=torch.float64, clamp=None):
    """(grad_rot, grad_trans, grad_pts) of sum_b grad_loss_b loss_b by autograd in ``dtype`` on the CPU."""
    ops = case.operands(dtype)
    leaves = [t.requires_grad_(True) for t in ops[:3]]
    kw = case.kwargs(dtype)
    if clamp is not None:
        kw["clamp"] = clamp
    l, _ = fape(*leaves, *ops[3:], **kw)
    return torch.autograd.grad((l * case.grad_loss.to(dtype)).sum(), leaves)


def gradient_xyz(case, dtype=torch.float64):
    """grad_xyz (B,N,A,3) of the chain xyz -> frames (masked residues replaced before the Gram-Schmidt) -> FAPE over every
    atom slot as a point, by autograd in ``dtype``."""
    x = case.xyz.detach().to(dtype).requires_grad_(True)
    stand_in = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], dtype=dtype)   # a1, a2, a3 of a masked residue
    bb = x[:, :, list(SLOTS[:3])]
    if case.frame_mask is not None:
        bb = torch.where((case.frame_mask != 0)[..., None, None], bb, stand_in)
    rot, trans = frames_from_xyz(bb, 0, 1, 2, 1)
    t = case.target_xyz.to(dtype)
    trot, ttrans = frames_from_xyz(t, *SLOTS)
    l, _ = fape(rot, trans, x.reshape(case.B, -1, 3), trot, ttrans, t.reshape(case.B, -1, 3), **case.kwargs(dtype))
    (g,) = torch.autograd.grad((l * case.grad_loss.to(dtype)).sum(), x)
    return g


def frames_gradient(xyz, slots, grad_rot, grad_trans, dtype=torch.float64):
    """grad_xyz of sum(grad_rot * rot) + sum(grad_trans * trans) through the restated Gram-Schmidt, by autograd."""
    x = xyz.detach().to(dtype).requires_grad_(True)
    rot, trans = frames_from_xyz(x, *slots)
    total = x.new_zeros(())
    if grad_rot is not None:
        total = total + (grad_rot.to(dtype) * rot).sum()
    if grad_trans is not None:
        total = total + (grad_trans.to(dtype) * trans).sum()
    (g,) = torch.autograd.grad(total, x)
    return g


def pick_clamp(case):
    """(B,) float32 clamps: per structure the midpoint of the widest gap between consecutive float64 d_ij in the window
    (10.0 for a structure with fewer than two valid pairs there).  Asserts half the gap >= GAP_FACTOR x the largest
    |d32 - d64| over the window's pairs."""
    d64, w = distances(*case.operands(torch.float64), case.frame_mask, case.point_mask, case.eps)
    d32, _ = distances(*case.operands(torch.float32), case.frame_mask, case.point_mask, case.eps)
    lo, hi = CLAMP_WINDOW
    out = torch.full((case.B,), 10.0)
    for b in range(case.B):
        inside = (w[b] != 0) & (d64[b] >= lo) & (d64[b] <= hi)
        v = d64[b][inside].sort().values
        if v.numel() < 2:
            continue
        gaps = v[1:] - v[:-1]
        k = int(gaps.argmax())
        half = float(gaps[k]) / 2
        err = float((d32[b].double() - d64[b])[inside].abs().max())
        assert half >= GAP_FACTOR * err, f"structure {b}: half-gap {half:.2e} < {GAP_FACTOR} x float32 error {err:.2e}: pick another seed"
        mid = torch.tensor(float(v[k]) + half, dtype=torch.float32)
        assert abs(float(mid) - (float(v[k]) + half)) < half / GAP_FACTOR     # the float32 clamp is still inside the gap
        out[b] = mid
    return out


def sqrt_f32(x):
    """The correctly rounded float32 square root of float32(x), decided in exact rational arithmetic: the float32 whose
    rounding interval (between the midpoints to its neighbours) contains the root.  A host's own float32 sqrt is not the
    yardstick: one CPU torch build returned 0x1.c0b1bep-5 for sqrt(float32(3e-3)), whose root 0.0547722559886 lies nearer
    to 0x1.c0b1c0p-5 (1.8e-9 against 1.9e-9)."""
    x32 = np.float32(x)
    if x32 == 0:
        return np.float32(0.0)
    exact = Fraction(float(x32))
    c = np.float32(math.sqrt(float(x32)))
    inf = np.float32(np.inf)
    for n in (np.nextafter(c, -inf), c, np.nextafter(c, inf)):
        lo = (Fraction(float(n)) + Fraction(float(np.nextafter(n, -inf)))) / 2
        hi = (Fraction(float(n)) + Fraction(float(np.nextafter(n, inf)))) / 2
        if lo * lo <= exact <= hi * hi:
            return n
    raise AssertionError(f"no float32 within one ulp of sqrt({x32!r})")


def floor_loss_f32(eps, scale):
    """float32(sqrt_f32(eps) / float32(scale)): the loss of perfectly placed points, correctly rounded (a quotient of two
    float32 numbers rounded through float64 is the correctly rounded float32 quotient)."""
    return np.float32(np.float64(sqrt_f32(eps)) / np.float64(np.float32(scale)))


MASKS = ["none", "frame", "point", "both"]
# (B, N, A): a few lanes of one wave; 15 slots with an odd length; more than one workgroup of frames (64 each); three
# workgroups of frames with an odd tail; and more points (1350: five staging tiles of 256 and a tail) than two tiles with
# more frames (150) than a workgroup holds.  The largest case stays at 2e5 pairs: beyond a million the widest gap between
# distances near the clamp shrinks to ~10 x the float32 error, and pick_clamp's assertion would depend on the host CPU.
SHAPES = [(2, 5, 4), (1, 33, 15), (2, 70, 4), (3, 130, 4), (1, 150, 9)]


def random_case(seed, B, N, A, mask_kind="none"):
    """Target 8 randn, prediction target + 4 randn; p = 0.8 masks; with a frame mask and B > 1 the LAST structure has every
    frame masked (no valid pair).  NaN-free; the NaN tests overwrite the masked entries themselves."""
    g = torch.Generator().manual_seed(seed)
    target = 8 * torch.randn(B, N, A, 3, generator=g)
    xyz = target + 4 * torch.randn(B, N, A, 3, generator=g)
    frame_mask = torch.rand(B, N, generator=g) < 0.8
    atom_mask = torch.rand(B, N, A, generator=g) < 0.8
    grad_loss = torch.randn(B, generator=g)
    if B > 1:
        frame_mask[-1] = False
    if mask_kind in ("none", "point"):
        frame_mask = None
    if mask_kind in ("none", "frame"):
        atom_mask = None
    point_mask = None if atom_mask is None else atom_mask.reshape(B, N * A)
    case = Case(xyz, target, frame_mask, point_mask, atom_mask, torch.full((B,), 10.0), grad_loss)
    case.clamp = pick_clamp(case)
    return case


def accuracy_cases():
    """(name, seed, B, N, A, mask kind) of every accuracy case."""
    return [(f"{B}x{N}x{A} mask={kind}", 3000 + 11 * N + B + 101 * k, B, N, A, kind)
            for (B, N, A) in SHAPES for k, kind in enumerate(MASKS)]
