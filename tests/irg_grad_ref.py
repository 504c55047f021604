"""Yardstick of the featuriser's backward pass (ps_inter_residue_geometry_backward_f32): a torch restatement of the six
float planes of ``inter_residue_geometry`` whose gradient comes from ``torch.autograd.grad``.

The active-entry rule is applied by ``torch.where`` ON THE INPUTS: an entry (b, i, j) of a plane is active when every
atom it reads is present in ``atom_mask`` and, for every plane but d_no, i != j.  The points of an inactive entry are
replaced by a fixed non-degenerate stand-in tetrahedron before any geometry is evaluated, so autograd never sees a NaN
coordinate (``from_pdb`` stores NaN for missing atoms), a sqrt(0), an atan2(0, 0) or a 0 / 0, and the inactive entry's
contribution to the gradient is an exact zero.  Upstream gradients are selected the same way (NaN at an inactive entry
never reaches the result).

The formulas are those of the oracle (oracle/protstruc_oracle.py: ``norm``, ``angle``, ``dihedral``), written with
differentiable torch ops: omega = dihedral(CA_i, CB_i, CA_j, CB_j) as the reference codes it, theta =
dihedral(N_i, CA_i, CB_i, CB_j), phi = angle(CA_i, CB_i, CB_j), no clamp before acos.
"""
import torch

N_SLOT, CA_SLOT, O_SLOT, CB_SLOT = 0, 1, 3, 4
USED_SLOTS = (N_SLOT, CA_SLOT, O_SLOT, CB_SLOT)
PLANES = ("d_ca", "d_cb", "d_no", "omega", "theta", "phi")
# plane -> (slots read from residue i, slots read from residue j), in the order the geometry takes its points
POINTS = {
    "d_ca": ((CA_SLOT,), (CA_SLOT,)),
    "d_cb": ((CB_SLOT,), (CB_SLOT,)),
    "d_no": ((N_SLOT,), (O_SLOT,)),
    "omega": ((CA_SLOT, CB_SLOT), (CA_SLOT, CB_SLOT)),
    "theta": ((N_SLOT, CA_SLOT, CB_SLOT), (CB_SLOT,)),
    "phi": ((CA_SLOT, CB_SLOT), (CB_SLOT,)),
}
# what an inactive entry evaluates instead of its own points: dihedral = -pi / 2, angle = pi / 2, distance = 1
STAND_IN = ((1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 1.0))


def active_entries(B, N, atom_mask=None, device="cpu"):
    """plane -> (B, N, N) bool on ``device``: the entries that contribute (every atom read is present; i != j except for
    d_no)."""
    present = torch.ones(B, N, 5, dtype=torch.bool, device=device) if atom_mask is None else (atom_mask != 0).to(device)
    off_diagonal = ~torch.eye(N, dtype=torch.bool, device=device)[None]
    out = {}
    for plane, (si, sj) in POINTS.items():
        a = torch.ones(B, N, N, dtype=torch.bool, device=device)
        for s in si:
            a = a & present[:, :, None, s]
        for s in sj:
            a = a & present[:, None, :, s]
        out[plane] = a if plane == "d_no" else a & off_diagonal
    return out


def _dot(x, y):
    return (x * y).sum(-1)


def _distance(a, b):
    return torch.linalg.vector_norm(a - b, dim=-1)


def _angle(a, b, c):
    ba, bc = a - b, c - b
    return torch.arccos(_dot(ba, bc) / (torch.linalg.vector_norm(ba, dim=-1) * torch.linalg.vector_norm(bc, dim=-1)))


def _dihedral(a, b, c, d):
    b0, b1, b2 = a - b, c - b, d - c
    n1 = torch.linalg.cross(b0, b1, dim=-1)
    n2 = torch.linalg.cross(b2, b1, dim=-1)
    m = torch.linalg.cross(n1, n2, dim=-1)
    return torch.atan2(_dot(m, b1) / torch.linalg.vector_norm(b1, dim=-1), _dot(n1, n2))


_GEOMETRY = {2: _distance, 3: _angle, 4: _dihedral}


def planes(xyz, atom_mask=None):
    """(dict plane -> (B, N, N) in xyz's dtype, dict plane -> (B, N, N) bool active).  Inactive entries hold the stand-in's
    value; differentiable with respect to ``xyz`` (any float dtype, on xyz's device)."""
    B, N = xyz.shape[:2]
    if xyz.shape[2] < 5:
        raise IndexError("inter_residue_geometry needs the N, CA, C, O, CB atom slots")
    active = active_entries(B, N, atom_mask, xyz.device)
    stand_in = torch.tensor(STAND_IN, dtype=xyz.dtype, device=xyz.device)
    out = {}
    for plane, (si, sj) in POINTS.items():
        pts = [xyz[:, :, None, s, :].expand(B, N, N, 3) for s in si] + [xyz[:, None, :, s, :].expand(B, N, N, 3) for s in sj]
        pts = [torch.where(active[plane][..., None], p, stand_in[q]) for q, p in enumerate(pts)]
        out[plane] = _GEOMETRY[len(pts)](*pts)
    return out, active


def weighted_sum(xyz, atom_mask, grads):
    """sum over planes and active entries of grads[plane] * plane: the scalar whose gradient the backward kernel returns."""
    vals, active = planes(xyz, atom_mask)
    total = xyz.new_zeros(())
    for plane, g in grads.items():
        g = torch.where(active[plane], g.to(xyz.dtype), torch.zeros((), dtype=xyz.dtype, device=xyz.device))
        total = total + (g * vals[plane]).sum()
    return total


def gradient(xyz, atom_mask, grads, dtype=torch.float64):
    """grad_xyz (B, N, A, 3) of ``weighted_sum`` by autograd, evaluated in ``dtype`` on the CPU.  ``grads``: any subset of
    the six planes."""
    for plane in grads:
        if plane not in PLANES:
            raise KeyError(plane)
    x = xyz.detach().cpu().to(dtype).requires_grad_(True)
    m = None if atom_mask is None else atom_mask.detach().cpu()
    total = weighted_sum(x, m, {k: v.detach().cpu() for k, v in grads.items()})
    if not grads:
        return torch.zeros_like(x)
    (g,) = torch.autograd.grad(total, x)
    return g


def residue_errors(got, want):
    """e(b, r) = max |got - want| over the residue's A x 3 entries / the residue's largest |want|, as float64 (B, N).
    A residue whose ``want`` is identically zero has e = 0 where ``got`` is exactly zero there and inf otherwise."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    B, N = want.shape[:2]
    err = (got - want).abs().reshape(B, N, -1)
    err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err).amax(-1)
    scale = want.abs().reshape(B, N, -1).amax(-1)
    exact = (got.reshape(B, N, -1) == 0).all(-1)
    zero = scale == 0
    e = err / torch.where(zero, torch.ones_like(scale), scale)
    return torch.where(zero, torch.where(exact, torch.zeros_like(e), torch.full_like(e, float("inf"))), e)


def worst_error(got, want):
    """E = max over residues of e(r); 0 for an empty batch."""
    e = residue_errors(got, want)
    return float(e.max()) if e.numel() else 0.0


# ---- the accuracy cases of the GPU test (and of tools/irg_backward_time.py, which reports E per case) ----
SHAPES = [(1, 1, 5), (1, 2, 15), (2, 5, 15), (4, 33, 15), (2, 64, 25), (3, 100, 15), (1, 229, 15), (2, 512, 15)]
MASKS = ["none", "bool", "float"]


def random_case(seed, B, N, A=15, mask_kind="bool"):
    """randn coordinates, a p = 0.9 atom mask (None / bool / float dtype) and randn upstream gradients, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(B, N, A, 3, generator=g)
    mask = torch.rand(B, N, A, generator=g) < 0.9
    mask = {"none": None, "bool": mask, "float": mask.float()}[mask_kind]
    grads = {k: torch.randn(B, N, N, generator=g) for k in PLANES}
    return xyz, mask, grads


def accuracy_cases():
    """(name, B, N, A, mask kind, seed) of every randn accuracy case."""
    return [(f"randn {(B, N, A)} mask={kind}", B, N, A, kind, 1000 + 7 * N + B) for (B, N, A) in SHAPES for kind in MASKS]


def pdb_case(path):
    """A PDB file through the package's own reader (NaN for missing atoms) with randn upstream gradients, on the CPU."""
    from protstruc_amd import StructureBatch
    sb = StructureBatch.from_pdb(path)
    xyz, mask = sb.xyz.cpu(), sb.atom_mask.cpu()
    g = torch.Generator().manual_seed(158)
    N = xyz.shape[1]
    return xyz, mask, {k: torch.randn(xyz.shape[0], N, N, generator=g) for k in PLANES}
