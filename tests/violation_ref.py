"""Yardstick of the structural-violation kernels (ps_clash_f32, ps_clash_backward_f32, ps_peptide_bond_f32,
ps_peptide_bond_backward_f32): a plain torch restatement of the definitions that runs in any dtype, builds (B, M, M)
tensors and makes no attempt at speed; its gradients come from ``torch.autograd.grad``.

    d_ij = sqrt(|x_i - x_j|^2 + eps)          s_ij = radius_i + radius_j - tolerance
    c_ij = p_i p_j [i != j] [group_i != group_j, when given] [not (link_i == link_j and link_i >= 0), when given]
    v_ij = max(0, s_ij - d_ij)                E_i = sum_j c_ij v_ij          n_i = sum_j c_ij [v_ij > 0]

    l  = sqrt(|N' - C|^2 + eps)               viol_0 = max(0, |l  - l0|       - tau sigma_l)      (proline: l0_pro, sigma_l_pro)
    ca = unit(CA - C) . unit(N' - C)          viol_1 = max(0, |ca - cos_cacn| - tau sigma_cacn)
    cn = unit(C - N') . unit(CA' - N')        viol_2 = max(0, |cn - cos_cnca| - tau sigma_cnca)     unit(v) = v / sqrt(|v|^2 + eps)

The masks are applied by ``torch.where`` ON THE INPUTS (a masked point, and an atom no valid junction reads, is replaced
by the origin before anything is evaluated), so autograd never sees a NaN that sits there and its gradient is an exact
zero.

One step cannot be decided in float32 where float64 sits on it: [v_ij > 0].  E is continuous across it, but n jumps by one
and the gradient by a unit vector times (w_i + w_j).  ``brackets`` therefore counts, in float64, every pair within BORDER
of s_ij = d_ij out and in; the points that own such a pair are OPEN: their n is only bracketed and their gradient is left
out of the error.  Likewise a junction with a term within BORDER of its kink makes its two residues open for the bond
gradient.  BORDER = 1e-4: the float32 error of s - d on these inputs (coordinates up to about 100 A) is below 1e-5.
"""
import os

import torch

from tests.irg_grad_ref import residue_errors, worst_error  # noqa: F401  (worst row error / the row's largest |value|)

BORDER = 1e-4
TOLERANCE = 1.5
EPS = 1e-10
RADII = (1.7, 1.55, 1.52, 1.8)   # C, N, O, S
BOND = dict(l0=1.329, sigma_l=0.014, l0_pro=1.341, sigma_l_pro=0.016, cos_cacn=-0.4473, sigma_cacn=0.0311,
            cos_cnca=-0.5203, sigma_cnca=0.0353, tau=12.0)
SLOTS = (0, 1, 2)   # N, CA, C


# ---- the clash term ----------------------------------------------------------------------------------------------------
def _clean(t, point_mask):
    if point_mask is None:
        return t
    keep = point_mask != 0
    return torch.where(keep.reshape(keep.shape + (1,) * (t.dim() - keep.dim())), t, torch.zeros_like(t))


def pair_terms(points, radius, point_mask=None, groups=None, link=None, tolerance=TOLERANCE, eps=EPS):
    """(s - d (B,M,M), allowed (B,M,M) bool = c_ij) in points' dtype."""
    x, r = _clean(points, point_mask), _clean(radius, point_mask)
    d = torch.sqrt(((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1) + eps)
    s = r[:, :, None] + r[:, None, :] - tolerance
    B, M = x.shape[:2]
    allowed = ~torch.eye(M, dtype=torch.bool, device=x.device).expand(B, M, M)
    if point_mask is not None:
        p = point_mask != 0
        allowed = allowed & p[:, :, None] & p[:, None, :]
    if groups is not None:
        allowed = allowed & (groups[:, :, None] != groups[:, None, :])
    if link is not None:
        allowed = allowed & ~((link[:, :, None] == link[:, None, :]) & (link[:, :, None] >= 0))
    return s - d, allowed


def clash(points, radius, point_mask=None, groups=None, link=None, tolerance=TOLERANCE, eps=EPS):
    """(E (B,M), n (B,M)) in points' dtype."""
    margin, allowed = pair_terms(points, radius, point_mask, groups, link, tolerance, eps)
    c = allowed.to(margin.dtype)
    v = torch.relu(margin)
    return (c * v).sum(-1), (c * (v > 0).to(margin.dtype)).sum(-1)


class Case:
    """One clash case on the CPU in float32: points and radii (NaN at masked points), the mask, the groups, the links and
    an upstream gradient dL/dE."""

    def __init__(self, points, radius, point_mask, groups, link, grad_E, tolerance=TOLERANCE, eps=EPS):
        self.points, self.radius, self.point_mask, self.groups, self.link = points, radius, point_mask, groups, link
        self.grad_E, self.tolerance, self.eps = grad_E, tolerance, eps
        self.B, self.M = points.shape[:2]

    def kwargs(self):
        return dict(point_mask=self.point_mask, groups=self.groups, link=self.link, tolerance=self.tolerance, eps=self.eps)

    def valid(self):
        return torch.ones(self.B, self.M, dtype=torch.bool) if self.point_mask is None else self.point_mask != 0


def forward(case, dtype=torch.float64, points=None):
    x = case.points if points is None else points
    return clash(x.to(dtype), case.radius.to(dtype), **case.kwargs())


def gradient(case, dtype=torch.float64):
    """grad_points (B,M,3) of sum_bi grad_E_bi E_bi by autograd in ``dtype`` on the CPU."""
    x = case.points.detach().to(dtype).requires_grad_(True)
    E, _ = clash(x, case.radius.to(dtype), **case.kwargs())
    (g,) = torch.autograd.grad((E * _clean(case.grad_E.to(dtype), case.point_mask)).sum(), x)
    return g


def brackets(case):
    """In float64: (n_lo, n_hi), each (B,M), with every pair within BORDER of s_ij = d_ij counted out (lo) and in (hi);
    and ``open`` (B,M) bool, the points that own such a pair."""
    margin, allowed = pair_terms(case.points.double(), case.radius.double(), **case.kwargs())
    sure, maybe = allowed & (margin > BORDER), allowed & (margin > -BORDER)
    n_lo, n_hi = sure.sum(-1).double(), maybe.sum(-1).double()
    return n_lo, n_hi, n_lo != n_hi


def random_walk(B, M, generator, step=1.5):
    """A centred random walk of M points with ``step`` A steps, (B,M,3) float32."""
    steps = torch.randn(B, M, 3, generator=generator, dtype=torch.float64)
    steps = step * steps / steps.norm(dim=-1, keepdim=True)
    walk = steps.cumsum(1)
    return (walk - walk.mean(1, keepdim=True)).float()


def random_case(B, M, mask_kind="none", groups=None, link=False, tolerance=TOLERANCE, seed=0):
    """A centred random walk with 1.5 A steps, radii drawn from the four element values.  ``mask_kind``: "none"; "p60"
    (each point kept with p = 0.6); "structure" (p = 0.8, the LAST structure fully masked).  NaN is written into the
    coordinates and the radii at masked points.  ``groups``: None, or the number of consecutive points that share a
    group; ``link``: the last point of each group and the first point of the next share an id."""
    g = torch.Generator().manual_seed(seed)
    points = random_walk(B, M, g)
    radius = torch.tensor(RADII)[torch.randint(0, len(RADII), (B, M), generator=g)]
    keep = torch.rand(B, M, generator=g)
    grad_E = torch.randn(B, M, generator=g)
    if mask_kind == "none":
        mask = None
    else:
        mask = keep < {"p60": 0.6, "structure": 0.8}[mask_kind]
        if mask_kind == "structure":
            mask[-1] = False
        nan = float("nan")
        points = torch.where(mask[..., None], points, torch.full_like(points, nan))
        radius = torch.where(mask, radius, torch.full_like(radius, nan))
    grp = lnk = None
    if groups is not None:
        index = torch.arange(M, dtype=torch.int32)
        grp = (index // groups).expand(B, M).contiguous()
        if link:
            last, first = index % groups == groups - 1, index % groups == 0
            one = torch.where(last, index // groups, torch.where(first, index // groups - 1, torch.full_like(index, -1)))
            lnk = one.expand(B, M).contiguous()
    return Case(points, radius, mask, grp, lnk, grad_E, tolerance)


def accuracy_cases():
    """{name: keyword arguments of random_case} of every clash case the GPU tests run, B = 3: no pair at all (M = 1); the
    edge of the 64-owner tile (63, 64, 65); one staged tile of 256 plus one point (257); several tiles with compaction
    active and NaN at the masked points, radii included (600, 40 % masked); a fully masked structure; groups of 4 with
    links; no groups; no tolerance with groups of 8."""
    return {
        "M=1": dict(B=3, M=1, seed=201),
        "M=63": dict(B=3, M=63, groups=4, seed=202),
        "M=64": dict(B=3, M=64, groups=4, seed=203),
        "M=65": dict(B=3, M=65, groups=4, seed=204),
        "M=257": dict(B=3, M=257, groups=4, seed=205),
        "M=600 p60": dict(B=3, M=600, mask_kind="p60", groups=4, seed=206),
        "M=130 structure masked": dict(B=3, M=130, mask_kind="structure", groups=4, seed=207),
        "M=130 groups of 4 linked": dict(B=3, M=130, groups=4, link=True, seed=208),
        "M=130 no groups": dict(B=3, M=130, seed=209),
        "M=70 tolerance 0": dict(B=3, M=70, groups=8, tolerance=0.0, seed=210),
    }


# ---- the peptide bond ----------------------------------------------------------------------------------------------------
def _unit(v, eps):
    return v / torch.sqrt((v * v).sum(-1, keepdim=True) + eps)


def bond_terms(xyz, junction_mask=None, next_is_proline=None, slots=SLOTS, eps=EPS, **constants):
    """((B,N-1,3) signed distances of the three terms to their kinks, |value - ideal| - tau sigma, valid (B,N-1) bool)."""
    k = {**BOND, **constants}
    n_slot, ca_slot, c_slot = slots
    B, N = xyz.shape[:2]
    valid = torch.ones(B, N - 1, dtype=torch.bool) if junction_mask is None else junction_mask[:, :-1] != 0
    used = torch.zeros(xyz.shape[:3], dtype=torch.bool)           # the atoms a valid junction reads
    used[:, :-1, c_slot] |= valid
    used[:, :-1, ca_slot] |= valid
    used[:, 1:, n_slot] |= valid
    used[:, 1:, ca_slot] |= valid
    x = torch.where(used[..., None], xyz, torch.zeros_like(xyz))
    C, CA, Nn, CAn = x[:, :-1, c_slot], x[:, :-1, ca_slot], x[:, 1:, n_slot], x[:, 1:, ca_slot]
    length = torch.sqrt(((Nn - C) ** 2).sum(-1) + eps)
    ca = (_unit(CA - C, eps) * _unit(Nn - C, eps)).sum(-1)
    cn = (_unit(C - Nn, eps) * _unit(CAn - Nn, eps)).sum(-1)
    if next_is_proline is None:
        l0, slack = k["l0"], k["tau"] * k["sigma_l"]
    else:
        pro = (next_is_proline[:, :-1] != 0) & valid
        const = lambda value: torch.tensor(value, dtype=xyz.dtype)  # noqa: E731
        l0 = torch.where(pro, const(k["l0_pro"]), const(k["l0"]))
        slack = torch.where(pro, const(k["tau"] * k["sigma_l_pro"]), const(k["tau"] * k["sigma_l"]))
    over = torch.stack([(length - l0).abs() - slack, (ca - k["cos_cacn"]).abs() - k["tau"] * k["sigma_cacn"],
                        (cn - k["cos_cnca"]).abs() - k["tau"] * k["sigma_cnca"]], dim=-1)
    return over, valid


def peptide_bond(xyz, junction_mask=None, next_is_proline=None, slots=SLOTS, eps=EPS, **constants):
    """viol (B,N,3) in xyz's dtype; row N-1 and invalid junctions are zeros."""
    B, N = xyz.shape[:2]
    out = torch.zeros(B, N, 3, dtype=xyz.dtype)
    if N < 2:
        # attached to the input through a selection that never takes it, so that autograd gives exact zeros
        return out + torch.where(torch.zeros_like(xyz, dtype=torch.bool), xyz, torch.zeros_like(xyz)).sum()
    over, valid = bond_terms(xyz, junction_mask, next_is_proline, slots, eps, **constants)
    viol = torch.where(valid[..., None], torch.relu(over), torch.zeros_like(over))
    return torch.cat([viol, torch.zeros(B, 1, 3, dtype=xyz.dtype)], dim=1)


class BondCase:
    def __init__(self, xyz, junction_mask, next_is_proline, grad_viol):
        self.xyz, self.junction_mask, self.next_is_proline, self.grad_viol = xyz, junction_mask, next_is_proline, grad_viol
        self.B, self.N = xyz.shape[:2]

    def kwargs(self):
        return dict(junction_mask=self.junction_mask, next_is_proline=self.next_is_proline)

    def valid(self):
        """(B,N) bool with entry N-1 False."""
        v = torch.ones(self.B, self.N, dtype=torch.bool) if self.junction_mask is None else self.junction_mask != 0
        v = v.clone()
        v[:, -1] = False
        return v


def bond_forward(case, dtype=torch.float64, **constants):
    return peptide_bond(case.xyz.to(dtype), **case.kwargs(), **constants)


def bond_gradient(case, dtype=torch.float64, **constants):
    """grad_xyz (B,N,A,3) of sum grad_viol viol by autograd in ``dtype`` on the CPU; grad_viol counts at valid junctions only."""
    x = case.xyz.detach().to(dtype).requires_grad_(True)
    viol = peptide_bond(x, **case.kwargs(), **constants)
    w = torch.where(case.valid()[..., None], case.grad_viol.to(dtype), torch.zeros((), dtype=dtype))
    (g,) = torch.autograd.grad((viol * w).sum(), x)
    return g


def bond_open(case, **constants):
    """(B,N) bool: the residues of a valid junction with a term within BORDER of its kink (the gradient jumps there)."""
    out = torch.zeros(case.B, case.N, dtype=torch.bool)
    if case.N < 2:
        return out
    over, valid = bond_terms(case.xyz.double(), **case.kwargs(), **constants)
    at_kink = valid & (over.abs() < BORDER).any(-1)
    out[:, :-1] |= at_kink
    out[:, 1:] |= at_kink
    return out


GOLDEN_PDB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "15c8_HL.pdb")


def pdb_batch():
    """tests/golden/15c8_HL.pdb through the repository's own reader, on the CPU (NaN at missing atoms)."""
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb(GOLDEN_PDB, device="cpu")


def bond_case(N=None, keep=1.0, proline=True, noise=0.3, seed=0, B=3):
    """The first ``N`` residues of 15c8_HL (all 229 with None) plus Gaussian noise of ``noise`` A, replicated to B
    structures; the junctions are the package's own (``structure_batch.valid_junctions``: backbone atoms present, the same
    chain -- the H/L chain break is no junction); with ``keep`` < 1 each residue is kept with that probability and the
    others are NaN; ``proline``: flags from the sequence."""
    from protstruc_amd.pdb import ONE_TO_INDEX
    from protstruc_amd.structure_batch import valid_junctions
    sb = pdb_batch()
    N = sb.xyz.shape[1] if N is None else N
    g = torch.Generator().manual_seed(seed)
    xyz = sb.xyz[:, :N].expand(B, -1, -1, -1) + noise * torch.randn(B, N, sb.xyz.shape[2], 3, generator=g)
    present = (sb.atom_mask[:, :N] != 0).expand(B, -1, -1)
    kept = torch.rand(B, N, generator=g) < keep
    grad_viol = torch.randn(B, N, 3, generator=g)
    present = present & kept[:, :, None]
    xyz = torch.where(present[..., None], xyz, torch.full_like(xyz, float("nan")))
    junctions = valid_junctions(present, sb.chain_idx[:, :N].expand(B, -1))
    pro = torch.roll(sb.get_seq_idx() == ONE_TO_INDEX["P"], -1, dims=1)[:, :N].expand(B, -1).contiguous() if proline else None
    return BondCase(xyz.contiguous(), junctions, pro, grad_viol)


def bond_cases():
    """{name: keyword arguments of bond_case}: no junction (N = 1), one (2), the edge of a wave (63, 64, 65), the whole
    file with its chain break (229), 20 % of the residues missing with NaN coordinates, and no proline flags."""
    return {
        "N=1": dict(N=1, seed=301),
        "N=2": dict(N=2, seed=302),
        "N=63": dict(N=63, seed=303),
        "N=64": dict(N=64, seed=304),
        "N=65": dict(N=65, seed=305),
        "N=229": dict(seed=306),
        "N=229 p80": dict(keep=0.8, seed=307),
        "N=229 no proline flags": dict(proline=False, seed=308),
    }
