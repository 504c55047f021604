"""Yardstick of the lDDT kernels (ps_lddt_f32, ps_lddt_backward_f32): a plain torch restatement of the definition that
runs in any dtype, builds (B, M, M) tensors and makes no attempt at speed; its gradient comes from ``torch.autograd.grad``.

    d_ij = sqrt(|x_i - x_j|^2 + eps)    d'_ij likewise on the target    delta_ij = |d_ij - d'_ij|
    c_ij = p_i p_j [i != j] [group_i != group_j, when groups are given] [d'_ij < cutoff]
    e_ij = (1/T) sum_t [delta_ij < thr_t]   (hard)       e_ij = (1/T) sum_t sigmoid(thr_t - delta_ij)   (smooth)
    S_i  = sum_j c_ij e_ij              n_i = sum_j c_ij

The mask is applied by ``torch.where`` ON THE INPUTS (a masked point is replaced by the origin before anything is
evaluated), so autograd never sees a NaN that sits at a masked point and the point's gradient is an exact zero.

Two steps of the definition cannot be decided in float32 where float64 sits on them, and one kink cannot either:
[d' < cutoff], [delta < thr_t], and the sign of d - d' in the gradient of |d - d'| (e'(0) is not zero, so a pair whose two
distances agree to rounding pulls one way or the other).  ``brackets`` therefore counts, in float64, every term within
BORDER of such a step out and in, and ``open_points`` names the points whose float32 result is not a rounding of the
float64 one.  BORDER = 1e-4: the float32 error of a distance on these inputs (random walks of up to 600 steps of 3.8 A,
coordinates up to about 100 A) is at most 1.7e-5, so the error of d - d' is at most 3.4e-5.
"""
import torch

from tests.irg_grad_ref import residue_errors, worst_error  # noqa: F401  (worst row error / the row's largest |value|)

BORDER = 1e-4
CUTOFF = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
EPS = 1e-10


def _clean(points, point_mask):
    if point_mask is None:
        return points
    return torch.where((point_mask != 0)[..., None], points, torch.zeros_like(points))


def pair_terms(points, target_points, point_mask=None, groups=None, cutoff=CUTOFF, eps=EPS):
    """(delta (B,M,M), d' (B,M,M), allowed (B,M,M) bool = p_i p_j [i != j] [group_i != group_j]) in points' dtype."""
    x, t = _clean(points, point_mask), _clean(target_points, point_mask)
    d = torch.sqrt(((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1) + eps)
    dt = torch.sqrt(((t[:, :, None, :] - t[:, None, :, :]) ** 2).sum(-1) + eps)
    B, M = x.shape[:2]
    allowed = ~torch.eye(M, dtype=torch.bool, device=x.device).expand(B, M, M)
    if point_mask is not None:
        p = point_mask != 0
        allowed = allowed & p[:, :, None] & p[:, None, :]
    if groups is not None:
        allowed = allowed & (groups[:, :, None] != groups[:, None, :])
    return (d - dt).abs(), dt, allowed


def lddt(points, target_points, point_mask=None, groups=None, cutoff=CUTOFF, thresholds=THRESHOLDS, smooth=False, eps=EPS):
    """(S (B,M), n (B,M)) in points' dtype."""
    delta, dt, allowed = pair_terms(points, target_points, point_mask, groups, cutoff, eps)
    c = (allowed & (dt < cutoff)).to(delta.dtype)
    thr = torch.tensor(thresholds, dtype=delta.dtype, device=delta.device)
    if smooth:
        e = torch.sigmoid(thr - delta[..., None]).sum(-1) / len(thresholds)
    else:
        e = (delta[..., None] < thr).to(delta.dtype).sum(-1) / len(thresholds)
    return (c * e).sum(-1), c.sum(-1)


def score(S, n, reduction="point"):
    if reduction == "point":
        return S / n.clamp(min=1)
    return S.sum(-1) / n.sum(-1).clamp(min=1)


class Case:
    """One accuracy case on the CPU in float32: both sides (NaN at masked points), the mask, the groups, the thresholds
    and an upstream gradient dL/dS."""

    def __init__(self, points, target, point_mask, groups, thresholds, grad_S, cutoff=CUTOFF, eps=EPS):
        self.points, self.target, self.point_mask, self.groups = points, target, point_mask, groups
        self.thresholds, self.grad_S, self.cutoff, self.eps = tuple(thresholds), grad_S, cutoff, eps
        self.B, self.M = points.shape[:2]

    def kwargs(self):
        return dict(point_mask=self.point_mask, groups=self.groups, cutoff=self.cutoff, thresholds=self.thresholds, eps=self.eps)

    def valid(self):
        return torch.ones(self.B, self.M, dtype=torch.bool) if self.point_mask is None else self.point_mask != 0


def forward(case, smooth, dtype=torch.float64, points=None):
    x = case.points if points is None else points
    return lddt(x.to(dtype), case.target.to(dtype), smooth=smooth, **case.kwargs())


def gradient(case, dtype=torch.float64):
    """grad_points (B,M,3) of sum_bi grad_S_bi S_bi (smooth) by autograd in ``dtype`` on the CPU."""
    x = case.points.detach().to(dtype).requires_grad_(True)
    S, _ = lddt(x, case.target.to(dtype), smooth=True, **case.kwargs())
    w = case.grad_S.to(dtype)
    if case.point_mask is not None:
        w = torch.where(case.point_mask != 0, w, torch.zeros_like(w))
    (g,) = torch.autograd.grad((S * w).sum(), x)
    return g


def brackets(case):
    """In float64: (lo, hi) of T * S_i (hard) and (lo, hi) of n_i, each (B,M), with every term within BORDER of the cutoff
    or of a threshold counted out (lo) and in (hi); and ``kink`` (B,M) bool, the points with a surely or possibly
    counted pair whose |d - d'| is below BORDER."""
    delta, dt, allowed = pair_terms(case.points.double(), case.target.double(), case.point_mask, case.groups, case.cutoff,
                                    case.eps)
    thr = torch.tensor(case.thresholds, dtype=torch.float64)
    sure = allowed & (dt < case.cutoff - BORDER)
    maybe = allowed & (dt < case.cutoff + BORDER)
    hits_lo = (delta[..., None] < thr - BORDER).sum(-1)
    hits_hi = (delta[..., None] < thr + BORDER).sum(-1)
    s_lo, s_hi = (sure * hits_lo).sum(-1).double(), (maybe * hits_hi).sum(-1).double()
    n_lo, n_hi = sure.sum(-1).double(), maybe.sum(-1).double()
    kink = (maybe & (delta < BORDER)).any(-1)
    return (s_lo, s_hi), (n_lo, n_hi), kink


def open_points(case):
    """(hard (B,M), smooth (B,M), grad (B,M)) bool: the points whose float32 result is not a rounding of the float64 one --
    hard: an open bracket of S or n; smooth: an open bracket of n (a pair at the cutoff); grad: that, or a kink pair."""
    (s_lo, s_hi), (n_lo, n_hi), kink = brackets(case)
    at_cutoff = n_lo != n_hi
    return (s_lo != s_hi) | at_cutoff, at_cutoff, at_cutoff | kink


def random_walk(B, M, generator):
    """A centred random walk of M points with 3.8 A steps, (B,M,3) float32."""
    steps = torch.randn(B, M, 3, generator=generator, dtype=torch.float64)
    steps = 3.8 * steps / steps.norm(dim=-1, keepdim=True)
    walk = steps.cumsum(1)
    return (walk - walk.mean(1, keepdim=True)).float()


def random_case(B, M, mask_kind="none", groups=None, noise=0.3, seed=0, thresholds=THRESHOLDS):
    """Target: a centred random walk with 3.8 A steps; prediction: the target plus Gaussian noise of ``noise`` A (0.3 or
    1.5).  ``mask_kind``: "none"; "p60" (each point kept with p = 0.6); "structure" (p = 0.8, the LAST structure fully
    masked).  NaN is written into both sides at masked points.  ``groups``: None, or the number of consecutive points
    that share a group."""
    g = torch.Generator().manual_seed(seed)
    target = random_walk(B, M, g)
    points = target + noise * torch.randn(B, M, 3, generator=g)
    keep = torch.rand(B, M, generator=g)
    grad_S = torch.randn(B, M, generator=g)
    if mask_kind == "none":
        mask = None
    else:
        mask = keep < {"p60": 0.6, "structure": 0.8}[mask_kind]
        if mask_kind == "structure":
            mask[-1] = False
        nan = torch.full_like(points, float("nan"))
        points, target = torch.where(mask[..., None], points, nan), torch.where(mask[..., None], target, nan)
    grp = None if groups is None else (torch.arange(M, dtype=torch.int32) // groups).expand(B, M).contiguous()
    return Case(points, target, mask, grp, thresholds, grad_S)


T8 = (0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def accuracy_cases():
    """{name: keyword arguments of random_case} of every case the GPU tests run, B = 3: no pair at all (M = 1); the edge of
    the 64-owner tile (63, 64, 65); one staged tile of 256 plus one point (257); several tiles with compaction active and
    NaN at the masked points (600, 40 % masked); a fully masked structure; groups of 4 consecutive points; one threshold and
    eight."""
    return {
        "M=1": dict(B=3, M=1, seed=101),
        "M=63": dict(B=3, M=63, noise=0.3, seed=102),
        "M=64": dict(B=3, M=64, noise=1.5, seed=103),
        "M=65": dict(B=3, M=65, noise=0.3, seed=104),
        "M=257": dict(B=3, M=257, noise=1.5, seed=105),
        "M=600 p60": dict(B=3, M=600, mask_kind="p60", noise=0.3, seed=106),
        "M=130 structure masked": dict(B=3, M=130, mask_kind="structure", noise=1.5, seed=107),
        "M=130 groups of 4": dict(B=3, M=130, groups=4, noise=0.3, seed=108),
        "M=70 T=1": dict(B=3, M=70, noise=0.3, seed=109, thresholds=(1.0,)),
        "M=70 T=8": dict(B=3, M=70, mask_kind="p60", groups=4, noise=1.5, seed=110, thresholds=T8),
    }
