"""Float64 numpy restatement of the pair-head kernels K33 - K36 (include/protstruc_pairhead.h) and of the functions built on
them: geometry to bin index, the binned cross-entropy with its gradient, softmax expectations, PAE, contact probability and
pTM.  The squared quantity of K33 keeps the stated operation order -- numpy rounds every float64 operation on its own --, so
bins and ``value`` are comparable for equality.  No GPU code; the yardstick of tests/test_pairhead_host.py and
tests/test_gpu_pairhead.py, which also take their cases from here."""
import math

import numpy as np

NO_TARGET = 255
F64 = np.float64


# ---- K33 -----------------------------------------------------------------------------------------------------------------------
def sq_breaks(breaks):
    b = np.asarray(breaks, dtype=np.float32).astype(F64)
    return b * b


def distance_v2(points):
    """(B,N,N) float64: [b,i,j] = |Xj - Xi|^2 as (dx*dx + dy*dy) + dz*dz"""
    X = np.asarray(points, dtype=np.float32).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = X[:, None, :, :] - X[:, :, None, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _local(rot, trans, points):
    """(B,N,N,3) float64: [b,i,j] = Ri^T (xj - ti), component c as (R0c*d0 + R1c*d1) + R2c*d2"""
    R, t, x = (np.asarray(a, dtype=np.float32).astype(F64) for a in (rot, trans, points))
    d = x[:, None, :, :] - t[:, :, None, :]
    return np.stack([(R[:, :, None, 0, c] * d[..., 0] + R[:, :, None, 1, c] * d[..., 1]) + R[:, :, None, 2, c] * d[..., 2]
                     for c in range(3)], axis=-1)


def aligned_v2(rot, trans, points, target_rot, target_trans, target_points):
    with np.errstate(invalid="ignore", over="ignore"):
        e = _local(rot, trans, points) - _local(target_rot, target_trans, target_points)
        return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def bins_of(v2, breaks, row_mask=None, col_mask=None):
    """(bins (B,N,N) uint8, value (B,N,N) float32) of the squared quantity v2"""
    B, N, _ = v2.shape
    row = np.ones((B, N), dtype=bool) if row_mask is None else np.asarray(row_mask) != 0
    col = np.ones((B, N), dtype=bool) if col_mask is None else np.asarray(col_mask) != 0
    counts = row[:, :, None] & col[:, None, :] & np.isfinite(v2)
    safe = np.where(counts, v2, 0.0)
    bins = (safe[..., None] > sq_breaks(breaks)).sum(-1)
    return (np.where(counts, bins, NO_TARGET).astype(np.uint8),
            np.where(counts, np.sqrt(safe), np.inf).astype(np.float32))


def bins_distance(points, breaks, row_mask=None, col_mask=None):
    return bins_of(distance_v2(points), breaks, row_mask, col_mask)


def bins_aligned_error(rot, trans, points, target_rot, target_trans, target_points, breaks, frame_mask=None, point_mask=None):
    return bins_of(aligned_v2(rot, trans, points, target_rot, target_trans, target_points), breaks, frame_mask, point_mask)


# ---- K34 / K35 / K36 -----------------------------------------------------------------------------------------------------------
class CrossEntropy:
    """Everything about the cross-entropy of ``logits`` (B,N,N,C) float32 against ``bins`` (B,N,N), in float64: ``counted``,
    ``lse`` and ``ce`` per pair (0 where not counted), ``p`` the softmax, ``row_loss`` and ``row_count`` (B,N)."""

    def __init__(self, logits, bins):
        x = np.asarray(logits, dtype=np.float32).astype(F64)
        C = x.shape[-1]
        bins = np.asarray(bins).astype(np.int64)
        self.counted = (bins >= 0) & (bins < C)
        x = np.where(self.counted[..., None], x, 0.0)          # the logits of an uncounted pair never reach anything
        with np.errstate(invalid="ignore", divide="ignore"):
            m = x.max(-1)
            self.lse = m + np.log(np.exp(x - m[..., None]).sum(-1))
            self.p = np.exp(x - self.lse[..., None])
        self.label = np.where(self.counted, bins, 0)
        target = np.take_along_axis(x, self.label[..., None], -1)[..., 0]
        self.ce = np.where(self.counted, self.lse - target, 0.0)
        self.lse = np.where(self.counted, self.lse, 0.0)
        self.row_loss = self.ce.sum(-1)
        self.row_count = self.counted.sum(-1).astype(np.int32)
        self.C = C

    def pair_bound(self):
        """the per-pair error bound of K34 (0 where not counted): 2^-22 (2 + ln C + |lse| + |ce|) + C 2^-24"""
        E = 2.0 ** -22 * (2.0 + math.log(self.C) + np.abs(self.lse) + np.abs(self.ce)) + self.C * 2.0 ** -24
        return np.where(self.counted, E, 0.0)

    def row_bound(self):
        return self.pair_bound().sum(-1) + 2.0 ** -24 * np.abs(self.row_loss)

    def backward(self, grad_row):
        """grad_logits (B,N,N,C) float64: grad_row * (p - onehot), exact zeros where not counted"""
        g = np.asarray(grad_row, dtype=np.float32).astype(F64)[:, :, None, None]
        onehot = np.arange(self.C) == self.label[..., None]
        return np.where(self.counted[..., None], g * (self.p - onehot), 0.0)


def softmax(logits):
    x = np.asarray(logits, dtype=np.float32).astype(F64)
    with np.errstate(invalid="ignore"):
        e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def expectation(logits, values):
    """(V,B,N,N) float64: sum_k softmax(x)_k values[b,v,k]"""
    return np.einsum("bijk,bvk->vbij", softmax(logits), np.asarray(values).astype(F64))


def expectation_bound(values, C):
    """max_k |v_k| (2^-22 (2 + ln C) + C 2^-23), per (v, b): shape (V,B,1,1)"""
    top = np.abs(np.asarray(values).astype(F64)).max(-1).T
    return top[:, :, None, None] * (2.0 ** -22 * (2.0 + math.log(C)) + C * 2.0 ** -23)


# ---- breaks, centres and what is read out of the logits ------------------------------------------------------------------------
def distogram_breaks(first=2.3125, last=21.6875, n_bins=64):
    return np.linspace(first, last, n_bins - 1).astype(np.float32)


def aligned_error_breaks(max_bin=31.0, n_bins=64):
    return np.linspace(0.0, max_bin, n_bins - 1).astype(np.float32)


def aligned_error_bin_centers(max_bin=31.0, n_bins=64):
    breaks = aligned_error_breaks(max_bin, n_bins).astype(F64)
    step = breaks[1] - breaks[0] if breaks.size > 1 else breaks[0]
    centers = breaks + step / 2
    return np.concatenate([centers, centers[-1:] + step])


def predicted_aligned_error(logits, max_bin=31.0):
    C = np.asarray(logits).shape[-1]
    return (softmax(logits) * aligned_error_bin_centers(max_bin, C)).sum(-1)


def contact_probability(logits, cutoff=8.0, breaks=None):
    C = np.asarray(logits).shape[-1]
    breaks = distogram_breaks(n_bins=C) if breaks is None else np.asarray(breaks, dtype=np.float32)
    inside = np.zeros(C)
    inside[:C - 1] = breaks <= np.float32(cutoff)
    return (softmax(logits) * inside).sum(-1)


def tm_kernel(n_residues, max_bin=31.0, n_bins=64):
    """(C,) float64: 1 / (1 + (c_k / d0)^2) with d0 of a structure of ``n_residues``"""
    d0 = 1.24 * (max(float(n_residues), 19.0) - 15.0) ** (1.0 / 3.0) - 1.8
    return 1.0 / (1.0 + (aligned_error_bin_centers(max_bin, n_bins) / d0) ** 2)


def predicted_tm_score(logits, residue_mask, chain_idx=None, interface=False, max_bin=31.0):
    p = softmax(logits)
    B, N, _, C = p.shape
    mask = (np.asarray(residue_mask) != 0).astype(F64)
    out = np.zeros(B)
    for b in range(B):
        term = (p[b] * tm_kernel(mask[b].sum(), max_bin, C)).sum(-1)
        pair = mask[b][:, None] * mask[b][None, :]
        if interface:
            chain = np.asarray(chain_idx)[b]
            pair = pair * (chain[:, None] != chain[None, :])
        per_row = (term * pair).sum(-1) / (1e-8 + pair.sum(-1))
        out[b] = (per_row * mask[b]).max()
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def masks(B, N, seed, keep=0.55):
    """(row_mask, col_mask) (B,N) bool, different from each other, 45 % masked; at N > 1 at least one of each kept"""
    rng = np.random.default_rng(seed)
    row, col = rng.random((B, N)) < keep, rng.random((B, N)) < keep
    row[:, 0], col[:, -1] = True, True
    return row, col


def backbone_case(B, N, seed):
    """(B,N,3,3) float32 N / CA / C coordinates of a random walk with 3.8 A steps: the chain frames are built from"""
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(B, N, 3))
    ca = np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=1)
    arms = rng.normal(size=(B, N, 2, 3))
    arms = 1.5 * arms / np.linalg.norm(arms, axis=-1, keepdims=True)
    return np.stack([ca + arms[:, :, 0], ca, ca + arms[:, :, 1]], axis=2).astype(np.float32)


def lattice_points(B, N, seed, extent=7):
    """integer points: squared distances are small integers, many of them perfect squares"""
    return np.random.default_rng(seed).integers(-extent, extent + 1, size=(B, N, 3)).astype(np.float32)


def lattice_frames(B, N, seed):
    """signed permutation matrices and integer origins: the aligned error of lattice points is an exact integer vector"""
    rng = np.random.default_rng(seed)
    rot = np.zeros((B, N, 3, 3), dtype=np.float32)
    for b in range(B):
        for i in range(N):
            rot[b, i, np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], size=3)
    return rot, rng.integers(-4, 5, size=(B, N, 3)).astype(np.float32)


LOGIT_FAMILIES = ("normal", "equal", "spread", "spike", "minus_inf", "nan_under_no_target")


def logits_case(family, B, N, C, seed):
    """(logits (B,N,N,C) float32, bins (B,N,N) uint8): about a tenth of the labels are 255, and in the last family NaN
    logits sit under every one of those"""
    rng = np.random.default_rng(seed)
    bins = rng.integers(0, C, size=(B, N, N)).astype(np.uint8)
    bins[rng.random((B, N, N)) < 0.1] = NO_TARGET
    x = rng.normal(size=(B, N, N, C))
    if family == "equal":
        x = np.full((B, N, N, C), 0.75)
    elif family == "spread":
        x = rng.uniform(-30.0, 30.0, size=(B, N, N, C))
    elif family == "spike":
        np.put_along_axis(x, rng.integers(0, C, size=(B, N, N, 1)), 1e4, axis=-1)
    x = x.astype(np.float32)
    if family == "minus_inf":
        gone = rng.random((B, N, N, C)) < 1.0 / 3.0
        label = np.where(bins < C, bins, 0).astype(np.int64)
        np.put_along_axis(gone, label[..., None], False, axis=-1)      # the target stays finite
        x[gone] = -np.inf
    elif family == "nan_under_no_target":
        x[bins == NO_TARGET] = np.nan
    return x, bins
