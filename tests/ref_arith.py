"""float32 models of the reference's arithmetic, in numpy, bit for bit.

The reference computes norms with ``torch.norm(x, dim=-1)`` and frames with
``torch.linalg.cross``; on the ATen CPU build the goldens were made with, both
use fused multiply-adds:

    torch.norm(v, dim=-1)      sqrt(fma(z, z, fma(y, y, x * x)))
    torch.linalg.cross(a, b)   fma(a_i, b_j, -(a_j * b_i)) per component
    (x * y).sum(-1)            (p0 + p1) + p2 (products rounded first)

while ``np.cross`` (the reference's dihedrals) is two rounded products and one
subtract.  These models are what the kernels' "exact" modes are held to;
``tests/test_reference_arithmetic.py`` pins each of them against ATen itself,
so a change of the ATen build fails there instead of silently moving the
target of the GPU tests.

numpy has no fused multiply-add, so ``fma_f32`` builds one: the float64
product of two float32 values is exact, ``p + c`` in float64 is exact up to
an error term recovered by TwoSum, and the only case in which rounding that
float64 sum to float32 differs from rounding the exact sum once is a float64
sum that lands exactly on a float32 midpoint while the error term is nonzero;
the sign of the error term then decides the direction.
"""
import numpy as np

F32 = np.float32
F64 = np.float64


def fma_f32(a, b, c):
    """Correctly rounded float32 a * b + c (IEEE fusedMultiplyAdd), elementwise."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    c = np.asarray(c, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(F64) * b.astype(F64)          # exact: 24 + 24 bits < 53, exponents within float64's range
        c64 = c.astype(F64)
        s = p + c64
        bb = s - p                                 # TwoSum: s + e == p + c exactly (when s is finite)
        e = (p - (s - bb)) + (c64 - bb)
        e = np.where(np.isfinite(e), e, 0.0)
        r = s.astype(F32)
        # the neighbour of r on the side of s, and r itself, as float64 (an overflowed r counts as +-2^128)
        r64 = np.where(np.isinf(r) & np.isfinite(s), np.copysign(2.0 ** 128, s), r.astype(F64))
        toward = np.where(s > r64, F32(np.inf), F32(-np.inf)).astype(F32)
        r_fin = np.where(np.isinf(r), np.copysign(np.finfo(F32).max, r), r).astype(F32)
        r2 = np.where(np.isinf(r), r_fin, np.nextafter(r, toward))
        r2_64 = r2.astype(F64)
        tie = np.isfinite(s) & (s != r64) & (s == (r64 + r2_64) * 0.5) & (e != 0)
        # at a tie the exact sum lies on r's side when e points from s toward r
        keep = (e > 0) == (r64 > s)
        out = np.where(tie & ~keep, r2, r)
    return out.astype(F32)


def dot_ref(a, b):
    """(a * b).sum(-1) over a last axis of 3: products rounded first, then (p0 + p1) + p2."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        return (p[..., 0] + p[..., 1]) + p[..., 2]


def norm_sq_ref(v):
    v = np.asarray(v, dtype=F32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return fma_f32(z, z, fma_f32(y, y, x * x))


def norm_ref(v):
    """torch.norm(v, dim=-1) over a last axis of 3."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(norm_sq_ref(v)).astype(F32)


def dist_ref(xyz):
    """pairwise_distance_matrix's dist for xyz (B, N, A, 3): (B, N, N, A, A), norm_ref of the differences."""
    xyz = np.asarray(xyz, dtype=F32)
    with np.errstate(invalid="ignore"):
        diff = xyz[:, :, None, :, None, :] - xyz[:, None, :, None, :, :]
    return norm_ref(diff)


def cross_fused(a, b):
    """torch.linalg.cross(a, b, dim=-1): each component fma(a_i, b_j, -(a_j * b_i))."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    a0, a1, a2 = a[..., 0], a[..., 1], a[..., 2]
    b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([fma_f32(a1, b2, -(a2 * b1)),
                         fma_f32(a2, b0, -(a0 * b2)),
                         fma_f32(a0, b1, -(a1 * b0))], axis=-1)


def cross_np(a, b):
    """np.cross(a, b) for (*, 3) operands: two rounded products and one subtract per component."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    a0, a1, a2 = a[..., 0], a[..., 1], a[..., 2]
    b0, b1, b2 = b[..., 0], b[..., 1], b[..., 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0], axis=-1)


def gram_schmidt_ref(a, b, c):
    """oracle.gram_schmidt from the models: (..., 3, 3) with columns e1, e2, e3."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    c = np.asarray(c, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v1 = c - b
        e1 = v1 / norm_ref(v1)[..., None]
        v2 = a - b
        u2 = v2 - dot_ref(e1, v2)[..., None] * e1
        e2 = u2 / norm_ref(u2)[..., None]
    e3 = cross_fused(e1, e2)
    return np.stack([e1, e2, e3], axis=-1)
