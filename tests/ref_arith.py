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


def _nudge(v, ulps):
    """Non-negative v moved one float32 step up (ulps = +1) or down (-1): a 1-ulp-off hardware result.  Zero, infinity
    and NaN stay (the instructions return those exactly)."""
    v = np.asarray(v, dtype=F32)
    if ulps == 0:
        return v
    with np.errstate(over="ignore", invalid="ignore"):
        moved = np.nextafter(v, F32(np.inf) if ulps > 0 else F32(0))
        return np.where(np.isfinite(v) & (v > 0), moved, v).astype(F32)


def atan2_ps_model(y, x, rcp_ulps=0):
    """atan2_ps (csrc/ps_common.hpp) operation for operation in float32, with v_rcp_f32 modelled as the correctly rounded
    reciprocal moved by ``rcp_ulps`` steps (the instruction is good to 1 ulp)."""
    y = np.asarray(y, dtype=F32)
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.fmax(ax, ay), np.fmin(ax, ay)
        a = mn * _nudge((1.0 / mx.astype(F64)).astype(F32), rcp_ulps)
        a = np.where(mx == 0, F32(0), a)
        a = np.where(mn == F32(np.inf), F32(1), a).astype(F32)
        s = a * a
        p = F32(0.0028340641874819994)
        for c in (-0.016005029901862144, 0.042587608098983765, -0.07495445758104324, 0.10636754333972931,
                  -0.14202570915222168, 0.19992484152317047, -0.3333306610584259, 1.0):
            p = fma_f32(p, s, F32(c))
        r = a * p
        r = np.where(ay > ax, F32(1.5707963267948966) - r, r)
        r = np.where(np.signbit(x), F32(3.141592653589793) - r, r)
        r = np.where(np.isnan(x) | np.isnan(y), F32(np.nan), r)
        return np.copysign(r, y).astype(F32)


def acos_ps_model(x, sqrt_ulps=0):
    """acos_ps (csrc/ps_common.hpp) operation for operation in float32, with v_sqrt_f32 modelled as the correctly rounded
    square root moved by ``sqrt_ulps`` steps."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        p = F32(-0.0012624911)
        for c in (0.0066700901, -0.0170881256, 0.0308918810, -0.0501743046, 0.0889789874, -0.2145988016, 1.5707963050):
            p = fma_f32(p, ax, F32(c))
        r = p * _nudge(np.sqrt(F32(1.0) - ax), sqrt_ulps)
        return np.where(np.signbit(x), F32(3.141592653589793) - r, r).astype(F32)


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
