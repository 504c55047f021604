"""Inputs for the arithmetic primitives' tests (tests/test_gpu_arith.py on the device, tests/test_arith_host.py for the
numpy restatement): special-value tables, a sample of the (y, x) plane, of cosines, of division operands and the mantissa
sweeps for the square root -- all seeded, so two calls give the same bits -- and the error bounds the fast forms are held
to, which are derived from the routines' arithmetic (below), not measured.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
SEED = 0x5A17


def from_bits(u):
    return np.ascontiguousarray(np.asarray(u, dtype=np.uint32)).view(F32)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32)


FLT_MIN = from_bits([0x00800000])[0]
FLT_MAX = from_bits([0x7F7FFFFF])[0]
SUB_MIN = from_bits([0x00000001])[0]
SUB_MAX = from_bits([0x007FFFFF])[0]
PI_F = F32(np.pi)            # 0x40490fdb
HALF_PI_F = F32(np.pi / 2)   # 0x3fc90fdb
SQRT_EXACT_FROM = F32(2.0e-31)   # sqrt_rn_mk is correctly rounded from here on (ps_common.hpp)

# ---- the bounds of the fast forms against float64, absolute, on the strict domain ----
# Strict domain of atan2: both arguments finite and max(|x|, |y|) in [2^-126, 2^126) (v_rcp_f32 neither overflows nor
# leaves the normal range).  First octant (0 <= |y| <= x; copysign makes y < 0 the same bits): the result is a * P(a^2)
# with a = min * rcp(max): 1.0e-7 for the polynomial and its evaluation, plus 0.9e-7 = 1.5 * 2^-23 * a / (1 + a^2) at
# a = 1 for a 1-ulp reciprocal and the rounded product.  Full plane: the two reflections add |fl(pi/2) - pi/2| = 4.4e-8,
# half an ulp in [1, 2) = 6.0e-8, |fl(pi) - pi| = 8.7e-8 and half an ulp in [2, 4) = 1.19e-7.
ATAN2_OCTANT_BOUND = 1.9e-7
ATAN2_PLANE_BOUND = 5.0e-7
# acos_ps, sign bit clear: a relative 3.1e-7 (Horner 1e-7, 1 - |x| 3e-8, a 1-ulp v_sqrt_f32 1.2e-7, the product 6e-8) of a
# value up to pi / 2, plus 2e-8 for the polynomial of Abramowitz & Stegun 4.4.46.  Sign bit set: plus the pi reflection
# (8.7e-8 + 1.19e-7).
ACOS_POS_BOUND = 5.1e-7
ACOS_NEG_BOUND = 7.2e-7
# atan2_lib / acos_lib against float64, in ulps of the float32 nearest the float64 value.  They are the device library's
# routines (held to its atan2f / acosf bit for bit), so these are the library's figures: acosf stays inside the 2 ulp
# k3_arith.hpp used to quote for both; atan2f does not -- the MI355X measures 2.65 ulp with the identity holding (its v / u
# division is the `!fpmath 2.5 ulp` form), so its bound is that figure rounded up to a whole ulp.
ATAN2_LIB_ULP_BOUND = 3.0
ACOS_LIB_ULP_BOUND = 2.0


def atan2_strict_domain(y, x):
    mx = np.maximum(np.abs(x), np.abs(y))
    return np.isfinite(x) & np.isfinite(y) & (mx >= F32(2.0 ** -126)) & (mx < F32(2.0 ** 126))


def atan2_first_octant(y, x):
    """x's sign bit clear and |y| <= |x|: no reflection is taken (y < 0 only flips the sign bit at the end)."""
    return ~np.signbit(x) & (np.abs(y) <= np.abs(x))


# ---- special tables ----
def pair_specials():
    """+0, -0, +inf, -inf, NaN, +-FLT_MIN, +-FLT_MAX, +-smallest subnormal, +-largest subnormal, +-1"""
    v = [F32(0.0), F32(-0.0), F32(np.inf), F32(-np.inf), F32(np.nan)]
    for m in (FLT_MIN, FLT_MAX, SUB_MIN, SUB_MAX, F32(1.0)):
        v += [m, -m]
    return np.array(v, dtype=F32)


def special_pairs():
    """Every ordered pair of pair_specials(): (a, b), 225 each."""
    v = pair_specials()
    return np.repeat(v, v.size).copy(), np.tile(v, v.size).copy()


def unary_specials():
    """+-0, +-1, +-nextafter(1, 0), +-nextafter(1, 2), +-0.5, +-nextafter(0.5, .) both ways, +-2, +-inf, NaN, subnormals"""
    one, half = F32(1.0), F32(0.5)
    m = [F32(0.0), one, np.nextafter(one, F32(0)), np.nextafter(one, F32(2)), half, np.nextafter(half, F32(0)),
         np.nextafter(half, F32(1)), F32(2.0), F32(np.inf), SUB_MIN, SUB_MAX]
    v = [F32(np.nan)]
    for x in m:
        v += [x, -x]
    return np.array(v, dtype=F32)


def ordinary(n, stream=0):
    """n ordinary values (normal, magnitude 2^-4 .. 2^4, either sign): the neighbours of the special tables."""
    rng = np.random.default_rng([SEED, 100, stream])
    return (np.exp2(rng.uniform(-4.0, 4.0, n)) * rng.choice([-1.0, 1.0], n)).astype(F32)


# ---- the (y, x) plane ----
def plane_sample(n_polar=1 << 21, n_ratio=1 << 20, n_edge=1 << 14):
    """(y, x), about 3.7 M points in three blocks: angle uniform in (-pi, pi] at a radius log-uniform in 2^-60 .. 2^60;
    min / max log-uniform in 2^-40 .. 1 in a random octant; the boundaries |y| == |x|, y == +-0, x == +-0 and one ulp
    either side of each, in all four sign combinations."""
    rng = np.random.default_rng([SEED, 1])
    th = np.pi - 2.0 * np.pi * rng.random(n_polar)                      # (-pi, pi]
    r = np.exp2(rng.uniform(-60.0, 60.0, n_polar))
    y1, x1 = (r * np.sin(th)).astype(F32), (r * np.cos(th)).astype(F32)

    mx = np.exp2(rng.uniform(-60.0, 60.0, n_ratio)).astype(F32)
    mn = (mx.astype(F64) * np.exp2(rng.uniform(-40.0, 0.0, n_ratio))).astype(F32)
    swap = rng.random(n_ratio) < 0.5
    sy, sx = rng.choice([-1.0, 1.0], n_ratio).astype(F32), rng.choice([-1.0, 1.0], n_ratio).astype(F32)
    y2, x2 = sy * np.where(swap, mx, mn), sx * np.where(swap, mn, mx)

    m = np.exp2(rng.uniform(-60.0, 60.0, n_edge)).astype(F32)
    up, dn = np.nextafter(m, F32(np.inf)), np.nextafter(m, F32(0))
    zero, tiny = np.zeros_like(m), np.full_like(m, SUB_MIN)
    ys, xs = [], []
    for ay, ax in ((m, m), (up, m), (dn, m), (m, up), (m, dn), (zero, m), (tiny, m), (m, zero), (m, tiny)):
        for qy in (1.0, -1.0):
            for qx in (1.0, -1.0):
                ys.append(F32(qy) * ay)
                xs.append(F32(qx) * ax)
    y = np.concatenate([y1, y2] + ys).astype(F32)
    x = np.concatenate([x1, x2] + xs).astype(F32)
    return y, x


# ---- cosines ----
def cosine_sample(n_uniform=1 << 21, n_per_k=1 << 13):
    """Uniform in [-1, 1]; +-(1 - 2^-k u), u in (0, 1], for k = 1 .. 24; every float within 64 ulp of 0.5, -0.5, 1, -1 and
    0 (those beyond +-1 are the |x| > 1 cases)."""
    rng = np.random.default_rng([SEED, 2])
    parts = [rng.uniform(-1.0, 1.0, n_uniform).astype(F32)]
    for k in range(1, 25):
        v = (1.0 - np.exp2(-k) * (1.0 - rng.random(n_per_k))).astype(F32)
        parts += [v, -v]
    step = np.arange(-64, 65, dtype=np.int64)
    for c in (0.5, 1.0):
        near = from_bits((int(bits([c])[0]) + step).astype(np.uint32))
        parts += [near, -near]
    sub = from_bits(np.arange(0, 65, dtype=np.uint32))
    parts += [sub, -sub]
    return np.concatenate(parts).astype(F32)


# ---- division operands ----
def _normal(rng, n):
    return from_bits((rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))
                     | (rng.integers(1, 255, n, dtype=np.uint32) << np.uint32(23))
                     | rng.integers(0, 1 << 23, n, dtype=np.uint32))


def division_sample(n_bits=1 << 24, n_normal=1 << 24, n_edge=1 << 22):
    """(a, b): uniformly random bit patterns; normal pairs at any exponent; pairs whose quotient is subnormal (or rounds to
    zero or FLT_MIN) or overflows; the special table."""
    rng = np.random.default_rng([SEED, 3])
    a1 = from_bits(rng.integers(0, 1 << 32, n_bits, dtype=np.uint64).astype(np.uint32))
    b1 = from_bits(rng.integers(0, 1 << 32, n_bits, dtype=np.uint64).astype(np.uint32))
    a2, b2 = _normal(rng, n_normal), _normal(rng, n_normal)
    # exponent difference ea - eb: -152 .. -126 (quotient below 2^-125: subnormal, zero or just normal) for three quarters,
    # 127 .. 130 (at or beyond the overflow threshold) for the rest
    d = np.where(rng.random(n_edge) < 0.75, rng.integers(-152, -125, n_edge), rng.integers(127, 131, n_edge))
    lo, hi = np.maximum(-126, -126 + d), np.minimum(127, 127 + d)        # ea's range such that eb = ea - d is normal too
    ea = lo + (rng.random(n_edge) * (hi - lo + 1)).astype(np.int64)
    eb = ea - d
    mant = lambda: rng.integers(0, 1 << 23, n_edge, dtype=np.uint32)     # noqa: E731
    sign = lambda: rng.integers(0, 2, n_edge, dtype=np.uint32) << np.uint32(31)   # noqa: E731
    a3 = from_bits(sign() | ((ea + 127).astype(np.uint32) << np.uint32(23)) | mant())
    b3 = from_bits(sign() | ((eb + 127).astype(np.uint32) << np.uint32(23)) | mant())
    a4, b4 = special_pairs()
    return np.concatenate([a1, a2, a3, a4]).astype(F32), np.concatenate([b1, b2, b3, b4]).astype(F32)


# ---- mantissa sweeps for the square root ----
def sqrt_sweep_exponents():
    """Biased exponents whose 2^23 mantissas are swept: 2^0 and 2^1 (both parities), the binade of 2.0e-31 and the one on
    either side, the lowest normal binade and the highest finite one."""
    e0 = int(bits([SQRT_EXACT_FROM])[0] >> 23)
    return (127, 128, e0 - 1, e0, e0 + 1, 1, 254)


def sqrt_sweep(biased_exponent):
    return from_bits(np.arange(1 << 23, dtype=np.uint32) | np.uint32(biased_exponent << 23))


def ulps_of_f32(err, ref):
    """|err| in ulps of the float32 nearest the float64 ``ref``."""
    with np.errstate(over="ignore"):
        spacing = np.spacing(np.abs(ref).astype(F32)).astype(F64)
    return np.abs(err) / spacing
