"""Host-side checks of the arithmetic probe (no GPU): the probe library compiles for gfx950 and refuses bad arguments
before touching a device; the input generators of tests/arith_cases.py are seeded; and a numpy float32 restatement of
atan2_ps / acos_ps (tests/ref_arith.py: fused multiply-adds modelled, the reciprocal and the square root correctly rounded
or one ulp off either way) stays inside the derived bounds tests/test_gpu_arith.py holds the device to, on the same
samples -- which keeps the bounds and the generators honest where there is no GPU."""
import ctypes

import numpy as np
import pytest

from tests import arith_cases as C
from tests import arith_probe as P
from tests import ref_arith as R


@pytest.fixture(scope="module")
def lib():
    return P.load()          # hipcc cross-compiles gfx950 without a GPU


def test_probe_builds_and_exports_only_the_entry_point(lib):
    from protstruc_amd import build
    assert not build.arith_probe_is_stale()
    assert hasattr(lib, P.ENTRY)
    product = ctypes.CDLL(build.build(force=False, verbose=False))
    assert not hasattr(product, P.ENTRY), "the probe must stay out of libprotstruc_hip.so"
    assert not hasattr(lib, "ps_abi_version"), "the probe library must not carry the product's entry points"
    codes = [code for code, _ in P.ARMS.values()]
    assert len(set(codes)) == len(codes) == 24


def test_probe_refuses_bad_arguments_without_a_device(lib):
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: every call below returns before any launch
    call = lib.ps_arith_probe_f32
    for name, (code, nargs) in P.ARMS.items():
        assert call(code, None, fake, fake, 8, None) == 1, name
        assert call(code, fake, fake, None, 8, None) == 1, name
        assert call(code, fake, fake, fake, -1, None) == 1, name
        if nargs == 2:
            assert call(code, fake, None, fake, 8, None) == 1, name
        assert call(code, fake, fake, fake, 0, None) == 0, name          # n == 0 launches nothing
        if nargs == 1:
            assert call(code, fake, None, fake, 0, None) == 0, name      # b is unused by one-argument arms
        else:
            assert call(code, fake, None, fake, 0, None) == 1, name
    for which in (-1, 7, 9, 14, 19, 25, 29, 35, 39, 43, 1 << 20):
        assert call(which, fake, fake, fake, 0, None) == 1, which


def test_generators_are_seeded():
    for make in (lambda: C.plane_sample(1 << 12, 1 << 12, 1 << 6), lambda: (C.cosine_sample(1 << 12, 1 << 6),),
                 lambda: C.division_sample(1 << 12, 1 << 12, 1 << 12), lambda: (C.ordinary(100, 3),), C.special_pairs,
                 lambda: (C.unary_specials(),)):
        for u, v in zip(make(), make()):
            assert u.dtype == np.float32 and np.array_equal(C.bits(u), C.bits(v))
    y, x = C.plane_sample()
    y2, x2 = C.plane_sample()
    assert np.array_equal(C.bits(y), C.bits(y2)) and np.array_equal(C.bits(x), C.bits(x2)) and 3.5e6 < y.size < 4.5e6


def test_generators_cover_what_they_promise():
    v = C.pair_specials()
    assert v.size == 15 and np.unique(C.bits(v)).size == 15 and C.special_pairs()[0].size == 225
    u = C.unary_specials()
    assert u.size == 23 and np.unique(C.bits(u)).size == 23
    cs = C.cosine_sample(1 << 10, 1 << 4)
    for c in (0.5, -0.5, 1.0, -1.0):
        centre = int(C.bits([c])[0])
        assert np.isin(np.arange(centre - 64, centre + 65, dtype=np.uint32), C.bits(cs)).all()
    assert np.isin(np.arange(0, 65, dtype=np.uint32), C.bits(cs)).all()
    assert np.isin(np.arange(0, 65, dtype=np.uint32) | np.uint32(1 << 31), C.bits(cs)).all()
    a, b = C.division_sample(1 << 8, 1 << 8, 1 << 14)
    with np.errstate(all="ignore"):
        q = np.abs(a[512:512 + (1 << 14)].astype(np.float64) / b[512:512 + (1 << 14)].astype(np.float64))
    assert ((q < 2.0 ** -125) | (q > 2.0 ** 126)).all() and (q < 2.0 ** -126).mean() > 0.6 and (q >= 2.0 ** 128).mean() > 0.1
    y, x = C.plane_sample(1 << 10, 1 << 10, 1 << 6)
    assert (np.abs(y) == np.abs(x)).sum() >= 4 * 64 and ((y == 0) & np.signbit(y)).any() and ((x == 0) & np.signbit(x)).any()
    e = C.sqrt_sweep_exponents()
    assert len(set(e)) == 7 and C.sqrt_sweep(e[3])[0] <= C.SQRT_EXACT_FROM < C.sqrt_sweep(e[4])[0]


@pytest.fixture(scope="module")
def plane():
    y, x = C.plane_sample()
    ok = C.atan2_strict_domain(y, x)
    y, x = y[ok], x[ok]
    return y, x, np.arctan2(y.astype(np.float64), x.astype(np.float64)), C.atan2_first_octant(y, x)


@pytest.mark.parametrize("rcp_ulps", [0, 1, -1])
def test_atan2_restatement_stays_inside_the_derived_bounds(plane, rcp_ulps):
    y, x, ref, octant = plane
    err = np.abs(R.atan2_ps_model(y, x, rcp_ulps).astype(np.float64) - ref)
    worst_octant, worst_plane = err[octant].max(), err.max()
    print(f"atan2_ps restatement, reciprocal {rcp_ulps:+d} ulp: first octant {worst_octant:.3e}, plane {worst_plane:.3e}")
    assert worst_octant <= C.ATAN2_OCTANT_BOUND and worst_plane <= C.ATAN2_PLANE_BOUND


@pytest.mark.parametrize("sqrt_ulps", [0, 1, -1])
def test_acos_restatement_stays_inside_the_derived_bounds(sqrt_ulps):
    x = C.cosine_sample()
    x = x[np.abs(x) <= 1]
    err = np.abs(R.acos_ps_model(x, sqrt_ulps).astype(np.float64) - np.arccos(x.astype(np.float64)))
    neg = np.signbit(x)
    worst_pos, worst_neg = err[~neg].max(), err[neg].max()
    print(f"acos_ps restatement, square root {sqrt_ulps:+d} ulp: x >= 0 {worst_pos:.3e}, x < 0 {worst_neg:.3e}")
    assert worst_pos <= C.ACOS_POS_BOUND and worst_neg <= C.ACOS_NEG_BOUND


def test_restatement_pins_the_special_results():
    y, x = C.special_pairs()
    got = R.atan2_ps_model(y, x)
    for yy, xx, want in ((0.0, -0.0, C.PI_F), (-0.0, 0.0, np.float32(-0.0)), (0.0, 0.0, np.float32(0.0)),
                         (-0.0, -0.0, -C.PI_F), (1.0, 0.0, C.HALF_PI_F), (-1.0, -0.0, -C.HALF_PI_F),
                         (1.0, np.inf, np.float32(0.0)), (-1.0, -np.inf, -C.PI_F), (np.inf, 1.0, C.HALF_PI_F)):
        at = (C.bits(y) == C.bits([yy])) & (C.bits(x) == C.bits([xx]))
        assert at.sum() == 1 and C.bits(got[at])[0] == C.bits([want])[0], (yy, xx)
    assert np.isnan(got[np.isnan(y) | np.isnan(x)]).all()
    u = C.unary_specials()
    a = R.acos_ps_model(u)
    assert C.bits(a[u == 1])[0] == 0 and C.bits(a[u == -1])[0] == C.bits([C.PI_F])[0]
    assert np.isnan(a[(np.abs(u) > 1) | np.isnan(u)]).all() and np.isfinite(a[np.abs(u) <= 1]).all()
