"""GPU tests of the float32 arithmetic primitives themselves (csrc/ps_common.hpp: sqrt_rn_mk, atan2_ps, acos_ps;
csrc/k3_arith.hpp: atan2_k3, atan2_lib, acos_lib, the packed *_v and multi-column *_vn forms, div_ieee_vn), one routine at
a time through the test-only probe (tests/native/arith_probe.hip, tests/arith_probe.py) on inputs the geometry kernels
never feed them: infinities, signed zeros, subnormals, |cos| > 1, the boundaries |y| == |x| and |x| == 0.5 and their
neighbours, whole binades of mantissas (tests/arith_cases.py).

Yardsticks: float64 np.arctan2 / np.arccos of the float32 inputs for accuracy, correctly rounded np.sqrt and numpy's
float32 division for the routines that claim correct rounding, the device library's own atan2f / acosf / sqrtf for the
routines that claim to BE the library, and the scalar forms for the packed and multi-column ones (bit for bit).  The
bounds of the fast forms are derived in tests/arith_cases.py, not measured; what the device measures is printed, and
written to the file PS_ARITH_RECORD names, if set (profiles/arith_probe_errors.json is such a record).

Device-against-device comparisons stay on the device (int32 views, any NaN equal to any NaN); data comes to the host only
for the float64 references.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import arith_cases as C
from tests import arith_probe as P

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7BEEF
TAILS = (1, 2, 7, 8, 9, 511, 512, 513)
SCALAR_OF = {form: scalar for scalar, forms in P.FORMS.items() for form in forms}
RESTATED = "k3_arith.hpp's atan2_lib / acos_lib were read off ROCm 7.2's ocml"


@pytest.fixture(scope="module")
def probe():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    P.load()                                  # builds the probe library if it is stale; a no-op when fresh
    return P


@pytest.fixture(scope="module")
def record():
    """Measured maxima per arm, printed (and written to $PS_ARITH_RECORD) when the module's tests are done."""
    rec = {"rocm": P.rocm_version(), "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
           "bounds": {"atan2_first_octant": C.ATAN2_OCTANT_BOUND, "atan2_plane": C.ATAN2_PLANE_BOUND,
                      "acos_ps_positive": C.ACOS_POS_BOUND, "acos_ps_negative": C.ACOS_NEG_BOUND,
                      "atan2_lib_ulp": C.ATAN2_LIB_ULP_BOUND, "acos_lib_ulp": C.ACOS_LIB_ULP_BOUND},
           "samples": {}, "measured": {}}
    yield rec
    text = json.dumps(rec, indent=1, sort_keys=True)
    print("\narith probe record:\n" + text)
    path = os.environ.get("PS_ARITH_RECORD")
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return (a.view(torch.int32) == b.view(torch.int32)) | (a.isnan() & b.isnan())


def assert_same_bits(got, want, what, *inputs, where=None, note=""):
    """got == want bit for bit (any NaN equals any NaN), on ``where`` if given; the message shows the first mismatches."""
    bad = ~same_bits(got, want)
    if where is not None:
        bad &= where
    n_bad = int(bad.sum().item())
    if n_bad:
        rows = []
        for i in bad.nonzero().flatten()[:6].tolist():
            ins = ", ".join("0x%08x (%r)" % (t[i].view(torch.int32).item() & 0xFFFFFFFF, t[i].item()) for t in inputs)
            rows.append("  [%d] in = %s: got 0x%08x (%r), want 0x%08x (%r)" % (
                i, ins, got[i].view(torch.int32).item() & 0xFFFFFFFF, got[i].item(),
                want[i].view(torch.int32).item() & 0xFFFFFFFF, want[i].item()))
        pytest.fail(f"{what}: {n_bad} of {got.numel()} differ{note}\n" + "\n".join(rows))


# ---- the samples, made once ----
@pytest.fixture(scope="module")
def plane(probe, record):
    y, x = C.plane_sample()
    record["samples"]["plane"] = int(y.size)
    return {"y": y, "x": x, "dy": dev(y), "dx": dev(x)}


@pytest.fixture(scope="module")
def cosines(probe, record):
    c = C.cosine_sample()
    record["samples"]["cosine"] = int(c.size)
    return {"c": c, "dc": dev(c)}


@pytest.fixture(scope="module")
def division(probe, record):
    a, b = C.division_sample()
    with np.errstate(all="ignore"):
        q = a / b          # numpy's float32 division: the float64 quotient rounded once, i.e. IEEE
    record["samples"]["division"] = int(a.size)
    return {"da": dev(a), "db": dev(b), "dq": dev(q)}


def table(nargs):
    return C.special_pairs() if nargs == 2 else (C.unary_specials(),)


def laid_out(tab, offset, spaced, stream=0):
    """The special table behind ``offset`` ordinary values -- contiguous (special neighbours) or, ``spaced``, as
    [ordinary, special, ordinary] triples (ordinary neighbours; 3 is coprime to every lane width, so over the offsets
    every special meets every (column, half) slot).  Returns the arrays and the positions of the specials."""
    n = tab[0].size
    outs = []
    for k, t in enumerate(tab):
        if spaced:
            body = C.ordinary(3 * n, stream + 10 * k + 1)
            body[1::3] = t
        else:
            body = t
        outs.append(np.concatenate([C.ordinary(offset, stream + 10 * k + 2), body]).astype(np.float32))
    pos = offset + (1 + 3 * np.arange(n) if spaced else np.arange(n))
    return outs, pos


# ---- 1. packed and multi-column forms equal the scalar forms bit for bit ----
@pytest.mark.parametrize("scalar", sorted(P.FORMS))
def test_forms_equal_the_scalar_form_on_the_samples(probe, plane, cosines, division, scalar):
    if P.ARMS[scalar][1] == 2:
        inputs = [("plane", plane["dy"], plane["dx"]), ("division", division["da"], division["db"])]
    else:
        inputs = [("cosine", cosines["dc"], None), ("plane y", plane["dy"], None), ("division a", division["da"], None)]
    for name, a, b in inputs:
        want = P.run(scalar, a, b)
        for form in P.FORMS[scalar]:
            assert_same_bits(P.run(form, a, b), want, f"{form} against {scalar} on the {name} sample", a, *([b] if b is not None else []))


@pytest.mark.parametrize("scalar", sorted(P.FORMS))
def test_forms_equal_the_scalar_form_on_specials_in_every_slot(probe, scalar):
    tab = table(P.ARMS[scalar][1])
    for form in P.FORMS[scalar]:
        lane = P.LANE_ELEMS[form]
        for spaced in (False, True):
            slots = np.zeros((tab[0].size, lane), dtype=bool)
            for offset in range(lane):
                arrays, pos = laid_out(tab, offset, spaced, stream=offset)
                slots[np.arange(pos.size), pos % lane] = True
                d = [dev(a) for a in arrays]
                assert_same_bits(P.run(form, *d), P.run(scalar, *d),
                                 f"{form} against {scalar}, special table at offset {offset}, spaced={spaced}", *d)
            assert slots.all(), "a special value missed a (column, half) slot"


@pytest.mark.parametrize("arm", sorted(P.ARMS))
def test_tails_are_computed_and_nothing_else_is_written(probe, arm):
    nargs = P.ARMS[arm][1]
    arrays, _ = laid_out(table(nargs), 0, True, stream=77)
    long = [dev(np.resize(a, 1024)) for a in arrays]
    want = P.run(SCALAR_OF.get(arm, arm), *long)
    front, back = 3, 9                       # out starts off any 8- or 16-byte boundary; back > the widest lane
    for n in TAILS:
        ins = [t[:n].clone() for t in long]
        buf = torch.full((front + n + back,), SENTINEL, dtype=torch.int32, device="cuda")
        out = buf.view(torch.float32)[front:front + n]
        P.run(arm, *ins, out=out)
        torch.cuda.synchronize()
        assert (buf[:front] == SENTINEL).all() and (buf[front + n:] == SENTINEL).all(), f"{arm}, n = {n}: a sentinel changed"
        assert_same_bits(out, want[:n], f"{arm}, n = {n}", *ins)


# ---- 2. sqrt_rn_mk against the correctly rounded square root ----
def assert_sqrt_rule(got, want, x, what):
    """Equal bits for every x >= 2.0e-31; at most 1 ulp below, on normal x; +-0, subnormals and +inf come back as x;
    negative normals, -inf and NaN give NaN."""
    exact_from = float(C.SQRT_EXACT_FROM)
    as_x = (x == 0) | (x.abs() < float(C.FLT_MIN)) | (x == float("inf"))
    nan = x.isnan() | ((x < 0) & ~as_x)
    assert_same_bits(got, x, f"{what}: zero, subnormal and +inf inputs come back unchanged", x, where=as_x)
    assert bool(got[nan].isnan().all()), f"{what}: negative or NaN input did not give NaN"
    assert_same_bits(got, want, f"{what}: x >= 2.0e-31", x, where=(x >= exact_from) & ~as_x)
    low = (x >= float(C.FLT_MIN)) & (x < exact_from)
    off = (got.view(torch.int32)[low] - want.view(torch.int32)[low]).abs()
    worst = int(off.max().item()) if off.numel() else 0
    assert worst <= 1, f"{what}: {worst} ulp off for a normal x below 2.0e-31"
    return worst, int((off != 0).sum().item()) if off.numel() else 0


def test_sqrt_rn_mk_is_correctly_rounded_on_the_mantissa_sweeps(probe, record):
    below = {}
    for e in C.sqrt_sweep_exponents():
        x = C.sqrt_sweep(e)
        dx, dref = dev(x), dev(np.sqrt(x))
        assert_same_bits(P.run("sqrtf", dx), dref, f"the library's sqrtf against np.sqrt, biased exponent {e}", dx)
        worst, count = assert_sqrt_rule(P.run("sqrt_rn_mk", dx), dref, dx, f"sqrt_rn_mk, biased exponent {e}")
        below[str(e)] = {"max_ulp_below_2e-31": worst, "inexact_below_2e-31": count}
    record["measured"]["sqrt_rn_mk_sweeps"] = below
    x = dev(np.concatenate([C.unary_specials(), C.pair_specials()]))
    with np.errstate(invalid="ignore"):
        ref = dev(np.sqrt(host(x)))
    assert_sqrt_rule(P.run("sqrt_rn_mk", x), ref, x, "sqrt_rn_mk on the special tables")


def test_sqrt_rn_mk_against_sqrtf_on_every_non_negative_float(probe, record):
    worst = inexact = 0
    for chunk in range(32):
        x = torch.arange(chunk << 26, (chunk + 1) << 26, dtype=torch.int64, device="cuda").to(torch.int32).view(torch.float32)
        got = P.run("sqrt_rn_mk", x)
        w, c = assert_sqrt_rule(got, P.run("sqrtf", x), x, f"sqrt_rn_mk against sqrtf, bit patterns from {chunk << 26:#x}")
        assert_same_bits(P.run("sqrt_rn_mk_v", x), got, f"sqrt_rn_mk_v against sqrt_rn_mk, bit patterns from {chunk << 26:#x}", x)
        worst, inexact = max(worst, w), inexact + c
    record["measured"]["sqrt_rn_mk_exhaustive"] = {"max_ulp_below_2e-31": worst, "inexact_below_2e-31": inexact}


# ---- 3. the divisions against numpy's float32 division ----
@pytest.mark.parametrize("arm", ["div", "div_ieee_vn2", "div_ieee_vn4"])
def test_division_is_ieee(probe, division, arm):
    a, b, q = division["da"], division["db"], division["dq"]
    got = P.run(arm, a, b)
    assert bool(got[q.isnan()].isnan().all()), f"{arm}: a NaN quotient came out as a number"
    assert_same_bits(got, q, f"{arm} against numpy float32 division", a, b, where=~q.isnan())


# ---- 4. the fast forms against float64 ----
def pinned_pairs():
    """The pairs of the special table without subnormal or FLT_MAX members (those are outside the strict domain)."""
    y, x = C.special_pairs()
    plain = lambda v: ~np.isfinite(v) | (v == 0) | ((np.abs(v) >= C.FLT_MIN) & (np.abs(v) <= 1))     # noqa: E731
    keep = plain(y) & plain(x)
    return y[keep], x[keep]


@pytest.mark.parametrize("arm", ["atan2_ps", "atan2_k3"])
def test_fast_atan2_signs_and_special_results(probe, arm):
    y, x = pinned_pairs()
    assert y.size == 81
    got = host(P.run(arm, dev(y), dev(x)))
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    want_nan = np.isnan(ref)
    unspecified = np.zeros_like(want_nan)
    if arm == "atan2_k3":
        # the documented deviations (k3_arith.hpp): an infinite x gives NaN; a NaN y alone is not propagated
        want_nan = np.isnan(x) | np.isinf(x)
        unspecified = np.isnan(y) & ~want_nan
    for i in range(y.size):
        what = f"{arm}({y[i]!r}, {x[i]!r}) = {got[i]!r}"
        if unspecified[i]:
            continue
        if want_nan[i]:
            assert np.isnan(got[i]), what
            continue
        assert not np.isnan(got[i]) and np.signbit(got[i]) == np.signbit(ref[i]), what + f", IEEE gives {ref[i]!r}"
        exact = y[i] == 0 or x[i] == 0 or (np.isinf(y[i]) != np.isinf(x[i]))       # 0, pi / 2 or pi
        if exact:
            assert C.bits([got[i]])[0] == C.bits([np.float32(ref[i])])[0], what + f", IEEE gives fl({ref[i]!r})"
        else:
            bound = C.ATAN2_OCTANT_BOUND if C.atan2_first_octant(y[i], x[i]) else C.ATAN2_PLANE_BOUND
            assert abs(float(got[i]) - ref[i]) <= bound, what + f", float64 gives {ref[i]!r}"
    if arm == "atan2_ps":       # the inf / inf quarters are the +-1 / +-1 ones (a = 1 in both)
        inf = np.isinf(y) & np.isinf(x)
        ones = host(P.run(arm, dev(np.sign(y[inf])), dev(np.sign(x[inf]))))
        assert inf.sum() == 4 and np.array_equal(C.bits(got[inf]), C.bits(ones))


@pytest.mark.parametrize("arm", ["atan2_ps", "atan2_k3"])
def test_fast_atan2_against_float64(probe, plane, record, arm):
    ty, tx = C.special_pairs()
    y, x = np.concatenate([plane["y"], ty]), np.concatenate([plane["x"], tx])
    got = host(P.run(arm, dev(y), dev(x))).astype(np.float64)
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    strict = C.atan2_strict_domain(y, x)
    octant = strict & C.atan2_first_octant(y, x)
    worst_octant, worst_plane = float(err[octant].max()), float(err[strict].max())
    # outside the strict domain (subnormal or >= 2^126 magnitudes: v_rcp_f32 over- or underflows): recorded, not bounded
    outside = np.isfinite(y) & np.isfinite(x) & ~strict
    fin = outside & np.isfinite(got)
    at = lambda m: [float(v) for v in (y[m][np.argmax(err[m])], x[m][np.argmax(err[m])])]     # noqa: E731
    rec = {"first_octant_max_abs_err": worst_octant, "plane_max_abs_err": worst_plane,
           "first_octant_worst_at_y_x": at(octant), "plane_worst_at_y_x": at(strict),
           "outside_worst_at_y_x": at(fin) if fin.any() else None,
           "strict_points": int(strict.sum()), "first_octant_points": int(octant.sum()),
           "outside_points": int(outside.sum()), "outside_not_finite": int((outside & ~np.isfinite(got)).sum()),
           "outside_max_abs_err_where_finite": float(err[fin].max()) if fin.any() else None}
    record["measured"][arm] = rec
    print(f"\n{arm}: {rec}")
    assert octant.sum() > 5e5 and outside.sum() > 50
    if arm == "atan2_k3":       # the clamp of max(|x|, |y|) at FLT_MIN keeps every finite pair's result finite (k3_arith.hpp)
        assert np.isfinite(got[outside]).all() and (np.abs(got[outside]) <= float(C.PI_F)).all()
    else:                       # a huge maximum only underflows the reciprocal: the result stays a finite angle
        huge = outside & (np.maximum(np.abs(x), np.abs(y)) >= 2.0 ** 126)
        assert huge.any() and np.isfinite(got[huge]).all() and (np.abs(got[huge]) <= float(C.PI_F)).all()
    assert worst_octant <= C.ATAN2_OCTANT_BOUND, f"{arm}: {worst_octant:.3e} in the first octant, derived bound {C.ATAN2_OCTANT_BOUND}"
    assert worst_plane <= C.ATAN2_PLANE_BOUND, f"{arm}: {worst_plane:.3e} on the plane, derived bound {C.ATAN2_PLANE_BOUND}"


def test_fast_acos_against_float64(probe, cosines, record):
    x = np.concatenate([cosines["c"], C.unary_specials()])
    got32 = host(P.run("acos_ps", dev(x)))
    got = got32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        ref = np.arccos(x.astype(np.float64))
        inside = np.abs(x) <= 1
    assert np.isnan(got[~inside]).all(), "acos_ps: |x| > 1 or NaN did not give NaN"
    assert (C.bits(got32[x == 1]) == 0).all() and (C.bits(got32[x == -1]) == C.bits([C.PI_F])[0]).all(), \
        "acos_ps(+-1) is not exactly 0 / fl(pi)"
    err = np.abs(got - ref)
    neg = np.signbit(x)
    worst_pos, worst_neg = float(err[inside & ~neg].max()), float(err[inside & neg].max())
    record["measured"]["acos_ps"] = {"positive_max_abs_err": worst_pos, "negative_max_abs_err": worst_neg,
                                     "positive_worst_at": float(x[inside & ~neg][np.argmax(err[inside & ~neg])]),
                                     "negative_worst_at": float(x[inside & neg][np.argmax(err[inside & neg])]),
                                     "points": int(inside.sum())}
    print(f"\nacos_ps: x >= 0 {worst_pos:.3e}, x < 0 {worst_neg:.3e}")
    assert worst_pos <= C.ACOS_POS_BOUND, f"acos_ps: {worst_pos:.3e} for x >= 0, derived bound {C.ACOS_POS_BOUND}"
    assert worst_neg <= C.ACOS_NEG_BOUND, f"acos_ps: {worst_neg:.3e} for x < 0, derived bound {C.ACOS_NEG_BOUND}"


# ---- 5. the faithful forms ARE the device library's ----
def library_note():
    return f" -- installed ROCm {P.rocm_version()}; {RESTATED}: if the library changed, restate it"


def test_atan2_lib_is_the_librarys_atan2f(probe, plane, division):
    ty, tx = (dev(t) for t in C.special_pairs())
    for name, y, x in (("plane", plane["dy"], plane["dx"]), ("division", division["da"], division["db"]), ("special table", ty, tx)):
        want = P.run("atan2f", y, x)
        for arm in ("atan2_lib", "atan2_lib_vn2", "atan2_lib_vn4"):
            assert_same_bits(P.run(arm, y, x), want, f"{arm} against atan2f on the {name} sample", y, x, note=library_note())


def test_acos_lib_is_the_librarys_acosf_on_every_float(probe):
    for chunk in range(-32, 32):
        x = torch.arange(chunk << 26, (chunk + 1) << 26, dtype=torch.int64, device="cuda").to(torch.int32).view(torch.float32)
        want = P.run("acosf", x)
        for arm in ("acos_lib", "acos_lib_vn2", "acos_lib_vn4"):
            assert_same_bits(P.run(arm, x), want, f"{arm} against acosf, bit patterns from {(chunk << 26) & 0xFFFFFFFF:#010x}", x,
                             note=library_note())


def test_faithful_forms_against_float64_in_ulps(probe, plane, cosines, record):
    y, x = plane["y"], plane["x"]
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    got = host(P.run("atan2_lib", plane["dy"], plane["dx"])).astype(np.float64)
    use = np.isfinite(y) & np.isfinite(x) & (np.abs(ref) >= 2.0 ** -100)
    ulps = C.ulps_of_f32(got[use] - ref[use], ref[use])
    ulp_atan2, worst = float(ulps.max()), int(np.argmax(ulps))
    c = cosines["c"]
    with np.errstate(invalid="ignore"):
        cref = np.arccos(c.astype(np.float64))
        cuse = (np.abs(c) <= 1) & (np.abs(cref) >= 2.0 ** -100)
    cgot = host(P.run("acos_lib", cosines["dc"])).astype(np.float64)
    culps = C.ulps_of_f32(cgot[cuse] - cref[cuse], cref[cuse])
    ulp_acos, cworst = float(culps.max()), int(np.argmax(culps))
    record["measured"]["atan2_lib"] = {"max_ulp_err": ulp_atan2, "max_abs_err": float(np.abs(got[use] - ref[use]).max()),
                                       "points": int(use.sum()), "worst_ulp_at_y_x": [float(y[use][worst]), float(x[use][worst])]}
    record["measured"]["acos_lib"] = {"max_ulp_err": ulp_acos, "max_abs_err": float(np.abs(cgot[cuse] - cref[cuse]).max()),
                                      "points": int(cuse.sum()), "worst_ulp_at": float(c[cuse][cworst])}
    print(f"\natan2_lib: {ulp_atan2:.3f} ulp, acos_lib: {ulp_acos:.3f} ulp")
    assert use.sum() > 3e6 and cuse.sum() > 2e6
    assert ulp_atan2 <= C.ATAN2_LIB_ULP_BOUND, f"atan2_lib is {ulp_atan2:.3f} ulp from float64"
    assert ulp_acos <= C.ACOS_LIB_ULP_BOUND, f"acos_lib is {ulp_acos:.3f} ulp from float64"
