"""Host-side checks of the diffusion yardstick (tests/diffusion_ref.py): the published Philox4x32-10 known-answer vectors,
the float32 uniform and its two edge values, the edge draws the GPU test reuses, that the tolerance of the GPU test tells
a wrong stream from the right one (perturbed copies of the reference, never of a kernel), and that the case tables of
tests/test_gpu_diffusion.py reach every arm of the kernels according to the launch model.  No GPU needed."""
import numpy as np
import pytest

from tests import diffusion_ref as D


def words(*hex_words):
    return [int(h, 16) for h in hex_words]


# ---- Philox --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    (words("0", "0", "0", "0"), words("0", "0"), words("6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8")),
    (words("ffffffff", "ffffffff", "ffffffff", "ffffffff"), words("ffffffff", "ffffffff"),
     words("408f276d", "41c83b0e", "a20bc7c6", "6d5451fd")),
    (words("243f6a88", "85a308d3", "13198a2e", "03707344"), words("a4093822", "299f31d0"),
     words("d16cfe09", "94fdcceb", "5001e420", "24126ea1")),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    """The three philox4x32-10 vectors of Random123's kat_vectors."""
    got = D.philox4x32_10(counter, key)
    assert got.shape == (4, 1) and got.dtype == np.uint64
    assert [int(w) for w in got[:, 0]] == want


def test_philox_is_vectorised_and_counter_layout():
    """An array of counters gives, per column, what the scalar call gives; group and offset land in the words the
    docstring names, high halves included."""
    g = np.array([0, 1, 5, 2 ** 32 + 3], dtype=np.uint64)
    seed, offset = 0xA4093822_00000007, 2 ** 40 + 1
    all_at_once = D.philox4x32_10(*D.counter_and_key(seed, offset, g))
    for col, group in enumerate(g.tolist()):
        one = D.philox4x32_10((group & 0xFFFFFFFF, group >> 32, offset & 0xFFFFFFFF, offset >> 32),
                              (seed & 0xFFFFFFFF, seed >> 32))
        assert all_at_once[:, col].tolist() == one[:, 0].tolist()
    assert np.array_equal(D.stream_words(seed, offset, 3, first_group=4)[:, 1], all_at_once[:, 2])
    # int64 words are taken by their bit pattern
    assert D.as_u64(-1) == 2 ** 64 - 1 and D.as_i64(2 ** 64 - 1) == -1 and D.as_i64(2 ** 63) == -2 ** 63
    assert np.array_equal(D.stream_words(-1, -2, 2), D.stream_words(2 ** 64 - 1, 2 ** 64 - 2, 2))


# ---- the uniform ---------------------------------------------------------------------------------------------------------
def test_uniform_edges_in_float32():
    top, zero = (2 ** 24 - 1) << 8, 0
    u = D.u01_f32(np.array([top, top | 0xFF, zero, 0xFF, (2 ** 23 - 1) << 8, (2 ** 23) << 8, (2 ** 23 + 1) << 8],
                           dtype=np.uint64))
    assert u.dtype == np.float32
    assert u[0] == 1.0 and u[1] == 1.0, "fl(2^24 - 1 + 0.5) ties to even: 2^24"
    assert u[2] == np.float32(2.0 ** -25) and u[3] == u[2]
    assert u[4] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24), "exact below 2^23"
    assert u[5] == np.float32(0.5) and u[6] == np.float32((2 ** 23 + 2) * 2.0 ** -24), "ties to even above"
    # the whole grid lies in [2^-25, 1]
    m = np.arange(0, 2 ** 24, 4093, dtype=np.uint64) << np.uint64(8)
    uu = D.u01_f32(m)
    assert uu.min() == np.float32(2.0 ** -25) and uu.max() <= 1.0 and np.all(np.diff(uu) >= 0)
    assert D.Z_MAX == pytest.approx(5.887050112577373, abs=1e-12)
    assert float(D.radius64(np.float32(2.0 ** -25))) == pytest.approx(D.Z_MAX, abs=1e-14)
    r_one = D.radius64(np.float32(1.0))
    assert r_one == 0.0 and not np.signbit(r_one)


def test_edge_draws_are_what_the_search_found():
    """Seed 2024, group 0: at the listed offsets word k is all-ones / all-zeros in its upper 24 bits, the uniform is
    exactly 1.0 / 2^-25, and noise64 stays finite with the values the formulas give there."""
    for word, off_one, off_zero in D.EDGE_DRAWS:
        w_one, w_zero = D.stream_words(D.EDGE_SEED, off_one, 1)[:, 0], D.stream_words(D.EDGE_SEED, off_zero, 1)[:, 0]
        assert int(w_one[word]) >> 8 == 2 ** 24 - 1 and D.u01_f32(w_one[word]) == 1.0
        assert int(w_zero[word]) >> 8 == 0 and D.u01_f32(w_zero[word]) == np.float32(2.0 ** -25)
        z_one, z_zero = D.noise64(D.EDGE_SEED, off_one, 4), D.noise64(D.EDGE_SEED, off_zero, 4)
        assert np.isfinite(z_one).all() and np.isfinite(z_zero).all()
        assert np.abs(z_one).max() <= D.Z_MAX and np.abs(z_zero).max() <= D.Z_MAX
        pair = slice(0, 2) if word < 2 else slice(2, 4)
        if word in (0, 2):      # radius words
            assert np.all(z_one[pair] == 0.0), "a radius word of 1.0 gives z = 0"
            assert np.hypot(*z_zero[pair]) == pytest.approx(D.Z_MAX, abs=1e-12), "a radius word of 2^-25: the largest |z|"
        else:                   # angle words: 1.0 is one whole revolution, 2^-25 a 1.9e-7 rad turn
            r = np.hypot(*z_one[pair])
            assert z_one[pair][0] == pytest.approx(r, abs=1e-12) and abs(z_one[pair][1]) <= 1e-12
            r = np.hypot(*z_zero[pair])
            assert z_zero[pair][0] == pytest.approx(r, abs=1e-12)
            assert z_zero[pair][1] == pytest.approx(r * 2 * np.pi * 2.0 ** -25, rel=1e-9)


def test_noise64_layout_and_finiteness():
    n = 10 ** 5 + 3
    z = D.noise64(2024, 7, n)
    assert z.shape == (n,) and z.dtype == np.float64 and np.isfinite(z).all() and np.abs(z).max() <= D.Z_MAX
    assert np.array_equal(z[:1001], D.noise64(2024, 7, 1001)), "a shorter buffer is a prefix"
    w = D.stream_words(2024, 7, 2)
    u = D.u01_f32(w).astype(np.float64)
    assert z[5] == np.sqrt(-2 * np.log(u[0, 1])) * np.sin(2 * np.pi * u[1, 1])
    assert z[6] == np.sqrt(-2 * np.log(u[2, 1])) * np.cos(2 * np.pi * u[3, 1])
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)


# ---- what the GPU test's tolerance tells apart -----------------------------------------------------------------------------
def _perturbed(name, seed, offset, n):
    groups = np.arange((n + 3) // 4, dtype=np.uint64)
    counter, key = D.counter_and_key(seed, offset, groups)
    if name == "nine rounds":
        w = D.philox4x32_10(counter, key, rounds=9)
    elif name == "counter words swapped":
        w = D.philox4x32_10((counter[2], counter[3], counter[0], counter[1]), key)
    elif name == "offset + 1":
        w = D.stream_words(seed, offset + 1, groups.size)
    elif name == "high key word ignored":
        w = D.philox4x32_10(counter, (key[0], np.uint64(0)))
    else:
        w = D.philox4x32_10(counter, key)
    z = D.normals64(w)
    if name == "sin and cos exchanged":
        z = z[:, [1, 0, 3, 2]]
    elif name == "w2 and w3 paired with the first radius":
        u = D.u01_f32(w).astype(np.float64)
        r0 = D.radius64(u[0])
        z = np.stack([z[:, 0], z[:, 1], r0 * np.cos(2 * np.pi * u[3]), r0 * np.sin(2 * np.pi * u[3])], axis=1)
    return z.reshape(-1)[:n]


@pytest.mark.parametrize("name", ["nine rounds", "counter words swapped", "offset + 1", "high key word ignored",
                                  "sin and cos exchanged", "w2 and w3 paired with the first radius"])
def test_a_wrong_stream_misses_by_far_more_than_the_tolerance(name):
    """Each mistake the GPU comparison is meant to catch moves at least 90 % of 10^5 draws by more than 1e-2 -- three
    orders of magnitude above any bound tests/test_gpu_diffusion.py asserts.  (The last one leaves z0, z1 alone: half
    of the draws; it is measured on the other half.)"""
    n = 10 ** 5
    seed, offset = 0x243F6A8885A308D3, 2 ** 40 + 1      # both high words in use
    right, wrong = D.noise64(seed, offset, n), _perturbed(name, seed, offset, n)
    assert np.array_equal(right, _perturbed("none", seed, offset, n))
    moved = np.abs(wrong - right) > 1e-2
    if name == "w2 and w3 paired with the first radius":
        assert not moved.reshape(-1, 4)[:, :2].any()
        moved = moved.reshape(-1, 4)[:, 2:]
    assert moved.mean() >= 0.9, f"{name}: only {moved.mean():.3f} of the draws moved"


# ---- the update ------------------------------------------------------------------------------------------------------------
def test_step_f32_is_the_unfused_float32_update():
    rng = np.random.default_rng(3)
    x, eps = rng.standard_normal((3, 2, 5, 3)).astype(np.float32), rng.standard_normal((3, 2, 5, 3)).astype(np.float32)
    beta = D.betas_for(3)
    assert beta[1] == 0.0 and beta[2] == 1.0
    out = D.step_f32(x, D.per_structure(beta), eps)
    assert out.dtype == np.float32
    assert np.array_equal(out[1], x[1]), "beta = 0 returns the coordinates"
    assert np.array_equal(out[2], eps[2]), "beta = 1 returns the noise"
    b = float(beta[0])
    keep, add = np.float32(np.sqrt(np.float64(np.float32(1) - np.float32(b)))), np.float32(np.sqrt(np.float64(b)))
    want = np.float32(np.float64(keep) * np.float64(x[0, 1, 2, 1])) + np.float32(np.float64(eps[0, 1, 2, 1]) * np.float64(add))
    assert out[0, 1, 2, 1] == np.float32(want)
    assert np.array_equal(D.step_f32(np.zeros_like(x), D.per_structure(np.ones(3)), eps), eps)
    for B in (1, 2, 3, 200, 1100):
        bt = D.betas_for(B)
        assert bt.dtype == np.float32 and len(set(bt.tolist())) == B and bt.min() >= 0 and bt.max() <= 1


# ---- the case tables ---------------------------------------------------------------------------------------------------------
def test_launch_model_on_hand_computed_cases():
    m = D.launch_model("k5", 1, 1, 3)
    assert (m.n_total, m.nps, m.grid) == (9, 9, 1) and m.workgroups[0] == D.Workgroup(0, 9, 1, True, True, None)
    m = D.launch_model("k5", 200, 1, 10)        # 30 per structure: 2048 = 68 * 30 + 8
    assert m.grid == 3 and [w.n_span for w in m.workgroups] == [69, 69, 64]
    assert [w.cached for w in m.workgroups] == [False, False, True]
    m = D.launch_model("trajectory", 256, 384, 15)      # the benchmark's shape: 768 workgroups, all float4
    assert m.grid == 768 and all(w.vec4 and w.n_span == 1 for w in m.workgroups)
    assert not any(w.vec4 for w in D.launch_model("trajectory", 256, 384, 15, out_xyz_aligned=False).workgroups)
    m = D.launch_model("fused", 300, 1, 3)
    assert m.grid == 3 and [w.n_span for w in m.workgroups] == [128, 128, 44] and m.workgroups[0].vec4 is None
    assert [w.length for w in m.workgroups] == [1152, 1152, 396]


def test_case_tables_reach_every_arm():
    """Every arm named in tests/test_gpu_diffusion.py's docstring is reached by a row of its tables, by the launch model
    of the kernels' constants.  If this fails after a kernel constant changed, derive the tables again."""
    k5 = {s: D.launch_model("k5", *s) for s in D.K5_CASES}
    spans = {s: [w.n_span for w in m.workgroups] for s, m in k5.items()}
    assert k5[(1, 1, 3)].grid == 1 and k5[(1, 1, 3)].n_total == 9 and k5[(1, 1, 3)].workgroups[0].partial_group
    assert [k5[s].n_total for s in [(2, 11, 31), (1, 683, 1), (4, 9, 19)]] == [2046, 2049, 2052]
    assert k5[(2, 11, 31)].grid == 1 and k5[(2, 11, 31)].workgroups[0].partial_group
    last = k5[(1, 683, 1)].workgroups[-1]
    assert k5[(1, 683, 1)].grid == 2 and last.length == 1 and last.partial_group
    last = k5[(4, 9, 19)].workgroups[-1]
    assert k5[(4, 9, 19)].grid == 2 and last.length == 4 and not last.partial_group
    assert k5[(200, 1, 11)].nps == 33 and spans[(200, 1, 11)][:-1] == [63, 63, 63]
    assert spans[(1100, 1, 11)][16] == 64 and max(spans[(1100, 1, 11)]) == 64, "the cache limit itself"
    assert all(w.cached for s in [(200, 1, 11), (1100, 1, 11), (3, 7, 15)] for w in k5[s].workgroups)
    assert k5[(200, 1, 10)].nps == 30 and set(spans[(200, 1, 10)][:-1]) == {69}
    big = D.launch_model("k5", 1100, 1, 10)
    assert {w.n_span for w in big.workgroups[:-1]} == {69, 70}, "30 per structure: 69 or 70, never 65 to 68"
    assert not any(w.cached for w in k5[(200, 1, 10)].workgroups[:-1])
    assert k5[(700, 1, 3)].nps == 9 and not any(w.cached for w in k5[(700, 1, 3)].workgroups[:-1])
    assert k5[(700, 1, 3)].nps % 4 != 0 and k5[(700, 1, 3)].grid == 4
    assert k5[(3, 7, 15)].grid == 1 and spans[(3, 7, 15)] == [3]

    for kind in ("fused", "trajectory"):
        f = {s: D.launch_model(kind, *s) for s in D.FUSED_CASES}
        sp = {s: [w.n_span for w in m.workgroups] for s, m in f.items()}
        assert sp[(300, 1, 3)] == [128, 128, 44] and [w.cached for w in f[(300, 1, 3)].workgroups] == [False, False, True]
        assert sp[(130, 2, 5)] == [64, 64, 2] and all(w.cached for w in f[(130, 2, 5)].workgroups)
        assert set(sp[(90, 3, 4)]) <= {43, 44, 5} and sp[(90, 3, 4)][:2] in ([43, 44], [44, 43], [43, 43], [44, 44])
        assert any(w.begin % f[(90, 3, 4)].nps for w in f[(90, 3, 4)].workgroups), "boundaries off the workgroup edges"
        assert f[(33, 4, 15)].grid == 2 and f[(33, 4, 15)].workgroups[1].length == 4 * 45
        assert f[(3, 43, 15)].grid == 2 and f[(3, 43, 15)].workgroups[1].length == 45
        assert f[(2, 5, 37)].n_total % 4 != 0 and f[(2, 5, 37)].workgroups[-1].partial_group
        assert f[(1, 129, 16)].grid == 2 and sp[(1, 129, 16)] == [1, 1]
    t = {s: D.launch_model("trajectory", *s) for s in D.FUSED_CASES}
    vec4_rows = [s for s in D.FUSED_CASES if all(w.vec4 for w in t[s].workgroups)]
    assert vec4_rows == [(90, 3, 4), (33, 4, 15), (1, 129, 16)] == D.vec4_cases()
    assert all(not w.vec4 for s in D.FUSED_CASES if s not in vec4_rows for w in t[s].workgroups)
    for s in vec4_rows:         # a 4-byte-offset out_xyz sends every one of them down the scalar arm
        assert not any(w.vec4 for w in D.launch_model("trajectory", *s, out_xyz_aligned=False).workgroups)

    for grid in D.TICKET_GRIDS:
        B, N, A = D.ticket_shape("k5", grid)
        m = D.launch_model("k5", B, N, A)
        assert m.grid == grid and 2048 * (grid - 1) < m.n_total <= 2048 * grid
        for kind in ("fused", "trajectory"):
            B, N, A = D.ticket_shape(kind, grid)
            assert D.launch_model(kind, B, N, A).grid == grid and B * N == 128 * (grid - 1) + 1 and A == 3
    assert {1, 31, 32, 33, 63, 64, 65} <= set(D.TICKET_GRIDS)
    # every buffer is small: the largest of all tables is a few hundred thousand floats
    shapes = D.K5_CASES + D.FUSED_CASES + [D.ticket_shape(k, g) for k in ("k5", "fused") for g in D.TICKET_GRIDS]
    assert max(3 * B * N * A for B, N, A in shapes) < 2 ** 18


def test_seed_and_offset_list_uses_the_high_words():
    assert D.SEEDS_OFFSETS[:2] == [(0, 0), (2024, 7)]
    assert any(D.as_u64(s) >> 32 and not D.as_u64(o) >> 32 for s, o in D.SEEDS_OFFSETS)
    assert any(D.as_u64(o) >> 32 for s, o in D.SEEDS_OFFSETS)
    assert (-1, 2 ** 32 - 1) in D.SEEDS_OFFSETS, "offset + 1 carries into the high word"
    for seed, offset in D.SEEDS_OFFSETS:        # every one fits the int64 words of rng_state
        assert -2 ** 63 <= D.as_i64(seed) < 2 ** 63 and D.as_u64(D.as_i64(seed)) == D.as_u64(seed)
        assert 0 <= offset < 2 ** 63
