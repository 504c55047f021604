"""GPU tests of the diffusion kernels (csrc/diffusion.hip: k5_diffuse, k54_diffuse_frames, k55_diffusion_trajectory) behind
ops.diffuse_, ops.diffuse_frames_ and ops.diffusion_trajectory_, against tests/diffusion_ref.py: the Philox4x32-10 noise
stream in float64, the strict float32 update, and a model of the launch geometry that the case tables are derived from
(tests/test_diffusion_host.py checks the yardstick itself, and that the tables reach the arms listed here).

The noise is read off the device with xyz = 0 and beta = 1: the update then returns eps itself, for a hand-set (seed, offset).

Arms and the table rows that reach them (diffusion_ref.launch_model):
    K5   one partial float4 group only                       (1, 1, 3)
         last workgroup: none / one partial / one full group  (2, 11, 31), (1, 683, 1), (4, 9, 19): 2046, 2049, 2052 coordinates
         span of 63 structures, and of exactly 64 (cached)    (200, 1, 11); (1100, 1, 11), workgroup 16
         span of 69 structures: beta_of's slow path           (200, 1, 10)      (65 to 68 cannot occur: nps is a multiple of 3)
         slow path, structure boundaries inside the groups    (700, 1, 3)
         plain cached case                                    (3, 7, 15)
    fused step and trajectory (128 residues per workgroup)
         128 structures per workgroup: slow path              (300, 1, 3)
         exactly 64 structures per workgroup                  (130, 2, 5)
         float4 arm of the trajectory                         (90, 3, 4), (33, 4, 15), (1, 129, 16)
         scalar arm                                           (300, 1, 3), (130, 2, 5), (3, 43, 15), (2, 5, 37)
         scalar arm through a 4-byte-offset out_xyz           the three float4 rows again
         partial last group (injected-noise tail)             (2, 5, 37)
    ticket protocol                                           grids of 1, 2, 31, 32, 33, 63, 64, 65 and 97 workgroups per kernel
    seed and offset words >= 2^32, offset crossing 2^32       SEEDS_OFFSETS; the trajectory from offset 2^32 - 2 with T = 4

Tolerance of the stream against the float64 reference.  The kernel evaluates log2, sqrt, sin and cos with the hardware
instructions; the bound is 4 x the largest error measured on an MI355X (the error is a smooth function of the two uniforms,
so the factor covers the draws not sampled), absolute and relative to max(1, |z|):
    max |eps - z| = 7.71e-7, max |eps - z| / max(1, |z|) = 3.13e-7 over 5 x 900 000 = 4.5e6 draws (> 2^22) spread over
    SEEDS_OFFSETS (test_stream_error_over_four_million_draws prints them); 1.80e-7 on the eight edge draws; 7.91e-7 and
    3.13e-7 over everything this file draws (the largest: offset 9 of seed 2024, in the ticket sweep).
    MEASURED_ABS = 7.92e-7 and MEASURED_REL = 3.14e-7 are those maxima; the bounds are 3.17e-6 and 1.26e-6, inside the
    ~1e-6-per-instruction error the kernel's own comment states and well under ten times it (1e-5).
A wrong stream misses by O(1) on 90 % of the draws (test_diffusion_host.py), five orders of magnitude above the bound.
Everything else is compared bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from tests import diffusion_ref as D

pytestmark = pytest.mark.gpu

MEASURED_ABS = 7.92e-7      # measured on an MI355X: see the docstring
MEASURED_REL = 3.14e-7
BOUND_ABS, BOUND_REL = 4 * MEASURED_ABS, 4 * MEASURED_REL

SLOTS = lambda A: [(0, 1, 2, 1), (A - 1, 0, 1, A - 1)]      # noqa: E731
SEED, OFFSET = 2024, 7


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import _lib, ops
    _lib.load()
    return ops


def gpu(x):
    return torch.from_numpy(np.array(x, order="C", copy=True)).cuda()      # a copy: the shared inputs are read-only


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(seed, offset, n_total):
    """noise64, computed once per draw and shared (never modified)."""
    z = D.noise64(seed, offset, n_total)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def coordinates(shape, salt=0):
    x = np.random.default_rng(77 + salt).standard_normal(shape + (3,)).astype(np.float32)
    x.setflags(write=False)
    return x


def new_state(ops, seed, offset):
    st = torch.zeros(ops.RNG_STATE_WORDS, dtype=torch.int64)
    st[0], st[1] = D.as_i64(seed), D.as_i64(offset)
    return st.cuda()


def check_state(st, seed, offset, where=""):
    """The seed untouched, the offset as an unsigned 64-bit value, every ticket word back at zero."""
    words = st.cpu()
    assert D.as_u64(words[0]) == D.as_u64(seed), where
    assert D.as_u64(words[1]) == D.as_u64(offset), f"{where}: offset {D.as_u64(words[1])}, expected {D.as_u64(offset)}"
    assert not words[2:].any(), f"{where}: ticket words left non-zero"


def stream_error(eps, seed, offset):
    """(max |eps - z|, max |eps - z| / max(1, |z|)) against the float64 reference of the same draw."""
    z = reference(seed, offset, eps.size)
    assert eps.dtype == np.float32 and np.isfinite(eps).all()
    d = np.abs(eps.reshape(-1).astype(np.float64) - z)
    return float(d.max()), float((d / np.maximum(1.0, np.abs(z))).max())


def assert_stream(eps, seed, offset, where):
    err_abs, err_rel = stream_error(eps, seed, offset)
    print(f"{where} seed {D.as_u64(seed):#x} offset {D.as_u64(offset):#x}: max abs {err_abs:.3e}  max rel {err_rel:.3e}")
    assert err_abs <= BOUND_ABS and err_rel <= BOUND_REL, f"{where}: stream off by {err_abs:.3e} abs, {err_rel:.3e} rel"
    assert np.abs(eps).max() <= D.Z_MAX + BOUND_ABS, "no draw lies outside |z| <= sqrt(50 ln 2)"


def extract(ops, shape, seed, offset, kind="k5"):
    """The device's own draw (seed, offset) for a (B, N, A, 3) buffer: xyz = 0, beta = 1 returns eps."""
    z = torch.zeros(shape + (3,), dtype=torch.float32, device="cuda")
    one = torch.ones(shape[0], dtype=torch.float32, device="cuda")
    st = new_state(ops, seed, offset)
    if kind == "k5":
        ops.diffuse_(z, one, st)
    elif kind == "fused":
        ops.diffuse_frames_(z, one, 0, 1, 2, 1, st)
    else:
        ops.diffusion_trajectory_(z, one[None], 0, 1, 2, 1, st, want_rot=False, want_trans=True)
    torch.cuda.synchronize()
    check_state(st, seed, D.as_u64(offset) + 1, f"{kind} {shape}")
    return host(z)


def same_bits(got, want, where):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (where, got.shape, want.shape)
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), f"{where}: {int(diff.sum())} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"


def betas(B, salt=0):
    return D.betas_for(B, salt)


def frames_of(ops, x, slots):
    rot, trans = ops.frames(gpu(x), *slots)
    return host(rot), host(trans)


# ---- the stream ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.K5_CASES, ids=str)
def test_k5_stream_matches_the_reference(ops, shape):
    for seed, offset in D.SEEDS_OFFSETS:
        assert_stream(extract(ops, shape, seed, offset), seed, offset, f"k5 {shape}")


@pytest.mark.parametrize("kind", ["fused", "trajectory"])
@pytest.mark.parametrize("shape", D.FUSED_CASES, ids=str)
def test_fused_and_trajectory_draw_the_same_stream(ops, shape, kind):
    for seed, offset in D.SEEDS_OFFSETS:
        eps = extract(ops, shape, seed, offset, kind)
        assert_stream(eps, seed, offset, f"{kind} {shape}")
        same_bits(eps, extract(ops, shape, seed, offset), f"{kind} {shape} against k5")


def test_edge_draws(ops):
    """The eight draws whose uniform is exactly 1.0 or 2^-25 (diffusion_ref.EDGE_DRAWS), at B = 1, N = 1, A = 3."""
    worst_abs = worst_rel = 0.0
    for word, off_one, off_zero in D.EDGE_DRAWS:
        pair = slice(0, 2) if word < 2 else slice(2, 4)
        for offset, top in ((off_one, True), (off_zero, False)):
            eps = extract(ops, (1, 1, 3), D.EDGE_SEED, offset).reshape(-1)
            assert_stream(eps, D.EDGE_SEED, offset, f"edge word {word} {'1.0' if top else '2^-25'}")
            e_abs, e_rel = stream_error(eps, D.EDGE_SEED, offset)
            worst_abs, worst_rel = max(worst_abs, e_abs), max(worst_rel, e_rel)
            if word in (0, 2) and top:
                assert np.all(eps[pair] == 0.0), "a radius word of 1.0 gives zero"
            if word in (0, 2) and not top:
                r = float(np.hypot(*eps[pair].astype(np.float64)))
                assert abs(r - D.Z_MAX) <= 2 * BOUND_ABS and np.abs(eps[pair]).max() <= D.Z_MAX + BOUND_ABS
    print(f"edge draws: max abs {worst_abs:.3e}  max rel {worst_rel:.3e}")


def test_stream_error_over_four_million_draws(ops):
    """The figures of the module docstring: 900 000 draws for each of the five (seed, offset) pairs."""
    shape, worst_abs, worst_rel = (4, 1000, 75), 0.0, 0.0
    for seed, offset in D.SEEDS_OFFSETS:
        eps = extract(ops, shape, seed, offset)
        e_abs, e_rel = stream_error(eps, seed, offset)
        print(f"seed {D.as_u64(seed):#x} offset {D.as_u64(offset):#x}: {eps.size} draws  max abs {e_abs:.4e}  max rel {e_rel:.4e}")
        worst_abs, worst_rel = max(worst_abs, e_abs), max(worst_rel, e_rel)
    n = 3 * shape[0] * shape[1] * shape[2] * len(D.SEEDS_OFFSETS)
    print(f"stream error over {n} draws: max abs {worst_abs:.4e}  max rel {worst_rel:.4e}  "
          f"(bounds {BOUND_ABS:.2e}, {BOUND_REL:.2e})")
    assert n >= 2 ** 22
    assert worst_abs <= BOUND_ABS and worst_rel <= BOUND_REL


# ---- the update, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.K5_CASES, ids=str)
def test_k5_update_is_the_unfused_float32_step(ops, shape):
    B = shape[0]
    x, beta = coordinates(shape), betas(B)
    eps = extract(ops, shape, SEED, OFFSET)
    want = D.step_f32(x, D.per_structure(beta), eps)
    if B >= 3:
        same_bits(want[B // 3], x[B // 3], "beta = 0 keeps the coordinates")
        same_bits(want[2 * B // 3], eps[2 * B // 3], "beta = 1 returns the noise")
    a, st = gpu(x), new_state(ops, SEED, OFFSET)
    ops.diffuse_(a, gpu(beta), st)
    b = gpu(x)
    ops.diffuse_(b, gpu(beta), None, gpu(eps))
    torch.cuda.synchronize()
    check_state(st, SEED, OFFSET + 1, f"k5 {shape}")
    same_bits(host(a), want, f"k5 {shape} sampler")
    same_bits(host(b), want, f"k5 {shape} injected noise")


@pytest.mark.parametrize("shape", D.FUSED_CASES, ids=str)
def test_fused_step_update_and_frames(ops, shape):
    B, N, A = shape
    x, beta = coordinates(shape), betas(B)
    eps = extract(ops, shape, SEED, OFFSET)
    want = D.step_f32(x, D.per_structure(beta), eps)
    for slots in SLOTS(A):
        want_rot, want_trans = frames_of(ops, want, slots)
        a, st = gpu(x), new_state(ops, SEED, OFFSET)
        rot_a, trans_a = ops.diffuse_frames_(a, gpu(beta), *slots, st)
        b = gpu(x)
        rot_b, trans_b = ops.diffuse_frames_(b, gpu(beta), *slots, None, gpu(eps))
        torch.cuda.synchronize()
        check_state(st, SEED, OFFSET + 1, f"fused {shape}")
        for tag, c, rot, trans in (("sampler", a, rot_a, trans_a), ("injected noise", b, rot_b, trans_b)):
            where = f"fused {shape} slots {slots} {tag}"
            same_bits(host(c), want, where + ": xyz")
            same_bits(host(rot), want_rot, where + ": rot")
            same_bits(host(trans), want_trans, where + ": trans")


def reference_steps(ops, shape, bt, seed, offset, x):
    """x_1 ... x_T by step_f32 with the device's draws offset, offset + 1, ... (each checked against noise64)."""
    out = []
    for t in range(bt.shape[0]):
        eps = extract(ops, shape, seed, D.as_u64(offset) + t)
        assert_stream(eps, seed, D.as_u64(offset) + t, f"draw {t} of {shape}")
        x = D.step_f32(x, D.per_structure(bt[t]), eps)
        out.append(x)
    return out


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("shape", D.FUSED_CASES, ids=str)
def test_trajectory_equals_reference_steps(ops, shape, T):
    B, N, A = shape
    bt = np.stack([betas(B, salt=t + 1) for t in range(T)])
    if B >= 2:
        assert not np.array_equal(bt[0], bt[-1]) or T == 1
    xs = reference_steps(ops, shape, bt, SEED, OFFSET, coordinates(shape))
    for slots in SLOTS(A):
        fr = [frames_of(ops, x, slots) for x in xs]
        want_rot, want_trans = np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])
        for wants in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
            a, st = gpu(coordinates(shape)), new_state(ops, SEED, OFFSET)
            rot, trans, traj = ops.diffusion_trajectory_(a, gpu(bt), *slots, st, *wants)
            torch.cuda.synchronize()
            where = f"trajectory {shape} T {T} slots {slots} wants {wants}"
            check_state(st, SEED, OFFSET + T, where)
            same_bits(host(a), xs[-1], where + ": xyz")
            assert (rot is not None, trans is not None, traj is not None) == wants
            if rot is not None:
                same_bits(host(rot), want_rot, where + ": rot")
            if trans is not None:
                same_bits(host(trans), want_trans, where + ": trans")
            if traj is not None:
                for t in range(T):
                    same_bits(host(traj[t]), xs[t], where + f": out_xyz[{t}]")


@pytest.mark.parametrize("shape", D.vec4_cases(), ids=str)
def test_trajectory_out_xyz_four_bytes_off_alignment(ops, shape):
    """An out_xyz that starts 4 bytes past a 16-byte boundary sends the float4 rows down the scalar arm: the same bits as
    the aligned run, and nothing written outside the view."""
    B, N, A = shape
    T, n = 2, 3 * B * N * A
    bt = np.stack([betas(B, salt=t + 1) for t in range(T)])
    a, st = gpu(coordinates(shape)), new_state(ops, SEED, OFFSET)
    rot_a, trans_a, traj_a = ops.diffusion_trajectory_(a, gpu(bt), 0, 1, 2, 1, st, want_xyz=True)
    assert traj_a.data_ptr() % 16 == 0
    sentinel = -12345.5
    storage = torch.full((T * n + 16,), sentinel, dtype=torch.float32, device="cuda")
    assert storage.data_ptr() % 16 == 0
    view = storage[1:1 + T * n].view(T, B, N, A, 3)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    b, st_b = gpu(coordinates(shape)), new_state(ops, SEED, OFFSET)
    rot_b, trans_b, traj_b = ops.diffusion_trajectory_(b, gpu(bt), 0, 1, 2, 1, st_b, out_xyz=view)
    torch.cuda.synchronize()
    assert traj_b.data_ptr() == view.data_ptr()
    check_state(st_b, SEED, OFFSET + T, f"misaligned {shape}")
    for got, want, what in ((b, a, "xyz"), (view, traj_a, "out_xyz"), (rot_b, rot_a, "rot"), (trans_b, trans_a, "trans")):
        same_bits(host(got), host(want), f"misaligned out_xyz {shape}: {what}")
    outside = torch.cat([storage[:1], storage[1 + T * n:]])
    assert bool((outside == sentinel).all()), "a sentinel around out_xyz changed"
    assert not bool((view == sentinel).any())


@pytest.mark.parametrize("shape", [(33, 4, 15), (2, 5, 37)], ids=str)
def test_trajectory_across_the_32_bit_offset_boundary(ops, shape):
    T, offset = 4, 2 ** 32 - 2
    bt = np.stack([betas(shape[0], salt=t + 1) for t in range(T)])
    xs = reference_steps(ops, shape, bt, SEED, offset, coordinates(shape))
    a, st = gpu(coordinates(shape)), new_state(ops, SEED, offset)
    _, _, traj = ops.diffusion_trajectory_(a, gpu(bt), 0, 1, 2, 1, st, want_xyz=True)
    torch.cuda.synchronize()
    check_state(st, SEED, 2 ** 32 + 2, f"trajectory {shape}")
    for t in range(T):
        same_bits(host(traj[t]), xs[t], f"step {t} (offset {offset + t:#x})")
    same_bits(host(a), xs[-1], "xyz")


# ---- the ticket protocol -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["k5", "fused", "trajectory"])
@pytest.mark.parametrize("grid", D.TICKET_GRIDS)
def test_ticket_protocol_at_every_grid_edge(ops, grid, kind):
    """Three launches back to back on one state, no synchronisation in between: launch k draws offset k (k T ... for the
    trajectory), the counter ends 3 (3 T) further with every ticket word at zero.  The noise of each offset comes from
    one isolated launch per offset, as in test_gpu_parity.py::test_k5_back_to_back_launches_draw_consecutive_offsets."""
    shape = D.ticket_shape(kind, grid)
    assert D.launch_model(kind, *shape).grid == grid
    B, T, start = shape[0], (2 if kind == "trajectory" else 1), 5
    bt = np.stack([betas(B, salt=k + 1) for k in range(3 * T)])
    want = reference_steps(ops, shape, bt, SEED, start, coordinates(shape))
    a, st = gpu(coordinates(shape)), new_state(ops, SEED, start)
    dev_bt = gpu(bt)
    for k in range(3):
        if kind == "k5":
            ops.diffuse_(a, dev_bt[k], st)
        elif kind == "fused":
            ops.diffuse_frames_(a, dev_bt[k], 0, 1, 2, 1, st)
        else:
            ops.diffusion_trajectory_(a, dev_bt[k * T:(k + 1) * T], 0, 1, 2, 1, st)
    torch.cuda.synchronize()
    check_state(st, SEED, start + 3 * T, f"{kind} grid {grid}")
    same_bits(host(a), want[-1], f"{kind} grid {grid}: a launch drew with another offset than its own")
