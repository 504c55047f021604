"""Closest-atom residue distances on the GPU (K31 / K32) against tests/closest_ref.py, the float64 restatement of their
definition.  Forward results are tested for EQUALITY -- the bits of ``dist``, every ``pair`` --; the gradient against the
derived bound below; and, since include/protstruc_contacts.h is not in the case table of tests/launch_cases.py, this file
also holds the two launchers to the launch contract: the caller's stream, capture, four threads, the batch limit."""
import functools
import math
import os
import threading

import numpy as np
import pytest
import torch

from tests import closest_ref as R
from tests.launch_cases import Case, on_device
from tests.test_gpu_launch_contract import (SENTINEL, SLEEP_CYCLES, assert_all_same, assert_batch_of_65535_repeats_the_three,
                                            raw, same, side_stream_beside_the_default_stream)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
INF = math.inf
SHAPES = ((1, 1), (2, 2), (63, 4), (64, 15), (65, 15), (129, 15), (130, 25))   # lane, wave and tile edges; 129: a mirrored tile
CUTOFFS = (INF, 8.0, 5.0, 0.0)
PDB_FILES = ("1a3r_HL", "1REX", "15c8_HL", "1a6v_HL")


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def chain(N, A):
    return R.chain_case(N, A, seed=100 + N)


@functools.lru_cache(maxsize=None)
def chain_reference(N, A, cutoff):
    """computed once per case and never modified"""
    return R.forward(*chain(N, A), cutoff)


def assert_equal_to_yardstick(got, want, what):
    dist, pair = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert dist.dtype == np.float32 and pair.dtype == np.int16 and dist.shape == want[0].shape == pair.shape, what
    wrong = np.flatnonzero(dist.view(np.int32).ravel() != want[0].view(np.int32).ravel())
    assert wrong.size == 0, (f"{what}: {wrong.size} dist differ in their bits, the first at {np.unravel_index(wrong[0], dist.shape)}: "
                             f"{dist.ravel()[wrong[0]]!r} for {want[0].ravel()[wrong[0]]!r}")
    wrong = np.flatnonzero(pair.ravel() != want[1].ravel())
    assert wrong.size == 0, (f"{what}: {wrong.size} pair differ, the first at {np.unravel_index(wrong[0], pair.shape)}: "
                             f"{pair.ravel()[wrong[0]]} for {want[1].ravel()[wrong[0]]}")


# ---- forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("N,A", SHAPES)
def test_synthetic_chains(pkg, N, A, cutoff):
    xyz, mask = chain(N, A)
    assert np.isnan(xyz[~mask]).all() and (N == 1 or (~mask.any(-1)).any(-1).all())
    want = chain_reference(N, A, cutoff)
    got = pkg.ops.closest_atoms(dev(xyz), dev(mask), cutoff)
    assert_equal_to_yardstick(got, want, f"N={N} A={A} cutoff={cutoff}")
    if N >= 63 and cutoff == 5.0:
        far = np.isinf(want[0]).mean()
        assert 0.5 < far < 1.0, f"the cutoff is meant to exclude most pairs and keep some ({far:.2f} excluded)"


@pytest.mark.parametrize("cutoff", (5.0, INF))
def test_integer_lattice_full_of_ties(pkg, cutoff):
    xyz, mask = R.lattice_case(70, 4)
    want = R.forward(xyz, mask, cutoff)
    free = R.forward(xyz, mask)[0]
    assert (free == np.float32(5.0)).sum() >= 20 and (free == np.float32(np.sqrt(26.0))).sum() >= 20
    assert_equal_to_yardstick(pkg.ops.closest_atoms(dev(xyz), dev(mask), cutoff), want, f"lattice, cutoff={cutoff}")
    # no mask: the slots that were masked now take part, and win
    assert_equal_to_yardstick(pkg.ops.closest_atoms(dev(xyz), None, cutoff), R.forward(xyz, None, cutoff), "lattice, no mask")


@pytest.mark.parametrize("N,A", ((70, 33), (45, 64)))
def test_more_than_32_atom_slots(pkg, N, A):
    """above 32 slots the forward kernel runs with tiles of 32 residues, and above 28 the backward kernel with 32 owners"""
    xyz, mask = chain(N, A)
    for cutoff in (INF, 5.0):
        want = chain_reference(N, A, cutoff)
        assert_equal_to_yardstick(pkg.ops.closest_atoms(dev(xyz), dev(mask), cutoff), want, f"N={N} A={A} cutoff={cutoff}")
    g = random_grad(want[1].shape, A)
    got = pkg.ops.closest_atoms_backward(dev(xyz), dev(want[1]), dev(g))
    assert_gradient_within_the_bound(got, xyz, want[1], g, f"N={N} A={A}")


def carve(n_bytes, offset, dtype):
    """(buffer, view): a sentinel-filled byte buffer and ``n_bytes`` of it as ``dtype``, starting ``offset`` bytes past a
    16-byte boundary with at least 32 bytes of sentinels on either side"""
    buf = torch.full((n_bytes + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
    start = 32 + (-(buf.data_ptr() + 32)) % 16 + offset
    view = buf[start:start + n_bytes].view(dtype)
    assert view.data_ptr() % 16 == offset
    return buf, view, start


@pytest.mark.parametrize("dist_off,pair_off", ((4, 2), (8, 6), (12, 14), (4, 4), (8, 8), (12, 12), (0, 0)))
def test_sentinels_and_alignment(pkg, dist_off, pair_off):
    from protstruc_amd import _lib
    N, A, B = 67, 4, 2
    xyz, mask = (t[:B] for t in R.chain_case(N, A, seed=7))
    want = R.forward(xyz, mask, 8.0)
    _, x, _ = carve(xyz.nbytes, 4, torch.float32)
    x.copy_(dev(xyz).reshape(-1))
    m = dev(mask)
    dbuf, d, dstart = carve(B * N * N * 4, dist_off, torch.float32)
    pbuf, p, pstart = carve(B * N * N * 2, pair_off, torch.int16)
    rc = _lib.load().ps_closest_atoms_f32(x.data_ptr(), m.data_ptr(), d.data_ptr(), p.data_ptr(), B, N, A, 8.0,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert_equal_to_yardstick((d.reshape(B, N, N), p.reshape(B, N, N)), want, f"dist {dist_off} and pair {pair_off} bytes off")
    for buf, start, n in ((dbuf, dstart, B * N * N * 4), (pbuf, pstart, B * N * N * 2)):
        assert bool((buf[:start] == SENTINEL).all()) and bool((buf[start + n:] == SENTINEL).all()), "a sentinel was overwritten"
    # the backward pass with xyz 4 bytes off and its output 4, 8 or 12
    g = torch.randn(B, N, N, device="cuda")
    gbuf, gx, gstart = carve(xyz.nbytes, dist_off, torch.float32)
    rc = _lib.load().ps_closest_atoms_backward_f32(x.data_ptr(), p.data_ptr(), g.data_ptr(), gx.data_ptr(), B, N, A,
                                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((gbuf[:gstart] == SENTINEL).all()) and bool((gbuf[gstart + xyz.nbytes:] == SENTINEL).all())
    assert same(gx.reshape(B, N, A, 3), pkg.ops.closest_atoms_backward(dev(xyz), dev(want[1]), g))


# ---- the PDB files -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pdb_batch():
    from protstruc_amd import StructureBatch
    return StructureBatch.from_pdb([os.path.join(GOLDEN_DIR, name + ".pdb") for name in PDB_FILES])


@functools.lru_cache(maxsize=None)
def pdb_reference(cutoff):
    batch = pdb_batch()
    return R.forward(batch.get_xyz().cpu().numpy(), batch._present_atoms().cpu().numpy(), cutoff)


@pytest.mark.parametrize("cutoff", (INF, 5.0))
def test_pdb_files(pkg, cutoff):
    batch = pdb_batch()
    assert batch.get_xyz().isnan().any(), "from_pdb stores NaN for missing atoms: the case is meant to carry them"
    A = batch.get_xyz().shape[2]
    want = pdb_reference(cutoff)
    got = batch.closest_atom_distances(cutoff=None if cutoff == INF else cutoff)
    pair = np.where(want[1] >= 0, want[1], -1)
    assert same(got.dist, dev(want[0])), "dist"
    assert torch.equal(got.atom_i, dev(np.where(pair >= 0, pair // A, -1).astype(np.int16)))
    assert torch.equal(got.atom_j, dev(np.where(pair >= 0, pair % A, -1).astype(np.int16)))
    assert_equal_to_yardstick(pkg.ops.closest_atoms(batch.get_xyz(), batch._present_atoms(), cutoff), want, f"PDB, cutoff={cutoff}")
    # the backbone only: the other slots are folded into the mask, and the slots returned are those of the full atom axis
    chosen = batch._present_atoms().cpu().numpy().copy()
    chosen[:, :, 4:] = False
    bb = batch.closest_atom_distances(atoms=("N", "CA", "C", "O"), cutoff=cutoff if cutoff != INF else None)
    want_bb = R.forward(batch.get_xyz().cpu().numpy(), chosen, cutoff)
    assert same(bb.dist, dev(want_bb[0])) and int(bb.atom_i.max()) == 3
    none = bb.atom_i < 0
    assert torch.equal(none, bb.atom_j < 0) and torch.equal(none, torch.isinf(bb.dist))
    assert torch.equal((bb.atom_i.long() * A + bb.atom_j.long()).masked_fill(none, -1), dev(want_bb[1]).long())


def test_structure_batch_contacts_interface_and_fnat(pkg):
    from protstruc_amd import StructureBatch
    batch = pdb_batch()
    B, N = batch.get_xyz().shape[:2]
    chain = batch._chain_keys().cpu().numpy()
    at5 = pdb_reference(5.0)[0]
    for kw in (dict(), dict(other_chains_only=True), dict(min_separation=3)):
        got = batch.residue_contacts(**kw)
        assert got.dtype == torch.bool and tuple(got.shape) == (B, N, N)
        for b in range(B):
            assert np.array_equal(got[b].cpu().numpy(), R.contacts(at5[b], chain[b], **kw)), (kw, b)
    face = batch.interface_residues()
    two_chains = [b for b in range(B) if len(batch.get_chain_ids()[b]) == 2]
    assert len(two_chains) >= 3
    for b in range(B):
        assert np.array_equal(face[b].cpu().numpy(), R.interface(at5[b], chain[b]))
        assert bool(face[b].any()) == (b in two_chains)
    # the CPU test's complex is structure 0
    from tests.test_closest_host import complex_1a3r
    n_own = complex_1a3r()[2].shape[0]
    assert np.array_equal(at5[0][:n_own, :n_own].view(np.int32), complex_1a3r()[3].view(np.int32))
    fnat, n_native = batch.fraction_native_contacts(batch)
    assert fnat.dtype == torch.float32 and n_native.dtype == torch.int64
    for b in range(B):
        ref = R.fnat(at5[b], at5[b], chain[b])
        assert int(n_native[b]) == ref[1] and (float(fnat[b]) == 1.0 if b in two_chains else math.isnan(float(fnat[b])))
    # one chain moved away by 30 A: no native contact is left
    moved = batch.get_xyz().clone()
    moved[batch.chain_idx == 1] += torch.tensor([30.0, 0.0, 0.0], device=moved.device)
    away = StructureBatch(moved, batch.get_atom_mask(), batch.chain_idx, batch.get_chain_ids())
    fnat, n_native = away.fraction_native_contacts(batch)
    for b in two_chains:
        assert float(fnat[b]) == 0.0 and int(n_native[b]) > 0
    ref_moved = R.forward(moved.cpu().numpy(), batch._present_atoms().cpu().numpy(), 5.0)[0]
    for b in range(B):
        ref = R.fnat(ref_moved[b], at5[b], chain[b])
        assert int(n_native[b]) == ref[1] and np.array_equal(np.float32(fnat[b].item()), ref[0], equal_nan=True)


# ---- gradient ----------------------------------------------------------------------------------------------------------------
def assert_gradient_within_the_bound(got, xyz, pair, g, what):
    """|got - ref| <= 2^-23 |ref| + 2^-39 S + 2^-149 for every output float.  The kernel and the restatement each carry at
    most (2N + 8) 2^-53 S <= 2^-41 S of double-precision sum error for N <= 2048 and the kernel rounds to float32 once,
    2^-24 |ref| relative; both terms doubled for slack.  Slots that win nothing are exact zeros."""
    ref, S = R.backward(xyz, pair, g)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -39 * S + 2.0 ** -149
    err = np.abs(got - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{what}: max |got - ref| = {err.max():.3e}, worst against the bound at {worst}: {err[worst]:.3e} for {bound[worst]:.3e}; "
          f"{int((S > 0).sum())} of {S.size} floats carry a term")
    assert (err <= bound).all(), what
    assert (got[S == 0] == 0).all(), f"{what}: a slot that wins no pair is not an exact zero"
    assert (S > 0).any()


def random_grad(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


@pytest.mark.parametrize("N,A", ((65, 15), (129, 15)))
def test_gradient_synthetic(pkg, N, A):
    xyz, mask = chain(N, A)
    pair = chain_reference(N, A, 8.0)[1]
    assert (pair < 0).any() and (pair >= 0).any()
    g = random_grad(pair.shape, N)                      # random on both triangles, and where dist is +inf
    got = pkg.ops.closest_atoms_backward(dev(xyz), dev(pair), dev(g))
    assert_gradient_within_the_bound(got, xyz, pair, g, f"N={N} A={A}")
    assert bool((got[dev(~mask)] == 0).all())
    # int64 pairs with wild values outside [0, A*A) are "none"
    wild = pair.astype(np.int64)
    wild[pair < 0] = np.random.default_rng(1).choice([-1, -32768, A * A, 32767, 2 ** 40], size=int((pair < 0).sum()))
    assert same(pkg.ops.closest_atoms_backward(dev(xyz), dev(wild), dev(g)), got)


def test_gradient_pdb(pkg):
    batch = pdb_batch()
    xyz = batch.get_xyz().cpu().numpy()
    pair = pdb_reference(5.0)[1]
    g = random_grad(pair.shape, 11)
    got = pkg.ops.closest_atoms_backward(batch.get_xyz(), dev(pair), dev(g))
    assert_gradient_within_the_bound(got, xyz, pair, g, "PDB batch")


def test_gradient_through_autograd(pkg):
    xyz, mask = chain(65, 15)
    x = dev(xyz).requires_grad_(True)
    out = pkg.geometry.closest_atom_distances(x, dev(mask), 8.0)
    assert out.dist.requires_grad and not out.atom_i.requires_grad and bool(torch.isinf(out.dist).any())
    torch.where(torch.isfinite(out.dist), out.dist, torch.zeros_like(out.dist)).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    pair = chain_reference(65, 15, 8.0)[1]
    assert_gradient_within_the_bound(x.grad, xyz, pair, np.isfinite(chain_reference(65, 15, 8.0)[0]).astype(np.float32),
                                     "autograd, the sum of the finite distances")
    # float64 coordinates get a float64 gradient of the same values
    x64 = dev(xyz).double().requires_grad_(True)
    d64 = pkg.geometry.closest_atom_distances(x64, dev(mask), 8.0).dist
    torch.where(torch.isfinite(d64), d64, torch.zeros_like(d64)).sum().backward()
    assert x64.grad.dtype == torch.float64 and torch.equal(x64.grad.float(), x.grad)


def test_end_to_end_from_backbone_dihedrals(pkg):
    """a contact restraint on a backbone built from its dihedrals: the loss reaches the angles"""
    from protstruc_amd import StructureBatch
    g = torch.Generator().manual_seed(5)
    dihedrals = ((torch.rand(2, 40, 3, generator=g) * 2 - 1) * math.pi).cuda().requires_grad_(True)
    batch = StructureBatch.from_backbone_dihedrals(dihedrals)
    dist = batch.closest_atom_distances(atoms=("N", "CA", "C")).dist
    assert bool(torch.isfinite(dist).all()) and dist.requires_grad
    (dist[:, 3, 30] + dist[:, 25, 7]).sum().backward()
    assert bool(torch.isfinite(dihedrals.grad).all()) and float(dihedrals.grad.abs().max()) > 0
    assert float(dihedrals.grad[:, 35:].abs().max()) == 0.0, "residues past both pairs do not move them"


def test_repeatability(pkg):
    xyz, mask = chain(129, 15)
    x, m = dev(xyz), dev(mask)
    first = pkg.ops.closest_atoms(x, m, 8.0)
    g = dev(random_grad(first[0].shape, 3))
    grad = pkg.ops.closest_atoms_backward(x, first[1], g)
    for _ in range(2):
        again = pkg.ops.closest_atoms(x, m, 8.0)
        assert same(again[0], first[0]) and same(again[1], first[1])
        assert same(pkg.ops.closest_atoms_backward(x, again[1], g), grad)


# ---- the launch contract -----------------------------------------------------------------------------------------------------
# Two seeded variants that differ in every output; float64 strided coordinates and a float mask, so that the shell's
# conversions are on the launch path that is checked (as the cases of tests/launch_cases.py).
def _contract_inputs(v):
    xyz, mask = R.chain_case(37, 5, seed=40 + {"A": 0, "B": 1}[v])
    pair = R.forward(xyz, mask, 9.0)[1]
    rng = np.random.default_rng(50 + {"A": 0, "B": 1}[v])
    return dict(xyz=torch.from_numpy(np.nan_to_num(xyz)).double(), atom_mask=torch.from_numpy(mask).float(),
                pair=torch.from_numpy(pair).long(), grad_dist=torch.from_numpy(rng.normal(size=pair.shape).astype(np.float32)))


def _ops():
    from protstruc_amd import ops
    return ops


CONTRACT = (
    Case("closest_atoms", ("ps_closest_atoms_f32",), _contract_inputs,
         lambda i: _ops().closest_atoms(i["xyz"], i["atom_mask"], 9.0), strided=("xyz",)),
    Case("closest_atoms_backward", ("ps_closest_atoms_backward_f32",), _contract_inputs,
         lambda i: (_ops().closest_atoms_backward(i["xyz"], i["pair"], i["grad_dist"]),), strided=("xyz",)),
)
BY_NAME = {case.name: case for case in CONTRACT}
NAMES = list(BY_NAME)


@functools.lru_cache(maxsize=None)
def inputs(name, variant):
    return on_device(BY_NAME[name], variant)


@functools.lru_cache(maxsize=None)
def eager(name, variant):
    """the case run eagerly on the default stream, once: the reference of every contract test (never modified)"""
    outs = tuple(BY_NAME[name].run(inputs(name, variant)))
    torch.cuda.synchronize()
    return outs


def assert_variants_differ(name):
    for k, (a, b) in enumerate(zip(eager(name, "A"), eager(name, "B"))):
        assert a.shape == b.shape and a.dtype == b.dtype and not same(a, b), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_contract_cases_meet_the_yardstick(pkg, name):
    assert_variants_differ(name)
    for v in "AB":
        i = _contract_inputs(v)
        xyz = i["xyz"].numpy().astype(np.float32)
        if name == "closest_atoms":
            assert_equal_to_yardstick(eager(name, v), R.forward(xyz, i["atom_mask"].numpy(), 9.0), f"{name} {v}")
        else:
            assert_gradient_within_the_bound(eager(name, v)[0], xyz, i["pair"].numpy(), i["grad_dist"].numpy(), f"{name} {v}")


@pytest.mark.parametrize("name", NAMES)
def test_launches_on_the_callers_stream(pkg, name):
    """As tests/test_gpu_launch_contract.py: on a side stream, a sleep, the copies of variant B over variant A, the op; a
    clone on the default stream meanwhile still sees variant A."""
    case = BY_NAME[name]
    assert_variants_differ(name)
    want_a, want_b = eager(name, "A"), eager(name, "B")
    a, b = inputs(name, "A"), inputs(name, "B")
    live = on_device(case, "A")
    side = side_stream_beside_the_default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        for k in live:
            live[k].copy_(b[k])
    control = live["xyz"].clone()                           # the default stream: runs while the side stream sleeps
    with torch.cuda.stream(side):
        outs = tuple(case.run(live))
    torch.cuda.synchronize()
    if not same(control, a["xyz"]):
        pytest.fail(f"{name}: inconclusive -- the control clone did not see variant A")
    assert_all_same(outs, want_b, f"{name} on a side stream")
    for k, (o, w) in enumerate(zip(outs, want_a)):
        assert not same(o, w), f"{name}: output {k} was computed from the inputs as they were before the side stream's copies"


@pytest.mark.parametrize("name", NAMES)
def test_inside_a_captured_graph(pkg, name):
    """captured on variant A after one eager call, replayed twice on variant B over overwritten outputs"""
    case = BY_NAME[name]
    assert_variants_differ(name)
    want_b, b = eager(name, "B"), inputs(name, "B")
    live = on_device(case, "A")
    case.run(live)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = tuple(case.run(live))
    torch.cuda.synchronize()
    for k in live:
        live[k].copy_(b[k])
    for replay in range(2):
        for o in outs:
            raw(o).fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert_all_same(outs, want_b, f"{name}, replay {replay + 1}")


def test_four_threads_on_four_streams(pkg):
    rounds, n_threads = 3, 4
    want = {(name, v): eager(name, v) for name in NAMES for v in "AB"}
    mine = [{name: on_device(BY_NAME[name], "AB"[t % 2]) for name in NAMES} for t in range(n_threads)]
    streams = [torch.cuda.Stream() for _ in range(n_threads)]
    torch.cuda.synchronize()
    gate = threading.Barrier(n_threads)
    failures = []

    def work(t):
        try:
            variant = "AB"[t % 2]
            order = NAMES[t % 2:] + NAMES[:t % 2]
            gate.wait(timeout=60)
            with torch.cuda.stream(streams[t]):
                for r in range(rounds):
                    results = [(name, tuple(BY_NAME[name].run(mine[t][name]))) for name in order]
                    streams[t].synchronize()
                    for name, outs in results:
                        for k, (o, w) in enumerate(zip(outs, want[name, variant])):
                            if not same(o, w):
                                failures.append(f"thread {t}, round {r}, {name}: output {k} differs from the serial result")
        except Exception as exc:  # noqa: BLE001 -- reported by the main thread
            failures.append(f"thread {t}: {type(exc).__name__}: {exc}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not failures, failures[:10]


def test_offsets_past_two_to_the_31(pkg):
    """B * N * N = 2.16e9 > 2^31 elements of dist, pair and grad_dist (A = 1 keeps the work small): structure b is
    structure b % 3, and every structure's results are those of the three, bit for bit -- the last ones lie past 2^31"""
    B, N = 33000, 256
    xyz = (np.random.default_rng(12).normal(size=(3, N, 1, 3)) * 10.0).astype(np.float32)
    want = R.forward(xyz)
    x3 = dev(xyz)
    small = pkg.ops.closest_atoms(x3)
    assert_equal_to_yardstick(small, want, "N = 256, A = 1")
    g3 = dev(random_grad(want[1].shape, 13))
    grad3 = pkg.ops.closest_atoms_backward(x3, small[1], g3)
    assert_gradient_within_the_bound(grad3, xyz, want[1], random_grad(want[1].shape, 13), "N = 256, A = 1")
    pick = torch.arange(B, device="cuda") % 3
    x = x3[pick]
    dist, pair = pkg.ops.closest_atoms(x)
    assert dist.numel() > 2 ** 31
    for b0 in range(0, B, 3000):
        rows = pick[b0:b0 + 3000]
        assert same(dist[b0:b0 + 3000], small[0][rows]) and same(pair[b0:b0 + 3000], small[1][rows]), f"structures from {b0} on"
    del dist
    grad = pkg.ops.closest_atoms_backward(x, pair, g3[pick])
    assert same(grad, grad3[pick])


def test_batch_limit(pkg):
    """B = 65535 at N = 2, A = 2: structure b is structure b % 3, and the results are those of the three, bit for bit"""
    xyz = (np.random.default_rng(9).normal(size=(3, 2, 2, 3)) * 3.0).astype(np.float32)
    mask = np.ones((3, 2, 2), dtype=bool)
    mask[1, 0, 1] = False                                   # one slot missing, with NaN under the mask
    xyz[1, 0, 1] = np.nan
    want = R.forward(xyz, mask)
    assert (want[1] >= 0).all() and len({tuple(want[0][b].ravel()) for b in range(3)}) == 3
    tensors = dict(xyz=dev(xyz), atom_mask=dev(mask))
    small = pkg.ops.closest_atoms(**tensors)
    assert_equal_to_yardstick(small, want, "N = 2, A = 2")
    assert_batch_of_65535_repeats_the_three(pkg.ops.closest_atoms, tensors, small, "closest_atoms")
    g = random_grad(want[1].shape, 4)
    tensors = dict(xyz=dev(xyz), pair=small[1], grad_dist=dev(g))
    grad = pkg.ops.closest_atoms_backward(**tensors)
    assert_gradient_within_the_bound(grad, xyz, want[1], g, "N = 2, A = 2")
    assert_batch_of_65535_repeats_the_three(pkg.ops.closest_atoms_backward, tensors, grad, "closest_atoms_backward")
