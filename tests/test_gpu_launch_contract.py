"""The launch contract of include/protstruc_hip.h ("Conventions (all entry points)") for every entry point of the case
table tests/launch_cases.py: the launch goes to the caller's stream; nothing on the launch path allocates behind
PyTorch's back, synchronises or reads device memory on the host, so the call can be captured into a graph; any number of
threads and streams may call at once; and a launcher that puts the structure on grid.y works at the 65535 structures its
argument check accepts.

Every comparison is BITWISE against the same call run eagerly on the default stream: all these ops are deterministic, so
no tolerance is involved.  The inputs are never poisoned: a launch that goes to the wrong stream, or a replay that reads a
stale temporary, computes on old, valid data and is caught because the two variants of a case differ in every output.
"""
import functools
import threading
import time

import numpy as np
import pytest
import torch

from tests import (dssp_ref, edge_ref, fape_ref, knn_ref, launch_cases, lddt_ref, sasa_ref, test_gpu_dssp, test_gpu_edge,
                   test_gpu_fape, test_gpu_knn, test_gpu_lddt, test_gpu_sasa, test_gpu_violation, violation_ref)

pytestmark = pytest.mark.gpu

CASES = launch_cases.CASES
NAMES = [case.name for case in CASES]
# torch.cuda._sleep on an MI355X: 100 000 000 cycles measured 41.6 - 46.9 ms from enqueue to the end of a device
# synchronise (10 000 000: 4.2 - 4.6 ms), against 0.06 - 1.3 ms to enqueue a case's copies, the control clone and the op
SLEEP_CYCLES = 100_000_000
SENTINEL = 0x5A
MAX_BATCH = 65535


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def raw(t):
    """the bytes of a tensor, as a view where it is contiguous"""
    return t.contiguous().view(torch.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


def assert_all_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"{what}: output {k} differs from the eager result on the default stream"


@functools.lru_cache(maxsize=None)
def inputs(name, variant):
    """the case's inputs on the device, made once and never modified"""
    return launch_cases.on_device(launch_cases.BY_NAME[name], variant)


@functools.lru_cache(maxsize=None)
def eager(name, variant):
    """the case run eagerly on the default stream, once: the reference of every test here (never modified)"""
    outs = tuple(launch_cases.BY_NAME[name].run(inputs(name, variant)))
    torch.cuda.synchronize()
    assert all(isinstance(o, torch.Tensor) and o.is_cuda and o.numel() for o in outs), name
    return outs


def assert_variants_differ(name):
    for k, (a, b) in enumerate(zip(eager(name, "A"), eager(name, "B"))):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, k)
        assert not same(a, b), f"{name}: output {k} is the same for both variants, so it cannot tell which inputs a launch read"


@pytest.mark.parametrize("name", NAMES)
def test_the_two_variants_differ_in_every_output(pkg, name):
    assert_variants_differ(name)
    again = tuple(launch_cases.BY_NAME[name].run(inputs(name, "A")))
    assert_all_same(again, eager(name, "A"), f"{name}, a second eager call")


def side_stream_beside_the_default_stream():
    """A fresh stream whose work runs BESIDE the default stream's.  HIP spreads a process's streams over a few hardware
    queues (four unless the environment says otherwise) and two streams on one queue take turns: behind a sleeping side
    stream on its own queue the default stream waits too, and the control of the test below cannot hold -- one fresh
    stream in four is such a stream.  So every candidate is tried: a tenth of the sleep on it and a clone on the default
    stream between two events; the candidate serves if the default stream took under a millisecond for that."""
    probe = torch.zeros(16, device="cuda")
    for attempt in range(32):
        side = torch.cuda.Stream()
        before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        before.record()
        with torch.cuda.stream(side):
            torch.cuda._sleep(SLEEP_CYCLES // 10)
        probe.clone()
        after.record()
        torch.cuda.synchronize()
        waited = before.elapsed_time(after)
        print(f"candidate {attempt}: the default stream took {waited:.3f} ms beside a sleeping side stream")
        if waited < 1.0:
            return side
    pytest.fail("no stream of 32 ran beside the default stream")


@pytest.mark.parametrize("name", NAMES)
def test_launches_on_the_callers_stream(pkg, name):
    """On a fresh side stream: a sleep of SLEEP_CYCLES, the in-place copies of variant B over variant A, the op.  Every
    kernel the call enqueues -- the shell's conversions included -- has to wait behind the copies, so the outputs are
    eager(B); one that went to another stream reads variant A.  The control: a clone taken on the default stream after
    the copies were enqueued still holds variant A, i.e. the sleep outlasted the enqueueing.  SLEEP_CYCLES = 100 000 000
    lasts 42 - 47 ms on an MI355X; enqueueing a case takes 0.06 - 1.3 ms."""
    case = launch_cases.BY_NAME[name]
    assert_variants_differ(name)
    want_a, want_b = eager(name, "A"), eager(name, "B")
    a, b = inputs(name, "A"), inputs(name, "B")
    live = launch_cases.on_device(case, "A")
    control_key = next(k for k in a if not same(a[k], b[k]))
    side = side_stream_beside_the_default_stream()
    torch.cuda.synchronize()
    start = time.perf_counter()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        for k in live:
            live[k].copy_(b[k])
    control = live[control_key].clone()                     # the default stream: runs while the side stream sleeps
    with torch.cuda.stream(side):
        outs = tuple(case.run(live))
    enqueued = time.perf_counter() - start
    torch.cuda.synchronize()
    drained = time.perf_counter() - start
    print(f"{name}: enqueued in {1e3 * enqueued:.2f} ms, drained after {1e3 * drained:.2f} ms")
    if not same(control, a[control_key]):
        pytest.fail(f"{name}: inconclusive -- the control clone did not see variant A: {SLEEP_CYCLES} cycles of sleep, "
                    f"enqueueing took {1e3 * enqueued:.2f} ms, everything drained after {1e3 * drained:.2f} ms")
    for k in live:
        assert same(live[k], b[k]), (name, k)
    assert_all_same(outs, want_b, f"{name} on a side stream")
    for k, (o, w) in enumerate(zip(outs, want_a)):
        assert not same(o, w), f"{name}: output {k} was computed from the inputs as they were before the side stream's copies"


@pytest.mark.parametrize("name", NAMES)
def test_inside_a_captured_graph(pkg, name):
    """One op, one graph, one stream (as tests/test_gpu_nerf_backward.py::test_inside_a_captured_graph): captured on
    variant A after one eager call, replayed twice on variant B with the outputs overwritten before each replay."""
    case = launch_cases.BY_NAME[name]
    assert_variants_differ(name)
    want_b, b = eager(name, "B"), inputs(name, "B")
    live = launch_cases.on_device(case, "A")
    case.run(live)                                          # eager first: loads the code object, fills the host caches
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs = tuple(case.run(live))
    torch.cuda.synchronize()
    assert all(o.is_contiguous() for o in outs)
    for k in live:
        live[k].copy_(b[k])
    for replay in range(2):
        for o in outs:
            raw(o).fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert_all_same(outs, want_b, f"{name}, replay {replay + 1}")


def test_four_threads_on_four_streams(pkg):
    """Four threads, each with its own stream and its own copies of the inputs (variants A, B, A, B), run the whole table
    three times, each from another starting point: every result equals the serial eager one.  The sphere cache of
    geometry.solvent_accessibility starts empty, so the threads also fill it at the same time."""
    rounds, n_threads = 3, 4
    want = {(name, v): eager(name, v) for name in NAMES for v in "AB"}
    mine = [{name: launch_cases.on_device(launch_cases.BY_NAME[name], "AB"[t % 2]) for name in NAMES} for t in range(n_threads)]
    streams = [torch.cuda.Stream() for _ in range(n_threads)]
    pkg.geometry._SPHERES.clear()
    torch.cuda.synchronize()
    gate = threading.Barrier(n_threads)
    failures = []

    def work(t):
        try:
            variant = "AB"[t % 2]
            first = t * len(NAMES) // n_threads
            order = NAMES[first:] + NAMES[:first]
            gate.wait(timeout=60)
            with torch.cuda.stream(streams[t]):
                for r in range(rounds):
                    results = [(name, tuple(launch_cases.BY_NAME[name].run(mine[t][name]))) for name in order]
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


# ---- the batch limit of the twelve launchers that put the structure on grid.y ------------------------------------------------
# Three distinct structures at the smallest size that gives the kernel real work, checked against the op's float64
# yardstick under the contract of the op's own test file; then 65535 structures, structure b being structure b % 3, whose
# results must be those of the three, bit for bit.
def cuda(t):
    if t is None:
        return None
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda()


def tile(t):
    """(3, ...) on the device -> (65535, ...), entry b = entry b % 3"""
    return None if t is None else t.index_select(0, torch.arange(MAX_BATCH, device=t.device) % 3)


def assert_batch_of_65535_repeats_the_three(run, tensors, small, what):
    """``run(**tensors)`` on the tiled tensors against ``small``, the results for the three structures"""
    big = run(**{k: tile(t) for k, t in tensors.items()})
    torch.cuda.synchronize()
    big = big if isinstance(big, tuple) else (big,)
    small = small if isinstance(small, tuple) else (small,)
    assert len(big) == len(small)
    for k, (g, s) in enumerate(zip(big, small)):
        if g is None and s is None:
            continue
        assert g.shape[0] == MAX_BATCH and same(g, tile(s)), \
            f"{what}: output {k} at B = {MAX_BATCH} is not the B = 3 result repeated"


def fape_small():
    """N = 2 frames, M = 3 points: the frames of two random residues, the first three atoms as points"""
    g = torch.Generator().manual_seed(21)
    target = 8 * torch.randn(3, 2, 3, 3, generator=g)
    xyz = target + 4 * torch.randn(3, 2, 3, 3, generator=g)
    rot, trans = fape_ref.frames_from_xyz(xyz, *fape_ref.SLOTS)
    trot, ttrans = fape_ref.frames_from_xyz(target, *fape_ref.SLOTS)
    operands = [rot, trans, xyz.reshape(3, 6, 3)[:, :3].contiguous(), trot, ttrans, target.reshape(3, 6, 3)[:, :3].contiguous()]
    return operands, torch.full((3,), 10.0), torch.randn(3, generator=g)


def fape_reference(operands, clamp, grad_loss, dtype):
    """(loss, count, (grad_rot, grad_trans, grad_pts)) of tests/fape_ref.py in ``dtype``, on float32 operands"""
    ops_ = [t.detach().to(dtype) for t in operands]
    leaves = [t.requires_grad_(True) for t in ops_[:3]]
    loss, count = fape_ref.fape(*leaves, *ops_[3:], clamp=clamp.to(dtype), scale=10.0, eps=1e-4)
    grads = torch.autograd.grad((loss * grad_loss.to(dtype)).sum(), leaves)
    return loss.detach(), count.detach(), grads


def test_batch_limit_fape(pkg):
    T = test_gpu_fape
    operands, clamp, grad_loss = fape_small()
    loss64, count64, grad64 = fape_reference(operands, clamp, grad_loss, torch.float64)
    loss32, _, grad32 = fape_reference(operands, clamp, grad_loss, torch.float32)
    names = ("rot", "trans", "points", "target_rot", "target_trans", "target_points")
    tensors = dict(zip(names, (t.cuda() for t in operands)), clamp=clamp.cuda(), grad_loss=grad_loss.cuda())

    def forward(grad_loss, clamp, **kw):
        return pkg.ops.fape(*[kw[k] for k in names], clamp=clamp)

    def backward(grad_loss, clamp, **kw):
        return pkg.ops.fape_backward(*[kw[k] for k in names], grad_loss, clamp=clamp)

    loss, count = forward(**tensors)
    assert torch.equal(count.cpu().double(), count64) and float(count64.min()) == 6.0
    e_kernel, e_f32 = T.relative_loss_error(loss, loss64), T.relative_loss_error(loss32, loss64)
    print(f"fape N=2 M=3: E_kernel = {e_kernel:.3e}  E_f32 = {e_f32:.3e}")
    assert e_kernel <= T.MARGIN * max(e_f32, 2.0 ** -24)
    grads = backward(**tensors)
    for what, g, want, f32 in zip(("grad_rot", "grad_trans", "grad_pts"), grads, grad64, grad32):
        T.check_rows("fape N=2 M=3", what, g.cpu(), want, f32)
    assert_batch_of_65535_repeats_the_three(forward, tensors, (loss, count), "fape")
    assert_batch_of_65535_repeats_the_three(backward, tensors, grads, "fape_backward")


def test_batch_limit_lddt(pkg):
    T, R = test_gpu_lddt, lddt_ref
    case = R.random_case(B=3, M=3, noise=0.3, seed=121)
    hard_open, smooth_open, grad_open = R.open_points(case)
    (s_lo, s_hi), (n_lo, n_hi), _ = R.brackets(case)
    ref = {"case": case, "n_lo": n_lo, "n_hi": n_hi}
    assert not hard_open.any() and not grad_open.any() and float(n_lo.min()) == 2.0     # every pair counts, none at a border
    tensors = dict(points=case.points.cuda(), target_points=case.target.cuda(), grad_S=case.grad_S.cuda())

    def forward(points, target_points, grad_S):
        return pkg.ops.lddt(points, target_points)

    def smooth(points, target_points, grad_S):
        return pkg.ops.lddt(points, target_points, smooth=True)

    def backward(points, target_points, grad_S):
        return pkg.ops.lddt_backward(points, target_points, grad_S)

    S, n = forward(**tensors)
    T.check_count("lddt M=3", n, ref)
    four = torch.tensor(4.0)
    assert ((s_lo.float() / four <= S.cpu()) & (S.cpu() <= s_hi.float() / four)).all(), "S outside its bracket"
    Ss, ns = smooth(**tensors)
    T.check_count("lddt M=3 smooth", ns, ref)
    T.check_rows("lddt M=3", "S", Ss.cpu(), R.forward(case, True)[0], R.forward(case, True, torch.float32)[0], smooth_open,
                 floor=2.0 ** -24)
    grad = backward(**tensors)
    T.check_rows("lddt M=3", "grad_points", grad.cpu(), R.gradient(case), R.gradient(case, torch.float32), grad_open)
    assert_batch_of_65535_repeats_the_three(forward, tensors, (S, n), "lddt")
    assert_batch_of_65535_repeats_the_three(smooth, tensors, (Ss, ns), "lddt, smooth")
    assert_batch_of_65535_repeats_the_three(backward, tensors, grad, "lddt_backward")


def test_batch_limit_clash(pkg):
    T, R = test_gpu_violation, violation_ref
    case = R.random_case(B=3, M=3, seed=221)
    n_lo, n_hi, open_ = R.brackets(case)
    assert not open_.any() and float(n_lo.sum()) > 0                                    # something clashes, nothing at the kink
    tensors = dict(points=case.points.cuda(), radius=case.radius.cuda(), grad_E=case.grad_E.cuda())

    def forward(points, radius, grad_E):
        return pkg.ops.clash(points, radius)

    def backward(points, radius, grad_E):
        return pkg.ops.clash_backward(points, radius, grad_E)

    E, n = forward(**tensors)
    T.check_rows("clash M=3", "E", E.cpu(), R.forward(case)[0], R.forward(case, torch.float32)[0])
    assert ((n_lo <= n.cpu().double()) & (n.cpu().double() <= n_hi)).all()
    grad = backward(**tensors)
    T.check_rows("clash M=3", "grad_points", grad.cpu(), R.gradient(case), R.gradient(case, torch.float32), open_)
    assert_batch_of_65535_repeats_the_three(forward, tensors, (E, n), "clash")
    assert_batch_of_65535_repeats_the_three(backward, tensors, grad, "clash_backward")


def helices(residues):
    """(3, len, 4, 3) float32: the given residues of an ideal alpha-, 3-10 and pi-helix of tests/dssp_ref.py"""
    builders = (dssp_ref.ideal_helix, dssp_ref.helix_310, dssp_ref.pi_helix)
    return np.stack([np.asarray(build(8))[list(pick)] for build, pick in zip(builders, residues)]).astype(np.float32)


def test_batch_limit_backbone_hbonds(pkg):
    """N = 3: residues 0, n-1 and n of a helix whose hydrogen bonds run i -> i+n, so that the last residue's amide hydrogen
    (placed from the middle residue, its true predecessor) bonds to the first residue's carbonyl"""
    T = test_gpu_dssp
    xyz = helices(((0, 3, 4), (0, 2, 3), (0, 4, 5)))
    complete = np.ones((3, 3), dtype=bool)
    junction = np.tile(np.array([False, True, False]), (3, 1))
    refs = [dssp_ref.dssp(xyz[b], complete[b], junction[b]) for b in range(3)]
    T.assert_margins(refs, "three helix fragments")
    assert all((bonds.acceptor_idx[2] == [0, -1]).all() for bonds, _ in refs), "every fragment has its one hydrogen bond"
    tensors = dict(xyz=cuda(xyz), complete=cuda(complete), junction=cuda(junction))
    small = pkg.geometry.backbone_hbonds(**tensors)
    T.assert_hbonds_equal(small, refs, "N = 3")
    assert_batch_of_65535_repeats_the_three(pkg.ops.backbone_hbonds, tensors, tuple(small), "backbone_hbonds")


def test_batch_limit_dssp_assign(pkg):
    """N = 5, not 3: no turn, bridge or bend fits into three residues, so every label would be '-'.  Five residues hold
    the alpha-helix's 4-turn and two consecutive 3-turns of the 3-10 helix."""
    T = test_gpu_dssp
    xyz = helices(((0, 1, 2, 3, 4),) * 3)
    complete = np.ones((3, 5), dtype=bool)
    junction = np.tile(np.array([True, True, True, True, False]), (3, 1))
    refs = [dssp_ref.dssp(xyz[b], complete[b], junction[b]) for b in range(3)]
    T.assert_margins(refs, "three helix starts")
    labels = [dssp_ref.strings(codes) for _, codes in refs]
    print("labels:", labels)
    assert len(set(labels)) == 3 and all(set(s) != {"-"} for s in labels[:2])
    acceptor = np.stack([bonds.acceptor_idx for bonds, _ in refs]).astype(np.int32)
    tensors = dict(xyz=cuda(xyz), complete=cuda(complete), junction=cuda(junction), acceptor_idx=cuda(acceptor))
    codes = pkg.ops.dssp_assign(**tensors)
    T.assert_codes_equal(codes, refs, "N = 5")
    assert_batch_of_65535_repeats_the_three(pkg.ops.dssp_assign, tensors, codes, "dssp_assign")


def test_batch_limit_solvent_accessibility(pkg):
    """M = 2 with a 4-point sphere: three pairs of atoms with different radii, the second atom along one direction of the
    table, between two of them, and 6 A away along another"""
    T = test_gpu_sasa
    sphere = sasa_ref.sphere_points(4)
    u = sphere.astype(np.float64)
    r = np.array([[1.7, 1.52], [1.55, 1.8], [1.8, 1.55]], dtype=np.float32)
    x = np.zeros((3, 2, 3), dtype=np.float32)
    x[0, 1], x[1, 1], x[2, 1] = 2.5 * u[0], 1.2 * (u[1] + u[2]), 6.0 * u[3]
    refs = sasa_ref.batch(x, r, sphere=sphere)
    T.assert_margin(refs, "M = 2, S = 4")
    assert sum(int(ref.buried.sum()) for ref in refs) > 0 and len({tuple(ref.count) for ref in refs}) > 1
    assert len({tuple(ref.area) for ref in refs}) == 3
    tensors = dict(points=cuda(x), radius=cuda(r))
    table = cuda(sphere)

    def run(points, radius):
        return pkg.ops.solvent_accessibility(points, radius, sphere=table)

    small = run(**tensors)
    T.assert_equal_to_yardstick(pkg.geometry.SolventAccessibility(*small), refs, "M = 2, S = 4")
    assert_batch_of_65535_repeats_the_three(run, tensors, small, "solvent_accessibility")


def test_batch_limit_nearest_neighbors(pkg):
    T = test_gpu_knn
    x = np.stack([knn_ref.cloud(3, seed=31 + b, spread=4.0) for b in range(3)])
    refs = knn_ref.batch(x, 2)
    tensors = dict(points=cuda(x))

    def run(points):
        return pkg.ops.nearest_neighbors(points, 2)

    small = run(**tensors)
    T.assert_equal_to_yardstick(small, refs, "M = 3, k = 2")
    assert int(small[2].min()) == 2
    assert_batch_of_65535_repeats_the_three(run, tensors, small, "nearest_neighbors")


def tiny_graph():
    """(3, 2, 1) int32: each of the two residues points at the other; in the last structure the second one is padding"""
    return np.array([[[1], [0]], [[1], [0]], [[1], [-1]]], dtype=np.int32)


def test_batch_limit_edge_rbf(pkg):
    T = test_gpu_edge
    xyz = (np.random.default_rng(41).normal(size=(3, 2, 2, 3)) * 3.0).astype(np.float32)
    idx = tiny_graph()
    centers, sigma = np.array([4.0], np.float32), 2.0
    ref = edge_ref.edge_rbf(xyz, idx, None, [0], [1], centers, sigma)
    assert ref.real.sum() == 5
    tensors = dict(xyz=cuda(xyz), idx=cuda(idx))

    def run(xyz, idx):
        return pkg.ops.edge_rbf(xyz, idx, pair_i=[0], pair_j=[1], centers=centers, sigma=sigma)

    small = run(**tensors)
    T.assert_rbf_meets_the_yardstick(small, ref, "N=2 k=1 P=1 R=1")
    assert_batch_of_65535_repeats_the_three(run, tensors, small, "edge_rbf")


def test_batch_limit_edge_frames(pkg):
    T = test_gpu_edge
    rot, trans = edge_ref.random_frames(3, 2, seed=42)
    idx = tiny_graph()
    ref = edge_ref.edge_frames(rot, trans, idx)
    assert ref.real.sum() == 5
    tensors = dict(rot=cuda(rot), trans=cuda(trans), idx=cuda(idx))
    small = pkg.ops.edge_frames(**tensors)
    T.assert_frames_equal_the_yardstick(small, ref, "N=2 k=1")
    assert_batch_of_65535_repeats_the_three(pkg.ops.edge_frames, tensors, small, "edge_frames")
