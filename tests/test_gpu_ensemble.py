"""The ensemble kernels on the GPU (K45, K46) against tests/ensemble_ref.py: the matrix of superposed RMSDs against the
float64 yardstick within the bound that include/protstruc_ensemble.h states (tests/test_ensemble_host.py shows by
arithmetic that every input used here lies inside it), its exact properties -- symmetry and the zero diagonal of self
mode, self mode against cross mode, a sub-batch against its block, repeatability --, a cross-check against K37 that does not
go through the restatement, the clustering for equality with its restatement, the StructureBatch methods on twelve
deformed copies of a PDB file; and, since include/protstruc_ensemble.h is not in the case table of tests/launch_cases.py,
this file also holds its two launchers to the launch contract: the caller's stream, capture, four threads, the batch limits.

Measured on an MI355X: the worst |rmsd - yardstick| over every case of test_matrix_against_the_yardstick is 0.495 of the
bound -- the rounding of the result to float32, half an ulp being 0.5 of the bound's 2^-23 rmsd term --, 0.40 on the PDB
ensemble, and 0.074 of the same bound against ops.superpose (test_cross_check_against_superpose); each test prints its figure, and DESIGN.md
section 4 records them."""
import functools
import threading

import numpy as np
import pytest
import torch

from tests import ensemble_ref as R
from tests.launch_cases import Case, on_device
from tests.test_ensemble_host import PDB_NAME, pdb_ensemble
from tests.test_gpu_closest import carve
from tests.test_gpu_launch_contract import (MAX_BATCH, SENTINEL, SLEEP_CYCLES, assert_all_same, raw, same,
                                            side_stream_beside_the_default_stream, tile)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    """a float or int tensor as int32 words: equality of these is equality bit for bit, NaN included"""
    return t.contiguous().view(torch.int32)


# ---- K45 -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def yardstick(case, mode):
    """(rmsd float64, count, E) of a case in "cross" or "self" mode, once"""
    a, b, ma, mb = R.rmsd_case(*case)
    args = (a, b, ma, mb) if mode == "cross" else (a, None, ma, None)
    ref, n = R.pairwise_rmsd(*args)
    return ref, n, R.formula(*args).E


def assert_matrix(got, ref, n, E, what, skip_diagonal=False):
    """counts equal, NaN where the yardstick has NaN, |rmsd - ref| inside the bound; returns the worst fraction of it"""
    rmsd, count = host(got.rmsd).astype(np.float64), host(got.count)
    assert rmsd.shape == ref.shape and got.rmsd.dtype == torch.float32 and got.count.dtype == torch.int32, what
    assert np.array_equal(count, n), what
    look = ~np.eye(ref.shape[0], dtype=bool) if skip_diagonal else np.ones(ref.shape, dtype=bool)
    assert np.array_equal(np.isnan(rmsd)[look], np.isnan(ref)[look]), what
    ok = look & ~np.isnan(ref)
    if not ok.any():
        return 0.0
    fraction = R.fraction_of_bound(np.abs(rmsd - ref)[ok], R.bound(ref, n, E)[ok])
    assert (fraction <= 1.0).all(), f"{what}: {float(fraction.max()):.3f} of the bound"
    return float(fraction.max())


@pytest.mark.parametrize("shape", R.SHAPES)
def test_matrix_against_the_yardstick(pkg, shape):
    geometry = pkg.geometry
    worst = 0.0
    for kind in R.MASK_KINDS:
        case = (*shape, kind)
        what = f"(Ba, Bb, M) = {shape}, masks {kind}"
        a, b, ma, mb = (dev(x) for x in R.rmsd_case(*case))
        cross = geometry.pairwise_rmsd(a, b, ma, mb)
        worst = max(worst, assert_matrix(cross, *yardstick(case, "cross"), what))
        # self mode: both planes exactly symmetric, the diagonal exactly 0 -- NaN for a structure that counts nothing --,
        # the rest inside the bound, and above the diagonal the bits of cross mode on (a, a)
        own = geometry.pairwise_rmsd(a, None, ma)
        ref, n, E = yardstick(case, "self")
        worst = max(worst, assert_matrix(own, ref, n, E, what + ", self mode", skip_diagonal=True))
        assert torch.equal(bits(own.rmsd), bits(own.rmsd.t())) and torch.equal(own.count, own.count.t()), what
        diagonal, counted = host(own.rmsd.diagonal()), np.diagonal(n) > 0
        assert (diagonal[counted] == 0).all() and np.isnan(diagonal[~counted]).all(), what
        twice = geometry.pairwise_rmsd(a, a, ma, ma)
        upper = torch.triu(torch.ones_like(own.count, dtype=torch.bool), 1)
        assert torch.equal(bits(own.rmsd)[upper], bits(twice.rmsd)[upper]) and torch.equal(own.count, twice.count), what
        # every third structure: the block of the full matrix, bit for bit
        third = (lambda m: None if m is None else (m if m.ndim == 1 else m[::3]))
        part = geometry.pairwise_rmsd(a[::3], b[::3], third(ma), third(mb))
        assert torch.equal(bits(part.rmsd), bits(cross.rmsd[::3, ::3])) and torch.equal(part.count, cross.count[::3, ::3]), what
        part = geometry.pairwise_rmsd(a[::3], None, third(ma))
        assert torch.equal(bits(part.rmsd), bits(own.rmsd[::3, ::3])) and torch.equal(part.count, own.count[::3, ::3]), what
        # and again: the same bits
        again, own_again = geometry.pairwise_rmsd(a, b, ma, mb), geometry.pairwise_rmsd(a, None, ma)
        assert torch.equal(bits(again.rmsd), bits(cross.rmsd)) and torch.equal(again.count, cross.count), what
        assert torch.equal(bits(own_again.rmsd), bits(own.rmsd)) and torch.equal(own_again.count, own.count), what
    print(f"(Ba, Bb, M) = {shape}: worst rmsd error {worst:.4f} of its bound")


def test_special_values(pkg):
    ops = pkg.ops
    a, b, _, _ = R.rmsd_case(16, 16, 63, "none")
    a, b = a.copy(), b.copy()
    a[2, 5, 1], b[7, 60, 0] = np.inf, np.nan
    ma, mb = np.ones((16, 63), bool), np.ones((16, 63), bool)
    mb[4, 5], ma[3, 60] = False, False           # they leave out the partner's broken point: those two pairs stay finite
    rmsd, count = (host(t) for t in ops.rmsd_matrix(dev(a), dev(b), dev(ma), dev(mb), return_count=True))
    want = np.zeros((16, 16), bool)
    want[2, :], want[:, 7] = True, True
    want[2, 4], want[3, 7] = False, False
    assert np.array_equal(np.isnan(rmsd), want)
    assert count[2, 4] == 62 and count[3, 7] == 62 and count[0, 0] == 63 and count[2, 7] == 63
    ref, _ = R.pairwise_rmsd(a, b, ma, mb)
    assert np.abs(rmsd - ref)[~want].max() < 1e-4
    only = ops.rmsd_matrix(dev(a), dev(b), dev(ma), dev(mb))                 # without the count plane
    assert only.shape == (16, 16) and np.array_equal(host(only).view(np.int32), rmsd.view(np.int32))
    # a first counted point that is not finite is the structure's origin and enters every x_p: all its pairs are NaN,
    # also those whose partner leaves that point out
    a, b = (x.copy() for x in R.rmsd_case(16, 16, 63, "none")[:2])
    a[5, 0, 2], b[9, 3, 0] = np.inf, np.nan
    ma, mb = np.ones((16, 63), bool), np.ones((16, 63), bool)
    mb[9, :3] = False                          # point 3 is the first that structure 9 of b counts
    mb[6, 0], ma[1, 3] = False, False          # partners that leave the broken origins out
    rmsd, count = (host(t) for t in ops.rmsd_matrix(dev(a), dev(b), dev(ma), dev(mb), return_count=True))
    want = np.zeros((16, 16), bool)
    want[5, :], want[:, 9] = True, True
    assert np.array_equal(np.isnan(rmsd), want) and count[5, 6] == 62 and count[1, 9] == 59 and count[5, 9] == 60
    ref, _ = R.pairwise_rmsd(a, b, ma, mb)
    assert np.abs(rmsd - ref)[~want].max() < 1e-4
    own = host(ops.rmsd_matrix(dev(a), None, dev(ma)))
    assert np.isnan(own[5]).all() and np.isnan(own[:, 5]).all() and np.isfinite(np.delete(np.delete(own, 5, 0), 5, 1)).all()
    empty = ops.rmsd_matrix(torch.zeros(0, 5, 3, device="cuda"), torch.zeros(4, 5, 3, device="cuda"), return_count=True)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4)


@pytest.mark.parametrize("shape", ((15, 17, 4), (16, 16, 63), (3, 65, 257)))
def test_cross_check_against_superpose(pkg, shape):
    """Unmasked pairs against K37 on the same pairs, which makes a pass over the residuals: inside the same bound (the
    two float32 roundings, half an ulp each, fit its 2^-23 rmsd term together)."""
    ops = pkg.ops
    case = (*shape, "none")
    a, b = (dev(x) for x in R.rmsd_case(*case)[:2])
    Ba, Bb, M = shape
    got = host(ops.rmsd_matrix(a, b)).astype(np.float64)
    pairs_a = a[:, None].expand(Ba, Bb, M, 3).reshape(Ba * Bb, M, 3)
    pairs_b = b[None, :].expand(Ba, Bb, M, 3).reshape(Ba * Bb, M, 3)
    fit = host(ops.superpose(pairs_a, pairs_b)[2]).astype(np.float64).reshape(Ba, Bb)
    _, n, E = yardstick(case, "cross")
    fraction = R.fraction_of_bound(np.abs(got - fit), R.bound(fit, n, E))
    assert (fraction <= 1.0).all(), float(fraction.max())
    print(f"{shape}: against ops.superpose, worst {float(fraction.max()):.4f} of the bound")


# ---- K46 -------------------------------------------------------------------------------------------------------------------------
def assert_clusters(pkg, family, B, rule=R.cluster):
    D, cutoff, valid = R.cluster_case(family, B)
    got = pkg.ops.cluster(dev(D), cutoff, dev(valid))
    want = R.cluster_all(D, cutoff, valid, rule=rule)
    for name, g, w in zip(("label", "center", "size", "n_clusters"), got, want):
        assert g.dtype == torch.int32 and np.array_equal(host(g), w), f"{family}, B = {B}: {name} differs from the restatement"
    again = pkg.ops.cluster(dev(D), cutoff, dev(valid))
    assert all(torch.equal(x, y) for x, y in zip(got, again)), (family, B)
    return int(want[3].max())


@pytest.mark.parametrize("family", R.CLUSTER_FAMILIES)
def test_clusters_equal_the_restatement(pkg, family):
    for B in R.CLUSTER_SIZES[:5]:
        assert_clusters(pkg, family, B, rule=R.cluster_plain)


@pytest.mark.parametrize("B", R.CLUSTER_SIZES[5:])
@pytest.mark.parametrize("family", R.LARGE_FAMILIES)
def test_large_clusters_equal_the_restatement(pkg, family, B):
    most = assert_clusters(pkg, family, B)
    print(f"{family}, B = {B}: up to {most} clusters")


def test_single_matrix_through_geometry(pkg):
    D, cutoff, valid = R.cluster_case("invalid", 65)
    got = pkg.geometry.cluster_by_cutoff(dev(D[1]), cutoff, dev(valid[1]))
    want = R.cluster_plain(D[1], cutoff, valid[1])
    assert got.label.shape == (65,) and got.n_clusters.shape == () and int(got.n_clusters) == want.n_clusters
    assert np.array_equal(host(got.label), want.label) and np.array_equal(host(got.center), want.center) and np.array_equal(host(got.size), want.size)


# ---- alignment and sentinels -----------------------------------------------------------------------------------------------------
def intact(buf, start, n_bytes):
    return bool((buf[:start] == SENTINEL).all()) and bool((buf[start + n_bytes:] == SENTINEL).all())


def carved(t, off, dtype=torch.float32):
    """a copy of tensor ``t`` ``off`` bytes past a 16-byte boundary"""
    _, view, _ = carve(t.numel() * t.element_size(), off, dtype)
    view.copy_(t.reshape(-1).view(dtype) if t.dtype != dtype else t.reshape(-1))
    return view


@pytest.mark.parametrize("off,mask_off", ((4, 1), (8, 6), (12, 15), (4, 9), (0, 0)))
def test_sentinels_and_alignment(pkg, off, mask_off):
    """every tensor ``off`` bytes past a 16-byte boundary (the masks ``mask_off``), the outputs and the workspace inside
    sentinels: the results of the aligned run through ``ops``, bit for bit, and no sentinel byte changes"""
    from protstruc_amd import _lib
    lib, ops = _lib.load(), pkg.ops
    stream = torch.cuda.current_stream().cuda_stream
    Ba, Bb, M = 17, 33, 64
    a, b, ma, mb = (dev(x) for x in R.rmsd_case(Ba, Bb, M, "own"))
    am, bm, mam, mbm = carved(a, off), carved(b, off), carved(ma, mask_off, torch.bool), carved(mb, mask_off, torch.bool)
    for self_mode in (False, True):
        n_out = Ba * (Ba if self_mode else Bb)
        want = ops.rmsd_matrix(a, None if self_mode else b, ma, None if self_mode else mb, return_count=True)
        out, cnt = carve(n_out * 4, off, torch.float32), carve(n_out * 4, off, torch.int32)
        rc = lib.ps_rmsd_matrix_f32(am.data_ptr(), mam.data_ptr(), None if self_mode else bm.data_ptr(),
                                    None if self_mode else mbm.data_ptr(), out[1].data_ptr(), cnt[1].data_ptr(), Ba,
                                    Ba if self_mode else Bb, M, stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(out[1]), bits(want[0]).reshape(-1)) and torch.equal(cnt[1], want[1].reshape(-1)), self_mode
        assert intact(out[0], out[2], n_out * 4) and intact(cnt[0], cnt[2], n_out * 4), self_mode
    G, B = 3, 65
    D, cutoff, valid = R.cluster_case("invalid", B)
    want = ops.cluster(dev(D), cutoff, dev(valid))
    n_ws = lib.ps_cluster_workspace_bytes(G, B)
    ws = carve(n_ws, off, torch.uint8)
    outs = [carve(n * 4, off, torch.int32) for n in (G * B, G * B, G * B, G)]
    assert lib.ps_cluster_f32(carved(dev(D), off).data_ptr(), carved(dev(valid), mask_off, torch.bool).data_ptr(), cutoff, ws[1].data_ptr(),
                              *[o[1].data_ptr() for o in outs], G, B, stream) == 0
    torch.cuda.synchronize()
    for (buf, view, start), w, n in zip(outs, want, (G * B, G * B, G * B, G)):
        assert torch.equal(view, w.reshape(-1)) and intact(buf, start, n * 4)
    assert intact(ws[0], ws[2], n_ws)


# ---- StructureBatch --------------------------------------------------------------------------------------------------------------
def test_structure_batch_methods(pkg):
    """twelve members made of one PDB file: three families of four, a 3 A deformation per family, 0.3 A of noise within,
    every member moved rigidly and a tenth of its atoms removed"""
    from protstruc_amd import StructureBatch
    xyz, atom_mask, family = pdb_ensemble()
    B, N, A = atom_mask.shape
    batch = StructureBatch(torch.from_numpy(xyz), torch.from_numpy(atom_mask))
    for atoms, points, mask in ((("CA",), xyz[:, :, 1], atom_mask[:, :, 1]),
                                (("N", "CA", "C"), xyz[:, :, :3].reshape(B, N * 3, 3), atom_mask[:, :, :3].reshape(B, N * 3)),
                                ("all", xyz.reshape(B, N * A, 3), atom_mask.reshape(B, N * A))):
        got = batch.rmsd_matrix(atoms=atoms)
        ref, n = R.pairwise_rmsd(points, None, mask, None)
        worst = assert_matrix(got, ref, n, R.formula(points, None, mask, None).E, f"{PDB_NAME}, atoms {atoms}", skip_diagonal=True)
        assert (host(got.rmsd.diagonal()) == 0).all()
        print(f"{PDB_NAME}, atoms {atoms}: worst rmsd error {worst:.4f} of its bound")
    # against another batch: the first five members against all twelve is the block of the full matrix
    part = StructureBatch(torch.from_numpy(xyz[:5]), torch.from_numpy(atom_mask[:5]))
    full = batch.rmsd_matrix()
    block = part.rmsd_matrix(batch)
    upper = torch.triu(torch.ones(5, 12, dtype=torch.bool, device="cuda"), 1)
    assert block.rmsd.shape == (5, 12) and torch.equal(bits(block.rmsd)[upper], bits(full.rmsd[:5])[upper]) and torch.equal(block.count, full.count[:5])
    with pytest.raises(ValueError, match="same number of residues"):
        batch.rmsd_matrix(StructureBatch(torch.from_numpy(xyz[:2, :-1]), torch.from_numpy(atom_mask[:2, :-1])))
    # the clustering at 1.5 A returns exactly the three families
    for atoms in (("CA",), "all"):
        found = batch.cluster(cutoff=1.5, atoms=atoms)
        label, size = host(found.label), host(found.size)
        assert int(found.n_clusters) == 3 and size.tolist() == [4, 4, 4] + [0] * 9, (atoms, size)
        for f in range(3):
            assert len(set(label[family == f].tolist())) == 1, (atoms, f, label, family)
        assert len(set(label.tolist())) == 3 and (family[host(found.center)[:3]] == [family[label == c][0] for c in range(3)]).all()


# ---- the launch contract ---------------------------------------------------------------------------------------------------------
# Two seeded variants that differ in every output; float64 strided points, a float mask and a float64 strided matrix, so
# that the shell's conversions are on the launch path that is checked (as the cases of tests/launch_cases.py).
CONTRACT_CUTOFF = 2.0


def _matrix_inputs(v):
    a, b, ma, mb = R.contract_case(v)
    t = torch.from_numpy
    return dict(a=t(a).double(), b=t(b), mask_a=t(ma).float(), mask_b=t(mb))


def _cluster_inputs(v):
    rng = np.random.default_rng(950 + "AB".index(v))
    D = np.stack([R.lattice_distances(40, rng) for _ in range(3)])
    return dict(D=torch.from_numpy(D).double(), valid=torch.from_numpy(rng.random((3, 40)) < 0.8).float())


def _ops():
    from protstruc_amd import ops
    return ops


CONTRACT = (
    Case("rmsd_matrix", ("ps_rmsd_matrix_f32",), _matrix_inputs,
         lambda i: _ops().rmsd_matrix(i["a"], i["b"], i["mask_a"], i["mask_b"], return_count=True), strided=("a",)),
    Case("rmsd_matrix_self", ("ps_rmsd_matrix_f32",), _matrix_inputs,
         lambda i: _ops().rmsd_matrix(i["a"], None, i["mask_a"], None, return_count=True), strided=("a",)),
    Case("cluster", ("ps_cluster_f32",), _cluster_inputs, lambda i: _ops().cluster(i["D"], CONTRACT_CUTOFF, i["valid"]), strided=("D",)),
)
BY_NAME = {case.name: case for case in CONTRACT}
NAMES = list(BY_NAME)
HOST_FUNCTIONS = {"ps_ensemble_api", "ps_cluster_workspace_bytes"}


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


def test_contract_cases_cover_the_header_and_meet_the_yardstick(pkg):
    from protstruc_amd import _lib
    assert sorted({s for case in CONTRACT for s in case.symbols}) == sorted(set(_lib.ENSEMBLE_SIGNATURES) - HOST_FUNCTIONS)
    for name in NAMES:
        assert_variants_differ(name)
    geometry = pkg.geometry
    for v in "AB":
        a, b, ma, mb = R.contract_case(v)
        for name, args in (("rmsd_matrix", (a, b, ma, mb)), ("rmsd_matrix_self", (a, None, ma, None))):
            ref, n = R.pairwise_rmsd(*args)
            assert_matrix(geometry.PairwiseRMSD(*eager(name, v)), ref, n, R.formula(*args).E, f"contract {name} {v}",
                          skip_diagonal=name.endswith("self"))
        i = {k: t.numpy() for k, t in _cluster_inputs(v).items()}
        want = R.cluster_all(i["D"].astype(np.float32), CONTRACT_CUTOFF, i["valid"] != 0, rule=R.cluster_plain)
        assert all(np.array_equal(host(g), w) for g, w in zip(eager("cluster", v), want)), v


@pytest.mark.parametrize("name", NAMES)
def test_launches_on_the_callers_stream(pkg, name):
    """As tests/test_gpu_launch_contract.py: on a side stream, a sleep, the copies of variant B over variant A, the op; a
    clone on the default stream meanwhile still sees variant A."""
    case = BY_NAME[name]
    assert_variants_differ(name)
    want_a, want_b = eager(name, "A"), eager(name, "B")
    a, b = inputs(name, "A"), inputs(name, "B")
    live = on_device(case, "A")
    first = next(iter(live))
    side = side_stream_beside_the_default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        for k in live:
            live[k].copy_(b[k])
    control = live[first].clone()                           # the default stream: runs while the side stream sleeps
    with torch.cuda.stream(side):
        outs = tuple(case.run(live))
    torch.cuda.synchronize()
    if not same(control, a[first]):
        pytest.fail(f"{name}: inconclusive -- the control clone did not see variant A")
    assert_all_same(outs, want_b, f"{name} on a side stream")
    assert any(not same(o, w) for o, w in zip(outs, want_a)), f"{name}: computed from the inputs as they were before the side stream's copies"


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
            order = NAMES[t % len(NAMES):] + NAMES[:t % len(NAMES)]
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


def test_batch_limits(pkg):
    ops = pkg.ops
    a, b, a3 = (dev(x) for x in R.limit_case())
    # Ba = 65535, Bb = 3, M = 4: structure i of a is structure i % 3, and the rows are those of the three, bit for bit
    small = ops.rmsd_matrix(a, b, return_count=True)
    ref, n = R.pairwise_rmsd(host(a), host(b))
    assert_matrix(pkg.geometry.PairwiseRMSD(*small), ref, n, R.formula(host(a), host(b)).E, "M = 4")
    big = ops.rmsd_matrix(tile(a), b, return_count=True)
    torch.cuda.synchronize()
    assert big[0].shape == (MAX_BATCH, 3) and same(big[0], tile(small[0])) and same(big[1], tile(small[1]))
    wide = ops.rmsd_matrix(b, tile(a), return_count=True)
    narrow = ops.rmsd_matrix(b, a, return_count=True)
    assert wide[0].shape == (3, MAX_BATCH) and same(wide[0].t().contiguous(), tile(narrow[0].t().contiguous()))
    assert same(wide[1].t().contiguous(), tile(narrow[1].t().contiguous()))
    # G = 65535 matrices of two items
    D = torch.tensor([[[0.0, 1.0], [9.0, 0.0]], [[0.0, 3.0], [0.0, 0.0]], [[0.0, float("nan")], [1.0, 0.0]]], device="cuda")
    valid = torch.tensor([[True, True], [True, True], [False, True]], device="cuda")
    small = ops.cluster(D, 2.0, valid)
    assert host(small[0]).tolist() == [[0, 0], [0, 1], [-1, 0]] and host(small[3]).tolist() == [1, 2, 1]
    assert host(small[1]).tolist() == [[0, -1], [0, 1], [1, -1]] and host(small[2]).tolist() == [[2, 0], [1, 1], [1, 0]]
    big = ops.cluster(tile(D), 2.0, tile(valid))
    torch.cuda.synchronize()
    assert all(g.shape[0] == MAX_BATCH and same(g, tile(s)) for g, s in zip(big, small))


def test_self_mode_past_two_to_the_32_bytes(pkg):
    """B = 32771 at M = 3: the last rows of both planes lie more than 2^32 bytes into them.  Structure i is structure
    i % 3 of three, so above the diagonal entry (i, j) is entry (i % 3, j % 3) of cross mode on the three, below it the
    mirror image, and the diagonal is 0: compared on the GPU, bit for bit."""
    ops = pkg.ops
    B = 32771
    a3 = dev(R.limit_case()[2])
    cross, cross_n = ops.rmsd_matrix(a3, a3, return_count=True)
    ref, n = R.pairwise_rmsd(host(a3))
    assert_matrix(pkg.geometry.PairwiseRMSD(cross, cross_n), ref, n, R.formula(host(a3)).E, "M = 3", skip_diagonal=True)
    idx = torch.arange(B, device="cuda") % 3
    rmsd, count = ops.rmsd_matrix(a3[idx], return_count=True)
    torch.cuda.synchronize()
    assert rmsd.shape == (B, B) and rmsd.numel() * 4 > 2 ** 32
    for got, three, diagonal in ((rmsd, cross, 0.0), (count, cross_n, 3)):
        want = torch.triu(three[idx][:, idx], 1)
        want = want + want.t()
        want.diagonal().fill_(diagonal)
        assert torch.equal(bits(got), bits(want))
        del want
