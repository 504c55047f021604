"""Message passing on graphs (K55 - K59, include/protstruc_aggregate.h) on the GPU, against the float64 restatement of
tests/aggregate_ref.py: bit for bit where the header promises bits (K55 in its four modes and both groupings with ``arg``,
K56, K57, and K59 given the kernel's own ``w``), within one float32 rounding for K58; exact +0 and -1 where they are
defined; NaN planted at every padding position; every tensor also 4, 8 and 12 bytes off a 16-byte boundary inside
sentinels, where the dword arm must give the bits of the 16-byte arm; the public functions and their autograd; one
attention layer end to end on the PDB files; and the launch contract (a side stream, a captured graph, four threads on four
streams, B = 65535).

The shapes are the smallest at which a kernel can still go wrong: 150 segments (both sides of lanes 64 and 128) with list
lengths from {0, 1, 2, 63, 64, 65, 200}, rows of 1 to 260 floats (both arms, L at and around a power of two, more than one
wave to a row), a bipartite pair, a star (in-degree 50 against 1), one list of 1000."""
import functools
import threading

import numpy as np
import pytest
import torch

from tests import aggregate_ref as A
from tests.test_gpu_edge import bits, dev, pdb_batch
from tests.test_gpu_launch_contract import (SENTINEL, SLEEP_CYCLES, assert_all_same, raw, same,
                                            side_stream_beside_the_default_stream)

pytestmark = pytest.mark.gpu

ROWS = ((1, 1), (1, 3), (1, 4), (1, 5), (3, 4), (8, 16), (1, 64), (1, 68), (4, 65), (1, 260))
SENT = 777.0
BACK = 9


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _aggregate, _lib, geometry, ops  # noqa: F401 -- reached through the package
    _lib.load()
    _aggregate.load()
    return protstruc_amd


# ---- the graphs ------------------------------------------------------------------------------------------------------------------------
class Graph:
    """an edge list with both groupings and both node indices, on the host and on the device"""

    def __init__(self, name, B, Q, M, row_ptr, col):
        self.name, self.B, self.Q, self.M = name, B, Q, M
        self.row_ptr, self.col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int32)
        self.E = len(self.col)
        self.real = A.real_positions(self.row_ptr, self.col, M)
        self.host = {at: A.grouping(self.row_ptr, self.col, B, Q, M, at) for at in ("source", "target")}
        self.index = {at: A.edge_index(self.row_ptr, self.col, Q, M, at) for at in ("source", "target")}

    @functools.lru_cache(maxsize=None)
    def device(self, at):
        """(ptr, perm, row_ptr, col, index) on the device; the target grouping is ops.csr_incoming_edges' own"""
        from protstruc_amd import ops
        row_ptr, col = dev(self.row_ptr), dev(self.col)
        ptr, perm = (row_ptr, None) if at == "source" else ops.csr_incoming_edges(row_ptr, col, self.B, self.Q, self.M)
        if at == "target":
            assert np.array_equal(ptr.cpu().numpy(), self.host[at][0]) and np.array_equal(perm.cpu().numpy(), self.host[at][1])
        return ptr, perm, row_ptr, col, dev(self.index[at])

    def dims(self):
        return dict(B=self.B, Q=self.Q, M=self.M)

    def plant(self, x):
        """a copy of the per-edge array ``x`` with NaN at the padding"""
        x = np.array(x, copy=True)
        x[~self.real] = np.nan
        return x


def lists_of(lengths, M, seed, tail=0, bad=()):
    rng = np.random.default_rng(seed)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = rng.integers(0, M, size=int(row_ptr[-1]) + tail).astype(np.int32)
    if tail:
        col[-tail:] = -1
    for p, value in bad:
        col[p] = value
    return row_ptr, col


@functools.lru_cache(maxsize=None)
def graph(name):
    rng = np.random.default_rng(41)
    if name == "main":      # 3 x 50 rows with every length of the set, a max_edges tail, and padding inside rows
        lengths = rng.permutation(np.resize([0, 1, 2, 63, 64, 65, 200], 150))
        row_ptr, col = lists_of(lengths, 50, 1, tail=7, bad=((5, -1), (70, 50), (71, 2 ** 31 - 1), (300, -1), (301, -7), (4000, 53)))
        return Graph(name, 3, 50, 50, row_ptr, col)
    if name in ("bipartite 1x64", "bipartite 65x130"):
        Q, M = (1, 64) if name.endswith("1x64") else (65, 130)
        row_ptr, col = lists_of(rng.integers(0, 9, size=2 * Q) if Q > 1 else [150, 61], M, 2, tail=3, bad=((1, -1),))
        return Graph(name, 2, Q, M, row_ptr, col)
    if name == "star":      # node 0 is in every row: in-degree 50 against 1
        col = np.stack([np.zeros(50, dtype=np.int32), (np.arange(50, dtype=np.int32) + 1) % 50], 1).reshape(-1)
        return Graph(name, 1, 50, 50, np.arange(51, dtype=np.int64) * 2, col)
    if name == "long":      # one row of 1000
        row_ptr, col = lists_of([1000, 0, 3], 40, 3)
        return Graph(name, 1, 3, 40, row_ptr, col)
    if name == "padded":    # a padded kNN list as the CSR list it is: -1 inside rows
        idx = rng.integers(0, 20, size=(2, 20, 6)).astype(np.int32)
        idx[rng.random(idx.shape) < 0.3] = -1
        return Graph(name, 2, 20, 20, np.arange(41, dtype=np.int64) * 6, idx.reshape(-1))
    raise KeyError(name)


OTHER_GRAPHS = ("bipartite 1x64", "bipartite 65x130", "star", "long", "padded")


# ---- raw calls with every tensor off a 16-byte boundary, inside sentinels -----------------------------------------------------------------
def shifted(t, front):
    """a contiguous copy of float tensor ``t`` that starts ``front`` floats past a 16-byte boundary"""
    if t is None:
        return None
    buf = torch.full((front + t.numel() + 4,), SENT, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[front:front + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def carve(shape, front, dtype=torch.float32):
    """(buffer of sentinels, the output ``front`` elements past its 16-byte aligned start)"""
    n = int(np.prod(shape))
    buf = torch.full((front + n + BACK,), SENT if dtype == torch.float32 else 777, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[front:front + n].view(shape)


def intact(buf, front):
    assert (buf[:front] == 777).all() and (buf[buf.numel() - BACK:] == 777).all(), "a sentinel around an output changed"


def p(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def raw_reduce(pkg, g, at, values, weight, mode, front, want_arg):
    lib = pkg._aggregate.load()
    ptr, perm, row_ptr, col, _ = g.device(at)
    E, H, D = values.shape
    S = g.B * (g.M if at == "target" else g.Q)
    v, w = shifted(values, front), shifted(weight, front)
    obuf, out = carve((S, H, D), front)
    abuf, arg = carve((S, H, D), front % 2, torch.int64) if want_arg else (None, None)
    rc = lib.ps_segment_reduce_f32(p(v), p(w), p(ptr), p(perm), 0 if perm is None else perm.shape[0], p(row_ptr), p(col), E,
                                   A.MODES.index(mode), p(out), p(arg), g.B, g.Q, g.M, H, D, stream())
    assert rc == 0
    torch.cuda.synchronize()
    intact(obuf, front)
    if want_arg:
        intact(abuf, front % 2)
    return out, arg


def equal_bits(got, want, what):
    want = want if isinstance(want, torch.Tensor) else dev(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert torch.equal(raw(got), raw(want)), f"{what}: not the restatement's bits"


# ---- 1. K55 --------------------------------------------------------------------------------------------------------------------------------
def reduce_case(g, H, D, seed=0):
    rng = np.random.default_rng(1000 * H + D + seed)
    values = np.round(rng.standard_normal((g.E, H, D)) * 4).astype(np.float32) / 4 + \
        (rng.standard_normal((g.E, H, D)) * 1e-3).astype(np.float32) * (rng.random((g.E, H, D)) < 0.5)   # ties for max / min
    weight = rng.standard_normal((g.E, H)).astype(np.float32)
    return g.plant(values.astype(np.float32)), g.plant(weight)


def check_reduce(pkg, g, H, D, fronts):
    ops = pkg.ops
    values, weight = reduce_case(g, H, D)
    dv, dw = dev(values), dev(weight)
    for at in ("source", "target"):
        ptr, perm, S = g.host[at]
        dptr, dperm, row_ptr, col, _ = g.device(at)
        for mode in A.MODES:
            extreme = mode in ("max", "min")
            want, want_arg = A.segment_reduce(values, ptr, perm, S, mode, None if extreme else weight, g.real)
            got = ops.segment_reduce(dv, dptr, dperm, **g.dims(), reduce=mode, weight=None if extreme else dw, row_ptr=row_ptr,
                                     col=col, return_arg=extreme)
            got, got_arg = got if extreme else (got, None)
            what = f"{g.name} ({H},{D}) {mode} at the {at}s"
            assert np.isfinite(want).all(), "NaN at the padding does not surface"
            equal_bits(got, want, what)
            if extreme:
                equal_bits(got_arg, want_arg, what + ", arg")
            for front in fronts:
                out, arg = raw_reduce(pkg, g, at, dv, None if extreme else dw, mode, front, extreme)
                equal_bits(out, got, what + f", {4 * front} bytes off")
                if extreme:
                    equal_bits(arg, got_arg, what + f", arg, {4 * front} bytes off")
        if at == "source":      # no weight, and no col: the padding inside the rows then counts, NaN and all
            plain = np.nan_to_num(values)
            want, _ = A.segment_reduce(plain, ptr, perm, S, "mean")
            equal_bits(ops.segment_reduce(dev(plain), dptr, None, **g.dims(), reduce="mean"), want, f"{g.name} mean without col")


@pytest.mark.parametrize("H,D", ROWS, ids=lambda v: str(v))
def test_segment_reduce_bits(pkg, H, D):
    g = graph("main")
    check_reduce(pkg, g, H, D, fronts=(0, 1, 2, 3))       # 0: the 16-byte arm inside sentinels too
    empty = np.flatnonzero(np.diff(g.row_ptr) == 0)
    assert len(empty) > 10
    values, _ = reduce_case(g, H, D)
    ptr, perm, row_ptr, col, _ = g.device("source")
    out, arg = pkg.ops.segment_reduce(dev(values), ptr, None, **g.dims(), reduce="min", row_ptr=row_ptr, col=col, return_arg=True)
    empty = torch.from_numpy(empty).cuda()
    assert (bits(out[empty]) == 0).all() and (arg[empty] == -1).all(), "an empty segment gives +0 and -1"


@pytest.mark.parametrize("name", OTHER_GRAPHS)
def test_segment_reduce_bits_on_the_other_graphs(pkg, name):
    for H, D in ((3, 4), (1, 5)):
        check_reduce(pkg, graph(name), H, D, fronts=(0, 1))


# ---- 2. K56 and K57 ------------------------------------------------------------------------------------------------------------------------
def check_gather_and_dot(pkg, g, H, D, fronts):
    ops, lib = pkg.ops, pkg._aggregate.load()
    rng = np.random.default_rng(7 * H + D)
    values, weight = reduce_case(g, H, D, seed=5)
    for at in ("source", "target"):
        S = g.host[at][2]
        index = g.index[at]
        node = rng.standard_normal((S, H, D)).astype(np.float32)
        dn, dv, dw, di = dev(node), dev(values), dev(weight), g.device(at)[4]
        what = f"{g.name} ({H},{D}) at the {at}s"
        gathered, copied, dots = ops.segment_gather(dn, di, dw), ops.segment_gather(dn, di), ops.edge_dot(dn, dv, di)
        equal_bits(gathered, A.segment_gather(node, index, weight), what + ": K56 with a weight")
        equal_bits(copied, A.segment_gather(node, index), what + ": K56 without")
        equal_bits(dots, A.edge_dot(node, values, index), what + ": K57")
        assert (bits(gathered[~torch.from_numpy(g.real).cuda()]) == 0).all() and bool(torch.isfinite(dots).all())
        for front in fronts:
            sn, sv, sw = shifted(dn, front), shifted(dv, front), shifted(dw, front)
            buf, out = carve((g.E, H, D), front)
            assert lib.ps_segment_gather_f32(p(sn), p(sw), p(di), g.E, S, H, D, p(out), stream()) == 0
            buf2, out2 = carve((g.E, H), front)
            assert lib.ps_edge_dot_f32(p(sn), p(sv), p(di), g.E, S, H, D, p(out2), stream()) == 0
            torch.cuda.synchronize()
            intact(buf, front), intact(buf2, front)
            equal_bits(out, gathered, what + f": K56 {4 * front} bytes off")
            equal_bits(out2, dots, what + f": K57 {4 * front} bytes off")


@pytest.mark.parametrize("H,D", ROWS, ids=lambda v: str(v))
def test_segment_gather_and_edge_dot_bits(pkg, H, D):
    check_gather_and_dot(pkg, graph("main"), H, D, fronts=(0, 1, 2, 3))


@pytest.mark.parametrize("name", OTHER_GRAPHS)
def test_segment_gather_and_edge_dot_bits_on_the_other_graphs(pkg, name):
    check_gather_and_dot(pkg, graph(name), 3, 4, fronts=(0, 2))


# ---- 3. K58 and K59 ------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "all equal", "one at +1e4", "one at -1e4", "some at -inf", "a row at -inf")


def logits_of(g, family, H, seed=0):
    rng = np.random.default_rng(len(family) + 10 * H + seed)
    x = (rng.standard_normal((g.E, H)) * 3).astype(np.float32)
    starts = g.row_ptr[:-1][np.diff(g.row_ptr) > 2]
    if family == "all equal":
        x[:] = 1.25
    elif family in ("one at +1e4", "one at -1e4"):
        x[np.minimum(starts + 1, g.E - 1)] = 1e4 if "+" in family else -1e4
    elif family == "some at -inf":
        x[rng.random(x.shape) < 0.2] = -np.inf
    elif family == "a row at -inf":
        for s in range(0, len(g.row_ptr) - 1, 3):
            x[g.row_ptr[s]:min(g.row_ptr[s + 1], g.E)] = -np.inf
    return g.plant(x)


def softmax_ratio(w, lse, want_w, want_lse):
    """the worst error / bound of K58: 2^-23 |ref| + 2^-126 for w -- one float32 rounding, doubled for the double exp's own
    error, and the smallest normal for a flushed subnormal --, 2^-23 |ref| for lse"""
    w, lse = w.cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    assert np.isfinite(w).all() and np.array_equal(np.isinf(lse), np.isinf(want_lse)) and not np.isnan(lse).any()
    assert (lse[np.isinf(lse)] < 0).all()
    ratio_w = (np.abs(w - want_w) / (2.0 ** -23 * np.abs(want_w) + 2.0 ** -126)).max()
    finite = np.isfinite(want_lse)
    ratio_lse = (np.abs(lse[finite] - want_lse[finite]) / np.maximum(2.0 ** -23 * np.abs(want_lse[finite]), 1e-300)).max() \
        if finite.any() else 0.0
    exact_zero = np.abs(want_lse[finite]) == 0
    if exact_zero.any():
        assert (lse[finite][exact_zero] == 0).all()
    return ratio_w, ratio_lse


def check_softmax(pkg, g, H, family, fronts):
    ops, lib = pkg.ops, pkg._aggregate.load()
    x = logits_of(g, family, H)
    dx = dev(x)
    rng = np.random.default_rng(3)
    grad = g.plant(rng.standard_normal((g.E, H)).astype(np.float32))
    worst = 0.0
    for at in ("source", "target"):
        ptr, perm, S = g.host[at]
        dptr, dperm, row_ptr, col, index = g.device(at)
        want_w, want_lse = A.segment_softmax(x, ptr, perm, S, g.real)
        w, lse = ops.segment_softmax(dx, dptr, dperm, **g.dims(), row_ptr=row_ptr, col=col, return_lse=True)
        what = f"{g.name} H={H} {family} at the {at}s"
        rw, rl = softmax_ratio(w, lse, want_w, want_lse)
        print(f"K58 {what}: worst error / bound {rw:.3f} (w), {rl:.3f} (lse)")
        assert rw <= 1.0 and rl <= 1.0, what
        worst = max(worst, rw, rl)
        host_w = w.cpu().numpy()
        assert (bits(w[~torch.from_numpy(g.real).cuda()]) == 0).all(), "exact +0 at the padding"
        assert (host_w[(x == -np.inf) & g.real[:, None]] == 0).all(), "a member at -inf gives 0"
        single = np.flatnonzero(np.bincount(index.cpu().numpy()[g.real], minlength=S) == 1)
        for s in single[:20]:
            e = np.flatnonzero(g.index[at] == s)[0]
            assert (host_w[e][np.isfinite(x[e])] == 1.0).all(), "a segment of one member gives exactly 1.0"
        equal_bits(ops.segment_softmax(dx, dptr, dperm, **g.dims(), row_ptr=row_ptr, col=col), w, what + ": without lse")
        # K59, given the kernel's own w
        gx = ops.segment_softmax_backward(w, dev(grad), dptr, dperm, **g.dims(), row_ptr=row_ptr, col=col)
        equal_bits(gx, A.segment_softmax_backward(host_w, grad, ptr, perm, S, g.real), what + ": K59")
        n_perm = 0 if dperm is None else dperm.shape[0]
        for front in fronts:
            sx, sg, sw = shifted(dx, front), shifted(dev(grad), front), shifted(w, front)
            wbuf, w2 = carve((g.E, H), front)
            lbuf, lse2 = carve((S, H), front)
            assert lib.ps_segment_softmax_f32(p(sx), p(dptr), p(dperm), n_perm, p(row_ptr), p(col), g.E, p(w2), p(lse2), g.B, g.Q,
                                              g.M, H, stream()) == 0
            gbuf, gx2 = carve((g.E, H), front)
            assert lib.ps_segment_softmax_backward_f32(p(sw), p(sg), p(dptr), p(dperm), n_perm, p(row_ptr), p(col), g.E, p(gx2),
                                                       g.B, g.Q, g.M, H, stream()) == 0
            torch.cuda.synchronize()
            intact(wbuf, front), intact(lbuf, front), intact(gbuf, front)
            equal_bits(w2, w, what + f": {4 * front} bytes off")
            equal_bits(lse2, lse, what + f": lse {4 * front} bytes off")
            equal_bits(gx2, gx, what + f": K59 {4 * front} bytes off")
    return worst


@pytest.mark.parametrize("family", FAMILIES)
def test_segment_softmax_within_one_rounding_and_its_backward_bits(pkg, family):
    """the worst error / bound ratios printed here are the figures of DESIGN.md section 4"""
    worst = max(check_softmax(pkg, graph("main"), H, family, fronts=(0, 1, 2, 3)) for H in (1, 3, 8))
    print(f"K58 {family}: worst error / bound over H = 1, 3, 8 and both groupings: {worst:.3f}")


@pytest.mark.parametrize("name", OTHER_GRAPHS)
def test_segment_softmax_on_the_other_graphs(pkg, name):
    for family in ("normal", "some at -inf"):
        check_softmax(pkg, graph(name), 2, family, fronts=(0, 3))


# ---- 4. consistency ------------------------------------------------------------------------------------------------------------------------
def as_radius_graph(pkg, g):
    count = np.diff(g.row_ptr).reshape(g.B, g.Q).astype(np.int32)
    return pkg.geometry.RadiusGraph(dev(g.row_ptr), dev(g.col), None, dev(count))


def layer(pkg, rg, logits, values, at, M):
    """the public route, forwards and backwards: (out, w, d logits, d values)"""
    geometry = pkg.geometry
    x, v = logits.clone().requires_grad_(), values.clone().requires_grad_()
    out = geometry.edge_attention(x, v, rg, at=at, n_targets=M)
    seed = torch.Generator(device="cuda").manual_seed(9)
    (out * torch.randn(out.shape, generator=seed, device="cuda")).sum().backward()
    return out.detach(), geometry.edge_softmax(logits, rg, at=at, n_targets=M), x.grad, v.grad


def test_repeats_agree_bit_for_bit_and_a_sub_batch_is_a_block(pkg):
    g = graph("main")
    rg = as_radius_graph(pkg, g)
    rng = np.random.default_rng(8)
    logits = dev(np.nan_to_num(g.plant(rng.standard_normal((g.E, 3)).astype(np.float32))))
    values = dev(rng.standard_normal((g.E, 3, 4)).astype(np.float32))
    for at in ("source", "target"):
        first = layer(pkg, rg, logits, values, at, g.M)
        assert_all_same(layer(pkg, rg, logits, values, at, g.M), first, f"a second run at the {at}s")
        assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in first)
        # structure 1 alone: its rows, its edges
        lo, hi = int(g.row_ptr[g.Q]), int(g.row_ptr[2 * g.Q])
        sub = Graph("sub", 1, g.Q, g.M, g.row_ptr[g.Q:2 * g.Q + 1] - lo, g.col[lo:hi])
        part = layer(pkg, as_radius_graph(pkg, sub), logits[lo:hi], values[lo:hi], at, g.M)
        # the random upstream gradient of ``layer`` depends on the shape: compare what does not, the forward results
        assert same(part[0][0], first[0][1]) and same(part[1], first[1][lo:hi]), f"a sub-batch at the {at}s is not the block"


def test_the_padded_form_and_its_csr_form_agree(pkg):
    geometry = pkg.geometry
    g = graph("padded")
    idx = dev(g.col.reshape(g.B, g.Q, 6))
    rg = geometry.neighbors_to_radius_graph(idx)
    keep = torch.from_numpy(g.col >= 0).cuda()
    rng = np.random.default_rng(12)
    logits = dev(g.plant(rng.standard_normal((g.E, 2)).astype(np.float32)))
    values = dev(g.plant(rng.standard_normal((g.E, 2, 5)).astype(np.float32)))
    node = dev(rng.standard_normal((g.B, g.M, 2, 5)).astype(np.float32))
    for at in ("source", "target"):
        w_pad = geometry.edge_softmax(logits.reshape(g.B, g.Q, 6, 2), idx, at=at)
        w_csr = geometry.edge_softmax(logits[keep], rg, at=at)
        assert w_pad.shape == (g.B, g.Q, 6, 2) and same(w_pad.reshape(-1, 2)[keep], w_csr) and bool((w_pad.reshape(-1, 2)[~keep] == 0).all())
        for reduce in A.MODES:
            a = geometry.edge_aggregate(values.reshape(g.B, g.Q, 6, 2, 5), idx, at=at, reduce=reduce)
            b = geometry.edge_aggregate(values[keep], rg, at=at, reduce=reduce)
            assert a.shape == (g.B, g.Q, 2, 5) and same(a, b), (at, reduce)
        a = geometry.edge_gather(node, idx, at=at)
        assert a.shape == (g.B, g.Q, 6, 2, 5) and same(a.reshape(-1, 2, 5)[keep], geometry.edge_gather(node, rg, at=at))
        assert bool((a.reshape(-1, 2, 5)[~keep] == 0).all())
    # Neighbors, numpy and CPU tensors
    nb = geometry.Neighbors(idx, None, None)
    assert same(geometry.edge_aggregate(values.reshape(g.B, g.Q, 6, 2, 5), nb), geometry.edge_aggregate(values[keep], rg))
    out = geometry.edge_aggregate(values.cpu().numpy().reshape(g.B, g.Q, 6, 2, 5), idx.cpu().numpy(), reduce="mean")
    assert isinstance(out, np.ndarray) and np.array_equal(out, geometry.edge_aggregate(values[keep], rg, reduce="mean").cpu().numpy())
    home = geometry.edge_softmax(logits.cpu()[:, 0].reshape(g.B, g.Q, 6), idx.cpu())
    assert home.device.type == "cpu" and home.shape == (g.B, g.Q, 6)


# ---- 5. the public functions and their gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("main", "bipartite 65x130"))
@pytest.mark.parametrize("at", ("source", "target"))
def test_the_public_functions_and_their_gradients_are_the_restatement(pkg, name, at):
    geometry = pkg.geometry
    g = graph(name)
    rg = as_radius_graph(pkg, g)
    H, D = 2, 6
    rng = np.random.default_rng(21)
    values, weight = reduce_case(g, H, D, seed=2)
    ptr, perm, S = g.host[at]
    nodes = g.M if at == "target" else g.Q
    index = g.index[at]
    up = rng.standard_normal((g.B, nodes, H, D)).astype(np.float32)
    kw = dict(at=at, n_targets=g.M)

    def leaves(*arrays):
        return [dev(a).requires_grad_() for a in arrays]
    # sum with a weight: K55 forwards, K56 and K57 backwards -- NaN at the padding in messages, weights and the result's users
    v, w = leaves(values, weight)
    out = geometry.edge_aggregate(v, rg, weight=w, **kw)
    equal_bits(out.detach().reshape(S, H, D), A.segment_reduce(values, ptr, perm, S, "sum", weight, g.real)[0], "edge_aggregate sum")
    (out * dev(up)).sum().backward()
    equal_bits(v.grad, A.segment_gather(up.reshape(S, H, D), index, weight), "d messages")
    equal_bits(w.grad, A.edge_dot(up.reshape(S, H, D), values, index), "d weight")
    # mean, one weight per edge
    v, w = leaves(values, weight[:, 0])
    out = geometry.edge_aggregate(v, rg, weight=w, reduce="mean", **kw)
    wide = np.repeat(weight[:, :1], H, 1)
    equal_bits(out.detach().reshape(S, H, D), A.segment_reduce(values, ptr, perm, S, "mean", wide, g.real)[0], "edge_aggregate mean")
    (out * dev(up)).sum().backward()
    n = np.maximum(np.bincount(index[g.real], minlength=S), 1).astype(np.float32)
    scaled = (up.reshape(S, H, D) / n[:, None, None]).astype(np.float32)
    equal_bits(v.grad, A.segment_gather(scaled, index, wide), "d messages of the mean")
    assert bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0 and w.grad.shape == (g.E,)
    # max: the gradient goes to arg
    (v,) = leaves(values)
    out, arg = geometry.edge_aggregate(v, rg, reduce="max", return_arg=True, **kw)
    want, want_arg = A.segment_reduce(values, ptr, perm, S, "max", None, g.real)
    equal_bits(out.detach().reshape(S, H, D), want, "edge_aggregate max")
    equal_bits(arg.reshape(S, H, D), want_arg, "arg")
    (out * dev(up)).sum().backward()
    grad = np.zeros((g.E, H, D), np.float32)
    for s, h, d in zip(*np.nonzero(want_arg >= 0)):
        grad[want_arg[s, h, d], h, d] = up.reshape(S, H, D)[s, h, d]
    equal_bits(v.grad, grad, "d messages of the max")
    # (E, C) messages are one head
    flat = geometry.edge_aggregate(dev(values).reshape(g.E, H * D), rg, reduce="min", **kw)
    equal_bits(flat.reshape(S, H, D), A.segment_reduce(values, ptr, perm, S, "min", None, g.real)[0], "(E, C) messages")
    # gather: K56 forwards, K55 at the same end and K57 backwards
    node = rng.standard_normal((g.B, nodes, H, D)).astype(np.float32)
    upe = g.plant(rng.standard_normal((g.E, H, D)).astype(np.float32))
    nd, w = leaves(node, weight)
    out = geometry.edge_gather(nd, rg, weight=w, **kw)
    equal_bits(out.detach(), A.segment_gather(node.reshape(S, H, D), index, weight), "edge_gather")
    out.backward(dev(upe))
    equal_bits(nd.grad.reshape(S, H, D), A.segment_reduce(upe, ptr, perm, S, "sum", weight, g.real)[0], "d values of the gather")
    equal_bits(w.grad, A.edge_dot(node.reshape(S, H, D), upe, index), "d weight of the gather")
    # softmax: K58 forwards, K59 backwards
    x = logits_of(g, "some at -inf", H, seed=4)
    (lx,) = leaves(x)
    w_out, lse = geometry.edge_softmax(lx, rg, return_lse=True, **kw)
    assert not lse.requires_grad and lse.shape == (g.B, nodes, H) and w_out.requires_grad
    upw = g.plant(rng.standard_normal((g.E, H)).astype(np.float32))
    w_out.backward(dev(upw))
    equal_bits(lx.grad, A.segment_softmax_backward(w_out.detach().cpu().numpy(), upw, ptr, perm, S, g.real), "d logits")
    with torch.no_grad():
        assert not geometry.edge_softmax(lx, rg, **kw).requires_grad
    assert not geometry.edge_aggregate(dev(values), rg, **kw).requires_grad


# ---- 5b. a padded list whose targets are not its queries, and a graph without edges -------------------------------------------------------
@pytest.mark.parametrize("Q,M,k", ((1, 64, 70), (65, 130, 5)))
@pytest.mark.parametrize("at", ("source", "target"))
def test_a_padded_bipartite_list_through_the_four_public_functions(pkg, Q, M, k, at):
    """a (B,Q,k) list of ``nearest_neighbors(points, k, queries=...)``: its rows are the Q queries, its indices name M
    targets.  Every function at both ends against the restatement on the CSR list ``arange(B*Q + 1) * k``"""
    geometry = pkg.geometry
    B, H, D = 2, 2, 5
    rng = np.random.default_rng(100 * Q + M)
    idx = rng.integers(0, M, size=(B, Q, k)).astype(np.int32)
    idx[rng.random(idx.shape) < 0.25] = -1
    g = Graph(f"padded {Q}x{M}", B, Q, M, np.arange(B * Q + 1, dtype=np.int64) * k, idx.reshape(-1))
    ptr, perm, S = g.host[at]
    index, nodes = g.index[at], (M if at == "target" else Q)
    assert g.real.sum() > 0.5 * g.E and not g.real.all() and S == B * nodes
    values, weight = reduce_case(g, H, D, seed=7)
    x = logits_of(g, "normal", H, seed=7)
    node = rng.standard_normal((B, nodes, H, D)).astype(np.float32)
    up = rng.standard_normal((B, nodes, H, D)).astype(np.float32)
    kw = dict(at=at, n_targets=M)
    edge = (B, Q, k)
    didx = dev(idx)
    # edge_aggregate: the weighted sum, and the maximum with its positions (flat over (B,Q,k))
    out = geometry.edge_aggregate(dev(values).reshape(*edge, H, D), didx, weight=dev(weight).reshape(*edge, H), **kw)
    assert out.shape == (B, nodes, H, D)
    equal_bits(out.reshape(S, H, D), A.segment_reduce(values, ptr, perm, S, "sum", weight, g.real)[0], "edge_aggregate sum")
    best, arg = geometry.edge_aggregate(dev(values).reshape(*edge, H, D), didx, reduce="max", return_arg=True, **kw)
    want, want_arg = A.segment_reduce(values, ptr, perm, S, "max", None, g.real)
    equal_bits(best.reshape(S, H, D), want, "edge_aggregate max")
    equal_bits(arg.reshape(S, H, D), want_arg, "edge_aggregate arg")
    mean = geometry.edge_aggregate(dev(values).reshape(*edge, H, D), didx, reduce="mean", **kw)
    equal_bits(mean.reshape(S, H, D), A.segment_reduce(values, ptr, perm, S, "mean", None, g.real)[0], "edge_aggregate mean")
    # edge_gather: M is read off values at the target, and given at the source
    got = geometry.edge_gather(dev(node), didx, weight=dev(weight).reshape(*edge, H), **kw)
    assert got.shape == (*edge, H, D)
    equal_bits(got.reshape(g.E, H, D), A.segment_gather(node.reshape(S, H, D), index, weight), "edge_gather")
    assert float(got.reshape(g.E, H, D)[-k:].abs().max()) > 0, "the last row is served, not taken for a tail"
    # edge_softmax, then edge_attention with its gradients, on the kernel's own weights
    w, lse = geometry.edge_softmax(dev(x).reshape(*edge, H), didx, return_lse=True, **kw)
    assert w.shape == (*edge, H) and lse.shape == (B, nodes, H)
    want_w, want_lse = A.segment_softmax(x, ptr, perm, S, g.real)
    rw, rl = softmax_ratio(w.reshape(g.E, H), lse.reshape(S, H), want_w, want_lse)
    assert rw <= 1.0 and rl <= 1.0
    w32 = w.reshape(g.E, H).cpu().numpy()
    lx, lv = dev(x).reshape(*edge, H).requires_grad_(), dev(values).reshape(*edge, H, D).requires_grad_()
    att = geometry.edge_attention(lx, lv, didx, **kw)
    equal_bits(att.detach().reshape(S, H, D), A.segment_reduce(values, ptr, perm, S, "sum", w32, g.real)[0], "edge_attention")
    (att * dev(up)).sum().backward()
    ups = up.reshape(S, H, D)
    equal_bits(lv.grad.reshape(g.E, H, D), A.segment_gather(ups, index, w32), "d values")
    equal_bits(lx.grad.reshape(g.E, H), A.segment_softmax_backward(w32, A.edge_dot(ups, values, index), ptr, perm, S, g.real),
               "d logits")
    # the same list in CSR form, which never went through the padded route
    rg = geometry.neighbors_to_radius_graph(didx)
    keep = torch.from_numpy(g.real).cuda()
    assert same(geometry.edge_aggregate(dev(values)[keep], rg, weight=dev(weight)[keep], **kw), out)


def test_a_graph_without_edges(pkg):
    """E == 0 -- ``radius_graph`` without ``max_edges`` on points further apart than the cutoff: zeros, -1 and -inf of the right
    shapes from all four functions, at both ends, with and without a graph to differentiate"""
    geometry = pkg.geometry
    B, N, H, D = 2, 5, 3, 4
    points = torch.arange(B * N * 3, dtype=torch.float32, device="cuda").reshape(B, N, 3) * 100.0
    g = geometry.radius_graph(points, 1.0)
    assert g.col.shape == (0,)
    for at in ("source", "target"):
        for grad in (False, True):
            x = torch.zeros(0, H, device="cuda", requires_grad=grad)
            v = torch.zeros(0, H, D, device="cuda", requires_grad=grad)
            node = torch.ones(B, N, H, D, device="cuda", requires_grad=grad)
            w, lse = geometry.edge_softmax(x, g, at=at, return_lse=True)
            assert w.shape == (0, H) and lse.shape == (B, N, H) and bool((lse == float("-inf")).all())
            assert geometry.edge_softmax(x[:, 0], g, at=at).shape == (0,)
            for reduce in A.MODES:
                out = geometry.edge_aggregate(v, g, at=at, reduce=reduce, weight=None if reduce in ("max", "min") else x)
                assert out.shape == (B, N, H, D) and bool((bits(out) == 0).all())
                if grad:
                    out.sum().backward()
                    assert v.grad.shape == (0, H, D)
            out, arg = geometry.edge_aggregate(v.reshape(0, H * D), g, at=at, reduce="min", return_arg=True)
            assert out.shape == (B, N, H * D) and bool((arg == -1).all())
            att = geometry.edge_attention(x, v, g, at=at)
            assert att.shape == (B, N, H, D) and bool((bits(att) == 0).all())
            assert geometry.edge_attention(x[:, 0], v.reshape(0, H * D), g, at=at).shape == (B, N, H * D)
            got = geometry.edge_gather(node, g, at=at, weight=x)
            assert got.shape == (0, H, D)
            if grad:
                (att.sum() + got.sum()).backward()
                assert bool((node.grad == 0).all()) and x.grad.shape == (0, H)


# ---- 6. end to end on the PDB files -------------------------------------------------------------------------------------------------------
def attention_end_to_end(pkg, batch, graph_obj, rbf, what):
    """rbf (edges..., 400) -> logits (H) and values (H, D) by seeded weights -> edge_attention -> a scalar -> backward().  Each
    stage is held to the restatement on the stage's own inputs, bit for bit (K58: its bound), and the whole to float64
    autograd of the composed route on the same float32 logits and values within the bound derived below."""
    geometry = pkg.geometry
    H, D = 4, 8
    seed = torch.Generator(device="cuda").manual_seed(31)
    w_logit = torch.randn(400, H, generator=seed, device="cuda") * 0.3
    w_value = torch.randn(400, H * D, generator=seed, device="cuda") * 0.2
    edge_shape = rbf.shape[:-1]
    logits = (rbf @ w_logit).detach().requires_grad_()
    values = (rbf @ w_value).reshape(*edge_shape, H, D).detach().requires_grad_()
    out = geometry.edge_attention(logits, values, graph_obj)
    w_up = torch.randn(out.shape, generator=seed, device="cuda")
    (out * w_up).sum().backward()
    w_gpu = geometry.edge_softmax(logits.detach(), graph_obj)
    torch.cuda.synchronize()
    # the list as CSR lists on the host
    B, N = batch.xyz.shape[:2]
    if isinstance(graph_obj, geometry.RadiusGraph):
        row_ptr, col = graph_obj.row_ptr.cpu().numpy(), graph_obj.col.cpu().numpy()
    else:
        k = graph_obj.idx.shape[2]
        row_ptr, col = np.arange(B * N + 1, dtype=np.int64) * k, graph_obj.idx.cpu().numpy().reshape(-1)
    E = len(col)
    real = A.real_positions(row_ptr, col, N)
    index = A.edge_index(row_ptr, col, N, N, "source")
    x, v = logits.detach().cpu().numpy().reshape(E, H), values.detach().cpu().numpy().reshape(E, H, D)
    up = w_up.cpu().numpy().reshape(B * N, H, D)
    w32 = w_gpu.cpu().numpy().reshape(E, H)
    S = B * N
    # stage by stage
    want_w, _ = A.segment_softmax(x, row_ptr, None, S, real)
    ratio = (np.abs(w32 - want_w) / (2.0 ** -23 * np.abs(want_w) + 2.0 ** -126)).max()
    print(f"{what}: {E} edges, K58 worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    equal_bits(out.detach().reshape(S, H, D), A.segment_reduce(v, row_ptr, None, S, "sum", w32, real)[0], what + ": the output")
    equal_bits(values.grad.reshape(E, H, D), A.segment_gather(up, index, w32), what + ": d values")
    g_w = A.edge_dot(up, v, index)
    equal_bits(logits.grad.reshape(E, H), A.segment_softmax_backward(w32, g_w, row_ptr, None, S, real), what + ": d logits")
    # the whole against float64 autograd of the composed route: a per-segment softmax by index ops, a weighted index_add.
    # Bounds (u = 2^-24): w carries 2u relative (its rounding and exp's last bit), so
    #   out:       2u sum_e |w_e v_e| for the weights, u |out| for the one rounding of the sum (held in double);
    #   d values:  w g rounded once from a w that carries 2u: 3u |ref|;
    #   d logits:  gx = w (g - t), g = K57 rounded once (u a, a = sum_d |up v|), t = sum w g carries 3u T, T = sum_e w_e a_e;
    #              w's 2u on the product (|g - t| <= a + T) and the final u: u (w (4 a + 6 T) + |gx|) covers the sum
    tx, tv = torch.from_numpy(x.astype(np.float64)).requires_grad_(), torch.from_numpy(v.astype(np.float64)).requires_grad_()
    treal, tindex = torch.from_numpy(real), torch.from_numpy(np.maximum(index, 0))
    neg = torch.full((S, H), -np.inf, dtype=torch.float64)
    m = neg.scatter_reduce(0, tindex[treal][:, None].expand(-1, H), tx[treal].detach(), "amax", include_self=True)
    ex = torch.where(treal[:, None], torch.exp(tx - m[tindex]), torch.zeros((), dtype=torch.float64))
    total = torch.zeros(S, H, dtype=torch.float64).index_add(0, tindex[treal], ex[treal])
    w64 = torch.where(treal[:, None], ex / total[tindex], torch.zeros((), dtype=torch.float64))
    out64 = torch.zeros(S, H, D, dtype=torch.float64).index_add(0, tindex[treal], (w64[:, :, None] * tv)[treal])
    (out64 * torch.from_numpy(up).double()).sum().backward()
    u = 2.0 ** -24
    mass = torch.zeros(S, H, D, dtype=torch.float64).index_add(0, tindex[treal], (w64[:, :, None] * tv).abs()[treal]).detach().numpy()
    tiny = 1e-37          # the float32 subnormals: a product below the smallest normal is rounded absolutely, not relatively
    err = np.abs(out.detach().cpu().numpy().reshape(S, H, D) - out64.detach().numpy())
    worst_out = (err / (2 * u * mass + u * np.abs(out64.detach().numpy()) + tiny)).max()
    err = np.abs(values.grad.cpu().numpy().reshape(E, H, D) - tv.grad.numpy())
    worst_v = (err / (3 * u * np.abs(tv.grad.numpy()) + tiny)).max()
    a = np.abs(up[np.maximum(index, 0)] * v).sum(-1) * real[:, None]
    T = np.zeros((S, H))
    np.add.at(T, index[real], (w64.detach().numpy() * a)[real])
    bound = u * (w64.detach().numpy() * (4 * a + 6 * T[np.maximum(index, 0)]) + np.abs(tx.grad.numpy())) + tiny
    worst_x = (np.abs(logits.grad.cpu().numpy().reshape(E, H) - tx.grad.numpy()) / bound).max()
    print(f"{what}: against float64 autograd, worst error / bound {worst_out:.3f} (out), {worst_v:.3f} (d values), {worst_x:.3f} (d logits)")
    assert worst_out <= 1.0 and worst_v <= 1.0 and worst_x <= 1.0
    assert float(logits.grad.abs().max()) > 0 and bool((logits.grad.reshape(E, H)[~treal.cuda()] == 0).all())


def test_pdb_attention_layer_on_the_radius_graph(pkg):
    batch = pdb_batch()
    g = batch.radius_graph(10.0)
    attention_end_to_end(pkg, batch, g, batch.edge_features(graph=g).rbf, "radius_graph(10.0)")


def test_pdb_attention_layer_on_the_knn_graph(pkg):
    batch = pdb_batch()
    nb = batch.knn_graph(30)
    attention_end_to_end(pkg, batch, nb, batch.edge_features(graph=nb).rbf, "knn_graph(30)")


# ---- 7. the launch contract ----------------------------------------------------------------------------------------------------------------
CONTRACT_EDGES = 1500
CONTRACT_N, CONTRACT_B, CONTRACT_H, CONTRACT_D = 37, 5, 4, 8
SYMBOLS = ("ps_edge_dot_f32", "ps_segment_gather_f32", "ps_segment_reduce_f32", "ps_segment_softmax_backward_f32",
           "ps_segment_softmax_f32")


def _contract_inputs(v):
    rng = np.random.default_rng(60 if v == "A" else 61)
    points = (rng.standard_normal((CONTRACT_B, CONTRACT_N, 3)) * 6.0).astype(np.float32)
    logits = rng.standard_normal((CONTRACT_EDGES, CONTRACT_H)).astype(np.float32)
    values = rng.standard_normal((CONTRACT_EDGES, CONTRACT_H, CONTRACT_D)).astype(np.float32)
    return dict(points=torch.from_numpy(points), logits=torch.from_numpy(logits), values=torch.from_numpy(values))


def _contract_state(inputs):
    """device copies that a test may overwrite in place: the points, and the leaves of the layer"""
    return dict(points=inputs["points"].cuda().clone(), logits=inputs["logits"].cuda().clone().requires_grad_(),
                values=inputs["values"].cuda().clone().requires_grad_())


def _contract_run(state):
    """radius_graph(max_edges=n) -> edge_attention at the sources and at the targets -> the gradients: no host read"""
    from protstruc_amd import geometry
    g = geometry.radius_graph(state["points"], 7.0, max_edges=CONTRACT_EDGES)
    out = geometry.edge_attention(state["logits"], state["values"], g)
    back = geometry.edge_attention(state["logits"], state["values"], g, at="target")
    loss = (out * out).sum() + (back * back).sum()
    d_logits, d_values = torch.autograd.grad(loss, (state["logits"], state["values"]))
    return (out.detach(), back.detach(), d_logits, d_values, g.row_ptr)


def _contract_load(state, inputs):
    """``inputs`` -- tensors already on the device -- over the state, in place, on the current stream"""
    with torch.no_grad():
        for name in ("points", "logits", "values"):
            state[name].copy_(inputs[name])


def _on_device(inputs):
    return {name: t.cuda() for name, t in inputs.items()}


@functools.lru_cache(maxsize=None)
def contract_eager(v):
    outs = _contract_run(_contract_state(_contract_inputs(v)))
    torch.cuda.synchronize()
    return outs


def test_contract_case_reaches_the_five_symbols_and_repeats_bit_for_bit(pkg, monkeypatch):
    seen = []
    launch = pkg.ops._launch_aggregate
    monkeypatch.setattr(pkg.ops, "_launch_aggregate", lambda name, *args: (seen.append(name), launch(name, *args))[1])
    outs = _contract_run(_contract_state(_contract_inputs("A")))
    torch.cuda.synchronize()
    assert tuple(sorted(set(seen))) == SYMBOLS
    a, b = contract_eager("A"), contract_eager("B")
    for again in (outs, _contract_run(_contract_state(_contract_inputs("A")))):
        assert_all_same(again, a, "a second run")
    for k in range(5):
        assert not same(a[k], b[k]), f"output {k} is the same for both variants"
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in a[:4])
    assert 200 < int(a[4][-1]) < CONTRACT_EDGES and 200 < int(b[4][-1]) < CONTRACT_EDGES, "the buffers leave a tail and cut nothing"


def test_launches_on_the_callers_stream(pkg):
    want_a, want_b = contract_eager("A"), contract_eager("B")
    a, b = _contract_inputs("A"), _contract_inputs("B")
    state = _contract_state(a)
    new = _on_device(b)                                                 # staged before the sleep: a host copy would wait for it
    side = side_stream_beside_the_default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        _contract_load(state, new)
    control = state["values"].detach().clone()                         # the default stream: runs while the side stream sleeps
    with torch.cuda.stream(side):
        outs = _contract_run(state)
    torch.cuda.synchronize()
    if not same(control, a["values"].cuda()):
        pytest.fail("inconclusive -- the control clone did not see variant A")
    assert_all_same(outs, want_b, "on a side stream")
    assert not same(outs[0], want_a[0]), "the layer was computed from the inputs as they were before the side stream's copy"


def test_forward_and_backward_inside_a_captured_graph(pkg):
    """radius_graph(max_edges=n) -> edge_attention at both ends -> the gradients, captured on variant A after one eager call
    and replayed twice on new inputs over overwritten outputs: no host read anywhere, the incoming lists included"""
    want_a, want_b = contract_eager("A"), contract_eager("B")
    state = _contract_state(_contract_inputs("A"))
    _contract_run(state)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(captured, stream=side):
            outs = _contract_run(state)
    torch.cuda.synchronize()
    for replay, (v, want) in enumerate((("B", want_b), ("A", want_a))):
        _contract_load(state, _on_device(_contract_inputs(v)))
        for o in outs:
            raw(o).fill_(SENTINEL)
        captured.replay()
        torch.cuda.synchronize()
        assert_all_same(outs, want, f"replay {replay + 1}, variant {v}")


def test_four_threads_on_four_streams(pkg):
    rounds, n_threads = 3, 4
    want = {v: contract_eager(v) for v in "AB"}
    mine = [_contract_state(_contract_inputs("AB"[t % 2])) for t in range(n_threads)]
    streams = [torch.cuda.Stream() for _ in range(n_threads)]
    torch.cuda.synchronize()
    gate = threading.Barrier(n_threads)
    failures = []

    def work(t):
        try:
            gate.wait(timeout=60)
            with torch.cuda.stream(streams[t]):
                for r in range(rounds):
                    outs = _contract_run(mine[t])
                    streams[t].synchronize()
                    for k, (o, w) in enumerate(zip(outs, want["AB"[t % 2]])):
                        if not same(o, w):
                            failures.append(f"thread {t}, round {r}: output {k} differs from the serial result")
        except Exception as exc:  # noqa: BLE001 -- reported by the main thread
            failures.append(f"thread {t}: {type(exc).__name__}: {exc}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not failures, failures[:10]


def test_batch_limit(pkg):
    """B = 65535 with Q = 1 against M = 3 targets: structure b is structure b % 3, and every result is that of the three,
    bit for bit"""
    geometry = pkg.geometry
    B, H, D = 65535, 2, 3
    rng = np.random.default_rng(14)
    lengths3 = np.array([2, 0, 3])
    cols3 = [np.array([2, 0]), np.array([], dtype=np.int64), np.array([0, 1, 2])]
    logits3, values3 = rng.standard_normal((5, H)).astype(np.float32), rng.standard_normal((5, H, D)).astype(np.float32)

    def run(reps):
        pk = np.arange(reps) % 3
        row_ptr = np.concatenate([[0], np.cumsum(lengths3[pk])]).astype(np.int64)
        col = np.concatenate([cols3[q] for q in pk]).astype(np.int32)
        rg = geometry.RadiusGraph(dev(row_ptr), dev(col), None, dev(lengths3[pk].reshape(reps, 1).astype(np.int32)))
        x = dev(logits3).repeat(reps // 3, 1).requires_grad_()
        v = dev(values3).repeat(reps // 3, 1, 1).requires_grad_()
        out = geometry.edge_attention(x, v, rg, n_targets=3)
        back = geometry.edge_aggregate(v, rg, at="target", n_targets=3, reduce="max")
        ((out * out).sum() + back.sum()).backward()
        torch.cuda.synchronize()
        return out.detach(), back.detach(), x.grad, v.grad
    small, big = run(3), run(B)
    for name, three, got in zip(("out", "max at the targets", "logits.grad", "values.grad"), small, big):
        assert float(three.abs().max()) > 0 and got.shape[0] == three.shape[0] * (B // 3)
        assert same(got, three.repeat(B // 3, *([1] * (three.ndim - 1)))), f"{name} at B = 65535 is not the B = 3 result repeated"
