#!/usr/bin/python3
"""Time message passing on graphs (ops.segment_reduce, K55; ops.segment_gather, K56; ops.edge_dot, K57;
ops.segment_softmax, K58; ops.segment_softmax_backward, K59; geometry.edge_attention forwards and backwards) and write
profiles/aggregate_time.json.

    python3 tools/aggregate_time.py [--outdir DIR]

Shapes, both at B = 128:
  k48        the padded kNN graph of tools/edge_time.py (N = 512, k = 48) as the CSR list it is, with H = 8 heads of D = 16
  atoms_5A   the all-atom 5 A radius graph of tools/radius_time.py (M = 7680, own residue excluded) with C = 32 (H = 1)
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20): every kernel at the sources and at the targets;
          ``scratch.copy_(messages)`` on the same buffers and the same copy of the REAL rows alone (the kernels read nothing
          at the padding, and 45 % of the kNN list's queries are masked), the floors; the incoming lists; and the whole
          ``geometry.edge_attention`` forwards and backwards.  ``real_edges`` and ``real_message_bytes`` count what is no
          padding, and the rates of K55 are of those bytes.  Lists are not split, so the median and the maximum number of
          real members of a list stand beside every time
  torch   the composed float32 route at the same batch -- ``index_add_`` for the sum, ``scatter_reduce`` for the maximum, a
          scatter softmax (amax, exp, index_add_, divide) and the attention layer forwards and backwards -- at the largest
          batch (B, B / 2, ...) that fits, with the allocator's peak

No ratio is fixed in advance and no speed is asserted here.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import edge_grad_time, edge_time
from tools.steps import largest_batch_that_fits, main, timed

B = edge_time.B
SHAPES = {"k48": (8, 16), "atoms_5A": (1, 32)}      # (H, D)
STEP_TIMEOUT_S = {"events": 400, "torch": 500}


def lists(shape, batch):
    """(row_ptr, col, Q = M) of the shape's graph on the GPU"""
    _, _, row_ptr, col, _, _, _, _ = edge_grad_time.inputs(shape, batch)
    return row_ptr, col, (row_ptr.shape[0] - 1) // batch


def real_positions(row_ptr, col, M):
    """bool (E,): the positions that are no padding"""
    import torch
    return (torch.arange(col.shape[0], device=col.device) < row_ptr[-1]) & (col >= 0) & (col < M)


def node_index(row_ptr, col, batch, M, at):
    """(E,) int64: the flat node of every edge position at that end, -1 at the padding (what the public functions build)"""
    import torch
    from protstruc_amd import ops
    b, row = ops.csr_edge_rows(row_ptr, M, col.shape[0])
    flat = b.long() * M + (col.long() if at == "target" else row.long())
    return torch.where(real_positions(row_ptr, col, M), flat, torch.full_like(flat, -1))


def lengths(ptr, perm, real):
    """the REAL members per segment: median and maximum, over all segments and over those that have any"""
    import torch
    flags = real if perm is None else real[perm]
    total = torch.cat([torch.zeros(1, dtype=torch.int64, device=real.device), torch.cumsum(flags.long(), 0)])
    n = (total[ptr[1:].clamp(0, flags.shape[0])] - total[ptr[:-1].clamp(0, flags.shape[0])]).float()
    some = n[n > 0]
    return {"median": float(torch.median(n)), "max": float(n.max()), "median_of_non_empty": float(torch.median(some)),
            "empty_segments": int((n == 0).sum()), "segments": int(n.numel())}


def step_events(outdir):
    import torch
    from protstruc_amd import geometry, ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "shapes": {}}
    for shape, (H, D) in SHAPES.items():
        row_ptr, col, M = lists(shape, B)
        E = col.shape[0]
        dims = dict(B=B, Q=M, M=M)
        messages = torch.randn(E, H, D, device="cuda")
        logits, weight = torch.randn(E, H, device="cuda"), torch.rand(E, H, device="cuda")
        real = real_positions(row_ptr, col, M)
        n_real = int(real.sum())
        entry = {"M": M, "H": H, "D": D, "edges": E, "message_bytes": messages.numel() * 4, "real_edges": n_real,
                 "real_message_bytes": n_real * H * D * 4}
        scratch = torch.empty_like(messages)
        entry["copy_of_messages"] = timed(lambda: scratch.copy_(messages))
        entry["copy_of_real_rows"] = timed(lambda: scratch[:n_real].copy_(messages[:n_real]))   # as many bytes, contiguous
        del scratch
        entry["incoming_lists"] = timed(lambda: ops.csr_incoming_edges(row_ptr, col, B, M, M))
        graph = geometry.RadiusGraph(row_ptr, col, None, torch.zeros(B, M, dtype=torch.int32, device="cuda"))
        for at in ("source", "target"):
            ptr, perm = (row_ptr, None) if at == "source" else ops.csr_incoming_edges(row_ptr, col, B, M, M)
            kw = dict(row_ptr=row_ptr, col=col, **dims)
            one = {"list_length": lengths(ptr, perm, real)}
            for mode in ("sum", "mean", "max"):
                one["k55_" + mode] = timed(lambda: ops.segment_reduce(messages, ptr, perm, reduce=mode, **kw))
            one["k55_sum_weighted"] = timed(lambda: ops.segment_reduce(messages, ptr, perm, weight=weight, **kw))
            one["k55_sum_over_copy_of_real_rows"] = one["k55_sum"]["median_us"] / entry["copy_of_real_rows"]["median_us"]
            one["k55_sum_read_GB_per_s"] = entry["real_message_bytes"] / one["k55_sum"]["median_us"] * 1e-3
            index = node_index(row_ptr, col, B, M, at)
            node = torch.randn(B * M, H, D, device="cuda")
            one["k56"] = timed(lambda: ops.segment_gather(node, index))
            one["k56_weighted"] = timed(lambda: ops.segment_gather(node, index, weight))
            one["k57"] = timed(lambda: ops.edge_dot(node, messages, index))
            one["k58"] = timed(lambda: ops.segment_softmax(logits, ptr, perm, **kw))
            w = ops.segment_softmax(logits, ptr, perm, **kw)
            one["k59"] = timed(lambda: ops.segment_softmax_backward(w, weight, ptr, perm, **kw))
            x, v = logits.clone().requires_grad_(), messages.clone().requires_grad_()
            one["edge_attention_forward"] = timed(lambda: geometry.edge_attention(logits, messages, graph, at=at), 2, 10)
            up = torch.randn(B, M, H, D, device="cuda")

            def both():
                x.grad = v.grad = None
                geometry.edge_attention(x, v, graph, at=at).backward(up)

            one["edge_attention_forward_backward"] = timed(both, 2, 10)
            entry[at] = one
            del node, index, w, x, v, up
        report["shapes"][shape] = entry
        del messages, logits, weight, row_ptr, col, graph, real
        torch.cuda.empty_cache()
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "aggregate_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def composed_softmax(logits, index, S):
    """the scatter softmax a user writes today: four passes with temporaries"""
    import torch
    H = logits.shape[1]
    at = index[:, None].expand(-1, H)
    m = torch.full((S, H), float("-inf"), device=logits.device).scatter_reduce(0, at, logits, "amax")
    e = torch.exp(logits - m[index])
    return e / torch.zeros(S, H, device=logits.device).index_add_(0, index, e)[index]


def step_torch(outdir):
    import torch
    entries = {}
    for shape, (H, D) in SHAPES.items():
        def measure(b):
            row_ptr, col, M = lists(shape, b)
            S = b * M
            real = real_positions(row_ptr, col, M)
            E = col.shape[0]
            messages, logits = torch.randn(E, H, D, device="cuda"), torch.randn(E, H, device="cuda")
            up = torch.randn(S, H, D, device="cuda")
            out = {"edges_at_that_batch": int(E)}
            for at in ("source", "target"):
                index = node_index(row_ptr, col, b, M, at)[real]
                msg, lg = messages[real], logits[real]
                wide = index[:, None, None].expand(-1, H, D)
                one = {"index_add_sum": timed(lambda: torch.zeros(S, H, D, device="cuda").index_add_(0, index, msg), 1, 5),
                       "scatter_reduce_amax": timed(lambda: torch.zeros(S, H, D, device="cuda").scatter_reduce(
                           0, wide, msg, "amax", include_self=False), 1, 5),
                       "scatter_softmax": timed(lambda: composed_softmax(lg, index, S), 1, 5)}
                x, v = lg.clone().requires_grad_(), msg.clone().requires_grad_()

                def both():
                    x.grad = v.grad = None
                    w = composed_softmax(x, index, S)
                    torch.zeros(S, H, D, device="cuda").index_add(0, index, w[:, :, None] * v).backward(up)

                one["attention_forward_backward"] = timed(both, 1, 3)
                out[at] = one
            return out

        entries[shape] = largest_batch_that_fits(B, measure)
    print(json.dumps(entries), flush=True)
    with open(os.path.join(outdir, "aggregate_time_torch.json"), "w") as f:
        json.dump(entries, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "aggregate_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "aggregate_time_torch.json")) as f:
        entries = json.load(f)
    for shape, c in entries.items():
        report["shapes"][shape]["composed_torch"] = c
        for at in ("source", "target"):
            if c.get("batch"):
                report["shapes"][shape][at]["composed_over_fused_attention"] = \
                    c[at]["attention_forward_backward"]["median_us"] * (B / c["batch"]) / \
                    report["shapes"][shape][at]["edge_attention_forward_backward"]["median_us"]
    os.remove(os.path.join(outdir, "aggregate_time_events.json"))
    os.remove(os.path.join(outdir, "aggregate_time_torch.json"))
    with open(os.path.join(outdir, "aggregate_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
