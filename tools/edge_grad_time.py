#!/usr/bin/python3
"""Time the backward kernels of the edge features (ops.csr_edge_rbf_backward, K52; ops.csr_edge_pair_grad_sum, K53;
ops.csr_edge_frames_backward, K54; ops.csr_incoming_edges) and write profiles/edge_grad_time.json.

    python3 tools/edge_grad_time.py [--outdir DIR]

Shapes, all at B = 128:
  k48, k30   the padded kNN graphs of tools/edge_time.py (N = 512, 15 atom slots, 45 % of the slots masked, P = 25, R = 16)
             as the CSR lists the backward kernels take them as: row_ptr = arange(B*N + 1) * k, col = idx.reshape(-1)
  atoms_5A   the all-atom graph of tools/csr_edge_time.py (M = 7680, own residue excluded, P = 1, R = 16)
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20): K52 into one buffer with a random ``g_rbf``;
          ``scratch.copy_(g_rbf)`` on K52's own input, the traffic yardstick (it reads what K52 reads and writes as much
          again); the incoming lists; K53; K54 on the N-CA-C frames (the residue graphs); and the whole differentiable call,
          ``geometry.*_edge_distance_features`` forwards and backwards
  torch   the composed float32 route forwards and backwards -- ``rbf.backward(g_rbf)`` down to ``xyz.grad`` -- at the largest
          batch (B, B / 2, ...) that fits, with the allocator's peak

The one comparison the project asks of this tool is ``composed_over_fused``: composed torch's forward + backward, scaled to
the full batch, over the fused forward + backward.  No speed is asserted here.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import csr_edge_time, edge_time
from tools.steps import largest_batch_that_fits, main, timed

B = edge_time.B
SHAPES = ("k48", "k30", "atoms_5A")
STEP_TIMEOUT_S = {"events": 400, "torch": 500}


def inputs(shape, batch):
    """(xyz (batch,M,A',3), atom mask, row_ptr, col, idx or None, pairs, centers, sigma) on the GPU"""
    import torch
    from protstruc_amd import ops
    if shape == "atoms_5A":
        points, pmask, key, cutoff, xyz, amask, pairs, centers, sigma = csr_edge_time.inputs(shape, batch)
        row_ptr, col, _, _ = ops.radius_graph(points, cutoff, pmask, exclude=key)
        return xyz, amask, row_ptr, col, None, pairs, centers, sigma
    xyz, mask, idx = edge_time.inputs(edge_time.SHAPES[shape], batch)
    pairs, centers, sigma = edge_time.tables()
    k = idx.shape[2]
    row_ptr = torch.arange(batch * edge_time.N + 1, dtype=torch.int64, device="cuda") * k
    return xyz, mask, row_ptr, idx.reshape(-1), idx, pairs, centers, sigma


def step_events(outdir):
    import ctypes

    import torch
    from protstruc_amd import _edgegrad, geometry, ops
    lib = _edgegrad.load()
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "shapes": {}}
    stream = torch.cuda.current_stream().cuda_stream
    for shape in SHAPES:
        xyz, amask, row_ptr, col, idx, pairs, centers, sigma = inputs(shape, B)
        M, A, P, R = xyz.shape[1], xyz.shape[2], len(pairs), len(centers)
        edges = col.shape[0]
        pair_i, pair_j = [p[0] for p in pairs], [p[1] for p in pairs]
        ints = ctypes.c_int * P
        am = amask.contiguous()
        g_rbf = torch.randn(edges, P * R, device="cuda")
        pair_grad = torch.empty(edges, P, 3, device="cuda")

        def k52():
            rc = lib.ps_csr_edge_rbf_backward_f32(xyz.data_ptr(), am.data_ptr(), None, None, row_ptr.data_ptr(), col.data_ptr(), edges,
                                                  ints(*pair_i), ints(*pair_j), P, (ctypes.c_float * R)(*centers.tolist()), R,
                                                  float(sigma), None, g_rbf.data_ptr(), pair_grad.data_ptr(), B, M, A, M, A, stream)
            assert rc == 0, rc

        entry = {"M": M, "P": P, "R": R, "edges": edges, "k52_input_bytes": g_rbf.numel() * 4, "k52_output_bytes": pair_grad.numel() * 4,
                 "k52": timed(k52)}
        scratch = torch.empty_like(g_rbf)
        entry["copy_of_g_rbf"] = timed(lambda: scratch.copy_(g_rbf))
        del scratch
        entry["k52_over_copy"] = entry["k52"]["median_us"] / entry["copy_of_g_rbf"]["median_us"]
        entry["k52_read_GB_per_s"] = entry["k52_input_bytes"] / entry["k52"]["median_us"] * 1e-3
        entry["copy_read_GB_per_s"] = entry["k52_input_bytes"] / entry["copy_of_g_rbf"]["median_us"] * 1e-3
        entry["incoming_lists"] = timed(lambda: ops.csr_incoming_edges(row_ptr, col, B, M, M))
        in_ptr, in_edge = ops.csr_incoming_edges(row_ptr, col, B, M, M)
        entry["k53"] = timed(lambda: ops.csr_edge_pair_grad_sum(pair_grad, row_ptr, in_ptr, in_edge, pair_i=pair_i, pair_j=pair_j,
                                                                B=B, M=M, A=A))
        if idx is not None:
            rot, trans = ops.frames(xyz, 0, 1, 2, 1)
            fmask = amask[:, :, :3].all(-1)
            g_pos, g_rot = torch.randn(edges, 3, device="cuda"), torch.randn(edges, 3, 3, device="cuda")
            entry["k54"] = timed(lambda: ops.csr_edge_frames_backward(rot, trans, row_ptr, col, in_ptr, in_edge, fmask, grad_pos=g_pos,
                                                                      grad_rot=g_rot))
            del rot, trans, g_pos, g_rot
        del pair_grad, in_ptr, in_edge
        torch.cuda.empty_cache()
        # the whole differentiable call: forward (K25 / K50), then K52, the incoming lists and K53
        x = xyz.clone().requires_grad_()
        kw = dict(pairs=pairs, centers=centers, sigma=sigma)
        graph = None if idx is not None else geometry.RadiusGraph(row_ptr, col, None, torch.zeros(B, M, dtype=torch.int32, device="cuda"))

        def fused():
            x.grad = None
            rbf = geometry.edge_distance_features(x, idx, am, **kw) if idx is not None else \
                geometry.radius_edge_distance_features(x, graph, am, **kw)
            rbf.backward(g_rbf.view(rbf.shape))

        entry["fused_forward_backward"] = timed(fused, 2, 10)
        report["shapes"][shape] = entry
        del x, g_rbf, xyz, amask, am, row_ptr, col, idx
        torch.cuda.empty_cache()
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "edge_grad_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch
    from protstruc_amd import geometry
    entries = {}
    for shape in SHAPES:
        def measure(b):
            xyz, amask, row_ptr, col, idx, pairs, centers, sigma = inputs(shape, b)
            pt, ct = torch.tensor(pairs, device="cuda"), torch.from_numpy(centers).cuda()
            x = torch.nan_to_num(xyz).requires_grad_()
            if idx is None:
                count = (row_ptr[1:] - row_ptr[:-1]).reshape(b, -1).to(torch.int32)
                bi, ii, jj = geometry.radius_graph_edges(geometry.RadiusGraph(row_ptr, col, None, count))
                forward = lambda: csr_edge_time.composed(x, amask, bi, ii, jj, pt, ct, sigma)   # noqa: E731
            else:
                forward = lambda: edge_time.composed(x, idx, amask, pt, ct, sigma)              # noqa: E731
            g = torch.randn_like(forward().detach())

            def both():
                x.grad = None
                forward().backward(g)

            return {"composed_forward_backward": timed(both, 1, 3), "edges_at_that_batch": int(col.numel())}

        entries[shape] = largest_batch_that_fits(B, measure)
    print(json.dumps(entries), flush=True)
    with open(os.path.join(outdir, "edge_grad_time_torch.json"), "w") as f:
        json.dump(entries, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "edge_grad_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "edge_grad_time_torch.json")) as f:
        entries = json.load(f)
    for shape, c in entries.items():
        report["shapes"][shape]["composed_torch"] = c
        if c.get("batch"):
            report["shapes"][shape]["composed_over_fused"] = \
                c["composed_forward_backward"]["median_us"] * (B / c["batch"]) / report["shapes"][shape]["fused_forward_backward"]["median_us"]
    os.remove(os.path.join(outdir, "edge_grad_time_events.json"))
    os.remove(os.path.join(outdir, "edge_grad_time_torch.json"))
    with open(os.path.join(outdir, "edge_grad_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
