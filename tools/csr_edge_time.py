#!/usr/bin/python3
"""Time the edge features on CSR graphs (ops.csr_edge_rbf, K50; ops.csr_edge_rows, K49; ops.csr_edge_frames, K51) and write
profiles/csr_edge_time.json.  K50, ``rbf`` only, is set against three yardsticks on the same GPU: a fill of the very buffer
it wrote (the store-rate yardstick K25 is held to, tools/edge_time.py), K25 (ops.edge_rbf) on a kNN graph of about the same
number of real edges, and the composed float32 torch route on the triples of ``geometry.radius_graph_edges``.  K49 and K51
are reported as plain times.

    python3 tools/csr_edge_time.py [--outdir DIR]

Shapes, all at B = 128, the graphs and inputs of tools/radius_time.py (the compact chain of tools/sasa_time.py: 512 residues
of 15 atom slots):
  residues_10A   the residue graph at 10 A, M = 512; xyz (B,512,15,3) with 45 % of the slots masked over NaN; the P = 25
                 ordered pairs of the first five slots, R = 16 centres over 2 .. 22 A; K51 on the N-CA-C frames
  atoms_5A       the all-atom graph at 5 A, M = 7680, own residue excluded; the (B, 7680, 1, 3) view, P = 1, R = 16 centres
                 over 0 .. 8 A
  atoms_8A       the same at 8 A
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20): K50 into one buffer, ``out.fill_(0)`` on that
          buffer, K25 on the kNN graph with k = ceil(edges / (B M)) (at most 64), K49, and K51 on the residue graph
  torch   the composed float32 evaluation at the largest batch (B, B / 2, ...) that fits, with the allocator's peak

No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import knn_time, sasa_time
from tools.steps import largest_batch_that_fits, main, timed

B, N, A = knn_time.B, sasa_time.N, sasa_time.A
SHAPES = {"residues_10A": ("residues_k48", 10.0), "atoms_5A": ("atoms_k64", 5.0), "atoms_8A": ("atoms_k64", 8.0)}
STEP_TIMEOUT_S = {"events": 300, "torch": 400}


def inputs(shape, batch):
    """(graph points, point mask, key, cutoff; xyz (batch,M,A',3), atom mask (batch,M,A'), pairs, centers, sigma) on the GPU"""
    from protstruc_amd import geometry
    family, cutoff = SHAPES[shape]
    points, mask, key = knn_time.inputs(family, batch)
    if family == "atoms_k64":
        centers, sigma = geometry.rbf_centers(16, 0.0, 8.0)
        return points, mask.contiguous(), key, cutoff, points.reshape(batch, N * A, 1, 3), mask.reshape(batch, N * A, 1), [(0, 0)], centers, sigma
    x, _, amask, _ = sasa_time.inputs(batch)
    centers, sigma = geometry.rbf_centers(16)
    return points, None, None, cutoff, x.reshape(batch, N, A, 3), amask.reshape(batch, N, A), list(geometry.BACKBONE_PAIRS), centers, sigma


def composed(xyz, mask, b, i, j, pairs, centers, sigma):
    """The float32 route a user writes today on (batch, row, col) triples: rbf (E, P*R); ``pairs`` (P,2) and ``centers`` (R,) tensors"""
    import torch
    ok = mask != 0
    x = torch.where(ok[..., None], xyz, torch.zeros_like(xyz))
    pi, pj = pairs[:, 0], pairs[:, 1]
    xi, xj = x[b, i][:, pi], x[b, j][:, pj]                                    # (E,P,3), gathered
    real = ok[b, i][:, pi] & ok[b, j][:, pj]
    d = (xj - xi).norm(dim=-1)
    z = (d[..., None] - centers) / sigma                                       # (E,P,R), broadcast
    return (torch.exp(-(z * z)) * real[..., None]).reshape(d.shape[0], -1)


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "shapes": {}}
    for shape in SHAPES:
        points, pmask, key, cutoff, xyz, amask, pairs, centers, sigma = inputs(shape, B)
        M, P, R = xyz.shape[1], len(pairs), len(centers)
        row_ptr, col, _, count = ops.radius_graph(points, cutoff, pmask, exclude=key)
        edges = col.shape[0]
        kw = dict(pair_i=[p[0] for p in pairs], pair_j=[p[1] for p in pairs], centers=centers, sigma=sigma, want_dist=False)
        # the launcher allocates its output: time the C entry point into one buffer, as tools/edge_time.py does
        import ctypes
        from protstruc_amd import _csredge
        lib = _csredge.load()
        out = torch.empty(edges, P * R, dtype=torch.float32, device="cuda")
        ints = ctypes.c_int * P
        tables = (ints(*kw["pair_i"]), ints(*kw["pair_j"]), P, (ctypes.c_float * R)(*centers.tolist()), R, float(sigma))
        am = amask.contiguous()
        stream = torch.cuda.current_stream().cuda_stream

        def k50():
            rc = lib.ps_csr_edge_rbf_f32(xyz.data_ptr(), am.data_ptr(), None, None, row_ptr.data_ptr(), col.data_ptr(), edges,
                                         *tables, None, out.data_ptr(), B, M, xyz.shape[2], M, xyz.shape[2], stream)
            assert rc == 0, rc

        entry = {"M": M, "cutoff": cutoff, "P": P, "R": R, "edges": edges, "longest_row": int(count.max().item()),
                 "output_bytes": out.numel() * 4, "k50_rbf": timed(k50)}
        entry["nonzero_fraction"] = float((out[:1 << 22] != 0).float().mean().item())
        entry["fill"] = timed(lambda: out.fill_(0))
        entry["k50_over_fill"] = entry["k50_rbf"]["median_us"] / entry["fill"]["median_us"]
        entry["k50_GB_per_s"] = entry["output_bytes"] / entry["k50_rbf"]["median_us"] * 1e-3
        entry["fill_GB_per_s"] = entry["output_bytes"] / entry["fill"]["median_us"] * 1e-3
        entry["k49_rows"] = timed(lambda: ops.csr_edge_rows(row_ptr, M, edges))
        del out
        torch.cuda.empty_cache()
        # K25 on a kNN graph of about as many real edges
        k = max(1, min(ops.KNN_MAX_K, -(-edges // (B * M))))
        idx = ops.nearest_neighbors(points, k, pmask, exclude=key)[0]
        out25 = torch.empty(B, M, k, P * R, dtype=torch.float32, device="cuda")
        from protstruc_amd import _lib
        k25 = _lib.load().ps_edge_rbf_f32

        def call25():
            rc = k25(xyz.data_ptr(), am.data_ptr(), idx.data_ptr(), *tables, None, out25.data_ptr(), B, M, xyz.shape[2], k, stream)
            assert rc == 0, rc

        entry["k25"] = {"k": k, "real_edges": int((idx >= 0).sum().item()), "output_bytes": out25.numel() * 4, "kernel": timed(call25)}
        entry["k25"]["fill"] = timed(lambda: out25.fill_(0))
        entry["k25"]["kernel_over_fill"] = entry["k25"]["kernel"]["median_us"] / entry["k25"]["fill"]["median_us"]
        entry["k25"]["GB_per_s"] = entry["k25"]["output_bytes"] / entry["k25"]["kernel"]["median_us"] * 1e-3
        entry["k50_rate_over_k25_rate"] = entry["k50_GB_per_s"] / entry["k25"]["GB_per_s"]
        del out25, idx
        torch.cuda.empty_cache()
        if shape == "residues_10A":
            rot, trans = ops.frames(xyz, 0, 1, 2, 1)
            fmask = amask[:, :, :3].all(-1)
            entry["k51_frames"] = timed(lambda: ops.csr_edge_frames(rot, trans, row_ptr, col, fmask))
            del rot, trans
        report["shapes"][shape] = entry
        del points, pmask, key, xyz, amask, row_ptr, col, count
        torch.cuda.empty_cache()
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "csr_edge_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch
    from protstruc_amd import geometry, ops
    entries = {}
    for shape in SHAPES:
        def measure(b):
            points, pmask, key, cutoff, xyz, amask, pairs, centers, sigma = inputs(shape, b)
            g = geometry.RadiusGraph(*ops.radius_graph(points, cutoff, pmask, exclude=key))
            bi, ii, jj = geometry.radius_graph_edges(g)
            pt, ct = torch.tensor(pairs, device="cuda"), torch.from_numpy(centers).cuda()
            with torch.no_grad():
                return {"composed": timed(lambda: composed(xyz, amask, bi, ii, jj, pt, ct, sigma), 1, 3), "edges_at_that_batch": int(bi.numel())}

        entries[shape] = largest_batch_that_fits(B, measure)
    print(json.dumps(entries), flush=True)
    with open(os.path.join(outdir, "csr_edge_time_torch.json"), "w") as f:
        json.dump(entries, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "csr_edge_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "csr_edge_time_torch.json")) as f:
        entries = json.load(f)
    for shape, c in entries.items():
        report["shapes"][shape]["composed_torch"] = c
        if c.get("batch"):
            report["shapes"][shape]["composed_over_k50"] = \
                c["composed"]["median_us"] * (B / c["batch"]) / report["shapes"][shape]["k50_rbf"]["median_us"]
    os.remove(os.path.join(outdir, "csr_edge_time_events.json"))
    os.remove(os.path.join(outdir, "csr_edge_time_torch.json"))
    with open(os.path.join(outdir, "csr_edge_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
