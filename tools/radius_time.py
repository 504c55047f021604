#!/usr/bin/python3
"""Time the radius graph (ops.radius_graph: K47 boxes, K48 count, ``torch.cumsum``, K48 fill) against K24
(``ops.nearest_neighbors(k=64)`` at the same cutoff, on the same inputs), against the composed float32 torch route --
``torch.cdist``, compare, ``nonzero`` -- and against ``fill_`` over the bytes of ``col`` + ``dist``, the floor of the fill
pass; write profiles/radius_time.json.

    python3 tools/radius_time.py [--outdir DIR]

Shapes, all at B = 128, the inputs of tools/knn_time.py (the compact chain of tools/sasa_time.py: 512 residues of 15 atom
slots, a random rotation per structure):
  residues_10A   M = 512 residue centroids, no mask, cutoff 10 A
  atoms_5A       M = 7680 atom slots, 45 % masked over NaN, the residue index as the exclusion key, cutoff 5 A
  atoms_8A       the same, cutoff 8 A
The composed route builds the (B,M,M) distance matrix; it runs at the largest batch (B, B / 2, ...) that fits and the
report says which, with the allocator's peak.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each launch and around the whole call (3 warm-ups, median / min of 20), the number of edges,
          the counters of the counting sweep (the share of blocks dropped at each level), K24 and the ``fill_`` floor
  torch   the composed float32 evaluation with the allocator's peak, and whether its edge count is the kernel's

No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import knn_time
from tools.steps import largest_batch_that_fits, main, timed

B = knn_time.B
SHAPES = {"residues_10A": ("residues_k48", 10.0), "atoms_5A": ("atoms_k64", 5.0), "atoms_8A": ("atoms_k64", 8.0)}
STEP_TIMEOUT_S = {"events": 300, "torch": 500}
STATS = ("blocks_walked", "blocks_dropped_by_the_wave_test", "blocks_dropped_by_the_lane_tests", "quarters_walked",
         "quarters_skipped", "columns_in_double")


def composed(points, cutoff, mask=None, key=None):
    """The float32 route a user writes today: (batch, row, col) int64 of every edge, from the dense matrix"""
    import torch
    b, m = points.shape[:2]
    mask = torch.ones(b, m, dtype=torch.bool, device=points.device) if mask is None else mask != 0
    x = torch.where(mask[:, :, None], points, torch.zeros_like(points))
    idx = torch.arange(m, device=points.device)
    near = torch.cdist(x, x) <= cutoff
    near &= mask[:, :, None] & mask[:, None, :] & (idx[:, None] != idx[None, :])
    if key is not None:
        near &= key[:, :, None] != key[:, None, :]
    return near.nonzero(as_tuple=True)


def launches(x, mask, key, cutoff):
    """The call of ops.radius_graph taken apart, on buffers made once: {name: a function that enqueues that part}, the
    number of edges, and the summed counters"""
    import torch
    from protstruc_amd import _lib, ops
    lib = _lib.load()
    batch, M = x.shape[:2]
    ptr = lambda t: None if t is None else t.data_ptr()                         # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    boxes = torch.empty(batch, (M + 63) // 64, ops.RADIUS_BOX_FLOATS, device=x.device)
    count = torch.empty(batch, M, dtype=torch.int32, device=x.device)
    row_ptr = torch.zeros(batch * M + 1, dtype=torch.int64, device=x.device)
    stats = torch.zeros(batch, (M + 63) // 64, ops.RADIUS_STATS, dtype=torch.int32, device=x.device)
    args = (ptr(x), ptr(mask), None, None, ptr(key), None, float(cutoff), 0, ptr(boxes))

    def check(rc):
        assert rc == 0, rc

    parts = {"boxes": lambda: check(lib.ps_radius_tile_boxes_f32(ptr(x), ptr(mask), ptr(boxes), batch, M, stream)),
             "count": lambda: check(lib.ps_radius_count_f32(*args, ptr(count), None, batch, M, M, stream)),
             "cumsum": lambda: torch.cumsum(count.reshape(-1), 0, dtype=torch.int64, out=row_ptr[1:])}
    for name in ("boxes", "count", "cumsum"):
        parts[name]()
    check(lib.ps_radius_count_f32(*args, ptr(count), ptr(stats), batch, M, M, stream))
    edges = int(row_ptr[-1])
    col = torch.empty(edges, dtype=torch.int32, device=x.device)
    dist = torch.empty(edges, dtype=torch.float32, device=x.device)
    parts["fill"] = lambda: check(lib.ps_radius_fill_f32(*args, ptr(row_ptr), edges, ptr(col), ptr(dist), batch, M, M, stream))
    parts["fill_floor"] = lambda: (col.fill_(0), dist.fill_(0.0))
    return parts, edges, dict(zip(STATS, stats.sum(dim=(0, 1)).tolist()))


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "shapes": {}}
    for shape, (family, cutoff) in SHAPES.items():
        x, mask, key = knn_time.inputs(family, B)
        mask = None if mask is None else mask.contiguous()
        parts, edges, stats = launches(x, mask, key, cutoff)
        walked, quarters = max(stats["blocks_walked"], 1), max(stats["quarters_walked"], 1)
        entry = {"M": x.shape[1], "cutoff": cutoff, "edges": edges,
                 "points_taking_part": int(x.shape[0] * x.shape[1] if mask is None else mask.sum().item()),
                 "counters": stats,
                 "share_of_blocks_dropped_by_the_wave_test": stats["blocks_dropped_by_the_wave_test"] / walked,
                 "share_of_blocks_dropped_by_the_lane_tests": stats["blocks_dropped_by_the_lane_tests"] / walked,
                 "share_of_quarters_of_staged_blocks_skipped": stats["quarters_skipped"] / quarters,
                 "parts": {name: timed(fn) for name, fn in parts.items()},
                 "fill_bytes": 8 * edges,
                 "total_max_edges_given": timed(lambda: ops.radius_graph(x, cutoff, mask, exclude=key, max_edges=edges)),
                 "total_with_host_read": timed(lambda: ops.radius_graph(x, cutoff, mask, exclude=key)),
                 "nearest_neighbors_k64_same_cutoff": timed(lambda: ops.nearest_neighbors(x, 64, mask, exclude=key, cutoff=cutoff))}
        count = ops.radius_graph(x, cutoff, mask, exclude=key, max_edges=0)[3]
        entry["rows_over_64"] = int((count > 64).sum().item())
        entry["longest_row"] = int(count.max().item())
        report["shapes"][shape] = entry
        del x, mask, key, parts, count
        torch.cuda.empty_cache()
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "radius_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch
    entries = {}
    for shape, (family, cutoff) in SHAPES.items():
        def measure(b):
            x, mask, key = knn_time.inputs(family, b)
            with torch.no_grad():
                t = timed(lambda: composed(x, cutoff, mask, key), 1, 3)
                edges = int(composed(x, cutoff, mask, key)[0].numel())
            return {"composed": t, "edges_at_that_batch": edges}

        entries[shape] = largest_batch_that_fits(B, measure)
    print(json.dumps(entries), flush=True)
    with open(os.path.join(outdir, "radius_time_torch.json"), "w") as f:
        json.dump(entries, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "radius_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "radius_time_torch.json")) as f:
        entries = json.load(f)
    for shape, c in entries.items():
        entry = report["shapes"][shape]
        entry["composed_torch"] = c
        total = entry["total_max_edges_given"]["median_us"]
        entry["k24_over_total"] = entry["nearest_neighbors_k64_same_cutoff"]["median_us"] / total
        if c.get("batch"):
            entry["composed_over_total"] = c["composed"]["median_us"] * (B / c["batch"]) / total
    os.remove(os.path.join(outdir, "radius_time_events.json"))
    os.remove(os.path.join(outdir, "radius_time_torch.json"))
    with open(os.path.join(outdir, "radius_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
