#!/usr/bin/python3
"""Time the nearest-neighbour kernel (ops.nearest_neighbors) against the composed float32 torch route -- ``torch.cdist``,
masking, ``torch.topk(largest=False)`` -- on the same GPU, and write profiles/knn_time.json.

    python3 tools/knn_time.py [--outdir DIR]

Shapes, all at B = 128 on the compact chain of tools/sasa_time.py (512 residues of 15 atom slots, 45 % of the slots masked
with NaN coordinates, a random rotation per structure):
  residues_k48   M = 512 residue centroids, no mask, k = 48        (ProteinMPNN's graph)
  residues_k30   the same, k = 30                                   (Structured Transformer, GVP)
  atoms_k64      M = 7680 atom slots with the mask, the residue index as the exclusion key, k = 64
The composed route builds the (B,M,M) distance matrix; it runs at the largest batch (B, B / 2, ...) that fits and the
report says which, with the allocator's peak.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each kernel call (3 warm-ups, median / min of 20), and how many rows of the composed result
          differ in ``idx`` from the kernel's at a batch of 2
  torch   the composed float32 evaluation with the allocator's peak

The rows that differ are float32 against double (and torch.topk's undefined order on ties against the lower index): not
an error measure.  No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import sasa_time
from tools.steps import largest_batch_that_fits, main, timed

B, N, A = 128, 512, 15
SHAPES = {"residues_k48": 48, "residues_k30": 30, "atoms_k64": 64}
STEP_TIMEOUT_S = {"events": 180, "torch": 400}


def inputs(shape, batch):
    """(points (batch,M,3), mask (batch,M) or None, key (batch,M) int32 or None) on the GPU"""
    import torch
    assert (sasa_time.N, sasa_time.A) == (N, A)
    x, _, mask, _ = sasa_time.inputs(batch)
    if shape == "atoms_k64":
        key = torch.arange(N, dtype=torch.int32, device=x.device).repeat_interleave(A).expand(batch, N * A).contiguous()
        return x, mask, key
    return torch.nanmean(x.reshape(batch, N, A, 3), dim=2).nan_to_num_(), None, None   # a residue with no atom left: the origin


def composed(points, k, mask=None, key=None):
    """The float32 route a user writes today: (idx (B,M,k) int32 with -1 padding, dist (B,M,k), count (B,M) int32)"""
    import math

    import torch
    b, m = points.shape[:2]
    mask = torch.ones(b, m, dtype=torch.bool, device=points.device) if mask is None else mask != 0
    x = torch.where(mask[:, :, None], points, torch.zeros_like(points))
    idx = torch.arange(m, device=points.device)
    ok = mask[:, :, None] & mask[:, None, :] & (idx[:, None] != idx[None, :])
    if key is not None:
        ok &= key[:, :, None] != key[:, None, :]
    d = torch.cdist(x, x).masked_fill_(~ok, math.inf)
    del ok
    kk = min(k, m)
    dist, nb = torch.topk(d, kk, dim=-1, largest=False)
    if kk < k:
        dist = torch.nn.functional.pad(dist, (0, k - kk), value=math.inf)
        nb = torch.nn.functional.pad(nb, (0, k - kk), value=-1)
    real = torch.isfinite(dist)
    return torch.where(real, nb, torch.full_like(nb, -1)).to(torch.int32), dist, real.sum(-1).to(torch.int32)


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "A": A, "shapes": {}}
    for shape, k in SHAPES.items():
        x, mask, key = inputs(shape, B)
        idx, _, count = ops.nearest_neighbors(x, k, mask, exclude=key)
        small = min(B, 2)
        ref = composed(x[:small], k, None if mask is None else mask[:small], None if key is None else key[:small])[0]
        report["shapes"][shape] = {
            "M": x.shape[1], "k": k, "points_taking_part": int(x.shape[0] * x.shape[1] if mask is None else mask.sum().item()),
            "mean_count": float(count.sum().item()) / (x.shape[0] * x.shape[1]),
            "kernel": timed(lambda: ops.nearest_neighbors(x, k, mask, exclude=key)),
            "rows_that_differ_from_composed_float32": int((ref != idx[:small]).any(-1).sum().item()),
            "rows_compared": small * x.shape[1]}
        del x, mask, key, idx, count, ref
        torch.cuda.empty_cache()
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "knn_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch
    entries = {}
    for shape, k in SHAPES.items():
        def measure(b):
            x, mask, key = inputs(shape, b)
            with torch.no_grad():
                return {"composed": timed(lambda: composed(x, k, mask, key), 1, 3)}

        entries[shape] = largest_batch_that_fits(B, measure)
    print(json.dumps(entries), flush=True)
    with open(os.path.join(outdir, "knn_time_torch.json"), "w") as f:
        json.dump(entries, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "knn_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "knn_time_torch.json")) as f:
        entries = json.load(f)
    for shape, c in entries.items():
        report["shapes"][shape]["composed_torch"] = c
        if c.get("batch"):
            report["shapes"][shape]["composed_over_kernel"] = \
                c["composed"]["median_us"] * (B / c["batch"]) / report["shapes"][shape]["kernel"]["median_us"]
    os.remove(os.path.join(outdir, "knn_time_events.json"))
    os.remove(os.path.join(outdir, "knn_time_torch.json"))
    with open(os.path.join(outdir, "knn_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
