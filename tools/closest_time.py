#!/usr/bin/python3
"""Time the closest-atom kernels (ops.closest_atoms, ops.closest_atoms_backward) against the composed route a user writes
without them -- ``ops.pairwise_distance`` into the (B,N,N,A,A) tensor, a NaN-safe ``amin`` over its last two axes -- and
against the store floor, ``fill_(0)`` on the very ``dist`` and ``pair`` buffers, and write profiles/closest_time.json.

    python3 tools/closest_time.py [--outdir DIR]

One shape: B = 128 structures on the compact chain of tools/sasa_time.py, N = 512 residues of A = 15 atom slots, 45 % of
the slots masked with NaN coordinates.  The composed route runs at the largest batch (B, B / 2, ...) that fits and the
report says which, with the allocator's peak.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20): the forward kernel at cutoff = inf, 8 A and 5 A, the
          backward kernel, the two fills; and how many entries of the composed float32 result differ from the kernel's at a
          batch of 2
  torch   the composed evaluation with the allocator's peak

The entries that differ are float32 arithmetic against double: not an error measure.  No speed is asserted anywhere.
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import sasa_time
from tools.steps import largest_batch_that_fits, main, timed

B, N, A = 128, 512, 15
CUTOFFS = {"cutoff_inf": math.inf, "cutoff_8A": 8.0, "cutoff_5A": 5.0}
STEP_TIMEOUT_S = {"events": 240, "torch": 400}


def inputs(batch):
    """(xyz (batch,N,A,3) with NaN in the masked slots, atom_mask (batch,N,A)) on the GPU"""
    assert (sasa_time.N, sasa_time.A) == (N, A)
    x, _, mask, _ = sasa_time.inputs(batch)
    return x.reshape(batch, N, A, 3), mask.reshape(batch, N, A)


def composed(xyz, atom_mask):
    """The route a user writes today: dist (B,N,N) float32, +inf where no pair of present atoms exists"""
    import torch
    from protstruc_amd import ops
    d, ok = ops.pairwise_distance(xyz, atom_mask)
    return torch.where(ok, d, torch.full_like(d, math.inf)).amin(dim=(-2, -1))


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    xyz, mask = inputs(B)
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "A": A, "atoms_taking_part": int(mask.sum().item()),
              "output_bytes": B * N * N * 6, "forward": {}}
    for name, cutoff in CUTOFFS.items():
        dist, pair = ops.closest_atoms(xyz, mask, cutoff)
        report["forward"][name] = {"kernel": timed(lambda: ops.closest_atoms(xyz, mask, cutoff)),
                                   "pairs_that_count": float(torch.isfinite(dist).float().mean().item())}
    dist, pair = ops.closest_atoms(xyz, mask)
    g = torch.randn_like(dist)
    report["backward"] = {"kernel": timed(lambda: ops.closest_atoms_backward(xyz, pair, g))}
    report["store_floor"] = {"fill_dist_and_pair": timed(lambda: (dist.fill_(0), pair.fill_(0)))}
    small = min(B, 2)
    ref = composed(xyz[:small], mask[:small])
    dist = ops.closest_atoms(xyz[:small], mask[:small])[0]
    report["entries_that_differ_from_composed_float32"] = int((ref != dist).sum().item())
    report["entries_compared"] = small * N * N
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "closest_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch

    def measure(b):
        xyz, mask = inputs(b)
        with torch.no_grad():
            return {"composed": timed(lambda: composed(xyz, mask), 1, 3)}

    entry = largest_batch_that_fits(B, measure)
    print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "closest_time_torch.json"), "w") as f:
        json.dump(entry, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "closest_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "closest_time_torch.json")) as f:
        c = json.load(f)
    report["composed_torch"] = c
    if c.get("batch"):
        report["composed_over_kernel_at_cutoff_inf"] = \
            c["composed"]["median_us"] * (B / c["batch"]) / report["forward"]["cutoff_inf"]["kernel"]["median_us"]
    os.remove(os.path.join(outdir, "closest_time_events.json"))
    os.remove(os.path.join(outdir, "closest_time_torch.json"))
    with open(os.path.join(outdir, "closest_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
