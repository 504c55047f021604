#!/usr/bin/python3
"""Time the solvent-accessibility kernel (ops.solvent_accessibility) against a composed-torch evaluation of the same
definition in float32 on the same GPU, and write profiles/sasa_time.json.

    python3 tools/sasa_time.py [--outdir DIR]

Shape: B = 128, N = 512, A = 15 (M = 7680 points per structure), S = 96 test points per atom, probe 1.4 A.  Inputs: one
compact chain -- a 3.8 A walk kept inside a sphere, every residue with 15 atom slots placed within 3.5 A of its CA --
turned by a random rotation in every structure, carbon radii, 45 % of the slots masked with NaN coordinates, which leaves
the eight atoms per residue and the forty-odd neighbours within 6.2 A per atom of a real protein.
The composed version finds every atom's neighbours from ``cdist`` (a dense (B,M,M) matrix), gathers the K closest
candidates and tests the (B,m,S,K) point-to-neighbour distances chunk by chunk over the atoms; it runs at the largest batch
(B, B / 2, ...) that fits and the report says which.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20), and the counts' agreement
  torch   the composed float32 evaluation with the allocator's peak

Reported: the times, how many counts of the composed version differ from the kernel's (float32 against double at the
sphere surfaces; not an error measure), and the ratio.  No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import largest_batch_that_fits, main, timed

B, N, A, S = 128, 512, 15, 96
PROBE = 1.4
STEP_TIMEOUT_S = {"events": 180, "torch": 400}


def inputs(batch, seed=1):
    """(points (batch,M,3), radius (batch,M), mask (batch,M), sphere (S,3)) on the GPU"""
    import numpy as np
    import torch
    from protstruc_amd import geometry
    rng = np.random.default_rng(seed)
    bound = (N * 140.0 * 3 / (4 * np.pi)) ** (1.0 / 3.0) * 1.5      # 140 A^3 per residue, loosely
    ca = np.zeros((N, 3))
    for k in range(1, N):
        for _ in range(200):
            d = rng.normal(size=3)
            cand = ca[k - 1] + 3.8 * d / np.linalg.norm(d)
            if np.linalg.norm(cand) < bound and (k < 3 or np.sqrt(((ca[:k - 2] - cand) ** 2).sum(-1)).min() > 5.0):
                break
        ca[k] = cand
    offsets = rng.normal(size=(N, A, 3))
    offsets *= (rng.random((N, A, 1)) ** (1 / 3)) * 3.5 / np.linalg.norm(offsets, axis=-1, keepdims=True)
    atoms = (ca[:, None, :] + offsets).reshape(N * A, 3)
    rot = np.linalg.qr(rng.normal(size=(batch, 3, 3)))[0]
    x = np.einsum("bij,mj->bmi", rot, atoms - atoms.mean(0)).astype(np.float32)
    mask = rng.random((batch, N * A)) >= 0.45
    x[~mask] = np.nan
    radius = np.full((batch, N * A), 1.7, dtype=np.float32)
    return (torch.from_numpy(x).cuda(), torch.from_numpy(radius).cuda(), torch.from_numpy(mask).cuda(),
            geometry.sphere_points(S).cuda())


def composed(points, radius, mask, sphere, probe=PROBE, isolate=None, chunk=32):
    """The definition with dense tensors, float32: (count (B,M) int32, area (B,M) float32)"""
    import math

    import torch
    b, m = mask.shape
    s = sphere.shape[0]
    mask = mask != 0
    x = torch.where(mask[:, :, None], points, torch.zeros_like(points))
    R = torch.where(mask, radius + probe, torch.zeros_like(radius))
    reach = R * sphere.norm(dim=-1).max()
    idx = torch.arange(m, device=points.device)
    near = mask[:, :, None] & mask[:, None, :] & (idx[:, None] != idx[None, :])
    near &= torch.cdist(x, x) < reach[:, :, None] + R[:, None, :] + 1e-3
    if isolate is not None:
        near &= isolate[:, :, None] == isolate[:, None, :]
    k = max(int(near.sum(-1).max().item()), 1) if near.numel() else 1
    k = min(k, m)
    taken, nb = torch.topk(near.to(torch.uint8), k, dim=-1) if m else (near[:, :, :0], near[:, :, :0].long())
    taken = taken != 0                                                         # (B,M,K): slot holds a real neighbour
    del near
    count = torch.zeros(b, m, dtype=torch.int32, device=points.device)
    rows = torch.arange(b, device=points.device)[:, None, None]
    for m0 in range(0, m, chunk):
        sl = slice(m0, min(m0 + chunk, m))
        p = x[:, sl, None, :] + R[:, sl, None, None] * sphere[None, None, :, :]   # (B,c,S,3)
        xn, Rn = x[rows, nb[:, sl]], R[rows, nb[:, sl]]                           # (B,c,K,3), (B,c,K)
        d2 = ((p[:, :, :, None, :] - xn[:, :, None, :, :]) ** 2).sum(-1)          # (B,c,S,K)
        buried = ((d2 < (Rn * Rn)[:, :, None, :]) & taken[:, sl, None, :]).any(-1)
        count[:, sl] = torch.where(mask[:, sl], s - buried.sum(-1), torch.zeros_like(buried.sum(-1))).to(torch.int32)
    area = (4.0 * math.pi) * R * R * count.to(torch.float32) / s
    return count, area


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    x, r, mask, sphere = inputs(B)
    count, area = ops.solvent_accessibility(x, r, mask, sphere=sphere, probe=PROBE)
    taking_part = int(mask.sum().item())
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "A": A, "S": S, "probe": PROBE, "atoms_taking_part": taking_part,
              "mean_open_points_per_atom": float(count.sum().item()) / max(taking_part, 1),
              "mean_area_per_structure": float(area.sum().item()) / B,
              "kernel": timed(lambda: ops.solvent_accessibility(x, r, mask, sphere=sphere, probe=PROBE))}
    small = min(B, 2)
    ref = composed(x[:small], r[:small], mask[:small], sphere)[0]
    report["counts_that_differ_from_composed_float32"] = int((ref != count[:small]).sum().item())
    report["counts_compared"] = small * N * A
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "sasa_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch

    def measure(b):
        x, r, mask, sphere = inputs(b)
        with torch.no_grad():
            return {"composed": timed(lambda: composed(x, r, mask, sphere), 1, 3)}

    entry = {"B": B, "N": N, "A": A, "S": S, **largest_batch_that_fits(B, measure)}
    print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "sasa_time_torch.json"), "w") as f:
        json.dump(entry, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "sasa_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "sasa_time_torch.json")) as f:
        c = json.load(f)
    report["composed_torch"] = c
    if c.get("batch"):
        report["composed_over_kernel"] = c["composed"]["median_us"] * (B / c["batch"]) / report["kernel"]["median_us"]
    os.remove(os.path.join(outdir, "sasa_time_events.json"))
    os.remove(os.path.join(outdir, "sasa_time_torch.json"))
    with open(os.path.join(outdir, "sasa_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
