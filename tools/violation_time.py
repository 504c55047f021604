#!/usr/bin/python3
"""Time the clash kernels (ops.clash, ops.clash_backward) against the torch restatement of tests/violation_ref.py run in
float32 with autograd on the same GPU, and write profiles/violation_time.json.

    python3 tools/violation_time.py [--outdir DIR]

Shapes: B = 8, M = 512 * 15 = 7680 (all atoms of 512 residues) and B = 128, M = 512 * 5 = 2560 (backbone + CB), the
residue index as the group; the composed version runs at the largest batch (B, B / 2, ...) that fits and the report says
which.  Inputs: a centred random walk of residues with 3.8 A steps, each residue's atoms the walk's point plus 1.5 A of
Gaussian scatter, radii drawn from the four element values -- a structure before any violation loss has acted on it, with
a clash at a few per cent of the atoms.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20), K17 and K18
  torch   the composed float32 restatement (forward; forward + autograd backward) with the allocator's peak

Reported per shape: the times, the number of clashing pairs, and the ratio to the composed version (scaled to the full
batch where the composed version had to run at a smaller one).  No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import largest_batch_that_fits, main, timed

SHAPES = [("all_atoms", 8, 512, 15), ("backbone_cb", 128, 512, 5)]     # name, B, residues, atoms per residue
STEP_TIMEOUT_S = {"events": 180, "torch": 300}


def inputs(B, N, A, seed=1):
    import torch
    from tests import violation_ref as R
    g = torch.Generator().manual_seed(seed)
    points = (R.random_walk(B, N, g, step=3.8)[:, :, None, :] + 1.5 * torch.randn(B, N, A, 3, generator=g)).reshape(B, N * A, 3)
    radius = torch.tensor(R.RADII)[torch.randint(0, len(R.RADII), (B, N * A), generator=g)]
    groups = torch.arange(N, dtype=torch.int32).repeat_interleave(A).expand(B, N * A).contiguous()
    return points.cuda(), radius.cuda(), groups.cuda()


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "tolerance": ops.CLASH_TOLERANCE, "shapes": []}
    for name, B, N, A in SHAPES:
        x, r, groups = inputs(B, N, A)
        w = torch.randn(B, N * A, device="cuda")
        E, n = ops.clash(x, r, None, groups)
        e = {"shape": name, "B": B, "M": N * A, "clashing_pairs": int(n.sum().item()) // 2, "all_pairs": B * (N * A) ** 2,
             "points_in_a_clash": int((n > 0).sum().item())}
        e["forward"] = timed(lambda: ops.clash(x, r, None, groups))
        e["backward"] = timed(lambda: ops.clash_backward(x, r, w, None, groups))
        report["shapes"].append(e)
        print(json.dumps(e), flush=True)
    with open(os.path.join(outdir, "violation_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch
    from tests import violation_ref as R
    out = []
    for name, B, N, A in SHAPES:
        def measure(b):
            x, r, groups = inputs(b, N, A)
            leaf = x.clone().requires_grad_(True)

            def forward():
                with torch.no_grad():
                    return R.clash(x, r, None, groups)

            def both():
                E, _ = R.clash(leaf, r, None, groups)
                return torch.autograd.grad(E.sum(), leaf)

            return {"forward": timed(forward, 1, 3), "forward_and_backward": timed(both, 1, 3)}

        entry = {"shape": name, "B": B, "M": N * A, **largest_batch_that_fits(B, measure)}
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "violation_time_torch.json"), "w") as f:
        json.dump(out, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "violation_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "violation_time_torch.json")) as f:
        composed = {c["shape"]: c for c in json.load(f)}
    for e in report["shapes"]:
        c = composed[e["shape"]]
        e["composed_torch"] = c
        if c.get("batch"):
            scale = e["B"] / c["batch"]
            e["composed_forward_over_kernel"] = c["forward"]["median_us"] * scale / e["forward"]["median_us"]
            e["composed_forward_and_backward_over_kernels"] = c["forward_and_backward"]["median_us"] * scale / (
                e["forward"]["median_us"] + e["backward"]["median_us"])
    os.remove(os.path.join(outdir, "violation_time_events.json"))
    os.remove(os.path.join(outdir, "violation_time_torch.json"))
    with open(os.path.join(outdir, "violation_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
