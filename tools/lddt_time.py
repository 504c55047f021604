#!/usr/bin/python3
"""Time the lDDT kernels (ops.lddt hard and smooth, ops.lddt_backward) against the torch restatement of tests/lddt_ref.py
run in float32 on the same GPU, and write profiles/lddt_time.json and profiles/lddt_kernel_stats.csv.

    python3 tools/lddt_time.py [--outdir DIR]

Shapes: B = 128, M = 512 (one CA per residue) and B = 8, M = 512 * 14 (all atoms, the residue index as the group); the
composed version runs at the largest batch (B, B / 2, ...) that fits and the report says which.  Inputs are those of the
tests: a centred random walk with 3.8 A steps (for the all-atom shape each residue's 14 atoms are the walk's point plus
1.5 A of Gaussian scatter) and a prediction 1 A of Gaussian noise away.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20)
  trace   the same launches under ``rocprofv3 --kernel-trace --stats``: the kernels' own times, without launch overhead
  torch   the composed float32 restatement (hard forward; smooth forward; smooth forward + autograd backward) with the
          allocator's peak

Reported per shape: the times, the ratio to the composed version, and for the smooth forward the achieved fraction of the
transcendental issue rate.  That bound is stated, not measured: a transcendental instruction (v_rsq_f32, v_exp_f32,
v_rcp_f32) retires 16 lanes per cycle per SIMD, on 256 CUs x 4 SIMDs at 2.4 GHz; the smooth pair executes 3 + T of them
(two square roots, one exponential, T reciprocals), and only the (64-owner wave, column) combinations in which some
owner counts the column execute them at all -- counted on the host from the first structure's target and scaled by B.
"""
import csv
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import kernel_stats, largest_batch_that_fits, main, timed

SHAPES = [("ca", 128, 512, 1), ("all_atoms", 8, 512, 14)]     # name, B, residues, atoms per residue
STEP_TIMEOUT_S = {"events": 180, "trace": 240, "torch": 300}
TRANSCENDENTAL_LANES_PER_S = 256 * 4 * 16 * 2.4e9
T = 4


def inputs(B, N, A, seed=1):
    import torch
    from tests import lddt_ref as R
    g = torch.Generator().manual_seed(seed)
    target = R.random_walk(B, N, g)
    if A > 1:
        target = (target[:, :, None, :] + 1.5 * torch.randn(B, N, A, 3, generator=g)).reshape(B, N * A, 3)
    points = target + 1.0 * torch.randn(target.shape, generator=g)
    groups = None if A == 1 else torch.arange(N, dtype=torch.int32).repeat_interleave(A).expand(B, N * A).contiguous()
    return points.cuda(), target.cuda(), None if groups is None else groups.cuda()


def executed_pair_slots(target, groups, cutoff=15.0):
    """Lane slots of the first structure that run the pair's second half: 64 x the number of (64-owner wave, column)
    combinations in which at least one owner counts the column."""
    import torch
    t = target[0]
    M = t.shape[0]
    slots = 0
    for i0 in range(0, M, 64):
        d = torch.cdist(t[i0:i0 + 64], t)
        inc = d < cutoff
        idx = torch.arange(i0, min(i0 + 64, M), device=t.device)
        if groups is None:
            inc[torch.arange(idx.numel()), idx] = False
        else:
            inc &= groups[0][idx][:, None] != groups[0][None, :]
        slots += 64 * int(inc.any(0).sum())
    return slots


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "thresholds": list(ops.LDDT_THRESHOLDS), "cutoff": 15.0, "shapes": []}
    for name, B, N, A in SHAPES:
        x, t, groups = inputs(B, N, A)
        w = torch.randn(B, N * A, device="cuda")
        _, n = ops.lddt(x, t, None, groups)
        e = {"shape": name, "B": B, "M": N * A, "counted_pairs": int(n.sum().item()), "all_pairs": B * (N * A) ** 2,
             "executed_pair_slots": executed_pair_slots(t, groups) * B}
        e["hard_forward"] = timed(lambda: ops.lddt(x, t, None, groups))
        e["smooth_forward"] = timed(lambda: ops.lddt(x, t, None, groups, smooth=True))
        e["smooth_backward"] = timed(lambda: ops.lddt_backward(x, t, w, None, groups))
        report["shapes"].append(e)
        print(json.dumps(e), flush=True)
    with open(os.path.join(outdir, "lddt_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_trace(_outdir):
    import torch
    from protstruc_amd import ops
    for name, B, N, A in SHAPES:
        x, t, groups = inputs(B, N, A)
        w = torch.randn(B, N * A, device="cuda")
        for _ in range(10):
            ops.lddt(x, t, None, groups)
            ops.lddt(x, t, None, groups, smooth=True)
            ops.lddt_backward(x, t, w, None, groups)
        torch.cuda.synchronize()


def step_torch(outdir):
    import torch
    from tests import lddt_ref as R
    out = []
    for name, B, N, A in SHAPES:
        def measure(b):
            x, t, groups = inputs(b, N, A)
            leaf = x.clone().requires_grad_(True)

            def hard():
                with torch.no_grad():
                    return R.lddt(x, t, None, groups)

            def smooth():
                with torch.no_grad():
                    return R.lddt(x, t, None, groups, smooth=True)

            def both():
                S, _ = R.lddt(leaf, t, None, groups, smooth=True)
                return torch.autograd.grad(S.sum(), leaf)

            return {"hard_forward": timed(hard, 1, 3), "smooth_forward": timed(smooth, 1, 3),
                    "smooth_forward_and_backward": timed(both, 1, 3)}

        entry = {"shape": name, "B": B, "M": N * A, **largest_batch_that_fits(B, measure)}
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "lddt_time_torch.json"), "w") as f:
        json.dump(out, f, indent=1)


STEPS = {"events": step_events, "trace": step_trace, "torch": step_torch}


def finish(outdir):
    tracedir = os.path.join(outdir, "lddt_trace")
    with open(os.path.join(outdir, "lddt_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "lddt_time_torch.json")) as f:
        composed = {c["shape"]: c for c in json.load(f)}
    rows = kernel_stats(tracedir)
    if rows:    # reduced to the lDDT kernels' rows
        with open(os.path.join(outdir, "lddt_kernel_stats.csv"), "w", newline="") as f:
            csv.writer(f).writerows(rows[:1] + [r for r in rows[1:] if any("k_lddt" in c for c in r)])
    report["kernel_stats"] = "lddt_kernel_stats.csv" if rows else None
    shutil.rmtree(tracedir, ignore_errors=True)
    for e in report["shapes"]:
        c = composed[e["shape"]]
        e["composed_torch"] = c
        if c.get("batch"):
            scale = e["B"] / c["batch"]
            e["composed_hard_forward_over_kernel"] = c["hard_forward"]["median_us"] * scale / e["hard_forward"]["median_us"]
            e["composed_smooth_forward_over_kernel"] = c["smooth_forward"]["median_us"] * scale / e["smooth_forward"]["median_us"]
            e["composed_smooth_forward_and_backward_over_kernels"] = c["smooth_forward_and_backward"]["median_us"] * scale / (
                e["smooth_forward"]["median_us"] + e["smooth_backward"]["median_us"])
        t = e["smooth_forward"]["median_us"] * 1e-6
        e["smooth_forward_fraction_of_transcendental_issue_rate"] = e["executed_pair_slots"] * (3 + T) / TRANSCENDENTAL_LANES_PER_S / t
    os.remove(os.path.join(outdir, "lddt_time_events.json"))
    os.remove(os.path.join(outdir, "lddt_time_torch.json"))
    with open(os.path.join(outdir, "lddt_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "trace", "torch"), STEP_TIMEOUT_S, finish, trace_step="trace", trace_name="lddt")
