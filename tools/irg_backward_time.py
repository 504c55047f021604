#!/usr/bin/python3
"""The featuriser's backward kernel (ops.inter_residue_geometry_backward) at B=128, N=512 (BASELINE config 3) and B=64,
N=256, and write irg_backward_time.json, irg_backward_error.json and irg_backward_kernel_stats.csv into --outdir (default
profiles/).

    python3 tools/irg_backward_time.py [--outdir DIR] [--no-errors]

Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around every launch (3 warm-ups, median / min of 20): the backward kernel, the forward featuriser,
          and the read-traffic floor -- every upstream plane is read twice, 2 * 6 * 4 bytes per pair, at the rate of a
          device-to-device copy of 1 GiB measured in the same process
  trace   ten launches of each shape under ``rocprofv3 --kernel-trace --stats`` (``--step trace`` alone is the payload of
          a ``rocprofv3 --pmc`` run)
  torch   the composed-torch autograd backward of the restatement (tests/irg_grad_ref.py) in float32 on the same GPU, at
          the largest batch that fits (the full batch first, then halves: it keeps several (B,N,N,3) temporaries per plane
          alive), with the allocator's peak over that run; scaled to the full batch only where the full batch did not fit
  errors  E_kernel / E_f32 per accuracy case of tests/test_gpu_irg_backward.py
"""
import csv
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import copy_rate, kernel_stats, largest_batch_that_fits, main, timed

SHAPES = [(128, 512), (64, 256)]
A = 15
# Three times each step's duration on the MI355X, rounded up to the next 60 s.  Measured there: in the single-process tool
# this one replaces, loading torch and the library took 1.5 s, the events phase with its inputs 1.2 s, the composed run 1.9 s
# (the full batch fitted at both shapes), the errors 1.1 s, and the trace payload as a process of its own 2.9 s; as steps of
# this tool, events 3.3 s, trace under rocprofv3 3.3 s, torch 4.4 s, errors 3.1 s.
STEP_TIMEOUT_S = {"events": 60, "trace": 60, "torch": 60, "errors": 60}


def inputs(B, N, seed=1):
    import torch
    from tests import irg_grad_ref as R
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(B, N, A, 3, generator=g).cuda()
    mask = (torch.rand(B, N, A, generator=g) < 0.9).cuda()
    grads = {k: torch.randn(B, N, N, generator=g).cuda() for k in R.PLANES}
    return xyz, mask, grads


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    rate, rate_t = copy_rate()
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each launch; 3 warm-ups, median / min of 20",
              "copy_rate_bytes_per_s": rate, "copy": rate_t, "shapes": []}
    for B, N in SHAPES:
        xyz, mask, grads = inputs(B, N)
        out = torch.empty_like(xyz)
        entry = {"B": B, "N": N, "A": A, "pairs": B * N * N}
        entry["backward_all_six"] = timed(lambda: ops.inter_residue_geometry_backward(xyz, grads, mask, out=out))
        entry["backward_no_mask"] = timed(lambda: ops.inter_residue_geometry_backward(xyz, grads, None, out=out))
        entry["backward_d_cb_only"] = timed(lambda: ops.inter_residue_geometry_backward(xyz, {"d_cb": grads["d_cb"]}, mask, out=out))
        entry["backward_angles_only"] = timed(lambda: ops.inter_residue_geometry_backward(
            xyz, {k: grads[k] for k in ("omega", "theta", "phi")}, mask, out=out))
        entry["forward"] = timed(lambda: ops.inter_residue_geometry(xyz, mask))
        floor_us = 2 * 6 * 4 * B * N * N / rate * 1e6
        entry["read_traffic_floor_us"] = floor_us
        entry["backward_over_floor"] = entry["backward_all_six"]["median_us"] / floor_us
        entry["backward_over_forward"] = entry["backward_all_six"]["median_us"] / entry["forward"]["median_us"]
        report["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "irg_backward_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_trace(_outdir):
    import torch
    from protstruc_amd import ops
    for B, N in SHAPES:
        xyz, mask, grads = inputs(B, N)
        out = torch.empty_like(xyz)
        for _ in range(10):
            ops.inter_residue_geometry_backward(xyz, grads, mask, out=out)
            ops.inter_residue_geometry(xyz, mask)
        torch.cuda.synchronize()


def step_torch(outdir):
    """peak_bytes_allocated is the allocator's peak over building the graph and the timed backward passes alone"""
    import torch
    from tests import irg_grad_ref as R
    out = []
    for B, N in SHAPES:
        def measure(b):
            xyz, mask, grads = inputs(b, N)
            x = xyz.clone().requires_grad_(True)
            loss = R.weighted_sum(x, mask, grads)
            return timed(lambda: torch.autograd.grad(loss, x, retain_graph=True), warmup=2, reps=5)

        entry = largest_batch_that_fits(B, measure)
        if entry["batch"] not in (0, B):
            entry["scaled_to_full_batch_us"] = entry["median_us"] * B / entry["batch"]
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "irg_backward_time_torch.json"), "w") as f:
        json.dump(out, f, indent=1)


def step_errors(outdir):
    import torch
    from protstruc_amd import ops
    from tests import irg_grad_ref as R
    cases = [("15c8_HL",) + R.pdb_case(os.path.join(ROOT, "tests", "golden", "15c8_HL.pdb"))]
    for name, B, N, A_, kind, seed in R.accuracy_cases():
        cases.append((name,) + R.random_case(seed, B, N, A_, kind))
    out = []
    for name, xyz, mask, grads in cases:
        want = R.gradient(xyz, mask, grads)
        f32 = R.gradient(xyz, mask, grads, dtype=torch.float32)
        got = ops.inter_residue_geometry_backward(xyz.cuda(), {k: v.cuda() for k, v in grads.items()},
                                                  None if mask is None else mask.cuda()).cpu()
        ek, ef = R.worst_error(got, want), R.worst_error(f32, want)
        out.append({"case": name, "E_kernel": ek, "E_f32": ef, "ratio": ek / ef if ef else None})
        print(f"{name:40s} E_kernel {ek:.3e}  E_f32 {ef:.3e}  ratio {ek / ef if ef else float('nan'):.2f}", flush=True)
    with open(os.path.join(outdir, "irg_backward_error.json"), "w") as f:
        json.dump({"definition": "E = max over residues of (max |error| over the residue's entries / the residue's largest "
                                 "|gradient|), against the float64 autograd gradient of tests/irg_grad_ref.py; E_f32: the same "
                                 "restatement by float32 autograd on the CPU", "cases": out}, f, indent=1)


STEPS = {"events": step_events, "trace": step_trace, "torch": step_torch, "errors": step_errors}


def finish(outdir):
    with open(os.path.join(outdir, "irg_backward_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "irg_backward_time_torch.json")) as f:
        composed = json.load(f)
    for entry, c in zip(report["shapes"], composed):
        entry["composed_torch_autograd_backward"] = c
    tracedir = os.path.join(outdir, "irg_backward_trace")
    rows = kernel_stats(tracedir)
    if rows:    # reduced to the featuriser's kernels' rows
        with open(os.path.join(outdir, "irg_backward_kernel_stats.csv"), "w", newline="") as f:
            csv.writer(f).writerows(rows[:1] + [r for r in rows[1:] if any("k3_" in c for c in r)])
    shutil.rmtree(tracedir, ignore_errors=True)
    os.remove(os.path.join(outdir, "irg_backward_time_events.json"))
    os.remove(os.path.join(outdir, "irg_backward_time_torch.json"))
    with open(os.path.join(outdir, "irg_backward_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "trace", "torch", "errors"), STEP_TIMEOUT_S, finish, trace_step="trace",
         trace_name="irg_backward", optional=("errors",))
