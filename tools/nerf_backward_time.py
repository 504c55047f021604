#!/usr/bin/python3
"""The backbone builder's backward kernel (K12, ops.backbone_from_dihedrals_backward) at B=128, N=512 and B=64, N=256
(include_cb, A=15), and write nerf_backward_time.json, nerf_backward_error.json and nerf_backward_kernel_stats.csv into
--outdir (default profiles/).

    python3 tools/nerf_backward_time.py [--outdir DIR] [--no-errors] [--no-torch]

Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around every launch (3 warm-ups, median / min of 20): K12 -- dihedrals only, and all three outputs --,
          K7's forward (ops.backbone_from_dihedrals) at the same shapes, and the read-traffic floor: the rows of xyz and
          grad_xyz are fetched whole (the used slots share 128-byte lines with the others), 2 * B * N * A * 12 bytes, at
          the rate of a device-to-device copy of 1 GiB measured in the same process
  trace   ten launches of each shape under ``rocprofv3 --kernel-trace --stats`` (``--step trace`` alone is the payload of
          a ``rocprofv3 --pmc`` run)
  torch   what K12 replaces: the autograd backward of the torch restatement of the sequential walk
          (tests/nerf_grad_ref.py) in float32 on the same GPU at the same shapes (median of 5), and that restatement's
          forward (one run).  It is a walk over N with (B, 3) temporaries and fits at the full shape: no smaller batch
          is tried
  errors  E_kernel / E_f32 per accuracy case of tests/test_gpu_nerf_backward.py
"""
import csv
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import copy_rate, kernel_stats, main, timed

SHAPES = [(128, 512), (64, 256)]
A = 15
# Three times each step's duration on the MI355X, rounded up to the next 60 s.  Measured there: in the single-process tool
# this one replaces, loading torch and the library took 1.4 s, the events phase 0.3 s, the torch restatement 8.0 s, the 33
# error cases with their float64 and float32 CPU references 38.0 s, and the trace payload as a process of its own 2.2 s; as
# steps of this tool, events 2.3 s, trace under rocprofv3 2.5 s, torch 9.5 s, errors 43.2 s (3 x = 130 s).
STEP_TIMEOUT_S = {"events": 60, "trace": 60, "torch": 60, "errors": 180}


def inputs(B, N, seed=1):
    import torch
    from tests import nerf_ref
    dih = torch.from_numpy(nerf_ref.chain_family("random", B, N, seed)).cuda()
    g = torch.randn(B, N, A, 3, generator=torch.Generator().manual_seed(seed)).cuda()
    return dih, g


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    stale = os.path.join(outdir, "nerf_backward_time_torch.json")
    if os.path.exists(stale):    # of a run that failed later on: under --no-torch finish would merge it into this run's report
        os.remove(stale)
    rate, rate_t = copy_rate()
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each launch; 3 warm-ups, median / min of 20",
              "copy_rate_bytes_per_s": rate, "copy": rate_t, "shapes": []}
    for B, N in SHAPES:
        dih, g = inputs(B, N)
        xyz, _ = ops.backbone_from_dihedrals(dih, include_cb=True, n_slots=A)
        outs = tuple(torch.empty(B, N, 3, device="cuda") for _ in range(3))
        entry = {"B": B, "N": N, "A": A, "include_cb": True}
        entry["backward_dihedrals_only"] = timed(lambda: ops.backbone_from_dihedrals_backward(
            xyz, g, include_cb=True, out=(outs[0], None, None)))
        entry["backward_all_three"] = timed(lambda: ops.backbone_from_dihedrals_backward(
            xyz, g, include_cb=True, want_bond_angles=True, want_bond_lengths=True, out=outs))
        entry["forward_k7"] = timed(lambda: ops.backbone_from_dihedrals(dih, include_cb=True, n_slots=A))
        floor_us = 2 * B * N * A * 12 / rate * 1e6
        entry["read_traffic_floor_us"] = floor_us
        entry["backward_over_floor"] = entry["backward_all_three"]["median_us"] / floor_us
        entry["backward_over_forward"] = entry["backward_all_three"]["median_us"] / entry["forward_k7"]["median_us"]
        report["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "nerf_backward_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_trace(_outdir):
    import torch
    from protstruc_amd import ops
    for B, N in SHAPES:
        dih, g = inputs(B, N)
        xyz, _ = ops.backbone_from_dihedrals(dih, include_cb=True, n_slots=A)
        outs = tuple(torch.empty(B, N, 3, device="cuda") for _ in range(3))
        for _ in range(10):
            ops.backbone_from_dihedrals_backward(xyz, g, include_cb=True, want_bond_angles=True, want_bond_lengths=True, out=outs)
        torch.cuda.synchronize()


def step_torch(outdir):
    """forward (one run, wall clock after a synchronise) and autograd backward (HIP events, median of 5) of the float32
    restatement on the GPU at the full shape"""
    import torch
    from tests import nerf_grad_ref as R
    out = []
    for B, N in SHAPES:
        dih, g = inputs(B, N)
        ang, lens = (t.cuda() for t in R.geometry_or_default(B, N))
        d = dih.clone().requires_grad_(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xyz = R.build(d, None, None, ang, lens, True, A)
        loss = (g * xyz).sum()
        torch.cuda.synchronize()
        fwd = (time.perf_counter() - t0) * 1e6
        t = timed(lambda: torch.autograd.grad(loss, d, retain_graph=True), warmup=2, reps=5)
        out.append({"batch": B, "forward_wall_us": fwd, **t, "measured_at_full_shape": True})
        print(json.dumps(out[-1]), flush=True)
    with open(os.path.join(outdir, "nerf_backward_time_torch.json"), "w") as f:
        json.dump(out, f, indent=1)


def step_errors(outdir):
    import torch
    from protstruc_amd import ops
    from tests import nerf_grad_ref as R
    out = []
    for case in R.accuracy_cases():
        c = R.make_case(case)
        want, f32 = R.case_gradients(c, torch.float64), R.case_gradients(c, torch.float32)
        cu = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        xyz, _ = ops.backbone_from_dihedrals(cu["dihedrals"], cu["chain_idx"], cu["residue_mask"], cu["bond_angles"],
                                             cu["bond_lengths"], include_cb=c["include_cb"], n_slots=c["n_slots"])
        got = ops.backbone_from_dihedrals_backward(xyz, cu["grad_xyz"], cu["chain_idx"], cu["residue_mask"],
                                                   include_cb=c["include_cb"], want_bond_angles=True, want_bond_lengths=True)
        ek, ef = R.worst_error([t.cpu() for t in got], want), R.worst_error(f32, want)
        out.append({"case": case["name"], "B": case["B"], "E_kernel": ek, "E_f32": ef, "ratio": ek / ef if ef else None})
        print(f"{case['name']:50s} E_kernel {ek:.3e}  E_f32 {ef:.3e}  ratio {ek / ef if ef else float('nan'):.3f}", flush=True)
    with open(os.path.join(outdir, "nerf_backward_error.json"), "w") as f:
        json.dump({"definition": "per structure and output kind e = max |error| / max |gradient|, E = the largest e of the case, "
                                 "against the float64 autograd gradient of tests/nerf_grad_ref.py; E_f32: the same restatement "
                                 "by float32 autograd on the CPU", "cases": out}, f, indent=1)


STEPS = {"events": step_events, "trace": step_trace, "torch": step_torch, "errors": step_errors}


def finish(outdir):
    with open(os.path.join(outdir, "nerf_backward_time_events.json")) as f:
        report = json.load(f)
    os.remove(os.path.join(outdir, "nerf_backward_time_events.json"))
    composed = os.path.join(outdir, "nerf_backward_time_torch.json")
    if os.path.exists(composed):    # absent under --no-torch
        with open(composed) as f:
            for entry, c in zip(report["shapes"], json.load(f)):
                entry["torch_restatement_autograd_backward"] = c
                entry["torch_over_kernel"] = c["median_us"] / entry["backward_dihedrals_only"]["median_us"]
        os.remove(composed)
    tracedir = os.path.join(outdir, "nerf_backward_trace")
    rows = kernel_stats(tracedir)
    if rows:    # reduced to the backbone builder's kernels' rows
        with open(os.path.join(outdir, "nerf_backward_kernel_stats.csv"), "w", newline="") as f:
            csv.writer(f).writerows(rows[:1] + [r for r in rows[1:] if any("_backbone_from_dihedrals" in c for c in r)])
    shutil.rmtree(tracedir, ignore_errors=True)
    with open(os.path.join(outdir, "nerf_backward_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "trace", "torch", "errors"), STEP_TIMEOUT_S, finish, trace_step="trace",
         trace_name="nerf_backward", optional=("errors", "torch"))
