#!/usr/bin/python3
"""Time the lDDT kernels (ops.lddt hard and smooth, ops.lddt_backward) against the torch restatement of tests/lddt_ref.py
run in float32 on the same GPU, and write profiles/lddt_time.json and profiles/lddt_kernel_stats.csv.

    python3 tools/lddt_time.py [--outdir DIR]

Shapes: B = 128, M = 512 (one CA per residue) and B = 8, M = 512 * 14 (all atoms, the residue index as the group); the
composed version runs at the largest batch (B, B / 2, ...) that fits and the report says which.  Inputs are those of the
tests: a centred random walk with 3.8 A steps (for the all-atom shape each residue's 14 atoms are the walk's point plus
1.5 A of Gaussian scatter) and a prediction 1 A of Gaussian noise away.
The orchestrator never touches the GPU itself: every GPU step is a fresh child process of this file under its own
``timeout``, and the steps are chained -- the first one that fails, faults or runs out of time ends the run, and nothing
more is started on the card.

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
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def timed(fn, warmup=3, reps=20):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "reps": reps, "warmup": warmup}


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
        b, entry = B, {"shape": name, "B": B, "M": N * A, "batch": 0}
        while b >= 1:
            try:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
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

                entry.update(batch=b, hard_forward=timed(hard, 1, 3), smooth_forward=timed(smooth, 1, 3),
                             smooth_forward_and_backward=timed(both, 1, 3),
                             peak_bytes_allocated=torch.cuda.max_memory_allocated() - before, measured_at_full_batch=b == B)
                break
            except torch.cuda.OutOfMemoryError:
                x = t = groups = leaf = None
                torch.cuda.empty_cache()
                b //= 2
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "lddt_time_torch.json"), "w") as f:
        json.dump(out, f, indent=1)


STEPS = {"events": step_events, "trace": step_trace, "torch": step_torch}


def copy_kernel_stats(tracedir, dest):
    """rocprofv3's kernel_stats csv (wherever under ``tracedir`` it wrote it), reduced to the lDDT kernels' rows."""
    for path in glob.glob(os.path.join(tracedir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        keep = [rows[0]] + [r for r in rows[1:] if any("k_lddt" in c for c in r)]
        with open(dest, "w", newline="") as f:
            csv.writer(f).writerows(keep)
        return True
    return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    if args.step:
        import torch
        assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
        STEPS[args.step](args.outdir)
        return
    me = [sys.executable, os.path.abspath(__file__), "--outdir", args.outdir, "--step"]
    tracedir = os.path.join(args.outdir, "lddt_trace")
    for step in ("events", "trace", "torch"):
        cmd = me + [step]
        if step == "trace":
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tracedir, "-o", "lddt", "--"] + cmd
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step])] + cmd
        print("[lddt_time]", " ".join(cmd), flush=True)
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            sys.exit(f"[lddt_time] step {step} ended with status {rc}: nothing more is started on the GPU")
    with open(os.path.join(args.outdir, "lddt_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(args.outdir, "lddt_time_torch.json")) as f:
        composed = {c["shape"]: c for c in json.load(f)}
    report["kernel_stats"] = "lddt_kernel_stats.csv" if copy_kernel_stats(tracedir, os.path.join(args.outdir, "lddt_kernel_stats.csv")) else None
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
    os.remove(os.path.join(args.outdir, "lddt_time_events.json"))
    os.remove(os.path.join(args.outdir, "lddt_time_torch.json"))
    with open(os.path.join(args.outdir, "lddt_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
