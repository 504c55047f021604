#!/usr/bin/python3
"""Time the clash kernels (ops.clash, ops.clash_backward) against the torch restatement of tests/violation_ref.py run in
float32 with autograd on the same GPU, and write profiles/violation_time.json.

    python3 tools/violation_time.py [--outdir DIR]

Shapes: B = 8, M = 512 * 15 = 7680 (all atoms of 512 residues) and B = 128, M = 512 * 5 = 2560 (backbone + CB), the
residue index as the group; the composed version runs at the largest batch (B, B / 2, ...) that fits and the report says
which.  Inputs: a centred random walk of residues with 3.8 A steps, each residue's atoms the walk's point plus 1.5 A of
Gaussian scatter, radii drawn from the four element values -- a structure before any violation loss has acted on it, with
a clash at a few per cent of the atoms.
The orchestrator never touches the GPU itself: every GPU step is a fresh child process of this file under its own
``timeout``, and the steps are chained -- the first one that fails, faults or runs out of time ends the run, and nothing
more is started on the card.

  events  HIP events around each call (3 warm-ups, median / min of 20), K17 and K18
  torch   the composed float32 restatement (forward; forward + autograd backward) with the allocator's peak

Reported per shape: the times, the number of clashing pairs, and the ratio to the composed version (scaled to the full
batch where the composed version had to run at a smaller one).  No speed is asserted anywhere.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
        b, entry = B, {"shape": name, "B": B, "M": N * A, "batch": 0}
        while b >= 1:
            try:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                x, r, groups = inputs(b, N, A)
                leaf = x.clone().requires_grad_(True)

                def forward():
                    with torch.no_grad():
                        return R.clash(x, r, None, groups)

                def both():
                    E, _ = R.clash(leaf, r, None, groups)
                    return torch.autograd.grad(E.sum(), leaf)

                entry.update(batch=b, forward=timed(forward, 1, 3), forward_and_backward=timed(both, 1, 3),
                             peak_bytes_allocated=torch.cuda.max_memory_allocated() - before, measured_at_full_batch=b == B)
                break
            except torch.cuda.OutOfMemoryError:
                x = r = groups = leaf = None
                torch.cuda.empty_cache()
                b //= 2
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "violation_time_torch.json"), "w") as f:
        json.dump(out, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


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
    for step in ("events", "torch"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step])] + me + [step]
        print("[violation_time]", " ".join(cmd), flush=True)
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            sys.exit(f"[violation_time] step {step} ended with status {rc}: nothing more is started on the GPU")
    with open(os.path.join(args.outdir, "violation_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(args.outdir, "violation_time_torch.json")) as f:
        composed = {c["shape"]: c for c in json.load(f)}
    for e in report["shapes"]:
        c = composed[e["shape"]]
        e["composed_torch"] = c
        if c.get("batch"):
            scale = e["B"] / c["batch"]
            e["composed_forward_over_kernel"] = c["forward"]["median_us"] * scale / e["forward"]["median_us"]
            e["composed_forward_and_backward_over_kernels"] = c["forward_and_backward"]["median_us"] * scale / (
                e["forward"]["median_us"] + e["backward"]["median_us"])
    os.remove(os.path.join(args.outdir, "violation_time_events.json"))
    os.remove(os.path.join(args.outdir, "violation_time_torch.json"))
    with open(os.path.join(args.outdir, "violation_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
