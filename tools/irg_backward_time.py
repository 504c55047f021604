#!/usr/bin/python3
"""The featuriser's backward kernel (ops.inter_residue_geometry_backward) at B=128, N=512 (BASELINE config 3) and B=64,
N=256: HIP events around every launch, 3 warm-ups, median / min of 20.  Next to it, in the same process:
  (a) the forward featuriser;
  (b) the composed-torch autograd backward of the restatement (tests/irg_grad_ref.py) in float32 on the same GPU, at the
      largest batch that fits (the full batch first, then halves: it keeps several (B,N,N,3) temporaries per plane alive),
      with the allocator's peak over that run; scaled to the full batch only where the full batch did not fit;
  (c) the read-traffic floor: every upstream plane is read twice, 2 * 6 * 4 bytes per pair, at the copy rate measured here.
Writes irg_backward_time.json and -- E_kernel / E_f32 per accuracy case of tests/test_gpu_irg_backward.py --
irg_backward_error.json into --outdir (default profiles/).

    python3 tools/irg_backward_time.py [--outdir DIR] [--trace-only] [--no-errors]

--trace-only: ten launches of each shape and nothing else (the payload of a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from protstruc_amd import ops
from tests import irg_grad_ref as R

SHAPES = [(128, 512), (64, 256)]
A = 15


def timed(fn, warmup=3, reps=20):
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


def inputs(B, N, seed=1):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(B, N, A, 3, generator=g).cuda()
    mask = (torch.rand(B, N, A, generator=g) < 0.9).cuda()
    grads = {k: torch.randn(B, N, N, generator=g).cuda() for k in R.PLANES}
    return xyz, mask, grads


def copy_rate():
    """bytes per second of a device-to-device copy of 1 GiB (read + write counted)"""
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src))
    return 2 * src.numel() * 4 / (t["median_us"] * 1e-6), t


def composed_torch(B, N):
    """autograd backward of the float32 restatement on the GPU, at the largest batch (B, B / 2, B / 4, ...) that fits;
    peak_bytes_allocated is the allocator's peak over building the graph and the timed backward passes alone"""
    b = B
    while b >= 1:
        try:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            xyz, mask, grads = inputs(b, N)
            x = xyz.clone().requires_grad_(True)
            loss = R.weighted_sum(x, mask, grads)
            t = timed(lambda: torch.autograd.grad(loss, x, retain_graph=True), warmup=2, reps=5)
            peak = torch.cuda.max_memory_allocated() - before
            del loss, x, xyz, mask, grads
            torch.cuda.empty_cache()
            out = {"batch": b, **t, "peak_bytes_allocated": peak, "measured_at_full_batch": b == B}
            if b != B:
                out["scaled_to_full_batch_us"] = t["median_us"] * B / b
            return out
        except torch.cuda.OutOfMemoryError:
            loss = x = xyz = mask = grads = None
            torch.cuda.empty_cache()
            b //= 2
    return {"batch": 0}


def error_cases():
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--no-errors", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    if args.trace_only:
        for B, N in SHAPES:
            xyz, mask, grads = inputs(B, N)
            out = torch.empty_like(xyz)
            for _ in range(10):
                ops.inter_residue_geometry_backward(xyz, grads, mask, out=out)
                ops.inter_residue_geometry(xyz, mask)
            torch.cuda.synchronize()
        return
    os.makedirs(args.outdir, exist_ok=True)
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
        del grads, out, xyz, mask
        torch.cuda.empty_cache()
        entry["composed_torch_autograd_backward"] = composed_torch(B, N)
        report["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(args.outdir, "irg_backward_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    if not args.no_errors:
        with open(os.path.join(args.outdir, "irg_backward_error.json"), "w") as f:
            json.dump({"definition": "E = max over residues of (max |error| over the residue's entries / the residue's largest "
                                     "|gradient|), against the float64 autograd gradient of tests/irg_grad_ref.py; E_f32: the same "
                                     "restatement by float32 autograd on the CPU", "cases": error_cases()}, f, indent=1)


if __name__ == "__main__":
    main()
