#!/usr/bin/python3
"""The backbone builder's backward kernel (K12, ops.backbone_from_dihedrals_backward) at B=128, N=512 and B=64, N=256
(include_cb, A=15): HIP events around every launch, 3 warm-ups, median / min of 20 -- dihedrals only, and all three
outputs.  Next to it, in the same process:
  (a) K7's forward (ops.backbone_from_dihedrals) at the same shapes;
  (b) what it replaces: the autograd backward of the torch restatement of the sequential walk (tests/nerf_grad_ref.py) in
      float32 on the same GPU at the same shapes (median of 5), and that restatement's forward (one run);
  (c) the read-traffic floor: the rows of xyz and grad_xyz are fetched whole (the used slots share 128-byte lines with the
      others), 2 * B * N * A * 12 bytes, at the copy rate measured here.
Writes nerf_backward_time.json and -- E_kernel / E_f32 per accuracy case of tests/test_gpu_nerf_backward.py --
nerf_backward_error.json into --outdir (default profiles/).

    python3 tools/nerf_backward_time.py [--outdir DIR] [--trace-only] [--no-errors] [--no-torch]

--trace-only: ten launches of each shape and nothing else (the payload of the rocprofv3 runs)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from protstruc_amd import ops
from tests import nerf_grad_ref as R
from tests import nerf_ref

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
    dih = torch.from_numpy(nerf_ref.chain_family("random", B, N, seed)).cuda()
    g = torch.randn(B, N, A, 3, generator=torch.Generator().manual_seed(seed)).cuda()
    return dih, g


def copy_rate():
    """bytes per second of a device-to-device copy of 1 GiB (read + write counted)"""
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src))
    return 2 * src.numel() * 4 / (t["median_us"] * 1e-6), t


def torch_restatement(B, N):
    """forward (one run, wall clock after a synchronise) and autograd backward (HIP events, median of 5) of the float32
    restatement on the GPU at the full shape"""
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
    return {"batch": B, "forward_wall_us": fwd, **t, "measured_at_full_shape": True}


def error_cases():
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--no-errors", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    if args.trace_only:
        for B, N in SHAPES:
            dih, g = inputs(B, N)
            xyz, _ = ops.backbone_from_dihedrals(dih, include_cb=True, n_slots=A)
            outs = tuple(torch.empty(B, N, 3, device="cuda") for _ in range(3))
            for _ in range(10):
                ops.backbone_from_dihedrals_backward(xyz, g, include_cb=True, want_bond_angles=True, want_bond_lengths=True, out=outs)
            torch.cuda.synchronize()
        return
    os.makedirs(args.outdir, exist_ok=True)
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
        if not args.no_torch:
            entry["torch_restatement_autograd_backward"] = torch_restatement(B, N)
            entry["torch_over_kernel"] = entry["torch_restatement_autograd_backward"]["median_us"] / entry["backward_dihedrals_only"]["median_us"]
        report["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(args.outdir, "nerf_backward_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    if not args.no_errors:
        with open(os.path.join(args.outdir, "nerf_backward_error.json"), "w") as f:
            json.dump({"definition": "per structure and output kind e = max |error| / max |gradient|, E = the largest e of the case, "
                                     "against the float64 autograd gradient of tests/nerf_grad_ref.py; E_f32: the same restatement "
                                     "by float32 autograd on the CPU", "cases": error_cases()}, f, indent=1)


if __name__ == "__main__":
    main()
