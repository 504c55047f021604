#!/usr/bin/python3
"""Time the frame-aligned point error kernels (ops.fape, ops.fape_backward, ops.frames_backward) and write
profiles/fape_time.json and profiles/fape_error.json.

    python3 tools/fape_time.py [--outdir DIR]

Shapes: B = 128, N = 512 with the backbone atoms as points (M = 1536) -- timed twice, as the gathered (B, 1536, 3) tensor
and as the (B, 7680, 3) view of all 15 slots with the other twelve masked -- and B = 16, N = 512 with all 15 slots under a
p = 0.9 atom mask (M = 7680 passed, ~6950 valid).
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20): forward, backward (all three gradients, the frame
          side alone, the point side alone), K4 and its backward
  trace   the same launches under ``rocprofv3 --kernel-trace --stats``: the kernels' own times, without launch overhead
  torch   the composed-torch float32 FAPE of tests/fape_ref.py with autograd on the same GPU, at the largest batch
          (B, B / 2, ...) that fits, with the allocator's peak
  errors  E_kernel / E_f32 of every accuracy case of tests/test_gpu_fape.py

Reported per shape: the times, the ratio to composed torch, and pairs per second against the VALU issue bound DESIGN.md
quotes for K3 (2.08 ns per wave instruction per SIMD on 256 CUs x 4 SIMDs), with the instructions per pair counted in the
kernels' inner loops (FWD_VALU_PER_PAIR, BWD_*_VALU_PER_PAIR below).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import kernel_stats, largest_batch_that_fits, main, timed

SHAPES = [(128, 512, 3), (16, 512, 15)]       # B, N, atom slots used as points (composed torch and the trace)
# the timed calls: (name, B, N, slots used, points passed as the 15-slot view + mask / gathered without a mask)
CALLS = [("backbone_gathered", 128, 512, 3, False), ("backbone_slot_view", 128, 512, 3, True), ("all_slots_view", 16, 512, 15, True)]
STEP_TIMEOUT_S = {"events": 240, "trace": 300, "torch": 240, "errors": 300}
# VALU instructions per pair in the inner loops: two differences (6), two R^T v (18), u - u' (3), squared length + eps (4),
# the correctly rounded square root (9), then -- forward: min, subtract, add (3); backward: compare / reciprocal / select
# (3), e (3) and the frame side's twelve accumulations or the point side's R e and three additions (12)
FWD_VALU_PER_PAIR = 43
BWD_FRAME_VALU_PER_PAIR = 58
BWD_POINT_VALU_PER_PAIR = 58
WAVE_INSTRUCTIONS_PER_S = 256 * 4 / 2.08e-9


def inputs(B, N, A, seed=1):
    import torch
    g = torch.Generator().manual_seed(seed)
    target = 8 * torch.randn(B, N, 15, 3, generator=g)
    xyz = target + 4 * torch.randn(B, N, 15, 3, generator=g)
    atom_mask = torch.rand(B, N, 15, generator=g) < 0.9
    atom_mask[:, :, :3] = True
    if A < 15:
        atom_mask[:, :, A:] = False
    return xyz.cuda(), target.cuda(), atom_mask.cuda()


def operands(xyz, target, atom_mask, gather=0):
    """The six tensors and the point mask of a call; ``gather`` > 0: the first ``gather`` slots as a tensor of their own,
    every point valid (those slots are never masked by ``inputs``)."""
    from protstruc_amd import ops
    if gather:
        xyz, target, atom_mask = xyz[:, :, :gather].contiguous(), target[:, :, :gather].contiguous(), None
    B, N, A = xyz.shape[:3]
    rot, trans = ops.frames(xyz, 0, 1, 2, 1)
    trot, ttrans = ops.frames(target, 0, 1, 2, 1)
    return ([rot, trans, xyz.reshape(B, N * A, 3), trot, ttrans, target.reshape(B, N * A, 3)],
            None if atom_mask is None else atom_mask.reshape(B, N * A))


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "shapes": []}
    for name, B, N, A, view in CALLS:
        xyz, target, atom_mask = inputs(B, N, A)
        args, pm = operands(xyz, target, atom_mask, 0 if view else A)
        g = torch.ones(B, device="cuda")
        g_rot, g_trans = torch.randn(B, N, 3, 3, device="cuda"), torch.randn(B, N, 3, device="cuda")
        _, count = ops.fape(*args, None, pm)
        M = args[2].shape[1]
        e = {"call": name, "B": B, "N": N, "M_passed": M,
             "M_valid_mean": M if pm is None else float(pm.sum().item()) / B, "pairs": int(count.sum().item())}
        e["forward"] = timed(lambda: ops.fape(*args, None, pm))
        e["backward"] = timed(lambda: ops.fape_backward(*args, g, None, pm))
        e["backward_frames_only"] = timed(lambda: ops.fape_backward(*args, g, None, pm, want_points=False))
        e["backward_points_only"] = timed(lambda: ops.fape_backward(*args, g, None, pm, want_rot=False, want_trans=False))
        e["k4_forward"] = timed(lambda: ops.frames(xyz, 0, 1, 2, 1))
        e["k4_backward"] = timed(lambda: ops.frames_backward(xyz, 0, 1, 2, 1, grad_rot=g_rot, grad_trans=g_trans))
        report["shapes"].append(e)
        print(json.dumps(e), flush=True)
    with open(os.path.join(outdir, "fape_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_trace(_outdir):
    import torch
    from protstruc_amd import ops
    for B, N, A in SHAPES:
        xyz, target, atom_mask = inputs(B, N, A)
        args, pm = operands(xyz, target, atom_mask)
        g = torch.ones(B, device="cuda")
        for _ in range(10):
            ops.fape(*args, None, pm)
            ops.fape_backward(*args, g, None, pm)
        torch.cuda.synchronize()


def step_torch(outdir):
    import torch
    from tests import fape_ref as R
    out = []
    for B, N, A in SHAPES:
        def measure(b):
            xyz, target, atom_mask = inputs(b, N, A)
            # composed torch gathers the valid slots first: it has no use for masked points
            x, t = xyz[:, :, :A].contiguous(), target[:, :, :A].contiguous()
            args = [a.clone() for a in operands(x, t, atom_mask[:, :, :A].contiguous())[0]]
            leaves = [a.requires_grad_(True) for a in args[:3]]

            def both():
                loss, _ = R.fape(*leaves, *args[3:])
                return torch.autograd.grad(loss.sum(), leaves)

            def forward():
                with torch.no_grad():
                    return R.fape(*args)

            return {"forward": timed(forward, 2, 5), "forward_and_backward": timed(both, 2, 5)}

        entry = {"B": B, "N": N, "M": N * A, "points": "the first A slots gathered, every one of them valid (no mask)",
                 **largest_batch_that_fits(B, measure)}
        out.append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "fape_time_torch.json"), "w") as f:
        json.dump(out, f, indent=1)


def step_errors(outdir):
    import torch
    from protstruc_amd import ops
    from tests import fape_ref as R
    cases = []
    for name, *rest in R.accuracy_cases():
        case = R.random_case(*rest)
        args = [t.cuda() for t in case.operands()]
        kw = dict(frame_mask=None if case.frame_mask is None else case.frame_mask.cuda(),
                  point_mask=None if case.point_mask is None else case.point_mask.cuda(), clamp=case.clamp.cuda())
        got = ops.fape_backward(*args, case.grad_loss.cuda(), **kw)
        want, f32 = R.gradient(case), R.gradient(case, torch.float32)
        entry = {"case": name}
        for what, g, w, f in zip(("grad_rot", "grad_trans", "grad_pts"), got, want, f32):
            ek, ef = R.worst_error(g.cpu(), w), R.worst_error(f, w)
            entry[what] = {"E_kernel": ek, "E_f32": ef, "ratio": ek / ef if ef else None}
        loss, _ = ops.fape(*args, **kw)
        l64, l32 = R.loss(case)[0], R.loss(case, torch.float32)[0]
        live = l64 != 0
        rel = lambda l: float(((l.cpu().double() - l64).abs()[live] / l64[live]).max()) if live.any() else 0.0  # noqa: E731
        entry["loss"] = {"E_kernel": rel(loss), "E_f32": rel(l32)}
        cases.append(entry)
        print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "fape_error.json"), "w") as f:
        json.dump({"definition": "gradients: E = max over rows (frames / points) of (max |error| over the row / the row's largest "
                                 "|gradient|) against the float64 autograd gradient of tests/fape_ref.py; loss: E = max_b |loss_b - "
                                 "loss64_b| / loss64_b; E_f32: the same restatement in float32 on the CPU", "cases": cases}, f, indent=1)


STEPS = {"events": step_events, "trace": step_trace, "torch": step_torch, "errors": step_errors}


def kernel_trace_times(tracedir):
    """kernel name -> {calls, average_us} from rocprofv3's kernel statistics under ``tracedir``, in either of the column
    spellings rocprofv3 has used."""
    out = {}
    header, *rows = kernel_stats(tracedir) or [[]]
    for row in (dict(zip(header, r)) for r in rows):
        name = row.get("name", "")
        for key in ("k_fape_forward", "k_fape_finish", "k_fape_backward", "k4_frames"):
            if key + "(" in name or name.endswith(key):
                calls = int(row.get("total_calls") or row.get("calls"))
                total_ns = float(row.get("total_duration") or row.get("totaldurationns"))
                out[key] = {"calls": calls, "average_us": total_ns / calls / 1e3}
    return out


def finish(outdir):
    tracedir = os.path.join(outdir, "fape_trace")
    with open(os.path.join(outdir, "fape_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "fape_time_torch.json")) as f:
        composed = json.load(f)
    report["kernel_trace"] = {"method": "rocprofv3 --kernel-trace --stats over 10 forward + 10 backward calls per shape; the "
                                        "average is over both shapes' launches", **kernel_trace_times(tracedir)}
    by_shape = {(c["B"], c["M"] // c["N"]): c for c in composed}
    slots = {name: A for name, _, _, A, _ in CALLS}
    for e in report["shapes"]:
        c = by_shape[(e["B"], slots[e["call"]])]
        e["composed_torch"] = c
        if c.get("batch"):
            scale = e["B"] / c["batch"]
            e["composed_torch_forward_over_kernel"] = c["forward"]["median_us"] * scale / e["forward"]["median_us"]
            e["composed_torch_forward_and_backward_over_kernels"] = c["forward_and_backward"]["median_us"] * scale / (
                e["forward"]["median_us"] + e["backward"]["median_us"])
        pairs = e["pairs"]
        for key, valu, sweeps in (("forward", FWD_VALU_PER_PAIR, 1), ("backward", BWD_FRAME_VALU_PER_PAIR + BWD_POINT_VALU_PER_PAIR, 1)):
            t = e[key]["median_us"] * 1e-6
            e[key + "_pairs_per_s"] = pairs * sweeps / t
            e[key + "_fraction_of_valu_issue_bound"] = pairs * valu / 64 / WAVE_INSTRUCTIONS_PER_S / t
    os.remove(os.path.join(outdir, "fape_time_events.json"))
    os.remove(os.path.join(outdir, "fape_time_torch.json"))
    with open(os.path.join(outdir, "fape_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "trace", "torch", "errors"), STEP_TIMEOUT_S, finish, trace_step="trace", trace_name="fape")
