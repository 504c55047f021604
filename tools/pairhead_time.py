#!/usr/bin/python3
"""Time the pair-head kernels (K33 - K36: ops.pair_bins_distance / pair_bins_aligned_error, ops.binned_cross_entropy and its
backward, ops.binned_expectation) against the read-plus-write floor -- ``grad.copy_(logits)`` on the very buffers K35 used --
and against the composed torch route a user writes without them, and write profiles/pairhead_time.json.

    python3 tools/pairhead_time.py [--outdir DIR]

One shape: B = 128 structures of N = 512 residues, C = 64 bins -- 2^31 floats of logits, made on the device from a seed --,
points on a random walk with 3.8 A steps, frames from ``ops.frames``, 5 % of the rows and 5 % of the columns masked (10 % of
the pairs).  Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run
(tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20): K33 in both modes with and without ``value``, K34,
          K35 into a buffer allocated once, K36 with V = 1 and V = 2, and the copy on K35's buffers; each with the bytes the
          algorithm has to move, computed from the shapes, over its median time
  torch   the composed route at the largest batch (B, B / 2, ...) that fits, with the allocator's peak of each part: the
          bins by broadcasting, ``F.cross_entropy`` forward, forward plus backward, ``softmax @ values``

No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import largest_batch_that_fits, main, timed

B, N, C = 128, 512, 64
STEP_TIMEOUT_S = {"events": 300, "torch": 400}


def geometry_inputs(batch):
    """points, frames of a chain and of a target 1 A away from it, and the two masks, on the GPU"""
    import torch
    from protstruc_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    steps = torch.randn(batch, N, 3, device="cuda", generator=g)
    ca = torch.cumsum(3.8 * steps / steps.norm(dim=-1, keepdim=True), dim=1)
    arms = torch.randn(batch, N, 2, 3, device="cuda", generator=g)
    arms = 1.5 * arms / arms.norm(dim=-1, keepdim=True)
    backbone = torch.stack([ca + arms[:, :, 0], ca, ca + arms[:, :, 1]], dim=2)
    target = backbone + torch.randn(backbone.shape, device="cuda", generator=g)
    rot, trans = ops.frames(backbone, 0, 1, 2, 1)
    trot, ttrans = ops.frames(target, 0, 1, 2, 1)
    row = torch.rand(batch, N, device="cuda", generator=g) >= 0.05
    col = torch.rand(batch, N, device="cuda", generator=g) >= 0.05
    return dict(rot=rot, trans=trans, points=backbone[:, :, 1].contiguous(), target_rot=trot, target_trans=ttrans,
                target_points=target[:, :, 1].contiguous(), row=row, col=col)


def logits_inputs(batch):
    import torch
    g = torch.Generator(device="cuda").manual_seed(2)
    return torch.randn(batch, N, N, C, device="cuda", generator=g)


def tables(batch, V):
    import torch
    from protstruc_amd import geometry
    centers = geometry.aligned_error_bin_centers(n_bins=C).float().cuda()
    return torch.stack([centers, 1.0 / (1.0 + (centers / 8.0) ** 2)])[:V].expand(batch, V, C).contiguous()


def with_rate(record, n_bytes):
    return {**record, "bytes": n_bytes, "bytes_per_s": n_bytes / (record["median_us"] * 1e-6)}


def step_events(outdir):
    import torch
    from protstruc_amd import _lib, geometry, ops
    geo = geometry_inputs(B)
    frames = [geo[k] for k in ("rot", "trans", "points", "target_rot", "target_trans", "target_points")]
    d_breaks, e_breaks = geometry.distogram_breaks(n_bins=C), geometry.aligned_error_breaks(n_bins=C)
    pairs = B * N * N
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "C": C, "logits_bytes": pairs * C * 4}
    report["K33"] = {
        "distance_bins": with_rate(timed(lambda: ops.pair_bins_distance(geo["points"], d_breaks, geo["row"], geo["col"])), pairs),
        "distance_bins_and_value": with_rate(timed(lambda: ops.pair_bins_distance(geo["points"], d_breaks, geo["row"], geo["col"],
                                                                                   return_value=True)), pairs * 5),
        "aligned_error_bins": with_rate(timed(lambda: ops.pair_bins_aligned_error(*frames, e_breaks, geo["row"], geo["col"])), pairs),
        "aligned_error_bins_and_value": with_rate(timed(lambda: ops.pair_bins_aligned_error(*frames, e_breaks, geo["row"], geo["col"],
                                                                                            return_value=True)), pairs * 5)}
    bins = ops.pair_bins_aligned_error(*frames, e_breaks, geo["row"], geo["col"])
    report["pairs_without_a_target"] = float((bins == ops.PAIRHEAD_NO_TARGET).float().mean().item())
    logits = logits_inputs(B)
    grad = torch.empty_like(logits)
    grad_row = torch.randn(B, N, device="cuda")
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream

    def backward():
        rc = lib.ps_binned_cross_entropy_backward_f32(logits.data_ptr(), bins.data_ptr(), grad_row.data_ptr(), grad.data_ptr(),
                                                      B, N, C, stream)
        assert rc == 0

    report["K34"] = with_rate(timed(lambda: ops.binned_cross_entropy(logits, bins)), pairs * (C * 4 + 1))
    report["K35"] = with_rate(timed(backward), pairs * (2 * C * 4 + 1))
    report["copy_on_the_buffers_of_K35"] = with_rate(timed(lambda: grad.copy_(logits)), pairs * 2 * C * 4)
    for V in (1, 2):
        values = tables(B, V)
        report[f"K36_V{V}"] = with_rate(timed(lambda: ops.binned_expectation(logits, values)), pairs * (C * 4 + V * 4))
    copy = report["copy_on_the_buffers_of_K35"]["median_us"]
    report["K35_over_copy"] = report["K35"]["median_us"] / copy
    report["K34_over_half_copy"] = report["K34"]["median_us"] / (copy / 2)
    report["K36_V1_over_half_copy"] = report["K36_V1"]["median_us"] / (copy / 2)
    report["K36_V2_over_half_copy"] = report["K36_V2"]["median_us"] / (copy / 2)
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "pairhead_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def composed_bins(points, breaks, row, col):
    """AlphaFold's route: the (B,N,N,3) differences, their squares summed, compared with the squared breaks"""
    import torch
    d2 = (points[:, None, :, :] - points[:, :, None, :]).square().sum(-1, keepdim=True)
    bins = (d2 > breaks.square()).sum(-1)
    return torch.where(row[:, :, None] & col[:, None, :], bins, torch.full_like(bins, -100))


def step_torch(outdir):
    import torch
    import torch.nn.functional as F
    from protstruc_amd import geometry

    breaks = geometry.distogram_breaks(n_bins=C).cuda()
    report = {}

    def part(name, build):
        """``build(b)`` returns the callable to time at batch b; its inputs are allocated before the peak is reset"""
        def measure(b):
            fn = build(b)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            return {"composed": timed(fn, 1, 3), "inputs_bytes": torch.cuda.memory_allocated()}
        report[name] = largest_batch_that_fits(B, measure)
        print(name, json.dumps(report[name]), flush=True)

    def bins_route(b):
        geo = geometry_inputs(b)
        return lambda: composed_bins(geo["points"], breaks, geo["row"], geo["col"])

    def labels_of(b):
        geo = geometry_inputs(b)
        return composed_bins(geo["points"], breaks, geo["row"], geo["col"])

    def forward_route(b):
        logits, labels = logits_inputs(b), labels_of(b)
        return lambda: F.cross_entropy(logits.view(-1, C), labels.view(-1), ignore_index=-100, reduction="sum")

    def forward_backward_route(b):
        logits, labels = logits_inputs(b).requires_grad_(True), labels_of(b)

        def run():
            logits.grad = None
            F.cross_entropy(logits.view(-1, C), labels.view(-1), ignore_index=-100, reduction="sum").backward()
        return run

    def expectation_route(b):
        logits, values = logits_inputs(b), tables(b, 2)
        return lambda: torch.einsum("bijk,bvk->vbij", torch.softmax(logits, dim=-1), values)

    with torch.no_grad():
        part("bins_by_broadcasting", bins_route)
        part("softmax_at_values_V2", expectation_route)
    part("cross_entropy_forward", forward_route)
    part("cross_entropy_forward_and_backward", forward_backward_route)
    with open(os.path.join(outdir, "pairhead_time_torch.json"), "w") as f:
        json.dump(report, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "pairhead_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "pairhead_time_torch.json")) as f:
        composed = json.load(f)
    report["composed_torch"] = composed

    def scaled(name):
        c = composed[name]
        return c["composed"]["median_us"] * (B / c["batch"]) if c.get("batch") else None

    ratios = {}
    for name, ours in (("bins_by_broadcasting", report["K33"]["distance_bins"]["median_us"]),
                       ("cross_entropy_forward", report["K34"]["median_us"]),
                       ("cross_entropy_forward_and_backward", report["K34"]["median_us"] + report["K35"]["median_us"]),
                       ("softmax_at_values_V2", report["K36_V2"]["median_us"])):
        if scaled(name) is not None:
            ratios[name] = scaled(name) / ours
    report["composed_over_kernel"] = ratios
    os.remove(os.path.join(outdir, "pairhead_time_events.json"))
    os.remove(os.path.join(outdir, "pairhead_time_torch.json"))
    with open(os.path.join(outdir, "pairhead_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
