#!/usr/bin/python3
"""Time the ensemble kernels (ops.rmsd_matrix, ops.cluster) and write profiles/ensemble_time.json.

    python3 tools/ensemble_time.py [--outdir DIR]

K45 in self mode at three shapes: B = 1024 members of M = 512 points, unmasked and with per-structure masks that leave out
10 % of the points (NaN in their place), and B = 1024 at M = 64, where the epilogue -- one 3x3 Jacobi solve per pair -- has
its largest share.  The members are noisy rigid copies of one cloud.  K46 at B = 1024 and B = 4096 items, points of the unit
square with a cutoff that gives a few dozen clusters.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  matrix     HIP events around each call (3 warm-ups, median / min of 20) of K45, with the fp64 fused multiply-adds of the
             pairs above the diagonal (17 per pair and point) per second as a fraction of the paper peak of the vector
             pipe, 78.6 TFLOP/s = 39.3e12 FMA/s
  superpose  the route through K37: ``ops.superpose`` over the same pairs above the diagonal, the coordinates broadcast
             over the pairs of 32 rows at a time (1 warm-up, median / min of 5 passes over the whole triangle)
  torch      the composed float32 route: the sums by ``einsum``, the singular values of the (B,B,3,3) covariances by a
             batched ``torch.linalg.svdvals`` -- cheaper than the full ``linalg.svd``, which the RMSD does not need, so
             the comparison errs in torch's favour --, at the largest B = 1024, 512, ... that fits; with how far its
             result is from K45's
  cluster    K46, both launches, with the number of clusters it found

No speed is asserted anywhere.  Not measured: any other shape, cross mode, the share of staging and of the epilogue inside
K45 (no counters were collected), the f64 MFMA alternative, the spread between runs and between machines.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import largest_batch_that_fits, main, timed

B = 1024
SHAPES = (("M512", 512, 0.0), ("M512_masked", 512, 0.1), ("M64", 64, 0.0))
PEAK_FMA_PER_S = 39.3e12      # 78.6 TFLOP/s fp64 vector, the data sheet's figure
ROWS = 32                     # the K37 route: pairs of 32 rows per launch
CLUSTER_SHAPES = ((1024, 0.12), (4096, 0.12))
STEP_TIMEOUT_S = {"matrix": 240, "superpose": 300, "torch": 300, "cluster": 240}


def inputs(batch, M, masked):
    """(a (batch,M,3), mask (batch,M) or None) on the GPU: noisy rigid copies of one cloud, NaN under the mask"""
    import torch
    g = torch.Generator().manual_seed(0)
    base = 2.5 * M ** (1 / 3) * torch.randn(M, 3, generator=g)
    q, _ = torch.linalg.qr(torch.randn(batch, 3, 3, generator=g))
    q = q * torch.sign(torch.linalg.det(q))[:, None, None]
    a = base[None] @ q.transpose(1, 2) + 10 * torch.randn(batch, 1, 3, generator=g) + 1.5 * torch.randn(batch, M, 3, generator=g)
    if not masked:
        return a.cuda(), None
    mask = torch.rand(batch, M, generator=g) >= masked
    a[~mask] = float("nan")
    return a.cuda(), mask.cuda()


def step_matrix(outdir):
    import torch
    from protstruc_amd import ops
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "peak_fma_per_s": PEAK_FMA_PER_S}
    for name, M, masked in SHAPES:
        a, mask = inputs(B, M, masked)
        t = timed(lambda: ops.rmsd_matrix(a, None, mask, None, return_count=True))
        fma = B * (B - 1) // 2 * M * 17
        report[name] = {"M": M, "masked": masked, "K45_rmsd_matrix_self": t, "fma_above_the_diagonal": fma,
                        "fraction_of_peak": fma / (t["median_us"] * 1e-6) / PEAK_FMA_PER_S}
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "ensemble_time_matrix.json"), "w") as f:
        json.dump(report, f, indent=1)


def superpose_triangle(ops, a, mask):
    """ops.superpose over the pairs above the diagonal, ROWS rows at a time; returns the last block's rmsd"""
    n, M = a.shape[:2]
    out = None
    for r0 in range(0, n, ROWS):
        rows, cols = a[r0:r0 + ROWS], a[r0:]
        R, C = rows.shape[0], cols.shape[0]
        x = rows[:, None].expand(R, C, M, 3).reshape(R * C, M, 3)
        y = cols[None, :].expand(R, C, M, 3).reshape(R * C, M, 3)
        both = None if mask is None else (mask[r0:r0 + ROWS, None] & mask[None, r0:]).reshape(R * C, M)
        out = ops.superpose(x, y, None, both)[2]
    return out


def step_superpose(outdir):
    from protstruc_amd import ops
    report = {"rows_per_launch": ROWS}
    for name, M, masked in SHAPES:
        a, mask = inputs(B, M, masked)
        report[name] = {"K37_over_the_triangle": timed(lambda: superpose_triangle(ops, a, mask), 1, 5)}
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "ensemble_time_superpose.json"), "w") as f:
        json.dump(report, f, indent=1)


def torch_matrix(a, mask):
    """The composed route in float32: the sums of every pair by einsum about each structure's own centroid, the batched
    singular values of the covariances, E0 - 2 (s0 + s1 + d s2); (B,B)"""
    import torch
    w = torch.ones(a.shape[:2], device=a.device) if mask is None else mask.float()
    x = torch.nan_to_num(a) * w[:, :, None]
    x = (x - x.sum(1, keepdim=True) / w.sum(1)[:, None, None]) * w[:, :, None]
    n = w @ w.t()
    s = torch.einsum("imc,jm->ijc", x, w)                      # sum over the common points of x_i, (B,B,3)
    q = torch.einsum("im,jm->ij", (x * x).sum(-1), w)
    H = torch.einsum("imc,jmd->ijcd", x, x) - s[:, :, :, None] * s.transpose(0, 1)[:, :, None, :] / n[:, :, None, None]
    e0 = q + q.t() - ((s * s).sum(-1) + (s.transpose(0, 1) ** 2).sum(-1)) / n
    sigma = torch.linalg.svdvals(H)
    d = torch.sign(torch.linalg.det(H))
    tr = sigma[..., 0] + sigma[..., 1] + d * sigma[..., 2]
    return ((e0 - 2 * tr) / n).clamp(min=0).sqrt()


def step_torch(outdir):
    import torch
    from protstruc_amd import ops
    report = {}
    for name, M, masked in SHAPES:
        a, mask = inputs(B, M, masked)

        def measure(b):
            x, m = a[:b], None if mask is None else mask[:b]
            with torch.no_grad():
                t = timed(lambda: torch_matrix(x, m), 1, 5)
                off = (torch_matrix(x, m) - ops.rmsd_matrix(x, None, m))
                off.diagonal().zero_()
            return {"torch_float32": t, "differs_from_K45_by_at_most": float(off.abs().max().item())}

        report[name] = largest_batch_that_fits(B, measure)
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "ensemble_time_torch.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_cluster(outdir):
    import torch
    from protstruc_amd import ops
    report = {}
    for n, cutoff in CLUSTER_SHAPES:
        g = torch.Generator().manual_seed(n)
        pts = torch.rand(n, 2, generator=g).cuda()
        D = torch.cdist(pts, pts)[None].contiguous()
        found = ops.cluster(D, cutoff)
        report[f"B{n}"] = {"B": n, "cutoff": cutoff, "n_clusters": int(found[3].item()), "largest": int(found[2][0, 0].item()),
                           "K46_cluster": timed(lambda: ops.cluster(D, cutoff))}
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "ensemble_time_cluster.json"), "w") as f:
        json.dump(report, f, indent=1)


STEPS = {"matrix": step_matrix, "superpose": step_superpose, "torch": step_torch, "cluster": step_cluster}
ORDER = ("matrix", "superpose", "torch", "cluster")


def finish(outdir):
    with open(os.path.join(outdir, "ensemble_time_matrix.json")) as f:
        report = json.load(f)
    for step in ORDER[1:]:
        with open(os.path.join(outdir, f"ensemble_time_{step}.json")) as f:
            part = json.load(f)
        if step == "cluster":
            report["cluster"] = part
            continue
        for name, _, _ in SHAPES:
            report[name].update(part[name])
        report.update({k: v for k, v in part.items() if k not in report and k not in [s[0] for s in SHAPES]})
    report["not_measured"] = ["other shapes", "cross mode", "the share of staging and of the epilogue inside K45",
                              "the f64 MFMA alternative", "the spread between runs and between machines"]
    for step in ORDER:
        os.remove(os.path.join(outdir, f"ensemble_time_{step}.json"))
    with open(os.path.join(outdir, "ensemble_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ORDER, STEP_TIMEOUT_S, finish)
