#!/usr/bin/python3
"""Time the superposition kernels (ops.superpose, ops.superpose_backward, ops.superpose_search) and write
profiles/superpose_time.json.

    python3 tools/superpose_time.py [--outdir DIR]

One shape: B = 128 structures of N = 512 points, 10 % of them masked with NaN coordinates; the model is the target moved
rigidly plus noise that grows from 0.2 A to 6 A along the chain, so that the chains of the search neither stop at once
nor all run to their limit.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  fit     HIP events around each call (3 warm-ups, median / min of 20): K37, K38, and the composed route at the same batch --
          a batched ``torch.linalg.svd`` Kabsch RMSD in float32, forwards, and forwards plus ``backward()``
  search  K39 + K40 for the six-objective launch (TM and the counts at 0.5, 1, 2, 4, 8 A) and for TM alone, with the chains
          run and an upper bound of chains x iterations per second (every chain counted at its limit of 20 iterations: the
          kernels do not report how many a chain took)

No speed is asserted anywhere.  Not measured: the number of iterations the chains actually take, the share of K40 in the
search's time, any other shape, the spread between runs and boxes.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import main, timed

B, N = 128, 512
MASKED = 0.1
STEP_TIMEOUT_S = {"fit": 240, "search": 300}


def inputs(batch):
    """(a (batch,N,3), b (batch,N,3), mask (batch,N)) on the GPU, NaN under the mask"""
    import torch
    g = torch.Generator().manual_seed(0)
    b = 2.5 * N ** (1 / 3) * torch.randn(batch, N, 3, generator=g)
    q, _ = torch.linalg.qr(torch.randn(batch, 3, 3, generator=g))
    q = q * torch.sign(torch.linalg.det(q))[:, None, None]
    sigma = torch.logspace(-0.7, 0.78, N)[None, :, None]
    a = b @ q.transpose(1, 2) + 10 * torch.randn(batch, 1, 3, generator=g) + sigma * torch.randn(batch, N, 3, generator=g)
    mask = torch.rand(batch, N, generator=g) >= MASKED
    a[~mask], b[~mask] = float("nan"), float("nan")
    return a.cuda(), b.cuda(), mask.cuda()


def svd_rmsd(a, b, mask):
    """The route a user writes without the kernels: masked batched Kabsch by torch.linalg.svd, then the RMSD, (B,) float32"""
    import torch
    w = mask.float()[:, :, None]
    a, b = torch.nan_to_num(a) * w, torch.nan_to_num(b) * w
    n = w.sum(dim=1)
    ca, cb = a.sum(dim=1) / n, b.sum(dim=1) / n
    x, y = (a - ca[:, None]) * w, (b - cb[:, None]) * w
    U, _, Vt = torch.linalg.svd(x.transpose(1, 2) @ y)
    V = Vt.transpose(1, 2)
    d = torch.sign(torch.linalg.det(V @ U.transpose(1, 2)))
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1))
    R = V @ D @ U.transpose(1, 2)
    e = x @ R.transpose(1, 2) - y
    return ((e ** 2).sum(dim=(1, 2)) / n[:, 0]).sqrt()


def step_fit(outdir):
    import torch
    from protstruc_amd import ops
    a, b, mask = inputs(B)
    fit = ops.superpose(a, b, None, mask)
    g = torch.ones(B, device="cuda")
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "points_that_count": int(mask.sum().item()),
              "K37_superpose": timed(lambda: ops.superpose(a, b, None, mask)),
              "K38_superpose_backward": timed(lambda: ops.superpose_backward(a, b, None, mask, *fit, g))}
    with torch.no_grad():
        report["torch_svd_forward"] = timed(lambda: svd_rmsd(a, b, mask))
    x = a.clone().requires_grad_(True)
    y = b.clone().requires_grad_(True)

    def both():
        x.grad = y.grad = None
        svd_rmsd(x, y, mask).sum().backward()

    report["torch_svd_forward_backward"] = timed(both)
    report["rmsd_differs_from_torch_float32_by_at_most"] = float((svd_rmsd(a, b, mask) - fit[2]).abs().max().item())
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "superpose_time_fit.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_search(outdir):
    import torch
    from protstruc_amd import _lib, geometry, ops
    a, b, mask = inputs(B)
    counts = mask.sum(dim=1)
    l_norm = torch.full((B,), float(N), device="cuda")
    d0 = geometry.tm_d0(N)
    six = [(ops.SUPERPOSE_TM, d0)] + [(ops.SUPERPOSE_COUNT, c) for c in (0.5, 1.0, 2.0, 4.0, 8.0)]
    lib = _lib.load()
    seeds = sum(lib.ps_superpose_seed_count(int(n)) for n in counts.tolist())
    report = {"B": B, "N": N, "d0": d0, "seeds_over_the_batch": seeds, "max_iterations_per_chain": 20}
    for name, objectives in (("six_objectives", six), ("tm_alone", six[:1])):
        t = timed(lambda: ops.superpose_search(a, b, mask, l_norm, objectives), 2, 10)
        chains = seeds * len(objectives)
        report[name] = {"K39_K40": t, "chains": chains,
                        "chain_iterations_per_second_if_every_chain_ran_20": chains * 20 / (t["median_us"] * 1e-6)}
    score = ops.superpose_search(a, b, mask, l_norm, six)[0]
    report["mean_tm"], report["mean_gdt_ts"] = float(score[:, 0].mean().item()), float(score[:, 2:6].mean().item())
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "superpose_time_search.json"), "w") as f:
        json.dump(report, f, indent=1)


STEPS = {"fit": step_fit, "search": step_search}


def finish(outdir):
    with open(os.path.join(outdir, "superpose_time_fit.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "superpose_time_search.json")) as f:
        report["search"] = json.load(f)
    report["not_measured"] = ["the iterations the chains actually take", "K40's share of the search", "other shapes",
                              "the spread between runs and between machines"]
    os.remove(os.path.join(outdir, "superpose_time_fit.json"))
    os.remove(os.path.join(outdir, "superpose_time_search.json"))
    with open(os.path.join(outdir, "superpose_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("fit", "search"), STEP_TIMEOUT_S, finish)
