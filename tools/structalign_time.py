#!/usr/bin/python3
"""Time the structure-alignment kernels (ops.nw_align, ops.structure_align) and write profiles/structalign_time.json.

    python3 tools/structalign_time.py [--outdir DIR]

B = 128 pairs at N = 128, 256 and 512: a chain of CA-like points (3.8 A steps), and the same chain with three segments cut
out, one segment inserted, a rigid motion and 0.7 A of noise -- what aligning a model with insertions and deletions onto its
template looks like.  Each step below runs as a child process of this file under its own ``timeout``; the first to fail
ends the run (tools/steps.py).

  n128, n256, n512   HIP events around each call (1 warm-up, median / min of 5): one DP pass -- K41 over a (B,N,N') matrix of
                     the TM terms, i.e. the pass of the refinement with its scores read from memory instead of computed --,
                     and the whole alignment (K42 + K43, both starts); the DP passes per pair are counted by the float64
                     restatement (tests/structalign_ref.py) on the first four pairs, with which the maps are compared
  cpu                the wall time of that restatement on one pair of N = 256, as a statement of what the CPU route costs

No speed is asserted anywhere.  A single run: the spread between runs and between machines is not measured, nor any other
shape, nor the share of the DP in the alignment's time.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import main, timed

B = 128
SIZES = (128, 256, 512)
STEP_TIMEOUT_S = {"n128": 240, "n256": 240, "n512": 300, "cpu": 120}


def pair(N, seed):
    """(a (N,3), b (N',3)) float32 numpy: b is a with indels, moved and perturbed"""
    import numpy as np
    rng = np.random.default_rng(seed)
    steps = rng.standard_normal((N, 3))
    steps = 0.6 * steps + 0.4 * np.roll(steps, 1, axis=0)          # some persistence, so that there is secondary structure
    a = np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=1, keepdims=True), axis=0)
    keep = np.ones(N, dtype=bool)
    for start in rng.choice(N - 12, 3, replace=False):
        keep[start:start + int(rng.integers(3, 10))] = False
    b = a[keep]
    at = int(rng.integers(10, b.shape[0] - 10))
    loop = b[at] + np.cumsum(3.8 * rng.standard_normal((6, 3)) / np.sqrt(3.0), axis=0)
    b = np.concatenate([b[:at], loop, b[at:]])
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    b = b @ q.T + rng.uniform(-20, 20, 3) + 0.7 * rng.standard_normal(b.shape)
    return a.astype(np.float32), b.astype(np.float32)


def batch(N):
    """(a (B,N,3), b (B,Mb,3), mask_b (B,Mb)) on the GPU, NaN under the mask, and the numpy pairs"""
    import numpy as np
    import torch
    pairs = [pair(N, 1000 * N + s) for s in range(B)]
    Mb = max(p[1].shape[0] for p in pairs)
    b, mask_b = np.full((B, Mb, 3), np.nan, np.float32), np.zeros((B, Mb), dtype=bool)
    for s, (_, pb) in enumerate(pairs):
        b[s, :pb.shape[0]], mask_b[s, :pb.shape[0]] = pb, True
    return torch.from_numpy(np.stack([p[0] for p in pairs])).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(mask_b).cuda(), pairs


def step_size(N, outdir):
    import numpy as np
    import torch
    from protstruc_amd import geometry, ops
    from tests import structalign_ref as ref
    a, b, mask_b, pairs = batch(N)
    d0 = geometry.tm_d0(torch.minimum(torch.full((B,), N, device="cuda"), mask_b.sum(dim=1))).float()
    found = ops.structure_align(a, b, None, mask_b, d0)
    # a score matrix of the refinement's kind for the DP alone: the TM terms under the alignment's transform
    moved = a @ found[3].transpose(1, 2) + found[4][:, None, :]
    score = 1.0 / (1.0 + ((moved[:, :, None, :] - torch.nan_to_num(b)[:, None, :, :]) ** 2).sum(-1) / (d0 * d0)[:, None, None])
    report = {"B": B, "N": N, "Mb": int(b.shape[1]), "method": "HIP events around each call; 1 warm-up, median / min of 5; a single run",
              "dp_pass_K41": timed(lambda: ops.nw_align(score, -0.6, None, mask_b), 1, 5),
              "alignment_K42_K43": timed(lambda: ops.structure_align(a, b, None, mask_b, d0), 1, 5),
              "mean_aligned": float(found[1].float().mean().item()), "mean_search_score": float(found[2].mean().item()),
              "share_won_by_the_secondary_structure_start": float(found[6].float().mean().item())}
    passes, agree = [], 0
    for s in range(4):
        want = ref.align(pairs[s][0], pairs[s][1], None, None, float(d0[s].item()))
        passes.append(want.passes)
        agree += int(np.array_equal(want.map, found[0][s].cpu().numpy()))
    report["dp_passes_per_pair_first_four"] = passes
    report["maps_equal_to_the_restatement_first_four"] = agree
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, f"structalign_time_{N}.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_cpu(outdir):
    import time
    from tests import structalign_ref as ref
    a, b = pair(256, 256000)
    t0 = time.perf_counter()
    got = ref.align(a, b)
    report = {"N": 256, "float64_numpy_restatement_wall_s_one_pair": time.perf_counter() - t0, "dp_passes": got.passes,
              "aligned": got.n_aligned}
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "structalign_time_cpu.json"), "w") as f:
        json.dump(report, f, indent=1)


STEPS = {"n128": lambda outdir: step_size(128, outdir), "n256": lambda outdir: step_size(256, outdir),
         "n512": lambda outdir: step_size(512, outdir), "cpu": step_cpu}


def finish(outdir):
    report = {"sizes": []}
    for N in SIZES:
        path = os.path.join(outdir, f"structalign_time_{N}.json")
        with open(path) as f:
            report["sizes"].append(json.load(f))
        os.remove(path)
    path = os.path.join(outdir, "structalign_time_cpu.json")
    with open(path) as f:
        report["cpu_route"] = json.load(f)
    os.remove(path)
    report["not_measured"] = ["the spread between runs and between machines (a single run)", "other shapes",
                              "the share of the DP, the chains and the trace back in the alignment's time"]
    with open(os.path.join(outdir, "structalign_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("n128", "n256", "n512", "cpu"), STEP_TIMEOUT_S, finish)
