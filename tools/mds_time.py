#!/usr/bin/python3
"""Time K10 / K11 (geometry.initialize_backbone_with_mds) with HIP events after warm-up and write one JSON line to
profiles/mds_time.json (and stdout).

    python3 tools/mds_time.py [reps]

Cases: B = 1, L = 229, K = 4 (the reference's call on 15c8_HL), B = 64, L = 256 and B = 8, L = 512, all K = 4 random
starts on exact N / CA / C distances of rigid ideal residues.  Per case: the whole function (max_iter = 500,
eps = 1e-6), the passes it took (the largest n_iter of the batch; the launches after that are no-ops), and the time of
one SMACOF pass with every start running (from two eps = 0 runs of 20 and 40 passes).  The pass is compared with
  * the VALU issue bound: SM_VALU_PER_PAIR VALU instructions per (pair, start) -- what the inner loop issues: the
    difference, squared distance, square root, IEEE division, three Guttman terms and the two float32 stress terms --
    at 2.08 ns per wave instruction per SIMD on 256 CUs x 4 SIMDs;
  * the bandwidth of reading D once per pass (n^2 fp32 per structure) at 8 TB/s.
sklearn's MDS is timed at B = 1, L = 229 only where sklearn can be imported.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from protstruc_amd import geometry as G, ops  # noqa: E402
from tests import distmat_ref as DM  # noqa: E402

SIZES = [(1, 229), (64, 256), (8, 512)]
K = 4
SM_VALU_PER_PAIR = 30
LANE_OPS_PER_S = 256 * 4 * 64 / 2.08e-9
HBM_BYTES_PER_S = 8.0e12


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return {"median_us": round(ts[len(ts) // 2], 2), "min_us": round(ts[0], 2)}


def distmats(B, L, seed):
    rng = np.random.default_rng(seed)
    n, ca, c, _ = DM.rigid_ideal_residues(rng, B, L, spread=4.0 + 2.0 * L ** (1 / 3))
    return DM.true_distmat(n, ca, c)   # (B, 3, 3, L, L) float64


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {"device": torch.cuda.get_device_name(0), "K": K, "sizes": []}
    for B, L in SIZES:
        dm = distmats(B, L, 7 + L)
        D = torch.from_numpy(dm.astype(np.float32)).cuda()
        n = 3 * L
        init = torch.from_numpy(ops.smacof_random_starts(B, K, 3, L, None, 0).astype(np.float32)).cuda()
        r = {"B": B, "L": L, "nodes": n}
        r["full_function"] = timed(lambda: G.initialize_backbone_with_mds(D, init=init), reps)
        _, _, it = ops.smacof(D, 3, init=init, max_iter=500, eps=1e-6)
        r["passes_taken"] = int(it.max().item())
        t20 = timed(lambda: ops.smacof(D, 3, init=init, max_iter=20, eps=0.0), reps)
        t40 = timed(lambda: ops.smacof(D, 3, init=init, max_iter=40, eps=0.0), reps)
        per_pass = (t40["median_us"] - t20["median_us"]) / 20
        r["pass_us"] = round(per_pass, 3)
        r["fixed_us"] = round(t20["median_us"] - 21 * per_pass, 2)
        valu_us = B * K * n * n * SM_VALU_PER_PAIR / LANE_OPS_PER_S * 1e6
        hbm_us = B * n * n * 4 / HBM_BYTES_PER_S * 1e6
        r["valu_issue_bound_us"] = round(valu_us, 3)
        r["fraction_of_issue_bound"] = round(valu_us / per_pass, 3)
        r["d_read_us"] = round(hbm_us, 3)
        r["fraction_of_d_bandwidth"] = round(hbm_us / per_pass, 3)
        out["sizes"].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    try:
        from sklearn.manifold import MDS
        dm = distmats(1, 229, 7 + 229)[0]
        pd = dm.transpose(0, 2, 1, 3).reshape(3 * 229, 3 * 229)
        t0 = time.perf_counter()
        MDS(3, max_iter=500, n_init=4, dissimilarity="precomputed", random_state=0).fit_transform(pd)
        out["sklearn_B1_L229_s"] = round(time.perf_counter() - t0, 3)
    except ImportError:
        out["sklearn_B1_L229_s"] = None
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mds_time.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
