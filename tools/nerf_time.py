#!/usr/bin/python3
"""Time the backbone builder (K7, ops.backbone_from_dihedrals) with HIP events after warm-up, against the loop a user
would otherwise write -- the reference's place_fourth_atom formula applied 3 N times in torch, vectorised over the
batch -- on the same GPU in the same process, and measure the builder's accuracy against the float64 walk of
tests/nerf_ref.py.  Prints one JSON object.

    python3 tools/nerf_time.py [reps] [--builder-only]

--builder-only skips the torch loop and the accuracy section (for a kernel trace: the loop launches ~10^5 kernels).
HIP events around one call also hold the op's host work (validation, two torch.empty) whenever the GPU waits for it; the
kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python3 tools/nerf_time.py 50 --builder-only`.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from protstruc_amd import geometry as G, ops  # noqa: E402
from tests import nerf_ref as R  # noqa: E402

SIZES = [(256, 384), (64, 512)]   # BASELINE config 5's shape, and a longer chain


def place_torch(a, b, c, length, planar, dihedral):
    """geometry.place_fourth_atom of the reference (geometry.py:127-168) in torch, (B, 3) points, (B, 1) parameters."""
    bc = b - c
    bc = bc / bc.norm(dim=-1, keepdim=True)
    n = torch.linalg.cross(b - a, bc, dim=-1)
    n = n / n.norm(dim=-1, keepdim=True)
    d = [bc, torch.linalg.cross(n, bc, dim=-1), n]
    m = [length * torch.cos(planar), length * torch.sin(planar) * torch.cos(dihedral),
         -length * torch.sin(planar) * torch.sin(dihedral)]
    return c + sum(mi * di for mi, di in zip(m, d))


def torch_loop(dih):
    """The sequential NeRF loop over residues, one torch op chain per placement, batch-vectorised; N/CA/C only."""
    B, N = dih.shape[:2]
    dev = dih.device
    full = lambda v: torch.full((B, 1), v, device=dev)  # noqa: E731
    la, lc, ln = full(G.IDEAL_NA), full(G.IDEAL_AC), full(G.IDEAL_C_N)
    a_nac, a_cacn, a_cnca = full(G.IDEAL_NAC), full(G.IDEAL_CACN), full(G.IDEAL_CNCA)
    out = torch.zeros(B, N, 15, 3, device=dev)
    n = torch.tensor([G.IDEAL_NA * np.cos(G.IDEAL_NAC), G.IDEAL_NA * np.sin(G.IDEAL_NAC), 0.0], dtype=torch.float32,
                     device=dev).expand(B, 3)
    ca = torch.zeros(B, 3, device=dev)
    c = torch.tensor([G.IDEAL_AC, 0.0, 0.0], dtype=torch.float32, device=dev).expand(B, 3)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = n, ca, c
    for i in range(1, N):
        n1 = place_torch(n, ca, c, ln, a_cacn, dih[:, i - 1, 1:2])
        ca1 = place_torch(ca, c, n1, la, a_cnca, dih[:, i - 1, 2:3])
        c1 = place_torch(c, n1, ca1, lc, a_nac, dih[:, i, 0:1])
        n, ca, c = n1, ca1, c1
        out[:, i, 0], out[:, i, 1], out[:, i, 2] = n, ca, c
    return out


def timed(fn, reps, warmup=3):
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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("nerf_time.py measures on the GPU; none is visible")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    builder_only = "--builder-only" in sys.argv
    reps = int(args[0]) if args else 200
    res = {"device": torch.cuda.get_device_name(0), "sizes": []}
    for B, N in SIZES:
        dih = torch.from_numpy(R.chain_family("random", B, N, seed=B + N)).cuda()
        out = {"B": B, "N": N, "bytes_written": B * N * 15 * 4 * 4}
        out["builder"] = timed(lambda: ops.backbone_from_dihedrals(dih), reps)
        xyz, mask = ops.backbone_from_dihedrals(dih)
        xyz_out = torch.empty_like(xyz)
        out["fill_same_bytes"] = timed(lambda: (xyz_out.fill_(0.0), mask.fill_(0.0)), reps)
        if builder_only:
            res["sizes"].append(out)
            continue
        out["torch_loop"] = timed(lambda: torch_loop(dih), max(3, reps // 50), warmup=1)
        out["speedup"] = round(out["torch_loop"]["median_us"] / out["builder"]["median_us"], 1)
        loop = torch_loop(dih)
        out["builder_vs_torch_loop_max_abs_A"] = float((loop[:, :, :3] - xyz[:, :, :3]).abs().max())
        res["sizes"].append(out)
    if builder_only:
        print(json.dumps(res))
        return
    acc = {}
    for kind in ("strand", "helix", "random"):
        for N in (512, 1024):
            dih = R.chain_family(kind, 2, N, seed=N)
            want, _ = R.build(dih)
            got = ops.backbone_from_dihedrals(torch.from_numpy(dih).cuda())[0].double().cpu().numpy()
            loop = torch_loop(torch.from_numpy(dih).cuda()).double().cpu().numpy()
            acc[f"{kind}_N{N}"] = {"max_abs_err_A": float(np.abs(got - want).max()), "extent_A": float(np.abs(want).max()),
                                   "bound_A": 5e-5 * N, "torch_loop_fp32_max_abs_err_A": float(np.abs(loop - want).max())}
    res["accuracy_vs_fp64"] = acc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
