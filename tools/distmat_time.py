#!/usr/bin/python3
"""Time the distance-matrix reconstruction (K8 + K9 + finish, geometry.reconstruct_backbone_distmat_from_interresidue_
geometry) and K9 alone with HIP events after warm-up, against the reference's Floyd-Warshall loop (geometry.py:325-330:
3 L iterations of stack + min) in torch on the same GPU, and measure the accuracy bounds that tests/test_gpu_distmat.py
holds.  Prints one JSON object.

    python3 tools/distmat_time.py [reps] [--fw-only]

--fw-only times K9 alone and skips the rest (for a kernel trace).  The issue-rate bound assumes one VALU instruction
per element and pivot (what the update kernel issues: one v_pk_add_f32 and one v_min3_f32 per two pivots), B n^3 lane
operations at 2.08 ns per wave instruction per SIMD (profiles/r05_valu_issue.log) on 256 CUs x 4 SIMDs; the HBM figure
counts one read and one write of D per pivot block of 64.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from protstruc_amd import geometry as G, ops  # noqa: E402
from tests import distmat_ref as M  # noqa: E402

SIZES = [(64, 256), (8, 512), (1, 229)]
LOOP_SIZE = (1, 229)
LANE_OPS_PER_S = 256 * 4 * 64 / 2.08e-9
HBM_BYTES_PER_S = 8.0e12
FW_BLOCK = 64


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


def reference_loop(D):
    """The reference's loop on a (3L, 3L) matrix, as it is written (stack, then min over the new axis)."""
    for i in range(D.shape[0]):
        d = D[i]
        D = torch.min(torch.stack([D, d[None, :] + d[:, None]]), dim=0).values
    return D


def inputs(B, L, seed):
    rng = np.random.default_rng(seed)
    n, ca, c, cb = M.rigid_ideal_residues(rng, B, L, spread=4.0 + 2.0 * L ** (1 / 3))
    geo = [torch.from_numpy(t.astype(np.float32)).cuda() for t in M.geometry_of(n, ca, cb)]
    mask = torch.from_numpy(rng.random((B, L, L)) >= 0.3).cuda()
    return geo, mask


def accuracy():
    """The quantities the GPU tests bound, at the tests' shapes."""
    from protstruc_amd import StructureBatch

    acc = {}
    k8, e2e = 0.0, 0.0
    for L in (5, 64, 229, 512):
        rng = np.random.default_rng(10 + L)
        n, ca, c, cb = M.rigid_ideal_residues(rng, 3, L, spread=4.0 + 2.0 * L ** (1 / 3))
        geo = [t.astype(np.float32) for t in M.geometry_of(n, ca, cb)]
        got = ops.backbone_distmat_init(*(torch.from_numpy(t).cuda() for t in geo)).cpu().numpy()
        want, cat = M.init64(*(t.astype(np.float64) for t in geo))
        scale = np.broadcast_to(geo[0][:, None, None], got.shape)
        k8 = max(k8, float((np.abs(got - want) / (scale + 4.0))[~cat].max()))
        if L <= 229:
            mask = rng.random((3, L, L)) >= 0.3
            full = G.reconstruct_backbone_distmat_from_interresidue_geometry(*geo, mask=mask)
            init, _ = M.init64(*(t.astype(np.float64) for t in geo), mask)
            ref = M.finish(M.from_nodes(M.fw_sequential(M.to_nodes(torch.from_numpy(init).cuda())), 3)).cpu().numpy()
            e2e = max(e2e, float((np.abs(full - ref) / (ref + 4.0)).max()))
    acc["k8_max_rel_err"] = k8
    acc["end_to_end_max_rel_err"] = e2e
    rt = 0.0
    for L in (12, 64, 229):
        rng = np.random.default_rng(30 + L)
        n, ca, c, cb = M.rigid_ideal_residues(rng, 2, L, spread=4.0 + 2.0 * L ** (1 / 3))
        xyz = np.zeros((2, L, 15, 3), dtype=np.float32)
        am = np.zeros((2, L, 15), dtype=bool)
        for slot, atom in ((0, n), (1, ca), (2, c), (4, cb)):
            xyz[:, :, slot], am[:, :, slot] = atom, True
        sb = StructureBatch.from_xyz(xyz, am, device="cuda")
        geo = featurise(sb)
        got = ops.backbone_distmat_init(*geo).cpu().numpy()
        x64 = xyz.astype(np.float64)
        true = M.true_distmat(x64[:, :, 0], x64[:, :, 1], x64[:, :, 2])
        _, cat = M.init64(*(t.double().cpu().numpy() for t in geo))
        rt = max(rt, float(np.abs(got - true)[~cat].max()))
    acc["round_trip_max_abs_err_A"] = rt
    sb = StructureBatch.from_pdb(os.path.join(ROOT, "tests", "golden", "15c8_HL.pdb"))
    chain = sb.get_chain_idx()[0].cpu().numpy()
    end = int(np.nonzero(chain[:-1] != chain[1:])[0][0])
    geo = featurise(sb)
    got = G.reconstruct_backbone_distmat_from_interresidue_geometry(*(t[0] for t in geo), chain_breaks=[end]).cpu().numpy()
    x = sb.get_xyz()[0].double().cpu().numpy()
    has = sb.get_atom_mask()[0].bool().cpu().numpy()[:, [0, 1, 2, 4]].all(-1)
    L = x.shape[0]
    true = M.true_distmat(x[None, :, 0], x[None, :, 1], x[None, :, 2])[0]
    sel = np.broadcast_to((has[:, None] & has[None, :] & ~np.eye(L, dtype=bool))[None, None], got.shape)
    err = np.abs(got - true)[sel]
    acc["pdb_15c8_non_gly"] = {"max_abs_err_A": float(err.max()), "median_abs_err_A": float(np.median(err)),
                               "p99_abs_err_A": float(np.quantile(err, 0.99))}
    return acc


def featurise(sb):
    dist, _ = sb.pairwise_distance_matrix()
    return (dist[:, :, :, 4, 4].contiguous(), sb.pairwise_dihedrals(["CA", "CB"], ["CB", "CA"]),
            sb.pairwise_dihedrals(["N", "CA", "CB"], ["CB"]), sb.pairwise_planar_angles(["CA", "CB"], ["CB"]))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("distmat_time.py measures on the GPU; none is visible")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    fw_only = "--fw-only" in sys.argv
    reps = int(args[0]) if args else 20
    res = {"device": torch.cuda.get_device_name(0), "sizes": []}
    for B, L in SIZES:
        geo, mask = inputs(B, L, B + L)
        n = 3 * L
        out = {"B": B, "L": L, "nodes": n}
        init = ops.backbone_distmat_init(*geo, mask)
        D = init.clone()
        out["k9_fw"] = timed(lambda: (D.copy_(init), ops.floyd_warshall_(D, G=3)), reps)
        out["copy_only"] = timed(lambda: D.copy_(init), reps)
        fw_us = out["k9_fw"]["median_us"] - out["copy_only"]["median_us"]
        bound_us = B * n ** 3 / LANE_OPS_PER_S * 1e6
        hbm_us = B * n * n * 8 * (n / FW_BLOCK) / HBM_BYTES_PER_S * 1e6
        out["k9_fw_net_us"] = round(fw_us, 2)
        out["valu_issue_bound_us"] = round(bound_us, 2)
        out["fraction_of_issue_bound"] = round(bound_us / fw_us, 3)
        out["hbm_stream_us"] = round(hbm_us, 2)
        out["fraction_of_hbm"] = round(hbm_us / fw_us, 3)
        if not fw_only:   # the timed size, checked bit for bit against the sequential loop
            ops.floyd_warshall_(D.copy_(init), G=3)
            out["k9_bit_equal_to_sequential_loop"] = bool(torch.equal(M.to_nodes(D), M.fw_sequential(M.to_nodes(init))))
            out["k8_init"] = timed(lambda: ops.backbone_distmat_init(*geo, mask), reps)
            out["full_function"] = timed(
                lambda: G.reconstruct_backbone_distmat_from_interresidue_geometry(*geo, mask=mask), reps)
        res["sizes"].append(out)
    if fw_only:
        print(json.dumps(res))
        return
    B, L = LOOP_SIZE
    geo, mask = inputs(B, L, 1)
    init = ops.backbone_distmat_init(*geo, mask)
    nodes = M.to_nodes(init)[0].contiguous()
    loop = {"B": B, "L": L, "torch_loop": timed(lambda: reference_loop(nodes), 3, warmup=1)}
    D = init.clone()
    loop["k9_fw"] = timed(lambda: (D.copy_(init), ops.floyd_warshall_(D, G=3)), reps)
    loop["speedup"] = round(loop["torch_loop"]["median_us"] / loop["k9_fw"]["median_us"], 1)
    ref = reference_loop(nodes)
    ops.floyd_warshall_(D.copy_(init), G=3)
    loop["bit_equal_to_torch_loop"] = bool(torch.equal(M.to_nodes(D)[0], ref))
    res["reference_loop"] = loop
    res["accuracy"] = accuracy()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
