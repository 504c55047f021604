#!/usr/bin/python3
"""Time the edge-RBF kernel (ops.edge_rbf, K25) against a fill of the very buffer it wrote and against the composed float32
torch route -- ``gather_neighbors``, norm, broadcast subtract / divide / square / exp -- on the same GPU, and write
profiles/edge_time.json.

    python3 tools/edge_time.py [--outdir DIR]

Shapes, at B = 128 on the compact chain of tools/sasa_time.py (512 residues of 15 atom slots, 45 % of the slots masked with
NaN coordinates): the CA graph of ``ops.nearest_neighbors`` with k = 48 (ProteinMPNN) and k = 30 (Structured Transformer,
GVP), the P = 25 ordered pairs of the first five slots, R = 16 centres over 2 .. 22 A.  Only ``rbf`` is asked for:
(B, N, k, 400) floats, 5.03 GB at k = 48.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20): the kernel writing into one buffer; ``out.fill_(0)``
          on that buffer, the store-rate yardstick; and the same kernel source built with non-temporal stores
          (-DPS_EDGE_RBF_NT=1, a library of that one file in build/, compiled by the orchestrating process before the
          steps), into a second buffer that must come out bitwise equal
  torch   the composed float32 evaluation at the largest batch (B, B / 2, ...) that fits, with the allocator's peak

No speed is asserted anywhere.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import sasa_time
from tools.steps import largest_batch_that_fits, main, timed

B, N, A, P, R = 128, 512, 15, 25, 16
SHAPES = {"k48": 48, "k30": 30}
STEP_TIMEOUT_S = {"events": 240, "torch": 400}
NT_LIB = os.path.join(ROOT, "build", "libedge_rbf_nt.so")


def build_nt_variant():
    """csrc/edge_features.hip alone, with non-temporal stores, as build/libedge_rbf_nt.so (no GPU needed)"""
    from protstruc_amd import build
    os.makedirs(os.path.dirname(NT_LIB), exist_ok=True)
    cmd = [build.HIPCC] + build.FLAGS + ["-DPS_EDGE_RBF_NT=1", "-o", NT_LIB, os.path.join(build.CSRC, "edge_features.hip")]
    print("[edge_time]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def inputs(k, batch):
    """(xyz (batch,N,A,3), atom mask (batch,N,A), the CA graph idx (batch,N,k) int32) on the GPU"""
    from protstruc_amd import ops
    assert (sasa_time.N, sasa_time.A) == (N, A)
    x, _, mask, _ = sasa_time.inputs(batch)
    xyz, mask = x.reshape(batch, N, A, 3), mask.reshape(batch, N, A)
    idx = ops.nearest_neighbors(xyz[:, :, 1], k, mask[:, :, 1])[0]
    return xyz, mask, idx


def tables():
    from protstruc_amd import geometry
    pairs = list(geometry.BACKBONE_PAIRS)
    centers, sigma = geometry.rbf_centers(R)
    assert len(pairs) == P
    return pairs, centers, sigma


def composed(xyz, idx, mask, pairs, centers, sigma):
    """The float32 route a user writes today: rbf (B,N,k,P*R); ``pairs`` (P,2) and ``centers`` (R,) tensors"""
    import torch
    from protstruc_amd import geometry
    ok = mask != 0
    x = torch.where(ok[..., None], xyz, torch.zeros_like(xyz))
    pi, pj = pairs[:, 0], pairs[:, 1]
    xj = geometry.gather_neighbors(x, idx)[:, :, :, pj]                        # (B,N,k,P,3)
    real = geometry.gather_neighbors(ok, idx, fill=False)[:, :, :, pj] & ok[:, :, None, pi]
    d = (xj - x[:, :, None, pi]).norm(dim=-1)                                  # (B,N,k,P)
    z = (d[..., None] - centers) / sigma                                       # (B,N,k,P,R)
    rbf = torch.exp(-(z * z)) * real[..., None]
    return rbf.reshape(*d.shape[:3], -1)


def step_events(outdir):
    import ctypes

    import torch
    from protstruc_amd import _lib
    pairs, centers, sigma = tables()
    ints, floats = ctypes.c_int * P, ctypes.c_float * R
    pair_i, pair_j, cen = ints(*(p[0] for p in pairs)), ints(*(p[1] for p in pairs)), floats(*centers.tolist())
    nt = ctypes.CDLL(NT_LIB).ps_edge_rbf_f32
    nt.restype, nt.argtypes = _lib.SIGNATURES["ps_edge_rbf_f32"]
    plain = _lib.load().ps_edge_rbf_f32
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "A": A, "P": P, "R": R, "shapes": {}}
    for shape, k in SHAPES.items():
        xyz, mask, idx = inputs(k, B)
        out = torch.empty(B, N, k, P * R, dtype=torch.float32, device="cuda")
        other = torch.empty_like(out)
        stream = torch.cuda.current_stream().cuda_stream

        def call(entry, buf):
            rc = entry(xyz.data_ptr(), mask.data_ptr(), idx.data_ptr(), pair_i, pair_j, P, cen, R, sigma, None,
                       buf.data_ptr(), B, N, A, k, stream)
            assert rc == 0, rc

        entry = {"k": k, "output_bytes": out.numel() * 4, "real_edges": float((idx >= 0).float().mean().item()),
                 "kernel": timed(lambda: call(plain, out))}
        entry["nonzero_fraction"] = float((out != 0).float().mean().item())
        entry["kernel_nt_stores"] = timed(lambda: call(nt, other))
        entry["nt_equals_plain"] = bool(torch.equal(out.view(torch.int32), other.view(torch.int32)))
        del other
        entry["fill"] = timed(lambda: out.fill_(0))
        entry["kernel_over_fill"] = entry["kernel"]["median_us"] / entry["fill"]["median_us"]
        entry["nt_over_plain"] = entry["kernel_nt_stores"]["median_us"] / entry["kernel"]["median_us"]
        entry["kernel_GB_per_s"] = entry["output_bytes"] / entry["kernel"]["median_us"] * 1e-3
        entry["fill_GB_per_s"] = entry["output_bytes"] / entry["fill"]["median_us"] * 1e-3
        report["shapes"][shape] = entry
        del xyz, mask, idx, out
        torch.cuda.empty_cache()
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "edge_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch
    pairs, centers, sigma = tables()
    entries = {}
    for shape, k in SHAPES.items():
        def measure(b):
            xyz, mask, idx = inputs(k, b)
            pt, ct = torch.tensor(pairs, device="cuda"), torch.from_numpy(centers).cuda()
            with torch.no_grad():
                return {"composed": timed(lambda: composed(xyz, idx, mask, pt, ct, sigma), 1, 3)}

        entries[shape] = largest_batch_that_fits(B, measure)
    print(json.dumps(entries), flush=True)
    with open(os.path.join(outdir, "edge_time_torch.json"), "w") as f:
        json.dump(entries, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "edge_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "edge_time_torch.json")) as f:
        entries = json.load(f)
    for shape, c in entries.items():
        report["shapes"][shape]["composed_torch"] = c
        if c.get("batch"):
            report["shapes"][shape]["composed_over_kernel"] = \
                c["composed"]["median_us"] * (B / c["batch"]) / report["shapes"][shape]["kernel"]["median_us"]
    os.remove(os.path.join(outdir, "edge_time_events.json"))
    os.remove(os.path.join(outdir, "edge_time_torch.json"))
    with open(os.path.join(outdir, "edge_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    source = os.path.join(ROOT, "protstruc_amd", "csrc", "edge_features.hip")
    if "--step" not in sys.argv and not (os.path.exists(NT_LIB) and os.path.getmtime(NT_LIB) >= os.path.getmtime(source)):
        build_nt_variant()   # by the orchestrating process, which stays off the GPU
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
