#!/usr/bin/python3
"""Time the four side-chain torsion kernels (K27 - K30: ops.chi, ops.chi_backward, ops.chi_set, ops.chi_set_backward)
against a copy of the coordinate tensor and against the composed float32 torch route -- a table gather to (B,N,4,4,3),
three cross products and an atan2 to measure; a Python loop of four masked Rodrigues rotations over (B,N,A,3) to set --
on the same GPU, and write profiles/chi_time.json.

    python3 tools/chi_time.py [--outdir DIR]

Shape: B = 128, N = 512, A = 15; synthetic residues of all 20 types in turn, every residue's atoms a random walk with steps
of 1 to 2 A, 10 % of the atoms masked with NaN coordinates under the mask.  Each step below runs as a child process of this
file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call of the C entry points on buffers allocated once (3 warm-ups, median / min of 20):
          the four kernels, and ``out.copy_(xyz)`` on the very buffers K29 read and wrote -- K29's floor: it has to read
          and write the tensor once
  torch   ``composed_measure`` and ``composed_set`` below, without autograd, at the largest batch (B, B / 2, ...) that
          fits, with the allocator's peak

No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import largest_batch_that_fits, main, timed

B, N, A = 128, 512, 15
MASKED = 0.10
STEP_TIMEOUT_S = {"events": 240, "torch": 300}


def inputs(batch, seed=0):
    """(xyz (batch,N,A,3) float32 with NaN at masked atoms, mask (batch,N,A) bool, types (batch,N) int32, chi
    (batch,N,4) float32) as numpy arrays"""
    import numpy as np
    rng = np.random.default_rng(seed)
    types = ((np.arange(batch * N) + rng.integers(0, 20)) % 20).astype(np.int32).reshape(batch, N)
    step = rng.normal(size=(batch, N, A, 3)).astype(np.float32)
    step *= (rng.uniform(1.0, 2.0, size=(batch, N, A)).astype(np.float32) / np.linalg.norm(step, axis=-1))[..., None]
    start = np.stack([3.8 * np.arange(N), np.zeros(N), np.zeros(N)], axis=-1).astype(np.float32)
    xyz = (start[None, :, None, :] + np.cumsum(step, axis=2)).astype(np.float32)
    mask = rng.random((batch, N, A)) >= MASKED
    xyz[~mask] = np.nan
    chi = rng.uniform(-np.pi, np.pi, size=(batch, N, 4)).astype(np.float32)
    return xyz, mask, types, chi


def _rows(types, table):
    """The table rows of the residues, with all -1 at padding types; ``table`` (T, ...) integers"""
    import torch
    known = (types >= 0) & (types < table.shape[0])
    rows = table[torch.where(known, types, torch.zeros_like(types)).long()]
    return torch.where(known.reshape(known.shape + (1,) * (rows.ndim - 2)), rows, torch.full_like(rows, -1))


def _dihedral(a, b, c, d):
    import torch
    b0, b1, b2 = a - b, c - b, d - c
    n1, n2 = torch.linalg.cross(b0, b1), torch.linalg.cross(b2, b1)
    m = torch.linalg.cross(n1, n2)
    return torch.atan2((m * b1).sum(-1) / b1.norm(dim=-1), (n1 * n2).sum(-1))


def composed_measure(xyz, mask, types, chi_atoms):
    """The float32 route a user writes today: (chi (B,N,4), 0 where undefined; defined (B,N,4) bool).  ``xyz`` (B,N,A,3),
    ``mask`` (B,N,A) bool, ``types`` (B,N) integers, ``chi_atoms`` (T,4,4) integer tensor; any device."""
    import torch
    Bn, Nn = types.shape
    rows = _rows(types, chi_atoms)                                          # (B,N,4,4)
    has = (rows >= 0).all(-1)
    at = rows.clamp(min=0).long().reshape(Bn, Nn, 16)
    x = torch.where(mask[..., None], xyz, torch.zeros_like(xyz))
    pts = torch.gather(x, 2, at[..., None].expand(Bn, Nn, 16, 3)).reshape(Bn, Nn, 4, 4, 3)
    defined = has & torch.gather(mask, 2, at).reshape(Bn, Nn, 4, 4).all(-1)
    chi = _dihedral(pts[..., 0, :], pts[..., 1, :], pts[..., 2, :], pts[..., 3, :])
    return torch.where(defined, chi, torch.zeros_like(chi)), defined


def composed_set(xyz, chi, mask, types, chi_atoms, chi_last):
    """The float32 route a user writes today, absolute mode: the (B,N,A,3) coordinates with every defined angle that has a
    range turned to ``chi`` (B,N,4), one masked Rodrigues rotation of the whole tensor per angle; masked atoms come back
    as 0.  ``chi_last`` (T,4) integer tensor."""
    import torch
    Bn, Nn, An = mask.shape
    rows, last = _rows(types, chi_atoms), _rows(types, chi_last)            # (B,N,4,4), (B,N,4)
    x = torch.where(mask[..., None], xyz, torch.zeros_like(xyz))
    slot = torch.arange(An, device=xyz.device)
    for k in range(4):
        at = rows[:, :, k].clamp(min=0).long()                              # (B,N,4)
        on = (rows[:, :, k] >= 0).all(-1) & torch.gather(mask, 2, at).all(-1) & (last[:, :, k] >= 0)
        a, b, c, d = (torch.gather(x, 2, at[:, :, j, None, None].expand(Bn, Nn, 1, 3))[:, :, 0] for j in range(4))
        delta = torch.where(on, chi[:, :, k] - _dihedral(a, b, c, d), torch.zeros_like(chi[:, :, k]))
        axis = c - b
        u = torch.where(on[..., None], axis / axis.norm(dim=-1, keepdim=True), torch.zeros_like(axis))[:, :, None]
        cs, sn = torch.cos(delta)[:, :, None, None], torch.sin(delta)[:, :, None, None]
        v = x - c[:, :, None]
        turned = c[:, :, None] + v * cs + torch.linalg.cross(u.expand_as(v), v) * sn + u * ((u * v).sum(-1, keepdim=True) * (1 - cs))
        moves = on[..., None] & mask & (slot >= rows[:, :, k, 3, None]) & (slot <= last[:, :, k, None])
        x = torch.where(moves[..., None], turned, x)
    return x


def _tables():
    from protstruc_amd import general
    return general.chi_atom_table(), general.chi_last_table()


def step_events(outdir):
    import ctypes

    import torch
    from protstruc_amd import _lib
    atoms_t, last_t = _tables()
    T = atoms_t.shape[0]
    atoms = (ctypes.c_int * atoms_t.numel())(*atoms_t.flatten().tolist())
    last = (ctypes.c_int * last_t.numel())(*last_t.flatten().tolist())
    xyz, mask, types, chi = (torch.from_numpy(t).cuda() for t in inputs(B))
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    out, grad_xyz = torch.empty_like(xyz), torch.empty_like(xyz)
    got, got_mask = torch.empty_like(chi), torch.empty(B, N, 4, dtype=torch.bool, device="cuda")
    grad_chi, upstream, upstream_chi = torch.empty_like(chi), torch.randn_like(xyz), torch.randn_like(chi)

    def checked(rc):
        assert rc == 0, rc

    calls = {
        "chi": lambda: checked(lib.ps_chi_f32(xyz.data_ptr(), mask.data_ptr(), types.data_ptr(), atoms, T, got.data_ptr(),
                                              got_mask.data_ptr(), B, N, A, stream)),
        "chi_backward": lambda: checked(lib.ps_chi_backward_f32(xyz.data_ptr(), mask.data_ptr(), types.data_ptr(), atoms, T,
                                                                upstream_chi.data_ptr(), grad_xyz.data_ptr(), B, N, A, stream)),
        "chi_set": lambda: checked(lib.ps_chi_set_f32(xyz.data_ptr(), mask.data_ptr(), types.data_ptr(), atoms, last, T,
                                                      chi.data_ptr(), None, 0, out.data_ptr(), B, N, A, stream)),
        "chi_set_backward": lambda: checked(lib.ps_chi_set_backward_f32(out.data_ptr(), mask.data_ptr(), types.data_ptr(),
                                                                        atoms, last, T, None, upstream.data_ptr(),
                                                                        grad_chi.data_ptr(), B, N, A, stream)),
    }
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "A": A, "masked": MASKED, "coordinate_bytes": xyz.numel() * 4, "kernels": {}}
    for name, call in calls.items():
        report["kernels"][name] = timed(call)
    report["defined_angles"] = float(got_mask.float().mean().item())
    report["turned_floats"] = float((out.view(torch.int32) != xyz.view(torch.int32)).float().mean().item())
    report["copy"] = timed(lambda: out.copy_(xyz))          # the very buffers K29 read and wrote
    report["chi_set_over_copy"] = report["kernels"]["chi_set"]["median_us"] / report["copy"]["median_us"]
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "chi_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch
    atoms_t, last_t = (t.cuda() for t in _tables())

    def measure(b):
        xyz, mask, types, chi = (torch.from_numpy(t).cuda() for t in inputs(b))
        with torch.no_grad():
            return {"composed_measure": timed(lambda: composed_measure(xyz, mask, types, atoms_t), 2, 10),
                    "composed_set": timed(lambda: composed_set(xyz, chi, mask, types, atoms_t, last_t), 2, 10)}

    entry = largest_batch_that_fits(B, measure)
    print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "chi_time_torch.json"), "w") as f:
        json.dump(entry, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "chi_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "chi_time_torch.json")) as f:
        entry = json.load(f)
    report["composed_torch"] = entry
    if entry.get("batch"):
        scale = B / entry["batch"]
        report["composed_measure_over_chi"] = \
            entry["composed_measure"]["median_us"] * scale / report["kernels"]["chi"]["median_us"]
        report["composed_set_over_chi_set"] = \
            entry["composed_set"]["median_us"] * scale / report["kernels"]["chi_set"]["median_us"]
    report["not_measured"] = "the composed route's backward passes; hardware counters of the four kernels"
    os.remove(os.path.join(outdir, "chi_time_events.json"))
    os.remove(os.path.join(outdir, "chi_time_torch.json"))
    with open(os.path.join(outdir, "chi_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
