#!/usr/bin/python3
"""Time the DSSP kernels (ops.backbone_hbonds, ops.dssp_assign) against a composed-torch evaluation of the same definition
in float32 on the same GPU, and write profiles/dssp_time.json.

    python3 tools/dssp_time.py [--outdir DIR]

Shape: B = 128, N = 512, four atom slots.  Inputs: an ideal alpha-helix, a two-strand hairpin and a centred random walk of
3.8 A steps with the backbone placed around it (the helpers of tests/dssp_ref.py), the same chain in every structure
turned by a random rotation, one chain break in the middle, a tenth of the residues incomplete.  The composed version
builds the dense (B,N,N) energies, takes ``topk`` per donor and finds the patterns with shifted boolean (B,N,N) maps; it
runs at the largest batch (B, B / 2, ...) that fits and the report says which.
Each step below runs as a child process of this file under its own ``timeout``; the first to fail ends the run (tools/steps.py).

  events  HIP events around each call (3 warm-ups, median / min of 20), K21 and K22, and the labels' agreement
  torch   the composed float32 evaluation with the allocator's peak

Reported: the times, how many labels of the composed version differ from the kernels' (float32 against double at the two
thresholds; not an error measure), and the ratio.  No speed is asserted anywhere.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.steps import largest_batch_that_fits, main, timed

B, N = 128, 512
STEP_TIMEOUT_S = {"events": 180, "torch": 300}


def inputs(batch, seed=1):
    """(xyz (batch,N,4,3), complete, junction) on the GPU"""
    import numpy as np
    import torch
    from tests import dssp_ref as R
    rng = np.random.default_rng(seed)
    chain = np.concatenate([R.ideal_helix(40), R.hairpin(12) + [0.0, 0.0, 15.0], R.backbone_on_trace(R.random_walk(N - 64, rng))])
    complete = rng.random((batch, N)) >= 0.1
    junction = np.stack([R.chain_junctions(c, (39, 51, 63, N // 2)) for c in complete])
    rot = np.linalg.qr(rng.normal(size=(batch, 3, 3)))[0]
    xyz = np.einsum("bij,nkj->bnki", rot, chain - chain.mean(axis=(0, 1))).astype(np.float32)
    xyz[~complete] = np.nan
    return torch.from_numpy(xyz).cuda(), torch.from_numpy(complete).cuda(), torch.from_numpy(junction).cuda()


def composed(xyz, complete, junction):
    """The definition with dense tensors, float32: (B,N) int8 codes"""
    import torch
    b, n = complete.shape
    x = torch.where(complete[:, :, None, None], xyz, torch.zeros_like(xyz))
    Np, CA, C, O = x[:, :, 0], x[:, :, 1], x[:, :, 2], x[:, :, 3]
    prev = torch.roll(junction, 1, dims=1)
    prev[:, 0] = False
    has_h = prev & complete
    co = torch.roll(C - O, 1, dims=1)
    H = Np + co / co.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    d = lambda p, q: torch.cdist(p, q)                                    # noqa: E731  [b, i, j]: acceptor atom i, donor atom j
    d_on, d_ch, d_oh, d_cn = d(O, Np), d(C, H), d(O, H), d(C, Np)
    E = 27.888 * (1 / d_on + 1 / d_ch - 1 / d_oh - 1 / d_cn)
    E = torch.where(torch.minimum(torch.minimum(d_on, d_ch), torch.minimum(d_oh, d_cn)) < 0.5, torch.full_like(E, -9.9), E)
    idx = torch.arange(n, device=xyz.device)
    ok = complete[:, :, None] & has_h[:, None, :] & (idx[:, None] != idx[None, :]) & (idx[None, :] != idx[:, None] + 1)
    ok &= d(CA, CA) < 9.0
    E = torch.where(ok & (E < -0.5), E, torch.zeros_like(E))
    best = torch.topk(E, min(2, n), dim=1, largest=False)                 # per donor j over the acceptors i
    hb = torch.zeros(b, n, n, dtype=torch.bool, device=xyz.device)
    hb.scatter_(1, best.indices, best.values < -0.5)                      # hb[b, i, j]: i is in donor j's kept list

    def shift(m, di, dj):
        """s[i, j] = m[i + di, j + dj], False outside"""
        out = torch.zeros_like(m)
        i0, i1, j0, j1 = max(0, -di), n - max(0, di), max(0, -dj), n - max(0, dj)
        if i1 > i0 and j1 > j0:
            out[:, i0:i1, j0:j1] = m[:, i0 + di:i1 + di, j0 + dj:j1 + dj]
        return out

    def shift1(v, k):
        """s[i] = v[i + k], False outside"""
        out = torch.zeros_like(v)
        i0, i1 = max(0, -k), n - max(0, k)
        if i1 > i0:
            out[:, i0:i1] = v[:, i0 + k:i1 + k]
        return out

    J = junction.clone()
    J[:, -1] = False

    def cont(first, k):
        """c[i] = junction[i + first .. i + first + k - 1] all true"""
        out = torch.ones_like(J)
        for t in range(k):
            out &= shift1(J, first + t)
        return out

    hbT = hb.transpose(1, 2)
    labels = {}
    turn_any = torch.zeros_like(J)
    for n_turn, name in ((3, "G"), (4, "H"), (5, "I")):
        reach = torch.zeros_like(J)                                       # reach[i] = hb[i, i + n_turn]
        if n > n_turn:
            reach[:, :n - n_turn] = torch.diagonal(hb, n_turn, 1, 2)
        turn = cont(0, n_turn) & reach
        start = turn & shift1(turn, -1)
        helix = torch.zeros_like(J)
        for t in range(n_turn):
            helix |= shift1(start, -t)
        for t in range(1, n_turn):
            turn_any |= shift1(turn, -t)
        labels[name] = helix
    c2 = cont(-1, 2)
    pair_ok = c2[:, :, None] & c2[:, None, :] & ((idx[:, None] - idx[None, :]).abs() >= 3)
    par = ((shift(hb, -1, 0) & shift(hbT, 1, 0)) | (shift(hbT, 0, -1) & shift(hb, 0, 1))) & pair_ok
    anti = ((hb & hbT) | (shift(hb, -1, 1) & shift(hbT, 1, -1))) & pair_ok
    ladder = (par & (shift(par, -1, -1) | shift(par, 1, 1))) | (anti & (shift(anti, -1, 1) | shift(anti, 1, -1)))
    labels["E"] = ladder.any(-1)
    labels["B"] = (par | anti).any(-1) & ~labels["E"]
    u, v = CA - torch.roll(CA, 2, dims=1), torch.roll(CA, -2, dims=1) - CA
    cos = (u * v).sum(-1) / (u.norm(dim=-1) * v.norm(dim=-1)).clamp(min=1e-6)
    labels["S"] = cont(-2, 4) & (cos < 0.3420201433256687)
    labels["T"] = turn_any
    codes = torch.zeros(b, n, dtype=torch.int8, device=xyz.device)
    for name in reversed("HBEGITS"):
        codes[labels[name]] = "-HBEGITS".index(name)
    codes[~complete] = 0
    return codes


def step_events(outdir):
    import torch
    from protstruc_amd import ops
    xyz, complete, junction = inputs(B)
    acc = ops.backbone_hbonds(xyz, complete, junction)[0]
    codes = ops.dssp_assign(xyz, complete, junction, acc)
    counts = torch.bincount(codes.long().flatten(), minlength=8).tolist()
    report = {"device": torch.cuda.get_device_name(0), "method": "HIP events around each call; 3 warm-ups, median / min of 20",
              "B": B, "N": N, "labels": dict(zip("-HBEGITS", counts)), "bonds_kept": int((acc >= 0).sum().item()),
              "hbonds": timed(lambda: ops.backbone_hbonds(xyz, complete, junction)),
              "assign": timed(lambda: ops.dssp_assign(xyz, complete, junction, acc))}
    small = min(B, 8)
    report["labels_that_differ_from_composed_float32"] = int((composed(xyz[:small], complete[:small], junction[:small]) != codes[:small]).sum().item())
    report["labels_compared"] = small * N
    print(json.dumps(report), flush=True)
    with open(os.path.join(outdir, "dssp_time_events.json"), "w") as f:
        json.dump(report, f, indent=1)


def step_torch(outdir):
    import torch

    def measure(b):
        xyz, complete, junction = inputs(b)
        with torch.no_grad():
            return {"composed": timed(lambda: composed(xyz, complete, junction), 1, 3)}

    entry = {"B": B, "N": N, **largest_batch_that_fits(B, measure)}
    print(json.dumps(entry), flush=True)
    with open(os.path.join(outdir, "dssp_time_torch.json"), "w") as f:
        json.dump(entry, f, indent=1)


STEPS = {"events": step_events, "torch": step_torch}


def finish(outdir):
    with open(os.path.join(outdir, "dssp_time_events.json")) as f:
        report = json.load(f)
    with open(os.path.join(outdir, "dssp_time_torch.json")) as f:
        c = json.load(f)
    report["composed_torch"] = c
    if c.get("batch"):
        report["composed_over_kernels"] = c["composed"]["median_us"] * (B / c["batch"]) / (
            report["hbonds"]["median_us"] + report["assign"]["median_us"])
    os.remove(os.path.join(outdir, "dssp_time_events.json"))
    os.remove(os.path.join(outdir, "dssp_time_torch.json"))
    with open(os.path.join(outdir, "dssp_time.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main(__file__, STEPS, ("events", "torch"), STEP_TIMEOUT_S, finish)
