#!/usr/bin/env python3
"""Host-side cost per call of the Python shell (wall clock over many asynchronous calls at a tiny shape, where the
GPU work is a few microseconds): what a single-structure user pays per method call."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from protstruc_amd import StructureBatch, _lib, geometry, ops

g = torch.Generator().manual_seed(0)
B, N = 1, 64
xyz = torch.randn(B, N, 15, 3, generator=g)
mask = torch.rand(B, N, 15, generator=g) < 0.9
mask[:, :, :3] = True
sb = StructureBatch.from_xyz(xyz, mask)
xg, mg = sb.get_xyz(), sb.get_atom_mask()
d = torch.empty(B, N, N, 15, 15, device="cuda")
m = torch.empty(B, N, N, 15, 15, dtype=torch.bool, device="cuda")
beta = torch.full((B,), 0.01, device="cuda")

# operands of the fused losses and structure features (K13 - K23), 64 residues / points: each of these wrappers checks its
# arguments (ops.check_*_shapes) on every call, which is most of what it costs at this size
pts = xg[:, :, 1].contiguous()                  # the CA atoms as (B, N, 3) points
tgt = pts + 0.25
rot, trans = ops.frames(xg, 0, 1, 2)
pmask = torch.ones(B, N, dtype=torch.bool, device="cuda")
groups = torch.arange(N, dtype=torch.int32, device="cuda").repeat(B, 1)
radius = torch.full((B, N), 1.7, device="cuda")
junction = pmask.clone()
junction[:, -1] = False
sphere = geometry.sphere_points(32).cuda()
g_rot, g_trans = torch.ones_like(rot), torch.ones_like(trans)

# operands of the graph, contact, pair-head, superposition and ensemble wrappers (K24 - K46), the same 64 residues / points
logits = torch.randn(B, N, N, 64, generator=g).cuda()
bins = torch.randint(0, 64, (B, N, N), generator=g).to(torch.uint8).cuda()
D = torch.cdist(pts, pts)
nbr = ops.nearest_neighbors(pts, 16, pmask)[0]
centers = [2.0 + 1.25 * c for c in range(16)]


def per_call(fn, n=2000):
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / n * 1e6


rows = [
    ("ops.pairwise_distance (preallocated outputs)", lambda: ops.pairwise_distance(xg, mg, out_dist=d, out_mask=m)),
    ("ops.pairwise_distance (allocating)", lambda: ops.pairwise_distance(xg, mg)),
    ("sb.pairwise_distance_matrix()", lambda: sb.pairwise_distance_matrix()),
    ("sb.backbone_dihedrals()", lambda: sb.backbone_dihedrals()),
    ("sb.backbone_orientations()", lambda: sb.backbone_orientations()),
    ("sb.pairwise_dihedrals(CA,CB|CA,CB)", lambda: sb.pairwise_dihedrals(["CA", "CB"], ["CA", "CB"])),
    ("sb.inter_residue_geometry()", lambda: sb.inter_residue_geometry()),
    ("sb.diffuse_xyz(beta)", lambda: sb.diffuse_xyz(beta)),
    ("ops.frames_backward", lambda: ops.frames_backward(xg, 0, 1, 2, grad_rot=g_rot, grad_trans=g_trans, residue_mask=pmask)),
    ("ops.fape", lambda: ops.fape(rot, trans, pts, rot, trans, tgt, pmask, pmask)),
    ("ops.lddt", lambda: ops.lddt(pts, tgt, pmask, groups)),
    ("ops.clash", lambda: ops.clash(pts, radius, pmask, groups)),
    ("ops.peptide_bond", lambda: ops.peptide_bond(xg, junction)),
    ("ops.backbone_hbonds", lambda: ops.backbone_hbonds(xg, pmask, junction)),
    ("ops.solvent_accessibility", lambda: ops.solvent_accessibility(pts, radius, pmask, sphere=sphere)),
    ("ops.nearest_neighbors (k = 16)", lambda: ops.nearest_neighbors(pts, 16, pmask)),
    ("ops.radius_graph (10 A, max_edges given)", lambda: ops.radius_graph(pts, 10.0, pmask, max_edges=N * N)),
    ("ops.edge_rbf (k = 16, 2 pairs, 16 centres)", lambda: ops.edge_rbf(xg, nbr, mg, pair_i=[1, 0], pair_j=[1, 3], centers=centers, sigma=1.25)),
    ("ops.closest_atoms", lambda: ops.closest_atoms(xg, mg)),
    ("ops.binned_cross_entropy (64 bins)", lambda: ops.binned_cross_entropy(logits, bins)),
    ("ops.superpose", lambda: ops.superpose(pts, tgt, None, pmask)),
    ("ops.rmsd_matrix", lambda: ops.rmsd_matrix(pts, tgt, pmask, pmask)),
    ("ops.cluster", lambda: ops.cluster(D, 8.0, pmask)),
    ("torch.empty + torch.add (reference point)", lambda: torch.add(xg, 1.0)),
    # config 5's eager step: diffuse_xyz + backbone_orientations
    ("config-5 eager step (diffuse_xyz + backbone_orientations)", lambda: (sb.diffuse_xyz(beta), sb.backbone_orientations())),
    # where the time goes
    ("  part: torch.empty (1 tensor, cuda)", lambda: torch.empty(B, N, 3, 3, device="cuda")),
    ("  part: ops._stream(xg)", lambda: ops._stream(xg)),
    ("  part: ctypes call of the K1 entry with B = 0 (no launch)", lambda: _K1(xg.data_ptr(), 0, d.data_ptr(), 0, 0, N, 15, 0, N, N, 0, _REF, 0)),
    ("  part: ops._f32c + shape + _u8c", lambda: (ops._f32c(xg, "xyz"), xg.shape[:3], ops._u8c(mg, "m"))),
    # the floor of any launch from Python: the C entry point called directly with prebuilt arguments (ctypes marshalling
    # + hipLaunchKernel), no validation, no allocation
    ("  floor: bare ctypes launch of ps_frames_f32 (K4)", lambda: _K4(_xp, _rp, None, B, N, 15, 0, 1, 2, 1, 0)),
    ("  floor: bare ctypes launch of the K1 entry", lambda: _K1(_xp, _mp, _dp, _mmp, B, N, 15, 0, N, N, 0, _REF, 0)),
]
_K4 = _lib.load().ps_frames_f32
_rot = torch.empty(B, N, 3, 3, device="cuda")
_xp, _rp, _mp, _dp, _mmp = xg.data_ptr(), _rot.data_ptr(), mg.data_ptr(), d.data_ptr(), m.data_ptr()
_K1 = _lib.load().ps_pairwise_distance_cfg_f32
_REF = _lib.k1_config_ref(0)
for name, fn in rows:
    print(f"{name:50s} {per_call(fn):8.1f} us/call", flush=True)
