"""GPU tests of the backbone builder (K7, StructureBatch.from_backbone_dihedrals) and geometry.place_fourth_atom.

Yardstick: the float64 sequential walk of tests/nerf_ref.py on the same float32 inputs.  Bounds (a float32 log-depth
scan of rigid transforms passes them with margin; a float32 sequential walk does not, from strand N = 512 on):
  * global: max |xyz - fp64| <= 5e-5 * N Angstrom;
  * local: bond lengths, bond angles and every used phi / psi / omega (measured through K2) within
    max(1e-4, 4e-6 * extent), extent = the structure's max |coordinate| (the absolute quantum of its fp32 coordinates).
"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import nerf_ref as R
from tests.conftest import GOLDEN_DIR, load_golden

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 63, 64, 65, 511, 512, 1024]
FAMILIES = ["strand", "helix", "random"]


@pytest.fixture(scope="module")
def SB():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from protstruc_amd import StructureBatch
    from protstruc_amd import _lib
    _lib.load()
    return StructureBatch


def ragged_batch(kind, N, seed):
    """Three structures: one chain; two chains with NaN-chain padding at the tail; one chain with a gap (a masked
    residue) in the middle.  Returns (dihedrals, chain_idx, chain_ids, residue_mask) as numpy."""
    B = 3
    dih = R.chain_family(kind, B, N, seed)
    chain = np.zeros((B, N), dtype=np.float32)
    chain[1, max(1, N // 2):] = 1
    rmask = np.ones((B, N), dtype=bool)
    pad = N // 5
    if pad:
        rmask[1, N - pad:] = False
        chain[1, N - pad:] = np.nan
    if N >= 3:
        rmask[2, N // 3] = False
    chain_ids = [["A"], ["A", "B"], ["A"]]
    return dih, chain, chain_ids, rmask


def local_tolerance(xyz_b):
    return max(1e-4, 4e-6 * float(np.abs(xyz_b).max()))


def check_local_geometry(sb, dih, chain, rmask, ang=None, lens=None):
    """Bond lengths / angles (host, float64 from the fp32 output) and the used dihedrals through K2 equal the inputs."""
    xyz = sb.get_xyz().double().cpu().numpy()
    B, N = dih.shape[:2]
    ang0, lens0 = R.default_geometry(B, N)
    ang = ang0 if ang is None else ang
    lens = lens0 if lens is None else lens
    used = R.used_angles(B, N, chain, rmask)
    live = np.ones((B, N), bool) if rmask is None else rmask
    k2, k2_mask = sb.backbone_dihedrals()
    k2, k2_mask = k2.double().cpu().numpy(), k2_mask.cpu().numpy()
    n, ca, c = xyz[:, :, 0], xyz[:, :, 1], xyz[:, :, 2]
    for b in range(B):
        tol = local_tolerance(xyz[b])
        lv, nx = live[b], used[b, :, 1]
        errs = {
            "|N-CA|": np.abs(np.linalg.norm(n[b] - ca[b], axis=-1) - lens[b, :, 0])[lv],
            "|CA-C|": np.abs(np.linalg.norm(ca[b] - c[b], axis=-1) - lens[b, :, 1])[lv],
            "N-CA-C": np.abs(R.angle(n[b], ca[b], c[b]) - ang[b, :, 0])[lv],
        }
        if N > 1:
            errs["|C-N'|"] = np.abs(np.linalg.norm(c[b, :-1] - n[b, 1:], axis=-1) - lens[b, :-1, 2])[nx[:-1]]
            errs["CA-C-N'"] = np.abs(R.angle(ca[b, :-1], c[b, :-1], n[b, 1:]) - ang[b, :-1, 1])[nx[:-1]]
            errs["C-N'-CA'"] = np.abs(R.angle(c[b, :-1], n[b, 1:], ca[b, 1:]) - ang[b, :-1, 2])[nx[:-1]]
        u = used[b]
        assert k2_mask[b][u].all(), "K2 reports an angle undefined that the builder used"
        errs["phi/psi/omega (K2)"] = R.angle_diff(k2[b], dih[b])[u]
        for name, e in errs.items():
            if e.size:
                assert np.isfinite(e).all() and e.max() <= tol, f"structure {b}: {name} off by {e.max():.3e} > {tol:.3e}"


# ---- 1. place_fourth_atom against the reference (golden G15) ----------------------------------------------------
def test_place_fourth_atom_golden(SB):
    from protstruc_amd import geometry as G
    g = {k: v.numpy() for k, v in load_golden("g15_place_fourth_atom").items()}
    for want, params in ((g["x"], (g["length"], g["planar"], g["dihedral"])),
                         (g["x_scalar"], (g["s_length"], g["s_planar"], g["s_dihedral"]))):
        x_np = G.place_fourth_atom(g["a"], g["b"], g["c"], *params)
        assert isinstance(x_np, np.ndarray) and x_np.shape == want.shape
        x_t = G.place_fourth_atom(*(torch.from_numpy(np.asarray(v)).cuda() for v in (g["a"], g["b"], g["c"]) + params))
        assert isinstance(x_t, torch.Tensor) and x_t.is_cuda
        for x in (x_np, x_t.cpu().numpy()):
            assert (np.abs(x - want) <= 1e-5 * (1 + np.abs(want))).all(), np.abs(x - want).max()


# ---- 2. global accuracy against the float64 walk ------------------------------------------------------------------
@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("N", NS)
def test_global_accuracy(SB, kind, N):
    dih, chain, ids, rmask = ragged_batch(kind, N, seed=N)
    sb = SB.from_backbone_dihedrals(dih, chain_idx=chain, chain_ids=ids, residue_mask=rmask)
    want, want_mask = R.build(dih, chain, rmask)
    got = sb.get_xyz().double().cpu().numpy()
    err = np.abs(got - want).max()
    assert np.isfinite(got).all() and err <= 5e-5 * N, f"{kind} N={N}: max |xyz - fp64| = {err:.3e} A > {5e-5 * N:.3e}"
    assert torch.equal(sb.get_atom_mask().cpu(), torch.from_numpy(want_mask).float())
    assert sb.get_atom_mask().dtype == torch.float32 and sb.get_xyz().shape == (3, N, 15, 3)


# ---- 3. local geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("N", NS + [5000])
def test_local_geometry(SB, kind, N):
    dih, chain, ids, rmask = ragged_batch(kind, N, seed=100 + N)
    sb = SB.from_backbone_dihedrals(dih, chain_idx=chain, chain_ids=ids, residue_mask=rmask)
    check_local_geometry(sb, dih, chain, rmask)


# ---- 4. PDB round trip ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.pdb"))), ids=os.path.basename)
def test_pdb_round_trip(SB, path):
    sb = SB.from_pdb(path)
    dih, dmask = sb.backbone_dihedrals()
    nterm = sb.get_n_terminal_mask()
    sb2 = SB.from_backbone_dihedrals(dih, sb.chain_idx, sb.chain_ids, residue_mask=sb.residue_mask)
    assert torch.equal(sb2.get_n_terminal_mask(), nterm)
    chain, rmask = sb.chain_idx.cpu().numpy(), sb.residue_mask.cpu().numpy()
    if rmask.all():   # without gaps, segments start exactly where K2 reports N-termini
        assert (R.segment_starts(*rmask.shape, chain, rmask) == nterm.cpu().numpy()).all()
    dih2, dmask2 = sb2.backbone_dihedrals()
    x2 = sb2.get_xyz().cpu().numpy()
    tol = local_tolerance(x2)
    sel = dmask.cpu().numpy() & R.used_angles(*rmask.shape, chain, rmask)
    d_in, d_out = dih.cpu().numpy(), dih2.cpu().numpy()
    assert np.isfinite(d_in[sel]).all() and dmask2.cpu().numpy()[sel].all()
    e = R.angle_diff(d_out, d_in)[sel]
    assert e.max() <= tol, f"round trip off by {e.max():.3e} > {tol:.3e}"
    if rmask.all():   # without gaps every angle K2 defines is recovered
        assert (sel == dmask.cpu().numpy()).all()


# ---- 5. unused angles -------------------------------------------------------------------------------------------
def test_unused_angles_are_never_read(SB):
    dih, chain, ids, rmask = ragged_batch("random", 300, seed=5)
    unused = R.unused_angles(3, 300, chain, rmask)
    d_nan, d_zero = dih.copy(), dih.copy()
    d_nan[unused], d_zero[unused] = np.nan, 0.0
    a = SB.from_backbone_dihedrals(d_nan, chain, ids, residue_mask=rmask, include_cb=True).get_xyz()
    b = SB.from_backbone_dihedrals(d_zero, chain, ids, residue_mask=rmask, include_cb=True).get_xyz()
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 6. per-residue overrides -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 700, 1500])
def test_per_residue_overrides(SB, N):
    dih, chain, ids, rmask = ragged_batch("random", N, seed=7)
    rng = np.random.default_rng(N)
    ang0, lens0 = R.default_geometry(3, N)
    ang = (ang0 + rng.uniform(-0.1, 0.1, ang0.shape)).astype(np.float32)
    lens = (lens0 + rng.uniform(-0.05, 0.05, lens0.shape)).astype(np.float32)
    sb = SB.from_backbone_dihedrals(dih, chain, ids, residue_mask=rmask, bond_angles=ang, bond_lengths=lens)
    check_local_geometry(sb, dih, chain, rmask, ang=ang, lens=lens)
    want, _ = R.build(dih, chain, rmask, bond_angles=ang, bond_lengths=lens)
    assert np.abs(sb.get_xyz().double().cpu().numpy() - want).max() <= 5e-5 * N


def test_defaults_are_the_float32_ideal_geometry(SB):
    """No overrides == the geometry.IDEAL_* values passed explicitly as float32 arrays, bit for bit."""
    from protstruc_amd import geometry as G
    dih = R.chain_family("helix", 2, 200, seed=9)
    ang = np.broadcast_to(np.array([G.IDEAL_NAC, G.IDEAL_CACN, G.IDEAL_CNCA], np.float32), dih.shape).copy()
    lens = np.broadcast_to(np.array([G.IDEAL_NA, G.IDEAL_AC, G.IDEAL_C_N], np.float32), dih.shape).copy()
    a = SB.from_backbone_dihedrals(dih).get_xyz()
    b = SB.from_backbone_dihedrals(dih, bond_angles=ang, bond_lengths=lens).get_xyz()
    assert torch.equal(a, b)


# ---- 7. CB ------------------------------------------------------------------------------------------------------
def test_cb_and_the_other_slots(SB):
    dih, chain, ids, rmask = ragged_batch("strand", 777, seed=11)
    sb = SB.from_backbone_dihedrals(dih, chain, ids, residue_mask=rmask, include_cb=True)
    x = sb.get_xyz()
    n, ca, c = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    bb, cc = ca - n, c - ca
    aa = torch.linalg.cross(bb, cc, dim=-1)
    cb = -0.58273431 * aa + 0.56802827 * bb - 0.54067466 * cc + ca
    assert ((x[:, :, 4] - cb).abs() <= 1e-5 * (1 + cb.abs())).all()
    rm = torch.from_numpy(rmask).cuda()
    other = [3] + list(range(5, 15))
    assert (x[:, :, other] == 0).all() and (x[~rm] == 0).all()
    m = sb.get_atom_mask()
    want = torch.zeros_like(m)
    want[:, :, [0, 1, 2, 4]] = 1.0
    want[~rm] = 0.0
    assert torch.equal(m, want)
    plain = SB.from_backbone_dihedrals(dih, chain, ids, residue_mask=rmask).get_xyz()
    assert torch.equal(plain[:, :, :3], x[:, :, :3]) and (plain[:, :, 3:] == 0).all()


# ---- 8. determinism / 9. graph capture ----------------------------------------------------------------------------
def test_deterministic(SB):
    from protstruc_amd import ops
    dih = torch.from_numpy(R.chain_family("random", 17, 2500, seed=13)).cuda()
    runs = [ops.backbone_from_dihedrals(dih, include_cb=True) for _ in range(3)]
    for xyz, mask in runs[1:]:
        assert torch.equal(xyz, runs[0][0]) and torch.equal(mask, runs[0][1])


def test_graph_capture(SB):
    from protstruc_amd import ops
    dih = torch.from_numpy(R.chain_family("random", 8, 1300, seed=17)).cuda()
    chain = torch.zeros(8, 1300, device="cuda")
    chain[:, 600:] = 1
    rmask = torch.ones(8, 1300, dtype=torch.bool, device="cuda")
    rmask[3, 100:110] = False
    ops.backbone_from_dihedrals(dih, chain, rmask)   # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gx, gm = ops.backbone_from_dihedrals(dih, chain, rmask, include_cb=True)
    dih.mul_(0.5)
    g.replay()
    torch.cuda.synchronize()
    ex, em = ops.backbone_from_dihedrals(dih, chain, rmask, include_cb=True)
    assert torch.equal(gx, ex) and torch.equal(gm, em)


# ---- 10. edge cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(0, 5), (3, 0), (0, 0)])
def test_empty(SB, B, N):
    sb = SB.from_backbone_dihedrals(torch.zeros(B, N, 3), include_cb=True)
    assert sb.get_xyz().shape == (B, N, 15, 3) and sb.get_atom_mask().shape == (B, N, 15)


def test_c_abi_rejects_bad_arguments(SB):
    from protstruc_amd import _lib
    lib = _lib.load()
    d = torch.zeros(1, 4, 3, device="cuda")
    x = torch.empty(1, 4, 15, 3, device="cuda")
    m = torch.empty(1, 4, 15, device="cuda")
    f = lib.ps_backbone_from_dihedrals_f32
    ok = f(d.data_ptr(), None, None, None, None, x.data_ptr(), m.data_ptr(), 1, 1, 4, 15, None)
    torch.cuda.synchronize()
    assert ok == 0
    assert f(None, None, None, None, None, x.data_ptr(), m.data_ptr(), 0, 1, 4, 15, None) != 0
    assert f(d.data_ptr(), None, None, None, None, x.data_ptr(), m.data_ptr(), 1, 1, 4, 4, None) != 0   # no CB slot
    assert f(d.data_ptr(), None, None, None, None, x.data_ptr(), m.data_ptr(), 0, 1, 4, 2, None) != 0
    assert f(d.data_ptr(), None, None, None, None, x.data_ptr(), m.data_ptr(), 0, -1, 4, 15, None) != 0


def test_other_slot_counts_and_misaligned_outputs(SB):
    """The run-time-A kernel and the scalar head / tail of the 16-byte stores: a narrower row (A = 5) written into
    buffers that start 4 bytes past a 16-byte boundary equals the A = 15 result's first five slots."""
    from protstruc_amd import _lib
    B, N, A = 3, 1031, 5
    dih = torch.from_numpy(R.chain_family("random", B, N, seed=19)).cuda()
    ref = SB.from_backbone_dihedrals(dih, include_cb=True)
    xbuf = torch.full((B * N * A * 3 + 1,), 7.0, device="cuda")
    mbuf = torch.full((B * N * A + 1,), 7.0, device="cuda")
    rc = _lib.load().ps_backbone_from_dihedrals_f32(dih.data_ptr(), None, None, None, None, xbuf[1:].data_ptr(),
                                                    mbuf[1:].data_ptr(), 1, B, N, A, None)
    torch.cuda.synchronize()
    assert rc == 0 and xbuf[0].item() == 7.0 and mbuf[0].item() == 7.0
    assert torch.equal(xbuf[1:].view(B, N, A, 3), ref.get_xyz()[:, :, :A])
    assert torch.equal(mbuf[1:].view(B, N, A), ref.get_atom_mask()[:, :, :A])
