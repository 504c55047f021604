"""The side-chain torsion kernels (K27 - K30) on the GPU against the float64 yardstick of tests/chi_ref.py: synthetic
residues at the edges of a wave and of a workgroup's 64 rows, with 15 and 16 atom slots (row strides of 45 floats, odd,
and 48, padded to 49 in LDS), 45 % of the atoms masked with NaN under the mask, padding types and a structure with every
atom masked; and four PDB files in one padded batch.  Every case runs once through ``ops`` on contiguous tensors and once
through the C ABI with ``xyz`` and every output as views 4, 8 and 12 bytes past a 16-byte boundary inside sentinel-filled
storage: the two must agree bit for bit -- which is also the determinism check -- and no sentinel may change."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import chi_ref as R

pytestmark = pytest.mark.gpu

PDB_FILES = ("1REX", "4EOT", "5cjx_HL", "4uuj")
CASES = [(N, A) for N in (1, 63, 64, 65, 129, 257) for A in (15, 16)] + ["pdb"]
SET_MODES = [(relative, selected) for relative in (False, True) for selected in (False, True)]
CHI_TOL = 4.8e-7      # two float32 spacings at pi: the arithmetic is double, only the rounding and atan2's last bit differ
SENTINEL = 777.0


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import protstruc_amd
    from protstruc_amd import _lib, geometry, ops  # noqa: F401 -- the submodules the tests reach through the package
    _lib.load()
    return protstruc_amd


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def circular(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))))


class Inputs:
    """One case with everything the tests share, computed once: the yardstick's results, and the random angles, selection
    and upstream gradients"""

    def __init__(self, key):
        self.key = key
        if key == "pdb":
            self.case = R.pdb_case([name + ".pdb" for name in PDB_FILES])
        else:
            N, A = key
            self.case = R.synthetic_case(3, N, A, seed=100 * N + A, masked=0.45)
        c = self.case
        self.atoms, self.last = R.tables()
        rng = np.random.default_rng(17)
        shape4 = c.types.shape + (4,)
        self.chi64, self.defined = R.measure(c.xyz, c.types, c.mask, self.atoms)
        self.g_chi = rng.normal(size=shape4).astype(np.float32)
        self.g_out = rng.normal(size=c.xyz.shape).astype(np.float32)
        self.want = rng.uniform(-np.pi, np.pi, size=shape4).astype(np.float32)
        self.select = rng.random(shape4) < 0.6
        self.clean = np.where(c.mask[..., None], c.xyz, 0).astype(np.float64)

    @functools.lru_cache(maxsize=None)
    def turned(self, relative, selected):
        c = self.case
        return R.set_chi(c.xyz, self.want, c.types, c.mask, self.atoms, self.last, self.select if selected else None, relative)

    def chi_input(self, selected):
        """the angles handed to the kernel: NaN wherever the yardstick does not use them"""
        used = self.turned(False, selected).turned
        return np.where(used, self.want, np.float32(np.nan)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(key):
    return Inputs(key)


def ids(key):
    return key if isinstance(key, str) else f"N{key[0]}-A{key[1]}"


# ---- K27 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES, ids=ids)
def test_chi_meets_the_yardstick(pkg, key):
    inp = inputs(key)
    c = inp.case
    assert np.isnan(c.xyz).any() or key == "pdb"
    chi, mask = pkg.ops.chi(dev(c.xyz), dev(c.types), dev(c.mask), chi_atoms=inp.atoms)
    chi, mask = chi.cpu().numpy(), mask.cpu().numpy()
    assert chi.dtype == np.float32 and mask.dtype == bool and chi.shape == mask.shape == c.types.shape + (4,)
    assert (mask == inp.defined).all()
    assert not np.isnan(chi).any()                                           # although there is NaN under the mask
    assert (chi[~inp.defined].view(np.int32) == 0).all()                     # exactly +0 where undefined
    if inp.defined.any():
        worst = circular(chi, inp.chi64)[inp.defined].max()
        print(f"[chi {ids(key)}] angles {int(inp.defined.sum())}, worst circular difference {worst:.3e}")
        assert worst <= CHI_TOL
    only_chi, none = pkg.ops.chi(dev(c.xyz), dev(c.types), dev(c.mask), chi_atoms=inp.atoms, want_mask=False)
    none2, only_mask = pkg.ops.chi(dev(c.xyz), dev(c.types), dev(c.mask), chi_atoms=inp.atoms, want_chi=False)
    assert none is None and none2 is None
    assert (bits(only_chi).cpu().numpy() == chi.view(np.int32)).all() and (only_mask.cpu().numpy() == mask).all()


# ---- K28 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES, ids=ids)
def test_chi_backward_meets_the_yardstick(pkg, key):
    inp = inputs(key)
    c = inp.case
    g_chi = np.where(inp.defined, inp.g_chi, np.float32(np.nan))            # not read at an undefined angle
    g64 = R.measure_backward(c.xyz, c.types, c.mask, inp.atoms, inp.g_chi)
    first = pkg.ops.chi_backward(dev(c.xyz), dev(c.types), dev(g_chi), dev(c.mask), chi_atoms=inp.atoms)
    second = pkg.ops.chi_backward(dev(c.xyz), dev(c.types), dev(g_chi), dev(c.mask), chi_atoms=inp.atoms)
    assert torch.equal(bits(first), bits(second))                            # two runs are bit-identical
    g = first.cpu().numpy()
    assert g.shape == c.xyz.shape and g.dtype == np.float32
    print(f"[chi_backward {ids(key)}] worst difference {np.abs(g - g64).max():.3e} at scale {np.abs(g64).max():.3e}")
    assert np.allclose(g, g64, rtol=1e-6, atol=1e-6)
    # slots that no defined angle reads, and whole residues without angles, are exact zeros
    read = np.zeros(c.mask.shape, dtype=bool)
    lay = R.layout(c.xyz.shape, c.types, c.mask, inp.atoms)
    b, n, k = np.nonzero(lay.defined)
    for j in range(4):
        read[b, n, lay.slots[b, n, k, j]] = True
    assert (g[~read].view(np.int32) == 0).all()
    # autograd through the public function gives the same tensor
    x = dev(c.xyz).requires_grad_()
    result = pkg.geometry.side_chain_torsions(x, dev(c.types), dev(c.mask))
    assert isinstance(result, pkg.geometry.SideChainTorsions) and not result.mask.requires_grad
    up = dev(inp.g_chi)
    torch.where(result.mask, result.chi * up, torch.zeros_like(up)).sum().backward()
    assert torch.equal(bits(x.grad), bits(first))


# ---- K29 ---------------------------------------------------------------------------------------------------------------
def bonded_change(before64, after64, mask):
    """the largest change of an intra-residue distance that was below 1.95 A between two present atoms"""
    d0 = np.linalg.norm(before64[:, :, :, None] - before64[:, :, None, :], axis=-1)
    d1 = np.linalg.norm(after64[:, :, :, None] - after64[:, :, None, :], axis=-1)
    bonded = mask[:, :, :, None] & mask[:, :, None, :] & (d0 < 1.95)
    return np.abs(d1 - d0)[bonded].max() if bonded.any() else 0.0


@pytest.mark.parametrize("relative,selected", SET_MODES, ids=lambda v: str(int(v)))
@pytest.mark.parametrize("key", CASES, ids=ids)
def test_chi_set_meets_the_yardstick(pkg, key, relative, selected):
    inp = inputs(key)
    c = inp.case
    ref = inp.turned(relative, selected)
    args = (dev(c.xyz), dev(inp.chi_input(selected)), dev(c.types), dev(c.mask), dev(inp.select) if selected else None)
    tables = dict(chi_atoms=inp.atoms, chi_last=inp.last, relative=relative)
    first, second = pkg.ops.chi_set(*args, **tables), pkg.ops.chi_set(*args, **tables)
    assert torch.equal(bits(first), bits(second))                            # two runs are bit-identical
    out = first.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == c.xyz.shape
    moved = np.broadcast_to(ref.moved[..., None], out.shape)
    # every float the yardstick did not turn is the input's bit pattern, NaN included
    assert (out.view(np.int32)[~moved] == c.xyz.view(np.int32)[~moved]).all()
    proline = c.types == 12
    assert (out.view(np.int32)[proline] == c.xyz.view(np.int32)[proline]).all()
    # every turned float is within one float32 spacing of the float64 result
    ref32 = np.where(moved, ref.out.astype(np.float32), c.xyz)
    if moved.any():
        off = np.abs(out.astype(np.float64) - ref.out)[moved]
        room = np.spacing(np.abs(ref.out).astype(np.float32)).astype(np.float64)[moved]
        print(f"[chi_set {ids(key)} rel={relative} sel={selected}] turned floats {int(moved.sum())}, "
              f"differing from the rounded yardstick {int((out != ref32)[moved].sum())}, worst {(off / room).max():.3f} spacings")
        assert (off <= room).all()
    # K27 on the output returns the requested angles, and bonded distances are kept: each within twice the yardstick's own
    # error on these inputs -- its float64 result rounded to float32 and measured again, rounding of the angle included
    target = inp.chi64 + inp.want if relative else inp.want.astype(np.float64)
    again_ref = R.measure(ref32, c.types, c.mask, inp.atoms)[0].astype(np.float32)
    again, _ = pkg.ops.chi(first, dev(c.types), dev(c.mask), chi_atoms=inp.atoms)
    again = again.cpu().numpy()
    if ref.turned.any():
        err_ref, err = circular(again_ref, target)[ref.turned].max(), circular(again, target)[ref.turned].max()
        print(f"    angles: kernel {err:.3e}, yardstick {err_ref:.3e}")
        assert err <= 2 * err_ref
    kept_ref = bonded_change(inp.clean, np.where(c.mask[..., None], ref32, 0).astype(np.float64), c.mask)
    kept = bonded_change(inp.clean, np.where(c.mask[..., None], out, 0).astype(np.float64), c.mask)
    print(f"    bonded distances: kernel {kept:.3e}, yardstick {kept_ref:.3e}")
    assert kept <= 2 * kept_ref


# ---- K30 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relative,selected", [(False, False), (True, True)], ids=lambda v: str(int(v)))
@pytest.mark.parametrize("key", CASES, ids=ids)
def test_chi_set_backward_meets_the_yardstick(pkg, key, relative, selected):
    inp = inputs(key)
    c = inp.case
    ref = inp.turned(relative, selected)
    select = dev(inp.select) if selected else None
    chi = dev(inp.chi_input(selected)).requires_grad_()
    tables = dict(chi_atoms=inp.atoms, chi_last=inp.last)
    out = pkg.ops.chi_set(dev(c.xyz), chi.detach(), dev(c.types), dev(c.mask), select, relative=relative, **tables)
    g_out = np.where(c.mask[..., None], inp.g_out, np.float32(np.nan))      # nothing is read under the mask
    first = pkg.ops.chi_set_backward(out, dev(g_out), dev(c.types), dev(c.mask), select, **tables)
    second = pkg.ops.chi_set_backward(out, dev(g_out), dev(c.types), dev(c.mask), select, **tables)
    assert torch.equal(bits(first), bits(second))
    g = first.cpu().numpy()
    g64 = R.set_chi_backward(out.cpu().numpy(), inp.g_out, c.types, c.mask, inp.atoms, inp.last, inp.select if selected else None)
    print(f"[chi_set_backward {ids(key)}] worst difference {np.abs(g - g64).max():.3e} at scale {np.abs(g64).max():.3e}")
    assert g.shape == c.types.shape + (4,) and np.allclose(g, g64, rtol=1e-5, atol=1e-5)
    assert (g[~ref.turned].view(np.int32) == 0).all()                        # exact 0 at angles that were not turned
    # autograd through the public function gives the same tensor
    turned = pkg.geometry.set_side_chain_torsions(dev(c.xyz), chi, dev(c.types), dev(c.mask), select, relative)
    assert torch.equal(bits(turned), bits(out))
    up = dev(inp.g_out)
    torch.where(dev(c.mask)[..., None], turned * up, torch.zeros_like(up)).sum().backward()
    assert torch.equal(bits(chi.grad), bits(first))


# ---- misaligned views inside sentinels ----------------------------------------------------------------------------------------
def carve(shape, front, dtype=torch.float32):
    """a view of ``shape`` that starts ``front`` elements into sentinel-filled storage whose start is 16-byte aligned"""
    back = 9
    n = int(np.prod(shape))
    buf = torch.full((front + n + back,), SENTINEL if dtype == torch.float32 else 77, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[front:front + n].view(shape)


def intact(buf, front, n):
    fill = SENTINEL if buf.dtype == torch.float32 else 77
    return bool((buf[:front] == fill).all()) and bool((buf[front + n:] == fill).all())


@pytest.mark.parametrize("front", [1, 2, 3])
@pytest.mark.parametrize("key", CASES, ids=ids)
def test_views_off_a_16_byte_boundary_inside_sentinels(pkg, key, front):
    """the C ABI with xyz and every output ``front`` floats (bytes for chi_mask) past a 16-byte boundary: bitwise what
    ``ops`` returns on contiguous tensors, and the sentinels before and after every output untouched"""
    inp = inputs(key)
    c = inp.case
    lib = pkg._lib.load()
    B, N, A = c.xyz.shape[:3]
    T = inp.atoms.shape[0]
    ints = lambda table: (ctypes.c_int * table.size)(*table.ravel().tolist())    # noqa: E731
    atoms, last = ints(inp.atoms), ints(inp.last)
    stream = torch.cuda.current_stream().cuda_stream
    types, mask, select = dev(c.types), dev(c.mask), dev(inp.select)
    _, xyz = carve(c.xyz.shape, front)
    xyz.copy_(dev(c.xyz))
    assert xyz.data_ptr() % 16 == 4 * front
    want, g_chi, g_out = dev(inp.chi_input(True)), dev(np.where(inp.defined, inp.g_chi, np.float32(0))), dev(np.where(c.mask[..., None], inp.g_out, np.float32(0)))
    n4, n3 = B * N * 4, B * N * A * 3
    chi_buf, chi = carve((B, N, 4), front)
    mask_buf, chi_mask = carve((B, N, 4), front, torch.uint8)
    grad_buf, grad_xyz = carve(c.xyz.shape, front)
    out_buf, out = carve(c.xyz.shape, front)
    gchi_buf, grad_chi = carve((B, N, 4), front)
    assert lib.ps_chi_f32(xyz.data_ptr(), mask.data_ptr(), types.data_ptr(), atoms, T, chi.data_ptr(), chi_mask.data_ptr(),
                          B, N, A, stream) == 0
    assert lib.ps_chi_backward_f32(xyz.data_ptr(), mask.data_ptr(), types.data_ptr(), atoms, T, g_chi.data_ptr(),
                                   grad_xyz.data_ptr(), B, N, A, stream) == 0
    assert lib.ps_chi_set_f32(xyz.data_ptr(), mask.data_ptr(), types.data_ptr(), atoms, last, T, want.data_ptr(),
                              select.data_ptr(), 0, out.data_ptr(), B, N, A, stream) == 0
    assert lib.ps_chi_set_backward_f32(out.data_ptr(), mask.data_ptr(), types.data_ptr(), atoms, last, T, select.data_ptr(),
                                       g_out.data_ptr(), grad_chi.data_ptr(), B, N, A, stream) == 0
    torch.cuda.synchronize()
    assert intact(chi_buf, front, n4) and intact(mask_buf, front, n4) and intact(gchi_buf, front, n4)
    assert intact(grad_buf, front, n3) and intact(out_buf, front, n3)
    x = dev(c.xyz)
    tables = dict(chi_atoms=inp.atoms, chi_last=inp.last)
    ref_chi, ref_mask = pkg.ops.chi(x, types, mask, chi_atoms=inp.atoms)
    assert torch.equal(bits(chi), bits(ref_chi)) and torch.equal(chi_mask, ref_mask.to(torch.uint8))
    assert torch.equal(bits(grad_xyz), bits(pkg.ops.chi_backward(x, types, g_chi, mask, chi_atoms=inp.atoms)))
    ref_out = pkg.ops.chi_set(x, want, types, mask, select, **tables)
    assert torch.equal(bits(out), bits(ref_out))
    assert torch.equal(bits(grad_chi), bits(pkg.ops.chi_set_backward(ref_out, g_out, types, mask, select, **tables)))


def test_no_mask_no_selection_and_another_table(pkg):
    """atom_mask None and chi_select None reach the kernels as NULL; a table of two types with one angle each"""
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(2, 70, 6, 3)).astype(np.float32) * 2
    types = rng.integers(-3, 4, size=(2, 70)).astype(np.int32)
    atoms = np.full((2, 4, 4), -1)
    atoms[0, 0], atoms[1, 2] = [0, 1, 2, 3], [5, 3, 1, 2]                    # any order of slots; angle 2 alone
    last = np.full((2, 4), -1)
    last[0, 0], last[1, 2] = 5, 2
    want = rng.uniform(-np.pi, np.pi, size=(2, 70, 4)).astype(np.float32)
    chi, mask = pkg.ops.chi(dev(xyz), dev(types), chi_atoms=atoms)
    ref, defined = R.measure(xyz, types, None, atoms)
    assert (mask.cpu().numpy() == defined).all() and defined.sum() == ((types == 0) | (types == 1)).sum()
    assert circular(chi.cpu().numpy(), ref)[defined].max() <= CHI_TOL
    out = pkg.ops.chi_set(dev(xyz), dev(want), dev(types), chi_atoms=atoms, chi_last=last).cpu().numpy()
    t = R.set_chi(xyz, want, types, None, atoms, last)
    moved = np.broadcast_to(t.moved[..., None], out.shape)
    assert (out.view(np.int32)[~moved] == xyz.view(np.int32)[~moved]).all()
    assert (np.abs(out - t.out) <= np.spacing(np.abs(t.out).astype(np.float32)))[moved].all()
    again = pkg.ops.chi(dev(out), dev(types), chi_atoms=atoms)[0].cpu().numpy()
    assert circular(again, want)[t.turned].max() < 1e-4


def test_ops_with_nothing_to_do_launch_nothing(pkg, monkeypatch):
    def no_launch(*args):
        raise AssertionError("an empty call was launched")

    monkeypatch.setattr(pkg.ops, "_launch", no_launch)
    atoms, last = R.tables()
    for B, N in ((0, 5), (3, 0)):
        xyz = torch.zeros(B, N, 15, 3, device="cuda")
        types = torch.zeros(B, N, dtype=torch.int32, device="cuda")
        chi = torch.zeros(B, N, 4, device="cuda")
        got, mask = pkg.ops.chi(xyz, types, chi_atoms=atoms)
        assert got.shape == mask.shape == (B, N, 4)
        assert pkg.ops.chi_backward(xyz, types, chi, chi_atoms=atoms).shape == (B, N, 15, 3)
        assert pkg.ops.chi_set(xyz, chi, types, chi_atoms=atoms, chi_last=last).shape == (B, N, 15, 3)
        assert pkg.ops.chi_set_backward(xyz, xyz, types, chi_atoms=atoms, chi_last=last).shape == (B, N, 4)


# ---- StructureBatch -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(pkg):
    import os
    return pkg.StructureBatch.from_pdb([os.path.join(R.GOLDEN, name + ".pdb") for name in PDB_FILES])


def test_structure_batch_torsions(pkg, batch):
    inp = inputs("pdb")
    result = batch.side_chain_torsions()
    present = batch.get_atom_mask() & batch.residue_mask[:, :, None]
    direct = pkg.geometry.side_chain_torsions(batch.get_xyz(), batch.get_seq_idx().to(torch.int32), present)
    assert torch.equal(bits(result.chi), bits(direct.chi)) and torch.equal(result.mask, direct.mask)
    assert (result.mask.cpu().numpy() == inp.defined).all() and int(result.mask.sum()) > 1500
    assert batch.get_xyz().shape[1] > min(int(n) for n in batch.get_total_lengths())          # there is padding
    periodic = batch.chi_pi_periodic()
    assert periodic.shape == result.mask.shape and periodic.dtype == torch.bool and periodic.is_cuda
    turned = batch.with_side_chain_torsions(result.chi)                      # the measured angles: nothing moves far
    assert (turned.get_xyz() - batch.get_xyz())[present].abs().max() < 1e-4
    assert turned.get_seq() is batch.get_seq() and torch.equal(turned.get_atom_mask(), batch.get_atom_mask())


def test_the_chain_from_angles_to_a_clash_loss(pkg):
    """chi -> with_side_chain_torsions -> steric_clashes -> backward, all in HIP: a plumbing check against a central
    finite difference (step 1e-3 rad) of the float64 yardstick of the set step followed by the project's clash kernel"""
    import os
    sb = pkg.StructureBatch.from_pdb(os.path.join(R.GOLDEN, "1REX.pdb"))
    case = R.pdb_case(["1REX.pdb"])
    atoms, last = R.tables()
    rng = np.random.default_rng(11)
    want = rng.uniform(-np.pi, np.pi, size=case.types.shape + (4,)).astype(np.float32)   # random rotamers: clashes
    chi = dev(want).requires_grad_()
    new = sb.with_side_chain_torsions(chi)
    assert new.get_xyz().requires_grad
    new.steric_clashes().sum().backward()
    grad = chi.grad.cpu().numpy()
    turned = R.set_chi(case.xyz, want, case.types, case.mask, atoms, last).turned
    assert np.isfinite(grad).all() and (grad != 0).any() and (grad[~turned] == 0).all()

    def loss_at(angles):
        t = R.set_chi(case.xyz, angles, case.types, case.mask, atoms, last)
        xyz = np.where(t.moved[..., None], t.out.astype(np.float32), case.xyz)
        moved = pkg.StructureBatch(dev(xyz), sb.get_atom_mask(), sb.chain_idx, sb.get_chain_ids(), sb.get_seq(), sb.residue_idx)
        return moved.steric_clashes().double().cpu().numpy()                 # per residue: the difference is taken in double

    sizeable = np.argwhere(np.abs(grad) > 0.2 * np.abs(grad).max())          # an angle the loss feels
    for b, n, k in sizeable[rng.choice(len(sizeable), size=3, replace=False)]:
        plus, minus = want.astype(np.float64), want.astype(np.float64)
        plus[b, n, k] += 1e-3
        minus[b, n, k] -= 1e-3
        fd = (loss_at(plus) - loss_at(minus)).sum() / 2e-3
        print(f"[chain] angle {(b, n, k)}: backward {grad[b, n, k]:.5f}, finite difference {fd:.5f}")
        assert abs(grad[b, n, k] - fd) <= 0.05 * abs(fd)
