"""The case table of tests/test_gpu_launch_contract.py: one small call per launching entry point of
include/protstruc_hip.h that no older test holds to the launch contract ("Conventions (all entry points)": the caller's
stream, no allocation / synchronisation / host read on the launch path, re-entrant from any thread and stream).

Not a test module, and nothing here touches ``torch.cuda`` at import time (tests/conftest.py starts processes before the
GPU is initialised).  A case gives

    name      the id of the parametrised tests
    symbols   the C symbols the call reaches
    build     "A" | "B" -> {input name: CPU tensor}: the same shapes and dtypes, different values, every integer input
              (idx, residue_type, exclude, groups ...) valid in both, masks with some false entries
    run       {input name: device tensor} -> the tuple of output tensors, through the public function (``ops.*``, or
              ``geometry.*`` where that is the public face); host tables and scalars are fixed inside
    strided   the inputs that are handed over as non-contiguous views

Every case hands at least one input over in a form the shell has to convert before the launch -- float64 or
non-contiguous coordinates, int64 indices, a float mask --, so the shell's temporaries are on the launch path that is
checked.  The in-place ops (standardize_, affine_, the diffusion steps) run on a clone made inside ``run``: the clone is
part of what is enqueued.  tests/test_launch_contract_table.py (no GPU) holds this table against the header.
"""
from typing import Callable, NamedTuple, Tuple

import numpy as np
import torch

from tests import chi_ref, dssp_ref, edge_ref, fape_ref, knn_ref, lddt_ref, sasa_ref, violation_ref

SEED = {"A": 0, "B": 1}


class Case(NamedTuple):
    name: str
    symbols: Tuple[str, ...]
    build: Callable
    run: Callable
    strided: Tuple[str, ...] = ()


def _gen(base, variant):
    return torch.Generator().manual_seed(1000 * base + SEED[variant])


def _np(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _ops():
    from protstruc_amd import ops
    return ops


def _geometry():
    from protstruc_amd import geometry
    return geometry


def on_device(case, variant, device="cuda"):
    """The inputs of ``case`` on the device; those named in ``case.strided`` as views of every second element of the last
    axis of a buffer twice as wide (same shape and values, not contiguous)."""
    out = {}
    for name, t in case.build(variant).items():
        if name in case.strided:
            wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=device)
            view = wide[..., ::2]
            view.copy_(t)
            assert not view.is_contiguous()
            out[name] = view
        else:
            out[name] = t.to(device)
    return out


# ---- frames, FAPE ------------------------------------------------------------------------------------------------------------
def _frames_backward(v):
    g = _gen(1, v)
    B, N, A = 2, 37, 5
    return dict(xyz=(8 * torch.randn(B, N, A, 3, generator=g)).double(), grad_rot=torch.randn(B, N, 3, 3, generator=g),
                grad_trans=torch.randn(B, N, 3, generator=g), residue_mask=torch.rand(B, N, generator=g) < 0.8)


def _run_frames_backward(i):
    return (_ops().frames_backward(i["xyz"], 0, 1, 2, 1, grad_rot=i["grad_rot"], grad_trans=i["grad_trans"],
                                   residue_mask=i["residue_mask"]),)


def _fape(v):
    g = _gen(2, v)
    B, N, A = 2, 9, 4
    target = 8 * torch.randn(B, N, A, 3, generator=g)
    xyz = target + 4 * torch.randn(B, N, A, 3, generator=g)
    rot, trans = fape_ref.frames_from_xyz(xyz, *fape_ref.SLOTS)
    trot, ttrans = fape_ref.frames_from_xyz(target, *fape_ref.SLOTS)
    return dict(rot=rot, trans=trans, points=xyz.reshape(B, N * A, 3), target_rot=trot, target_trans=ttrans,
                target_points=target.reshape(B, N * A, 3).double(), frame_mask=torch.rand(B, N, generator=g) < 0.8,
                point_mask=torch.rand(B, N * A, generator=g) < 0.8, clamp=8 + 4 * torch.rand(B, generator=g),
                grad_loss=torch.randn(B, generator=g))


_FAPE_ARGS = ("rot", "trans", "points", "target_rot", "target_trans", "target_points")


def _run_fape(i):
    # a float clamp: the shell fills the (B,) device tensor itself
    return _ops().fape(*[i[k] for k in _FAPE_ARGS], i["frame_mask"], i["point_mask"], clamp=10.0)


def _run_fape_backward(i):
    return _ops().fape_backward(*[i[k] for k in _FAPE_ARGS], i["grad_loss"], i["frame_mask"], i["point_mask"],
                                clamp=i["clamp"])


# ---- lDDT, clash, peptide bond -----------------------------------------------------------------------------------------------
def _lddt(v):
    c = lddt_ref.random_case(B=3, M=40, mask_kind="p60", groups=4, noise=1.5, seed=300 + SEED[v])
    return dict(points=c.points, target_points=c.target.double(), point_mask=c.point_mask, groups=c.groups.long(),
                grad_S=c.grad_S)


def _run_lddt(i):
    return _ops().lddt(i["points"], i["target_points"], i["point_mask"], i["groups"])


def _run_lddt_backward(i):
    return (_ops().lddt_backward(i["points"], i["target_points"], i["grad_S"], i["point_mask"], i["groups"]),)


def _clash(v):
    c = violation_ref.random_case(B=3, M=40, mask_kind="p60", groups=4, link=True, seed=400 + SEED[v])
    return dict(points=c.points, radius=c.radius.double(), point_mask=c.point_mask, groups=c.groups.long(), link=c.link,
                grad_E=c.grad_E)


def _run_clash(i):
    return _ops().clash(i["points"], i["radius"], i["point_mask"], i["groups"], i["link"])


def _run_clash_backward(i):
    return (_ops().clash_backward(i["points"], i["radius"], i["grad_E"], i["point_mask"], i["groups"], i["link"]),)


def _peptide_bond(v):
    c = violation_ref.bond_case(N=33, keep=0.8, seed=500 + SEED[v], B=2)
    # the junction mask as floats: the shell reduces it to its truth value first
    return dict(xyz=c.xyz, junction_mask=c.junction_mask.float(), next_is_proline=c.next_is_proline, grad_viol=c.grad_viol)


def _run_peptide_bond(i):
    return (_ops().peptide_bond(i["xyz"], i["junction_mask"], i["next_is_proline"]),)


def _run_peptide_bond_backward(i):
    return (_ops().peptide_bond_backward(i["xyz"], i["grad_viol"], i["junction_mask"], i["next_is_proline"]),)


# ---- DSSP, SASA, nearest neighbours ------------------------------------------------------------------------------------------
def _dssp(v):
    c = dssp_ref.synthetic_case(N=40, seed=1 + SEED[v], with_donor=True, helix_break=(v == "B"))
    # the partner lists the assignment reads: the yardstick's own, so that they are valid in both variants
    acceptor = np.stack([dssp_ref.hbonds(c.xyz[b], c.complete[b], c.junction[b], c.donor[b]).acceptor_idx for b in range(3)])
    return dict(xyz=_np(c.xyz).double(), complete=_np(c.complete), junction=_np(c.junction), donor=_np(c.donor),
                acceptor_idx=_np(acceptor).long())


def _run_backbone_hbonds(i):
    return _ops().backbone_hbonds(i["xyz"], i["complete"], i["junction"], i["donor"])


def _run_dssp_assign(i):
    return (_ops().dssp_assign(i["xyz"], i["complete"], i["junction"], i["acceptor_idx"]),)


def _run_dssp(reduced):
    def run(i):
        return (_geometry().dssp(i["xyz"], i["complete"], i["junction"], i["donor"], reduced=reduced),)
    return run


def _sasa(v):
    c = sasa_ref.synthetic_case(40, seed=3 + SEED[v], keys=2)
    return dict(points=_np(c.x), radius=_np(c.r).double(), point_mask=_np(c.mask), isolate=_np(c.isolate).long(),
                sphere=_geometry().sphere_points(24))          # the table is the same in both variants


def _run_sasa(i):
    return _ops().solvent_accessibility(i["points"], i["radius"], i["point_mask"], i["isolate"], sphere=i["sphere"])


def _run_sasa_cached_sphere(i):
    # the table of geometry._SPHERES: on the device since the first (eager) call
    return tuple(_geometry().solvent_accessibility(i["points"], i["radius"], i["point_mask"], i["isolate"], n_points=32))


def _knn(v):
    M, Q = 40, 24
    c = knn_ref.chain_case(M, seed=7 + SEED[v])
    rng = np.random.default_rng(70 + SEED[v])
    queries = np.stack([knn_ref.cloud(Q, seed=71 + 3 * SEED[v] + b) for b in range(3)])
    return dict(points=_np(c.x), point_mask=_np(c.mask), queries=_np(queries).double(), query_mask=_np(rng.random((3, Q)) < 0.8),
                exclude=_np(np.broadcast_to(np.arange(M) // 4, (3, M))).long(), query_exclude=_np(rng.integers(0, 10, (3, Q))))


def _run_knn(i):
    return _ops().nearest_neighbors(i["points"], 5, i["point_mask"], queries=i["queries"], query_mask=i["query_mask"],
                                    exclude=i["exclude"], query_exclude=i["query_exclude"])


# ---- edge features -----------------------------------------------------------------------------------------------------------
def _edge_rbf(v):
    c = edge_ref.residue_case(33, 5, seed=7 + SEED[v])
    return dict(xyz=_np(c.xyz), atom_mask=_np(c.mask), idx=_np(edge_ref.random_graph(3, 33, 6, seed=80 + SEED[v])).long())


def _run_edge_rbf(i):
    return _ops().edge_rbf(i["xyz"], i["idx"], i["atom_mask"], pair_i=[0, 1, 4], pair_j=[1, 1, 2],
                           centers=[2.0, 4.0, 6.0, 8.0, 10.0], sigma=2.0)


def _edge_frames(v):
    rot, trans = edge_ref.random_frames(3, 33, seed=90 + SEED[v])
    mask = np.random.default_rng(91 + SEED[v]).random((3, 33)) >= 0.3
    return dict(rot=_np(rot).double(), trans=_np(trans), frame_mask=_np(mask),
                idx=_np(edge_ref.random_graph(3, 33, 6, seed=92 + SEED[v])).long())


def _run_edge_frames(i):
    return _ops().edge_frames(i["rot"], i["trans"], i["idx"], i["frame_mask"])


# ---- side-chain torsions -----------------------------------------------------------------------------------------------------
def _chi(v):
    c = chi_ref.synthetic_case(3, 33, 15, seed=600 + SEED[v])
    rng = np.random.default_rng(601 + SEED[v])
    shape4 = c.types.shape + (4,)
    return dict(xyz=_np(c.xyz), atom_mask=_np(c.mask), residue_type=_np(c.types).long(),
                chi=_np(rng.uniform(-np.pi, np.pi, size=shape4).astype(np.float32)), chi_select=_np(rng.random(shape4) < 0.6),
                grad_chi=_np(rng.normal(size=shape4).astype(np.float32)),
                grad_out=_np(rng.normal(size=c.xyz.shape).astype(np.float32)))


def _chi_tables():
    atoms, last = chi_ref.tables()
    return dict(chi_atoms=atoms, chi_last=last)


def _run_chi(i):
    return _ops().chi(i["xyz"], i["residue_type"], i["atom_mask"], chi_atoms=_chi_tables()["chi_atoms"])


def _run_chi_backward(i):
    return (_ops().chi_backward(i["xyz"], i["residue_type"], i["grad_chi"], i["atom_mask"],
                                chi_atoms=_chi_tables()["chi_atoms"]),)


def _run_chi_set(i):
    return (_ops().chi_set(i["xyz"], i["chi"], i["residue_type"], i["atom_mask"], i["chi_select"], **_chi_tables()),)


def _run_chi_set_backward(i):
    # any coordinates are a valid ``out``: the derivative is taken on them
    return (_ops().chi_set_backward(i["xyz"], i["grad_out"], i["residue_type"], i["atom_mask"], i["chi_select"],
                                    **_chi_tables()),)


# ---- rigid-body ops ----------------------------------------------------------------------------------------------------------
def _rotations(g, *shape):
    return torch.linalg.qr(torch.randn(*shape, 3, 3, generator=g, dtype=torch.float64))[0]


def _rigid(v):
    g = _gen(7, v)
    B, N, A = 2, 19, 4
    return dict(xyz=8 * torch.randn(B, N, A, 3, generator=g), R=_rotations(g, B, N), t=torch.randn(B, 3, generator=g))


def _run_rigid(i):
    return (_ops().rigid(i["xyz"], i["R"], i["t"], transpose=True),)


def _center_of_mass(v):
    return dict(xyz=(8 * torch.randn(2, 19, 4, 3, generator=_gen(8, v))).double())


def _run_center_of_mass(i):
    return (_ops().center_of_mass(i["xyz"], atom=1),)


def _frames_to_backbone(v):
    g = _gen(9, v)
    ideal = _geometry().ideal_backbone_coordinates((), include_cb=True).contiguous() * (1.0 + 0.1 * SEED[v])
    return dict(rot=_rotations(g, 2, 19).float(), trans=8 * torch.randn(2, 19, 3, generator=g), ideal=ideal)


def _run_frames_to_backbone(i):
    return (_ops().frames_to_backbone(i["rot"], i["trans"], i["ideal"], 6),)


def _kabsch(v):
    g = _gen(10, v)
    src = 8 * torch.randn(3, 12, 4, 3, generator=g)
    dst = (src @ _rotations(g, 3, 1).float() + torch.randn(3, 12, 4, 3, generator=g)).double()
    return dict(src=src, dst=dst, atom_mask=(torch.rand(3, 12, 4, generator=g) < 0.8).float())


def _run_kabsch(i):
    return _ops().kabsch(i["src"], i["dst"], i["atom_mask"])


def _min_dist(v):
    g = _gen(11, v)
    return dict(xyz_one=8 * torch.randn(29, 4, 3, generator=g), query=(8 * torch.randn(7, 3, generator=g)).double())


def _run_min_dist(i):
    return (_ops().min_dist_to_points(i["xyz_one"], i["query"], atom=1),)


# ---- the older entry points that no capture test reaches ---------------------------------------------------------------------
def _backbone_dihedrals(v):
    g = _gen(12, v)
    B, N = 2, 21
    cut = 8 + 5 * SEED[v]
    chain = (torch.arange(N) >= cut).float().expand(B, N).contiguous()
    return dict(xyz=(3 * torch.randn(B, N, 4, 3, generator=g)).double(), chain_idx=chain,
                residue_mask=torch.rand(B, N, generator=g) < 0.8)


def _run_backbone_dihedrals(i):
    return _ops().backbone_dihedrals(i["xyz"], i["chain_idx"], i["residue_mask"])


def _pointwise(v):
    g = _gen(13, v)
    n = 50
    d = torch.stack([1 + torch.rand(n, generator=g), 1 + torch.rand(n, generator=g), 6 * torch.rand(n, generator=g) - 3], dim=-1)
    return dict(a=(3 * torch.randn(n, 3, generator=g)).double(), b=3 * torch.randn(n, 3, generator=g),
                c=3 * torch.randn(n, 3, generator=g), d=d)


def _run_pointwise(i):
    return (_ops().pointwise(3, i["a"], i["b"], i["c"], i["d"]),)


def _standardize(v):
    g = _gen(14, v)
    return dict(xyz=8 * torch.randn(2, 19, 4, 3, generator=g) + 3, atom_mask=(torch.rand(2, 19, 4, generator=g) < 0.8).float())


def _run_standardize(i):
    x = i["xyz"].clone()
    return (x,) + tuple(_ops().standardize_(x, i["atom_mask"]))


def _run_standardize_streaming(i):
    """variant 1 of ps_standardize_variant_f32, the three-sweep kernel: the C ABI has it, the shell has no function for it"""
    from protstruc_amd import _lib
    x, m = i["xyz"].clone(), (i["atom_mask"] != 0).contiguous()
    B, N, A = x.shape[:3]
    mu, std = torch.empty(B, 3, device=x.device), torch.empty(B, 3, device=x.device)
    rc = _lib.load().ps_standardize_variant_f32(x.data_ptr(), m.data_ptr(), mu.data_ptr(), std.data_ptr(), B, N, A, 1,
                                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return x, mu, std


def _affine(v):
    g = _gen(15, v)
    return dict(xyz=8 * torch.randn(2, 19, 4, 3, generator=g), scale=(1 + torch.rand(2, 3, generator=g)).double(),
                shift=torch.randn(2, 3, generator=g))


def _run_affine(i):
    return (_ops().affine_(i["xyz"].clone(), i["scale"], i["shift"]),)


def _diffusion(v):
    g = _gen(16, v)
    B, N, A, T = 2, 19, 4, 3
    state = torch.zeros(_ops().RNG_STATE_WORDS, dtype=torch.int64)
    state[0], state[1] = 99 + SEED[v], 5
    return dict(xyz=8 * torch.randn(B, N, A, 3, generator=g), beta=(0.1 + 0.5 * torch.rand(B, generator=g)).double(),
                betas=0.1 + 0.5 * torch.rand(T, B, generator=g), noise=torch.randn(B, N, A, 3, generator=g), rng_state=state)


def _run_diffuse_frames(i):
    x = i["xyz"].clone()
    return (x,) + tuple(_ops().diffuse_frames_(x, i["beta"], 0, 1, 2, 1, noise=i["noise"]))


def _run_diffusion_trajectory(i):
    x, state = i["xyz"].clone(), i["rng_state"].clone()      # the kernel advances the state: every run starts from the input's
    rot, trans, _ = _ops().diffusion_trajectory_(x, i["betas"], 0, 1, 2, 1, state)
    return x, rot, trans, state


def _mds_finish(v):
    g = _gen(17, v)
    lengths = torch.tensor([15, 11] if v == "A" else [12, 15])
    return dict(X=(5 * torch.randn(2, 3, 15, 3, generator=g)).double(), lengths=lengths)


def _run_mds_finish(i):
    return (_ops().mds_backbone_finish(i["X"], i["lengths"]),)


CASES = (
    Case("frames_backward", ("ps_frames_backward_f32",), _frames_backward, _run_frames_backward),
    Case("fape", ("ps_fape_f32",), _fape, _run_fape, strided=("points",)),
    Case("fape_backward", ("ps_fape_backward_f32",), _fape, _run_fape_backward, strided=("trans",)),
    Case("lddt", ("ps_lddt_f32",), _lddt, _run_lddt),
    Case("lddt_backward", ("ps_lddt_backward_f32",), _lddt, _run_lddt_backward, strided=("points",)),
    Case("clash", ("ps_clash_f32",), _clash, _run_clash),
    Case("clash_backward", ("ps_clash_backward_f32",), _clash, _run_clash_backward, strided=("points",)),
    Case("peptide_bond", ("ps_peptide_bond_f32",), _peptide_bond, _run_peptide_bond, strided=("xyz",)),
    Case("peptide_bond_backward", ("ps_peptide_bond_backward_f32",), _peptide_bond, _run_peptide_bond_backward,
         strided=("grad_viol",)),
    Case("backbone_hbonds", ("ps_backbone_hbonds_f32",), _dssp, _run_backbone_hbonds),
    Case("dssp_assign", ("ps_dssp_assign",), _dssp, _run_dssp_assign),
    Case("dssp", ("ps_backbone_hbonds_f32", "ps_dssp_assign"), _dssp, _run_dssp(False)),
    Case("dssp_reduced", ("ps_backbone_hbonds_f32", "ps_dssp_assign"), _dssp, _run_dssp(True)),
    Case("solvent_accessibility", ("ps_solvent_accessibility_f32",), _sasa, _run_sasa, strided=("points",)),
    Case("solvent_accessibility_cached_sphere", ("ps_solvent_accessibility_f32",), _sasa, _run_sasa_cached_sphere),
    Case("nearest_neighbors", ("ps_nearest_neighbors_f32",), _knn, _run_knn, strided=("points",)),
    Case("edge_rbf", ("ps_edge_rbf_f32",), _edge_rbf, _run_edge_rbf, strided=("xyz",)),
    Case("edge_frames", ("ps_edge_frames_f32",), _edge_frames, _run_edge_frames),
    Case("chi", ("ps_chi_f32",), _chi, _run_chi, strided=("xyz",)),
    Case("chi_backward", ("ps_chi_backward_f32",), _chi, _run_chi_backward),
    Case("chi_set", ("ps_chi_set_f32",), _chi, _run_chi_set, strided=("chi",)),
    Case("chi_set_backward", ("ps_chi_set_backward_f32",), _chi, _run_chi_set_backward, strided=("grad_out",)),
    Case("rigid", ("ps_rigid_f32",), _rigid, _run_rigid, strided=("t",)),
    Case("center_of_mass", ("ps_center_of_mass_f32",), _center_of_mass, _run_center_of_mass),
    Case("frames_to_backbone", ("ps_frames_to_backbone_f32",), _frames_to_backbone, _run_frames_to_backbone, strided=("rot",)),
    Case("kabsch", ("ps_kabsch_f32",), _kabsch, _run_kabsch),
    Case("min_dist_to_points", ("ps_min_dist_to_points_f32",), _min_dist, _run_min_dist, strided=("xyz_one",)),
    Case("backbone_dihedrals", ("ps_backbone_dihedrals_f32",), _backbone_dihedrals, _run_backbone_dihedrals),
    Case("pointwise", ("ps_pointwise_f32",), _pointwise, _run_pointwise, strided=("b",)),
    Case("standardize_", ("ps_standardize_f32",), _standardize, _run_standardize),
    Case("standardize_streaming", ("ps_standardize_variant_f32",), _standardize, _run_standardize_streaming),
    Case("affine_", ("ps_affine_f32",), _affine, _run_affine),
    Case("diffuse_frames_", ("ps_diffuse_frames_f32",), _diffusion, _run_diffuse_frames),
    Case("diffusion_trajectory_", ("ps_diffusion_trajectory_f32",), _diffusion, _run_diffusion_trajectory),
    Case("mds_backbone_finish", ("ps_mds_backbone_finish_f32",), _mds_finish, _run_mds_finish),
)
BY_NAME = {case.name: case for case in CASES}
assert len(BY_NAME) == len(CASES)


def symbols():
    """every C symbol some case reaches"""
    return sorted({s for case in CASES for s in case.symbols})
