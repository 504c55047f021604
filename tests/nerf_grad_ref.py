"""Yardstick of the backbone builder's backward pass (ps_backbone_from_dihedrals_backward_f32): the sequential builder of
tests/nerf_ref.py restated in torch, differentiated by ``torch.autograd.grad``.

``build`` walks the chain one atom after another with the segment rules of ``nerf_ref.build`` (a start at residue 0, at a
change of ``chain_idx`` with NaN != NaN, and after a masked residue), vectorised over the batch: at every residue both
the placed triple and the ideal start triple are evaluated and ``torch.where`` picks one, so a start never sees the
atoms before it.  Inputs are float32 (the defaults rounded to float32 as the kernel rounds them) promoted to the
working dtype.  ``gradient`` is the gradient of sum(grad_xyz * xyz) over the slots the builder writes and the rows of
unmasked residues, selected by ``torch.where`` (NaN anywhere else never enters): float64 is the reference ("want"),
float32 on the CPU the comparison.

``torque_gradient`` is the closed form the kernel evaluates -- an internal coordinate moves everything downstream of it
as a rigid body, so its gradient is a projection of the downstream force G and torque T (segmented suffix sums over the
3 N backbone atoms) -- written with torch ops from the coordinates alone.  tests/test_nerf_backward_host.py pins it to
the autograd gradient in float64, so the kernel's formulas are tested without a GPU.
"""
import numpy as np
import torch

from tests import nerf_ref

KINDS = ("dihedrals", "bond_angles", "bond_lengths")
CB_SLOT = 4


def _t(x, dtype):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.detach().cpu().to(dtype)


def _unit(v):
    return v / torch.linalg.vector_norm(v, dim=-1, keepdim=True)


def _cross(a, b):
    return torch.linalg.cross(a, b, dim=-1)


def place_fourth_atom(a, b, c, length, planar, dihedral):
    """nerf_ref.place_fourth_atom in torch; a, b, c (B, 3), the three parameters (B,)."""
    bc = _unit(b - c)
    n = _unit(_cross(b - a, bc))
    m = _cross(n, bc)
    length, planar, dihedral = length[:, None], planar[:, None], dihedral[:, None]
    return c + (length * torch.cos(planar)) * bc + (length * torch.sin(planar) * torch.cos(dihedral)) * m \
        - (length * torch.sin(planar) * torch.sin(dihedral)) * n


def geometry_or_default(B, N, bond_angles=None, bond_lengths=None):
    """(bond_angles, bond_lengths) as float32 (B, N, 3) CPU tensors: the given ones or nerf_ref.default_geometry."""
    ang, lens = nerf_ref.default_geometry(B, N)
    ang = torch.from_numpy(ang) if bond_angles is None else _t(bond_angles, torch.float32)
    lens = torch.from_numpy(lens) if bond_lengths is None else _t(bond_lengths, torch.float32)
    return ang, lens


def _rules(B, N, chain_idx, residue_mask):
    ch = None if chain_idx is None else _t(chain_idx, torch.float32).numpy()
    rm = None if residue_mask is None else (_t(residue_mask, torch.float32) != 0).numpy()
    start = torch.from_numpy(nerf_ref.segment_starts(B, N, ch, rm))
    live = torch.ones(B, N, dtype=torch.bool) if rm is None else torch.from_numpy(rm)
    return start, live


def build(dihedrals, chain_idx=None, residue_mask=None, bond_angles=None, bond_lengths=None, include_cb=False, n_slots=15):
    """xyz (B, N, n_slots, 3) in the dtype of ``dihedrals`` by the sequential walk; differentiable with respect to
    ``dihedrals``, ``bond_angles`` and ``bond_lengths`` (tensors of one floating dtype on one device; the last two are
    required here)."""
    B, N = dihedrals.shape[:2]
    dt, dev = dihedrals.dtype, dihedrals.device
    start, live = (t.to(dev) for t in _rules(B, N, chain_idx, residue_mask))
    zero = torch.zeros(B, dtype=dt, device=dev)
    rows = []
    n = ca = c = None
    for i in range(N):
        na, ac, nac = bond_lengths[:, i, 0], bond_lengths[:, i, 1], bond_angles[:, i, 0]
        n_s = torch.stack([na * torch.cos(nac), na * torch.sin(nac), zero], dim=-1)
        ca_s = torch.zeros(B, 3, dtype=dt, device=dev)
        c_s = torch.stack([ac, zero, zero], dim=-1)
        if i == 0:
            n, ca, c = n_s, ca_s, c_s
        else:
            n1 = place_fourth_atom(n, ca, c, bond_lengths[:, i - 1, 2], bond_angles[:, i - 1, 1], dihedrals[:, i - 1, 1])
            ca1 = place_fourth_atom(ca, c, n1, bond_lengths[:, i, 0], bond_angles[:, i - 1, 2], dihedrals[:, i - 1, 2])
            c1 = place_fourth_atom(c, n1, ca1, bond_lengths[:, i, 1], bond_angles[:, i, 0], dihedrals[:, i, 0])
            s = start[:, i, None]
            n, ca, c = torch.where(s, n_s, n1), torch.where(s, ca_s, ca1), torch.where(s, c_s, c1)
        slots = [n, ca, c] + [torch.zeros(B, 3, dtype=dt, device=dev)] * (n_slots - 3)
        if include_cb:
            bb, cc = ca - n, c - ca
            slots[CB_SLOT] = nerf_ref.CB_COEF[0] * _cross(bb, cc) + nerf_ref.CB_COEF[1] * bb + nerf_ref.CB_COEF[2] * cc + ca
        row = torch.stack(slots, dim=1)
        rows.append(torch.where(live[:, i, None, None], row, torch.zeros_like(row)))
    if not rows:
        return torch.zeros(B, 0, n_slots, 3, dtype=dt, device=dev)
    return torch.stack(rows, dim=1)


def read_entries(B, N, A, residue_mask=None, include_cb=False):
    """(B, N, A) bool: the entries of grad_xyz the backward pass reads (slots 0, 1, 2, and 4 with CB, of unmasked rows)."""
    _, live = _rules(B, N, None, residue_mask)
    used = torch.zeros(B, N, A, dtype=torch.bool)
    used[:, :, :3] = True
    if include_cb:
        used[:, :, CB_SLOT] = True
    return used & live[:, :, None]


def leaves(dihedrals, bond_angles=None, bond_lengths=None, dtype=torch.float64):
    """The three inputs as float32-rounded leaf tensors of ``dtype`` that require grad."""
    B, N = dihedrals.shape[:2]
    ang, lens = geometry_or_default(B, N, bond_angles, bond_lengths)
    return tuple(x.to(dtype).requires_grad_(True) for x in (_t(dihedrals, torch.float32), ang, lens))


def gradient(dihedrals, grad_xyz, chain_idx=None, residue_mask=None, bond_angles=None, bond_lengths=None, include_cb=False,
             dtype=torch.float64):
    """(grad_dihedrals, grad_bond_angles, grad_bond_lengths), each (B, N, 3), of sum(grad_xyz * xyz) over the entries the
    backward pass reads, by autograd of the sequential walk in ``dtype`` on the CPU."""
    B, N, A = grad_xyz.shape[:3]
    dih, ang, lens = leaves(dihedrals, bond_angles, bond_lengths, dtype)
    if B == 0 or N == 0:
        return tuple(torch.zeros(B, N, 3, dtype=dtype) for _ in KINDS)
    xyz = build(dih, chain_idx, residue_mask, ang, lens, include_cb, A)
    used = read_entries(B, N, A, residue_mask, include_cb)
    g = torch.where(used[..., None], _t(grad_xyz, dtype), torch.zeros((), dtype=dtype))
    grads = torch.autograd.grad((g * xyz).sum(), (dih, ang, lens), allow_unused=True)
    return tuple(torch.zeros(B, N, 3, dtype=dtype) if x is None else x for x in grads)


def coordinates(dihedrals, chain_idx=None, residue_mask=None, bond_angles=None, bond_lengths=None, include_cb=False,
                n_slots=15, dtype=torch.float64):
    """``build`` on float32-rounded inputs in ``dtype``, detached."""
    dih, ang, lens = leaves(dihedrals, bond_angles, bond_lengths, dtype)
    with torch.no_grad():
        return build(dih, chain_idx, residue_mask, ang, lens, include_cb, n_slots)


def torque_gradient(xyz, grad_xyz, chain_idx=None, residue_mask=None, include_cb=False, dtype=torch.float64):
    """The closed form of the kernel in ``dtype`` torch ops: the three (B, N, 3) gradients from the coordinates, the
    upstream gradient and the segment rules alone (include/protstruc_hip.h states the formulas)."""
    x = _t(xyz, dtype)
    B, N, A = x.shape[:3]
    out = [torch.zeros(B, N, 3, dtype=dtype) for _ in KINDS]
    if B == 0 or N == 0:
        return tuple(out)
    start, live = _rules(B, N, chain_idx, residue_mask)
    used = read_entries(B, N, A, residue_mask, include_cb)
    g = torch.where(used[..., None], _t(grad_xyz, dtype), torch.zeros((), dtype=dtype))
    lv = live[..., None]
    z3 = torch.zeros((), dtype=dtype)
    xn, xa, xc = (torch.where(lv, x[:, :, s], z3) for s in range(3))
    gn, ga, gc = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    if include_cb:
        k0, k1, k2 = nerf_ref.CB_COEF
        gb = g[:, :, CB_SLOT]
        bb, cc = xa - xn, xc - xa
        g_bb = k0 * _cross(cc, gb) + k1 * gb
        g_cc = k0 * _cross(gb, bb) + k2 * gb
        gn, ga, gc = gn - g_bb, ga + g_bb - g_cc + gb, gc + g_cc
    # segmented inclusive suffix sums at each residue's C, CA and N (a masked residue is the last of its segment and
    # contributes nothing)
    last = torch.ones(B, N, dtype=torch.bool)
    last[:, :-1] = start[:, 1:]
    G = torch.zeros(B, N, 3, 3, dtype=dtype)   # [b, i, atom (N, CA, C)]
    T = torch.zeros(B, N, 3, 3, dtype=dtype)
    Gs, Ts = torch.zeros(B, 3, dtype=dtype), torch.zeros(B, 3, dtype=dtype)
    for i in range(N - 1, -1, -1):
        Gs = torch.where(last[:, i, None], z3, Gs)
        Ts = torch.where(last[:, i, None], z3, Ts)
        for a, (xa_, ga_) in ((2, (xc, gc)), (1, (xa, ga)), (0, (xn, gn))):
            Gs = Gs + ga_[:, i]
            Ts = Ts + _cross(xa_[:, i], ga_[:, i])
            G[:, i, a], T[:, i, a] = Gs, Ts

    def dot(u, v):
        return (u * v).sum(-1)

    def turn(u, p, k, a):   # u . (T[k] - p x G[k])
        return dot(u, T[:, k, a] - _cross(p, G[:, k, a]))

    d, ang, lens = out
    zero = torch.zeros((), dtype=dtype)
    if True:
        # a residue's own parameters
        i = torch.arange(N)
        cont = ~start & live          # continues a segment and is visible
        head = start & live
        u_na, u_ac = _unit(xa - xn), _unit(xc - xa)
        d[:, :, 0] = torch.where(cont, turn(u_na, xa, i, 2), zero)
        w = _unit(_cross(xn - xa, xc - xa))
        zax = _unit(_cross(xc - xa, xn - xa))
        ang[:, :, 0] = torch.where(cont, turn(w, xa, i, 2), torch.where(head, dot(zax, _cross(xn - xa, gn)), zero))
        lens[:, :, 0] = torch.where(cont, dot(u_na, G[:, :, 1]), torch.where(head, dot(_unit(xn - xa), gn), zero))
        lens[:, :, 1] = torch.where(live, dot(u_ac, G[:, :, 2]), zero)
        if N > 1:
            # the junction j -> i = j + 1
            j, i = torch.arange(N - 1), torch.arange(1, N)
            c = cont[:, 1:]
            cj, aj, ni, ai = xc[:, :-1], xa[:, :-1], xn[:, 1:], xa[:, 1:]
            u_cn = _unit(ni - cj)
            d[:, :-1, 1] = torch.where(c, turn(_unit(cj - aj), cj, i, 0), zero)
            d[:, :-1, 2] = torch.where(c, turn(u_cn, ni, i, 1), zero)
            ang[:, :-1, 1] = torch.where(c, turn(_unit(_cross(aj - cj, ni - cj)), cj, i, 0), zero)
            ang[:, :-1, 2] = torch.where(c, turn(_unit(_cross(cj - ni, ai - ni)), ni, i, 1), zero)
            lens[:, :-1, 2] = torch.where(c, dot(u_cn, G[:, 1:, 0]), zero)
    return tuple(out)


def kind_errors(got, want):
    """e (B,) float64 of one output kind: max |got - want| / max |want| per structure; a structure whose ``want`` is
    identically zero has e = 0 where ``got`` is exactly zero and inf otherwise.  NaN in ``got`` counts as inf."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    B = want.shape[0]
    if want.numel() == 0:
        return torch.zeros(B, dtype=torch.float64)
    err = (got - want).abs().reshape(B, -1)
    err = torch.where(err.isnan(), torch.full_like(err, float("inf")), err).amax(-1)
    scale = want.abs().reshape(B, -1).amax(-1)
    exact = (got.reshape(B, -1) == 0).all(-1)
    zero = scale == 0
    e = err / torch.where(zero, torch.ones_like(scale), scale)
    return torch.where(zero, torch.where(exact, torch.zeros_like(e), torch.full_like(e, float("inf"))), e)


def worst_error(got, want):
    """E = the largest e over the three kinds and the structures of a case (``got`` / ``want``: the three gradients)."""
    es = [kind_errors(g, w) for g, w in zip(got, want)]
    return max((float(e.max()) for e in es if e.numel()), default=0.0)


# ---- the accuracy cases of the GPU test (and of tools/nerf_backward_time.py, which reports E per case) ----
LENGTHS = (5, 64, 229, 512, 1024, 1025, 2048)
FAMILIES = ("strand", "helix", "random")


def chains_and_masks(B, N):
    """(chain_idx (B, N) float32, residue_mask (B, N) bool): two chains in even structures and three in odd ones, with
    masked residues at index 0, at the end of the first chain and two adjacent ones inside the second chain."""
    chain = np.zeros((B, N), dtype=np.float32)
    mask = np.ones((B, N), dtype=bool)
    for b in range(B):
        cuts = [N // 2] if b % 2 == 0 else [N // 3, (2 * N) // 3]
        for c in cuts:
            chain[b, c:] += 1
        mask[b, 0] = False
        mask[b, cuts[0] - 1] = False
        mid = cuts[0] + max(2, (N - cuts[0]) // 4)
        mask[b, mid:mid + 2] = False
    return chain, mask


def perturbed_geometry(B, N, seed):
    """float32 (B, N, 3) bond angles within +-0.05 rad and bond lengths within +-0.02 A of the ideal values."""
    rng = np.random.default_rng(seed)
    ang, lens = nerf_ref.default_geometry(B, N)
    ang = (ang + rng.uniform(-0.05, 0.05, size=ang.shape)).astype(np.float32)
    lens = (lens + rng.uniform(-0.02, 0.02, size=lens.shape)).astype(np.float32)
    return ang, lens


def accuracy_cases():
    """dicts name / family / B / N / A / include_cb / perturbed / chains / seed: the three families plain at every length,
    every option alone and all together at N = 64 and 229, chains plus masks (with CB and perturbed geometry) again at
    1025 and 2048."""
    cases = []

    def add(family, N, A=15, include_cb=False, perturbed=False, chains=False, B=2):
        opts = [o for o, on in (("cb", include_cb), ("perturbed", perturbed), ("chains+masks", chains), (f"A={A}", A != 15)) if on]
        cases.append(dict(name=f"{family} N={N}" + (" " + " ".join(opts) if opts else " plain"), family=family, B=B, N=N, A=A,
                          include_cb=include_cb, perturbed=perturbed, chains=chains, seed=7000 + 13 * N + len(cases)))

    for N in LENGTHS:
        for family in FAMILIES:
            add(family, N)
    for N in (64, 229):
        add("helix", N, include_cb=True)
        add("strand", N, perturbed=True)
        add("random", N, chains=True, B=3)
        add("helix", N, A=7)
        add("random", N, A=7, include_cb=True, perturbed=True, chains=True, B=3)
    for N in (1025, 2048):
        add("strand", N, include_cb=True, perturbed=True, chains=True)
    return cases


def make_case(case):
    """The CPU tensors of an accuracy case: dict dihedrals, chain_idx, residue_mask, bond_angles, bond_lengths (None where
    the case leaves them out), grad_xyz (B, N, A, 3) randn, include_cb, n_slots."""
    B, N, A = case["B"], case["N"], case["A"]
    dih = torch.from_numpy(nerf_ref.chain_family(case["family"], B, N, case["seed"]))
    chain = rmask = ang = lens = None
    if case["chains"]:
        chain, rmask = (torch.from_numpy(x) for x in chains_and_masks(B, N))
    if case["perturbed"]:
        ang, lens = (torch.from_numpy(x) for x in perturbed_geometry(B, N, case["seed"] + 1))
    g = torch.Generator().manual_seed(case["seed"] + 2)
    return dict(dihedrals=dih, chain_idx=chain, residue_mask=rmask, bond_angles=ang, bond_lengths=lens,
                grad_xyz=torch.randn(B, N, A, 3, generator=g), include_cb=case["include_cb"], n_slots=A)


def case_gradients(c, dtype):
    return gradient(c["dihedrals"], c["grad_xyz"], c["chain_idx"], c["residue_mask"], c["bond_angles"], c["bond_lengths"],
                    c["include_cb"], dtype=dtype)
