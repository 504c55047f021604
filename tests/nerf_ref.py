"""Float64 host restatement of the backbone builder behind StructureBatch.from_backbone_dihedrals, for the tests.

``place_fourth_atom`` is the reference's geometry.place_fourth_atom (geometry.py:127-168) in numpy; ``build`` is the
NeRF recurrence it implies, one atom after another, with the segment rules of include/protstruc_hip.h (K7).  In float64
the sequential walk is exact to ~1e-9 A at the sizes tested, so it is the yardstick for the float32 kernel: both are
fed the same float32 inputs (defaults included, rounded to float32 as the kernel rounds them).
"""
import math

import numpy as np

# geometry.IDEAL_NA / IDEAL_AC / IDEAL_C_N, IDEAL_NAC / IDEAL_CACN / IDEAL_CNCA
IDEAL_LENGTHS = (1.458, 1.523, 1.329)
IDEAL_ANGLES = (1.937, math.radians(116.2), math.radians(121.7))
CB_COEF = (-0.58273431, 0.56802827, -0.54067466)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def place_fourth_atom(a, b, c, length, planar, dihedral):
    """X with |X - c| = length, angle(X, c, b) = planar, dihedral(a, b, c, X) = dihedral (reference formula)."""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    length, planar, dihedral = (np.asarray(x, dtype=np.float64) for x in (length, planar, dihedral))
    bc = _unit(b - c)
    n = _unit(np.cross(b - a, bc))
    d = [bc, np.cross(n, bc), n]
    m = [length * np.cos(planar), length * np.sin(planar) * np.cos(dihedral), -length * np.sin(planar) * np.sin(dihedral)]
    return c + sum(mi * di for mi, di in zip(m, d))


def dihedral(a, b, c, d):
    """Signed dihedral of a-b-c-d in (-pi, pi] (the convention of geometry.dihedral and K2)."""
    b0, b1, b2 = a - b, c - b, d - c
    n1, n2 = np.cross(b0, b1), np.cross(b2, b1)
    x = (n1 * n2).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):   # zero rows of masked residues
        y = (np.cross(n1, n2) * b1).sum(-1) / np.linalg.norm(b1, axis=-1)
    return np.arctan2(y, x)


def angle(a, b, c):
    ba, bc = a - b, c - b
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (ba * bc).sum(-1) / (np.linalg.norm(ba, axis=-1) * np.linalg.norm(bc, axis=-1))
    return np.arccos(np.clip(cos, -1.0, 1.0))


def angle_diff(x, y):
    """|x - y| modulo 2 pi."""
    d = np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def default_geometry(B, N):
    """(bond_angles, bond_lengths) of the ideal geometry as float32 (B, N, 3) arrays."""
    ang = np.broadcast_to(np.array(IDEAL_ANGLES, dtype=np.float32), (B, N, 3)).copy()
    lens = np.broadcast_to(np.array(IDEAL_LENGTHS, dtype=np.float32), (B, N, 3)).copy()
    return ang, lens


def segment_starts(B, N, chain_idx=None, residue_mask=None):
    """(B, N) bool: residue i starts a segment (i = 0, chain change with NaN != NaN, or residue i-1 masked)."""
    start = np.zeros((B, N), dtype=bool)
    if N:
        start[:, 0] = True
    if chain_idx is not None:
        ch = np.asarray(chain_idx, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            start[:, 1:] |= ch[:, 1:] != ch[:, :-1]
    if residue_mask is not None:
        start[:, 1:] |= ~np.asarray(residue_mask, dtype=bool)[:, :-1]
    return start


def used_angles(B, N, chain_idx=None, residue_mask=None):
    """(B, N, 3) bool: the angles that shape visible atoms -- phi_i of an unmasked non-start residue, psi_i / omega_i
    when residue i+1 continues the segment and is unmasked."""
    start = segment_starts(B, N, chain_idx, residue_mask)
    live = np.ones((B, N), dtype=bool) if residue_mask is None else np.asarray(residue_mask, dtype=bool)
    used = np.zeros((B, N, 3), dtype=bool)
    used[:, :, 0] = ~start & live
    nxt = np.zeros((B, N), dtype=bool)
    nxt[:, :-1] = ~start[:, 1:] & live[:, 1:]
    used[:, :, 1] = nxt
    used[:, :, 2] = nxt
    return used


def unused_angles(B, N, chain_idx=None, residue_mask=None):
    """(B, N, 3) bool: phi at a segment's first residue, psi / omega at its last -- never read by the builder."""
    start = segment_starts(B, N, chain_idx, residue_mask)
    last = np.ones((B, N), dtype=bool)
    last[:, :-1] = start[:, 1:]
    return np.stack([start, last, last], axis=-1)


def build(dihedrals, chain_idx=None, residue_mask=None, bond_angles=None, bond_lengths=None, include_cb=False, n_slots=15):
    """(xyz (B, N, n_slots, 3) float64, atom_mask (B, N, n_slots) float64) by the sequential float64 walk."""
    dih = np.asarray(dihedrals, dtype=np.float32).astype(np.float64)
    B, N = dih.shape[:2]
    ang, lens = default_geometry(B, N)
    if bond_angles is not None:
        ang = np.asarray(bond_angles, dtype=np.float32)
    if bond_lengths is not None:
        lens = np.asarray(bond_lengths, dtype=np.float32)
    ang, lens = ang.astype(np.float64), lens.astype(np.float64)
    start = segment_starts(B, N, chain_idx, residue_mask)
    live = np.ones((B, N), dtype=bool) if residue_mask is None else np.asarray(residue_mask, dtype=bool)
    xyz = np.zeros((B, N, n_slots, 3))
    mask = np.zeros((B, N, n_slots))
    for b in range(B):
        n = ca = c = None
        for i in range(N):
            if start[b, i]:
                na, nac = lens[b, i, 0], ang[b, i, 0]
                n = np.array([na * math.cos(nac), na * math.sin(nac), 0.0])
                ca = np.zeros(3)
                c = np.array([lens[b, i, 1], 0.0, 0.0])
            else:
                n1 = place_fourth_atom(n, ca, c, lens[b, i - 1, 2], ang[b, i - 1, 1], dih[b, i - 1, 1])
                ca1 = place_fourth_atom(ca, c, n1, lens[b, i, 0], ang[b, i - 1, 2], dih[b, i - 1, 2])
                c1 = place_fourth_atom(c, n1, ca1, lens[b, i, 1], ang[b, i, 0], dih[b, i, 0])
                n, ca, c = n1, ca1, c1
            if not live[b, i]:
                continue
            xyz[b, i, 0], xyz[b, i, 1], xyz[b, i, 2] = n, ca, c
            mask[b, i, :3] = 1.0
            if include_cb:
                bb, cc = ca - n, c - ca
                aa = np.cross(bb, cc)
                xyz[b, i, 4] = CB_COEF[0] * aa + CB_COEF[1] * bb + CB_COEF[2] * cc + ca
                mask[b, i, 4] = 1.0
    return xyz, mask


def chain_family(kind, B, N, seed):
    """float32 (B, N, 3) [phi, psi, omega]: 'strand' (-2.1, 2.3, pi), 'helix' (-1.0, -0.82, pi), each +-0.1 uniform
    noise, or 'random' (uniform phi / psi, omega = pi +- 0.1)."""
    rng = np.random.default_rng(seed)
    noise = rng.uniform(-0.1, 0.1, size=(B, N, 3))
    if kind == "strand":
        d = np.array([-2.1, 2.3, np.pi]) + noise
    elif kind == "helix":
        d = np.array([-1.0, -0.82, np.pi]) + noise
    elif kind == "random":
        d = np.concatenate([rng.uniform(-np.pi, np.pi, size=(B, N, 2)), np.pi + noise[..., 2:]], axis=-1)
    else:
        raise ValueError(kind)
    d = (d + np.pi) % (2 * np.pi) - np.pi
    return d.astype(np.float32)
