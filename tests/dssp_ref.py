"""The yardstick of the DSSP kernels: float64, dense N x N, plain loops, written from the definition alone (Kabsch &
Sander 1983 with the two-best-partners rule of the DSSP programs; energies not rounded, ladders not joined across
beta-bulges, labels by a pure per-residue priority).  It shares no code with the package.

    hbonds(xyz, complete, junction, donor)  ->  HBonds (the four kept lists, the dense energies, the two margins)
    assign(hbonds, xyz, complete, junction) ->  codes (N,) int8, indices into CODES

plus the helpers the tests build their inputs with: a float64 backbone builder from dihedral angles, a backbone around a
CA trace, an ideal alpha-helix, a two-strand antiparallel hairpin, random 3.8 A walks, and a reader of the HELIX / SHEET
records of a PDB file.
"""
import math
from typing import NamedTuple

import numpy as np

CODES = "-HBEGITS"
Q = 27.888
E_MAX = -0.5
E_FLOOR = -9.9
D_MIN = 0.5
CA_MAX = 9.0


class HBonds(NamedTuple):
    acceptor_idx: np.ndarray       # (N,2) the two best acceptors i of donor j's N-H; -1 where empty
    acceptor_energy: np.ndarray    # (N,2) float64; 0 where empty
    donor_idx: np.ndarray          # (N,2) the two best donors j of acceptor i's C=O
    donor_energy: np.ndarray
    energy: np.ndarray             # (N,N) E[i, j], acceptor i, donor j; NaN where the pair is not evaluated
    energy_margin: float           # the smallest |E + 0.5| over the evaluated pairs (inf if none)
    ca_margin: float               # the smallest | |CA_i - CA_j| - 9 | over the pairs of complete residues (inf if none)


def _dist(a, b):
    x, y, z = float(a[0]) - float(b[0]), float(a[1]) - float(b[1]), float(a[2]) - float(b[2])
    return math.sqrt((x * x + y * y) + z * z)


def hydrogens(xyz, complete, junction, donor=None, n=0, c=2, o=3):
    """(has_h (N,), H (N,3)): residue j has an H iff junction[j-1], complete[j] and donor[j]."""
    N = xyz.shape[0]
    has_h, H = np.zeros(N, dtype=bool), np.zeros((N, 3))
    for j in range(1, N):
        if junction[j - 1] and complete[j] and (donor is None or donor[j]):
            co = xyz[j - 1, c] - xyz[j - 1, o]
            H[j] = xyz[j, n] + co / math.sqrt((co[0] * co[0] + co[1] * co[1]) + co[2] * co[2])
            has_h[j] = True
    return has_h, H


def pair_energy(O, C, Nd, H):
    """E of the acceptor C=O and the donor N-H, kcal/mol."""
    d_on, d_ch, d_oh, d_cn = _dist(O, Nd), _dist(C, H), _dist(O, H), _dist(C, Nd)
    if min(d_on, d_ch, d_oh, d_cn) < D_MIN:
        return E_FLOOR
    return Q * (((1.0 / d_on + 1.0 / d_ch) - 1.0 / d_oh) - 1.0 / d_cn)


def _two_best(column, order):
    """The two lowest energies below E_MAX of ``column`` (NaN = not evaluated); ties to the lower index."""
    kept = sorted((float(column[k]), k) for k in order if not math.isnan(column[k]) and column[k] < E_MAX)[:2]
    idx, en = [-1, -1], [0.0, 0.0]
    for slot, (e, k) in enumerate(kept):
        idx[slot], en[slot] = k, e
    return idx, en


def hbonds(xyz, complete, junction, donor=None, n=0, ca=1, c=2, o=3) -> HBonds:
    xyz = np.asarray(xyz, dtype=np.float64)
    N = xyz.shape[0]
    complete = np.asarray(complete, dtype=bool)
    junction = np.asarray(junction, dtype=bool)
    has_h, H = hydrogens(xyz, complete, junction, donor, n, c, o)
    H, P = H.tolist(), xyz.tolist()           # Python floats are float64: the loops below run on them
    E = np.full((N, N), np.nan)
    energy_margin = ca_margin = math.inf
    for i in range(N):
        if not complete[i]:
            continue
        for j in range(N):
            if not complete[j] or i == j:
                continue
            d_ca = _dist(P[i][ca], P[j][ca])
            ca_margin = min(ca_margin, abs(d_ca - CA_MAX))
            if not has_h[j] or j == i + 1 or not d_ca < CA_MAX:
                continue
            E[i, j] = pair_energy(P[i][o], P[i][c], P[j][n], H[j])
            energy_margin = min(energy_margin, abs(E[i, j] - E_MAX))
    acc_idx, acc_e = np.full((N, 2), -1, dtype=np.int64), np.zeros((N, 2))
    don_idx, don_e = np.full((N, 2), -1, dtype=np.int64), np.zeros((N, 2))
    for r in range(N):
        acc_idx[r], acc_e[r] = _two_best(E[:, r], range(N))
        don_idx[r], don_e[r] = _two_best(E[r, :], range(N))
    return HBonds(acc_idx, acc_e, don_idx, don_e, E, energy_margin, ca_margin)


def assign(hb_lists, xyz, complete, junction, ca=1):
    """(N,) int8 codes into CODES from the kept acceptor lists (``HBonds`` or an (N,2) array)."""
    acc = np.asarray(hb_lists.acceptor_idx if isinstance(hb_lists, HBonds) else hb_lists).tolist()
    xyz = np.asarray(xyz, dtype=np.float64)
    N = xyz.shape[0]
    complete = np.asarray(complete, dtype=bool)
    junction = np.asarray(junction, dtype=bool).tolist()
    if N:
        junction[N - 1] = False

    def hb(i, j):
        return 0 <= i < N and 0 <= j < N and i in acc[j]

    def cont(i, k):
        return i >= 0 and i + k <= N and all(junction[i + t] for t in range(k))

    def bridge(i, j):
        """the set of bridge types of the pair"""
        kinds = set()
        if not (0 <= i < N and 0 <= j < N) or abs(i - j) < 3 or not cont(i - 1, 2) or not cont(j - 1, 2):
            return kinds
        if (hb(i - 1, j) and hb(j, i + 1)) or (hb(j - 1, i) and hb(i, j + 1)):
            kinds.add("P")
        if (hb(i, j) and hb(j, i)) or (hb(i - 1, j + 1) and hb(j - 1, i + 1)):
            kinds.add("A")
        return kinds

    holds = {label: np.zeros(N, dtype=bool) for label in "HBEGITS"}
    for n_turn, label in ((3, "G"), (4, "H"), (5, "I")):
        turn = [cont(i, n_turn) and hb(i, i + n_turn) for i in range(N)]
        for i in range(N):
            if turn[i]:
                holds["T"][i + 1:i + n_turn] = True
            if i >= 1 and turn[i] and turn[i - 1]:
                holds[label][i:i + n_turn] = True
    for i in range(N):
        for j in range(N):
            kinds = bridge(i, j)
            if not kinds:
                continue
            ladder = ("P" in kinds and ("P" in bridge(i - 1, j - 1) or "P" in bridge(i + 1, j + 1))) or \
                     ("A" in kinds and ("A" in bridge(i - 1, j + 1) or "A" in bridge(i + 1, j - 1)))
            holds["E" if ladder else "B"][i] = True
    holds["B"] &= ~holds["E"]
    for i in range(N):
        if cont(i - 2, 4):
            u, v = xyz[i, ca] - xyz[i - 2, ca], xyz[i + 2, ca] - xyz[i, ca]
            cos = float(np.dot(u, v)) / (math.sqrt(float(np.dot(u, u))) * math.sqrt(float(np.dot(v, v))))
            holds["S"][i] = math.degrees(math.acos(max(-1.0, min(1.0, cos)))) > 70.0
    codes = np.zeros(N, dtype=np.int8)
    for label in reversed("HBEGITS"):          # the first that holds wins: write the last first
        codes[holds[label]] = CODES.index(label)
    codes[~complete] = 0
    return codes


def dssp(xyz, complete, junction, donor=None, n=0, ca=1, c=2, o=3):
    """(HBonds, codes) of one structure."""
    bonds = hbonds(xyz, complete, junction, donor, n, ca, c, o)
    return bonds, assign(bonds, xyz, complete, junction, ca)


def reduce_codes(codes):
    """H, G, I -> 1 (H); E, B -> 2 (E); everything else -> 0 (C): indices into "CHE"."""
    table = np.array([0, 1, 2, 2, 1, 1, 0, 0], dtype=np.int8)
    return table[np.asarray(codes)]


def strings(codes, alphabet=CODES):
    return "".join(alphabet[int(k)] for k in codes)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def place(a, b, c, length, angle, torsion):
    """The point X with |X - c| = length, angle(b, c, X) = angle and dihedral(a, b, c, X) = torsion (radians)."""
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    return c + length * (-math.cos(angle) * bc + math.sin(angle) * math.cos(torsion) * m + math.sin(angle) * math.sin(torsion) * nrm)


def backbone_from_dihedrals(phi, psi, omega=None):
    """(N,4,3) float64 N, CA, C, O of a chain with ideal bond lengths and angles and the given dihedrals in degrees
    (phi[0] and psi[-1] only place the ends' O)."""
    L = len(phi)
    omega = [180.0] * L if omega is None else omega
    r = math.radians
    out = np.zeros((L, 4, 3))
    out[0, 0] = (1.458 * math.cos(r(111.0)), 1.458 * math.sin(r(111.0)), 0.0)
    out[0, 1] = (0.0, 0.0, 0.0)
    out[0, 2] = (1.525, 0.0, 0.0)
    for k in range(L):
        if k > 0:
            out[k, 0] = place(out[k - 1, 0], out[k - 1, 1], out[k - 1, 2], 1.329, r(116.2), r(psi[k - 1]))
            out[k, 1] = place(out[k - 1, 1], out[k - 1, 2], out[k, 0], 1.458, r(121.7), r(omega[k - 1]))
            out[k, 2] = place(out[k - 1, 2], out[k, 0], out[k, 1], 1.525, r(111.0), r(phi[k]))
        out[k, 3] = place(out[k, 0], out[k, 1], out[k, 2], 1.231, r(120.5), r(psi[k] + 180.0))
    return out


def ideal_helix(L):
    return backbone_from_dihedrals([-57.0] * L, [-47.0] * L)


def pi_helix(L):
    return backbone_from_dihedrals([-57.0] * L, [-70.0] * L)


def helix_310(L):
    return backbone_from_dihedrals([-49.0] * L, [-26.0] * L)


def hairpin(L):
    """(2L,4,3): an extended strand and its copy turned by 180 degrees about an axis normal to the sheet, 4.8 A away --
    an antiparallel pair; residue L - 1 - k faces residue L + k.  There is no loop: L - 1 -> L is no peptide bond."""
    strand = backbone_from_dihedrals([-139.0] * L, [135.0] * L)
    axis = strand[-1, 1] - strand[0, 1]
    axis /= np.linalg.norm(axis)
    mid = L // 2
    side = strand[mid, 3] - strand[mid, 2]
    side -= np.dot(side, axis) * axis
    side /= np.linalg.norm(side)
    normal = np.cross(axis, side)
    centre = 0.5 * (strand[mid, 2] + strand[mid, 0]) + 2.4 * side   # between the C=O and the N-H that point this way
    turn = 2.0 * np.outer(normal, normal) - np.eye(3)
    other = centre + (strand - centre) @ turn.T
    return np.concatenate([strand, other], axis=0)


def random_walk(L, rng, step=3.8):
    """(L,3) a CA trace with ``step`` between neighbours and no sharp reversal"""
    ca = np.zeros((L, 3))
    direction = np.array([1.0, 0.0, 0.0])
    for k in range(1, L):
        while True:
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            if np.dot(d, direction) > -0.3:
                break
        direction = d
        ca[k] = ca[k - 1] + step * d
    return ca


def backbone_on_trace(ca):
    """(L,4,3) N, CA, C, O around a CA trace: a planar trans peptide between neighbours (C at 1.52 A of its CA, N at 1.47 A
    of the next, C-N 1.33 A, C=O 1.23 A), the plane turned about the CA-CA axis by the trace's own curvature; the ends'
    missing neighbours are mirrored."""
    L = ca.shape[0]
    out = np.zeros((L, 4, 3))
    out[:, 1] = ca
    ext = np.concatenate([[2 * ca[0] - ca[min(1, L - 1)] + [0.0, 0.1, 0.0]], ca, [2 * ca[-1] - ca[max(L - 2, 0)] + [0.0, 0.0, 0.1]]])
    if L == 1:
        ext[0], ext[2] = ca[0] - [3.8, 0.0, 0.0], ca[0] + [3.8, 0.0, 0.0]
    for k in range(L + 1):                       # the peptide between ext[k] and ext[k + 1]
        a, b = ext[k], ext[k + 1]
        u = (b - a) / np.linalg.norm(b - a)
        ref = ext[k + 2] - b if k + 2 < L + 2 else a - ext[k - 1]
        p = np.cross(u, ref)
        if np.linalg.norm(p) < 1e-6:
            p = np.cross(u, [0.0, 0.0, 1.0]) if abs(u[2]) < 0.9 else np.cross(u, [0.0, 1.0, 0.0])
        p /= np.linalg.norm(p)
        scale = np.linalg.norm(b - a) / 3.8
        if k >= 1:                               # C and O belong to residue k - 1
            out[k - 1, 2] = a + scale * (1.46 * u + 0.42 * p)
            out[k - 1, 3] = a + scale * (1.70 * u + 1.62 * p)
        if k < L:                                # N belongs to residue k
            out[k, 0] = a + scale * (2.42 * u - 0.50 * p)
    return out


def chain_junctions(complete, breaks=()):
    """(N,) bool: r -> r+1 is a peptide bond where both residues are complete and r is no break."""
    complete = np.asarray(complete, dtype=bool)
    N = complete.shape[0]
    j = np.zeros(N, dtype=bool)
    if N > 1:
        j[:-1] = complete[:-1] & complete[1:]
    for r in breaks:
        j[r] = False
    return j


# ---- the records of a PDB file -------------------------------------------------------------------------------------------
def pdb_records(path):
    """([(class, chain, first, last)] of the HELIX records, [(chain, first, last)] of the SHEET records), by residue
    number."""
    helices, strands = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("HELIX "):
                helices.append((int(line[38:40]), line[19], int(line[21:25]), int(line[33:37])))
            elif line.startswith("SHEET "):
                strands.append((line[21], int(line[22:26]), int(line[33:37])))
    return helices, strands



def structure_inputs(atom_mask, chain_idx, seq=None):
    """(complete, junction, donor) of one structure from its (N,A) atom mask (N, CA, C, O in slots 0-3), its (N,) chain
    index (NaN in the padding) and, where known, its one-letter sequence (padding beyond its length donates)."""
    atom_mask = np.asarray(atom_mask, dtype=bool)
    chain_idx = np.asarray(chain_idx, dtype=np.float64)
    N = atom_mask.shape[0]
    complete = atom_mask[:, :4].all(-1)
    junction = np.zeros(N, dtype=bool)
    for r in range(N - 1):
        junction[r] = complete[r] and complete[r + 1] and chain_idx[r] == chain_idx[r + 1]
    donor = None
    if seq is not None:
        donor = np.array([k >= len(seq) or seq[k] != "P" for k in range(N)])
    return complete, junction, donor


class Case(NamedTuple):
    xyz: np.ndarray         # (B,N,A,3) float32, NaN at incomplete residues
    complete: np.ndarray    # (B,N) bool
    junction: np.ndarray    # (B,N) bool
    donor: object           # (B,N) bool or None
    slots: tuple            # (n, ca, c, o)


def synthetic_case(N, seed, B=3, masked=0.1, helix_break=False, with_donor=False, A=4, slots=(0, 1, 2, 3)) -> Case:
    """B structures of N residues: structure 1 is all padding; the others are an ideal alpha-helix of 14, a hairpin of
    2 x 7 and a 3.8 A random walk with the backbone placed around it (``backbone_on_trace``) -- the last structure also a
    pi-helix of 9 and a 3-10 helix of 8 -- in two different orders, cut to N; the pieces are separate chains.  A fraction ``masked`` of the residues is incomplete (NaN coordinates);
    ``helix_break`` cuts the peptide bond in the middle of the helix; ``with_donor`` takes the amide hydrogen from a sixth
    of the residues.  Coordinates are float32 values."""
    rng = np.random.default_rng(seed)
    xyz = np.full((B, N, A, 3), np.nan, dtype=np.float32)
    complete = np.zeros((B, N), dtype=bool)
    junction = np.zeros((B, N), dtype=bool)
    for b in range(B):
        if b == 1:
            continue
        walk = backbone_on_trace(random_walk(max(N, 1), rng))
        helix = ideal_helix(14) + rng.normal(size=3) * 4.0
        pin = hairpin(7) + rng.normal(size=3) * 4.0 + [0.0, 0.0, 12.0]
        third = max(N // 3, 1)
        pieces = [helix, pin, walk] if b == 0 else [walk[:third], pin, pi_helix(9) - [0.0, 15.0, 0.0], helix_310(8) - [15.0, 0.0, 0.0],
                                                    helix, walk[third:] + [6.0, 0.0, 0.0]]
        breaks, start, helix_at = [], 0, 0
        for piece in pieces:
            if piece is helix:
                helix_at = start
            if piece is pin:
                breaks.append(start + 6)
            start += len(piece)
            breaks.append(start - 1)
        if helix_break:
            breaks.append(helix_at + 6)
        atoms = np.concatenate(pieces)[:N].astype(np.float32)
        ok = rng.random(N) >= masked
        complete[b] = ok
        for k, s in enumerate(slots):
            xyz[b, :, s] = np.where(ok[:, None], atoms[:, k], np.nan)
        junction[b] = chain_junctions(ok, [r for r in breaks if r < N])
    donor = rng.random((B, N)) >= 1.0 / 6.0 if with_donor else None
    return Case(xyz, complete, junction, donor, tuple(slots))


def case_reference(case: Case):
    """[(HBonds, codes)] per structure of a case, in float64 on the case's float32 values."""
    n, ca, c, o = case.slots
    return [dssp(case.xyz[b], case.complete[b], case.junction[b], None if case.donor is None else case.donor[b], n, ca, c, o)
            for b in range(case.xyz.shape[0])]
