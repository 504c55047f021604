"""Atom-slot vocabulary of the geometry hot path.

Only the data the hot path needs is restated here, as a table: the five backbone atom slots with the spellings the
reference accepts for each (reference protstruc/general.py:4-20) and the 15-slot residue width
(protstruc/constants/__init__.py:1).
"""
import enum

MAX_N_ATOMS_PER_RESIDUE = 15

# slot -> (canonical name, accepted alternative spellings); the slot is the index on a residue's atom axis
_BACKBONE = (
    ("N", ("n",)),
    ("CA", ("Ca", "ca")),
    ("C", ("c",)),
    ("O", ("o",)),
    ("CB", ("Cb", "cb")),
)


class _AtomSlot(enum.IntEnum):
    """Behaviour of the enumeration below (an IntEnum without members can be extended through the functional API)."""

    @classmethod
    def is_valid(cls, name):
        # as in the reference, validity is judged on the upper-cased spelling against the canonical names only
        return name.upper() in cls._member_names_

    def __str__(self):
        return self.name


# ATOM["ca"], ATOM["Ca"] and ATOM["CA"] all resolve to slot 1 (later spellings of a slot become aliases of the
# canonical member); an unknown name raises KeyError; int(ATOM.CB) == 4.
ATOM = _AtomSlot("ATOM", [(spelling, slot) for slot, (canonical, others) in enumerate(_BACKBONE)
                          for spelling in (canonical,) + others])


def vdw_radius_table():
    """Van der Waals radius of every atom slot of every residue type: a (21, 15) float32 tensor indexed by
    [``pdb.ONE_TO_INDEX`` code][slot], from ``pdb.ATOM_SLOT`` with the element taken as the first letter of the atom name
    (``ops.VDW_RADII``), OXT in slot 14, and 0 where a type has no such atom (glycine's CB, the slots past a side chain's
    end).  The unknown type X has N, CA, C, O, CB and OXT only."""
    import torch

    from .ops import VDW_RADII
    from .pdb import ATOM_SLOT, ONE_TO_INDEX, THREE_TO_ONE

    table = torch.zeros(len(ONE_TO_INDEX), MAX_N_ATOMS_PER_RESIDUE, dtype=torch.float32)
    for three, one in THREE_TO_ONE.items():
        slots = ATOM_SLOT.get(three)
        if slots is None:   # X: the slots every residue type with a side chain shares
            slots = {name: k for k, (name, _) in enumerate(_BACKBONE)}
            slots["OXT"] = MAX_N_ATOMS_PER_RESIDUE - 1
        for name, slot in slots.items():
            table[ONE_TO_INDEX[one], slot] = VDW_RADII[name[0]]
    return table


# theoretical maximum solvent accessibility of a residue X in Gly-X-Gly, A^2 (Tien et al. 2013, PLoS ONE 8(11): e80635)
_MAX_ACCESSIBILITY = dict(A=129.0, R=274.0, N=195.0, D=193.0, C=167.0, E=223.0, Q=225.0, G=104.0, H=224.0, I=197.0,
                          L=201.0, K=236.0, M=224.0, F=240.0, P=159.0, S=155.0, T=172.0, W=285.0, Y=263.0, V=174.0)


def max_accessibility_table():
    """Theoretical maximum solvent-accessible surface area of every residue type (Tien et al. 2013), A^2: a (21,) float32
    tensor indexed by ``pdb.ONE_TO_INDEX``; NaN for the unknown type X.  What relative accessibility divides by."""
    import torch

    from .pdb import ONE_TO_INDEX

    table = torch.full((len(ONE_TO_INDEX),), float("nan"), dtype=torch.float32)
    for one, value in _MAX_ACCESSIBILITY.items():
        table[ONE_TO_INDEX[one]] = value
    return table


# the atoms after CB along which chi1 .. chi4 are defined: chi1 = N CA CB X, chi2 = CA CB X Y, chi3 = CB X Y Z, chi4 = X Y Z W
# (IUPAC-IUB 1970; the table of AlphaFold 2's torsion-angle loss).  ALA, GLY and the unknown type X have none.
_CHI_CHAIN = {
    "ARG": "CG CD NE CZ", "LYS": "CG CD CE NZ", "MET": "CG SD CE", "GLN": "CG CD OE1", "GLU": "CG CD OE1",
    "ASN": "CG OD1", "ASP": "CG OD1", "HIS": "CG ND1", "LEU": "CG CD1", "PHE": "CG CD1", "TRP": "CG CD1", "TYR": "CG CD1",
    "ILE": "CG1 CD1", "PRO": "CG CD", "CYS": "SG", "SER": "OG", "THR": "OG1", "VAL": "CG1",
}
# (residue, angle): chi and chi + pi name the same structure (the two atoms the angle ends in are equivalent)
_CHI_PI_PERIODIC = (("ASP", 1), ("GLU", 2), ("PHE", 1), ("TYR", 1))


def chi_atom_table():
    """The four atoms of every side-chain torsion: a (21, 4, 4) int32 tensor indexed [``pdb.ONE_TO_INDEX`` code][chi][a, b,
    c, d], atom slots from ``pdb.ATOM_SLOT``, -1 where a residue type has no such angle.  chi1 is N CA CB X, chi2 CA CB X
    Y, chi3 CB X Y Z and chi4 X Y Z W along the type's chain of atoms after CB (CG CD NE CZ for ARG, ..., SG for CYS)."""
    import torch

    from .pdb import ATOM_SLOT, ONE_TO_INDEX, THREE_TO_ONE

    table = torch.full((len(ONE_TO_INDEX), 4, 4), -1, dtype=torch.int32)
    for three, chain in _CHI_CHAIN.items():
        names = ["N", "CA", "CB"] + chain.split()
        for k in range(len(names) - 3):
            table[ONE_TO_INDEX[THREE_TO_ONE[three]], k] = torch.tensor([ATOM_SLOT[three][a] for a in names[k:k + 4]],
                                                                       dtype=torch.int32)
    return table


def chi_last_table():
    """The last atom slot every side-chain torsion moves: a (21, 4) int32 tensor.  Turning chi k moves the slots from its
    fourth atom through the last side-chain slot of the type, both inclusive (ILE's chi2 moves CD1 alone), never OXT in
    slot 14.  -1 where there is no angle, and for both angles of proline: they can be measured, but turning them would
    open the ring."""
    import torch

    from .pdb import ATOM_SLOT, ONE_TO_INDEX, THREE_TO_ONE

    atoms = chi_atom_table()
    table = torch.full((len(ONE_TO_INDEX), 4), -1, dtype=torch.int32)
    for three in _CHI_CHAIN:
        if three == "PRO":
            continue
        row = ONE_TO_INDEX[THREE_TO_ONE[three]]
        side_chain_end = max(slot for name, slot in ATOM_SLOT[three].items() if name != "OXT")
        table[row] = torch.where(atoms[row, :, 3] >= 0, torch.tensor(side_chain_end, dtype=torch.int32), table[row])
    return table


def chi_pi_periodic_table():
    """(21, 4) bool: chi and chi + pi name the same structure -- ASP chi2, GLU chi3, PHE chi2 and TYR chi2."""
    import torch

    from .pdb import ONE_TO_INDEX, THREE_TO_ONE

    table = torch.zeros(len(ONE_TO_INDEX), 4, dtype=torch.bool)
    for three, k in _CHI_PI_PERIODIC:
        table[ONE_TO_INDEX[THREE_TO_ONE[three]], k] = True
    return table
