"""`StructureBatch` -- the reference's batch API, with the geometry on MI355X.

Drop-in for the geometric-feature hot path of ``protstruc.StructureBatch``
(reference protstruc/protstruc.py:32-956): same constructor, method names,
argument meaning, return arity / shape / dtype and exception types; the
arithmetic of every featuriser runs in the hand-written HIP kernels of
``libprotstruc_hip.so`` (see include/protstruc_hip.h).  There is no CPU path:
a batch that lives on the CPU can be constructed and inspected, but calling a
featuriser on it raises.

Deliberate, documented differences from the reference (SURVEY.md quirk list):

* device: every derived tensor lives on ``xyz``'s device (the reference
  hard-codes CPU, protstruc.py:71-73,84); CPU / numpy inputs are moved to the
  current GPU when one is present (``device=`` overrides).
* Q1 ``standardize`` uses per-structure statistics for any batch size (the
  reference only runs for B == 1).  Q3/Q4: its mask arguments work.
* Q2 ``pairwise_distance_matrix`` without an ``atom_mask`` returns an all-True
  mask instead of raising ``TypeError``.
* Q6 the third frame axis is the last-axis cross product for every shape.
* Q8 ``diffuse_xyz`` / ``standardize`` / ``unstandardize`` update the coordinate
  buffer in place (hipGraph-friendly); earlier ``get_xyz()`` results alias it.
* coordinates are held as contiguous float32 (float64 input is down-cast).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from . import ops
from .general import ATOM


def _always_tensor(x):
    return torch.from_numpy(x) if isinstance(x, np.ndarray) else x


class EdgeFeatures(NamedTuple):
    """The edge features of a neighbour graph (``StructureBatch.edge_features``)."""
    idx: torch.Tensor                   # (B,N,k) int32: the graph; -1 at the padding
    mask: torch.Tensor                  # (B,N,k) bool: idx >= 0
    rbf: torch.Tensor                   # (B,N,k,P*n_rbf) fp32: radial basis functions of the atom-pair distances
    offset: torch.Tensor                # (B,N,k) int64: the class of the sequence offset
    local_pos: Optional[torch.Tensor]   # (B,N,k,3) fp32: the neighbour's CA in the source residue's frame, or None
    rel_rot: Optional[torch.Tensor]     # (B,N,k,3,3) fp32: the neighbour's frame in the source residue's frame, or None


class RadiusEdgeFeatures(NamedTuple):
    """The edge features of a radius graph (``StructureBatch.edge_features(graph=radius_graph(...))``), flat over the E
    entries of the graph's ``col``."""
    batch: torch.Tensor                 # (E,) int32: the structure of every edge; -1 past the last edge
    row: torch.Tensor                   # (E,) int32: its source residue; -1 past the last edge
    col: torch.Tensor                   # (E,) int32: its neighbour, an index into the N axis of structure ``batch``
    mask: torch.Tensor                  # (E,) bool: batch >= 0
    rbf: torch.Tensor                   # (E,P*n_rbf) fp32: radial basis functions of the atom-pair distances
    offset: torch.Tensor                # (E,) int64: the class of the sequence offset
    local_pos: Optional[torch.Tensor]   # (E,3) fp32: the neighbour's CA in the source residue's frame, or None
    rel_rot: Optional[torch.Tensor]     # (E,3,3) fp32: the neighbour's frame in the source residue's frame, or None


class AtomEdgeFeatures(NamedTuple):
    """The edge features of an atom radius graph (``StructureBatch.atom_edge_features``), flat over the E entries of ``col``."""
    batch: torch.Tensor   # (E,) int32: the structure of every edge; -1 past the last edge
    atom: torch.Tensor    # (E,) int32: its source atom, an index into the flattened N*A atom axis; -1 past the last edge
    col: torch.Tensor     # (E,) int32: its neighbour, likewise
    mask: torch.Tensor    # (E,) bool: batch >= 0
    rbf: torch.Tensor     # (E,n_rbf) fp32: radial basis functions of the distance


class StructuralAlignment(NamedTuple):
    """``geometry.StructureAlignment`` with the sequence identity of the aligned pairs (``StructureBatch.structural_alignment``)."""
    map: torch.Tensor            # (B,N) int32: the residue of the target aligned to a residue of this batch, or -1
    n_aligned: torch.Tensor      # (B,) int32
    tm_a: torch.Tensor           # (B,) fp32: TM-score normalised by this batch's length
    tm_b: torch.Tensor           # (B,) fp32: ... by the target's
    rmsd: torch.Tensor           # (B,) fp32
    rot: torch.Tensor            # (B,3,3) fp32: the transform of tm_b
    trans: torch.Tensor          # (B,3) fp32
    search_score: torch.Tensor   # (B,) fp32
    start: torch.Tensor          # (B,) int32
    identity: torch.Tensor       # (B,) fp32: the fraction of aligned pairs with the same residue type


def _default_device() -> torch.device:
    if torch.cuda.is_available():
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


def valid_junctions(present: torch.Tensor, chain_idx: torch.Tensor, residue_idx: Optional[torch.Tensor] = None,
                    n_slot: int = 0, ca_slot: int = 1, c_slot: int = 2) -> torch.Tensor:
    """(B,N) bool, entry r = the junction from residue r to residue r+1 is a peptide bond: C and CA of r and N and CA of
    r+1 are ``present`` (B,N,A; a residue outside the residue mask has no atom present), both residues carry the same
    ``chain_idx`` (NaN, the padding, equals nothing) and, where ``residue_idx`` (B,N) is given, r+1 follows r.  Entry N-1
    is False.  Plain tensor arithmetic on the inputs' device."""
    B, N = present.shape[:2]
    ok = torch.zeros(B, N, dtype=torch.bool, device=present.device)
    if N < 2:
        return ok
    here = present[:, :-1, c_slot] & present[:, :-1, ca_slot]
    there = present[:, 1:, n_slot] & present[:, 1:, ca_slot]
    ok[:, :-1] = here & there & (chain_idx[:, :-1] == chain_idx[:, 1:])
    if residue_idx is not None:
        ok[:, :-1] &= (residue_idx[:, 1:] - residue_idx[:, :-1]) == 1
    return ok


def clash_links(junctions: torch.Tensor, A: int, is_cys: Optional[torch.Tensor] = None, n_slot: int = 0, c_slot: int = 2,
                sg_slot: int = 5) -> torch.Tensor:
    """(B, N*A) int32 ``link`` of ``geometry.steric_clash`` for all atom slots: C of residue r and N of residue r+1 share
    the id r at every valid junction (the peptide bond is no clash), every SG of a cysteine (``is_cys`` (B,N) bool)
    carries the id N (nor is a disulphide bridge), every other atom -1."""
    B, N = junctions.shape
    link = torch.full((B, N, A), -1, dtype=torch.int32, device=junctions.device)
    ids = torch.arange(N, dtype=torch.int32, device=junctions.device).expand(B, N)
    none = torch.full_like(ids, -1)
    link[:, :, c_slot] = torch.where(junctions, ids, none)
    if N > 1:
        link[:, 1:, n_slot] = torch.where(junctions[:, :-1], ids[:, :-1], none[:, :-1])
    if is_cys is not None and sg_slot < A:
        link[:, :, sg_slot] = torch.where(is_cys, torch.full_like(ids, N), none)
    return link.reshape(B, N * A)


class StructureBatch:
    """A padded batch of protein structures: ``xyz (B, N_res, N_atom, 3)`` + masks."""

    def __init__(
        self,
        xyz: torch.Tensor,
        atom_mask: torch.BoolTensor = None,
        chain_idx: torch.Tensor = None,
        chain_ids: List[str] = None,
        seq: List[Dict[str, str]] = None,
        residue_idx: torch.LongTensor = None,
        device: Union[str, torch.device, None] = None,
    ):
        # reference protstruc.py:55-60
        if (chain_idx is not None and chain_ids is None) or (chain_idx is None and chain_ids is not None):
            raise ValueError("Both `chain_idx` and `chain_ids` should be provided or None.")

        xyz = _always_tensor(xyz)
        atom_mask = _always_tensor(atom_mask)
        chain_idx = _always_tensor(chain_idx)
        if xyz.ndim != 4 or xyz.shape[-1] != 3:
            raise ValueError(f"xyz must have shape (batch, residues, atoms, 3), got {tuple(xyz.shape)}")

        if device is None:
            device = xyz.device if xyz.is_cuda else _default_device()
        self.device = torch.device(device)

        if chain_idx is not None:
            # reference protstruc.py:75-80 -- checked on the host copy, before anything is launched
            for i, chidx in enumerate(chain_idx):
                valid = chidx[~torch.isnan(chidx)]
                assert valid.numel() > 0 and valid.min() == 0, f"Protein {i}: Chain index should start from zero"

        self.xyz = xyz.to(device=self.device, dtype=torch.float32).contiguous()
        self.atom_mask = None if atom_mask is None else atom_mask.to(self.device)
        self.batch_size, self.n_residues, self.max_n_atoms_per_residue = self.xyz.shape[:3]

        if self.atom_mask is not None:
            self.residue_mask = self.atom_mask.any(dim=-1)
        else:
            self.residue_mask = torch.ones(self.batch_size, self.n_residues, dtype=torch.bool, device=self.device)

        if chain_idx is not None:
            self.chain_idx = chain_idx.to(self.device)
        else:
            self.chain_idx = torch.zeros(self.batch_size, self.n_residues, device=self.device)

        self.chain_ids = chain_ids
        self.seq = seq
        self.residue_idx = residue_idx
        self._standardized = False
        self._rng_state = None  # device int64 [seed, offset] of the diffusion sampler

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_xyz(
        cls,
        xyz: Union[np.ndarray, torch.Tensor],
        atom_mask: Union[np.ndarray, torch.Tensor] = None,
        chain_idx: Union[np.ndarray, torch.Tensor] = None,
        chain_ids: List[List[str]] = None,
        seq: List[Dict[str, str]] = None,
        **kwargs,
    ) -> "StructureBatch":
        """Reference protstruc.py:94-128."""
        return cls(xyz, atom_mask, chain_idx, chain_ids, seq, **kwargs)

    @classmethod
    def from_pdb(cls, pdb_path: Union[str, List[str]], **kwargs) -> "StructureBatch":
        """Initialize from one PDB file or a list of them (reference protstruc.py:131-193).

        Parsing is host-side plumbing (``protstruc_amd/pdb.py``); the padded batch is then moved to the GPU."""
        from . import pdb as _pdb

        paths = pdb_path if isinstance(pdb_path, list) else [pdb_path]
        xyz, mask, chain_idx, chain_ids, seq, residue_idx = _pdb.read_batch(paths)
        return cls(xyz, mask, chain_idx, chain_ids, seq, residue_idx, **kwargs)

    @classmethod
    def from_backbone_orientations_translations(
        cls,
        orientations: Union[np.ndarray, torch.Tensor],
        translations: Union[np.ndarray, torch.Tensor],
        chain_idx: Union[np.ndarray, torch.Tensor] = None,
        chain_ids: List[List[str]] = None,
        seq: List[Dict[str, str]] = None,
        residue_idx: Union[np.ndarray, torch.Tensor] = None,
        include_cb: bool = False,
        **kwargs,
    ) -> "StructureBatch":
        """Ideal backbone (N, CA, C[, CB]) placed by per-residue frames (reference protstruc.py:264-319).
        The atom mask is float32 ones / zeros, as in the reference."""
        from .general import MAX_N_ATOMS_PER_RESIDUE
        from .geometry import ideal_backbone_coordinates

        orientations, translations = _always_tensor(orientations), _always_tensor(translations)
        dev = kwargs.get("device") or (orientations.device if orientations.is_cuda else _default_device())
        ideal = ideal_backbone_coordinates((), include_cb)  # (3 or 4, 3)
        n_atoms = ideal.shape[0]
        xyz = ops.frames_to_backbone(orientations.to(dev), translations.to(dev), ideal, MAX_N_ATOMS_PER_RESIDUE)
        B, N = xyz.shape[:2]
        atom_mask = torch.zeros(B, N, MAX_N_ATOMS_PER_RESIDUE, device=xyz.device)
        atom_mask[:, :, :n_atoms] = 1.0
        return cls(xyz, atom_mask, chain_idx, chain_ids, seq, residue_idx, **kwargs)

    @classmethod
    def from_pdb_id(cls, pdb_id, **kwargs) -> "StructureBatch":
        """The reference downloads entries from RCSB through biotite (protstruc.py:195-261).  Network access and
        biotite are outside this build's scope: download the files yourself and use :meth:`from_pdb`."""
        raise NotImplementedError("from_pdb_id needs network access and biotite; fetch the PDB file(s) and call "
                                  "StructureBatch.from_pdb(path) instead")

    @classmethod
    def from_backbone_dihedrals(
        cls,
        dihedrals: Union[np.ndarray, torch.Tensor],
        chain_idx: Union[np.ndarray, torch.Tensor] = None,
        chain_ids: List[List[str]] = None,
        seq: List[Dict[str, str]] = None,
        residue_idx: Union[np.ndarray, torch.Tensor] = None,
        residue_mask: Union[np.ndarray, torch.Tensor] = None,
        bond_angles: Union[np.ndarray, torch.Tensor] = None,
        bond_lengths: Union[np.ndarray, torch.Tensor] = None,
        include_cb: bool = False,
        **kwargs,
    ) -> "StructureBatch":
        """Backbone (N, CA, C[, CB]) built from ``dihedrals`` (B, N, 3) = [phi, psi, omega] in radians, the layout
        :meth:`backbone_dihedrals` returns -- its inverse (what the reference's ``from_dihedrals`` documents).

        A segment starts at the first residue, where ``chain_idx`` changes (NaN counts as a change) and after a residue
        whose ``residue_mask`` is False; each segment's first residue sits at the ideal position (CA at the origin, C on
        +x, N in the xy-plane) and the others follow by ``geometry.place_fourth_atom``.  phi at a segment's first residue
        and psi / omega at its last are never used.  ``bond_angles`` / ``bond_lengths`` (B, N, 3) override the ideal
        [N-CA-C, CA-C-N(next), C-N(next)-CA(next)] and [|N-CA|, |CA-C|, |C-N(next)|] (defaults: ``geometry.IDEAL_*``).
        Masked residues get zero coordinates and a zero mask; the atom mask is float32 ones / zeros.  Computed in float32
        by one HIP launch (a segmented prefix scan of per-residue rigid transforms), on ``device=`` or the current GPU.
        When grad is enabled and ``dihedrals``, ``bond_angles`` or ``bond_lengths`` requires grad, the batch's coordinates
        stay attached to the autograd graph (``geometry.backbone_from_dihedrals``: one HIP kernel backwards), so a loss on
        e.g. :meth:`inter_residue_geometry` reaches the angles; the values are the same either way."""
        from .general import MAX_N_ATOMS_PER_RESIDUE

        if (chain_idx is not None and chain_ids is None) or (chain_idx is None and chain_ids is not None):
            raise ValueError("Both `chain_idx` and `chain_ids` should be provided or None.")
        dihedrals, chain_idx, residue_idx, residue_mask, bond_angles, bond_lengths = (
            _always_tensor(x) for x in (dihedrals, chain_idx, residue_idx, residue_mask, bond_angles, bond_lengths))
        ops.check_backbone_from_dihedrals_shapes(dihedrals, chain_idx, residue_mask, bond_angles, bond_lengths)
        dev = kwargs.get("device") or (dihedrals.device if dihedrals.is_cuda else _default_device())

        def on_dev(t):
            return None if t is None else t.to(dev)

        builder = ops.backbone_from_dihedrals
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (dihedrals, bond_angles, bond_lengths)):
            from . import geometry
            builder = geometry.backbone_from_dihedrals   # the same launch, with the HIP backward kernel attached
        xyz, atom_mask = builder(
            on_dev(dihedrals), on_dev(chain_idx), on_dev(residue_mask), on_dev(bond_angles), on_dev(bond_lengths),
            include_cb=include_cb, n_slots=MAX_N_ATOMS_PER_RESIDUE)
        return cls(xyz, atom_mask, chain_idx, chain_ids, seq, residue_idx, **kwargs)

    @classmethod
    def from_dihedrals(cls, dihedrals, chain_idx=None, chain_ids=None, **kwargs):
        """Unimplemented in the reference as well (`# TODO`, protstruc.py:321-339); kept as the reference has it.
        :meth:`from_backbone_dihedrals` builds a batch from backbone dihedral angles."""
        raise NotImplementedError("from_dihedrals is a TODO stub in the reference (protstruc.py:321-339)")

    # ------------------------------------------------------------------ getters (protstruc.py:341-433)
    def get_batch_size(self) -> int:
        return self.batch_size

    def get_xyz(self) -> torch.Tensor:
        return self.xyz

    def get_local_xyz(self) -> torch.Tensor:
        """Atoms in the local frame of their residue: R^T x minus the (global) CA position, exactly as the
        reference computes it (protstruc.py:347-362)."""
        rot = self.backbone_orientations()
        ca = self.xyz[:, :, ATOM.CA].contiguous()
        return ops.rigid(self.xyz, rot, -ca, transpose=True)

    def get_atom_mask(self) -> torch.BoolTensor:
        return self.atom_mask

    def get_residue_mask(self) -> torch.BoolTensor:
        # Q5: the getter is the CA slot, not atom_mask.any(-1) (protstruc.py:378)
        return self.atom_mask[:, :, ATOM.CA].bool()

    def get_chain_idx(self) -> torch.LongTensor:
        return self.chain_idx.long()

    def get_chain_ids(self):
        return self.chain_ids

    def get_seq(self):
        return self.seq

    def get_seq_idx(self) -> torch.LongTensor:
        """(B,N) integer amino-acid codes of the chains' sequences, UNK (20) in the padding (protstruc.py:394-409)."""
        from .pdb import ONE_TO_INDEX

        seq_idx = torch.full((self.batch_size, self.n_residues), ONE_TO_INDEX["X"], dtype=torch.long)
        for i, (seqdict, chain_ids) in enumerate(zip(self.seq, self.chain_ids)):
            concat = "".join(seqdict[c] for c in chain_ids)
            seq_idx[i, : len(concat)] = torch.tensor([ONE_TO_INDEX[r] for r in concat], dtype=torch.long)
        return seq_idx.to(self.device)

    def get_total_lengths(self) -> torch.LongTensor:
        return self.residue_mask.cumsum(dim=1).argmax(dim=1) + 1

    def get_max_n_residues(self) -> int:
        return self.n_residues

    def get_max_n_atoms_per_residue(self) -> int:
        return self.max_n_atoms_per_residue

    # ------------------------------------------------------------------ A2 terminal masks
    def get_n_terminal_mask(self) -> torch.BoolTensor:
        """True at the first residue of each chain (protstruc.py:435-443)."""
        return ops.backbone_dihedrals(self.xyz, self.chain_idx, self.residue_mask, want_dihedrals=False,
                                      want_mask=False, want_cterm=False)[2]

    def get_c_terminal_mask(self) -> torch.BoolTensor:
        """True at the last residue of each chain (protstruc.py:445-453)."""
        return ops.backbone_dihedrals(self.xyz, self.chain_idx, self.residue_mask, want_dihedrals=False,
                                      want_mask=False, want_nterm=False)[3]

    # ------------------------------------------------------------------ A1 pairwise distances
    def pairwise_distance_matrix(self) -> Tuple[torch.FloatTensor, torch.BoolTensor]:
        """All-atom distance between every pair of residues (protstruc.py:455-484).

        Returns ``dist (B,N,N,A,A)`` fp32 and ``dist_mask`` of the same shape in
        the dtype of ``atom_mask`` (bool normally).  The mask is not applied to
        ``dist``."""
        dist, dmask = ops.pairwise_distance(self.xyz, self.atom_mask)
        if self.atom_mask is not None and self.atom_mask.dtype != torch.bool:
            dmask = dmask.to(self.atom_mask.dtype)  # Q7: mask dtype follows atom_mask
        return dist, dmask

    def pairwise_distance_matrix_sharded(self, group=None, gather=True, impl=None):
        """Multi-GPU form of :meth:`pairwise_distance_matrix` (one process per GPU, ``torch.distributed`` initialised;
        every rank holds the same batch): this rank computes residue rows [lo, hi) = its share of N straight into a
        full-size buffer; ``gather=True`` reassembles the whole matrix on every rank (RCCL all-gather over xGMI),
        ``gather=False`` leaves the row-sharded result, ``gather="recompute"`` computes everything locally with no
        collective.  Returns ``(dist, dist_mask, (lo, hi))``; see ``protstruc_amd.distributed``."""
        from . import distributed

        dist, dmask, rows = distributed.pairwise_distance_matrix_sharded(self.xyz, self.atom_mask, group=group,
                                                                        gather=gather, impl=impl)
        if self.atom_mask is not None and self.atom_mask.dtype != torch.bool:
            dmask = dmask.to(self.atom_mask.dtype)
        return dist, dmask, rows

    # ------------------------------------------------------------------ A3 backbone dihedrals
    def backbone_dihedrals(self) -> Tuple[torch.FloatTensor, torch.BoolTensor]:
        """phi, psi, omega per residue and their validity mask (protstruc.py:486-541)."""
        dih, dmask, _, _ = ops.backbone_dihedrals(self.xyz, self.chain_idx, self.residue_mask, want_nterm=False,
                                                  want_cterm=False)
        return dih, dmask

    # ------------------------------------------------------------------ A4 / A5 frames
    def backbone_orientations(self, a1: str = "N", a2: str = "CA", a3: str = "C") -> torch.FloatTensor:
        """Gram-Schmidt frame of each residue, basis vectors as columns (protstruc.py:543-571)."""
        s1, s2, s3 = ATOM[a1], ATOM[a2], ATOM[a3]  # KeyError on unknown names, as in the reference
        if torch.is_grad_enabled() and self.xyz.requires_grad:
            from . import geometry
            return geometry.backbone_frames(self.xyz, s1, s2, s3, atom=None)[0]  # the same launch, with the HIP backward kernel attached
        return ops.frames(self.xyz, s1, s2, s3, want_trans=False)[0]

    def backbone_translations(self, atom: str = "CA") -> torch.FloatTensor:
        """Coordinates of one backbone atom per residue -- a view, as in the reference (protstruc.py:573-587)."""
        return self.xyz[:, :, ATOM[atom]]

    def backbone_orientations_and_translations(self, a1: str = "N", a2: str = "CA", a3: str = "C", atom: str = "CA"):
        """Both frame outputs from one launch (rotation (B,N,3,3), translation (B,N,3), contiguous).  Like
        :meth:`backbone_orientations`, differentiable with respect to coordinates that require grad
        (``geometry.backbone_frames``); the values are the same either way."""
        if torch.is_grad_enabled() and self.xyz.requires_grad:
            from . import geometry
            return geometry.backbone_frames(self.xyz, ATOM[a1], ATOM[a2], ATOM[a3], ATOM[atom])
        return ops.frames(self.xyz, ATOM[a1], ATOM[a2], ATOM[a3], ATOM[atom])

    def frame_aligned_point_error(self, target: "StructureBatch", atoms=("N", "CA", "C"), a1: str = "N", a2: str = "CA",
                                  a3: str = "C", clamp=10.0, scale: float = 10.0, eps: float = 1e-4) -> torch.Tensor:
        """Frame-aligned point error of this batch against ``target`` per structure, (B,) (AlphaFold 2 suppl. alg. 28;
        ``geometry.frame_aligned_point_error``).  Frames are the Gram-Schmidt frames of (a1, a2, a3) with the origin at
        ``a2``, from this batch and from ``target``; points are the named ``atoms`` of every residue, or every atom slot
        with ``atoms=None``.  The frame mask is the residues whose three frame atoms are present in both batches, the
        point mask the atoms present in both; the points reach the kernel as the (B, N*A, 3) view of the coordinates with
        the slot selection folded into the mask -- no gather, no copy.  A single-structure target serves the whole batch,
        as in :meth:`align`.  ``clamp`` is a float or a (B,) tensor (``inf`` = unclamped).  Differentiable with respect to
        this batch's coordinates where they require grad (frames and points both; HIP kernels all the way); the target is
        a constant.  NaN coordinates of missing atoms never reach the loss or the gradient."""
        from . import geometry

        B, N, A = self.xyz.shape[:3]
        if target.get_batch_size() != 1 and B != target.get_batch_size():
            raise ValueError("Batch size of the two structures must be the same.")
        txyz = target.get_xyz().detach().to(self.device)
        if tuple(txyz.shape[1:]) != (N, A, 3):
            raise ValueError(f"target coordinates {tuple(txyz.shape)} do not match this batch's {tuple(self.xyz.shape)}")
        s1, s2, s3 = int(ATOM[a1]), int(ATOM[a2]), int(ATOM[a3])
        present = torch.ones(B, N, A, dtype=torch.bool, device=self.device)
        for m in (self.atom_mask, target.get_atom_mask()):
            if m is not None:
                present = present & (m.to(self.device) != 0)      # (1,N,A) of a single-structure target broadcasts
        frame_mask = present[:, :, s1] & present[:, :, s2] & present[:, :, s3]
        if atoms is not None:
            for atom in atoms:
                if not ATOM.is_valid(atom):
                    raise ValueError(f"Atom {atom} is not valid.")
            chosen = torch.zeros(A, dtype=torch.bool, device=self.device)
            chosen[[int(ATOM[a]) for a in atoms]] = True
            present = present & chosen
        if txyz.shape[0] != B:
            txyz = txyz.expand(B, N, A, 3).contiguous()
        with torch.no_grad():
            target_rot, target_trans = ops.frames(txyz, s1, s2, s3, s2)
        rot, trans = geometry.backbone_frames(self.xyz, s1, s2, s3, s2, residue_mask=frame_mask)
        return geometry.frame_aligned_point_error(rot, trans, self.xyz.reshape(B, N * A, 3), target_rot, target_trans,
                                                  txyz.reshape(B, N * A, 3), frame_mask, present.reshape(B, N * A),
                                                  clamp=clamp, scale=scale, eps=eps)

    def lddt(self, target: "StructureBatch", atoms=("CA",), cutoff: float = 15.0, per_residue: bool = True,
             smooth: bool = False) -> torch.Tensor:
        """lDDT of this batch against ``target`` (``geometry.lddt``) over the named ``atoms`` of every residue
        (``atoms="all"``: every atom slot), with the default thresholds 0.5, 1, 2 and 4: per residue, (B,N), the counted
        pairs of a residue's atoms pooled before the division (``per_residue=True``), or per structure, (B,), over all
        counted pairs.  A point counts where its atom is present in both batches and its residue is in both residue
        masks; with more than one atom per residue, pairs inside a residue are excluded (they are rigid).  One atom per
        residue reaches the kernel as the slot's (B,N,3) view of the coordinates; several as the (B, N*A, 3) view with
        the selection folded into the point mask and the residue index as the group -- no gather.  A single-structure
        target serves the whole batch.  A residue (a structure) without a counted pair scores 0.

        ``smooth=False`` is the metric and carries no ``grad_fn``: per residue it is the training target of a pLDDT
        head.  ``smooth=True`` is the sigmoid form, differentiable with respect to this batch's coordinates where they
        require grad (HIP kernels forwards and backwards); the target is a constant.  NaN coordinates of missing atoms
        never reach the score or the gradient."""
        from . import geometry

        B, N, A = self.xyz.shape[:3]
        if target.get_batch_size() != 1 and B != target.get_batch_size():
            raise ValueError("Batch size of the two structures must be the same.")
        txyz = target.get_xyz().detach().to(self.device)
        if tuple(txyz.shape[1:]) != (N, A, 3):
            raise ValueError(f"target coordinates {tuple(txyz.shape)} do not match this batch's {tuple(self.xyz.shape)}")
        if isinstance(atoms, str) and atoms == "all":
            slots = list(range(A))
        else:
            for atom in atoms:
                if not ATOM.is_valid(atom):
                    raise ValueError(f"Atom {atom} is not valid.")
            slots = sorted({int(ATOM[a]) for a in atoms})
            if not slots or slots[-1] >= A:
                raise ValueError(f"atoms {tuple(atoms)} do not fit the {A} atom slots of this batch")
        present = (self.residue_mask & target.residue_mask.to(self.device))[:, :, None].expand(B, N, A)
        for m in (self.atom_mask, target.get_atom_mask()):
            if m is not None:
                present = present & (m.to(self.device) != 0)      # (1,N,A) of a single-structure target broadcasts
        if txyz.shape[0] != B:
            txyz = txyz.expand(B, N, A, 3)
        if len(slots) == 1:
            s = slots[0]
            S, n = geometry.lddt(self.xyz[:, :, s], txyz[:, :, s], present[:, :, s], cutoff=cutoff, smooth=smooth,
                                 reduction="none")
        else:
            chosen = torch.zeros(A, dtype=torch.bool, device=self.device)
            chosen[slots] = True
            groups = torch.arange(N, dtype=torch.int32, device=self.device).repeat_interleave(A).expand(B, N * A)
            S, n = geometry.lddt(self.xyz.reshape(B, N * A, 3), txyz.reshape(B, N * A, 3),
                                 (present & chosen).reshape(B, N * A), groups, cutoff=cutoff, smooth=smooth,
                                 reduction="none")
            S, n = S.reshape(B, N, A).sum(-1), n.reshape(B, N, A).sum(-1)
        if per_residue:
            return S / n.clamp(min=1)
        return S.sum(-1) / n.sum(-1).clamp(min=1)

    # ------------------------------------------------------------------ structural violations
    def _present_atoms(self) -> torch.Tensor:
        """(B,N,A) bool: the atom is there and its residue is in the residue mask."""
        B, N, A = self.xyz.shape[:3]
        present = self.residue_mask[:, :, None].expand(B, N, A)
        if self.atom_mask is not None:
            present = present & (self.atom_mask != 0)
        return present

    def _valid_junctions(self) -> torch.Tensor:
        return valid_junctions(self._present_atoms(), self.chain_idx,
                               None if self.residue_idx is None else _always_tensor(self.residue_idx).to(self.device))

    def _atom_slots(self, atoms) -> List[int]:
        A = self.max_n_atoms_per_residue
        if isinstance(atoms, str) and atoms == "all":
            return list(range(A))
        for atom in atoms:
            if not ATOM.is_valid(atom):
                raise ValueError(f"Atom {atom} is not valid.")
        slots = sorted({int(ATOM[a]) for a in atoms})
        if not slots or slots[-1] >= A:
            raise ValueError(f"atoms {tuple(atoms)} do not fit the {A} atom slots of this batch")
        return slots

    def _atom_points(self, atoms, radii):
        """What the all-atom sweeps take (:meth:`steric_clashes`, :meth:`solvent_accessibility`): the (B, N*A, 3) view of
        the coordinates -- no gather --, the radii (B, N*A) from the sequence (``general.vdw_radius_table``) or from
        ``radii`` (B,N,A), the point mask (B, N*A) with the selection ``atoms`` folded in (present, chosen and with a
        radius above 0; NaN radii compare false), and the sequence codes (B,N) or None."""
        from .general import vdw_radius_table
        from .pdb import ONE_TO_INDEX

        B, N, A = self.xyz.shape[:3]
        slots = self._atom_slots(atoms)
        seq_idx = None if self.seq is None or self.chain_ids is None else self.get_seq_idx()
        if radii is not None:
            radius = _always_tensor(radii).to(device=self.device, dtype=torch.float32)
            if tuple(radius.shape) != (B, N, A):
                raise ValueError(f"radii must have shape {(B, N, A)}, got {tuple(radius.shape)}")
        else:
            table = vdw_radius_table().to(self.device)
            if seq_idx is None and slots[-1] > int(ATOM.CB):
                raise ValueError("without a sequence only the elements of N, CA, C, O and CB are known: pass `radii` "
                                 "(B,N,A), or restrict `atoms` to those five")
            if A > table.shape[1] and slots[-1] >= table.shape[1]:
                raise ValueError(f"the radius table covers {table.shape[1]} atom slots; pass `radii` for {A}")
            rows = table[seq_idx] if seq_idx is not None else table[ONE_TO_INDEX["X"]].expand(B, N, -1)
            radius = torch.zeros(B, N, A, dtype=torch.float32, device=self.device)
            width = min(A, table.shape[1])
            radius[:, :, :width] = rows[:, :, :width]
        chosen = torch.zeros(A, dtype=torch.bool, device=self.device)
        chosen[slots] = True
        takes_part = self._present_atoms() & chosen & (radius > 0)      # NaN radii compare false
        return self.xyz.reshape(B, N * A, 3), radius.reshape(B, N * A), takes_part.reshape(B, N * A), seq_idx

    def steric_clashes(self, atoms="all", tolerance: float = 1.5, radii: Optional[torch.Tensor] = None,
                       per_residue: bool = True) -> torch.Tensor:
        """Steric clash energy (``geometry.steric_clash``; AlphaFold 2 suppl. 1.9.11) between the named ``atoms`` of
        different residues (``atoms="all"``: every atom slot): per residue, (B,N), the sum over the residue's atoms
        (``per_residue=True``), or per structure, (B,), the mean over the atoms that take part.  Two atoms clash where
        they are closer than the sum of their van der Waals radii minus ``tolerance``; every clashing pair counts for
        both of its atoms.  The radii come from the sequence (``general.vdw_radius_table``) or from ``radii`` (B,N,A);
        a batch without a sequence knows the elements of N, CA, C, O and CB only, so any other selection needs ``radii``
        (ValueError).  Atoms without a radius (0) take no part.  The peptide bond C(r) - N(r+1) at a valid junction is no
        clash, nor are two cysteine SG atoms (a disulphide bridge).  The points reach the kernel as the (B, N*A, 3) view of
        the coordinates with the selection folded into the point mask and the residue index as the group -- no gather.
        Differentiable with respect to this batch's coordinates where they require grad (HIP kernels forwards and
        backwards); NaN coordinates of missing atoms never reach the energy or the gradient."""
        from . import geometry
        from .pdb import ONE_TO_INDEX

        B, N, A = self.xyz.shape[:3]
        points, radius, takes_part, seq_idx = self._atom_points(atoms, radii)
        groups = torch.arange(N, dtype=torch.int32, device=self.device).repeat_interleave(A).expand(B, N * A)
        is_cys = None if seq_idx is None else seq_idx == ONE_TO_INDEX["C"]
        link = clash_links(self._valid_junctions(), A, is_cys)
        E, _ = geometry.steric_clash(points, radius, takes_part, groups, link, tolerance=tolerance, reduction="none")
        if per_residue:
            return E.reshape(B, N, A).sum(-1)
        return E.sum(-1) / takes_part.sum(-1).clamp(min=1)

    def solvent_accessibility(self, atoms="all", probe: float = 1.4, n_points: int = 96,
                              radii: Optional[torch.Tensor] = None, per_residue: bool = True, relative: bool = False,
                              per_chain: bool = False) -> torch.Tensor:
        """Solvent-accessible surface area in A^2 (``geometry.solvent_accessibility``; Shrake & Rupley 1973 with
        ``n_points`` test points per atom and a solvent of radius ``probe``) of the named ``atoms`` (``"all"``: every atom
        slot): per residue, (B,N), the sum over the residue's atoms (``per_residue=True``), or per atom, (B,N,A).  Only
        the chosen atoms occlude.  The radii come from the sequence (``general.vdw_radius_table``) or from ``radii``
        (B,N,A), with the rules of :meth:`steric_clashes`; atoms that are missing or have no radius neither occlude nor
        are measured (0), and NaN coordinates there never reach the result.  ``relative=True`` divides a residue's area
        by the theoretical maximum of its type (``general.max_accessibility_table``; Tien et al. 2013): it needs a
        sequence and ``per_residue`` (ValueError), and residues of type X, masked and padded residues are NaN.
        ``per_chain=True`` measures every chain alone, as if the others were not there.  Hydrogens are not modelled, as
        usual for crystal structures.  One HIP kernel; not differentiable."""
        from . import geometry
        from .general import max_accessibility_table

        B, N, A = self.xyz.shape[:3]
        has_seq = self.seq is not None and self.chain_ids is not None
        if relative and not (has_seq and per_residue):
            raise ValueError("relative accessibility is per residue and needs a sequence: use per_residue=True on a batch "
                             "that has one")
        points, radius, takes_part, seq_idx = self._atom_points(atoms, radii)
        isolate = None
        if per_chain:
            isolate = self._chain_keys().repeat_interleave(A, dim=1)
        area = geometry.solvent_accessibility(points, radius, takes_part, isolate, probe=probe, n_points=n_points).area
        area = area.reshape(B, N, A)
        if not per_residue:
            return area
        # summed, and divided, in double and rounded once: a residue's area is as close to the definition as an atom's
        area = area.sum(-1, dtype=torch.float64)
        if relative:
            area = area / max_accessibility_table().to(device=self.device, dtype=torch.float64)[seq_idx]
            area = torch.where(self.residue_mask, area, torch.full_like(area, float("nan")))
        return area.to(torch.float32)

    def interface_area(self) -> torch.Tensor:
        """The surface every residue buries against the other chains, (B,N) A^2:
        ``solvent_accessibility(per_chain=True) - solvent_accessibility()``, the residue's accessible area in its chain
        alone less its area in the whole structure.  Non-negative up to rounding and exactly 0 for a structure of one
        chain; summed over two chains it is the buried surface of their interface."""
        return self.solvent_accessibility(per_chain=True) - self.solvent_accessibility()

    # ------------------------------------------------------------------ neighbour graphs
    def _chain_keys(self) -> torch.Tensor:
        """(B,N) int32 chain index; the padding's NaN becomes -1 (padded residues are outside every mask anyway)."""
        return torch.nan_to_num(self.chain_idx.to(torch.float32), nan=-1.0).to(torch.int32)

    def _residue_points(self, atom, other_chains_only):
        """What the residue graphs take (:meth:`knn_graph`, :meth:`radius_graph`): the residues' ``atom`` (B,N,3), where it
        is present (B,N), and the chain keys (B,N) that leave only the other chains, or None."""
        if not ATOM.is_valid(atom):
            raise ValueError(f"Atom {atom} is not valid.")
        (slot,) = self._atom_slots((atom,))
        exclude = self._chain_keys() if other_chains_only else None
        return self.xyz[:, :, slot], self._present_atoms()[:, :, slot], exclude

    def _flat_atom_points(self, atoms, exclude_same_residue):
        """What the atom graphs take (:meth:`atom_knn_graph`, :meth:`atom_radius_graph`): the (B, N*A, 3) view of the
        coordinates -- no gather --, the point mask (B, N*A) with the selection ``atoms`` folded in, and the residue keys
        (B, N*A) that leave out an atom's own residue, or None."""
        B, N, A = self.xyz.shape[:3]
        chosen = torch.zeros(A, dtype=torch.bool, device=self.device)
        chosen[self._atom_slots(atoms)] = True
        takes_part = (self._present_atoms() & chosen).reshape(B, N * A)
        residue = None
        if exclude_same_residue:
            residue = torch.arange(N, dtype=torch.int32, device=self.device).repeat_interleave(A).expand(B, N * A)
        return self.xyz.reshape(B, N * A, 3), takes_part, residue

    def knn_graph(self, k: int = 30, atom: str = "CA", cutoff: Optional[float] = None, include_self: bool = False,
                  other_chains_only: bool = False):
        """The ``k`` nearest residues of every residue by the distance between their ``atom`` (default CA):
        ``geometry.Neighbors(idx, dist, count)`` with ``idx`` and ``dist`` (B,N,k), nearest first, and ``count`` (B,N).
        A residue takes part -- as a query and as a neighbour -- where it is in the residue mask and has the atom; the
        others get no neighbours, and NaN coordinates there never reach the result.  ``cutoff`` (A) drops residues
        further away; a residue with fewer than ``k`` neighbours is padded with index -1 and distance +inf.  A residue is
        not its own neighbour unless ``include_self``; ``other_chains_only`` keeps the residues of the other chains only
        (the interface graph).  Equal distances go to the lower index.  One HIP kernel (``geometry.nearest_neighbors``);
        no (B,N,N) tensor is built; not differentiable -- ``geometry.gather_neighbors`` rebuilds differentiable edges."""
        from . import geometry

        points, present, exclude = self._residue_points(atom, other_chains_only)
        return geometry.nearest_neighbors(points, k, present, exclude=exclude,
                                          cutoff=float("inf") if cutoff is None else cutoff, include_self=include_self)

    def atom_knn_graph(self, k: int = 32, atoms="all", cutoff: Optional[float] = None, exclude_same_residue: bool = True):
        """The ``k`` nearest atoms of every atom, over the (B, N*A, 3) view of the coordinates -- no gather:
        ``geometry.Neighbors(idx, dist, count)`` with ``idx`` and ``dist`` (B, N*A, k) and ``count`` (B, N*A).  ``idx``
        indexes the flattened atom axis: ``idx // A`` is the neighbour's residue and ``idx % A`` its atom slot (padding
        -1: test ``idx >= 0`` first).  An atom takes part where it is present, its residue is in the residue mask and its
        slot is among ``atoms`` (``"all"``: every slot); the selection is folded into the point mask, and atoms outside
        it get no neighbours.  ``exclude_same_residue`` leaves out the atoms of the atom's own residue (the residue index
        is the exclusion key); without it only the atom itself is left out.  ``cutoff`` (A) drops atoms further away.
        Needs neither a sequence nor radii.  One HIP kernel; no (B, N*A, N*A) tensor is built; not differentiable."""
        from . import geometry

        points, takes_part, residue = self._flat_atom_points(atoms, exclude_same_residue)
        return geometry.nearest_neighbors(points, k, takes_part, exclude=residue,
                                          cutoff=float("inf") if cutoff is None else cutoff)

    def radius_graph(self, cutoff: float = 10.0, atom: str = "CA", include_self: bool = False,
                     other_chains_only: bool = False, max_edges: Optional[int] = None):
        """Every residue within ``cutoff`` (A, inclusive) of every residue by the distance between their ``atom`` (default
        CA): ``geometry.RadiusGraph(row_ptr, col, dist, count)`` -- row ``b * N + i`` is ``col[row_ptr[r]:row_ptr[r + 1]]``,
        the neighbours of residue i of structure b, ascending, with no cap on their number; ``count`` is (B,N).  Who takes
        part, ``include_self`` and ``other_chains_only`` are as in :meth:`knn_graph`; ``max_edges`` as in
        ``geometry.radius_graph`` (None reads the number of edges from the device; an integer makes no host read and
        cuts the list there).  ``geometry.radius_graph_edges`` gives (batch, row, col) triples; not differentiable."""
        from . import geometry

        points, present, exclude = self._residue_points(atom, other_chains_only)
        return geometry.radius_graph(points, cutoff, present, exclude=exclude,
                                     include_self=include_self, max_edges=max_edges)

    def atom_radius_graph(self, cutoff: float = 5.0, atoms="all", exclude_same_residue: bool = True,
                          max_edges: Optional[int] = None):
        """Every atom within ``cutoff`` (A, inclusive) of every atom, over the (B, N*A, 3) view of the coordinates -- no
        gather: ``geometry.RadiusGraph(row_ptr, col, dist, count)`` with ``count`` (B, N*A); ``col`` indexes the flattened
        atom axis (``col // A`` is the neighbour's residue, ``col % A`` its atom slot).  Who takes part, ``atoms`` and
        ``exclude_same_residue`` are as in :meth:`atom_knn_graph`; ``max_edges`` as in ``geometry.radius_graph``.  An
        atom has hundreds of neighbours at 8 - 12 A: nothing is cut.  Not differentiable."""
        from . import geometry

        points, takes_part, residue = self._flat_atom_points(atoms, exclude_same_residue)
        return geometry.radius_graph(points, cutoff, takes_part, exclude=residue, max_edges=max_edges)

    # ------------------------------------------------------------------ residue contacts
    def closest_atom_distances(self, atoms="all", cutoff: Optional[float] = None):
        """How close every pair of residues comes (``geometry.closest_atom_distances``): ``geometry.ClosestAtoms(dist,
        atom_i, atom_j)``, each (B,N,N) -- the smallest distance between a chosen atom of residue i and one of residue j,
        and the two atom slots that attain it (slots of this batch's full atom axis, whatever ``atoms`` selects).  An atom
        takes part where it is present, its residue is in the residue mask and its slot is among ``atoms`` (``"all"``:
        every slot); the selection is folded into the atom mask, no coordinate is copied, and NaN coordinates of missing
        atoms never reach the result.  ``dist`` is +inf and the slots -1 where a residue has no such atom or, with
        ``cutoff`` (A, inclusive), where the residues are further apart.  Exactly symmetric; equal distances go to the
        lower slots.  One HIP kernel; differentiable with respect to this batch's coordinates where they require grad (a
        second HIP kernel backwards; +inf entries pass no gradient)."""
        from . import geometry

        chosen = torch.zeros(self.max_n_atoms_per_residue, dtype=torch.bool, device=self.device)
        chosen[self._atom_slots(atoms)] = True
        return geometry.closest_atom_distances(self.xyz, self._present_atoms() & chosen,
                                               float("inf") if cutoff is None else cutoff)

    def residue_contacts(self, cutoff: float = 5.0, atoms="all", other_chains_only: bool = False,
                         min_separation: int = 1) -> torch.Tensor:
        """The contact map, (B,N,N) bool: residues i and j have two chosen atoms within ``cutoff`` A of each other
        (inclusive; :meth:`closest_atom_distances`).  The diagonal is False, as is every pair with a residue that is
        masked or has none of the ``atoms``.  ``other_chains_only`` keeps the pairs of different chains only;
        ``min_separation`` drops the pairs of one chain that are fewer than that many positions apart along the residue
        axis (1: only the residue itself).  Symmetric.  Not differentiable."""
        if isinstance(min_separation, bool) or not isinstance(min_separation, (int, np.integer)) or min_separation < 0:
            raise ValueError(f"min_separation must be a non-negative integer, got {min_separation!r}")
        N = self.n_residues
        with torch.no_grad():
            dist = self.closest_atom_distances(atoms, cutoff).dist
        position = torch.arange(N, device=self.device)
        apart = (position[:, None] - position[None, :]).abs()
        chain = self._chain_keys()
        other = chain[:, :, None] != chain[:, None, :]
        keep = other if other_chains_only else other | (apart >= int(min_separation))[None]
        return torch.isfinite(dist) & keep & (apart > 0)[None]

    def interface_residues(self, cutoff: float = 5.0, atoms="all") -> torch.Tensor:
        """(B,N) bool: the residue has a chosen atom within ``cutoff`` A of one of a residue of another chain -- the
        interface, epitope or paratope residues of a complex.  All False for a structure of one chain."""
        return self.residue_contacts(cutoff, atoms, other_chains_only=True).any(dim=-1)

    def fraction_native_contacts(self, native: "StructureBatch", cutoff: float = 5.0, atoms="all"):
        """Fnat of CAPRI and DockQ: ``(fnat (B,) float32, n_native (B,) int64)``.  Of the pairs of residues of different
        chains that are in contact in ``native`` (:meth:`residue_contacts` with ``other_chains_only``; every unordered
        pair once), ``n_native`` of them, ``fnat`` is the fraction that is in contact in this batch too; NaN where
        ``n_native`` is 0.  ``native`` has this batch's shape and chain layout (ValueError otherwise)."""
        if not isinstance(native, StructureBatch):
            raise TypeError("native must be a StructureBatch")
        if tuple(native.xyz.shape) != tuple(self.xyz.shape):
            raise ValueError(f"native has coordinates of shape {tuple(native.xyz.shape)}, this batch {tuple(self.xyz.shape)}")
        if native.device != self.device:
            raise ValueError(f"native lives on {native.device}, this batch on {self.device}")
        if not torch.equal(native._chain_keys(), self._chain_keys()):
            raise ValueError("native has another chain layout: the chain index of every residue must be the same")
        upper = torch.ones(self.n_residues, self.n_residues, dtype=torch.bool, device=self.device).triu(1)
        want = native.residue_contacts(cutoff, atoms, other_chains_only=True) & upper
        have = self.residue_contacts(cutoff, atoms, other_chains_only=True) & want
        n_native = want.sum(dim=(1, 2))
        fnat = have.sum(dim=(1, 2)).to(torch.float64) / n_native.to(torch.float64)     # 0 / 0 = NaN
        return fnat.to(torch.float32), n_native

    # ------------------------------------------------------------------ pair heads
    def _pseudo_beta(self):
        """(points (B,N,3), mask (B,N)): CB where the residue has one, else CA (glycine), with the mask to match"""
        present = self._present_atoms()
        ca = int(ATOM.CA)
        cb = int(ATOM.CB)
        if self.max_n_atoms_per_residue <= cb:
            return self.xyz[:, :, ca], present[:, :, ca]
        has_cb = present[:, :, cb]
        points = torch.where(has_cb[:, :, None], self.xyz[:, :, cb], self.xyz[:, :, ca])
        return points, has_cb | present[:, :, ca]

    def distogram_loss(self, logits: torch.Tensor, breaks=None) -> torch.Tensor:
        """AlphaFold 2's distogram loss of a distogram head's ``logits`` (B,N,N,C) against this batch, (B,)
        (``geometry.distogram_loss``): the cross-entropy against the bins of the distances between pseudo-beta atoms -- CB
        where present, else CA -- over the pairs of residues that have one.  ``breaks``: ``C - 1`` bin edges (default 2.3125
        .. 21.6875 A).  Differentiable with respect to ``logits``; the coordinates only choose the bins."""
        from . import geometry

        points, mask = self._pseudo_beta()
        return geometry.distogram_loss(logits, points, mask, breaks)

    def _aligned_error_operands(self, target: "StructureBatch", a1: str, a2: str, a3: str, atom: str):
        """Frames, points and masks of this batch and of ``target`` as :meth:`frame_aligned_point_error` builds them: the
        Gram-Schmidt frames of (a1, a2, a3) with the origin at ``a2``, ``atom`` of every residue as its point, the frame
        mask the residues whose three frame atoms are present in both batches, the point mask those whose ``atom`` is."""
        B, N, A = self.xyz.shape[:3]
        if target.get_batch_size() != 1 and B != target.get_batch_size():
            raise ValueError("Batch size of the two structures must be the same.")
        txyz = target.get_xyz().detach().to(self.device)
        if tuple(txyz.shape[1:]) != (N, A, 3):
            raise ValueError(f"target coordinates {tuple(txyz.shape)} do not match this batch's {tuple(self.xyz.shape)}")
        s1, s2, s3, sp = int(ATOM[a1]), int(ATOM[a2]), int(ATOM[a3]), int(ATOM[atom])
        present = torch.ones(B, N, A, dtype=torch.bool, device=self.device)
        for m in (self.atom_mask, target.get_atom_mask()):
            if m is not None:
                present = present & (m.to(self.device) != 0)      # (1,N,A) of a single-structure target broadcasts
        frame_mask = present[:, :, s1] & present[:, :, s2] & present[:, :, s3]
        if txyz.shape[0] != B:
            txyz = txyz.expand(B, N, A, 3).contiguous()
        with torch.no_grad():
            rot, trans = ops.frames(self.xyz.detach(), s1, s2, s3, s2)
            target_rot, target_trans = ops.frames(txyz, s1, s2, s3, s2)
        return (rot, trans, self.xyz.detach()[:, :, sp], target_rot, target_trans, txyz[:, :, sp], frame_mask, present[:, :, sp])

    def aligned_error(self, target: "StructureBatch", a1: str = "N", a2: str = "CA", a3: str = "C",
                      atom: str = "CA") -> torch.Tensor:
        """The aligned-error matrix of this batch against ``target``, (B,N,N) (``geometry.aligned_error``): the error of
        residue j's ``atom`` seen from residue i's frame, ``|R_i^T (x_j - t_i) - R*_i^T (x*_j - t*_i)|`` -- the training
        target of a PAE head.  Frames and masks as in :meth:`frame_aligned_point_error`; +inf where frame i or point j is
        missing in either batch.  A single-structure target serves the whole batch.  Not differentiable."""
        from . import geometry

        return geometry.aligned_error(*self._aligned_error_operands(target, a1, a2, a3, atom))

    def aligned_error_loss(self, logits: torch.Tensor, target: "StructureBatch", a1: str = "N", a2: str = "CA", a3: str = "C",
                           atom: str = "CA", breaks=None) -> torch.Tensor:
        """AlphaFold 2's predicted-aligned-error loss of a PAE head's ``logits`` (B,N,N,C), (B,)
        (``geometry.aligned_error_loss``): the cross-entropy against the bins of :meth:`aligned_error` of this batch -- the
        prediction -- against ``target``.  ``breaks``: ``C - 1`` bin edges (default 0 .. 31 A).  Differentiable with
        respect to ``logits``; the coordinates only choose the bins."""
        from . import geometry

        *operands, frame_mask, point_mask = self._aligned_error_operands(target, a1, a2, a3, atom)
        return geometry.aligned_error_loss(logits, *operands, frame_mask, point_mask, breaks)

    def predicted_aligned_error(self, logits: torch.Tensor) -> torch.Tensor:
        """The expected aligned error under a PAE head's ``logits`` (B,N,N,C), (B,N,N)
        (``geometry.predicted_aligned_error``); +inf where either residue is outside this batch's residue mask."""
        from . import geometry

        pae = geometry.predicted_aligned_error(logits)
        inside = self.residue_mask[:, :, None] & self.residue_mask[:, None, :]
        return pae.masked_fill(~inside, float("inf"))

    def predicted_tm_score(self, logits: torch.Tensor, interface: bool = False) -> torch.Tensor:
        """AlphaFold's predicted TM-score of a PAE head's ``logits`` (B,N,N,C) over this batch's residue mask, (B,)
        (``geometry.predicted_tm_score``); with ``interface`` over the pairs of residues of different chains only (ipTM)."""
        from . import geometry

        return geometry.predicted_tm_score(logits, self.residue_mask, self._chain_keys(), interface)

    # ------------------------------------------------------------------ superposition scores
    def _paired_with(self, target: "StructureBatch"):
        """(target coordinates (B,N,A,3), atoms present here and in ``target`` (B,N,A), atoms present in ``target``
        (B,N,A)); a single-structure target serves the whole batch."""
        B, N, A = self.xyz.shape[:3]
        if target.get_batch_size() != 1 and B != target.get_batch_size():
            raise ValueError("Batch size of the two structures must be the same.")
        txyz = target.get_xyz().detach().to(self.device)
        if tuple(txyz.shape[1:]) != (N, A, 3):
            raise ValueError(f"target coordinates {tuple(txyz.shape)} do not match this batch's {tuple(self.xyz.shape)}")
        there = target._present_atoms().to(self.device).expand(B, N, A)
        return txyz.expand(B, N, A, 3), self._present_atoms() & there, there

    def rmsd(self, target: "StructureBatch", atoms=("CA",), superimpose: bool = True):
        """The RMSD of this batch against ``target`` over the named ``atoms`` (``"all"``: every slot) that are present in
        both.  ``superimpose=True``: after the optimal superposition, ``SuperpositionRMSD(rmsd (B,), rot (B,3,3), trans (B,3))``
        (``geometry.superposition_rmsd``, HIP kernels forwards and backwards) -- differentiable with respect to this
        batch's coordinates through ``rmsd``; the target is a constant.  ``superimpose=False``: as the structures lie,
        (B,), plain torch on the masked atoms.  A structure without a common atom gives NaN."""
        from . import geometry

        B, N, A = self.xyz.shape[:3]
        txyz, both, _ = self._paired_with(target)
        chosen = torch.zeros(A, dtype=torch.bool, device=self.device)
        chosen[self._atom_slots(atoms)] = True
        mask = (both & chosen).reshape(B, N * A)
        if superimpose:
            return geometry.superposition_rmsd(self.xyz.reshape(B, N * A, 3), txyz.reshape(B, N * A, 3), None, mask)
        diff = torch.where(mask[:, :, None], self.xyz.reshape(B, N * A, 3) - txyz.reshape(B, N * A, 3), torch.zeros((), device=self.device))
        return ((diff.double() ** 2).sum(dim=(1, 2)) / mask.sum(dim=1)).sqrt().float()      # 0 / 0 = NaN

    def _score_operands(self, target: "StructureBatch", atom: str):
        if not ATOM.is_valid(atom):
            raise ValueError(f"Atom {atom} is not valid.")
        s = self._atom_slots((atom,))[0]
        txyz, both, there = self._paired_with(target)
        l_norm = there[:, :, s].sum(dim=1).clamp(min=1).float()
        return self.xyz.detach()[:, :, s], txyz[:, :, s], both[:, :, s], l_norm

    def tm_score(self, target: "StructureBatch", atom: str = "CA"):
        """The TM-score of this batch -- the model -- against ``target``, residue i of one being residue i of the other:
        ``SuperpositionScore(score (B,), rot (B,3,3), trans (B,3))`` (``geometry.tm_score``).  The pairs are the residues
        whose ``atom`` is present in both batches; the score is normalised by, and d0 taken from, the number of residues
        whose ``atom`` is present in the target.  Not differentiable."""
        from . import geometry

        return geometry.tm_score(*self._score_operands(target, atom))

    def gdt_ts(self, target: "StructureBatch", atom: str = "CA") -> torch.Tensor:
        """GDT-TS of this batch against ``target``, (B,) (``geometry.gdt_ts``); pairs and normalisation as :meth:`tm_score`."""
        from . import geometry

        return geometry.gdt_ts(*self._score_operands(target, atom))

    def gdt_ha(self, target: "StructureBatch", atom: str = "CA") -> torch.Tensor:
        """GDT-HA of this batch against ``target``, (B,) (``geometry.gdt_ha``); pairs and normalisation as :meth:`tm_score`."""
        from . import geometry

        return geometry.gdt_ha(*self._score_operands(target, atom))

    def superposition_scores(self, target: "StructureBatch", atom: str = "CA"):
        """``SuperpositionScores(tm, gdt_ts, gdt_ha)`` of this batch against ``target`` from one search of six objectives
        (``geometry.superposition_scores``); pairs and normalisation as :meth:`tm_score`."""
        from . import geometry

        return geometry.superposition_scores(*self._score_operands(target, atom))

    def structural_alignment(self, target: "StructureBatch", atom: str = "CA", use_secondary_structure: bool = True):
        """Align this batch onto ``target`` WITHOUT a residue correspondence, in the manner of TM-align
        (``geometry.structure_alignment``): ``StructuralAlignment(map, n_aligned, tm_a, tm_b, rmsd, rot, trans, search_score,
        start, identity)``.  The two batches have the same batch size (or ``target`` holds one structure for all) and may
        have different numbers of residues; the points are the residues whose ``atom`` is present.  ``map`` (B,N) int32
        holds for a residue of this batch the residue of ``target`` aligned to it, or -1; ``tm_a`` is normalised by this
        batch's length and ``tm_b`` by the target's; ``identity`` (B,) is the fraction of aligned pairs with the same residue
        type, from the two sequences (ValueError without them; NaN where nothing is aligned).  Not differentiable."""
        from . import geometry

        if not ATOM.is_valid(atom):
            raise ValueError(f"Atom {atom} is not valid.")
        B = self.get_batch_size()
        if target.get_batch_size() not in (1, B):
            raise ValueError("Batch size of the two structures must be the same.")
        s, ts = self._atom_slots((atom,))[0], target._atom_slots((atom,))[0]
        txyz = target.get_xyz().detach().to(self.device)[:, :, ts]
        there = target._present_atoms().to(self.device)[:, :, ts]
        Nt = txyz.shape[1]
        mine = self._residue_types("structural_alignment").long()          # before anything is launched: ValueError without a sequence
        theirs = target._residue_types("structural_alignment").long().to(self.device).expand(B, Nt)
        found = geometry.structure_alignment(self.xyz.detach()[:, :, s], txyz.expand(B, Nt, 3), self._present_atoms()[:, :, s],
                                             there.expand(B, Nt), None, use_secondary_structure)
        paired = found.map >= 0
        same = paired & (mine == torch.gather(theirs, 1, found.map.clamp(min=0).long()))
        identity = same.sum(dim=1).float() / paired.sum(dim=1).float()          # 0 / 0 = NaN
        return StructuralAlignment(*found, identity)

    # ------------------------------------------------------------------ ensembles
    def _ensemble_points(self, atoms):
        """((B,P,3) points, (B,P) mask) of the named ``atoms``: with ``"all"`` (or every slot) the zero-copy (B, N*A, 3) view
        of the coordinates, else the chosen slots gathered, (B, N*len(atoms), 3); the mask is the atoms present"""
        B, N, A = self.xyz.shape[:3]
        slots = self._atom_slots(atoms)
        xyz, present = self.xyz.detach(), self._present_atoms()
        if len(slots) != A:
            xyz, present = xyz[:, :, slots], present[:, :, slots]
        return xyz.reshape(B, N * len(slots), 3), present.reshape(B, N * len(slots))

    def rmsd_matrix(self, other: Optional["StructureBatch"] = None, atoms=("CA",)):
        """The RMSD after optimal superposition of every structure of this batch against every structure of ``other``
        (None: against every other structure of this batch) over the named ``atoms`` (``"all"``: every slot, on the
        zero-copy view of the coordinates): ``PairwiseRMSD(rmsd (B,Bo) fp32, count (B,Bo) int32)``
        (``geometry.pairwise_rmsd``, one HIP kernel).  Atom k of residue i of one is atom k of residue i of the other, so
        the two batches have the same number of residues; a pair is compared over the atoms present in both, ``count`` of
        them, and is NaN without any.  Not differentiable."""
        from . import geometry

        points, mask = self._ensemble_points(atoms)
        if other is None:
            return geometry.pairwise_rmsd(points, None, mask, None)
        if other.get_max_n_residues() != self.get_max_n_residues() or other.max_n_atoms_per_residue != self.max_n_atoms_per_residue:
            raise ValueError(f"the other batch's coordinates {tuple(other.xyz.shape)} do not match this batch's "
                             f"{tuple(self.xyz.shape)}: the same number of residues and atom slots is required")
        theirs, their_mask = other._ensemble_points(atoms)
        return geometry.pairwise_rmsd(points, theirs.to(self.device), mask, their_mask.to(self.device))

    def cluster(self, cutoff: float = 2.0, atoms=("CA",)):
        """Cluster the structures of this batch by their mutual superposed RMSD over ``atoms`` (:meth:`rmsd_matrix`) with
        the rule of Daura et al. at ``cutoff`` A (``geometry.cluster_by_cutoff``): ``Clusters(label (B,), center (B,), size
        (B,), n_clusters ())``.  ``center[0]`` is the medoid of the largest cluster.  A structure without any of the atoms is
        no member of anything (label -1).  HIP kernels from the coordinates to the labels, no host read."""
        from . import geometry

        found = self.rmsd_matrix(None, atoms)
        return geometry.cluster_by_cutoff(found.rmsd, cutoff, found.count.diagonal() > 0)

    # ------------------------------------------------------------------ edge features
    def _edge_offsets(self, idx: torch.Tensor, max_offset: int) -> torch.Tensor:
        """(B,N,k) int64 class of every edge of ``idx`` (padding -1): ``clip(r_i - r_j + max_offset, 0, 2 max_offset)``
        within a chain, ``2 max_offset + 1`` across chains, 0 at the padding; ``r`` is ``residue_idx`` where the batch holds
        one and the position along N otherwise.  Plain torch, on any device."""
        from . import geometry

        B, N = self.xyz.shape[:2]
        if self.residue_idx is None:
            r = torch.arange(N, device=self.device).expand(B, N)
        else:   # the padding's NaN becomes 0; padded residues are nobody's neighbour
            r = torch.nan_to_num(_always_tensor(self.residue_idx).to(self.device, torch.float64), nan=0.0).long()
        chain = self._chain_keys()
        within = geometry.gather_neighbors(chain, idx, fill=-2) == chain[:, :, None]
        offset = (r[:, :, None] - geometry.gather_neighbors(r, idx) + max_offset).clamp(0, 2 * max_offset)
        offset = torch.where(within, offset, torch.full_like(offset, 2 * max_offset + 1))
        return offset.masked_fill(idx < 0, 0)

    def _flat_edge_offsets(self, batch: torch.Tensor, row: torch.Tensor, col: torch.Tensor, max_offset: int) -> torch.Tensor:
        """(E,) int64: the classes of :meth:`_edge_offsets` for the flat edges (batch, row, col) of a radius graph, 0 where
        ``batch`` is negative or ``col`` outside [0, N).  Plain torch, no host read."""
        B, N = self.xyz.shape[:2]
        if not (B and N and batch.shape[0]):
            return torch.zeros(batch.shape[0], dtype=torch.int64, device=batch.device)
        if self.residue_idx is None:
            r = torch.arange(N, device=self.device).expand(B, N)
        else:   # the padding's NaN becomes 0; padded residues are nobody's neighbour
            r = torch.nan_to_num(_always_tensor(self.residue_idx).to(self.device, torch.float64), nan=0.0).long()
        chain = self._chain_keys()
        real = (batch >= 0) & (col >= 0) & (col < N)
        b, i, j = batch.clamp(min=0).long(), row.clamp(min=0).long(), col.clamp(0, N - 1).long()
        offset = (r[b, i] - r[b, j] + max_offset).clamp(0, 2 * max_offset)
        offset = torch.where(chain[b, i] == chain[b, j], offset, torch.full_like(offset, 2 * max_offset + 1))
        return offset.masked_fill(~real, 0)

    def _tracks_grad(self) -> bool:
        """whether the float outputs of the edge features carry a graph: the coordinates require grad and grad mode is on"""
        return torch.is_grad_enabled() and self.xyz.requires_grad

    def _edge_frames(self, present: torch.Tensor):
        """The N-CA-C frames and CA positions the edge features are taken of.  Where they carry a graph, residues that
        lack one of the three atoms are kept out of its backward pass, so NaN coordinates there never reach a gradient."""
        if self._tracks_grad():
            from . import geometry
            return geometry.backbone_frames(self.xyz, "N", "CA", "C", "CA", residue_mask=present[:, :, :3].all(dim=-1))
        return self.backbone_orientations_and_translations()

    def _radius_edge_features(self, graph, slots, n_rbf, d_min, d_max, frames, max_offset) -> RadiusEdgeFeatures:
        """:meth:`edge_features` on a ``geometry.RadiusGraph`` over the residues: K49 - K51 and the offsets, no host read."""
        from . import geometry

        B, N, A = self.xyz.shape[:3]
        if tuple(graph.count.shape) != (B, N):
            raise ValueError(f"graph.count must have shape {(B, N)}, the residues of this batch, got {tuple(graph.count.shape)}")
        graph = geometry.RadiusGraph(*(None if t is None else _always_tensor(t).to(self.device) for t in graph))
        centers, sigma = geometry.rbf_centers(n_rbf, d_min, d_max)
        present = self._present_atoms()
        with torch.set_grad_enabled(self._tracks_grad()):   # the float outputs carry a graph where the coordinates require grad
            batch, row = geometry.radius_edge_rows(graph)
            rbf = geometry.radius_edge_distance_features(self.xyz, graph, present, pairs=[(a, b) for a in slots for b in slots],
                                                         centers=centers, sigma=sigma)
            local_pos = rel_rot = None
            if frames:
                if A < 3:
                    raise ValueError(f"frames need the N, CA and C slots; this batch has {A} atom slots")
                rot, trans = self._edge_frames(present)
                local_pos, rel_rot = geometry.radius_edge_frame_features(rot, trans, graph, present[:, :, :3].all(dim=-1))
            col = graph.col if graph.col.dtype == torch.int32 else graph.col.clamp(-1, N).to(torch.int32)
            offset = self._flat_edge_offsets(batch, row, col, int(max_offset))
        return RadiusEdgeFeatures(batch, row, col, batch >= 0, rbf, offset, local_pos, rel_rot)

    def atom_edge_features(self, graph, n_rbf: int = 16, d_min: float = 0.0, d_max: float = 8.0) -> AtomEdgeFeatures:
        """The edge features of an atom graph of :meth:`atom_radius_graph`: ``AtomEdgeFeatures(batch, atom, col, mask, rbf)``,
        flat over the E entries of ``graph.col``.  ``batch`` and ``atom`` (E,) int32 are the structure and the source atom
        of every edge -- ``atom`` and ``col`` index the flattened N*A atom axis, ``// A`` the residue and ``% A`` the slot
        --, -1 from position ``row_ptr[-1]`` on; ``mask`` is ``batch >= 0``.  ``rbf`` (E, n_rbf): ``n_rbf`` Gaussians
        (``geometry.rbf_centers(n_rbf, d_min, d_max)``) of the distance between the two atoms, exactly 0 where ``mask`` is
        False.  Two HIP kernels over the zero-copy (B, N*A, 1, 3) view of the coordinates
        (``geometry.radius_edge_rows``, ``.radius_edge_distance_features``); with a ``max_edges`` graph no host read.
        ``rbf`` is differentiable with respect to this batch's coordinates where they require grad (HIP kernels backwards
        too: K52, K53); the indices and the mask carry no graph."""
        from . import geometry

        B, N, A = self.xyz.shape[:3]
        if not isinstance(graph, geometry.RadiusGraph) or tuple(graph.count.shape) != (B, N * A):
            raise ValueError(f"graph must be a geometry.RadiusGraph over the {(B, N * A)} atoms of this batch (atom_radius_graph)")
        graph = geometry.RadiusGraph(*(None if t is None else _always_tensor(t).to(self.device) for t in graph))
        centers, sigma = geometry.rbf_centers(n_rbf, d_min, d_max)
        with torch.set_grad_enabled(self._tracks_grad()):
            batch, atom = geometry.radius_edge_rows(graph)
            rbf = geometry.radius_edge_distance_features(self.xyz.reshape(B, N * A, 1, 3), graph,
                                                         self._present_atoms().reshape(B, N * A, 1), pairs=((0, 0),),
                                                         centers=centers, sigma=sigma)
        col = graph.col if graph.col.dtype == torch.int32 else graph.col.clamp(-1, N * A).to(torch.int32)
        return AtomEdgeFeatures(batch, atom, col, batch >= 0, rbf)

    def edge_features(self, graph=None, k: int = 30, atoms=("N", "CA", "C", "O", "CB"), n_rbf: int = 16, d_min: float = 2.0,
                      d_max: float = 22.0, frames: bool = True, max_offset: int = 32):
        """What a structure network computes on every edge of a neighbour graph, between :meth:`knn_graph` and its first
        linear layer (ProteinMPNN, Structured Transformer, GVP, PiFold): ``EdgeFeatures(idx, mask, rbf, offset, local_pos,
        rel_rot)``.

        ``graph`` is a ``geometry.Neighbors`` or an index tensor (B,N,k) on the residues; None: ``self.knn_graph(k)``.
        ``idx`` (B,N,k) int32 is the graph with every entry outside [0, N) turned into -1, the padding, and ``mask`` is
        ``idx >= 0``.  ``rbf`` (B,N,k,P*n_rbf): ``n_rbf`` Gaussians (``geometry.rbf_centers(n_rbf, d_min, d_max)``) of the
        distances between the P = len(atoms)^2 ordered atom pairs, pair ``p = a * len(atoms) + b`` being ``atoms[a]`` of the
        source residue against ``atoms[b]`` of the neighbour, at ``rbf[..., p * n_rbf + c]``; exactly 0 at the padding and
        where either atom is missing (the atom mask is the atoms present in residues of the residue mask).  ``offset``
        (B,N,k) int64 is the class of the sequence offset: ``clip(r_i - r_j + max_offset, 0, 2 max_offset)`` within a chain
        and ``2 max_offset + 1`` across chains, with ``r`` the batch's residue numbering (the position along N where it
        holds none); 0 at the padding.  With ``frames``, ``local_pos`` (B,N,k,3) and ``rel_rot`` (B,N,k,3,3) are the
        neighbour's CA and N-CA-C frame in the source residue's frame, ``R_i^T (t_j - t_i)`` and ``R_i^T R_j``, zero
        where either residue lacks N, CA or C; otherwise both are None.  Two HIP kernels
        (``geometry.edge_distance_features``, ``.edge_frame_features``); the offsets are plain torch.  ``rbf``,
        ``local_pos`` and ``rel_rot`` are differentiable with respect to this batch's coordinates where they require grad
        and grad mode is on -- HIP kernels backwards too (K52 - K54, then the frames' own backward kernel), nothing of the
        size of the forward's output kept alive --; ``idx``, ``mask`` and ``offset`` carry no graph, and neither does
        anything where the coordinates do not require grad.

        ``graph`` may also be a ``geometry.RadiusGraph`` over the residues (:meth:`radius_graph`): lists of any length.
        The result is then ``RadiusEdgeFeatures(batch, row, col, mask, rbf, offset, local_pos, rel_rot)``, the same
        features flat over the E entries of ``graph.col`` -- ``rbf`` (E,P*n_rbf), ``offset`` (E,), ``local_pos`` (E,3),
        ``rel_rot`` (E,3,3) -- with ``batch`` and ``row`` (E,) int32 the structure and the source residue of every edge and
        ``mask = batch >= 0``; everything is 0 (``batch`` and ``row`` -1) from position ``row_ptr[-1]`` on.  ``col`` indexes
        the N axis of the edge's own structure: with ``batch`` and ``row`` it is the edge list, not a flat
        ``edge_index`` over a concatenated batch.  Three HIP kernels (``geometry.radius_edge_rows``,
        ``.radius_edge_distance_features``, ``.radius_edge_frame_features``); with a graph made by
        ``radius_graph(max_edges=n)`` the whole call makes no host read and runs inside ``torch.cuda.graph``."""
        from . import geometry

        if isinstance(max_offset, bool) or not isinstance(max_offset, (int, np.integer)) or max_offset < 0:
            raise ValueError(f"max_offset must be a non-negative integer, got {max_offset!r}")
        for atom in atoms:
            if not ATOM.is_valid(atom):
                raise ValueError(f"Atom {atom} is not valid.")
        slots = [int(ATOM[a]) for a in atoms]
        A, N = self.max_n_atoms_per_residue, self.n_residues
        if not slots or max(slots) >= A:
            raise ValueError(f"atoms {tuple(atoms)} do not fit the {A} atom slots of this batch")
        if isinstance(graph, geometry.RadiusGraph):
            return self._radius_edge_features(graph, slots, n_rbf, d_min, d_max, frames, max_offset)
        if graph is None:
            graph = self.knn_graph(k)
        idx = _always_tensor(graph.idx if isinstance(graph, geometry.Neighbors) else graph).to(self.device)
        idx = torch.where((idx >= 0) & (idx < N), idx, torch.full_like(idx, -1)).to(torch.int32)
        centers, sigma = geometry.rbf_centers(n_rbf, d_min, d_max)
        present = self._present_atoms()
        with torch.set_grad_enabled(self._tracks_grad()):
            rbf = geometry.edge_distance_features(self.xyz, idx, present, pairs=[(a, b) for a in slots for b in slots],
                                                  centers=centers, sigma=sigma)
            local_pos = rel_rot = None
            if frames:
                if A < 3:
                    raise ValueError(f"frames need the N, CA and C slots; this batch has {A} atom slots")
                rot, trans = self._edge_frames(present)
                local_pos, rel_rot = geometry.edge_frame_features(rot, trans, idx, present[:, :, :3].all(dim=-1))
            offset = self._edge_offsets(idx, int(max_offset))
        return EdgeFeatures(idx, idx >= 0, rbf, offset, local_pos, rel_rot)

    # ------------------------------------------------------------------ side-chain torsions
    def _residue_types(self, what: str) -> torch.Tensor:
        """(B,N) int32 codes of ``pdb.ONE_TO_INDEX`` from the sequence, which ``what`` needs: ValueError without one."""
        if self.seq is None or self.chain_ids is None:
            raise ValueError(f"{what} needs a sequence: which atoms a chi angle joins depends on the residue type "
                             "(construct the batch with `seq` and `chain_ids`, or use from_pdb)")
        return self.get_seq_idx().to(torch.int32)

    def side_chain_torsions(self):
        """The side-chain torsions chi1 .. chi4 of every residue (``geometry.side_chain_torsions``):
        ``SideChainTorsions(chi (B,N,4) fp32 in radians, mask (B,N,4) bool)``, with the atoms of every angle from
        ``general.chi_atom_table()`` by the sequence.  An angle is defined where the residue type has it, the residue is
        in the residue mask and its four atoms are present; elsewhere ``chi`` is exactly 0 and ``mask`` False.  Needs a
        sequence (ValueError).  One HIP kernel; differentiable with respect to this batch's coordinates where they
        require grad (a second HIP kernel backwards)."""
        from . import geometry

        return geometry.side_chain_torsions(self.xyz, self._residue_types("side_chain_torsions"), self._present_atoms())

    def chi_pi_periodic(self) -> torch.Tensor:
        """(B,N,4) bool: chi and chi + pi name the same structure (``general.chi_pi_periodic_table()`` by the sequence:
        ASP chi2, GLU chi3, PHE chi2, TYR chi2) -- what a torsion-angle loss needs next to the angles.  False where the
        residue type has no such angle.  Needs a sequence (ValueError)."""
        from .general import chi_pi_periodic_table

        return chi_pi_periodic_table().to(self.device)[self._residue_types("chi_pi_periodic").long()]

    def with_side_chain_torsions(self, chi: torch.Tensor, chi_select: Optional[torch.Tensor] = None,
                                 relative: bool = False) -> "StructureBatch":
        """A new batch whose side chains are turned to the angles ``chi`` (B,N,4) -- by them with ``relative`` --
        (``geometry.set_side_chain_torsions`` with ``general.chi_atom_table()`` and ``general.chi_last_table()`` by the
        sequence); this batch is untouched.  Only the angles :meth:`side_chain_torsions` reports as defined are turned,
        of those only where ``chi_select`` (B,N,4; None = all) is true, and never proline's; every other coordinate is
        copied bit for bit.  The new batch shares the masks, chains, sequence and numbering.  Differentiable with respect
        to ``chi`` (HIP kernels on both passes), so a loss of the new batch -- :meth:`steric_clashes`, :meth:`lddt`,
        :meth:`frame_aligned_point_error` -- reaches the angles; this batch's coordinates are a constant and must not
        require grad (ValueError).  Needs a sequence (ValueError)."""
        from . import geometry

        types = self._residue_types("with_side_chain_torsions")
        chi = _always_tensor(chi).to(self.device)
        if chi_select is not None:
            chi_select = _always_tensor(chi_select).to(self.device)
        xyz = geometry.set_side_chain_torsions(self.xyz, chi, types, self._present_atoms(), chi_select, relative)
        new = StructureBatch(xyz, self.atom_mask, self.chain_idx, self.chain_ids, self.seq, self.residue_idx,
                             device=self.device)
        if self._standardized:
            new.mu, new.std, new._standardized = self.mu, self.std, True
        return new

    def peptide_bond_violations(self, **constants) -> torch.Tensor:
        """Peptide-bond violations at every junction r -> r+1, (B,N,3): bond length |C - N'|, cos of CA-C-N', cos of
        C-N'-CA' (``geometry.peptide_bond_violations``; ``tau=12.0`` and the other constants of ``ops.PEPTIDE_BOND`` by
        keyword).  A junction is valid where both residues are in the residue mask and of the same chain, C, CA, N' and CA'
        are present and, where ``residue_idx`` is given, the two residues are consecutive; invalid junctions and the last
        row are exact zeros.  Prolines (from the sequence, where there is one) have their own ideal bond length.
        Differentiable with respect to this batch's coordinates where they require grad."""
        from . import geometry
        from .pdb import ONE_TO_INDEX

        next_is_proline = None
        if self.seq is not None and self.chain_ids is not None:
            next_is_proline = torch.roll(self.get_seq_idx() == ONE_TO_INDEX["P"], -1, dims=1)   # entry N-1 is ignored
        return geometry.peptide_bond_violations(self.xyz, self._valid_junctions(), next_is_proline, int(ATOM.N),
                                                int(ATOM.CA), int(ATOM.C), **constants)

    def structural_violation_loss(self, tolerance: float = 1.5, tau: float = 12.0) -> torch.Tensor:
        """The structural-violation loss of AlphaFold 2 (suppl. 1.9.11, without the within-residue term) per structure,
        (B,): the mean over the valid junctions of each of the three peptide-bond violations
        (:meth:`peptide_bond_violations`), plus the mean clash energy per atom (:meth:`steric_clashes`; every atom slot
        where the batch has a sequence, N, CA, C, O and CB where it has none).  Differentiable with respect to this
        batch's coordinates where they require grad -- HIP kernels on both passes -- so also with respect to the angles
        the coordinates were built from (:meth:`from_backbone_dihedrals`)."""
        viol = self.peptide_bond_violations(tau=tau)
        junctions = self._valid_junctions().sum(-1).clamp(min=1)
        has_seq = self.seq is not None and self.chain_ids is not None
        atoms = "all" if has_seq else tuple(a for a in ("N", "CA", "C", "O", "CB") if int(ATOM[a]) < self.max_n_atoms_per_residue)
        return viol.sum(dim=(1, 2)) / junctions + self.steric_clashes(atoms=atoms, tolerance=tolerance, per_residue=False)

    # ------------------------------------------------------------------ hydrogen bonds and secondary structure
    def _dssp_inputs(self):
        """(complete, junction, donor) of ``geometry.backbone_hbonds`` / ``geometry.dssp``: a residue is complete where
        its N, CA, C and O are present; a junction joins two complete residues (:meth:`_valid_junctions`); where there
        is a sequence a proline donates no amide hydrogen."""
        from .pdb import ONE_TO_INDEX

        if self.max_n_atoms_per_residue <= int(ATOM.O):
            raise ValueError(f"hydrogen bonds need the N, CA, C and O slots; this batch has "
                             f"{self.max_n_atoms_per_residue} atoms per residue")
        present = self._present_atoms()
        complete = present[:, :, int(ATOM.N)] & present[:, :, int(ATOM.CA)] & present[:, :, int(ATOM.C)] & present[:, :, int(ATOM.O)]
        junction = self._valid_junctions()
        junction[:, :-1] &= complete[:, :-1] & complete[:, 1:]
        donor = None
        if self.seq is not None and self.chain_ids is not None:
            donor = self.get_seq_idx() != ONE_TO_INDEX["P"]
        return complete, junction, donor

    def backbone_hbonds(self):
        """The two best backbone hydrogen-bond partners of every residue by the Kabsch-Sander energy of DSSP
        (``geometry.backbone_hbonds``): a named tuple ``(acceptor_idx, acceptor_energy, donor_idx, donor_energy)``, each
        (B,N,2) -- the residues whose C=O accepts this residue's N-H, and the residues whose N-H donate to this residue's
        C=O, lowest energy first, -1 / 0 where there is none.  A residue takes part where its N, CA, C and O are present and
        it is in the residue mask; the amide hydrogen needs a valid junction to the residue before (same chain,
        consecutive, both complete); prolines do not donate where the batch has a sequence.  NaN coordinates of missing
        atoms never reach the result."""
        from . import geometry

        complete, junction, donor = self._dssp_inputs()
        return geometry.backbone_hbonds(self.xyz, complete, junction, donor, int(ATOM.N), int(ATOM.CA), int(ATOM.C),
                                        int(ATOM.O))

    def secondary_structure(self, reduced: bool = False, as_strings: bool = False):
        """DSSP secondary structure (``geometry.dssp``; Kabsch & Sander 1983 on :meth:`backbone_hbonds`): (B,N) int8
        indices into ``geometry.DSSP_CODES`` = "-HBEGITS", or with ``reduced=True`` into ``geometry.DSSP_REDUCED_CODES`` =
        "CHE" (H, G, I -> H; E, B -> E; everything else -> C); ``as_strings=True`` returns a list of B ``str`` instead,
        each as long as its structure.  Incomplete and padded residues are 0.  Energies are not rounded to 0.001, ladders
        are not joined across beta-bulges and the label is a pure per-residue priority, so single residues can differ from
        the DSSP programs' output."""
        from . import geometry

        complete, junction, donor = self._dssp_inputs()
        codes = geometry.dssp(self.xyz, complete, junction, donor, reduced=reduced)
        if as_strings:
            return geometry.dssp_strings(codes, self.get_total_lengths(), reduced=reduced)
        return codes

    # ------------------------------------------------------------------ A6-A8 inter-residue angles
    @staticmethod
    def _pairwise_atom_slots(atoms_i: List[str], atoms_j: List[str]):
        """Name validation of _pairwise_xyz (protstruc.py:603-608); the (B,N^2,n,3) gather itself is never built."""
        for atom in atoms_i + atoms_j:
            if not ATOM.is_valid(atom):
                raise ValueError(f"Atom {atom} is not valid.")
        return [int(ATOM[a]) for a in atoms_i], [int(ATOM[a]) for a in atoms_j]

    def _pairwise_xyz(self, atoms_i: List[str], atoms_j: List[str]) -> torch.FloatTensor:
        """(B, N*N, n_i+n_j, 3) gather of the reference (protstruc.py:589-618), kept for API compatibility only:
        the angle kernels never build it (it is 1.6 GB at B=128, N=512)."""
        si, sj = self._pairwise_atom_slots(atoms_i, atoms_j)
        n = self.n_residues
        coords_i = self.xyz[:, :, si].repeat_interleave(n, dim=1)
        coords_j = self.xyz[:, :, sj].repeat(1, n, 1, 1)
        return torch.cat([coords_i, coords_j], dim=-2)

    def pairwise_dihedrals(self, atoms_i: List[str], atoms_j: List[str]) -> torch.FloatTensor:
        """Dihedral of the four points (atoms_i of residue i ++ atoms_j of residue j) for all (i,j) (protstruc.py:620-640)."""
        si, sj = self._pairwise_atom_slots(atoms_i, atoms_j)
        return ops.pairwise_angles(self.xyz, si, sj, 4)

    def pairwise_planar_angles(self, atoms_i: List[str], atoms_j: List[str]) -> torch.FloatTensor:
        """Planar angle of the three points (protstruc.py:642-660)."""
        si, sj = self._pairwise_atom_slots(atoms_i, atoms_j)
        return ops.pairwise_angles(self.xyz, si, sj, 3)

    def pairwise_dihedrals_sharded(self, atoms_i: List[str], atoms_j: List[str], group=None, gather=True, impl=None):
        """Row-sharded :meth:`pairwise_dihedrals` (see :meth:`pairwise_distance_matrix_sharded`).  Returns ``(out, (lo, hi))``."""
        from . import distributed

        si, sj = self._pairwise_atom_slots(atoms_i, atoms_j)
        return distributed.pairwise_angles_sharded(self.xyz, si, sj, 4, group=group, gather=gather, impl=impl)

    def pairwise_planar_angles_sharded(self, atoms_i: List[str], atoms_j: List[str], group=None, gather=True, impl=None):
        """Row-sharded :meth:`pairwise_planar_angles`.  Returns ``(out, (lo, hi))``."""
        from . import distributed

        si, sj = self._pairwise_atom_slots(atoms_i, atoms_j)
        return distributed.pairwise_angles_sharded(self.xyz, si, sj, 3, group=group, gather=gather, impl=impl)

    def inter_residue_geometry(self) -> Dict[str, torch.Tensor]:
        """trRosetta-style inter-residue features (protstruc.py:790-817).  Differentiable with respect to coordinates that
        require grad (``geometry.inter_residue_geometry``); the values are the same either way."""
        if torch.is_grad_enabled() and self.xyz.requires_grad:
            from . import geometry
            g = geometry.inter_residue_geometry(self.xyz, self.atom_mask)  # the same launch, with the HIP backward kernel attached
        else:
            g = ops.inter_residue_geometry(self.xyz, self.atom_mask)  # one fused launch, no (B,N,N,A,A) tensor
        if self.atom_mask is not None and self.atom_mask.dtype != torch.bool:
            for k in ("d_ca_mask", "d_cb_mask", "d_no_mask"):
                g[k] = g[k].to(self.atom_mask.dtype)
        order = ["d_ca", "d_ca_mask", "d_cb", "d_cb_mask", "d_no", "d_no_mask", "omega", "theta", "phi"]
        return {k: g[k] for k in order}

    # ------------------------------------------------------------------ rigid-body ops
    def translate(self, translation: torch.Tensor, atomwise: bool = False):
        """In-place translation by (B,N,3) / (B,1,3), or (B,N,A,3) with ``atomwise`` (protstruc.py:662-679)."""
        translation = translation.to(self.device)
        want = 4 if atomwise else 3
        if translation.ndim != want:
            raise ValueError(f"translation must have {want} dimensions, got {translation.ndim}")
        ops.rigid(self.xyz, None, translation, inplace=True)

    def rotate(self, rotation: torch.Tensor):
        """x <- R x with R (B,3,3) per structure or (3,3) shared (protstruc.py:681-694)."""
        self.xyz = ops.rigid(self.xyz, rotation.to(self.device), None)

    def center_of_mass(self) -> torch.Tensor:
        """(B,3) mean CA position ignoring NaNs (protstruc.py:746-757)."""
        return ops.center_of_mass(self.xyz, ATOM.CA)

    def center_at(self, center: torch.Tensor = None):
        """Translate so that the CA centre sits at ``center`` ((B,3) or (3,); origin by default) (protstruc.py:759-788)."""
        if center is None:
            center = torch.zeros(1, 3)
        if center.ndim > 2 or center.shape[-1] != 3:
            raise ValueError(f"`center` must have a shape of (batch_size, 3) or (3,), got {center.shape}.")
        if center.ndim == 2 and center.shape[0] != self.batch_size and not (center.shape[0] == 1):
            raise ValueError(f"`center` must have a shape of (batch_size, 3) or (3,), got {center.shape}.")
        center = center.to(self.device, torch.float32).reshape(-1, 3)
        translation = center - self.center_of_mass()          # (B,3) by broadcasting
        ops.rigid(self.xyz, None, translation.contiguous(), inplace=True)

    def align(self, target: "StructureBatch", atom_mask: torch.BoolTensor = None) -> torch.Tensor:
        """Superimpose every structure on ``target`` (Kabsch, over the atoms present in both) and move the
        coordinates (reference protstruc.py:880-918).  One batched launch instead of the reference's Python
        loop + SVD per structure.  A single-structure target serves the whole batch (the reference's loop
        stops after the first structure in that case and applies its rotation to all).  Returns the
        rotations (B,3,3) (the reference documents that but returns None).

        Every rotation is a proper one (det +1), so the structures keep their shape whatever the selection.  Two
        selected atoms or collinear ones leave a family of optimal rotations, of which one is applied; one selected
        atom moves the structure by b - a without turning it; a structure without a selected atom becomes NaN, as in
        the reference (``ops.kabsch``)."""
        if target.get_batch_size() != 1 and self.batch_size != target.get_batch_size():
            raise ValueError("Batch size of the two structures must be the same.")
        if atom_mask is None:
            atom_mask = self.atom_mask * target.get_atom_mask().to(self.device)
        R, t = ops.kabsch(self.xyz, target.get_xyz(), atom_mask.bool())
        self.xyz = ops.rigid(self.xyz, R, t)
        return R

    def get_topk_nearest_residue_mask(self, query_xyz: torch.FloatTensor, k: int = 128,
                                      mask: torch.BoolTensor = None) -> torch.BoolTensor:
        """(1, N) mask of the k residues whose CA is nearest to any query point (protstruc.py:819-862)."""
        if self.batch_size > 1:
            raise ValueError("get_topk_nearest_residue_mask method is not defined "
                             "for a StructureBatch with batch size > 1.")
        dist = ops.min_dist_to_points(self.xyz[0], query_xyz, ATOM.CA)
        _mask = self.residue_mask[0]
        if mask is not None:
            _mask = _mask & mask.to(self.device)
        dist[~_mask] = 1e9
        k = min(k, int(_mask.sum()))
        _, idx = dist.topk(k, largest=False)   # selection of k indices: plain tensor op on the device
        ret = torch.zeros(self.n_residues, dtype=torch.bool, device=self.device).scatter(0, idx, True)
        return ret.unsqueeze(0)

    def residue_masked_select(self, mask: torch.BoolTensor) -> "StructureBatch":
        """Single-structure batch restricted to the residues in ``mask`` (protstruc.py:920-956)."""
        if self.batch_size > 1:
            raise ValueError("residue_masked_select method is not defined "
                             "for a StructureBatch with batch size > 1.")
        if mask.shape != self.residue_mask.shape:
            raise ValueError(f"Mask shape {mask.shape} does not match residue mask shape {self.residue_mask.shape}.")
        if mask.dtype != torch.bool:
            raise ValueError("Mask must be a boolean tensor.")
        mask = mask.to(self.device)
        return StructureBatch(self.xyz[mask].unsqueeze(0), self.atom_mask[mask].unsqueeze(0),
                              self.chain_idx[mask].unsqueeze(0), self.chain_ids, self.seq, device=self.device)

    # ------------------------------------------------------------------ A9 standardize
    def standardize(self, atom_mask: torch.BoolTensor = None, residue_mask: torch.BoolTensor = None):
        """Per-structure, per-axis zero-mean / unit-std coordinates (protstruc.py:696-734)."""
        if atom_mask is not None and residue_mask is not None:
            raise ValueError("Only one of atom_mask and residue_mask can be specified.")
        if self._standardized:
            raise ValueError("Coordinates are already standardized.")
        base = self.atom_mask
        if atom_mask is not None:
            m = atom_mask.to(self.device)
            m = m if base is None else m * base
        elif residue_mask is not None:
            m = residue_mask.to(self.device).unsqueeze(-1)
            m = m.expand(-1, -1, self.max_n_atoms_per_residue) if base is None else m * base
        else:
            m = base
        self.mu, self.std = ops.standardize_(self.xyz, m)
        self._standardized = True

    def unstandardize(self):
        """Undo ``standardize`` (protstruc.py:736-744)."""
        if not self._standardized:
            raise ValueError("Cannot unstandardize structures that are not standardized.")
        ops.affine_(self.xyz, self.std, self.mu)
        self._standardized = False

    # ------------------------------------------------------------------ A10 diffusion
    def manual_seed(self, seed: int) -> "StructureBatch":
        """Seed the device sampler used by ``diffuse_xyz`` (Philox4x32-10, counter reset to 0)."""
        # layout of ps_diffuse_f32's rng_state: word 0 seed, word 1 draw offset, rest zeroed tickets
        state = torch.zeros(ops.RNG_STATE_WORDS, dtype=torch.int64)
        state[0] = int(seed) & 0x7FFFFFFFFFFFFFFF
        self._rng_state = state.to(self.device)
        return self

    def diffuse_xyz(self, beta: torch.FloatTensor, noise: Optional[torch.Tensor] = None):
        """One forward-diffusion step ``xyz <- sqrt(1-beta) xyz + sqrt(beta) eps`` (protstruc.py:864-878).

        ``noise`` (optional, not in the reference) supplies ``eps`` explicitly;
        by default it is drawn on the device."""
        if noise is None and self._rng_state is None:
            self.manual_seed(torch.initial_seed())
        ops.diffuse_(self.xyz, beta.to(self.device), self._rng_state, None if noise is None else noise.to(self.device))

    def diffuse_xyz_and_frames(self, beta: torch.FloatTensor, a1: str = "N", a2: str = "CA", a3: str = "C",
                               atom: str = "CA", noise: Optional[torch.Tensor] = None, out_rot=None, out_trans=None):
        """One diffusion step fused with the frame computation of the new coordinates (one launch):
        equivalent to ``diffuse_xyz(beta)`` followed by ``backbone_orientations(a1, a2, a3)`` and a
        contiguous ``backbone_translations(atom)``; draws the same noise as ``diffuse_xyz`` would."""
        if noise is None and self._rng_state is None:
            self.manual_seed(torch.initial_seed())
        return ops.diffuse_frames_(self.xyz, beta.to(self.device), ATOM[a1], ATOM[a2], ATOM[a3], ATOM[atom],
                                   self._rng_state, None if noise is None else noise.to(self.device),
                                   out_rot=out_rot, out_trans=out_trans)

    def diffuse_trajectory(self, betas: torch.FloatTensor, a1: str = "N", a2: str = "CA", a3: str = "C",
                           atom: str = "CA", want_orientations: bool = True, want_translations: bool = True,
                           want_xyz: bool = False, out_orientations: Optional[torch.Tensor] = None,
                           out_translations: Optional[torch.Tensor] = None, out_xyz: Optional[torch.Tensor] = None):
        """The diffusion loop ``for t: diffuse_xyz(betas[t]); backbone_orientations()`` as ONE launch.

        ``betas`` has shape (T, B).  The coordinates stay in on-chip LDS between steps; only the
        per-step outputs that are asked for are written: orientations (T,B,N,3,3), translations
        (T,B,N,3), coordinates (T,B,N,A,3).  The result is bit-identical to T calls of
        ``diffuse_xyz_and_frames`` and ``get_xyz()`` ends at step T.  ``out_*`` supply caller-owned buffers."""
        if self._rng_state is None:
            self.manual_seed(torch.initial_seed())
        return ops.diffusion_trajectory_(self.xyz, betas.to(self.device), ATOM[a1], ATOM[a2], ATOM[a3], ATOM[atom],
                                         self._rng_state, want_orientations, want_translations, want_xyz,
                                         out_rot=out_orientations, out_trans=out_translations, out_xyz=out_xyz)
