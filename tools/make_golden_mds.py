#!/usr/bin/env python3
"""Generate tests/golden/g16_mds.npz by running the reference's own geometry.initialize_backbone_with_mds
(geometry.py:350-386, sklearn's MDS) on the exact N / CA / C distance matrix of a 16-residue fragment of 15c8_HL.
Runs only where the reference checkout and sklearn are available:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_mds.py --reference <path to the reference checkout>

The reference draws its MDS starts from numpy's global state; the fixture holds the seed, the four starts that
np.random.seed(seed) makes it draw (random_state.uniform(size=3 n) each, n = 3 L), the input matrix (float64) and the
reference's (5, L, 3) output (N, CA, C, O, CB; mirrored unconditionally by its fix_chirality).  The reference's
place_fourth_atom calls torch.cross, so its numpy arrays are passed through as float64 tensors for that step only.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def backbone_15c8(L):
    """N, CA, C of the first L residues of 15c8_HL (ATOM records in file order): (3, L, 3) float64."""
    res = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "15c8_HL.pdb")):
        if line.startswith("ATOM") and line[12:16].strip() in ("N", "CA", "C"):
            key = (line[21], line[22:27])
            res.setdefault(key, {})[line[12:16].strip()] = [float(line[30:38]), float(line[38:46]), float(line[46:54])]
    residues = [r for r in res.values() if len(r) == 3][:L]
    return np.array([[r[a] for r in residues] for a in ("N", "CA", "C")], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--length", type=int, default=16)
    args = ap.parse_args()
    _, geom = import_reference(args.reference)

    L = args.length
    xyz = backbone_15c8(L)                                  # (3, L, 3) float64: N, CA, C
    X = xyz.reshape(3 * L, 3)
    D = np.linalg.norm(X[:, None] - X[None], axis=-1)       # nodes g L + i
    dist_mat = D.reshape(3, L, 3, L).transpose(0, 2, 1, 3)  # (3, 3, L, L)

    np.random.seed(args.seed)
    starts = np.stack([np.random.uniform(size=9 * L).reshape(3 * L, 3) for _ in range(4)])

    place = geom.place_fourth_atom
    as_t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64))  # noqa: E731
    geom.place_fourth_atom = lambda a, b, c, *p: place(*(as_t(v) for v in (a, b, c) + p)).numpy()
    np.random.seed(args.seed)
    coords = geom.initialize_backbone_with_mds(np.ascontiguousarray(dist_mat), max_iter=500)
    geom.place_fourth_atom = place

    path = os.path.join(args.out, "g16_mds.npz")
    np.savez_compressed(path, seed=np.int64(args.seed), dist_mat=dist_mat, starts=starts, coords=np.asarray(coords),
                        true_backbone=xyz)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
