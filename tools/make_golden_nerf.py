#!/usr/bin/env python3
"""Generate tests/golden/g15_place_fourth_atom.npz by running the reference's own geometry.place_fourth_atom
(geometry.py:127-168) on seeded inputs.  Runs only where the reference checkout is available:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_nerf.py --reference <path to the reference checkout>

Inputs are float32 values; the reference is evaluated on them in float64 (its torch ops take either), so the fixture
pins the formula and its conventions, not one float32 rounding.  n = 24 points (never 3: the reference's torch.cross
without `dim` would take the first axis of size 3, quirk Q6).  Two parameter layouts: (n, 1) columns, the documented
shape, and 0-d parameters broadcast against the points.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden"))
    args = ap.parse_args()
    _, geom = import_reference(args.reference)

    rng = np.random.default_rng(15)
    n = 24
    a, b, c = (rng.normal(scale=2.0, size=(n, 3)).astype(np.float32) for _ in range(3))
    length = rng.uniform(0.9, 2.5, size=(n, 1)).astype(np.float32)
    planar = rng.uniform(0.3, np.pi - 0.3, size=(n, 1)).astype(np.float32)
    dihedral = rng.uniform(-np.pi, np.pi, size=(n, 1)).astype(np.float32)
    s_length, s_planar, s_dihedral = np.float32(1.329), np.float32(2.028), np.float32(-2.9)

    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))  # noqa: E731
    x = geom.place_fourth_atom(t(a), t(b), t(c), t(length), t(planar), t(dihedral)).numpy()
    x_scalar = geom.place_fourth_atom(t(a), t(b), t(c), t(s_length), t(s_planar), t(s_dihedral)).numpy()
    path = os.path.join(args.out, "g15_place_fourth_atom.npz")
    np.savez_compressed(path, a=a, b=b, c=c, length=length, planar=planar, dihedral=dihedral, x=x,
                        s_length=s_length, s_planar=s_planar, s_dihedral=s_dihedral, x_scalar=x_scalar)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
