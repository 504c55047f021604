"""The yardstick of the closest-atom kernels (K31 / K32): their definition in numpy float64, operation for operation, on
the same float32 inputs the kernels get.  Neither a port of the kernels nor a caller of them.

    X = (double)x      dx = Xjc.x - Xia.x, dy, dz likewise      d2 = (dx*dx + dy*dy) + dz*dz
    over the present atoms a of residue i and c of residue j, i <= j; non-finite d2 are skipped; the winner is the minimum
    under (d2, a, c); it counts iff d2 <= C2 = (double)cutoff * (double)cutoff
    dist[i,j] = (float)sqrt(d2), pair[i,j] = a * A + c;  +inf and -1 where nothing counts
    entry (j,i) is the mirror of (i,j): the same dist and pair[j,i] = c * A + a

Every numpy operation rounds on its own, as the kernel's do under -ffp-contract=off, and a double square root and its
conversion to float32 are correctly rounded on both sides: the tests demand EQUAL pairs and bitwise equal distances.

    grad[i,a,:] = sum over j != i with pair[i,j] = a * A + c of (g[i,j] + g[j,i]) (Xia - Xjc) / sqrt(d2)

over j ascending in double; terms with pair outside [0, A*A) or d2 equal to 0 or non-finite contribute nothing.  ``backward``
returns the double sums and S, the sums of the terms' absolute values, which the error bound of the tests is stated in.

Also here: the numpy versions of what ``StructureBatch`` derives from the distances (contact maps, interface residues,
Fnat) and the case builders.
"""
import numpy as np

from tests import edge_ref


def forward(xyz, mask=None, cutoff=np.inf, rows=64):
    """xyz (B,N,A,3) float32, mask (B,N,A) or None -> (dist (B,N,N) float32, pair (B,N,N) int16).  Chunked over ``rows``
    row residues at a time; masked coordinates are replaced before any arithmetic."""
    x = np.asarray(xyz)
    assert x.dtype == np.float32 and x.ndim == 4, "the yardstick takes the kernel's own float32 values"
    B, N, A = x.shape[:3]
    ok = np.ones((B, N, A), dtype=bool) if mask is None else np.asarray(mask) != 0
    X = np.where(ok[..., None], x, np.float32(0)).astype(np.float64)
    C2 = np.float64(np.float32(cutoff)) * np.float64(np.float32(cutoff))
    d2min = np.full((B, N, N), np.inf)
    best = np.zeros((B, N, N), dtype=np.int64)
    for b in range(B):
        for r0 in range(0, N, rows):
            r1 = min(r0 + rows, N)
            with np.errstate(invalid="ignore", over="ignore"):
                # [i, j, a, c]: the atom c of the column residue j minus the atom a of the row residue i
                dx, dy, dz = (X[b, None, :, None, :, k] - X[b, r0:r1, None, :, None, k] for k in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                both = ok[b, r0:r1, None, :, None] & ok[b, None, :, None, :]
                d2 = np.where(both & np.isfinite(d2), d2, np.inf).reshape(r1 - r0, N, A * A)
            first = np.argmin(d2, axis=-1)          # the first minimum in the order of a * A + c: ties to the lower a, then c
            best[b, r0:r1] = first
            d2min[b, r0:r1] = np.take_along_axis(d2, first[..., None], axis=-1)[..., 0]
    counts = np.isfinite(d2min) & (d2min <= C2)
    with np.errstate(invalid="ignore"):
        dist = np.where(counts, np.sqrt(d2min), np.inf).astype(np.float32)
    pair = np.where(counts, best, -1)
    mirrored = np.where(counts, (best % A) * A + best // A, -1)
    upper = np.arange(N)[:, None] <= np.arange(N)[None, :]
    dist = np.where(upper, dist, dist.transpose(0, 2, 1))
    pair = np.where(upper, pair, mirrored.transpose(0, 2, 1))
    return dist, pair.astype(np.int16)


def backward(xyz, pair, g):
    """xyz (B,N,A,3) float32, pair (B,N,N) integers, g (B,N,N) float32 -> (grad (B,N,A,3) float64, S (B,N,A,3) float64)."""
    x = np.asarray(xyz)
    assert x.dtype == np.float32
    B, N, A = x.shape[:3]
    p = np.asarray(pair).astype(np.int64)
    G = np.asarray(g).astype(np.float64)
    G = G + G.transpose(0, 2, 1)
    grad = np.zeros((B, N, A, 3))
    S = np.zeros((B, N, A, 3))
    bb, ii = np.meshgrid(np.arange(B), np.arange(N), indexing="ij")
    for j in range(N):
        pj = p[:, :, j]
        real = (pj >= 0) & (pj < A * A) & (ii != j)
        a, c = np.where(real, pj // A, 0), np.where(real, pj % A, 0)
        Xa = x[bb, ii, a].astype(np.float64)
        Xc = x[bb, j, c].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            dx, dy, dz = (Xc[..., k] - Xa[..., k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            real &= np.isfinite(d2) & (d2 > 0)
            term = G[:, :, j, None] * (Xa - Xc) / np.sqrt(d2)[..., None]
        term = np.where(real[..., None], term, 0.0)
        grad[bb, ii, a] += term          # one term per (b, i): no index repeats
        S[bb, ii, a] += np.abs(term)
    return grad, S


# ---- what StructureBatch derives from the distances --------------------------------------------------------------------------
def contacts(dist, chain, other_chains_only=False, min_separation=1):
    """dist (N,N) float32 of ``forward`` at the cutoff, chain (N,) integers -> (N,N) bool"""
    N = dist.shape[0]
    apart = np.abs(np.arange(N)[:, None] - np.arange(N)[None, :])
    other = chain[:, None] != chain[None, :]
    keep = other if other_chains_only else other | (apart >= min_separation)
    return np.isfinite(dist) & keep & (apart > 0)


def interface(dist, chain):
    return contacts(dist, chain, other_chains_only=True).any(axis=-1)


def fnat(dist, native_dist, chain):
    """(fnat as float32, n_native) over the unordered inter-chain pairs in contact in the native structure"""
    upper = np.triu(np.ones(dist.shape, dtype=bool), 1)
    want = contacts(native_dist, chain, other_chains_only=True) & upper
    have = contacts(dist, chain, other_chains_only=True) & want
    n = int(want.sum())
    return np.float32(np.float64(have.sum()) / np.float64(n)) if n else np.float32(np.nan), n


# ---- cases -------------------------------------------------------------------------------------------------------------------
def chain_case(N, A, seed, masked=0.45):
    """(xyz (3,N,A,3) float32, mask (3,N,A) bool): residues of A atoms around compact random chains, every slot within about
    2 A of its residue's centre.  In EVERY structure a fraction ``masked`` of the slots is masked with NaN coordinates
    under the mask and one residue is masked entirely (where N > 1)."""
    full = edge_ref.residue_case(N, A, seed, masked=0.0)
    rng = np.random.default_rng(seed + 2000)
    xyz = np.stack([full.xyz[0], full.xyz[2], full.xyz[2][::-1] + np.float32(1.5)]).astype(np.float32)
    mask = rng.random((3, N, A)) >= masked
    if N > 1:
        for b in range(3):
            mask[b, rng.integers(N)] = False
    xyz[~mask] = np.nan
    return xyz, mask


def lattice_case(N=70, A=4, seed=5):
    """(xyz (2,N,A,3) float32, mask (2,N,A) bool) on integer coordinates: residue r sits at (3 (r % 10), 4 (r // 10), 0) and
    each of its atoms there or one unit above, so every squared distance is an exact small integer and a great many are
    equal.  Two residues 3 apart along x and 4 along y come as close as d2 = 25 exactly where they have atoms at the same
    height and d2 = 26 where they have not; the masked slots keep their lattice coordinates, which would win if read."""
    rng = np.random.default_rng(seed)
    r = np.arange(N)
    centre = np.stack([3 * (r % 10), 4 * (r // 10), 0 * r], axis=-1).astype(np.float32)
    offset = np.zeros((2, N, A, 3), dtype=np.float32)
    level = rng.integers(0, 2, size=(2, N, 1))            # three residues in five have all their atoms at one height
    offset[..., 2] = np.where(rng.random((2, N, 1)) < 0.6, level, rng.integers(0, 2, size=(2, N, A)))
    xyz = centre[None, :, None, :] + offset
    mask = rng.random((2, N, A)) >= 0.2
    return xyz.astype(np.float32), mask
