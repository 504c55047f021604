"""Yardstick of the diffusion kernels (csrc/diffusion.hip: k5_diffuse, k54_diffuse_frames, k55_diffusion_trajectory):
the noise stream, the update and the launch geometry, in numpy alone -- no torch, no GPU.

The stream.  Four consecutive coordinates of the flat buffer form group g = e // 4.  Philox4x32-10 (Salmon, Moraes, Dror,
Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; written here from the paper's round function) is run on
    counter = (g & 0xffffffff, g >> 32, offset & 0xffffffff, offset >> 32)      key = (seed & 0xffffffff, seed >> 32)
with seed and offset taken as the unsigned 64-bit pattern of the int64 words of rng_state.  Each output word w becomes a
uniform on a 2^24-point grid IN FLOAT32 ARITHMETIC, u = fl(fl(fl(w >> 8) + 0.5) * 2^-24): the sum is exact below 2^23 and
rounds to even above, so u = 1.0 is reached by w >> 8 = 2^24 - 1 and the smallest u is 2^-25.  Everything after the uniform
is float64 here (Box-Muller):
    z[4g + 0] = sqrt(-2 ln u(w0)) cos(2 pi u(w1))        z[4g + 1] = sqrt(-2 ln u(w0)) sin(2 pi u(w1))
    z[4g + 2] = sqrt(-2 ln u(w2)) cos(2 pi u(w3))        z[4g + 3] = sqrt(-2 ln u(w2)) sin(2 pi u(w3))
so |z| <= sqrt(-2 ln 2^-25) = sqrt(50 ln 2) = 5.887, and a radius word of 1.0 gives z = 0.

The update is the unfused float32 x <- fl(fl(sqrt(fl(1 - beta)) x) + fl(eps fl(sqrt(beta)))) with correctly rounded roots.

The launch geometry (launch_model) mirrors these lines of csrc/diffusion.hip; if one of them changes, the case tables below
have to be derived again (tests/test_diffusion_host.py::test_case_tables_reach_every_arm says which arm went missing):
    K5_COORDS_PER_WG  = 2048    k5_diffuse: blk_begin = blockIdx.x * (1024u * K5_GPL), K5_GPL = 2
    FUSED_RES_PER_WG  = 128     ps_diffuse_frames_f32 / ps_diffusion_trajectory_f32: constexpr int RB = 128
    MAX_SPAN          = 64      #define PS_MAX_SPAN 64 (beta_span_fill: sp.cached = n_span <= PS_MAX_SPAN)
    vec4              k55_diffusion_trajectory: ((e_begin | len | nps | n_total) & 3u) == 0 && out_xyz 16-byte aligned
"""
import collections

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MASK64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
Z_MAX = float(np.sqrt(50.0 * np.log(2.0)))      # sqrt(-2 ln 2^-25)

K5_COORDS_PER_WG = 2048
FUSED_RES_PER_WG = 128
MAX_SPAN = 64


# ---- the stream ------------------------------------------------------------------------------------------------------
def philox4x32_10(counter_words, key_words, rounds=10):
    """Philox4x32 on arrays: ``counter_words`` four and ``key_words`` two uint64 arrays (or scalars) holding 32-bit words.
    Returns the four output words as a (4, n) uint64 array.  ``rounds`` exists for the host test that shows what a
    nine-round generator would do to the stream."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & M32 for c in counter_words)
    k0, k1 = (np.atleast_1d(np.asarray(k, dtype=np.uint64)) & M32 for k in key_words)
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3))


def as_u64(word):
    """The unsigned 64-bit pattern of an int64 word of rng_state (a seed of -1 is 0xffffffffffffffff)."""
    return int(word) & MASK64


def as_i64(word):
    """The int64 that carries the unsigned 64-bit pattern ``word``: what is written into rng_state."""
    word = int(word) & MASK64
    return word - (1 << 64) if word >> 63 else word


def counter_and_key(seed, offset, groups):
    """(counter_words, key_words) of the float4 groups ``groups`` (uint64 array) of draw ``offset`` under ``seed``."""
    seed, offset = as_u64(seed), as_u64(offset)
    groups = np.asarray(groups, dtype=np.uint64)
    counter = (groups & M32, groups >> np.uint64(32), np.uint64(offset & 0xFFFFFFFF), np.uint64(offset >> 32))
    return counter, (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))


def stream_words(seed, offset, n_groups, first_group=0):
    """The (4, n_groups) Philox words of groups first_group ... first_group + n_groups - 1."""
    groups = np.arange(first_group, first_group + n_groups, dtype=np.uint64)
    return philox4x32_10(*counter_and_key(seed, offset, groups))


def u01_f32(w):
    """The uniform of a 32-bit word, in float32 arithmetic: fl(fl(fl(w >> 8) + 0.5) * 2^-24), a float32 array."""
    m = (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)      # < 2^24: exact
    return (m + np.float32(0.5)) * np.float32(2.0 ** -24)


def radius64(u):
    """sqrt(-2 ln u) in float64; u = 1 gives (+)0."""
    return np.sqrt(np.abs(-2.0 * np.log(np.asarray(u, dtype=np.float64))))


def normals64(words):
    """(n, 4) float64 normals of the (4, n) words: (w0, w1) -> z0, z1 and (w2, w3) -> z2, z3."""
    u = u01_f32(words).astype(np.float64)
    r0, r1 = radius64(u[0]), radius64(u[2])
    t0, t1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1)


def noise64(seed, offset, n_total):
    """float64 normals of a flat buffer of ``n_total`` coordinates: draw ``offset`` of the stream keyed by ``seed``."""
    n_groups = (n_total + 3) // 4
    return normals64(stream_words(seed, offset, n_groups)).reshape(-1)[:n_total]


# ---- the update ------------------------------------------------------------------------------------------------------
def step_f32(x, beta, eps):
    """One diffusion step in strict unfused float32: fl(fl(sqrt(fl(1 - beta)) x) + fl(eps fl(sqrt(beta)))).  ``beta``
    broadcasts against ``x`` (per_structure() shapes it); numpy's float32 sqrt is correctly rounded."""
    x, eps = np.asarray(x, dtype=np.float32), np.asarray(eps, dtype=np.float32)
    beta = np.asarray(beta, dtype=np.float32)
    keep, add = np.sqrt(np.float32(1) - beta), np.sqrt(beta)
    return (keep * x).astype(np.float32) + (eps * add).astype(np.float32)


def per_structure(beta, ndim=4):
    """(B,) -> (B, 1, 1, 1): broadcastable against (B, N, A, 3)."""
    beta = np.asarray(beta, dtype=np.float32)
    return beta.reshape(beta.shape + (1,) * (ndim - 1))


def betas_for(B, salt=0):
    """Distinct float32 betas in (0.01, 0.99), one per structure; with three structures or more, structure B // 3 is
    exactly 0.0 (its coordinates must come back bit-identical) and structure 2 B // 3 exactly 1.0."""
    rng = np.random.default_rng(1000 + salt)
    beta = (0.01 + 0.98 * (rng.permutation(B) + rng.random(B)) / B).astype(np.float32)
    assert len(set(beta.tolist())) == B
    if B >= 3:
        beta[B // 3], beta[2 * B // 3] = 0.0, 1.0
    return beta


# ---- the launch geometry ---------------------------------------------------------------------------------------------
Workgroup = collections.namedtuple("Workgroup", "begin length n_span cached partial_group vec4")
Launch = collections.namedtuple("Launch", "kind shape n_total nps grid workgroups")


def launch_model(kind, B, N, A, out_xyz_aligned=True):
    """The launch of ``kind`` ('k5', 'fused' or 'trajectory') on (B, N, A, 3) coordinates: the grid and, per workgroup,
    its element span [begin, begin + length), the number of structures the span touches, whether their betas are cached
    (n_span <= MAX_SPAN; otherwise beta_of takes its slow path), whether the span holds the buffer's partial last float4
    group, and -- for the trajectory kernel, None otherwise -- whether its float4 arm is taken."""
    assert kind in ("k5", "fused", "trajectory")
    rf = 3 * A
    nps, n_total = N * rf, B * N * rf
    per_wg = K5_COORDS_PER_WG if kind == "k5" else FUSED_RES_PER_WG * rf
    grid = -(-n_total // per_wg)
    wgs = []
    for w in range(grid):
        begin = w * per_wg
        length = min(per_wg, n_total - begin)
        n_span = (begin + length - 1) // nps - begin // nps + 1
        partial = n_total % 4 != 0 and begin + length == n_total
        vec4 = None
        if kind == "trajectory":
            vec4 = (begin | length | nps | n_total) & 3 == 0 and out_xyz_aligned
        wgs.append(Workgroup(begin, length, n_span, n_span <= MAX_SPAN, partial, vec4))
    return Launch(kind, (B, N, A), n_total, nps, grid, tuple(wgs))


# ---- the case tables of tests/test_gpu_diffusion.py (B, N, A) ----------------------------------------------------------
# K5.  A workgroup covers 2048 coordinates, and nps = 3 N A is a multiple of 3, so a span of 64 structures needs nps = 33
# and a workgroup that starts 32 coordinates into a structure (2048 w = 32 mod 33: w = 16, B >= 1056); spans of 65 to 68
# structures do not exist (nps = 32, 31 are no multiples of 3): the next ones are 69 and 70, at nps = 30.
K5_CASES = [
    (1, 1, 3),        # 9 coordinates: full groups and one partial group, one workgroup
    (2, 11, 31),      # n_total = 2046: one workgroup, filled but for two coordinates of its last group
    (1, 683, 1),      # n_total = 2049: the second workgroup holds one partial group of one coordinate
    (4, 9, 19),       # n_total = 2052: the second workgroup holds exactly one full group
    (200, 1, 11),     # 33 coordinates per structure: every full workgroup spans 63 structures, cached
    (1100, 1, 11),    # the same, long enough for workgroup 16, which spans exactly 64: the cache limit
    (200, 1, 10),     # 30 per structure: 69 or 70 structures, the slow path
    (700, 1, 3),      # 9 per structure: slow path, a structure boundary inside most float4 groups
    (3, 7, 15),       # plain cached case
]

# Fused step and trajectory: a workgroup covers 128 residues.
FUSED_CASES = [
    (300, 1, 3),      # 128 structures per workgroup: slow path; three workgroups, the last partial (44, cached)
    (130, 2, 5),      # exactly 64 structures per full workgroup
    (90, 3, 4),       # 43 or 44 structures per workgroup, every quantity a multiple of 4: vec4
    (33, 4, 15),      # vec4 at A = 15 with a 4-residue last workgroup
    (3, 43, 15),      # scalar arm (nps odd), 1-residue last workgroup
    (2, 5, 37),       # n_total = 1110 is no multiple of 4: the buffer's last group is partial
    (1, 129, 16),     # one structure across two workgroups; vec4 by the model as well
]

def vec4_cases():
    """The rows of FUSED_CASES whose every trajectory workgroup takes the float4 arm (with an aligned out_xyz)."""
    return [s for s in FUSED_CASES if all(w.vec4 for w in launch_model("trajectory", *s).workgroups)]


SEEDS_OFFSETS = [(0, 0), (2024, 7), (2 ** 32 + 5, 3), (-1, 2 ** 32 - 1), (0x243F6A8885A308D3, 2 ** 40 + 1)]

# Draws of seed 2024, group 0, found by exhaustive search over the offset: (word, offset with w >> 8 = 2^24 - 1, offset
# with w >> 8 = 0).  Words 0 and 2 are the radii of (z0, z1) and (z2, z3), words 1 and 3 their angles.
EDGE_SEED = 2024
EDGE_DRAWS = [(0, 4684430, 74831412), (1, 11246949, 294471), (2, 66932507, 36744153), (3, 10841531, 54532819)]

TICKET_GRIDS = [1, 2, 31, 32, 33, 63, 64, 65, 97]


def ticket_shape(kind, grid):
    """The smallest (B, N, A) of the sweep whose launch has ``grid`` workgroups: K5 with two structures and
    3 B N A in (2048 (G - 1), 2048 G]; fused and trajectory with B N = 128 (G - 1) + 1 residues at A = 3."""
    if kind == "k5":
        return (2, K5_COORDS_PER_WG * (grid - 1) // 6 + 1, 1)
    return (1, FUSED_RES_PER_WG * (grid - 1) + 1, 3)
