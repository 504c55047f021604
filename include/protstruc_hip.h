/*
 * protstruc_hip.h -- C ABI of libprotstruc_hip.so (gfx950 / MI355X).
 *
 * The reference (dohlee/protstruc v0.0.7) has no FFI: its geometry hot path is
 * a set of Python methods on `StructureBatch` (protstruc/protstruc.py) and free
 * functions in protstruc/geometry.py.  Each entry point below replaces the
 * arithmetic of exactly one of those methods; the Python shell in
 * `protstruc_amd/structure_batch.py` binds them with ctypes and keeps the
 * reference's method signatures.  `file:line` citations are relative to the
 * reference checkout.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (the only exception
 *     are the two small `src` / `atom` descriptor arrays of K3, which are HOST
 *     arrays read before the launch); the library never allocates, frees or
 *     retains memory;
 *   - coordinates are contiguous fp32 `xyz[B][N][A][3]`; masks are contiguous
 *     one-byte booleans (0 / 1; any non-zero input byte counts as true);
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream);
 *   - launches are asynchronous, perform no allocation, no synchronisation and
 *     no host read of device memory, so they may be captured into a hipGraph;
 *   - the library holds no mutable state (no tuning globals, no caches, no handles):
 *     every entry point is re-entrant and may be called concurrently from any
 *     number of threads, devices and streams;
 *   - the return value is a `hipError_t` as int (0 = success); argument errors
 *     return hipErrorInvalidValue (1) before anything is launched.
 */
#ifndef PROTSTRUC_HIP_H
#define PROTSTRUC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_RNG_STATE_WORDS 528

/* ABI version of this header (bumped on any signature change); ps_abi_version() returns the library's. */
#define PS_ABI_VERSION 16
int ps_abi_version(void);

/* Always 0: the library contains no timing experiments.  (Kept for ABI stability: earlier versions had a tools-only build
 * with experiments that could write wrong values, which returned 1.) */
int ps_has_experiments(void);

/* Human-readable text for a code returned by any ps_* function. */
const char* ps_error_string(int code);

/*
 * Launch configuration of K1.  The library holds NO mutable state: every launcher is a pure function of its
 * arguments, so two threads / two devices / two streams of one process can never see each other's settings.
 * A NULL configuration (and ps_pairwise_distance_f32, which takes none) means ps_k1_config_default().
 * Every setting produces the same bits (the two square-root modes differ by at most 1 ulp); the knobs only move
 * work between kernels and change the granule a workgroup writes.  Not part of the drop-in surface; no reference
 * counterpart.
 *
 * Two kinds of fields (the layout is one flat struct for ABI stability):
 *   PRODUCTION -- what a caller or the explicit tuner (ops.autotune_pairwise_distance) sets:
 *       exact_sqrt; rows_per_block, lds_pad_kb, jt (pattern kernel granule and residency); flat_cpw, flat_lds_pad_kb,
 *       flat_fl_log2 = 0 / 6 / 7 (flat kernel granule); xcd_remap.
 *   DIAGNOSTIC -- kept only so that closed A/B comparisons and the cross-check tests stay reproducible; no caller needs
 *   them and the defaults (0) are the product:
 *       variant = 1 (the simple kernels everywhere: the cross-check of the parity tests), flat = 0 / 2 / 4 and
 *       rowphase = 1 / 2 (force or forbid a kernel family; + 16: an A/B switch of the row-phase kernel), store_nt = 1 (non-temporal stores: slower),
 *       flat_fl_log2 = 4 / 5 (the small granules of round 3's bounded A/B).
 *   RESERVED -- experiment: must be 0, any other value is refused.
 */
typedef struct ps_k1_config {
    int struct_size;      /* = sizeof(ps_k1_config); a launcher refuses any other value (caller built against another header) */
    int exact_sqrt;       /* 0: hardware v_sqrt_f32 (exact for 85 % of inputs, 1 ulp off otherwise); 1: correctly rounded,
                             the reference's torch.norm bit for bit */
    int variant;          /* [diagnostic] 0: fast kernels (pattern / flat pattern / row-tile / row-phase / fixed-A flat); 1: the simple
                             kernels everywhere (slot-decode kernel for A = 15, element-per-lane kernel otherwise) */
    int flat;             /* 0: none of the fast kernels for A != 15 and no flat kernel for A = 15; 1 (default): every kernel
                             where it is the fast path; 2: force the A = 15 flat pattern kernel; 4: force the fixed-A flat
                             pattern kernel (A = 14, 15, 16, 24, 32) and no row-tile / row-phase kernel.  (3 was the any-A
                             flat kernel of rounds 1-2, removed: the row-phase kernel is faster at every atom count) */
    int rows_per_block;   /* pattern kernel: residue rows per workgroup, 1..32 (default 1, which for chains shorter than 64
                             residues means ceil(64 / N) rows); row-phase kernel: rows per lane when > 1 (default: 12 / 16 / 24
                             by atom count); row-tile kernel: rows per workgroup when > 1 (default 6) */
    int lds_pad_kb;       /* pattern kernel: KB of idle LDS per workgroup (caps resident workgroups per CU), 0..120; -1 (default): by chain
                             length -- 36 KB (3 workgroups per CU) from 256 residues on, 20 KB (5 per CU) below: eight boxes of round 4,
                             B=64, N=512: 36 KB 1.5-3.8 % ahead of 20 KB on seven; one box, N = 256 .. 2048 +2-3 %, N = 128 even, N <= 64 -7 % */
    int flat_cpw;         /* flat kernels: consecutive chunks per workgroup, 1..64 (default 1) */
    int flat_lds_pad_kb;  /* flat pattern kernel: idle LDS per workgroup, 0..100 */
    int jt;               /* pattern kernel: column residues per tile, 16 / 32 / 64 / 128, 0 = the default (32; 128 for a launch
                             that writes the mask plane only) */
    int xcd_remap;        /* 1 (default): each XCD sweeps one contiguous eighth of the output; 0: natural grid order */
    int store_nt;         /* [diagnostic] 1: non-temporal stores (slower on MI355X; kept for A/B runs) */
    int flat_fl_log2;     /* A = 15 flat pattern kernel: log2(pairs per chunk), 4..7; 0 = the default, 6 (64 pairs, 72 KB per chunk) */
    int rowphase;         /* [diagnostic] row-phase kernel (atom counts up to 64 other than 4, 8): 0 (default) where it is the default
                             dispatch -- every count up to 64 without a row-tile or fixed-A flat kernel, short chains excepted (A = 1, 8..255
                             residues; 2 <= A <= 16 up to 7..64 residues; full matrices): they take the two flat kernels; 1 also for A = 14, 15, 16, 24, 32 and
                             for those CA traces (A/B runs); 2 never (fixed-A flat / element kernels instead).  Bits 4..7 (value / 16) are A/B
                             switches of that kernel: 16 = the A = 1 seam slots written element-wise from both rows (round 3) */
    int experiment;       /* [reserved] must be 0; a launcher refuses any other value (the field selected timing experiments in a
                             tools-only build that no longer exists, and keeps its place for the layout) */
} ps_k1_config;

/* Fills *cfg with the defaults listed above (struct_size included). */
void ps_k1_config_default(ps_k1_config* cfg);

/*
 * K1 -- replaces StructureBatch.pairwise_distance_matrix (protstruc.py:455-484).
 *
 *   dist[b][i][j][a][c]      = | xyz[b][i][a] - xyz[b][j][c] |_2            (fp32)
 *   dist_mask[b][i][j][a][c] = atom_mask[b][i][a] && atom_mask[b][j][c]     (u8)
 *
 * The mask is NOT applied to dist (NaN / padded atoms propagate), as in the
 * reference.  Only residue rows i in [row_begin, row_end) are produced, which is
 * how the residue axis is sharded across GPUs.  The output buffers hold
 * `out_rows` residue rows per structure and row i is written at local row
 * `i - out_row_origin`:
 *     full-size buffers:   out_rows = N,                   out_row_origin = 0
 *     compact shard:       out_rows = row_end - row_begin, out_row_origin = row_begin
 * `atom_mask` may be NULL (all atoms present); `dist_mask` may be NULL (mask
 * plane not produced); `dist` may be NULL (only the mask plane produced).
 * Limits (hipErrorInvalidValue beyond them): B * out_rows * N < 2^32 pairs per launch for the flat kernels
 * (A = 15 at any N >= 16 that is not a multiple of 16; A = 14, 16, 24, 32), 2^31 workgroups for the pattern, row-tile
 * and row-phase kernels (the latter also N * A * A <= 2^28); B <= 65535 only for the two simple kernels that put the
 * structure on grid.z (A = 15 on unaligned planes or with variant = 1; A > 64; unaligned planes).  K2 / K3 run on 1-D grids:
 * any batch size up to 2^31 workgroups per launch.
 * Arithmetic: sqrt(fma(dz, dz, fma(dy, dy, dx*dx))) in fp32, the squared length of the
 * reference's torch.norm; the square root is the hardware instruction (exact for 85 % of
 * inputs, 1 ulp off otherwise) unless ps_k1_config.exact_sqrt selects the correctly rounded
 * routine, which gives the reference's bits.
 */
int ps_pairwise_distance_f32(const float* xyz, const uint8_t* atom_mask,
                             float* dist, uint8_t* dist_mask,
                             int B, int N, int A,
                             int row_begin, int row_end,
                             int out_rows, int out_row_origin,
                             void* stream);

/* The same with an explicit launch configuration (NULL = defaults). */
int ps_pairwise_distance_cfg_f32(const float* xyz, const uint8_t* atom_mask,
                                 float* dist, uint8_t* dist_mask,
                                 int B, int N, int A,
                                 int row_begin, int row_end,
                                 int out_rows, int out_row_origin,
                                 const ps_k1_config* cfg, void* stream);

/*
 * Which K1 kernel a launch with these arguments takes -- a pure host query, nothing is launched and no device memory is
 * touched.  It runs the launcher's OWN dispatcher in a record-only mode (same eligibility predicates, same grid and LDS
 * arithmetic), so the answer cannot drift from what ps_pairwise_distance_cfg_f32 does.  `dist_misalign` /
 * `mask_misalign`: address of the plane modulo 16 (0 for anything torch.empty returns), or -1 when that plane is not
 * requested (NULL); `has_atom_mask`: whether atom_mask would be non-NULL.  Argument errors are the launcher's
 * (hipErrorInvalidValue).  No reference counterpart: it exists so that benchmarks and tests can name the kernel that ran
 * and assert that every kernel family is reached by some tested shape.
 */
typedef struct ps_k1_plan {
    int struct_size;            /* in: sizeof(ps_k1_plan) */
    int n_launches;             /* 0 (empty input) or 1 (every kernel writes both planes in one launch) */
    char family[48];            /* "pattern" | "flat" | "slot_decode" (A = 15); "rowtile" | "rowphase" | "flatA" |
                                   "ca_flat" | "small_flat" | "element" (other atom counts); "empty"; a second launch would be appended with " + " */
    char kernel[96];            /* kernel name with its leading template argument, e.g. "k1_pairdist_a15_pat<32>" */
    unsigned n_workgroups;      /* grid of the first launch */
    unsigned lds_bytes;         /* static + dynamic LDS per workgroup of the first launch */
    int threads_per_workgroup;
    unsigned n_workgroups_2;    /* second launch, if any */
    unsigned lds_bytes_2;
} ps_k1_plan;

int ps_k1_plan_f32(int B, int N, int A, int row_begin, int row_end, int out_rows, int out_row_origin,
                   int dist_misalign, int mask_misalign, int has_atom_mask,
                   const ps_k1_config* cfg, ps_k1_plan* plan);

/*
 * K2 -- replaces StructureBatch.backbone_dihedrals together with
 * get_n_terminal_mask / get_c_terminal_mask (protstruc.py:435-453, :486-541)
 * and geometry.dihedral (geometry.py:74-124).
 *
 *   dihedrals[b][i] = (phi, psi, omega), zero at the batch edge and at chain
 *   termini; dihedral_mask[b][i] = !(nterm, cterm, cterm) && residue_mask[b][i].
 * chain_idx is fp32 (NaN marks padding; NaN != NaN makes a terminus).
 * Atom slots 0,1,2 (N, CA, C) of each residue are read.  Any of the four
 * outputs may be NULL.
 */
int ps_backbone_dihedrals_f32(const float* xyz, const float* chain_idx,
                              const uint8_t* residue_mask,
                              float* dihedrals, uint8_t* dihedral_mask,
                              uint8_t* nterm, uint8_t* cterm,
                              int B, int N, int A, void* stream);

/*
 * K3 -- replaces StructureBatch.pairwise_dihedrals / pairwise_planar_angles and
 * the (B, N*N, n, 3) gather of _pairwise_xyz (protstruc.py:589-660), with
 * geometry.dihedral / geometry.angle (geometry.py:39-124) evaluated per pair.
 *
 *   n_points == 4: out[b][i][j] = dihedral(p0, p1, p2, p3)
 *   n_points == 3: out[b][i][j] = angle(p0, p1, p2)   (acos, no clamp -> NaN as in the reference)
 * where p_k = xyz[b][ src[k] ? j : i ][ atom[k] ].  Rows i in
 * [row_begin, row_end) are produced into an (B, out_rows, N) buffer with the same
 * row addressing as K1.
 * exact_angles (ABI 4; bit field since ABI 5), the angle counterpart of ps_k1_config.exact_sqrt:
 *   bit 0 -- arithmetic.
 *     0  the fast arithmetic: triple-product dihedral with one reciprocal square root, polynomial atan2 / acos, cosine
 *        through v_rsq_f32 -- exact where the reference is exact (+0 diagonal, NaN positions), otherwise within the
 *        conditioning gates of SURVEY hard part 3 (3.8e-6 of off-diagonal dihedrals more than 1e-5 from the reference
 *        at unit scale, max 6.5e-5; profiles/r04_k3_error_stats.log);
 *     1  the reference's order of operations (geometry.py:110-124, :64-66): three cross products, y / |b1| with a
 *        correctly rounded square root and an IEEE division, the device library's atan2f / acosf restated instruction
 *        for instruction (atan2_lib / acos_lib; no kernel calls the library).  No entry more than 1e-5 from the reference
 *        on well-conditioned inputs.  Since ABI 5 on the same per-CU sweep kernels as the fast arithmetic (the
 *        restatement in packed form, bit-identical to the scalar restatement the one-column kernel runs and to the
 *        library's own results); DESIGN.md section 4 has both modes' times side by side.
 *   bit 1 -- [diagnostic] the simple one-column kernel at every shape, in the arithmetic bit 0 selects: the layout-free
 *        cross-check kernel of the parity tests, like ps_k1_config.variant = 1.  Same bits as without it.
 *   (So 0 = fast, 1 = faithful, 2 = fast / one-column, 3 = faithful / one-column; anything else: hipErrorInvalidValue.)
 * The device a launch runs on is the stream's (hipStreamGetDevice); for the NULL stream, the calling thread's current device.
 */
int ps_pairwise_angles_f32(const float* xyz, float* out,
                           int B, int N, int A,
                           int n_points, const int* src, const int* atom,
                           int row_begin, int row_end,
                           int out_rows, int out_row_origin,
                           int exact_angles, void* stream);

/*
 * Which K3 / featuriser kernel a launch with these arguments takes -- pure host queries (ABI 5): nothing is launched,
 * no device memory is touched and NO HIP call is made.  They run the launchers' OWN dispatchers in a record-only mode
 * (same predicates, same grid and LDS arithmetic; K1 has the same arrangement: ps_k1_plan_f32), so the answer cannot
 * drift from what ps_pairwise_angles_f32 / ps_inter_residue_geometry_f32 do.  `out_misalign`: address of `out` modulo
 * 16 (a multiple of 4; 0 for anything torch.empty returns); `float_misalign` / `mask_misalign`: the OR of the six fp32 /
 * three mask plane addresses modulo 128; `cu_count`: compute units of the device (<= 0: 256, an MI355X).  Argument errors
 * are the launchers' (hipErrorInvalidValue).  No reference counterpart: they exist so that benchmarks and tests can name
 * the kernel that ran and assert that every arm of the dispatchers is reached by a shape that is held to the oracle.
 */
typedef struct ps_k3_plan {
    int struct_size;            /* in: sizeof(ps_k3_plan) */
    int n_launches;             /* 0 (empty input) or 1 */
    char family[32];            /* "sweep" | "flat_tiles" | "small" | "one_column" (K3); "featurise" | "featurise_tiles" | "one_column" (featuriser); "empty" */
    char kernel[96];            /* kernel name with its template arguments, e.g. "k3_sweep<NP=4,SRC=12,NC=4,VEC=1,FAITHFUL=0>" */
    int columns_per_lane;       /* sweep / featurise: 2 or 4 column residues per lane; flat_tiles: chains per lane (a 2 x 2 tile);
                                   small: the padded chain length (16 / 32); else 1 */
    int vector_stores;          /* 1: the lane's columns are adjacent (8- / 16-byte stores); 0: 64 apart / dword stores (any N);
                                   flat_tiles / featurise_tiles: 2 = four-column tiles, 16-byte stores (N % 4 == 0), 1 = two-column tiles, 8-byte stores */
    int skips_dead_groups;      /* 1: dead 64-column groups of a row's last strip are not evaluated */
    int mask_store_mode;        /* featuriser: 4 four bytes / 3 two bytes per tile row (tiles), 2 strip-local 16-byte stores, 1 flat 16-byte stores, 0 bytes */
    int write_through;          /* featuriser: sc1 stores */
    int faithful;               /* bit 0 of exact_angles */
    int rows_per_task;          /* rows of one pulled task (sweep / featurise); rows per workgroup otherwise */
    int workgroups_per_cu;      /* 1 or 2 for the per-CU kernels (their LDS request pins it), 0: not pinned */
    int structures_per_segment; /* sweep / featurise: 1; flat: structures staged in LDS together; else 0 */
    unsigned n_workgroups;
    int threads_per_workgroup;
    unsigned lds_bytes;         /* static + dynamic LDS per workgroup */
    unsigned n_tasks;           /* per-CU kernels: length of the task list, and a workgroup's share of it */
    unsigned tasks_per_workgroup;
} ps_k3_plan;

int ps_k3_plan_f32(int B, int N, int A, int n_points, const int* src, const int* atom,
                   int row_begin, int row_end, int out_rows, int out_row_origin,
                   int out_misalign, int exact_angles, int cu_count, ps_k3_plan* plan);

/*
 * K4 -- replaces StructureBatch.backbone_orientations + backbone_translations
 * (protstruc.py:543-587) and geometry.gram_schmidt (geometry.py:413-439).
 *
 *   rot[b][i] (3x3 row-major) has columns e1 = unit(a3-a2),
 *   e2 = unit((a1-a2) - (e1.(a1-a2)) e1), e3 = e1 x e2;  trans[b][i] = xyz[b][i][t_atom].
 * Either output may be NULL.
 */
int ps_frames_f32(const float* xyz, float* rot, float* trans,
                  int B, int N, int A, int a1, int a2, int a3, int t_atom,
                  void* stream);

/*
 * Backward pass of ps_frames_f32 (ABI 11): the vector-Jacobian product of the Gram-Schmidt frame (v1 = a3 - a2,
 * e1 = v1 / |v1|, u2 = (a1 - a2) - (e1 . (a1 - a2)) e1, e2 = u2 / |u2|, e3 = e1 x e2) and of the translation pick, per
 * residue:  grad_xyz[b][i][s][:] = sum over the entries of rot[b][i] and trans[b][i] of their upstream gradient times
 * their derivative with respect to xyz[b][i][s][:].  grad_rot (B,N,3,3) is an unconstrained 3x3 gradient (not assumed
 * tangent to the rotations), grad_trans (B,N,3); either may be NULL (zero; its arithmetic is skipped), not both.
 * Contributions are summed where slots coincide (t_atom == a2 is the normal case).  EVERY element of grad_xyz (B,N,A,3)
 * is written: slots that are not read, and every slot of a residue whose residue_mask byte is 0 (NULL = all present),
 * receive exact zeros by selection -- NaN coordinates or NaN upstream values of a masked residue never reach the result.
 */
int ps_frames_backward_f32(const float* xyz, const float* grad_rot, const float* grad_trans,
                           const uint8_t* residue_mask, float* grad_xyz,
                           int B, int N, int A, int a1, int a2, int a3, int t_atom, void* stream);

/*
 * Point-wise geometry primitives -- replace the free functions geometry.angle,
 * geometry.dihedral and geometry.gram_schmidt (geometry.py:39-124, :413-439) on
 * (n,3) point arrays:  mode 0: out[n] = angle(a,b,c);  mode 1: out[n] =
 * dihedral(a,b,c,d);  mode 2: out[n][3][3] = gram_schmidt(a,b,c);  mode 3 (ABI 6):
 * out[n][3] = place_fourth_atom(a,b,c, d[n][0], d[n][1], d[n][2]) (geometry.py:127-168)
 * with d packed (length, planar, dihedral): |X-c| = length, angle(X,c,b) = planar,
 * dihedral(a,b,c,X) = dihedral.  Radians.
 */
int ps_pointwise_f32(int mode, const float* a, const float* b, const float* c, const float* d,
                     float* out, long long n, void* stream);

/*
 * K5 -- replaces StructureBatch.diffuse_xyz (protstruc.py:864-878), in place:
 *   xyz[b] <- sqrt(1 - beta[b]) * xyz[b] + sqrt(beta[b]) * eps,  eps ~ N(0,1) iid.
 * `n_per_struct` = N*A*3.  If `noise` is non-NULL it supplies eps (parity with
 * the reference's deterministic part); otherwise eps comes from Philox4x32-10 +
 * Box-Muller keyed by rng_state[0] (seed) at counter offset rng_state[1], and
 * rng_state[1] is advanced on the device by the last workgroup to finish, so that
 * a captured graph replays with fresh noise without a second launch.  rng_state is
 * a device array of PS_RNG_STATE_WORDS (528) uint64: word 0 = seed, word 1 =
 * offset, the rest are completion tickets that must be zero when a call starts
 * (the kernels leave them zero).
 *
 * The stream (tests/diffusion_ref.py::noise64 is this paragraph in numpy).  Coordinate
 * e of the flat (B * n_per_struct) buffer belongs to group g = e / 4.  Philox4x32-10
 * (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten
 * rounds) runs on
 *   counter = (g & 0xffffffff, g >> 32, offset & 0xffffffff, offset >> 32)
 *   key     = (seed & 0xffffffff, seed >> 32)
 * with seed and offset the unsigned 64-bit words 0 and 1 of rng_state, and returns
 * four 32-bit words w0..w3.  Each becomes a uniform in float32 arithmetic,
 *   u(w) = ((float)(w >> 8) + 0.5f) * 2^-24,
 * a 2^24-point grid in [2^-25, 1]: the sum rounds to even from 2^23 on, and
 * w >> 8 = 2^24 - 1 gives exactly 1.0.  Box-Muller pairs them as
 *   eps[4g + 0] = sqrt(-2 ln u(w0)) * cos(2 pi u(w1))
 *   eps[4g + 1] = sqrt(-2 ln u(w0)) * sin(2 pi u(w1))
 *   eps[4g + 2] = sqrt(-2 ln u(w2)) * cos(2 pi u(w3))
 *   eps[4g + 3] = sqrt(-2 ln u(w2)) * sin(2 pi u(w3))
 * evaluated with the hardware's float32 log2, sqrt, sin and cos (within 8e-7 of
 * the exact value over 4.5e6 draws measured on an MI355X; |eps| <= sqrt(50 ln 2)
 * = 5.887).  The call then stores
 * offset + 1.  ps_diffuse_frames_f32 draws the same numbers from the same
 * rng_state, and step t of ps_diffusion_trajectory_f32 draws those of offset + t.
 */
int ps_diffuse_f32(float* xyz, const float* beta, int B, int n_per_struct,
                   uint64_t* rng_state, const float* noise, void* stream);

/*
 * K6 -- replaces StructureBatch.standardize (protstruc.py:696-734), in place,
 * with per-structure statistics (what the reference computes at B == 1; its
 * B > 1 broadcast is a defect):
 *   cnt = sum(mask); mu = sum(nan_to_num(xyz*mask))/cnt;
 *   std = sqrt(sum((nan_to_num(xyz)-mu)^2 * mask)/cnt); xyz <- (xyz-mu)/std.
 * mu and std are (B,3) outputs.
 */
int ps_standardize_f32(float* xyz, const uint8_t* atom_mask, float* mu, float* std,
                       int B, int N, int A, void* stream);

/* The same with the kernel chosen explicitly: variant 0 = what ps_standardize_f32 does (the LDS-resident kernel --
 * one read and one write of the coordinates -- when a structure fits in 150 KB of LDS, i.e. N*A <= 12800 atoms);
 * variant 1 = always the three-sweep streaming kernel.  Both produce the same bits; this entry point exists for
 * that cross-check and for timing. */
int ps_standardize_variant_f32(float* xyz, const uint8_t* atom_mask, float* mu, float* std,
                               int B, int N, int A, int variant, void* stream);

/*
 * Replaces StructureBatch.unstandardize (protstruc.py:736-744), in place:
 *   xyz[b] <- xyz[b] * scale[b] + shift[b]   per coordinate axis; scale, shift are (B,3).
 */
int ps_affine_f32(float* xyz, const float* scale, const float* shift,
                  int B, int n_atoms_per_struct, void* stream);

/*
 * Fused step of the diffusion loop (BASELINE config 5): K5 followed by K4 on the
 * freshly diffused coordinates in one launch -- replaces the pair of calls
 * diffuse_xyz (protstruc.py:864-878) + backbone_orientations / backbone_translations
 * (protstruc.py:543-587).  Arguments as K5 and K4; the noise stream is identical
 * to the one ps_diffuse_f32 would draw from the same rng_state.
 */
int ps_diffuse_frames_f32(float* xyz, const float* beta, int B, int N, int A,
                          uint64_t* rng_state, const float* noise,
                          float* rot, float* trans, int a1, int a2, int a3, int t_atom,
                          void* stream);

/*
 * The whole diffusion loop (BASELINE config 5) in one launch: T steps of
 * ps_diffuse_frames_f32 with the coordinates resident in LDS between steps.
 * betas is (T, B); rot (T,B,N,3,3), trans (T,B,N,3) and xyz_traj (T,B,N,A,3) are
 * optional per-step outputs (NULL = not produced); xyz holds the final
 * coordinates.  Bit-identical to T successive calls of ps_diffuse_frames_f32
 * from the same rng_state (which ends up advanced by T).  rng_state is required.
 */
int ps_diffusion_trajectory_f32(float* xyz, const float* betas, int T, int B, int N, int A,
                                uint64_t* rng_state, float* rot, float* trans, float* xyz_traj,
                                int a1, int a2, int a3, int t_atom, void* stream);

/*
 * Fused trRosetta featuriser -- replaces StructureBatch.inter_residue_geometry
 * (protstruc.py:790-817) without materialising the (B,N,N,A,A) tensor: writes
 * six (B,N,N) fp32 planes d_ca, d_cb, d_no (slices [CA,CA], [CB,CB], [N,O] of
 * K1's dist), omega = dihedral(CA_i,CB_i,CA_j,CB_j), theta =
 * dihedral(N_i,CA_i,CB_i,CB_j), phi = angle(CA_i,CB_i,CB_j), and the three
 * (B,N,N) u8 mask planes.  atom_mask may be NULL (all present).  Needs A >= 5.
 * exact_sqrt: the square root of the three distance planes, as ps_k1_config.exact_sqrt -- 0: hardware v_sqrt_f32
 * (K1's default: the planes are then bit-identical to the slices of a default K1 launch), 1: correctly rounded
 * (bit-identical to K1 with exact_sqrt = 1).
 * exact_angles (ABI 4; bit field since ABI 5): omega, theta and phi in the arithmetic ps_pairwise_angles_f32 uses for the
 * same value (bit 0: 0 fast, 1 the reference's order of operations; bit 1: the one-column kernel at every shape): the three
 * planes equal the corresponding K3 launches bit for bit in every mode.
 * Placement of the nine planes: any 4-byte (fp32) / 1-byte (mask) boundary, each plane its own; results do not depend on
 * it.  Fastest where every plane starts on a 16-byte boundary (vector stores; the three mask planes then share one 16-byte
 * grid) -- protstruc_amd.ops pads the plane stride accordingly.
 */
int ps_inter_residue_geometry_f32(const float* xyz, const uint8_t* atom_mask,
                                  float* d_ca, float* d_cb, float* d_no,
                                  float* omega, float* theta, float* phi,
                                  uint8_t* d_ca_mask, uint8_t* d_cb_mask, uint8_t* d_no_mask,
                                  int B, int N, int A, int exact_sqrt, int exact_angles, void* stream);

/* The featuriser's twin of ps_k3_plan_f32 (ABI 5; see there). */
int ps_featuriser_plan_f32(int B, int N, int A, int float_misalign, int mask_misalign,
                           int exact_sqrt, int exact_angles, int cu_count, ps_k3_plan* plan);

/*
 * Backward pass of ps_inter_residue_geometry_f32 (ABI 9; no reference counterpart: the reference's dihedral goes
 * through numpy and is not differentiable).  A vector-Jacobian product in one launch:
 *   grad_xyz[b][r][s][:] = sum over the six float planes and over (i, j) of g_plane[b][i][j] * d plane[b][i][j] / d xyz[b][r][s][:]
 * g_d_ca .. g_phi are the (B,N,N) fp32 upstream gradients of the planes of the same name; any of them may be NULL, which
 * means zero (its arithmetic is skipped).  grad_xyz is (B,N,A,3) fp32 and EVERY element of it is written: slots other
 * than N (0), CA (1), O (3) and CB (4) receive exact zeros, so the buffer need not be initialised.
 * Active entries.  Entry (b, i, j) of a plane contributes only when (1) every atom it reads is present in atom_mask
 * (NULL = all present) -- d_ca: CA_i, CA_j; d_cb: CB_i, CB_j; d_no: N_i, O_j; omega: CA_i, CB_i, CA_j, CB_j; theta: N_i,
 * CA_i, CB_i, CB_j; phi: CA_i, CB_i, CB_j -- and (2) i != j, for every plane but d_no (sqrt(0), atan2(0, 0) and 0 / 0 have
 * no derivative; the diagonal of d_no is an ordinary N_i - O_i distance).  Every other entry contributes exactly zero, by
 * selection and not by multiplication: NaN coordinates of absent atoms and NaN upstream values at inactive entries never
 * reach the result.  The derivative is that of the mathematical functions the forward evaluates (omega is
 * dihedral(CA_i,CB_i,CA_j,CB_j) as coded; sign of geometry.dihedral).  There is one arithmetic: exact_sqrt / exact_angles
 * of the forward select no backward variant.  Deterministic: no atomics, a fixed order of summation, so two launches on
 * the same inputs agree bit for bit.  Needs A >= 5 and N <= 2048 (a structure's four used slots are staged in LDS, 52 bytes
 * per residue); a longer chain is refused with hipErrorInvalidValue.  One kernel, one dispatch arm.
 */
int ps_inter_residue_geometry_backward_f32(const float* xyz, const uint8_t* atom_mask,
                                           const float* g_d_ca, const float* g_d_cb, const float* g_d_no,
                                           const float* g_omega, const float* g_theta, const float* g_phi,
                                           float* grad_xyz, int B, int N, int A, void* stream);

/*
 * K13 (ABI 11) -- frame-aligned point error (FAPE; AlphaFold 2 suppl. alg. 28), fused: no (B,N,M) pair tensor exists.
 * For structure b with frames (R_i, t_i), i < N (rot (B,N,3,3) row-major with the basis vectors as columns, as
 * ps_frames_f32 writes them; trans (B,N,3)), points x_j, j < M (pts (B,M,3)) and the same for the target (_t):
 *   u_ij = R_i^T (x_j - t_i)    u'_ij = R'_i^T (x'_j - t'_i)    d_ij = sqrt(|u_ij - u'_ij|^2 + eps)
 *   loss[b] = (1 / scale) * sum_ij f_i p_j min(d_ij, clamp[b]) / max(sum_ij f_i p_j, 1)
 * f = frame_mask (B,N), p = point_mask (B,M), one byte each, NULL = all present; clamp (B,) fp32 on the device, +inf =
 * unclamped; scale > 0, eps >= 0.  count[b] = sum_ij f_i p_j as fp32 (exact below 2^24 pairs).  A structure without a
 * valid pair has loss 0.  Masked frames and points are dropped by selection: NaN there never reaches the result.  Points
 * may be any (B,M,3) view of coordinates, e.g. all N*A atom slots with the atom mask as point_mask: masked points are
 * compacted away while a tile is staged, at no cost to the pair loop.
 * partials: caller-owned scratch of B * ceil(N / PS_FAPE_FRAME_TILE) doubles (one partial sum per workgroup; a second
 * small launch adds them in index order).  The sums run over min(d_ij, clamp) - min(sqrt(eps), clamp), the excess over
 * the value of a perfectly placed point, which is added back once at the end: a structure compared with itself gives
 * sqrt(eps) / scale exactly.  No atomics, fixed summation order: bit-for-bit repeatable.  Any N and M.
 * B <= 65535; N, M <= 2^30.
 */
#define PS_FAPE_FRAME_TILE 64
int ps_fape_f32(const float* rot_p, const float* trans_p, const float* pts_p,
                const float* rot_t, const float* trans_t, const float* pts_t,
                const uint8_t* frame_mask, const uint8_t* point_mask, const float* clamp,
                float scale, float eps, float* loss, float* count, double* partials,
                int B, int N, int M, void* stream);

/*
 * K14 (ABI 11) -- backward pass of ps_fape_f32 with respect to the predicted side (the target is a constant), in one
 * launch that recomputes every pair; nothing is saved from the forward.  With
 *   w_ij = grad_loss[b] f_i p_j [d_ij < clamp[b]] / (scale * max(count[b], 1))   and   e_ij = (u_ij - u'_ij) / d_ij:
 *   grad_pts[b][j]   =  sum_i w_ij R_i e_ij
 *   grad_trans[b][i] = -R_i sum_j w_ij e_ij
 *   grad_rot[b][i]   =  sum_j w_ij (x_j - t_i) e_ij^T        (unconstrained 3x3)
 * Any of the three outputs may be NULL (not all): the frame-owned workgroups (grad_rot, grad_trans) or the point-owned
 * ones (grad_pts) are then not launched.  Every element of a given output is written; masked frames and points, and
 * every entry of a structure without a valid pair, receive exact zeros by selection (NaN coordinates, rotations or
 * translations at a masked frame or point never reach an output).  Owner-computes on both sides: no atomics, fixed
 * summation order, bit-for-bit repeatable.  Limits as ps_fape_f32.  With eps = 0 a valid pair with u_ij == u'_ij has
 * d_ij = 0 and no derivative (0 * inf): its owners' rows come out NaN, as under autograd; use eps > 0 where prediction
 * and target can coincide.
 */
int ps_fape_backward_f32(const float* rot_p, const float* trans_p, const float* pts_p,
                         const float* rot_t, const float* trans_t, const float* pts_t,
                         const uint8_t* frame_mask, const uint8_t* point_mask, const float* clamp,
                         float scale, float eps, const float* grad_loss,
                         float* grad_rot, float* grad_trans, float* grad_pts,
                         int B, int N, int M, void* stream);

/*
 * K15 (ABI 12) -- lDDT (local distance difference test) per point, fused: no (B,M,M) tensor exists.  For structure b
 * with predicted points x_i and target points x'_i, i < M (pts_p, pts_t (B,M,3)), p = point_mask (B,M), one byte each,
 * NULL = all present, and groups (B,M) int32 on the device, NULL = none:
 *   d_ij = sqrt(|x_i - x_j|^2 + eps)    d'_ij likewise on the target    delta_ij = |d_ij - d'_ij|
 *   c_ij = p_i p_j [i != j] [groups_i != groups_j, when groups are given] [d'_ij < cutoff]
 *   e_ij = (1/T) sum_t [delta_ij < thresholds[t]]             (smooth == 0: the metric)
 *   e_ij = (1/T) sum_t sigmoid(thresholds[t] - delta_ij)      (smooth != 0: AlphaFold 3 suppl. alg. 27)
 *   S[b][i] = sum_j c_ij e_ij        count[b][i] = sum_j c_ij
 * S and count are (B,M) fp32; count is integer-valued (exact below 2^24 pairs per point).  A score is S / max(count, 1):
 * a point without an included pair has S = 0 and count = 0, never 1 or NaN.  thresholds is a HOST array of T floats,
 * 1 <= T <= PS_LDDT_MAX_THRESHOLDS, strictly increasing, each in (0, PS_LDDT_MAX_THRESHOLD]; cutoff > 0 and eps >= 0,
 * finite.  The inclusion test is evaluated as |x'_i - x'_j|^2 + eps < cutoff^2 in fp32 (no square root; the same bits for
 * (i, j) and (j, i)), so a target pair within fp32 rounding of the cutoff may fall on either side.  Masked points are
 * dropped by selection -- they are compacted away while a tile is staged, NaN there never reaches an output -- and get
 * S = count = 0.  pts may be any (B,M,3) view of coordinates, e.g. all N*A atom slots with the atom mask as point_mask
 * and the residue index as groups.  Owner-computes, PS_LDDT_POINT_TILE points per workgroup; no atomics, fixed
 * summation order: bit-for-bit repeatable.  Any M.  B <= 65535; M <= 2^30.
 */
#define PS_LDDT_POINT_TILE 64
#define PS_LDDT_MAX_THRESHOLDS 8
#define PS_LDDT_MAX_THRESHOLD 64.0f
int ps_lddt_f32(const float* pts_p, const float* pts_t, const uint8_t* point_mask, const int32_t* groups,
                float cutoff, const float* thresholds, int T, int smooth, float eps,
                float* S, float* count, int B, int M, void* stream);

/*
 * K16 (ABI 12) -- backward pass of the smooth form of ps_lddt_f32 with respect to the predicted points (the target is a
 * constant), in one launch that recomputes every pair; nothing is saved from the forward.  With w = grad_S (B,M) =
 * dL/dS, s_t = sigmoid(thresholds[t] - delta_ij) and e'(delta) = -(1/T) sum_t s_t (1 - s_t):
 *   grad_pts[b][i] = sum_j c_ij (w_i + w_j) e'(delta_ij) sign(d_ij - d'_ij) (x_i - x_j) / d_ij
 * with sign(0) = 0, as under autograd: a prediction equal to its target has an exactly zero gradient.  c is symmetric, so
 * this is one row sweep per owner: no atomics, fixed summation order, bit-for-bit repeatable.  Every element of grad_pts
 * (B,M,3) is written; masked points get exact zeros by selection (NaN coordinates or NaN grad_S there never reach an
 * output).  Arguments and limits as ps_lddt_f32.  With eps = 0 an included pair of coincident predicted points has
 * d_ij = 0 and no derivative (0 * inf): its owners' rows come out NaN, as under autograd; keep eps > 0.
 */
int ps_lddt_backward_f32(const float* pts_p, const float* pts_t, const uint8_t* point_mask, const int32_t* groups,
                         float cutoff, const float* thresholds, int T, float eps,
                         const float* grad_S, float* grad_pts, int B, int M, void* stream);

/*
 * K17 (ABI 13) -- steric clash energy per point (AlphaFold 2 suppl. 1.9.11, eq. 46), fused: no (B,M,M) tensor exists.
 * For structure b with points x_i, i < M (pts (B,M,3)), radius (B,M) fp32, p = point_mask (B,M), one byte each, NULL =
 * all present, and groups, link (B,M) int32 on the device, NULL = none:
 *   d_ij = sqrt(|x_i - x_j|^2 + eps)          s_ij = radius_i + radius_j - tolerance
 *   c_ij = p_i p_j [i != j] [groups_i != groups_j, when given] [not (link_i == link_j and link_i >= 0), when given]
 *   v_ij = max(0, s_ij - d_ij)
 *   E[b][i] = sum_j c_ij v_ij                 count[b][i] = sum_j c_ij [v_ij > 0]
 * E and count are (B,M) fp32; count is integer-valued.  Every clashing pair appears in both owners' sums.  link expresses
 * covalent bonds between groups: two points that carry the same non-negative id never clash.  Whether a pair is evaluated
 * at all is decided in fp32 without a square root, [s_ij > 0 and |x_i - x_j|^2 + eps < s_ij^2] (the same bits for (i, j)
 * and (j, i)), so a pair within fp32 rounding of s_ij = d_ij may fall on either side -- its v is that small; the pairs
 * that pass are evaluated in double (v is a difference of nearly equal numbers), E is accumulated in double and rounded
 * once.  Masked points are dropped by selection -- they are compacted away while a tile is staged, NaN coordinates or
 * radii there never reach an output -- and get E = count = 0.  pts may be any (B,M,3) view of coordinates, e.g. all N*A
 * atom slots with the atom mask as point_mask and the residue index as groups.  Owner-computes, PS_CLASH_POINT_TILE
 * points per workgroup; no atomics, fixed summation order: bit-for-bit repeatable.  Any M.  B <= 65535; M <= 2^30;
 * tolerance finite; eps >= 0 and finite.
 */
#define PS_CLASH_POINT_TILE 64
int ps_clash_f32(const float* pts, const float* radius, const uint8_t* point_mask, const int32_t* groups,
                 const int32_t* link, float tolerance, float eps,
                 float* E, float* count, int B, int M, void* stream);

/*
 * K18 (ABI 13) -- backward pass of ps_clash_f32 with respect to the points (the radii are constants), in one launch that
 * recomputes every pair; nothing is saved from the forward.  With w = grad_E (B,M) = dL/dE:
 *   grad_pts[b][i] = - sum_j c_ij [v_ij > 0] (w_i + w_j) (x_i - x_j) / d_ij
 * with relu'(0) = 0, as under autograd.  c and the test are symmetric, so this is one row sweep per owner: no atomics,
 * fixed summation order, bit-for-bit repeatable.  Every element of grad_pts (B,M,3) is written; masked points get exact
 * zeros by selection (NaN coordinates, radii or grad_E there never reach an output).  Arguments and limits as
 * ps_clash_f32.  With eps = 0 a counted pair of coincident points has d_ij = 0 and no derivative (0 / 0): its owners' rows
 * come out NaN, as under autograd; keep eps > 0.
 */
int ps_clash_backward_f32(const float* pts, const float* radius, const uint8_t* point_mask, const int32_t* groups,
                          const int32_t* link, float tolerance, float eps,
                          const float* grad_E, float* grad_pts, int B, int M, void* stream);

/*
 * K19 (ABI 13) -- peptide-bond geometry at every junction r -> r+1 (AlphaFold 2 suppl. 1.9.11, eq. 44-45).  xyz
 * (B,N,A,3); junction_mask (B,N), one byte each, entry r = the junction from residue r to residue r+1, NULL = every
 * junction valid (entry N-1 is ignored and taken as 0); next_is_proline (B,N) bytes, entry r = residue r+1 is a proline,
 * NULL = none (ignored where the mask is 0).  n_slot, ca_slot, c_slot: three different atom slots in [0, A).  constants:
 * a HOST array of PS_PEPTIDE_BOND_CONSTANTS floats (l0, sigma_l, l0_pro, sigma_l_pro, cos_cacn, sigma_cacn, cos_cnca,
 * sigma_cnca, tau, eps, 0, 0), all finite, the sigmas, tau and eps non-negative.  With C, CA of residue r, N', CA' of
 * residue r+1 and unit(v) = v / sqrt(|v|^2 + eps):
 *   l  = sqrt(|N' - C|^2 + eps)           viol[b][r][0] = max(0, |l  - l0|       - tau * sigma_l)
 *   ca = unit(CA - C) . unit(N' - C)      viol[b][r][1] = max(0, |ca - cos_cacn| - tau * sigma_cacn)
 *   cn = unit(C - N') . unit(CA' - N')    viol[b][r][2] = max(0, |cn - cos_cnca| - tau * sigma_cnca)
 * with (l0_pro, sigma_l_pro) in place of (l0, sigma_l) where next_is_proline is set.  viol is (B,N,3) fp32, every element
 * written; invalid junctions and row N-1 get exact zeros by selection, whatever NaN sits there.  One lane per junction,
 * evaluated in double and rounded once.  B * N <= 2^31.
 */
#define PS_PEPTIDE_BOND_CONSTANTS 12
int ps_peptide_bond_f32(const float* xyz, const uint8_t* junction_mask, const uint8_t* next_is_proline,
                        int n_slot, int ca_slot, int c_slot, const float* constants,
                        float* viol, int B, int N, int A, void* stream);

/*
 * K20 (ABI 13) -- backward pass of ps_peptide_bond_f32: grad_xyz (B,N,A,3) from grad_viol (B,N,3).  One lane per residue
 * recomputes its two junctions (r-1 -> r and r -> r+1) and writes the residue's whole (A,3) row -- slots it does not read
 * get zeros -- so there are no atomics and the result repeats bit for bit; correct at chain ends and at N = 1.  |.| and
 * max(0, .) have derivative 0 at the kink.  An invalid junction contributes exact zeros, and neither the coordinates nor
 * grad_viol are read there.  Arguments and limits as ps_peptide_bond_f32.
 */
int ps_peptide_bond_backward_f32(const float* xyz, const uint8_t* junction_mask, const uint8_t* next_is_proline,
                                 int n_slot, int ca_slot, int c_slot, const float* constants,
                                 const float* grad_viol, float* grad_xyz, int B, int N, int A, void* stream);

/*
 * K21 (ABI 14) -- backbone hydrogen bonds of DSSP (Kabsch & Sander 1983, with the two-best-partners rule of the DSSP
 * programs), fused: no (B,N,N) tensor exists.  xyz (B,N,A,3); complete, junction, donor (B,N), one byte each: complete[r]
 * = residue r has its N, CA, C and O and is in the residue mask; junction[r] = r -> r+1 is a peptide bond between two
 * complete residues (entry N-1 is ignored and taken as 0); donor[r] =
 * residue r can donate its amide hydrogen (0 for proline), NULL = every residue.  n_slot, ca_slot, c_slot, o_slot: four
 * different atom slots in [0, A).  Residue j has an amide hydrogen iff junction[j-1], complete[j] and donor[j]:
 *   H_j = N_j + (C_{j-1} - O_{j-1}) / |C_{j-1} - O_{j-1}|
 * For the acceptor C=O of residue i and the donor N-H of residue j, both complete, j with an H, i != j, j != i+1 and
 * |CA_i - CA_j| < 9:
 *   E(i,j) = 27.888 (1/d(O_i,N_j) + 1/d(C_i,H_j) - 1/d(O_i,H_j) - 1/d(C_i,N_j))  kcal/mol
 * and E = -9.9 where one of the four distances is below 0.5.  Energies are not rounded to 0.001.  Every donor keeps its two
 * lowest energies among those below -0.5, ties to the lower acceptor index: acceptor_idx[b][j][0..1] (int32) and
 * acceptor_energy[b][j][0..1] (fp32); every acceptor likewise its two best donors: donor_idx[b][i][0..1], donor_energy.
 * An empty slot holds index -1 and energy 0; every element of the four (B,N,2) outputs is written.  The CA test is taken
 * in fp32 on the squared distance; the pairs that pass are evaluated in double (the coordinates are fp32 values, so their
 * differences are exact; H is computed in double) and rounded to fp32 once.  Incomplete residues are compacted away while
 * a tile is staged: NaN coordinates there never reach arithmetic.  Owner-computes, PS_DSSP_RESIDUE_TILE residues per
 * workgroup; no atomics, one fixed order per list: bit-for-bit repeatable.  B <= 65535; N <= 2^24; A >= 4.
 */
#define PS_DSSP_RESIDUE_TILE 64
int ps_backbone_hbonds_f32(const float* xyz, const uint8_t* complete, const uint8_t* junction, const uint8_t* donor,
                           int n_slot, int ca_slot, int c_slot, int o_slot,
                           int32_t* acceptor_idx, float* acceptor_energy, int32_t* donor_idx, float* donor_energy,
                           int B, int N, int A, void* stream);

/*
 * K22 (ABI 14) -- DSSP secondary-structure labels from the kept hydrogen bonds: codes (B,N) int8, indices into "-HBEGITS".
 * acceptor_idx (B,N,2) int32 as ps_backbone_hbonds_f32 writes it (an index outside [0, N) is no partner); xyz, complete
 * and junction as there; only the CA slot of xyz is read.  With hb(i,j) = "i is in donor j's kept list" and cont(i,k) =
 * "junction[i .. i+k-1] are all set":
 *   n-turn at i (n = 3, 4, 5): cont(i,n) and hb(i,i+n)
 *   G, H, I on residues i .. i+n-1 where an n-turn sits at both i-1 and i;  T on i+1 .. i+n-1 of any n-turn
 *   bridge(i,j): |i-j| >= 3, cont(i-1,2), cont(j-1,2) and
 *     parallel [hb(i-1,j) and hb(j,i+1)] or [hb(j-1,i) and hb(i,j+1)], or
 *     antiparallel [hb(i,j) and hb(j,i)] or [hb(i-1,j+1) and hb(j-1,i+1)]
 *   E: residue i has a bridge (i,j) whose neighbour pair -- (i-1,j-1) or (i+1,j+1) for parallel, (i-1,j+1) or (i+1,j-1) for
 *   antiparallel -- is a bridge of the same type;  B: a bridge and not E;  ladders are not joined across beta-bulges
 *   S: cont(i-2,4) and the angle between CA_i - CA_{i-2} and CA_{i+2} - CA_i above 70 degrees
 * The label is the first of H, B, E, G, I, T, S that holds (a pure per-residue priority), else '-'; incomplete residues
 * get 0.  One workgroup per structure with the lists and flags in LDS, O(N): N <= PS_DSSP_MAX_RESIDUES; B * N <= 2^31.
 */
#define PS_DSSP_MAX_RESIDUES 2048
int ps_dssp_assign(const float* xyz, const uint8_t* complete, const uint8_t* junction, const int32_t* acceptor_idx,
                   int ca_slot, int8_t* codes, int B, int N, int A, void* stream);

/*
 * K23 (ABI 15) -- solvent-accessible surface area by Shrake & Rupley (1973), fused: no pair list and no (B,M,M) or
 * (B,M,S) tensor exists.  points (B,M,3); radius (B,M); point_mask (B,M), one byte each, NULL = every point; isolate
 * (B,M) int32, NULL = none: two points see each other only where their keys are equal (e.g. the chain index, to measure
 * every chain alone); sphere (S,3): the directions of the test points, a DEVICE array (unit vectors; |u_k| need be 1
 * only to rounding, and any other length is honoured as given); probe: the solvent radius.  With
 * R_i = (double)radius_i + (double)probe:
 *   p_ik = x_i + R_i u_k
 *   buried(i,k) iff some j != i exists, i and j both in the mask, isolate_i == isolate_j when given, |p_ik - x_j|^2 < R_j^2
 *   count[b][i] = the number of k that are not buried (int32)      area[b][i] = 4 pi R_i^2 count / S (fp32)
 * Atoms of the same residue occlude each other: there are no group or link exclusions.  A pair is dropped in fp32 only
 * where |x_i - x_j|^2 > (R_i + R_j)^2 (1 + 2^-20), which no pair that buries a point satisfies; the pairs that pass are
 * evaluated in double as q = R_i u_k - (x_j - x_i), q.q < R_j^2 (the coordinates and radii are fp32 values, so the
 * differences are exact; |u_k|^2 is carried, never taken as 1), and the area is computed in double and rounded once.
 * Masked points are compacted away while a tile is staged -- NaN coordinates or radii there never reach arithmetic -- and
 * get count = area = 0.  Owner-computes, PS_SASA_POINT_TILE points per workgroup, a mask of PS_SASA_MAX_SPHERE_POINTS
 * bits per owner in registers; no atomics: bit-for-bit repeatable.  Any M.  B <= 65535; M <= 2^24; 1 <= S <=
 * PS_SASA_MAX_SPHERE_POINTS; probe >= 0 and finite.
 */
#define PS_SASA_POINT_TILE 64
#define PS_SASA_MAX_SPHERE_POINTS 256
int ps_solvent_accessibility_f32(const float* points, const float* radius, const uint8_t* point_mask,
                                 const int32_t* isolate, const float* sphere, float probe,
                                 int32_t* count, float* area, int B, int M, int S, void* stream);

/*
 * K24 (ABI 16) -- k nearest neighbours, fused: for every query point its k nearest candidate points of the same
 * structure, sorted by distance; no (B,Q,M) tensor exists.  points (B,M,3); point_mask (B,M), one byte each, NULL = every
 * point; queries (B,Q,3), NULL = the points themselves (the self graph: Q must equal M and query_mask and query_exclude
 * must be NULL -- they are point_mask and exclude); query_mask (B,Q), NULL = every query; exclude (B,M) and query_exclude
 * (B,Q) int32, both or neither: a candidate is skipped for a query with an equal key (the residue index for atom graphs,
 * the chain index for interface graphs); 1 <= k <= PS_KNN_MAX_K; cutoff > 0, +inf = none; include_self: the self graph
 * only -- without it candidate j == q is skipped.  With X = (double)x:
 *   dx = Xj.x - Xq.x, dy, dz likewise       d2 = (dx*dx + dy*dy) + dz*dz       in double, in exactly this order
 *   j is a neighbour of q iff both are in their masks, their keys differ where keys are given, j != q in the self graph
 *   unless include_self, d2 is finite, and d2 <= C2 = (double)cutoff * (double)cutoff
 *   the neighbours ordered by (d2, j) ascending -- equal distances go to the lower index --, the first k kept
 *   idx[b][q][0..k-1] (int32, into the M axis; padding -1)      dist[b][q][0..k-1] = (float)sqrt(d2) (padding +inf)
 *   count[b][q] = the number of real neighbours, at most k (int32)
 * Every element of the three outputs is written; a masked query gets count 0 and all padding.  The library is built with
 * -ffp-contract=off, which is part of the definition: a float64 restatement gives the same bits.  A NaN or infinite
 * coordinate makes d2 non-finite, so such a point is nobody's neighbour and such a query has none; masked points are
 * compacted away while a tile is staged, so NaN there never reaches arithmetic.  A column is dropped in fp32 only where
 * fl32(|xj - xq|^2) > fl32(tau) (1 + 2^-20) + 2^-126, tau the owner's current k-th best d2 (C2 until it has k), which no pair
 * the double test keeps satisfies; the pairs that pass are decided in double.  Each wave owns 64 queries, one max-heap of k
 * entries per query in LDS; no atomics, one fixed order per list: bit-for-bit repeatable.  Any M and Q.  B <= 65535;
 * M, Q <= 2^24; cutoff not NaN.
 */
#define PS_KNN_MAX_K 64
int ps_nearest_neighbors_f32(const float* points, const uint8_t* point_mask, const float* queries,
                             const uint8_t* query_mask, const int32_t* exclude, const int32_t* query_exclude,
                             int k, float cutoff, int include_self, int32_t* idx, float* dist, int32_t* count,
                             int B, int M, int Q, void* stream);

/*
 * K25 (additive to ABI 16: a new symbol changes no signature) -- radial basis functions of the atom-pair distances along
 * the edges of a neighbour graph, fused: no gathered (B,N,k,A,3) tensor and no broadcast (B,N,k,P,R) intermediate exists.
 * xyz (B,N,A,3); atom_mask (B,N,A), one byte each, NULL = every atom; idx (B,N,k) int32, the neighbour lists of K24 on the
 * same N axis: ANY entry outside [0, N) is padding, not only -1, so no value in idx makes the kernel read out of bounds.
 * pair_i[p], pair_j[p], p < P: the atom slot on the source residue i and on the neighbour j; centers[c], c < R: HOST
 * arrays, read and validated before the call returns.  1 <= k <= PS_KNN_MAX_K, 1 <= P <= PS_EDGE_MAX_PAIRS,
 * 1 <= R <= PS_EDGE_MAX_RBF, slots in [0, A), sigma > 0 and finite with sqrt(log2 e) / sigma a normal float32;
 * B <= 65535, N <= 2^24.  Outputs, either may be NULL, not both: dist (B,N,k,P) and rbf (B,N,k,P*R), element [p*R + c].
 * For the edge (i, s), j = idx[b][i][s], with X = (double)x:
 *   dx = Xj.x - Xi.x, dy, dz likewise     d2 = (dx*dx + dy*dy) + dz*dz in double, in exactly this order
 *   dist = (float)sqrt(d2), as K24's: defined bit for bit (the library is built with -ffp-contract=off)
 *   rbf[p*R + c] = exp(-z*z), z = (dist - centers[c]) / sigma, evaluated in fp32: within 1e-6 absolute of that expression
 *   in float64 on the fp32 dist, centers and sigma (evaluated as exp2(-(w*w)), w = (dist - centers[c]) * fl32(sqrt(log2 e) /
 *   sigma): under 2e-7 by analysis).
 * dist and rbf are exactly 0 where the edge is padding or either atom of the pair is outside atom_mask; coordinates
 * there are never read, so NaN under a mask never reaches arithmetic; an unmasked NaN propagates.  Every output element
 * is written (the caller need not clear them), from any 4-byte aligned base -- 16-byte stores start at the first 16-byte
 * boundary of each row's actual address --; all output offsets are 64-bit.  No atomics: two calls agree bit for bit.
 */
#define PS_EDGE_MAX_PAIRS 64
#define PS_EDGE_MAX_RBF 64
int ps_edge_rbf_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* idx, const int32_t* pair_i,
                    const int32_t* pair_j, int P, const float* centers, int R, float sigma, float* dist, float* rbf,
                    int B, int N, int A, int k, void* stream);

/*
 * K26 (additive to ABI 16) -- the neighbour's frame in the source residue's frame along the edges of a neighbour graph.
 * Frames as in K4 and K13: rot (B,N,3,3) row-major with the basis vectors as columns, trans (B,N,3); frame_mask (B,N),
 * one byte each, NULL = every frame; idx (B,N,k) int32 as for K25 (any entry outside [0, N) is padding).  Outputs, either
 * may be NULL, not both: local_pos (B,N,k,3) = R_i^T (t_j - t_i) and rel_rot (B,N,k,3,3) = R_i^T R_j, in double on the
 * fp32 inputs in exactly this order, each value rounded to fp32 once:
 *   v = t_j - t_i
 *   local_pos[c]  = (R_i[0][c]*v0 + R_i[1][c]*v1) + R_i[2][c]*v2
 *   rel_rot[a][c] = (R_i[0][a]*R_j[0][c] + R_i[1][a]*R_j[1][c]) + R_i[2][a]*R_j[2][c]
 * Exactly 0 at the padding and where i or j is outside frame_mask (frames there are never read); every element is
 * written.  rot and trans are both required.  1 <= k <= PS_KNN_MAX_K; B <= 65535, N <= 2^24.  Deterministic.
 */
int ps_edge_frames_f32(const float* rot, const float* trans, const uint8_t* frame_mask, const int32_t* idx,
                       float* local_pos, float* rel_rot, int B, int N, int k, void* stream);

/*
 * K27 - K30 (additive to ABI 16) -- side-chain torsions: the chi angles of every residue, measured and set, with both
 * gradients.  The kernels know no amino acids; two HOST tables, read and validated before the call returns, say what an
 * angle is: chi_atoms (T,4,4) int32, the atom slots a, b, c, d of angle k of residue type t -- all -1 (no such angle) or
 * four distinct slots in [0, A) --, and chi_last (T,4) int32: angle k turns the slots [d, last]; -1 (measured, never
 * turned), or in [d, A) with none of a, b, c inside [d, last].  1 <= T <= PS_CHI_MAX_TYPES.  xyz (B,N,A,3);
 * residue_type (B,N) int32, the table row of each residue: a value outside [0, T) is padding, which has no angles and
 * never indexes the table; atom_mask (B,N,A), one byte each, NULL = every atom.  Angle k of a residue is DEFINED where
 * the table has it and all four atoms are in the mask; coordinates outside the mask never reach arithmetic.  All
 * arithmetic is in double on the fp32 values, in the order written here (the library is built with -ffp-contract=off),
 * with u x v = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x) and u . v = (u.x v.x + u.y v.y) + u.z v.z.
 * One lane owns one residue; no atomics: every result repeats bit for bit.  Every tensor may start at any 4-byte
 * aligned address.  B * N <= 2^31; 1 <= A <= 64; B = 0 or N = 0 launches nothing.
 *
 * K27, ps_chi_f32: chi (B,N,4) fp32 and chi_mask (B,N,4) bytes; either may be NULL, not both.
 *   b0 = a - b     b1 = c - b     b2 = d - c     n1 = b0 x b1     n2 = b2 x b1     m = n1 x n2
 *   x = n1 . n2    y = (m . b1) / sqrt(b1 . b1)  chi = (float)atan2(y, x)       -- the sign of mode 1 of ps_pointwise_f32, IUPAC
 * An undefined angle gives exact 0 and mask 0.
 *
 * K28, ps_chi_backward_f32: grad_xyz (B,N,A,3) from grad_chi (B,N,4).  With l = sqrt(b1 . b1), p = (b0 . b1) / (b1 . b1),
 * q = (b2 . b1) / (b1 . b1):
 *   ga = (l / (n1 . n1)) n1     gd = -(l / (n2 . n2)) n2     gb = (p - 1) ga + q gd     gc = -(p ga) - (1 + q) gd
 * each times (double)grad_chi[k]; an atom's contributions are summed in the order k = 0..3 and rounded once.  The whole
 * (A,3) row of every residue is written, exact zeros in the slots no defined angle reads; grad_chi is not read at an
 * undefined angle.
 */
#define PS_CHI_MAX_TYPES 32
int ps_chi_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* residue_type, const int32_t* chi_atoms, int T,
               float* chi, uint8_t* chi_mask, int B, int N, int A, void* stream);
int ps_chi_backward_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* residue_type,
                        const int32_t* chi_atoms, int T, const float* grad_chi, float* grad_xyz, int B, int N, int A,
                        void* stream);

/*
 * K29, ps_chi_set_f32: out (B,N,A,3), the coordinates with the chi angles turned to chi (B,N,4) -- by chi if relative is
 * non-zero.  chi_select (B,N,4), one byte each, NULL = every angle.  For k = 0, 1, 2, 3 in this order, where angle k is
 * defined, chi_last[t][k] >= 0 and chi_select is NULL or non-zero, on the residue's CURRENT coordinates (doubles between
 * the steps):
 *   delta = (double)chi[k] - phi, phi the angle of K27 before its rounding;   delta = (double)chi[k] if relative
 *   e = c - b     u = e / sqrt(e . e)     cs = cos(delta)     sn = sin(delta)
 *   for every slot s in [d, last] inside the mask:   v = p_s - c     p_s = ((c + v cs) + (u x v) sn) + u ((u . v) (1 - cs))
 * Each result is rounded to fp32 once, at the store.  Every other float of out, and every float of a residue with nothing
 * to turn, is the input's bit pattern -- the NaN of a missing atom, the padding.  chi[k] is not read where it is not
 * used.  out may not alias xyz.
 *
 * K30, ps_chi_set_backward_f32: grad_chi (B,N,4) from grad_out (B,N,A,3) and the coordinates `out` that K29 wrote, with
 * K29's atom_mask, residue_type, tables and chi_select:
 *   grad_chi[k] = sum over the slots s in [d, last] inside the mask, in slot order, of (u x (p_s - c)) . g_s
 * with u and c of angle k as above, on `out`; exact 0 at an angle K29 did not turn.  This is the whole derivative in both
 * modes: a turn about an inner axis carries the outer axes along rigidly.  xyz is a constant of K29.
 */
int ps_chi_set_f32(const float* xyz, const uint8_t* atom_mask, const int32_t* residue_type, const int32_t* chi_atoms,
                   const int32_t* chi_last, int T, const float* chi, const uint8_t* chi_select, int relative,
                   float* out, int B, int N, int A, void* stream);
int ps_chi_set_backward_f32(const float* out, const uint8_t* atom_mask, const int32_t* residue_type,
                            const int32_t* chi_atoms, const int32_t* chi_last, int T, const uint8_t* chi_select,
                            const float* grad_out, float* grad_chi, int B, int N, int A, void* stream);

/*
 * Rigid-body ops.  ps_rigid_f32 replaces StructureBatch.translate,
 * rotate, center_at and get_local_xyz (protstruc.py:662-694, :759-788, :347-362):
 *   out = R x + t   (transpose = 0)   or   out = R^T x + t   (transpose = 1)
 * r_mode: 0 none, 1 one shared 3x3, 2 per structure (B,3,3), 3 per residue (B,N,3,3);
 * t_mode: 0 none, 1 one shared (3), 2 per structure (B,3), 3 per residue (B,N,3),
 *         4 per atom (B,N,A,3).  xyz_out may alias xyz_in.
 */
int ps_rigid_f32(const float* xyz_in, float* xyz_out, const float* R, int r_mode, int transpose,
                 const float* t, int t_mode, int B, int N, int A, void* stream);

/* Replaces StructureBatch.center_of_mass (protstruc.py:746-757): com[b] = nanmean over residues of xyz[b][:][atom]. */
int ps_center_of_mass_f32(const float* xyz, float* com, int B, int N, int A, int atom, void* stream);

/*
 * Replaces the coordinate construction of StructureBatch.from_backbone_orientations_translations
 * (protstruc.py:289-312): xyz[b][n][a] = rot[b][n] * ideal[a] + trans[b][n] for a < n_ideal, 0 for
 * the remaining slots.  ideal is a device array (n_ideal, 3).
 */
int ps_frames_to_backbone_f32(const float* rot, const float* trans, const float* ideal, int n_ideal,
                              float* xyz, int B, int N, int A, void* stream);

/*
 * K7 (ABI 6) -- backbone coordinates from dihedral angles: the inverse of ps_backbone_dihedrals, behind
 * StructureBatch.from_backbone_dihedrals (the reference's from_dihedrals is a TODO, protstruc.py:321-339).
 *   dihedrals[b][i]    = (phi_i, psi_i, omega_i) in ps_backbone_dihedrals_f32's layout;
 *   bond_angles[b][i]  = (N_i-CA_i-C_i, CA_i-C_i-N_i+1, C_i-N_i+1-CA_i+1), radians  (NULL: 1.937, 116.2 deg, 121.7 deg);
 *   bond_lengths[b][i] = (|N_i-CA_i|, |CA_i-C_i|, |C_i-N_i+1|), Angstrom          (NULL: 1.458, 1.523, 1.329);
 *   chain_idx (B,N) fp32 and residue_mask (B,N) bytes are optional (NULL: one chain, every residue present).
 * A segment starts at i = 0, where chain_idx changes (NaN != NaN) and after a residue whose mask is 0; each segment's
 * first residue sits at the ideal position (CA at the origin, C on +x, N in the xy-plane with y > 0), and
 *   N_i+1 = place(N_i, CA_i, C_i, |C-N|, CA-C-N, psi_i),  CA_i+1 = place(CA_i, C_i, N_i+1, |N-CA|, C-N-CA, omega_i),
 *   C_i+1 = place(C_i, N_i+1, CA_i+1, |CA-C|, N-CA-C, phi_i+1)   (place = mode 3 of ps_pointwise_f32).
 * phi at a segment's first residue and psi / omega at its last are never read into the result.  Evaluated as a
 * segmented prefix scan of per-residue rigid transforms (error growing with log N, not N).  Writes every byte of
 * xyz (B,N,A,3) -- slots 0/1/2 = N/CA/C, slot 4 = CB when include_cb (A >= 5), zeros elsewhere and for masked
 * residues -- and atom_mask (B,N,A) fp32 1 / 0.  Deterministic (no atomics).
 */
int ps_backbone_from_dihedrals_f32(const float* dihedrals, const float* bond_angles, const float* bond_lengths,
                                   const float* chain_idx, const uint8_t* residue_mask, float* xyz, float* atom_mask,
                                   int include_cb, int B, int N, int A, void* stream);

/*
 * K12 (ABI 10) -- backward pass of ps_backbone_from_dihedrals_f32: the vector-Jacobian product of the coordinates with
 * respect to the dihedrals, bond angles and bond lengths, in one launch and from the coordinates alone.
 *   xyz (B,N,A,3)       what the forward wrote (the same chain_idx, residue_mask, include_cb and A);
 *   grad_xyz (B,N,A,3)  the upstream gradient;
 *   grad_dihedrals, grad_bond_angles, grad_bond_lengths (B,N,3) fp32, in the forward's layouts; the last two may be NULL
 *   (not wanted: their arithmetic is skipped).  chain_idx and residue_mask may be NULL as in the forward.
 * An internal coordinate moves everything after it in its segment as a rigid body, so with the effective atom gradients
 * g (the CB gradient pushed back first: with bb = CA - N, cc = C - CA and CB = k0 (bb x cc) + k1 bb + k2 cc + CA,
 * g_bb = k0 (cc x g_CB) + k1 g_CB, g_cc = k0 (g_CB x bb) + k2 g_CB, g_N -= g_bb, g_CA += g_bb - g_cc + g_CB, g_C += g_cc)
 * and the segmented inclusive suffix sums over the backbone atoms in chain order, G[k] = sum g_a and T[k] = sum x_a x g_a
 * over the atoms a >= k of k's segment, a rotation about the unit axis u through p that moves the atoms k.. has the
 * gradient u . (T[k] - p x G[k]) and a bond length along u has u . G[k].  For residue i continuing a segment (j = i - 1):
 *   psi_j    atoms N_i..,  u = unit(C_j - CA_j), p = C_j      angle CA_j-C_j-N_i   atoms N_i..,  u = unit((CA_j - C_j) x (N_i - C_j)), p = C_j
 *   omega_j  atoms CA_i.., u = unit(N_i - C_j),  p = N_i      angle C_j-N_i-CA_i   atoms CA_i.., u = unit((C_j - N_i) x (CA_i - N_i)), p = N_i
 *   phi_i    atoms C_i..,  u = unit(CA_i - N_i), p = CA_i     angle N_i-CA_i-C_i   atoms C_i..,  u = unit((N_i - CA_i) x (C_i - CA_i)), p = CA_i
 *   |C_j-N_i|, |N_i-CA_i|, |CA_i-C_i|  atoms N_i.., CA_i.., C_i..  along unit(N_i - C_j), unit(CA_i - N_i), unit(C_i - CA_i).
 * A segment's first residue sits in the fixed frame: |N_i-CA_i| and the angle N_i-CA_i-C_i move N_i alone
 * (unit(N_i - CA_i) . g_N and unit((C_i - CA_i) x (N_i - CA_i)) . ((N_i - CA_i) x g_N)), |CA_i-C_i| moves C_i and
 * everything after it, phi_i nothing.
 * Contract.  Every element of every non-NULL output is written; entries the forward never reads (phi at a segment's
 * first residue, psi / omega / the two peptide angles / |C-N| at its last, every parameter that only moves masked
 * residues) are exact zeros.  Only slots 0, 1, 2 (and 4 with include_cb) of xyz and grad_xyz are read; rows of masked
 * residues and all other slots are excluded by selection, so NaN there never reaches the result.  No atomics and a
 * fixed order of every sum: two launches agree bit for bit.  Any N (tiles of 512 residues walked from the chain's end
 * with the running G, T carried); nothing is allocated, synchronised or read back, so the launch can be captured in a
 * graph.  B == 0 or N == 0 returns 0 without a launch.  No second derivatives.
 */
int ps_backbone_from_dihedrals_backward_f32(const float* xyz, const float* grad_xyz, const float* chain_idx,
                                            const uint8_t* residue_mask, float* grad_dihedrals, float* grad_bond_angles,
                                            float* grad_bond_lengths, int include_cb, int B, int N, int A, void* stream);

/*
 * K8 / K9 (ABI 7) -- backbone N / CA / C distance matrices from inter-residue geometry (trRosetta), behind
 * geometry.reconstruct_backbone_distmat_from_interresidue_geometry (reference geometry.py:229-347).  Three steps,
 * launched in this order on one stream:
 *
 * ps_backbone_distmat_init_f32 (K8): d_cb, omega, theta, phi (B,L,L) fp32 -> out (B,3,3,L,L) fp32, planes (a, b) with
 * atom order N, CA, C.  x = the reference's ideal_local_frame() (N, CA, C, CB).  Per pair i != j, in residue i's frame:
 *   CB' = place(N, CA, CB, d_cb[i,j], phi[i,j], theta[i,j]),   CA' = place(CA, CB, CB', |CB-CA|, phi[j,i], omega[i,j]),
 *   N'  = place(CB, CB', CA', |CA-N|, CB-CA-N, theta[j,i]),    C'  = place(CB', CA', N', |N-C|, CA-N-C, CB-CA-N-C)
 * (place = mode 3 of ps_pointwise_f32), out[a][b][i][j] = |x_a - y_b|.  omega is the trRosetta dihedral
 * (CA_i, CB_i, CB_j, CA_j), theta[i,j] = dihedral(N_i, CA_i, CB_i, CB_j), phi[i,j] = angle(CA_i, CB_i, CB_j).  Then:
 * the diagonal i = j is 0 for a = b and the ideal intra-residue distance otherwise; [C][N][i][i+1] = [N][C][i+1][i] =
 * 1.329 (the peptide bond), or MASK = 12345679 where chain_breaks[b][i] != 0; all nine planes are MASK where
 * mask[b][i][j] == 0; NaN becomes MASK and +-inf +-FLT_MAX (torch.nan_to_num).  chain_breaks (B,L) bytes ("chain ends
 * after residue i"), mask (B,L,L) bytes and lengths (B) int32 are optional (NULL: no break, every pair, L).  A residue
 * i >= lengths[b] is an inert node: 0 on its own diagonal planes (a = b, i = j), MASK everywhere else.
 *
 * ps_floyd_warshall_f32 (K9): in place on D (B,G,G,L,L) fp32 with node (g, i) = g * L + i, n = G L nodes (G = 3: the
 * distance-matrix layout above; G = 1: a plain (B,L,L) matrix), for k = 0 .. n-1 in order:
 *   D[r][c] = min(D[r][c], D[k][r] + D[k][c])     (the reference's rule, geometry.py:327-330; it reads row k only).
 * Blocked in 64-pivot panels; equal to that sequential float32 loop bit for bit when every entry is >= 0 and not NaN
 * (what K8 writes).  workspace: device memory of at least ps_floyd_warshall_workspace_bytes(B, G, L) bytes, 4-byte
 * aligned, overwritten.  Requires (G L)^2 < 2^31.
 *
 * ps_backbone_distmat_finish_f32: in place on out (B,3,3,L,L): D = (D + D^T) / 2 over the 3L nodes, then the bonds
 * again -- [N][CA][i][i] = [CA][N][i][i] = 1.458, [CA][C][i][i] = [C][CA][i][i] = 1.523, [C][N][i][i+1] =
 * [N][C][i+1][i] = 1.329 except where chain_breaks[b][i] != 0 (the reference re-bonds chain breaks here; this does not)
 * -- and NaN in every entry of a residue i >= lengths[b].
 *
 * Requires B <= 65535 and 9 L^2 < 2^31.  Deterministic (no atomics).
 */
int ps_backbone_distmat_init_f32(const float* d_cb, const float* omega, const float* theta, const float* phi,
                                 const uint8_t* mask, const uint8_t* chain_breaks, const int* lengths, float* out,
                                 int B, int L, void* stream);
/* Host-only query: the workspace ps_floyd_warshall_f32 needs, in bytes (-1 for invalid arguments). */
long long ps_floyd_warshall_workspace_bytes(int B, int G, int L);
int ps_floyd_warshall_f32(float* D, int B, int G, int L, void* workspace, long long workspace_bytes, void* stream);
int ps_backbone_distmat_finish_f32(float* D, const uint8_t* chain_breaks, const int* lengths, int B, int L,
                                   void* stream);

/*
 * K10 / K11 (ABI 8) -- backbone coordinates from a distance matrix, behind geometry.initialize_backbone_with_mds
 * (reference geometry.py:350-410).
 *
 * ps_smacof_f32 (K10): metric SMACOF (sklearn 1.7's smacof) on D (B,G,G,L,L) fp32, node (g, i) = g * L + i as in
 * ps_floyd_warshall_f32 (G = 3: a reconstructed distance matrix; G = 1: a plain (B,L,L) matrix), read in place.  With
 * lengths (B) int32 (NULL: L) only nodes with i < lengths[b] take part: n = G lengths[b].  K starts per structure,
 * init (B,K,G L,3) fp32 (entries of padded nodes are not read).  Per start, for t = 0, 1, ...:
 *   d~_ij = |x_i - x_j| (1e-5 where exactly 0),  x_i <- (1/n) sum_j (D_ij / d~_ij)(x_i - x_j)  (the Guttman transform),
 *   sigma_{t+1} = 1/2 sum_ij (d_ij - D_ij)^2,  S_{t+1} = sum_ij d_ij^2  (of the new x; float64 sums),
 * stopping after X^{t+1} when t >= 1 and (sigma_t - sigma_{t+1}) / (S_{t+1} / 2) < eps, or at t + 1 = max_iter.  The
 * start with the smallest final sigma wins (the lowest index on ties; a NaN stress never replaces an earlier start):
 * X_out (B,G L,3) fp32 (NaN for padded nodes), stress_out (B) float64, n_iter_out (B) int32.  A structure of length 0
 * gives stress 0, n_iter 0.  Issues max_iter + 2 launches on `stream` whatever the convergence (the ones after it are
 * no-ops): capturable, bitwise deterministic.  workspace: at least ps_smacof_workspace_bytes(B, K, G, L) bytes of device
 * memory, 8-byte aligned, overwritten.  Requires B <= 65535, K >= 1, max_iter >= 1, eps >= 0, (G L)^2 < 2^31 and
 * B K G L 3 < 2^31.
 *
 * ps_mds_backbone_finish_f32 (K11): X (B,3,L,3) fp32 (N, CA, C) -> out (B,n_atoms_out,L,3), n_atoms_out = 3 (N, CA, C)
 * or 5 (N, CA, C, O, CB).  mirror_mode 1: z is negated iff the mean of phi_i = dihedral(C_{i-1}, N_i, CA_i, C_i) over
 * i = 1 .. len-1 is positive (the reference's documented intent; its code mirrors unconditionally); 0: never.  Then
 * CB = place(C, N, CA, 1.522, 1.927, -2.143) and O = place(N_{(i+1) mod len}, CA, C, 1.231, 2.108, -3.142) (place = mode 3
 * of ps_pointwise_f32; the wrap at the last residue is the reference's np.roll).  Residues i >= lengths[b] are NaN; a
 * NaN anywhere in a structure's first lengths[b] residues makes that structure's whole output NaN.
 */
long long ps_smacof_workspace_bytes(int B, int K, int G, int L);
int ps_smacof_f32(const float* D, int B, int G, int L, const int* lengths, const float* init, int K, int max_iter,
                  double eps, float* X_out, double* stress_out, int* n_iter_out, void* workspace, long long workspace_bytes,
                  void* stream);
int ps_mds_backbone_finish_f32(const float* X, const int* lengths, int B, int L, int mirror_mode, int n_atoms_out,
                               float* out, void* stream);

/*
 * Batched Kabsch fit -- replaces the per-structure loop of StructureBatch.align and
 * geometry.kabsch (protstruc.py:880-918, geometry.py:442-480): R[b] (3x3), t[b] (3) minimising the RMSD of
 * R a + t against b over the atoms with atom_mask != 0.  src/dst are (B, n_atoms, 3); dst_is_shared /
 * mask_is_shared = 1 when one target / one mask serves every structure.  Apply with ps_rigid_f32.
 * The contract, for every selection with at least one atom: R is always a proper rotation (R R^T = I and
 * det R = +1 to float32 rounding; a mirror-image target gets the best rotation, never the reflection) and
 * reaches the optimal RMSD.  Where the covariance is rank-deficient (two atoms, collinear atoms) the optimum
 * is one of a family -- any turn about the line fits as well -- and R is one member of it.  One selected atom,
 * or coincident selected atoms: R = I exactly and t = b - a (the reference's SVD of the zero matrix).  No
 * selected atom (an all-zero mask, or n_atoms = 0): R and t are NaN, the reference's 0 / 0.  Atoms with
 * atom_mask = 0 are never read, so NaN may sit there.  The 3x3 solve is csrc/kabsch_solve.hpp.
 */
int ps_kabsch_f32(const float* src_xyz, const float* dst_xyz, const uint8_t* atom_mask, float* R, float* t,
                  int B, int n_atoms, int dst_is_shared, int mask_is_shared, void* stream);

/*
 * Distance of one atom slot of every residue of ONE structure to its nearest query point -- the distance
 * part of StructureBatch.get_topk_nearest_residue_mask (protstruc.py:844-849).  xyz (N,A,3), query (n_query,3).
 * A NaN query point turns every output NaN, a NaN atom its own output.  n_query = 0 is hipErrorInvalidValue
 * before any launch (the reference's min over no point raises as well); ops.min_dist_to_points raises ValueError.
 */
int ps_min_dist_to_points_f32(const float* xyz, const float* query, float* out, int N, int A, int atom,
                              int n_query, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROTSTRUC_HIP_H */
