// K7 -- backbone N, CA, C (and CB) from phi / psi / omega: the inverse of K2.  Backs
// StructureBatch.from_backbone_dihedrals, the constructor the reference documents as from_dihedrals but leaves a
// TODO (protstruc.py:321-339), with its geometry.place_fourth_atom (geometry.py:127-168) as the placement rule.
//
// NeRF is a chain of 3 N dependent placements.  Walked one atom after another in fp32, every rounding of a rotation is
// carried, with a growing lever arm, into every later atom (0.4 A at 512 strand residues).  Here the chain is a
// segmented prefix scan of per-residue rigid transforms, so every atom is at the end of a composition tree of depth
// ~log N instead of N.  One workgroup per structure, tiles of 1024 residues:
//   1. per residue i (four consecutive residues per lane): M_i, the rigid motion from residue i-1's (N, CA, C) frame to
//      residue i's -- the three placements (place4) run in i-1's local coordinates from its canonical triple, the frame
//      of the placed triple by Gram-Schmidt.  At a segment start M_i is the identity (the residue sits at the ideal
//      position: CA at the origin, C on +x, N in the xy-plane, y > 0) and carries a reset flag;
//   2. segmented inclusive scan of the 3x4 transforms, (R1,t1) o (R2,t2) = (R1 R2, R1 t2 + t1): a sequential run over
//      the lane's four residues, a wave scan with __shfl_up over 64 lanes, one cross-wave step through LDS, and the
//      running transform carried from tile to tile, so any N works without a grid-wide dependency;
//   3. F_i applied to residue i's local N / CA / C (and CB from the global N, CA, C, as ideal_backbone_coordinates
//      places it); the whole A-slot row, zeros included, and the float mask are written from LDS by the workgroup with
//      16-byte stores, so one launch writes every output byte.
// No atomics, nothing that depends on launch order: the output is the same bits on every run.
#include "ps_common.hpp"

namespace {

constexpr int NERF_THREADS = 256;
constexpr int NERF_PER_LANE = 4;
constexpr int NERF_TILE = NERF_THREADS * NERF_PER_LANE;
constexpr int NERF_WAVES = NERF_THREADS / PS_WAVE;

// geometry.IDEAL_* of the Python package, rounded from the same doubles (reference constants/ideal.py: NA, AC, C_N,
// NAC; Engh & Huber for the two peptide-bond angles, which the reference has no constant for)
constexpr double NERF_PI = 3.141592653589793;
constexpr float kNA = (float)1.458, kAC = (float)1.523, kCN = (float)1.329, kNAC = (float)1.937;
constexpr float kCACN = (float)(116.2 * (NERF_PI / 180.0)), kCNCA = (float)(121.7 * (NERF_PI / 180.0));

// a rigid transform (row-major R, t) and the segment-start flag of the scan element
struct SegRt {
    float r[9];
    float t[3];
    int reset;
};

__device__ __forceinline__ SegRt seg_identity() {
    SegRt x;
#pragma unroll
    for (int k = 0; k < 9; ++k) x.r[k] = (k % 4 == 0) ? 1.f : 0.f;
    x.t[0] = x.t[1] = x.t[2] = 0.f;
    x.reset = 0;
    return x;
}

// the scan operator: a is the earlier element.  A reset on the right discards everything before it by selection (no
// arithmetic touches the discarded prefix, so a NaN there cannot reach the result).
__device__ __forceinline__ SegRt seg_combine(const SegRt& a, const SegRt& b) {
    SegRt o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o.r[i * 3 + j] = (a.r[i * 3] * b.r[j] + a.r[i * 3 + 1] * b.r[3 + j]) + a.r[i * 3 + 2] * b.r[6 + j];
        o.t[i] = ((a.r[i * 3] * b.t[0] + a.r[i * 3 + 1] * b.t[1]) + a.r[i * 3 + 2] * b.t[2]) + a.t[i];
    }
    if (b.reset) o = b;
    o.reset = a.reset | b.reset;
    return o;
}

__device__ __forceinline__ SegRt seg_shfl_up(const SegRt& x, int delta) {
    SegRt o;
#pragma unroll
    for (int k = 0; k < 9; ++k) o.r[k] = __shfl_up(x.r[k], delta);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.t[k] = __shfl_up(x.t[k], delta);
    o.reset = __shfl_up(x.reset, delta);
    return o;
}

// residue i's canonical N in its own frame (CA at the origin, C at (|CA-C|, 0, 0)); stage 1 (for residue i-1) and
// stage 3 (for residue i) evaluate the same expression, so the two agree bit for bit
__device__ __forceinline__ f3 local_n(float len_na, float ang_nac) {
    float s, c;
    sincosf(ang_nac, &s, &c);
    return f3{len_na * c, len_na * s, 0.f};
}

struct ResParams {
    float na, ac, cn;        // |N-CA|, |CA-C|, |C-N(next)|
    float nac, cacn, cnca;   // angle N-CA-C, CA-C-N(next), C-N(next)-CA(next)
};

__device__ __forceinline__ ResParams res_params(const float* __restrict__ bond_angles,
                                                const float* __restrict__ bond_lengths, size_t res) {
    ResParams p{kNA, kAC, kCN, kNAC, kCACN, kCNCA};
    if (bond_lengths) {
        p.na = bond_lengths[res * 3];
        p.ac = bond_lengths[res * 3 + 1];
        p.cn = bond_lengths[res * 3 + 2];
    }
    if (bond_angles) {
        p.nac = bond_angles[res * 3];
        p.cacn = bond_angles[res * 3 + 1];
        p.cnca = bond_angles[res * 3 + 2];
    }
    return p;
}

// 16-byte stores of n floats at dst (4-byte aligned), value(e) for e in [0, n): scalar head up to the first 16-byte
// boundary, float4 body, scalar tail.  Every lane of the workgroup takes part.
template <typename F>
__device__ __forceinline__ void store_region(float* __restrict__ dst, unsigned n, F value) {
    const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u);
    const unsigned head = min(n, (4u - mis) & 3u);
    if (threadIdx.x < head) dst[threadIdx.x] = value(threadIdx.x);
    const unsigned nv = (n - head) >> 2;
    float4* dv = reinterpret_cast<float4*>(dst + head);
    for (unsigned q = threadIdx.x; q < nv; q += NERF_THREADS) {
        const unsigned e = head + 4 * q;
        dv[q] = make_float4(value(e), value(e + 1), value(e + 2), value(e + 3));
    }
    const unsigned tail = head + 4 * nv + threadIdx.x;
    if (tail < n) dst[tail] = value(tail);
}

// AT: the number of atom slots when it is known at compile time (15, the package's layout), 0 = the run-time A
template <int AT>
__global__ __launch_bounds__(NERF_THREADS) void k7_backbone_from_dihedrals(
    const float* __restrict__ dihedrals, const float* __restrict__ bond_angles, const float* __restrict__ bond_lengths,
    const float* __restrict__ chain_idx, const uint8_t* __restrict__ residue_mask, float* __restrict__ xyz,
    float* __restrict__ atom_mask, int include_cb, int N, int A_rt) {
    const unsigned A = AT ? (unsigned)AT : (unsigned)A_rt;
    const unsigned row = 3 * A;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const size_t base = (size_t)b * N;

    __shared__ float atoms[NERF_TILE * 12];   // per residue of the tile: N, CA, C, CB (zeros for masked residues)
    __shared__ float on[NERF_TILE];           // residue_mask as 0 / 1
    __shared__ SegRt wtot[NERF_WAVES];

    SegRt carry = seg_identity();   // composition of every earlier tile
    for (int t0 = 0; t0 < N; t0 += NERF_TILE) {
        const int nt = min(NERF_TILE, N - t0);

        // ---- stage 1 + the lane's sequential run ----
        SegRt f[NERF_PER_LANE];
#pragma unroll
        for (int j = 0; j < NERF_PER_LANE; ++j) {
            const int i = t0 + (int)threadIdx.x * NERF_PER_LANE + j;
            SegRt m = seg_identity();
            if (i < N) {
                const size_t res = base + i;
                bool start = (i == 0);
                if (!start && chain_idx) start = chain_idx[res] != chain_idx[res - 1];   // NaN != NaN: a new segment
                if (!start && residue_mask) start = residue_mask[res - 1] == 0;
                if (start) {
                    m.reset = 1;
                } else {
                    const ResParams pp = res_params(bond_angles, bond_lengths, res - 1);
                    const ResParams pc = res_params(bond_angles, bond_lengths, res);
                    const float phi = dihedrals[res * 3];
                    const float psi_prev = dihedrals[(res - 1) * 3 + 1], omega_prev = dihedrals[(res - 1) * 3 + 2];
                    // residue i-1's canonical triple; i's N, CA, C placed in i-1's frame
                    const f3 n0 = local_n(pp.na, pp.nac), a0 = mk3(0.f, 0.f, 0.f), c0 = mk3(pp.ac, 0.f, 0.f);
                    const f3 n1 = place4(n0, a0, c0, pp.cn, pp.cacn, psi_prev);
                    const f3 a1 = place4(a0, c0, n1, pc.na, pp.cnca, omega_prev);
                    const f3 c1 = place4(c0, n1, a1, pc.ac, pc.nac, phi);
                    f3 e1, e2, e3;
                    gram_schmidt3(n1, a1, c1, e1, e2, e3);   // columns: unit(C-CA), the N side, e1 x e2
                    m.r[0] = e1.x; m.r[1] = e2.x; m.r[2] = e3.x;
                    m.r[3] = e1.y; m.r[4] = e2.y; m.r[5] = e3.y;
                    m.r[6] = e1.z; m.r[7] = e2.z; m.r[8] = e3.z;
                    m.t[0] = a1.x; m.t[1] = a1.y; m.t[2] = a1.z;
                }
            }
            if (j == 0) f[j] = m;
            else f[j] = seg_combine(f[j - 1], m);
        }

        // ---- stage 2: wave scan of the lane totals, then across the waves ----
        SegRt inc = f[NERF_PER_LANE - 1];
#pragma unroll
        for (int off = 1; off < PS_WAVE; off <<= 1) {
            const SegRt o = seg_shfl_up(inc, off);
            if (lane >= off) inc = seg_combine(o, inc);
        }
        SegRt excl = seg_shfl_up(inc, 1);
        if (lane == 0) excl = seg_identity();
        if (lane == PS_WAVE - 1) wtot[wave] = inc;
        __syncthreads();
        SegRt pre = carry;
        for (int w = 0; w < wave; ++w) pre = seg_combine(pre, wtot[w]);
        for (int w = 0; w < NERF_WAVES; ++w) carry = seg_combine(carry, wtot[w]);
        pre = seg_combine(pre, excl);

        // ---- stage 3: atoms of the lane's residues into LDS ----
#pragma unroll
        for (int j = 0; j < NERF_PER_LANE; ++j) {
            const int k = (int)threadIdx.x * NERF_PER_LANE + j;
            const int i = t0 + k;
            if (i >= N) break;
            const size_t res = base + i;
            const SegRt F = seg_combine(pre, f[j]);
            const bool live = !residue_mask || residue_mask[res] != 0;
            const ResParams pc = res_params(bond_angles, bond_lengths, res);
            const f3 nl = local_n(pc.na, pc.nac);
            const f3 n = mk3((F.r[0] * nl.x + F.r[1] * nl.y) + F.t[0], (F.r[3] * nl.x + F.r[4] * nl.y) + F.t[1],
                             (F.r[6] * nl.x + F.r[7] * nl.y) + F.t[2]);
            const f3 ca = mk3(F.t[0], F.t[1], F.t[2]);
            const f3 c = mk3(F.r[0] * pc.ac + F.t[0], F.r[3] * pc.ac + F.t[1], F.r[6] * pc.ac + F.t[2]);
            f3 cb = mk3(0.f, 0.f, 0.f);
            if (include_cb) {   // geometry.ideal_backbone_coordinates' tetrahedral placement on the global atoms
                const f3 bb = sub3(ca, n), cc = sub3(c, ca), aa = cross3(bb, cc);
                cb = mk3(((-0.58273431f * aa.x + 0.56802827f * bb.x) - 0.54067466f * cc.x) + ca.x,
                         ((-0.58273431f * aa.y + 0.56802827f * bb.y) - 0.54067466f * cc.y) + ca.y,
                         ((-0.58273431f * aa.z + 0.56802827f * bb.z) - 0.54067466f * cc.z) + ca.z);
            }
            const float z = 0.f;
            float* o = atoms + k * 12;
            o[0] = live ? n.x : z;   o[1] = live ? n.y : z;   o[2] = live ? n.z : z;
            o[3] = live ? ca.x : z;  o[4] = live ? ca.y : z;  o[5] = live ? ca.z : z;
            o[6] = live ? c.x : z;   o[7] = live ? c.y : z;   o[8] = live ? c.z : z;
            o[9] = live ? cb.x : z;  o[10] = live ? cb.y : z; o[11] = live ? cb.z : z;
            on[k] = live ? 1.f : 0.f;
        }
        __syncthreads();

        // ---- the tile's rows, zeros included: xyz (nt * 3A floats) and the mask (nt * A floats) ----
        const bool cb = include_cb != 0;
        store_region(xyz + (base + t0) * row, (unsigned)nt * row, [&](unsigned e) {
            const unsigned r = e / row, o = e - r * row;
            return o < 9 ? atoms[r * 12 + o] : ((cb && o >= 12 && o < 15) ? atoms[r * 12 + o - 3] : 0.f);
        });
        store_region(atom_mask + (base + t0) * A, (unsigned)nt * A, [&](unsigned e) {
            const unsigned r = e / A, s = e - r * A;
            return (s < 3 || (cb && s == 4)) ? on[r] : 0.f;
        });
        __syncthreads();   // the next tile overwrites atoms / on / wtot
    }
}

// ---- K12: the backward pass of K7 -- gradients with respect to the dihedrals, bond angles and bond lengths ----
// An internal coordinate of a chain moves everything downstream of it as a rigid body, so its gradient is a projection
// of the downstream force G = sum g_a and torque T = sum x_a x g_a (about the origin, where K7 puts every segment's
// first CA): a rotation about the unit axis u through p gives u . (T - p x G), a bond length along u gives u . G.  No
// scan of transforms is needed backwards: G and T are segmented inclusive SUFFIX sums over the 3 N backbone atoms, six
// floats and a flag per element.  Everything is read off the forward's coordinates; the angles are not needed.
// One workgroup per structure, tiles of 512 residues walked from the chain's END with the running (G, T) carried from
// tile to tile (as K7 carries its transform forwards), two residues per lane in descending order:
//   1. the tile's N / CA / C / CB coordinates (with residue t0 - 1 as a halo) and upstream gradients staged in LDS by
//      the whole workgroup -- only slots 0, 1, 2 (and 4 with include_cb) are ever addressed;
//   2. per residue: the CB gradient pushed back onto N, CA, C, then the residue's (sum g, sum x x g).  A masked residue
//      contributes zeros BY SELECTION (its row of grad_xyz may hold NaN);
//   3. segmented scan over descending residues (lane pair, __shfl_up over the wave, the four wave totals through LDS);
//      a residue that is the last of its segment carries the reset flag, which discards everything after it by selection;
//   4. per residue i: G, T at C_i, CA_i, N_i from the exclusive prefix, then residue i's own parameters (phi_i, angle
//      N-CA-C, |N-CA|, |CA-C|) and those of the junction to i - 1 (psi, omega, the two peptide angles, |C-N|), each
//      stored by exactly one lane; parameters that move no visible atom are stored as exact zeros.
// No atomics and a fixed order of every sum: the same bits on every run.
constexpr int NB_THREADS = 256;
constexpr int NB_PER_LANE = 2;
constexpr int NB_TILE = NB_THREADS * NB_PER_LANE;
constexpr int NB_WAVES = NB_THREADS / PS_WAVE;
constexpr float kCB0 = -0.58273431f, kCB1 = 0.56802827f, kCB2 = -0.54067466f;   // K7's CB placement

struct SegGT {
    f3 g, t;
    int reset;
};

__device__ __forceinline__ f3 add3(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ f3 sel3(bool c, f3 a, f3 b) { return f3{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }
__device__ __forceinline__ f3 unit3(f3 a) { return div3(a, norm3(a)); }

__device__ __forceinline__ SegGT gt_identity() { return SegGT{mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f), 0}; }

// a is the earlier element of the scan (the residues AFTER b's in the chain); a reset on b discards it by selection
__device__ __forceinline__ SegGT gt_combine(const SegGT& a, const SegGT& b) {
    SegGT o;
    o.g = sel3(b.reset != 0, b.g, add3(a.g, b.g));
    o.t = sel3(b.reset != 0, b.t, add3(a.t, b.t));
    o.reset = a.reset | b.reset;
    return o;
}

__device__ __forceinline__ SegGT gt_shfl_up(const SegGT& x, int delta) {
    SegGT o;
    o.g = mk3(__shfl_up(x.g.x, delta), __shfl_up(x.g.y, delta), __shfl_up(x.g.z, delta));
    o.t = mk3(__shfl_up(x.t.x, delta), __shfl_up(x.t.y, delta), __shfl_up(x.t.z, delta));
    o.reset = __shfl_up(x.reset, delta);
    return o;
}

// u . (T - p x G): the gradient of a rotation about the unit axis u through p that moves the atoms summed in (G, T)
__device__ __forceinline__ float turn3(f3 u, f3 p, f3 G, f3 T) { return dot3(u, sub3(T, cross3(p, G))); }

__global__ __launch_bounds__(NB_THREADS) void k12_backbone_from_dihedrals_backward(
    const float* __restrict__ xyz, const float* __restrict__ grad_xyz, const float* __restrict__ chain_idx,
    const uint8_t* __restrict__ residue_mask, float* __restrict__ grad_dihedrals, float* __restrict__ grad_bond_angles,
    float* __restrict__ grad_bond_lengths, int include_cb, int N, int A) {
    const size_t row = 3 * (size_t)A;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
    const size_t base = (size_t)b * N;
    const bool cb = include_cb != 0;

    __shared__ float sx[(NB_TILE + 1) * 12];   // N, CA, C, CB of residues t0 - 1 (the halo) .. t0 + nt - 1
    __shared__ float sg[NB_TILE * 12];         // their upstream gradients, residues t0 .. t0 + nt - 1
    __shared__ SegGT wtot[NB_WAVES];

    SegGT carry = gt_identity();   // the suffix sums at the lowest residue of the tile above
    for (int t0 = ((N - 1) / NB_TILE) * NB_TILE; t0 >= 0; t0 -= NB_TILE) {
        const int nt = min(NB_TILE, N - t0);

        // ---- stage 1: the used slots of the tile into LDS ----
        for (int e = threadIdx.x; e < (nt + 1) * 12; e += NB_THREADS) {
            const int r = e / 12, o = e - r * 12;
            const int i = t0 + r - 1;
            float v = 0.f;
            if (i >= 0 && (o < 9 || cb)) v = xyz[(base + i) * row + (o < 9 ? o : o + 3)];
            sx[e] = v;
        }
        for (int e = threadIdx.x; e < nt * 12; e += NB_THREADS) {
            const int r = e / 12, o = e - r * 12;
            float v = 0.f;
            if (o < 9 || cb) v = grad_xyz[(base + t0 + r) * row + (o < 9 ? o : o + 3)];
            sg[e] = v;
        }
        __syncthreads();

        // ---- stage 2: per residue, descending: lane l holds residues t0 + nt - 1 - 2 l and the one below ----
        f3 xn[NB_PER_LANE], xa[NB_PER_LANE], xc[NB_PER_LANE], gn[NB_PER_LANE], ga[NB_PER_LANE], gc[NB_PER_LANE];
        bool live[NB_PER_LANE], start[NB_PER_LANE];
        SegGT el[NB_PER_LANE];
#pragma unroll
        for (int j = 0; j < NB_PER_LANE; ++j) {
            const int k = nt - 1 - ((int)threadIdx.x * NB_PER_LANE + j);
            el[j] = gt_identity();
            live[j] = start[j] = false;
            xn[j] = xa[j] = xc[j] = gn[j] = ga[j] = gc[j] = mk3(0.f, 0.f, 0.f);
            if (k < 0) continue;
            const int i = t0 + k;
            const size_t res = base + i;
            const bool lv = !residue_mask || residue_mask[res] != 0;
            bool st = (i == 0);
            if (!st && chain_idx) st = chain_idx[res] != chain_idx[res - 1];   // NaN != NaN: a new segment
            if (!st && residue_mask) st = residue_mask[res - 1] == 0;
            bool last = (i == N - 1) || !lv;                                    // the residue after a masked one starts a segment
            if (!last && chain_idx) last = chain_idx[res + 1] != chain_idx[res];
            const float* x = sx + (k + 1) * 12;
            const float* g = sg + k * 12;
            const f3 z = mk3(0.f, 0.f, 0.f);
            xn[j] = sel3(lv, load3(x), z);
            xa[j] = sel3(lv, load3(x + 3), z);
            xc[j] = sel3(lv, load3(x + 6), z);
            f3 n = sel3(lv, load3(g), z), a = sel3(lv, load3(g + 3), z), c = sel3(lv, load3(g + 6), z);
            if (cb) {   // CB = k0 (bb x cc) + k1 bb + k2 cc + CA with bb = CA - N, cc = C - CA
                const f3 gb = sel3(lv, load3(g + 9), z);
                const f3 bb = sub3(xa[j], xn[j]), cc = sub3(xc[j], xa[j]);
                const f3 g_bb = add3(scale3(cross3(cc, gb), kCB0), scale3(gb, kCB1));
                const f3 g_cc = add3(scale3(cross3(gb, bb), kCB0), scale3(gb, kCB2));
                n = sub3(n, g_bb);
                a = add3(sub3(add3(a, g_bb), g_cc), gb);
                c = add3(c, g_cc);
            }
            gn[j] = n; ga[j] = a; gc[j] = c;
            live[j] = lv; start[j] = st;
            el[j].g = add3(add3(c, a), n);
            el[j].t = add3(add3(cross3(xc[j], c), cross3(xa[j], a)), cross3(xn[j], n));
            el[j].reset = last ? 1 : 0;
        }

        // ---- stage 3: the segmented scan over descending residues ----
        SegGT inc = gt_combine(el[0], el[1]);
#pragma unroll
        for (int off = 1; off < PS_WAVE; off <<= 1) {
            const SegGT o = gt_shfl_up(inc, off);
            if (lane >= off) inc = gt_combine(o, inc);
        }
        SegGT excl = gt_shfl_up(inc, 1);
        if (lane == 0) excl = gt_identity();
        if (lane == PS_WAVE - 1) wtot[wave] = inc;
        __syncthreads();
        SegGT pre = carry;
        for (int w = 0; w < wave; ++w) pre = gt_combine(pre, wtot[w]);
        for (int w = 0; w < NB_WAVES; ++w) carry = gt_combine(carry, wtot[w]);
        pre = gt_combine(pre, excl);

        // ---- stage 4: the parameters of residue i and of its junction to i - 1 ----
#pragma unroll
        for (int j = 0; j < NB_PER_LANE; ++j) {
            const int k = nt - 1 - ((int)threadIdx.x * NB_PER_LANE + j);
            if (k < 0) break;
            const int i = t0 + k;
            const size_t res = base + i;
            const SegGT after = (j == 0) ? pre : gt_combine(pre, el[0]);   // the residues after i
            const bool last = el[j].reset != 0;
            const f3 z = mk3(0.f, 0.f, 0.f);
            const f3 Gc = add3(gc[j], sel3(last, z, after.g)), Tc = add3(cross3(xc[j], gc[j]), sel3(last, z, after.t));
            const f3 Ga = add3(ga[j], Gc), Ta = add3(cross3(xa[j], ga[j]), Tc);
            const f3 Gn = add3(gn[j], Ga), Tn = add3(cross3(xn[j], gn[j]), Ta);
            const bool cont = !start[j] && live[j], head = start[j] && live[j];
            const f3 an = sub3(xn[j], xa[j]), ac = sub3(xc[j], xa[j]);   // CA -> N, CA -> C
            const f3 u_ac = unit3(ac);
            // phi_i turns C_i.. about N_i -> CA_i; the angle N-CA-C turns them about (N - CA) x (C - CA) through CA_i
            const float d_phi = turn3(unit3(sub3(xa[j], xn[j])), xa[j], Gc, Tc);
            const float d_nac = turn3(unit3(cross3(an, ac)), xa[j], Gc, Tc);
            const float d_na = dot3(unit3(sub3(xa[j], xn[j])), Ga);
            // a segment's first residue sits in the fixed frame: |N-CA| and the angle move N_i alone
            const float h_nac = dot3(unit3(cross3(ac, an)), cross3(an, gn[j]));
            const float h_na = dot3(unit3(an), gn[j]);
            grad_dihedrals[res * 3] = cont ? d_phi : 0.f;
            if (grad_bond_angles) grad_bond_angles[res * 3] = cont ? d_nac : (head ? h_nac : 0.f);
            if (grad_bond_lengths) {
                grad_bond_lengths[res * 3] = cont ? d_na : (head ? h_na : 0.f);
                grad_bond_lengths[res * 3 + 1] = live[j] ? dot3(u_ac, Gc) : 0.f;
            }
            if (i > 0) {
                const f3 aj = load3(sx + k * 12 + 3), cj = load3(sx + k * 12 + 6);   // CA and C of residue i - 1
                const f3 cn = sub3(xn[j], cj);
                const f3 u_cn = unit3(cn);
                // psi_j turns N_i.. about CA_j -> C_j, omega_j turns CA_i.. about C_j -> N_i
                const float d_psi = turn3(unit3(sub3(cj, aj)), cj, Gn, Tn);
                const float d_omega = turn3(u_cn, xn[j], Ga, Ta);
                grad_dihedrals[(res - 1) * 3 + 1] = cont ? d_psi : 0.f;
                grad_dihedrals[(res - 1) * 3 + 2] = cont ? d_omega : 0.f;
                if (grad_bond_angles) {
                    const float d_cacn = turn3(unit3(cross3(sub3(aj, cj), cn)), cj, Gn, Tn);
                    const float d_cnca = turn3(unit3(cross3(sub3(cj, xn[j]), sub3(xa[j], xn[j]))), xn[j], Ga, Ta);
                    grad_bond_angles[(res - 1) * 3 + 1] = cont ? d_cacn : 0.f;
                    grad_bond_angles[(res - 1) * 3 + 2] = cont ? d_cnca : 0.f;
                }
                if (grad_bond_lengths) grad_bond_lengths[(res - 1) * 3 + 2] = cont ? dot3(u_cn, Gn) : 0.f;
            }
            if (i == N - 1) {   // nothing follows the last residue
                grad_dihedrals[res * 3 + 1] = 0.f;
                grad_dihedrals[res * 3 + 2] = 0.f;
                if (grad_bond_angles) grad_bond_angles[res * 3 + 1] = grad_bond_angles[res * 3 + 2] = 0.f;
                if (grad_bond_lengths) grad_bond_lengths[res * 3 + 2] = 0.f;
            }
        }
        __syncthreads();   // the next tile overwrites sx / sg / wtot
    }
}

}  // namespace

extern "C" int ps_backbone_from_dihedrals_backward_f32(const float* xyz, const float* grad_xyz, const float* chain_idx,
                                                       const uint8_t* residue_mask, float* grad_dihedrals,
                                                       float* grad_bond_angles, float* grad_bond_lengths, int include_cb,
                                                       int B, int N, int A, void* stream) {
    if (!xyz || !grad_xyz || !grad_dihedrals || B < 0 || N < 0 || A < 3 || (include_cb && A < 5)) return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0) return 0;
    return ps_launch(k12_backbone_from_dihedrals_backward, dim3((unsigned)B), dim3(NB_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), xyz, grad_xyz, chain_idx, residue_mask, grad_dihedrals,
                     grad_bond_angles, grad_bond_lengths, include_cb, N, A);
}

extern "C" int ps_backbone_from_dihedrals_f32(const float* dihedrals, const float* bond_angles, const float* bond_lengths,
                                              const float* chain_idx, const uint8_t* residue_mask, float* xyz,
                                              float* atom_mask, int include_cb, int B, int N, int A, void* stream) {
    if (!dihedrals || !xyz || !atom_mask || B < 0 || N < 0 || A < 3 || (include_cb && A < 5)) return (int)hipErrorInvalidValue;
    // one tile's rows are indexed in 32 bits
    if ((unsigned long long)NERF_TILE * 3ull * (unsigned long long)A > 0xFFFFFFFFull) return (int)hipErrorInvalidValue;
    if (((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(atom_mask)) & 3u) != 0) return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0) return 0;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (A == 15)
        return ps_launch(k7_backbone_from_dihedrals<15>, dim3((unsigned)B), dim3(NERF_THREADS), 0, s, dihedrals,
                         bond_angles, bond_lengths, chain_idx, residue_mask, xyz, atom_mask, include_cb, N, A);
    return ps_launch(k7_backbone_from_dihedrals<0>, dim3((unsigned)B), dim3(NERF_THREADS), 0, s, dihedrals, bond_angles,
                     bond_lengths, chain_idx, residue_mask, xyz, atom_mask, include_cb, N, A);
}
