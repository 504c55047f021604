// The fused trRosetta featuriser (inter_residue_geometry, reference protstruc.py:790-817): K1's three atom-pair planes,
// their masks and K3's three angle features of every residue pair in one pass.  The arithmetic (k3_arith.hpp, both the
// fast and the faithful one), the lane maps and the launch context (k3_launch.hpp) are K3's (pairwise_angles.hip); the
// backward pass is featuriser_backward.hip.
//
// Kernels, in the order of this file (DESIGN.md section 4 has the dispatch table and the numbers; ps_featuriser_plan_f32
// names the one a launch takes), then their thresholds and launchers, then the entry points:
//   k3_inter_residue_geometry   one column per lane: the layout-free twin the other two are held to bit for bit, and the fallback
//   k3_featurise                the sweep of k3_sweep over all nine planes (>= 40 residues)
//   k3_featurise_tiles          the tile map of k3_flat over all nine planes (8..96 residues and where a sweep would idle lanes)
#include "k3_arith.hpp"
#include "k3_launch.hpp"

#include <initializer_list>
#include <type_traits>

namespace {

// Fused trRosetta featuriser (reference protstruc.py:790-817): the three atom-pair planes of K1 that
// inter_residue_geometry slices out (CA-CA, CB-CB, N-O), their masks, and the three K3 features, in
// one sweep -- 27 bytes written per residue pair instead of 1125.  Same lane layout as K3.
template <bool EXACT, bool FAITHFUL>
__global__ __launch_bounds__(256) void k3_inter_residue_geometry(
    const float* __restrict__ xyz, const uint8_t* __restrict__ amask, float* __restrict__ d_ca,
    float* __restrict__ d_cb, float* __restrict__ d_no, float* __restrict__ omega, float* __restrict__ theta,
    float* __restrict__ phi, uint8_t* __restrict__ m_ca, uint8_t* __restrict__ m_cb, uint8_t* __restrict__ m_no, int N,
    int A, int IR, int n_tiles, int n_chunks) {
    const unsigned w = blockIdx.x;   // 1-D grid as in k3_pairwise_angles
    const unsigned tile = w % (unsigned)n_tiles, rest = w / (unsigned)n_tiles;
    const int b = (int)(rest / (unsigned)n_chunks);
    const int j = (int)tile * (int)blockDim.x + threadIdx.x;   // a workgroup is 64, 128, 192 or 256 lanes wide (short chains)
    const int i0 = (int)(rest % (unsigned)n_chunks) * IR, i1 = min(i0 + IR, N);
    const bool live = j < N;
    const int jc = live ? j : N - 1;
    const float* sj = xyz + ((size_t)b * N + jc) * (size_t)A * 3;
    const f3 ca_j = load3(sj + 3), o_j = load3(sj + 9), cb_j = load3(sj + 12);
    uint8_t mj_ca = 1, mj_o = 1, mj_cb = 1;
    if (amask) {
        const uint8_t* mj = amask + ((size_t)b * N + jc) * A;
        mj_ca = mj[1] != 0; mj_o = mj[3] != 0; mj_cb = mj[4] != 0;
    }
    auto row_scalars = [&](int i, f3& n_i, f3& ca_i, f3& cb_i, uint8_t& mi_n, uint8_t& mi_ca, uint8_t& mi_cb) {
        const float* si = xyz + ((size_t)b * N + i) * (size_t)A * 3;  // wave-uniform
        n_i = load3(si); ca_i = load3(si + 3); cb_i = load3(si + 12);
        mi_n = mi_ca = mi_cb = 1;
        if (amask) {
            const uint8_t* mi = amask + ((size_t)b * N + i) * A;
            mi_n = mi[0] != 0; mi_ca = mi[1] != 0; mi_cb = mi[4] != 0;
        }
    };
    auto row_planes = [&](size_t o, f3 n_i, f3 ca_i, f3 cb_i, uint8_t mi_n, uint8_t mi_ca, uint8_t mi_cb) {
        d_ca[o] = dist3_t<EXACT>(ca_i, ca_j);
        d_cb[o] = dist3_t<EXACT>(cb_i, cb_j);
        d_no[o] = dist3_t<EXACT>(n_i, o_j);
        m_ca[o] = mi_ca & mj_ca;
        m_cb[o] = mi_cb & mj_cb;
        m_no[o] = mi_n & mj_o;
        phi[o] = FAITHFUL ? angle3_ref(ca_i, cb_i, cb_j) : angle3(ca_i, cb_i, cb_j);
    };
    int i = i0;
    for (; !FAITHFUL && i + 1 < i1; i += 2) {  // two rows per trip: distances, planar angle and both dihedrals as packed float2 math
        f3 n0, ca0, cb0, n1, ca1, cb1;
        uint8_t a0, b0, c0, a1, b1, c1;
        row_scalars(i, n0, ca0, cb0, a0, b0, c0);
        row_scalars(i + 1, n1, ca1, cb1, a1, b1, c1);
        if (!live) continue;
        const size_t o = ((size_t)b * N + i) * N + j;
        const f3v cav = mk3v(ca0, ca1), cbv = mk3v(cb0, cb1), nv = mk3v(n0, n1);
        const f3v cajv = mk3v(ca_j, ca_j), cbjv = mk3v(cb_j, cb_j), ojv = mk3v(o_j, o_j);
        const f32x2 dca = dist3v_t<EXACT>(cav, cajv), dcb = dist3v_t<EXACT>(cbv, cbjv), dno = dist3v_t<EXACT>(nv, ojv);
        const f32x2 ph = angle3v(cav, cbv, cbjv);
        const f32x2 om = dihedral4v_k3(cav, cbv, cajv, cbjv);   // as coded at protstruc.py:811
        const f32x2 th = dihedral4v_k3(nv, cav, cbv, cbjv);
        d_ca[o] = dca.x; d_ca[o + N] = dca.y;
        d_cb[o] = dcb.x; d_cb[o + N] = dcb.y;
        d_no[o] = dno.x; d_no[o + N] = dno.y;
        m_ca[o] = b0 & mj_ca; m_ca[o + N] = b1 & mj_ca;
        m_cb[o] = c0 & mj_cb; m_cb[o + N] = c1 & mj_cb;
        m_no[o] = a0 & mj_o;  m_no[o + N] = a1 & mj_o;
        phi[o] = ph.x; phi[o + N] = ph.y;
        omega[o] = om.x; omega[o + N] = om.y;
        theta[o] = th.x; theta[o + N] = th.y;
    }
    for (; i < i1; ++i) {
        f3 n_i, ca_i, cb_i;
        uint8_t mi_n, mi_ca, mi_cb;
        row_scalars(i, n_i, ca_i, cb_i, mi_n, mi_ca, mi_cb);
        if (!live) continue;
        const size_t o = ((size_t)b * N + i) * N + j;
        row_planes(o, n_i, ca_i, cb_i, mi_n, mi_ca, mi_cb);
        omega[o] = FAITHFUL ? dihedral4_ref(ca_i, cb_i, ca_j, cb_j) : dihedral4_k3(ca_i, cb_i, ca_j, cb_j);   // as coded at protstruc.py:811
        theta[o] = FAITHFUL ? dihedral4_ref(n_i, ca_i, cb_i, cb_j) : dihedral4_k3(n_i, ca_i, cb_i, cb_j);
    }
}

// The featuriser on the skeleton of k3_sweep (round 4): one workgroup per CU (1024 threads at NC = 2, 512 at NC = 4), the row
// residues' N / CA / CB points and their three mask bits staged in LDS (pair-interleaved), tasks pulled from an LDS
// counter, and the two dihedrals' and the planar angle's chains interleaved across the NC columns of a lane.  Same
// arithmetic per pair as k3_inter_residue_geometry above: same bits.
//   * Small tasks, in memory order.  The column points (CA, O, CB: staged once per structure, 36 bytes per residue) come from
//     LDS per task and strip.  The first cut gave a workgroup one (structure, strip) segment at a time, 8-row tasks and the
//     column points in registers for the whole segment.  That is only good when a workgroup's share divides into whole
//     segments (B = 128, N = 512: half a structure each): the waves of a workgroup wait for each other at every segment
//     boundary for up to one task, and a share cut into a short and a long segment (any other B, N) idled them for a fifth
//     of the time; and its staging loops walked ~13 dependent round trips to L2 per segment (an element per thread; now a
//     residue per thread with its nine loads in flight: N = 512 178 -> 168 us).  N = 500 284 us, N = 510 415, N = 200 344
//     against 211 at N = 512, 2^25 pairs each (profiles/r04_k3_featuriser_shapes.log).
//   * VEC: the lane's NC columns are consecutive and every float plane goes out in 4 * NC-byte stores (N % NC == 0, planes
//     4 * NC-byte aligned).  !VEC (any N, any 4-byte alignment): the columns are 64 apart and a store instruction writes 64
//     consecutive floats of a row, as in k3_sweep.
//   * M16 (VEC, N % 16 == 0, 16-byte aligned mask planes): the mask planes have their own lane map inside a strip:
//     a lane owns 16 consecutive column residues of one row, a store instruction carries four rows x 256 bytes (NC = 2:
//     up to eight rows x 128).
//     !M16: the mask planes are written FLAT.  The mask bytes of a task's rows are one contiguous run of every plane
//     (rows are contiguous in memory), whatever N is; the run is cut on the plane's absolute 16-byte grid -- a group that
//     starts in the task's rows belongs to the task, also where it runs into the next task's first row -- and a lane
//     builds 16 bytes at a time from bit sets: 16 bits of the structure's column mask (two LDS words, one v_alignbit) AND
//     the row's bit, the next row's where the group wraps, spread to bytes: a store instruction writes 1 KB.  The task of every
//     fourth chunk's first strip writes the masks of 16 rows (full lanes, one set-up).  Only at a structure's two ends are
//     the bytes outside whole groups written as bytes.
//   * WT: write-through stores (sc1) where every store covers whole 128-byte lines and strips are whole (N % 128 == 0);
//     write-back otherwise, so that lines shared by two stores merge in L2 instead of going out as two partial writes.
template <bool EXACT, int NC, bool VEC, bool M16, bool WT, bool FAITHFUL = false>
__global__ __launch_bounds__((NC == 4 || FAITHFUL) ? 512 : 1024) void k3_featurise(
    const float* __restrict__ xyz, const uint8_t* __restrict__ amask, float* __restrict__ d_ca,
    float* __restrict__ d_cb, float* __restrict__ d_no, float* __restrict__ omega, float* __restrict__ theta,
    float* __restrict__ phi, uint8_t* __restrict__ m_ca, uint8_t* __restrict__ m_cb, uint8_t* __restrict__ m_no, int N,
    int A, int CH, int n_strips, int n_chunks, unsigned n_tasks, unsigned tasks_per_wg, unsigned rcpN, int KS, int slot_bytes, int pull) {
    static_assert(NC == 2 || NC == 4, "columns per lane");
    static_assert(!M16 || VEC, "16-byte strip mask stores ride on the vector kernels");
    constexpr int POL = WT ? 16 : 0;
    extern __shared__ __attribute__((aligned(16))) f32x2 k3_rowbuf[];   // [row pair][N, CA, CB][xyz]; then the row mask words, the column points, the column masks
    __shared__ unsigned next_task;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x >> 6);
    const unsigned t0 = blockIdx.x * tasks_per_wg, t1 = min(t0 + tasks_per_wg, n_tasks);
    if (t0 >= t1) return;                         // whole workgroup
    const int max_pairs = (N + 2) / 2, Np = (N + 3) & ~3;
    // one structure's slot: [row pair][N, CA, CB][xyz] as f32x2; the row mask words (per row pair: byte 0 = row 2r, byte 1 = row
    // 2r + 1; bits n = 1, ca = 2, cb = 4; 8 spare); the column points [CA, O, CB][xyz][Np]; the column masks -- M16:
    // colmask[plane][column] as bytes; !M16: colbits[plane][word] = bit sets (planes CA, CB, O; zero beyond N and two zero
    // words of padding), same region, 16-byte aligned.  KS slots of slot_bytes each (round 5: several structures per staging
    // pass -- short chains paid two barriers and a round trip to L2 per 4 096 pairs).
    const size_t colpts_off = ((size_t)max_pairs * (9 * 8 + 4) + 32 + 15) & ~(size_t)15;
    const int nw = (N + 31) / 32 + 2;
    const int row_bytes = N * 4;
    // tasks of one structure: (chunk of CH rows, strip), a chunk's strips adjacent.  (Tried: a chunk of two rows x ALL strips,
    // the wave walking the strips inside the row pair, so that every 64-byte segment two stores share is completed by one
    // wave within a trip: 3-7 % SLOWER than four-row tasks per strip, N = 500 267 against 259 us -- the column points then
    // come from LDS every trip.  Two-row tasks per strip are what helped: see the launcher.)
    const int tpc = n_strips;                                         // tasks per chunk
    const unsigned n_sub = (unsigned)n_chunks * (unsigned)tpc;
    const unsigned b_first = t0 / n_sub, b_last = (t1 - 1u) / n_sub;
    for (unsigned bs = b_first; bs <= b_last; bs += (unsigned)KS) {     // the structures of this workgroup's tasks, KS per staging pass
        const unsigned ks = min((unsigned)KS, b_last - bs + 1u);
        __syncthreads();                                          // the previous pass's readers are done
        // a team of tw waves per structure (all of them when the pass is one structure; one wave each from n_waves structures on)
        const int tw = max(1, n_waves / (int)ks), n_teams = n_waves / tw;
        const int team = wave / tw, tl = (wave - team * tw) * 64 + lane, tsz = tw * 64;   // (waves beyond n_teams * tw: no team)
        for (unsigned s = (unsigned)team; s < ks && team < n_teams; s += (unsigned)n_teams) {
            char* slot = reinterpret_cast<char*>(k3_rowbuf) + (size_t)s * slot_bytes;
            uint32_t* rowmask = reinterpret_cast<uint32_t*>(slot + (size_t)max_pairs * 72);
            float* colpts = reinterpret_cast<float*>(slot + colpts_off);
            uint8_t* colmask = reinterpret_cast<uint8_t*>(colpts + 9 * Np);
            uint32_t* colbits = reinterpret_cast<uint32_t*>(colmask);
            const float* xb = xyz + (size_t)(bs + s) * N * (size_t)A * 3;   // uniform
            const uint8_t* mb = amask ? amask + (size_t)(bs + s) * N * A : nullptr;
            // one residue per thread, its loads in flight together (an element per thread made every workgroup walk
            // 9 N / 512 dependent round trips to L2 per structure: ~10 us of a 170 us launch): rows N, CA, CB; columns CA, O, CB
            float* rb = reinterpret_cast<float*>(slot);
            for (int row = tl; row < Np; row += tsz) {
                const float* pr = xb + (size_t)min(row, N - 1) * (size_t)A * 3;   // (the padding repeats the last residue)
                const float v[15] = {pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[12], pr[13], pr[14], pr[9], pr[10], pr[11]};
                if (row < N) {
#pragma unroll
                    for (int qc = 0; qc < 9; ++qc) rb[(((row >> 1) * 9 + qc) << 1) + (row & 1)] = v[qc];
                }
                colpts[0 * Np + row] = v[3]; colpts[1 * Np + row] = v[4]; colpts[2 * Np + row] = v[5];       // CA
                colpts[3 * Np + row] = v[9]; colpts[4 * Np + row] = v[10]; colpts[5 * Np + row] = v[11];     // O
                colpts[6 * Np + row] = v[6]; colpts[7 * Np + row] = v[7]; colpts[8 * Np + row] = v[8];       // CB
            }
            const int n_pairs = N / 2 + 1 + (M16 ? 0 : (16 - CH) / 2);   // !M16: up to 16 - CH rows and one beyond the tasks' own (flat mask groups)
            for (int r = tl; r < n_pairs; r += tsz) {
                uint32_t w = 0x0707u;
                if (mb) {
                    const int ia = min(2 * r, N - 1), ib = min(ia + 1, N - 1);
                    const uint8_t* pa = mb + (size_t)ia * A;
                    const uint8_t* pb = mb + (size_t)ib * A;
                    w = (pa[0] != 0 ? 1u : 0u) | (pa[1] != 0 ? 2u : 0u) | (pa[4] != 0 ? 4u : 0u) |
                        (pb[0] != 0 ? 0x100u : 0u) | (pb[1] != 0 ? 0x200u : 0u) | (pb[4] != 0 ? 0x400u : 0u);
                }
                rowmask[r] = w;
            }
            if constexpr (M16) {
                for (int j = tl; j < N; j += tsz) {
                    uint8_t a = 1, c2 = 1, o = 1;
                    if (mb) {
                        const uint8_t* mj = mb + (size_t)j * A;
                        a = mj[1] != 0; c2 = mj[4] != 0; o = mj[3] != 0;
                    }
                    colmask[j] = a; colmask[N + j] = c2; colmask[2 * N + j] = o;
                }
            } else {
                for (int base = (wave - team * tw) * 64; base < nw * 32; base += tsz) {   // (uniform per wave)
                    const int j = base + lane;
                    bool a = false, c2 = false, o = false;
                    if (j < N) {
                        a = c2 = o = true;
                        if (mb) {
                            const uint8_t* mj = mb + (size_t)j * A;
                            a = mj[1] != 0; c2 = mj[4] != 0; o = mj[3] != 0;
                        }
                    }
                    const unsigned long long ba = __ballot(a), bc = __ballot(c2), bo = __ballot(o);
                    if (lane == 0) {
                        const int k = base >> 5;
                        colbits[k] = (uint32_t)ba; colbits[nw + k] = (uint32_t)bc; colbits[2 * nw + k] = (uint32_t)bo;
                        if (k + 1 < nw) {
                            colbits[k + 1] = (uint32_t)(ba >> 32); colbits[nw + k + 1] = (uint32_t)(bc >> 32);
                            colbits[2 * nw + k + 1] = (uint32_t)(bo >> 32);
                        }
                    }
                }
            }
        }
        const unsigned seg_t0 = max(t0, bs * n_sub), seg_t1 = min(t1, (bs + ks) * n_sub);
        if (threadIdx.x == 0) next_task = seg_t0 + (unsigned)(n_waves * pull);   // the first n_waves pulls are pre-assigned
        __syncthreads();
        constexpr int GS = 4 * NC, RS = 64 / GS;                  // M16: 16-column groups of a strip, rows of a store instruction (4 / 8)
        const int gq = lane % GS, rq = lane / GS;                 // ... this lane's group and row
        // a wave takes `pull` consecutive tasks at a time (1 in the product; round 5 tried 2 and 4 at rows that are not whole 64-byte
        // segments, so that the segments adjacent tasks share are completed by one wave: NOTES.md)
        unsigned t = seg_t0 + (unsigned)(wave * pull), t_end = min(t + (unsigned)pull, seg_t1);
        while (t < seg_t1) {
            // the task's structure (uniform): its slot in LDS, and per plane the structure's rows as one buffer (uniform base, the
            // lane's constant byte offset, the row's byte offset as a scalar)
            const unsigned b = t / n_sub;
            const int c = (int)(t - b * n_sub);
            const char* slot = reinterpret_cast<const char*>(k3_rowbuf) + (size_t)(b - bs) * slot_bytes;
            const f32x2* rowbuf = reinterpret_cast<const f32x2*>(slot);
            const uint32_t* rowmask = reinterpret_cast<const uint32_t*>(slot + (size_t)max_pairs * 72);
            const float* colpts = reinterpret_cast<const float*>(slot + colpts_off);
            const uint8_t* colmask = reinterpret_cast<const uint8_t*>(colpts + 9 * Np);
            const uint32_t* colbits = reinterpret_cast<const uint32_t*>(colmask);
            constexpr int r_lo = 0;
            const int r_hi = N;
            const size_t seg = (size_t)b * N * N, sbase = seg;
            auto rs = [&](void* base) { return __builtin_amdgcn_make_buffer_rsrc(base, 0, 0xFFFFFFFFu, 0x00020000u); };
            const __amdgpu_buffer_rsrc_t r_dca = rs(d_ca + seg), r_dcb = rs(d_cb + seg), r_dno = rs(d_no + seg), r_om = rs(omega + seg),
                                         r_th = rs(theta + seg), r_ph = rs(phi + seg);
            const __amdgpu_buffer_rsrc_t r_mca = rs(m_ca + sbase), r_mcb = rs(m_cb + sbase), r_mno = rs(m_no + sbase);
            const int chunk = c / tpc, strip0 = c - chunk * tpc;
            const int i0 = chunk * CH - r_lo;                     // rows relative to r_lo (CH is even: pairs stay aligned)
            const int i1 = min(i0 + CH, r_hi - r_lo);
            // !M16: the mask bytes of 16 rows (several chunks: full lanes, and the set-up once per 16 rows), flat, plane by plane
            // (each plane has its own 16-byte grid), by the task of their first chunk's first strip.  What a task owns must not
            // depend on the workgroup that runs it: the rows' mask words are staged up to 16 rows beyond the workgroup's own rows.
            if (!M16 && strip0 == 0 && (chunk * CH) % 16 == 0) {
                const int R0 = chunk * CH, R1 = min(R0 + 16, N);
                const unsigned rel0 = (unsigned)R0 * (unsigned)N, rel1 = (unsigned)R1 * (unsigned)N;   // bytes from the structure's first
                const bool first = chunk == 0, more = R1 < N;     // the structure's first / not its last rows
                auto row_word = [&](unsigned i) {                 // the three mask bits of absolute row i (staged: r_lo <= i <= r_hi)
                    const unsigned ri = i - (unsigned)r_lo;
                    return rowmask[ri >> 1] >> (8u * (ri & 1u));
                };
                // one 16-byte group of one plane: 16 bits of the column mask from column j on (zero beyond N), AND the row's
                // bit; where the group runs into row i + 1 (N >= 64: at most once), that row's first columns
                auto group = [&](const uint32_t* W, uint32_t bit, uint32_t w0, uint32_t w1, unsigned j, bool wrap) {
                    const unsigned k = j >> 5, sh = j & 31u;
                    uint32_t x = (w0 & bit) ? (__builtin_amdgcn_alignbit(W[k + 1], W[k], sh) & 0xFFFFu) : 0u;
                    if (wrap && (w1 & bit)) x |= (W[0] << ((unsigned)N - j)) & 0xFFFFu;
                    return k3_u32x4{((x & 15u) * 0x00204081u) & 0x01010101u, (((x >> 4) & 15u) * 0x00204081u) & 0x01010101u,
                                    (((x >> 8) & 15u) * 0x00204081u) & 0x01010101u, (((x >> 12) & 15u) * 0x00204081u) & 0x01010101u};
                };
                auto span = [&](const uint8_t* first_byte, unsigned& bs, unsigned& be) {   // the whole groups that start in these rows
                    const unsigned sb16 = (unsigned)(reinterpret_cast<uintptr_t>(first_byte) & 15u);   // the structure's first byte on the grid
                    bs = rel0 + ((16u - ((sb16 + rel0) & 15u)) & 15u);
                    be = more ? rel1 + ((16u - ((sb16 + rel1) & 15u)) & 15u) : rel1 - ((sb16 + rel1) & 15u);
                };
                auto ends = [&](const __amdgpu_buffer_rsrc_t& rsrc, const uint32_t* W, uint32_t bit, unsigned bs, unsigned be) {
                    if ((first && bs > rel0) || (!more && be < rel1)) {   // (uniform) the structure's ends: bytes outside whole groups
                        const bool head = lane < 16;
                        const unsigned f = head ? rel0 + (unsigned)lane : be + (unsigned)(lane - 16);
                        if (lane < 32 && (head ? (first && f < bs) : (!more && f < rel1))) {
                            unsigned i = __umulhi(f, rcpN), j = f - i * (unsigned)N;
                            if (j >= (unsigned)N) ++i, j -= (unsigned)N;
                            const uint8_t v = (row_word(i) & bit) ? (uint8_t)((W[j >> 5] >> (j & 31u)) & 1u) : (uint8_t)0;
                            __builtin_amdgcn_raw_buffer_store_b8(v, rsrc, (int)f, 0, POL);
                        }
                    }
                };
                unsigned bs_ca, be_ca, bs_cb, be_cb, bs_no, be_no;
                span(m_ca + sbase, bs_ca, be_ca); span(m_cb + sbase, bs_cb, be_cb); span(m_no + sbase, bs_no, be_no);
                if (bs_ca == bs_cb && bs_ca == bs_no) {           // (uniform) one grid for the three planes: one decode per group
                    for (unsigned f = bs_ca + 16u * (unsigned)lane; f < be_ca; f += 16u * 64u) {   // a store instruction writes 1 KB
                        unsigned i = __umulhi(f, rcpN), j = f - i * (unsigned)N;
                        if (j >= (unsigned)N) ++i, j -= (unsigned)N;
                        const bool wrap = j + 16u > (unsigned)N;
                        const uint32_t w0 = row_word(i), w1 = wrap ? row_word(i + 1u) : 0u;
                        k3_u32x4 g1 = group(colbits, 2u, w0, w1, j, wrap), g2 = group(colbits + nw, 4u, w0, w1, j, wrap), g3 = group(colbits + 2 * nw, 1u, w0, w1, j, wrap);
                        __builtin_amdgcn_raw_buffer_store_b128(g1, r_mca, (int)f, 0, POL);
                        __builtin_amdgcn_raw_buffer_store_b128(g2, r_mcb, (int)f, 0, POL);
                        __builtin_amdgcn_raw_buffer_store_b128(g3, r_mno, (int)f, 0, POL);
                    }
                } else {
                    auto plane = [&](const __amdgpu_buffer_rsrc_t& rsrc, const uint32_t* W, uint32_t bit, unsigned bs, unsigned be) {
                        for (unsigned f = bs + 16u * (unsigned)lane; f < be; f += 16u * 64u) {
                            unsigned i = __umulhi(f, rcpN), j = f - i * (unsigned)N;
                            if (j >= (unsigned)N) ++i, j -= (unsigned)N;
                            const bool wrap = j + 16u > (unsigned)N;
                            __builtin_amdgcn_raw_buffer_store_b128(group(W, bit, row_word(i), wrap ? row_word(i + 1u) : 0u, j, wrap), rsrc, (int)f, 0, POL);
                        }
                    };
                    plane(r_mca, colbits, 2u, bs_ca, be_ca);
                    plane(r_mcb, colbits + nw, 4u, bs_cb, be_cb);
                    plane(r_mno, colbits + 2 * nw, 1u, bs_no, be_no);
                }
                ends(r_mca, colbits, 2u, bs_ca, be_ca);
                ends(r_mcb, colbits + nw, 4u, bs_cb, be_cb);
                ends(r_mno, colbits + 2 * nw, 1u, bs_no, be_no);
            }
            {
                const int strip = strip0;
                // this lane's NC columns of the strip
                const int jbase = VEC ? (strip * 64 + lane) * NC : strip * 64 * NC + lane;
                bool lv[NC];
                f3 ca_j[NC], o_j[NC], cb_j[NC];
                if constexpr (VEC) {                              // consecutive columns: one LDS read per coordinate
                    const int jr = min(jbase, Np - NC);
                    typedef typename std::conditional<NC == 4, k3_f32x4, f32x2>::type cvec;
                    cvec t[9];
#pragma unroll
                    for (int qc = 0; qc < 9; ++qc) t[qc] = *reinterpret_cast<const cvec*>(colpts + qc * Np + jr);
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc) {
                        lv[cc] = jbase < N;                       // N % NC == 0: a lane's columns are all in or all out
                        ca_j[cc] = f3{t[0][cc], t[1][cc], t[2][cc]};
                        o_j[cc] = f3{t[3][cc], t[4][cc], t[5][cc]};
                        cb_j[cc] = f3{t[6][cc], t[7][cc], t[8][cc]};
                    }
                } else {
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc) {
                        const int j = jbase + 64 * cc, jr = min(j, N - 1);
                        lv[cc] = j < N;
                        ca_j[cc] = f3{colpts[jr], colpts[Np + jr], colpts[2 * Np + jr]};
                        o_j[cc] = f3{colpts[3 * Np + jr], colpts[4 * Np + jr], colpts[5 * Np + jr]};
                        cb_j[cc] = f3{colpts[6 * Np + jr], colpts[7 * Np + jr], colpts[8 * Np + jr]};
                    }
                }
                const bool live = lv[0];
                const int lane_off = jbase * 4;
                if constexpr (M16) {                              // the strip's mask planes: four (NC = 2: eight) rows per store instruction
                    const int jg = strip * 64 * NC + 16 * gq;
                    if (jg < N) {                                 // N % 16 == 0: a group is in or out
                        const k3_u32x4 cm_ca = *reinterpret_cast<const k3_u32x4*>(colmask + jg);
                        const k3_u32x4 cm_cb = *reinterpret_cast<const k3_u32x4*>(colmask + N + jg);
                        const k3_u32x4 cm_o = *reinterpret_cast<const k3_u32x4*>(colmask + 2 * N + jg);
                        for (int k4 = i0; k4 < i1; k4 += RS) {
                            const int rr = k4 + rq;
                            if (rr < i1) {
                                const uint32_t w = rowmask[rr >> 1] >> (8 * (rr & 1));
                                const int vo = rr * N + jg;
                                const k3_u32x4 z = {0, 0, 0, 0};
                                __builtin_amdgcn_raw_buffer_store_b128((w & 2u) ? cm_ca : z, r_mca, vo, 0, POL);
                                __builtin_amdgcn_raw_buffer_store_b128((w & 4u) ? cm_cb : z, r_mcb, vo, 0, POL);
                                __builtin_amdgcn_raw_buffer_store_b128((w & 1u) ? cm_o : z, r_mno, vo, 0, POL);
                            }
                        }
                    }
                }
                // !VEC: the last strip of a row may have fewer than NC live column groups (64 columns each) -- the chains of
                // the dead ones are not evaluated (N = 129 at NC = 4: three of four; N = 300 at NC = 2: one of two)
                int i_from = i0;
                auto sweep_rows = [&](auto ncl_tag) {
                constexpr int L = decltype(ncl_tag)::value;
                for (int i = i_from; i < i1; i += 2) {
                    const int r = i >> 1;
                    const bool two = i + 1 < i1;                  // the last row of an odd N has no partner (uniform)
                    const f3v nv = {rowbuf[r * 9 + 0], rowbuf[r * 9 + 1], rowbuf[r * 9 + 2]};
                    const f3v cav = {rowbuf[r * 9 + 3], rowbuf[r * 9 + 4], rowbuf[r * 9 + 5]};
                    const f3v cbv = {rowbuf[r * 9 + 6], rowbuf[r * 9 + 7], rowbuf[r * 9 + 8]};
                    const int so = i * row_bytes;
                    // plane by plane, so that only one plane's results are live at a time; each plane's results are pinned
                    // before its store (see k3_sweep)
                    auto emit = [&](const __amdgpu_buffer_rsrc_t& rr, f32x2 (&v)[L]) {
#pragma unroll
                        for (int cc = 0; cc < L; ++cc) asm volatile("" : "+v"(v[cc]));
                        if constexpr (!VEC) {
#pragma unroll
                            for (int cc = 0; cc < L; ++cc)
                                if (lv[cc]) {
                                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[cc].x), rr, lane_off + 256 * cc, so, POL);
                                    if (two) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[cc].y), rr, lane_off + 256 * cc, so + row_bytes, POL);
                                }
                        } else if (live) {
                            if constexpr (NC == 4) {
                                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k3_u32x4, k3_f32x4{v[0].x, v[1].x, v[2].x, v[3].x}), rr, lane_off, so, POL);
                                if (two) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k3_u32x4, k3_f32x4{v[0].y, v[1].y, v[2].y, v[3].y}), rr, lane_off, so + row_bytes, POL);
                            } else {
                                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].x, v[1].x}), rr, lane_off, so, POL);
                                if (two) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].y, v[1].y}), rr, lane_off, so + row_bytes, POL);
                            }
                        }
                    };
                    f3v NV[L], CAV[L], CBV[L], CAJ[L], CBJ[L];
                    f32x2 v[L];
#pragma unroll
                    for (int cc = 0; cc < L; ++cc) {
                        NV[cc] = nv; CAV[cc] = cav; CBV[cc] = cbv;
                        CAJ[cc] = mk3v(ca_j[cc], ca_j[cc]); CBJ[cc] = mk3v(cb_j[cc], cb_j[cc]);
                    }
#pragma unroll
                    for (int cc = 0; cc < L; ++cc) v[cc] = dist3v_t<EXACT>(cav, CAJ[cc]);
                    emit(r_dca, v);
#pragma unroll
                    for (int cc = 0; cc < L; ++cc) v[cc] = dist3v_t<EXACT>(cbv, CBJ[cc]);
                    emit(r_dcb, v);
#pragma unroll
                    for (int cc = 0; cc < L; ++cc) v[cc] = dist3v_t<EXACT>(nv, mk3v(o_j[cc], o_j[cc]));
                    emit(r_dno, v);
                    if constexpr (FAITHFUL) angle3v_ref_n<L>(CAV, CBV, CBJ, v);
                    else angle3v_n<L>(CAV, CBV, CBJ, v);
                    emit(r_ph, v);
                    if constexpr (FAITHFUL) dihedral4v_ref_n<L>(CAV, CBV, CAJ, CBJ, v);      // as coded at protstruc.py:811
                    else dihedral4v_k3_n<L>(CAV, CBV, CAJ, CBJ, v);
                    emit(r_om, v);
                    if constexpr (FAITHFUL) dihedral4v_ref_n<L>(NV, CAV, CBV, CBJ, v);
                    else dihedral4v_k3_n<L>(NV, CAV, CBV, CBJ, v);
                    emit(r_th, v);
                }
                };
                // One live column group (chains of up to 64 residues in the 64-apart layout): a lane has a single column, so its four
                // interleaved chains are four consecutive ROW PAIRS instead of four columns (round 5; with one chain per lane the
                // dependent instructions of a chain followed each other with nothing in between)
                auto sweep_rows_by_row_pairs = [&]() {
                    constexpr int R = 4;
                    const f3v caj = mk3v(ca_j[0], ca_j[0]), cbj = mk3v(cb_j[0], cb_j[0]), oj = mk3v(o_j[0], o_j[0]);
                    int i = i0;
                    for (; i + 2 * R <= i1; i += 2 * R) {
                        f3v NV[R], CAV[R], CBV[R], CAJ[R], CBJ[R];
                        f32x2 v[R];
#pragma unroll
                        for (int q = 0; q < R; ++q) {
                            const int r = (i >> 1) + q;
                            NV[q] = f3v{rowbuf[r * 9 + 0], rowbuf[r * 9 + 1], rowbuf[r * 9 + 2]};
                            CAV[q] = f3v{rowbuf[r * 9 + 3], rowbuf[r * 9 + 4], rowbuf[r * 9 + 5]};
                            CBV[q] = f3v{rowbuf[r * 9 + 6], rowbuf[r * 9 + 7], rowbuf[r * 9 + 8]};
                            CAJ[q] = caj; CBJ[q] = cbj;
                        }
                        const int so = i * row_bytes;
                        auto emit = [&](const __amdgpu_buffer_rsrc_t& rr, f32x2 (&w)[R]) {
#pragma unroll
                            for (int q = 0; q < R; ++q) asm volatile("" : "+v"(w[q]));
                            if (lv[0]) {
#pragma unroll
                                for (int q = 0; q < R; ++q) {
                                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(w[q].x), rr, lane_off, so + 2 * q * row_bytes, POL);
                                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(w[q].y), rr, lane_off, so + (2 * q + 1) * row_bytes, POL);
                                }
                            }
                        };
#pragma unroll
                        for (int q = 0; q < R; ++q) v[q] = dist3v_t<EXACT>(CAV[q], caj);
                        emit(r_dca, v);
#pragma unroll
                        for (int q = 0; q < R; ++q) v[q] = dist3v_t<EXACT>(CBV[q], cbj);
                        emit(r_dcb, v);
#pragma unroll
                        for (int q = 0; q < R; ++q) v[q] = dist3v_t<EXACT>(NV[q], oj);
                        emit(r_dno, v);
                        if constexpr (FAITHFUL) angle3v_ref_n<R>(CAV, CBV, CBJ, v);
                        else angle3v_n<R>(CAV, CBV, CBJ, v);
                        emit(r_ph, v);
                        if constexpr (FAITHFUL) dihedral4v_ref_n<R>(CAV, CBV, CAJ, CBJ, v);      // as coded at protstruc.py:811
                        else dihedral4v_k3_n<R>(CAV, CBV, CAJ, CBJ, v);
                        emit(r_om, v);
                        if constexpr (FAITHFUL) dihedral4v_ref_n<R>(NV, CAV, CBV, CBJ, v);
                        else dihedral4v_k3_n<R>(NV, CAV, CBV, CBJ, v);
                        emit(r_th, v);
                    }
                    i_from = i;                                    // the task's remaining rows (fewer than eight): one pair at a time
                    if (i < i1) sweep_rows(std::integral_constant<int, 1>{});
                };
                if constexpr (VEC) {
                    sweep_rows(std::integral_constant<int, NC>{});
                } else {
                    const int ncl = min(NC, (N - strip * 64 * NC + 63) >> 6);   // live column groups of this strip (uniform)
                    if ((NC == 4 || FAITHFUL) && ncl == 1 && N <= 64) sweep_rows_by_row_pairs();   // (the instantiations with 256 VGPRs)
                    else if (ncl == NC) sweep_rows(std::integral_constant<int, NC>{});
                    else if (NC == 4 && ncl == 3) sweep_rows(std::integral_constant<int, NC == 4 ? 3 : 1>{});
                    else if (NC == 4 && ncl == 2) sweep_rows(std::integral_constant<int, NC == 4 ? 2 : 1>{});
                    else sweep_rows(std::integral_constant<int, 1>{});
                }
            }
            if (++t >= t_end) {
                unsigned nx = 0;
                if (lane == 0) nx = atomicAdd(&next_task, (unsigned)pull);
                t = (unsigned)__builtin_amdgcn_readfirstlane((int)nx);
                t_end = min(t + (unsigned)pull, seg_t1);
            }
        }
    }
}

// The featuriser on the TILE map of k3_flat (round 5): a lane's element is two row pairs x two adjacent columns of one structure
// (four interleaved chains per feature), the N / CA / CB row atoms, CA / O / CB column atoms and the six mask bits per residue of
// KS structures staged per pass, two workgroups per CU, tasks of 64 tiles pulled from an LDS counter.  Chains of up to a few hundred
// residues: every lane has work whatever N is, what depends on a row pair or a column alone is shared inside the tile, and
// the set-up of a structure is paid once per KS structures.  Float planes: 8-byte stores of the tile's two columns (N even, planes
// 8-byte aligned; else dword stores); mask planes: two bytes per row of the tile (N even, planes 2-byte aligned; else bytes).
// Same arithmetic per pair as k3_inter_residue_geometry: same bits.
template <bool EXACT, bool FAITHFUL>
__global__ __launch_bounds__(512) void k3_featurise_tiles(
    const float* __restrict__ xyz, const uint8_t* __restrict__ amask, float* __restrict__ d_ca,
    float* __restrict__ d_cb, float* __restrict__ d_no, float* __restrict__ omega, float* __restrict__ theta,
    float* __restrict__ phi, uint8_t* __restrict__ m_ca, uint8_t* __restrict__ m_cb, uint8_t* __restrict__ m_no, int N,
    int A, int KS, unsigned tps, unsigned n_tasks, unsigned tasks_per_wg, unsigned rcpN, unsigned rcpTC, int slot_vec4, int vecf,
    int vecm) {
    // [slot]: column atoms CA, O, CB as {x, y, z, -} per (atom, residue): 3 N vec4; row atoms N, CA, CB pair-interleaved
    // {x0, x1, y0, y1}, {z0, z1, -, -} per (row pair, atom): 6 RP vec4; then one byte per residue: bits 0..2 = row side
    // (N, CA, CB present), bits 4..6 = column side (CA, CB, O present)
    extern __shared__ __attribute__((aligned(16))) k3_f32x4 k3_tilebuf[];
    __shared__ unsigned next_task;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned n_waves = blockDim.x >> 6;
    const unsigned t0 = blockIdx.x * tasks_per_wg, t1 = min(t0 + tasks_per_wg, n_tasks);
    if (t0 >= t1) return;                         // whole workgroup
    const int n_rp = (N + 1) >> 1;
    const int col_vec4 = 3 * N, row_vec4 = 6 * n_rp;
    // tiles of two row pairs x two columns -- or four (vecf == 4: N % 4 == 0, 16-byte float rows, 4-byte mask rows)
    const bool wide = vecf == 4;                  // (uniform)
    const unsigned TC = wide ? (unsigned)N >> 2 : (unsigned)(N + 1) >> 1, TR = (unsigned)(n_rp + 1) >> 1, FT = TR * TC;
    const unsigned b_first = t0 / tps, b_last = (t1 - 1u) / tps;
    for (unsigned bs = b_first; bs <= b_last; bs += (unsigned)KS) {
        const unsigned ks = min((unsigned)KS, b_last - bs + 1u);
        __syncthreads();                                          // the previous pass's readers are done
        for (unsigned it = threadIdx.x; it < ks * (unsigned)N; it += blockDim.x) {   // one residue of one structure per thread
            unsigned sidx = __umulhi(it, rcpN), r = it - sidx * (unsigned)N;
            if (r >= (unsigned)N) ++sidx, r -= (unsigned)N;
            const float* pr = xyz + ((size_t)(bs + sidx) * N + r) * (size_t)A * 3;
            k3_f32x4* slot = k3_tilebuf + (size_t)sidx * slot_vec4;
            const float v[15] = {pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[9], pr[10], pr[11], pr[12], pr[13], pr[14]};   // N, CA, O, CB
            unsigned bits = 0x77u;
            if (amask) {
                const uint8_t* mr = amask + ((size_t)(bs + sidx) * N + r) * A;
                const unsigned mn = mr[0] != 0, mca = mr[1] != 0, mo = mr[3] != 0, mcb = mr[4] != 0;
                bits = mn | (mca << 1) | (mcb << 2) | (mca << 4) | (mcb << 5) | (mo << 6);
            }
            slot[0 * N + (int)r] = k3_f32x4{v[3], v[4], v[5], 0.0f};        // CA
            slot[1 * N + (int)r] = k3_f32x4{v[6], v[7], v[8], 0.0f};        // O
            slot[2 * N + (int)r] = k3_f32x4{v[9], v[10], v[11], 0.0f};      // CB
            float* rb = reinterpret_cast<float*>(slot + col_vec4) + (size_t)(r >> 1) * 24 + (r & 1);
            rb[0] = v[0]; rb[2] = v[1]; rb[4] = v[2];                       // N
            rb[8] = v[3]; rb[10] = v[4]; rb[12] = v[5];                     // CA
            rb[16] = v[9]; rb[18] = v[10]; rb[20] = v[11];                  // CB
            reinterpret_cast<uint8_t*>(slot + col_vec4 + row_vec4)[r] = (uint8_t)bits;
        }
        const unsigned seg_t0 = max(t0, bs * tps), seg_t1 = min(t1, (bs + ks) * tps);
        if (threadIdx.x == 0) next_task = seg_t0 + n_waves;       // the first n_waves tasks are pre-assigned
        __syncthreads();
        unsigned t = seg_t0 + (unsigned)wave;
        while (t < seg_t1) {
            const unsigned b = t / tps, chunk = t - b * tps;      // (uniform)
            const k3_f32x4* slot = k3_tilebuf + (size_t)(b - bs) * slot_vec4;
            const k3_f32x4* rowp = slot + col_vec4;
            const uint8_t* mbits = reinterpret_cast<const uint8_t*>(slot + col_vec4 + row_vec4);
            const size_t sbase = (size_t)b * N * N;
            auto rs = [&](void* base, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x00020000u); };
            const unsigned fbytes = (unsigned)N * (unsigned)N * 4u, mbytes = (unsigned)N * (unsigned)N;   // this structure's planes, exactly
            const __amdgpu_buffer_rsrc_t r_dca = rs(d_ca + sbase, fbytes), r_dcb = rs(d_cb + sbase, fbytes), r_dno = rs(d_no + sbase, fbytes),
                                         r_om = rs(omega + sbase, fbytes), r_th = rs(theta + sbase, fbytes), r_ph = rs(phi + sbase, fbytes);
            const __amdgpu_buffer_rsrc_t r_mca = rs(m_ca + sbase, mbytes), r_mcb = rs(m_cb + sbase, mbytes), r_mno = rs(m_no + sbase, mbytes);
            const unsigned ti = chunk * 64u + (unsigned)lane;
            const bool lt = ti < FT;
            const unsigned tcl = min(ti, FT - 1u);
            unsigned tr = __umulhi(tcl, rcpTC), tc = tcl - tr * TC;
            if (tc >= TC) ++tr, tc -= TC;
            const int c0 = (int)(wide ? 4u * tc : 2u * tc);
            const int rpA = (int)(2u * tr), rpB = min(rpA + 1, n_rp - 1);
            const bool lc1 = c0 + 1 < N, lrB = rpA + 1 < n_rp;
            // rows 2 rpA (always there), 2 rpA + 1, 2 rpB, 2 rpB + 1
            const int iA0 = 2 * rpA, iA1 = min(iA0 + 1, N - 1), iB0 = 2 * rpB, iB1 = min(iB0 + 1, N - 1);
            const bool rA1 = iA0 + 1 < N, rB0 = lrB, rB1 = lrB && iB0 + 1 < N;
            // chain c of a half: row pair A (c = 0, 1) or B (2, 3) x the half's first / second column; .x / .y = the pair's rows
            f3v NV[4], CAV[4], CBV[4], CAJ[2][4], CBJ[2][4], OJ[2][4];
            {
                auto row_atom = [&](int rp, int q) {
                    const k3_f32x4 xy = rowp[(rp * 3 + q) * 2];
                    const f32x2 z = *reinterpret_cast<const f32x2*>(rowp + (rp * 3 + q) * 2 + 1);
                    return f3v{f32x2{xy.x, xy.y}, f32x2{xy.z, xy.w}, z};
                };
                NV[0] = NV[1] = row_atom(rpA, 0); CAV[0] = CAV[1] = row_atom(rpA, 1); CBV[0] = CBV[1] = row_atom(rpA, 2);
                NV[2] = NV[3] = row_atom(rpB, 0); CAV[2] = CAV[3] = row_atom(rpB, 1); CBV[2] = CBV[3] = row_atom(rpB, 2);
                auto cols = [&](int ca, f3v (&CA)[4], f3v (&CB)[4], f3v (&O)[4]) {
                    const int cb = min(ca + 1, N - 1);            // clamped: a dead column is never stored
                    const k3_f32x4 ca0 = slot[ca], ca1 = slot[cb], o0 = slot[N + ca], o1 = slot[N + cb], cb0 = slot[2 * N + ca], cb1 = slot[2 * N + cb];
                    CA[0] = CA[2] = mk3v(f3{ca0.x, ca0.y, ca0.z}, f3{ca0.x, ca0.y, ca0.z});
                    CA[1] = CA[3] = mk3v(f3{ca1.x, ca1.y, ca1.z}, f3{ca1.x, ca1.y, ca1.z});
                    O[0] = O[2] = mk3v(f3{o0.x, o0.y, o0.z}, f3{o0.x, o0.y, o0.z});
                    O[1] = O[3] = mk3v(f3{o1.x, o1.y, o1.z}, f3{o1.x, o1.y, o1.z});
                    CB[0] = CB[2] = mk3v(f3{cb0.x, cb0.y, cb0.z}, f3{cb0.x, cb0.y, cb0.z});
                    CB[1] = CB[3] = mk3v(f3{cb1.x, cb1.y, cb1.z}, f3{cb1.x, cb1.y, cb1.z});
                };
                cols(c0, CAJ[0], CBJ[0], OJ[0]);
                cols(wide ? c0 + 2 : c0, CAJ[1], CBJ[1], OJ[1]);   // (the second half exists only in a four-column tile)
            }
            constexpr int DEAD = 0x7FFFFFF0;    // beyond num_records: dropped by the range check
            const int offA = (int)__umul24((unsigned)iA0, (unsigned)N) + c0, offB = (int)__umul24((unsigned)iB0, (unsigned)N) + c0;   // in elements
            const bool l1 = lt && lc1;
            // one plane's chains: v = the tile's first two columns, w = its third and fourth (four-column tiles only)
            auto emit = [&](const __amdgpu_buffer_rsrc_t& rr, f32x2 (&v)[4], f32x2 (&w)[4]) {
#pragma unroll
                for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(v[c]));
                if (wide) {      // (uniform) a row of the tile is one 16-byte store
#pragma unroll
                    for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(w[c]));
                    auto st4 = [&](float a, float b, float c, float d, int off) {
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k3_u32x4, k3_f32x4{a, b, c, d}), rr, off, 0, 0);
                    };
                    st4(v[0].x, v[1].x, w[0].x, w[1].x, lt ? offA * 4 : DEAD);
                    st4(v[0].y, v[1].y, w[0].y, w[1].y, (lt && rA1) ? (offA + N) * 4 : DEAD);
                    st4(v[2].x, v[3].x, w[2].x, w[3].x, (lt && rB0) ? offB * 4 : DEAD);
                    st4(v[2].y, v[3].y, w[2].y, w[3].y, (lt && rB1) ? (offB + N) * 4 : DEAD);
                } else if (vecf == 2) {
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].x, v[1].x}), rr, lt ? offA * 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].y, v[1].y}), rr, (lt && rA1) ? (offA + N) * 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[2].x, v[3].x}), rr, (lt && rB0) ? offB * 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[2].y, v[3].y}), rr, (lt && rB1) ? (offB + N) * 4 : DEAD, 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[0].x), rr, lt ? offA * 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[1].x), rr, l1 ? offA * 4 + 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[0].y), rr, (lt && rA1) ? (offA + N) * 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[1].y), rr, (l1 && rA1) ? (offA + N) * 4 + 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[2].x), rr, (lt && rB0) ? offB * 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[3].x), rr, (l1 && rB0) ? offB * 4 + 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[2].y), rr, (lt && rB1) ? (offB + N) * 4 : DEAD, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[3].y), rr, (l1 && rB1) ? (offB + N) * 4 + 4 : DEAD, 0, 0);
                }
            };
            // the three mask planes first (their stores drain while the arithmetic runs): rows' bits 0..2 = N, CA, CB; columns' bits 4..6 = CA, CB, O
            {
                const unsigned mA0 = mbits[iA0], mA1 = mbits[iA1], mB0 = mbits[iB0], mB1 = mbits[iB1];
                const unsigned mc0 = mbits[c0] >> 4, mc1 = mbits[min(c0 + 1, N - 1)] >> 4;
                const unsigned mc2 = mbits[min(c0 + 2, N - 1)] >> 4, mc3 = mbits[min(c0 + 3, N - 1)] >> 4;   // (four-column tiles)
                auto plane = [&](const __amdgpu_buffer_rsrc_t& rr, unsigned rbit, unsigned cbit) {
                    const unsigned k0 = (mc0 >> cbit) & 1u, k1 = (mc1 >> cbit) & 1u;
                    const unsigned a0 = (mA0 >> rbit) & 1u, a1 = (mA1 >> rbit) & 1u, b0 = (mB0 >> rbit) & 1u, b1 = (mB1 >> rbit) & 1u;
                    if (wide) {      // (uniform) four bytes per row of the tile
                        const unsigned kk = k0 | (k1 << 8) | (((mc2 >> cbit) & 1u) << 16) | (((mc3 >> cbit) & 1u) << 24);
                        __builtin_amdgcn_raw_buffer_store_b32(a0 ? kk : 0u, rr, lt ? offA : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(a1 ? kk : 0u, rr, (lt && rA1) ? offA + N : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(b0 ? kk : 0u, rr, (lt && rB0) ? offB : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(b1 ? kk : 0u, rr, (lt && rB1) ? offB + N : DEAD, 0, 0);
                    } else if (vecm == 2) {     // (uniform) two bytes per row of the tile
                        const unsigned kk = k0 | (k1 << 8);
                        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(a0 ? kk : 0u), rr, lt ? offA : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(a1 ? kk : 0u), rr, (lt && rA1) ? offA + N : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(b0 ? kk : 0u), rr, (lt && rB0) ? offB : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(b1 ? kk : 0u), rr, (lt && rB1) ? offB + N : DEAD, 0, 0);
                    } else {
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(a0 & k0), rr, lt ? offA : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(a0 & k1), rr, l1 ? offA + 1 : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(a1 & k0), rr, (lt && rA1) ? offA + N : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(a1 & k1), rr, (l1 && rA1) ? offA + N + 1 : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(b0 & k0), rr, (lt && rB0) ? offB : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(b0 & k1), rr, (l1 && rB0) ? offB + 1 : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(b1 & k0), rr, (lt && rB1) ? offB + N : DEAD, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)(b1 & k1), rr, (l1 && rB1) ? offB + N + 1 : DEAD, 0, 0);
                    }
                };
                plane(r_mca, 1u, 0u);      // CA_i & CA_j
                plane(r_mcb, 2u, 1u);      // CB_i & CB_j
                plane(r_mno, 0u, 2u);      // N_i & O_j
            }
            f32x2 v[4], w[4];
            // each plane: the first half's four chains, the second half's (four-column tiles), the stores
#define K3F_TILE_PLANE(RSRC, EXPR0, EXPR1)      \
            { EXPR0; if (wide) { EXPR1; } emit(RSRC, v, w); }
#define K3F_DIST(R, C, OUT) _Pragma("unroll") for (int c = 0; c < 4; ++c) OUT[c] = dist3v_t<EXACT>(R[c], C[c])
            K3F_TILE_PLANE(r_dca, K3F_DIST(CAV, CAJ[0], v), K3F_DIST(CAV, CAJ[1], w))
            K3F_TILE_PLANE(r_dcb, K3F_DIST(CBV, CBJ[0], v), K3F_DIST(CBV, CBJ[1], w))
            K3F_TILE_PLANE(r_dno, K3F_DIST(NV, OJ[0], v), K3F_DIST(NV, OJ[1], w))
            if constexpr (FAITHFUL) {
                K3F_TILE_PLANE(r_ph, angle3v_ref_n<4>(CAV, CBV, CBJ[0], v), angle3v_ref_n<4>(CAV, CBV, CBJ[1], w))
                K3F_TILE_PLANE(r_om, dihedral4v_ref_n<4>(CAV, CBV, CAJ[0], CBJ[0], v), dihedral4v_ref_n<4>(CAV, CBV, CAJ[1], CBJ[1], w))   // as coded at protstruc.py:811
                K3F_TILE_PLANE(r_th, dihedral4v_ref_n<4>(NV, CAV, CBV, CBJ[0], v), dihedral4v_ref_n<4>(NV, CAV, CBV, CBJ[1], w))
            } else {
                K3F_TILE_PLANE(r_ph, angle3v_n<4>(CAV, CBV, CBJ[0], v), angle3v_n<4>(CAV, CBV, CBJ[1], w))
                K3F_TILE_PLANE(r_om, dihedral4v_k3_n<4>(CAV, CBV, CAJ[0], CBJ[0], v), dihedral4v_k3_n<4>(CAV, CBV, CAJ[1], CBJ[1], w))
                K3F_TILE_PLANE(r_th, dihedral4v_k3_n<4>(NV, CAV, CBV, CBJ[0], v), dihedral4v_k3_n<4>(NV, CAV, CBV, CBJ[1], w))
            }
#undef K3F_DIST
#undef K3F_TILE_PLANE
            unsigned nx = 0;
            if (lane == 0) nx = atomicAdd(&next_task, 1u);
            t = (unsigned)__builtin_amdgcn_readfirstlane((int)nx);
        }
    }
}

// ---- thresholds and launchers (every launch goes through k3_go: launch or record, k3_launch.hpp) ----
// The per-CU sweep (tasks of two rows, a structure's column points in LDS, two workgroups per CU, and since round 5
// several structures per staging pass) pays from 40 residues on (K3's sweeps, pairwise_angles.hip: from 100): same-box, 2^25 pairs, min of 20 launches, sweep / one-column kernel:
// N = 63 276 / 344 us, 56 306 / 352, 48 333 / 371, 40 386 / 417, 33 480 / 449 (profiles/r05_featuriser_shapes.log)
constexpr int K3_FEATURISE_MIN_N = 40;
// the featuriser's tile kernel: chain lengths it takes (same-box A/B against the sweep and the one-column kernel: profiles/r05_featuriser_shapes.log)
// same box, 2^25 pairs, min of 20 launches, tiles / product before: N = 16 428 / 666 us, 24 372 / 605, 33 363 / 433, 40 271 / 355,
// 48 258 / 297, 64 224 / 234, 80 233 / 277, 99 265 / 267, 100 243-275 / 252, 129 262 / 339, 160 211 / 280, 200 221-245 / 232;
// the sweep wins where its lanes are full (128: 185 against 206, 256: 161 / 194) and at odd lengths above ~100 (101: 272 / 288:
// the tiles' stores are dwords and bytes there)
constexpr int K3F_TILES_MIN_N = 8, K3F_TILES_MAX_N = 96;     // every chain of 8 .. 96 residues ...
constexpr int K3F_TILES_MAX_N_EVEN = 200, K3F_TILES_UTIL_PERCENT = 85;   // ... and even lengths up to 200 where < 85 % of the sweep's lanes would have a column

// The arguments of one featuriser call (a plan query leaves the pointers NULL).  alf / alm: the low seven bits of the float /
// mask planes' addresses, OR-ed over the planes.
struct K3fCall {
    const float* xyz;
    const uint8_t* amask;
    float *d_ca, *d_cb, *d_no, *omega, *theta, *phi;
    uint8_t *m_ca, *m_cb, *m_no;
    int B, N, A, exact_sqrt;
    uintptr_t alf, alm;
};

// argument checks shared by the featuriser's launcher and its plan query
inline int k3f_check_args(int B, int N, int A, int exact_sqrt, int exact_angles) {
    if (B < 0 || N < 0 || A < 5 || (exact_sqrt != 0 && exact_sqrt != 1) || exact_angles < 0 || exact_angles > 3)
        return (int)hipErrorInvalidValue;
    return 0;
}

// The featuriser sweep's layout for a chain length and float-plane alignment: vector float stores where rows and planes allow
// (else 64 consecutive floats per store instruction: any N); columns per lane by the lanes a strip wastes
struct K3fSweepLayout {
    int nc;
    bool vec;
};
template <bool FAITHFUL>
inline K3fSweepLayout k3f_sweep_layout(int N, uintptr_t alf) {
    const bool v4 = N % 4 == 0 && (alf & 15u) == 0, v2 = N % 2 == 0 && (alf & 7u) == 0;
    const long long w4 = (long long)((N + 255) / 256) * 256, w2 = (long long)((N + 127) / 128) * 128;
    // ... or none at all: with the 64-floats-per-store layout the dead column groups of a row's last strip are skipped, so
    // it computes ceil(N / 64) groups per row pair where the vector layouts compute whole strips (N = 140: 3 against 4,
    // 342 against 376 us at 2^25 pairs) -- taken where that saves more than the ~15 % its dword stores cost
    // four columns per lane: 512-thread workgroups (two waves per SIMD, 256 VGPRs each)
    constexpr bool CAN4 = !FAITHFUL;   // (the faithful chains of four columns do not fit 256 VGPRs)
    const long long gn = (N + 63) / 64, gv = (CAN4 ? std::min(w4, w2) : w2) / 64;
    const bool prefer_scalar = gn * 115 < gv * 100;
    int NC = (CAN4 && w4 <= w2) ? 4 : 2;
    const bool vec = (NC == 4 ? v4 : v2) && !prefer_scalar;
    // ... in which four columns per lane beat two from three groups on (same-box A/B: N = 383 234 against 260 us, 301
    // 257 / 267; two groups, N = 101: 338 / 310)
    if (!vec) NC = (CAN4 && (gn > 2 || N <= 64)) ? 4 : 2;   // (N <= 64: one column group, four row pairs per lane -- the 256-VGPR instantiation)
    return K3fSweepLayout{NC, vec};
}

// LDS of one structure in the tile kernel, in 16-byte units: column atoms, row atoms, one byte per residue
inline size_t k3f_tiles_slot_vec4(int N) { return (size_t)3 * N + (size_t)6 * ((N + 1) / 2) + ((size_t)N + 15) / 16; }

// The tile kernel (several structures per pass, every lane busy): chains of K3F_TILES_MIN_N .. K3F_TILES_MAX_N residues, and ...
template <bool FAITHFUL>
inline bool k3f_tiles_eligible(const K3fCall& c) {
    const int N = c.N;
    const uintptr_t alf = c.alf, alm = c.alm;
    // (odd lengths -- dword and byte stores in the tile kernel -- only below 70 %: N = 129 262 against 339 us, but 101 288 against 272)
    const bool tiles_even = N <= K3F_TILES_MAX_N_EVEN && (long long)N * 100 < (long long)(N % 2 == 0 ? K3F_TILES_UTIL_PERCENT : 70) * 64 * ((N + 63) / 64);
    // ... and even lengths whose sweep would fall back to its 64-floats-per-store layout (three or five column groups: N = 176,
    // 192, 272 .. 320): the tiles keep their 8-byte stores (192: 222 against 289 us, 288: 216-255 / 318, 320: 232 / 300,
    // profiles/r05_featuriser_shapes.log)
    const bool tiles_dword_sweep = N % 2 == 0 && (alf & 7u) == 0 && (alm & 1u) == 0 && !k3f_sweep_layout<FAITHFUL>(N, alf).vec;
    // ... and, in the faithful arithmetic (whose sweep has two columns per lane), every length with four-column tiles: level
    // with the sweep at 192 / 256 / 320 / 384, 5-12 % faster at 128, 224, 352, 448-500 (profiles/r05_featuriser_tile_width.log)
    const bool tiles_faithful = FAITHFUL && N % 4 == 0 && (alf & 15u) == 0 && (alm & 3u) == 0;
    return N >= K3F_TILES_MIN_N && (N <= K3F_TILES_MAX_N || tiles_even || tiles_dword_sweep || tiles_faithful) && (alf & 3u) == 0 &&
           k3f_tiles_slot_vec4(N) * 16 <= 48 * 1024 && (unsigned long long)N * N < (1ull << 29);
}

template <bool FAITHFUL>
int launch_featurise_tiles(const K3fCall& c, const K3Go& go) {
    const int N = c.N, n_rp = (N + 1) / 2;
    const uintptr_t alf = c.alf, alm = c.alm;
    const size_t slot_vec4 = k3f_tiles_slot_vec4(N);
    // four-column tiles where a row of the tile is one 16-byte float store and one 4-byte mask store and they pay
    const unsigned TR = (unsigned)(n_rp + 1) / 2;
    int vecf = (N % 2 == 0 && (alf & 7u) == 0) ? 2 : 0, vecm = (N % 2 == 0 && (alm & 1u) == 0) ? 2 : 0;
    if (N % 4 == 0 && (alf & 15u) == 0 && (alm & 3u) == 0 && k3_wide_tiles_pay(TR, N)) vecf = vecm = 4;
    const unsigned TC = vecf == 4 ? (unsigned)N / 4 : (unsigned)(N + 1) / 2;
    const unsigned tps = (TR * TC + 63u) / 64u;
    const unsigned long long n_tasks = (unsigned long long)tps * c.B;
    if (n_tasks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    // two 256-thread workgroups per CU (their LDS requests admit exactly that many; 132 / 167 VGPRs: three waves per SIMD;
    // 2 / 3 / 4 workgroups per CU: no difference beyond noise), one workgroup per resident slot
    const size_t tiles_lds = K3_LDS_TWO_PER_CU;
    const unsigned slots = (unsigned)go.cus * 2u;
    const unsigned tasks_per_wg = (unsigned)std::max<unsigned long long>((n_tasks + slots - 1) / slots, 4ull);
    const unsigned grid = (unsigned)((n_tasks + tasks_per_wg - 1) / tasks_per_wg);
    const unsigned share = (tasks_per_wg + tps - 1) / tps + 1;
    const int KS = (int)std::max<size_t>(1, std::min<size_t>(tiles_lds / (slot_vec4 * 16), (share + 3) / 4));
    char name[96];
    snprintf(name, sizeof name, "k3_featurise_tiles<EXACT=%d,FAITHFUL=%d>", c.exact_sqrt, (int)FAITHFUL);
    K3Shape sh;
    sh.nc = 4; sh.vec = vecf / 2; sh.skips = 1; sh.mask_mode = vecm == 4 ? 4 : vecm == 2 ? 3 : 0; sh.faithful = FAITHFUL; sh.wgs_per_cu = 2; sh.structs_per_segment = KS;
    sh.n_tasks = (unsigned)n_tasks; sh.tasks_per_wg = tasks_per_wg;
    static unsigned long long prep[2][1] = {{0}, {0}};
    auto tiles = [&](auto kernel, unsigned long long (&prepared)[1]) {
        return k3_go(go, "featurise_tiles", name, sh, kernel, &prepared, dim3(grid), dim3(256), tiles_lds, 4u, c.xyz, c.amask, c.d_ca, c.d_cb,
                     c.d_no, c.omega, c.theta, c.phi, c.m_ca, c.m_cb, c.m_no, N, c.A, KS, tps, (unsigned)n_tasks, tasks_per_wg,
                     (unsigned)((1ull << 32) / (unsigned)N), (unsigned)((1ull << 32) / std::max(1u, TC)), (int)slot_vec4, vecf, vecm);
    };
    return c.exact_sqrt ? tiles(k3_featurise_tiles<true, FAITHFUL>, prep[0]) : tiles(k3_featurise_tiles<false, FAITHFUL>, prep[1]);
}

// LDS of one structure in the featuriser's sweep: its rows (points + mask words), its column points, its column masks (bytes or bit sets)
inline size_t k3f_sweep_need(int N) {
    return (size_t)((N + 2) / 2) * (9 * 8 + 4) + 32 + 16 + (size_t)((N + 3) & ~3) * 36 +
           std::max<size_t>(3 * (size_t)N, 3 * ((size_t)(N + 31) / 32 + 2) * 4) + 16;
}

// the per-CU sweep: any N >= K3_FEATURISE_MIN_N whose rows fit in LDS
inline bool k3f_sweep_eligible(const K3fCall& c) {
    return c.N >= K3_FEATURISE_MIN_N && k3f_sweep_need(c.N) <= K3_LDS_MAX && (c.alf & 3u) == 0 && (unsigned long long)c.N * c.N < (1ull << 31);
}

template <bool FAITHFUL>
int launch_featurise_sweep(const K3fCall& c, const K3Go& go) {
    const int N = c.N, cus = go.cus;
    const uintptr_t alf = c.alf, alm = c.alm;
    const size_t need = k3f_sweep_need(N);
    constexpr bool CAN4 = !FAITHFUL;   // (as in k3f_sweep_layout)
    const K3fSweepLayout lay = k3f_sweep_layout<FAITHFUL>(N, alf);
    const int NC = lay.nc;
    const bool vec = lay.vec;
    const bool m16 = vec && N % 16 == 0 && (alm & 15u) == 0;   // strip-local 16-byte mask stores: whole 16-column groups
    // write-through where strips are whole and every store covers whole lines; same-box A/B, trace: N = 512 174 against 178 us,
    // 256 181 / 187 -- but N = 480 (15 lines per row, a 224-column second strip) 239 against 212 and 160 308 / 297: there write-back
    const bool wt = m16 && N % 128 == 0 && (alf & 127u) == 0 && (alm & 127u) == 0;
    const int n_strips = (N + 64 * NC - 1) / (64 * NC);
    // a task is CH rows x one strip, the strips of a row chunk adjacent tasks: a workgroup's share has to be many tasks
    // per wave whatever B and N are -- its waves wait for each other at every structure boundary for up to one task.
    // Four rows with the M16 mask stores (four rows per instruction; rows are whole 64-byte segments there).  TWO
    // otherwise: where rows are not whole segments, the segment a row's strips share and the one a row's end shares with
    // the next row's start get their halves from adjacent tasks, i.e. from two waves up to a task apart -- with
    // four-row tasks (~16 us) longer than a line stays in L2 at this store rate, so that half of them went out as two
    // partial writes (2.2 % of the write requests at N = 500, none at N = 496: profiles/r04_featuriser_pmc.log);
    // same-box A/B, trace: N = 500 260 -> 228 us, 511 264 -> 241, 255 238 -> 218.
    const bool two_wg = (unsigned long long)c.B >= 4ull * cus;
    // (chains of up to 64 residues in the 64-apart layout: eight rows, so that a lane's four chains are four row pairs)
    const int CH = m16 ? 4 : (!vec && N <= 64) ? 8 : 2;
    const int n_chunks = (N + CH - 1) / CH;
    const unsigned long long n_tasks = (unsigned long long)n_chunks * n_strips * c.B;
    if (n_tasks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    // One workgroup per CU -- or, when a CU's share is four or more structures (chains of ~128 residues in large
    // batches), TWO of half the width: staging a structure (two barriers, a round trip to L2 for its rows and column
    // points) idles all of a workgroup's waves, and the other workgroup computes meanwhile.  Their LDS requests admit
    // exactly one / two per CU.
    const bool two = two_wg && need <= K3_LDS_TWO_PER_CU;
    const int wgs = two ? 2 * cus : cus;
    const unsigned tasks_per_wg = (unsigned)std::max<unsigned long long>((n_tasks + wgs - 1) / wgs, 4ull);
    const unsigned grid = (unsigned)((n_tasks + tasks_per_wg - 1) / tasks_per_wg);
    const size_t dyn = two ? K3_LDS_TWO_PER_CU : std::max(need, K3_LDS_ONE_PER_CU);
    // structures per staging pass (round 5): what the LDS request holds, at most a quarter of a workgroup's share (so that
    // the workgroups of a CU interleave their passes) -- short chains paid two barriers and a round trip to L2 per structure
    const size_t slot_bytes = (need + 15) & ~(size_t)15;
    const unsigned long long n_sub = (unsigned long long)n_chunks * n_strips;
    const unsigned long long share = (tasks_per_wg + n_sub - 1) / n_sub + 1;
    const int KS = (int)std::max<unsigned long long>(1, std::min<unsigned long long>(dyn / slot_bytes, (share + 3) / 4));
    const unsigned rcpN = (unsigned)((1ull << 32) / (unsigned)N);
    // four columns per lane need ~200 VGPRs (three column points x four columns + four interleaved chains): 8 waves; so do
    // the faithful chains of two columns
    const dim3 block((unsigned)(((NC == 4 || FAITHFUL) ? 512 : 1024) >> (two ? 1 : 0)));
    K3Shape sh;
    sh.nc = NC; sh.vec = vec; sh.skips = !vec; sh.mask_mode = m16 ? 2 : 1; sh.wt = wt; sh.faithful = FAITHFUL; sh.rows_per_task = CH;
    sh.wgs_per_cu = two ? 2 : 1; sh.structs_per_segment = KS; sh.n_tasks = (unsigned)n_tasks; sh.tasks_per_wg = tasks_per_wg;
    // one instantiation by its switches (the kernel's last argument: tasks a wave pulls at a time)
    auto sweep = [&](auto nc_, auto vec_, auto m16_, auto wt_) {
        constexpr int NC_ = nc_;
        constexpr bool VEC_ = vec_, M16_ = m16_, WT_ = wt_;
        static unsigned long long prep[2][1] = {{0}, {0}};   // (per instantiation of this lambda, i.e. per kernel)
        char name[96];
        snprintf(name, sizeof name, "k3_featurise<EXACT=%d,NC=%d,VEC=%d,M16=%d,WT=%d,FAITHFUL=%d>", (int)(c.exact_sqrt != 0), NC_, (int)VEC_, (int)M16_,
                 (int)WT_, (int)FAITHFUL);
        auto run = [&](auto kernel, unsigned long long (&prepared)[1]) {
            return k3_go(go, "featurise", name, sh, kernel, &prepared, dim3(grid), block, dyn, 4u, c.xyz, c.amask, c.d_ca, c.d_cb, c.d_no, c.omega,
                         c.theta, c.phi, c.m_ca, c.m_cb, c.m_no, N, c.A, CH, n_strips, n_chunks, (unsigned)n_tasks, tasks_per_wg, rcpN, KS,
                         (int)slot_bytes, 1);
        };
        return c.exact_sqrt ? run(k3_featurise<true, NC_, VEC_, M16_, WT_, FAITHFUL>, prep[0])
                            : run(k3_featurise<false, NC_, VEC_, M16_, WT_, FAITHFUL>, prep[1]);
    };
    using C2 = std::integral_constant<int, 2>;
    using C4 = std::integral_constant<int, 4>;
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (wt && NC == 2) return sweep(C2{}, yes, yes, yes);
    if (m16 && NC == 2) return sweep(C2{}, yes, yes, no);
    if constexpr (CAN4) {
        if (wt) return sweep(C4{}, yes, yes, yes);
        if (m16) return sweep(C4{}, yes, yes, no);
        if (NC == 4) return vec ? sweep(C4{}, yes, no, no) : sweep(C4{}, no, no, no);
    }
    return vec ? sweep(C2{}, yes, no, no) : sweep(C2{}, no, no, no);
}

template <bool FAITHFUL>
int launch_featurise_one_column(const K3fCall& c, const K3Go& go) {
    const int N = c.N, IR = 16, thr1 = k3_one_column_threads(N);
    const int n_tiles = (N + thr1 - 1) / thr1, n_chunks = (N + IR - 1) / IR;
    const unsigned long long n_wg = (unsigned long long)n_tiles * n_chunks * c.B;
    if (n_wg > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    char name[96];
    snprintf(name, sizeof name, "k3_inter_residue_geometry<EXACT=%d,FAITHFUL=%d>", c.exact_sqrt, (int)FAITHFUL);
    K3Shape sh;
    sh.faithful = FAITHFUL; sh.rows_per_task = IR;
    auto one = [&](auto kernel) {
        return k3_go(go, "one_column", name, sh, kernel, nullptr, dim3((unsigned)n_wg), dim3(thr1), 0, 0u, c.xyz, c.amask, c.d_ca, c.d_cb, c.d_no,
                     c.omega, c.theta, c.phi, c.m_ca, c.m_cb, c.m_no, N, c.A, IR, n_tiles, n_chunks);
    };
    return c.exact_sqrt ? one(k3_inter_residue_geometry<true, FAITHFUL>) : one(k3_inter_residue_geometry<false, FAITHFUL>);
}

// exact_angles of the C ABI as for K3: bit 0 = FAITHFUL, bit 1 = the one-column kernel whatever the shape
inline int k3f_run(const K3fCall& c, int exact_angles, const K3Go& go) {
    const bool faithful = (exact_angles & 1) != 0, simple = (exact_angles & 2) != 0;
    if (!simple && (faithful ? k3f_tiles_eligible<true>(c) : k3f_tiles_eligible<false>(c)))
        return faithful ? launch_featurise_tiles<true>(c, go) : launch_featurise_tiles<false>(c, go);
    if (!simple && k3f_sweep_eligible(c)) return faithful ? launch_featurise_sweep<true>(c, go) : launch_featurise_sweep<false>(c, go);
    return faithful ? launch_featurise_one_column<true>(c, go) : launch_featurise_one_column<false>(c, go);
}

}  // namespace

extern "C" int ps_inter_residue_geometry_f32(const float* xyz, const uint8_t* atom_mask, float* d_ca, float* d_cb,
                                             float* d_no, float* omega, float* theta, float* phi, uint8_t* d_ca_mask,
                                             uint8_t* d_cb_mask, uint8_t* d_no_mask, int B, int N, int A,
                                             int exact_sqrt, int exact_angles, void* stream) {
    if (!xyz || !d_ca || !d_cb || !d_no || !omega || !theta || !phi || !d_ca_mask || !d_cb_mask || !d_no_mask)
        return (int)hipErrorInvalidValue;
    if (const int e = k3f_check_args(B, N, A, exact_sqrt, exact_angles)) return e;
    if (B == 0 || N == 0) return 0;
    uintptr_t alf = 0, alm = 0;
    for (const void* p : {(const void*)d_ca, (const void*)d_cb, (const void*)d_no, (const void*)omega, (const void*)theta, (const void*)phi})
        alf |= reinterpret_cast<uintptr_t>(p);
    for (const void* p : {(const void*)d_ca_mask, (const void*)d_cb_mask, (const void*)d_no_mask}) alm |= reinterpret_cast<uintptr_t>(p);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const K3fCall c{xyz, atom_mask, d_ca, d_cb, d_no, omega, theta, phi, d_ca_mask, d_cb_mask, d_no_mask, B, N, A, exact_sqrt, alf & 127u, alm & 127u};
    return k3f_run(c, exact_angles, K3Go{s, nullptr, k3_cu_count(s)});
}

extern "C" int ps_featuriser_plan_f32(int B, int N, int A, int float_misalign, int mask_misalign, int exact_sqrt, int exact_angles,
                                      int cu_count, ps_k3_plan* plan) {
    if (!plan || plan->struct_size != (int)sizeof(ps_k3_plan)) return (int)hipErrorInvalidValue;
    k3_plan_reset(plan);
    if (const int e = k3f_check_args(B, N, A, exact_sqrt, exact_angles)) return e;
    if (float_misalign < 0 || float_misalign > 127 || mask_misalign < 0 || mask_misalign > 127) return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0) return 0;
    K3fCall c{};
    c.B = B, c.N = N, c.A = A, c.exact_sqrt = exact_sqrt, c.alf = (uintptr_t)float_misalign, c.alm = (uintptr_t)mask_misalign;
    return k3f_run(c, exact_angles, K3Go{nullptr, plan, cu_count > 0 ? cu_count : 256});
}
