// K3 -- inter-residue dihedrals and planar angles over all residue pairs.
// Replaces StructureBatch.pairwise_dihedrals / pairwise_planar_angles and the
// (B, N*N, n_i+n_j, 3) gather of _pairwise_xyz (reference protstruc.py:589-660);
// geometry.dihedral / geometry.angle (geometry.py:39-124) are evaluated per pair
// in registers, so the 1.6 GB gather of the reference is never materialised.
//
// Which point comes from which side is a template parameter (SRC bit k = 1: point k
// from the column residue j), so nothing is selected at run time and what depends on
// one side only is shared or hoisted.  4 bytes are written per pair against ~90 flops
// and an atan2 / acos: the kernels are bound by the vector unit, not by HBM.
// Two arithmetics (exact_angles bit 0, k3_arith.hpp): the fast one spends the 1e-5
// parity tolerance (triple-product dihedral, polynomial atan2 / acos), the faithful one
// is the reference's order of operations; every kernel below exists in both.
//
// Kernels, in the order of this file (DESIGN.md section 4 has the dispatch table and
// the numbers; ps_k3_plan_f32 names the one a launch takes), then their launchers and
// thresholds, then the entry points.  The fused featuriser, which shares the lane maps
// and k3_launch.hpp, is featuriser.hip:
//   k3_pairwise_angles   one column per lane, rows by scalar loads: the layout-free twin
//                        every other kernel is held to bit for bit, and the fallback
//   k3_small             N <= 32: one wave per structure
//   k3_flat              33..99 residues (and wherever a sweep would idle its lanes): a lane's
//                        element is a 2 x 2 tile (row pairs x columns), several structures staged per pass
//   k3_sweep             >= 100 residues: one workgroup per CU, rows staged in LDS, tasks
//                        pulled from an LDS counter, NC column residues per lane
#include "k3_arith.hpp"
#include "k3_launch.hpp"

namespace {

template <int NP, int SRC, bool FAITHFUL>
__global__ __launch_bounds__(256) void k3_pairwise_angles(const float* __restrict__ xyz, float* __restrict__ out,
                                                          int N, int A, AtomSel sel, int row_begin, int row_end,
                                                          int out_rows, int out_row_origin, int IR, int n_tiles,
                                                          int n_chunks) {
    // 1-D grid (column tile fastest, then row chunk, then structure): no 65 535 limit on any axis
    const unsigned w = blockIdx.x;
    const unsigned tile = w % (unsigned)n_tiles, rest = w / (unsigned)n_tiles;
    const int b = (int)(rest / (unsigned)n_chunks);
    const int j = (int)tile * (int)blockDim.x + threadIdx.x;   // a workgroup is 64, 128, 192 or 256 lanes wide (short chains)
    const int i0 = row_begin + (int)(rest % (unsigned)n_chunks) * IR;
    const int i1 = min(i0 + IR, row_end);
    const bool live = j < N;
    const int jc = live ? j : N - 1;

    const float* sj = xyz + ((size_t)b * N + jc) * (size_t)A * 3;
    f3 pj[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) pj[k] = ((SRC >> k) & 1) ? load3(sj + sel.atom[k] * 3) : mk3(0.f, 0.f, 0.f);

    int i = i0;
    if constexpr (FAITHFUL) {   // the reference's order of operations (dihedral4_ref / angle3_ref), one row per trip
        for (; i < i1; ++i) {
            const float* si = xyz + ((size_t)b * N + i) * (size_t)A * 3;  // wave-uniform
            f3 p[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) p[k] = ((SRC >> k) & 1) ? pj[k] : load3(si + sel.atom[k] * 3);
            float v;
            if constexpr (NP == 4)
                v = dihedral4_ref(p[0], p[1], p[2], p[3]);
            else
                v = angle3_ref(p[0], p[1], p[2]);
            if (live) out[((size_t)b * out_rows + (size_t)(i - out_row_origin)) * N + j] = v;
        }
        return;
    }
    // two rows per trip in the two halves of float2 registers -> packed v_pk_* math (bit-identical per element);
    // dihedrals and planar angles alike
    for (; i + 1 < i1; i += 2) {
        const float* s0 = xyz + ((size_t)b * N + i) * (size_t)A * 3;  // wave-uniform
        const float* s1 = s0 + (size_t)A * 3;
        f3v p[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k)
            p[k] = ((SRC >> k) & 1) ? mk3v(pj[k], pj[k]) : mk3v(load3(s0 + sel.atom[k] * 3), load3(s1 + sel.atom[k] * 3));
        f32x2 v;
        if constexpr (NP == 4)
            v = dihedral4v_k3(p[0], p[1], p[2], p[3]);
        else
            v = angle3v(p[0], p[1], p[2]);
        if (live) {
            float* o = out + ((size_t)b * out_rows + (size_t)(i - out_row_origin)) * N + j;
            o[0] = v.x;
            o[N] = v.y;
        }
    }
    for (; i < i1; ++i) {
        const float* si = xyz + ((size_t)b * N + i) * (size_t)A * 3;  // wave-uniform
        f3 p[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) p[k] = ((SRC >> k) & 1) ? pj[k] : load3(si + sel.atom[k] * 3);
        float v;
        if constexpr (NP == 4)
            v = dihedral4_k3(p[0], p[1], p[2], p[3]);
        else
            v = angle3(p[0], p[1], p[2]);
        if (live) out[((size_t)b * out_rows + (size_t)(i - out_row_origin)) * N + j] = v;
    }
}

// Short chains (N <= 64; peptide batches).  A 64-lane wave of the one-column kernel covers 64 column residues, so a
// 16-residue chain uses a quarter of it.  Here a wave owns one structure and its lanes are (row group, column): Npad = 16, 32
// or 64 columns x G = 64 / Npad rows at a time; the row-side points are per-lane vector loads (the Npad lanes of a row group
// share an address), four rows per trip (two packed pairs, their chains interleaved), and a store instruction writes G
// consecutive rows of the structure.  Same arithmetic per pair as the one-column kernel: same bits.
template <int NP, int SRC, bool FAITHFUL = false>
__global__ __launch_bounds__(256) void k3_small(const float* __restrict__ xyz, float* __restrict__ out, int B, int N, int A,
                                                AtomSel sel, int row_begin, int row_end, int out_rows, int out_row_origin,
                                                int lg_npad) {
    const int lane = threadIdx.x & 63;
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);   // one wave per structure
    if (b >= B) return;
    const int npad = 1 << lg_npad, G = 64 >> lg_npad;
    const int j = lane & (npad - 1), ri = lane >> lg_npad;
    const bool live_j = j < N;
    const float* xb = xyz + (size_t)b * N * (size_t)A * 3;
    const float* sj = xb + (size_t)min(j, N - 1) * (size_t)A * 3;
    f3 pj[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) pj[k] = ((SRC >> k) & 1) ? load3(sj + sel.atom[k] * 3) : mk3(0.f, 0.f, 0.f);
    float* ob = out + (size_t)b * out_rows * N;
    for (int i0 = row_begin + ri; i0 < row_end; i0 += 4 * G) {     // rows i0, i0 + G, i0 + 2G, i0 + 3G of this lane
        f3v P[NP][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* sa = xb + (size_t)min(i0 + 2 * h * G, N - 1) * (size_t)A * 3;
            const float* sb2 = xb + (size_t)min(i0 + (2 * h + 1) * G, N - 1) * (size_t)A * 3;
#pragma unroll
            for (int k = 0; k < NP; ++k)
                P[k][h] = ((SRC >> k) & 1) ? mk3v(pj[k], pj[k]) : mk3v(load3(sa + sel.atom[k] * 3), load3(sb2 + sel.atom[k] * 3));
        }
        f32x2 v[2];
        if constexpr (NP == 4 && FAITHFUL)
            dihedral4v_ref_n<2>(P[0], P[1], P[2], P[3], v);
        else if constexpr (NP == 4)
            dihedral4v_k3_n<2>(P[0], P[1], P[2], P[3], v);
        else if constexpr (FAITHFUL)
            angle3v_ref_n<2>(P[0], P[1], P[2], v);
        else
            angle3v_n<2>(P[0], P[1], P[2], v);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ia = i0 + 2 * h * G, ib = ia + G;
            if (live_j && ia < row_end) ob[(size_t)(ia - out_row_origin) * N + j] = v[h].x;
            if (live_j && ib < row_end) ob[(size_t)(ib - out_row_origin) * N + j] = v[h].y;
        }
    }
}

// Chains of 33 .. ~100 residues, and longer ones wherever a sweep would idle its lanes (round 5): several structures per
// staging pass, every lane busy whatever N is.
// The per-CU sweep gives a wave a strip of 64 * NC columns of ONE structure: below ~100 residues most lanes of a strip have no
// column, a (structure, strip) segment has fewer tasks than the workgroup has waves, and every segment costs two barriers and
// a round trip to L2 (N = 64: 143 us at 2^25 pairs, which is why such chains stayed with the one-column kernel: 85 us).  Here
//   * the selected atoms of KS structures are staged at once (column-side atoms as {x, y, z, -} per (atom, residue), row-side
//     atoms pair-interleaved as {x0, x1, y0, y1}, {z0, z1, -, -} per (row pair, atom): every read in the loop is 16 bytes),
//     so the two barriers and the load latency of a pass are paid once per KS * N * N pairs instead of once per 4 096;
//   * TWO 512-thread workgroups share a CU and a workgroup's share takes four or more passes: while one workgroup waits for
//     its next structures the other computes;
//   * both sides of a pair come from LDS per lane (lanes of one row pair read the same address: a broadcast);
//   * tasks are pulled from an LDS counter, as in the sweep; stores are unconditional (a dead element's offset lies beyond the
//     buffer descriptor's range and the hardware drops it), so the four chains stay in one basic block and interleave.
// Lane map: a lane's element is a 2 x 2 TILE -- two row pairs x two adjacent columns, four chains -- so that what depends on
// the row pair alone is shared by the tile's two columns and what depends on the column alone by its two row pairs (as in the
// sweep), the index arithmetic is paid once per tile and two columns are one 8-byte store: ~300 VALU instructions per 8 pairs,
// 57-64 us per 2^25 pairs from 64 to 220 residues.  Measured and removed (profiles/r05_k3_flat_lane_maps.log, NOTES.md): four
// elements 64 apart in the flat index (408 instructions per 8 pairs, 68-77 us), a lane per column with four consecutive row
// pairs (N <= 64: 324 instructions, 69 us at N = 64), a plain coalesced copy of the coordinates instead of the gather of the
// selected atoms (88 us: it reads all 15 atoms), one 1024-thread workgroup staging its whole share at once (74 us).
// Same arithmetic per pair as the one-column kernel: same bits.
template <int NP, int SRC, bool FAITHFUL>
__global__ __launch_bounds__(1024) void k3_flat(const float* __restrict__ xyz, float* __restrict__ out, int N, int A,
                                                AtomSel sel, int row_begin, int row_end, int out_rows,
                                                int out_row_origin, int KS, unsigned tps, unsigned n_tasks,
                                                unsigned tasks_per_wg, unsigned rcpN, int col_vec4, int slot_vec4,
                                                unsigned rcpTC, int vec) {
    constexpr int NPI = NP - __builtin_popcount(SRC & ((1 << NP) - 1)), NPJ = NP - NPI;
    constexpr int NPIq = NPI > 0 ? NPI : 1, NPJq = NPJ > 0 ? NPJ : 1;
    // [structure slot][column part: (atom, residue) -> {x, y, z, -} | row part: (row pair, atom) -> {x0, x1, y0, y1}, {z0, z1, -, -}]
    extern __shared__ __attribute__((aligned(16))) k3_f32x4 k3_flatbuf[];
    __shared__ unsigned next_task;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned n_waves = blockDim.x >> 6;
    const unsigned t0 = blockIdx.x * tasks_per_wg, t1 = min(t0 + tasks_per_wg, n_tasks);
    if (t0 >= t1) return;                         // whole workgroup
    int amap_i[NPIq], amap_j[NPJq];
    {
        int qi = 0, qj = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if ((SRC >> k) & 1) amap_j[qj++] = sel.atom[k];
            else amap_i[qi++] = sel.atom[k];
        }
        if (NPI == 0) amap_i[0] = 0;
        if (NPJ == 0) amap_j[0] = 0;
    }
    const int rows = row_end - row_begin, n_rp = (rows + 1) >> 1;
    const unsigned b_first = t0 / tps, b_last = (t1 - 1u) / tps;
    for (unsigned bs = b_first; bs <= b_last; bs += (unsigned)KS) {
        const unsigned ks = min((unsigned)KS, b_last - bs + 1u);
        __syncthreads();                                          // the previous pass's readers are done
        for (unsigned it = threadIdx.x; it < ks * (unsigned)N; it += blockDim.x) {   // one residue of one structure per thread
            unsigned s = __umulhi(it, rcpN), r = it - s * (unsigned)N;
            if (r >= (unsigned)N) ++s, r -= (unsigned)N;
            const float* pr = xyz + ((size_t)(bs + s) * N + r) * (size_t)A * 3;
            k3_f32x4* slot = k3_flatbuf + (size_t)s * slot_vec4;
            float vj[NPJq * 3], vi[NPIq * 3];
#pragma unroll
            for (int q = 0; q < NPJ; ++q) { vj[q * 3] = pr[amap_j[q] * 3]; vj[q * 3 + 1] = pr[amap_j[q] * 3 + 1]; vj[q * 3 + 2] = pr[amap_j[q] * 3 + 2]; }
            const int rr = (int)r - row_begin;
            const bool in_rows = NPI > 0 && rr >= 0 && rr < rows;
            if (in_rows) {
#pragma unroll
                for (int q = 0; q < NPI; ++q) { vi[q * 3] = pr[amap_i[q] * 3]; vi[q * 3 + 1] = pr[amap_i[q] * 3 + 1]; vi[q * 3 + 2] = pr[amap_i[q] * 3 + 2]; }
            }
#pragma unroll
            for (int q = 0; q < NPJ; ++q) slot[q * N + (int)r] = k3_f32x4{vj[q * 3], vj[q * 3 + 1], vj[q * 3 + 2], 0.0f};
            if (in_rows) {
                float* rb = reinterpret_cast<float*>(slot + col_vec4) + (size_t)(rr >> 1) * (NPI * 8) + (rr & 1);
#pragma unroll
                for (int q = 0; q < NPI; ++q) { rb[q * 8] = vi[q * 3]; rb[q * 8 + 2] = vi[q * 3 + 1]; rb[q * 8 + 4] = vi[q * 3 + 2]; }
            }
        }
        const unsigned seg_t0 = max(t0, bs * tps), seg_t1 = min(t1, (bs + ks) * tps);
        if (threadIdx.x == 0) next_task = seg_t0 + n_waves;       // the first n_waves tasks are pre-assigned
        __syncthreads();
        unsigned t = seg_t0 + (unsigned)wave;
        while (t < seg_t1) {
            const unsigned b = t / tps, chunk = t - b * tps;      // (uniform)
            const k3_f32x4* slot = k3_flatbuf + (size_t)(b - bs) * slot_vec4;
            const k3_f32x4* rowp = slot + col_vec4;
            float* obase = out + ((size_t)b * out_rows + (size_t)(row_begin - out_row_origin)) * N;
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(obase, 0, (int)(rows * N * 4), 0x00020000u);   // this structure's rows, exactly
            // the lane's tile: two row pairs x two adjacent columns (four chains) -- or, where a row of FOUR columns is one aligned
            // 16-byte store (vec == 4: N % 4 == 0), two such halves that share the index arithmetic and the row-side points
            // (N = 64 .. 220: 58-65 / 60-66 / 43-50 us per 2^25 pairs against 62-73 / 68-79 / 48-59; without the wide store the
            // four-column tile loses: N = 99 76 against 70 us, N = 33 148 against 129; profiles/r05_k3_flat_tile_width.log)
            const bool wide = vec == 4;                      // (uniform)
            const unsigned TC = wide ? (unsigned)N >> 2 : (unsigned)(N + 1) >> 1, TR = (unsigned)(n_rp + 1) >> 1, FT = TR * TC;
            const unsigned ti = chunk * 64u + (unsigned)lane;
            const bool lt = ti < FT;
            const unsigned tcl = min(ti, FT - 1u);
            unsigned tr = __umulhi(tcl, rcpTC), tc = tcl - tr * TC;
            if (tc >= TC) ++tr, tc -= TC;
            const int c0 = (int)(wide ? 4u * tc : 2u * tc);
            const int rpA = (int)(2u * tr), rpB = min(rpA + 1, n_rp - 1);
            const bool lc1 = c0 + 1 < N, lrB = rpA + 1 < n_rp;
            f3v RA[NPIq], RB[NPIq];                   // the row-side points of the two row pairs ({row 2 rp, row 2 rp + 1} per component)
#pragma unroll
            for (int qi = 0; qi < NPI; ++qi) {
                const k3_f32x4 xa = rowp[(rpA * NPI + qi) * 2], xb = rowp[(rpB * NPI + qi) * 2];
                const f32x2 za = *reinterpret_cast<const f32x2*>(rowp + (rpA * NPI + qi) * 2 + 1);
                const f32x2 zb = *reinterpret_cast<const f32x2*>(rowp + (rpB * NPI + qi) * 2 + 1);
                RA[qi] = f3v{f32x2{xa.x, xa.y}, f32x2{xa.z, xa.w}, za};
                RB[qi] = f3v{f32x2{xb.x, xb.y}, f32x2{xb.z, xb.w}, zb};
            }
            // columns ca, ca + 1 (clamped: a dead column is never stored) against the two row pairs:
            // v[0], v[1] = row pair A x the two columns; v[2], v[3] = row pair B; .x / .y = the pair's rows
            auto half = [&](int ca, f32x2 (&v)[4]) {
                const int cb = min(ca + 1, N - 1);
                f3v P[NP][4];
                int qi = 0, qj = 0;
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    if ((SRC >> k) & 1) {
                        const k3_f32x4 p0 = slot[qj * N + ca], p1 = slot[qj * N + cb];
                        P[k][0] = P[k][2] = mk3v(f3{p0.x, p0.y, p0.z}, f3{p0.x, p0.y, p0.z});
                        P[k][1] = P[k][3] = mk3v(f3{p1.x, p1.y, p1.z}, f3{p1.x, p1.y, p1.z});
                        ++qj;
                    } else {
                        P[k][0] = P[k][1] = RA[qi];
                        P[k][2] = P[k][3] = RB[qi];
                        ++qi;
                    }
                }
                if constexpr (NP == 4 && FAITHFUL)
                    dihedral4v_ref_n<4>(P[0], P[1], P[2], P[3], v);
                else if constexpr (NP == 4)
                    dihedral4v_k3_n<4>(P[0], P[1], P[2], P[3], v);
                else if constexpr (FAITHFUL)
                    angle3v_ref_n<4>(P[0], P[1], P[2], v);
                else
                    angle3v_n<4>(P[0], P[1], P[2], v);
#pragma unroll
                for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(v[c]));
            };
            f32x2 v[4];
            half(c0, v);
            const int offA = (int)__umul24((unsigned)(2 * rpA), (unsigned)N) * 4 + c0 * 4;
            const int offB = (int)__umul24((unsigned)(2 * rpB), (unsigned)N) * 4 + c0 * 4;
            const bool rA1 = 2 * rpA + 1 < rows, rB0 = lrB, rB1 = lrB && 2 * rpB + 1 < rows;   // rows 2 rpA + 1, 2 rpB, 2 rpB + 1 exist
            constexpr int DEAD = 0x7FFFFFF0;    // beyond num_records: dropped by the range check
            if (wide) {              // N % 4 == 0 and the rows 16-byte aligned: a row of the tile is one store
                f32x2 w[4];
                half(c0 + 2, w);     // (c0 + 3 < N)
                auto st4 = [&](float a, float b, float c, float d, int off) {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k3_u32x4, k3_f32x4{a, b, c, d}), rsrc, off, 0, 0);
                };
                st4(v[0].x, v[1].x, w[0].x, w[1].x, lt ? offA : DEAD);
                st4(v[0].y, v[1].y, w[0].y, w[1].y, (lt && rA1) ? offA + N * 4 : DEAD);
                st4(v[2].x, v[3].x, w[2].x, w[3].x, (lt && rB0) ? offB : DEAD);
                st4(v[2].y, v[3].y, w[2].y, w[3].y, (lt && rB1) ? offB + N * 4 : DEAD);
            } else if (vec == 2) {   // (uniform) N even and the rows 8-byte aligned: the tile's two columns are one store
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].x, v[1].x}), rsrc, lt ? offA : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].y, v[1].y}), rsrc, (lt && rA1) ? offA + N * 4 : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[2].x, v[3].x}), rsrc, (lt && rB0) ? offB : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[2].y, v[3].y}), rsrc, (lt && rB1) ? offB + N * 4 : DEAD, 0, 0);
            } else {
                const bool l1 = lt && lc1;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[0].x), rsrc, lt ? offA : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[1].x), rsrc, l1 ? offA + 4 : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[0].y), rsrc, (lt && rA1) ? offA + N * 4 : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[1].y), rsrc, (l1 && rA1) ? offA + N * 4 + 4 : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[2].x), rsrc, (lt && rB0) ? offB : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[3].x), rsrc, (l1 && rB0) ? offB + 4 : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[2].y), rsrc, (lt && rB1) ? offB + N * 4 : DEAD, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[3].y), rsrc, (l1 && rB1) ? offB + N * 4 + 4 : DEAD, 0, 0);
            }
            unsigned nx = 0;
            if (lane == 0) nx = atomicAdd(&next_task, 1u);
            t = (unsigned)__builtin_amdgcn_readfirstlane((int)nx);
        }
    }
}

// The sweep for even N (round 4): ONE 1024-thread workgroup per CU, NC = 2 or 4 consecutive column residues per lane
// (8- or 16-byte stores), two rows per trip in the halves of float2 registers.
//   * Work list: task t = (b * n_strips + strip) * n_chunks + chunk = CH rows x one strip of 64 * NC columns of one
//     structure.  A workgroup owns a contiguous range of it (1 / #CUs of the list); its LDS request keeps a second
//     workgroup off the CU, so every CU gets the same share whatever the dispatcher does.
//   * The row-side points of a (b, strip) segment are staged ONCE in LDS, pair-interleaved: one broadcast ds_read_b64 /
//     b128 delivers {row 2r, row 2r + 1} of a component already in the packed layout -- no scalar loads, no s_waitcnt on
//     SMEM and no SGPR -> VGPR moves inside the loop (the kernels before staged nothing: rows came by s_load per trip).
//   * The 16 waves PULL tasks from an LDS counter.  The SIMD arbiter serves its oldest wave first: with equal static
//     shares the four waves of a SIMD finish one after the other (18 / 28 / 38 / 47 us at config 3) and the last one runs
//     alone at half the issue rate; pulling lets the favoured waves take more tasks and all of them end together.
//   * Stores are write-through (sc1): the 134 MB of config 3 would otherwise leave up to 32 MB dirty in the L2s for the
//     end-of-kernel write-back, which is serial with everything (3-4 us of 57).
//   * The arithmetic of the NC columns is evaluated step by step across the columns (dihedral4v_k3_n, angle3v_n).
// Same operations per pair as the one-column kernel above: same bits.
// VEC = false (odd N, or an output that is not 4 * NC-byte aligned): the lane's NC columns are 64 apart instead of adjacent
// (column = strip * 64 * NC + 64 * c + lane), so every store instruction writes 64 consecutive floats of one row -- no
// alignment is needed at all -- at the price of NC dword stores per row instead of one vector store.
// One task's row pairs for L of the lane's NC columns (see the kernel; pinned results and interleaved chains as described there).
#define K3_SWEEP_ROWS(L)                                                                                                  \
    {                                                                                                                     \
            int i = i0;                                                                                                  \
            for (; i + 1 < i1; i += 2) {                                                                                 \
                f3v cur[NP];                                                                                             \
                rows(i >> 1, cur);                                                                                       \
                f3v P[NP][L];                                                                                            \
_Pragma("unroll")                                                                                                        \
                for (int k = 0; k < NP; ++k)                                                                             \
_Pragma("unroll")                                                                                                        \
                    for (int cc = 0; cc < L; ++cc) P[k][cc] = ((SRC >> k) & 1) ? mk3v(pj[cc][k], pj[cc][k]) : cur[k];    \
                f32x2 v[L];                                                                                              \
                if constexpr (NP == 4 && FAITHFUL)                                                                       \
                    dihedral4v_ref_n<L>(P[0], P[1], P[2], P[3], v);                                                      \
                else if constexpr (NP == 4)                                                                              \
                    dihedral4v_k3_n<L>(P[0], P[1], P[2], P[3], v);                                                       \
                else if constexpr (FAITHFUL)                                                                             \
                    angle3v_ref_n<L>(P[0], P[1], P[2], v);                                                               \
                else                                                                                                     \
                    angle3v_n<L>(P[0], P[1], P[2], v);                                                                   \
_Pragma("unroll")                                                                                                        \
                for (int cc = 0; cc < L; ++cc) asm volatile("" : "+v"(v[cc]));                                           \
                if constexpr (!VEC) {                                                                                    \
                    const int so = i * row_bytes;                                                                        \
_Pragma("unroll")                                                                                                        \
                    for (int cc = 0; cc < L; ++cc)                                                                       \
                        if (j0 + 64 * cc < N) {                                                                          \
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[cc].x), rsrc, lane_off + 256 * cc, so, POL); \
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[cc].y), rsrc, lane_off + 256 * cc, so + row_bytes, POL); \
                        }                                                                                                \
                } else if (live) {                                                                                       \
                    const int so = i * row_bytes;                                                                        \
                    if constexpr (NC == 4) {                                                                             \
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k3_u32x4, k3_f32x4{v[0].x, v[1].x, v[2].x, v[3].x}), rsrc, lane_off, so, POL); \
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k3_u32x4, k3_f32x4{v[0].y, v[1].y, v[2].y, v[3].y}), rsrc, lane_off, so + row_bytes, POL); \
                    } else {                                                                                             \
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].x, v[1].x}), rsrc, lane_off, so, POL); \
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0].y, v[1].y}), rsrc, lane_off, so + row_bytes, POL); \
                    }                                                                                                    \
                }                                                                                                        \
            }                                                                                                            \
            if (i < i1) {                                                                                                \
                f3v cur[NP];                                                                                             \
                rows(i >> 1, cur);                                                                                       \
                float v[NC];                                                                                             \
_Pragma("unroll")                                                                                                        \
                for (int cc = 0; cc < L; ++cc) {                                                                         \
                    f3 p[NP];                                                                                            \
_Pragma("unroll")                                                                                                        \
                    for (int k = 0; k < NP; ++k) p[k] = ((SRC >> k) & 1) ? pj[cc][k] : mk3(cur[k].x.x, cur[k].y.x, cur[k].z.x); \
                    if constexpr (NP == 4)                                                                               \
                        v[cc] = FAITHFUL ? dihedral4_ref(p[0], p[1], p[2], p[3]) : dihedral4_k3(p[0], p[1], p[2], p[3]); \
                    else                                                                                                 \
                        v[cc] = FAITHFUL ? angle3_ref(p[0], p[1], p[2]) : angle3(p[0], p[1], p[2]);                      \
                }                                                                                                        \
                if constexpr (!VEC) {                                                                                    \
                    const int so = i * row_bytes;                                                                        \
_Pragma("unroll")                                                                                                        \
                    for (int cc = 0; cc < L; ++cc)                                                                       \
                        if (j0 + 64 * cc < N) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[cc]), rsrc, lane_off + 256 * cc, so, POL); \
                } else if (live) {                                                                                       \
                    const int so = i * row_bytes;                                                                        \
                    if constexpr (NC == 4)                                                                               \
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(k3_u32x4, k3_f32x4{v[0], v[1], v[2], v[3]}), rsrc, lane_off, so, POL); \
                    else                                                                                                 \
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(k3_u32x2, f32x2{v[0], v[1]}), rsrc, lane_off, so, POL); \
                }                                                                                                        \
            }                                                                                                            \
    }

template <int NP, int SRC, int NC, bool VEC, bool FAITHFUL = false>
__global__ __launch_bounds__(k3_sweep_threads(NC, FAITHFUL)) void k3_sweep(const float* __restrict__ xyz, float* __restrict__ out, int N, int A,
                                                 AtomSel sel, int row_begin, int row_end, int out_rows,
                                                 int out_row_origin, int CH, int n_strips, int n_chunks,
                                                 unsigned n_tasks, unsigned tasks_per_wg) {
    static_assert(NC == 2 || NC == 4, "columns per lane");
    constexpr int NPI = NP - __builtin_popcount(SRC & ((1 << NP) - 1));   // points taken from the row residue
    constexpr int NPIq = NPI > 0 ? NPI : 1;
    constexpr int POL = 16;                       // sc1: write-through
    extern __shared__ __attribute__((aligned(16))) f32x2 k3_rowbuf[];   // [row pair][row point][xyz] of the current segment
    __shared__ unsigned next_task;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x >> 6);
    const unsigned t0 = blockIdx.x * tasks_per_wg, t1 = min(t0 + tasks_per_wg, n_tasks);
    if (t0 >= t1) return;                         // whole workgroup
    int amap[NPIq];
    {
        int q = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (!((SRC >> k) & 1)) amap[q++] = sel.atom[k];
        if (NPI == 0) amap[0] = 0;
    }
    const int row_bytes = N * 4;
    int staged_b = -1, staged_lo = -1, staged_hi = -1;
    for (unsigned g = t0 / (unsigned)n_chunks; g <= (t1 - 1u) / (unsigned)n_chunks; ++g) {   // g = b * n_strips + strip
        const int c_lo = (int)(max(t0, g * (unsigned)n_chunks) - g * (unsigned)n_chunks);
        const int c_hi = (int)(min(t1, (g + 1u) * (unsigned)n_chunks) - g * (unsigned)n_chunks);
        const int b = (int)(g / (unsigned)n_strips), strip = (int)(g % (unsigned)n_strips);
        const int r_lo = row_begin + c_lo * CH, r_hi = min(row_begin + c_hi * CH, row_end);
        const float* xb = xyz + (size_t)b * N * (size_t)A * 3;   // uniform
        __syncthreads();                                          // the previous segment's readers are done
        // the column-side points are requested BEFORE the rows are staged: the two global-memory latencies of a segment's
        // set-up overlap instead of following each other (a 128-residue segment computes for ~6 us; its set-up was ~2)
        // VEC: NC adjacent columns (j0 .. j0 + NC - 1), N % NC == 0 so that they are all in or all out; otherwise NC columns 64 apart
        const int j0 = VEC ? (strip * 64 + lane) * NC : strip * 64 * NC + lane;
        constexpr int CSTEP = VEC ? 1 : 64;
        const bool live = j0 < N;                                 // the lane's FIRST column (VEC: all of them)
        f3 pj[NC][NP];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float* sj = xb + (size_t)min(j0 + c * CSTEP, N - 1) * (size_t)A * 3;   // clamped: dead columns are never stored
#pragma unroll
            for (int k = 0; k < NP; ++k) pj[c][k] = ((SRC >> k) & 1) ? load3(sj + sel.atom[k] * 3) : mk3(0.f, 0.f, 0.f);
        }
        if (NPI > 0 && (b != staged_b || r_lo != staged_lo || r_hi != staged_hi)) {
            // a row per thread, its 3 * NPI loads in flight together (an element per thread walked three dependent round
            // trips to L2 per 512-row segment)
            float* rb = reinterpret_cast<float*>(k3_rowbuf);
            for (int row = (int)threadIdx.x; row < r_hi - r_lo; row += (int)blockDim.x) {
                const float* pr = xb + (size_t)(r_lo + row) * (size_t)A * 3;
                float v[NPIq * 3];
#pragma unroll
                for (int q = 0; q < NPI; ++q) {
                    v[q * 3] = pr[amap[q] * 3]; v[q * 3 + 1] = pr[amap[q] * 3 + 1]; v[q * 3 + 2] = pr[amap[q] * 3 + 2];
                }
#pragma unroll
                for (int qc = 0; qc < NPI * 3; ++qc) rb[(((row >> 1) * (NPI * 3) + qc) << 1) + (row & 1)] = v[qc];
            }
            staged_b = b; staged_lo = r_lo; staged_hi = r_hi;
        }
        if (threadIdx.x == 0) next_task = (unsigned)(c_lo + n_waves);   // the first n_waves tasks are pre-assigned
        __syncthreads();
        // the segment's rows as one buffer: uniform base, the lane's constant byte offset, the row's byte offset as a scalar
        float* obase = out + ((size_t)b * out_rows + (size_t)(r_lo - out_row_origin)) * N;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(obase, 0, 0xFFFFFFFFu, 0x00020000u);
        const int lane_off = j0 * 4;
        auto rows = [&](int r, f3v (&p)[NP]) {                    // r = row pair index inside the segment
            int q = 0;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                if ((SRC >> k) & 1) {
                    p[k] = mk3v(mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f));
                } else {
                    p[k] = f3v{k3_rowbuf[(r * NPI + q) * 3 + 0], k3_rowbuf[(r * NPI + q) * 3 + 1], k3_rowbuf[(r * NPI + q) * 3 + 2]};
                    ++q;
                }
            }
        };
        int c = c_lo + wave;
        while (c < c_hi) {
            const int i0 = (c - c_lo) * CH;                       // rows relative to r_lo (CH is even: pairs stay aligned)
            const int i1 = min(i0 + CH, r_hi - r_lo);
            // the row pairs of the task (K3_SWEEP_ROWS, defined in front of the kernel; a macro rather than a generic lambda: inside
            // a lambda the register allocator spilled 1-30 registers in four instantiations).  !VEC: a strip may have fewer than NC
            // live column groups (64 columns each; the last strip of a row) -- the chains of the dead ones are not evaluated.
            if constexpr (VEC) {
                K3_SWEEP_ROWS(NC)
            } else {
                // (not three of four: that variant spilled 3-5 registers in some instantiations)
                constexpr bool SKIP = true;
                const int ncl = SKIP ? min(NC, (N - strip * 64 * NC + 63) >> 6) : NC;   // live column groups of this strip (uniform)
                if (!SKIP || ncl == NC || ncl == 3) K3_SWEEP_ROWS(NC)
                else if (NC == 4 && ncl == 2) K3_SWEEP_ROWS((NC == 4 ? 2 : 1))
                else K3_SWEEP_ROWS(1)
            }
            unsigned nx = 0;
            if (lane == 0) nx = atomicAdd(&next_task, 1u);
            c = __builtin_amdgcn_readfirstlane((int)nx);
        }
    }
}

#undef K3_SWEEP_ROWS

// ---- launchers and thresholds (every launch goes through k3_go: launch or record, k3_launch.hpp) ----
// The arguments of one K3 call (a plan query leaves the pointers NULL; out_misalign: the low four address bits of `out`)
struct K3Call {
    const float* xyz;
    float* out;
    int B, N, A;
    AtomSel sel;
    int row_begin, row_end, out_rows, out_row_origin;
    unsigned out_misalign;
    int rows() const { return row_end - row_begin; }
};

template <int NP, int SRC, int NC, bool VEC, bool FAITHFUL>
int launch_sweep(const K3Call& c, const K3Go& go) {
    constexpr int NPI = NP - __builtin_popcount(SRC & ((1 << NP) - 1));
    constexpr int THREADS = k3_sweep_threads(NC, FAITHFUL);
    const int N = c.N, rows = c.rows(), cus = go.cus;
    const int n_strips = (N + 64 * NC - 1) / (64 * NC);
    const int CH = k3_rows_per_task(rows, 2);
    const int n_chunks = (rows + CH - 1) / CH;
    const unsigned long long n_tasks = (unsigned long long)n_strips * n_chunks * c.B;
    if (n_tasks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    const size_t need = (size_t)((rows + 2) / 2) * (NPI > 0 ? NPI : 1) * 3 * 8;   // one segment's rows, pair-interleaved
    // Every CU one full-width workgroup -- or, when a workgroup would walk four or more (structure, strip) segments (chains
    // of ~128 residues in large batches), TWO of half the width: a segment's set-up (two barriers, the global-load latency
    // of its rows and column points) idles all of a workgroup's waves for ~1.8 us, and a second workgroup on the CU computes
    // meanwhile.  Their LDS requests admit exactly two per CU.  Short lists: at least 4 tasks per workgroup.
    const unsigned long long segs = (unsigned long long)n_strips * c.B;
    const bool two = segs >= 4ull * cus * 2 && need <= K3_LDS_TWO_PER_CU;
    const unsigned slots = (unsigned)cus * (two ? 2u : 1u);
    const unsigned tasks_per_wg = (unsigned)std::max<unsigned long long>((n_tasks + slots - 1) / slots, 4ull);
    const unsigned grid = (unsigned)((n_tasks + tasks_per_wg - 1) / tasks_per_wg);
    const size_t dyn = two ? K3_LDS_TWO_PER_CU : std::max(need, K3_LDS_ONE_PER_CU);
    static unsigned long long prepared[1] = {0};   // bit d: device d allows this kernel its dynamic LDS
    char name[96];
    snprintf(name, sizeof name, "k3_sweep<NP=%d,SRC=%d,NC=%d,VEC=%d,FAITHFUL=%d>", NP, SRC, NC, (int)VEC, (int)FAITHFUL);
    K3Shape sh;
    sh.nc = NC; sh.vec = VEC; sh.skips = !VEC; sh.faithful = FAITHFUL; sh.rows_per_task = CH;
    sh.wgs_per_cu = two ? 2 : 1; sh.structs_per_segment = 1; sh.n_tasks = (unsigned)n_tasks; sh.tasks_per_wg = tasks_per_wg;
    return k3_go(go, "sweep", name, sh, k3_sweep<NP, SRC, NC, VEC, FAITHFUL>, &prepared, dim3(grid), dim3(THREADS >> (two ? 1 : 0)), dyn, 4u,
                 c.xyz, c.out, N, c.A, c.sel, c.row_begin, c.row_end, c.out_rows, c.out_row_origin, CH, n_strips, n_chunks, (unsigned)n_tasks,
                 tasks_per_wg);
}

template <int NP, int SRC, bool FAITHFUL>
int launch_flat(const K3Call& c, const K3Go& go) {
    constexpr int NPI = NP - __builtin_popcount(SRC & ((1 << NP) - 1)), NPJ = NP - NPI;
    const int N = c.N, rows = c.rows(), rp = (rows + 1) / 2;
    // a row of the tile as one 16-byte store (then the tile is four columns wide), or as one 8-byte store, where the chain length
    // and the rows' alignment allow it
    const unsigned mis = c.out_misalign + (unsigned)(((long long)c.row_begin - c.out_row_origin) * N * 4);
    int vec = (N % 4 == 0 && (mis & 15u) == 0) ? 4 : (N % 2 == 0 && (mis & 7u) == 0) ? 2 : 0;
    const unsigned TR = (unsigned)(rp + 1) / 2;
    if (vec == 4 && !k3_wide_tiles_pay(TR, N)) vec = 2;
    const unsigned TC = vec == 4 ? (unsigned)N / 4 : (unsigned)(N + 1) / 2;       // tiles of two row pairs x four / two columns
    const unsigned tps = (TR * TC + 63u) / 64u;                                   // tasks (64 tiles) per structure
    const unsigned long long n_tasks = (unsigned long long)tps * c.B;
    if (n_tasks > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    const int col_vec4 = NPJ * N, slot_vec4 = col_vec4 + rp * NPI * 2;   // 16-byte units: {x, y, z, -} per column atom; two per row-pair atom
    // two 512-thread workgroups per CU (their LDS requests admit exactly two): one computes while the other stages
    const unsigned slots = (unsigned)go.cus * 2u;
    const unsigned tasks_per_wg = (unsigned)std::max<unsigned long long>((n_tasks + slots - 1) / slots, 4ull);
    const unsigned grid = (unsigned)((n_tasks + tasks_per_wg - 1) / tasks_per_wg);
    // structures per staging pass: a quarter of a workgroup's share (so that the two workgroups of a CU interleave their
    // passes), at most what the LDS holds
    const unsigned share = (tasks_per_wg + tps - 1) / tps + 1;
    const size_t by_share = std::max<size_t>(1, (share + 3) / 4);
    const int KS = (int)std::max<size_t>(1, std::min<size_t>(K3_LDS_TWO_PER_CU / ((size_t)slot_vec4 * 16), by_share));
    static unsigned long long prepared[1] = {0};
    char name[96];
    snprintf(name, sizeof name, "k3_flat<NP=%d,SRC=%d,FAITHFUL=%d>", NP, SRC, (int)FAITHFUL);
    K3Shape sh;
    sh.nc = 4; sh.skips = 1; sh.faithful = FAITHFUL; sh.rows_per_task = 0; sh.wgs_per_cu = 2; sh.structs_per_segment = KS;
    sh.vec = vec / 2;                       // ps_k3_plan.vector_stores: 0 dword, 1 8-byte, 2 16-byte stores
    sh.n_tasks = (unsigned)n_tasks; sh.tasks_per_wg = tasks_per_wg;
    return k3_go(go, "flat_tiles", name, sh, k3_flat<NP, SRC, FAITHFUL>, &prepared, dim3(grid), dim3(512), K3_LDS_TWO_PER_CU, 4u, c.xyz, c.out, N,
                 c.A, c.sel, c.row_begin, c.row_end, c.out_rows, c.out_row_origin, KS, tps, (unsigned)n_tasks, tasks_per_wg,
                 (unsigned)((1ull << 32) / (unsigned)N), col_vec4, slot_vec4, (unsigned)((1ull << 32) / std::max(1u, TC)), vec);
}

// whether one structure's selected atoms fit the flat kernel's LDS (two workgroups per CU)
inline bool k3_flat_fits(int N) { return (size_t)N * 4 * 16 + (size_t)((N + 1) / 2) * 4 * 32 <= K3_LDS_TWO_PER_CU; }

// The per-CU sweep kernels pay two workgroup barriers and a staging pass per (structure, strip) segment and give a wave a
// strip of 64 * NC columns: below ~100 residues a segment has fewer tasks than the workgroup has waves and most lanes of a
// strip idle (N = 64: 143 us against 93 for the one-column kernel at 2^25 pairs; N = 16: 1427 against 282;
// profiles/r04_k3_shapes.log) -- shorter chains take k3_flat (round 5; the one-column kernel before).
constexpr int K3_SWEEP_MIN_N = 100;
constexpr int K3_FLAT_MAX_N = 256;        // ... up to this length (above it the fast sweeps are level with the tiles: 57-64 / 59-66 / 38-42 us)
constexpr int K3_FLAT_MAX_N_WIDE = 448;   // ... this one where the tiles are four columns wide (N % 4 == 0, 16-byte rows): 56-59 / 54-61 / 38-44 us from 288 to 448
                                          // residues against the sweeps' 56-72 / 59-69 / 39-49 (level at 256 and 384; from 480 on the sweeps win)
constexpr int K3_FLAT_MAX_N_FAITHFUL = 480;   // (faithful: N = 300 94 / 84 / 60 us against 117 / 97 / 66; from 500 on the sweeps win)
constexpr int K3_FLAT_UTIL_PERCENT = 95; // ... and instead of a sweep of which fewer than this share of the lanes would have a column
constexpr int K3_FLAT_UTIL_PERCENT_FAITHFUL = 95;   // (the faithful sweeps, two waves per SIMD, lose even more to idle lanes: N = 160 149 us against 98)
constexpr int K3_SMALL_MAX_N = 32;    // k3_small: one wave per structure (33..64 measured: no better than the one-column kernel)

template <int NP, int SRC, bool FAITHFUL>
int launch_one_column(const K3Call& c, const K3Go& go) {
    const int N = c.N, thr1 = k3_one_column_threads(N), IR = 16;
    const int n_tiles = (N + thr1 - 1) / thr1, n_chunks = (c.rows() + IR - 1) / IR;
    const unsigned long long n_wg = (unsigned long long)n_tiles * n_chunks * c.B;
    if (n_wg > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    char name[96];
    snprintf(name, sizeof name, "k3_pairwise_angles<NP=%d,SRC=%d,FAITHFUL=%d>", NP, SRC, (int)FAITHFUL);
    K3Shape sh;
    sh.faithful = FAITHFUL; sh.rows_per_task = IR;
    return k3_go(go, "one_column", name, sh, k3_pairwise_angles<NP, SRC, FAITHFUL>, nullptr, dim3((unsigned)n_wg), dim3(thr1), 0, 0u, c.xyz,
                 c.out, N, c.A, c.sel, c.row_begin, c.row_end, c.out_rows, c.out_row_origin, IR, n_tiles, n_chunks);
}

template <int NP, int SRC, bool FAITHFUL>
int launch_small(const K3Call& c, const K3Go& go) {   // short chains: lanes = (row group, column), one wave per structure
    const int N = c.N;
    const unsigned long long n_wg = ((unsigned long long)c.B + 3) / 4;
    if (n_wg > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    char name[96];
    snprintf(name, sizeof name, "k3_small<NP=%d,SRC=%d,FAITHFUL=%d>", NP, SRC, (int)FAITHFUL);
    K3Shape sh;
    sh.faithful = FAITHFUL; sh.rows_per_task = 4 * (64 >> (N <= 16 ? 4 : 5)); sh.nc = N <= 16 ? 16 : 32;
    return k3_go(go, "small", name, sh, k3_small<NP, SRC, FAITHFUL>, nullptr, dim3((unsigned)n_wg), dim3(256), 0, 0u, c.xyz, c.out, c.B, N, c.A,
                 c.sel, c.row_begin, c.row_end, c.out_rows, c.out_row_origin, N <= 16 ? 4 : N <= 32 ? 5 : 6);
}

// The sweep layout a launch would take: vector stores or columns 64 apart, columns per lane, and the 64-column groups it
// evaluates per row pair.  NC columns per lane in the vector layout need N % NC == 0 and 4 * NC-byte aligned rows (`fits`: the
// sweep can run at all; `can4`: the instantiation keeps its registers at four columns, see launch).
struct K3SweepLayout {
    int nc;
    bool vec;
    long long groups;
};
inline K3SweepLayout k3_sweep_layout(int N, unsigned out_misalign, bool fits, bool can4) {
    const bool ok4 = can4 && fits && N % 4 == 0 && (out_misalign & 15u) == 0, ok2 = fits && N % 2 == 0 && (out_misalign & 7u) == 0;
    // lanes past the last column idle: take the width that wastes fewer of them (a tie goes to the wider stores)
    const long long w4 = (long long)((N + 255) / 256) * 256, w2 = (long long)((N + 127) / 128) * 128;
    const bool vec4 = ok4 && (!ok2 || w4 <= w2);
    // The 64-apart layout skips the dead column groups of a row's last strip (every instantiation does since the fast (2,2)
    // dihedral takes two columns per lane: round 5): it computes ceil(N / 64) groups per row pair where the vector layouts
    // compute whole strips -- taken also for even N where that saves more than its dword stores cost; four columns per lane
    // from three groups on
    const long long gn = (N + 63) / 64, gv = (vec4 ? w4 : w2) / 64;
    if ((ok4 || ok2) && !(gn * 115 < gv * 100)) return K3SweepLayout{vec4 ? 4 : 2, true, gv};
    return K3SweepLayout{(can4 && gn > 2) ? 4 : 2, false, gn};
}

// mode = exact_angles of the C ABI: bit 0 = the reference's order of operations (FAITHFUL), bit 1 = the one-column kernel
// whatever the shape (diagnostic: the layout-free twin the sweep kernels are held to, bit for bit, in either arithmetic)
template <int NP, int SRC, bool FAITHFUL>
int launch(const K3Call& c, bool simple, const K3Go& go) {
    constexpr int NPI = NP - __builtin_popcount(SRC & ((1 << NP) - 1));
    const int N = c.N, rows = c.rows();
    if (simple) return launch_one_column<NP, SRC, FAITHFUL>(c, go);
    if (N <= K3_SMALL_MAX_N) return launch_small<NP, SRC, FAITHFUL>(c, go);
    // the segment's rows have to fit the LDS, and its output has to be addressable by the kernel's 32-bit byte offsets (a
    // row-sharded call on a very long chain)
    const bool fits = N >= K3_SWEEP_MIN_N && (size_t)((rows + 2) / 2) * (NPI > 0 ? NPI : 1) * 3 * 8 <= K3_LDS_MAX &&
                      (unsigned long long)rows * (unsigned long long)N * 4ull < (1ull << 31);
    // four columns per lane only where the instantiation keeps its registers (three or two column-side points of a
    // dihedral times four columns do not fit the 128 VGPRs of a 1024-thread workgroup: 4-95 spilled registers -- the (2,2)
    // split fitted with 124 until round 5's three-instruction dot products pushed it to 128 + 9 spilled; at two columns it
    // runs as fast (same-box A/B 54.8 / 52.5 against 54.0 / 52.0 us, profiles/r05_k3_modes_first.log) and skips dead groups;
    // the faithful kernels' 512-thread workgroups have 256 and take four columns for every split: at most 247 of the 256
    // VGPRs, nothing spilled: tools/kernel_resources.sh; same-box A/B at config 3 against two columns at 1024 threads:
    // 80 / 66 / 43 us against 83 / 74 / 48, profiles/r05_k3_modes_first.log)
    constexpr bool NC4 = FAITHFUL || (NP == 3 || SRC == 0 || SRC == 1 || SRC == 2 || SRC == 4 || SRC == 8 || SRC == 15);
    const K3SweepLayout lay = k3_sweep_layout(N, c.out_misalign, fits, NC4);
    // The flat kernel in its 2 x 2 tile map (every lane has an element whatever N is; 59-66 / 66-77 / 45-55 us per 2^25 pairs from
    // 48 to 140 residues, profiles/r05_k3_shapes.log): every chain shorter than the sweeps' minimum, and up to 256 residues wherever
    // fewer than K3_FLAT_UTIL_PERCENT of the sweep's lanes would have a column (N = 140: three groups of 64 for 140 columns,
    // 59 against 102 us; N = 180: 59 / 66 / 46 against 61 / 74 / 50).
    constexpr int flat_util = FAITHFUL ? K3_FLAT_UTIL_PERCENT_FAITHFUL : K3_FLAT_UTIL_PERCENT;
    const bool wide_tiles = N % 4 == 0 && (c.out_misalign & 15u) == 0;
    const int flat_max = FAITHFUL ? K3_FLAT_MAX_N_FAITHFUL : wide_tiles ? K3_FLAT_MAX_N_WIDE : K3_FLAT_MAX_N;
    if (k3_flat_fits(N) &&
        (!fits || (N <= flat_max && ((long long)N * 100 < (long long)flat_util * 64 * lay.groups ||
                                     // ... or where the sweep would write dwords (its columns 64 apart) and the tiles whole 16-byte rows: N = 192
                                     (!lay.vec && wide_tiles)))))
        return launch_flat<NP, SRC, FAITHFUL>(c, go);
    if (!fits) return launch_one_column<NP, SRC, FAITHFUL>(c, go);
    // vector stores, or (odd N, a misaligned output, or fewer groups) the lane's columns 64 apart and dword stores
    if constexpr (NC4) {
        if (lay.nc == 4) return lay.vec ? launch_sweep<NP, SRC, 4, true, FAITHFUL>(c, go) : launch_sweep<NP, SRC, 4, false, FAITHFUL>(c, go);
    }
    return lay.vec ? launch_sweep<NP, SRC, 2, true, FAITHFUL>(c, go) : launch_sweep<NP, SRC, 2, false, FAITHFUL>(c, go);
}

template <int NP, int... SRCS>
int dispatch(int srcmask, const K3Call& c, int mode, const K3Go& go) {
    int rc = (int)hipErrorInvalidValue;
    const bool simple = (mode & 2) != 0;
    if (mode & 1)
        (void)((srcmask == SRCS ? (rc = launch<NP, SRCS, true>(c, simple, go), true) : false) || ...);
    else
        (void)((srcmask == SRCS ? (rc = launch<NP, SRCS, false>(c, simple, go), true) : false) || ...);
    return rc;
}

// argument checks shared by the launcher and the plan query
inline int k3_check_args(int B, int N, int A, int n_points, const int* src, const int* atom, int row_begin, int row_end, int out_rows,
                         int out_row_origin, int exact_angles, AtomSel& sel, int& srcmask) {
    if (!src || !atom || B < 0 || N < 0 || A <= 0) return (int)hipErrorInvalidValue;
    if (exact_angles < 0 || exact_angles > 3) return (int)hipErrorInvalidValue;
    if (n_points != 3 && n_points != 4) return (int)hipErrorInvalidValue;
    if (row_begin < 0 || row_end > N || row_begin > row_end) return (int)hipErrorInvalidValue;
    if (out_row_origin > row_begin || row_end - out_row_origin > out_rows) return (int)hipErrorInvalidValue;
    sel = AtomSel{};
    srcmask = 0;
    for (int k = 0; k < n_points; ++k) {
        if (atom[k] < 0 || atom[k] >= A || (src[k] != 0 && src[k] != 1)) return (int)hipErrorInvalidValue;
        sel.atom[k] = atom[k];
        srcmask |= src[k] << k;
    }
    return 0;
}

inline int k3_run(const K3Call& c, int n_points, int srcmask, int exact_angles, const K3Go& go) {
    if (n_points == 4) return dispatch<4, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15>(srcmask, c, exact_angles, go);
    return dispatch<3, 0, 1, 2, 3, 4, 5, 6, 7>(srcmask, c, exact_angles, go);
}

}  // namespace

extern "C" int ps_pairwise_angles_f32(const float* xyz, float* out, int B, int N, int A, int n_points, const int* src,
                                      const int* atom, int row_begin, int row_end, int out_rows, int out_row_origin,
                                      int exact_angles, void* stream) {
    if (!xyz || !out) return (int)hipErrorInvalidValue;
    K3Call c{xyz, out, B, N, A, AtomSel{}, row_begin, row_end, out_rows, out_row_origin, (unsigned)(reinterpret_cast<uintptr_t>(out) & 15u)};
    int srcmask = 0;
    if (const int e = k3_check_args(B, N, A, n_points, src, atom, row_begin, row_end, out_rows, out_row_origin, exact_angles, c.sel, srcmask))
        return e;
    if (B == 0 || N == 0 || row_begin == row_end) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return k3_run(c, n_points, srcmask, exact_angles, K3Go{s, nullptr, k3_cu_count(s)});
}

extern "C" int ps_k3_plan_f32(int B, int N, int A, int n_points, const int* src, const int* atom, int row_begin, int row_end,
                              int out_rows, int out_row_origin, int out_misalign, int exact_angles, int cu_count,
                              ps_k3_plan* plan) {
    if (!plan || plan->struct_size != (int)sizeof(ps_k3_plan)) return (int)hipErrorInvalidValue;
    k3_plan_reset(plan);
    K3Call c{nullptr, nullptr, B, N, A, AtomSel{}, row_begin, row_end, out_rows, out_row_origin, (unsigned)out_misalign};
    int srcmask = 0;
    if (const int e = k3_check_args(B, N, A, n_points, src, atom, row_begin, row_end, out_rows, out_row_origin, exact_angles, c.sel, srcmask))
        return e;
    if (out_misalign < 0 || out_misalign > 15 || (out_misalign & 3)) return (int)hipErrorInvalidValue;
    if (B == 0 || N == 0 || row_begin == row_end) return 0;
    return k3_run(c, n_points, srcmask, exact_angles, K3Go{nullptr, plan, cu_count > 0 ? cu_count : 256});
}
