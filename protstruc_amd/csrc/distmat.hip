// K8 / K9 -- backbone N / CA / C distance matrices from inter-residue geometry: the inverse of the featuriser, behind
// geometry.reconstruct_backbone_distmat_from_interresidue_geometry (reference geometry.py:229-347, the trRosetta step).
//
//   K8  (ps_backbone_distmat_init_f32)  steps 1-6: per pair (i, j), residue j's N / CA / C / CB placed in residue i's
//       ideal frame from d_cb, phi, theta, omega (four place4), the nine |x_a - y_b|, and every categorical entry
//       (diagonal, bonds, chain breaks, pair mask, nan_to_num, padded residues) in the same launch.
//   K9  (ps_floyd_warshall_f32)  step 7: the reference's all-pairs update, D[r][c] <- min(D[r][c], D[k][r] + D[k][c])
//       for k = 0 .. n-1 in order, blocked.  The rule reads row k only, and with every entry >= 0 row k does not change
//       during its own step.  So for a pivot block K:
//         (A) panel -- the |K| rows of K evolve through |K| sequential steps (in registers); P[k] = row k as step k
//             reads it;
//         (B) update -- every row r outside K takes min(D[r][c], min_k P[k][r] + P[k][c]), a min-plus product of the
//             snapshot panel with its own transpose.
//       Every candidate is the same single float32 addition of the same operands as in the sequential loop, and min
//       is exact and order-free, so the blocked result equals the sequential loop bit for bit.
//   finish (ps_backbone_distmat_finish_f32)  steps 8-9: (D + D^T) / 2 in place, the bond overrides again, NaN for
//       padded residues.
// No atomics, no grid-wide barriers: every launch is a pure function of the buffers, and the sequence is capturable.
#include "ps_common.hpp"

#include <cfloat>

namespace {

constexpr float kMASK = 12345679.0f;   // geometry.MASK (reference geometry.py:21); exact in float32

// reference constants/ideal.py, rounded to float32
constexpr float kNA = (float)1.458, kAC = (float)1.523, kC_N = (float)1.329, kNC = (float)2.460;
constexpr float kBA = (float)1.522, kBAN = (float)1.927, kANC = (float)0.615, kBANC = (float)-2.143;

// ideal_local_frame() (reference geometry.py:171-188: N at the origin, CA on +z) evaluated in float64, rounded to
// float32: N, CA, C, CB
constexpr float kXca_z = 1.4579999446868896f;
constexpr float kXc_x = -1.1932344436645508f, kXc_y = -0.7685407996177673f, kXc_z = 2.0092625617980957f;
constexpr float kXcb_y = 1.4264601469039917f, kXcb_z = 1.9887498617172241f;

// the diagonal of the nine planes before the overrides: 0 for a == b, ideal.as_dict["ab"] otherwise
__device__ __forceinline__ float diag_value(int a, int b) {
    if (a == b) return 0.f;
    if (a + b == 1) return kNA;          // N-CA, CA-N
    if (a + b == 3) return kAC;          // CA-C, C-CA
    return kNC;                          // N-C, C-N
}

__device__ __forceinline__ float nan_to_mask(float v) {   // torch.nan_to_num(v, nan=MASK)
    if (v != v) return kMASK;
    return fminf(fmaxf(v, -FLT_MAX), FLT_MAX);
}

// ---- K8 ---------------------------------------------------------------------------------------------------------------
constexpr int K8_TILE = 32;                 // 32 x 32 pairs per workgroup, 4 consecutive j per lane
constexpr int K8_THREADS = 256;

template <bool VEC>
__global__ __launch_bounds__(K8_THREADS) void k8_distmat_init(
    const float* __restrict__ d_cb, const float* __restrict__ omega, const float* __restrict__ theta,
    const float* __restrict__ phi, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ breaks,
    const int* __restrict__ lengths, float* __restrict__ out, int L) {
    __shared__ float phiT[K8_TILE][K8_TILE + 1];     // phiT[jj][ii] = phi[j0 + jj][i0 + ii]
    __shared__ float thetaT[K8_TILE][K8_TILE + 1];
    const int j0 = blockIdx.x * K8_TILE, i0 = blockIdx.y * K8_TILE, b = blockIdx.z;
    const size_t LL = (size_t)L * L;
    const size_t sb = (size_t)b * LL;

    // the transposed operands phi[j, i] and theta[j, i], read along rows (coalesced) and staged through LDS
    for (int e = threadIdx.x; e < K8_TILE * K8_TILE; e += K8_THREADS) {
        const int jj = e / K8_TILE, ii = e % K8_TILE;
        const int j = j0 + jj, i = i0 + ii;
        const bool in = j < L && i < L;
        phiT[jj][ii] = in ? phi[sb + (size_t)j * L + i] : 0.f;
        thetaT[jj][ii] = in ? theta[sb + (size_t)j * L + i] : 0.f;
    }
    __syncthreads();

    const int ii = threadIdx.x / (K8_TILE / 4), jq = threadIdx.x % (K8_TILE / 4);
    const int i = i0 + ii;
    if (i >= L) return;
    const int len = lengths ? min(max(lengths[b], 0), L) : L;

    const f3 xN = mk3(0.f, 0.f, 0.f), xCA = mk3(0.f, 0.f, kXca_z), xC = mk3(kXc_x, kXc_y, kXc_z),
             xCB = mk3(0.f, kXcb_y, kXcb_z);
    const f3 xs[3] = {xN, xCA, xC};

    float v[9][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int jj = jq * 4 + q, j = j0 + jj;
        if (j >= L) {
#pragma unroll
            for (int e = 0; e < 9; ++e) v[e][q] = 0.f;
            continue;
        }
        if (i >= len || j >= len) {   // a padded residue: an inert node
#pragma unroll
            for (int e = 0; e < 9; ++e) v[e][q] = (i == j && e % 4 == 0) ? 0.f : kMASK;
            continue;
        }
        if (i == j) {
#pragma unroll
            for (int e = 0; e < 9; ++e) v[e][q] = diag_value(e / 3, e % 3);
        } else {
            const size_t p = sb + (size_t)i * L + j;
            const float phi_ij = phi[p], theta_ij = theta[p], phi_ji = phiT[jj][ii], theta_ji = thetaT[jj][ii];
            const f3 yCB = place4(xN, xCA, xCB, d_cb[p], phi_ij, theta_ij);
            const f3 yCA = place4(xCA, xCB, yCB, kBA, phi_ji, omega[p]);
            const f3 yN = place4(xCB, yCB, yCA, kNA, kBAN, theta_ji);
            const f3 yC = place4(yCB, yCA, yN, kNC, kANC, kBANC);
            const f3 ys[3] = {yN, yCA, yC};
#pragma unroll
            for (int e = 0; e < 9; ++e) v[e][q] = dist3(xs[e / 3], ys[e % 3]);
        }
        // the peptide bonds and chain breaks: [C, N, i, i+1] and [N, C, i+1, i]
        if (j == i + 1) v[2 * 3 + 0][q] = (breaks && breaks[(size_t)b * L + i]) ? kMASK : kC_N;
        if (i == j + 1) v[0 * 3 + 2][q] = (breaks && breaks[(size_t)b * L + j]) ? kMASK : kC_N;
        if (mask && !mask[sb + (size_t)i * L + j]) {
#pragma unroll
            for (int e = 0; e < 9; ++e) v[e][q] = kMASK;
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) v[e][q] = nan_to_mask(v[e][q]);
    }

    const int jbase = j0 + jq * 4;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        float* row = out + ((size_t)b * 9 + e) * LL + (size_t)i * L;
        if (VEC) {   // L % 4 == 0 and a 16-byte aligned base: the four j are one aligned float4 (or all beyond L)
            if (jbase < L) *reinterpret_cast<float4*>(row + jbase) = make_float4(v[e][0], v[e][1], v[e][2], v[e][3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (jbase + q < L) row[jbase + q] = v[e][q];
        }
    }
}

// ---- K9 ---------------------------------------------------------------------------------------------------------------
// node (g, i) = g * L + i of a (G, G, L, L) matrix: D[(g, i)][(h, j)] at (g * G + h) * L * L + i * L + j, the sum of a
// row offset and a column offset (32-bit: the host refuses n * n >= 2^31)
constexpr int FW_B = 64;          // pivot block
constexpr int FW_PT = 64;         // panel: columns per workgroup
constexpr int FW_PTHREADS = 1024;   // 4 rows of a column per lane: 16 waves hide the per-step barrier
constexpr int FW_UT = 128;        // update: a 128 x 128 tile per workgroup, 8 x 8 elements per lane (16 x 16 lanes)
constexpr int FW_UTHREADS = 256;

__device__ __forceinline__ unsigned fw_rowoff(int r, int G, int L) {
    const unsigned g = (unsigned)r / (unsigned)L, i = (unsigned)r - g * (unsigned)L;
    return (g * (unsigned)G * (unsigned)L + i) * (unsigned)L;
}
__device__ __forceinline__ unsigned fw_coloff(int c, int L) {
    const unsigned h = (unsigned)c / (unsigned)L, j = (unsigned)c - h * (unsigned)L;
    return h * (unsigned)L * (unsigned)L + j;
}

// (A): workgroup (column tile, structure).  Evolves the nb x nb diagonal block and its own nb x FW_PT column tile
// through the nb steps of the block (the diagonal block redundantly in every workgroup), writes the snapshots
// P[k][c] and, at the end, the final rows of K.  Lane (c, grp) holds rows FW_PROWS grp .. FW_PROWS grp + FW_PROWS - 1
// (4 rows) of column c of both in registers; at step kk the owners of row kk publish it through a double-buffered LDS
// row, so a step costs one barrier.  Every workgroup of a structure reads the initial diagonal block D[K][K], so D[K][K]
// must not change during this launch: the workgroup whose column tile is K writes its final block to F instead, and
// the update launch, stream-ordered after this one, stores F into D.  Every other workgroup writes only its own
// columns of the rows of K, which no other workgroup reads.
constexpr int FW_PROWS = FW_B / (FW_PTHREADS / FW_PT);   // rows per lane
static_assert(FW_PT == FW_B && FW_PROWS % 4 == 0, "the panel lays the diagonal block out like a column tile");

__global__ __launch_bounds__(FW_PTHREADS) void k9_fw_panel(float* D, float* __restrict__ P, float* __restrict__ F,
                                                          int G, int L, int k0, int nb) {
    __shared__ __attribute__((aligned(16))) float rowT[2][FW_PT];   // row kk of the column tile
    __shared__ __attribute__((aligned(16))) float rowD[2][FW_B];    // row kk of the diagonal block
    const int n = G * L;
    const int c0 = blockIdx.x * FW_PT, b = blockIdx.y;
    float* Db = D + (size_t)b * n * n;   // read and written in disjoint places (see above)
    float* __restrict__ Pb = P + (size_t)b * FW_B * n;
    const bool diag_tile = c0 == k0;
    const int c = threadIdx.x % FW_PT, grp = threadIdx.x / FW_PT, rbase = grp * FW_PROWS;
    const bool c_in = c0 + c < n, m_in = c < nb;
    const unsigned coff = c_in ? fw_coloff(c0 + c, L) : 0u, moff = m_in ? fw_coloff(k0 + c, L) : 0u;
    float t[FW_PROWS], d[FW_PROWS];   // tile[rbase + q][c], diag[rbase + q][c]
#pragma unroll
    for (int q = 0; q < FW_PROWS; ++q) {
        const bool r_in = rbase + q < nb;
        const unsigned roff = r_in ? fw_rowoff(k0 + rbase + q, G, L) : 0u;
        t[q] = (r_in && c_in) ? Db[roff + coff] : 0.f;
        d[q] = (r_in && m_in) ? Db[roff + moff] : 0.f;
    }
    for (int g = 0; g * FW_PROWS < nb; ++g) {
#pragma unroll
        for (int q = 0; q < FW_PROWS; ++q) {
            const int kk = g * FW_PROWS + q;
            if (kk >= nb) break;
            const int buf = kk & 1;
            if (grp == g) {   // the owners of row kk publish it (it does not change during its own step)
                rowT[buf][c] = t[q];
                rowD[buf][c] = d[q];
                if (c_in) Pb[(size_t)kk * n + c0 + c] = t[q];
            }
            __syncthreads();   // one barrier per step: the other buffer was last read before this barrier
            const float tk = rowT[buf][c], dk = rowD[buf][c];
            float w[FW_PROWS];   // diag[kk][rbase + q2]
#pragma unroll
            for (int h = 0; h < FW_PROWS / 4; ++h) {
                const float4 v = reinterpret_cast<const float4*>(&rowD[buf][rbase])[h];
                w[4 * h] = v.x; w[4 * h + 1] = v.y; w[4 * h + 2] = v.z; w[4 * h + 3] = v.w;
            }
#pragma unroll
            for (int q2 = 0; q2 < FW_PROWS; ++q2) {
                if (rbase + q2 == kk) continue;   // row kk is read, never written, during its own step
                t[q2] = fminf(t[q2], w[q2] + tk);
                d[q2] = fminf(d[q2], w[q2] + dk);
            }
        }
    }
    if (diag_tile) {   // c_in == m_in here: the tile's columns are K
        float* __restrict__ Fb = F + (size_t)b * FW_B * FW_B;
#pragma unroll
        for (int q = 0; q < FW_PROWS; ++q)
            if (rbase + q < nb && m_in) Fb[(rbase + q) * FW_B + c] = t[q];
    } else if (c_in) {
#pragma unroll
        for (int q = 0; q < FW_PROWS; ++q)
            if (rbase + q < nb) Db[fw_rowoff(k0 + rbase + q, G, L) + coff] = t[q];
    }
}

// (B): workgroup (column tile, row tile, structure).  Lane (tx, ty) owns rows r0 + ty + 16 p and columns c0 + tx + 16 q
// (p, q < 8): its D loads and stores coalesce over tx.  The snapshots sit in LDS as float2 pairs of consecutive pivots,
// permuted so that a lane's eight rows (columns) are 16 contiguous floats; each pair of pivots then costs per element
// one packed add (v_pk_add_f32) and one three-way min.  Rows of K are not updated (the panel wrote them), except for
// D[K][K], which the workgroup covering it copies from the panel's F.
__global__ __launch_bounds__(FW_UTHREADS) void k9_fw_update(float* __restrict__ D, const float* __restrict__ P,
                                                           const float* __restrict__ F, int G, int L, int k0, int nb) {
    __shared__ __attribute__((aligned(16))) f32x2 pr[FW_B / 2][FW_UT];   // pr[kp][perm(x)] = (P[2kp][r0 + x], P[2kp + 1][r0 + x])
    __shared__ __attribute__((aligned(16))) f32x2 pc[FW_B / 2][FW_UT];
    const int n = G * L;
    const int c0 = blockIdx.x * FW_UT, r0 = blockIdx.y * FW_UT, b = blockIdx.z;
    float* __restrict__ Db = D + (size_t)b * n * n;
    const float* __restrict__ Pb = P + (size_t)b * FW_B * n;
    const float* __restrict__ Fb = F + (size_t)b * FW_B * FW_B;
    const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;

    const int nbp = (nb + 1) / 2;
    for (int e = threadIdx.x; e < nbp * 2 * FW_UT; e += FW_UTHREADS) {
        const int kk = e / FW_UT, x = e % FW_UT;
        const int pos = (x % 16) * 8 + x / 16;
        const bool k_in = kk < nb;   // an odd block's missing pivot contributes +inf candidates
        const float vr = !k_in ? __builtin_inff() : (r0 + x < n ? Pb[(size_t)kk * n + r0 + x] : 0.f);
        const float vc = !k_in ? __builtin_inff() : (c0 + x < n ? Pb[(size_t)kk * n + c0 + x] : 0.f);
        reinterpret_cast<float*>(&pr[kk / 2][pos])[kk % 2] = vr;
        reinterpret_cast<float*>(&pc[kk / 2][pos])[kk % 2] = vc;
    }

    unsigned roff[8], coff[8];
    bool rin[8], cin[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int r = r0 + ty + 16 * p, c = c0 + tx + 16 * p;
        rin[p] = r < n && !(r >= k0 && r < k0 + nb);
        cin[p] = c < n;
        roff[p] = r < n ? fw_rowoff(r, G, L) : 0u;
        coff[p] = cin[p] ? fw_coloff(c, L) : 0u;
    }
    float acc[8][8];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[p][q] = (rin[p] && cin[q]) ? Db[roff[p] + coff[q]] : 0.f;
    __syncthreads();

    for (int kp = 0; kp < nbp; ++kp) {
        f32x2 a[8], w[8];
        const float4* ar = reinterpret_cast<const float4*>(&pr[kp][ty * 8]);
        const float4* wc = reinterpret_cast<const float4*>(&pc[kp][tx * 8]);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const float4 x = ar[h], y = wc[h];
            a[2 * h] = f32x2{x.x, x.y};
            a[2 * h + 1] = f32x2{x.z, x.w};
            w[2 * h] = f32x2{y.x, y.y};
            w[2 * h + 1] = f32x2{y.z, y.w};
        }
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x2 s = a[p] + w[q];   // (P[k][r] + P[k][c], P[k+1][r] + P[k+1][c])
                acc[p][q] = fminf(fminf(acc[p][q], s.x), s.y);
            }
    }

#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (rin[p] && cin[q]) {
                Db[roff[p] + coff[q]] = acc[p][q];
            } else {   // the panel's final diagonal block D[K][K]
                const int rk = r0 + ty + 16 * p - k0, ck = c0 + tx + 16 * q - k0;
                if (rk >= 0 && rk < nb && ck >= 0 && ck < nb) Db[roff[p] + coff[q]] = Fb[rk * FW_B + ck];
            }
        }
}

// ---- finish -------------------------------------------------------------------------------------------------------------
constexpr int FIN_T = 32;
constexpr int FIN_THREADS = 256;

// step 9 and the padding on a symmetrised entry of node pair ((a, i), (c, j))
__device__ __forceinline__ float finish_value(float s, int a, int i, int c, int j, int len,
                                              const uint8_t* __restrict__ brk) {
    if (i >= len || j >= len) return __builtin_nanf("");
    if (i == j && a + c == 1 && a != c) return kNA;
    if (i == j && a + c == 3 && a != c) return kAC;
    if (a == 2 && c == 0 && j == i + 1 && !(brk && brk[i])) return kC_N;
    if (a == 0 && c == 2 && i == j + 1 && !(brk && brk[j])) return kC_N;
    return s;
}

// workgroup (column tile tc, row tile tr, structure) with tr <= tc: reads tiles (tr, tc) and (tc, tr), writes both
__global__ __launch_bounds__(FIN_THREADS) void k9_distmat_finish(float* __restrict__ D, const uint8_t* __restrict__ breaks,
                                                                const int* __restrict__ lengths, int L) {
    const int tc = blockIdx.x, tr = blockIdx.y, b = blockIdx.z;
    if (tr > tc) return;
    __shared__ float A[FIN_T][FIN_T + 1];    // A[y][x] = D[r0 + y][c0 + x]
    __shared__ float Bt[FIN_T][FIN_T + 1];   // Bt[y][x] = D[c0 + y][r0 + x]
    const int n = 3 * L;
    const int r0 = tr * FIN_T, c0 = tc * FIN_T;
    float* __restrict__ Db = D + (size_t)b * n * n;
    const uint8_t* brk = breaks ? breaks + (size_t)b * L : nullptr;
    const int len = lengths ? min(max(lengths[b], 0), L) : L;
    const int x = threadIdx.x % FIN_T;
    for (int y = threadIdx.x / FIN_T; y < FIN_T; y += FIN_THREADS / FIN_T) {
        A[y][x] = (r0 + y < n && c0 + x < n) ? Db[fw_rowoff(r0 + y, 3, L) + fw_coloff(c0 + x, L)] : 0.f;
        Bt[y][x] = (c0 + y < n && r0 + x < n) ? Db[fw_rowoff(c0 + y, 3, L) + fw_coloff(r0 + x, L)] : 0.f;
    }
    __syncthreads();
    for (int y = threadIdx.x / FIN_T; y < FIN_T; y += FIN_THREADS / FIN_T) {
        if (r0 + y < n && c0 + x < n) {   // entry (r0 + y, c0 + x)
            const int r = r0 + y, c = c0 + x;
            const float s = (A[y][x] + Bt[x][y]) / 2.0f;
            Db[fw_rowoff(r, 3, L) + fw_coloff(c, L)] = finish_value(s, r / L, r % L, c / L, c % L, len, brk);
        }
        if (tr != tc && c0 + y < n && r0 + x < n) {   // entry (c0 + y, r0 + x)
            const int r = c0 + y, c = r0 + x;
            const float s = (Bt[y][x] + A[x][y]) / 2.0f;
            Db[fw_rowoff(r, 3, L) + fw_coloff(c, L)] = finish_value(s, r / L, r % L, c / L, c % L, len, brk);
        }
    }
}

constexpr long long kMaxNodes2 = 0x7FFFFFFFll;   // n * n indexed in 32 bits

}  // namespace

extern "C" int ps_backbone_distmat_init_f32(const float* d_cb, const float* omega, const float* theta, const float* phi,
                                            const uint8_t* mask, const uint8_t* chain_breaks, const int* lengths,
                                            float* out, int B, int L, void* stream) {
    if (!d_cb || !omega || !theta || !phi || !out || B < 0 || L < 0 || B > 65535) return (int)hipErrorInvalidValue;
    if ((long long)9 * L * L > kMaxNodes2) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(out) & 3u) != 0) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0) return 0;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned nt = (unsigned)((L + K8_TILE - 1) / K8_TILE);
    const dim3 grid(nt, nt, (unsigned)B);
    if (L % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0)
        return ps_launch(k8_distmat_init<true>, grid, dim3(K8_THREADS), 0, s, d_cb, omega, theta, phi, mask,
                         chain_breaks, lengths, out, L);
    return ps_launch(k8_distmat_init<false>, grid, dim3(K8_THREADS), 0, s, d_cb, omega, theta, phi, mask, chain_breaks,
                     lengths, out, L);
}

extern "C" long long ps_floyd_warshall_workspace_bytes(int B, int G, int L) {
    if (B < 0 || G < 1 || L < 0) return -1;
    // P: FW_B snapshot rows of n floats per structure; F: the panel's final FW_B x FW_B diagonal block per structure
    return (long long)B * FW_B * ((long long)G * L + FW_B) * (long long)sizeof(float);
}

extern "C" int ps_floyd_warshall_f32(float* D, int B, int G, int L, void* workspace, long long workspace_bytes,
                                     void* stream) {
    if (!D || B < 0 || G < 1 || L < 0 || B > 65535) return (int)hipErrorInvalidValue;
    const long long n = (long long)G * L;
    if (n * n > kMaxNodes2) return (int)hipErrorInvalidValue;
    if (B == 0 || n == 0) return 0;
    if (!workspace || workspace_bytes < ps_floyd_warshall_workspace_bytes(B, G, L)) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(workspace) & 3u) != 0 || (reinterpret_cast<uintptr_t>(D) & 3u) != 0)
        return (int)hipErrorInvalidValue;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* P = static_cast<float*>(workspace);
    float* F = P + (size_t)B * FW_B * n;
    const unsigned npt = (unsigned)((n + FW_PT - 1) / FW_PT), nut = (unsigned)((n + FW_UT - 1) / FW_UT);
    for (int k0 = 0; k0 < n; k0 += FW_B) {
        const int nb = (int)((n - k0) < FW_B ? (n - k0) : FW_B);
        int rc = ps_launch(k9_fw_panel, dim3(npt, (unsigned)B), dim3(FW_PTHREADS), 0, s, D, P, F, G, L, k0, nb);
        if (rc) return rc;
        // always launched: besides the rows outside K it stores the panel's final D[K][K]
        rc = ps_launch(k9_fw_update, dim3(nut, nut, (unsigned)B), dim3(FW_UTHREADS), 0, s, D, P, F, G, L, k0, nb);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int ps_backbone_distmat_finish_f32(float* D, const uint8_t* chain_breaks, const int* lengths, int B, int L,
                                              void* stream) {
    if (!D || B < 0 || L < 0 || B > 65535) return (int)hipErrorInvalidValue;
    if ((long long)9 * L * L > kMaxNodes2) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(D) & 3u) != 0) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0) return 0;
    const unsigned nt = (unsigned)((3 * L + FIN_T - 1) / FIN_T);
    return ps_launch(k9_distmat_finish, dim3(nt, nt, (unsigned)B), dim3(FIN_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), D, chain_breaks, lengths, L);
}
