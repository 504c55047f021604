// K10 / K11 -- backbone coordinates from a distance matrix: metric SMACOF (sklearn 1.7's smacof / _smacof_single), then
// the hand and the O / CB atoms, behind geometry.initialize_backbone_with_mds (reference geometry.py:350-410).
//
//   K10 (ps_smacof_f32)  K starts per structure, pass q = 0 .. max_iter, one launch each, then a finish launch.  Pass q
//       reads X^q of every running start and, per row block,
//         * first reduces the per-block float64 partials of sigma_{q-1} and S_{q-1} that pass q-1 wrote, in a fixed
//           order, and applies the stop rule to them -- every workgroup of a structure makes the same decision, so no
//           atomics and no grid-wide barrier are needed (row block 0 carries the per-start state to the next pass);
//         * then, for the starts still running, one sweep over its rows of D: d_ij^q, the Guttman sums
//           X^{q+1}_i = (1/n) sum_j (delta_ij / d~_ij) (x_i - x_j), and the row block's share of
//           sigma_q = 1/2 sum (d - delta)^2 and S_q = sum d^2 (the stress of X^q, which pass q + 1 reduces).
//       A start that stopped at X^t (decided in pass t + 1) is skipped from then on; X^t stays in its half of the double
//       buffer because nothing writes that half again.  After convergence the remaining launches are no-ops, so the
//       launch sequence is fixed by max_iter alone: capturable and bitwise deterministic.
//   K11 (ps_mds_backbone_finish_f32)  per structure: mean phi = dihedral(C_{i-1}, N_i, CA_i, C_i) over i = 1 .. len-1,
//       mirror z iff it is positive (mode 1; mode 0 never mirrors), then CB and O by place4 -- O of the last residue
//       from N of the first (the reference's np.roll).
#include "ps_common.hpp"

namespace {

// ---- K10 ----------------------------------------------------------------------------------------------------------------
constexpr int SM_ROWS = 16;                  // rows (nodes) per workgroup; fixed, so results do not depend on B or K
constexpr int SM_TPR = 16;                   // lanes per row
constexpr int SM_THREADS = SM_ROWS * SM_TPR;
constexpr int SM_KG = 4;                     // starts per sweep over D
constexpr int SM_CT = 512;                   // columns per LDS tile

struct SmState {     // per (structure, start), double-buffered by pass parity
    int done;        // stopped at X^n_iter
    int n_iter;
    double sigma_prev;   // sigma of the previous iterate (the stop rule's sigma_t)
    double stress;       // sigma_{n_iter} once done
    double pad;
};
static_assert(sizeof(SmState) == 32, "SmState layout");

struct SmArgs {
    const float* D;
    const int* lengths;
    const float* init;   // (B, K, G L, 3)
    float* X;            // workspace: 2 x (B, K, G L, 3)
    double* part;        // workspace: 2 x (B, K, nblk, 2)
    SmState* state;      // workspace: 2 x (B, K)
    float* X_out;        // (B, G L, 3)
    double* stress_out;  // (B)
    int* n_iter_out;     // (B)
    int B, G, L, K, max_iter, nblk;
    double eps;
};

__device__ __forceinline__ int sm_len(const SmArgs& a, int b) {
    return a.lengths ? min(max(a.lengths[b], 0), a.L) : a.L;
}

// full-layout index of compact node r of a structure with `len` residues: (g, i) = (r / len, r % len) -> g L + i
__device__ __forceinline__ int sm_full(int r, int len, int L) {
    const int g = r / len;
    return g * L + (r - g * len);
}

// Pass q's decisions for starts k0 .. k0 + SM_KG - 1 (q = max_iter + 1 is the finish): reduces the partials of
// sigma_{q-1}, S_{q-1} in a fixed order (every workgroup of the structure computes the same bits), applies the stop rule,
// and leaves the states in s_st.  Row block 0 (write_state) stores them for the next pass.  Needs the whole workgroup.
__device__ void sm_decide(const SmArgs& a, int b, int k0, int q, int nblk_b, bool write_state, SmState* s_st) {
    const int kn = min(SM_KG, a.K - k0);
    __syncthreads();   // s_st of the previous group is no longer read
    if (threadIdx.x < SM_KG) {
        SmState st{0, 0, 0.0, 0.0, 0.0};
        if (q > 0 && (int)threadIdx.x < kn) st = a.state[((size_t)((q - 1) & 1) * a.B + b) * a.K + k0 + threadIdx.x];
        s_st[threadIdx.x] = st;
    }
    __syncthreads();
    if (q > 0) {
        const int w = threadIdx.x / PS_WAVE, lane = threadIdx.x % PS_WAVE;
        if (w < kn && !s_st[w].done) {   // wave w reduces start k0 + w
            const double* p = a.part + (((size_t)((q - 1) & 1) * a.B + b) * a.K + k0 + w) * (size_t)a.nblk * 2;
            double sg = 0.0, ss = 0.0;
            for (int blk = lane; blk < nblk_b; blk += PS_WAVE) {
                sg += p[2 * blk];
                ss += p[2 * blk + 1];
            }
#pragma unroll
            for (int m = PS_WAVE / 2; m >= 1; m >>= 1) {
                sg += __shfl_xor(sg, m);
                ss += __shfl_xor(ss, m);
            }
            if (lane == 0) {
                SmState st = s_st[w];
                const int t1 = q - 1;   // sg = sigma of X^t1
                if (t1 >= 2 && (st.sigma_prev - sg) / (ss / 2.0) < a.eps) {
                    st.done = 1;
                    st.n_iter = t1;
                    st.stress = sg;
                } else if (t1 >= a.max_iter) {
                    st.done = 1;
                    st.n_iter = t1;
                    st.stress = sg;
                } else {
                    st.sigma_prev = sg;
                }
                s_st[w] = st;
            }
        }
    }
    __syncthreads();
    if (write_state && (int)threadIdx.x < kn)
        a.state[((size_t)(q & 1) * a.B + b) * a.K + k0 + threadIdx.x] = s_st[threadIdx.x];
}

// workgroup (row block, structure); lane (row rr, column phase c) sweeps columns c, c + SM_TPR, ... of row rb*16 + rr
__global__ __launch_bounds__(SM_THREADS) void k10_smacof_pass(SmArgs a, int q) {
    __shared__ __attribute__((aligned(16))) float4 sx[SM_CT][SM_KG];   // X^q of the tile's columns, per start
    __shared__ unsigned s_coff[SM_CT];                                   // column offset h L L + j of D
    __shared__ SmState s_st[SM_KG];
    __shared__ double s_red[SM_ROWS][SM_KG][2];
    const int rb = blockIdx.x, b = blockIdx.y;
    const int len = sm_len(a, b), n = a.G * len, nfull = a.G * a.L;
    if (n == 0) return;
    const int nblk_b = (n + SM_ROWS - 1) / SM_ROWS;
    if (rb >= nblk_b) return;
    const int rr = threadIdx.x / SM_TPR, c = threadIdx.x % SM_TPR;
    const int r = rb * SM_ROWS + rr;
    const bool r_in = r < n;
    const int rf = r_in ? sm_full(r, len, a.L) : 0;
    const size_t LL = (size_t)a.L * a.L;
    // row r of D: D[b][g][h][i][j] = Db[g G L L + i L + h L L + j]
    const float* Drow = nullptr;
    if (r_in) {
        const int g = rf / a.L, i = rf - g * a.L;
        Drow = a.D + (size_t)b * a.G * a.G * LL + (size_t)g * a.G * LL + (size_t)i * a.L;
    }
    const float* Xin = q == 0 ? a.init : a.X + (size_t)(q & 1) * a.B * a.K * nfull * 3;
    float* Xnext = a.X + (size_t)((q + 1) & 1) * a.B * a.K * nfull * 3;
    const float inv_n = 1.0f / (float)n;

    for (int k0 = 0; k0 < a.K; k0 += SM_KG) {
        sm_decide(a, b, k0, q, nblk_b, rb == 0, s_st);
        const int kn = min(SM_KG, a.K - k0);
        bool act[SM_KG];
        bool any = false;
#pragma unroll
        for (int k = 0; k < SM_KG; ++k) {
            act[k] = k < kn && !s_st[k].done;
            any |= act[k];
        }
        if (!any) continue;   // uniform over the workgroup

        f3 xi[SM_KG];
        float ax[SM_KG], ay[SM_KG], az[SM_KG];
        double sg[SM_KG], ss[SM_KG];
#pragma unroll
        for (int k = 0; k < SM_KG; ++k) {
            xi[k] = (act[k] && r_in) ? load3(Xin + (((size_t)b * a.K + k0 + k) * nfull + rf) * 3) : mk3(0.f, 0.f, 0.f);
            ax[k] = ay[k] = az[k] = 0.f;
            sg[k] = ss[k] = 0.0;
        }
        for (int c0 = 0; c0 < n; c0 += SM_CT) {
            const int nc = min(SM_CT, n - c0);
            __syncthreads();   // the previous tile is no longer read
            for (int e = threadIdx.x; e < nc * SM_KG; e += SM_THREADS) {
                const int cc = e / SM_KG, k = e % SM_KG;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < kn && !s_st[k].done) {
                    const float* p = Xin + (((size_t)b * a.K + k0 + k) * nfull + sm_full(c0 + cc, len, a.L)) * 3;
                    v = make_float4(p[0], p[1], p[2], 0.f);
                }
                sx[cc][k] = v;
                if (k == 0) {
                    const int cf = sm_full(c0 + cc, len, a.L);
                    const int h = cf / a.L;
                    s_coff[cc] = (unsigned)h * (unsigned)LL + (unsigned)(cf - h * a.L);
                }
            }
            __syncthreads();
            if (r_in) {
                float tsg[SM_KG], tss[SM_KG];
#pragma unroll
                for (int k = 0; k < SM_KG; ++k) tsg[k] = tss[k] = 0.f;
                for (int cc = c; cc < nc; cc += SM_TPR) {
                    const float delta = Drow[s_coff[cc]];
#pragma unroll
                    for (int k = 0; k < SM_KG; ++k) {
                        if (!act[k]) continue;
                        const float4 xj = sx[cc][k];
                        const float dx = xi[k].x - xj.x, dy = xi[k].y - xj.y, dz = xi[k].z - xj.z;
                        const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                        const float d = __builtin_sqrtf(d2);
                        const float ratio = delta / (d2 == 0.f ? 1e-5f : d);
                        ax[k] += ratio * dx;
                        ay[k] += ratio * dy;
                        az[k] += ratio * dz;
                        const float e = d - delta;
                        tsg[k] += e * e;
                        tss[k] += d * d;
                    }
                }
#pragma unroll
                for (int k = 0; k < SM_KG; ++k) {
                    sg[k] += (double)tsg[k];
                    ss[k] += (double)tss[k];
                }
            }
        }
        // the SM_TPR lanes of a row (aligned groups of 16 in a wave): fixed butterfly
#pragma unroll
        for (int k = 0; k < SM_KG; ++k) {
#pragma unroll
            for (int m = SM_TPR / 2; m >= 1; m >>= 1) {
                ax[k] += __shfl_xor(ax[k], m);
                ay[k] += __shfl_xor(ay[k], m);
                az[k] += __shfl_xor(az[k], m);
                sg[k] += __shfl_xor(sg[k], m);
                ss[k] += __shfl_xor(ss[k], m);
            }
        }
        if (c == 0) {
#pragma unroll
            for (int k = 0; k < SM_KG; ++k) {
                s_red[rr][k][0] = r_in ? 0.5 * sg[k] : 0.0;
                s_red[rr][k][1] = r_in ? ss[k] : 0.0;
                if (act[k] && r_in && q < a.max_iter) {
                    float* p = Xnext + (((size_t)b * a.K + k0 + k) * nfull + rf) * 3;
                    p[0] = ax[k] * inv_n;
                    p[1] = ay[k] * inv_n;
                    p[2] = az[k] * inv_n;
                }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < kn && act[threadIdx.x]) {
            double tg = 0.0, ts = 0.0;
            for (int y = 0; y < SM_ROWS; ++y) {
                tg += s_red[y][threadIdx.x][0];
                ts += s_red[y][threadIdx.x][1];
            }
            double* p = a.part + (((size_t)(q & 1) * a.B + b) * a.K + k0 + threadIdx.x) * (size_t)a.nblk * 2;
            p[2 * rb] = tg;
            p[2 * rb + 1] = ts;
        }
        // s_st and s_red are rewritten by the next group only after the barriers in sm_decide
    }
}

// one workgroup per structure: the last reduction (sigma_{max_iter}), the best start (smallest stress, lowest index on
// ties, a NaN stress never replaces an earlier start -- sklearn's `stress < best_stress`), and its X^n_iter
__global__ __launch_bounds__(SM_THREADS) void k10_smacof_finish(SmArgs a) {
    __shared__ SmState s_st[SM_KG];
    __shared__ int s_best;
    __shared__ double s_best_stress;
    __shared__ int s_best_iter;
    const int b = blockIdx.x;
    const int len = sm_len(a, b), n = a.G * len, nfull = a.G * a.L;
    const float qnan = __builtin_nanf("");
    if (n == 0) {
        for (int e = threadIdx.x; e < nfull * 3; e += SM_THREADS) a.X_out[(size_t)b * nfull * 3 + e] = qnan;
        if (threadIdx.x == 0) {
            a.stress_out[b] = 0.0;
            a.n_iter_out[b] = 0;
        }
        return;
    }
    const int nblk_b = (n + SM_ROWS - 1) / SM_ROWS;
    if (threadIdx.x == 0) {
        s_best = 0;
        s_best_stress = 0.0;
        s_best_iter = 0;
    }
    for (int k0 = 0; k0 < a.K; k0 += SM_KG) {
        sm_decide(a, b, k0, a.max_iter + 1, nblk_b, false, s_st);
        if (threadIdx.x == 0) {
            for (int k = 0; k < min(SM_KG, a.K - k0); ++k) {
                const double s = s_st[k].stress;
                if (k0 + k == 0 || s < s_best_stress) {
                    s_best = k0 + k;
                    s_best_stress = s;
                    s_best_iter = s_st[k].n_iter;
                }
            }
        }
        __syncthreads();
    }
    const int kb = s_best, it = s_best_iter;
    const float* src = a.X + (((size_t)(it & 1) * a.B + b) * a.K + kb) * (size_t)nfull * 3;
    float* dst = a.X_out + (size_t)b * nfull * 3;
    for (int e = threadIdx.x; e < nfull * 3; e += SM_THREADS) {
        const int node = e / 3, i = node % a.L;
        dst[e] = i < len ? src[e] : qnan;
    }
    if (threadIdx.x == 0) {
        a.stress_out[b] = s_best_stress;
        a.n_iter_out[b] = it;
    }
}

// ---- K11 ----------------------------------------------------------------------------------------------------------------
constexpr int FX_THREADS = 256;

// reference constants/ideal.py
constexpr float kAB = (float)1.522, kNAB = (float)1.927, kBANC = (float)-2.143;
constexpr float kCO = (float)1.231, kACO = (float)2.108, kNACO = (float)-3.142;

// one workgroup per structure; X (B, 3, L, 3) in the order N, CA, C; out (B, A_out, L, 3) with A_out = 3 or 5
__global__ __launch_bounds__(FX_THREADS) void k11_mds_backbone_finish(const float* __restrict__ X,
                                                                     const int* __restrict__ lengths,
                                                                     float* __restrict__ out, int L, int mirror_mode,
                                                                     int n_out) {
    __shared__ double s_phi[FX_THREADS];
    const int b = blockIdx.x;
    const int len = lengths ? min(max(lengths[b], 0), L) : L;
    const float* Xb = X + (size_t)b * 3 * L * 3;
    float* ob = out + (size_t)b * n_out * L * 3;
    auto atom = [&](int a, int i) { return load3(Xb + ((size_t)a * L + i) * 3); };
    bool has_nan = false;
    double acc = 0.0;
    for (int i = threadIdx.x; i < len; i += FX_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const f3 p = atom(a, i);
            has_nan |= p.x != p.x || p.y != p.y || p.z != p.z;
        }
        if (i >= 1) acc += (double)dihedral4(atom(2, i - 1), atom(0, i), atom(1, i), atom(2, i));
    }
    s_phi[threadIdx.x] = acc;
    const bool all_nan = __syncthreads_or(has_nan) != 0;   // a NaN anywhere in the valid block: all NaN
    for (int m = FX_THREADS / 2; m >= 1; m >>= 1) {   // fixed-order tree
        if ((int)threadIdx.x < m) s_phi[threadIdx.x] += s_phi[threadIdx.x + m];
        __syncthreads();
    }
    // mean phi > 0  <=>  sum > 0 for len >= 2; with no phi (len < 2) the reference's mean is NaN: no mirror
    const bool mirror = mirror_mode == 1 && len >= 2 && s_phi[0] > 0.0;
    const float qnan = __builtin_nanf("");
    for (int i = threadIdx.x; i < L; i += FX_THREADS) {
        f3 v[5];
        if (i >= len || all_nan) {
#pragma unroll
            for (int a = 0; a < 5; ++a) v[a] = mk3(qnan, qnan, qnan);
        } else {
            f3 nn = atom(0, i), ca = atom(1, i), cc = atom(2, i), nx = atom(0, i + 1 < len ? i + 1 : 0);
            if (mirror) {
                nn.z = -nn.z;
                ca.z = -ca.z;
                cc.z = -cc.z;
                nx.z = -nx.z;
            }
            v[0] = nn;
            v[1] = ca;
            v[2] = cc;
            if (n_out == 5) {
                v[3] = place4(nx, ca, cc, kCO, kACO, kNACO);    // O, with N of residue (i + 1) mod len
                v[4] = place4(cc, nn, ca, kAB, kNAB, kBANC);   // CB
            }
        }
        for (int a = 0; a < n_out; ++a) {
            float* p = ob + ((size_t)a * L + i) * 3;
            p[0] = v[a].x;
            p[1] = v[a].y;
            p[2] = v[a].z;
        }
    }
}

constexpr long long kMaxNodes2 = 0x7FFFFFFFll;   // n * n indexed in 32 bits

long long sm_nblk(int G, int L) { return ((long long)G * L + SM_ROWS - 1) / SM_ROWS; }

}  // namespace

extern "C" long long ps_smacof_workspace_bytes(int B, int K, int G, int L) {
    if (B < 0 || K < 1 || G < 1 || L < 0) return -1;
    const long long bk = (long long)B * K;
    return 2 * bk * (long long)sizeof(SmState) + 2 * bk * sm_nblk(G, L) * 2 * (long long)sizeof(double) +
           2 * bk * (long long)G * L * 3 * (long long)sizeof(float);
}

extern "C" int ps_smacof_f32(const float* D, int B, int G, int L, const int* lengths, const float* init, int K,
                             int max_iter, double eps, float* X_out, double* stress_out, int* n_iter_out,
                             void* workspace, long long workspace_bytes, void* stream) {
    if (B < 0 || B > 65535 || G < 1 || L < 0 || K < 1 || K > 65535 || max_iter < 1 || !(eps >= 0.0))
        return (int)hipErrorInvalidValue;
    const long long n = (long long)G * L;
    if (n * n > kMaxNodes2 || (long long)B * K * n * 3 > kMaxNodes2) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!stress_out || !n_iter_out || (n > 0 && (!D || !init || !X_out))) return (int)hipErrorInvalidValue;
    if (!workspace || workspace_bytes < ps_smacof_workspace_bytes(B, K, G, L)) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || (reinterpret_cast<uintptr_t>(stress_out) & 7u) != 0 ||
        (reinterpret_cast<uintptr_t>(n_iter_out) & 3u) != 0 || (reinterpret_cast<uintptr_t>(D) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(init) & 3u) != 0 || (reinterpret_cast<uintptr_t>(X_out) & 3u) != 0)
        return (int)hipErrorInvalidValue;
    SmArgs a{};
    a.D = D;
    a.lengths = lengths;
    a.init = init;
    char* ws = static_cast<char*>(workspace);
    const long long bk = (long long)B * K;
    a.state = reinterpret_cast<SmState*>(ws);
    a.part = reinterpret_cast<double*>(ws + 2 * bk * sizeof(SmState));
    a.X = reinterpret_cast<float*>(ws + 2 * bk * sizeof(SmState) + 2 * bk * sm_nblk(G, L) * 2 * sizeof(double));
    a.X_out = X_out;
    a.stress_out = stress_out;
    a.n_iter_out = n_iter_out;
    a.B = B;
    a.G = G;
    a.L = L;
    a.K = K;
    a.max_iter = max_iter;
    a.nblk = (int)sm_nblk(G, L);
    a.eps = eps;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n > 0) {
        for (int q = 0; q <= max_iter; ++q) {
            const int rc = ps_launch(k10_smacof_pass, dim3((unsigned)a.nblk, (unsigned)B), dim3(SM_THREADS), 0, s, a, q);
            if (rc) return rc;
        }
    }
    return ps_launch(k10_smacof_finish, dim3((unsigned)B), dim3(SM_THREADS), 0, s, a);
}

extern "C" int ps_mds_backbone_finish_f32(const float* X, const int* lengths, int B, int L, int mirror_mode,
                                          int n_atoms_out, float* out, void* stream) {
    if (B < 0 || B > 65535 || L < 0 || (mirror_mode != 0 && mirror_mode != 1) || (n_atoms_out != 3 && n_atoms_out != 5))
        return (int)hipErrorInvalidValue;
    if ((long long)5 * L * 3 > kMaxNodes2) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0) return 0;
    if (!X || !out) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(X) & 3u) != 0 || (reinterpret_cast<uintptr_t>(out) & 3u) != 0)
        return (int)hipErrorInvalidValue;
    return ps_launch(k11_mds_backbone_finish, dim3((unsigned)B), dim3(FX_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), X, lengths, out, L, mirror_mode, n_atoms_out);
}
