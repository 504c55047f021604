// Batched Kabsch alignment -- replaces the per-structure Python loop of
// StructureBatch.align + geometry.kabsch (reference protstruc.py:880-918, geometry.py:442-480):
// for every structure, the rotation R and translation t that minimise the RMSD of R a + t against b over
// the masked atoms.  One workgroup per structure: masked centroids and the 3x3 covariance H = sum (a-ca)(b-cb)^T
// by fp64 block reductions, then (one lane, in double, no atomics) the optimal rotation from the singular vectors of H
// itself, H = U S V^T  =>  R = V diag(1, 1, sign det(V U^T)) U^T -- ps_kabsch_solve of kabsch_solve.hpp, which returns
// a proper rotation for every covariance: rank 2, rank 1 (two atoms, collinear atoms) and H = 0 (one atom: R = I)
// included.  No selected atom: the centroids are 0 / 0 and R, t are set to NaN, as in the reference.  Masked-out atoms
// are never read.  Also emits the minimum distance of every residue's atom to a point set
// (get_topk_nearest_residue_mask, protstruc.py:819-862).
#include "ps_common.hpp"
#include "kabsch_solve.hpp"

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = PS_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// block-wide sums of NV doubles (result in every thread)
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red /* NV*4 + NV */) {
    const int lane = threadIdx.x & (PS_WAVE - 1), wave = threadIdx.x / PS_WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum_d(v[k]);
    __syncthreads();
    if (lane == 0)
        for (int k = 0; k < NV; ++k) red[k * 4 + wave] = v[k];
    __syncthreads();
    if (threadIdx.x < NV) red[NV * 4 + threadIdx.x] = red[threadIdx.x * 4] + red[threadIdx.x * 4 + 1] + red[threadIdx.x * 4 + 2] + red[threadIdx.x * 4 + 3];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = red[NV * 4 + k];
}

__global__ __launch_bounds__(256) void k_kabsch(const float* __restrict__ src, const float* __restrict__ dst,
                                                const uint8_t* __restrict__ mask, float* __restrict__ R_out,
                                                float* __restrict__ t_out, unsigned n_atoms, size_t dst_stride,
                                                size_t mask_stride) {
    __shared__ double red[9 * 4 + 9];
    const unsigned b = blockIdx.x;
    const float* a = src + (size_t)b * n_atoms * 3;
    const float* bb = dst + (size_t)b * dst_stride;
    const uint8_t* m = mask + (size_t)b * mask_stride;

    double s7[7] = {0, 0, 0, 0, 0, 0, 0};  // sum a (3), sum b (3), count
    for (unsigned k = threadIdx.x; k < n_atoms; k += 256)
        if (m[k]) {
            s7[0] += a[k * 3]; s7[1] += a[k * 3 + 1]; s7[2] += a[k * 3 + 2];
            s7[3] += bb[k * 3]; s7[4] += bb[k * 3 + 1]; s7[5] += bb[k * 3 + 2];
            s7[6] += 1.0;
        }
    block_sum<7>(s7, red);
    const double ca[3] = {s7[0] / s7[6], s7[1] / s7[6], s7[2] / s7[6]};
    const double cb[3] = {s7[3] / s7[6], s7[4] / s7[6], s7[5] / s7[6]};

    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // H[i][j] = sum (a_i - ca_i)(b_j - cb_j)
    for (unsigned k = threadIdx.x; k < n_atoms; k += 256)
        if (m[k]) {
            const double da[3] = {a[k * 3] - ca[0], a[k * 3 + 1] - ca[1], a[k * 3 + 2] - ca[2]};
            const double db[3] = {bb[k * 3] - cb[0], bb[k * 3 + 1] - cb[1], bb[k * 3 + 2] - cb[2]};
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) h[i * 3 + j] += da[i] * db[j];
        }
    block_sum<9>(h, red);
    if (threadIdx.x != 0) return;

    double R[3][3];
    ps_kabsch_solve(h, &R[0][0]);
    if (s7[6] == 0.0)   // no selected atom: H is an empty sum, 0, but the reference's centroids are 0 / 0 and its R is NaN
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = ca[0];   // NaN
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R_out[b * 9 + i * 3 + j] = (float)R[i][j];
        t_out[b * 3 + i] = (float)(cb[i] - (R[i][0] * ca[0] + R[i][1] * ca[1] + R[i][2] * ca[2]));
    }
}

// out[n] = min over query points q of | xyz[n][atom] - q |   (one structure)
__global__ __launch_bounds__(256) void k_min_dist(const float* __restrict__ xyz, const float* __restrict__ query,
                                                  float* __restrict__ out, unsigned N, unsigned A, unsigned atom,
                                                  unsigned n_query) {
    const unsigned n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const f3 p = load3(xyz + ((size_t)n * A + atom) * 3);
    float best = __builtin_huge_valf();
    bool any_nan = false;
    for (unsigned q = 0; q < n_query; ++q) {
        const f3 d = sub3(p, load3(query + (size_t)q * 3));
        const float dist = norm3(d);
        any_nan |= (dist != dist);
        best = fminf(best, dist);
    }
    out[n] = any_nan ? __builtin_nanf("") : best;  // torch.min propagates NaN
}

}  // namespace

extern "C" int ps_kabsch_f32(const float* src_xyz, const float* dst_xyz, const uint8_t* atom_mask, float* R, float* t,
                             int B, int n_atoms, int dst_is_shared, int mask_is_shared, void* stream) {
    if (!src_xyz || !dst_xyz || !atom_mask || !R || !t || B < 0 || n_atoms < 0) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    return ps_launch(k_kabsch, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src_xyz, dst_xyz,
                       atom_mask, R, t, (unsigned)n_atoms, dst_is_shared ? (size_t)0 : (size_t)n_atoms * 3,
                       mask_is_shared ? (size_t)0 : (size_t)n_atoms);
}

extern "C" int ps_min_dist_to_points_f32(const float* xyz, const float* query, float* out, int N, int A, int atom,
                                         int n_query, void* stream) {
    if (!xyz || !query || !out || N < 0 || A <= 0 || atom < 0 || atom >= A || n_query <= 0) return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    return ps_launch(k_min_dist, dim3((N + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xyz, query,
                       out, (unsigned)N, (unsigned)A, (unsigned)atom, (unsigned)n_query);
}
