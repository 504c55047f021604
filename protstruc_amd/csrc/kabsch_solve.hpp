// The 3x3 solve of the Kabsch fit: covariance H = sum (a - ca)(b - cb)^T in, rotation R out (both row-major), in double.
// Usable on the host and on the device: the qualifiers expand to nothing when the translation unit is not compiled as HIP,
// so a plain C++ program can run the very code the kernel runs (tools/kabsch_solve_host.cpp, tests/test_align_host.py).
//
//   H = U S V^T,  s0 >= s1 >= s2 >= 0,   R = V diag(1, 1, sign det(V U^T)) U^T = v0 u0^T + v1 u1^T + det(V) v2 (u0 x u1)^T
//
// The last form needs u0 and u1 only, and it is a proper rotation (R R^T = I, det R = +1) whenever V is orthogonal and
// u0, u1 are orthonormal, whatever the rank of H.  Both are obtained from H itself by a one-sided (Hestenes) Jacobi:
// plane rotations J from the right until the columns of G = H J1 J2 ... are mutually orthogonal; then V = J1 J2 ..., and
// the columns of G are s_k u_k.  (The eigenvectors of H^T H, which this replaces, square the condition number: the second
// singular direction was lost from s1 / s0 ~ 1e-8 on, and u1 = H v1 / |H v1| was then neither unit nor orthogonal to u0.)
//   * u0 = g0 / |g0|; u1 = g1 made orthogonal to u0 (twice, so that rounding in the first pass is removed by the second)
//     and normalised.  Its direction carries an error of about eps s0 / s1, which costs the fit s1 (eps s0 / s1)^2: nothing.
//   * rank 1 (two atoms, collinear atoms): when what is left of g1 is below KABSCH_RANK_TOL * s0, u1 is an explicit
//     orthogonal complement of u0.  The optimum is then a family (any turn about the line fits as well); this picks one
//     member.  The fit loses at most 2 s1 <= 2e-14 s0 against the optimum.
//   * H = 0 (one atom, coincident atoms): R = I, the reference's result (the SVD of the zero matrix is U = V = I).
//   * a NaN or infinite entry of H: every entry of R is NaN.  (No selected atom is the caller's case: H is then an empty
//     sum, 0, and the kernel sets R to NaN itself, as the reference's 0 / 0 centroids do.)
// H is divided by its largest entry first: R does not depend on the scale of H, and the thresholds become relative.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PS_HOST_DEVICE __host__ __device__
#else
#define PS_HOST_DEVICE
#endif

#define KABSCH_RANK_TOL 1e-14
#define KABSCH_MAX_SWEEPS 30

PS_HOST_DEVICE inline void ps_kabsch_solve(const double h[9], double R[9]) {
    double big = 0.0;
    bool finite = true;
    for (int i = 0; i < 9; ++i) {
        const double x = fabs(h[i]);
        finite = finite && (x <= 1.7976931348623157e308);   // false for NaN and inf
        big = x > big ? x : big;
    }
    if (!finite) {
        for (int i = 0; i < 9; ++i) R[i] = NAN;
        return;
    }
    if (big == 0.0) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double G[3][3], V[3][3];   // columns g_k = H v_k
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            G[i][j] = h[i * 3 + j] / big;
            V[i][j] = (i == j) ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < KABSCH_MAX_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = G[0][p] * G[0][p] + G[1][p] * G[1][p] + G[2][p] * G[2][p];
                const double beta = G[0][q] * G[0][q] + G[1][q] * G[1][q] + G[2][q] * G[2][q];
                const double gamma = G[0][p] * G[0][q] + G[1][p] * G[1][q] + G[2][p] * G[2][q];
                if (gamma == 0.0 || fabs(gamma) <= 2.220446049250313e-16 * (sqrt(alpha) * sqrt(beta))) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = c * t;
                for (int k = 0; k < 3; ++k) {
                    const double gp = G[k][p], gq = G[k][q], vp = V[k][p], vq = V[k][q];
                    G[k][p] = c * gp - s * gq;
                    G[k][q] = s * gp + c * gq;
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
    double n2[3];
    for (int k = 0; k < 3; ++k) n2[k] = G[0][k] * G[0][k] + G[1][k] * G[1][k] + G[2][k] * G[2][k];
    int o0 = 0, o1 = 1, o2 = 2;   // singular values descending
    if (n2[o0] < n2[o1]) { const int x = o0; o0 = o1; o1 = x; }
    if (n2[o0] < n2[o2]) { const int x = o0; o0 = o2; o2 = x; }
    if (n2[o1] < n2[o2]) { const int x = o1; o1 = o2; o2 = x; }
    const double s0 = sqrt(n2[o0]);   // >= 1 / sqrt(3): the largest entry of G was 1 and the rotations keep |G|_F
    double u0[3], u1[3];
    for (int i = 0; i < 3; ++i) {
        u0[i] = G[i][o0] / s0;
        u1[i] = G[i][o1];
    }
    double d = u1[0] * u0[0] + u1[1] * u0[1] + u1[2] * u0[2];
    for (int i = 0; i < 3; ++i) u1[i] -= d * u0[i];
    double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    if (!(n1 > KABSCH_RANK_TOL * s0)) {   // rank 1: complete the basis from the axis u0 is furthest from
        const double ax = fabs(u0[0]), ay = fabs(u0[1]), az = fabs(u0[2]);
        const int j = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
        for (int i = 0; i < 3; ++i) u1[i] = (i == j ? 1.0 : 0.0) - u0[j] * u0[i];
        n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);   // >= sqrt(2 / 3)
    }
    for (int i = 0; i < 3; ++i) u1[i] /= n1;
    d = u1[0] * u0[0] + u1[1] * u0[1] + u1[2] * u0[2];
    for (int i = 0; i < 3; ++i) u1[i] -= d * u0[i];
    n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    for (int i = 0; i < 3; ++i) u1[i] /= n1;
    const double ux[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
    const double detV = V[0][o0] * (V[1][o1] * V[2][o2] - V[2][o1] * V[1][o2]) -
                        V[1][o0] * (V[0][o1] * V[2][o2] - V[2][o1] * V[0][o2]) +
                        V[2][o0] * (V[0][o1] * V[1][o2] - V[1][o1] * V[0][o2]);
    const double sgn = detV < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = V[i][o0] * u0[j] + V[i][o1] * u1[j] + sgn * V[i][o2] * ux[j];
}
