// The box test of the radius graph (K47 / K48): which blocks of candidate points a wave of queries may drop unseen.
// Compiles for the device and, with a plain C++ compiler, for the host: tools/radius_box_host.cpp runs these very
// functions on the CPU (tests/test_radius_host.py), as tools/kabsch_solve_host.cpp does for csrc/kabsch_solve.hpp.
//
// A BOX is the axis-aligned bounding box of the finite points of a set, lo[3] and hi[3], and their number n.  min and max
// of float32 values are exact, so a box is the same in whatever order it is accumulated, and every point p of the set has
// lo[a] <= p[a] <= hi[a] exactly.  An empty box is lo = +inf, hi = -inf, n = 0.
//
// THE TEST.  For boxes A (queries) and B (candidates), per axis
//     gap_a = max(0, A.lo[a] - B.hi[a], B.lo[a] - A.hi[a])                  in float32
//     G     = (gap_x * gap_x + gap_y * gap_y) + gap_z * gap_z               in float32, every operation rounded on its own
// and B is DROPPED for A iff  B.n == 0  or  G > reject_above(C2) = fl32(C2) * (1 + 2^-20) + 2^-126   (K24's bound, with
// the cutoff in the place of its threshold).
//
// WHY NO NEIGHBOUR PAIR IS EVER DROPPED.  Take q in A, j in B with the pair's double d2 <= C2 (the definition of
// include/protstruc_graph.h).  In real numbers |j[a] - q[a]| >= g_a, the exact gap of the two boxes on axis a, because q
// and j lie inside them; so the real squared distance is >= S = sum g_a^2, and the double d2, five roundings of 2^-53 off
// the real one, is >= S (1 - 2^-50).  The float32 G differs from S by five roundings of u = 2^-24 relative -- the
// subtraction that forms a gap (max and the comparison with 0 are exact), its square, the two sums: G <= S (1 + u)^5.  The
// bound carries three roundings -- the conversion of C2, the product, the sum --: it is >= C2 (1 - u)^3 (1 + 16 u).  So
// d2 <= C2 gives G <= C2 (1 + u)^5 / (1 - 2^-50) < C2 (1 + 6 u), and the bound is > C2 (1 + 12 u): G <= bound.  The
// margin of 2^-20 = 16 u covers the eight float32 roundings twice over (K24's budget, knn.hip).  Underflow: a float32 subtraction
// is exact where its result is subnormal; a square, the conversion of C2 or its product can underflow and then err by at most
// 2^-149 each, at most five times, which the 2^-126 covers.  Overflow: a gap that overflows to +inf comes from points
// more than 2^128 (1 - 2^-25) apart on that axis, further than any finite float32 cutoff; fl32(C2) = +inf makes the
// bound +inf, and G > +inf is false: nothing is dropped.  A NaN never arises: boxes hold finite values only, and
// inf - inf cannot occur because an empty box is dropped by its n before any arithmetic.
//
// A single point is the box lo = hi = the point: the same function tests one query against a box (the per-lane level).
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PS_BOX_HD __host__ __device__ __forceinline__
#else
#define PS_BOX_HD inline
#endif

struct ps_box {
    float lo[3], hi[3];
    int n;
};

PS_BOX_HD ps_box ps_box_empty() {
    return ps_box{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0};
}

PS_BOX_HD bool ps_finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;   // false for NaN
}

// the box with the point (x, y, z) added; a point with a NaN or infinite coordinate is left out
PS_BOX_HD ps_box ps_box_add(ps_box b, float x, float y, float z) {
    if (!ps_finite3(x, y, z)) return b;
    const float p[3] = {x, y, z};
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = p[a] < b.lo[a] ? p[a] : b.lo[a];
        b.hi[a] = p[a] > b.hi[a] ? p[a] : b.hi[a];
    }
    ++b.n;
    return b;
}

// what the float32 G of two boxes that hold a pair with d2 <= C2 never exceeds
PS_BOX_HD float ps_radius_reject_above(double C2) { return (float)C2 * (1.0f + 0x1p-20f) + 0x1p-126f; }

// G of the header: the squared gap between two non-empty boxes, in float32
PS_BOX_HD float ps_box_gap2(const float* alo, const float* ahi, const float* blo, const float* bhi) {
    float g[3];
    for (int a = 0; a < 3; ++a) {
        const float d1 = alo[a] - bhi[a], d2 = blo[a] - ahi[a];
        const float d = d1 > d2 ? d1 : d2;
        g[a] = d > 0.0f ? d : 0.0f;
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

// whether candidates (blo, bhi, bn) are dropped for queries (alo, ahi); `bound` = ps_radius_reject_above(C2)
PS_BOX_HD bool ps_box_dropped(const float* alo, const float* ahi, const float* blo, const float* bhi, int bn, float bound) {
    return bn == 0 || ps_box_gap2(alo, ahi, blo, bhi) > bound;
}
