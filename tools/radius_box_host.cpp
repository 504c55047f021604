// The box test of the radius graph on the host: protstruc_amd/csrc/radius_box.hpp, the code the kernels run,
// compiled with a plain C++ compiler (tests/test_radius_host.py).
//
//   c++ -std=c++17 -O2 -ffp-contract=off -I protstruc_amd/csrc tools/radius_box_host.cpp -o radius_box_host
//
// stdin, one case per line, every float32 as the decimal of its bit pattern:
//   cutoff nA nB   then 3 * nA coordinates of the queries, then 3 * nB coordinates of the candidates
// stdout, per case:  dropped (0 / 1)   the bits of G (0 where a box is empty)   the bits of the bound   A.n   B.n
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "radius_box.hpp"

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

static bool read_box(int n, ps_box& box) {
    box = ps_box_empty();
    for (int i = 0; i < n; ++i) {
        uint32_t p[3];
        if (scanf("%u %u %u", &p[0], &p[1], &p[2]) != 3) return false;
        box = ps_box_add(box, from_bits(p[0]), from_bits(p[1]), from_bits(p[2]));
    }
    return true;
}

int main() {
    uint32_t cutoff_bits;
    int na, nb;
    while (scanf("%u %d %d", &cutoff_bits, &na, &nb) == 3) {
        ps_box a, b;
        if (!read_box(na, a) || !read_box(nb, b)) return 1;
        const float cutoff = from_bits(cutoff_bits);
        const float bound = ps_radius_reject_above((double)cutoff * (double)cutoff);
        const bool drop = a.n == 0 || ps_box_dropped(a.lo, a.hi, b.lo, b.hi, b.n, bound);
        const float G = a.n && b.n ? ps_box_gap2(a.lo, a.hi, b.lo, b.hi) : 0.0f;
        printf("%d %u %u %d %d\n", drop ? 1 : 0, bits(G), bits(bound), a.n, b.n);
    }
    return 0;
}
