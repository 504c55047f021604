// Stand-alone host program around the Kabsch 3x3 solve of the kernel (protstruc_amd/csrc/kabsch_solve.hpp), so that the
// solve can be checked -- and, built by hand with -fsanitize=address,undefined, sanitized -- without a GPU:
//
//     c++ -std=c++17 -O2 -ffp-contract=off -I protstruc_amd/csrc tools/kabsch_solve_host.cpp -o kabsch_solve_host
//
// Reads covariances from standard input, nine numbers each (row-major H; "nan" and "inf" are accepted), and writes one
// line of nine numbers per covariance: the rotation R, row-major, with 17 significant digits.
// tests/test_align_host.py feeds it the covariances of the case builders of tests/align_ref.py.
#include <stdio.h>

#include "kabsch_solve.hpp"

int main() {
    double h[9], R[9];
    for (;;) {
        int got = 0;
        while (got < 9 && scanf("%lf", &h[got]) == 1) ++got;
        if (got == 0) return 0;
        if (got < 9) {
            fprintf(stderr, "kabsch_solve_host: %d numbers left over (a covariance has nine)\n", got);
            return 1;
        }
        ps_kabsch_solve(h, R);
        for (int i = 0; i < 9; ++i) printf("%.17g%c", R[i], i == 8 ? '\n' : ' ');
    }
}
