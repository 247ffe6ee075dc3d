/* sym3_eigen_host.cpp -- a stand-alone HOST program around threecrate_amd/csrc/sym3_eigen.h (test infrastructure): reads symmetric 3x3
 * matrices from standard input, six numbers a00 a01 a02 a11 a12 a22 per line, and prints per matrix one line of the sweeps used, the three
 * eigenvalues ascending and the nine eigenvector components (vector k at 3k .. 3k + 2), all with 17 significant digits.
 * tests/test_ground_cpu.py compiles it with the host compiler and compares it with numpy.linalg.eigh: no GPU is needed for the
 * numerically sharpest part of ground segmentation.
 * Build: g++ -std=c++17 -O2 -ffp-contract=off -Ithreecrate_amd/csrc tests/abi/sym3_eigen_host.cpp
 */
#include <cstdio>

#include "sym3_eigen.h"

int main() {
    double a[6];
    while (std::scanf("%lf %lf %lf %lf %lf %lf", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 6) {
        double w[3], v[9];
        const int sweeps = tc::sym3_eigen(a, w, v);
        std::printf("%d", sweeps);
        for (double x : w) std::printf(" %.17g", x);
        for (double x : v) std::printf(" %.17g", x);
        std::printf("\n");
    }
    return 0;
}
