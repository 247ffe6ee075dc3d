// sym3_eigen.h -- the symmetric 3x3 eigen-problem in f64, for host and device alike (ground.hip's plane fits; tests/test_ground_cpu.py
// compiles a stand-alone host program around it and holds it to numpy.linalg.eigh).
//   Cyclic Jacobi: sweeps over the pairs (0,1), (0,2), (1,2), each rotation annihilating one off-diagonal entry.  There is no
// characteristic polynomial and so no branch on a degenerate discriminant: equal eigenvalues, a zero matrix and a diagonal matrix all take
// the same road (they simply need no rotation).  The sweep limit is fixed; a 3x3 matrix converges quadratically and is diagonal to the last
// bit after five to eight sweeps.  An off-diagonal entry that no longer changes either of its diagonal neighbours when added to them
// a hundredfold is set to zero, which is what ends the iteration in finitely many steps.
//   Plain C++ without a library call other than sqrt and fabs; no FMA is asked for (the units that include it are built without contraction).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TC_SYM3_HD __host__ __device__
#else
#define TC_SYM3_HD
#endif

namespace tc {

constexpr int kSym3MaxSweeps = 24;

// a = {a00, a01, a02, a11, a12, a22}.  w: the eigenvalues ascending; v[3 * k + 0..2]: the unit eigenvector of w[k].  Returns the sweeps used.
// Entries that are not finite give values that are not finite and no fault.
TC_SYM3_HD inline int sym3_eigen(const double a[6], double w[3], double v[9]) {
    double m[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
    double e[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};      // columns: the eigenvectors so far
    int sweeps = 0;
    for (; sweeps < kSym3MaxSweeps; ++sweeps) {
        const double off = fabs(m[0][1]) + fabs(m[0][2]) + fabs(m[1][2]);
        if (!(off > 0.0)) break;                                // diagonal (or not a number: no rotation would help)
        for (int p = 0; p < 2; ++p) {
            for (int q = p + 1; q < 3; ++q) {
                const double apq = m[p][q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq);
                if (fabs(m[p][p]) + g == fabs(m[p][p]) && fabs(m[q][q]) + g == fabs(m[q][q])) {
                    m[p][q] = m[q][p] = 0.0;
                    continue;
                }
                const double theta = (m[q][q] - m[p][p]) / (2.0 * apq);
                // the smaller root of t^2 + 2 theta t - 1 = 0; theta^2 overflowing to infinity gives t = 0, the right limit
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                const int r = 3 - p - q;                        // the third index
                const double arp = m[r][p], arq = m[r][q];
                m[p][p] = m[p][p] - t * apq;
                m[q][q] = m[q][q] + t * apq;
                m[p][q] = m[q][p] = 0.0;
                m[r][p] = m[p][r] = c * arp - s * arq;
                m[r][q] = m[q][r] = s * arp + c * arq;
                for (int k = 0; k < 3; ++k) {
                    const double ekp = e[k][p], ekq = e[k][q];
                    e[k][p] = c * ekp - s * ekq;
                    e[k][q] = s * ekp + c * ekq;
                }
            }
        }
    }
    int o0 = 0, o1 = 1, o2 = 2;                                 // ascending order of the diagonal, a three-element sorting network
    if (m[o1][o1] < m[o0][o0]) { const int x = o0; o0 = o1; o1 = x; }
    if (m[o2][o2] < m[o1][o1]) { const int x = o1; o1 = o2; o2 = x; }
    if (m[o1][o1] < m[o0][o0]) { const int x = o0; o0 = o1; o1 = x; }
    const int order[3] = {o0, o1, o2};
    for (int k = 0; k < 3; ++k) {
        const int c = order[k];
        w[k] = m[c][c];
        const double x = e[0][c], y = e[1][c], z = e[2][c];
        const double len = sqrt(x * x + y * y + z * z);          // the product of rotations is orthogonal to a few ulp: renormalised
        const double inv = len > 0.0 ? 1.0 / len : 1.0;
        v[3 * k] = x * inv; v[3 * k + 1] = y * inv; v[3 * k + 2] = z * inv;
    }
    return sweeps;
}

}  // namespace tc
