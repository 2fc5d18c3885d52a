// sym_eig.h -- host only: the symmetric eigendecomposition behind the batched Exact propagation (propagate_api.hip).
// A quadratic form z^T M z of a symmetric d x d matrix (d <= 64) becomes a signed sum of squares of d transformed coordinates:
//   M = V diag(lam) V^T,  T_km = sqrt|lam_k| V_mk,  s_k = sign(lam_k)   =>   z^T M z = sum_k s_k ((T z)_k)^2
// so that a kernel pays O(d) per pair instead of O(d^2) whether M is diagonal or full, and keeps the sign of every direction (M need not be
// positive semi-definite).  Plain C++: no HIP, no allocation beyond the vectors it is given.
#pragma once
#include <math.h>

#include <vector>

// cyclic Jacobi in fp64 on the symmetric part of M [d, d] (row-major): lam [d], V [d, d] with the eigenvectors as COLUMNS.  A diagonal M
// needs no rotation and comes back as it is (V = I).  Ends when the off-diagonal mass is below 1e-32 of the matrix's, at most 64 sweeps.
static inline void sym_eig_jacobi(const double *M, int d, std::vector<double> &lam, std::vector<double> &V)
{
    std::vector<double> A((size_t)d * d);
    V.assign((size_t)d * d, 0.0);
    lam.assign(d, 0.0);
    double fro = 0.0;
    for (int i = 0; i < d; ++i) {
        V[(size_t)i * d + i] = 1.0;
        for (int j = 0; j < d; ++j) {
            A[(size_t)i * d + j] = 0.5 * (M[i * d + j] + M[j * d + i]);
            fro += A[(size_t)i * d + j] * A[(size_t)i * d + j];
        }
    }
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q) off += 2.0 * A[(size_t)p * d + q] * A[(size_t)p * d + q];
        if (!(off > 1e-32 * fro)) break;
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q) {
                const double apq = A[(size_t)p * d + q];
                if (apq == 0.0) continue;
                const double tau = (A[(size_t)q * d + q] - A[(size_t)p * d + p]) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < d; ++k) {   // columns p, q of A and of V
                    const double akp = A[(size_t)k * d + p], akq = A[(size_t)k * d + q];
                    A[(size_t)k * d + p] = c * akp - s * akq;
                    A[(size_t)k * d + q] = s * akp + c * akq;
                    const double vkp = V[(size_t)k * d + p], vkq = V[(size_t)k * d + q];
                    V[(size_t)k * d + p] = c * vkp - s * vkq;
                    V[(size_t)k * d + q] = s * vkp + c * vkq;
                }
                for (int k = 0; k < d; ++k) {   // rows p, q of A
                    const double apk = A[(size_t)p * d + k], aqk = A[(size_t)q * d + k];
                    A[(size_t)p * d + k] = c * apk - s * aqk;
                    A[(size_t)q * d + k] = s * apk + c * aqk;
                }
                A[(size_t)p * d + q] = 0.0;
                A[(size_t)q * d + p] = 0.0;
            }
    }
    for (int k = 0; k < d; ++k) lam[k] = A[(size_t)k * d + k];
}

// T [d, d] (row k = sqrt|lam_k| times eigenvector k) and sgn [d] (+1, -1, or 0 for a zero eigenvalue) of scale * sym(M)
static inline void sym_square_transform(const double *M, int d, double scale, double *T, double *sgn)
{
    std::vector<double> S((size_t)d * d), lam, V;
    for (int i = 0; i < d * d; ++i) S[i] = scale * M[i];
    sym_eig_jacobi(S.data(), d, lam, V);
    for (int k = 0; k < d; ++k) {
        const double r = sqrt(fabs(lam[k]));
        sgn[k] = lam[k] > 0.0 ? 1.0 : (lam[k] < 0.0 ? -1.0 : 0.0);
        for (int m = 0; m < d; ++m) T[(size_t)k * d + m] = r * V[(size_t)m * d + k];
    }
}
