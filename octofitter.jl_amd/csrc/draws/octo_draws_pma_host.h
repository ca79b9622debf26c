// octo_draws_pma_host.h — the table algebra of the catalogue proper-motion anomaly (octo_draws_pma.hip; include/octofitter_hip_draws.h, "The
// eighteenth"), made once on the host by octo_draws_pma_set: from the catalogue covariance Σ [Q][Q] and the constant design H [Q][K] the matrices and
// constants the device applies per walker.
//   sampled     M = Σ⁻¹                                    c = −½·log det(2πΣ)
//   marginal    M = P_m = Σ⁻¹ − Σ⁻¹H·N⁻¹·HᵀΣ⁻¹, N = HᵀΣ⁻¹H    c = −½·log det(2πΣ) + (K/2)·log 2π − ½·log det N        G = N⁻¹HᵀΣ⁻¹ (γ̂ = G·r)
// by Cholesky factors: Σ = C·Cᵀ, Y = C⁻¹H, N = YᵀY = D·Dᵀ. Every matrix is stored at the fixed strides PMA_Q and PMA_K with zeros behind Q and K, so
// that the device runs its loops at the fixed sizes. Plain host C++ on <cmath> alone: it compiles and is tested by itself (tests/test_pma_layout.py).
#pragma once

#include <cmath>
#include <cstdint>

constexpr int PMA_Q = 8, PMA_K = 4;      // OCTO_DRAWS_PMA_MAX_Q, OCTO_DRAWS_PMA_MAX_K
constexpr double PMA_LOG2PI = 1.8378770664093454835606594728112;
// a pivot of a Cholesky factor must exceed this fraction of its diagonal entry: the pivot of the correlation form, 1 for a diagonal matrix
constexpr double PMA_PIVOT = 1e-12;

struct PmaTable {
    double M[2][PMA_Q * PMA_Q];      // [mode]: Σ⁻¹, P_m; symmetric
    double H[PMA_Q * PMA_K];         // [q][k]
    double G[PMA_K * PMA_Q];         // [k][q] N⁻¹HᵀΣ⁻¹
    double d[PMA_Q];
    double cst[2];                   // [mode]
    int32_t marg_ok;                 // K > 0 and N positive definite: the marginal mode's condition
};

// A = F·Fᵀ in place on the lower triangle of the n leading rows and columns (stride s); false: not positive definite. logdet = log det A.
inline bool pma_cholesky(double* A, int n, int s, double& logdet) {
    logdet = 0.0;
    for (int j = 0; j < n; ++j) {
        const double ajj = A[j * s + j];
        double x = ajj;
        for (int k = 0; k < j; ++k) x -= A[j * s + k] * A[j * s + k];
        if (!(ajj > 0.0) || !(x > PMA_PIVOT * ajj) || !std::isfinite(x)) return false;
        const double f = std::sqrt(x);
        A[j * s + j] = f;
        logdet += std::log(x);
        for (int i = j + 1; i < n; ++i) {
            double y = A[i * s + j];
            for (int k = 0; k < j; ++k) y -= A[i * s + k] * A[j * s + k];
            A[i * s + j] = y / f;
        }
    }
    return true;
}

// x := F⁻¹x (forward) for the m columns of x [n][sx], F lower with stride s
inline void pma_forward(const double* F, int n, int s, double* x, int m, int sx) {
    for (int c = 0; c < m; ++c)
        for (int i = 0; i < n; ++i) {
            double y = x[i * sx + c];
            for (int k = 0; k < i; ++k) y -= F[i * s + k] * x[k * sx + c];
            x[i * sx + c] = y / F[i * s + i];
        }
}
// x := F⁻ᵀx (backward)
inline void pma_backward(const double* F, int n, int s, double* x, int m, int sx) {
    for (int c = 0; c < m; ++c)
        for (int i = n - 1; i >= 0; --i) {
            double y = x[i * sx + c];
            for (int k = i + 1; k < n; ++k) y -= F[k * s + i] * x[k * sx + c];
            x[i * sx + c] = y / F[i * s + i];
        }
}

// The table of (cov [Q][Q], H [Q][K] or null with K = 0, d [Q]). 0: made · 1: Σ is not symmetric (beyond 1e-12·√(Σ_ii Σ_jj)) · 2: Σ is not positive
// definite. A rank-deficient H is no error: marg_ok = 0.
inline int pma_table_build(const double* cov, const double* H, const double* d, int Q, int K, PmaTable* out) {
    *out = PmaTable{};
    double C[PMA_Q * PMA_Q] = {};
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j <= i; ++j) {
            const double a = cov[i * Q + j], b = cov[j * Q + i];
            if (!(std::fabs(a - b) <= 1e-12 * std::sqrt(std::fabs(cov[i * Q + i] * cov[j * Q + j])))) return 1;
            C[i * PMA_Q + j] = a;
        }
    double logdet = 0.0;
    if (!pma_cholesky(C, Q, PMA_Q, logdet)) return 2;
    // Σ⁻¹ = C⁻ᵀC⁻¹: the columns of the identity through both solves
    double Si[PMA_Q * PMA_Q] = {};
    for (int i = 0; i < Q; ++i) Si[i * PMA_Q + i] = 1.0;
    pma_forward(C, Q, PMA_Q, Si, Q, PMA_Q);
    pma_backward(C, Q, PMA_Q, Si, Q, PMA_Q);
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j <= i; ++j) {
            const double x = 0.5 * (Si[i * PMA_Q + j] + Si[j * PMA_Q + i]);
            out->M[0][i * PMA_Q + j] = out->M[0][j * PMA_Q + i] = x;
        }
    out->cst[0] = -0.5 * ((double)Q * PMA_LOG2PI + logdet);
    for (int q = 0; q < Q; ++q) {
        out->d[q] = d[q];
        for (int k = 0; k < K; ++k) out->H[q * PMA_K + k] = H[q * K + k];
    }
    if (K == 0) return 0;
    // Y = C⁻¹H, N = YᵀY
    double Y[PMA_Q * PMA_K] = {}, N[PMA_K * PMA_K] = {};
    for (int i = 0; i < Q * PMA_K; ++i) Y[i] = out->H[i];
    pma_forward(C, Q, PMA_Q, Y, K, PMA_K);
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) {
            double x = 0.0;
            for (int q = 0; q < Q; ++q) x += Y[q * PMA_K + i] * Y[q * PMA_K + j];
            N[i * PMA_K + j] = x;
        }
    double logdetN = 0.0;
    if (!pma_cholesky(N, K, PMA_K, logdetN)) return 0;      // marg_ok stays 0
    // Σ⁻¹H = C⁻ᵀY [Q][K]; Gᵀ = Σ⁻¹H·N⁻¹ row by row: N⁻¹ applied to each row of Σ⁻¹H
    double SH[PMA_Q * PMA_K];
    for (int i = 0; i < PMA_Q * PMA_K; ++i) SH[i] = Y[i];
    pma_backward(C, Q, PMA_Q, SH, K, PMA_K);
    for (int q = 0; q < Q; ++q) {
        double x[PMA_K] = {};
        for (int k = 0; k < K; ++k) x[k] = SH[q * PMA_K + k];
        pma_forward(N, K, PMA_K, x, 1, 1);
        pma_backward(N, K, PMA_K, x, 1, 1);
        for (int k = 0; k < K; ++k) out->G[k * PMA_Q + q] = x[k];
    }
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j <= i; ++j) {
            double x = 0.0, y = 0.0;      // (Σ⁻¹H·G)[i][j] and its transpose: P_m is symmetric
            for (int k = 0; k < K; ++k) {
                x += SH[i * PMA_K + k] * out->G[k * PMA_Q + j];
                y += SH[j * PMA_K + k] * out->G[k * PMA_Q + i];
            }
            out->M[1][i * PMA_Q + j] = out->M[1][j * PMA_Q + i] = out->M[0][i * PMA_Q + j] - 0.5 * (x + y);
        }
    out->cst[1] = out->cst[0] + 0.5 * (double)K * PMA_LOG2PI - 0.5 * logdetN;
    out->marg_ok = 1;
    return 0;
}
