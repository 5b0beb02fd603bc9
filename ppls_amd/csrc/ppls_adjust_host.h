// ppls_adjust_host.h -- the host side of the covariate adjustment: fixed-order Grams of the design's
// rows, the Cholesky factor with lm.fit's pivot rule, and the triangular solves of Cholesky-QR2.
// Plain C++ (no HIP): ppls_capi.cpp uses it, and a stand-alone program can.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// lm.fit's tol: a column whose norm after the earlier columns were taken out is at most this share
// of its own norm is aliased.
constexpr double PPLS_ADJ_TOL = 1e-7;

// G = A'A of the n x k row-major A (k x k row-major, both triangles), every sum in row order.
inline void ppls_adj_gram(const double* A, int64_t n, int k, double* G) {
  for (int a = 0; a < k * k; ++a) G[a] = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const double* r = A + i * k;
    for (int a = 0; a < k; ++a)
      for (int b = 0; b <= a; ++b) G[a * k + b] += r[a] * r[b];
  }
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < a; ++b) G[b * k + a] = G[a * k + b];
}

// Cholesky G = L L' (L lower, k x k row-major; its upper triangle is zeroed).  A pivot L_jj that is
// not > tol is refused: returns the 1-based column, 0 when every pivot passed.
inline int ppls_adj_chol(const double* G, int k, double tol, double* L) {
  for (int a = 0; a < k * k; ++a) L[a] = 0.0;
  for (int j = 0; j < k; ++j) {
    double d = G[j * k + j];
    for (int m = 0; m < j; ++m) d -= L[j * k + m] * L[j * k + m];
    if (!(d > tol * tol) || !std::isfinite(d)) return j + 1;
    const double l = std::sqrt(d);
    L[j * k + j] = l;
    for (int i = j + 1; i < k; ++i) {
      double s = G[i * k + j];
      for (int m = 0; m < j; ++m) s -= L[i * k + m] * L[j * k + m];
      L[i * k + j] = s / l;
    }
  }
  return 0;
}

// A <- A L^-T, row by row (forward substitution): the Q of A = Q L'.
inline void ppls_adj_solve_rows(double* A, int64_t n, int k, const double* L) {
  for (int64_t i = 0; i < n; ++i) {
    double* r = A + i * k;
    for (int j = 0; j < k; ++j) {
      double s = r[j];
      for (int m = 0; m < j; ++m) s -= r[m] * L[j * k + m];
      r[j] = s / L[j * k + j];
    }
  }
}

// B <- L^-T B for the k x m row-major B (back substitution with the upper triangular L').
inline void ppls_adj_backsolve(const double* L, int k, double* B, int64_t m) {
  for (int j = k - 1; j >= 0; --j) {
    double* bj = B + (int64_t)j * m;
    for (int i = j + 1; i < k; ++i) {
      const double l = L[i * k + j];
      const double* bi = B + (int64_t)i * m;
      for (int64_t c = 0; c < m; ++c) bj[c] -= l * bi[c];
    }
    const double d = L[j * k + j];
    for (int64_t c = 0; c < m; ++c) bj[c] /= d;
  }
}

// B <- L^-1 B for the k x m row-major B (forward substitution).
inline void ppls_adj_fwdsolve(const double* L, int k, double* B, int64_t m) {
  for (int j = 0; j < k; ++j) {
    double* bj = B + (int64_t)j * m;
    for (int i = 0; i < j; ++i) {
      const double l = L[j * k + i];
      const double* bi = B + (int64_t)i * m;
      for (int64_t c = 0; c < m; ++c) bj[c] -= l * bi[c];
    }
    const double d = L[j * k + j];
    for (int64_t c = 0; c < m; ++c) bj[c] /= d;
  }
}
