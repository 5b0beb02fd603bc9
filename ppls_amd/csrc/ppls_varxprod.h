// ppls_varxprod.h -- launch interface of ppls_varxprod.hip: the observed-information matrices of
// variances.PPLS_simult (Package/PPLS/R/EM_W_multi.R:838-857) for all components at once, read off the
// cross-products S where they lie (ppls_variances_xprod).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppls_math.h"

// For component i < a and the p x p diagonal block of S at (off, off) (S row-major P x P; g = its entry),
//   sse_i[a][b] = (ctt_i g[a][b] - x_ia k1_i w_ib - w_ia k1_i x_ib + w_ia k2_i w_ib) / s4 / N
//   J_i         = sse_i - bstar_i I       the observed information -(B_exp - SSt_exp)
//   sst_exp_i   = sse_i                   (nullable)
//   sst_star_i  = (x_ia - w_ia ctt_i)(x_ib - w_ib ctt_i) / s4   (nullable)
// x_i = cxt + i ldc (Cxt of component i), w_i = w + i ldw, p entries each.  Outputs: a consecutive
// column-major p x p matrices (batch stride p^2), each symmetric bit for bit.
struct PplsVarinfoArgs {
  const double* S;
  int P, off, p, a;   // P and off even, off + p <= P, 1 <= a <= PPLS_RMAX
  const double* cxt;
  int64_t ldc;
  const double* w;
  int64_t ldw;
  double ctt[PPLS_RMAX], k1[PPLS_RMAX], k2[PPLS_RMAX], bstar[PPLS_RMAX];
  double s4, N;
  double* J;
  double* sst_exp;
  double* sst_star;
};

extern "C" {
hipError_t ppls_launch_varinfo_batched(const PplsVarinfoArgs* a, hipStream_t st);
// The batch after its inverse: se[z p + j] = sqrt(M_z[j][j]) (NaN where negative, as R's sqrt) and, with
// mirror, the lower triangle of every M_z copied into the upper one (what the Cholesky inverse leaves).
hipError_t ppls_launch_varfinish_batched(double* M, int p, int a, int mirror, double* se, hipStream_t st);
}
