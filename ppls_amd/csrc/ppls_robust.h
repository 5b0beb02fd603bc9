// ppls_robust.h -- launch interface of the weights and t log-likelihood kernel (ppls_robust.hip) behind
// ppls_robust_weights: the E-step of the multivariate-t PPLS model.  Input per row: the
// three doubles ppls_launch_rowdiag leaves (odx2, ody2, sd2); the rows themselves are not read again.
//   d2_i = (odx2_i / sigE^2 + ody2_i / sigF^2) + sd2_i     the order and the divisions of rowdiag_collect:
//                                                          the bits ppls_row_diagnostics reports
//   w_i  = (nu_keep + P) / (nu_keep + d2_i)                the E-step weight for one chosen nu
//   sums[j] = sum_i log1p(d2_i / nu_j), j < m <= 16;  sums[m] = sum_i w_i
//
// Determinism: a row block is PPLS_ROBUST_BLOCK rows; thread t of the workgroup that takes block b adds
// the rows b BLOCK + t, + 256, ... in that order, the 256 thread sums meet in a fixed xor tree (lanes,
// then the four waves as (0 + 1) + (2 + 3)), and the block partials are summed by one workgroup in the
// same way (thread t adds the partials t, t + 256, ...).  Workgroups take blocks by a grid stride, so
// which workgroup ran a block does not matter: the sums depend on n alone, bitwise, for any grid.  No
// atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPLS_ROBUST_BLOCK 1024   // rows per partial
#define PPLS_ROBUST_MAXNU 16
#define PPLS_ROBUST_SUMS (PPLS_ROBUST_MAXNU + 1)   // doubles per partial and in the result

struct PplsRobustNu {
  double nu[PPLS_ROBUST_MAXNU];
};

extern "C" {
int64_t ppls_robust_blocks(int64_t n);   // partials of n rows (>= 1)
int ppls_robust_grid(int64_t n, int num_cus);

// w, d2: n doubles each (d2 nullable); part: ppls_robust_blocks(n) * PPLS_ROBUST_SUMS doubles; sums:
// PPLS_ROBUST_SUMS doubles (entries m .. 15 are zero, entry 16 is sum w).  n = 0 writes zero sums.
// grid: workgroups of the row pass (>= 1; ppls_robust_grid's by default -- any value gives the same bits).
hipError_t ppls_launch_robust_weights(const double* odx2, const double* ody2, const double* sd2, int64_t n, double sE2,
                                      double sF2, const PplsRobustNu* nu, int m, int keep, double P, double* w,
                                      double* d2, double* part, double* sums, int grid, hipStream_t st);
}
