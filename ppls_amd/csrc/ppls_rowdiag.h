// ppls_rowdiag.h -- launch interface of the row diagnostics kernel (ppls_rowdiag.hip) behind
// ppls_row_diagnostics / ppls_row_diagnostics_new: per row (x, y) and a fit with orthonormal W, C
//   a = W'x, b = C'y, odx2 = ||x - W a||^2, ody2 = ||y - C b||^2,
//   sd2 = sum_k (s22_k a_k^2 - 2 s12_k a_k b_k + s11_k b_k^2) / det_k,
// and optionally Expect_M's posterior means mu_T = a alpha + b beta, mu_U = a gamma + b delta.
// odx2 / sigE^2 + ody2 / sigF^2 + sd2 is the row's summand of loglC_fast's traceL.
//
// Determinism: every sum of a row is taken inside the one wave that owns the row, in an order fixed
// by p, q, the component tile (k <= 8 or k <= 16) and the storage type alone (they pick the
// rows per wave, ppls_rowdiag_rows_per_wave) -- a lane adds the
// 16-byte units lane, lane + 64, ... of the row in that order, the 64 lane partials meet in a fixed
// six-level xor tree that is the same for every slot of the wave's row group, and the k terms of sd2
// in a fixed tree over the tile.  So a row's outputs are bitwise the same whatever the other rows of
// the call, the subset, the grid, the shard or the row stride: nothing is added across waves.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPLS_ROWDIAG_WAVES 4   // waves of a workgroup
// Rows a wave owns at a time (a power of two, rows x tile <= 64), measured choices: for
// k <= 8 two rows while the longer row of a block is at most 16 KB (C3's), four beyond; for k <= 16 four.
#ifndef PPLS_ROWDIAG_ROWS8_SHORT
#define PPLS_ROWDIAG_ROWS8_SHORT 2
#endif
#ifndef PPLS_ROWDIAG_ROWS8
#define PPLS_ROWDIAG_ROWS8 4
#endif
#define PPLS_ROWDIAG_SHORT_BYTES 16384
#ifndef PPLS_ROWDIAG_ROWS16
#define PPLS_ROWDIAG_ROWS16 4
#endif
#define PPLS_ROWDIAG_COEF 8    // per component: s11, s12, s22, det, alpha, beta, gamma, delta

extern "C" {
// Rows a wave owns at a time for pa, qb columns of a storage type and k components, and the launch's
// workgroups for nrows rows.
int ppls_rowdiag_rows_per_wave(int pa, int qb, int f32, int k);
int ppls_rowdiag_grid(int64_t nrows, int pa, int qb, int f32, int k, int num_cus);

// The selected rows (rows = nullptr: rows 0 .. nrows-1; device indices, any order, repeats allowed)
// of X (lda elements per row, pa real columns; f32: floats, else doubles; rows are 16-byte multiples
// with zero padding) and Y likewise.  W: lda4 x k column-major, lda4 = (pa + 3) & ~3, zero padding;
// C likewise with qb.  coef: PPLS_ROWDIAG_COEF x 16 doubles, coef[j * 16 + m] for component m.
// Output i belongs to the i-th selected row: odx2, ody2, sd2 (nrows each) and, when mu_T is given,
// mu_T and mu_U (ldmu x k column-major, ldmu >= nrows; both or neither).
hipError_t ppls_launch_rowdiag(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, int f32,
                               const int64_t* rows, int64_t nrows, const double* W, const double* C,
                               const double* coef, int k, double* odx2, double* ody2, double* sd2, double* mu_T,
                               double* mu_U, int64_t ldmu, int grid, hipStream_t st);
}
