// ppls_po2_rowdiag.h -- launch interface of the PO2PLS row diagnostics kernel (ppls_po2_rowdiag.hip) behind
// ppls_po2_row_diagnostics{,_new} and ppls_po2_robust_weights: per row (x, y), orthonormal bases Qx (p x kx)
// of [W Wo] and Qy (q x ky) of [C Co], and two small dense matrices the host prepares,
//   a = Qx'x, b = Qy'y, odx2 = ||x - Qx a||^2, ody2 = ||y - Qy b||^2,
//   sd2 = ||Uc (a; b)||^2 with Sigma_c^-1 = Uc'Uc, Sigma_c the covariance of (a; b),
// and optionally the posterior means mu = (a; b)' Kmu of z = (t, to, u, uo).
//
// Determinism: every sum of a row is taken inside the one wave that owns the row, in an order fixed by p, q,
// kx, ky and the storage type alone (they pick the tiles and the rows per wave).  The row sums are
// ppls_rowdiag.hip's: a lane adds the 16-byte units lane, lane + 64, ... of the row in that order and the 64
// lane partials meet in a fixed six-level xor tree.  The dense part: lane i adds the k products of row i of
// Uc in the order j = 0 .. k - 1 to one accumulator, and the k squares meet in a fixed five-level tree over
// lanes 0 .. 31; column i of Kmu likewise in lane 32 + i.  Nothing is added across waves.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPLS_PO2_ROWDIAG_WAVES 4   // waves of a workgroup
// Rows a wave owns at a time (a power of two, rows x the wider tile <= 64): ppls_rowdiag.h's measured choices
// at the wider of the two tiles.
#define PPLS_PO2_ROWDIAG_ROWS8_SHORT 2
#define PPLS_PO2_ROWDIAG_ROWS8 4
#define PPLS_PO2_ROWDIAG_SHORT_BYTES 16384
#define PPLS_PO2_ROWDIAG_ROWS16 4
// The dense table: PPLS_PO2_ROWDIAG_KMAX rows of 64 doubles.  tab[j * 64 + i] = Uc[i][j] and
// tab[j * 64 + 32 + i] = Kmu[j][i] for i, j < k, zero elsewhere.
#define PPLS_PO2_ROWDIAG_KMAX 32
#define PPLS_PO2_ROWDIAG_TAB (PPLS_PO2_ROWDIAG_KMAX * 64)

extern "C" {
// The tile (8 or 16) of a block of kb columns, the rows a wave owns at a time, and the launch's workgroups.
int ppls_po2_rowdiag_tile(int kb);
int ppls_po2_rowdiag_rows_per_wave(int pa, int qb, int f32, int kx, int ky);
int ppls_po2_rowdiag_grid(int64_t nrows, int pa, int qb, int f32, int kx, int ky, int num_cus);

// The selected rows (rows = nullptr: rows 0 .. nrows-1; device indices, any order, repeats allowed) of X
// (lda elements per row, pa real columns; f32: floats, else doubles; rows are 16-byte multiples with zero
// padding) and Y likewise.  Qx: lda4 x kx column-major, lda4 = (pa + 3) & ~3, zero padding; Qy likewise with
// qb, ky.  tab: PPLS_PO2_ROWDIAG_TAB doubles as above.  Output i belongs to the i-th selected row: odx2, ody2,
// sd2 (nrows each) and, when mu is given, mu (ldmu x (kx + ky) column-major, ldmu >= nrows).
hipError_t ppls_launch_po2_rowdiag(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, int f32,
                                   const int64_t* rows, int64_t nrows, const double* Qx, int kx, const double* Qy,
                                   int ky, const double* tab, double* odx2, double* ody2, double* sd2, double* mu,
                                   int64_t ldmu, int grid, hipStream_t st);
}
