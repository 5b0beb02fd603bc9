// ppls_scale.h -- launch interface of the column centring / scaling kernels (ppls_scale.hip) behind
// ppls_scale_data: R's scale(x, center, scale) on the resident X and Y, in place.
//
// A matrix is rows of ld elements (f32: floats, else doubles; ld a 16-byte multiple, padding zero).
// A thread owns one 16-byte unit of the row (2 doubles / 4 floats) and walks the rows of its row
// block in order; a workgroup is tx x ty threads: tx consecutive units of ty row blocks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// Launch shape for an n x cols matrix: a function of n, cols, the storage type and num_cus only.
typedef struct {
  int units;         // 16-byte units of a row that hold real columns
  int ldc;           // columns those units hold (units * 2 or * 4): the stride of a row of partials
  int tx, ty;        // workgroup = tx x ty threads (tx * ty = 256)
  int grid_x;        // column tiles of tx units
  int grid_y;        // workgroups along the rows
  int64_t nblocks;   // row blocks (<= grid_y * ty): block b owns rows [b n / nblocks, (b + 1) n / nblocks)
} PplsScalePlan;

extern "C" {
PplsScalePlan ppls_scale_plan(int64_t n, int cols, int f32, int num_cus);

// part[b * ldc + j] = sum over the rows i of block b, in row order, of x_ij (sq = 0) or of
// (x_ij - centre[j])^2 (sq = 1; centre: ldc doubles).  nt: loads with the non-temporal policy.
hipError_t ppls_launch_col_partials(const void* X, int64_t ld, int64_t n, int f32, const PplsScalePlan* pl,
                                    const double* centre, int sq, int nt, double* part, hipStream_t st);
// out[j] = sum_b part[b * ldc + j] for j < cols, added in block order (bitwise repeatable).
hipError_t ppls_launch_col_reduce(const double* part, const PplsScalePlan* pl, int cols, double* out, hipStream_t st);
// x_ij <- (x_ij - centre[j]) / scale[j] for j < cols, in place (fp64 arithmetic, a true division; fp32
// storage: one rounding, at the store).  Columns >= cols of a row are neither read nor written.
hipError_t ppls_launch_col_apply(void* X, int64_t ld, int64_t n, int cols, int f32, const PplsScalePlan* pl,
                                 const double* centre, const double* scale, int nt, hipStream_t st);
}
