// ppls_cv.h -- launch interface of the cross-validation kernels (ppls_cv.hip): the device row
// gather behind ppls_set_data_from / ppls_xprod_downdate, the downdate S - S_out, and the
// prediction / held-out residual kernel family behind ppls_predict / ppls_heldout_sse
// (predict.PPLS and cv_PPLS, Package/PPLS/R/crossval_PPLS.R:12-52).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPLS_CV_WAVES 4   // waves of a scoring workgroup; each wave owns 64 / KT rows at a time

extern "C" {
// dst row i = src row rows[i] (i < nrows): copy16 16-byte units of every row, then zeros up to
// dst16 units (the destination's own padding).  Strides in 16-byte units; rows: device indices.
hipError_t ppls_launch_gather_rows(const void* src, int64_t src16, void* dst, int64_t dst16, int copy16,
                                   const int64_t* rows, int64_t nrows, hipStream_t st);

// out = a - b, elementwise over len doubles (len even; out may alias a).
hipError_t ppls_launch_downdate(const double* a, const double* b, double* out, int64_t len, hipStream_t st);

// Rows a scoring wave owns at a time for k components, and the launch's workgroups for nrows rows.
int ppls_cv_rows_per_wave(int k);
int ppls_cv_grid(int64_t nrows, int k, int num_cus);

// t_i = x_i A (k scores), then per row of the selected rows (rows = nullptr: rows 0 .. nrows-1)
//   pred == nullptr: the residuals y_i - sum_{m <= j} t_im s_m b_m for every prefix j = 1..k, their
//                    squares summed per wave into part[(workgroup * PPLS_CV_WAVES + wave) * k + j-1];
//   pred != nullptr: pred row i (ldo doubles, even) = sum_m t_im s_m b_m.
// X: rows of lda elements (f32: floats, else doubles; 16-byte multiples, padding zero); A: lda4 x k
// column-major with lda4 = (pa + 3) & ~3 and zero padding; Y / Bm likewise with q columns; s: k.
hipError_t ppls_launch_cv_score(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, int f32,
                                const int64_t* rows, int64_t nrows, const double* A, const double* Bm,
                                const double* s, int k, double* part, double* pred, int64_t ldo, int grid,
                                hipStream_t st);
// sse[j] = sum over the nparts wave partials, in index order (one workgroup; bitwise repeatable).
hipError_t ppls_launch_cv_sse_reduce(const double* part, int nparts, int k, double* sse, hipStream_t st);
}
