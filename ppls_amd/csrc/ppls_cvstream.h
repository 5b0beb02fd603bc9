// ppls_cvstream.h -- launch interface of the kernels behind cross-validation on streamed data
// (ppls_cvstream.hip): a stream opened with folds keeps one cross-product matrix S_k per
// fold (P x P row-major, the joint padded layout of ppls_stream.h, exactly symmetric, padding 0), all
// K contiguous.  The finish recentres them to the global mean and standardises them, a selection sums
// folds into the working S, and the held-out error of a fit is a quadratic form in the fold's S_k.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPLS_CVS_KMAX 16   // components of ppls_launch_cvs_heldout (= PPLS_RMAX, ppls_heldout_sse's limit)

extern "C" {
// dsum_j = sum_k (S_k,jj + (w_k e_kj) e_kj), added in fold order, for j < P (0 in the padding).
// S: K matrices of P x P; e: K x P (fold mean - global mean, joint layout); w: K (the folds' rows).
// The term is formed exactly as ppls_launch_cvs_finish forms it.
hipError_t ppls_launch_cvs_diag(const double* S, int K, int p, int ldx, int q, int ldy, const double* e,
                                const double* w, double* dsum, hipStream_t st);

// Recentre to the global mean and standardise in one pass over every fold matrix:
//   S_k,ij <- (S_k,ij + (w_k e_ki) e_kj) / (d_i d_j)        (d: P doubles, 1 where nothing is scaled)
// over the 64 x 64 blocks of the lower triangle (blockIdx.y = fold), 16-byte accesses, the mirror
// block written from an LDS copy, padding written 0: 16 P^2 bytes per fold.
hipError_t ppls_launch_cvs_finish(double* S, int K, int p, int ldx, int q, int ldy, const double* e,
                                  const double* w, const double* d, hipStream_t st);

// out = sum of the fold matrices l != skip, added in fold order (skip = -1: all of them).  K reads and
// one write of P^2 doubles; the sum of exactly symmetric matrices in one order is exactly symmetric.
hipError_t ppls_launch_cvs_select(const double* S, int K, int skip, int64_t PP, double* out, hipStream_t st);

// The held-out error of a fit from one fold's cross-products Sk.  W: ((p + 3) & ~3) x k column-major,
// zero padded; C likewise with q rows; B: k.  work: 4 p k doubles.  With A = W' S_xx W, D_m = w_m' S_xy c_m,
// G = C'C, for every prefix j = 1..k
//   sse[j-1] = tr(S_yy) - 2 sum_{m<=j} b_m D_m + sum_{m,l<=j} b_m b_l A_ml G_ml
// and mag[j-1] the same sum with every elementary product replaced by its absolute value.  One read of
// the X rows of Sk; every sum has a fixed order.
hipError_t ppls_launch_cvs_heldout(const double* Sk, int p, int ldx, int q, int ldy, const double* W, const double* C,
                                   const double* B, int k, double* work, double* sse, double* mag, hipStream_t st);
}
