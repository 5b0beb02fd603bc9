// ppls_xprod_meta.h -- launch interface of the cross-product form of one meta_PPLSi EM step
// (ppls_xprod_meta.hip).
//
// meta_EMstep splits the rows by population and takes X and Y as given, so every statistic of the
// step is a quadratic form in the population's own cross-products S_j = [X_j Y_j]'[X_j Y_j]: with the
// shared unit loadings w, c and M_j = S_j blockdiag(w, c) (P x 2),
//   X_j'mu_T = S_j,xx w alpha_j + S_j,xy c beta_j  = M_j[X rows] (alpha_j | beta_j)
//   Y_j'mu_U = S_j,yx w gamma_j + S_j,yy c delta_j = M_j[Y rows] (gamma_j | delta_j)
//   Gram([X_j w, Y_j c]) = blockdiag(w, c)' M_j
// The K matrices are those a stream opened with folds keeps (ppls_cvstream.h: a fold label is a
// population label), or the ones a resident context forms under option meta_xprod.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppls_math.h"

extern "C" {
// Whether the pass over K matrices of P x P doubles uses non-temporal loads: decided on all K 8 P^2
// bytes one step reads (the single-matrix kernel decides on its one matrix), against the same 200 MiB.
int ppls_xprod_meta_nt(int K, int P);

// Rows of S_j per wave of the rows kernel (rw_opt 1, 2, 4 or 8 forces it; 0 = auto).  The auto rule
// differs from the single-matrix kernel's (ppls_xprod_tile_rows): K matrices give K times the
// workgroups, and without a barrier per tile more rows per wave only add loads in flight.
int ppls_xprod_meta_rows(int K, int P, int rw_opt, int num_cus);

// The statistics blocks of all K populations (r = 1) in two launches.  S: K matrices, P x P row-major
// (P = ldx + ldy, the joint padded layout, exactly symmetric, padding 0), contiguous.  Wp (ldx), Cp
// (ldy): the shared loadings, 0 in the padding.  sc: K scalars.  Population j's block goes to
// stats + j part_ld: [X_j'mu_T (ldx) | Y_j'mu_U (ldy) | Gram 2 x 2 column-major, exactly symmetric]
// (PplsMetaStepArgs::stats).  M: K x 2 P doubles of scratch (M_j column-major at M + j 2 P).
// rw: rows of S_j per wave (1, 2, 4 or 8; ppls_xprod_meta_rows).  The rows kernel has the population
// as grid dimension y and reads every S_j once; the Gram kernel (3 entries x K workgroups) forms
// blockdiag(w, c)' M_j.  Every sum has a fixed order.  stop: both kernels exit if it is set (or nullptr).
hipError_t ppls_launch_xprod_meta(const double* S, int K, int ldx, int ldy, int rw, const double* Wp, const double* Cp,
                                  const PplsScalars* sc, double* stats, int64_t part_ld, double* M, const int* stop,
                                  hipStream_t st);
}
