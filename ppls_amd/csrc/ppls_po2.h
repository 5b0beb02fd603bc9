// ppls_po2.h -- launch interface of the PO2PLS iteration from the cross-products S (ppls_po2.hip,
// DESIGN.md §26).
//
// The model adds X- and Y-specific components to PPLS_simult's (the reference's simulC / loglC /
// EMstepC, Package/PPLS/src/loglC.cpp:268-315, :36-113, :116-250):
//   x = W t + Wo to + e,  y = C u + Co uo + f,  u = B t + h.
// With G = blockdiag(Gx, Gy), Gx = [W Wo] (kx = r + rx columns), Gy = [C Co] (ky = r + ry), every
// statistic of an EM step is a quadratic form in S = [X Y]'[X Y]: M = S G (P x k, k = kx + ky),
// Q = G'M (k x k) and the diagonal blocks of G'G, then k x k algebra.  The latent vector is ordered
// z = (t, to | u, uo).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppls_math.h"

#define PPLS_PO2_KMAX (2 * PPLS_RMAX)
#define PPLS_PO2_BATCH_MAX 256   // models of one batched iteration

// The scalars of theta (standard deviations, as in ppls_theta).
struct PplsPo2Scalars {
  double b[PPLS_RMAX], sT[PPLS_RMAX], sTo[PPLS_RMAX], sUo[PPLS_RMAX];
  double sE, sF, sH, pad0;
};

// What the small kernel leaves behind (device memory; every matrix column-major with ld k, r or as noted).
struct PplsPo2Small {
  double Czz[PPLS_PO2_KMAX * PPLS_PO2_KMAX];   // posterior second moments of z, k x k
  double K[PPLS_PO2_KMAX * PPLS_PO2_KMAX];     // D Lambda^-1, k x k: C_dz = M K / N
  double Chh[PPLS_RMAX * PPLS_RMAX];           // r x r
  double Cee, Cff, loglik, logdetL;
};

// Status words the kernels leave in *status (0 = fine); the first failure stays.
#define PPLS_PO2_ST_SIGMA (-21)    // a sigma of theta is non-positive or non-finite
#define PPLS_PO2_ST_LAMBDA (-22)   // Lambda is not positive definite
#define PPLS_PO2_ST_VAR (-23)      // an updated variance is non-positive or non-finite
#define PPLS_PO2_ST_RANK (-24)     // a loading update is rank deficient

struct PplsPo2Args {
  const double* S;   // P x P, P = ldx + ldy
  int ldx, ldy, p, q, r, rx, ry;
  int type;          // orth of the loading update: PPLS_ORTH_SVD (0) the polar factor, PPLS_ORTH_QR (1)
  double* Gx;        // kx columns of ldx: W then Wo (padding rows zero)
  double* Gy;        // ky columns of ldy: C then Co
  PplsPo2Scalars* sc;
  double* M;         // the X part of M = S G: P x kx, column-major, ld P
  double* My;        // the Y part: P x ky, ld P.  One model alone: M + kx P (M is then P x k).  In a batch both lie
                     // inside the batch's shared P x sum kx and P x sum ky buffers
  double* Q;         // k x k
  double* GGx;       // kx x kx
  double* GGy;       // ky x ky
  PplsPo2Small* sm;
  double* Z;         // scratch of the loading update: 16 (ldx + ldy) doubles
  double* loglik;    // the history (device)
  int* stop;         // 2 ints: {pass the stop rule fired at, 1 if its increment was NaN}; may be NULL
  int* stop_mirror;  // host-mapped mirror of stop[0]; may be NULL
  int* status;
  double N, ssqX, ssqY, atol;
};

extern "C" {

// One panel of M = S G: Mout (P x R, ld P) = S[:, soff : soff + width] B, B = R columns of ldb.  One
// read of the panel's columns of S; rw rows of S per wave as ppls_xprod_tile_rows chooses; non-temporal
// loads when S is larger than the Infinity Cache (the same rule as ppls_launch_xprod_tile).
hipError_t ppls_launch_po2_panel(const double* S, int P, int soff, int width, const double* B, int ldb, int R, int rw,
                                 double* Mout, const int* stop, hipStream_t st);
// Whether the panel launch takes the non-temporal instantiation for this P.
int ppls_po2_panel_nt(int P);

// Q = G'M and the diagonal blocks of G'G: one workgroup per upper-triangle entry, fixed-order sums, mirrored.
hipError_t ppls_launch_po2_gram(const PplsPo2Args* a, hipStream_t st);

// The k x k algebra of pass number `pass` (1-based) at the theta the pass used: moments, log-likelihood
// into loglik[pass - 1], then by mode
//   0  nothing more (E-step / log-likelihood alone);
//   1  the stop rule (pass >= 2, check != 0: loglik[pass - 1] - loglik[pass - 2] < atol sets *stop = pass)
//      and, when it does not fire, the new scalars into *sc.
hipError_t ppls_launch_po2_small(const PplsPo2Args* a, int pass, int mode, int check, hipStream_t st);

// The ECM loading updates from M, K and Czz (one workgroup per side; W then Wo, C then Co), orth by a->type.
hipError_t ppls_launch_po2_update(const PplsPo2Args* a, hipStream_t st);

// The same three kernel bodies over a batch of m models: args is a DEVICE array of m
// PplsPo2Args, workgroup row blockIdx.y serves args[blockIdx.y].  Every model has its own stop pair, status,
// scalars, moments and history; a model whose stop[0] is set returns at once in all three.  The Gram's grid is
// (max_entries, m), max_entries = the largest k(k+1)/2 + kx(kx+1)/2 + ky(ky+1)/2 of the batch; workgroups past
// a model's own count return.  pass, mode, check: as ppls_launch_po2_small, the same for every model.
hipError_t ppls_launch_po2_gram_batch(const PplsPo2Args* args, int m, int max_entries, hipStream_t st);
hipError_t ppls_launch_po2_small_batch(const PplsPo2Args* args, int m, int pass, int mode, int check, hipStream_t st);
hipError_t ppls_launch_po2_update_batch(const PplsPo2Args* args, int m, hipStream_t st);

}
