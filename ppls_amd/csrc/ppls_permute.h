// ppls_permute.h -- the row-permuted cross block C_pi = sum_i x_i y_pi(i)' on fp64 MFMA (ppls_permute.hip,
// DESIGN §22): the one block of S = [X Y_pi]'[X Y_pi] that a permutation of Y's rows against X's changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPLS_XPERM_PAD 32       // int32 entries behind the n row indices that the kernel may read (zeros)
#define PPLS_XPERM_MAXSPLIT 64  // row splits at most

extern "C" {

// Workgroups of the permuted cross-block kernel per compute unit (fp64 or fp32 storage).
int ppls_xperm_occupancy(int f32);
// Row splits over n rows: nsplit_req > 0 equal splits, 0 the guided schedule of ppls_gram_plan over the
// block's own quadrants.  bounds (may be NULL): nsplit + 1 row boundaries.  Returns the split count.
int ppls_xperm_plan(int p, int q, int64_t n, int wave_slots, int nsplit_req, int64_t* bounds);
// 64 x 64 quadrants of the p x q block, and the partials' length for nsplit splits.
int ppls_xperm_quads(int p, int q);
int64_t ppls_xperm_part_doubles(int p, int q, int nsplit);
// part[split][quadrant][64 x 64] = sum over the split's rows i of x_i y_perm[i]'.  perm: n row indices in
// [0, n) followed by PPLS_XPERM_PAD readable entries; bounds: nsplit + 1 device row boundaries.
hipError_t ppls_launch_xperm(const void* X, int ldx, int p, const void* Y, int ldy, int q, int f32, int64_t n,
                             const int32_t* perm, const int64_t* bounds, int nsplit, double* part, hipStream_t st);
// C (ldx x ldy column-major, the padding zero) = the splits' partials added in split order.
hipError_t ppls_launch_xperm_finish(const double* part, int nsplit, int p, int q, int ldx, int ldy, double* C,
                                    hipStream_t st);
// S (P x P column-major, P = ldx + ldy): S[a, ldx + b] = S[ldx + b, a] = C[a, b].
hipError_t ppls_launch_xperm_scatter(const double* C, int ldx, int ldy, double* S, hipStream_t st);

}  // extern "C"
