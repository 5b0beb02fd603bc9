// ppls_stream.h -- launch interface of the streamed-data kernels (ppls_stream.hip) behind
// ppls_stream_begin / _rows / _end: the cross-products S = [X Y]'[X Y] of centred (and scaled) data
// accumulated from row chunks, with no rows resident.
//
// S is P x P row-major (P = ldx + ldy, the joint padded layout of ppls_xprod.h: X's p real columns at
// [0, p), Y's q at [ldx, ldx + q), zero padding elsewhere) and exactly symmetric.  Both S kernels walk
// the 64 x 64 blocks of the lower triangle, one workgroup each, with 16-byte accesses, and write every
// block's mirror image from an LDS copy, so symmetry holds bit for bit; padding entries are written 0.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// Per chunk of nc rows, after the chunk's column sums (joint layout, P doubles):
//   mc_j = sum_j / nc (0 in the padding), delta_j = mc_j - mean_j, mean_j += delta_j nc / (N + nc)
// with N the rows merged before this chunk.
hipError_t ppls_launch_stream_mean(const double* sum, int P, int p, int ldx, int q, double nc, double N, double* mc,
                                   double* delta, double* mean, hipStream_t st);

// The Gram's finish step fused with the pairwise (Chan) merge: for every live entry of the lower
// triangle, in this fixed order,
//   S_ij <- ((S_ij + part_0 + part_1 + ... + part_{nsplit-1}) + (w delta_i) delta_j)
// with part the per-split quadrant partials of ppls_launch_gram_joint (ppls_gram_part_doubles layout).
// nsplit = 0 (part may be null): the rank-1 term only (the cross-rank merge).  delta = null: no rank-1
// term (uncentred streams).  One read and one write of S: 16 P^2 bytes plus the partials.
hipError_t ppls_launch_stream_merge(double* S, int p, int ldx, int q, int ldy, const double* part, int nsplit,
                                    const double* delta, double w, hipStream_t st);

// S_ij <- S_ij / (d_i d_j) over the live entries (d: P doubles, joint layout; staged in LDS), the
// lower triangle computed and mirrored; the padding stays 0.
hipError_t ppls_launch_stream_standardise(double* S, int p, int ldx, int q, int ldy, const double* d, hipStream_t st);
}
