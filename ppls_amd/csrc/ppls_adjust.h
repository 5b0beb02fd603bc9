// ppls_adjust.h -- launch interface of the covariate-adjustment kernels (ppls_adjust.hip) behind
// ppls_adjust_data (the resident X, Y residualised on an orthonormal design Q, in place) and
// ppls_xprod_adjust (the k trailing columns of a cross-product matrix partialled out of the rest).
//
// The row passes take ppls_scale.h's launch shape: a matrix is rows of ld elements, a thread owns one
// 16-byte unit of the row and walks the rows of its row block in order.  Q is n x KT doubles, row-major,
// KT in {4, 8, 16}: the design's k1 orthonormal columns, zero in the KT - k1 padding slots.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppls_scale.h"

constexpr int PPLS_ADJ_KMAX = 16;   // design columns (and partialled-out columns) at most

// The tile for k1 design columns: 4, 8 or 16 (0: k1 outside [1, 16]).
inline int ppls_adjust_kt(int k1) { return k1 < 1 || k1 > PPLS_ADJ_KMAX ? 0 : k1 <= 4 ? 4 : k1 <= 8 ? 8 : 16; }

extern "C" {
// part[(b * KT + a) * ldc + j] = sum over the rows i of block b, in row order, of q_ia x_ij as one
// fma chain per (a, j) in fp64.  part: nblocks * KT * ldc doubles.  nt: non-temporal loads of X.
hipError_t ppls_launch_adjust_partials(const void* X, int64_t ld, int64_t n, int f32, const PplsScalePlan* pl,
                                       const double* Q, int kt, int nt, double* part, hipStream_t st);
// G[a * ldc + j] = sum_b part[(b * KT + a) * ldc + j], added in block order (bitwise repeatable).
hipError_t ppls_launch_adjust_reduce(const double* part, const PplsScalePlan* pl, int kt, double* G, hipStream_t st);
// x_ij <- x_ij - sum_a q_ia g_aj for j < cols, in place: acc = x_ij, then acc = fma(-q_ia, g_aj, acc)
// for a ascending (fp32 storage: one rounding, at the store).  G: KT rows of ldg >= ldc doubles, this
// matrix's columns from G[0].  Columns >= cols of a row are neither read nor written.
hipError_t ppls_launch_adjust_apply(void* X, int64_t ld, int64_t n, int cols, int f32, const PplsScalePlan* pl,
                                    const double* Q, const double* G, int64_t ldg, int kt, int nt, hipStream_t st);

// dst_ij = src_ij - sum_a F_ia F_ja (a ascending, one fma chain from src_ij) over the live entries of
// dst's joint layout (X's p columns at [0, p), Y's q at [ldx, ldx + q), P_dst = ldx + ldy_dst even);
// src is row-major with row stride P_src >= P_dst and shares ldx, so a live column has the same index
// in both.  F: 16 x P_dst doubles, row-major (row a = component a over dst's joint columns, 0 beyond k).  One workgroup per 64 x 64
// block of dst's lower triangle; the mirror is written from LDS, a diagonal block from its lower
// triangle, so dst is exactly symmetric; padding is written 0.
hipError_t ppls_launch_adjust_schur(const double* src, int P_src, double* dst, int p, int ldx, int q, int ldy_dst,
                                    const double* F, int k, hipStream_t st);
}
