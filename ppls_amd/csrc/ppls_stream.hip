// ppls_stream.hip -- kernels of the streamed-data path (launch interface: ppls_stream.h).
//
//   ppls_stream_mean_kernel   chunk mean, delta = chunk mean - running mean, running mean update.
//   ppls_stream_tile_kernel   one 64 x 64 block of the lower triangle of S per workgroup:
//                             MERGE   S += sum of the Gram's split partials + w delta delta' (the MFMA
//                                     Gram's finish step and Chan's pairwise update in one pass over S),
//                             SCALE   S_ij /= d_i d_j.
// The walk over S, its staging, padding, LDS copy and mirror write are ppls_symtile_pass
// (ppls_symtile.h); the kernels here supply the per-entry update.  Every entry is one fixed chain of
// additions: bitwise repeatable.  Plain HIP, vector stores only.
#include <hip/hip_runtime.h>

#include "ppls_kernels.h"
#include "ppls_stream.h"
#include "ppls_symtile.h"

namespace {

constexpr int SB = PPLS_SYM_SB;
constexpr int ST_THREADS = PPLS_SYM_THREADS;
using StreamCols = PplsSymCols;

__global__ __launch_bounds__(ST_THREADS) void ppls_stream_mean_kernel(const double* __restrict__ sum, StreamCols g, double nc,
                                                                      double N, double* __restrict__ mc,
                                                                      double* __restrict__ delta, double* __restrict__ mean) {
  const int j = blockIdx.x * ST_THREADS + threadIdx.x;
  if (j >= g.P) return;
  const double m = ppls_sym_col_live(g, j) ? sum[j] / nc : 0.0;
  const double d = m - mean[j];
  mc[j] = m;
  delta[j] = d;
  mean[j] += d * (nc / (N + nc));
}

// MERGE: the Gram partials of the block, in the layout ppls_gram_wave_item writes and
// ppls_gram_finish_kernel reads (ppls_variances.hip): item = (split, lower 128-tile
// t = I (I + 1) / 2 + J, quadrant 2 (row half) + (column half)), 64 x 64 doubles each, row-major;
// split_stride is ppls_gram_part_doubles(P, 1).  The split partials are added in split order, then
// (w delta_i) delta_j.
struct StreamMerge {
  const double* part;   // at the block's first partial
  int nsplit;
  int64_t split_stride;
  double w;
  __device__ double2 operator()(double2 v, int r, int c2, const double (&va)[1][SB], const double (&vb)[1][SB]) const {
    const double* pp = part + r * SB + c2;
    for (int s = 0; s < nsplit; ++s) {
      const double2 a = *(const double2*)(pp + (int64_t)s * split_stride);
      v.x += a.x;
      v.y += a.y;
    }
    const double wa = w * va[0][r];
    v.x += wa * vb[0][c2];
    v.y += wa * vb[0][c2 + 1];
    return v;
  }
};

// SCALE: S_ij /= d_i d_j
struct StreamScale {
  __device__ double2 operator()(double2 v, int r, int c2, const double (&va)[1][SB], const double (&vb)[1][SB]) const {
    v.x /= va[0][r] * vb[0][c2];
    v.y /= va[0][r] * vb[0][c2 + 1];
    return v;
  }
};

template <bool MERGE>
__global__ __launch_bounds__(ST_THREADS) void ppls_stream_tile_kernel(double* __restrict__ S, StreamCols g,
                                                                      const double* __restrict__ part, int nsplit,
                                                                      int64_t split_stride, const double* __restrict__ vec,
                                                                      double w) {
  const PplsSymBlock blk = ppls_sym_block(blockIdx.x);
  const double* const v[1] = {vec};
  if (MERGE) {
    const int I = blk.qi >> 1, J = blk.qj >> 1;
    const int64_t poff = ((int64_t)(I * (I + 1) / 2 + J) * 4 + (((blk.qi & 1) << 1) | (blk.qj & 1))) * (SB * SB);
    ppls_symtile_pass<1>(S, g, blk, v, {0.0}, StreamMerge{part + poff, nsplit, split_stride, w});
  } else {
    ppls_symtile_pass<1>(S, g, blk, v, {1.0}, StreamScale{});
  }
}

}  // namespace

extern "C" {

hipError_t ppls_launch_stream_mean(const double* sum, int P, int p, int ldx, int q, double nc, double N, double* mc,
                                   double* delta, double* mean, hipStream_t st) {
  if (!sum || !mc || !delta || !mean || P < 2 || !(nc >= 1.0) || N < 0.0 || ldx + q > P) return hipErrorInvalidValue;
  const StreamCols g{P, p, ldx, ldx + q};
  hipLaunchKernelGGL(ppls_stream_mean_kernel, dim3((P + ST_THREADS - 1) / ST_THREADS), dim3(ST_THREADS), 0, st, sum, g, nc, N,
                     mc, delta, mean);
  return hipGetLastError();
}

hipError_t ppls_launch_stream_merge(double* S, int p, int ldx, int q, int ldy, const double* part, int nsplit,
                                    const double* delta, double w, hipStream_t st) {
  if (!S || !ppls_sym_shape_ok(p, ldx, q, ldy) || nsplit < 0 || (nsplit > 0 && !part)) return hipErrorInvalidValue;
  const int P = ldx + ldy;
  const StreamCols g{P, p, ldx, ldx + q};
  hipLaunchKernelGGL(ppls_stream_tile_kernel<true>, dim3(ppls_sym_blocks(P)), dim3(ST_THREADS), 0, st, S, g, part, nsplit,
                     ppls_gram_part_doubles(P, 1), delta, delta ? w : 0.0);
  return hipGetLastError();
}

hipError_t ppls_launch_stream_standardise(double* S, int p, int ldx, int q, int ldy, const double* d, hipStream_t st) {
  if (!S || !d || !ppls_sym_shape_ok(p, ldx, q, ldy)) return hipErrorInvalidValue;
  const int P = ldx + ldy;
  const StreamCols g{P, p, ldx, ldx + q};
  hipLaunchKernelGGL(ppls_stream_tile_kernel<false>, dim3(ppls_sym_blocks(P)), dim3(ST_THREADS), 0, st, S, g, (const double*)nullptr, 0,
                     (int64_t)0, d, 0.0);
  return hipGetLastError();
}

}  // extern "C"
