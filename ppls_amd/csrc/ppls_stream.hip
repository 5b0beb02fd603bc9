// ppls_stream.hip -- kernels of the streamed-data path (launch interface: ppls_stream.h).
//
//   ppls_stream_mean_kernel   chunk mean, delta = chunk mean - running mean, running mean update.
//   ppls_stream_tile_kernel   one 64 x 64 block of the lower triangle of S per workgroup:
//                             MERGE   S += sum of the Gram's split partials + w delta delta' (the MFMA
//                                     Gram's finish step and Chan's pairwise update in one pass over S),
//                             SCALE   S_ij /= d_i d_j.
// A thread owns one 16-byte column pair of 8 rows of the block (a row of the block is 32 threads =
// 512 contiguous bytes); the new values go to S and into an LDS copy, from which the mirror block is
// written with the same 16-byte stores.  A diagonal block takes every entry from its lower triangle
// (as the Gram's own finish does), so S stays exactly symmetric.  Every entry is one fixed chain of
// additions: bitwise repeatable.  Plain HIP, vector stores only.
#include <hip/hip_runtime.h>

#include "ppls_kernels.h"
#include "ppls_stream.h"

namespace {

constexpr int SB = 64;          // block edge = the MFMA Gram's quadrant edge (PPLS_GQ of ppls_variances.hip)
constexpr int ST_THREADS = 256;

struct StreamCols {
  int P, p, ldx, yend;   // live columns: [0, p) and [ldx, yend)
};

__device__ inline bool col_live(const StreamCols& g, int c) { return c < g.p || (c >= g.ldx && c < g.yend); }

__global__ __launch_bounds__(ST_THREADS) void ppls_stream_mean_kernel(const double* __restrict__ sum, StreamCols g, double nc,
                                                                      double N, double* __restrict__ mc,
                                                                      double* __restrict__ delta, double* __restrict__ mean) {
  const int j = blockIdx.x * ST_THREADS + threadIdx.x;
  if (j >= g.P) return;
  const double m = col_live(g, j) ? sum[j] / nc : 0.0;
  const double d = m - mean[j];
  mc[j] = m;
  delta[j] = d;
  mean[j] += d * (nc / (N + nc));
}

template <bool MERGE>
__global__ __launch_bounds__(ST_THREADS) void ppls_stream_tile_kernel(double* __restrict__ S, StreamCols g,
                                                                      const double* __restrict__ part, int nsplit,
                                                                      int64_t split_stride, const double* __restrict__ vec,
                                                                      double w) {
  // block t of the lower triangle in row order: (qi, qj), qj <= qi, t = qi (qi + 1) / 2 + qj
  const int t_blk = blockIdx.x;
  int qi = (int)((sqrt(8.0 * t_blk + 1.0) - 1.0) * 0.5);
  while ((qi + 1) * (qi + 2) / 2 <= t_blk) ++qi;
  while (qi * (qi + 1) / 2 > t_blk) --qi;
  const int qj = t_blk - qi * (qi + 1) / 2;
  __shared__ double T[SB][SB + 1];
  __shared__ double va[SB], vb[SB];   // vec over the block's rows / columns (MERGE: delta, else d)
  const int t = threadIdx.x;
  const int P = g.P;
  if (t < 2 * SB) {
    const int c = (t < SB ? qi * SB + t : qj * SB + (t - SB));
    const double v = (vec && c < P) ? vec[c] : (MERGE ? 0.0 : 1.0);
    if (t < SB) va[t] = v; else vb[t - SB] = v;
  }
  __syncthreads();
  const int c2 = (t & 31) * 2, rb = t >> 5;
  const int lo = qj * SB + c2;
  const bool diag = qi == qj;
  // the Gram partials of this block, in the layout ppls_gram_wave_item writes and
  // ppls_gram_finish_kernel reads (ppls_variances.hip): item = (split, lower 128-tile
  // t = I (I + 1) / 2 + J, quadrant 2 (row half) + (column half)), 64 x 64 doubles each, row-major;
  // split_stride is ppls_gram_part_doubles(P, 1)
  const int I = qi >> 1, J = qj >> 1;
  const int64_t poff = ((int64_t)(I * (I + 1) / 2 + J) * 4 + (((qi & 1) << 1) | (qj & 1))) * (SB * SB);
#pragma unroll
  for (int k = 0; k < SB / 8; ++k) {
    const int r = rb + 8 * k, hi = qi * SB + r;
    double2 v = make_double2(0.0, 0.0);
    if (hi < P && lo < P) {   // P is even: lo + 1 < P as well
      double* sp = S + (int64_t)hi * P + lo;
      v = *(const double2*)sp;
      if (MERGE) {
        const double* pp = part + poff + r * SB + c2;
        for (int s = 0; s < nsplit; ++s) {
          const double2 a = *(const double2*)(pp + (int64_t)s * split_stride);
          v.x += a.x;
          v.y += a.y;
        }
        const double wa = w * va[r];
        v.x += wa * vb[c2];
        v.y += wa * vb[c2 + 1];
      } else {
        v.x /= va[r] * vb[c2];
        v.y /= va[r] * vb[c2 + 1];
      }
      const bool lh = col_live(g, hi);
      if (!lh || !col_live(g, lo)) v.x = 0.0;
      if (!lh || !col_live(g, lo + 1)) v.y = 0.0;
      if (!diag) *(double2*)sp = v;
    }
    T[r][c2] = v.x;
    T[r][c2 + 1] = v.y;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SB / 8; ++k) {
    const int r = rb + 8 * k;
    if (diag) {   // entry (r, c) from the lower triangle: (max, min)
      const int hi = qi * SB + r;
      if (hi < P && lo < P) {
        const double x = c2 <= r ? T[r][c2] : T[c2][r];
        const double y = c2 + 1 <= r ? T[r][c2 + 1] : T[c2 + 1][r];
        *(double2*)(S + (int64_t)hi * P + lo) = make_double2(x, y);
      }
    } else {      // the mirror block (qj, qi): row qj SB + r, columns qi SB + c2, c2 + 1
      const int mr = qj * SB + r, mc = qi * SB + c2;
      if (mr < P && mc < P) *(double2*)(S + (int64_t)mr * P + mc) = make_double2(T[c2][r], T[c2 + 1][r]);
    }
  }
}

bool shape_ok(int p, int ldx, int q, int ldy) {
  return p >= 1 && q >= 1 && p <= ldx && q <= ldy && ldx % 2 == 0 && ldy % 2 == 0 && (int64_t)ldx + ldy < (1 << 30);
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
  if (!S || !shape_ok(p, ldx, q, ldy) || nsplit < 0 || (nsplit > 0 && !part)) return hipErrorInvalidValue;
  const int P = ldx + ldy, nq = (P + SB - 1) / SB;
  const StreamCols g{P, p, ldx, ldx + q};
  hipLaunchKernelGGL(ppls_stream_tile_kernel<true>, dim3(nq * (nq + 1) / 2), dim3(ST_THREADS), 0, st, S, g, part, nsplit,
                     ppls_gram_part_doubles(P, 1), delta, delta ? w : 0.0);
  return hipGetLastError();
}

hipError_t ppls_launch_stream_standardise(double* S, int p, int ldx, int q, int ldy, const double* d, hipStream_t st) {
  if (!S || !d || !shape_ok(p, ldx, q, ldy)) return hipErrorInvalidValue;
  const int P = ldx + ldy, nq = (P + SB - 1) / SB;
  const StreamCols g{P, p, ldx, ldx + q};
  hipLaunchKernelGGL(ppls_stream_tile_kernel<false>, dim3(nq * (nq + 1) / 2), dim3(ST_THREADS), 0, st, S, g, (const double*)nullptr, 0,
                     (int64_t)0, d, 0.0);
  return hipGetLastError();
}

}  // extern "C"
