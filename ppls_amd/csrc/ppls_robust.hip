// ppls_robust.hip -- E-step of the multivariate-t PPLS model on the device: distances to weights and the
// sums of the t log-likelihood (launch interface and the determinism statement: ppls_robust.h; the
// model: DESIGN.md §24).
//
//   ppls_robust_rows_kernel    per row d2, the weight for one nu, log1p(d2 / nu_j) for up to 16 nu; one
//                              partial of PPLS_ROBUST_SUMS doubles per block of PPLS_ROBUST_BLOCK rows
//   ppls_robust_reduce_kernel  the partials summed by one workgroup, a fixed tree
//
// HBM-bound: 24 B read and 16 B written per row.  Plain HIP: no inline asm, no atomics.
#include <hip/hip_runtime.h>

#include "ppls_robust.h"

namespace {

constexpr int NS = PPLS_ROBUST_SUMS;

// The 256 threads' values of each of the NS sums into out[0 .. NS): lanes by an xor tree (every lane ends
// with the same bits), then the four waves as (0 + 1) + (2 + 3).
__device__ inline void block_sums(double (&acc)[NS], double (&sh)[4][NS], double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    double v = acc[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) sh[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) out[threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
  __syncthreads();   // sh is reused by the caller's next block
}

__global__ __launch_bounds__(256) void ppls_robust_rows_kernel(const double* __restrict__ odx2, const double* __restrict__ ody2,
                                                               const double* __restrict__ sd2, int64_t n, double sE2, double sF2,
                                                               PplsRobustNu nu, int m, double nuk, double P,
                                                               double* __restrict__ w, double* __restrict__ d2o,
                                                               double* __restrict__ part) {
  __shared__ double sh[4][NS];
  const int64_t nblocks = (n + PPLS_ROBUST_BLOCK - 1) / PPLS_ROBUST_BLOCK;
  for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    double acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    const int64_t i0 = b * PPLS_ROBUST_BLOCK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PPLS_ROBUST_BLOCK / 256; ++k) {
      const int64_t i = i0 + 256 * k;
      if (i < n) {
        const double d2 = (odx2[i] / sE2 + ody2[i] / sF2) + sd2[i];
        const double wi = (nuk + P) / (nuk + d2);
        w[i] = wi;
        if (d2o) d2o[i] = d2;
#pragma unroll
        for (int j = 0; j < PPLS_ROBUST_MAXNU; ++j)
          if (j < m) acc[j] += log1p(d2 / nu.nu[j]);
        acc[PPLS_ROBUST_MAXNU] += wi;
      }
    }
    block_sums(acc, sh, part + b * NS);
  }
}

__global__ __launch_bounds__(256) void ppls_robust_reduce_kernel(const double* __restrict__ part, int64_t nblocks,
                                                                 double* __restrict__ sums) {
  __shared__ double sh[4][NS];
  double acc[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) acc[j] = 0.0;
  for (int64_t b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] += part[b * NS + j];
  block_sums(acc, sh, sums);
}

}  // namespace

extern "C" {

int64_t ppls_robust_blocks(int64_t n) {
  const int64_t b = (n + PPLS_ROBUST_BLOCK - 1) / PPLS_ROBUST_BLOCK;
  return b < 1 ? 1 : b;
}

int ppls_robust_grid(int64_t n, int num_cus) {
  const int64_t b = ppls_robust_blocks(n), cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
  return (int)(b < cap ? b : cap);
}

hipError_t ppls_launch_robust_weights(const double* odx2, const double* ody2, const double* sd2, int64_t n, double sE2,
                                      double sF2, const PplsRobustNu* nu, int m, int keep, double P, double* w,
                                      double* d2, double* part, double* sums, int grid, hipStream_t st) {
  if (n < 0 || !nu || m < 1 || m > PPLS_ROBUST_MAXNU || keep < 0 || keep >= m || !sums || grid < 1)
    return hipErrorInvalidValue;
  if (n == 0) return hipMemsetAsync(sums, 0, sizeof(double) * NS, st);
  if (!odx2 || !ody2 || !sd2 || !w || !part) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_robust_rows_kernel, dim3((unsigned)grid), dim3(256), 0, st, odx2, ody2, sd2, n, sE2, sF2, *nu, m,
                     nu->nu[keep], P, w, d2, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ppls_robust_reduce_kernel, dim3(1), dim3(256), 0, st, part, ppls_robust_blocks(n), sums);
  return hipGetLastError();
}

}  // extern "C"
