// ppls_permute.hip -- C_pi = sum_i x_i y_pi(i)' on v_mfma_f64_16x16x4_f64: the p x q block of
// S = [X Y_pi]'[X Y_pi] that a permutation pi of Y's rows against X's changes; X'X and Y'Y do not depend
// on pi.  A rectangular kernel of its own, not an instantiation of ppls_gram_wave_item: the joint Gram's
// fp64 form sits at the register limit of two waves per SIMD, and a gathered operand there would have
// changed the code generated for the forms that exist.
//   ppls_xperm_kernel          one wave per (row split, 64 x 64 quadrant of the block): X's rows in storage
//                              order, Y's row taken at perm[row]; per-item partials, fixed order
//   ppls_xperm_finish_kernel   the splits added in split order into the ldx x ldy block (padding 0)
//   ppls_xperm_scatter_kernel  the block written into both off-diagonal blocks of S, from one value
#include "ppls_permute.h"

#include <algorithm>

#define PPLS_PQ 64     // quadrant edge
#define PPLS_PRING 3   // k-steps of MFMA operands in flight per wave (the joint Gram's depth)

namespace {

// A lane's MFMA operands of one 4-row k-step of one side, as the joint Gram loads them (PplsGramOps):
// lane l reads one row and, for fp64, the column pairs 2 i, 2 i + 1 and 32 + 2 i, 33 + 2 i of the side's 64
// (i = l & 15: each 16-lane group reads 256 contiguous bytes per load -- of one row, so a gathered row
// keeps that); for fp32 the quad 4 i .. 4 i + 3.
template <typename T>
struct PermOps;
template <>
struct PermOps<double> {
  static constexpr int NL = 2;
  double2 v[2];
  __device__ __forceinline__ void load(const double* const* ptr, int64_t off) {
    v[0] = *(const double2*)(ptr[0] + off);
    v[1] = *(const double2*)(ptr[1] + off);
  }
  __device__ __forceinline__ double op(int m) const { return m == 0 ? v[0].x : m == 1 ? v[0].y : m == 2 ? v[1].x : v[1].y; }
  __host__ __device__ static int lcol(int l, int i) { return 32 * l + 2 * i; }
  __host__ __device__ static int col(int m, int i) { return 32 * (m >> 1) + 2 * i + (m & 1); }
};
template <>
struct PermOps<float> {
  static constexpr int NL = 1;
  float4 v[1];
  __device__ __forceinline__ void load(const float* const* ptr, int64_t off) { v[0] = *(const float4*)(ptr[0] + off); }
  __device__ __forceinline__ double op(int m) const {
    return (double)(m == 0 ? v[0].x : m == 1 ? v[0].y : m == 2 ? v[0].z : v[0].w);
  }
  __host__ __device__ static int lcol(int, int i) { return 4 * i; }
  __host__ __device__ static int col(int m, int i) { return 4 * i + m; }
};

// One item = split s x quadrant (qa, qb) on one wave: 4 x 4 MFMA blocks, 64 fp64 accumulators per lane,
// operands straight from global memory into a ring PPLS_PRING k-steps deep, no LDS, no barrier.  The A
// side (X's 64 columns) reads row r0 + kr + 4 step; the B side (Y's 64 columns) reads row
// perm[r0 + kr + 4 step], whose index rides in the ring one ring length ahead of the operands it
// addresses (a load that waited for an index fetched in the same step would drain the ring: vector
// loads return in order).  Column vectors at or past the row stride read column 0: they only meet output
// rows / columns the finish never reads.  Rows past the split's end are zeros (the one partial k-step).
// The sums depend on (rows, perm, bounds) alone: same call, same bits.
template <typename T>
__global__ __launch_bounds__(256, 2) void ppls_xperm_kernel(const T* __restrict__ X, int ldx, const T* __restrict__ Y,
                                                             int ldy, const int32_t* __restrict__ perm,
                                                             const int64_t* __restrict__ bounds, int nqb, int per,
                                                             int nitems, double* __restrict__ part) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  typedef PermOps<T> Op;
  constexpr int D = PPLS_PRING;
  const int it = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (it >= nitems) return;
  const int s = it / per, t = it - s * per;
  const int qa = t / nqb, qb = t - qa * nqb;
  const int64_t r0 = bounds[s], r1 = bounds[s + 1];
  const int lane = threadIdx.x & 63, kr = lane >> 4, li = lane & 15;
  const T* pa[Op::NL];
  const T* pb[Op::NL];   // B: the column only; the row comes from perm
#pragma unroll
  for (int l = 0; l < Op::NL; ++l) {
    const int ca = qa * PPLS_PQ + Op::lcol(l, li), cb = qb * PPLS_PQ + Op::lcol(l, li);
    pa[l] = X + (ca < ldx ? ca : 0) + (r0 + kr) * (int64_t)ldx;
    pb[l] = Y + (cb < ldy ? cb : 0);
  }
  const int64_t sa = 4 * (int64_t)ldx;
  const int32_t* pi = perm + r0 + kr;   // this lane's row index of the next k-step to fetch
  Op ra[D], rb[D];
  int32_t ri[D];
  auto ld_step = [&](int d) {
    const int64_t off = (int64_t)ri[d] * ldy;
    ra[d].load(pa, 0);
    rb[d].load(pb, off);
    ri[d] = *pi;   // of the k-step D later (past the split's end: unused; past n: the array's padding)
    pi += 4;
#pragma unroll
    for (int l = 0; l < Op::NL; ++l) pa[l] += sa;
  };
  d4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[m][q] = d4{0.0, 0.0, 0.0, 0.0};
  auto mma = [&](const Op& A, const Op& B) {
    double a[4], b[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) a[m] = A.op(m);
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = B.op(q);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[q], acc[m][q], 0, 0, 0);
  };
  const int64_t nfull = (r1 - r0) / 4;   // whole 4-row k-steps
  int64_t kk = 0;
  if (nfull >= 2 * D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      ri[d] = *pi;
      pi += 4;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      ld_step(d);
      __builtin_amdgcn_sched_barrier(0);
    }
    for (; kk + 2 * D <= nfull; kk += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        mma(ra[d], rb[d]);
        ld_step(d);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) mma(ra[d], rb[d]);
    kk += D;
  }
  // the last < 2 D whole k-steps and the partial one fetch their index first, then the operands
  const int32_t* pt = perm + r0 + kr;
  for (; kk < nfull; ++kk) {
    Op A, B;
    A.load(pa, 0);
    B.load(pb, (int64_t)pt[4 * kk] * ldy);
#pragma unroll
    for (int l = 0; l < Op::NL; ++l) pa[l] += sa;
    mma(A, B);
  }
  if (r1 - r0 > 4 * nfull) {
    Op A, B;
#pragma unroll
    for (int l = 0; l < Op::NL; ++l) {
      A.v[l] = {};
      B.v[l] = {};
    }
    if (r0 + 4 * nfull + kr < r1) {   // (the only rows of this k-step whose index is read)
      A.load(pa, 0);
      B.load(pb, (int64_t)pt[4 * nfull] * ldy);
    }
    mma(A, B);
  }
  double* out = part + (int64_t)it * (PPLS_PQ * PPLS_PQ);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = Op::col(q, li);
#pragma unroll
      for (int g = 0; g < 4; ++g)   // f64 MFMA D map: row (lane >> 4) + 4 g, column lane & 15
        out[Op::col(m, kr + 4 * g) * PPLS_PQ + b] = acc[m][q][g];
    }
}

__global__ void ppls_xperm_finish_kernel(const double* __restrict__ part, int nsplit, int p, int q, int ldx, int ldy,
                                         int nqb, int per, double* __restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)ldx * ldy) return;
  const int b = (int)(e / ldx), a = (int)(e - (int64_t)b * ldx);
  double v = 0.0;
  if (a < p && b < q) {
    const int64_t off = ((int64_t)(a >> 6) * nqb + (b >> 6)) * (PPLS_PQ * PPLS_PQ) + (a & 63) * PPLS_PQ + (b & 63);
    const int64_t stride = (int64_t)per * (PPLS_PQ * PPLS_PQ);
    for (int s = 0; s < nsplit; ++s) v += part[(int64_t)s * stride + off];
  }
  C[e] = v;
}

__global__ void ppls_xperm_scatter_kernel(const double* __restrict__ C, int ldx, int ldy, double* __restrict__ S) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)ldx * ldy) return;
  const int b = (int)(e / ldx), a = (int)(e - (int64_t)b * ldx);
  const int64_t P = (int64_t)ldx + ldy;
  const double v = C[e];
  S[a + (ldx + b) * P] = v;
  S[(ldx + b) + a * P] = v;
}

}  // namespace

extern "C" {

int ppls_xperm_occupancy(int f32) {
  int occ = 0;
  hipError_t e = f32 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ppls_xperm_kernel<float>, 256, 0)
                     : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ppls_xperm_kernel<double>, 256, 0);
  return e == hipSuccess && occ > 0 ? occ : 1;
}

int ppls_xperm_quads(int p, int q) { return ((p + PPLS_PQ - 1) / PPLS_PQ) * ((q + PPLS_PQ - 1) / PPLS_PQ); }

int64_t ppls_xperm_part_doubles(int p, int q, int nsplit) {
  return (int64_t)nsplit * ppls_xperm_quads(p, q) * PPLS_PQ * PPLS_PQ;
}

// ppls_gram_plan's guided schedule with the block's own quadrant count: workgroups are dispatched in
// item order, split by split, so each split holds about half the remaining work per wave slot and the
// run ends on short ones.
int ppls_xperm_plan(int p, int q, int64_t n, int wave_slots, int nsplit_req, int64_t* bounds) {
  if (nsplit_req > 0) {
    if (nsplit_req > PPLS_XPERM_MAXSPLIT) nsplit_req = PPLS_XPERM_MAXSPLIT;
    if (bounds)
      for (int s = 0; s <= nsplit_req; ++s) bounds[s] = n * s / nsplit_req;
    return nsplit_req;
  }
  const double w1 = (double)ppls_xperm_quads(p, q);
  const double slots = wave_slots > 0 ? (double)wave_slots : 1.0;
  int maxs = (int)(4.0e9 / (w1 * PPLS_PQ * PPLS_PQ * 8.0));
  maxs = maxs < 1 ? 1 : (maxs > PPLS_XPERM_MAXSPLIT ? PPLS_XPERM_MAXSPLIT : maxs);
  int64_t smin = (int64_t)(0.01 * w1 * (double)n / slots);
  if (smin < 256) smin = 256;
  int ns = 0;
  int64_t done = 0;
  if (bounds) bounds[0] = 0;
  while (done < n) {
    const int64_t R = n - done;
    int64_t sz = (int64_t)(w1 * (double)R / (2.0 * slots));
    if (sz > R / 2) sz = R / 2;
    if (sz < smin) sz = smin;
    if (R - sz < smin || ns + 1 >= maxs) sz = R;
    done += sz;
    ++ns;
    if (bounds) bounds[ns] = done;
  }
  if (ns < 1) {
    ns = 1;
    if (bounds) bounds[1] = n;
  }
  return ns;
}

hipError_t ppls_launch_xperm(const void* X, int ldx, int p, const void* Y, int ldy, int q, int f32, int64_t n,
                             const int32_t* perm, const int64_t* bounds, int nsplit, double* part, hipStream_t st) {
  const int ev = f32 ? 4 : 2;
  if (n <= 0 || n > 0x7fffffffLL || p < 1 || q < 1 || p > ldx || q > ldy || ldx % ev || ldy % ev || nsplit < 1 ||
      nsplit > PPLS_XPERM_MAXSPLIT || !perm || !bounds || !part)
    return hipErrorInvalidValue;
  const int nqb = (q + PPLS_PQ - 1) / PPLS_PQ, per = ppls_xperm_quads(p, q);
  const int64_t nitems = (int64_t)per * nsplit;
  if (nitems > 0x7fffffffLL - 4) return hipErrorInvalidValue;
  const dim3 gd((unsigned)((nitems + 3) / 4)), bd(256);
  if (f32)
    hipLaunchKernelGGL(ppls_xperm_kernel<float>, gd, bd, 0, st, (const float*)X, ldx, (const float*)Y, ldy, perm, bounds,
                       nqb, per, (int)nitems, part);
  else
    hipLaunchKernelGGL(ppls_xperm_kernel<double>, gd, bd, 0, st, (const double*)X, ldx, (const double*)Y, ldy, perm,
                       bounds, nqb, per, (int)nitems, part);
  return hipGetLastError();
}

hipError_t ppls_launch_xperm_finish(const double* part, int nsplit, int p, int q, int ldx, int ldy, double* C,
                                    hipStream_t st) {
  const int64_t len = (int64_t)ldx * ldy;
  hipLaunchKernelGGL(ppls_xperm_finish_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, part, nsplit, p, q,
                     ldx, ldy, (q + PPLS_PQ - 1) / PPLS_PQ, ppls_xperm_quads(p, q), C);
  return hipGetLastError();
}

hipError_t ppls_launch_xperm_scatter(const double* C, int ldx, int ldy, double* S, hipStream_t st) {
  const int64_t len = (int64_t)ldx * ldy;
  hipLaunchKernelGGL(ppls_xperm_scatter_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, C, ldx, ldy, S);
  return hipGetLastError();
}

}  // extern "C"
