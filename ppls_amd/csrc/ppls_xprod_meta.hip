// ppls_xprod_meta.hip -- the cross-product form of one meta_PPLSi EM step (ppls_xprod_meta.h).
//
//   ppls_xprod_meta_rows_kernel   M_j = S_j blockdiag(w, c) for all K populations in one launch
//                                 (blockIdx.y = population), and from it the X_j'mu_T, Y_j'mu_U rows:
//                                 one read of every S_j, HBM/MALL-bound
//   ppls_xprod_meta_gram_kernel   the 2 x 2 Grams blockdiag(w, c)' M_j, one workgroup per upper entry
//                                 and population, mirrored
// r = 1 only, so the body is a batched symmetric matrix times two vectors: a wave owns RW rows of
// S_j and walks their columns 128 at a time (16-B loads, two columns per lane) -- the X columns
// against w, then the Y columns against c.  With one column of B the LDS staging of
// ppls_xprod_tile_kernel buys nothing: w and c are P doubles, read per 128-column step from L1/L2
// (1 / RW of S's traffic), and no barrier ties the waves of a workgroup together.
// Every sum has a fixed order: a lane adds its columns in ascending order, the 64 lanes are summed
// by a butterfly, so the same inputs give the same bits in every launch and context.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppls_xprod_meta.h"

namespace {

constexpr int kWaves = 4;   // waves per workgroup of the rows kernel (independent of each other)

typedef double d2v __attribute__((ext_vector_type(2)));

// acc[rr] += S[row rr, soff + (0 .. width)] . b[0 .. width), this lane's columns in ascending order.
template <int RW, bool NT>
__device__ __forceinline__ void ppls_xpm_phase(const double* const (&srow)[RW], const double* __restrict__ b, int width,
                                               int soff, double (&acc)[RW], int lane) {
#pragma unroll 4
  for (int c = 2 * lane; c < width; c += 128) {
    const d2v bv = *(const d2v*)(b + c);
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      d2v s;
      if constexpr (NT) s = __builtin_nontemporal_load((const d2v*)(srow[rr] + soff + c));
      else s = *(const d2v*)(srow[rr] + soff + c);
      acc[rr] = fma(s.y, bv.y, fma(s.x, bv.x, acc[rr]));
    }
  }
}

template <int RW, bool NT>
__global__ __launch_bounds__(64 * kWaves) void ppls_xprod_meta_rows_kernel(
    const double* __restrict__ S, int ldx, int ldy, const double* __restrict__ Wp, const double* __restrict__ Cp,
    const PplsScalars* __restrict__ sc, double* __restrict__ stats, int64_t part_ld, double* __restrict__ M,
    const int* __restrict__ stop) {
  if (stop && *stop) return;   // the fit ended at an earlier step
  const int P = ldx + ldy;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = blockIdx.y;
  const int64_t i0 = ((int64_t)blockIdx.x * kWaves + wave) * RW;   // this wave's first row of S_j
  if (i0 >= P) return;
  const double* Sj = S + (int64_t)j * P * P;
  const double* srow[RW];
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) srow[rr] = Sj + (i0 + rr < P ? i0 + rr : (int64_t)P - 1) * P;   // rows past P: dropped
  double mw[RW], mc[RW];
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) mw[rr] = mc[rr] = 0.0;
  ppls_xpm_phase<RW, NT>(srow, Wp, ldx, 0, mw, lane);
  ppls_xpm_phase<RW, NT>(srow, Cp, ldy, ldx, mc, lane);
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mw[rr] += __shfl_xor(mw[rr], o);
      mc[rr] += __shfl_xor(mc[rr], o);
    }
  }
  const PplsScalars* s = sc + j;
  double* Mj = M + (int64_t)j * 2 * P;
  double* st = stats + (int64_t)j * part_ld;
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) {   // lane rr writes row rr (every lane holds every sum)
    const int64_t i = i0 + rr;
    if (lane != rr || i >= P) continue;
    Mj[i] = mw[rr];
    Mj[P + i] = mc[rr];
    if (i < ldx) st[i] = s->alpha[0] * mw[rr] + s->beta[0] * mc[rr];   // X_j'mu_T
    else st[i] = s->gamma[0] * mw[rr] + s->delta[0] * mc[rr];          // Y_j'mu_U (at ldx + (i - ldx))
  }
}

// Gram entry e of population blockIdx.y: 0 = w'M_0[X] (0,0), 1 = w'M_1[X] (0,1) and its mirror,
// 2 = c'M_1[Y] (1,1).  The sums are ppls_xprod_gram_kernel's.
__global__ __launch_bounds__(256) void ppls_xprod_meta_gram_kernel(int ldx, int ldy, const double* __restrict__ Wp,
                                                                   const double* __restrict__ Cp,
                                                                   const double* __restrict__ M,
                                                                   double* __restrict__ stats, int64_t part_ld,
                                                                   const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ double red[4];
  const int P = ldx + ldy;
  const int e = blockIdx.x, j = blockIdx.y;
  const int a = e == 2 ? 1 : 0, b = e == 0 ? 0 : 1;
  const double* Bcol = a == 0 ? Wp : Cp;
  const double* Mcol = M + (int64_t)j * 2 * P + (int64_t)b * P + (a == 0 ? 0 : ldx);
  const int rows = a == 0 ? ldx : ldy;
  double v4[4] = {0.0, 0.0, 0.0, 0.0};
  int i = threadIdx.x;
  for (; i + 3 * 256 < rows; i += 4 * 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) v4[u] = fma(Bcol[i + u * 256], Mcol[i + u * 256], v4[u]);
  }
  for (; i < rows; i += 256) v4[0] = fma(Bcol[i], Mcol[i], v4[0]);
  double v = (v4[0] + v4[1]) + (v4[2] + v4[3]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double g = (red[0] + red[1]) + (red[2] + red[3]);
    double* G = stats + (int64_t)j * part_ld + ldx + ldy;
    G[b * 2 + a] = g;
    G[a * 2 + b] = g;
  }
}

template <int RW>
hipError_t launch_rows(const double* S, int K, int ldx, int ldy, const double* Wp, const double* Cp, const PplsScalars* sc,
                       double* stats, int64_t part_ld, double* M, const int* stop, hipStream_t st) {
  const int P = ldx + ldy;
  const dim3 grid((unsigned)((P + kWaves * RW - 1) / (kWaves * RW)), (unsigned)K);
  if (ppls_xprod_meta_nt(K, P))
    hipLaunchKernelGGL((ppls_xprod_meta_rows_kernel<RW, true>), grid, dim3(64 * kWaves), 0, st, S, ldx, ldy, Wp, Cp, sc,
                       stats, part_ld, M, stop);
  else
    hipLaunchKernelGGL((ppls_xprod_meta_rows_kernel<RW, false>), grid, dim3(64 * kWaves), 0, st, S, ldx, ldy, Wp, Cp, sc,
                       stats, part_ld, M, stop);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int ppls_xprod_meta_rows(int K, int P, int rw_opt, int num_cus) {
  if (rw_opt == 1 || rw_opt == 2 || rw_opt == 4 || rw_opt == 8) return rw_opt;
  // four rows per wave while that leaves two workgroups per CU over all K matrices (C3: 83.5 against
  // 89.4 us at K = 4, 490 against 520 us at K = 25; profiles/meta_xprod_rw_ab.txt), else one
  return (int64_t)K * P / (4 * kWaves) >= 2 * (int64_t)num_cus ? 4 : 1;
}

int ppls_xprod_meta_nt(int K, int P) { return 8.0 * (double)K * P * (double)P > 200.0 * (1 << 20) ? 1 : 0; }

hipError_t ppls_launch_xprod_meta(const double* S, int K, int ldx, int ldy, int rw, const double* Wp, const double* Cp,
                                  const PplsScalars* sc, double* stats, int64_t part_ld, double* M, const int* stop,
                                  hipStream_t st) {
  if (K < 1 || K > 65535 || ldx < 2 || ldy < 2 || (ldx & 1) || (ldy & 1) || part_ld < (int64_t)ldx + ldy + 4)
    return hipErrorInvalidValue;
  if (((uintptr_t)S | (uintptr_t)Wp | (uintptr_t)Cp) & 15) return hipErrorInvalidValue;   // 16-B loads
  hipError_t e;
  switch (rw) {
    case 1: e = launch_rows<1>(S, K, ldx, ldy, Wp, Cp, sc, stats, part_ld, M, stop, st); break;
    case 2: e = launch_rows<2>(S, K, ldx, ldy, Wp, Cp, sc, stats, part_ld, M, stop, st); break;
    case 4: e = launch_rows<4>(S, K, ldx, ldy, Wp, Cp, sc, stats, part_ld, M, stop, st); break;
    case 8: e = launch_rows<8>(S, K, ldx, ldy, Wp, Cp, sc, stats, part_ld, M, stop, st); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ppls_xprod_meta_gram_kernel, dim3(3, (unsigned)K), dim3(256), 0, st, ldx, ldy, Wp, Cp, M, stats,
                     part_ld, stop);
  return hipGetLastError();
}

}  // extern "C"
