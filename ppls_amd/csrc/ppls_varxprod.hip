// ppls_varxprod.hip -- kernels of ppls_variances_xprod (launch interface: ppls_varxprod.h).
//
//   ppls_varinfo_batched_kernel    the observed information J_i = SSt_exp_i - B_exp_i of every component
//                                  (and SSt_exp_i, SSt_star_i on request) from the p x p diagonal block
//                                  of S, read in place: one 64 x 64 block of the block's lower triangle
//                                  per workgroup, its S tile loaded once (16-byte loads) and kept in
//                                  registers while the components are looped over.
//   ppls_varfinish_batched_kernel  after the inverse: the lower triangles mirrored, seLoad.
//
// The walk is ppls_symtile.h's: a thread owns one column pair of 8 rows of the block.  Per component
// the block's values go to the output and into an LDS copy, from which the mirror block is written, so
// every matrix is symmetric bit for bit; a diagonal block takes every entry from its lower triangle.
// Cxt and w of the block's rows and columns are staged in LDS once, for all components.  The outputs
// are column-major p x p with p of either parity: 16-byte stores where the address is 16-byte aligned,
// 8-byte stores elsewhere.  Plain HIP, vector stores only.
#include <hip/hip_runtime.h>

#include "ppls_symtile.h"
#include "ppls_varxprod.h"

namespace {

constexpr int SB = PPLS_SYM_SB;
constexpr int VX_THREADS = PPLS_SYM_THREADS;

// out[e], out[e + 1] <- x, y (the second only with two): one 16-byte store where the address itself is
// 16-byte aligned (for odd p the parity of e alone does not say: component i starts at i p^2), else 8-byte stores
__device__ __forceinline__ void vx_store(double* __restrict__ out, int64_t e, double x, double y, bool two) {
  if (two && ((uintptr_t)(out + e) & 15) == 0) {
    *(double2*)(out + e) = make_double2(x, y);
  } else {
    out[e] = x;
    if (two) out[e + 1] = y;
  }
}

// One entry of SSt_exp: two products per cross term, three additions, two divisions, each rounded
// once (no contraction: the a-priori bar of tests/varinfo_bar.py counts these roundings).
__device__ __forceinline__ double vx_sse(double g, double xa, double wa, double xb, double wb, double ctt, double k1,
                                         double k2, double s4, double N) {
#pragma clang fp contract(off)
  return (ctt * g - xa * k1 * wb - wa * k1 * xb + wa * k2 * wb) / s4 / N;
}

__device__ __forceinline__ double vx_star(double xa, double wa, double xb, double wb, double ctt, double s4) {
#pragma clang fp contract(off)
  return (xa - wa * ctt) * (xb - wb * ctt) / s4;
}

// LDS: T 64 x 65 doubles (33,280 B) + the staged vectors 4 x 16 x 64 doubles (32,768 B) = 66,048 B:
// two workgroups per compute unit (145 VGPRs would allow three).
__global__ __launch_bounds__(VX_THREADS) void ppls_varinfo_batched_kernel(const PplsVarinfoArgs A) {
  __shared__ double T[SB][SB + 1];
  __shared__ double xr[PPLS_RMAX][SB], wr[PPLS_RMAX][SB];   // Cxt, w over the block's rows ...
  __shared__ double xc[PPLS_RMAX][SB], wc[PPLS_RMAX][SB];   // ... and over its columns
  const PplsSymBlock blk = ppls_sym_block(blockIdx.x);
  const int qi = blk.qi, qj = blk.qj;
  const int t = threadIdx.x, p = A.p, na = A.a;
  for (int e = t; e < na * SB; e += VX_THREADS) {
    const int i = e / SB, l = e - i * SB;
    const int ra = qi * SB + l, cb = qj * SB + l;
    xr[i][l] = ra < p ? A.cxt[i * A.ldc + ra] : 0.0;
    wr[i][l] = ra < p ? A.w[i * A.ldw + ra] : 0.0;
    xc[i][l] = cb < p ? A.cxt[i * A.ldc + cb] : 0.0;
    wc[i][l] = cb < p ? A.w[i * A.ldw + cb] : 0.0;
  }
  const int c2 = (t & 31) * 2, rb = t >> 5;
  const int lo = qj * SB + c2;
  const bool diag = qi == qj;
  const bool two = lo + 1 < p;
  // the S tile, once: rows off + hi, columns off + lo, off + lo + 1 (off, lo and P even: 16-byte
  // aligned; for odd p the pair at lo = p - 1 ends on the row's padding column, which is dropped)
  double2 g[SB / 8];
#pragma unroll
  for (int k = 0; k < SB / 8; ++k) {
    const int hi = qi * SB + rb + 8 * k;
    g[k] = make_double2(0.0, 0.0);
    if (hi < p && lo < p) {
      g[k] = *(const double2*)(A.S + (int64_t)(A.off + hi) * A.P + (A.off + lo));
      if (!two) g[k].y = 0.0;
    }
  }
  __syncthreads();
  const int64_t pp = (int64_t)p * p;
  const double s4 = A.s4, N = A.N;
  for (int i = 0; i < na; ++i) {
    const double ctt = A.ctt[i], k1 = A.k1[i], k2 = A.k2[i], bs = A.bstar[i];
    double* __restrict__ Ji = A.J + i * pp;
    double* __restrict__ Ei = A.sst_exp ? A.sst_exp + i * pp : nullptr;
    double* __restrict__ Si = A.sst_star ? A.sst_star + i * pp : nullptr;
    const double xb0 = xc[i][c2], xb1 = xc[i][c2 + 1], wb0 = wc[i][c2], wb1 = wc[i][c2 + 1];
#pragma unroll
    for (int k = 0; k < SB / 8; ++k) {
      const int r = rb + 8 * k, hi = qi * SB + r;
      const double xa = xr[i][r], wa = wr[i][r];
      const double vx = vx_sse(g[k].x, xa, wa, xb0, wb0, ctt, k1, k2, s4, N);
      const double vy = vx_sse(g[k].y, xa, wa, xb1, wb1, ctt, k1, k2, s4, N);
      T[r][c2] = vx;
      T[r][c2 + 1] = vy;
      if (hi < p && lo < p) {
        // the pair (hi, lo), (hi, lo + 1): by symmetry the column-major entries (lo, hi), (lo + 1, hi)
        const int64_t e = (int64_t)hi * p + lo;
        if (!diag) {   // (an off-diagonal block holds no diagonal entry)
          vx_store(Ji, e, vx, vy, two);
          if (Ei) vx_store(Ei, e, vx, vy, two);
        }
        if (Si) vx_store(Si, e, vx_star(xa, wa, xb0, wb0, ctt, s4), vx_star(xa, wa, xb1, wb1, ctt, s4), two);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SB / 8; ++k) {
      const int r = rb + 8 * k;
      if (diag) {   // entry (r, c) from the lower triangle: (max, min)
        const int hi = qi * SB + r;
        if (hi < p && lo < p) {
          const double x = c2 <= r ? T[r][c2] : T[c2][r];
          const double y = c2 + 1 <= r ? T[r][c2 + 1] : T[c2 + 1][r];
          const int64_t e = (int64_t)hi * p + lo;
          vx_store(Ji, e, hi == lo ? x - bs : x, hi == lo + 1 ? y - bs : y, two);
          if (Ei) vx_store(Ei, e, x, y, two);
        }
      } else {      // the mirror block (qj, qi): row qj SB + r, columns qi SB + c2, c2 + 1
        const int mr = qj * SB + r, mc = qi * SB + c2;
        if (mr < p && mc < p) {
          const bool mtwo = mc + 1 < p;
          const int64_t e = (int64_t)mr * p + mc;
          vx_store(Ji, e, T[c2][r], T[c2 + 1][r], mtwo);
          if (Ei) vx_store(Ei, e, T[c2][r], T[c2 + 1][r], mtwo);
          if (Si) {
            const double xa = xc[i][r], wa = wc[i][r];
            vx_store(Si, e, vx_star(xr[i][c2], wr[i][c2], xa, wa, ctt, s4),
                     vx_star(xr[i][c2 + 1], wr[i][c2 + 1], xa, wa, ctt, s4), mtwo);
          }
        }
      }
    }
    __syncthreads();   // T is rewritten by the next component
  }
}

// The batched form of ppls_symdiag_kernel / ppls_negdiag_kernel (ppls_variances.hip): blockIdx.y = matrix.
__global__ __launch_bounds__(256) void ppls_varfinish_batched_kernel(double* __restrict__ M, int p, int mirror,
                                                                     double* __restrict__ se) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pp = (int64_t)p * p;
  if (e >= pp) return;
  double* Mz = M + (int64_t)blockIdx.y * pp;
  const int b = (int)(e / p), a = (int)(e - (int64_t)b * p);   // element (a, b), column-major
  if (mirror && a < b) Mz[e] = Mz[(int64_t)a * p + b];
  else if (a == b) se[(int64_t)blockIdx.y * p + a] = sqrt(Mz[e]);
}

}  // namespace

extern "C" {

hipError_t ppls_launch_varinfo_batched(const PplsVarinfoArgs* a, hipStream_t st) {
  if (!a || !a->S || !a->cxt || !a->w || !a->J || a->p < 1 || a->a < 1 || a->a > PPLS_RMAX || a->off < 0 ||
      (a->P & 1) || (a->off & 1) || (int64_t)a->off + a->p + (a->p & 1) > a->P || a->ldc < a->p || a->ldw < a->p)
    return hipErrorInvalidValue;
  const int nq = (a->p + SB - 1) / SB;
  hipLaunchKernelGGL(ppls_varinfo_batched_kernel, dim3((unsigned)(nq * (nq + 1) / 2)), dim3(VX_THREADS), 0, st, *a);
  return hipGetLastError();
}

hipError_t ppls_launch_varfinish_batched(double* M, int p, int a, int mirror, double* se, hipStream_t st) {
  if (!M || !se || p < 1 || a < 1) return hipErrorInvalidValue;
  const int64_t pp = (int64_t)p * p;
  hipLaunchKernelGGL(ppls_varfinish_batched_kernel, dim3((unsigned)((pp + 255) / 256), (unsigned)a), dim3(256), 0, st, M,
                     p, mirror, se);
  return hipGetLastError();
}

}  // extern "C"
