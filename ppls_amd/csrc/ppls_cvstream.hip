// ppls_cvstream.hip -- kernels of cross-validation on streamed data (launch interface:
// ppls_cvstream.h).
//
//   ppls_cvs_diag_kernel      the diagonal of sum_k (S_k recentred to the global mean), in fold order:
//                             what the scale d_j = sqrt(. / (N - 1)) is formed from.
//   ppls_cvs_finish_kernel    one 64 x 64 block of the lower triangle of one fold matrix per workgroup:
//                             S_k,ij <- (S_k,ij + (N_k e_ki) e_kj) / (d_i d_j), recentring and
//                             standardising in one pass: ppls_symtile_pass (ppls_symtile.h, the walk
//                             ppls_stream_tile_kernel uses) around that update.
//   ppls_cvs_select_kernel    working S = the fold matrices but one (or all), added in fold order.
//   ppls_cvs_rows_kernel      held-out error, pass over the X rows of S_k: a wave per row i forms
//                             (S_xx W)_i. and (S_xy C)_i. and the same sums of absolute values.
//   ppls_cvs_sse_kernel       A = W'(S_xx W), D, G = C'C, tr(S_yy) and the k prefix sums, one workgroup.
//
// Plain HIP, vector stores only.  Every entry and every sum is one fixed chain of operations.
#include <hip/hip_runtime.h>

#include "ppls_cvstream.h"
#include "ppls_symtile.h"

namespace {

constexpr int SB = PPLS_SYM_SB;
constexpr int CT = PPLS_SYM_THREADS;
using CvsCols = PplsSymCols;

// the recentring term, formed in one place: S + (w e_i) e_j with a single rounding of the sum
__device__ inline double recentred(double s, double we_i, double e_j) { return fma(we_i, e_j, s); }

__global__ __launch_bounds__(CT) void ppls_cvs_diag_kernel(const double* __restrict__ S, int K, CvsCols g,
                                                          const double* __restrict__ e, const double* __restrict__ w,
                                                          double* __restrict__ dsum) {
  const int j = blockIdx.x * CT + threadIdx.x;
  if (j >= g.P) return;
  double acc = 0.0;
  if (ppls_sym_col_live(g, j)) {
    const int64_t PP = (int64_t)g.P * g.P;
    for (int k = 0; k < K; ++k) {
      const double ej = e[(int64_t)k * g.P + j];
      acc += recentred(S[k * PP + (int64_t)j * g.P + j], w[k] * ej, ej);
    }
  }
  dsum[j] = acc;
}

// (S_ij + (N_k e_i) e_j) / (d_i d_j); staged vector 0 is the fold's e, 1 is d
struct CvsFinish {
  double w;
  __device__ double2 operator()(double2 v, int r, int c2, const double (&a)[2][SB], const double (&b)[2][SB]) const {
    const double wa = w * a[0][r];
    v.x = recentred(v.x, wa, b[0][c2]) / (a[1][r] * b[1][c2]);
    v.y = recentred(v.y, wa, b[0][c2 + 1]) / (a[1][r] * b[1][c2 + 1]);
    return v;
  }
};

__global__ __launch_bounds__(CT) void ppls_cvs_finish_kernel(double* __restrict__ Sall, CvsCols g,
                                                            const double* __restrict__ eall,
                                                            const double* __restrict__ wall,
                                                            const double* __restrict__ d) {
  const int fold = blockIdx.y;
  const double* const v[2] = {eall + (int64_t)fold * g.P, d};
  ppls_symtile_pass<2>(Sall + (int64_t)fold * g.P * g.P, g, ppls_sym_block(blockIdx.x), v, {0.0, 1.0},
                       CvsFinish{wall[fold]});
}

__global__ __launch_bounds__(CT) void ppls_cvs_select_kernel(const double2* __restrict__ S, int K, int skip, int64_t len2,
                                                            double2* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x; i < len2; i += (int64_t)gridDim.x * CT) {
    double2 acc = make_double2(0.0, 0.0);
    for (int l = 0; l < K; ++l) {
      if (l == skip) continue;
      const double2 v = S[l * len2 + i];
      acc.x += v.x;
      acc.y += v.y;
    }
    out[i] = acc;
  }
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// work[i * 4k + {0, k, 2k, 3k} + m] = (S_xx W)_im, (|S_xx| |W|)_im, (S_xy C)_im, (|S_xy| |C|)_im
__global__ __launch_bounds__(CT) void ppls_cvs_rows_kernel(const double* __restrict__ Sk, int P, int p, int ldx, int q,
                                                          const double* __restrict__ W, const double* __restrict__ C,
                                                          int k, double* __restrict__ work) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  if (i >= p) return;   // (whole waves leave; no barrier below)
  const double* srow = Sk + (int64_t)i * P;
  const int ldw = (p + 3) & ~3, ldc = (q + 3) & ~3;
  double acc[4][PPLS_CVS_KMAX];
#pragma unroll
  for (int m = 0; m < PPLS_CVS_KMAX; ++m) acc[0][m] = acc[1][m] = acc[2][m] = acc[3][m] = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double* s0 = srow + (h ? ldx : 0);
    const double* M = h ? C : W;
    const int n2 = ((h ? q : p) + 1) / 2, ld = h ? ldc : ldw;
    for (int ch = lane; ch < n2; ch += 64) {
      const double2 s = *(const double2*)(s0 + 2 * ch);
#pragma unroll
      for (int m = 0; m < PPLS_CVS_KMAX; ++m) {
        if (m < k) {
          const double2 c = *(const double2*)(M + (int64_t)m * ld + 2 * ch);
          acc[2 * h][m] += s.x * c.x + s.y * c.y;
          acc[2 * h + 1][m] += fabs(s.x) * fabs(c.x) + fabs(s.y) * fabs(c.y);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < PPLS_CVS_KMAX; ++m) {
    if (m < k) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double tot = wave_sum(acc[a][m]);
        if (lane == 0) work[(int64_t)i * 4 * k + a * k + m] = tot;
      }
    }
  }
}

__global__ __launch_bounds__(CT) void ppls_cvs_sse_kernel(const double* __restrict__ Sk, int P, int p, int ldx, int q,
                                                         const double* __restrict__ W, const double* __restrict__ C,
                                                         const double* __restrict__ B, int k,
                                                         const double* __restrict__ work, double* __restrict__ sse,
                                                         double* __restrict__ mag) {
  constexpr int KM = PPLS_CVS_KMAX;
  __shared__ double sA[KM][KM], sAm[KM][KM], sG[KM][KM], sGm[KM][KM], sD[KM], sDm[KM], sTr;
  const int m = threadIdx.x / KM, l = threadIdx.x % KM;
  const int ldw = (p + 3) & ~3, ldc = (q + 3) & ~3;
  if (m < k && l < k) {
    double a = 0.0, am = 0.0, d = 0.0, dm = 0.0, gg = 0.0, gm = 0.0;
    for (int i = 0; i < p; ++i) {
      const double w = W[(int64_t)m * ldw + i];
      const double* r = work + (int64_t)i * 4 * k;
      a += w * r[l];
      am += fabs(w) * r[k + l];
      if (m == l) {
        d += w * r[2 * k + m];
        dm += fabs(w) * r[3 * k + m];
      }
    }
    for (int j = 0; j < q; ++j) {
      const double x = C[(int64_t)m * ldc + j] * C[(int64_t)l * ldc + j];
      gg += x;
      gm += fabs(x);
    }
    sA[m][l] = a;
    sAm[m][l] = am;
    sG[m][l] = gg;
    sGm[m][l] = gm;
    if (m == l) {
      sD[m] = d;
      sDm[m] = dm;
    }
  }
  if (threadIdx.x == CT - 1) {   // tr(S_yy), in column order
    double tr = 0.0;
    for (int j = 0; j < q; ++j) tr += Sk[(int64_t)(ldx + j) * P + ldx + j];
    sTr = tr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 0; j < k; ++j) {
      double lin = 0.0, linm = 0.0, quad = 0.0, quadm = 0.0;
      for (int a = 0; a <= j; ++a) {
        lin += B[a] * sD[a];
        linm += fabs(B[a]) * sDm[a];
        for (int b = 0; b <= j; ++b) {
          quad += (B[a] * B[b]) * (sA[a][b] * sG[a][b]);
          quadm += fabs(B[a] * B[b]) * (sAm[a][b] * sGm[a][b]);
        }
      }
      sse[j] = (sTr - 2.0 * lin) + quad;
      mag[j] = (fabs(sTr) + 2.0 * linm) + quadm;
    }
  }
}

bool shape_ok(int K, int p, int ldx, int q, int ldy) { return K >= 1 && K <= 65535 && ppls_sym_shape_ok(p, ldx, q, ldy); }

}  // namespace

extern "C" {

hipError_t ppls_launch_cvs_diag(const double* S, int K, int p, int ldx, int q, int ldy, const double* e,
                                const double* w, double* dsum, hipStream_t st) {
  if (!S || !e || !w || !dsum || !shape_ok(K, p, ldx, q, ldy)) return hipErrorInvalidValue;
  const int P = ldx + ldy;
  const CvsCols g{P, p, ldx, ldx + q};
  hipLaunchKernelGGL(ppls_cvs_diag_kernel, dim3((P + CT - 1) / CT), dim3(CT), 0, st, S, K, g, e, w, dsum);
  return hipGetLastError();
}

hipError_t ppls_launch_cvs_finish(double* S, int K, int p, int ldx, int q, int ldy, const double* e,
                                  const double* w, const double* d, hipStream_t st) {
  if (!S || !e || !w || !d || !shape_ok(K, p, ldx, q, ldy)) return hipErrorInvalidValue;
  const int P = ldx + ldy;
  const CvsCols g{P, p, ldx, ldx + q};
  hipLaunchKernelGGL(ppls_cvs_finish_kernel, dim3(ppls_sym_blocks(P), K), dim3(CT), 0, st, S, g, e, w, d);
  return hipGetLastError();
}

hipError_t ppls_launch_cvs_select(const double* S, int K, int skip, int64_t PP, double* out, hipStream_t st) {
  if (!S || !out || K < 1 || skip < -1 || skip >= K || PP < 2 || (PP & 1)) return hipErrorInvalidValue;
  const int64_t len2 = PP / 2, blocks = (len2 + CT - 1) / CT;
  hipLaunchKernelGGL(ppls_cvs_select_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(CT), 0, st,
                     (const double2*)S, K, skip, len2, (double2*)out);
  return hipGetLastError();
}

hipError_t ppls_launch_cvs_heldout(const double* Sk, int p, int ldx, int q, int ldy, const double* W, const double* C,
                                   const double* B, int k, double* work, double* sse, double* mag, hipStream_t st) {
  if (!Sk || !W || !C || !B || !work || !sse || !mag || k < 1 || k > PPLS_CVS_KMAX || !shape_ok(1, p, ldx, q, ldy))
    return hipErrorInvalidValue;
  const int P = ldx + ldy, wpb = CT / 64;
  hipLaunchKernelGGL(ppls_cvs_rows_kernel, dim3((p + wpb - 1) / wpb), dim3(CT), 0, st, Sk, P, p, ldx, q, W, C, k, work);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ppls_cvs_sse_kernel, dim3(1), dim3(CT), 0, st, Sk, P, p, ldx, q, W, C, B, k, work, sse, mag);
  return hipGetLastError();
}

}  // extern "C"
