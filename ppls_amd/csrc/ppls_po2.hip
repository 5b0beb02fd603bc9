// ppls_po2.hip -- one PO2PLS EM (ECM) iteration from the cross-products S (ppls_po2.h).
//
// The reference states the model (simulC, Package/PPLS/src/loglC.cpp:268-315), its likelihood (loglC,
// :36-113) and its E-step (EMstepC, :116-250) through the dense (p+q) x (p+q) covariance and has no
// M-step (:228).  Here every statistic is a quadratic form in S = [X Y]'[X Y]:
//
//   ppls_po2_panel_kernel   one panel of M = S G (G = blockdiag([W Wo], [C Co])): the X columns of S
//                           against Gx, the Y columns against Gy, each templated on its own width --
//                           the column-tile phase of ppls_xprod.hip (ppls_xprod_phase.h), one read of S
//   ppls_po2_gram_kernel    Q = G'M and the diagonal blocks of G'G, one workgroup per upper-triangle
//                           entry, fixed-order sums, mirrored (exactly symmetric)
//   ppls_po2_small_kernel   one workgroup: Sigma_z^-1, Lambda = Sigma_z^-1 + D G'G, its Cholesky,
//                           Lambda^-1, K = D Lambda^-1, C_zz, Cee, Cff, Chh, the log-likelihood, the stop
//                           rule and the new scalars
//   ppls_po2_update_kernel  the two ECM stages of the loadings per side (W then Wo | C then Co) from
//                           the rows of M, each followed by orth of a tall matrix: Cholesky-QR2
//                           with fixed-order Grams, then ppls_small_polar of R2 R1 or R's QR sign rule
//
// Loadings, scalars, moments and the log-likelihood history stay on the device; the stop rule follows
// ppls_em_run's flag (every kernel returns at once when it is set).
//
// The Gram, small and update kernels are thin wrappers over __device__ bodies that take a PplsPo2Args; their
// batched twins (ppls_po2_*_batch_kernel) read args[blockIdx.y] from a device array and call the
// same bodies, one model per workgroup row, each model with its own stop flag.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppls_device.h"
#include "ppls_po2.h"
#include "ppls_xprod_phase.h"

namespace {

// ---------------------------------------------------------------------------------------------- panel
// A wave owns RW rows of S and walks `width` columns from column soff against the R columns of B; the
// wave's RW x R sums are reduce-scattered and written to Mout (ld P).  Rows past P are dropped.
template <int R, int RW, bool NT>
__global__ __launch_bounds__(64 * ppls_xp_waves(R)) void ppls_po2_panel_kernel(const double* __restrict__ S, int P, int soff,
                                                                                int width, const double* __restrict__ B,
                                                                                int ldb, double* __restrict__ Mout,
                                                                                const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ double sB[2 * R * 128 * ppls_xp_tpb(R)];
  constexpr int NV = RW * R;
  constexpr int LEFT = ppls_rs_left(NV, 0);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t i0 = ((int64_t)blockIdx.x * ppls_xp_waves(R) + wave) * RW;
  const double* srow[RW];
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) srow[rr] = S + (i0 + rr < P ? i0 + rr : (int64_t)P - 1) * P;
  double acc[NV + 1];
#pragma unroll
  for (int v = 0; v <= NV; ++v) acc[v] = 0.0;
  ppls_xprod_tile_phase<R, RW, NT>(srow, B, ldb, width, soff, acc, sB, lane);
  int idx = 0, nreal = 0;
  bool canon = true;
  ppls_rs<NV, 0, NV + 1>(acc, lane, idx, canon, nreal);
  if (canon) {
#pragma unroll
    for (int j = 0; j < LEFT; ++j)
      if (j < nreal && idx + j < NV) {
        const int rr = (idx + j) / R, t = idx + j - rr * R;
        if (i0 + rr < P) Mout[(int64_t)t * P + i0 + rr] = acc[j];
      }
  }
}

constexpr bool po2_nt(int P) { return 8.0 * P * (double)P > 200.0 * (1 << 20); }   // as ppls_xprod.hip's launch_tile

template <int R, int RW>
hipError_t launch_panel(const double* S, int P, int soff, int width, const double* B, int ldb, double* Mout,
                        const int* stop, hipStream_t st) {
  constexpr int NWV = ppls_xp_waves(R);
  const unsigned blocks = (unsigned)((P + NWV * RW - 1) / (NWV * RW));
  if (po2_nt(P))
    hipLaunchKernelGGL((ppls_po2_panel_kernel<R, RW, true>), dim3(blocks), dim3(64 * NWV), 0, st, S, P, soff, width, B, ldb,
                       Mout, stop);
  else
    hipLaunchKernelGGL((ppls_po2_panel_kernel<R, RW, false>), dim3(blocks), dim3(64 * NWV), 0, st, S, P, soff, width, B,
                       ldb, Mout, stop);
  return hipGetLastError();
}

template <int R>
hipError_t launch_panel_rw(int rw, const double* S, int P, int soff, int width, const double* B, int ldb, double* Mout,
                           const int* stop, hipStream_t st) {
  if (rw == 1) return launch_panel<R, 1>(S, P, soff, width, B, ldb, Mout, stop, st);
  if (rw == 2) return launch_panel<R, 2>(S, P, soff, width, B, ldb, Mout, stop, st);
  if (rw == 4) return launch_panel<R, 4>(S, P, soff, width, B, ldb, Mout, stop, st);
  if constexpr (R <= 8)
    if (rw == 8) return launch_panel<R, 8>(S, P, soff, width, B, ldb, Mout, stop, st);
  return hipErrorInvalidValue;
}

// ----------------------------------------------------------------------------------------------- Gram
// Workgroup t: entry (a, b), a <= b, of Q (t < nQ), of Gx'Gx (next nX) or of Gy'Gy (last nY).
__device__ __forceinline__ void po2_tri(int t, int& a, int& b) {
  b = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((b + 1) * (b + 2) / 2 <= t) ++b;
  while (b * (b + 1) / 2 > t) --b;
  a = t - b * (b + 1) / 2;
}

// The body serves ppls_po2_gram_kernel and its batched twin; workgroups past the model's own entry count
// (a batch's grid is as wide as its largest model) return.
__device__ __forceinline__ void po2_gram_body(const PplsPo2Args& g) {
  if (g.stop && *g.stop) return;
  __shared__ double red[4];
  const int kx = g.r + g.rx, ky = g.r + g.ry, k = kx + ky, P = g.ldx + g.ldy;
  const int nQ = k * (k + 1) / 2, nX = kx * (kx + 1) / 2;
  int t = blockIdx.x, a, b, rows, ldo;
  if (t >= nQ + nX + ky * (ky + 1) / 2) return;
  const double *u, *v;
  double* out;
  if (t < nQ) {   // column a of G lives on the X rows (a < kx) or the Y rows
    po2_tri(t, a, b);
    rows = a < kx ? g.ldx : g.ldy;
    u = a < kx ? g.Gx + (int64_t)a * g.ldx : g.Gy + (int64_t)(a - kx) * g.ldy;
    v = (b < kx ? g.M + (int64_t)b * P : g.My + (int64_t)(b - kx) * P) + (a < kx ? 0 : g.ldx);
    out = g.Q;
    ldo = k;
  } else if (t < nQ + nX) {
    po2_tri(t - nQ, a, b);
    rows = g.ldx;
    u = g.Gx + (int64_t)a * g.ldx;
    v = g.Gx + (int64_t)b * g.ldx;
    out = g.GGx;
    ldo = kx;
  } else {
    po2_tri(t - nQ - nX, a, b);
    rows = g.ldy;
    u = g.Gy + (int64_t)a * g.ldy;
    v = g.Gy + (int64_t)b * g.ldy;
    out = g.GGy;
    ldo = ky;
  }
  // four independent partial sums per thread, added in fixed order (as ppls_xprod_gram_kernel)
  double v4[4] = {0.0, 0.0, 0.0, 0.0};
  int i = threadIdx.x;
  for (; i + 3 * 256 < rows; i += 4 * 256) {
#pragma unroll
    for (int w = 0; w < 4; ++w) v4[w] = fma(u[i + w * 256], v[i + w * 256], v4[w]);
  }
  for (; i < rows; i += 256) v4[0] = fma(u[i], v[i], v4[0]);
  double s = (v4[0] + v4[1]) + (v4[2] + v4[3]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double e = (red[0] + red[1]) + (red[2] + red[3]);
    out[(int64_t)b * ldo + a] = e;
    out[(int64_t)a * ldo + b] = e;
  }
}

__global__ __launch_bounds__(256) void ppls_po2_gram_kernel(PplsPo2Args g) { po2_gram_body(g); }
__global__ __launch_bounds__(256) void ppls_po2_gram_batch_kernel(const PplsPo2Args* __restrict__ args) {
  const PplsPo2Args g = args[blockIdx.y];   // wave-uniform: one copy in scalar registers
  po2_gram_body(g);
}

// ---------------------------------------------------------------------------------------------- small
__device__ __forceinline__ bool po2_pos(double v) { return v > 0.0 && isfinite(v); }

// Entry (a, b) of Sigma_z^-1 for z = (t, to | u, uo): block diagonal but for the (t_j, u_j) pairs, whose
// 2 x 2 covariance [[sT^2, sT^2 b], [sT^2 b, sT^2 b^2 + sH^2]] has the inverse
// [[1/sT^2 + b^2/sH^2, -b/sH^2], [-b/sH^2, 1/sH^2]].
__device__ __forceinline__ double po2_sigz_inv(const PplsPo2Scalars& s, int r, int kx, int a, int b) {
  const double iH = 1.0 / (s.sH * s.sH);
  if (a == b) {
    if (a < r) return 1.0 / (s.sT[a] * s.sT[a]) + s.b[a] * s.b[a] * iH;
    if (a < kx) return 1.0 / (s.sTo[a - r] * s.sTo[a - r]);
    if (a < kx + r) return iH;
    return 1.0 / (s.sUo[a - kx - r] * s.sUo[a - kx - r]);
  }
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  if (lo < r && hi == kx + lo) return -s.b[lo] * iH;
  return 0.0;
}

__device__ __forceinline__ void po2_small_body(const PplsPo2Args& g, int pass, int mode, int check) {
  if (g.stop && *g.stop) return;
  constexpr int KM = PPLS_PO2_KMAX;
  __shared__ double sA[KM * KM], sI[KM * KM], sK[KM * KM], sQ[KM * KM], sT[KM * KM], sC[KM * KM];
  __shared__ PplsPo2Scalars sc;
  __shared__ int sfail;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int r = g.r, kx = r + g.rx, ky = r + g.ry, k = kx + ky, kk = k * k;
  for (int e = tid; e < (int)(sizeof(PplsPo2Scalars) / sizeof(double)); e += nt) ((double*)&sc)[e] = ((const double*)g.sc)[e];
  if (tid == 0) sfail = 0;
  __syncthreads();
  if (tid == 0) {
    bool ok = po2_pos(sc.sE) && po2_pos(sc.sF) && po2_pos(sc.sH);
    for (int j = 0; j < r; ++j) ok = ok && po2_pos(sc.sT[j]) && isfinite(sc.b[j]);
    for (int j = 0; j < g.rx; ++j) ok = ok && po2_pos(sc.sTo[j]);
    for (int j = 0; j < g.ry; ++j) ok = ok && po2_pos(sc.sUo[j]);
    if (!ok) sfail = PPLS_PO2_ST_SIGMA;
  }
  __syncthreads();
  const double dE = 1.0 / (sc.sE * sc.sE), dF = 1.0 / (sc.sF * sc.sF);
  if (!sfail) {
    // Lambda = Sigma_z^-1 + D blockdiag(Gx'Gx, Gy'Gy)
    for (int e = tid; e < kk; e += nt) {
      const int a = e % k, b = e / k;
      double v = po2_sigz_inv(sc, r, kx, a, b);
      if (a < kx && b < kx) v += dE * g.GGx[b * kx + a];
      else if (a >= kx && b >= kx) v += dF * g.GGy[(b - kx) * ky + (a - kx)];
      sA[e] = v;
      sQ[e] = g.Q[e];
    }
    // right-looking Cholesky, lower triangle of sA
    for (int j = 0; j < k; ++j) {
      __syncthreads();
      if (tid == 0) {
        double piv = sA[j + j * k];
        if (!po2_pos(piv)) {
          sfail = PPLS_PO2_ST_LAMBDA;
          piv = 1.0;
        }
        sA[j + j * k] = sqrt(piv);
      }
      __syncthreads();
      if (tid > j && tid < k) sA[tid + j * k] /= sA[j + j * k];
      __syncthreads();
      for (int e = tid; e < kk; e += nt) {
        const int i = e % k, m = e / k;
        if (m > j && i >= m) sA[e] -= sA[i + j * k] * sA[m + j * k];
      }
    }
    __syncthreads();
  }
  if (sfail) {   // uniform: nothing is written but the status and the stop flag
    if (tid == 0) {
      if (*g.status == 0) *g.status = sfail;
      if (g.stop) g.stop[0] = pass;
      if (g.stop_mirror) *g.stop_mirror = pass;
      __threadfence_system();
    }
    return;
  }
  // Lambda^-1 by columns: L y = e_c, L' x = y; then mirrored from its lower triangle
  if (tid < k) {
    const int c = tid;
    for (int i = 0; i < c; ++i) sI[i + c * k] = 0.0;
    for (int i = c; i < k; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int m = c; m < i; ++m) s -= sA[i + m * k] * sI[m + c * k];
      sI[i + c * k] = s / sA[i + i * k];
    }
    for (int i = k - 1; i >= 0; --i) {
      double s = sI[i + c * k];
      for (int m = i + 1; m < k; ++m) s -= sA[m + i * k] * sI[m + c * k];
      sI[i + c * k] = s / sA[i + i * k];
    }
  }
  __syncthreads();
  for (int e = tid; e < kk; e += nt) {
    const int a = e % k, b = e / k;
    if (a < b) sI[e] = sI[b + a * k];
  }
  __syncthreads();
  for (int e = tid; e < kk; e += nt) sK[e] = ((e % k) < kx ? dE : dF) * sI[e];   // K = D Lambda^-1
  __syncthreads();
  for (int e = tid; e < kk; e += nt) {   // T = Q K
    const int a = e % k, b = e / k;
    double s = 0.0;
    for (int m = 0; m < k; ++m) s = fma(sQ[a + m * k], sK[m + b * k], s);
    sT[e] = s;
  }
  __syncthreads();
  for (int e = tid; e < kk; e += nt) {   // C_zz = Lambda^-1 + K'(Q K) / N, lower triangle
    const int a = e % k, b = e / k;
    if (a < b) continue;
    double s = 0.0;
    for (int m = 0; m < k; ++m) s = fma(sK[m + a * k], sT[m + b * k], s);
    sC[e] = sI[e] + s / g.N;
  }
  __syncthreads();
  for (int e = tid; e < kk; e += nt) {
    const int a = e % k, b = e / k;
    if (a < b) sC[e] = sC[b + a * k];
  }
  __syncthreads();
  for (int e = tid; e < kk; e += nt) {
    g.sm->Czz[e] = sC[e];
    g.sm->K[e] = sK[e];
  }
  for (int e = tid; e < r * r; e += nt) {   // Chh = Cuu - B Ctu - Cut B + B Ctt B
    const int j = e % r, l = e / r;
    const double cuu = sC[(kx + j) + (kx + l) * k], ctu = sC[j + (kx + l) * k], cut = sC[(kx + j) + l * k];
    g.sm->Chh[e] = cuu - sc.b[j] * ctu - cut * sc.b[l] + sc.b[j] * sC[j + l * k] * sc.b[l];
  }
  __syncthreads();
  if (tid != 0) return;
  double trx = 0.0, try_ = 0.0, trd = 0.0, ggx = 0.0, ggy = 0.0, ldl = 0.0, lds = 0.0, trh = 0.0;
  for (int a = 0; a < kx; ++a) trx += sT[a + a * k];
  for (int a = kx; a < k; ++a) try_ += sT[a + a * k];
  trd = dE * trx + dF * try_;   // tr(Lambda^-1 D Q D) = sum_a d_a (Q K)_aa
  for (int b = 0; b < kx; ++b)
    for (int a = 0; a < kx; ++a) ggx = fma(g.GGx[b * kx + a], sC[b + a * k], ggx);
  for (int b = 0; b < ky; ++b)
    for (int a = 0; a < ky; ++a) ggy = fma(g.GGy[b * ky + a], sC[(kx + b) + (kx + a) * k], ggy);
  const double Cee = (g.ssqX / g.N - 2.0 * trx / g.N + ggx) / (double)g.p;
  const double Cff = (g.ssqY / g.N - 2.0 * try_ / g.N + ggy) / (double)g.q;
  for (int a = 0; a < k; ++a) ldl += log(sA[a + a * k]);
  ldl *= 2.0;
  for (int j = 0; j < r; ++j) lds += 2.0 * log(sc.sT[j]);
  lds += 2.0 * r * log(sc.sH);
  for (int j = 0; j < g.rx; ++j) lds += 2.0 * log(sc.sTo[j]);
  for (int j = 0; j < g.ry; ++j) lds += 2.0 * log(sc.sUo[j]);
  const double pd = (double)g.p, qd = (double)g.q;
  const double ll = -0.5 * g.N * (pd + qd) * log(2.0 * M_PI) -
                    0.5 * g.N * (pd * 2.0 * log(sc.sE) + qd * 2.0 * log(sc.sF) + lds + ldl) -
                    0.5 * (g.ssqX * dE + g.ssqY * dF - trd);
  g.sm->Cee = Cee;
  g.sm->Cff = Cff;
  g.sm->loglik = ll;
  g.sm->logdetL = ldl;
  g.loglik[pass - 1] = ll;
  if (mode == 0) return;
  if (check && pass >= 2) {
    const double inc = ll - g.loglik[pass - 2];
    if (!(inc >= g.atol)) {   // fires on NaN as well (reported through stop[1])
      g.stop[0] = pass;
      g.stop[1] = inc != inc ? 1 : 0;
      if (g.stop_mirror) *g.stop_mirror = pass;
      __threadfence_system();
      return;
    }
  }
  // the new scalars (step 3 of the ECM cycle), refused as a whole if a variance is not positive
  for (int j = 0; j < r; ++j) trh += g.sm->Chh[j + j * r];
  bool ok = po2_pos(Cee) && po2_pos(Cff) && po2_pos(trh);
  for (int j = 0; j < r; ++j) ok = ok && po2_pos(sC[j + j * k]) && isfinite(sC[(kx + j) + j * k]);
  for (int j = 0; j < g.rx; ++j) ok = ok && po2_pos(sC[(r + j) + (r + j) * k]);
  for (int j = 0; j < g.ry; ++j) ok = ok && po2_pos(sC[(kx + r + j) + (kx + r + j) * k]);
  if (!ok) {
    if (*g.status == 0) *g.status = PPLS_PO2_ST_VAR;
    if (g.stop) g.stop[0] = pass;
    if (g.stop_mirror) *g.stop_mirror = pass;
    __threadfence_system();
    return;
  }
  for (int j = 0; j < r; ++j) {
    g.sc->b[j] = sC[(kx + j) + j * k] / sC[j + j * k];
    g.sc->sT[j] = sqrt(sC[j + j * k]);
  }
  for (int j = 0; j < g.rx; ++j) g.sc->sTo[j] = sqrt(sC[(r + j) + (r + j) * k]);
  for (int j = 0; j < g.ry; ++j) g.sc->sUo[j] = sqrt(sC[(kx + r + j) + (kx + r + j) * k]);
  g.sc->sE = sqrt(Cee);
  g.sc->sF = sqrt(Cff);
  g.sc->sH = sqrt(trh / (double)r);
}

__global__ __launch_bounds__(256) void ppls_po2_small_kernel(PplsPo2Args g, int pass, int mode, int check) {
  po2_small_body(g, pass, mode, check);
}
__global__ __launch_bounds__(256) void ppls_po2_small_batch_kernel(const PplsPo2Args* __restrict__ args, int pass, int mode,
                                                                   int check) {
  const PplsPo2Args g = args[blockIdx.y];
  po2_small_body(g, pass, mode, check);
}

// --------------------------------------------------------------------------------------------- update
constexpr int PO2_UT = 1024;   // threads of the loading update's workgroup
constexpr int PO2_C = PPLS_RMAX;

// Gm (c x c, ld PO2_C) = Z'Z for the n x c matrix Z (ld): per column b the threads' strided partial
// sums of (a, b), a <= b, a wave butterfly, then the waves in order: the same bits every run.
__device__ void po2_block_gram(const double* __restrict__ Z, int ld, int n, int c, double* Gm, double* sh) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = 0; b < c; ++b) {
    double acc[PO2_C];
#pragma unroll
    for (int a = 0; a < PO2_C; ++a) acc[a] = 0.0;
    for (int i = tid; i < n; i += PO2_UT) {
      const double zb = Z[(int64_t)b * ld + i];
#pragma unroll
      for (int a = 0; a < PO2_C; ++a)
        if (a <= b) acc[a] = fma(Z[(int64_t)a * ld + i], zb, acc[a]);
    }
#pragma unroll
    for (int a = 0; a < PO2_C; ++a) {
      if (a <= b) {
        double v = acc[a];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) sh[wave * PO2_C + a] = v;
      }
    }
    __syncthreads();
    if (tid <= b) {
      double s = 0.0;
      for (int w = 0; w < PO2_UT / 64; ++w) s += sh[w * PO2_C + tid];
      Gm[tid + b * PO2_C] = s;
      Gm[b + tid * PO2_C] = s;
    }
    __syncthreads();
  }
}

// Lower Cholesky factor of Gm in place (thread 0; ld PO2_C).  false: numerically rank deficient -- a
// pivot at or below 64 c u of its diagonal entry, i.e. a column within rounding of the span of the ones
// before it (Cholesky-QR2 needs kappa^2 u < 1; a pivot that small is rounding noise of the Gram, which
// may come out positive).
__device__ bool po2_chol_serial(double* Gm, int c) {
  for (int j = 0; j < c; ++j) {
    const double gjj = Gm[j + j * PO2_C];
    double d = gjj;
    for (int m = 0; m < j; ++m) d -= Gm[j + m * PO2_C] * Gm[j + m * PO2_C];
    if (!po2_pos(d) || !(d > gjj * (64.0 * c * 1.1102230246251565e-16))) return false;
    d = sqrt(d);
    Gm[j + j * PO2_C] = d;
    for (int i = j + 1; i < c; ++i) {
      double s = Gm[i + j * PO2_C];
      for (int m = 0; m < j; ++m) s -= Gm[i + m * PO2_C] * Gm[j + m * PO2_C];
      Gm[i + j * PO2_C] = s / d;
    }
  }
  return true;
}

// z <- z R^-1 for R = L' (forward substitution along the row), c values in registers.
__device__ __forceinline__ void po2_row_solve(double (&z)[PO2_C], const double* L, int c) {
#pragma unroll
  for (int j = 0; j < PO2_C; ++j) {
    if (j < c) {
      double s = z[j];
#pragma unroll
      for (int m = 0; m < PO2_C; ++m)
        if (m < j) s -= z[m] * L[j + m * PO2_C];
      z[j] = s / L[j + j * PO2_C];
    }
  }
}

// out (n x c, ld) = polar factor of Z (n x c, ld; overwritten): Cholesky-QR2 (Z = Q R2 R1), then
// Q polar(R2 R1).  Every thread returns the same flag (false: rank deficient; out is then untouched).
// qr: instead orth(type = "QR") = sign_e qr.Q(qr(Z)), sign_e = sign(R_11) (functions.R:257-259).  Householder QR
// of Z = Q R (R's diagonal positive, as Cholesky-QR gives it) has the reflectors of Householder QR of Q itself,
// so qr.Q = Q diag(s) with s_k = -sign of the k-th pivot of the reflections applied to Q.  Q's columns stay
// orthonormal under them and column k is zero above row k, so v_k'a_j = -alpha_k a_kj and v_k'v_k = 2 (1 + |a_kk|):
// the pivots follow from Q's top c x c block alone, T_ij += T_ik alpha_k T_kj / (1 + |T_kk|), alpha_k = -sign(T_kk)
// (a last row, n = c, has nothing to reflect: s = sign(T_kk)).
__device__ bool po2_orth_polar(double* __restrict__ Z, int ld, int n, int c, double* __restrict__ out, double* w, int qr) {
  double *L1 = w, *L2 = w + 256, *Rt = w + 512, *Pm = w + 768, *jw = w + 1024, *sh = w + 1536;
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  po2_block_gram(Z, ld, n, c, L1, sh);
  if (tid == 0 && !po2_chol_serial(L1, c)) bad = 1;
  __syncthreads();
  if (bad) return false;
  for (int i = tid; i < n; i += PO2_UT) {
    double z[PO2_C];
#pragma unroll
    for (int j = 0; j < PO2_C; ++j) z[j] = j < c ? Z[(int64_t)j * ld + i] : 0.0;
    po2_row_solve(z, L1, c);
#pragma unroll
    for (int j = 0; j < PO2_C; ++j)
      if (j < c) Z[(int64_t)j * ld + i] = z[j];
  }
  __syncthreads();
  po2_block_gram(Z, ld, n, c, L2, sh);
  if (tid == 0) {
    if (!po2_chol_serial(L2, c)) {
      bad = 1;
    } else if (qr) {
      for (int i = 0; i < c; ++i)   // the top block of Q = Z R2^-1, row by row
        for (int j = 0; j < c; ++j) {
          double s = Z[(int64_t)j * ld + i];
          for (int m = 0; m < j; ++m) s -= Rt[i + m * c] * L2[j + m * PO2_C];
          Rt[i + j * c] = s / L2[j + j * PO2_C];
        }
      double s0 = 1.0;
      for (int k = 0; k < c; ++k) {
        const double akk = Rt[k + k * c];
        const bool last = k == n - 1;
        const double alpha = last ? (akk < 0.0 ? -1.0 : 1.0) : (akk >= 0.0 ? -1.0 : 1.0);
        if (!last) {
          const double f = alpha / (1.0 + fabs(akk));
          for (int j = k + 1; j < c; ++j)
            for (int i = k + 1; i < c; ++i) Rt[i + j * c] += Rt[i + k * c] * f * Rt[k + j * c];
        }
        if (k == 0) s0 = alpha;
        for (int i = 0; i < c; ++i) Pm[i + k * c] = i == k ? s0 * alpha : 0.0;
      }
    } else {
      // R = R2 R1 with R_i = L_i' (upper), column-major ld c for the small polar
      for (int j = 0; j < c; ++j)
        for (int i = 0; i < c; ++i) {
          double s = 0.0;
          for (int m = i; m <= j; ++m) s += L2[m + i * PO2_C] * L1[j + m * PO2_C];
          Rt[i + j * c] = i <= j ? s : 0.0;
        }
      if (ppls_small_polar_ws<PPLS_RMAX>(Rt, c, Pm, jw, jw + 256) != 0) bad = 1;
    }
  }
  __syncthreads();
  if (bad) return false;
  for (int i = tid; i < n; i += PO2_UT) {
    double z[PO2_C];
#pragma unroll
    for (int j = 0; j < PO2_C; ++j) z[j] = j < c ? Z[(int64_t)j * ld + i] : 0.0;
    po2_row_solve(z, L2, c);
    for (int j = 0; j < c; ++j) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < PO2_C; ++m)
        if (m < c) s = fma(z[m], Pm[m + j * c], s);
      out[(int64_t)j * ld + i] = s;
    }
  }
  __syncthreads();
  return true;
}

// Workgroup 0: W <- orth(Cxt - Wo Ctto'), then Wo <- orth(Cxto - W_new Ctto); workgroup 1 the same for
// C, Co with Cuuo.  C_dz = M K / N row by row; the moments are those of the pass (g.sm).
__device__ __forceinline__ void po2_update_body(const PplsPo2Args& g) {
  if (g.stop && *g.stop) return;
  __shared__ double cK[PPLS_PO2_KMAX * PO2_C], cC[PO2_C * PO2_C], w[1536 + (PO2_UT / 64) * PO2_C];
  const int tid = threadIdx.x, side = blockIdx.x;
  const int r = g.r, kx = r + g.rx, k = kx + r + g.ry, P = g.ldx + g.ldy;
  const int n = side ? g.q : g.p, ld = side ? g.ldy : g.ldx, cs = side ? g.ry : g.rx, zoff = side ? kx : 0;
  double* G = side ? g.Gy : g.Gx;
  const double* Mxrow = g.M + (side ? g.ldx : 0);   // this side's rows of the X and Y parts of M
  const double* Myrow = g.My + (side ? g.ldx : 0);
  double* Z = g.Z + (side ? (int64_t)PO2_C * g.ldx : 0);
  for (int stage = 0; stage < 2; ++stage) {
    const int c = stage ? cs : r, koff = zoff + (stage ? r : 0);
    if (c == 0) break;
    const int co = stage ? r : cs;              // columns of the other block of this side
    const double* Go = G + (int64_t)(stage ? 0 : r) * ld;
    __syncthreads();
    for (int e = tid; e < k * c; e += PO2_UT) cK[(e % k) + (e / k) * PPLS_PO2_KMAX] = g.sm->K[(e % k) + (koff + e / k) * k];
    for (int e = tid; e < co * c; e += PO2_UT) {   // cC[m, j]: the coefficient of other column m in new column j
      const int m = e % co, j = e / co;
      cC[m + j * PO2_C] = stage ? g.sm->Czz[(zoff + m) + (zoff + r + j) * k]    // Ctto[m, j]
                                : g.sm->Czz[(zoff + j) + (zoff + r + m) * k];   // Ctto'[m, j] = Ctto[j, m]
    }
    __syncthreads();
    for (int i = tid; i < n; i += PO2_UT) {
      double acc[PO2_C];
#pragma unroll
      for (int j = 0; j < PO2_C; ++j) acc[j] = 0.0;
      for (int a = 0; a < k; ++a) {
        const double mv = a < kx ? Mxrow[(int64_t)a * P + i] : Myrow[(int64_t)(a - kx) * P + i];
#pragma unroll
        for (int j = 0; j < PO2_C; ++j)
          if (j < c) acc[j] = fma(mv, cK[a + j * PPLS_PO2_KMAX], acc[j]);
      }
#pragma unroll
      for (int j = 0; j < PO2_C; ++j) acc[j] /= g.N;
      for (int m = 0; m < co; ++m) {
        const double gv = Go[(int64_t)m * ld + i];
#pragma unroll
        for (int j = 0; j < PO2_C; ++j)
          if (j < c) acc[j] = fma(-gv, cC[m + j * PO2_C], acc[j]);
      }
#pragma unroll
      for (int j = 0; j < PO2_C; ++j)
        if (j < c) Z[(int64_t)j * ld + i] = acc[j];
    }
    __syncthreads();
    if (!po2_orth_polar(Z, ld, n, c, G + (int64_t)(stage ? r : 0) * ld, w, g.type)) {
      if (tid == 0) {
        if (*g.status == 0) *g.status = PPLS_PO2_ST_RANK;
        if (g.stop) g.stop[0] = 1 << 30;
        if (g.stop_mirror) *g.stop_mirror = 1 << 30;
        __threadfence_system();
      }
      return;
    }
  }
}

__global__ __launch_bounds__(PO2_UT) void ppls_po2_update_kernel(PplsPo2Args g) { po2_update_body(g); }
__global__ __launch_bounds__(PO2_UT) void ppls_po2_update_batch_kernel(const PplsPo2Args* __restrict__ args) {
  const PplsPo2Args g = args[blockIdx.y];
  po2_update_body(g);
}

}  // namespace

extern "C" {

int ppls_po2_panel_nt(int P) { return po2_nt(P) ? 1 : 0; }

hipError_t ppls_launch_po2_panel(const double* S, int P, int soff, int width, const double* B, int ldb, int R, int rw,
                                 double* Mout, const int* stop, hipStream_t st) {
  if (P < 2 || (P & 1) || (soff & 1) || (width & 1) || width < 2 || soff < 0 || soff + width > P || (ldb & 1) || ldb < width)
    return hipErrorInvalidValue;
  if (((uintptr_t)S | (uintptr_t)B) & 15) return hipErrorInvalidValue;   // 16-B loads
  switch (R) {
#define PPLS_PO2_CASE(k) \
    case k: return launch_panel_rw<k>(rw, S, P, soff, width, B, ldb, Mout, stop, st);
    PPLS_PO2_CASE(1) PPLS_PO2_CASE(2) PPLS_PO2_CASE(3) PPLS_PO2_CASE(4) PPLS_PO2_CASE(5) PPLS_PO2_CASE(6)
    PPLS_PO2_CASE(7) PPLS_PO2_CASE(8) PPLS_PO2_CASE(9) PPLS_PO2_CASE(10) PPLS_PO2_CASE(11) PPLS_PO2_CASE(12)
    PPLS_PO2_CASE(13) PPLS_PO2_CASE(14) PPLS_PO2_CASE(15) PPLS_PO2_CASE(16)
#undef PPLS_PO2_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t ppls_launch_po2_gram(const PplsPo2Args* a, hipStream_t st) {
  const int kx = a->r + a->rx, ky = a->r + a->ry, k = kx + ky;
  const unsigned n = (unsigned)(k * (k + 1) / 2 + kx * (kx + 1) / 2 + ky * (ky + 1) / 2);
  hipLaunchKernelGGL(ppls_po2_gram_kernel, dim3(n), dim3(256), 0, st, *a);
  return hipGetLastError();
}

hipError_t ppls_launch_po2_small(const PplsPo2Args* a, int pass, int mode, int check, hipStream_t st) {
  if (pass < 1 || (mode && check && !a->stop)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_po2_small_kernel, dim3(1), dim3(256), 0, st, *a, pass, mode, check);
  return hipGetLastError();
}

hipError_t ppls_launch_po2_update(const PplsPo2Args* a, hipStream_t st) {
  hipLaunchKernelGGL(ppls_po2_update_kernel, dim3(2), dim3(PO2_UT), 0, st, *a);
  return hipGetLastError();
}

hipError_t ppls_launch_po2_gram_batch(const PplsPo2Args* args, int m, int max_entries, hipStream_t st) {
  if (!args || m < 1 || m > PPLS_PO2_BATCH_MAX || max_entries < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_po2_gram_batch_kernel, dim3((unsigned)max_entries, (unsigned)m), dim3(256), 0, st, args);
  return hipGetLastError();
}

hipError_t ppls_launch_po2_small_batch(const PplsPo2Args* args, int m, int pass, int mode, int check, hipStream_t st) {
  if (!args || m < 1 || m > PPLS_PO2_BATCH_MAX || pass < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_po2_small_batch_kernel, dim3(1, (unsigned)m), dim3(256), 0, st, args, pass, mode, check);
  return hipGetLastError();
}

hipError_t ppls_launch_po2_update_batch(const PplsPo2Args* args, int m, hipStream_t st) {
  if (!args || m < 1 || m > PPLS_PO2_BATCH_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_po2_update_batch_kernel, dim3(2, (unsigned)m), dim3(PO2_UT), 0, st, args);
  return hipGetLastError();
}

}  // extern "C"
