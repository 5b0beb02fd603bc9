// ppls_rowdiag.hip -- per-row diagnostics of a fitted PPLS_simult model on the device (launch
// interface and the determinism statement: ppls_rowdiag.h; algebra: DESIGN.md §23).
//
//   ppls_rowdiag_kernel   a wave owns RW rows at a time (ppls_rowdiag_rows_per_wave), its lanes the 16-byte
//                         units of a row.  Per block (X with W, then Y with C): phase 1 forms the scores
//                         a_i = W'x_i with the fixed-tree wave reduce-scatter of ppls_cv.hip, phase 2 reads
//                         the same rows again (at the bench shapes past the L2: measured in DESIGN.md
//                         §23), forms the residual x_i - W a_i directly and its squared norm.  Then the
//                         2 x 2 forms of sd2 and, when asked, the posterior means.  The rows are read in
//                         place through an optional index list; nothing is copied and nothing is summed
//                         across waves.
//
// The block order (both phases on X before Y is touched) halves what has to stay cached between a
// block's two phases: the wave's rows of one block, not of both.  fp64 arithmetic on fp64 or fp32
// storage; the residual norm is never formed as ||x||^2 - ||a||^2, which cancels when the fit is good.
//
// Plain HIP: no inline asm, no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ppls_rowdiag.h"

namespace {

template <typename T>
struct Unit16;
template <>
struct Unit16<double> {
  static constexpr int VE = 2;
  static __device__ inline void load(const double* p, double (&o)[2]) {
    const double2 v = *reinterpret_cast<const double2*>(p);
    o[0] = v.x;
    o[1] = v.y;
  }
};
template <>
struct Unit16<float> {
  static constexpr int VE = 4;
  static __device__ inline void load(const float* p, double (&o)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = (double)v.x;
    o[1] = (double)v.y;
    o[2] = (double)v.z;
    o[3] = (double)v.w;
  }
};

template <int VE>
__device__ inline void load_coef(const double* p, double (&o)[VE]) {
#pragma unroll
  for (int e = 0; e < VE; e += 2) {
    const double2 v = *reinterpret_cast<const double2*>(p + e);
    o[e] = v.x;
    o[e + 1] = v.y;
  }
}

// One step of the reduce-scatter over the wave (as in ppls_cv.hip): after H = 32 .. 1, v[0] of lane L
// is the sum of value L over all 64 lanes.  The tree pairs lanes that differ in bit 5, then 4, .. 0,
// for every value alike, and a + b == b + a: the sum does not depend on the slot the value sits in.
template <int H, int NV>
__device__ inline void scatter_step(double (&v)[NV], int lane) {
  if constexpr (NV < 2 * H) return;
  else {
    const bool up = (lane & H) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const double keep = up ? v[i + H] : v[i];
      const double send = up ? v[i] : v[i + H];
      v[i] = keep + __shfl_xor(send, H, 64);
    }
  }
}

__device__ inline double lane_value(double v, int l) {   // l: the same in every lane
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__device__ inline double wave_total(double v) {   // xor tree: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The NV = RW KT values of a wave's row group, reduce-scattered over the lane bits NV / 2 .. 1; then the
// copies that lanes NV apart hold are added over the lane bits 32 .. NV: a fixed tree of six levels.
template <int NV>
__device__ inline double reduce_scores(double (&v)[NV], int lane) {
  scatter_step<32, NV>(v, lane);
  scatter_step<16, NV>(v, lane);
  scatter_step<8, NV>(v, lane);
  scatter_step<4, NV>(v, lane);
  scatter_step<2, NV>(v, lane);
  scatter_step<1, NV>(v, lane);
  double t = v[0];
#pragma unroll
  for (int o = 32; o >= NV; o >>= 1) t += __shfl_xor(t, o, 64);
  return t;
}

// Phase 1 of a block: every lane L with L % (RW KT) == rr * KT + m returns row rr's score against column m
// of A (0 for m >= k).
template <typename T, int KT, int RW>
__device__ inline double block_scores(const T* __restrict__ X, int64_t ld, const int64_t (&idx)[RW], int nu, int ld4,
                                      const double* __restrict__ A, int k, int lane) {
  constexpr int NV = RW * KT, VE = Unit16<T>::VE;
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0;
  for (int ch = lane; ch < nu; ch += 64) {
    double xv[RW][VE];
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) Unit16<T>::load(X + idx[rr] * ld + (int64_t)ch * VE, xv[rr]);
#pragma unroll
    for (int m = 0; m < KT; ++m) {
      if (m < k) {
        double a[VE];
        load_coef<VE>(A + (int64_t)m * ld4 + (int64_t)ch * VE, a);
#pragma unroll
        for (int rr = 0; rr < RW; ++rr)
#pragma unroll
          for (int e = 0; e < VE; ++e) v[rr * KT + m] += xv[rr][e] * a[e];
      }
    }
  }
  return reduce_scores<NV>(v, lane);
}

// Phase 2 of a block: r2[rr] = ||x_rr - sum_m t_rr,m a_m||^2 in every lane, t from block_scores.  The
// loop's trip count is the same in every lane and lanes past the row's end are masked, not branched
// out: the scores are read from other lanes (lane_value), which needs those lanes active.
template <typename T, int KT, int RW>
__device__ inline void block_resid(const T* __restrict__ X, int64_t ld, const int64_t (&idx)[RW], int nu, int ld4,
                                   const double* __restrict__ A, int k, double t, int lane, double (&r2)[RW]) {
  constexpr int VE = Unit16<T>::VE;
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) r2[rr] = 0.0;
  for (int base = 0; base < nu; base += 64) {
    const bool act = base + lane < nu;
    const int ch = act ? base + lane : 0;
    double x[RW][VE];
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) Unit16<T>::load(X + idx[rr] * ld + (int64_t)ch * VE, x[rr]);
#pragma unroll
    for (int m = 0; m < KT; ++m) {
      if (m < k) {
        double a[VE];
        load_coef<VE>(A + (int64_t)m * ld4 + (int64_t)ch * VE, a);
#pragma unroll
        for (int rr = 0; rr < RW; ++rr) {
          const double trm = lane_value(t, rr * KT + m);
#pragma unroll
          for (int e = 0; e < VE; ++e) x[rr][e] -= trm * a[e];
        }
      }
    }
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      double s = 0.0;
#pragma unroll
      for (int e = 0; e < VE; ++e) s += x[rr][e] * x[rr][e];
      r2[rr] += act ? s : 0.0;
    }
  }
#pragma unroll
  for (int rr = 0; rr < RW; ++rr) r2[rr] = wave_total(r2[rr]);
}

template <typename T, int KT, int RW, bool MU>
__global__ __launch_bounds__(64 * PPLS_ROWDIAG_WAVES) void ppls_rowdiag_kernel(
    const T* __restrict__ X, int64_t lda, int pa, const T* __restrict__ Y, int64_t ldb, int qb,
    const int64_t* __restrict__ rows, int64_t nrows, const double* __restrict__ W, const double* __restrict__ C,
    const double* __restrict__ coef, int k, double* __restrict__ odx2, double* __restrict__ ody2,
    double* __restrict__ sd2, double* __restrict__ mu_T, double* __restrict__ mu_U, int64_t ldmu) {
  constexpr int NV = RW * KT, VE = Unit16<T>::VE;
  static_assert(NV <= 64 && (NV & (NV - 1)) == 0, "a wave's row group holds a power of two of at most 64 scores");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * PPLS_ROWDIAG_WAVES + wave, nw = (int64_t)gridDim.x * PPLS_ROWDIAG_WAVES;
  const int64_t ngroups = (nrows + RW - 1) / RW;
  const int lda4 = (pa + 3) & ~3, ldb4 = (qb + 3) & ~3;
  const int na = (pa + VE - 1) / VE, nb = (qb + VE - 1) / VE;   // 16-byte units holding real columns
  // lane L ends up with the scores of (row (L % NV) / KT, component L % KT); lanes < NV write
  const int m = lane & (KT - 1), myrr = (lane & (NV - 1)) / KT;
  const bool on = m < k;
  const double s11 = on ? coef[0 * 16 + m] : 1.0, s12 = on ? coef[1 * 16 + m] : 0.0;
  const double s22 = on ? coef[2 * 16 + m] : 1.0, det = on ? coef[3 * 16 + m] : 1.0;
  double al = 0.0, be = 0.0, ga = 0.0, de = 0.0;
  if (MU && on) {
    al = coef[4 * 16 + m];
    be = coef[5 * 16 + m];
    ga = coef[6 * 16 + m];
    de = coef[7 * 16 + m];
  }

  for (int64_t g = gw; g < ngroups; g += nw) {
    const int64_t i0 = g * RW;
    const int nvalid = (int)(nrows - i0 < RW ? nrows - i0 : RW);
    int64_t idx[RW];
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      const int64_t i = i0 + (rr < nvalid ? rr : 0);   // rows past the end repeat the first: read, not written
      idx[rr] = rows ? rows[i] : i;
    }
    double rx[RW], ry[RW];
    const double ta = block_scores<T, KT, RW>(X, lda, idx, na, lda4, W, k, lane);
    block_resid<T, KT, RW>(X, lda, idx, na, lda4, W, k, ta, lane, rx);
    const double tb = block_scores<T, KT, RW>(Y, ldb, idx, nb, ldb4, C, k, lane);
    block_resid<T, KT, RW>(Y, ldb, idx, nb, ldb4, C, k, tb, lane, ry);
    // the component's 2 x 2 form, then a fixed tree over the tile (components >= k add exact zeros)
    double sd = on ? ((s22 * (ta * ta) - 2.0 * s12 * (ta * tb)) + s11 * (tb * tb)) / det : 0.0;
#pragma unroll
    for (int o = KT / 2; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
    double ox = 0.0, oy = 0.0;
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      if (rr == myrr) {
        ox = rx[rr];
        oy = ry[rr];
      }
    }
    if (lane < NV && myrr < nvalid) {
      const int64_t o = i0 + myrr;
      if (m == 0) {
        odx2[o] = ox;
        ody2[o] = oy;
        sd2[o] = sd;
      }
      if (MU && on) {
        mu_T[(int64_t)m * ldmu + o] = al * ta + be * tb;
        mu_U[(int64_t)m * ldmu + o] = ga * ta + de * tb;
      }
    }
  }
}

template <typename T>
hipError_t rowdiag_launch(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, const int64_t* rows,
                          int64_t nrows, const double* W, const double* C, const double* coef, int k, double* odx2,
                          double* ody2, double* sd2, double* mu_T, double* mu_U, int64_t ldmu, int grid, hipStream_t st) {
  const dim3 g(grid), b(64 * PPLS_ROWDIAG_WAVES);
  const int rw = ppls_rowdiag_rows_per_wave(pa, qb, sizeof(T) == 4, k);
#define PPLS_ROWDIAG_GO(KT, RW, MU)                                                                                \
  hipLaunchKernelGGL((ppls_rowdiag_kernel<T, KT, RW, MU>), g, b, 0, st, (const T*)X, lda, pa, (const T*)Y, ldb, qb, \
                     rows, nrows, W, C, coef, k, odx2, ody2, sd2, mu_T, mu_U, ldmu)
#define PPLS_ROWDIAG_MU(KT, RW)              \
  do {                                       \
    if (mu_T) PPLS_ROWDIAG_GO(KT, RW, true); \
    else PPLS_ROWDIAG_GO(KT, RW, false);     \
  } while (0)
  if (k > 8) PPLS_ROWDIAG_MU(16, PPLS_ROWDIAG_ROWS16);
  else if (rw == PPLS_ROWDIAG_ROWS8_SHORT) PPLS_ROWDIAG_MU(8, PPLS_ROWDIAG_ROWS8_SHORT);
  else PPLS_ROWDIAG_MU(8, PPLS_ROWDIAG_ROWS8);
#undef PPLS_ROWDIAG_MU
#undef PPLS_ROWDIAG_GO
  return hipGetLastError();
}

}  // namespace

extern "C" {

int ppls_rowdiag_rows_per_wave(int pa, int qb, int f32, int k) {
  if (k > 8) return PPLS_ROWDIAG_ROWS16;
  const int64_t row_bytes = (int64_t)std::max(pa, qb) * (f32 ? 4 : 8);
  return row_bytes <= PPLS_ROWDIAG_SHORT_BYTES ? PPLS_ROWDIAG_ROWS8_SHORT : PPLS_ROWDIAG_ROWS8;
}

int ppls_rowdiag_grid(int64_t nrows, int pa, int qb, int f32, int k, int num_cus) {
  const int rw = ppls_rowdiag_rows_per_wave(pa, qb, f32, k);
  const int64_t per = (int64_t)rw * PPLS_ROWDIAG_WAVES;
  const int64_t blocks = (nrows + per - 1) / per, cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 4;
  return (int)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

hipError_t ppls_launch_rowdiag(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, int f32,
                               const int64_t* rows, int64_t nrows, const double* W, const double* C,
                               const double* coef, int k, double* odx2, double* ody2, double* sd2, double* mu_T,
                               double* mu_U, int64_t ldmu, int grid, hipStream_t st) {
  if (k < 1 || k > 16 || grid < 1 || nrows < 0 || pa < 1 || qb < 1) return hipErrorInvalidValue;
  if (!X || !Y || !W || !C || !coef || !odx2 || !ody2 || !sd2) return hipErrorInvalidValue;
  if ((mu_T == nullptr) != (mu_U == nullptr) || (mu_T && ldmu < nrows)) return hipErrorInvalidValue;
  const int ve = f32 ? 4 : 2;   // a row holds whole 16-byte units of real columns
  if (lda < (int64_t)(pa + ve - 1) / ve * ve || ldb < (int64_t)(qb + ve - 1) / ve * ve || lda % ve || ldb % ve)
    return hipErrorInvalidValue;
  if (nrows == 0) return hipSuccess;
  if (f32)
    return rowdiag_launch<float>(X, lda, pa, Y, ldb, qb, rows, nrows, W, C, coef, k, odx2, ody2, sd2, mu_T, mu_U, ldmu,
                                 grid, st);
  return rowdiag_launch<double>(X, lda, pa, Y, ldb, qb, rows, nrows, W, C, coef, k, odx2, ody2, sd2, mu_T, mu_U, ldmu,
                                grid, st);
}

}  // extern "C"
