// ppls_cv.hip -- the kernels under predict.PPLS / cv_PPLS / crossval_PPLS on the device
// (Package/PPLS/R/crossval_PPLS.R:12-114; launch interface: ppls_cv.h).
//
//   ppls_gather_rows_kernel   dst row i = src row rows[i]: whole rows, 16-byte loads and stores along
//                             a row, the destination's padding zeroed.  R's X[-folds[ii], ] (:48)
//                             without the host round trip.
//   ppls_downdate_kernel      S_train = S - S_out over the padded (ldx + ldy)^2 layout.
//   ppls_cv_score_kernel      predict(fit, X[fold, ], "X") (:19-21) and the residual of :49 in one
//                             pass: t_i = x_i W, then either the prediction row sum_m t_im B_m c_m or,
//                             for every prefix j of the components, ||y_i - sum_{m<=j} t_im B_m c_m||^2.
//                             fp64 arithmetic on fp64 or fp32 storage; the residual is formed directly
//                             (no ||Y||^2 - 2 tr + tr expansion, which cancels when the fit is good).
//
// Plain HIP: no inline asm, no LDS-DMA.  Every sum has a fixed order for a given grid.
#include <hip/hip_runtime.h>

#include "ppls_cv.h"

namespace {

// ------------------------------------------------------------------------------ row gather
// 2^lg threads share a row (lg chosen by the launcher from the row length), so short rows do not
// leave most of a workgroup idle and long rows (16 KB at C3, 40 KB at C5) are read by whole waves.
__global__ __launch_bounds__(256) void ppls_gather_rows_kernel(const uint4* __restrict__ src, int64_t src16,
                                                               uint4* __restrict__ dst, int64_t dst16, int copy16,
                                                               const int64_t* __restrict__ rows, int64_t nrows,
                                                               int lg) {
  const int tpr = 1 << lg, sub = threadIdx.x & (tpr - 1);
  const int64_t rpb = 256 >> lg;
  for (int64_t r = (int64_t)blockIdx.x * rpb + (threadIdx.x >> lg); r < nrows; r += (int64_t)gridDim.x * rpb) {
    const uint4* s = src + rows[r] * src16;
    uint4* d = dst + r * dst16;
    for (int c = sub; c < (int)dst16; c += tpr) d[c] = c < copy16 ? s[c] : make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ __launch_bounds__(256) void ppls_downdate_kernel(const double2* __restrict__ a, const double2* __restrict__ b,
                                                            double2* __restrict__ out, int64_t len2) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len2; i += (int64_t)gridDim.x * 256) {
    const double2 x = a[i], y = b[i];
    out[i] = make_double2(x.x - y.x, x.y - y.y);
  }
}

// ------------------------------------------------------------------------------ scoring
template <typename T>
struct Row16;
template <>
struct Row16<double> {
  static constexpr int VE = 2;
  static __device__ inline void load(const double* p, double (&o)[2]) {
    const double2 v = *reinterpret_cast<const double2*>(p);
    o[0] = v.x;
    o[1] = v.y;
  }
};
template <>
struct Row16<float> {
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

// One step of the reduce-scatter over the wave: lanes with bit H set keep the upper H values, the
// others the lower H, each adding its partner's.  After H = 32 .. 1, v[0] of lane L is the sum of
// value L over all 64 lanes, added in a fixed tree.
template <int H>
__device__ inline void scatter_step(double (&v)[64], int lane) {
  const bool up = (lane & H) != 0;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const double keep = up ? v[i + H] : v[i];
    const double send = up ? v[i] : v[i + H];
    v[i] = keep + __shfl_xor(send, H, 64);
  }
}

__device__ inline double lane_value(double v, int l) {   // l: the same in every lane
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__device__ inline double wave_total(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A wave owns RW = 64 / KT rows at a time (so the loadings' 16-byte column slices are read from
// cache once per RW rows, by the four waves of a workgroup for 4 RW adjacent rows), its lanes the
// 16-byte units of a row.
template <typename T, int KT, bool PRED>
__global__ __launch_bounds__(64 * PPLS_CV_WAVES) void ppls_cv_score_kernel(
    const T* __restrict__ X, int64_t lda, int pa, const T* __restrict__ Y, int64_t ldb, int qb,
    const int64_t* __restrict__ rows, int64_t nrows, const double* __restrict__ A, const double* __restrict__ Bm,
    const double* __restrict__ s, int k, double* __restrict__ part, double* __restrict__ pred, int64_t ldo) {
  constexpr int RW = 64 / KT, VE = Row16<T>::VE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * PPLS_CV_WAVES + wave, nw = (int64_t)gridDim.x * PPLS_CV_WAVES;
  const int64_t ngroups = (nrows + RW - 1) / RW;
  const int lda4 = (pa + 3) & ~3, ldb4 = (qb + 3) & ~3;
  const int na = (pa + VE - 1) / VE, nb = (qb + VE - 1) / VE;   // 16-byte units holding real columns
  double sse[KT];
#pragma unroll
  for (int m = 0; m < KT; ++m) sse[m] = 0.0;
  const double sm = (lane & (KT - 1)) < k ? s[lane & (KT - 1)] : 0.0;   // lane L ends up with value (L / KT, L % KT)

  for (int64_t g = gw; g < ngroups; g += nw) {
    const int64_t i0 = g * RW;
    const int nvalid = (int)(nrows - i0 < RW ? nrows - i0 : RW);
    int64_t idx[RW];
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      const int64_t i = i0 + (rr < nvalid ? rr : 0);   // rows past the end repeat the first: read, not used
      idx[rr] = rows ? rows[i] : i;
    }
    // scores: v[rr * KT + m] = this lane's part of x_rr . a_m
    double v[64];
#pragma unroll
    for (int e = 0; e < 64; ++e) v[e] = 0.0;
    for (int ch = lane; ch < na; ch += 64) {
      double xv[RW][VE];
#pragma unroll
      for (int rr = 0; rr < RW; ++rr) Row16<T>::load(X + idx[rr] * lda + (int64_t)ch * VE, xv[rr]);
#pragma unroll
      for (int m = 0; m < KT; ++m) {
        if (m < k) {
          double a[VE];
          load_coef<VE>(A + (int64_t)m * lda4 + (int64_t)ch * VE, a);
#pragma unroll
          for (int rr = 0; rr < RW; ++rr)
#pragma unroll
            for (int e = 0; e < VE; ++e) v[rr * KT + m] += xv[rr][e] * a[e];
        }
      }
    }
    scatter_step<32>(v, lane);
    scatter_step<16>(v, lane);
    scatter_step<8>(v, lane);
    scatter_step<4>(v, lane);
    scatter_step<2>(v, lane);
    scatter_step<1>(v, lane);
    const double t = v[0] * sm;   // lane rr * KT + m: t_rr,m s_m
    // second factor: lanes over the 16-byte units of the output / response row.  The loop's trip
    // count is the same in every lane and lanes past the row's end are masked, not branched out:
    // the scores are read from other lanes (lane_value), which needs those lanes active.
    for (int base = 0; base < nb; base += 64) {
      const bool act = base + lane < nb;
      const int ch = act ? base + lane : 0;
      double y[RW][VE];
#pragma unroll
      for (int rr = 0; rr < RW; ++rr) {
        if (PRED) {
#pragma unroll
          for (int e = 0; e < VE; ++e) y[rr][e] = 0.0;
        } else {
          Row16<T>::load(Y + idx[rr] * ldb + (int64_t)ch * VE, y[rr]);
        }
      }
#pragma unroll
      for (int m = 0; m < KT; ++m) {
        if (m < k) {
          double b[VE];
          load_coef<VE>(Bm + (int64_t)m * ldb4 + (int64_t)ch * VE, b);
          double r2 = 0.0;
#pragma unroll
          for (int rr = 0; rr < RW; ++rr) {
            const double trm = lane_value(t, rr * KT + m);
            if (rr < nvalid) {
#pragma unroll
              for (int e = 0; e < VE; ++e) {
                if (PRED) {
                  y[rr][e] += trm * b[e];
                } else {
                  y[rr][e] -= trm * b[e];
                  r2 += y[rr][e] * y[rr][e];
                }
              }
            }
          }
          sse[m] += act ? r2 : 0.0;
        }
      }
      if (PRED && act) {
#pragma unroll
        for (int rr = 0; rr < RW; ++rr)
          if (rr < nvalid)
            *reinterpret_cast<double2*>(pred + (i0 + rr) * ldo + (int64_t)ch * 2) = make_double2(y[rr][0], y[rr][1]);
      }
    }
  }
  if (!PRED) {
#pragma unroll
    for (int m = 0; m < KT; ++m) {
      if (m < k) {
        const double tot = wave_total(sse[m]);
        if (lane == 0) part[gw * k + m] = tot;
      }
    }
  }
}

__global__ __launch_bounds__(256) void ppls_cv_sse_reduce_kernel(const double* __restrict__ part, int nparts, int k,
                                                                 double* __restrict__ sse) {
  __shared__ double sh[256];
  const int per = (nparts + 255) / 256;
  for (int m = 0; m < k; ++m) {
    double acc = 0.0;
    const int b = threadIdx.x * per, e = b + per < nparts ? b + per : nparts;
    for (int i = b; i < e; ++i) acc += part[(int64_t)i * k + m];
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;
      for (int i = 0; i < 256; ++i) tot += sh[i];
      sse[m] = tot;
    }
    __syncthreads();
  }
}

template <typename T, bool PRED>
hipError_t score_launch(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, const int64_t* rows,
                        int64_t nrows, const double* A, const double* Bm, const double* s, int k, double* part,
                        double* pred, int64_t ldo, int grid, hipStream_t st) {
  if (k <= 8)
    hipLaunchKernelGGL((ppls_cv_score_kernel<T, 8, PRED>), dim3(grid), dim3(64 * PPLS_CV_WAVES), 0, st, (const T*)X, lda,
                       pa, (const T*)Y, ldb, qb, rows, nrows, A, Bm, s, k, part, pred, ldo);
  else
    hipLaunchKernelGGL((ppls_cv_score_kernel<T, 16, PRED>), dim3(grid), dim3(64 * PPLS_CV_WAVES), 0, st, (const T*)X,
                       lda, pa, (const T*)Y, ldb, qb, rows, nrows, A, Bm, s, k, part, pred, ldo);
  return hipGetLastError();
}

}  // namespace

extern "C" {

hipError_t ppls_launch_gather_rows(const void* src, int64_t src16, void* dst, int64_t dst16, int copy16,
                                   const int64_t* rows, int64_t nrows, hipStream_t st) {
  if (nrows <= 0 || dst16 <= 0) return hipSuccess;
  if (copy16 < 0 || copy16 > src16 || copy16 > dst16 || dst16 > 0x7fffffff) return hipErrorInvalidValue;
  int lg = 4;
  while (lg < 8 && (1 << lg) < dst16) ++lg;
  const int64_t rpb = 256 >> lg;
  const int64_t blocks = (nrows + rpb - 1) / rpb;
  const int grid = (int)(blocks < 4096 ? blocks : 4096);
  hipLaunchKernelGGL(ppls_gather_rows_kernel, dim3(grid), dim3(256), 0, st, (const uint4*)src, src16, (uint4*)dst, dst16,
                     copy16, rows, nrows, lg);
  return hipGetLastError();
}

hipError_t ppls_launch_downdate(const double* a, const double* b, double* out, int64_t len, hipStream_t st) {
  if (len <= 0) return hipSuccess;
  if (len & 1) return hipErrorInvalidValue;
  const int64_t len2 = len / 2, blocks = (len2 + 255) / 256;
  const int grid = (int)(blocks < 2048 ? blocks : 2048);
  hipLaunchKernelGGL(ppls_downdate_kernel, dim3(grid), dim3(256), 0, st, (const double2*)a, (const double2*)b,
                     (double2*)out, len2);
  return hipGetLastError();
}

int ppls_cv_rows_per_wave(int k) { return k <= 8 ? 8 : 4; }

int ppls_cv_grid(int64_t nrows, int k, int num_cus) {
  const int64_t per = (int64_t)ppls_cv_rows_per_wave(k) * PPLS_CV_WAVES;
  const int64_t blocks = (nrows + per - 1) / per, cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 4;
  return (int)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

hipError_t ppls_launch_cv_score(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, int f32,
                                const int64_t* rows, int64_t nrows, const double* A, const double* Bm,
                                const double* s, int k, double* part, double* pred, int64_t ldo, int grid,
                                hipStream_t st) {
  if (k < 1 || k > 16 || grid < 1 || nrows < 0 || pa < 1 || qb < 1) return hipErrorInvalidValue;
  if (pred) {
    if (f32 || (ldo & 1) || ldo < ((qb + 1) & ~1)) return hipErrorInvalidValue;   // predictions are staged in fp64
    if (nrows == 0) return hipSuccess;
    return score_launch<double, true>(X, lda, pa, nullptr, 0, qb, rows, nrows, A, Bm, s, k, nullptr, pred, ldo, grid, st);
  }
  if (!part) return hipErrorInvalidValue;
  if (f32) return score_launch<float, false>(X, lda, pa, Y, ldb, qb, rows, nrows, A, Bm, s, k, part, nullptr, 0, grid, st);
  return score_launch<double, false>(X, lda, pa, Y, ldb, qb, rows, nrows, A, Bm, s, k, part, nullptr, 0, grid, st);
}

hipError_t ppls_launch_cv_sse_reduce(const double* part, int nparts, int k, double* sse, hipStream_t st) {
  if (nparts < 0 || k < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_cv_sse_reduce_kernel, dim3(1), dim3(256), 0, st, part, nparts, k, sse);
  return hipGetLastError();
}

}  // extern "C"
