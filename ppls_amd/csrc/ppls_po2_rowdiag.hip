// ppls_po2_rowdiag.hip -- per-row diagnostics of a fitted PO2PLS model on the device (launch interface and the
// determinism statement: ppls_po2_rowdiag.h; algebra: DESIGN.md §29).
//
//   ppls_po2_rowdiag_kernel   ppls_rowdiag.hip's two phases per block with a width and a tile per block: a
//                             wave owns RW rows at a time, its lanes the 16-byte units of a row.  X with Qx
//                             (kx columns, tile KTX), then Y with Qy (ky, KTY): phase 1 forms the scores
//                             a_i = Qx'x_i with the fixed-tree wave reduce-scatter, phase 2 reads the same
//                             rows again and forms ||x_i - Qx a_i||^2 from the residual.  Then the dense
//                             in-plane part, row after row of the group: the row's k = kx + ky scores are
//                             broadcast one at a time (readlane), lane i < 32 adds row i of Uc against them
//                             and lane 32 + i column i of Kmu; the squares of lanes 0 .. 31 meet in a fixed
//                             tree (sd2), lanes 32 .. 32 + k - 1 hold the posterior means.
//
// Uc and Kmu lie in LDS as one 32 x 64 table (ppls_po2_rowdiag.h), column j a 512-byte line that the 64
// lanes read side by side: no bank conflict.  It is written once per workgroup; the rows are never staged.
// fp64 arithmetic on fp64 or fp32 storage.  Plain HIP: no inline asm, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ppls_po2_rowdiag.h"

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

// One step of the reduce-scatter over the wave (as in ppls_rowdiag.hip): after H = 32 .. 1, v[0] of lane L
// is the sum of value L over all 64 lanes; the sum does not depend on the slot the value sits in.
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
  static_assert(NV <= 64 && (NV & (NV - 1)) == 0, "a wave's row group holds a power of two of at most 64 scores");
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

template <typename T, int KTX, int KTY, int RW, bool MU>
__global__ __launch_bounds__(64 * PPLS_PO2_ROWDIAG_WAVES) void ppls_po2_rowdiag_kernel(
    const T* __restrict__ X, int64_t lda, int pa, const T* __restrict__ Y, int64_t ldb, int qb,
    const int64_t* __restrict__ rows, int64_t nrows, const double* __restrict__ Qx, int kx, const double* __restrict__ Qy,
    int ky, const double* __restrict__ tab, double* __restrict__ odx2, double* __restrict__ ody2, double* __restrict__ sd2,
    double* __restrict__ mu, int64_t ldmu) {
  constexpr int VE = Unit16<T>::VE;
  __shared__ double stab[PPLS_PO2_ROWDIAG_TAB];
  const int k = kx + ky;   // <= PPLS_PO2_ROWDIAG_KMAX, checked by the launcher
  for (int e = threadIdx.x; e < k * 64; e += 64 * PPLS_PO2_ROWDIAG_WAVES) stab[e] = tab[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * PPLS_PO2_ROWDIAG_WAVES + wave, nw = (int64_t)gridDim.x * PPLS_PO2_ROWDIAG_WAVES;
  const int64_t ngroups = (nrows + RW - 1) / RW;
  const int lda4 = (pa + 3) & ~3, ldb4 = (qb + 3) & ~3;
  const int na = (pa + VE - 1) / VE, nb = (qb + VE - 1) / VE;   // 16-byte units holding real columns

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
    const double ta = block_scores<T, KTX, RW>(X, lda, idx, na, lda4, Qx, kx, lane);
    block_resid<T, KTX, RW>(X, lda, idx, na, lda4, Qx, kx, ta, lane, rx);
    const double tb = block_scores<T, KTY, RW>(Y, ldb, idx, nb, ldb4, Qy, ky, lane);
    block_resid<T, KTY, RW>(Y, ldb, idx, nb, ldb4, Qy, ky, tb, lane, ry);
    // the dense part: the row's scores in the order (a_0 .. a_kx-1, b_0 .. b_ky-1), one accumulator per lane
#pragma unroll
    for (int rr = 0; rr < RW; ++rr) {
      double acc = 0.0;
      for (int j = 0; j < kx; ++j) acc += stab[j * 64 + lane] * lane_value(ta, rr * KTX + j);
      for (int j = 0; j < ky; ++j) acc += stab[(kx + j) * 64 + lane] * lane_value(tb, rr * KTY + j);
      double sd = lane < 32 ? acc * acc : 0.0;   // lanes i >= k of the lower half hold zero rows of Uc
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) sd += __shfl_xor(sd, o, 64);
      if (rr < nvalid) {
        const int64_t o = i0 + rr;
        if (lane == 0) {
          odx2[o] = rx[rr];
          ody2[o] = ry[rr];
          sd2[o] = sd;
        }
        if (MU && lane >= 32 && lane - 32 < k) mu[(int64_t)(lane - 32) * ldmu + o] = acc;
      }
    }
  }
}

template <typename T>
hipError_t po2_rowdiag_launch(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, const int64_t* rows,
                              int64_t nrows, const double* Qx, int kx, const double* Qy, int ky, const double* tab,
                              double* odx2, double* ody2, double* sd2, double* mu, int64_t ldmu, int grid, hipStream_t st) {
  const dim3 g(grid), b(64 * PPLS_PO2_ROWDIAG_WAVES);
  const int rw = ppls_po2_rowdiag_rows_per_wave(pa, qb, sizeof(T) == 4, kx, ky);
  const int tx = ppls_po2_rowdiag_tile(kx), ty = ppls_po2_rowdiag_tile(ky);
#define PPLS_PO2RD_GO(KTX, KTY, RW, MU)                                                                                 \
  hipLaunchKernelGGL((ppls_po2_rowdiag_kernel<T, KTX, KTY, RW, MU>), g, b, 0, st, (const T*)X, lda, pa, (const T*)Y, ldb, \
                     qb, rows, nrows, Qx, kx, Qy, ky, tab, odx2, ody2, sd2, mu, ldmu)
#define PPLS_PO2RD_MU(KTX, KTY, RW)             \
  do {                                          \
    if (mu) PPLS_PO2RD_GO(KTX, KTY, RW, true);  \
    else PPLS_PO2RD_GO(KTX, KTY, RW, false);    \
  } while (0)
  if (tx == 16 && ty == 16) PPLS_PO2RD_MU(16, 16, PPLS_PO2_ROWDIAG_ROWS16);
  else if (tx == 16) PPLS_PO2RD_MU(16, 8, PPLS_PO2_ROWDIAG_ROWS16);
  else if (ty == 16) PPLS_PO2RD_MU(8, 16, PPLS_PO2_ROWDIAG_ROWS16);
  else if (rw == PPLS_PO2_ROWDIAG_ROWS8_SHORT) PPLS_PO2RD_MU(8, 8, PPLS_PO2_ROWDIAG_ROWS8_SHORT);
  else PPLS_PO2RD_MU(8, 8, PPLS_PO2_ROWDIAG_ROWS8);
#undef PPLS_PO2RD_MU
#undef PPLS_PO2RD_GO
  return hipGetLastError();
}

}  // namespace

extern "C" {

int ppls_po2_rowdiag_tile(int kb) { return kb > 8 ? 16 : 8; }

int ppls_po2_rowdiag_rows_per_wave(int pa, int qb, int f32, int kx, int ky) {
  if (std::max(kx, ky) > 8) return PPLS_PO2_ROWDIAG_ROWS16;
  const int64_t row_bytes = (int64_t)std::max(pa, qb) * (f32 ? 4 : 8);
  return row_bytes <= PPLS_PO2_ROWDIAG_SHORT_BYTES ? PPLS_PO2_ROWDIAG_ROWS8_SHORT : PPLS_PO2_ROWDIAG_ROWS8;
}

int ppls_po2_rowdiag_grid(int64_t nrows, int pa, int qb, int f32, int kx, int ky, int num_cus) {
  const int rw = ppls_po2_rowdiag_rows_per_wave(pa, qb, f32, kx, ky);
  const int64_t per = (int64_t)rw * PPLS_PO2_ROWDIAG_WAVES;
  const int64_t blocks = (nrows + per - 1) / per, cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 4;
  return (int)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

hipError_t ppls_launch_po2_rowdiag(const void* X, int64_t lda, int pa, const void* Y, int64_t ldb, int qb, int f32,
                                   const int64_t* rows, int64_t nrows, const double* Qx, int kx, const double* Qy,
                                   int ky, const double* tab, double* odx2, double* ody2, double* sd2, double* mu,
                                   int64_t ldmu, int grid, hipStream_t st) {
  if (kx < 1 || kx > 16 || ky < 1 || ky > 16 || kx > pa || ky > qb || grid < 1 || nrows < 0) return hipErrorInvalidValue;
  if (!X || !Y || !Qx || !Qy || !tab || !odx2 || !ody2 || !sd2) return hipErrorInvalidValue;
  if (mu && ldmu < nrows) return hipErrorInvalidValue;
  const int ve = f32 ? 4 : 2;   // a row holds whole 16-byte units of real columns
  if (lda < (int64_t)(pa + ve - 1) / ve * ve || ldb < (int64_t)(qb + ve - 1) / ve * ve || lda % ve || ldb % ve)
    return hipErrorInvalidValue;
  if (nrows == 0) return hipSuccess;
  if (f32)
    return po2_rowdiag_launch<float>(X, lda, pa, Y, ldb, qb, rows, nrows, Qx, kx, Qy, ky, tab, odx2, ody2, sd2, mu, ldmu,
                                     grid, st);
  return po2_rowdiag_launch<double>(X, lda, pa, Y, ldb, qb, rows, nrows, Qx, kx, Qy, ky, tab, odx2, ody2, sd2, mu, ldmu,
                                    grid, st);
}

}  // extern "C"
