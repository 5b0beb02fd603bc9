// ppls_scale.hip -- R's scale(x, center, scale) on the resident X, Y (launch interface: ppls_scale.h).
//
//   ppls_col_partials_kernel  column sums of x (SQ = false) or of (x - centre_j)^2 (SQ = true) per row
//                             block: a thread owns one 16-byte unit of the row, keeps fp64
//                             accumulators for its 2 / 4 columns and adds its block's rows in row
//                             order (the loads of 8 rows are issued together, the adds stay in order).
//   ppls_col_reduce_kernel    the row blocks' partials added in block order, one thread per column.
//   ppls_col_apply_kernel     x <- (x - centre_j) / scale_j in place over the real columns only: the
//                             padding columns and the slack behind the last row are never written.
//
// Two passes over the data for the statistics, as R's scale() makes them: the second pass sums the
// squares of the centred values, which keeps sd accurate when |mean| >> sd.  Plain HIP: no inline asm.
// Every sum has a fixed order for a given PplsScalePlan, which depends on the shape and num_cus only.
#include <hip/hip_runtime.h>

#include "ppls_scale.h"

namespace {

constexpr int SCALE_THREADS = 256;
constexpr int SCALE_MIN_ROWS = 16;       // a row block is not made smaller than this
constexpr int SCALE_MAX_BLOCKS = 2048;   // row blocks: the length of the reduce kernel's serial sums
constexpr int SCALE_WG_PER_CU = 8;

template <typename T>
struct Unit16;
template <>
struct Unit16<double> {
  static constexpr int VE = 2;
  typedef double vec __attribute__((ext_vector_type(2)));
};
template <>
struct Unit16<float> {
  static constexpr int VE = 4;
  typedef float vec __attribute__((ext_vector_type(4)));
};

template <typename T, bool NT>
__device__ inline typename Unit16<T>::vec load16(const T* p) {
  typedef typename Unit16<T>::vec vec;
  if constexpr (NT) return __builtin_nontemporal_load((const vec*)p);
  return *(const vec*)p;
}

// The unit and the row range of this thread; false: nothing to do.
struct Owned {
  int u;
  int64_t b, r0, r1;
};
__device__ inline bool owned(int lgx, int units, int64_t nblocks, int64_t n, Owned* o) {
  const int tx = 1 << lgx;
  o->u = blockIdx.x * tx + (threadIdx.x & (tx - 1));
  o->b = (int64_t)blockIdx.y * (SCALE_THREADS >> lgx) + (threadIdx.x >> lgx);
  if (o->u >= units || o->b >= nblocks) return false;
  o->r0 = o->b * n / nblocks;   // the even split
  o->r1 = (o->b + 1) * n / nblocks;
  return true;
}

template <typename T, bool SQ, bool NT>
__global__ __launch_bounds__(SCALE_THREADS) void ppls_col_partials_kernel(const T* __restrict__ X, int64_t ld, int64_t n,
                                                                          int units, int ldc, int64_t nblocks, int lgx,
                                                                          const double* __restrict__ centre,
                                                                          double* __restrict__ part) {
  constexpr int VE = Unit16<T>::VE, UR = 8;
  typedef typename Unit16<T>::vec vec;
  Owned o;
  if (!owned(lgx, units, nblocks, n, &o)) return;
  double c[VE], acc[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    c[e] = SQ ? centre[o.u * VE + e] : 0.0;
    acc[e] = 0.0;
  }
  const T* p = X + o.r0 * ld + (int64_t)o.u * VE;
  int64_t i = o.r0;
  for (; i + UR <= o.r1; i += UR, p += UR * ld) {
    vec v[UR];
#pragma unroll
    for (int k = 0; k < UR; ++k) v[k] = load16<T, NT>(p + k * ld);
#pragma unroll
    for (int k = 0; k < UR; ++k)
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const double d = (double)v[k][e] - c[e];
        acc[e] += SQ ? d * d : d;
      }
  }
  for (; i < o.r1; ++i, p += ld) {
    const vec v = load16<T, NT>(p);
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      const double d = (double)v[e] - c[e];
      acc[e] += SQ ? d * d : d;
    }
  }
#pragma unroll
  for (int e = 0; e < VE; ++e) part[o.b * ldc + o.u * VE + e] = acc[e];
}

__global__ __launch_bounds__(SCALE_THREADS) void ppls_col_reduce_kernel(const double* __restrict__ part, int64_t nblocks,
                                                                        int ldc, int cols, double* __restrict__ out) {
  const int j = blockIdx.x * SCALE_THREADS + threadIdx.x;
  if (j >= cols) return;
  // the loads of UR blocks are issued together (a serial chain of dependent-latency loads otherwise:
  // thousands of blocks for a narrow matrix); the adds stay in block order
  constexpr int UR = 16;
  double acc = 0.0;
  int64_t b = 0;
  for (; b + UR <= nblocks; b += UR) {
    double v[UR];
#pragma unroll
    for (int k = 0; k < UR; ++k) v[k] = part[(b + k) * ldc + j];
#pragma unroll
    for (int k = 0; k < UR; ++k) acc += v[k];
  }
  for (; b < nblocks; ++b) acc += part[b * ldc + j];
  out[j] = acc;
}

template <typename T, bool NT>
__global__ __launch_bounds__(SCALE_THREADS) void ppls_col_apply_kernel(T* __restrict__ X, int64_t ld, int64_t n, int cols,
                                                                       int units, int64_t nblocks, int lgx,
                                                                       const double* __restrict__ centre,
                                                                       const double* __restrict__ scale) {
  constexpr int VE = Unit16<T>::VE, UR = 4;
  typedef typename Unit16<T>::vec vec;
  Owned o;
  if (!owned(lgx, units, nblocks, n, &o)) return;
  // real columns of this unit: VE, fewer in the row's last unit when cols is no multiple of VE
  const int real = cols - o.u * VE < VE ? cols - o.u * VE : VE;
  double c[VE], s[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    c[e] = e < real ? centre[o.u * VE + e] : 0.0;
    s[e] = e < real ? scale[o.u * VE + e] : 1.0;
  }
  T* p = X + o.r0 * ld + (int64_t)o.u * VE;
  if (real == VE) {
    int64_t i = o.r0;
    for (; i + UR <= o.r1; i += UR, p += UR * ld) {
      vec v[UR];
#pragma unroll
      for (int k = 0; k < UR; ++k) v[k] = load16<T, NT>(p + k * ld);
#pragma unroll
      for (int k = 0; k < UR; ++k) {
#pragma unroll
        for (int e = 0; e < VE; ++e) v[k][e] = (T)(((double)v[k][e] - c[e]) / s[e]);
        *(vec*)(p + k * ld) = v[k];
      }
    }
    for (; i < o.r1; ++i, p += ld) {
      vec v = load16<T, NT>(p);
#pragma unroll
      for (int e = 0; e < VE; ++e) v[e] = (T)(((double)v[e] - c[e]) / s[e]);
      *(vec*)p = v;
    }
  } else {   // the unit that also holds padding columns: element stores, the padding is left alone
    for (int64_t i = o.r0; i < o.r1; ++i, p += ld)
#pragma unroll
      for (int e = 0; e < VE; ++e)
        if (e < real) p[e] = (T)(((double)p[e] - c[e]) / s[e]);
  }
}

bool plan_ok(const PplsScalePlan* pl, int64_t ld, int f32) {
  if (!pl || pl->units < 1 || pl->tx < 1 || pl->tx * pl->ty != SCALE_THREADS || (pl->tx & (pl->tx - 1))) return false;
  if (pl->grid_x < 1 || pl->grid_y < 1 || pl->grid_y > 65535 || pl->nblocks < 1) return false;
  if ((int64_t)pl->grid_x * pl->tx < pl->units || (int64_t)pl->grid_y * pl->ty < pl->nblocks) return false;
  const int ve = f32 ? 4 : 2;
  return pl->ldc == pl->units * ve && (int64_t)pl->ldc <= ld && ld % ve == 0;   // every unit lies inside the row
}

int lg_of(int tx) {
  int lg = 0;
  while ((1 << lg) < tx) ++lg;
  return lg;
}

}  // namespace

extern "C" {

PplsScalePlan ppls_scale_plan(int64_t n, int cols, int f32, int num_cus) {
  PplsScalePlan pl;
  const int ve = f32 ? 4 : 2;
  pl.units = (cols + ve - 1) / ve;
  if (pl.units < 1) pl.units = 1;
  pl.ldc = pl.units * ve;
  pl.tx = 1;
  while (pl.tx < pl.units && pl.tx < SCALE_THREADS) pl.tx *= 2;
  pl.ty = SCALE_THREADS / pl.tx;
  pl.grid_x = (pl.units + pl.tx - 1) / pl.tx;
  const int64_t wgs = (int64_t)(num_cus > 0 ? num_cus : 256) * SCALE_WG_PER_CU;
  const int64_t gy = wgs / pl.grid_x > 1 ? wgs / pl.grid_x : 1;
  int64_t nb = (n + SCALE_MIN_ROWS - 1) / SCALE_MIN_ROWS;
  if (nb > gy * pl.ty) nb = gy * pl.ty;
  if (nb > SCALE_MAX_BLOCKS) nb = SCALE_MAX_BLOCKS;
  if (nb < 1) nb = 1;
  pl.nblocks = nb;
  pl.grid_y = (int)((nb + pl.ty - 1) / pl.ty);
  return pl;
}

hipError_t ppls_launch_col_partials(const void* X, int64_t ld, int64_t n, int f32, const PplsScalePlan* pl,
                                    const double* centre, int sq, int nt, double* part, hipStream_t st) {
  if (!plan_ok(pl, ld, f32) || n < 1 || !X || !part || (sq && !centre)) return hipErrorInvalidValue;
  const dim3 grid(pl->grid_x, pl->grid_y), block(SCALE_THREADS);
  const int lgx = lg_of(pl->tx);
#define PPLS_SCALE_PARTIALS(T, SQ, NT)                                                                          \
  hipLaunchKernelGGL((ppls_col_partials_kernel<T, SQ, NT>), grid, block, 0, st, (const T*)X, ld, n, pl->units, \
                     pl->ldc, pl->nblocks, lgx, centre, part)
  if (f32) {
    if (sq) { if (nt) PPLS_SCALE_PARTIALS(float, true, true); else PPLS_SCALE_PARTIALS(float, true, false); }
    else { if (nt) PPLS_SCALE_PARTIALS(float, false, true); else PPLS_SCALE_PARTIALS(float, false, false); }
  } else {
    if (sq) { if (nt) PPLS_SCALE_PARTIALS(double, true, true); else PPLS_SCALE_PARTIALS(double, true, false); }
    else { if (nt) PPLS_SCALE_PARTIALS(double, false, true); else PPLS_SCALE_PARTIALS(double, false, false); }
  }
#undef PPLS_SCALE_PARTIALS
  return hipGetLastError();
}

hipError_t ppls_launch_col_reduce(const double* part, const PplsScalePlan* pl, int cols, double* out, hipStream_t st) {
  if (!pl || !part || !out || cols < 1 || cols > pl->ldc || pl->nblocks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_col_reduce_kernel, dim3((cols + SCALE_THREADS - 1) / SCALE_THREADS), dim3(SCALE_THREADS), 0, st,
                     part, pl->nblocks, pl->ldc, cols, out);
  return hipGetLastError();
}

hipError_t ppls_launch_col_apply(void* X, int64_t ld, int64_t n, int cols, int f32, const PplsScalePlan* pl,
                                 const double* centre, const double* scale, int nt, hipStream_t st) {
  if (!plan_ok(pl, ld, f32) || n < 1 || !X || !centre || !scale) return hipErrorInvalidValue;
  if (cols < 1 || cols > pl->ldc || cols <= pl->ldc - (f32 ? 4 : 2)) return hipErrorInvalidValue;
  const dim3 grid(pl->grid_x, pl->grid_y), block(SCALE_THREADS);
  const int lgx = lg_of(pl->tx);
#define PPLS_SCALE_APPLY(T, NT)                                                                                  \
  hipLaunchKernelGGL((ppls_col_apply_kernel<T, NT>), grid, block, 0, st, (T*)X, ld, n, cols, pl->units, pl->nblocks, \
                     lgx, centre, scale)
  if (f32) { if (nt) PPLS_SCALE_APPLY(float, true); else PPLS_SCALE_APPLY(float, false); }
  else { if (nt) PPLS_SCALE_APPLY(double, true); else PPLS_SCALE_APPLY(double, false); }
#undef PPLS_SCALE_APPLY
  return hipGetLastError();
}

}  // extern "C"
