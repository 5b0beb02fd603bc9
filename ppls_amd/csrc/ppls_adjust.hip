// ppls_adjust.hip -- covariate adjustment (launch interface: ppls_adjust.h).
//
//   ppls_adjust_partials_kernel  G = Q'X per row block: a thread owns one 16-byte unit of the row, keeps
//                                KT x 2 (fp64) / KT x 4 (fp32 storage) fp64 accumulators and adds its
//                                block's rows in row order, one fma per (a, column) and row.
//   ppls_adjust_apply_kernel     x_ij <- x_ij - sum_a q_ia g_aj in place over the real columns only: the
//                                thread's G columns stay in registers, one fma chain per element.
//   ppls_adjust_schur_kernel     dst = src_dd - F F' over the 64 x 64 blocks of dst's lower triangle,
//                                F's rows of the block's row and column ranges staged in LDS, the mirror
//                                written from LDS (ppls_symtile.h's scheme, with distinct src and dst).
//
// A row's Q values are the same for every unit of the row.  Where a wave lies inside one row block (tx
// >= 64: UNI) the row-block index is made wave-uniform, so the row loop and the address of Q are scalar
// and Q arrives by scalar loads; narrower plans read Q with per-lane broadcast loads.  Plain HIP: no
// inline asm, vector stores only.  Every sum has a fixed order for a given PplsScalePlan.
#include <hip/hip_runtime.h>

#include "ppls_adjust.h"
#include "ppls_symtile.h"

namespace {

constexpr int ADJ_THREADS = 256;   // = ppls_scale.hip's workgroup: the plan's tx * ty

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

// The unit and the row range of this thread (ppls_scale.hip's split); false: nothing to do.
struct Owned {
  int u;
  int64_t b, r0, r1;
};
template <bool UNI>
__device__ inline bool owned(int lgx, int units, int64_t nblocks, int64_t n, Owned* o) {
  const int tx = 1 << lgx;
  o->u = blockIdx.x * tx + (threadIdx.x & (tx - 1));
  int by = threadIdx.x >> lgx;
  if constexpr (UNI) by = __builtin_amdgcn_readfirstlane(by);   // tx >= 64: one row block per wave
  o->b = (int64_t)blockIdx.y * (ADJ_THREADS >> lgx) + by;
  if (o->b >= nblocks) return false;
  o->r0 = o->b * n / nblocks;   // the even split
  o->r1 = (o->b + 1) * n / nblocks;
  return o->u < units;
}

template <typename T, int KT, bool NT, bool UNI>
__global__ __launch_bounds__(ADJ_THREADS) void ppls_adjust_partials_kernel(const T* __restrict__ X, int64_t ld, int64_t n,
                                                                           int units, int ldc, int64_t nblocks, int lgx,
                                                                           const double* __restrict__ Q,
                                                                           double* __restrict__ part) {
  constexpr int VE = Unit16<T>::VE, UR = 4;
  typedef typename Unit16<T>::vec vec;
  Owned o;
  if (!owned<UNI>(lgx, units, nblocks, n, &o)) return;
  double acc[KT][VE];
#pragma unroll
  for (int a = 0; a < KT; ++a)
#pragma unroll
    for (int e = 0; e < VE; ++e) acc[a][e] = 0.0;
  const T* p = X + o.r0 * ld + (int64_t)o.u * VE;
  const double* qp = Q + o.r0 * KT;
  int64_t i = o.r0;
  for (; i + UR <= o.r1; i += UR, p += UR * ld, qp += UR * KT) {
    vec v[UR];
#pragma unroll
    for (int k = 0; k < UR; ++k) v[k] = load16<T, NT>(p + k * ld);
#pragma unroll
    for (int k = 0; k < UR; ++k)
#pragma unroll
      for (int a = 0; a < KT; ++a) {
        const double qa = qp[k * KT + a];
#pragma unroll
        for (int e = 0; e < VE; ++e) acc[a][e] = fma(qa, (double)v[k][e], acc[a][e]);
      }
  }
  for (; i < o.r1; ++i, p += ld, qp += KT) {
    const vec v = load16<T, NT>(p);
#pragma unroll
    for (int a = 0; a < KT; ++a) {
      const double qa = qp[a];
#pragma unroll
      for (int e = 0; e < VE; ++e) acc[a][e] = fma(qa, (double)v[e], acc[a][e]);
    }
  }
  typedef double dvec __attribute__((ext_vector_type(2)));
  double* out = part + o.b * KT * (int64_t)ldc + (int64_t)o.u * VE;   // ldc and u VE are even: 16-byte stores
#pragma unroll
  for (int a = 0; a < KT; ++a)
#pragma unroll
    for (int e = 0; e < VE; e += 2) *(dvec*)(out + (int64_t)a * ldc + e) = dvec{acc[a][e], acc[a][e + 1]};
}

template <typename T, int KT, bool NT, bool UNI>
__global__ __launch_bounds__(ADJ_THREADS) void ppls_adjust_apply_kernel(T* __restrict__ X, int64_t ld, int64_t n, int cols,
                                                                        int units, int64_t ldg, int64_t nblocks, int lgx,
                                                                        const double* __restrict__ Q,
                                                                        const double* __restrict__ G) {
  constexpr int VE = Unit16<T>::VE, UR = 4;
  typedef typename Unit16<T>::vec vec;
  Owned o;
  if (!owned<UNI>(lgx, units, nblocks, n, &o)) return;
  // real columns of this unit: VE, fewer in the row's last unit when cols is no multiple of VE
  const int real = cols - o.u * VE < VE ? cols - o.u * VE : VE;
  double g[KT][VE];
#pragma unroll
  for (int a = 0; a < KT; ++a)
#pragma unroll
    for (int e = 0; e < VE; ++e) g[a][e] = e < real ? G[(int64_t)a * ldg + o.u * VE + e] : 0.0;
  T* p = X + o.r0 * ld + (int64_t)o.u * VE;
  const double* qp = Q + o.r0 * KT;
  if (real == VE) {
    int64_t i = o.r0;
    for (; i + UR <= o.r1; i += UR, p += UR * ld, qp += UR * KT) {
      vec v[UR];
#pragma unroll
      for (int k = 0; k < UR; ++k) v[k] = load16<T, NT>(p + k * ld);
#pragma unroll
      for (int k = 0; k < UR; ++k) {
        double x[VE];
#pragma unroll
        for (int e = 0; e < VE; ++e) x[e] = (double)v[k][e];
#pragma unroll
        for (int a = 0; a < KT; ++a) {
          const double nq = -qp[k * KT + a];
#pragma unroll
          for (int e = 0; e < VE; ++e) x[e] = fma(nq, g[a][e], x[e]);
        }
#pragma unroll
        for (int e = 0; e < VE; ++e) v[k][e] = (T)x[e];
        *(vec*)(p + k * ld) = v[k];
      }
    }
    for (; i < o.r1; ++i, p += ld, qp += KT) {
      vec v = load16<T, NT>(p);
      double x[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) x[e] = (double)v[e];
#pragma unroll
      for (int a = 0; a < KT; ++a) {
        const double nq = -qp[a];
#pragma unroll
        for (int e = 0; e < VE; ++e) x[e] = fma(nq, g[a][e], x[e]);
      }
#pragma unroll
      for (int e = 0; e < VE; ++e) v[e] = (T)x[e];
      *(vec*)p = v;
    }
  } else {   // the unit that also holds padding columns: element accesses, the padding is left alone
    for (int64_t i = o.r0; i < o.r1; ++i, p += ld, qp += KT)
#pragma unroll
      for (int e = 0; e < VE; ++e)
        if (e < real) {
          double x = (double)p[e];
#pragma unroll
          for (int a = 0; a < KT; ++a) x = fma(-qp[a], g[a][e], x);
          p[e] = (T)x;
        }
  }
}

// F: PPLS_ADJ_KMAX x P_dst doubles (row a = component a over dst's joint columns).
__global__ __launch_bounds__(PPLS_SYM_THREADS) void ppls_adjust_schur_kernel(const double* __restrict__ src, int P_src,
                                                                            double* __restrict__ dst, PplsSymCols g,
                                                                            const double* __restrict__ F, int k) {
  constexpr int SB = PPLS_SYM_SB, KM = PPLS_ADJ_KMAX;
  const PplsSymBlock blk = ppls_sym_block(blockIdx.x);
  const int qi = blk.qi, qj = blk.qj;
  __shared__ double T[SB][SB + 1];
  __shared__ double Fa[KM][SB], Fb[KM][SB];
  const int t = threadIdx.x;
  const int P = g.P;
  for (int idx = t; idx < 2 * KM * SB; idx += PPLS_SYM_THREADS) {
    const int side = idx / (KM * SB), rem = idx - side * (KM * SB);
    const int a = rem / SB, rr = rem - a * SB;
    const int c = (side ? qj : qi) * SB + rr;
    const double v = (a < k && c < P && ppls_sym_col_live(g, c)) ? F[(int64_t)a * P + c] : 0.0;
    if (side) Fb[a][rr] = v; else Fa[a][rr] = v;
  }
  __syncthreads();
  const int c2 = (t & 31) * 2, rb = t >> 5;
  const int lo = qj * SB + c2;
  const bool diag = qi == qj;
#pragma unroll
  for (int m = 0; m < SB / 8; ++m) {
    const int r = rb + 8 * m, hi = qi * SB + r;
    double2 v = make_double2(0.0, 0.0);
    if (hi < P && lo < P) {   // P is even: lo + 1 < P as well; P <= P_src and both even: a 16-byte load
      v = *(const double2*)(src + (int64_t)hi * P_src + lo);
      for (int a = 0; a < k; ++a) {
        const double fa = -Fa[a][r];
        v.x = fma(fa, Fb[a][c2], v.x);
        v.y = fma(fa, Fb[a][c2 + 1], v.y);
      }
      const bool lh = ppls_sym_col_live(g, hi);
      if (!lh || !ppls_sym_col_live(g, lo)) v.x = 0.0;
      if (!lh || !ppls_sym_col_live(g, lo + 1)) v.y = 0.0;
      if (!diag) *(double2*)(dst + (int64_t)hi * P + lo) = v;
    }
    T[r][c2] = v.x;
    T[r][c2 + 1] = v.y;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < SB / 8; ++m) {
    const int r = rb + 8 * m;
    if (diag) {   // entry (r, c) from the lower triangle: (max, min)
      const int hi = qi * SB + r;
      if (hi < P && lo < P) {
        const double x = c2 <= r ? T[r][c2] : T[c2][r];
        const double y = c2 + 1 <= r ? T[r][c2 + 1] : T[c2 + 1][r];
        *(double2*)(dst + (int64_t)hi * P + lo) = make_double2(x, y);
      }
    } else {      // the mirror block (qj, qi): row qj SB + r, columns qi SB + c2, c2 + 1
      const int mr = qj * SB + r, mc = qi * SB + c2;
      if (mr < P && mc < P) *(double2*)(dst + (int64_t)mr * P + mc) = make_double2(T[c2][r], T[c2 + 1][r]);
    }
  }
}

bool plan_ok(const PplsScalePlan* pl, int64_t ld, int f32) {
  if (!pl || pl->units < 1 || pl->tx < 1 || pl->tx * pl->ty != ADJ_THREADS || (pl->tx & (pl->tx - 1))) return false;
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

template <typename T, int KT>
void launch_partials(const void* X, int64_t ld, int64_t n, const PplsScalePlan* pl, const double* Q, int nt, double* part,
                     hipStream_t st) {
  const dim3 grid(pl->grid_x, pl->grid_y), block(ADJ_THREADS);
  const int lgx = lg_of(pl->tx);
#define PPLS_ADJ_PARTIALS(NT, UNI)                                                                                   \
  hipLaunchKernelGGL((ppls_adjust_partials_kernel<T, KT, NT, UNI>), grid, block, 0, st, (const T*)X, ld, n, pl->units, \
                     pl->ldc, pl->nblocks, lgx, Q, part)
  if (pl->tx >= 64) { if (nt) PPLS_ADJ_PARTIALS(true, true); else PPLS_ADJ_PARTIALS(false, true); }
  else { if (nt) PPLS_ADJ_PARTIALS(true, false); else PPLS_ADJ_PARTIALS(false, false); }
#undef PPLS_ADJ_PARTIALS
}

template <typename T, int KT>
void launch_apply(void* X, int64_t ld, int64_t n, int cols, const PplsScalePlan* pl, const double* Q, const double* G,
                  int64_t ldg, int nt, hipStream_t st) {
  const dim3 grid(pl->grid_x, pl->grid_y), block(ADJ_THREADS);
  const int lgx = lg_of(pl->tx);
#define PPLS_ADJ_APPLY(NT, UNI)                                                                                       \
  hipLaunchKernelGGL((ppls_adjust_apply_kernel<T, KT, NT, UNI>), grid, block, 0, st, (T*)X, ld, n, cols, pl->units, \
                     ldg, pl->nblocks, lgx, Q, G)
  if (pl->tx >= 64) { if (nt) PPLS_ADJ_APPLY(true, true); else PPLS_ADJ_APPLY(false, true); }
  else { if (nt) PPLS_ADJ_APPLY(true, false); else PPLS_ADJ_APPLY(false, false); }
#undef PPLS_ADJ_APPLY
}

}  // namespace

extern "C" {

hipError_t ppls_launch_adjust_partials(const void* X, int64_t ld, int64_t n, int f32, const PplsScalePlan* pl,
                                       const double* Q, int kt, int nt, double* part, hipStream_t st) {
  if (!plan_ok(pl, ld, f32) || n < 1 || !X || !Q || !part) return hipErrorInvalidValue;
  if (f32) {
    if (kt == 4) launch_partials<float, 4>(X, ld, n, pl, Q, nt, part, st);
    else if (kt == 8) launch_partials<float, 8>(X, ld, n, pl, Q, nt, part, st);
    else if (kt == 16) launch_partials<float, 16>(X, ld, n, pl, Q, nt, part, st);
    else return hipErrorInvalidValue;
  } else {
    if (kt == 4) launch_partials<double, 4>(X, ld, n, pl, Q, nt, part, st);
    else if (kt == 8) launch_partials<double, 8>(X, ld, n, pl, Q, nt, part, st);
    else if (kt == 16) launch_partials<double, 16>(X, ld, n, pl, Q, nt, part, st);
    else return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t ppls_launch_adjust_reduce(const double* part, const PplsScalePlan* pl, int kt, double* G, hipStream_t st) {
  if (!pl || (kt != 4 && kt != 8 && kt != 16) || (int64_t)kt * pl->ldc >= (1 << 30)) return hipErrorInvalidValue;
  PplsScalePlan r = *pl;   // a block's KT x ldc partials as one row of KT * ldc columns
  r.ldc = kt * pl->ldc;
  return ppls_launch_col_reduce(part, &r, r.ldc, G, st);
}

hipError_t ppls_launch_adjust_apply(void* X, int64_t ld, int64_t n, int cols, int f32, const PplsScalePlan* pl,
                                    const double* Q, const double* G, int64_t ldg, int kt, int nt, hipStream_t st) {
  if (!plan_ok(pl, ld, f32) || n < 1 || !X || !Q || !G || ldg < pl->ldc) return hipErrorInvalidValue;
  if (cols < 1 || cols > pl->ldc || cols <= pl->ldc - (f32 ? 4 : 2)) return hipErrorInvalidValue;
  if (f32) {
    if (kt == 4) launch_apply<float, 4>(X, ld, n, cols, pl, Q, G, ldg, nt, st);
    else if (kt == 8) launch_apply<float, 8>(X, ld, n, cols, pl, Q, G, ldg, nt, st);
    else if (kt == 16) launch_apply<float, 16>(X, ld, n, cols, pl, Q, G, ldg, nt, st);
    else return hipErrorInvalidValue;
  } else {
    if (kt == 4) launch_apply<double, 4>(X, ld, n, cols, pl, Q, G, ldg, nt, st);
    else if (kt == 8) launch_apply<double, 8>(X, ld, n, cols, pl, Q, G, ldg, nt, st);
    else if (kt == 16) launch_apply<double, 16>(X, ld, n, cols, pl, Q, G, ldg, nt, st);
    else return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t ppls_launch_adjust_schur(const double* src, int P_src, double* dst, int p, int ldx, int q, int ldy_dst,
                                    const double* F, int k, hipStream_t st) {
  if (!src || !dst || !F || src == dst || k < 1 || k > PPLS_ADJ_KMAX || !ppls_sym_shape_ok(p, ldx, q, ldy_dst))
    return hipErrorInvalidValue;
  const int P = ldx + ldy_dst;
  if (P_src < P || P_src % 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ppls_adjust_schur_kernel, dim3(ppls_sym_blocks(P)), dim3(PPLS_SYM_THREADS), 0, st, src, P_src, dst,
                     PplsSymCols{P, p, ldx, ldx + q}, F, k);
  return hipGetLastError();
}

}  // extern "C"
