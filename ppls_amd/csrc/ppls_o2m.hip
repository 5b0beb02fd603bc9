// ppls_o2m.hip -- the one-pass operator of the 'o2m_xprod' starting values (ppls_o2m.h).
//
//   u_i = a_i . v - d_i,   z = sum_i u_i a_i
//
// over a rows x L block A of the cross-products S.  Fused path (L <= PPLS_O2M_FUSED_LMAX): a wave
// takes R rows at a time; lane l holds the column pairs 2 (l + 64 j), j < NJ, of v and of the z
// accumulators in registers (as the split sweep keeps W and X'mu_T), loads its 16 bytes of each row
// once, reduces the dot over the wave (ppls_device.h) and adds u_i a_i to its accumulators.  The
// waves of a workgroup are summed through LDS in wave order, the workgroups' partials by a second
// kernel in a fixed order: no floating-point atomics, and the same bits on every launch.  Rows of
// more than 512 values are shared by the four waves of a workgroup (ppls_o2m_fused_wide_kernel).
// Two-phase path (longer rows): u = A v - d by one wave per row, then z = A'u over 128-column
// slices x row groups with the same fixed-order end; A is read twice there and only there.
#include "ppls_o2m.h"

#include <algorithm>

#include "ppls_device.h"

namespace {

constexpr int O2M_THREADS = 256;
constexpr int O2M_WAVES = O2M_THREADS / 64;
constexpr int O2M_WIDE_R = 4;   // rows per workgroup step of the wide fused kernel

struct O2mPlan {
  int path;      // PPLS_O2M_PATH_FUSED / _TWOPHASE, 0 = refused
  int NJ, R;     // fused: column pairs per lane, rows per wave step
  int nb;        // fused: workgroups; two-phase: row groups
  int nslices;   // two-phase: 128-column slices
  int ldp;       // doubles per partial row of the workspace
};

int o2m_nj(int L) {
  const int Lp = (L + 1) & ~1;
  int NJ = 1;
  while (NJ * 128 < Lp) NJ *= 2;
  return NJ;
}

int o2m_rows_per_step(int NJ) { return NJ <= 2 ? 8 : NJ <= 4 ? 4 : 2; }

O2mPlan o2m_plan(int rows, int L, int num_cus, int path_opt) {
  O2mPlan pl{};
  const int cus = num_cus > 0 ? num_cus : 256;
  const bool fits = L <= PPLS_O2M_FUSED_LMAX;
  if (path_opt == PPLS_O2M_PATH_FUSED && !fits) return pl;
  const bool fused = path_opt == PPLS_O2M_PATH_FUSED || (path_opt != PPLS_O2M_PATH_TWOPHASE && fits);
  if (fused) {
    pl.path = PPLS_O2M_PATH_FUSED;
    pl.NJ = o2m_nj(L);
    pl.R = o2m_rows_per_step(pl.NJ);
    // two steps of R rows per wave where the rows allow, at most one workgroup per CU: every wave
    // loads v once and every workgroup writes one partial of z, and both are overhead beside A
    const int per_wg = O2M_WAVES * pl.R * 2;
    pl.nb = std::max(1, std::min((rows + per_wg - 1) / per_wg, cus));
    pl.ldp = pl.NJ * 128;
    if (pl.NJ >= 8) {
      // rows of more than 512 values: the workgroup's waves share each row (ppls_o2m_fused_wide_kernel),
      // R rows per workgroup step, two steps per workgroup where the rows allow
      pl.R = O2M_WIDE_R;
      const int nsteps = (rows + pl.R - 1) / pl.R;
      pl.nb = std::max(1, std::min((nsteps + 1) / 2, 2 * cus));
    }
  } else {
    pl.path = PPLS_O2M_PATH_TWOPHASE;
    const int Lp = (L + 1) & ~1;
    pl.nslices = (Lp + 127) / 128;
    pl.nb = std::max(1, std::min((4 * cus + pl.nslices - 1) / pl.nslices, (rows + 31) / 32));
    pl.ldp = pl.nslices * 128;
  }
  return pl;
}

__device__ __forceinline__ double o2m_wave_sum(double x, int lane) {
  double a[2] = {x, 0.0};
  int idx = 0;
  bool canon = true;
  ppls_rs<1, 0, 2>(a, lane, idx, canon);   // M = 1: a butterfly, every lane ends with the same sum
  return a[0];
}

// The workgroup's four waves' accumulators -> part[blockIdx.x][.], waves added in order 0..3.
template <int NJ>
__device__ __forceinline__ void o2m_block_out(const double2 (&zz)[NJ], int lane, int wave, double* __restrict__ dst) {
  __shared__ double2 red[O2M_WAVES][64];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    red[wave][lane] = zz[j];
    __syncthreads();
    if (wave == 0) {
      double2 s = red[0][lane];
#pragma unroll
      for (int w = 1; w < O2M_WAVES; ++w) {
        s.x += red[w][lane].x;
        s.y += red[w][lane].y;
      }
      *reinterpret_cast<double2*>(dst + 2 * (lane + 64 * j)) = s;
    }
    __syncthreads();
  }
}

template <int NJ, int R>
__global__ __launch_bounds__(O2M_THREADS) void ppls_o2m_fused_kernel(const double* __restrict__ A, int64_t ld, int rows,
                                                                      int L, const double* __restrict__ v,
                                                                      const double* __restrict__ d,
                                                                      double* __restrict__ u,
                                                                      double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * O2M_WAVES + wave, nw = gridDim.x * O2M_WAVES;
  double2 vv[NJ], zz[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = 2 * (lane + 64 * j);
    vv[j].x = c < L ? v[c] : 0.0;
    vv[j].y = c + 1 < L ? v[c + 1] : 0.0;
    zz[j] = make_double2(0.0, 0.0);
  }
  const int nsteps = (rows + R - 1) / R;
  for (int s = gw; s < nsteps; s += nw) {   // wave-uniform: the reductions below run with all lanes
    double2 a[R][NJ];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = s * R + r;
      const double* ap = A + (int64_t)i * ld;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = 2 * (lane + 64 * j);
        a[r][j] = make_double2(0.0, 0.0);
        if (i < rows && c < L) {           // the pair (c, c + 1) lies within L rounded up to 2
          a[r][j] = *reinterpret_cast<const double2*>(ap + c);
          if (c + 1 >= L) a[r][j].y = 0.0;   // the pad column of an odd L: read, never used
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = s * R + r;
      double dot = 0.0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) dot = fma(a[r][j].y, vv[j].y, fma(a[r][j].x, vv[j].x, dot));
      dot = o2m_wave_sum(dot, lane);
      const double ui = i < rows ? dot - (d ? d[i] : 0.0) : 0.0;
      if (lane == 0 && i < rows) u[i] = ui;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        zz[j].x = fma(ui, a[r][j].x, zz[j].x);
        zz[j].y = fma(ui, a[r][j].y, zz[j].y);
      }
    }
  }
  o2m_block_out<NJ>(zz, lane, wave, part + (size_t)blockIdx.x * (NJ * 128));
}

// The fused pass for rows of more than 512 values (NJ >= 8 above would leave one wave per SIMD and
// nothing to hide its loads behind).  The four waves of a workgroup share each row: wave w holds
// the 128-column chunks w, w + 4, ... (NJW of them) of v and of the z accumulators, so a quarter of the registers; a row's dot is the four wave sums added in wave
// order through LDS (double-buffered by step parity: one barrier per step); the next step's rows are
// loaded before the current step's arithmetic.  Each wave owns its columns of the workgroup's partial.
template <int NJW>
__global__ __launch_bounds__(O2M_THREADS) void ppls_o2m_fused_wide_kernel(const double* __restrict__ A, int64_t ld, int rows,
                                                                           int L, const double* __restrict__ v,
                                                                           const double* __restrict__ d,
                                                                           double* __restrict__ u,
                                                                           double* __restrict__ part) {
  constexpr int R = O2M_WIDE_R;
  __shared__ double sdot[2][R][O2M_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double2 vv[NJW], zz[NJW];
#pragma unroll
  for (int j = 0; j < NJW; ++j) {
    const int c = 2 * (lane + 64 * (wave + O2M_WAVES * j));
    vv[j].x = c < L ? v[c] : 0.0;
    vv[j].y = c + 1 < L ? v[c + 1] : 0.0;
    zz[j] = make_double2(0.0, 0.0);
  }
  const int nsteps = (rows + R - 1) / R;
  auto load = [&](int s, double2 (&a)[R][NJW]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = s * R + r;
      const double* ap = A + (int64_t)i * ld;
#pragma unroll
      for (int j = 0; j < NJW; ++j) {
        const int c = 2 * (lane + 64 * (wave + O2M_WAVES * j));
        a[r][j] = make_double2(0.0, 0.0);
        if (i < rows && c < L) {
          a[r][j] = *reinterpret_cast<const double2*>(ap + c);
          if (c + 1 >= L) a[r][j].y = 0.0;
        }
      }
    }
  };
  double2 a[R][NJW], an[R][NJW];
  load(blockIdx.x, a);   // (past the last step: all zero)
  int t = 0;
  for (int s = blockIdx.x; s < nsteps; s += gridDim.x, t ^= 1) {   // workgroup-uniform: barriers inside
    load(s + (int)gridDim.x, an);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double dot = 0.0;
#pragma unroll
      for (int j = 0; j < NJW; ++j) dot = fma(a[r][j].y, vv[j].y, fma(a[r][j].x, vv[j].x, dot));
      dot = o2m_wave_sum(dot, lane);
      if (lane == 0) sdot[t][r][wave] = dot;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = s * R + r;
      const double dot = ((sdot[t][r][0] + sdot[t][r][1]) + sdot[t][r][2]) + sdot[t][r][3];
      const double ui = i < rows ? dot - (d ? d[i] : 0.0) : 0.0;
      if (threadIdx.x == 0 && i < rows) u[i] = ui;
#pragma unroll
      for (int j = 0; j < NJW; ++j) {
        zz[j].x = fma(ui, a[r][j].x, zz[j].x);
        zz[j].y = fma(ui, a[r][j].y, zz[j].y);
        a[r][j] = an[r][j];
      }
    }
  }
  double* dst = part + (size_t)blockIdx.x * (NJW * O2M_WAVES * 128);
#pragma unroll
  for (int j = 0; j < NJW; ++j)
    *reinterpret_cast<double2*>(dst + 2 * (lane + 64 * (wave + O2M_WAVES * j))) = zz[j];
}

// Two-phase, first half: u_i = a_i . v - d_i, one wave per row.
__global__ __launch_bounds__(O2M_THREADS) void ppls_o2m_av_kernel(const double* __restrict__ A, int64_t ld, int rows, int L,
                                                                   const double* __restrict__ v,
                                                                   const double* __restrict__ d,
                                                                   double* __restrict__ u) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gw = blockIdx.x * O2M_WAVES + wave, nw = gridDim.x * O2M_WAVES;
  for (int i = gw; i < rows; i += nw) {
    const double* ap = A + (int64_t)i * ld;
    double dot = 0.0;
#pragma unroll 4
    for (int c = 2 * lane; c < L; c += 128) {
      const double2 a = *reinterpret_cast<const double2*>(ap + c);
      dot = fma(a.x, v[c], dot);
      if (c + 1 < L) dot = fma(a.y, v[c + 1], dot);
    }
    dot = o2m_wave_sum(dot, lane);
    if (lane == 0) u[i] = dot - (d ? d[i] : 0.0);
  }
}

// Two-phase, second half: the partial of z over row group blockIdx.y for the 128 columns of slice
// blockIdx.x; wave w takes the group's rows w, w + 4, ...
__global__ __launch_bounds__(O2M_THREADS) void ppls_o2m_atu_kernel(const double* __restrict__ A, int64_t ld, int rows, int L,
                                                                    const double* __restrict__ u, int rows_per_group,
                                                                    double* __restrict__ part, int ldp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = 2 * (lane + 64 * (int)blockIdx.x);
  const int r0 = (int)blockIdx.y * rows_per_group;
  const int r1 = min(rows, r0 + rows_per_group);
  double2 zz[1] = {make_double2(0.0, 0.0)};
  if (c < L) {
    const bool pad = c + 1 >= L;
#pragma unroll 8
    for (int i = r0 + wave; i < r1; i += O2M_WAVES) {
      double2 a = *reinterpret_cast<const double2*>(A + (int64_t)i * ld + c);
      if (pad) a.y = 0.0;
      const double ui = u[i];
      zz[0].x = fma(ui, a.x, zz[0].x);
      zz[0].y = fma(ui, a.y, zz[0].y);
    }
  }
  o2m_block_out<1>(zz, lane, wave, part + (size_t)blockIdx.y * ldp + 128 * (size_t)blockIdx.x);
}

// z[c] = sum_b part[b][c] in a fixed order: a workgroup takes 16 columns; thread (c, g) adds the
// partials b = g, g + 16, ... in that order, then the sixteen group sums are added in order g = 0..15.
constexpr int O2M_FIN_COLS = 16, O2M_FIN_GROUPS = O2M_THREADS / O2M_FIN_COLS;
__global__ __launch_bounds__(O2M_THREADS) void ppls_o2m_finish_kernel(const double* __restrict__ part, int nb, int ldp, int L,
                                                                       double* __restrict__ z) {
  __shared__ double red[O2M_FIN_GROUPS][O2M_FIN_COLS];
  const int col = threadIdx.x % O2M_FIN_COLS, g = threadIdx.x / O2M_FIN_COLS;
  const int c = blockIdx.x * O2M_FIN_COLS + col;
  double s = 0.0;
  if (c < L)
    for (int b = g; b < nb; b += O2M_FIN_GROUPS) s += part[(size_t)b * ldp + c];
  red[g][col] = s;
  __syncthreads();
  if (g == 0 && c < L) {
    double t = red[0][col];
#pragma unroll
    for (int k = 1; k < O2M_FIN_GROUPS; ++k) t += red[k][col];
    z[c] = t;
  }
}

template <int NJ, int R>
void o2m_launch_fused(const O2mPlan& pl, const double* A, int64_t ld, int rows, int L, const double* v, const double* d,
                      double* u, double* ws, hipStream_t st) {
  hipLaunchKernelGGL((ppls_o2m_fused_kernel<NJ, R>), dim3(pl.nb), dim3(O2M_THREADS), 0, st, A, ld, rows, L, v, d, u, ws);
}

}  // namespace

extern "C" {

int64_t ppls_o2m_ws_doubles(int rows, int L, int num_cus) {
  const O2mPlan two = o2m_plan(rows, L, num_cus, PPLS_O2M_PATH_TWOPHASE);
  int64_t need = (int64_t)two.nb * two.ldp;
  if (L <= PPLS_O2M_FUSED_LMAX) {
    const O2mPlan f = o2m_plan(rows, L, num_cus, PPLS_O2M_PATH_FUSED);
    need = std::max(need, (int64_t)f.nb * f.ldp);
  }
  return need;
}

hipError_t ppls_launch_o2m_pass(const double* S, int64_t ld, int64_t row0, int64_t col0, int rows, int L,
                                const double* v, const double* d, double* u, double* z, double* ws, int num_cus,
                                int path_opt, int* path_out, hipStream_t st) {
  if (!S || !v || !u || !z || !ws || rows < 1 || L < 1 || row0 < 0 || col0 < 0) return hipErrorInvalidValue;
  if (path_opt < 0 || path_opt > 2) return hipErrorInvalidValue;
  const int64_t Lp = ((int64_t)L + 1) & ~(int64_t)1;
  if ((ld & 1) || (col0 & 1) || col0 + Lp > ld) return hipErrorInvalidValue;   // 16-byte rows, pairs within the row
  const double* A = S + row0 * ld + col0;
  if (reinterpret_cast<uintptr_t>(A) & 15) return hipErrorInvalidValue;
  const O2mPlan pl = o2m_plan(rows, L, num_cus, path_opt);
  if (!pl.path) return hipErrorInvalidValue;   // the fused path forced past its budget
  if (path_out) *path_out = pl.path;
  if (pl.path == PPLS_O2M_PATH_FUSED) {
    switch (pl.NJ) {
      case 1: o2m_launch_fused<1, 8>(pl, A, ld, rows, L, v, d, u, ws, st); break;
      case 2: o2m_launch_fused<2, 8>(pl, A, ld, rows, L, v, d, u, ws, st); break;
      case 4: o2m_launch_fused<4, 4>(pl, A, ld, rows, L, v, d, u, ws, st); break;
      case 8:
        hipLaunchKernelGGL(ppls_o2m_fused_wide_kernel<2>, dim3(pl.nb), dim3(O2M_THREADS), 0, st, A, ld, rows, L, v, d, u, ws);
        break;
      case 16:
        hipLaunchKernelGGL(ppls_o2m_fused_wide_kernel<4>, dim3(pl.nb), dim3(O2M_THREADS), 0, st, A, ld, rows, L, v, d, u, ws);
        break;
      default: return hipErrorInvalidValue;
    }
  } else {
    const int cus = num_cus > 0 ? num_cus : 256;
    const int nb_av = std::max(1, std::min((rows + O2M_WAVES - 1) / O2M_WAVES, 8 * cus));
    hipLaunchKernelGGL(ppls_o2m_av_kernel, dim3(nb_av), dim3(O2M_THREADS), 0, st, A, ld, rows, L, v, d, u);
    const int rpg = (rows + pl.nb - 1) / pl.nb;
    hipLaunchKernelGGL(ppls_o2m_atu_kernel, dim3(pl.nslices, pl.nb), dim3(O2M_THREADS), 0, st, A, ld, rows, L, u, rpg,
                       ws, pl.ldp);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ppls_o2m_finish_kernel, dim3((L + O2M_FIN_COLS - 1) / O2M_FIN_COLS), dim3(O2M_THREADS), 0, st, ws,
                     pl.nb, pl.ldp, L, z);
  return hipGetLastError();
}

}  // extern "C"
