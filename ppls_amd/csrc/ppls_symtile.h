// ppls_symtile.h -- one pass over a symmetric P x P matrix in the joint layout, a 64 x 64 block of
// its lower triangle per workgroup: what ppls_stream_tile_kernel (merge, standardise) and
// ppls_cvs_finish_kernel share.  Only the per-entry update differs between them; it comes in as a functor.
//
// A thread owns one 16-byte column pair of 8 rows of the block (a row of the block is 32 threads =
// 512 contiguous bytes); the new values go to S and into an LDS copy, from which the mirror block is
// written with the same 16-byte stores.  A diagonal block takes every entry from its lower triangle
// (as the Gram's own finish does), so S stays exactly symmetric.  Padding is written 0.  Plain HIP,
// vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int PPLS_SYM_SB = 64;        // block edge = the MFMA Gram's quadrant edge (PPLS_GQ of ppls_variances.hip)
constexpr int PPLS_SYM_THREADS = 256;  // workgroup of ppls_symtile_pass

struct PplsSymCols {
  int P, p, ldx, yend;   // live columns: [0, p) and [ldx, yend)
};

__device__ inline bool ppls_sym_col_live(const PplsSymCols& g, int c) { return c < g.p || (c >= g.ldx && c < g.yend); }

// the joint layouts the pass (and the launch functions around it) take
inline bool ppls_sym_shape_ok(int p, int ldx, int q, int ldy) {
  return p >= 1 && q >= 1 && p <= ldx && q <= ldy && ldx % 2 == 0 && ldy % 2 == 0 && (int64_t)ldx + ldy < (1 << 30);
}

// lower-triangle blocks of a P x P matrix: the grid's x extent
inline int ppls_sym_blocks(int P) {
  const int nq = (P + PPLS_SYM_SB - 1) / PPLS_SYM_SB;
  return nq * (nq + 1) / 2;
}

struct PplsSymBlock {
  int qi, qj;   // block row and column, qj <= qi
};

// block t of the lower triangle in row order: (qi, qj), qj <= qi, t = qi (qi + 1) / 2 + qj
__device__ inline PplsSymBlock ppls_sym_block(int t_blk) {
  int qi = (int)((sqrt(8.0 * t_blk + 1.0) - 1.0) * 0.5);
  while ((qi + 1) * (qi + 2) / 2 <= t_blk) ++qi;
  while (qi * (qi + 1) / 2 > t_blk) --qi;
  return PplsSymBlock{qi, t_blk - qi * (qi + 1) / 2};
}

// S_ij <- f(...) over block b of S and its mirror, by a workgroup of PPLS_SYM_THREADS.  NV (1 or 2)
// vectors of P are staged over the block's rows (a[v][r]) and columns (b[v][c]); vec[v] may be null,
// and pad[v] stands in for it and beyond P.  f(v, r, c2, a, b) gets the pair S[row r][c2, c2 + 1] of
// the block and returns its new value.  (g by value: through a reference the compiler splits the
// 16-byte loads of S.)
template <int NV, class F>
__device__ __forceinline__ void ppls_symtile_pass(double* __restrict__ S, PplsSymCols g, PplsSymBlock blk,
                                                  const double* const (&vec)[NV], const double (&pad)[NV], F f) {
  constexpr int SB = PPLS_SYM_SB;
  const int qi = blk.qi, qj = blk.qj;
  __shared__ double T[SB][SB + 1];
  __shared__ double a[NV][SB], b[NV][SB];
  const int t = threadIdx.x;
  const int P = g.P;
  if (t < 2 * SB) {
    const int c = (t < SB ? qi * SB + t : qj * SB + (t - SB));
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const double v = (vec[i] && c < P) ? vec[i][c] : pad[i];
      if (t < SB) a[i][t] = v; else b[i][t - SB] = v;
    }
  }
  __syncthreads();
  const int c2 = (t & 31) * 2, rb = t >> 5;
  const int lo = qj * SB + c2;
  const bool diag = qi == qj;
#pragma unroll
  for (int k = 0; k < SB / 8; ++k) {
    const int r = rb + 8 * k, hi = qi * SB + r;
    double2 v = make_double2(0.0, 0.0);
    if (hi < P && lo < P) {   // P is even: lo + 1 < P as well
      double* sp = S + (int64_t)hi * P + lo;
      v = *(const double2*)sp;
      v = f(v, r, c2, a, b);
      const bool lh = ppls_sym_col_live(g, hi);
      if (!lh || !ppls_sym_col_live(g, lo)) v.x = 0.0;
      if (!lh || !ppls_sym_col_live(g, lo + 1)) v.y = 0.0;
      if (!diag) *(double2*)sp = v;
    }
    T[r][c2] = v.x;
    T[r][c2 + 1] = v.y;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SB / 8; ++k) {
    const int r = rb + 8 * k;
    if (diag) {   // entry (r, c) from the lower triangle: (max, min)
      const int hi = qi * SB + r;
      if (hi < P && lo < P) {
        const double x = c2 <= r ? T[r][c2] : T[c2][r];
        const double y = c2 + 1 <= r ? T[r][c2 + 1] : T[c2 + 1][r];
        *(double2*)(S + (int64_t)hi * P + lo) = make_double2(x, y);
      }
    } else {      // the mirror block (qj, qi): row qj SB + r, columns qi SB + c2, c2 + 1
      const int mr = qj * SB + r, mc = qi * SB + c2;
      if (mr < P && mc < P) *(double2*)(S + (int64_t)mr * P + mc) = make_double2(T[c2][r], T[c2 + 1][r]);
    }
  }
}
