// ppls_xprod_phase.h -- the column-tile phase of a pass over the cross-products S, shared by the
// PPLS_simult tile kernel (ppls_xprod.hip) and the PO2PLS panel kernel (ppls_po2.hip): a wave's RW
// rows of S against R columns of B over `width` columns of S, B staged in LDS per tile, S in a
// register ring.  Moved here verbatim from ppls_xprod.hip (as ppls_symtile.h was from the Gram), so
// ppls_xprod_tile_kernel's instantiations are the ones they were.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef PPLS_XP_DEPTH
#define PPLS_XP_DEPTH 1   // staged tiles of S in flight per wave (1: loaded right before use; round 3: 2, 3, 4, 6
                          // equal within 1 %; round 4, with two sub-tiles per barrier at r <= 5: 1 is fastest --
                          // C3 tile 22.9 -> 21.7 us, C5 202 -> 200 us; profiles/r4_xprod_depth_ab_*.txt)
#endif
#ifndef PPLS_XP_WAVES
#define PPLS_XP_WAVES 0   // waves per tile-kernel workgroup sharing each staged B tile (0: ppls_xp_waves)
#endif
#ifndef PPLS_XP_TPB
#define PPLS_XP_TPB 0     // 128-column sub-tiles per staged B tile and workgroup barrier (0: ppls_xp_tpb)
#endif

namespace {

// Sub-tiles per staged B tile (one workgroup barrier each): 2 for r <= 5 (C3: tile 23.5 -> 22.9 us),
// else 1 (C5, r = 10: 2 is 6 % slower, 4 is slower at C3; profiles/r4_xprod_tpb_ab.txt).
constexpr int ppls_xp_tpb(int r) { return PPLS_XP_TPB > 0 ? PPLS_XP_TPB : (r <= 5 ? 2 : 1); }
// Waves per workgroup: 8 for r <= 5 (C3 tile 21.7 -> 21.5 us), else 4 (C5: 8 is 1-3 % slower, 2 is
// 25 % slower everywhere; profiles/r4_xprod_waves8_depth1_ab.txt, r4_xprod_waves2_ab.txt).
constexpr int ppls_xp_waves(int r) { return PPLS_XP_WAVES > 0 ? PPLS_XP_WAVES : (r <= 5 ? 8 : 4); }

// Values a lane holds after ppls_rs's six butterfly levels on M values (M > 64: several).
constexpr int ppls_rs_left(int m, int l) { return l == 6 ? m : (m == 1 ? 1 : ppls_rs_left((m + 1) / 2, l + 1)); }

// Row-tile form: a workgroup owns 4 RW rows of S (RW per wave) and walks the columns
// in tiles of 128 -- first the X columns, then the Y columns.  Each tile's 128 x R values of B (W on
// X columns, C on Y columns) are staged in LDS once per workgroup and read by all its rows, so W and
// C cost ~R / (4 RW) of S's traffic from L2.  S tiles are loaded into a register ring
// PPLS_XP_DEPTH - 1 staged tiles ahead of their use (default: none -- the 16 resident waves per CU
// keep enough bytes in flight, and fewer live registers measured faster), B one tile ahead through
// LDS; one barrier per staged tile of ppls_xp_tpb(R) 128-column sub-tiles.
template <int R, int RW, bool NT>
__device__ __forceinline__ void ppls_xprod_tile_phase(const double* const (&srow)[RW], const double* __restrict__ Bsrc,
                                                      int ldb, int width, int soff, double (&acc)[RW * R + 1],
                                                      double* __restrict__ sB, int lane) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  constexpr int TP = ppls_xp_tpb(R);         // 128-column sub-tiles per staged tile (one barrier each)
  constexpr int TV = TP * R * 64;            // 16-B values of B per staged tile
  constexpr int NTH = 64 * ppls_xp_waves(R);
  constexpr int NB = (TV + NTH - 1) / NTH;   // 16-B B loads per thread and tile
  constexpr int D = PPLS_XP_DEPTH;           // S tiles in flight per wave (register ring)
  const int tid = threadIdx.x;
  const int ntile = (width + 128 * TP - 1) / (128 * TP);
  if (ntile == 0) return;
  d2v bn[NB], ring[D][RW][TP];
  auto ld_s = [&](int n, d2v (&dst)[RW][TP]) {   // tile n: S values of this lane's two columns per sub-tile
#pragma unroll
    for (int sp = 0; sp < TP; ++sp) {
      const int c = (n * TP + sp) * 128 + 2 * lane;
#pragma unroll
      for (int rr = 0; rr < RW; ++rr) {
        if (c < width) {
          if constexpr (NT) dst[rr][sp] = __builtin_nontemporal_load((const d2v*)(srow[rr] + soff + c));
          else dst[rr][sp] = *(const d2v*)(srow[rr] + soff + c);
        } else {
          dst[rr][sp] = d2v{0.0, 0.0};
        }
      }
    }
  };
  auto ld_b = [&](int n) {   // tile n: this thread's share of the TP x 128 x R values of B
#pragma unroll
    for (int v = 0; v < NB; ++v) {
      const int e = tid + NTH * v, sp = e / (R * 64), f = e - sp * R * 64, t = f >> 6;
      const int cb = (n * TP + sp) * 128 + 2 * (f & 63);
      bn[v] = (e < TV && cb < width) ? *(const d2v*)(Bsrc + (int64_t)t * ldb + cb) : d2v{0.0, 0.0};
    }
  };
  auto st_b = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NB; ++v) {
      const int e = tid + NTH * v;
      if (e < TV) ((d2v*)sB)[buf * TV + e] = bn[v];
    }
  };
#pragma unroll
  for (int u = 0; u < D - 1; ++u)
    if (u < ntile) ld_s(u, ring[u]);
  ld_b(0);
  st_b(0);
  __syncthreads();
  for (int n0 = 0; n0 < ntile; n0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int n = n0 + u;
      if (n >= ntile) break;
      // B of the next tile first: the wait for it before st_b (vmcnt counts in issue order) then
      // leaves the S loads issued after it in flight
      if (n + 1 < ntile) ld_b(n + 1);
      if (n + D - 1 < ntile) ld_s(n + D - 1, ring[(u + D - 1) % D]);
#pragma unroll
      for (int sp = 0; sp < TP; ++sp) {   // sub-tiles in column order: the sums equal TP = 1's
        const d2v* b = (const d2v*)sB + (n & 1) * TV + sp * R * 64 + lane;
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const d2v bv = b[t * 64];
#pragma unroll
          for (int rr = 0; rr < RW; ++rr)
            acc[rr * R + t] = fma(ring[u][rr][sp].y, bv.y, fma(ring[u][rr][sp].x, bv.x, acc[rr * R + t]));
        }
      }
      if (n + 1 < ntile) st_b((n + 1) & 1);
      __syncthreads();
    }
  }
}

}  // namespace
