// ppls_o2m.h -- launch interface of the one-pass operator behind the 'o2m_xprod' starting values
// (ppls_o2m.hip): for a block A (rows x L, row-major, row stride ld) of the cross-products S,
//   u_i = a_i . v - d_i   (i over rows),   z = sum_i u_i a_i   (L values).
// With d = Wp T' (A'Wp)' v this is one application of M'M for the deflated M = P_k .. P_1 A Q_1 .. Q_k
// (EM_W_multi.R:270-271), whose first eigenpair is o2m's W., C. (:126-131).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define PPLS_O2M_PATH_AUTO 0
#define PPLS_O2M_PATH_FUSED 1      // A read once: v and the z accumulators in registers
#define PPLS_O2M_PATH_TWOPHASE 2   // u = A v - d, then z = A'u over column slices: A read twice
#define PPLS_O2M_FUSED_LMAX 2048   // the fused path's register budget: 16 column pairs per lane

extern "C" {
// Doubles of workspace a pass over rows x L needs (any path).
int64_t ppls_o2m_ws_doubles(int rows, int L, int num_cus);

// One pass.  A = S + row0 * ld + col0 must be 16-byte aligned with ld even (checked:
// hipErrorInvalidValue); only columns [col0, col0 + L rounded up to 2) of rows [row0, row0 + rows)
// are read.  v (L), d (rows; NULL = 0), u (rows), z (L) and ws are device pointers.  Every sum runs
// in an order fixed by (rows, L, num_cus) alone: workgroup partials of z go to ws and are added in a
// fixed order by a second kernel, so two launches agree bit for bit.  *path_out (host, may be NULL)
// = the path taken.
hipError_t ppls_launch_o2m_pass(const double* S, int64_t ld, int64_t row0, int64_t col0, int rows, int L,
                                const double* v, const double* d, double* u, double* z, double* ws, int num_cus,
                                int path_opt, int* path_out, hipStream_t st);
}
