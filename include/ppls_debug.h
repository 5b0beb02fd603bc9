/* ppls_debug.h -- measurement and diagnostic entry points of libppls_amd.so.
 *
 * Not part of the reference's interface (include/ppls.h is the drop-in boundary): these exist for
 * bench.py's roofline and collective timings, for the parity tests that pin a production kernel by
 * name or check one statistics step in isolation, and for the tools/ trace scripts.  The same
 * library exports them; nothing on the EM path calls them.
 */
#ifndef PPLS_AMD_PPLS_DEBUG_H
#define PPLS_AMD_PPLS_DEBUG_H

#include "ppls.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sum of HIP-event durations of the statistics launches (sweep, or the cross-product tile kernel)
 * recorded since the last reset (option "timing" = N brackets every N-th launch). */
int ppls_sweep_timing(ppls_ctx* ctx, double* total_ms, int64_t* launches, int reset);
/* The split sweep's calibrated row partition (option "balance"): the per-XCD-class weights w8[8]
 * (1.0 before calibration) and up to cap of the grid + 1 row boundaries (*n_bounds = grid + 1, or 0
 * while the even split is used). */
int ppls_sweep_balance(ppls_ctx* ctx, double* w8, int64_t* bounds, int cap, int* n_bounds);
/* The communicator as RCCL reports it (ncclCommCount / ncclCommUserRank; without RCCL the
 * context's own nranks/rank, i.e. 1/0 or the host reducer's) and the summed HIP-event durations of
 * the per-iteration statistics all-reduce on the timed sweeps (option "timing"; RCCL only). */
int ppls_comm_info(ppls_ctx* ctx, int* nranks, int* rank, double* allreduce_ms, int64_t* allreduce_calls,
                   int reset);
/* Cross-product form: *ready = S is formed for the current data, *bytes_per_pass = the bytes of S
 * one iteration reads (8 P^2, P = padded p + q), *flops = 2 n_local x the lower 128 x 128 tiles of
 * P^2 as the Gram computes them, *rows_per_wave = rows of S per wave of the tile kernel. */
int ppls_xprod_info(ppls_ctx* ctx, int r, int* ready, int64_t* bytes_per_pass, double* flops, int* rows_per_wave);
/* The last formation of S: the MFMA Gram (HIP events), the all-reduce of S over ranks (wall clock
 * around the collective and its stream synchronisation; 0 on one rank) and the whole setup. */
int ppls_xprod_setup_times(ppls_ctx* ctx, double* gram_ms, double* allreduce_ms, double* total_ms);
/* The cross-product tile kernel alone, reps launches back to back between two HIP events, for the
 * current theta of an ppls_em_begin session (S formed): *ms = the average per launch.  Rewrites the
 * session's statistics buffer with that theta's (the next ppls_em_iterate recomputes it anyway). */
int ppls_xprod_tile_timing(ppls_ctx* ctx, int reps, double* ms);
/* One statistics step from S for theta: stats = [X'mu_T p x r | Y'mu_U q x r | Gram 2r x 2r], all
 * column-major, as ppls_finalize_host takes them (unit parity against the sweep and a host S B). */
int ppls_xprod_stats(ppls_ctx* ctx, const ppls_theta* th, int r, double* stats);
/* The pass of ppls_xprod_stats alone on a caller's inputs, through the launcher the EM loop uses: M = S
 * blockdiag(W, C) (P x 2r column-major, padding rows included) and stats in the kernel's own padded layout
 * [X'mu_T ldx x r | Y'mu_U ldy x r | Gram 2r x 2r], ldy = P - ldx.  S: host, row-major P x P with the X
 * block ldx wide (ldx, ldy even, >= 2), uploaded around the launch -- or NULL for the S the context holds
 * (P, ldx must then be its own); a context without data serves when S is given.  W (ldx x r) and C
 * (ldy x r): host column-major, padding rows included.  alpha, beta, gamma, delta (r each) are written
 * into the device scalars as given: no theta is involved.  1 <= r <= 16; rw rows of S per wave (1, 2, 4,
 * 8 (r <= 8); 0 = what a fit takes); with_gram 0 leaves the Gram slot unwritten (the finalize forms it);
 * stop: the value of the device stop flag the launch is given (1: both kernels return at once).  Every
 * output is written between NaN guards, which are checked (PPLS_E_NUMERIC when one was written); what
 * the launch did not write reads NaN.  *rw_used, *nt_used (nullable): the rows per wave and the
 * instantiation (1 non-temporal, 0 cached) that ran.  Bad arguments are PPLS_E_ARG before any launch. */
int ppls_xprod_pass(ppls_ctx* ctx, const double* S, int P, int ldx, const double* W, const double* C,
                    const double* alpha, const double* beta, const double* gamma, const double* delta, int r, int rw,
                    int with_gram, int stop, double* M, double* stats, int* rw_used, int* nt_used);
/* Whether the tile kernel of that pass takes its non-temporal instantiation for a P x P matrix of doubles
 * (1) or the cached one (0): 8 P^2 bytes against 200 MiB.  Host only; the launcher itself calls it. */
int ppls_xprod_tile_nt(int P);
/* Rows of S per wave of the tile kernel for r components on num_cus compute units (rw_opt 1, 2, 4 or 8
 * (r <= 8) forces it; else 2 while P / 8 >= 2 num_cus, else 1).  Host only. */
int ppls_xprod_tile_rows(int P, int r, int rw_opt, int num_cus);
/* One statistics step by the sweep for theta, the twin of ppls_xprod_stats: the kernel is the one
 * ppls_sweep_kernel names under the context's current options; stats in the same layout.  want_mu:
 * the sweep also writes the moments (its waits then drain the DMA ring instead of counting), and mu
 * (nullable) receives this rank's n_local x 2r [mu_T | mu_U], column-major.  Needs resident rows. */
int ppls_sweep_stats(ppls_ctx* ctx, const ppls_theta* th, int r, int want_mu, double* stats, double* mu);
/* One production finalize on given statistics, the twin of ppls_sweep_stats and ppls_xprod_stats for
 * the other half of an EM iteration: on a context with data loaded (p, q, the padded widths, the sums
 * of squares and N are its own) theta, the host stats ([SX p x r | SY q x r | G 2r x 2r], column-major,
 * as ppls_finalize_host takes them) and the nullable gram_cur ([W'W | C'C], 2 r^2; NULL: the scalar
 * block forms them from theta's loadings), vstate_in ([V_W | V_C], 2 r^2; NULL: identity) and xpM (the
 * M = S B buffer of a cross-product step, (ldx + ldy) x 2r column-major; then the scalar block forms
 * the Gram B'M itself and stats' G is ignored; r <= 8) are uploaded into the context's own buffers
 * and the launch goes through the function the EM loop uses, under the current options (polar1,
 * polar1_kappa, team_rows, exact_gram, vorth): teams, LDS staging and mode bits are production's.
 * iter is the kernel's logl_index (< 0: no log-likelihood; it also decides whether option "vorth"
 * re-orthonormalises the carried V on this call).  ldx, ldy: the padded widths the caller sized xpM,
 * W_next and C_next for (PPLS_E_ARG unless they are the context's).  Out, all nullable: W_next
 * (ldx x r) and C_next (ldy x r) with their padding rows (rows the launch did not write read NaN);
 * scalars = [B r | sigT r |
 * sigE sigF sigH | alpha r | beta r | gamma r | delta r] of the next theta; the moments; loglik[iter];
 * gram_nxt (2 r^2; 0 where the kernel has none, r > 10); vstate_out (2 r^2); gram_stats (4 r^2: stats'
 * Gram slot after the launch) and status3 = {the status word, the form that produced W_next, C_next:
 * 1 Cholesky-QR1, 2 Cholesky-QR2, 3 Householder (after a refused fast form, or r > 10), 4 QR type}.
 * A status that signals rank deficiency is data here: the call still returns PPLS_OK. */
int ppls_finalize_stats(ppls_ctx* ctx, const ppls_theta* th, int r, int type, int iter, const double* stats,
                        const double* gram_cur, const double* vstate_in, const double* xpM, int ldx, int ldy,
                        double* W_next, double* C_next, double* scalars, ppls_expect* mom, double* loglik,
                        double* gram_nxt, double* vstate_out, double* gram_stats, int* status3);
/* The launch geometry of the next finalize with r components and orth type under the current options,
 * from the function the launcher itself calls: *templated (1: ppls_finalize_kernel<r>, r <= 10; 0: the
 * runtime-r kernel), *KX, *KY workgroups per polar factor, *staged (members keep their rows of S in
 * LDS) and *stage_budget, the bytes of LDS the instantiation leaves for that (staged iff r x the
 * largest member's rows x 8 fits).  All nullable. */
int ppls_finalize_plan(ppls_ctx* ctx, int r, int type, int* templated, int* KX, int* KY, int* staged,
                       int64_t* stage_budget);
/* Shape facts for the roofline: bytes of X and Y one sweep reads (algorithmic), kernel variant. */
int ppls_sweep_info(ppls_ctx* ctx, int r, int64_t* bytes_per_sweep, int* variant, int* grid);
/* The sweep kernel instantiation the next EM iteration with r components launches, as text
 * (e.g. "split<5,4,512,2,false,4,4> nt"): tests assert the production kernel is the one checked. */
int ppls_sweep_kernel(ppls_ctx* ctx, int r, char* buf, int len);
/* The Gram by the int8-MFMA Chinese-remainder form (ppls_ozaki.hip) alone, for tests and
 * benchmarks: which = 0 X'X, 1 Y'Y, 2 the joint [X Y]'[X Y] (P = ldx + ldy, padding columns 0);
 * G (column-major, nullable); *nmod moduli, *L bits of the widest column's integers; ms[4] = stats +
 * residues, SYRK, CRT, total (HIP events).  PPLS_E_NUMERIC when the columns' spread is too wide. */
int ppls_gram_int8(ppls_ctx* ctx, int which, double* G, int* nmod, int* L, double* ms);
/* The per-column scalings of the last int8 Gram (x'_kj = rint(D_kj 2^shift[j]); 0 for empty and
 * padding columns): the first min(P, *count) of them, *count = its column count. */
int ppls_gram_shifts(ppls_ctx* ctx, int* shift, int P, int* count);
/* Host copies of the int8 Gram's arithmetic (no GPU needed; tests/test_ozaki_host.py): the symmetric
 * residue of x' = rint(x 2^shift) modulo the l-th modulus (|x'| < 2^62), the l-th modulus, and the
 * CRT of nmod residues (0 <= r_l < m_l) to the nearest double of the integer in (-M/2, M/2). */
int ppls_oz_residue_host(double x, int shift, int l, int* r);
int ppls_oz_crt_host(const int* r, int nmod, double* out);
int ppls_oz_modulus(int l);
/* Which Gram ran last -- forming S, or ppls_variances' X'X / Y'Y (1 int8 CRT form, 0 fp64 MFMA) -- its
 * moduli, bits and phases (ms[4]). */
int ppls_gram_info(ppls_ctx* ctx, int* int8_used, int* nmod, int* L, double* ms);
/* The path the last ppls_meta_ppls / ppls_meta_ppls_stream took: 0 none yet, 1 the host loop, 2 the
 * device loop on the split sweep (one segmented launch per EM step), 3 the device loop on the panel
 * sweep (one launch per population and step), 4 the device loop on the cross-products of resident
 * populations (option "meta_xprod"), 5 the device loop on a fold stream's matrices. */
int ppls_meta_info(ppls_ctx* ctx, int* path);
/* The population cross-products of option "meta_xprod" on this context: *npop the matrices held now
 * (0: none), *formations how often they were formed since the context was created (a fit that finds
 * them cached adds nothing), *form_ms the wall clock of the last formation (the K Grams and their
 * all-reduce).  All nullable. */
int ppls_meta_xprod_info(ppls_ctx* ctx, int* npop, int64_t* formations, double* form_ms);
/* The statistics pass of a meta EM step alone (ppls_xprod_meta.hip), as ppls_xprod_stats is for the
 * single-matrix kernel: on a context that holds population matrices -- streamed with folds, or resident
 * after a "meta_xprod" = 1 call; else PPLS_E_STATE -- the K blocks for the shared loadings W (p), C (q)
 * and params (K x 5 column-major: B_T, sigX, sigY, sigH, sigT).  stats: K x (p + q + 4), population j
 * at stats + j (p + q + 4): [X_j'mu_T p | Y_j'mu_U q | Gram 2 x 2 column-major], unpadded. */
int ppls_xprod_meta_stats(ppls_ctx* ctx, const double* W, const double* C, const double* params, double* stats);
/* Average ms of that statistics pass (both launches) over reps back-to-back passes, HIP events around
 * the batch, on the population matrices the context holds (else PPLS_E_STATE); the loadings and scalars
 * are zeroed (the time does not depend on them).  Ends an ppls_em_begin session. */
int ppls_xprod_meta_timing(ppls_ctx* ctx, int reps, double* ms);
/* Whether that pass takes its non-temporal instantiation for K matrices of P x P doubles (1) or the
 * cached one (0): decided on all K 8 P^2 bytes a step reads, against 200 MiB. */
int ppls_xprod_meta_nt(int K, int P);
/* Host only: the mu coefficients {alpha, beta, gamma, delta} the rank-1 and meta sweeps and the pass
 * above use for one population's scalars params5 = {B_T, sigX, sigY, sigH, sigT} (EMstepC_fast's
 * formulas, src/loglC.cpp:354-361, evaluated in fp64 exactly as the library stages them), so a test
 * can hand a reference the very inputs the kernel had. */
int ppls_rank1_mu_coefficients(const double* params5, double* coef4);
/* The Gram D'D alone (D = X for xory 0, Y for 1, the joint [X Y] for 2; nsplit 0 = auto; this rank's
 * rows), for tests, benchmarks and the 'o2m' starting values of the Python PPLS / PPLSi /
 * meta_PPLSi: G (p x p, q x q or (p + q) x (p + q) without padding columns, column-major,
 * nullable), *ms = the MFMA kernel's duration. */
int ppls_gram(ppls_ctx* ctx, int xory, int nsplit, double* G, double* ms);
/* The weighted instantiation of that kernel alone: G = sum_i count_i d_i d_i' over this rank's rows
 * (count: n_local host counts >= 0, else PPLS_E_ARG), xory and nsplit as for ppls_gram -- the Gram of
 * the rows with row i repeated count_i times (ppls_xprod_resample). */
int ppls_gram_weighted(ppls_ctx* ctx, int xory, int nsplit, const int32_t* count, double* G, double* ms);
/* The real-weighted instantiation alone: G = sum_i weight_i d_i d_i' over this rank's rows, each term
 * formed as (weight_i x_a) x_b (weight: n_local finite host doubles >= 0, held on the device as fp64,
 * else PPLS_E_ARG), xory and nsplit as for ppls_gram (ppls_xprod_weighted).  Weights that
 * are all 1 give ppls_gram's bits, integer weights ppls_gram_weighted's. */
int ppls_gram_weighted_real(ppls_ctx* ctx, int xory, int nsplit, const double* weight, double* G, double* ms);
/* The permuted cross block alone: C (p x q column-major, nullable) = sum_i x_i y_perm[i]' over this rank's
 * rows (perm: a permutation of 0 .. n_local - 1 on the host, else PPLS_E_ARG; nsplit 0 = auto, at most 64),
 * *ms = the MFMA kernel's duration (ppls_xprod_permute). */
int ppls_xgram_permuted(ppls_ctx* ctx, int nsplit, const int64_t* perm, double* C /* p x q col-major */, double* ms);
/* Workgroups of that kernel one compute unit holds at once (storage type f32 0 / 1). */
int ppls_xperm_occupancy(int f32);
/* Wall-clock milliseconds of the last ppls_xprod_permute with ctx as dst: ms4 = {the host check of perm,
 * staging and upload of the indices, kernel + finish (with the copy of the diagonal blocks when it was
 * due), the whole call}. */
int ppls_xperm_timing(ppls_ctx* ctx, double* ms4);
/* Workgroups of the Gram kernel one compute unit holds at once: the unweighted instantiation for the
 * storage type (f32 0 / 1), which sizes the grid and the split plan, and the count-weighted and
 * real-weighted ones -- all equal. */
int ppls_gram_occupancy(int f32);
int ppls_gram_occupancy_weighted(int f32);
int ppls_gram_occupancy_real(int f32);
/* Inverse of a batch of symmetric positive definite matrices (host A: a x p x p, column-major, stride
 * p^2) as variances.PPLS_simult inverts the observed information: method 1 the hand-written blocked
 * Cholesky + inverse (ppls_linalg.hip), 2 rocSOLVER potrf + potri.  out: the full symmetric inverses;
 * info[z] = 0, or the 1-based column of the first non-positive pivot of matrix z (then out[z] is
 * not meaningful); *ms = device time of the factorisation and inverse. */
int ppls_spd_inverse(ppls_ctx* ctx, const double* A, int p, int a, int method, double* out, int* info, double* ms);
/* The generator's Philox4x32-10 block function on the device, for known-answer checks: out[4i..4i+3]
 * = philox4x32_10(ctr[4i..4i+3], key = {key & 0xffffffff, key >> 32}), i < count (host arrays).
 * The generator uses ctr = {pair lo, pair hi, stream, 0}, key = seed. */
int ppls_philox4x32_10(ppls_ctx* ctx, const uint32_t* ctr, int64_t count, uint64_t key, uint32_t* out);

/* Wall-clock stamps of the last finalize's phases (PPLS_FTRACE_LEN = 3 blocks x 16 slots; 0 = slot
 * not reached) and the tick length in ns.  Requires set_option("ftrace", 1). */
#define PPLS_FTRACE_LEN 48
int ppls_finalize_trace(ppls_ctx* ctx, int64_t* stamps, double* tick_ns);
/* Wall-clock stamps of the last split sweep per workgroup (entry, ring prologue done, row loop done,
 * partials written; 4 per workgroup, row-major), up to PPLS_STRACE_MAX_WG workgroups; *n =
 * workgroups copied.  Requires set_option("strace", 1). */
#define PPLS_STRACE_MAX_WG 4096
int ppls_sweep_trace(ppls_ctx* ctx, int64_t* stamps, int cap, int* n, double* tick_ns);
/* The cross-validation calls on ctx since the last reset (ppls_set_data_from and
 * ppls_xprod_downdate with ctx as the source, ppls_heldout_sse and ppls_cv_ppls on ctx):
 * out6 = {row gathers (HIP events), held-out Gram + downdate incl. its all-reduce (wall clock, the
 * gather taken out), the fits of ppls_cv_ppls (wall clock: a host-driven loop), scoring kernel and
 * its reduction (HIP events)} in ms, then the bytes the gathers read + wrote and the bytes the
 * scoring kernel read. */
int ppls_cv_timing(ppls_ctx* ctx, double* out6, int reset);

/* The cross-products S as the context holds them (ready: formed, prepared, downdated or streamed; else
 * PPLS_E_STATE): *P = ldx + ldy and *ldx (X's padded width; Y's columns start there), and, if S is
 * not null, the P x P doubles of S (row-major; symmetric, padding rows and columns included). */
int ppls_xprod_get(ppls_ctx* ctx, double* S, int* P, int* ldx);

/* The passes of the last ppls_scale_data on this context: {column sums, centred squares, apply},
 * X and Y together: ms3 from HIP events around the pass's kernels (0 for a pass that did not run),
 * bytes3 the bytes the pass read (the apply pass: read + written) on this rank. */
int ppls_scale_timing(ppls_ctx* ctx, double* ms3, double* bytes3);

/* One fold of a context streamed with folds (ppls_stream_begin_folds): S (nullable) the P x P doubles
 * of the fold's cross-products as finished (about the global mean, standardised; row-major, padding
 * included), mean (nullable, P doubles, joint padded layout) the fold's own mean of the loaded values,
 * *n the fold's rows over all ranks. */
int ppls_stream_fold_get(ppls_ctx* ctx, int fold, double* S, double* mean, int64_t* n);

/* ppls_variances_xprod's information kernel alone on host inputs, uploaded and downloaded around one
 * launch: S (row-major P x P; only the p x p block at (off, off) is read, apart from the padding
 * column next to an odd block, whose value is dropped; P and off even, off + p (+ 1 for odd p) <= P),
 * a <= 16 components with cxt and w (p x a, column-major) and the scalars ctt, k1, k2, bstar (a
 * each); the kernel divides by s4 = (sigE sigE) (sigE sigE) and by N.  Out, a consecutive column-major
 * p x p matrices each: J = SSt_exp - bstar I, and the nullable sst_exp and sst_star. */
int ppls_varinfo(ppls_ctx* ctx, const double* S, int P, int off, int p, int a, const double* cxt, const double* w,
                 const double* ctt, const double* k1, const double* k2, const double* bstar, double sigE, double N,
                 double* J, double* sst_exp, double* sst_star);
/* Benchmark (tools/bench_variances_xprod.py): that kernel (J only) against the launches it replaces in
 * ppls_variances' S path -- the block copy out of S, a ppls_varmat_kernel launches, the copy of the
 * batch and the negate -- on the context's S, after a ppls_variances_xprod call with a components:
 * reps times each between HIP events after one untimed round; *ms_new, *ms_old = the averages.  It reads
 * the statistics and loadings that call left on the context (PPLS_E_STATE without it) and runs with
 * every scalar set to 1: the times do not depend on the values, and the matrices it forms in its own
 * scratch are meaningless and freed on return; no output of the context changes. */
int ppls_varinfo_timing(ppls_ctx* ctx, int xory, int a, int reps, double* ms_new, double* ms_old);

/* The 'o2m_xprod' pass alone (ppls_o2m.hip) on a host matrix S (row-major P x ld, uploaded and
 * downloaded around one launch): for the block of `rows` rows from row0 and L columns from col0 (row0
 * + rows <= P, col0 even, ld even, col0 + L rounded up to 2 <= ld), u_i = a_i . v - d_i (rows values)
 * and z = sum_i u_i a_i (L values); d may be NULL (0).  Option "o2m_path" picks the path; *path = the
 * one taken (1 fused, 2 two-phase).  Forcing the fused path past its budget is PPLS_E_ARG. */
int ppls_o2m_pass(ppls_ctx* ctx, const double* S, int P, int ld, int row0, int col0, int rows, int L, const double* v,
                  const double* d, double* u, double* z, int* path);
/* The last ppls_o2m_start (or the last start inside ppls_ppls_o2m): side (0: the block's rows are X's
 * columns, q <= p; 1: Y's), path of its passes, Lanczos passes (operator applications), the residual
 * estimate |beta_m s_m| and theta = sigma_1^2; *fits = rank-1 device fits of the last ppls_ppls_o2m,
 * counted by the sequential loop after each fit (not by the starts). */
int ppls_o2m_info(ppls_ctx* ctx, int* side, int* path, int* passes, double* resid, double* theta, int* fits);
/* Benchmark (tools/bench_o2m.py): reps back-to-back passes on the context's S (which must be ready)
 * between HIP events after one untimed pass; *ms = the average, *bytes = the 8 rows L bytes of A. */
int ppls_o2m_pass_timing(ppls_ctx* ctx, int reps, double* ms, double* bytes, int* path);

/* Benchmark (tools/rowdiag_timing.py): the row diagnostics kernel over all local rows with r
 * components, reps launches between HIP events after one untimed launch; ms[0] = the average
 * without, ms[1] with the posterior means written.  Unit loadings and scalars (the time does not
 * depend on the values); the results go to scratch of the call. */
int ppls_rowdiag_timing(ppls_ctx* ctx, int r, int reps, double* ms /* [2] */);
/* Benchmark (tools/bench_robust.py): the weights and t log-likelihood kernels of ppls_robust_weights alone
 * over all local rows (24 B read, 16 B written per row), reps launches between HIP events after one
 * untimed launch; ms[0] = the average for one nu, ms[1] for 16.  The results go to scratch of the call:
 * kept weights are not touched. */
int ppls_robust_timing(ppls_ctx* ctx, int reps, double* ms /* [2] */);

/* ppls_adjust_data's coefficient pass and its reduce alone on the resident rows with a caller-supplied
 * Q (this rank's n_local x k1 rows, row-major; 1 <= k1 <= 16): G (k1 x (p + q), row-major) = Q'[X Y]
 * over all ranks' rows.  The data are not modified.  Collective when the rows are sharded. */
int ppls_adjust_coef(ppls_ctx* ctx, const double* Q, int k1, double* G);
/* What those passes run for k1 design columns on the resident rows: *kt the tile (4, 8 or 16) and
 * plans[10] = {tx, ty, grid_x, grid_y, nblocks} of X's launch, then of Y's (ppls_scale_plan). */
int ppls_adjust_info(ppls_ctx* ctx, int k1, int* kt, int64_t* plans);
/* sum_a G_aj^2 per column (p + q values) of the last ppls_adjust_data on these data: the sum of
 * squares the design explained (with an intercept: the mean's share included). */
int ppls_adjust_explained(ppls_ctx* ctx, double* ss);
/* ppls_xprod_adjust's Schur kernel alone on a host matrix, uploaded and downloaded around one launch
 * (and, with scale = 1, the stream's standardise pass with d_j = sqrt(S_jj): a unit diagonal): S_src
 * is row-major (ldx + ldy_src)^2 in the joint layout of p and q_src columns, its last k real Y columns
 * the covariates; S_dst receives the (ldx + ldy_dst)^2 matrix of p and q_src - k columns (ldx, ldy_src,
 * ldy_dst even, ldy_dst <= ldy_src).  The output is written between NaN guards, which are checked. */
int ppls_xadjust_matrix(ppls_ctx* ctx, const double* S_src, int p, int ldx, int q_src, int ldy_src, int k, int ldy_dst,
                        int scale, double* S_dst);
/* HIP-event times (ms) of the last coefficient pass (partials + reduce, X and Y), apply pass, Schur pass
 * and, behind a Schur pass with scale = 1, the stream's standardise pass on the same matrix (else 0) on
 * this context (ppls_xprod_adjust records on dst). */
int ppls_adjust_timing(ppls_ctx* ctx, double* ms4);

/* ---- PO2PLS ----
 * The statistics pass and the Gram alone on a caller's S: M = S blockdiag(Gx, Gy) (P x (kx + ky),
 * column-major), Q = G'M ((kx + ky)^2) and GG = [Gx'Gx (kx^2) | Gy'Gy (ky^2)].  S: host, row-major
 * P x P with the X block ldx wide (ldx, P - ldx even), uploaded around the launches -- or NULL for the
 * S the context holds (P, ldx must then be its own).  Gx: ldx x kx, Gy: (P - ldx) x ky host
 * column-major, padding rows included; 1 <= kx, ky <= 16.  rw: rows of S per wave (1, 2, 4, 8 (a
 * width <= 8); 0 = what the fit takes).  Every output is written between NaN guards, which are
 * checked.  A context without data serves when S is given. */
int ppls_po2_stats(ppls_ctx* ctx, const double* S, int P, int ldx, const double* Gx, int kx, const double* Gy, int ky,
                   int rw, double* M, double* Q, double* GG);
/* The small kernel alone on given Q, GG = [Gx'Gx | Gy'Gy] and the scalars of th (its loadings are not
 * read), for p, q real columns, N rows and the traces ssqX, ssqY: the moment blocks and K into out
 * (Cxt.. are not written), the log-likelihood, and the kernel's status word (0, or PPLS_PO2_ST_*: -21
 * a sigma, -22 Lambda not positive definite).  Returns PPLS_E_NUMERIC with out and *loglik untouched
 * when the status is not 0. */
int ppls_po2_small(ppls_ctx* ctx, const double* Q, const double* GG, const ppls_po2_theta* th, int r, int rx, int ry,
                   int p, int q, double N, double ssqX, double ssqY, ppls_po2_expect* out, double* loglik, int* status);
/* One ECM step at theta exactly as the device leaves it -- pass, Gram, small kernel, loading update of
 * the given orth type -- with NO canonical form applied: theta_out (caller's buffers, written only on
 * success) carries the column signs and order of the update itself (the check of R's QR sign rule). */
int ppls_po2_em_step(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, int type, ppls_po2_theta* theta_out);
/* HIP-event times (ms per launch, reps launches back to back each) on the context's S at theta:
 * ms6 = {the pass (both panels), the Gram, the small kernel, the loading update (polar type), one whole
 * iteration, the loading update of the QR type -- the same work without the Jacobi polar factor}.
 * Theta on the device is restored between the parts; nothing of the context changes. */
int ppls_po2_timing(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, int reps, double* ms6);
/* The twin of ppls_po2_stats for the batched pass: m models' loadings side by side, Gx
 * ldx x sum kx and Gy (P - ldx) x sum ky (host, column-major, padding rows included), through the shared
 * panel launches in chunks of 16 columns and the batched Gram.  Outputs packed model after model:
 * M (P x (kx_j + ky_j)), Q ((kx_j + ky_j)^2), GG ([kx_j^2 | ky_j^2]).  1 <= m <= 256; S as in
 * ppls_po2_stats.  Every output lies between NaN fills, which are checked. */
/* HIP-event times (ms per EM iteration: the mean over reps rounds of `steps` forced iterations each, after one
 * untimed round) on the context's S for m models from their thetas: ms4 = {one batched iteration (shared panels, one
 * Gram, small and update launch for all models), the same iteration of the m models one after another through the
 * single-model launches, the batched pass alone (panels and Gram), the m single passes one after another}.  Device
 * time only: no uploads, no read-back.  Nothing of the context changes. */
int ppls_po2_timing_batch(ppls_ctx* ctx, int m, const ppls_po2_theta* th, const int* r, const int* rx, const int* ry,
                          int steps, int reps, double* ms4);
int ppls_po2_stats_batch(ppls_ctx* ctx, const double* S, int P, int ldx, int m, const int* kx, const int* ky,
                         const double* Gx, const double* Gy, double* M, double* Q, double* GG);

/* What ppls_po2_row_diagnostics runs for p, q columns of a storage type (f32: 0 or 1) and sizes (r, rx, ry):
 * the tile (8 or 16) of the X block (kx = r + rx columns) and of the Y block (ky = r + ry), and the rows a
 * wave owns at a time.  Host only.  PPLS_E_ARG: sizes outside §26's.  All outputs nullable. */
int ppls_po2_rowdiag_info(int p, int q, int f32, int r, int rx, int ry, int* tile_x, int* tile_y, int* rows_per_wave);
/* Benchmark (tools/bench_po2_rowdiag.py): the PO2PLS row kernel over all local rows at theta, reps launches
 * between HIP events after one untimed launch; ms[0] = the average without, ms[1] with the posterior means
 * written.  The results go to scratch of the call. */
int ppls_po2_rowdiag_timing(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, int reps, double* ms /* [2] */);

#ifdef __cplusplus
}
#endif
#endif /* PPLS_AMD_PPLS_DEBUG_H */
