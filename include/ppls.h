/* ppls.h -- C ABI of the MI355X-native PPLS_simult EM inner loop (libppls_amd.so).
 *
 * Drop-in boundary for the hot path of selbouhaddani/PPLS (paths relative to the reference):
 *   - the only native call on the loop today is
 *       .Call('PPLS_loglC_fast', PACKAGE='PPLS', W, C, X, Y, sigX, sigY, sig2T, c1, c2, c3, Kc)
 *     Package/PPLS/R/RcppExports.R:32-34 -> Package/PPLS/src/RcppExports.cpp:79-99
 *     -> Package/PPLS/src/loglC.cpp:318-338;              replaced by ppls_loglC_fast()
 *   - the R closures on the loop have no native boundary; their C-ABI counterparts are
 *       Expect_M   Package/PPLS/R/EM_W_multi.R:637-717      -> ppls_estep()
 *       Maximiz_M  Package/PPLS/R/EM_W_multi.R:729-742      -> ppls_mstep()
 *       Expect_M %>% Maximiz_M (one loop body, :782)         -> ppls_em_step()
 *       logl_W     Package/PPLS/R/EM_W_multi.R:297-323      -> ppls_loglik()
 *       PPLS_simult loop :780-807 (given theta0)             -> ppls_em_run()
 *
 * Conventions: all matrices crossing the ABI are column-major fp64 (R's layout), sizes are
 * int64_t for the sample dimension, the caller owns every host buffer, the context owns every
 * device buffer.  No exception crosses the ABI: every call returns PPLS_OK (0) or a negative
 * PPLS_E_* code, with a message in ppls_last_error(ctx).  A context is bound to one GPU and one
 * host thread; it is not re-entrant.
 */
#ifndef PPLS_AMD_PPLS_H
#define PPLS_AMD_PPLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPLS_OK 0
#define PPLS_E_ARG (-1)     /* invalid argument (R: stop()) */
#define PPLS_E_HIP (-2)     /* HIP runtime / device error */
#define PPLS_E_NUMERIC (-3) /* rank-deficient X'mu_T / Y'mu_U, non-finite update */
#define PPLS_E_STATE (-4)   /* no data loaded / wrong call order */
#define PPLS_E_COMM (-5)    /* RCCL error */
#define PPLS_E_NOMEM (-6)   /* device allocation failed */

#define PPLS_ORTH_SVD 0 /* orth(., type = "SVD"): polar factor U V' (default of PPLS_simult) */
#define PPLS_ORTH_QR 1  /* orth(., type = "QR"):  qr.Q(qr(.)) */

#define PPLS_LAYOUT_COLMAJOR 0 /* R matrices */
#define PPLS_LAYOUT_ROWMAJOR 1

typedef struct ppls_ctx ppls_ctx;

/* theta = (W, C, B, sigE, sigF, sigH, sigT) of Expect_M's argument list (EM_W_multi.R:637). */
typedef struct {
  double* W;    /* p x r column-major */
  double* C;    /* q x r column-major */
  double* B;    /* r: diag(B) */
  double* sigT; /* r: diag(sigT) (standard deviations) */
  double sigE;  /* == sigX */
  double sigF;  /* == sigY */
  double sigH;
} ppls_theta;

/* Expect_M's return list (EM_W_multi.R:715-716).  Ctt, Cuu, Cut are diagonal r x r matrices in the
 * reference; only their diagonals are exchanged.  mu_T / mu_U may be NULL (not requested). */
typedef struct {
  double* mu_T; /* n_local x r column-major (this rank's rows) */
  double* mu_U; /* n_local x r column-major */
  double* Ctt;  /* r */
  double* Cuu;  /* r */
  double* Cut;  /* r */
  double Cee;
  double Cff;
  double* Chh;  /* r x r column-major */
} ppls_expect;

int ppls_version(void);
const char* ppls_strerror(int code);

/* ---- context ---------------------------------------------------------------------------- */
int ppls_ctx_create(int device, ppls_ctx** out);
void ppls_ctx_destroy(ppls_ctx* ctx);
const char* ppls_last_error(const ppls_ctx* ctx);
/* keys: "sweep" (0 auto: the single-pass split sweep where W, C and the X'mu accumulators fit in
 *                registers, else the panel sweep; 3 panel (wide p, two passes)),
 *       "rows_per_step" (split sweep: 0 auto, 1, 2), "pipe" (split sweep software pipelining, 0/1),
 *       "grid" (workgroups, 0 = auto),
 *       "polar1" (finalize polar factor: 1 (default) one Cholesky-QR pass when
 *                 ||R1||_F ||R1^-1||_F <= k (R1 = chol(S'S)), else Cholesky-QR2; 0 always Cholesky-QR2),
 *       "polar1_kappa" (that bound k: 0 = the default min(8 r, 40); up to 255),
 *       "exact_gram" (finalize: 1 (default) the Gram W'W, C'C of the new loadings exactly, 0 the
 *                     identity -- faster, less accurate at small sigma_E),
 *       "team_rows" (finalize polar factor: rows of S per workgroup of a team; 0 = default 2048),
 *       "dtype" (storage of X, Y: 0 fp64, 1 fp32; arithmetic stays fp64; set before loading data),
 *       "nt" (sweep loads with the non-temporal cache policy: -1 auto (default: when X, Y exceed
 *             the 256 MB MALL), 0 off, 1 on),
 *       "timing" (N > 0: record HIP events around every N-th sweep launch; 0 off),
 *       "balance" (split sweep row partition: 0 (default) the even split -- bitwise reproducible
 *                  across processes; 1 per-XCD weights calibrated once per context and data shape
 *                  with 8 timed launches, from 2048 rows per workgroup: ~0.5 % faster at C3, but
 *                  the row grouping of the sums, hence the last bits, then vary between contexts),
 *       "xprod" (statistics of ppls_em_run / ppls_em_iterate: 0 (default) one streaming sweep over X, Y
 *                per iteration; 1 from the cross-products S = [X Y]'[X Y], formed once per data set
 *                on MFMA and all-reduced once, after which an iteration reads S (8 (p+q)^2 bytes) and
 *                needs no collective; -1 auto: S when a cost model of max_steps iterations says so
 *                and S with its Gram partials fits the smallest free HBM over all ranks (measured when
 *                the data were loaded; falls back to streaming, on every rank alike, if S cannot be
 *                allocated); S stays resident (8 (p+q)^2 bytes) until the data change, xprod goes from
 *                non-zero to 0 (not for an S of ppls_xprod_prepare), or ppls_xprod_release; setting 0
 *                ends an ppls_em_begin session that reads S: ppls_em_iterate then returns
 *                PPLS_E_STATE until the next ppls_em_begin -- never a silent switch to streaming),
 *       "meta_device" (ppls_meta_ppls: 1, default, the whole loop on the device -- the statistics of
 *                      every population from one read of X, Y per EM step (the split sweep: one
 *                      segmented launch; fp32 storage / wide p, the panel sweep: one launch per
 *                      population); 0 the per-population loop driven by the host),
 *       "meta_xprod" (ppls_meta_emstep / ppls_meta_ppls on resident rows: 0, default, sweep the rows
 *                     every EM step; 1 take every statistic from the populations' cross-products
 *                     S_j = [X_j Y_j]'[X_j Y_j]: formed once on the fp64 MFMA Gram from each
 *                     population's local row block (either storage type; "gram_int8" does not apply),
 *                     all-reduced once when sharded (all K matrices in one all-reduce, after the ranks
 *                     agreed that each could allocate them: else PPLS_E_NOMEM on every rank alike), then
 *                     an EM step reads K 8 (p+q)^2 bytes and needs no collective.  The K matrices stay
 *                     with the pop_local / pop_total they were formed for -- a second fit with other
 *                     starting values or atol forms nothing -- until the data change (ppls_set_data,
 *                     ppls_generate_synthetic, ppls_scale_data, ppls_set_data_from, a stream), other
 *                     populations are passed, meta_xprod goes to 0 or ppls_ctx_destroy.  The
 *                     populations' sums of squares stay those of the rows.  Takes precedence over
 *                     "meta_device"; at most 1024 populations.  One formation costs about one full
 *                     Gram, so it pays only for long or repeated fits: opt-in),
 *       "gram_int8" (the Gram that forms S and ppls_variances' X'X: 0, default, fp64 MFMA; 1 the
 *                    int8-MFMA Chinese-remainder form when the columns' spread allows it -- else the
 *                    fp64 one; ppls_gram_info.  Its residue planes (17 x n x (p + q) bytes at C3's
 *                    spread) are a workspace kept between formations -- also across
 *                    ppls_xprod_release and new data -- until gram_int8 = 0 or ppls_ctx_destroy; a
 *                    device allocation of the library that fails frees them and tries again),
 *       "vorth" (the finalize re-orthonormalises the Jacobi warm start it carries between
 *                iterations every vorth-th iteration: 1 .. 255, default 8),
 *       "xprod_rw" (rows of S per wave of the cross-product tile kernel and of the meta statistics pass
 *                   over the population matrices: 0 auto -- each kernel's own rule --, 1, 2, 4, 8),
 *       "xprod_fuse" (1, default: the finalize after a cross-product step forms the 2r x 2r Gram
 *                     itself when r <= 8 and p + q <= 6144; 0: a separate Gram kernel),
 *       "dots_rows" (panel sweep dots: rows per wave, 0 auto (64 from 32768 rows, else 32), 32, 64),
 *       "dots_pair" (panel sweep dots: a wave pair per row tile, -1 auto (when row tiles are fewer
 *                    than resident wave slots), 0, 1),
 *       "acc_chunks" (panel sweep accumulation: row chunks, 0 auto, else that many),
 *       "var_chol" (ppls_variances' inverse of the observed information: 1, default, the
 *                   hand-written batched Cholesky + inverse (ppls_linalg.hip); 2 rocSOLVER
 *                   potrf/potri; 0 rocSOLVER LU getrf/getri; a matrix that is not positive definite
 *                   sends the batch to LU, as R's solve() would) */
int ppls_set_option(ppls_ctx* ctx, const char* key, int64_t value);

/* ---- multi-GPU: samples are sharded over ranks; one RCCL all-reduce per EM iteration ---- */
void ppls_shard_range(int64_t n_total, int nranks, int rank, int64_t* row0, int64_t* n_local);
int ppls_comm_unique_id(char id[128]);
int ppls_comm_init(ppls_ctx* ctx, int nranks, int rank, const char id[128]);
/* Host-side reduction in place of RCCL (MPI, gloo, a test harness, k contexts on one GPU, ...):
 * fn(user, buf, count) must replace buf[0..count) by its element-wise sum over all ranks and return
 * 0 (non-zero -> PPLS_E_COMM).  Every collective of the library (per-iteration sufficient statistics,
 * ||X||^2 and ||Y||^2, population and deflation sums, variances) then runs device -> host -> fn ->
 * device, synchronously, in the same order on every rank.  fn = NULL restores RCCL (or no
 * reduction).  Collective when data is resident (||X||^2, ||Y||^2 are re-reduced). */
typedef int (*ppls_reduce_fn)(void* user, double* buf, int64_t count);
int ppls_set_reducer(ppls_ctx* ctx, ppls_reduce_fn fn, void* user);

/* ---- data (X: n_local x p, Y: n_local x q; this rank's rows of an n_total-sample problem) ----
 * A NaN or Inf anywhere in X or Y (on any rank) -> PPLS_E_ARG on every rank, with the data dropped:
 * the reference's svd() in orth() stops on non-finite data (EM_W_multi.R:732-733).  It is detected
 * from the all-reduced sums of squares, so all ranks return together (no rank waits alone in a
 * collective).  Fits (ppls_em_run, ppls_em_begin, ppls_ppls*, ppls_meta_ppls) refuse an all-zero X
 * or Y with PPLS_E_ARG: the reference's fit stops on the NA increment that data produce. */
int ppls_set_data(ppls_ctx* ctx, const double* X, const double* Y, int64_t n_local, int p, int q,
                  int layout, int64_t n_total);
/* simulC-model synthetic data generated on the device (src/loglC.cpp:268-315, r >= 1):
 * X = T W' + sigE E, Y = U C' + sigF F, U = T B + H, T = N(0,1) diag(sigT), H = sigH N(0,1);
 * counter-based Philox4x32-10 normals keyed by (seed, element index): independent of sharding. */
int ppls_generate_synthetic(ppls_ctx* ctx, int64_t n_total, int64_t row0, int64_t n_local, int p,
                            int q, int r, const ppls_theta* truth, uint64_t seed);
int ppls_get_data(ppls_ctx* ctx, double* X, double* Y, int64_t row_begin, int64_t nrows);
/* The same rows in row-major layout (X: nrows x p, Y: nrows x q, C order), streamed without a
 * device-side transpose: what a row-oriented host consumer (the CPU baseline) reads. */
int ppls_get_data_rows(ppls_ctx* ctx, double* X, double* Y, int64_t row_begin, int64_t nrows);
int ppls_data_ssq(ppls_ctx* ctx, double* ssqX, double* ssqY);   /* global (all ranks) */

/* R's scale(X, center, scale) and scale(Y, center, scale) applied to the resident data, in place
 * (columns over ALL ranks' rows): center_j = sum_i x_ij / n_total, then scale_j =
 * sqrt(sum_i (x_ij - center_j)^2 / (n_total - 1)) (center = 0: center_j = 0, R's root-mean-square),
 * then x_ij <- (x_ij - center_j) / scale_j.  fp64 arithmetic on either storage dtype (fp32 storage:
 * one rounding, at the store); fixed-order sums, so the result is bitwise repeatable.  Collective
 * when the rows are sharded: one all-reduce of p + q doubles per statistic; a rank with n_local = 0
 * still joins.  center = scale = 0 is a no-op.  PPLS_E_ARG, with the data untouched and on every
 * rank alike: scale = 1 with n_total < 2, or with a column whose scale_j is not > 0 or not finite (R
 * would fill it with NaN); the message names the block and the column, 1-based.  Afterwards the
 * context is as if the transformed matrix had been loaded with ppls_set_data: ||X||^2, ||Y||^2
 * recomputed, a resident S dropped (the next run that reads S forms it from the new values), an
 * ppls_em_begin session ended (ppls_em_iterate returns PPLS_E_STATE until the next ppls_em_begin). */
int ppls_scale_data(ppls_ctx* ctx, int center, int scale);
/* The transform the resident data carry relative to what was loaded:
 * loaded = resident * scale + center, column-wise.  p + q values each (X's columns, then Y's);
 * center 0 / scale 1 after ppls_set_data, ppls_generate_synthetic; calls of ppls_scale_data compose;
 * ppls_set_data_from copies the source's. */
int ppls_get_scaling(ppls_ctx* ctx, double* center, double* scale);

/* Covariate adjustment of the resident data, in place: X and Y <- their least-squares residuals on the
 * design [1 Z] (intercept = 1) or Z (intercept = 0) over ALL ranks' rows -- R's
 * resid(lm(cbind(X, Y) ~ Z)); centring is the case Z = 1.  Z: this rank's n_local x k host rows in
 * `layout`; k1 = k + intercept design columns, 1 <= k1 <= 16.  The host centres (intercept = 1) and
 * unit-scales Z's columns and orthonormalises them, together with the constant column, by two rounds of
 * Cholesky-QR (fixed-order sums, one all-reduce of the k1 x k1 Gram per round, and one of k + 1 doubles
 * for the means before them); the
 * device forms G = Q'[X Y] in one read of the rows (fixed-order sums, bitwise repeatable; sharded: one
 * all-reduce of G) and subtracts Q G in place: one fma chain per element in fp64 (fp32 storage: one
 * rounding, at the store).  N stays n_total: no degrees-of-freedom correction, as in the reference.
 * Aliased covariates are refused, not dropped: a column whose centred norm is at most 1e-7 of its raw
 * norm (constant beside the intercept), or whose Cholesky pivot given the columns before it is at most
 * 1e-7 (lm.fit's tol), is PPLS_E_ARG, and the message names the column, 1-based.  PPLS_E_ARG also: Z
 * NULL on a rank with rows or a NaN / Inf in Z on any rank, k < 1 or k1 > 16, n_total <= k1.
 * PPLS_E_STATE: no data, a streamed context or an open stream, data that ppls_scale_data has changed
 * (adjust before scaling: R's resid(), then scale()), data that are adjusted already.  Every refusal
 * is taken on all ranks alike and leaves the rows and the records untouched.  Afterwards the context
 * is as if the residuals had been loaded with ppls_set_data, exactly as after ppls_scale_data (||X||^2,
 * ||Y||^2 recomputed, S, the meta_xprod matrices and kept robust weights dropped, an ppls_em_begin
 * session ended); ppls_scale_data after it composes.  A rank with n_local = 0 still joins. */
int ppls_adjust_data(ppls_ctx* ctx, const double* Z, int k, int layout, int intercept);
/* The covariate part of the transform the data carry:
 *   loaded = resident * scale + center + (z - zcenter) Gamma
 * with scale, center of ppls_get_scaling (center: the column means with an intercept, else 0), zcenter
 * (k) Z's column means (0 without an intercept) and Gamma k x (p + q) row-major (X's columns, then
 * Y's), in the loaded units.  Each output nullable; *k = 0 when the data are not adjusted (nothing else
 * is written then).  ppls_set_data_from and the derived cross-product contexts copy it; ppls_set_data,
 * the generator and ppls_stream_begin clear it. */
int ppls_get_adjustment(ppls_ctx* ctx, int* k, double* zcenter, double* Gamma);
/* The same adjustment for contexts that hold only S.  src's LAST k columns of Y are the covariates
 * (its shape is p, q + k; 1 <= k <= 16, k < q_src); dst receives the cross-products of [X | Y_1..q] with
 * those columns partialled out, the Schur complement S_dd - S_dz S_zz^-1 S_zd = S_dd - F F', F = S_dz
 * L^-T, as a context that holds S and no rows (the lifecycle of ppls_xprod_resample's dst).  There is
 * no intercept here: a src that was streamed or scaled with center = 1 has removed it.  src: streamed
 * without folds, a resample / permute / weighted destination, or resident (S is then formed and kept,
 * as ppls_xprod_downdate does).  S is the same on every rank, so nothing below is collective.  scale =
 * 1: then d_j = sqrt(S_jj / (n_total - 1)) and S_ij /= d_i d_j.  dst afterwards: n_total src's, ||X||^2,
 * ||Y||^2 the traces, the scaling record src's for the kept columns composed with d, the adjustment
 * record zcenter = src's centres of the k columns and Gamma = S_zz^-1 S_zd in src's units; a repeated
 * call of unchanged shape reuses dst's S.  PPLS_E_ARG, with dst as it was: k out of range, dst == src,
 * contexts on different devices, S_zz singular (a zero diagonal entry, or a pivot of its unit-diagonal
 * form at most 1e-7; the message names the column), scale = 1 with a d_j that is not > 0 or not finite.
 * PPLS_E_STATE: src without data, with an open stream, or streamed with folds. */
int ppls_xprod_adjust(ppls_ctx* dst, ppls_ctx* src, int k, int scale);

/* ---- the hot path ------------------------------------------------------------------------ */
int ppls_estep(ppls_ctx* ctx, const ppls_theta* th, int r, ppls_expect* out);
int ppls_mstep(ppls_ctx* ctx, const ppls_expect* fit, int r, int type, ppls_theta* out);
int ppls_em_step(ppls_ctx* ctx, const ppls_theta* in, int r, int type, ppls_theta* out,
                 ppls_expect* fit /* nullable: Expect_M of `in` */);
int ppls_loglik(ppls_ctx* ctx, const ppls_theta* th, int r, double* out);
/* PPLS_simult's loop and tail (EM_W_multi.R:773-806) from an explicit theta0 (in `th`).
 * On return `th` holds the canonicalised estimates (:794-799), loglik[0..*steps_done-1] the
 * log-likelihood trace, and eout (nullable) Expect_M at the un-canonicalised final theta (:802).
 * Returns PPLS_OK; *negative_increment = 1 where the reference warns (:801).  A NaN log-likelihood
 * increment under a finite atol is R's `if (NA < atol)` error (:792): the run stops there and
 * returns PPLS_E_NUMERIC, as it does for any non-finite trace entry or estimate -- never PPLS_OK. */
int ppls_em_run(ppls_ctx* ctx, ppls_theta* th, int r, int max_steps, double atol, int type,
                double* loglik, int* steps_done, int* negative_increment, ppls_expect* eout);

/* Device-resident iteration (benchmark / long runs): ppls_em_begin uploads theta0 (canonicalised as
 * :773-778); ppls_em_iterate enqueues exactly `nsteps` EM iterations (sweep + reduce + all-reduce +
 * finalize each, no host synchronisation, no stop rule); ppls_em_state downloads the current theta
 * (un-canonicalised) and the log-likelihood history logl(theta_1..theta_{k-1}) after k iterations. */
int ppls_em_begin(ppls_ctx* ctx, const ppls_theta* theta0, int r);
int ppls_em_iterate(ppls_ctx* ctx, int nsteps, int type);
int ppls_em_state(ppls_ctx* ctx, ppls_theta* out, double* loglik, int loglik_cap, int* n_loglik);

/* ---- sequential initialiser: PPLS(X, Y, a, EMsteps, atol, initialGuess) -------------------------
 * Replaces the R functions PPLS (Package/PPLS/R/EM_W_multi.R:229-279), PPLSi (:116-180) and
 * EMstep_W (:51-73) -> .Call('PPLS_EMstepC_fast') (R/RcppExports.R:36-38, src/loglC.cpp:340-397),
 * i.e. the f0 = PPLS(X, Y, a, 20, 1e-4, 'random') that PPLS_simult starts from (:762).
 * a rank-1 EM fits, component k on X, Y deflated by components 1..k-1 (:270-271; implicit here).
 * init: a starting values (theta with r = 1: W p, C q, B[1], sigT[1], sigE, sigF, sigH), i.e. the
 * initialGuess draws the R side makes (:126-145).  Stop rule per component: increment < atol
 * (critfunc = identity), no constraints.  If a component's sigE or sigF falls below
 * 100 * DBL_EPSILON the fit stops there (:152-154, :258-263): ncomp < a. */
/* scores.PPLS (Package/PPLS/R/EM_W_multi.R:411-420): T = X W (n_local x k), U = Y C (n_local x k),
 * column-major, for this rank's rows; one pass over the resident data.  T or U may be NULL. */
int ppls_scores(ppls_ctx* ctx, const double* W, const double* C, int k, double* T, double* U);

typedef struct {
  double* W;               /* p x a, column-major (R's W) */
  double* C;               /* q x a */
  double* B;               /* a */
  double* sig;             /* a x 4, column-major: sigX, sigY, sigH, sigT (R's sig) */
  double* logvalue;        /* nullable: a x (EMsteps + 1), row k = component k's logvalue, NaN padded */
  double* last_increment;  /* nullable: a (Other_output$Last_increment) */
  int* number_steps;       /* nullable: a (Other_output$Number_steps) */
  double* loglikelihoods;  /* nullable: a (Other_output$Loglikelihoods: logl_W of X, Y, comps 1..k) */
  int ncomp;               /* out: components fitted */
  int not_monotone;        /* out: bit k set if component k's logvalue decreased (warning, :177) */
} ppls_seq_fit;
int ppls_ppls(ppls_ctx* ctx, int a, int max_steps, double atol, const ppls_theta* init, ppls_seq_fit* out);
/* PPLS / PPLSi with the reference's optional arguments: critfunc (crit_abs 0 = identity, 1 = abs)
 * and constraints = list(fconstraint(...)) per component (Package/PPLS/R/EM_W_multi.R:85-92,
 * :141-145, :165-169): each non-NULL pointer fixes that parameter (W: p, C: q, the rest: 1 value)
 * at the start and after every EM step.  cons: a entries, or NULL (no constraints). */
typedef struct {
  const double* W;
  const double* C;
  const double* B;
  const double* sigE;
  const double* sigF;
  const double* sigH;
  const double* sigT;
} ppls_constraint;
int ppls_ppls_ex(ppls_ctx* ctx, int a, int max_steps, double atol, int crit_abs, const ppls_theta* init,
                 const ppls_constraint* cons, ppls_seq_fit* out);
/* ---- 'o2m' starting values from the cross-products S (initialGuess = "o2m_xprod") ----------------
 * Replaces PPLSi's `initialGuess == "o2m"` branch (Package/PPLS/R/EM_W_multi.R:126-131; meta_PPLSi
 * :520-525): W., C. = the first singular pair of Xc'Yc, B = Tt'U / Tt'Tt, sig and siglat from ssq(Xc),
 * ssq(Yc), ssq(Tt), ssq(U), for Xc = X P_1 .. P_k, Yc = Y Q_1 .. Q_k, P_j = I - w_j w_j' (:270-271;
 * Wprev p x k, Cprev q x k column-major, 0 <= k <= PPLS_RMAX - 1; NULL when k = 0; the loadings need not
 * be orthonormal).  Everything is read off the context's working S = [X Y]'[X Y]: a streamed context,
 * a fold stream's current selection, a resample destination, or resident data -- a resident context
 * without S forms and keeps it exactly as ppls_xprod_prepare does (collective on row shards, with the
 * same agreement on allocation).  The pair is the top eigenpair of M'M, M the deflated off-diagonal
 * block with the shorter rows, by symmetric Lanczos (start 1/sqrt(L), full reorthogonalisation, host
 * recurrence) on one device pass over the block per operator application (ppls_o2m.hip); it stops at
 * a residual estimate <= 2^-43 theta, at a basis of L vectors, or after 200 passes (accepted there
 * if <= 2^-26 theta, else PPLS_E_NUMERIC).  theta <= 2^-104 ssq(X) ssq(Y), with the sums of squares of
 * the context's data before any deflation (sigma_1 within rounding of ||X|| ||Y||: the deflated X'Y
 * vanishes, theta = 0 included): PPLS_E_NUMERIC.  S formed by this call costs 8 (ldx + ldy)^2 bytes of
 * device memory (128 MB at p = q = 2000, 925 MB at p = 10^4, q = 500) and stays until
 * ppls_xprod_release or new data; an S that option xprod had formed keeps that option's lifetime.
 * Sign: the entry of W. of largest magnitude (lowest index on a tie) is positive, C. follows; R's svd
 * fixes only the joint sign, so a comparison is up to it.  Every rank holds the same S and computes
 * the same bits with no collective.  out: theta with r = 1 (W p, C q, B[1], sigT[1]). */
int ppls_o2m_start(ppls_ctx* ctx, const double* Wprev, const double* Cprev, int k, ppls_theta* out);
/* ppls_ppls_ex with component k's start taken from ppls_o2m_start on the loop's own deflation by the
 * fitted components 1..k-1 (PPLS :256-257 with PPLSi :126-131), its constraints applied on top
 * (:141-145): every component is fitted once.  The fits read S or sweep the rows as option xprod says. */
int ppls_ppls_o2m(ppls_ctx* ctx, int a, int max_steps, double atol, int crit_abs, const ppls_constraint* cons,
                  ppls_seq_fit* out);
int ppls_synchronize(ppls_ctx* ctx);

/* ---- multi-population rank-1 fits: meta_EMstep / meta_PPLSi ----------------------------------
 * Replace the R functions meta_EMstep (Package/PPLS/R/EM_W_multi.R:446-485) -> .Call meta_Estep /
 * meta_Mstep (R/RcppExports.R:40-46, src/loglC.cpp:399-474) and meta_PPLSi (:509-589): one shared
 * loading pair (W., C.) and per-population scalars (B_T, sigX, sigY, sigH, sigT).
 * Populations are contiguous row blocks in level order: population j is global rows
 * [N_1 + .. + N_{j-1}, N_1 + .. + N_j), exactly the reference's X[popui, ] with popui from
 * cumsum(table(Ipopu)) (:451-458, :537-541).  pop_local[j] = rows of population j in this rank's
 * shard (contiguous, in order; they sum to n_local), pop_total[j] = N_j over all ranks.
 * params: npop x 5 column-major, columns B_T, sigX, sigY, sigH, sigT (params[[j]] of the reference).
 * Each population is one r = 1 sweep over its rows (one all-reduce when sharded). */
int ppls_meta_emstep(ppls_ctx* ctx, int npop, const int64_t* pop_local, const int64_t* pop_total,
                     const double* W, const double* C, const double* params_in, double* W_out,
                     double* C_out, double* params_out, double* Cxt /* p x npop, nullable */,
                     double* Cyu /* q x npop, nullable */);
typedef struct {
  double* W;       /* p (out): c(Wnw) */
  double* C;       /* q (out) */
  double* params;  /* npop x 5 (out) */
  double* log;     /* nullable: (EMsteps + 1) x npop column-major logvalue; row 0 = the initial
                      rep(logl_W(X, Y, theta0), npop) (:544), rows 1..steps the EM steps; NaN padded */
  int steps;       /* out: EM steps made (the reference's i) */
} ppls_meta_fit;
/* crit_abs: 0 critfunc = identity (default), 1 critfunc = abs.  init: theta with r = 1. */
int ppls_meta_ppls(ppls_ctx* ctx, int npop, const int64_t* pop_local, const int64_t* pop_total,
                   int max_steps, double atol, int crit_abs, const ppls_theta* init, ppls_meta_fit* out);
/* The same two on a context streamed with folds (ppls_stream_begin_folds .. ppls_stream_end, below):
 * the fold labels are the populations in level order 0 .. K-1, N_j the fold's rows over all ranks; no
 * rows and no row arguments.  meta_PPLSi takes X and Y as given and splits them by Ipopu without
 * centring per population, which is exactly what the fold matrices S_j hold (centred and scaled as a
 * whole, if the stream was asked to), and every statistic of a step is a quadratic form in S_j:
 *   X_j'mu_T = S_j,xx w alpha_j + S_j,xy c beta_j,   Y_j'mu_U = S_j,yx w gamma_j + S_j,yy c delta_j,
 *   Gram([X_j w, Y_j c]) = blockdiag(w, c)' S_j blockdiag(w, c),   ssq(X_j), ssq(Y_j) = the traces of
 * S_j's diagonal blocks (summed in column order).  An EM step reads K 8 (p+q)^2 bytes in one pass with
 * fixed-order sums.  Meaning, outputs and error returns are those of ppls_meta_emstep /
 * ppls_meta_ppls, the PPLS_E_NUMERIC of a NaN increment and the refusal of all-zero X or Y included
 * (judged on all streamed rows).  ppls_meta_ppls_stream runs the whole loop on the device.
 * PPLS_E_STATE: a context not streamed with folds (a plain stream, an open stream, resident data, no
 * data) and while an ppls_em_begin session is active.  The calls read the fold matrices directly: they
 * neither need nor change the selection of ppls_stream_select.  No collective: after ppls_stream_end
 * every rank holds identical fold matrices, so every rank computes identical bits.  One population
 * cannot be streamed this way (a fold stream has K >= 2); ppls_ppls on a plain stream is that fit. */
int ppls_meta_emstep_stream(ppls_ctx* ctx, const double* W, const double* C, const double* params_in,
                            double* W_out, double* C_out, double* params_out,
                            double* Cxt /* p x K, nullable */, double* Cyu /* q x K, nullable */);
int ppls_meta_ppls_stream(ppls_ctx* ctx, int max_steps, double atol, int crit_abs, const ppls_theta* init,
                          ppls_meta_fit* out);

/* loglC_fast (src/loglC.cpp:318-338) with the reference's argument list.  X, Y (column-major
 * n x p / n x q host matrices) are uploaded into ctx like Rcpp's input_parameter copies them;
 * pass X = Y = NULL to evaluate on the data already resident in ctx (zero-copy). */
int ppls_loglC_fast(ppls_ctx* ctx, const double* W, const double* C, const double* X, const double* Y,
                    int64_t n, int p, int q, int a, double sigX, double sigY, const double* sig2T,
                    const double* c1, const double* c2, const double* c3, const double* Kc,
                    double* out);

/* ---- variances.PPLS_simult(fit, data, XorY) (Package/PPLS/R/EM_W_multi.R:830-860) ---------------
 * mu: this rank's rows of fit$Expectations$mu_T (xory 0, "X") or $mu_U (xory 1, "Y"), n_local x a
 * column-major; Cdiag: diag of $Ctt (or $Cuu), a; sigE: fit$estimates$sigE (the reference uses sigE
 * for both XorY).  Outputs (p = ncol(data)): W = orth(t(data) %*% mu, "SVD") p x a; B_exp[i]: the
 * reference's B_exp of component i is B_exp[i] * diag(p); varMatrix, SSt_exp, SSt_star (each a
 * consecutive p x p column-major matrices, nullable) and seLoad (p x a).  t(data) diag(Ctt) data is
 * Ctt * data'data: one MFMA Gram for all components. */
int ppls_variances(ppls_ctx* ctx, const double* mu, const double* Cdiag, double sigE, int a, int xory,
                   double* W, double* B_exp, double* varMatrix, double* SSt_exp, double* SSt_star,
                   double* seLoad);

/* The same list from the cross-products S = [X Y]'[X Y] alone, for contexts that hold no rows: the
 * rows enter :830-860 only through N Ctt_ii X'X (S's diagonal block), Cxt = X'mu_T and
 * W = orth(X'mu_T) (the statistic and the polar factor of one cross-product EM step at th) and
 * crossprod(mu_T[, i]) (a quadratic form in that step's Gram of [XW YC]).  th: the theta at which the
 * reference's Expectations are taken (fit$estimates); r: its components; xory 0 "X" / 1 "Y" (th->sigE
 * for both, like the reference).  Outputs as ppls_variances (W p x r, B_exp r, varMatrix / SSt_exp /
 * SSt_star r consecutive column-major p x p, seLoad p x r) plus Cdiag (r: the Ctt_ii or Cuu_ii used);
 * Cdiag, varMatrix, SSt_exp and SSt_star are nullable.  Option "var_chol" as in ppls_variances: a
 * matrix that is not positive definite sends the batch to LU.
 * Works on every context that holds S: streamed (a fold stream: the working S and N of the current
 * ppls_stream_select), the destination of ppls_xprod_resample, resident with S formed.  Resident
 * without S: S is formed as by ppls_xprod_prepare and kept -- the call's only collective; with S
 * present no rank communicates, and every rank returns the same bits.
 * PPLS_E_STATE: no data, or a stream is open.  PPLS_E_ARG: th, W, B_exp or seLoad NULL, xory not 0 or
 * 1, r outside [1, 16] or above the block's columns.  PPLS_E_NUMERIC: a rank-deficient orth or an
 * exactly singular matrix (ppls_variances' messages).  A refused call leaves the context's data and S
 * as they were (like every call that stages a theta it ends an ppls_em_begin session). */
int ppls_variances_xprod(ppls_ctx* ctx, const ppls_theta* th, int r, int xory, double* W, double* Cdiag,
                         double* B_exp, double* varMatrix, double* SSt_exp, double* SSt_star, double* seLoad);

/* ---- cross-product form (option "xprod") ----------------------------------------------------
 * Form S = [X Y]'[X Y] now (*ms = the MFMA Gram kernel time, *total_ms = with the all-reduce and
 * allocation; both nullable) -- otherwise the first run that reads S forms it.  Collective when the
 * rows are sharded: every rank calls it (one all-reduce of (p+q)^2 doubles). */
int ppls_xprod_prepare(ppls_ctx* ctx, double* ms, double* total_ms);
/* Free S (and its scratch) now; the next run that reads S forms it again.  (The int8 Gram's
 * residue planes stay: see option "gram_int8".) */
int ppls_xprod_release(ppls_ctx* ctx);

/* ---- cross-validation: predict.PPLS, cv_PPLS, crossval_PPLS ----------------------------------
 * Package/PPLS/R/crossval_PPLS.R:12-114.  The reference refits on X[-folds[ii], ], Y[-folds[ii], ]
 * (:48), copied from R into Eigen on every EM step; here a fold's training rows are gathered on the
 * device, their cross-products are S - S_fold, and the held-out rows are scored where they lie. */

/* X[rows, ], Y[rows, ] of src into dst, on the device (replaces the row subsetting of :48 and the
 * upload of its result).  rows: nrows strictly ascending local row indices into src's resident
 * data; dst then holds those rows in that order as if ppls_set_data had been called with them: src's
 * storage dtype, dst's own padded layout with zeroed slack, ||X||^2 and ||Y||^2 recomputed and
 * all-reduced, the non-finite verdict, a stale S dropped.  n_total: the subset's rows over all ranks
 * (<= 0: nrows).  With shards each rank passes its own rows; a rank with nrows = 0 still joins the
 * collectives.  PPLS_E_ARG: an index out of range or not ascending, dst == src, src without data,
 * contexts on different devices. */
int ppls_set_data_from(ppls_ctx* dst, ppls_ctx* src, const int64_t* rows, int64_t nrows, int64_t n_total);

/* dst's cross-products as src's minus the Gram of src's rows out_rows (n_out strictly ascending
 * local indices), marked ready as by ppls_xprod_prepare; src's S is formed first if it is not ready.
 * The caller guarantees that dst's data are src's rows without out_rows (what ppls_set_data_from
 * loaded); the row counts are checked, on this rank and over all ranks, and a mismatch is
 * PPLS_E_ARG on every rank.  Entrywise S - S_out carries the rounding of the Gram of all rows,
 * u sum_i |x_ij x_il| over all of them: at most K / (K - 1) times the bound of a direct Gram of the
 * training rows when 1 / K of the rows are held out.  More rows held out than kept (over all ranks)
 * is refused with PPLS_E_ARG: form S directly then.  Collective when the rows are sharded (the
 * ranks first agree that every allocation succeeded, then all-reduce the held-out Gram).  Replaces
 * the K re-reads of X[-fold, ] per EM step behind :48. */
int ppls_xprod_downdate(ppls_ctx* dst, ppls_ctx* src, const int64_t* out_rows, int64_t n_out);

/* Resampled cross-products: dst's S becomes sum_i count_i d_i d_i' over src's resident
 * rows d_i = [x_i y_i] as they stand (scaled in place or not, either storage type) -- the S of the data
 * with row i repeated count_i times, which is what a bootstrap replicate X[i, ], Y[i, ] with
 * i = sample(N, replace = TRUE) is -- by the weighted instantiation of the fp64 MFMA Gram (option
 * "gram_int8" does not apply), with no copy of the rows, all-reduced over src's ranks in the same order
 * on every rank (src's stream, Gram queue and communicator, as ppls_xprod_downdate).  count: this
 * rank's n_local non-negative counts (host).  src is left as it was: rows, its own S if formed, options,
 * an open ppls_em_begin session.  dst ends "streamed" (ppls_stream_info state 2, rows_local 0, no
 * folds): p, q, the paddings and the scaling record are src's, n_total = sum count over all ranks,
 * ||X||^2, ||Y||^2 the traces of S_c's diagonal blocks; every fit that reads only S runs on it and
 * what needs rows is refused as on any streamed context.  A repeated call on the same dst of unchanged
 * shape reuses dst's S, its device counts and its Gram partials (no allocation per replicate) and ends
 * an ppls_em_begin session of dst.
 * PPLS_E_ARG: a negative count on any rank (every rank returns it: the flag rides in the reduction of
 * sum count), sum count = 0 over all ranks, dst == src, contexts on different devices, count == NULL
 * with n_local > 0.  PPLS_E_STATE: src without data or streamed.  After such a refusal dst holds what
 * it held before; an allocation or HIP error leaves dst without data, never with a half-formed S.  A
 * rank with n_local = 0 takes part in the collectives. */
int ppls_xprod_resample(ppls_ctx* dst, ppls_ctx* src, const int32_t* count /* host, src's n_local */);

/* Permuted cross-products: dst's S becomes [X Y_pi]'[X Y_pi] with Y_pi[i, ] = Y[perm[i], ]
 * over src's resident rows as they stand (scaled in place or not, either storage type) -- the S of a
 * permutation replicate, which pairs x_i with another row's y and so destroys the X-Y link while keeping
 * both margins.  The diagonal blocks X'X and Y'Y do not depend on perm: they are copied device to device
 * from src's S, bit for bit (src's S is formed first, and kept, if it is not ready, as by
 * ppls_xprod_downdate).  Only the p x q block C_pi = sum_i x_i y_perm[i]' is formed, by a rectangular fp64
 * MFMA kernel over the rows where they lie (no copy of them, fixed-order sums: the same call gives the
 * same bits), and written into both off-diagonal blocks from one value, so S is exactly symmetric and
 * its padding zero.  perm: a permutation of this rank's 0 .. n_local - 1 (host), checked in O(n) before
 * any device work; at most 2^31 - 1 local rows (more: PPLS_E_ARG).  Sharded, each rank permutes its own
 * rows -- a permutation within shards, which is still an exact test under exchangeability of the rows --
 * and the ranks all-reduce the ldx x ldy block alone, in the same order on every rank (src's stream and
 * communicator or reducer); a rank with n_local = 0 takes part.  src is left as it was: rows, its own S,
 * options, an open ppls_em_begin session.  dst ends "streamed" (ppls_stream_info state 2, rows_local 0,
 * no folds): p, q, the paddings, the scaling record, n_total, ||X||^2 and ||Y||^2 are src's; every fit
 * that reads only S runs on it and what needs rows is refused as on any streamed context.  A repeated
 * call on the same dst of unchanged shape reuses dst's S (the diagonal blocks are not copied again while
 * src's S is the same), its device index array and its partials, and ends an ppls_em_begin session of dst.
 * PPLS_E_ARG: an entry out of range or repeated on any rank (every rank returns it: the flag rides in
 * the agreement that precedes the collective), perm == NULL with n_local > 0, dst == src, contexts on
 * different devices.  PPLS_E_STATE: src without data or streamed.  After such a refusal dst holds what it
 * held before; an allocation or HIP error leaves dst without data, never with a half-formed S. */
int ppls_xprod_permute(ppls_ctx* dst, ppls_ctx* src, const int64_t* perm /* host, src's n_local */);

/* predict.PPLS (:12-24): xory 0 ("X") pred = newdata W diag(B) C' (n x q), xory 1 ("Y") pred =
 * newdata C diag(1/B) W' (n x p); W p x k, C q x k column-major, B k, with p, q the shape of the
 * data last loaded into ctx (newdata itself is independent of the resident rows: it is streamed
 * through a device staging buffer in row blocks, in fp64 whatever the storage dtype).  newdata:
 * n x p (or n x q) host matrix in `layout`; pred: column-major.  The column-count check of :16-17 is
 * the caller's. */
int ppls_predict(ppls_ctx* ctx, const double* W, const double* C, const double* B, int k, int xory,
                 const double* newdata, int64_t n, int layout, double* pred);

/* The held-out error of :49 for every number of components at once, on the resident rows `rows`
 * (nrows strictly ascending local indices): with yhat_i(j) = sum_{m <= j} (x_i w_m) B_m c_m,
 * sse[j-1] = sum_i ||y_i - yhat_i(j)||^2 for j = 1..k, all-reduced over ranks.  One pass over X and Y
 * of those rows (fp64 arithmetic on either storage dtype), the residual formed directly, fixed-order
 * sums.  A rank with nrows = 0 still joins the all-reduce. */
int ppls_heldout_sse(ppls_ctx* ctx, const double* W, const double* C, const double* B, int k,
                     const int64_t* rows, int64_t nrows, double* sse /* k values */);

/* cv_PPLS's loop (:40-52) for given folds.  fold_of_row: the fold (0..nfolds-1) of each of this
 * rank's rows; fold_total: rows per fold over all ranks; init: nfolds x a starting values (fold f's
 * are init[f*a .. f*a+a), as for ppls_ppls).  Per fold: the other rows, in their order (R's
 * X[-folds[ii], ] keeps it), go into a training context the library creates once and reuses
 * (ppls_set_data_from; ctx's options xprod, dtype, gram_int8 and its reducer / communicator carry
 * over); if the fits read S it comes from ppls_xprod_downdate; ppls_ppls_ex fits a components;
 * ppls_heldout_sse scores the fold's rows in ctx.
 *   rmsep[f*a + j] = sqrt(sse_j / (fold_total[f] q))        (nfolds x a, fold-major)
 * is sqrt(mse(Y[fold, ], predict(fit, X[fold, ], "X"))) of :49 for the (j+1)-component fit -- PPLS is
 * sequential, so components 1..j of an a-component fit are the j-component fit, and one fit per fold
 * gives every prefix.  mse is OmicsPLS's, mse(x, y) = mean((x - y)^2); OmicsPLS is not vendored with
 * the reference, so that definition, and with it parity against an R run, is unpinned.  A fold whose
 * fit stops early (ncomp[f] < a, the rank-collapse rule of :258-263) gets NaN for the components it
 * did not reach. */
int ppls_cv_ppls(ppls_ctx* ctx, int a, int nfolds, const int32_t* fold_of_row /* n_local, 0..nfolds-1 */,
                 const int64_t* fold_total /* nfolds: rows per fold over all ranks */,
                 int max_steps, double atol, int crit_abs, const ppls_theta* init /* nfolds x a */,
                 double* rmsep /* nfolds x a, fold-major */, int* ncomp /* nfolds */);
/* The same loop with initialGuess = "o2m_xprod" (crossval_PPLS.R:47 with PPLSi :126-131 on the
 * training rows): no init; each fold's fit is ppls_ppls_o2m on the training context, whose S always
 * comes from ppls_xprod_downdate (formed from the training rows where the fold outnumbers them). */
int ppls_cv_ppls_o2m(ppls_ctx* ctx, int a, int nfolds, const int32_t* fold_of_row, const int64_t* fold_total,
                     int max_steps, double atol, int crit_abs, double* rmsep, int* ncomp);

/* ---- streamed data: fit from row chunks, no rows resident -------------------------------------
 * Since the cross-product form a PPLS_simult iteration and every rank-1 step of PPLS read only
 * S = [X Y]'[X Y] (8 (p+q)^2 bytes); the rows are needed once, to form S.  These calls form S -- of the
 * data centred and scaled as R's scale() does, if asked -- from row chunks that come from the host or
 * from another context's resident rows, so neither a host array nor HBM ever holds all rows.
 * Afterwards the context is "streamed": have data, n_local = 0, n_total = the rows streamed over all
 * ranks, S ready and kept as if by ppls_xprod_prepare.  The library never computes from the zero
 * resident rows:
 *   - statistics come from S whatever option "xprod" holds (setting it to 0 neither frees S nor ends a
 *     session): ppls_em_run, ppls_em_begin / _iterate / _state, ppls_em_step, ppls_estep,
 *     ppls_loglik, ppls_loglC_fast(X = Y = NULL), ppls_ppls / ppls_ppls_ex, ppls_data_ssq,
 *     ppls_get_scaling and ppls_predict work (ppls_ppls_ex keeps the running ||Xc||^2 where a resident
 *     context would recompute a cancelled one from the rows);
 *   - PPLS_E_STATE "the rows were streamed and are not resident", before any work: mu_T / mu_U asked of
 *     ppls_estep, ppls_em_step or ppls_em_run; ppls_mstep (X'mu_T of caller-supplied mu needs the rows);
 *     ppls_scores; ppls_get_data / _rows; ppls_variances (whose mu are rows: the standard errors of a
 *     streamed context come from ppls_variances_xprod); ppls_heldout_sse; ppls_cv_ppls;
 *     ppls_set_data_from / ppls_xprod_downdate / ppls_xprod_resample with a streamed source;
 *     ppls_scale_data;
 *     ppls_meta_emstep / ppls_meta_ppls (a context streamed with folds fits the multi-population
 *     model with ppls_meta_emstep_stream / ppls_meta_ppls_stream instead); ppls_comm_init and
 *     ppls_set_reducer (set them before ppls_stream_begin); option "dtype";
 *   - ppls_xprod_resample leaves its dst in this state too (S_c of src's resampled rows, no stream);
 *   - so does ppls_xprod_permute (S of src's rows with Y's permuted against X's, no stream);
 *   - ppls_xprod_release, ppls_set_data, ppls_generate_synthetic and ppls_stream_begin end the state
 *     (after ppls_xprod_release the context has no data).
 * While a stream is open (between begin and end) the context has no data: every fit and data entry
 * point returns PPLS_E_STATE, and so do ppls_comm_init, ppls_set_reducer and a change of option
 * "dtype" (what ppls_stream_end's collectives run over is fixed at ppls_stream_begin). */

/* Open a stream of p + q columns: drops resident data, S and an ppls_em_begin session; allocates S
 * (P x P, P = ldx + ldy in the padded layout) zeroed and the running column means; the row count
 * starts at 0.  center, scale: 0 or 1, R's meaning as in ppls_scale_data (scale without center: the
 * root-mean-square). */
int ppls_stream_begin(ppls_ctx* ctx, int p, int q, int center, int scale);
/* One chunk of nrows >= 1 rows (X nrows x p, Y nrows x q, either layout; nrows = 0: no-op).  The
 * chunk is staged in a device buffer the context owns -- always fp64, whatever option "dtype" holds,
 * since nothing becomes resident; two buffers sized to the largest chunk seen so far (plus, for
 * column-major chunks, one nrows x max(p, q) scratch), so the caller's chunk size bounds the device
 * memory: 16 nrows (ldx + ldy) bytes.  Returns as soon as the chunk is on the device: the caller may
 * reuse X, Y at once; the chunk's device work (column means, centring, the fp64 MFMA Gram -- option
 * "gram_int8" is ignored here --, the merge into S) runs on a second HIP stream behind the next
 * call's upload.  With center = 1 the merge is the pairwise update S += G_c + (N n_c / (N + n_c)) d d',
 * d = chunk mean - running mean, with G_c the Gram of the chunk centred about its own mean -- not the
 * one-pass S - N m m'.  Fixed-order sums: the same chunk sequence gives the same S bit for bit.  An
 * asynchronous failure is reported by the next ppls_stream_* call; from then the stream is unusable
 * (PPLS_E_STATE) until the next ppls_stream_begin. */
int ppls_stream_rows(ppls_ctx* ctx, const double* X, const double* Y, int64_t nrows, int layout);
/* All of src's resident rows as one chunk, device to device (fp32 storage is widened); src is left
 * untouched.  PPLS_E_ARG: src on another device, without data, of another shape, or ctx itself. */
int ppls_stream_rows_from(ppls_ctx* ctx, ppls_ctx* src);
/* Close the stream.  Collective when sharded (RCCL or the host reducer; a rank that streamed no rows
 * still joins): all-reduce {N_r, N_r m_r} -> the global N and mean m; each rank adds
 * N_r (m_r - m)(m_r - m)' to its S; the ranks agree that nobody failed; one all-reduce of S.  scale = 1:
 * d_j = sqrt(S_jj / (N - 1)), then S_ij <- S_ij / (d_i d_j) (exactly symmetric, padding zero);
 * PPLS_E_ARG on every rank alike, with the stream dropped, for N < 2 or a d_j that is not > 0 or not
 * finite (the message names the block and the 1-based column).  ||X||^2, ||Y||^2 are the traces of
 * S's diagonal blocks; a NaN or Inf in any chunk makes them non-finite -> PPLS_E_ARG, stream dropped.
 * Records the transform for ppls_get_scaling (center = m or 0, scale = d or 1).  Every error return
 * drops the stream (no data afterwards); a HIP error on one rank is agreed on in the collectives, so
 * every rank returns. */
int ppls_stream_end(ppls_ctx* ctx);
/* state: 0 none, 1 open, 2 streamed; rows_local / chunks: this rank's so far; n_total: rows over all
 * ranks once streamed (while open: this rank's so far).  All nullable. */
int ppls_stream_info(ppls_ctx* ctx, int* state, int64_t* rows_local, int64_t* n_total, int64_t* chunks);

/* ---- cross-validation from row chunks: one cross-product matrix per fold ------------------------
 * A fold's training cross-products are the sum of the other folds' cross-products, and the held-out
 * error sum_i ||y_i - x_i W diag(B) C'||^2 is a quadratic form in the held-out fold's own: K-fold
 * cross-validation needs no rows and no second pass, only (K + 1) 8 P^2 bytes of device memory.  The
 * data are centred and scaled once, as a whole (R: scale() on all rows, then folds taken without
 * re-centring, crossval_PPLS.R:40-52); ppls_scale_data followed by ppls_cv_ppls on resident rows
 * computes the same.  A stream opened with ppls_stream_begin has no folds and behaves as before; on it
 * the labelled calls and the calls below return PPLS_E_STATE, as do the unlabelled ppls_stream_rows /
 * _rows_from on a fold stream.  A context streamed with folds is "streamed" (everything that needs
 * rows keeps its refusal) and additionally serves ppls_stream_fold_info, ppls_stream_select,
 * ppls_heldout_sse_fold, ppls_cv_ppls_stream and ppls_meta_emstep_stream / ppls_meta_ppls_stream (the
 * folds as populations); what ends the streamed state frees the fold matrices. */

/* ppls_stream_begin with nfolds >= 2 Chan states (N_k, mean_k, S_k) instead of one; the nfolds fold
 * matrices are allocated up front, contiguously (PPLS_E_NOMEM: the stream is not opened). */
int ppls_stream_begin_folds(ppls_ctx* ctx, int p, int q, int center, int scale, int nfolds);
/* ppls_stream_rows / ppls_stream_rows_from with the fold (0 .. nfolds-1) of every row of the chunk
 * (of src's resident rows).  A label out of range: PPLS_E_ARG before any device work, the stream stays
 * usable.  The host builds the chunk's stable fold order (a counting sort), the staged rows are
 * gathered into it on the device, and every fold present in the chunk runs the plain stream's four
 * steps on its segment against its own state, in fold order; a fold absent from the chunk launches
 * nothing.  The same chunks and labels give the same bits in any context. */
int ppls_stream_rows_folds(ppls_ctx* ctx, const double* X, const double* Y, int64_t nrows, int layout,
                           const int32_t* fold /* nrows */);
int ppls_stream_rows_from_folds(ppls_ctx* ctx, ppls_ctx* src, const int32_t* fold /* src's n_local */);
/* ppls_stream_end on a fold stream (collective when sharded, like the plain one: one all-reduce of
 * {failed, N_rk, N_rk mean_rk}, each rank's S_k recentred to the global fold mean, the agreement, one
 * all-reduce of all fold matrices) then, on every rank alone and with identical bits: N = sum N_k and
 * m = sum N_k mean_k / N in fold order; S_k <- S_k + N_k (mean_k - m)(mean_k - m)'; scale = 1:
 * d_j = sqrt(sum_k S_k,jj / (N - 1)) in fold order and S_k,ij <- S_k,ij / (d_i d_j), in the same pass.
 * The plain stream's refusals hold; a fold without a row over all ranks is PPLS_E_ARG with a message
 * naming the fold, the stream dropped.  Leaves the context selected on all folds (-1). */

/* nfolds: 0 for a context that is not (being) streamed with folds; fold_total (nfolds values): rows
 * per fold over all ranks once streamed (while open: this rank's so far); selected: the fold the
 * working cross-products leave out, -1 none.  All nullable. */
int ppls_stream_fold_info(ppls_ctx* ctx, int* nfolds, int64_t* fold_total, int* selected);
/* The working cross-products S <- the sum of the fold matrices l != fold, added in fold order (fold
 * = -1: all of them) -- by addition, never S_all - S_fold, so an entry carries the rounding of the
 * selected rows only and no fold size is refused -- with n_total and ||X||^2, ||Y||^2 (the traces) to
 * match: every fit entry point then works on the selected rows.  PPLS_E_STATE while an ppls_em_begin
 * session is active. */
int ppls_stream_select(ppls_ctx* ctx, int fold);
/* Held-out error of a fit from fold `fold`'s cross-products S_k alone: with A = W' S_k,xx W,
 * D_m = w_m' S_k,xy c_m and G = C'C, for every prefix j = 1..k
 *   sse[j-1] = tr(S_k,yy) - 2 sum_{m<=j} b_m D_m + sum_{m,l<=j} b_m b_l A_ml G_ml.
 * mag[j-1] (nullable) is the same sum with every elementary product replaced by its absolute value:
 * the rounding error of sse_j is bounded by a small multiple of gamma_n mag_j, so mag_j / sse_j tells
 * how many digits survive (the expansion cancels when the fit is good; with no rows there is no
 * direct residual to form instead).  One read of the X rows of S_k; fixed-order sums, identical on
 * every rank (no collective).  W: p x k, C: q x k column-major, k <= 16 as for ppls_heldout_sse. */
int ppls_heldout_sse_fold(ppls_ctx* ctx, const double* W, const double* C, const double* B, int k, int fold,
                          double* sse /* k */, double* mag /* k, nullable */);
/* cv_PPLS's loop on the stream's folds: per fold ppls_stream_select, ppls_ppls_ex with a components
 * from init[f*a .. f*a+a), ppls_heldout_sse_fold.  rmsep[f*a + j] = sqrt(sse_j / (N_f q)) and ncomp
 * as for ppls_cv_ppls; cond (nullable, nfolds x a) = mag_j / sse_j.  Ends selected on -1, also on an
 * error return. */
int ppls_cv_ppls_stream(ppls_ctx* ctx, int a, int max_steps, double atol, int crit_abs,
                        const ppls_theta* init /* nfolds x a */, double* rmsep /* nfolds x a */,
                        int* ncomp /* nfolds */, double* cond /* nfolds x a, nullable */);
/* The same loop with initialGuess = "o2m_xprod" (crossval_PPLS.R:47 with PPLSi :126-131): no init; each
 * fold's fit is ppls_ppls_o2m on the selection that leaves the fold out. */
int ppls_cv_ppls_stream_o2m(ppls_ctx* ctx, int a, int max_steps, double atol, int crit_abs, double* rmsep,
                            int* ncomp, double* cond);

/* ---- row diagnostics: which rows does the fitted model not explain? ----------------------------
 * For a row (x, y) and a PPLS_simult fit theta with orthonormal W, C: a = W'x, b = C'y and, per
 * component k, s11 = sigT_k^2 + sigE^2, s12 = B_k sigT_k^2, s22 = B_k^2 sigT_k^2 + sigH^2 + sigF^2,
 * det = s11 s22 - s12^2.  Then
 *   odx2 = ||x - W a||^2, ody2 = ||y - C b||^2          (orthogonal distances, formed from the residual)
 *   sd2  = sum_k (s22 a_k^2 - 2 s12 a_k b_k + s11 b_k^2) / det     (score distance)
 *   d2   = odx2 / sigE^2 + ody2 / sigF^2 + sd2          (the row's summand of loglC_fast's traceL)
 *   loglik = -(p+q)/2 log 2 pi - ((p-r) log sigE^2 + (q-r) log sigF^2 + sum_k log det_k)/2 - d2/2,
 * whose sum over all rows is ppls_loglik's value; mu_T, mu_U are Expect_M's posterior means.  Under the
 * model odx2/sigE^2, ody2/sigF^2, sd2 and d2 are chi-square with p-r, q-r, 2r and p+q degrees of
 * freedom.  One kernel pass over the rows, read in place; a row's results are bitwise the same
 * whatever the other rows, the subset, the shard or the entry point (fp64 storage).  Every array of
 * ppls_row_diag is nullable.  PPLS_E_ARG, with the outputs untouched: r outside 1..16 or above
 * min(p, q), a non-finite theta, sigE, sigF or a det_k not above 0, a row index out of range, NULL or
 * non-finite rows. */
typedef struct {
  double *odx2, *ody2, *sd2, *d2, *loglik; /* nrows each */
  double *mu_T, *mu_U;                     /* nrows x r column-major */
} ppls_row_diag;
/* This rank's resident rows, either storage type; no collective.  rows: local indices in any order,
 * repeats allowed; NULL: all n_local rows (nrows is not read).  PPLS_E_STATE when the context holds
 * no rows (streamed). */
int ppls_row_diagnostics(ppls_ctx* ctx, const ppls_theta* th, int r, const int64_t* rows, int64_t nrows,
                         ppls_row_diag* out);
/* n host rows in the fit's units, staged through the device in blocks as ppls_predict stages them;
 * the context supplies the device and the shape (p, q) only: streamed, replicate and empty contexts
 * work, and the context's own data are not touched. */
int ppls_row_diagnostics_new(ppls_ctx* ctx, const ppls_theta* th, int r, const double* X, const double* Y, int64_t n,
                             int layout, ppls_row_diag* out);

/* ---- robust fit: the multivariate-t PPLS model by EM ------------------------------
 * With Sigma(theta) the PPLS covariance, P = p + q and d2_i the distance above, the t model's E-step
 * weight of a row is u_i = (nu + P) / (nu + d2_i) and its M-step is the Gaussian one on
 * S_u = sum_i u_i d_i d_i' with divisor N.  Its log-likelihood is
 *   l_t(theta, nu) = N [lgamma((nu + P)/2) - lgamma(nu/2) - (P/2) log(nu pi)] - (N/2) logdet
 *                    - ((nu + P)/2) sum_i log1p(d2_i / nu),
 *   logdet = (p-r) log sigE^2 + (q-r) log sigF^2 + sum_k log det_k.
 * No intercept: the data are centred beforehand and the rows are reweighted as they stand.
 *
 * ppls_robust_weights: on the resident rows of either storage type, the distance pass of
 * ppls_row_diagnostics and one small kernel over its 24 B per row.  nu: m values (1 <= m <= 16); the
 * weights for nu[keep] and the distances are kept in device arrays the context owns (n_local doubles
 * each, reused across calls; a row's d2 has the bits ppls_row_diagnostics reports).  loglik_t[j] =
 * l_t(theta, nu[j]) over all ranks' rows (N = n_total), sum_w (nullable) = sum_i u_i; the m + 1 sums are
 * formed in an order fixed by n_local alone (no atomics: the same bits for every launch and grid) and
 * all-reduced through the context's communicator or reducer in the same order on every rank.
 * PPLS_E_ARG, with the outputs and the kept weights untouched: whatever ppls_row_diagnostics refuses
 * about the fit, m outside 1..16, a nu that is not finite or not above 0, keep outside 0..m-1.
 * PPLS_E_STATE: a context without rows (streamed).  What replaces or rescales the rows
 * (ppls_set_data, the generator, ppls_scale_data, a stream, being the dst of ppls_set_data_from, a
 * change of dtype) drops the kept weights. */
int ppls_robust_weights(ppls_ctx* ctx, const ppls_theta* th, int r, const double* nu, int m, int keep,
                        double* loglik_t /* m */, double* sum_w /* nullable */);
/* Host copies of the kept weights and their distances (n_local each, nullable).  PPLS_E_STATE when
 * nothing is kept. */
int ppls_robust_get(ppls_ctx* ctx, double* w, double* d2);
/* ppls_xprod_resample for real case weights: dst's S becomes sum_i weight_i d_i d_i' over src's
 * resident rows, by the real-weighted instantiation of the fp64 MFMA Gram (each term (weight_i x_a) x_b;
 * the device holds the weights as fp64).  weight: this rank's n_local host doubles, or NULL for the
 * weights src keeps from ppls_robust_weights, with no host round trip.  The lifecycle is
 * ppls_xprod_resample's: the agreement across ranks, dst's reused S and partials, src left as it was,
 * dst "streamed".  n_total is src's -- the weights are relative to N, not renormalised: the M-step of
 * the t model divides S_u by N, not by sum u -- and ||X||^2, ||Y||^2 are the traces of S_u's diagonal
 * blocks.  PPLS_E_ARG: a negative or non-finite weight on any rank (every rank returns it), all weights
 * zero over all ranks, dst == src, contexts on different devices.  PPLS_E_STATE: src without data or
 * streamed, NULL weight with nothing kept.  After such a refusal dst holds what it held before. */
int ppls_xprod_weighted(ppls_ctx* dst, ppls_ctx* src, const double* weight /* host, src's n_local, or NULL */);

/* ---- PO2PLS: X- and Y-specific components, fitted from the cross-products ----------
 * The reference's wider data model (simulC, Package/PPLS/src/loglC.cpp:268-315):
 *   x = W t + Wo to + e,  y = C u + Co uo + f,  u = B t + h,
 * Wo its P_Yosc (structured variation only X has), Co its P_Xosc.  Sizes: r >= 1, rx, ry >= 0,
 * r + rx <= min(16, p), r + ry <= min(16, q).  Every sigma is a standard deviation.  The latent
 * vector is ordered z = (t, to | u, uo), k = 2 r + rx + ry.  Loadings need not be orthonormal. */
typedef struct {
  double* W;     /* p x r column-major */
  double* Wo;    /* p x rx (unused when rx = 0) */
  double* C;     /* q x r */
  double* Co;    /* q x ry (unused when ry = 0) */
  double* B;     /* r: diag(B) */
  double* sigT;  /* r */
  double* sigTo; /* rx */
  double* sigUo; /* ry */
  double sigE;
  double sigF;
  double sigH;   /* a scalar, as in EMstepC and PPLS_simult */
} ppls_po2_theta;

/* EMstepC's list (loglC.cpp:231-249) from S.  Every pointer is nullable (not requested); all
 * matrices column-major and full, as EMstepC returns them. */
typedef struct {
  double* Cxt;   /* p x r:  E[x t'] */
  double* Cxto;  /* p x rx */
  double* Cyu;   /* q x r */
  double* Cyuo;  /* q x ry */
  double* Ctt;   /* r x r */
  double* Ctoto; /* rx x rx */
  double* Ctto;  /* r x rx */
  double* Cuu;   /* r x r */
  double* Cuouo; /* ry x ry */
  double* Cuuo;  /* r x ry */
  double* Cut;   /* r x r:  E[u t'] */
  double* Chh;   /* r x r */
  double* K;     /* k x k:  D Lambda^-1; the posterior means of the rows are [X Gx | Y Gy] K */
  double Cee;
  double Cff;
} ppls_po2_expect;

/* All four use the S the context holds (streamed, fold-selected, resampled, permuted, weighted,
 * adjusted); on resident rows with no S they form it by the route 'o2m_xprod' uses and keep it until
 * ppls_xprod_release or new data.  N is the row count ppls_em_run uses.  They need no collective on
 * sharded contexts (S is replicated), end no ppls_em_begin session, change no option and leave S bit
 * for bit.  Refusals, each with the outputs and theta untouched: PPLS_E_ARG (sizes outside the above,
 * a NULL loading, a non-finite value, a sigma that is not above 0), PPLS_E_STATE (no data, or an open
 * stream), PPLS_E_NUMERIC (Lambda not positive definite, an updated variance not above 0, a
 * rank-deficient loading update).
 *
 * ppls_po2_estep replaces EMstepC (loglC.cpp:116-250): the E-step moments at theta, without the dense
 * (p+q) x (p+q) inverse of :139-141.  ppls_po2_loglik replaces loglC (:36-113), with the constant
 * -N (p+q)/2 log 2 pi (as loglC_fast :336; loglC:81 has p alone). */
int ppls_po2_estep(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, ppls_po2_expect* out);
int ppls_po2_loglik(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, double* out);
/* The EM loop the reference leaves unwritten (loglC.cpp:228, "Maximization step is done in R"): per
 * iteration one pass over S at theta_{i-1}, its log-likelihood as a by-product, the stop rule
 * (i >= 2 and l_{i-1} - l_{i-2} < atol returns theta_{i-1}; atol = -Inf never stops), else one ECM
 * cycle: W <- orth(Cxt - Wo Ctto'), C <- orth(Cyu - Co Cuuo'); Wo <- orth(Cxto - W Ctto),
 * Co <- orth(Cyuo - C Cuuo) with the new W, C and the same moments; then the scalars.  One last pass
 * gives l and the moments at the estimates when the rule never fired: *n_loglik = steps + 1 entries
 * (at most cap are copied; cap >= max_steps + 1 holds them all), and expect_out belongs to the
 * returned theta.  The loop runs on the device: loadings, scalars and the history stay there, the
 * stop rule sets the flag ppls_em_run's kernels use.  type: PPLS_ORTH_SVD (the polar factor) or
 * PPLS_ORTH_QR (sign_e qr.Q(qr(.)), R's sign rule, functions.R:257-259).  th is overwritten with the estimates in
 * canonical form: the joint part by PPLS_simult's sign and order rule (EM_W_multi.R:794-799), the
 * specific components by decreasing sigma, each column's sign so that its sum is >= 0.
 * *negative_increment (nullable): whether the history has a negative increment. */
int ppls_po2_em_run(ppls_ctx* ctx, ppls_po2_theta* th, int r, int rx, int ry, int max_steps, double atol, int type,
                    double* loglik, int cap, int* n_loglik, int* negative_increment, ppls_po2_expect* expect_out);

/* Default start values.  Joint part (W, C, B, sigT, sigE, sigF, sigH): the 'o2m_xprod' sequential fit
 * ppls_ppls_o2m(ctx, r, 1, 1e-4, ...) -- the cross-covariance directions after one EM step per
 * component (more steps of that shared-only model pull a joint loading towards the strongest X-only
 * direction).  That fit runs on a scratch context of the call holding a copy of S (8 P^2
 * bytes for its duration), because the sequential fit keeps its state in its context: this context's
 * ppls_em_begin session, options and 'o2m_xprod' record (ppls_o2m_info) stay as they are.  Wo: the dominant rx-dimensional invariant subspace of
 * (I - P_W) S_xx (I - P_W), P_W the projector onto W's columns, by `steps` orthogonal-iteration steps
 * of the statistics pass (both sides in one read of S per step; the p x rx projection and QR on the
 * host) from V0x (p x rx, host, e.g. normal draws), then sigTo = sqrt(diag(V'S_xx V) / N); Co, sigUo
 * alike from V0y (q x ry).  V0x / V0y are not read when rx / ry = 0.  PPLS_E_NUMERIC: a
 * rank-deficient block.  theta_out (caller's buffers) is written only on success. */
int ppls_po2_start(ppls_ctx* ctx, int r, int rx, int ry, const double* V0x, const double* V0y, int steps,
                   ppls_po2_theta* theta_out);

/* ---- choosing (r, rx, ry): batched fits, prediction, cross-validation ---------------
 * ppls_po2_em_run for m models at once on the S the context holds (1 <= m <= 256; shapes may repeat,
 * so restarts of one model are a batch too).  Every model runs ppls_po2_em_run's loop with its own stop
 * rule: one that stops, or fails, freezes while the others go on, and model j's estimates, history and
 * count are bit for bit those of ppls_po2_em_run(ctx, &th[j], r[j], rx[j], ry[j], ...) alone.  Per
 * pass the models share the panel launches (their loading columns lie side by side: ceil(sum kx / 16)
 * + ceil(sum ky / 16) launches for the whole batch) and one launch each of the Gram, the k x k algebra
 * and the loading update; the device holds m (8 P k + 16 * 8 P) bytes plus small terms.
 * th: m thetas, in: the starts, out: the estimates in canonical form.  loglik: m x cap, model-major
 * (nullable with cap = 0); n_loglik, status: m; negative_increment: m, nullable.
 * Every model and shape is validated before any device work, with ppls_po2_em_run's refusals and
 * everything untouched.  Otherwise the call returns PPLS_OK and status[j] is PPLS_OK or
 * PPLS_E_NUMERIC; for a failed model th[j] and row j of loglik are untouched, n_loglik[j] = 0, and
 * ppls_last_error names the first failed model and its reason.  The context rules are
 * ppls_po2_em_run's: no session is ended, no option changed, S is left bit for bit. */
int ppls_po2_em_run_batch(ppls_ctx* ctx, int m, ppls_po2_theta* th, const int* r, const int* rx, const int* ry, int max_steps,
                          double atol, int type, double* loglik, int cap, int* n_loglik, int* negative_increment,
                          int* status);

/* The linear map of the model's prediction (host only, no GPU), in the form ppls_predict and
 * ppls_heldout_sse(_fold) take (their W need not be orthonormal):
 *   xory = 0:  E[y | x] = C diag(B) E[t | x].  Lambda_x = diag(sigT, sigTo)^-2 + Gx'Gx / sigE^2, Gx = [W Wo];
 *              L (p x r) = the first r columns of Gx Lambda_x^-1 / sigE^2, Bp = B:
 *              ppls_predict(ctx, L, C, Bp, r, 0, ...) is the prediction of y.
 *   xory = 1:  E[x | y] = W diag(beta) E[u | y], beta_j = sigT_j^2 b_j / (sigT_j^2 b_j^2 + sigH^2).
 *              Lambda_y = diag(sigT^2 b^2 + sigH^2, sigUo^2)^-1 + Gy'Gy / sigF^2, Gy = [C Co];
 *              L (q x r) = the first r columns of Gy Lambda_y^-1 / sigF^2, Bp = 1 / beta (the form
 *              ppls_predict(xory = 1) divides by): ppls_predict(ctx, W, L, Bp, r, 1, ...).
 * Lambda is factored by Cholesky on the host.  PPLS_E_ARG as for the other PO2 entries; PPLS_E_NUMERIC:
 * Lambda not positive definite, or (xory = 1) a b_j that is 0.  L, Bp are written only on success. */
int ppls_po2_predict_map(const ppls_po2_theta* th, int r, int rx, int ry, int p, int q, int xory, double* L, double* Bp);

/* Cross-validated X -> Y prediction error of ncand candidate sizes on a context streamed with folds
 * (anything else: PPLS_E_STATE, as ppls_cv_ppls_stream).  Per fold f: ppls_stream_select(f); per candidate
 * the start ppls_po2_start gives on that selection from the leading rx / ry columns of V0x (p x max rx) /
 * V0y (q x max ry); one ppls_po2_em_run_batch over the candidates; per fitted candidate
 * ppls_po2_predict_map(xory = 0) and ppls_heldout_sse_fold(L, C, B, r, f):
 * rmsep = sqrt(sse[r - 1] / (N_f q)), cond = mag / sse, steps = the EM iterations run.  All outputs
 * nfolds x ncand, fold-major; cond, steps and fits (caller's buffers, written for fitted candidates) are
 * nullable.  A failed start or fit gives NaN and its status (PPLS_E_NUMERIC).  The context ends selected
 * on -1, also on an error return. */
int ppls_po2_cv_stream(ppls_ctx* ctx, int ncand, const int* r, const int* rx, const int* ry, int max_steps, double atol,
                       int type, const double* V0x, const double* V0y, int start_steps, double* rmsep, double* cond,
                       int* steps, int* status, ppls_po2_theta* fits);

/* ---- PO2PLS row by row: diagnostics and the t-model weights --------------------------
 * For a row (x, y) and a PO2PLS fit theta, Gx = [W Wo] = Qx Rx and Gy = [C Co] = Qy Ry (Householder QR on
 * the host, fp64, R's diagonal positive; the loadings need not be orthonormal), a = Qx'x, b = Qy'y,
 * R = blockdiag(Rx, Ry) and Sigma_c = R Sigma_z R' + diag(sigE^2 I_kx, sigF^2 I_ky), the covariance of (a; b):
 *   odx2 = ||x - Qx a||^2, ody2 = ||y - Qy b||^2       (orthogonal distances, formed from the residual)
 *   sd2  = ||Uc (a; b)||^2, Sigma_c^-1 = Uc'Uc, Uc upper triangular      (score distance, >= 0 as formed)
 *   d2   = (odx2 / sigE^2 + ody2 / sigF^2) + sd2       (the squared Mahalanobis distance of (x; y))
 *   loglik = -(p+q)/2 log 2 pi - logdet / 2 - d2 / 2,
 *   logdet = (p-kx) log sigE^2 + (q-ky) log sigF^2 + log|Sigma_c|
 *          = p log sigE^2 + q log sigF^2 + log|Sigma_z| + log|Lambda|        (DESIGN §26's),
 * whose sum over all rows is ppls_po2_loglik's value on the same rows; mu = (a; b)' Kmu, Kmu = Sigma_c^-1 R
 * Sigma_z = R K with §26's K: the posterior means [X Gx | Y Gy] K of z = (t, to, u, uo).  Under the model
 * odx2/sigE^2, ody2/sigF^2, sd2 and d2 are chi-square with p-kx, q-ky, kx+ky and p+q degrees of freedom.
 * One kernel pass over the rows, read in place (ppls_po2_rowdiag.hip); a row's results are bitwise the same
 * whatever the other rows, the subset, the shard or the entry point (fp64 storage).  Every array is nullable.
 * The row lists, NULL for all rows, the _new staging and PPLS_E_STATE on a context without rows are
 * ppls_row_diagnostics{,_new}'s.  Unlike the other ppls_po2_* entries these read no S and form none; they end
 * no ppls_em_begin session, change no option and leave the data bit for bit.
 * PPLS_E_ARG, with the outputs (and the kept weights) untouched: sizes outside §26's, a NULL loading, a
 * non-finite value, a sigma not above 0, a rank-deficient [W Wo] or [C Co] (a QR pivot with R_kk^2 <=
 * 64 c u ||column k||^2, §26's rule), Sigma_c not positive definite, a row index out of range, NULL or
 * non-finite rows. */
typedef struct {
  double *odx2, *ody2, *sd2, *d2, *loglik; /* nrows each, nullable */
  double* mu;                              /* nrows x k column-major, order (t, to, u, uo), nullable */
} ppls_po2_row_diag;
int ppls_po2_row_diagnostics(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, const int64_t* rows,
                             int64_t nrows, ppls_po2_row_diag* out);
int ppls_po2_row_diagnostics_new(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, const double* X,
                                 const double* Y, int64_t n, int layout, ppls_po2_row_diag* out);
/* ppls_robust_weights under a PO2PLS fit: the distance pass above, then the same weight kernel on its three
 * arrays.  The weights for nu[keep] and the distances go to the arrays ppls_robust_weights keeps (a row's d2
 * has the bits ppls_po2_row_diagnostics reports), so ppls_robust_get and ppls_xprod_weighted(dst, src, NULL)
 * work as they are and the same events drop them.  loglik_t[j] is §24's l_t with the logdet above; the m + 1
 * sums and their all-reduce are §24's.  Refusals as above and §24's on m, nu and keep. */
int ppls_po2_robust_weights(ppls_ctx* ctx, const ppls_po2_theta* th, int r, int rx, int ry, const double* nu, int m,
                            int keep, double* loglik_t /* m */, double* sum_w /* nullable */);

/* ---- host-side algebra (no GPU; the same code the device finalize runs) ------------------------ */
/* From the all-reduced sufficient statistics of one sweep with theta (stats = [X'mu_T p x r |
 * Y'mu_U q x r | Gram 2r x 2r], all column-major) compute Expect_M's moments, logl_W(theta) and
 * the M-step scalars.  W_next/C_next (nullable) receive orth(X'mu_T)/orth(Y'mu_U). */
int ppls_finalize_host(const double* SX, const double* SY, const double* G, double ssqX, double ssqY,
                       double N, int p, int q, int r, const ppls_theta* th, int type,
                       ppls_theta* next, ppls_expect* moments, double* loglik);
/* alpha, beta, gamma, delta (4r) with mu_T = Xw diag(alpha) + Yc diag(beta) and
 * mu_U = Xw diag(gamma) + Yc diag(delta) (EM_W_multi.R:691-694). */
int ppls_mu_coefficients(const ppls_theta* th, int r, double* coef4r);

#ifdef __cplusplus
}
#endif
#endif /* PPLS_AMD_PPLS_H */
