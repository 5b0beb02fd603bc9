// ppls_capi.cpp -- host runtime + C ABI (include/ppls.h) of the MI355X PPLS_simult EM inner loop.
//
// One context = one GPU = one process rank.  Per EM iteration the host enqueues, on one HIP
// stream and without synchronising: sweep (1 pass over X, Y) -> deterministic reduction of the
// workgroup partials -> [RCCL all-reduce of (p+q) r + 4 r^2 doubles] -> finalize (E-step moments,
// log-likelihood, M-step incl. the polar factor).  The host only reads back the log-likelihood
// when the convergence test of PPLS_simult (EM_W_multi.R:792) needs it.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ppls.h"
#include "../../include/ppls_debug.h"
#include "ppls_kernels.h"
#include "ppls_math.h"
#include "ppls_cv.h"
#include "ppls_robust.h"
#include "ppls_po2_rowdiag.h"
#include "ppls_rowdiag.h"
#include "ppls_o2m.h"
#include "ppls_permute.h"
#include "ppls_scale.h"
#include "ppls_adjust.h"
#include "ppls_adjust_host.h"
#include "ppls_cvstream.h"
#include "ppls_stream.h"
#include "ppls_varxprod.h"
#include "ppls_po2.h"
#include "ppls_xprod.h"
#include "ppls_xprod_meta.h"

struct ppls_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int num_cus = 256;
  // options
  int sweep_mode = 0;      // 0 auto, 3 panel
  int grid_opt = 0;
  int rp_opt = 0;   // rows per pipeline step: 0 auto (2 where the kernel fits in registers)
  int pipe_opt = 1;     // split kernel: software-pipelined order
  int dots_rows = 0;   // panel dots rows per wave: 0 auto, 32, 64 (tests of both forms)
  int dots_pair = -1;  // panel dots wave pair per row tile: -1 auto, 0, 1
  int acc_chunks = 0;  // panel accumulation row chunks: 0 auto (ppls_panel_chunks), else forced
  int team_rows = 0;   // finalize polar team: rows of S per member (0: PPLS_TEAM_ROWS)
  int polar1 = 1;   // finalize polar: Cholesky-QR1 fast path when kappa(X'mu) <= PPLS_POLAR1_KAPPA
  int polar1_kappa = 0;   // its bound on ||R1||_F ||R1^-1||_F (0 = min(8 r, 40))
  int exact_gram = 1;     // finalize: compute W'W, C'C of the new loadings (1, default) or use I (0):
                          // I saves ~0.5 % at the C4/C5 shares but, through the cancellation in
                          // Cee at small sigma_E, moved mu_T by 1e-8 (golden stress_sig005)
  int ldpad = 1;   // row padding of the panel sweep's rows (ld_of); 0 = 16-B rows (experiment)
  int dtype = 0;           // storage of X, Y: 0 fp64, 1 fp32 (arithmetic is fp64 either way)
  int nt_loads = -1;       // sweep LDS-DMA non-temporal: -1 auto (when X, Y exceed the MALL), 0 off, 1 on
  int timing = 0;          // 0 off; N > 0: bracket every N-th sweep launch with HIP events
  int64_t sweep_count = 0;
  // row segment the next sweeps cover (meta_* per-population sweeps); seg_rows < 0 = all rows
  int64_t seg_row0 = 0, seg_rows = -1;
  // communicator: RCCL, or a caller-supplied host reduction (ppls_set_reducer)
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  ppls_reduce_fn reducer = nullptr;
  void* reducer_user = nullptr;
  std::vector<double> reduce_host;
  // data
  bool have_data = false;
  int64_t n_local = 0, n_total = 0;
  int p = 0, q = 0, ldx = 0, ldy = 0;
  double* X = nullptr;
  double* Y = nullptr;
  double* ssq = nullptr;       // {||X||^2, ||Y||^2} (global)
  double ssq_host[2] = {0, 0};
  // the smallest free HBM over all ranks when the data were loaded (all-reduced beside ||X||^2,
  // ||Y||^2, so every rank sees the same value): the cross-product form's memory gate
  double mem_free_min = 0.0;
  double* flag = nullptr;      // 8 doubles for small agreement all-reduces (allocated with the data)
  // per-r state
  int r_alloc = 0;
  double* W[2] = {nullptr, nullptr};
  double* C[2] = {nullptr, nullptr};
  PplsScalars* sc[2] = {nullptr, nullptr};
  double* gram[2] = {nullptr, nullptr};   // [W'W | C'C] of W[i], C[i]
  double* vstate = nullptr;   // polar Jacobi warm start [V_W | V_C], reset on every theta upload
  PplsMoments* mom = nullptr;
  double* stats = nullptr;
  double* part = nullptr;
  int64_t part_ld = 0;
  int part_groups = 0;
  double* Z = nullptr;
  int z_cols = 0;          // columns allocated in Z (2r two-pass, 4r panel)
  double* mu = nullptr;
  double* loglik = nullptr;
  int loglik_cap = 0;
  double* work = nullptr;
  int* status = nullptr;
  long long* ftrace = nullptr;   // finalize phase timestamps (diagnostics)
  unsigned* team_bar = nullptr;  // finalize polar teams (wide p): counters (self-resetting) + partials
  double* team_part = nullptr;
  long long* strace = nullptr;   // split sweep per-workgroup stamps (diagnostics, PPLS_STRACE_MAX_WG x 4)
  // split-sweep load balance: the XCDs of one MI355X stream rows at rates that differ by up to ~3 %,
  // the same way every iteration (profiles/r3_sweep_balance_*.txt), so the even row split leaves a
  // tail.  The first full split sweep of the data is timed per workgroup (untimed calibration
  // launches), workgroup g then owns a row block proportional to the measured rate of its class
  // g % 8 (the XCD under round-robin dispatch); fixed afterwards, so results stay deterministic.
  int balance = 0;                 // option "balance": 1 calibrate, 0 the even split (default: bitwise
                                   // reproducible across processes; the calibrated split regroups the sums)
  bool bal_done = false;           // calibrated for (bal_n, bal_grid)
  int64_t bal_n = -1;
  int bal_grid = -1;
  double bal_w[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  int64_t* bal_bounds = nullptr;   // device: grid + 1 row boundaries
  double* coefs = nullptr;     // loglC_fast coefficient block (5r)
  double* scratch = nullptr;   // generic device scratch
  size_t scratch_bytes = 0;
  // ppls_em_run's device-side stop rule: a device flag every kernel of the run checks, set by the
  // finalize that sees logl[i] - logl[i-1] < atol, and its host-mapped mirror the host polls
  int* stop_d = nullptr;
  int* stop_mirror = nullptr;       // host pointer (hipHostMalloc, mapped, coherent)
  int* stop_mirror_dev = nullptr;   // its device address
  const int* sweep_stop = nullptr;  // non-null only inside ppls_em_run with a finite atol
  double stop_atol = 0.0;
  // device-resident iteration state (ppls_em_begin / ppls_em_iterate)
  int em_r = 0, em_cur = 0, em_iter = 0;
  bool em_active = false;
  // cross-product form of the iteration (ppls_xprod.hip): S = [X Y]'[X Y] (P x P, P = ldx + ldy)
  // formed once per data set, then every statistics step reads S instead of X and Y
  int xprod = 0;            // option "xprod": 0 stream X, Y (default), 1 cross-products, -1 auto (cost model)
  int xprod_rw = 0;         // option "xprod_rw": rows of S per wave of the tile kernel (0 auto)
  int gram_int8 = 0;        // option "gram_int8": S by the int8-MFMA CRT form (1, when the column spread
                            // allows; else the fp64 MFMA Gram) or the fp64 MFMA Gram (0)
  int oz_used = 0, oz_nmod = 0, oz_L = 0;   // the last formation of S: which Gram, moduli, bits
  std::vector<int> oz_shift;                 // its per-column scalings x' = rint(D 2^shift)
  double oz_ms[4] = {0, 0, 0, 0};           // its phases (HIP events): stats+residues, SYRK, CRT, total
  // the int8 Gram's residue planes and SYRK output, kept between formations (allocating and freeing
  // tens of GB per call made later calls' hipMalloc / hipFree take ~1 s each after a dozen calls,
  // tools/oz_repeat_probe.py); freed with ppls_xprod_release, new data, gram_int8 = 0 or the context
  int8_t* oz_planes = nullptr;
  uint8_t* oz_res = nullptr;
  size_t oz_planes_len = 0, oz_res_len = 0;
  bool xp_ready = false;    // S holds the (all-reduced) cross-products of the current data
  bool xp_active = false;   // statistics steps of the current run read S
  bool xp_pending_gram = false;   // the last statistics step left the Gram B'M to the next finalize
  int xprod_fuse = 1;       // option "xprod_fuse": the finalize forms the Gram (r <= 8, P <= 6144)
  bool xp_explicit = false; // S was formed by ppls_xprod_prepare: kept until ppls_xprod_release / new data
  int meta_path = 0;        // the last ppls_meta_ppls: 1 host loop, 2 device split, 3 device panel,
                            // 4 resident cross-products (meta_xprod), 5 streamed (ppls_meta_ppls_stream)
  int meta_xprod = 0;       // option "meta_xprod": resident meta_* take their statistics from the
                            // populations' cross-products S_j
  double* mx_S = nullptr;   // the cached S_j: mx_K matrices of P x P, contiguous, all-reduced
  int mx_K = 0;
  std::vector<int64_t> mx_local, mx_total;   // the pop_local / pop_total they were formed for
  int64_t mx_formations = 0;                 // formations of the K matrices on this context
  double mx_form_ms = 0.0;                   // the last one: wall clock incl. its all-reduce
  int meta_device = 1;      // option "meta_device": meta_PPLSi's loop on the device (1) or per population
                            // from the host (0; also where the split sweep does not apply)
  int vorth = 8;            // option "vorth": the finalize re-orthonormalises its carried Jacobi V every
                            // vorth-th iteration (1 = every iteration)
  double* xp_S = nullptr;
  double* xp_M = nullptr;   // M = S blockdiag(W, C), P x 2r scratch
  double xp_setup_ms = 0.0; // last formation of S: Gram kernel (HIP events), and with the all-reduce
  double xp_setup_total_ms = 0.0;
  double xp_setup_ar_ms = 0.0;   // the all-reduce of S (wall clock around it and its stream sync)
  int xp_nsplit = 0;
  // the MFMA Gram's work queue (S, variances' X'X), prepared for one shape
  int* gram_q = nullptr;
  // (p, xreal, xcols, yreal, n, nsplit_req, nsplit, wave slots) of gram_q: the queue layout depends
  // on the split count and the slot count, which follow the storage dtype's occupancy
  int64_t gq_key[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  rocblas_handle blas = nullptr;   // rocSOLVER (variances.PPLS_simult's p x p inverse), created lazily
  int var_chol = 1;                // option "var_chol": that inverse by Cholesky when positive definite: 1 hand-written
                                   // (ppls_linalg.hip), 2 rocSOLVER potrf/potri; 0 LU (rocSOLVER getrf/getri)
  // timing
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t ev_used = 0;
  double timed_ms = 0.0;
  int64_t timed_launches = 0;
  // the statistics all-reduce of the timed sweeps (RCCL only), same bookkeeping
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_ar;
  size_t ev_ar_used = 0;
  double ar_ms = 0.0;
  int64_t ar_calls = 0;
  // cross-validation (ppls_cv_ppls): the training context, created once and reused for every fold
  // (it borrows this context's communicator), and the phases of the calls since the last reset --
  // {gather, held-out Gram + downdate, fits, scoring} in ms and the bytes the gather and the scoring
  // kernel moved (ppls_cv_timing)
  ppls_ctx* cv_train = nullptr;
  double cv_ms[4] = {0, 0, 0, 0};
  double cv_bytes[2] = {0, 0};
  // ppls_scale_data: the transform the resident data carry relative to what was loaded
  // (loaded = resident * scale + center; p + q values each, X's columns then Y's; empty = identity),
  // and the last call's passes {sums, centred squares, apply}: ms (HIP events) and bytes moved
  std::vector<double> sc_center, sc_scale;
  double scale_ms[3] = {0, 0, 0};
  double scale_bytes[3] = {0, 0, 0};
  // ppls_adjust_data / ppls_xprod_adjust: the covariate part of that transform,
  // loaded = resident * scale + center + (z - zcenter) Gamma; adj_k = 0: not adjusted.  adj_gamma is
  // adj_k x (p + q) row-major.  adj_ms: the last coefficient, apply, Schur and standardise pass (HIP events).
  int adj_k = 0;
  std::vector<double> adj_zcenter, adj_gamma;
  std::vector<double> adj_ss;   // sum_a G_aj^2 per column of the last ppls_adjust_data (the explained sums of squares)
  double adj_ms[4] = {0, 0, 0, 0};
  // streamed data (ppls_stream_*): S and the column means accumulated from row chunks, no rows
  // resident.  A chunk is staged in one of two fp64 device buffers (each [X rows | Y rows] in the
  // padded row layout, sized for the largest chunk seen); its device work runs on st_stream while
  // the next chunk uploads on `stream`, st_done[b] marking buffer b free again.
  int st_state = 0;          // 0 none, 1 open (between begin and end), 2 streamed (fits read S only)
  bool st_failed = false;    // an open stream hit an error: PPLS_E_STATE until the next ppls_stream_begin
  int st_center = 0, st_scale = 0;
  int64_t st_rows = 0, st_chunks = 0;   // this rank's rows and chunks so far
  hipStream_t st_stream = nullptr;
  hipEvent_t st_done[2] = {nullptr, nullptr};
  double* st_buf[2] = {nullptr, nullptr};
  int64_t st_cap = 0;        // rows a staging buffer holds
  int st_next = 0;           // the buffer the next chunk goes to
  double* st_cm = nullptr;   // column-major upload scratch (rows x max(p, q))
  int64_t st_cm_len = 0;
  double* st_vec = nullptr;  // joint-layout vectors of P: chunk sums, chunk mean, delta, mean, ones; then a fold stream's st_nfolds weights
  double* st_part = nullptr; // the chunk Gram's split partials
  int64_t st_part_len = 0;
  double* st_colpart = nullptr;   // the column sums' row-block partials
  int64_t st_colpart_len = 0;
  // a stream opened with folds (ppls_stream_begin_folds): one Chan state (N_k, mean_k,
  // S_k) per fold; once streamed, the fold matrices stay and xp_S is the working selection of them
  int st_nfolds = 0;              // 0: a plain stream
  double* st_fS = nullptr;        // the st_nfolds fold matrices, P x P each, contiguous
  double* st_fmean = nullptr;     // st_nfolds x P running fold means (while the stream is open)
  double* st_gbuf = nullptr;      // the staged chunk in fold order (the layout of st_buf)
  int64_t st_gbuf_len = 0;
  int64_t* st_idx[2] = {nullptr, nullptr};   // per staging buffer: the chunk's stable fold order
  int64_t st_idx_len[2] = {0, 0};
  std::vector<int64_t> st_fN;     // rows per fold: this rank's while open, over all ranks once streamed
  std::vector<double> st_fmean_h; // once streamed: the folds' means (st_nfolds x P, joint layout)
  std::vector<int64_t> st_seg;    // the current chunk's st_nfolds + 1 segment offsets
  std::vector<int*> st_fq;        // per staging buffer and fold: the segment Gram's work queue (device)
  std::vector<int64_t> st_fq_len;
  int st_sel = -1;                // the fold xp_S leaves out (-1: none)
  // ppls_xprod_resample with this context as dst: the row counts on the device and the weighted Gram's
  // split partials, kept from call to call (a bootstrap allocates nothing per replicate)
  int32_t* rs_cnt = nullptr;
  int64_t rs_cnt_len = 0;
  double* rs_part = nullptr;
  int64_t rs_part_len = 0;
  // ppls_xprod_weighted with this context as dst and host weights: their device copy, kept likewise
  double* rs_wt = nullptr;
  int64_t rs_wt_len = 0;
  // ppls_robust_weights on this context: the weights of the resident rows for the nu last
  // kept and their distances, n_local each, reused across calls; rb_kept while they belong to the rows
  // as they stand.  Option "robust_grid": the row pass's workgroups (0 auto; any value, the same bits).
  double *rb_w = nullptr, *rb_d2 = nullptr;
  int64_t rb_len = 0;
  bool rb_kept = false;
  int rb_grid = 0;
  // ppls_xprod_permute with this context as dst: the device array [row indices | padding |
  // split bounds] with its host staging, the ldx x ldy block the ranks all-reduce, and the host byte map
  // of the permutation check, kept from call to call (the split partials are rs_part).  xp_serial numbers
  // every formation of xp_S; dst's diagonal blocks are src's while pm_self_serial is dst's own serial and
  // pm_src_serial is src's.
  int32_t* pm_idx = nullptr;
  int64_t pm_idx_len = 0;
  double* pm_blk = nullptr;
  int64_t pm_blk_len = 0;
  std::vector<int32_t> pm_host;
  std::vector<uint8_t> pm_seen;
  uint64_t xp_serial = 0, pm_self_serial = 0, pm_src_serial = 0;
  double pm_ms[4] = {0, 0, 0, 0};   // the last permute, wall clock: check, staging + upload, kernel + finish, whole call
  // 'o2m_xprod' starting values (ppls_o2m.hip): option "o2m_path" (0 auto, 1 fused,
  // 2 two-phase), the pass's device vectors [v (L) | d (rows) | u (rows) | z (L) | workspace], and the
  // last start's record {side (0: rows = p, 1: rows = q), path, passes, fits} / {residual estimate, theta}
  int o2m_path = 0;
  double* o2m_buf = nullptr;
  int64_t o2m_buf_len = 0;
  int o2m_last[4] = {0, 0, 0, 0};
  int seq_fits = 0;   // rank-1 device fits the last sequential loop (seq_fit) ran
  double o2m_last_d[2] = {0, 0};
};

namespace {

std::atomic<uint64_t> g_xp_serial{0};   // one number per formation of any context's S (ppls_ctx::xp_serial)

int fail(ppls_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(c, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((c), PPLS_E_HIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                              \
  } while (0)

#define RCCLCHK(c, call)                                                                  \
  do {                                                                                    \
    ncclResult_t e_ = (call);                                                             \
    if (e_ != ncclSuccess)                                                                \
      return fail((c), PPLS_E_COMM, "%s: %s", #call, ncclGetErrorString(e_));            \
  } while (0)

void oz_free(ppls_ctx* c);
bool oz_held(const ppls_ctx* c);

template <typename T>
int dalloc(ppls_ctx* c, T** p, size_t count) {
  if (*p) {
    (void)hipFree(*p);
    *p = nullptr;
  }
  if (count == 0) count = 1;
  hipError_t e = hipMalloc((void**)p, count * sizeof(T));
  if (e == hipErrorOutOfMemory && oz_held(c) && (void*)p != (void*)&c->oz_planes && (void*)p != (void*)&c->oz_res) {
    // the int8 Gram's kept workspace gives way first
    (void)hipGetLastError();
    (void)hipStreamSynchronize(c->stream);
    oz_free(c);
    e = hipMalloc((void**)p, count * sizeof(T));
  }
  if (e != hipSuccess) {
    *p = nullptr;
    return fail(c, PPLS_E_NOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
  }
  return PPLS_OK;
}

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

// A device buffer that is freed on every return path until a context takes it (release).
struct DevGuard {
  double* p = nullptr;
  ~DevGuard() { dfree(p); }
  double* release() {
    double* r = p;
    p = nullptr;
    return r;
  }
};

// A device buffer the context keeps across calls and only ever grows: *len elements, 0 after a failure.
template <typename T>
int grow(ppls_ctx* c, T** buf, int64_t* len, int64_t need) {
  if (*len >= need) return PPLS_OK;
  *len = 0;
  const int rc = dalloc(c, buf, (size_t)need);
  if (!rc) *len = need;
  return rc;
}

// Row stride (elements) of the resident X or Y.  16-B rows for narrow data and for the fp64 rows of
// the split sweep (p <= 2048: its DMA ring streams whole row ranges, alignment beyond 16 B is moot,
// and C3's 16,000-B rows stay unpadded).  Rows the panel sweep reads (fp32 storage, wider fp64) are
// padded to 128 B (one cache line per dots tile) and from 16 KB to 4 KB: the accumulation pass reads
// 4-KB column segments of every row, and 4-KB-aligned segments stream faster -- 5e5 x 40 KB rows,
// no arithmetic: 16-B-aligned stride 3.24 ms, 128-B 3.07 ms, 4-KB 2.93 ms
// (tools/acc_pattern_probe.hip, profiles/r2_row_alignment_probe.txt).  Padding columns are zero.
int ld_of(int p, int f32 = 0, int pad = 1) {
  const int es = f32 ? 4 : 8;
  const long bytes = (long)p * es;
  if (!pad || bytes < 1024 || (!f32 && p <= 2048)) return f32 ? (p + 3) & ~3 : (p + 1) & ~1;
  const long al = bytes >= 16384 ? 4096 : 128;
  return (int)(((bytes + al - 1) / al * al) / es);
}

int check_theta(ppls_ctx* c, const ppls_theta* th, int r) {
  if (!th || !th->W || !th->C || !th->B || !th->sigT) return fail(c, PPLS_E_ARG, "theta has NULL fields");
  if (r < 1 || r > PPLS_RMAX) return fail(c, PPLS_E_ARG, "r=%d outside [1,%d]", r, PPLS_RMAX);
  if (!(th->sigE > 0) || !(th->sigF > 0) || !(th->sigH >= 0))
    return fail(c, PPLS_E_ARG, "variances must be positive");
  bool fin = std::isfinite(th->sigE) && std::isfinite(th->sigF) && std::isfinite(th->sigH);
  for (int k = 0; k < r; ++k) fin = fin && std::isfinite(th->B[k]) && std::isfinite(th->sigT[k]);
  if (!fin) return fail(c, PPLS_E_ARG, "theta has non-finite B, sigT or variances");
  // PPLS: stopifnot(ncol(X) >= nr_comp, ncol(Y) >= nr_comp)  (EM_W_multi.R:245)
  if (c && c->p > 0 && (c->p < r || c->q < r))
    return fail(c, PPLS_E_ARG, "ncol(X)=%d, ncol(Y)=%d must be >= number of components %d", c->p, c->q, r);
  return PPLS_OK;
}

PplsScalars scalars_of(const ppls_theta* th, int r) {
  PplsScalars s;
  memset(&s, 0, sizeof s);
  for (int k = 0; k < r; ++k) {
    s.b[k] = th->B[k];
    s.t[k] = th->sigT[k];
  }
  s.sigE = th->sigE;
  s.sigF = th->sigF;
  s.sigH = th->sigH;
  ppls_mu_coef(&s, r);
  return s;
}

int ensure_r(ppls_ctx* c, int r, int max_steps) {
  int rc;
  c->em_active = false;   // every entry point that (re)stages theta ends an ppls_em_begin session
  c->xp_active = false;
  if (r != c->r_alloc) {
    for (int i = 0; i < 2; ++i) {
      if ((rc = dalloc(c, &c->W[i], (size_t)c->ldx * r))) return rc;
      if ((rc = dalloc(c, &c->C[i], (size_t)c->ldy * r))) return rc;
      if ((rc = dalloc(c, &c->sc[i], 1))) return rc;
      if ((rc = dalloc(c, &c->gram[i], (size_t)2 * r * r))) return rc;
    }
    if ((rc = dalloc(c, &c->mom, 1))) return rc;
    if ((rc = dalloc(c, &c->vstate, (size_t)2 * r * r))) return rc;
    c->part_ld = (int64_t)r * c->ldx + (int64_t)r * c->ldy + 4 * (int64_t)r * r;
    if ((rc = dalloc(c, &c->stats, (size_t)c->part_ld))) return rc;
    if ((rc = dalloc(c, &c->work, (size_t)2 * (c->p + c->q) * r + 16))) return rc;
    if ((rc = dalloc(c, &c->status, PPLS_STATUS_INTS))) return rc;
    if ((rc = dalloc(c, &c->coefs, (size_t)5 * r))) return rc;
    dfree(c->part);
    dfree(c->Z);
    c->z_cols = 0;
    dfree(c->mu);
    c->part_groups = 0;
    c->r_alloc = r;
  }
  if (max_steps + 2 > c->loglik_cap) {
    if ((rc = dalloc(c, &c->loglik, (size_t)max_steps + 2))) return rc;
    c->loglik_cap = max_steps + 2;
  }
  return PPLS_OK;
}

int upload_theta(ppls_ctx* c, const ppls_theta* th, int r, int slot) {
  // W, C: p x r column-major -> ldx x r padded
  std::vector<double> buf((size_t)std::max(c->ldx, c->ldy) * r, 0.0);
  for (int k = 0; k < r; ++k)
    for (int i = 0; i < c->ldx; ++i) buf[(size_t)k * c->ldx + i] = i < c->p ? th->W[(size_t)k * c->p + i] : 0.0;
  HIPCHK(c, hipMemcpyAsync(c->W[slot], buf.data(), sizeof(double) * c->ldx * r, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < r; ++k)
    for (int i = 0; i < c->ldy; ++i) buf[(size_t)k * c->ldy + i] = i < c->q ? th->C[(size_t)k * c->q + i] : 0.0;
  HIPCHK(c, hipMemcpyAsync(c->C[slot], buf.data(), sizeof(double) * c->ldy * r, hipMemcpyHostToDevice, c->stream));
  PplsScalars s = scalars_of(th, r);
  HIPCHK(c, hipMemcpyAsync(c->sc[slot], &s, sizeof s, hipMemcpyHostToDevice, c->stream));
  // [W'W | C'C] for the finalize's scalar block (later iterations get it from the polar blocks)
  std::vector<double> g((size_t)2 * r * r);
  for (int a = 0; a < r; ++a)
    for (int b = 0; b < r; ++b) {
      double w = 0.0, cc = 0.0;
      for (int i = 0; i < c->p; ++i) w += th->W[(size_t)a * c->p + i] * th->W[(size_t)b * c->p + i];
      for (int i = 0; i < c->q; ++i) cc += th->C[(size_t)a * c->q + i] * th->C[(size_t)b * c->q + i];
      g[(size_t)b * r + a] = w;
      g[(size_t)r * r + (size_t)b * r + a] = cc;
    }
  HIPCHK(c, hipMemcpyAsync(c->gram[slot], g.data(), sizeof(double) * g.size(), hipMemcpyHostToDevice, c->stream));
  // identity warm start for the polar Jacobi: a run's result depends only on its own theta0
  std::vector<double> eye(g.size());
  for (size_t e = 0; e < eye.size(); ++e) eye[e] = ((e % ((size_t)r * r)) % (size_t)(r + 1)) == 0 ? 1.0 : 0.0;
  HIPCHK(c, hipMemcpyAsync(c->vstate, eye.data(), sizeof(double) * eye.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

int download_theta(ppls_ctx* c, int r, int slot, ppls_theta* th) {
  std::vector<double> buf((size_t)std::max(c->ldx, c->ldy) * r);
  HIPCHK(c, hipMemcpy(buf.data(), c->W[slot], sizeof(double) * c->ldx * r, hipMemcpyDeviceToHost));
  for (int k = 0; k < r; ++k)
    for (int i = 0; i < c->p; ++i) th->W[(size_t)k * c->p + i] = buf[(size_t)k * c->ldx + i];
  HIPCHK(c, hipMemcpy(buf.data(), c->C[slot], sizeof(double) * c->ldy * r, hipMemcpyDeviceToHost));
  for (int k = 0; k < r; ++k)
    for (int i = 0; i < c->q; ++i) th->C[(size_t)k * c->q + i] = buf[(size_t)k * c->ldy + i];
  PplsScalars s;
  HIPCHK(c, hipMemcpy(&s, c->sc[slot], sizeof s, hipMemcpyDeviceToHost));
  for (int k = 0; k < r; ++k) {
    th->B[k] = s.b[k];
    th->sigT[k] = s.t[k];
  }
  th->sigE = s.sigE;
  th->sigF = s.sigF;
  th->sigH = s.sigH;
  return PPLS_OK;
}

int download_moments(ppls_ctx* c, int r, ppls_expect* e) {
  if (!e) return PPLS_OK;
  PplsMoments m;
  HIPCHK(c, hipMemcpy(&m, c->mom, sizeof m, hipMemcpyDeviceToHost));
  for (int k = 0; k < r; ++k) {
    if (e->Ctt) e->Ctt[k] = m.Ctt[k];
    if (e->Cuu) e->Cuu[k] = m.Cuu[k];
    if (e->Cut) e->Cut[k] = m.Cut[k];
  }
  e->Cee = m.Cee;
  e->Cff = m.Cff;
  if (e->Chh)
    for (int i = 0; i < r * r; ++i) e->Chh[i] = m.Chh[i];
  return PPLS_OK;
}

int download_mu(ppls_ctx* c, int r, ppls_expect* e) {
  if (!e || (!e->mu_T && !e->mu_U) || c->n_local == 0) return PPLS_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t blk = sizeof(double) * (size_t)c->n_local * r;
  if (e->mu_T) HIPCHK(c, hipMemcpy(e->mu_T, c->mu, blk, hipMemcpyDeviceToHost));
  if (e->mu_U) HIPCHK(c, hipMemcpy(e->mu_U, c->mu + (size_t)c->n_local * r, blk, hipMemcpyDeviceToHost));
  return PPLS_OK;
}

// The finalize's Cholesky-QR1 acceptance bound on ||R1||_F ||R1^-1||_F (>= kappa_2): CholQR1 loses
// ~eps kappa^2 of orthogonality, so the default keeps kappa <= 40 (<= 1e-13); at C3/C4 it lets
// Y'mu_U (kappa ~ 20) skip the second Cholesky-QR pass (profiles/r3_polar1_kappa_ab.txt).
int polar1_bound(const ppls_ctx* c, int r) {
  if (c->polar1_kappa > 0) return c->polar1_kappa;
  return std::min(8 * r, 40);
}

int grid_of(ppls_ctx* c) { return c->grid_opt > 0 ? c->grid_opt : c->num_cus; }

// Allreduce in place (sum) over ranks, on the context stream: RCCL, or the caller's host
// reduction (ppls_set_reducer: device -> host, fn sums over the caller's ranks, host -> device).
int allreduce(ppls_ctx* c, double* buf, size_t count) {
  if (c->reducer) {
    if (c->reduce_host.size() < count) c->reduce_host.resize(count);
    double* h = c->reduce_host.data();
    HIPCHK(c, hipMemcpyAsync(h, buf, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = c->reducer(c->reducer_user, h, (int64_t)count);
    if (rc != 0) return fail(c, PPLS_E_COMM, "host reducer returned %d", rc);
    HIPCHK(c, hipMemcpyAsync(buf, h, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PPLS_OK;
  }
  if (!c->comm) return PPLS_OK;   // a 1-rank communicator still takes the RCCL path
  RCCLCHK(c, ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, c->comm, c->stream));
  return PPLS_OK;
}

// Whether other ranks take part in this context's calls.
bool collective(const ppls_ctx* c) { return c->nranks > 1 || c->reducer; }

// The agreement before a large collective: vals[0..n) (n <= 8, the length of c->flag) summed over
// the ranks, in place and waited for.  A rank puts 1 where a step of its own failed, and nobody
// enters the collective that follows alone.  Nothing happens without other ranks.
int agree(ppls_ctx* c, double* vals, int n) {
  if (!collective(c)) return PPLS_OK;
  HIPCHK(c, hipMemcpyAsync(c->flag, vals, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  const int rc = allreduce(c, c->flag, (size_t)n);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(vals, c->flag, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

// Per-group partials plus, behind them, the two-stage reduction's chunk sums (sized for the largest
// group count seen, so the tail pointer part + part_groups * part_ld is always in bounds).
int ensure_part(ppls_ctx* c, int groups) {
  if (groups <= c->part_groups && c->part) return PPLS_OK;
  const size_t tmp = (size_t)ppls_reduce_tmp_len(groups, c->part_ld);
  int rc = dalloc(c, &c->part, (size_t)groups * c->part_ld + tmp);
  c->part_groups = rc ? 0 : groups;
  return rc;
}

// Which sweep kernel runs for this shape: 3 = split ownership (default), 4 = panel (wide p, large r
// or fp32 storage, or option sweep = 3); a->grid is the workgroup count.
int64_t sweep_rows(const ppls_ctx* c) { return c->seg_rows >= 0 ? c->seg_rows : c->n_local; }

int sweep_plan(ppls_ctx* c, int r, PplsSweepArgs* a) {
  const int64_t nrows = sweep_rows(c);
  const int nsplit = ppls_split_supported(r, c->ldx, c->ldy);
  memset(a, 0, sizeof *a);
  a->ldx = c->ldx;
  a->ldy = c->ldy;
  a->p = c->p;
  a->q = c->q;
  a->r = r;
  a->threads = 512;
  a->num_cus = c->num_cus;
  a->dots_rows = c->dots_rows;
  a->dots_pair = c->dots_pair;
  if (c->sweep_mode != 3 && !c->dtype && nsplit > 0) {
    a->ns = nsplit;
    a->pipe = c->pipe_opt;
    a->rp = c->rp_opt;             // 0 = auto: two rows per step wherever instantiated
    int occ = 0;
    a->occ_out = &occ;
    if (ppls_launch_sweep_split(a, c->stream) != hipSuccess || occ < 1) occ = 1;
    a->occ_out = nullptr;
    a->grid = c->grid_opt > 0 ? c->grid_opt : c->num_cus * occ;
    return 3;
  }
  // wide data / large r / fp32 storage: the panel sweep (two GEMM-shaped passes)
  a->grid = c->acc_chunks > 0 ? c->acc_chunks
          : c->grid_opt > 0 ? c->grid_opt : ppls_panel_chunks(nrows, c->ldx, c->ldy, c->num_cus, c->dtype, r);
  a->dots_grid = c->grid_opt;   // the grid option also sets the dots grid (tests: grid-stride path)
  return 4;
}

// Split-sweep row balance (see the context's bal_* fields).  For a full sweep of n_local rows on
// `grid` workgroups, the first call runs PPLS_BAL_CAL calibration launches with per-workgroup
// stamps (host syncs; their partials are overwritten by the real launch that follows): each times
// when every workgroup's row loop ends under the current partition, and the rows of XCD class x
// (g % 8) are rescaled by sqrt(mean end time / class end time) -- a damped fixed-point iteration
// (the first launch only warms up), since a class that finishes early hands its HBM share to the
// others, so the rates move with the partition.  Later calls reuse the boundaries, so results are
// deterministic for the context.  Shapes with fewer than PPLS_BAL_MIN_ROWS rows per workgroup keep
// the even split.
#define PPLS_BAL_CAL 8
#define PPLS_BAL_MIN_ROWS 2048   // C3: 3,906 rows per workgroup; at 488 (one GPU's C4 share) the calibration noise costs more than the tail
namespace {
void bal_bounds_of(const double* w, int grid, int64_t n, std::vector<int64_t>& bnd) {
  bnd.assign((size_t)grid + 1, 0);
  double tot = 0.0;
  for (int g = 0; g < grid; ++g) tot += w[g % 8];
  double cum = 0.0;
  for (int g = 0; g < grid; ++g) {
    cum += w[g % 8];
    int64_t b = g + 1 == grid ? n : std::min<int64_t>(n, (int64_t)std::llround(cum / tot * (double)n));
    bnd[(size_t)g + 1] = std::max(b, bnd[g]);
  }
}
}  // namespace

int balance_rows(ppls_ctx* c, PplsSweepArgs* a) {
  const int grid = a->grid;
  const int64_t n = a->n_local;
  if (grid < 16 || grid > PPLS_STRACE_MAX_WG || n < (int64_t)PPLS_BAL_MIN_ROWS * grid) return PPLS_OK;
  if (!(c->bal_done && c->bal_n == n && c->bal_grid == grid)) {
    int rc;
    struct OwnTrace {   // a stamp buffer of our own unless tracing is on; freed on every exit path
      ppls_ctx* c;
      bool own;
      ~OwnTrace() {
        if (own && c->strace) { (void)hipFree(c->strace); c->strace = nullptr; }
      }
    } tg{c, c->strace == nullptr};
    if (tg.own) HIPCHK(c, hipMalloc(&c->strace, (size_t)PPLS_STRACE_MAX_WG * 4 * sizeof(long long)));
    if ((rc = dalloc(c, &c->bal_bounds, (size_t)grid + 1))) return rc;
    PplsSweepArgs b = *a;
    b.trace = c->strace;
    b.row_bounds = c->bal_bounds;
    b.stop = nullptr;
    b.mu = nullptr;
    b.write_mu = 0;
    double w[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    std::vector<int64_t> bnd;
    std::vector<long long> st((size_t)grid * 4);
    for (int k = 0; k < PPLS_BAL_CAL; ++k) {
      bal_bounds_of(w, grid, n, bnd);
      HIPCHK(c, hipMemcpyAsync(c->bal_bounds, bnd.data(), sizeof(int64_t) * bnd.size(), hipMemcpyHostToDevice,
                               c->stream));
      HIPCHK(c, ppls_launch_sweep_split(&b, c->stream));
      HIPCHK(c, hipMemcpyAsync(st.data(), c->strace, st.size() * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      long long t0 = st[0];
      for (int g = 1; g < grid; ++g) t0 = std::min(t0, st[(size_t)g * 4]);
      double cls[8] = {0}, cnt[8] = {0}, mean = 0.0;
      for (int g = 0; g < grid; ++g) {
        cls[g % 8] += (double)(st[(size_t)g * 4 + 2] - t0);   // this workgroup's row loop ends
        cnt[g % 8] += 1.0;
      }
      bool ok = true;
      for (int x = 0; x < 8; ++x) {
        cls[x] = cnt[x] > 0 ? cls[x] / cnt[x] : 0.0;
        ok = ok && cls[x] > 0.0;
        mean += cls[x] / 8.0;
      }
      if (!ok) break;
      if (k == 0) continue;   // the first launch warms caches and clocks; its times are not used
      for (int x = 0; x < 8; ++x) w[x] *= std::sqrt(mean / cls[x]);   // damped: the rates move with the load
      double wm = 0.0;
      for (int x = 0; x < 8; ++x) wm += w[x] / 8.0;
      for (int x = 0; x < 8; ++x) w[x] = std::min(1.1, std::max(0.9, w[x] / wm));   // a mis-measurement
    }                                                                                 // cannot starve an XCD
    for (int x = 0; x < 8; ++x) c->bal_w[x] = std::round(w[x] * 4096.0) / 4096.0;
    bal_bounds_of(c->bal_w, grid, n, bnd);
    HIPCHK(c, hipMemcpy(c->bal_bounds, bnd.data(), sizeof(int64_t) * bnd.size(), hipMemcpyHostToDevice));
    c->bal_done = true;
    c->bal_n = n;
    c->bal_grid = grid;
  }
  a->row_bounds = c->bal_bounds;
  return PPLS_OK;
}

// The next pair of timing events for a statistics launch, when option "timing" selects this one.
int timing_pair(ppls_ctx* c, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!(c->timing > 0 && (c->sweep_count++ % c->timing) == 0)) return PPLS_OK;
  if (c->ev_used == c->ev.size()) {
    std::pair<hipEvent_t, hipEvent_t> pr;
    HIPCHK(c, hipEventCreate(&pr.first));
    HIPCHK(c, hipEventCreate(&pr.second));
    c->ev.push_back(pr);
  }
  *e0 = c->ev[c->ev_used].first;
  *e1 = c->ev[c->ev_used].second;
  ++c->ev_used;
  return PPLS_OK;
}

// One sweep with theta[slot] -> c->stats (all-reduced).  mu_only: just this rank's mu rows (the
// statistics are not reduced: no collective).
int xprod_stats(ppls_ctx* c, int r, int slot, bool fuse = false);

#define PPLS_STREAMED_MSG "the rows were streamed and are not resident"
#define NEED_ROWS(c)                                                        \
  do {                                                                      \
    if ((c)->st_state == 2) return fail((c), PPLS_E_STATE, PPLS_STREAMED_MSG); \
  } while (0)

// The ranks of an open stream hold half-accumulated S, N and means: what ppls_stream_end's
// collectives run over cannot change under them.
#define NOT_WHILE_OPEN(c, what)                                                                          \
  do {                                                                                                   \
    if ((c)->st_state == 1)                                                                              \
      return fail((c), PPLS_E_STATE, "a stream is open: %s cannot change before ppls_stream_end", what); \
  } while (0)

int sweep(ppls_ctx* c, int r, int slot, bool write_mu, bool mu_only = false) {
  int rc;
  if (c->st_state == 2) {   // streamed: the statistics come from S, never from the zero resident rows
    if (write_mu || mu_only || c->seg_rows >= 0) return fail(c, PPLS_E_STATE, PPLS_STREAMED_MSG);
    return xprod_stats(c, r, slot, false);
  }
  PplsSweepArgs a;
  const int plan = sweep_plan(c, r, &a);
  const int64_t nrows = sweep_rows(c);
  if (c->seg_rows >= 0 && write_mu) return fail(c, PPLS_E_STATE, "mu write-out is not available for row segments");
  const int groups = a.grid;
  if ((rc = ensure_part(c, groups))) return rc;
  if (write_mu && !c->mu)
    if ((rc = dalloc(c, &c->mu, (size_t)std::max<int64_t>(c->n_local, 1) * 2 * r))) return rc;
  if (plan == 4 && c->z_cols < 4 * r) {
    dfree(c->Z);
    c->z_cols = 0;
    if ((rc = dalloc(c, &c->Z, (size_t)ppls_panel_z_len(c->n_local, c->ldx, c->ldy, r)))) return rc;
    c->z_cols = 4 * r;
  }
  if (nrows == 0) {
    if (mu_only) return PPLS_OK;
    HIPCHK(c, hipMemsetAsync(c->stats, 0, sizeof(double) * c->part_ld, c->stream));
  } else {
    const size_t esz = c->dtype ? sizeof(float) : sizeof(double);
    a.X = (const double*)((const char*)c->X + (size_t)c->seg_row0 * c->ldx * esz);
    a.Y = (const double*)((const char*)c->Y + (size_t)c->seg_row0 * c->ldy * esz);
    a.n_local = nrows;
    a.Wp = c->W[slot];
    a.Cp = c->C[slot];
    a.sc = c->sc[slot];
    a.part = c->part;
    a.part_ld = c->part_ld;
    a.mu = write_mu ? c->mu : nullptr;
    a.write_mu = write_mu ? 1 : 0;
    // once-read streams bigger than the 256 MB MALL: the non-temporal policy lands 3-9 % faster
    // (6.53 vs 6.34 TB/s at C3); smaller X, Y stay MALL-resident across iterations by default
    const bool nt = c->nt_loads > 0 ||
                    (c->nt_loads < 0 && 8.0 * nrows * (double)(c->ldx + c->ldy) > 256.0 * (1 << 20));
    a.nt = nt ? 1 : 0;
    a.stop = c->sweep_stop;
    a.trace = (plan == 3 && a.grid <= PPLS_STRACE_MAX_WG) ? c->strace : nullptr;
    // the row partition (its one-time calibration launches stay outside the timed events)
    if (plan == 3 && c->balance && c->seg_rows < 0 && (rc = balance_rows(c, &a))) return rc;
    if (mu_only) {   // the rows' mu only (untimed): the panel sweep's dots pass, or the split sweep
      if (plan == 4) HIPCHK(c, ppls_launch_panel_dots(&a, c->dtype, c->Z, c->stream));
      else HIPCHK(c, ppls_launch_sweep_split(&a, c->stream));
      return PPLS_OK;
    }
    hipEvent_t e0, e1;
    if ((rc = timing_pair(c, &e0, &e1))) return rc;
    const bool timed = e0 != nullptr;
    if (timed) HIPCHK(c, hipEventRecord(e0, c->stream));
    if (plan == 3) HIPCHK(c, ppls_launch_sweep_split(&a, c->stream));
    else HIPCHK(c, ppls_launch_sweep_panel(&a, c->dtype, c->Z, a.grid, c->stream));
    if (timed) HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, ppls_launch_reduce2(c->part, groups, c->part_ld, c->part_ld, c->stats,
                                  c->part + (size_t)c->part_groups * c->part_ld, c->sweep_stop, c->stream));
    if (timed && c->comm && !c->reducer) {   // time this iteration's RCCL all-reduce as well
      if (c->ev_ar_used == c->ev_ar.size()) {
        std::pair<hipEvent_t, hipEvent_t> pr;
        HIPCHK(c, hipEventCreate(&pr.first));
        HIPCHK(c, hipEventCreate(&pr.second));
        c->ev_ar.push_back(pr);
      }
      const auto& pr = c->ev_ar[c->ev_ar_used++];
      HIPCHK(c, hipEventRecord(pr.first, c->stream));
      const int rc = allreduce(c, c->stats, (size_t)c->part_ld);
      HIPCHK(c, hipEventRecord(pr.second, c->stream));
      return rc;
    }
  }
  return allreduce(c, c->stats, (size_t)c->part_ld);
}

// The arguments of one finalize launch under the context's current options (everything but the
// pending cross-product Gram, which finalize() below consumes).
int finalize_args(ppls_ctx* c, int r, int cur, int nxt, int logl_index, int type, int stop_step, PplsFinalizeArgs* out) {
  PplsFinalizeArgs& f = *out;
  f.stats = c->stats;
  f.ssq = c->ssq;
  f.N = (double)c->n_total;
  f.p = c->p;
  f.q = c->q;
  f.r = r;
  f.ldx = c->ldx;
  f.ldy = c->ldy;
  f.Wc = c->W[cur];
  f.Cc = c->C[cur];
  f.sc_cur = c->sc[cur];
  f.Wn = c->W[nxt];
  f.Cn = c->C[nxt];
  f.sc_nxt = c->sc[nxt];
  f.mom = c->mom;
  f.loglik = c->loglik;
  f.logl_index = logl_index;
  f.work = c->work;
  f.status = c->status;
  f.qr = type == PPLS_ORTH_QR ? 1 : 0;
  f.mode = 3 | (c->polar1 ? 4 : 0) | (c->exact_gram ? 16 : 0) | (polar1_bound(c, r) << 8) | (c->vorth << 16);
  f.trace = c->ftrace;
  f.gram_cur = c->gram[cur];
  f.gram_nxt = c->gram[nxt];
  f.vstate = c->vstate;
  if (!c->team_bar) {
    int rc;
    if ((rc = dalloc(c, &c->team_bar, 8)) || (rc = dalloc(c, &c->team_part, (size_t)2 * 3 * PPLS_TEAM_MAX * 64)))
      return rc;
    HIPCHK(c, hipMemsetAsync(c->team_bar, 0, 8 * sizeof(unsigned), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  f.team_bar = c->team_bar;
  f.team_rows = c->team_rows;
  f.team_part = c->team_part;
  f.stop = c->sweep_stop ? c->stop_d : nullptr;
  f.stop_mirror = c->sweep_stop ? c->stop_mirror_dev : nullptr;
  f.stop_check = stop_step > 0 ? 1 : 0;
  f.stop_step = stop_step;
  f.atol = c->stop_atol;
  f.xpM = nullptr;
  return PPLS_OK;
}

// own_gram: the scalar block forms W'W, C'C of the current loadings itself (ppls_finalize_stats only;
// every EM path hands it the Gram the previous finalize or the upload left in gram[cur]).
int finalize(ppls_ctx* c, int r, int cur, int nxt, int logl_index, int type, int stop_step = 0,
             bool own_gram = false) {
  PplsFinalizeArgs f;
  int rc;
  if ((rc = finalize_args(c, r, cur, nxt, logl_index, type, stop_step, &f))) return rc;
  if (own_gram) f.gram_cur = nullptr;
  f.xpM = c->xp_pending_gram ? c->xp_M : nullptr;   // the Gram of a cross-product step, formed here
  c->xp_pending_gram = false;
  HIPCHK(c, ppls_launch_finalize(&f, c->stream));
  return PPLS_OK;
}

// The column space of one MFMA Gram (ppls_variances.hip): joint = S = [X Y]'[X Y] over the padded
// rows (X's p real columns of ldx, then Y's q of ldy), else D'D for D = X (xory 0) or Y.
struct GramShape {
  int p, xreal, xcols, yreal;
  const void* X;
  int ldx;
  const void* Y;
  int ldy, ycols;
};

GramShape gram_shape(const ppls_ctx* c, bool joint, int xory) {
  if (joint) return GramShape{c->ldx + c->ldy, c->p, c->ldx, c->q, c->X, c->ldx, c->Y, c->ldy, c->ldy};
  const int p = xory ? c->q : c->p, ld = xory ? c->ldy : c->ldx;
  return GramShape{p, p, ld, 0, xory ? (const void*)c->Y : (const void*)c->X, ld, nullptr, 0, 0};
}

// f32: the storage type of the rows the Gram reads (-1: the context's resident rows, option dtype;
// the streamed chunks are staged in fp64 whatever that option holds and pass 0)
int gram_wave_slots(const ppls_ctx* c, int f32 = -1) {
  return c->num_cus * ppls_gram_occupancy(f32 < 0 ? c->dtype : f32) * 4;
}

// Row splits of a Gram over n rows (0 = auto: halving splits, ppls_gram_plan).
int gram_nsplit(const ppls_ctx* c, const GramShape& g, int64_t n, int req, int f32 = -1) {
  return ppls_gram_plan(g.p, g.xreal, g.xcols, g.yreal, n, gram_wave_slots(c, f32), req, nullptr);
}

// The Gram's work queue for (shape, n, req, split plan, wave slots), prepared once and kept while
// all of them repeat.  drain: a stream whose launches may still read the kept queue (the streamed
// chunks' second stream); it is synchronised before the queue is rebuilt.
int gram_queue(ppls_ctx* c, const GramShape& g, int64_t n, int req, int** q, int f32 = -1, hipStream_t drain = nullptr) {
  const int nsplit = gram_nsplit(c, g, n, req, f32);
  const int64_t key[8] = {g.p, g.xreal, g.xcols, g.yreal, n, req, nsplit, gram_wave_slots(c, f32)};
  if (c->gram_q && !memcmp(key, c->gq_key, sizeof key)) {
    *q = c->gram_q;
    return PPLS_OK;
  }
  *q = nullptr;
  int rc;
  c->gq_key[0] = -1;
  if (drain) HIPCHK(c, hipStreamSynchronize(drain));
  if ((rc = dalloc(c, &c->gram_q, (size_t)ppls_gram_queue_ints(g.p, nsplit)))) return rc;
  HIPCHK(c, ppls_gram_queue_prepare(c->gram_q, g.p, g.xreal, g.xcols, g.yreal, n, gram_wave_slots(c, f32), req, c->stream));
  memcpy(c->gq_key, key, sizeof key);
  *q = c->gram_q;
  return PPLS_OK;
}

// G (device, p x p column-major) = the Gram of this rank's n rows: the MFMA kernel into per-item
// partials, then the finish (sum over splits, mirrored).  ms: the MFMA kernel's duration (HIP
// events), if not null.  The partials are allocated here and freed, unless the caller passes them
// (part_in, ppls_gram_part_doubles(g.p, nsplit) doubles; the caller frees them).  cnt: NULL, or n device
// counts, one per row: the weighted Gram sum_i cnt[i] d_i d_i' (DESIGN §19).  wt: NULL, or n device
// weights likewise; not both.
int gram_run(ppls_ctx* c, const GramShape& g, int64_t n, int req, double* G, float* ms, double* part_in = nullptr,
             const int32_t* cnt = nullptr, const double* wt = nullptr) {
  int rc;
  const int nsplit = gram_nsplit(c, g, n, req);
  double* part = part_in;
  int* q = nullptr;
  if (!part_in && (rc = dalloc(c, &part, (size_t)ppls_gram_part_doubles(g.p, nsplit)))) return rc;
  if ((rc = gram_queue(c, g, n, req, &q))) { if (!part_in) dfree(part); return rc; }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipSuccess;
  if (ms) {
    e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
  }
  if (e == hipSuccess)
    e = ppls_launch_gram_joint(g.X, g.ldx, g.xcols, g.xreal, g.Y, g.ldy, g.ycols, g.yreal, c->dtype, n, g.p, nsplit, part,
                               q, cnt, wt, c->stream);
  if (e == hipSuccess && ms) e = hipEventRecord(e1, c->stream);
  if (e == hipSuccess) e = ppls_launch_gram_finish(part, nsplit, g.p, g.xreal, g.xcols, g.yreal, G, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess && ms) e = hipEventElapsedTime(ms, e0, e1);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (!part_in) dfree(part);
  if (e != hipSuccess) return fail(c, PPLS_E_HIP, "MFMA Gram: %s", hipGetErrorString(e));
  return PPLS_OK;
}

// The int8-MFMA (Chinese-remainder) form of the same Gram (ppls_ozaki.hip).  Plan from the column
// statistics: e_j with max_k |D_kj| < 2^e_j, c_j = 2^e_j sqrt(n / sum_k D_kj^2) (>= 1; about 8 for
// Gaussian columns), L_j = 53 + ceil(log2 c_j) + 2 bits for column j's integers x' = rint(D 2^s_j),
// s_j = L_j - e_j -- the rounding error of every S_ij is then
// <= 2^-(s_i+1) sum|D_kj| + 2^-(s_j+1) sum|D_ki| <= 2^-55 sqrt(S_ii S_jj), under the fp64 GEMM's own
// bound u sum_k |D_ki D_kj| wherever sum |D_ki D_kj| >= sqrt(S_ii S_jj) / 4 (tests/test_gpu_ozaki.py
// checks both on sampled entries against double-double sums) -- and the fewest moduli with
// prod m_l > 2 max_j sum_k x'_kj^2 (>= |sum_k x'_ki x'_kj| by Cauchy-Schwarz).  Per-column widths keep
// every column's sum_k x'^2 below n 2^112 (one shared L = max_j L_j put up to 2 more bits on columns of
// small c_j).  Returns 1 (not an error) when L = max_j L_j > 62, more than PPLS_OZ_MAXMOD moduli are
// needed or the residue planes do not fit: the caller then runs the fp64 MFMA Gram.
bool oz_held(const ppls_ctx* c) { return c->oz_planes || c->oz_res; }

void oz_free(ppls_ctx* c) {
  dfree(c->oz_planes);
  dfree(c->oz_res);
  c->oz_planes = nullptr;
  c->oz_res = nullptr;
  c->oz_planes_len = c->oz_res_len = 0;
}

int gram_run_oz(ppls_ctx* c, const GramShape& g, int64_t n, double* G, float* ms) {
  const int P = g.p, Pp = (P + 255) / 256 * 256;
  const int64_t nkb = (n + PPLS_OZ_KS - 1) / PPLS_OZ_KS;
  const int dtype = c->dtype;
  struct Bufs {
    double* part = nullptr;
    double* st = nullptr;
    int* shift = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Bufs() {
      dfree(part); dfree(st); dfree(shift);
      for (auto e : ev) if (e) (void)hipEventDestroy(e);
    }
  } b;
  int rc;
  const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(256, n / 2048));
  if ((rc = dalloc(c, &b.part, (size_t)chunks * 2 * Pp)) || (rc = dalloc(c, &b.st, (size_t)2 * Pp)) ||
      (rc = dalloc(c, &b.shift, (size_t)Pp)))
    return rc;
  for (auto& e : b.ev) HIPCHK(c, hipEventCreate(&e));
  HIPCHK(c, hipEventRecord(b.ev[0], c->stream));
  HIPCHK(c, ppls_launch_oz_colstats(g.X, g.ldx, g.xcols, g.xreal, g.Y, g.ldy, g.yreal, dtype, Pp, n, chunks, b.part,
                                    b.st, c->stream));
  std::vector<double> st((size_t)2 * Pp);
  HIPCHK(c, hipMemcpyAsync(st.data(), b.st, sizeof(double) * st.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  auto live = [&](int j) { return j < g.xreal || (j >= g.xcols && j - g.xcols < g.yreal); };
  int L = 55;
  std::vector<int> shift((size_t)Pp, 0);
  double qmax = 0.0;   // max_j sum_k x'_kj^2 <= (2^s_j ||D_j|| + sqrt(n) / 2)^2
  for (int j = 0; j < P; ++j) {
    if (!live(j) || !(st[(size_t)j] > 0.0)) continue;
    int ex = 0;
    (void)std::frexp(st[(size_t)j], &ex);   // max = f 2^ex, f in [0.5, 1): max < 2^ex
    const double cj = std::max(1.0, std::ldexp(1.0, ex) * std::sqrt((double)n / st[(size_t)Pp + j]));
    const int Lj = 53 + (int)std::ceil(std::log2(cj)) + 2;
    L = std::max(L, Lj);
    shift[(size_t)j] = Lj - ex;
    const double q = std::ldexp(std::sqrt(st[(size_t)Pp + j]), Lj - ex) + 0.5 * std::sqrt((double)n);
    qmax = std::max(qmax, q * q);
  }
  c->oz_L = L;
  c->oz_shift.assign(shift.begin(), shift.begin() + P);
  if (L > 62) return 1;
  // M > 2 max |sum| (the CRT's range (-M/2, M/2)); qmax is an upper bound up to the rounding of the
  // device's sum of squares (relative <= n u ~ 1e-10 at 1e6 rows), covered by the 1e-7 bit
  const double need = std::log2(std::max(qmax, 1.0)) + 1.0 + 1e-7;
  double bits = 0.0;
  int nmod = 0;
  while (nmod < PPLS_OZ_MAXMOD && bits < need) bits += std::log2((double)ppls_oz_modulus(nmod++));
  if (bits < need) return 1;
  nmod = std::max(nmod, 12);
  c->oz_nmod = nmod;
  const int T = Pp / 256, ntiles = T * (T + 1) / 2, nsplit = ppls_oz_splits(nkb);
  const int64_t pstride = nkb * Pp * PPLS_OZ_KS;
  const size_t need_planes = (size_t)nmod * pstride, need_res = (size_t)nmod * nsplit * ntiles * 65536;
  if (need_planes > c->oz_planes_len || need_res > c->oz_res_len) {   // (re)allocate the kept buffers
    HIPCHK(c, hipStreamSynchronize(c->stream));
    oz_free(c);
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return 1;
    const double want = (double)need_planes + (double)need_res;
    if (want > (double)fr - std::max(1073741824.0, 0.05 * (double)fr)) return 1;
    if (dalloc(c, &c->oz_planes, need_planes) || dalloc(c, &c->oz_res, need_res)) {
      c->err.clear();
      oz_free(c);
      return 1;
    }
    c->oz_planes_len = need_planes;
    c->oz_res_len = need_res;
  }
  int8_t* planes = c->oz_planes;
  uint8_t* res = c->oz_res;
  HIPCHK(c, hipMemcpyAsync(b.shift, shift.data(), sizeof(int) * Pp, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, ppls_launch_oz_residues(g.X, g.ldx, g.xcols, g.xreal, g.Y, g.ldy, g.yreal, dtype, Pp, n, nkb, b.shift,
                                    nmod, planes, pstride, c->stream));
  HIPCHK(c, hipEventRecord(b.ev[1], c->stream));
  HIPCHK(c, ppls_launch_oz_syrk(planes, pstride, Pp, nkb, nmod, res, c->stream));
  HIPCHK(c, hipEventRecord(b.ev[2], c->stream));
  HIPCHK(c, ppls_launch_oz_finish(res, nmod, nsplit, Pp, g.xcols, g.xreal, g.yreal, P, b.shift, G, c->stream));
  HIPCHK(c, hipEventRecord(b.ev[3], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float t01 = 0.f, t12 = 0.f, t23 = 0.f, t03 = 0.f;
  HIPCHK(c, hipEventElapsedTime(&t01, b.ev[0], b.ev[1]));
  HIPCHK(c, hipEventElapsedTime(&t12, b.ev[1], b.ev[2]));
  HIPCHK(c, hipEventElapsedTime(&t23, b.ev[2], b.ev[3]));
  HIPCHK(c, hipEventElapsedTime(&t03, b.ev[0], b.ev[3]));
  c->oz_ms[0] = t01;
  c->oz_ms[1] = t12;
  c->oz_ms[2] = t23;
  c->oz_ms[3] = t03;
  if (ms) *ms = t03;
  return PPLS_OK;
}

// The Gram of the joint columns for S: the int8 form when option gram_int8 asks for it and the data
// allow it, else (or on its fallback) the fp64 MFMA Gram; c->oz_used records which ran.
int gram_run_s(ppls_ctx* c, const GramShape& g, int64_t n, double* G, float* ms, double* part) {
  c->oz_used = 0;
  if (c->gram_int8) {
    const int rc = gram_run_oz(c, g, n, G, ms);
    if (rc == PPLS_OK) {
      c->oz_used = 1;
      return PPLS_OK;
    }
    if (rc < 0) return rc;
  }
  return gram_run(c, g, n, 0, G, ms, part);
}

int xprod_setup(ppls_ctx* c);
bool xprod_choose(ppls_ctx* c, int max_steps, int r);

// Rows per rank the cross-product setup is sized for: the same on every rank (ceil(n_total / nranks)).
int64_t xprod_rows(const ppls_ctx* c) { return (c->n_total + c->nranks - 1) / c->nranks; }

// HBM the cross-product form allocates: S (8 P^2 B), the Gram partials while S is formed (32 KB
// per quadrant item and split; a rank with fewer rows plans no more splits) and M (P x 2 RMAX doubles).
double xprod_bytes(ppls_ctx* c) {
  const GramShape g = gram_shape(c, true, 0);
  const double PP = (double)g.p * g.p;
  return 8.0 * PP + 8.0 * (double)ppls_gram_part_doubles(g.p, gram_nsplit(c, g, xprod_rows(c), 0)) +
         16.0 * g.p * PPLS_RMAX;
}

// Start a run (or session) on the cross-products when the policy picks them.  In auto mode (-1) a
// failed allocation of S -- which xprod_setup reports on every rank alike -- falls back to streaming.
int xprod_begin(ppls_ctx* c, int steps, int r) {
  c->xp_active = c->seg_rows < 0 && xprod_choose(c, steps, r);
  if (!c->xp_active) return PPLS_OK;
  const int rc = xprod_setup(c);
  if (rc == PPLS_OK) return PPLS_OK;
  c->xp_active = false;
  if (rc == PPLS_E_NOMEM && c->xprod < 0) {
    c->err.clear();
    return PPLS_OK;
  }
  return rc;
}

// Cross-product form (ppls_xprod.hip): S = [X Y]'[X Y] over the local rows on MFMA (fp64 products
// of the stored values, exact for fp32 storage), summed over ranks by ONE all-reduce of P^2 doubles;
// afterwards an iteration needs no collective at all (every rank holds the same S and theta).
int xprod_setup(ppls_ctx* c) {
  if (c->xp_ready) return PPLS_OK;
  const int P = c->ldx + c->ldy;
  const size_t PP = (size_t)P * P;
  int rc;
  const auto t0 = std::chrono::steady_clock::now();
  // S, the Gram partials and the Gram's work queue; with collectives every rank must know that all
  // ranks allocated them before anyone enters the all-reduce of S (a rank that returned here alone
  // would leave the others waiting in it), so the allocation outcome is all-reduced first, and the
  // partials and queue allocated here are the ones gram_run uses (no allocation after the agreement)
  const GramShape g = gram_shape(c, true, 0);
  double* part = nullptr;
  int rc_alloc = dalloc(c, &c->xp_S, PP);
  if (!rc_alloc && c->n_local > 0) {
    int* q = nullptr;
    rc_alloc = dalloc(c, &part, (size_t)ppls_gram_part_doubles(P, gram_nsplit(c, g, c->n_local, 0)));
    if (!rc_alloc) rc_alloc = gram_queue(c, g, c->n_local, 0, &q);
  }
  double tot = rc_alloc ? 1.0 : 0.0;
  if (collective(c)) {
    if (!(rc = agree(c, &tot, 1)) && tot > 0.0)
      rc = fail(c, PPLS_E_NOMEM, "cross-products S: %d rank(s) could not allocate %.3g GB of S and Gram partials",
                (int)tot, xprod_bytes(c) / 1e9);
  } else {
    rc = rc_alloc;
  }
  if (rc) {
    dfree(c->xp_S);
    dfree(part);
    return rc;
  }
  c->xp_setup_ms = 0.0;
  if (c->n_local > 0) {
    c->xp_nsplit = gram_nsplit(c, g, c->n_local, 0);
    float ms = 0.f;
    rc = gram_run_s(c, g, c->n_local, c->xp_S, &ms, part);
    dfree(part);
    if (rc) { dfree(c->xp_S); return rc; }
    c->xp_setup_ms = ms;
  } else {
    HIPCHK(c, hipMemsetAsync(c->xp_S, 0, sizeof(double) * PP, c->stream));
  }
  const auto ta = std::chrono::steady_clock::now();
  if ((rc = allreduce(c, c->xp_S, PP))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->xp_setup_ar_ms = collective(c) ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count() : 0.0;
  c->xp_setup_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  c->xp_ready = true;
  c->xp_serial = ++g_xp_serial;
  return PPLS_OK;
}

// Whether a run of max_steps iterations reads S: option xprod = 1 always, 0 never, -1 when the
// modelled cost of forming S plus max_steps + 1 passes over it undercuts max_steps + 1 streaming
// sweeps and S fits.  The model and the memory gate use only values every rank shares (n_total /
// nranks, P, and the smallest free HBM over all ranks, all-reduced when the data were loaded), so
// every rank of a sharded run takes the same path and issues the same collectives.  Memory gate:
// S, its Gram partials and M (xprod_bytes) within the smallest free HBM less max(1 GiB, 5 %).
bool xprod_choose(ppls_ctx* c, int max_steps, int r) {
  if (c->st_state == 2) return true;   // streamed: S is all there is, whatever the option says
  if (c->xprod == 0) return false;
  if (c->xprod == 1) return true;   // forced: xprod_setup reports a failed allocation (all ranks alike)
  if (!c->xp_ready && xprod_bytes(c) > c->mem_free_min - std::max(1073741824.0, 0.05 * c->mem_free_min))
    return false;
  const double P = (double)(c->ldx + c->ldy);
  const double n = (double)((c->n_total + c->nranks - 1) / c->nranks);
  const double esz = c->dtype ? 4.0 : 8.0;
  // the split sweep reads X, Y once; the panel sweep (wide p, r > 8, fp32 storage) twice -- also
  // at r = 1 (C5's initialiser steps: 7.3 ms each, like its r = 10 iterations)
  const bool split = c->sweep_mode != 3 && !c->dtype && ppls_split_supported(r, c->ldx, c->ldy) > 0;
  const double t_sweep = (split ? 1.0 : 2.0) * esz * n * P / 6.5e12 + 5e-6;
  const double t_pass = 8.0 * P * P / 6.5e12 + 5e-6;
  // the Gram's rate in n P^2 per second: fp64 MFMA ~55e12 (C3 226 ms); the int8 CRT form ~1e14
  const double gram_rate = c->gram_int8 ? 1.0e14 : 55e12;
  const double t_setup = c->xp_ready ? 0.0 : n * P * P / gram_rate + (c->nranks > 1 ? 16.0 * P * P / 100e9 : 0.0);
  return ((double)max_steps + 1.0) * (t_sweep - t_pass) > t_setup;
}

// One statistics step from S: c->stats for theta[slot] (no collective: S is global).  fuse: a
// finalize follows, which may form the Gram itself (its scalar block runs in the polar blocks'
// slack: C3 ~2 us of it against the Gram kernel's 4 us + a launch boundary).
int xprod_stats(ppls_ctx* c, int r, int slot, bool fuse) {
  int rc;
  const int P = c->ldx + c->ldy;
  if (!c->xp_ready && (rc = xprod_setup(c))) return rc;
  if (!c->xp_M) {
    if ((rc = dalloc(c, &c->xp_M, (size_t)P * 2 * PPLS_RMAX))) return rc;
  }
  hipEvent_t e0, e1;
  if ((rc = timing_pair(c, &e0, &e1))) return rc;
  if (e0) HIPCHK(c, hipEventRecord(e0, c->stream));
  const int rw = ppls_xprod_tile_rows(P, r, c->xprod_rw, c->num_cus);
  const bool defer = fuse && c->xprod_fuse && r <= 8 && P <= 6144;
  HIPCHK(c, ppls_launch_xprod_tile(c->xp_S, c->ldx, c->ldy, r, rw, c->W[slot], c->C[slot], c->sc[slot], c->stats,
                                   c->xp_M, c->sweep_stop, defer ? 0 : 1, c->stream));
  c->xp_pending_gram = defer;
  if (e1) HIPCHK(c, hipEventRecord(e1, c->stream));
  return PPLS_OK;
}

// The statistics of theta[slot] for an EM iteration: from S when the run reads the cross-products
// (not for the mu write-out, which needs the rows), else one streaming sweep.
int stats_step(ppls_ctx* c, int r, int slot, bool write_mu, bool finalize_next = false) {
  c->xp_pending_gram = false;
  if (c->xp_active && !write_mu && c->seg_rows < 0) return xprod_stats(c, r, slot, finalize_next);
  return sweep(c, r, slot, write_mu);
}

// The device stop flag (2 ints) and its host-mapped mirror, allocated on first use.
int ensure_stop(ppls_ctx* c) {
  if (c->stop_d) return PPLS_OK;
  int rc;
  if ((rc = dalloc(c, &c->stop_d, 2))) return rc;
  HIPCHK(c, hipHostMalloc((void**)&c->stop_mirror, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
  HIPCHK(c, hipHostGetDevicePointer((void**)&c->stop_mirror_dev, c->stop_mirror, 0));
  return PPLS_OK;
}

int reset_stop(ppls_ctx* c) {
  HIPCHK(c, hipMemsetAsync(c->stop_d, 0, 2 * sizeof(int), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  __atomic_store_n(c->stop_mirror, 0, __ATOMIC_SEQ_CST);
  return PPLS_OK;
}

int check_status(ppls_ctx* c) {
  int st = 0;
  HIPCHK(c, hipMemcpy(&st, c->status, sizeof st, hipMemcpyDeviceToHost));
  if (st == -7) {   // a polar team member waited too long: clear the team counters, report
    if (c->team_bar) HIPCHK(c, hipMemset(c->team_bar, 0, 8 * sizeof(unsigned)));
    return fail(c, PPLS_E_HIP, "finalize polar team barrier timed out (status -7)");
  }
  if (st != 0) return fail(c, PPLS_E_NUMERIC, "rank-deficient X'mu_T or Y'mu_U in the M-step (status %d)", st);
  return PPLS_OK;
}

// End a stream (open or finished): wait for its device work, free the staging buffers.  S itself is
// xprod_free's.
void stream_release(ppls_ctx* c) {
  if (c->st_stream) (void)hipStreamSynchronize(c->st_stream);
  (void)hipGetLastError();
  for (int b = 0; b < 2; ++b) dfree(c->st_buf[b]);
  dfree(c->st_cm);
  dfree(c->st_vec);
  dfree(c->st_part);
  dfree(c->st_colpart);
  dfree(c->st_gbuf);
  dfree(c->st_fmean);
  for (int b = 0; b < 2; ++b) {
    dfree(c->st_idx[b]);
    c->st_idx_len[b] = 0;
  }
  for (int*& q : c->st_fq) dfree(q);
  c->st_fq.clear();
  c->st_fq_len.clear();
  c->st_cap = c->st_cm_len = c->st_part_len = c->st_colpart_len = c->st_gbuf_len = 0;
  c->st_state = 0;
  c->st_failed = false;
}

// The fold matrices of a stream opened with folds go with S.
void fold_free(ppls_ctx* c) {
  dfree(c->st_fS);
  c->st_nfolds = 0;
  c->st_sel = -1;
  c->st_fN.clear();
  c->st_fmean_h.clear();
}

// The population cross-products of option meta_xprod go with the data they were formed from.
void meta_xp_free(ppls_ctx* c) {
  dfree(c->mx_S);
  c->mx_K = 0;
  c->mx_local.clear();
  c->mx_total.clear();
}

void xprod_free(ppls_ctx* c) {
  meta_xp_free(c);
  if (c->st_state) {   // S is all a streamed (or streaming) context has: without it there is no data
    stream_release(c);
    c->have_data = false;
    c->em_active = false;
  }
  c->xp_ready = false;
  c->xp_explicit = false;
  c->xp_active = false;
  dfree(c->xp_S);
  dfree(c->xp_M);
  fold_free(c);
  // (the int8 Gram's residue planes are a workspace, not S: kept until gram_int8 = 0, the context's
  // end or an allocation that needs the room -- freeing and re-allocating tens of GB per formation
  // cost 1-5 s per call on some boxes, profiles/r6_gram_int8_percol_c3.jsonl)
}

int compute_ssq(ppls_ctx* c) {
  int rc;
  xprod_free(c);   // data or communicator changed: the cross-products are stale

  const int nb = 1024;
  const int nred = 2 + c->nranks;   // {||X||^2, ||Y||^2, free HBM of rank 0, 1, ...}
  if ((rc = dalloc(c, &c->scratch, (size_t)nb + nred))) return rc;
  HIPCHK(c, hipMemsetAsync(c->ssq, 0, 2 * sizeof(double), c->stream));
  if (c->n_local > 0 && c->dtype) {
    HIPCHK(c, ppls_launch_sumsq_f32((const float*)c->X, c->n_local * c->ldx, c->scratch, nb, c->ssq, c->stream));
    HIPCHK(c, ppls_launch_sumsq_f32((const float*)c->Y, c->n_local * c->ldy, c->scratch, nb, c->ssq + 1, c->stream));
  } else if (c->n_local > 0) {
    HIPCHK(c, ppls_launch_sumsq(c->X, c->n_local * c->ldx, c->scratch, nb, c->ssq, 0, c->stream));
    HIPCHK(c, ppls_launch_sumsq(c->Y, c->n_local * c->ldy, c->scratch, nb, c->ssq + 1, 0, c->stream));
  }
  // one all-reduce carries the sums of squares and every rank's free HBM (in its own slot), so the
  // cross-product form's memory gate (xprod_choose) is the same on every rank
  size_t mfree = 0, mtot = 0;
  HIPCHK(c, hipMemGetInfo(&mfree, &mtot));
  std::vector<double> slots((size_t)c->nranks, 0.0);
  slots[(size_t)c->rank] = (double)mfree;
  double* red = c->scratch + nb;
  HIPCHK(c, hipMemcpyAsync(red, c->ssq, 2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(red + 2, slots.data(), sizeof(double) * slots.size(), hipMemcpyHostToDevice, c->stream));
  if ((rc = allreduce(c, red, (size_t)nred))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->ssq, red, 2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  std::vector<double> h((size_t)nred);
  HIPCHK(c, hipMemcpyAsync(h.data(), red, sizeof(double) * nred, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ssq_host[0] = h[0];
  c->ssq_host[1] = h[1];
  c->mem_free_min = h[2];
  for (int k = 1; k < c->nranks; ++k) c->mem_free_min = std::min(c->mem_free_min, h[(size_t)2 + k]);
  dfree(c->scratch);
  return PPLS_OK;
}

// Non-finite data: R's svd() in orth() refuses X'mu_T with NaN/Inf entries (EM_W_multi.R:732-733),
// so the reference stops on such data.  Detected from the all-reduced sums of squares (a NaN or Inf
// element -- or values past ~1.3e154, whose squares overflow -- makes the global sum non-finite), so
// every rank of a sharded run reaches the same verdict and none is left waiting in a collective.
int check_finite_data(ppls_ctx* c) {
  for (int m = 0; m < 2; ++m)
    if (!std::isfinite(c->ssq_host[m])) {
      c->have_data = false;
      xprod_free(c);
      return fail(c, PPLS_E_ARG,
                  "%c contains NaN or Inf (its sum of squares over all ranks is %g; values beyond 1.3e154 "
                  "also overflow it): the reference's svd() in orth() stops on non-finite data "
                  "(EM_W_multi.R:732-733)",
                  m ? 'Y' : 'X', c->ssq_host[m]);
    }
  return PPLS_OK;
}

// A fit needs ssq(X) > 0 and ssq(Y) > 0: on an all-zero block the reference's first EM step
// divides 0 by 0 (EMstepC_fast's loading normalisation, loglC.cpp:357,385), its log-likelihood
// increment is NA and `if (NA < atol)` stops the fit (EM_W_multi.R:173, :792).
int check_fit_data(ppls_ctx* c) {
  for (int m = 0; m < 2; ++m)
    if (!(c->ssq_host[m] > 0.0))
      return fail(c, PPLS_E_ARG,
                  "%c is all zero (sum of squares over all ranks = 0): the PPLS model is degenerate and the "
                  "reference's fit stops on the NA log-likelihood increment it produces (EM_W_multi.R:173,792)",
                  m ? 'Y' : 'X');
  return PPLS_OK;
}

// The transform record: what the held values carry relative to what was loaded (ppls_get_scaling,
// ppls_get_adjustment).  Every writer of the whole record goes through here.  adj_ss is
// ppls_adjust_data's alone and describes its last call: a record from anywhere else has none.
void record_set(ppls_ctx* c, const std::vector<double>& center, const std::vector<double>& scale, int k,
                const std::vector<double>& zcenter, const std::vector<double>& gamma) {
  c->sc_center = center;
  c->sc_scale = scale;
  c->adj_k = k;
  c->adj_zcenter = zcenter;
  c->adj_gamma = gamma;
  c->adj_ss.clear();
}

// dst's rows or cross-products keep the transform they carry in src.
void record_copy(ppls_ctx* dst, const ppls_ctx* src) {
  record_set(dst, src->sc_center, src->sc_scale, src->adj_k, src->adj_zcenter, src->adj_gamma);
}

// ppls_get_scaling: center 0, scale 1; ppls_get_adjustment: k = 0.
void record_clear(ppls_ctx* c) { record_set(c, {}, {}, 0, {}, {}); }

int alloc_data(ppls_ctx* c, int64_t n_local, int p, int q, int64_t n_total) {
  int rc;
  c->em_active = false;
  if (c->st_state) xprod_free(c);   // new data end a stream and the streamed state
  if (n_local < 0 || p < 1 || q < 1) return fail(c, PPLS_E_ARG, "bad shape n=%lld p=%d q=%d", (long long)n_local, p, q);
  c->n_local = n_local;
  c->n_total = n_total > 0 ? n_total : n_local;
  c->p = p;
  c->q = q;
  c->ldx = ld_of(p, c->dtype, c->ldpad);
  c->ldy = ld_of(q, c->dtype, c->ldpad);
  // X, Y storage (fp64, or fp32 packed into the double allocation)
  const size_t es = c->dtype ? 4 : 8;
  // + 64 doubles of slack: the panel dots kernel reads whole 128-B column tiles, so the last row's
  // partial tile may run past the end (those values meet zero rows of the transposed W, so the
  // slack must hold finite values: it is zeroed here -- reused device memory can hold NaN patterns)
  const size_t xb = (size_t)std::max<int64_t>(n_local, 1) * c->ldx * es, yb = (size_t)std::max<int64_t>(n_local, 1) * c->ldy * es;
  if ((rc = dalloc(c, &c->X, (xb + 7) / 8 + 64))) return rc;
  if ((rc = dalloc(c, &c->Y, (yb + 7) / 8 + 64))) return rc;
  HIPCHK(c, hipMemsetAsync((char*)c->X + xb, 0, ((xb + 7) / 8 + 64) * 8 - xb, c->stream));
  HIPCHK(c, hipMemsetAsync((char*)c->Y + yb, 0, ((yb + 7) / 8 + 64) * 8 - yb, c->stream));
  if (!c->ssq && (rc = dalloc(c, &c->ssq, 2))) return rc;
  if (!c->flag && (rc = dalloc(c, &c->flag, 8))) return rc;
  c->r_alloc = 0;   // force per-r buffers to be re-sized for the new shape
  dfree(c->part);
  dfree(c->Z);
  c->z_cols = 0;
  dfree(c->mu);
  c->part_groups = 0;
  c->have_data = false;
  record_clear(c);        // new data carry no transform and no covariate adjustment
  c->rb_kept = false;     // kept robust weights belonged to the rows that were here
  return PPLS_OK;
}

// ---- contexts derived from another context ---------------------------------------------
// ppls_set_data_from, ppls_xprod_downdate, ppls_xprod_resample / _weighted, ppls_xprod_permute and
// ppls_xprod_adjust fill dst from src; the last three leave dst streamed on a derived S with no rows.

// What no pair of contexts may be: missing, one and the same, on two devices.
int pair_check(ppls_ctx* dst, const ppls_ctx* src) {
  if (!dst || !src) return dst ? fail(dst, PPLS_E_ARG, "NULL source context") : PPLS_E_ARG;
  if (dst == src) return fail(dst, PPLS_E_ARG, "source and destination are the same context");
  if (dst->device != src->device)
    return fail(dst, PPLS_E_ARG, "contexts on different devices (%d, %d)", dst->device, src->device);
  return PPLS_OK;
}

// c without data after an error past the point of no return: never a half-formed S, never an open stream.
int drop_to_no_data(ppls_ctx* c, int rc) {
  if (!c->st_state) c->st_state = 2;   // (xprod_free then releases the stream and clears have_data and any EM session)
  xprod_free(c);
  c->have_data = false;
  return rc;
}

// Whether dst already holds streamed cross-products (no folds) of this shape: the call writes into its S.
bool derived_reuse(const ppls_ctx* dst, int p, int q, int ldx, int ldy) {
  return dst->have_data && dst->st_state == 2 && dst->st_nfolds == 0 && dst->xp_ready && dst->xp_S && dst->p == p &&
         dst->q == q && dst->ldx == ldx && dst->ldy == ldy;
}

// The point of no return: dst's own pending work is waited for (an EM session may still read the S that is
// about to be overwritten), then dst is a streamed context of this shape with no rows, no EM session and an S
// that is not ready -- its own (reuse) or Snew, which it takes.  On any other return than PPLS_OK the
// caller ends with drop_to_no_data; Snew stays the guard's.  what: the entry point, whose: the planned
// paddings' origin, both for the messages.
int derived_begin(ppls_ctx* dst, const char* what, const char* whose, int dtype, int ldpad, int p, int q, int ldx, int ldy,
                  DevGuard& Snew, bool reuse) {
  int rc = hipStreamSynchronize(dst->stream) == hipSuccess ? PPLS_OK : fail(dst, PPLS_E_HIP, "%s: dst's stream failed", what);
  if (!rc && reuse) {
    meta_xp_free(dst);
  } else if (!rc) {
    // (alloc_data / xprod_free do not know the buffers dst keeps across calls: they are dst's, not the data's)
    dst->dtype = dtype;   // the paddings follow the storage type and the padding option (ld_of)
    dst->ldpad = ldpad;
    if (!(rc = alloc_data(dst, 0, p, q, 0))) {
      xprod_free(dst);
      if (dst->ldx != ldx || dst->ldy != ldy)
        rc = fail(dst, PPLS_E_STATE, "%s: paddings %d, %d differ from %s %d, %d", what, dst->ldx, dst->ldy, whose, ldx, ldy);
    }
    if (!rc) {
      dst->xp_S = Snew.release();
      dst->st_state = 2;
      dst->st_center = dst->st_scale = 0;
      dst->n_local = 0;
    }
  }
  dst->st_rows = dst->st_chunks = 0;
  dst->have_data = false;
  dst->em_active = false;
  dst->xp_active = false;
  dst->xp_pending_gram = false;
  return rc;
}

// The close of a call that formed S: the context has data again, under a new serial number.
void derived_publish(ppls_ctx* c, int64_t n_total, double mem_free_min) {
  c->n_total = n_total;
  c->mem_free_min = mem_free_min;
  c->xp_ready = true;
  c->xp_serial = ++g_xp_serial;
  c->xp_explicit = true;   // given by the caller, like ppls_xprod_prepare's: kept until new data or release
  c->have_data = true;
}

// The ranks of src agree on a derived call's allocations and arguments before anyone starts work, so that
// they return together.  noun, alloc_what, bad_what: the messages' parts.
struct AgreeSpec {
  const char *noun, *alloc_what, *bad_what;
  bool args_first;   // which refusal a rank reports when ranks failed in both ways
  bool drop;         // a failed allocation leaves dst without data, and a rank that failed keeps its own message
};

// rc_alloc: this rank's allocations; bad: its verdict on its arguments, with the message bad_err; extra
// (may be NULL): a value summed over the ranks beside the flags.  PPLS_OK: every rank goes on.
int ranks_agree(ppls_ctx* dst, ppls_ctx* src, const AgreeSpec& sp, int rc_alloc, int bad, const std::string& bad_err,
                double* extra) {
  const bool coll = collective(src);
  double f[3] = {rc_alloc ? 1.0 : 0.0, bad ? 1.0 : 0.0, extra ? *extra : 0.0};
  int rc;
  if (coll && (rc = agree(src, f, extra ? 3 : 2))) {
    dst->err = src->err;
    return rc;
  }
  if (extra) *extra = f[2];
  for (int t = 0; t < 2; ++t) {
    if ((t == 0) == sp.args_first) {
      if (!(f[1] > 0.0)) continue;   // a refusal: dst holds what it held (buffers that grew are not its data)
      if (bad) dst->err = bad_err;
      return bad ? bad : fail(dst, PPLS_E_ARG, "%s: %d other rank(s) passed %s", sp.noun, (int)f[1], sp.bad_what);
    }
    if (!(f[0] > 0.0)) continue;
    if (!rc_alloc || (coll && !sp.drop))
      rc_alloc = fail(dst, PPLS_E_NOMEM, "%s: %d %srank(s) could not allocate %s", sp.noun, (int)f[0], sp.drop ? "other " : "",
                      sp.alloc_what);
    return sp.drop ? drop_to_no_data(dst, rc_alloc) : rc_alloc;
  }
  return PPLS_OK;
}

// Canonicalisation of EM_W_multi.R:773-778 / :794-799 applied to a host theta.
void canonicalize(ppls_theta* th, int p, int q, int r) {
  int rot[PPLS_RMAX];
  double sgn[PPLS_RMAX];
  ppls_canonical_order(th->sigT, th->B, r, rot, sgn);
  std::vector<double> W((size_t)p * r), C((size_t)q * r);
  double B[PPLS_RMAX], T[PPLS_RMAX];
  for (int j = 0; j < r; ++j) {
    // W.[,rotLoad] %*% diag(signLoad): column j <- old column rot[j] scaled by signLoad[j]
    for (int i = 0; i < p; ++i) W[(size_t)j * p + i] = th->W[(size_t)rot[j] * p + i] * sgn[j];
    for (int i = 0; i < q; ++i) C[(size_t)j * q + i] = th->C[(size_t)rot[j] * q + i] * sgn[j];
    B[j] = th->B[rot[j]] * sgn[rot[j]];   // diag(B %*% diag(signLoad))[rotLoad]
    T[j] = th->sigT[rot[j]];
  }
  memcpy(th->W, W.data(), sizeof(double) * W.size());
  memcpy(th->C, C.data(), sizeof(double) * C.size());
  for (int j = 0; j < r; ++j) {
    th->B[j] = B[j];
    th->sigT[j] = T[j];
  }
}

bool theta_finite(const ppls_theta* th, int p, int q, int r) {
  bool ok = std::isfinite(th->sigE) && std::isfinite(th->sigF) && std::isfinite(th->sigH);
  for (int k = 0; k < r && ok; ++k) ok = std::isfinite(th->B[k]) && std::isfinite(th->sigT[k]);
  for (size_t e = 0; e < (size_t)p * r && ok; ++e) ok = std::isfinite(th->W[e]);
  for (size_t e = 0; e < (size_t)q * r && ok; ++e) ok = std::isfinite(th->C[e]);
  return ok;
}

// Sequential Householder QR of the n x c matrix S (ld n, c <= n): E becomes the first c columns of Q (n x c) and
// R the c x c factor (column-major, upper; its diagonal carries the reflectors' signs).  floor2: per column,
// what the squared norm of the pivot column must exceed (NULL: 0).  Returns the first column whose pivot does
// not, or -1.
int host_householder(const double* S, int n, int c, const double* floor2, std::vector<double>& E, double* R) {
  std::vector<double> A(S, S + (size_t)n * c), vtv(c);
  std::fill(R, R + (size_t)c * c, 0.0);
  for (int k = 0; k < c; ++k) {
    double s2 = 0.0;
    for (int i = k; i < n; ++i) s2 += A[(size_t)k * n + i] * A[(size_t)k * n + i];
    const double sig = std::sqrt(s2), akk = A[(size_t)k * n + k];
    if (!(s2 > (floor2 ? floor2[k] : 0.0))) return k;
    const bool last = k == n - 1;   // nothing to reflect: R_kk = a_kk (dqrdc2, dlarfg), H_k = I
    const double alpha = last ? akk : akk >= 0.0 ? -sig : sig;
    vtv[k] = last ? 0.0 : 2.0 * sig * (sig + std::fabs(akk));
    A[(size_t)k * n + k] = akk - alpha;
    R[k * c + k] = alpha;
    for (int j = k + 1; j < c; ++j) {
      double d = 0.0;
      for (int i = k; i < n; ++i) d += A[(size_t)k * n + i] * A[(size_t)j * n + i];
      const double f = 2.0 * d / vtv[k];
      for (int i = k; i < n; ++i) A[(size_t)j * n + i] -= f * A[(size_t)k * n + i];
      R[j * c + k] = A[(size_t)j * n + k];
    }
  }
  E.assign((size_t)n * c, 0.0);
  for (int j = 0; j < c; ++j) E[(size_t)j * n + j] = 1.0;
  for (int k = c - 1; k >= 0; --k)
    for (int j = 0; j < c; ++j) {
      double d = 0.0;
      for (int i = k; i < n; ++i) d += A[(size_t)k * n + i] * E[(size_t)j * n + i];
      const double f = vtv[k] > 0.0 ? 2.0 * d / vtv[k] : 0.0;
      for (int i = k; i < n; ++i) E[(size_t)j * n + i] -= f * A[(size_t)k * n + i];
    }
  return -1;
}

// Host polar factor / QR factor of the p x r matrix S (ld p): sequential Householder QR, then the
// same small Jacobi polar as the device.  out: p x r.
int host_orth(const double* S, int p, int r, int type, double* out) {
  std::vector<double> E;
  double R[PPLS_RMAX * PPLS_RMAX], P[PPLS_RMAX * PPLS_RMAX];
  if (host_householder(S, p, r, nullptr, E, R) >= 0) return PPLS_E_NUMERIC;
  if (type == PPLS_ORTH_QR) {   // sign_e * qr.Q(qr(S)), sign_e = sign(<e_1, S_1>) = sign(R_11) (functions.R:257-259)
    const double sg = R[0] < 0.0 ? -1.0 : 1.0;
    for (size_t e = 0; e < E.size(); ++e) out[e] = sg * E[e];
    return PPLS_OK;
  }
  if (ppls_small_polar(R, r, P) != 0) return PPLS_E_NUMERIC;
  for (int j = 0; j < r; ++j)
    for (int i = 0; i < p; ++i) {
      double s = 0.0;
      for (int k = 0; k < r; ++k) s += E[(size_t)k * p + i] * P[j * r + k];
      out[(size_t)j * p + i] = s;
    }
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_version(void) { return 100; }

const char* ppls_strerror(int code) {
  switch (code) {
    case PPLS_OK: return "ok";
    case PPLS_E_ARG: return "invalid argument";
    case PPLS_E_HIP: return "HIP runtime error";
    case PPLS_E_NUMERIC: return "numerical failure";
    case PPLS_E_STATE: return "invalid state";
    case PPLS_E_COMM: return "RCCL error";
    case PPLS_E_NOMEM: return "out of device memory";
    default: return "unknown error";
  }
}

int ppls_ctx_create(int device, ppls_ctx** out) {
  if (!out) return PPLS_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PPLS_E_HIP;
  if (device < 0 || device >= ndev) return PPLS_E_ARG;
  ppls_ctx* c = new ppls_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return PPLS_E_HIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    c->num_cus = prop.multiProcessorCount;
  *out = c;
  return PPLS_OK;
}

void ppls_ctx_destroy(ppls_ctx* c) {
  if (!c) return;
  if (c->cv_train) {   // the training context of ppls_cv_ppls borrowed c's communicator
    c->cv_train->comm = nullptr;
    ppls_ctx_destroy(c->cv_train);
    c->cv_train = nullptr;
  }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) ncclCommDestroy(c->comm);
  dfree(c->X); dfree(c->Y); dfree(c->ssq); dfree(c->flag);
  for (int i = 0; i < 2; ++i) { dfree(c->W[i]); dfree(c->C[i]); dfree(c->sc[i]); dfree(c->gram[i]); }
  dfree(c->vstate);
  dfree(c->mom); dfree(c->stats); dfree(c->part); dfree(c->Z); dfree(c->mu); dfree(c->loglik);
  c->z_cols = 0;
  dfree(c->work); dfree(c->status); dfree(c->coefs); dfree(c->scratch);
  if (c->ftrace) (void)hipFree(c->ftrace);
  if (c->strace) (void)hipFree(c->strace);
  dfree(c->stop_d);
  c->st_state = 0;
  stream_release(c);
  fold_free(c);
  for (int b = 0; b < 2; ++b)
    if (c->st_done[b]) (void)hipEventDestroy(c->st_done[b]);
  if (c->st_stream) (void)hipStreamDestroy(c->st_stream);
  dfree(c->xp_S);
  dfree(c->xp_M);
  dfree(c->mx_S);
  oz_free(c);
  dfree(c->bal_bounds);
  dfree(c->team_bar);
  dfree(c->team_part);
  dfree(c->gram_q);
  dfree(c->rs_cnt);
  dfree(c->rs_part);
  dfree(c->rs_wt);
  dfree(c->rb_w);
  dfree(c->rb_d2);
  dfree(c->pm_idx);
  dfree(c->pm_blk);
  dfree(c->o2m_buf);
  if (c->stop_mirror) (void)hipHostFree(c->stop_mirror);
  for (auto& e : c->ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (auto& e : c->ev_ar) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (c->blas) (void)rocblas_destroy_handle(c->blas);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* ppls_last_error(const ppls_ctx* c) { return c ? c->err.c_str() : "null context"; }

int ppls_set_option(ppls_ctx* c, const char* key, int64_t value) {
  if (!c || !key) return PPLS_E_ARG;
  if (!strcmp(key, "sweep")) {
    if (value != 0 && value != 3) return fail(c, PPLS_E_ARG, "sweep must be 0 (auto) or 3 (panel)");
    c->sweep_mode = (int)value;
  } else if (!strcmp(key, "grid")) {
    if (value < 0 || value > 65535) return fail(c, PPLS_E_ARG, "grid out of range");
    c->grid_opt = (int)value;
    c->part_groups = 0;
    dfree(c->part);
  } else if (!strcmp(key, "robust_grid")) {
    if (value < 0 || value > 65535) return fail(c, PPLS_E_ARG, "robust_grid out of range");
    c->rb_grid = (int)value;
  } else if (!strcmp(key, "rows_per_step")) {
    if (value < 0 || value > 2) return fail(c, PPLS_E_ARG, "rows_per_step must be 0 (auto), 1 or 2");
    c->rp_opt = (int)value;
  } else if (!strcmp(key, "team_rows")) {
    if (value < 0 || value > (1 << 30)) return fail(c, PPLS_E_ARG, "team_rows must be >= 0");
    c->team_rows = (int)value;
  } else if (!strcmp(key, "polar1")) {
    c->polar1 = value ? 1 : 0;
  } else if (!strcmp(key, "exact_gram")) {
    c->exact_gram = value ? 1 : 0;
  } else if (!strcmp(key, "balance")) {
    c->balance = value ? 1 : 0;
  } else if (!strcmp(key, "polar1_kappa")) {
    if (value < 0 || value > 255) return fail(c, PPLS_E_ARG, "polar1_kappa must be in [0, 255]");
    c->polar1_kappa = (int)value;
  } else if (!strcmp(key, "pipe")) {
    c->pipe_opt = value ? 1 : 0;
  } else if (!strcmp(key, "ldpad")) {   // applies to data set or generated afterwards
    c->ldpad = value ? 1 : 0;
  } else if (!strcmp(key, "dots_rows")) {
    if (value != 0 && value != 32 && value != 64) return fail(c, PPLS_E_ARG, "dots_rows must be 0 (auto), 32 or 64");
    c->dots_rows = (int)value;
  } else if (!strcmp(key, "dots_pair")) {
    if (value < -1 || value > 1) return fail(c, PPLS_E_ARG, "dots_pair must be -1 (auto), 0 or 1");
    c->dots_pair = (int)value;
  } else if (!strcmp(key, "acc_chunks")) {
    if (value < 0 || value > 65535) return fail(c, PPLS_E_ARG, "acc_chunks must be in [0, 65535]");
    c->acc_chunks = (int)value;
  } else if (!strcmp(key, "strace")) {
    if (value && !c->strace) {
      HIPCHK(c, hipMalloc(&c->strace, (size_t)PPLS_STRACE_MAX_WG * 4 * sizeof(long long)));
      HIPCHK(c, hipMemset(c->strace, 0, (size_t)PPLS_STRACE_MAX_WG * 4 * sizeof(long long)));
    } else if (!value && c->strace) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->strace);
      c->strace = nullptr;
    }
  } else if (!strcmp(key, "ftrace")) {
    if (value && !c->ftrace) {
      HIPCHK(c, hipMalloc(&c->ftrace, PPLS_FTRACE_LEN * sizeof(long long)));
      HIPCHK(c, hipMemset(c->ftrace, 0, PPLS_FTRACE_LEN * sizeof(long long)));
    } else if (!value && c->ftrace) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->ftrace);
      c->ftrace = nullptr;
    }
  } else if (!strcmp(key, "dtype")) {
    if (value != 0 && value != 1) return fail(c, PPLS_E_ARG, "dtype must be 0 (fp64) or 1 (fp32 storage)");
    if (c->dtype != (int)value) {
      // a change would ask for the rows again: a streamed context has none, an open stream's layout is fixed
      if (c->st_state == 2) return fail(c, PPLS_E_STATE, PPLS_STREAMED_MSG);
      if (c->st_state == 1) return fail(c, PPLS_E_STATE, "a stream is open: dtype cannot change before ppls_stream_end");
      c->dtype = (int)value;
      c->have_data = false;   // the data must be (re)loaded in the new storage type
      c->rb_kept = false;
    }
  } else if (!strcmp(key, "nt")) {
    if (value < -1 || value > 1) return fail(c, PPLS_E_ARG, "nt must be -1 (auto), 0 or 1");
    c->nt_loads = (int)value;
  } else if (!strcmp(key, "xprod")) {
    if (value < -1 || value > 1) return fail(c, PPLS_E_ARG, "xprod must be -1 (auto), 0 (stream X, Y) or 1 (cross-products)");
    // the path of an ppls_em_begin session is fixed at em_begin: a session on S does not switch to
    // streaming under it -- xprod = 0 ends it (ppls_em_iterate then asks for ppls_em_begin)
    if (value == 0 && c->em_active && c->xp_active && c->st_state != 2) {
      c->em_active = false;
      c->xp_active = false;
    }
    const int was = c->xprod;
    c->xprod = (int)value;
    // streaming from now on: S's 8 (p+q)^2 bytes go back -- unless S came from ppls_xprod_prepare
    // (kept for variances() and later runs until ppls_xprod_release)
    if (value == 0 && was != 0 && !c->xp_explicit && c->st_state == 0) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      xprod_free(c);
    }
  } else if (!strcmp(key, "meta_device")) {
    c->meta_device = value ? 1 : 0;
  } else if (!strcmp(key, "meta_xprod")) {
    if (value != 0 && value != 1) return fail(c, PPLS_E_ARG, "meta_xprod must be 0 (sweep the rows) or 1 (population cross-products)");
    c->meta_xprod = (int)value;
    if (!c->meta_xprod && c->mx_S) {   // back to the sweeps: the K matrices' bytes go back
      HIPCHK(c, hipStreamSynchronize(c->stream));
      meta_xp_free(c);
    }
  } else if (!strcmp(key, "vorth")) {
    if (value < 1 || value > 255) return fail(c, PPLS_E_ARG, "vorth must be in [1, 255]");
    c->vorth = (int)value;
  } else if (!strcmp(key, "xprod_fuse")) {
    c->xprod_fuse = value ? 1 : 0;
  } else if (!strcmp(key, "var_chol")) {
    if (value < 0 || value > 2) return fail(c, PPLS_E_ARG, "var_chol must be 0 (LU), 1 (Cholesky) or 2 (rocSOLVER Cholesky)");
    c->var_chol = (int)value;
  } else if (!strcmp(key, "gram_int8")) {
    if (value < 0 || value > 1) return fail(c, PPLS_E_ARG, "gram_int8 must be 0 (fp64 MFMA Gram) or 1 (int8 CRT form)");
    if ((int)value != c->gram_int8) {
      c->gram_int8 = (int)value;
      if (c->xp_ready && !c->xp_explicit) {   // a different Gram: S is formed again when next needed
        dfree(c->xp_S);
        c->xp_ready = false;
      }
      if (!c->gram_int8) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        oz_free(c);
      }
    }
  } else if (!strcmp(key, "xprod_rw")) {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
      return fail(c, PPLS_E_ARG, "xprod_rw must be 0, 1, 2, 4 or 8");
    c->xprod_rw = (int)value;
  } else if (!strcmp(key, "o2m_path")) {
    if (value < 0 || value > 2) return fail(c, PPLS_E_ARG, "o2m_path must be 0 (auto), 1 (fused) or 2 (two-phase)");
    c->o2m_path = (int)value;
  } else if (!strcmp(key, "timing")) {
    if (value < 0) return fail(c, PPLS_E_ARG, "timing must be >= 0");
    c->timing = (int)value;
    c->sweep_count = 0;
  } else {
    return fail(c, PPLS_E_ARG, "unknown option '%s'", key);
  }
  return PPLS_OK;
}

void ppls_shard_range(int64_t n_total, int nranks, int rank, int64_t* row0, int64_t* n_local) {
  if (nranks < 1) nranks = 1;
  const int64_t b = n_total * rank / nranks, e = n_total * (rank + 1) / nranks;
  if (row0) *row0 = b;
  if (n_local) *n_local = e - b;
}

int ppls_comm_unique_id(char id[128]) {
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return PPLS_E_COMM;
  static_assert(sizeof(u.internal) == 128, "unexpected ncclUniqueId size");
  memcpy(id, u.internal, 128);
  return PPLS_OK;
}

int ppls_comm_init(ppls_ctx* c, int nranks, int rank, const char id[128]) {
  if (!c || nranks < 1 || rank < 0 || rank >= nranks) return PPLS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  NEED_ROWS(c);   // ||X||^2, ||Y||^2 would be re-reduced from the rows
  NOT_WHILE_OPEN(c, "the communicator");
  if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
  if (nranks > 1 && !id) return fail(c, PPLS_E_ARG, "nranks=%d needs the root's unique id", nranks);
  c->nranks = nranks;
  c->rank = rank;
  if (id) {
    ncclUniqueId u;
    memcpy(u.internal, id, 128);
    RCCLCHK(c, ncclCommInitRank(&c->comm, nranks, u, rank));
  }
  if (c->have_data) return compute_ssq(c);
  return PPLS_OK;
}

int ppls_set_reducer(ppls_ctx* c, ppls_reduce_fn fn, void* user) {
  if (!c) return PPLS_E_ARG;
  NEED_ROWS(c);
  NOT_WHILE_OPEN(c, "the reducer");
  HIPCHK(c, hipSetDevice(c->device));
  c->reducer = fn;
  c->reducer_user = user;
  if (c->have_data) return compute_ssq(c);   // ||X||^2, ||Y||^2 summed by the new reduction
  return PPLS_OK;
}

int ppls_set_data(ppls_ctx* c, const double* X, const double* Y, int64_t n_local, int p, int q,
                  int layout, int64_t n_total) {
  if (!c || (n_local > 0 && (!X || !Y))) return c ? fail(c, PPLS_E_ARG, "NULL data") : PPLS_E_ARG;
  if (layout != PPLS_LAYOUT_COLMAJOR && layout != PPLS_LAYOUT_ROWMAJOR)
    return fail(c, PPLS_E_ARG, "layout must be 0 (column-major) or 1 (row-major)");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = alloc_data(c, n_local, p, q, n_total);
  if (rc) return rc;
  if (n_local > 0 && c->dtype) {   // fp32 storage: build fp64 row-major chunks, then convert
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_local, (int64_t)(256 << 20) / (8LL * (c->ldx + p))));
    double *tmp = nullptr, *tcm = nullptr;
    const int wmax = std::max(c->ldx, c->ldy), cmax = std::max(p, q);
    if ((rc = dalloc(c, &tmp, (size_t)chunk * wmax))) return rc;
    if ((rc = dalloc(c, &tcm, (size_t)chunk * cmax))) { dfree(tmp); return rc; }
    for (int m = 0; m < 2 && !rc; ++m) {
      const double* src = m == 0 ? X : Y;
      const int cols = m == 0 ? p : q, ld = m == 0 ? c->ldx : c->ldy;
      float* dst = (float*)(m == 0 ? c->X : c->Y);
      for (int64_t r0 = 0; r0 < n_local && !rc; r0 += chunk) {
        const int64_t nc = std::min(chunk, n_local - r0);
        hipError_t e;
        if (layout == PPLS_LAYOUT_ROWMAJOR) {
          e = hipMemset2DAsync(tmp, sizeof(double) * ld, 0, sizeof(double) * ld, nc, c->stream);
          if (e == hipSuccess)
            e = hipMemcpy2DAsync(tmp, sizeof(double) * ld, src + r0 * cols, sizeof(double) * cols,
                                 sizeof(double) * cols, nc, hipMemcpyHostToDevice, c->stream);
        } else {   // column-major n_local x cols: rows [r0, r0 + nc) of every column
          e = hipMemcpy2DAsync(tcm, sizeof(double) * nc, src + r0, sizeof(double) * n_local, sizeof(double) * nc,
                               cols, hipMemcpyHostToDevice, c->stream);
          if (e == hipSuccess) e = ppls_launch_to_rowmajor(tcm, nc, cols, ld, tmp, c->stream);
        }
        if (e == hipSuccess) e = ppls_launch_convert(tmp, 0, dst + r0 * ld, 1, nc * ld, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, PPLS_E_HIP, "fp32 upload: %s", hipGetErrorString(e));
      }
    }
    dfree(tmp);
    dfree(tcm);
    if (rc) return rc;
  } else if (n_local > 0) {
    for (int m = 0; m < 2; ++m) {
      const double* src = m == 0 ? X : Y;
      const int cols = m == 0 ? p : q, ld = m == 0 ? c->ldx : c->ldy;
      double* dst = m == 0 ? c->X : c->Y;
      if (layout == PPLS_LAYOUT_ROWMAJOR) {
        HIPCHK(c, hipMemset2DAsync(dst, sizeof(double) * ld, 0, sizeof(double) * ld, n_local, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(dst, sizeof(double) * ld, src, sizeof(double) * cols, sizeof(double) * cols,
                                   n_local, hipMemcpyHostToDevice, c->stream));
      } else {
        double* tmp = nullptr;
        if ((rc = dalloc(c, &tmp, (size_t)n_local * cols))) return rc;
        HIPCHK(c, hipMemcpyAsync(tmp, src, sizeof(double) * n_local * cols, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, ppls_launch_to_rowmajor(tmp, n_local, cols, ld, dst, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(tmp);
      }
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_data = true;
  if ((rc = compute_ssq(c))) return rc;
  return check_finite_data(c);
}

int ppls_generate_synthetic(ppls_ctx* c, int64_t n_total, int64_t row0, int64_t n_local, int p, int q,
                            int r, const ppls_theta* truth, uint64_t seed) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = check_theta(c, truth, r))) return rc;
  if (row0 < 0 || n_local < 0 || row0 + n_local > n_total) return fail(c, PPLS_E_ARG, "bad row range");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = alloc_data(c, n_local, p, q, n_total))) return rc;
  double *Wt = nullptr, *Ct = nullptr, *TU = nullptr;
  if ((rc = dalloc(c, &Wt, (size_t)p * r))) return rc;
  if ((rc = dalloc(c, &Ct, (size_t)q * r))) { dfree(Wt); return rc; }
  if ((rc = dalloc(c, &TU, (size_t)std::max<int64_t>(n_local, 1) * 2 * r))) { dfree(Wt); dfree(Ct); return rc; }
  PplsScalars s = scalars_of(truth, r);
  hipError_t e = hipMemcpy(Wt, truth->W, sizeof(double) * p * r, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(Ct, truth->C, sizeof(double) * q * r, hipMemcpyHostToDevice);
  if (e == hipSuccess && !c->dtype)
    e = ppls_launch_generate(n_local, row0, p, q, c->ldx, c->ldy, r, &s, Wt, Ct, seed, TU, c->X, c->Y, c->stream);
  if (e == hipSuccess && c->dtype) {   // fp32 storage: generate fp64 row chunks, convert
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(n_local, 1),
                                                                 (int64_t)(512 << 20) / (8LL * (c->ldx + c->ldy))));
    double *gx = nullptr, *gy = nullptr;
    if (dalloc(c, &gx, (size_t)chunk * c->ldx) || dalloc(c, &gy, (size_t)chunk * c->ldy)) e = hipErrorOutOfMemory;
    for (int64_t o = 0; o < n_local && e == hipSuccess; o += chunk) {
      const int64_t nc = std::min(chunk, n_local - o);
      e = ppls_launch_generate(nc, row0 + o, p, q, c->ldx, c->ldy, r, &s, Wt, Ct, seed, TU, gx, gy, c->stream);
      if (e == hipSuccess) e = ppls_launch_convert(gx, 0, (float*)c->X + o * c->ldx, 1, nc * c->ldx, c->stream);
      if (e == hipSuccess) e = ppls_launch_convert(gy, 0, (float*)c->Y + o * c->ldy, 1, nc * c->ldy, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    dfree(gx);
    dfree(gy);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  dfree(Wt); dfree(Ct); dfree(TU);
  if (e != hipSuccess) return fail(c, PPLS_E_HIP, "synthetic generation: %s", hipGetErrorString(e));
  c->have_data = true;
  if ((rc = compute_ssq(c))) return rc;
  return check_finite_data(c);
}

int ppls_philox4x32_10(ppls_ctx* c, const uint32_t* ctr, int64_t count, uint64_t key, uint32_t* out) {
  if (!c) return PPLS_E_ARG;
  if (count < 0 || (count > 0 && (!ctr || !out))) return fail(c, PPLS_E_ARG, "bad counter array");
  if (count == 0) return PPLS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  uint32_t* d = nullptr;
  HIPCHK(c, hipMalloc(&d, sizeof(uint32_t) * 8 * count));
  hipError_t e = hipMemcpy(d, ctr, sizeof(uint32_t) * 4 * count, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = ppls_launch_philox(d, count, key, d + 4 * count, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d + 4 * count, sizeof(uint32_t) * 4 * count, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(c, PPLS_E_HIP, "philox: %s", hipGetErrorString(e));
  return PPLS_OK;
}

int ppls_get_data_rows(ppls_ctx* c, double* X, double* Y, int64_t row_begin, int64_t nrows) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (row_begin < 0 || nrows < 0 || row_begin + nrows > c->n_local) return fail(c, PPLS_E_ARG, "bad row range");
  if (nrows == 0) return PPLS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nrows, (int64_t)(256 << 20) / (8LL * std::max(c->ldx, c->ldy))));
  double* wide = nullptr;
  if (c->dtype && (rc = dalloc(c, &wide, (size_t)chunk * std::max(c->ldx, c->ldy)))) return rc;
  for (int m = 0; m < 2; ++m) {
    double* dst = m == 0 ? X : Y;
    if (!dst) continue;
    const int cols = m == 0 ? c->p : c->q, ld = m == 0 ? c->ldx : c->ldy;
    for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
      const int64_t nc = std::min(chunk, nrows - r0), g0 = row_begin + r0;
      const double* src = (m == 0 ? c->X : c->Y) + g0 * ld;
      hipError_t e = hipSuccess;
      if (c->dtype) {   // fp32 storage: widen the rows first
        e = ppls_launch_convert((const float*)(m == 0 ? c->X : c->Y) + g0 * ld, 1, wide, 0, nc * ld, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        src = wide;
      }
      if (e == hipSuccess)
        e = hipMemcpy2D(dst + r0 * cols, sizeof(double) * cols, src, sizeof(double) * ld, sizeof(double) * cols, nc,
                        hipMemcpyDeviceToHost);
      if (e != hipSuccess) {
        dfree(wide);
        return fail(c, PPLS_E_HIP, "copy back: %s", hipGetErrorString(e));
      }
    }
  }
  dfree(wide);
  return PPLS_OK;
}

int ppls_get_data(ppls_ctx* c, double* X, double* Y, int64_t row_begin, int64_t nrows) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (row_begin < 0 || nrows < 0 || row_begin + nrows > c->n_local) return fail(c, PPLS_E_ARG, "bad row range");
  if (nrows == 0) return PPLS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  for (int m = 0; m < 2; ++m) {
    double* dst = m == 0 ? X : Y;
    if (!dst) continue;
    const int cols = m == 0 ? c->p : c->q, ld = m == 0 ? c->ldx : c->ldy;
    const double* src = (m == 0 ? c->X : c->Y) + row_begin * ld;
    double *tmp = nullptr, *wide = nullptr;
    if ((rc = dalloc(c, &tmp, (size_t)nrows * cols))) return rc;
    if (c->dtype) {   // fp32 storage: widen the rows first
      if ((rc = dalloc(c, &wide, (size_t)nrows * ld))) { dfree(tmp); return rc; }
      HIPCHK(c, ppls_launch_convert((const float*)(m == 0 ? c->X : c->Y) + row_begin * ld, 1, wide, 0, nrows * ld,
                                    c->stream));
      src = wide;
    }
    HIPCHK(c, ppls_launch_to_colmajor(src, nrows, cols, ld, tmp, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipError_t e = hipMemcpy(dst, tmp, sizeof(double) * nrows * cols, hipMemcpyDeviceToHost);
    dfree(tmp);
    dfree(wide);
    if (e != hipSuccess) return fail(c, PPLS_E_HIP, "copy back: %s", hipGetErrorString(e));
  }
  return PPLS_OK;
}

int ppls_data_ssq(ppls_ctx* c, double* ssqX, double* ssqY) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (ssqX) *ssqX = c->ssq_host[0];
  if (ssqY) *ssqY = c->ssq_host[1];
  return PPLS_OK;
}

int ppls_estep(ppls_ctx* c, const ppls_theta* th, int r, ppls_expect* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  if (out && (out->mu_T || out->mu_U)) NEED_ROWS(c);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, 1))) return rc;
  if ((rc = upload_theta(c, th, r, 0))) return rc;
  HIPCHK(c, hipMemsetAsync(c->status, 0, PPLS_STATUS_INTS * sizeof(int), c->stream));
  const bool wm = out && (out->mu_T || out->mu_U);
  if ((rc = sweep(c, r, 0, wm))) return rc;
  if ((rc = finalize(c, r, 0, 1, -1, PPLS_ORTH_SVD))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = download_moments(c, r, out))) return rc;
  return download_mu(c, r, out);
}

int ppls_em_step(ppls_ctx* c, const ppls_theta* in, int r, int type, ppls_theta* out, ppls_expect* fit) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  if ((rc = check_theta(c, in, r))) return rc;
  if (!out || !out->W || !out->C || !out->B || !out->sigT) return fail(c, PPLS_E_ARG, "NULL output theta");
  if (fit && (fit->mu_T || fit->mu_U)) NEED_ROWS(c);
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, 1))) return rc;
  if ((rc = upload_theta(c, in, r, 0))) return rc;
  HIPCHK(c, hipMemsetAsync(c->status, 0, PPLS_STATUS_INTS * sizeof(int), c->stream));
  const bool wm = fit && (fit->mu_T || fit->mu_U);
  if ((rc = sweep(c, r, 0, wm))) return rc;
  if ((rc = finalize(c, r, 0, 1, -1, type))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = check_status(c))) return rc;
  if ((rc = download_moments(c, r, fit))) return rc;
  if ((rc = download_mu(c, r, fit))) return rc;
  return download_theta(c, r, 1, out);
}

int ppls_mstep(ppls_ctx* c, const ppls_expect* fit, int r, int type, ppls_theta* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);   // X'mu_T and Y'mu_U of caller-supplied mu need the rows
  if (!fit || !fit->mu_T || !fit->mu_U || !fit->Ctt || !fit->Cut || !fit->Chh)
    return fail(c, PPLS_E_ARG, "Maximiz_M needs mu_T, mu_U, Ctt, Cut, Cee, Cff, Chh");
  if (!out || !out->W || !out->C || !out->B || !out->sigT) return fail(c, PPLS_E_ARG, "NULL output theta");
  if (r < 1 || r > PPLS_RMAX) return fail(c, PPLS_E_ARG, "bad r");
  if (c->dtype) return fail(c, PPLS_E_ARG, "Maximiz_M from caller-supplied moments needs fp64 storage (dtype 0)");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_r(c, r, 1))) return rc;
  const int grid = grid_of(c);
  const int groups = ppls_acc_groups(std::max<int64_t>(c->n_local, 1), grid);
  if ((rc = ensure_part(c, groups))) return rc;
  if (c->z_cols < 2 * r) {
    dfree(c->Z);
    c->z_cols = 2 * r;
    if ((rc = dalloc(c, &c->Z, (size_t)std::max<int64_t>(c->n_local, 1) * 2 * r))) return rc;
  }
  // Z = [mu_T | mu_U] row-major, coefficients alpha = delta = 1, beta = gamma = 0:
  // the accumulate pass then computes exactly X'mu_T and Y'mu_U (EM_W_multi.R:732-733).
  PplsScalars s;
  memset(&s, 0, sizeof s);
  for (int k = 0; k < r; ++k) { s.alpha[k] = 1.0; s.delta[k] = 1.0; }
  HIPCHK(c, hipMemcpy(c->sc[0], &s, sizeof s, hipMemcpyHostToDevice));
  if (c->n_local > 0) {
    double* tmp = nullptr;
    if ((rc = dalloc(c, &tmp, (size_t)c->n_local * 2 * r))) return rc;
    HIPCHK(c, hipMemcpy(tmp, fit->mu_T, sizeof(double) * c->n_local * r, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(tmp + (size_t)c->n_local * r, fit->mu_U, sizeof(double) * c->n_local * r, hipMemcpyHostToDevice));
    HIPCHK(c, ppls_launch_to_rowmajor(tmp, c->n_local, 2 * r, 2 * r, c->Z, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(tmp);
    PplsSweepArgs a;
    memset(&a, 0, sizeof a);
    a.X = c->X; a.Y = c->Y; a.n_local = c->n_local; a.ldx = c->ldx; a.ldy = c->ldy;
    a.sc = c->sc[0]; a.part = c->part; a.part_ld = c->part_ld; a.r = r; a.grid = grid;
    HIPCHK(c, ppls_launch_accumulate(&a, c->Z, c->stream));
    HIPCHK(c, ppls_launch_reduce(c->part, groups, c->part_ld, c->part_ld, c->stats, 0, c->stream));
  } else {
    HIPCHK(c, hipMemsetAsync(c->stats, 0, sizeof(double) * c->part_ld, c->stream));
  }
  if ((rc = allreduce(c, c->stats, (size_t)c->part_ld))) return rc;
  HIPCHK(c, hipMemsetAsync(c->status, 0, PPLS_STATUS_INTS * sizeof(int), c->stream));
  PplsFinalizeArgs f;
  memset(&f, 0, sizeof f);
  f.stats = c->stats; f.ssq = c->ssq; f.N = (double)c->n_total; f.p = c->p; f.q = c->q; f.r = r;
  f.ldx = c->ldx; f.ldy = c->ldy; f.Wn = c->W[1]; f.Cn = c->C[1]; f.work = c->work; f.status = c->status;
  f.logl_index = -1; f.qr = type == PPLS_ORTH_QR ? 1 : 0; f.mode = 1 | (c->polar1 ? 4 : 0) | (polar1_bound(c, r) << 8);   // polar only
  HIPCHK(c, ppls_launch_finalize(&f, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = check_status(c))) return rc;
  // scalar updates on the given moments (EM_W_multi.R:734-738)
  PplsMoments m;
  memset(&m, 0, sizeof m);
  for (int k = 0; k < r; ++k) { m.Ctt[k] = fit->Ctt[k]; m.Cut[k] = fit->Cut[k]; m.Cuu[k] = fit->Cuu ? fit->Cuu[k] : 0.0; }
  m.Cee = fit->Cee;
  m.Cff = fit->Cff;
  for (int i = 0; i < r * r; ++i) m.Chh[i] = fit->Chh[i];
  PplsScalars nx;
  memset(&nx, 0, sizeof nx);
  ppls_mstep_scalars(&m, r, &nx);
  HIPCHK(c, hipMemcpy(c->sc[1], &nx, sizeof nx, hipMemcpyHostToDevice));
  return download_theta(c, r, 1, out);
}

int ppls_loglik(ppls_ctx* c, const ppls_theta* th, int r, double* out) {
  if (!c || !out) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, 1))) return rc;
  if ((rc = upload_theta(c, th, r, 0))) return rc;
  if ((rc = sweep(c, r, 0, false))) return rc;
  if ((rc = finalize(c, r, 0, 1, 0, PPLS_ORTH_SVD))) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->loglik, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

int ppls_em_run(ppls_ctx* c, ppls_theta* th, int r, int max_steps, double atol, int type, double* loglik,
                int* steps_done, int* negative_increment, ppls_expect* eout) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  if (max_steps < 1) return fail(c, PPLS_E_ARG, "EMsteps must be >= 1");
  if (type != PPLS_ORTH_SVD && type != PPLS_ORTH_QR) return fail(c, PPLS_E_ARG, "type must be SVD (0) or QR (1)");
  if (eout && (eout->mu_T || eout->mu_U)) NEED_ROWS(c);
  if ((rc = check_fit_data(c))) return rc;
  if (!theta_finite(th, c->p, c->q, r)) return fail(c, PPLS_E_ARG, "theta0 has non-finite entries");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, max_steps))) return rc;
  // :773-778 canonicalise theta0 (on a copy; th is overwritten with the estimates at the end)
  {
    std::vector<double> W(th->W, th->W + (size_t)c->p * r), C(th->C, th->C + (size_t)c->q * r);
    std::vector<double> B(th->B, th->B + r), T(th->sigT, th->sigT + r);
    ppls_theta t0 = {W.data(), C.data(), B.data(), T.data(), th->sigE, th->sigF, th->sigH};
    canonicalize(&t0, c->p, c->q, r);
    if ((rc = upload_theta(c, &t0, r, 0))) return rc;
  }
  HIPCHK(c, hipMemsetAsync(c->status, 0, PPLS_STATUS_INTS * sizeof(int), c->stream));
  const bool want_mu = eout && (eout->mu_T || eout->mu_U);
  const bool do_check = !(atol == -INFINITY);   // atol = -Inf: the stop rule never fires
  // statistics from the cross-products S (option xprod; formed here if needed, outside the loop)
  if ((rc = xprod_begin(c, max_steps, r))) return rc;
  // The stop rule (EM_W_multi.R:792) runs on the device: the finalize that sees
  // logl[i] - logl[i-1] < atol sets a flag, and every later kernel of the run exits at once, so the
  // host enqueues iterations without a per-iteration read-back.  It polls the flag's host-mapped
  // mirror and stays at most EM_LOOKAHEAD iterations ahead of the device (events), so a long
  // EMsteps stops launching soon after convergence.  With collectives (RCCL or a host reducer) the
  // break must be the same on every rank: the mirror holds the iteration the rule fired at, which
  // every rank computes from the same all-reduced statistics, and a rank breaks at iteration s
  // iff that iteration is <= s - EM_LOOKAHEAD -- the iteration whose event it has just synced, so
  // the answer does not depend on how far each device has run.
  if (do_check) {
    if ((rc = ensure_stop(c)) || (rc = reset_stop(c))) return rc;
    c->sweep_stop = c->stop_d;
    c->stop_atol = atol;
  }
  struct StopGuard {   // the flag applies to this run only
    ppls_ctx* c;
    std::vector<hipEvent_t> evs;
    ~StopGuard() {
      c->sweep_stop = nullptr;
      c->xp_active = false;
      for (auto e : evs) (void)hipEventDestroy(e);
    }
  } guard{c, {}};
  constexpr int EM_LOOKAHEAD = 8;
  std::vector<hipEvent_t>& evs = guard.evs;
  int cur = 0;
  for (int s = 1; s <= max_steps + 1; ++s) {
    if (do_check && s > EM_LOOKAHEAD) {
      HIPCHK(c, hipEventSynchronize(evs[(size_t)(s - 1 - EM_LOOKAHEAD) % EM_LOOKAHEAD]));
      const int fired = __atomic_load_n(c->stop_mirror, __ATOMIC_ACQUIRE);
      if (fired != 0 && fired <= s - EM_LOOKAHEAD) break;   // converged: stop launching
    }
    const int nxt = cur ^ 1;
    const bool wm = want_mu && !c->xp_active && (do_check || s == max_steps + 1);
    if ((rc = stats_step(c, r, cur, wm, true))) return rc;
    if ((rc = finalize(c, r, cur, nxt, s >= 2 ? s - 2 : -1, type, do_check && s >= 3 ? s : 0))) return rc;
    if (do_check) {
      const size_t k = (size_t)(s - 1) % EM_LOOKAHEAD;
      if (evs.size() <= k) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        evs.push_back(e);
      }
      HIPCHK(c, hipEventRecord(evs[k], c->stream));
    }
    cur = nxt;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // the iteration the run ended at: the finalize of sweep s_stop saw the stop rule fire, so
  // theta_{s_stop - 1} (slot (s_stop - 1) & 1) is the estimate and logl[1 .. s_stop - 1] the trace
  int stopv[2] = {0, 0};   // {sweep the stop rule fired at, 1 if its increment was NaN}
  if (do_check) HIPCHK(c, hipMemcpy(stopv, c->stop_d, sizeof stopv, hipMemcpyDeviceToHost));
  const int s_stop = stopv[0];
  const int i_final = s_stop > 0 ? s_stop - 1 : max_steps;
  cur = i_final & 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = check_status(c))) return rc;
  if (stopv[1])   // every rank saw the same all-reduced increment, so every rank returns this
    return fail(c, PPLS_E_NUMERIC,
                "the log-likelihood increment of EM iteration %d is NaN: the reference stops PPLS_simult with "
                "an error there (`if (NA < atol)`, EM_W_multi.R:792)", i_final);
  if (c->xp_active && want_mu) {
    // Eout's mu_T, mu_U (:802) need the rows: one sweep of theta_{i_final} that only writes this
    // rank's mu rows (mu = a_i diag(alpha) + b_i diag(beta), ... from the rank's own rows and
    // theta's scalars: no collective, so ranks may ask for mu or not independently).  Eout's
    // moments are those the loop's finalize computed from S for theta_{i_final}.
    c->sweep_stop = nullptr;
    if ((rc = sweep(c, r, cur, true, true))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  std::vector<double> l(i_final);
  HIPCHK(c, hipMemcpy(l.data(), c->loglik, sizeof(double) * i_final, hipMemcpyDeviceToHost));
  if (loglik) std::copy(l.begin(), l.end(), loglik);
  if (negative_increment) {
    int neg = 0;
    for (int i = 1; i < i_final; ++i) neg |= (l[i] - l[i - 1] < 0);
    *negative_increment = neg;   // warning("Negative increments of likelihood"), :801
  }
  if (steps_done) *steps_done = i_final;
  if ((rc = download_theta(c, r, cur, th))) return rc;
  // never PPLS_OK with a non-finite trace or estimate (with atol = -Inf no stop rule looks at them)
  for (int i = 0; i < i_final; ++i)
    if (!std::isfinite(l[i]))
      return fail(c, PPLS_E_NUMERIC, "non-finite log-likelihood %g at EM iteration %d", l[i], i + 1);
  if (!theta_finite(th, c->p, c->q, r)) return fail(c, PPLS_E_NUMERIC, "non-finite estimates after %d EM iterations", i_final);
  canonicalize(th, c->p, c->q, r);   // :794-799
  if ((rc = download_moments(c, r, eout))) return rc;
  return download_mu(c, r, eout);
}

// ============================================================================ sequential initialiser
// PPLS (EM_W_multi.R:229-279) -> PPLSi (:116-180) -> EMstep_W (:51-73) -> EMstepC_fast
// (loglC.cpp:340-397).  Component k is fitted on Xc = X P_1 ... P_{k-1}, P_j = I - w_j w_j'
// (:270-271; Yc likewise with c_j) without forming Xc: the r = 1 sweep runs on X with the weight
// P_1..P_{k-1} w (so Xw of the sweep is Xc w), Xc' mu_T = P_{k-1}..P_1 X' mu_T, and
// ||Xc||^2 = ||X||^2 - sum_j ||Xc_j w_j||^2 (w_j unit).  The sweeps (all the data traffic) run on
// the device; the O((p+q) k) rank-1 update between them runs here on the host.
}  // extern "C"

namespace {

// v <- P_{m-1} ... P_0 v (first_last = true: P_0 applied first) or P_0 ... P_{m-1} v.
void deflate(const std::vector<double>& Wp, int m, int n, double* v, bool first_last) {
  for (int jj = 0; jj < m; ++jj) {
    const int j = first_last ? jj : m - 1 - jj;
    const double* w = Wp.data() + (size_t)j * n;
    double d = 0.0;
    for (int i = 0; i < n; ++i) d += w[i] * v[i];
    for (int i = 0; i < n; ++i) v[i] -= d * w[i];
  }
}

struct Rank1 {
  std::vector<double> w, c;   // unit loadings (the estimates)
  double B, sigE, sigF, sigH, sigT;
};

PplsRank1 r1_of(const Rank1& t) { return PplsRank1{t.B, t.sigE, t.sigF, t.sigH, t.sigT}; }

// The meta calls' params (5 x K: B, sigE, sigF, sigH, sigT, population j at [. K + j]) to the scalars
// of population j (no loadings), and back from a Rank1 or a PplsRank1.
Rank1 rank1_from_params(const double* params, int K, int j) {
  Rank1 t;
  t.B = params[j];
  t.sigE = params[K + j];
  t.sigF = params[2 * K + j];
  t.sigH = params[3 * K + j];
  t.sigT = params[4 * K + j];
  return t;
}

template <class R>
void rank1_to_params(const R& t, double* params, int K, int j) {
  params[j] = t.B;
  params[K + j] = t.sigE;
  params[2 * K + j] = t.sigF;
  params[3 * K + j] = t.sigH;
  params[4 * K + j] = t.sigT;
}

// A one-component start (the first component of init) with its loadings.
Rank1 rank1_from_init(const ppls_theta* init, int p, int q) {
  Rank1 t;
  t.w.assign(init->W, init->W + p);
  t.c.assign(init->C, init->C + q);
  t.B = init->B[0];
  t.sigE = init->sigE;
  t.sigF = init->sigF;
  t.sigH = init->sigH;
  t.sigT = init->sigT[0];
  return t;
}

// EMstep_W's coefficients (:60-70) and EMstepC_fast's mu coefficients (:354, :358) (ppls_math.h).
void rank1_coefs(const Rank1& t, double* c1, double* c2, double* c3, double* al, double* be, double* ga,
                 double* de) {
  const PplsRank1 s = r1_of(t);
  ppls_rank1_coefs(&s, c1, c2, c3, al, be, ga, de);
}

// Stage component t for an r = 1 sweep over the deflated data: weights P_0..P_{m-1} w, P_0..P_{m-1} c
// (so the sweep over X, Y computes Xc w, Yc c) and the sweep scalars.
int rank1_stage(ppls_ctx* c, const Rank1& t, const std::vector<double>& Wp, const std::vector<double>& Cp, int m) {
  std::vector<double> wv(c->ldx, 0.0), cv(c->ldy, 0.0);
  std::copy(t.w.begin(), t.w.end(), wv.begin());
  std::copy(t.c.begin(), t.c.end(), cv.begin());
  deflate(Wp, m, c->p, wv.data(), false);   // X P_0 .. P_{m-1} w
  deflate(Cp, m, c->q, cv.data(), false);
  PplsScalars s;
  const PplsRank1 r1 = r1_of(t);
  ppls_rank1_sweep_scalars(&r1, &s);
  HIPCHK(c, hipMemcpyAsync(c->W[0], wv.data(), sizeof(double) * c->ldx, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->C[0], cv.data(), sizeof(double) * c->ldy, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->sc[0], &s, sizeof s, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host vectors go out of scope
  return PPLS_OK;
}

// One r = 1 sweep of theta t over the deflated data: stats -> host (SX p, SY q, G 2 x 2).
int rank1_sweep(ppls_ctx* c, const Rank1& t, const std::vector<double>& Wp, const std::vector<double>& Cp,
                int m, std::vector<double>& SX, std::vector<double>& SY, double G[4]) {
  int rc;
  if ((rc = rank1_stage(c, t, Wp, Cp, m))) return rc;
  if ((rc = stats_step(c, 1, 0, false))) return rc;
  std::vector<double> st((size_t)c->part_ld);
  HIPCHK(c, hipMemcpyAsync(st.data(), c->stats, sizeof(double) * c->part_ld, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  SX.assign(st.begin(), st.begin() + c->p);
  SY.assign(st.begin() + c->ldx, st.begin() + c->ldx + c->q);
  for (int e = 0; e < 4; ++e) G[e] = st[(size_t)c->ldx + c->ldy + e];
  return PPLS_OK;
}

// logl_W(Xc, Yc, w, c, B, sigE, sigF, sigH, sigT) from the sweep's Gram (:297-323, r = 1).
double rank1_loglik(const Rank1& t, const double G[4], double ssqX, double ssqY, double N, int p, int q) {
  const PplsRank1 s = r1_of(t);
  return ppls_rank1_loglik(&s, G, ssqX, ssqY, N, p, q);
}

// The rank-1 E-step moments and M-step scalars from one sweep's Gram (ppls_rank1_scalars, shared
// with the device step kernel): the arithmetic of EMstepC_fast (loglC.cpp:353-387) and meta_Estep /
// meta_Mstep (loglC.cpp:399-474).
void rank1_scalars(const Rank1& t, const double G[4], double ssqX, double ssqY, double N, int p, int q,
                   Rank1* n) {
  const PplsRank1 s = r1_of(t);
  PplsRank1 o;
  ppls_rank1_scalars(&s, G, ssqX, ssqY, N, p, q, &o);
  n->B = o.B;
  n->sigE = o.sigE;
  n->sigF = o.sigF;
  n->sigH = o.sigH;
  n->sigT = o.sigT;
}

// Device buffers of one PPLSi fit (ppls_rank1_step_kernel's state).
struct Rank1Dev {
  double* Wp = nullptr;   // deflation vectors (p x a), (q x a)
  double* Cp = nullptr;
  double* tw = nullptr;   // the component's loadings (p), (q)
  double* tc = nullptr;
  double* consW = nullptr;
  double* consC = nullptr;
  double* lv = nullptr;   // logvalue (EMsteps + 1) and the last Gram (4)
  PplsRank1* st = nullptr;
  ~Rank1Dev() { dfree(Wp); dfree(Cp); dfree(tw); dfree(tc); dfree(consW); dfree(consC); dfree(lv); dfree(st); }
};

// PPLSi's EM loop for component m (EM_W_multi.R:147-173) entirely on the device: per step one r = 1
// sweep and one ppls_rank1_step_kernel (loglik, stop rule, EMstepC_fast update, constraints, next
// weights), no host round trip.  The host enqueues up to EMsteps steps, at most EM_LOOKAHEAD ahead
// of the device, and stops launching once the step kernel reports the end of the fit (host-mapped
// flag = the step it ended at + 1; a rank breaks at step s iff that step is <= s - LOOKAHEAD, whose
// event it has synced, so all ranks break at the same step and their collectives stay matched).
// t: in = the constrained initial component, out = the fit.  lv: logvalue[0..i]; G: the last Gram.
int rank1_fit_device(ppls_ctx* c, Rank1Dev& d, Rank1& t, const ppls_constraint* ck, int m, double ssqX,
                     double ssqY, int max_steps, double atol, int crit_abs, const std::vector<double>& Wp,
                     const std::vector<double>& Cp, std::vector<double>& lv, int* steps, bool* na, double G[4]) {
  int rc;
  const int p = c->p, q = c->q;
  if ((rc = rank1_stage(c, t, Wp, Cp, m))) return rc;
  const PplsRank1 r1 = r1_of(t);
  HIPCHK(c, hipMemcpyAsync(d.tw, t.w.data(), sizeof(double) * p, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.tc, t.c.data(), sizeof(double) * q, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.st, &r1, sizeof r1, hipMemcpyHostToDevice, c->stream));
  PplsRank1StepArgs a;
  memset(&a, 0, sizeof a);
  if (ck) {
    if (ck->W) HIPCHK(c, hipMemcpyAsync(d.consW, ck->W, sizeof(double) * p, hipMemcpyHostToDevice, c->stream));
    if (ck->C) HIPCHK(c, hipMemcpyAsync(d.consC, ck->C, sizeof(double) * q, hipMemcpyHostToDevice, c->stream));
    a.consW = ck->W ? d.consW : nullptr;
    a.consC = ck->C ? d.consC : nullptr;
    if (ck->B) { a.cons_mask |= 1; a.cons_val.B = ck->B[0]; }
    if (ck->sigE) { a.cons_mask |= 2; a.cons_val.sigE = ck->sigE[0]; }
    if (ck->sigF) { a.cons_mask |= 4; a.cons_val.sigF = ck->sigF[0]; }
    if (ck->sigH) { a.cons_mask |= 8; a.cons_val.sigH = ck->sigH[0]; }
    if (ck->sigT) { a.cons_mask |= 16; a.cons_val.sigT = ck->sigT[0]; }
  }
  if ((rc = ensure_stop(c)) || (rc = reset_stop(c))) return rc;
  a.stats = c->stats;
  a.p = p; a.q = q; a.ldx = c->ldx; a.ldy = c->ldy;
  a.N = (double)c->n_total; a.ssqX = ssqX; a.ssqY = ssqY;
  a.Wp = d.Wp; a.Cp = d.Cp; a.m = m;
  a.st = d.st; a.tw = d.tw; a.tc = d.tc;
  a.Wdst = c->W[0]; a.Cdst = c->C[0]; a.scdst = c->sc[0];
  a.lv = d.lv; a.Gkeep = d.lv + max_steps + 1;
  a.max_steps = max_steps; a.crit_abs = crit_abs; a.atol = atol;
  a.stop = c->stop_d; a.stop_mirror = c->stop_mirror_dev;
  struct Guard {
    ppls_ctx* c;
    std::vector<hipEvent_t> evs;
    ~Guard() {
      c->sweep_stop = nullptr;
      for (auto e : evs) (void)hipEventDestroy(e);
    }
  } guard{c, {}};
  c->sweep_stop = c->stop_d;
  constexpr int LOOKAHEAD = 8;
  for (int step = 0; step <= max_steps; ++step) {
    if (step >= LOOKAHEAD) {
      HIPCHK(c, hipEventSynchronize(guard.evs[(size_t)(step - LOOKAHEAD) % LOOKAHEAD]));
      const int ended = __atomic_load_n(c->stop_mirror, __ATOMIC_ACQUIRE);
      if (ended != 0 && ended - 1 <= step - LOOKAHEAD) break;   // the fit ended
    }
    if ((rc = stats_step(c, 1, 0, false))) return rc;
    a.step = step;
    HIPCHK(c, ppls_launch_rank1_step(&a, c->stream));
    {
      const size_t k = (size_t)step % LOOKAHEAD;
      if (guard.evs.size() <= k) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        guard.evs.push_back(e);
      }
      HIPCHK(c, hipEventRecord(guard.evs[k], c->stream));
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int stop[2] = {0, 0};
  HIPCHK(c, hipMemcpy(stop, c->stop_d, sizeof stop, hipMemcpyDeviceToHost));
  if (stop[1] == 2)   // every rank computed the same all-reduced increment
    return fail(c, PPLS_E_NUMERIC,
                "PPLSi component %d: the log-likelihood increment of EM step %d is NaN; the reference stops with "
                "an error there (`if (critfunc(NA) < atol)`, EM_W_multi.R:173)", m + 1, stop[0]);
  *na = stop[1] != 0;
  *steps = stop[0] > 0 ? stop[0] : stop[0] < 0 ? -stop[0] : max_steps;   // < 0: sigma collapse at step -stop[0]-1
  std::vector<double> buf((size_t)max_steps + 5);
  HIPCHK(c, hipMemcpy(buf.data(), d.lv, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
  lv.assign(buf.begin(), buf.begin() + (*steps + 1));
  for (int e = 0; e < 4; ++e) G[e] = buf[(size_t)max_steps + 1 + e];
  PplsRank1 o;
  HIPCHK(c, hipMemcpy(&o, d.st, sizeof o, hipMemcpyDeviceToHost));
  t.B = o.B; t.sigE = o.sigE; t.sigF = o.sigF; t.sigH = o.sigH; t.sigT = o.sigT;
  HIPCHK(c, hipMemcpy(t.w.data(), d.tw, sizeof(double) * p, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(t.c.data(), d.tc, sizeof(double) * q, hipMemcpyDeviceToHost));
  return PPLS_OK;
}

// ||X P_0..P_{m-1}||^2 (and the Y analogue) by an exact residual pass over the resident data,
// all-reduced over ranks.  Used when the running ||X||^2 - sum ||Xc_j w_j||^2 has cancelled to
// below 1e-6 ||X||^2, where its absolute error (~eps ||X||^2) would hide a rank collapse.
int deflated_ssq(ppls_ctx* c, const std::vector<double>& Wp, int m, bool isx, double* out) {
  int rc;
  const int n = isx ? c->p : c->q;
  const int nb = 1024;
  double* Wd = nullptr;
  double* buf = nullptr;
  if ((rc = dalloc(c, &Wd, (size_t)n * std::max(m, 1)))) return rc;
  if ((rc = dalloc(c, &buf, (size_t)nb + 1))) { dfree(Wd); return rc; }
  double res = 0.0;
  hipError_t e = hipMemcpyAsync(Wd, Wp.data(), sizeof(double) * n * m, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = ppls_launch_deflated_ssq(isx ? c->X : c->Y, c->dtype, c->n_local, isx ? c->ldx : c->ldy, n, Wd, m, buf,
                                 nb, buf + nb, c->stream);
  if (e == hipSuccess && c->n_local == 0) e = hipMemsetAsync(buf + nb, 0, sizeof(double), c->stream);
  rc = e == hipSuccess ? allreduce(c, buf + nb, 1) : fail(c, PPLS_E_HIP, "deflated ssq: %s", hipGetErrorString(e));
  if (!rc) {
    e = hipMemcpyAsync(&res, buf + nb, sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, PPLS_E_HIP, "deflated ssq: %s", hipGetErrorString(e));
  }
  dfree(Wd);
  dfree(buf);
  *out = res;
  return rc;
}

using SeqStart = std::function<int(int, const std::vector<double>&, const std::vector<double>&, double, double, Rank1&)>;
int seq_fit(ppls_ctx* c, int a, int max_steps, double atol, int crit_abs, const ppls_constraint* cons,
            ppls_seq_fit* out, const SeqStart& start);

}  // namespace

extern "C" {

int ppls_ppls(ppls_ctx* c, int a, int max_steps, double atol, const ppls_theta* init, ppls_seq_fit* out) {
  return ppls_ppls_ex(c, a, max_steps, atol, 0, init, nullptr, out);
}

int ppls_ppls_ex(ppls_ctx* c, int a, int max_steps, double atol, int crit_abs, const ppls_theta* init,
                 const ppls_constraint* cons, ppls_seq_fit* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (!init) return fail(c, PPLS_E_ARG, "NULL argument");
  const int p = c->p, q = c->q;
  return seq_fit(c, a, max_steps, atol, crit_abs, cons, out,
                 [&](int k, const std::vector<double>&, const std::vector<double>&, double, double, Rank1& t) {
                   if (k < 0) {   // the loop's argument check, after its own
                     for (int j = 0; j < a; ++j)
                       if (!init[j].W || !init[j].C || !init[j].B || !init[j].sigT)
                         return fail(c, PPLS_E_ARG, "init[%d] has NULL fields", j);
                     return (int)PPLS_OK;
                   }
                   t.w.assign(init[k].W, init[k].W + p);
                   t.c.assign(init[k].C, init[k].C + q);
                   t.B = init[k].B[0];
                   t.sigT = init[k].sigT[0];
                   t.sigE = init[k].sigE;
                   t.sigF = init[k].sigF;
                   t.sigH = init[k].sigH;
                   return (int)PPLS_OK;
                 });
}

}  // extern "C"

namespace {

// PPLS's loop (EM_W_multi.R:229-279) behind ppls_ppls_ex and ppls_ppls_o2m: start(k, Wp, Cp, ssqX,
// ssqY, t) supplies component k's starting values, given the fitted loadings w_1..w_k, c_1..c_k
// (column-major) and ||Xc||^2, ||Yc||^2 of the data they deflate.
int seq_fit(ppls_ctx* c, int a, int max_steps, double atol, int crit_abs, const ppls_constraint* cons,
            ppls_seq_fit* out, const SeqStart& start) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (!out || !out->W || !out->C || !out->B || !out->sig) return fail(c, PPLS_E_ARG, "NULL argument");
  if (a < 1 || a > PPLS_RMAX) return fail(c, PPLS_E_ARG, "nr_comp=%d outside [1,%d]", a, PPLS_RMAX);
  if (c->p < a || c->q < a)   // stopifnot(ncol(X) >= nr_comp, ncol(Y) >= nr_comp) (:245)
    return fail(c, PPLS_E_ARG, "ncol(X)=%d, ncol(Y)=%d must be >= number of components %d", c->p, c->q, a);
  if (max_steps < 1) return fail(c, PPLS_E_ARG, "EMsteps must be >= 1");
  int rc;
  if ((rc = check_fit_data(c))) return rc;
  {
    Rank1 none;
    static const std::vector<double> empty;
    if ((rc = start(-1, empty, empty, 0.0, 0.0, none))) return rc;   // the start's own argument check
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, 1, max_steps))) return rc;
  // the rank-1 steps' statistics from the cross-products S (option xprod): the sweep's weights are
  // the deflated P_0..P_{m-1} w, so S blockdiag(P w, P c) gives exactly the sweep's X'mu_T and Gram
  if ((rc = xprod_begin(c, a * max_steps, 1))) return rc;
  struct XpGuard {
    ppls_ctx* c;
    ~XpGuard() { c->xp_active = false; }
  } xp_guard{c};
  const int p = c->p, q = c->q;
  const double N = (double)c->n_total;
  double ssqX = c->ssq_host[0], ssqY = c->ssq_host[1];   // ||Xc||^2, ||Yc||^2 of the current deflation
  std::vector<double> Wp, Cp;                            // w_1..w_k, c_1..c_k (column-major)
  std::vector<double> gA, gD, gB;                        // ||X w_j||^2, <X w_j, Y c_j>, ||Y c_j||^2
  bool fixed_wc = false;                                 // some component had W or C fixed
  Rank1Dev dev;
  if ((rc = dalloc(c, &dev.Wp, (size_t)p * a)) || (rc = dalloc(c, &dev.Cp, (size_t)q * a)) ||
      (rc = dalloc(c, &dev.tw, (size_t)p)) || (rc = dalloc(c, &dev.tc, (size_t)q)) ||
      (rc = dalloc(c, &dev.consW, (size_t)p)) || (rc = dalloc(c, &dev.consC, (size_t)q)) ||
      (rc = dalloc(c, &dev.lv, (size_t)max_steps + 5)) || (rc = dalloc(c, &dev.st, 1)))
    return rc;
  out->ncomp = 0;
  out->not_monotone = 0;
  c->seq_fits = 0;
  if (out->logvalue)
    for (size_t e = 0; e < (size_t)a * (max_steps + 1); ++e) out->logvalue[e] = NAN;
  for (int k = 0; k < a; ++k) {
    Rank1 t;
    if ((rc = start(k, Wp, Cp, ssqX, ssqY, t))) return rc;
    // PPLSi's constraints (fconstraint, :85-92): fixed values replace the estimates at the start
    // (:141-145) and after every EM step (:165-169)
    const ppls_constraint* ck = cons ? &cons[k] : nullptr;
    auto constrain = [&](Rank1& u) {
      if (!ck) return;
      if (ck->W) u.w.assign(ck->W, ck->W + p);
      if (ck->C) u.c.assign(ck->C, ck->C + q);
      if (ck->B) u.B = ck->B[0];
      if (ck->sigE) u.sigE = ck->sigE[0];
      if (ck->sigF) u.sigF = ck->sigF[0];
      if (ck->sigH) u.sigH = ck->sigH[0];
      if (ck->sigT) u.sigT = ck->sigT[0];
    };
    if (ck && (ck->W || ck->C)) fixed_wc = true;
    constrain(t);
    if (k > 0) {   // deflation vectors w_1..w_k, c_1..c_k on the device
      HIPCHK(c, hipMemcpyAsync(dev.Wp, Wp.data(), sizeof(double) * Wp.size(), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(dev.Cp, Cp.data(), sizeof(double) * Cp.size(), hipMemcpyHostToDevice, c->stream));
    }
    // PPLSi's EM loop (:147-173) on the device; i = the reference's final i (steps made)
    double G[4];
    std::vector<double> lv;
    int i = 0;
    bool na = false;
    if ((rc = rank1_fit_device(c, dev, t, ck, k, ssqX, ssqY, max_steps, atol, crit_abs, Wp, Cp, lv, &i, &na, G)))
      return rc;
    ++c->seq_fits;
    if (na) break;   // PPLS: "residuals are of rank < 1e-14", keep components 1..k-1 (:258-263)
    if (i > max_steps) i = max_steps;
    for (int e = 0; e < p; ++e) out->W[(size_t)k * p + e] = t.w[e];
    for (int e = 0; e < q; ++e) out->C[(size_t)k * q + e] = t.c[e];
    out->B[k] = t.B;
    out->sig[k] = t.sigE;             // cbind(sigX, sigY, sigH, sigT), a x 4
    out->sig[a + k] = t.sigF;
    out->sig[2 * a + k] = t.sigH;
    out->sig[3 * a + k] = t.sigT;
    if (out->logvalue)
      for (int e = 0; e <= i; ++e) out->logvalue[(size_t)k * (max_steps + 1) + e] = lv[e];
    if (out->last_increment) out->last_increment[k] = lv[i] - lv[i - 1];   // :176
    if (out->number_steps) out->number_steps[k] = i;
    for (int e = 1; e <= i; ++e)
      if (lv[e] - lv[e - 1] < 0) out->not_monotone |= 1 << k;              // warning("Not monotone") :177
    // deflation (:270-271): the last sweep used theta_final, so its Gram holds ||Xc_k w_k||^2
    gA.push_back(G[0]);
    gD.push_back(G[1]);
    gB.push_back(G[3]);
    // ||Xc (I - w w')||^2 = ||Xc||^2 - (2 - w'w) ||Xc w||^2 (w'w = 1 unless W is a fixed constraint)
    if (ck && ck->W) {
      double ww = 0.0;
      for (int e = 0; e < p; ++e) ww += t.w[e] * t.w[e];
      ssqX -= (2.0 - ww) * G[0];
    } else {
      ssqX -= G[0];
    }
    if (ck && ck->C) {
      double cc = 0.0;
      for (int e = 0; e < q; ++e) cc += t.c[e] * t.c[e];
      ssqY -= (2.0 - cc) * G[3];
    } else {
      ssqY -= G[3];
    }
    Wp.insert(Wp.end(), t.w.begin(), t.w.end());
    Cp.insert(Cp.end(), t.c.begin(), t.c.end());
    // (streamed data: no rows for the exact residual pass; the running difference stands)
    if (k + 1 < a && ssqX < 1e-6 * c->ssq_host[0] && c->st_state != 2)
      if ((rc = deflated_ssq(c, Wp, k + 1, true, &ssqX))) return rc;
    if (k + 1 < a && ssqY < 1e-6 * c->ssq_host[1] && c->st_state != 2)
      if ((rc = deflated_ssq(c, Cp, k + 1, false, &ssqY))) return rc;
    out->ncomp = k + 1;
    // Other_output$Loglikelihoods[k] = logl_W(X, Y, W[,1:k], C[,1:k], diag(B[1:k]), sigX_k, sigY_k,
    // sigH_k, diag(sigT[1:k])) (:274).  loglC_fast only reads the Gram diagonal, and X w_j = Xc_j w_j
    // because w_j is orthogonal to w_1..w_{j-1}, so the per-component Grams above suffice.
    if (out->loglikelihoods) {
      const int r = k + 1;
      if (fixed_wc) {   // fixed W / C need not be orthogonal: X w_j from undeflated sweeps
        for (int j = 0; j < r; ++j) {
          Rank1 u = t;
          u.w.assign(Wp.begin() + (size_t)j * p, Wp.begin() + (size_t)(j + 1) * p);
          u.c.assign(Cp.begin() + (size_t)j * q, Cp.begin() + (size_t)(j + 1) * q);
          double Gj[4];
          std::vector<double> sx, sy;
          static const std::vector<double> none;
          if ((rc = rank1_sweep(c, u, none, none, 0, sx, sy, Gj))) return rc;
          gA[j] = Gj[0];
          gD[j] = Gj[1];
          gB[j] = Gj[3];
        }
      }
      std::vector<double> Gf((size_t)4 * r * r, 0.0);
      PplsScalars s;
      memset(&s, 0, sizeof s);
      for (int j = 0; j < r; ++j) {
        PPLS_GA(Gf.data(), r, j, j) = gA[j];
        PPLS_GD(Gf.data(), r, j, j) = gD[j];
        PPLS_GB(Gf.data(), r, j, j) = gB[j];
        s.b[j] = out->B[j];
        s.t[j] = out->sig[3 * a + j];
      }
      s.sigE = t.sigE;
      s.sigF = t.sigF;
      s.sigH = t.sigH;
      out->loglikelihoods[k] = ppls_loglik_from_gram(Gf.data(), c->ssq_host[0], c->ssq_host[1], N, p, q, r, &s);
    }
  }
  return PPLS_OK;
}

// ---- 'o2m' starting values from the cross-products (initialGuess = "o2m_xprod") ----

// The largest eigenpair (theta, s) of the symmetric tridiagonal matrix with diagonal al[0..m) and
// off-diagonal be[0..m-1): theta by bisection on the Sturm count, s (unit) by three inverse
// iterations through a row-pivoted tridiagonal elimination (a zero pivot is replaced by eps ||T||).
void tridiag_top(const std::vector<double>& al, const std::vector<double>& be, int m, double* theta,
                 std::vector<double>& s) {
  s.assign((size_t)m, 1.0 / std::sqrt((double)m));
  if (m == 1) {
    *theta = al[0];
    return;
  }
  double lo = al[0], hi = al[0];
  for (int i = 0; i < m; ++i) {
    const double rad = (i > 0 ? std::fabs(be[i - 1]) : 0.0) + (i + 1 < m ? std::fabs(be[i]) : 0.0);
    lo = std::min(lo, al[i] - rad);
    hi = std::max(hi, al[i] + rad);
  }
  const double scale = std::max(std::fabs(lo), std::fabs(hi));
  const double tiny = std::max(scale * 2.220446049250313e-16, 1e-300);
  auto below = [&](double x) {   // eigenvalues < x
    int cnt = 0;
    double qv = 1.0;
    for (int i = 0; i < m; ++i) {
      qv = al[i] - x - (i > 0 ? be[i - 1] * be[i - 1] / qv : 0.0);
      if (qv == 0.0) qv = -tiny;
      if (qv < 0.0) ++cnt;
    }
    return cnt;
  };
  hi += tiny;   // below(hi) == m, below(lo) < m
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (!(mid > lo && mid < hi)) break;
    if (below(mid) == m) hi = mid; else lo = mid;
  }
  const double th = 0.5 * (lo + hi);
  *theta = th;
  std::vector<double> dl((size_t)m), dd((size_t)m), du((size_t)m), du2((size_t)m);
  for (int round = 0; round < 3; ++round) {
    for (int i = 0; i < m; ++i) {
      dd[i] = al[i] - th;
      dl[i] = du[i] = i + 1 < m ? be[i] : 0.0;
      du2[i] = 0.0;
    }
    std::vector<double>& b = s;
    for (int i = 0; i + 1 < m; ++i) {
      if (std::fabs(dd[i]) >= std::fabs(dl[i])) {
        if (dd[i] == 0.0) dd[i] = tiny;
        const double mult = dl[i] / dd[i];
        dd[i + 1] -= mult * du[i];
        b[i + 1] -= mult * b[i];
      } else {   // rows i, i + 1 change places
        const double mult = dd[i] / dl[i];
        dd[i] = dl[i];
        const double tmp = dd[i + 1];
        dd[i + 1] = du[i] - mult * tmp;
        if (i + 2 < m) {
          du2[i] = du[i + 1];
          du[i + 1] = -mult * du2[i];
        }
        du[i] = tmp;
        const double tb = b[i];
        b[i] = b[i + 1];
        b[i + 1] = tb - mult * b[i + 1];
      }
    }
    if (dd[m - 1] == 0.0) dd[m - 1] = tiny;
    b[m - 1] /= dd[m - 1];
    b[m - 2] = (b[m - 2] - du[m - 2] * b[m - 1]) / dd[m - 2];
    for (int i = m - 3; i >= 0; --i) b[i] = (b[i] - du[i] * b[i + 1] - du2[i] * b[i + 2]) / dd[i];
    double big = 0.0;
    for (int i = 0; i < m; ++i) big = std::max(big, std::fabs(b[i]));
    if (!(big > 0.0) || !std::isfinite(big)) {
      s.assign((size_t)m, 1.0 / std::sqrt((double)m));
      return;
    }
    double nn = 0.0;
    for (int i = 0; i < m; ++i) {
      b[i] /= big;
      nn += b[i] * b[i];
    }
    nn = std::sqrt(nn);
    for (int i = 0; i < m; ++i) b[i] /= nn;
  }
}

double hdot(const double* a, const double* b, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += a[i] * b[i];
  return s;
}

// The block of S the passes read and what the loop keeps from component to component.
struct O2mState {
  int side = 0;   // 0: q <= p, A = S[0:p, ldx:ldx+q]; 1: A = S[ldx:ldx+q, 0:p]
  int rows = 0, L = 0;
  int64_t row0 = 0, col0 = 0;
  std::vector<double> AW;   // A'l_j (L each) for the left deflation vectors l_1.. seen so far
  int kdone = 0;
};

void o2m_shape(const ppls_ctx* c, O2mState& st) {
  st.side = c->q <= c->p ? 0 : 1;
  st.rows = st.side ? c->q : c->p;
  st.L = st.side ? c->p : c->q;
  st.row0 = st.side ? c->ldx : 0;
  st.col0 = st.side ? 0 : c->ldx;
}

inline int64_t even_up(int64_t n) { return (n + 1) & ~(int64_t)1; }

int o2m_ensure_buf(ppls_ctx* c, int rows, int L) {
  const int64_t need = 2 * even_up(L) + 2 * even_up(rows) + ppls_o2m_ws_doubles(rows, L, c->num_cus);
  if (c->o2m_buf && c->o2m_buf_len >= need) return PPLS_OK;
  int rc;
  c->o2m_buf_len = 0;
  if ((rc = dalloc(c, &c->o2m_buf, (size_t)need))) return rc;
  c->o2m_buf_len = need;
  return PPLS_OK;
}

// One pass over A (rows x L at (row0, col0) of S, row stride ld) with host vectors: v (L), d (rows, or
// NULL = 0) in; u (rows) and z (L) out, either nullable.
int o2m_pass_host(ppls_ctx* c, const double* S, int64_t ld, const O2mState& st, const double* v, const double* d,
                  double* u, double* z, int* path) {
  int rc;
  if ((rc = o2m_ensure_buf(c, st.rows, st.L))) return rc;
  double* dv = c->o2m_buf;
  double* dd = dv + even_up(st.L);
  double* du = dd + even_up(st.rows);
  double* dz = du + even_up(st.rows);
  double* ws = dz + even_up(st.L);
  HIPCHK(c, hipMemcpyAsync(dv, v, sizeof(double) * st.L, hipMemcpyHostToDevice, c->stream));
  if (d) HIPCHK(c, hipMemcpyAsync(dd, d, sizeof(double) * st.rows, hipMemcpyHostToDevice, c->stream));
  int pth = 0;
  const hipError_t e = ppls_launch_o2m_pass(S, ld, st.row0, st.col0, st.rows, st.L, dv, d ? dd : nullptr, du, dz, ws,
                                            c->num_cus, c->o2m_path, &pth, c->stream);
  if (e == hipErrorInvalidValue)
    return fail(c, PPLS_E_ARG, "o2m pass over %d x %d (o2m_path=%d): the fused path holds rows of at most %d values, "
                "and the block must start at an even column of rows of even length", st.rows, st.L, c->o2m_path,
                PPLS_O2M_FUSED_LMAX);
  HIPCHK(c, e);
  if (u) HIPCHK(c, hipMemcpyAsync(u, du, sizeof(double) * st.rows, hipMemcpyDeviceToHost, c->stream));
  if (z) HIPCHK(c, hipMemcpyAsync(z, dz, sizeof(double) * st.L, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (path) *path = pth;
  return PPLS_OK;
}

// PPLSi's 'o2m' start (:126-131) for the data deflated by the k loadings Wp (p x k), Cp (q x k), from
// the context's S (ready); ssqX, ssqY = ||Xc||^2, ||Yc||^2 of that deflation.
int o2m_start_core(ppls_ctx* c, O2mState& st, const std::vector<double>& Wp, const std::vector<double>& Cp, int k,
                   double ssqX, double ssqY, Rank1& t) {
  int rc;
  const int p = c->p, q = c->q, rows = st.rows, L = st.L;
  const int64_t P = (int64_t)c->ldx + c->ldy;
  const double* S = c->xp_S;
  const std::vector<double>& Lv = st.side ? Cp : Wp;   // deflation of A's rows (rows x k)
  const std::vector<double>& Rv = st.side ? Wp : Cp;   // ... of its columns (L x k)
  int path = 0;
  // A'l_j: one pass with v = 0, d = -l_j (u = l_j, z = A'l_j), kept across components
  {
    std::vector<double> zero((size_t)L, 0.0), neg((size_t)rows);
    for (int j = st.kdone; j < k; ++j) {
      for (int i = 0; i < rows; ++i) neg[i] = -Lv[(size_t)j * rows + i];
      st.AW.resize((size_t)(j + 1) * L);
      if ((rc = o2m_pass_host(c, S, P, st, zero.data(), neg.data(), nullptr, st.AW.data() + (size_t)j * L, &path)))
        return rc;
    }
    st.kdone = k;
  }
  // P_k .. P_1 = I - Lv T Lv' (T lower triangular: row j = -(l_j'Lv_{<j}) T_{<j}, T_jj = 1), so
  // (P_k .. P_1)'(P_k .. P_1) = I - Lv T' Lv' with T' = T + T' - T'(Lv'Lv)T
  std::vector<double> Tp((size_t)k * k, 0.0);
  if (k > 0) {
    std::vector<double> G((size_t)k * k), T((size_t)k * k, 0.0), GT((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) G[(size_t)i * k + j] = hdot(&Lv[(size_t)i * rows], &Lv[(size_t)j * rows], rows);
    for (int j = 0; j < k; ++j) {
      T[(size_t)j * k + j] = 1.0;
      for (int e = 0; e < j; ++e) {
        double sacc = 0.0;
        for (int i = e; i < j; ++i) sacc += G[(size_t)j * k + i] * T[(size_t)i * k + e];
        T[(size_t)j * k + e] = -sacc;
      }
    }
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) {
        double sacc = 0.0;
        for (int e = 0; e < k; ++e) sacc += G[(size_t)i * k + e] * T[(size_t)e * k + j];
        GT[(size_t)i * k + j] = sacc;
      }
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) {
        double sacc = 0.0;
        for (int e = 0; e < k; ++e) sacc += T[(size_t)e * k + i] * GT[(size_t)e * k + j];
        Tp[(size_t)i * k + j] = T[(size_t)i * k + j] + T[(size_t)j * k + i] - sacc;
      }
  }
  std::vector<double> vp((size_t)L), dvec((size_t)rows), h((size_t)std::max(k, 1)), g((size_t)std::max(k, 1));
  // v' = Q_1 .. Q_k y and d = Lv T' (A'Lv)' v'
  auto stage = [&](const double* y) {
    std::copy(y, y + L, vp.begin());
    deflate(Rv, k, L, vp.data(), false);
    if (k == 0) return;
    for (int j = 0; j < k; ++j) h[j] = hdot(&st.AW[(size_t)j * L], vp.data(), L);
    for (int i = 0; i < k; ++i) {
      g[i] = 0.0;
      for (int j = 0; j < k; ++j) g[i] += Tp[(size_t)i * k + j] * h[j];
    }
    std::fill(dvec.begin(), dvec.end(), 0.0);
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < rows; ++i) dvec[i] += g[j] * Lv[(size_t)j * rows + i];
  };
  // out = M'M y, one pass
  auto apply = [&](const double* y, double* out) {
    stage(y);
    int r2 = o2m_pass_host(c, S, P, st, vp.data(), k ? dvec.data() : nullptr, nullptr, out, &path);
    if (r2) return r2;
    deflate(Rv, k, L, out, true);
    return (int)PPLS_OK;
  };
  // symmetric Lanczos with full reorthogonalisation (twice) against the kept basis
  constexpr int CAP = 200;
  std::vector<std::vector<double>> Q;
  Q.emplace_back((size_t)L, 1.0 / std::sqrt((double)L));
  std::vector<double> al, be, s, r((size_t)L);
  double theta = 0.0, est = 0.0;
  int passes = 0;
  for (int m = 1;; ++m) {
    if ((rc = apply(Q[(size_t)m - 1].data(), r.data()))) return rc;
    ++passes;
    const double alpha = hdot(Q[(size_t)m - 1].data(), r.data(), L);
    al.push_back(alpha);
    for (int i = 0; i < L; ++i) r[i] -= alpha * Q[(size_t)m - 1][i];
    if (m > 1)
      for (int i = 0; i < L; ++i) r[i] -= be[(size_t)m - 2] * Q[(size_t)m - 2][i];
    for (int twice = 0; twice < 2; ++twice)
      for (int j = 0; j < m; ++j) {
        const double dj = hdot(Q[(size_t)j].data(), r.data(), L);
        for (int i = 0; i < L; ++i) r[i] -= dj * Q[(size_t)j][i];
      }
    const double beta = std::sqrt(hdot(r.data(), r.data(), L));
    tridiag_top(al, be, m, &theta, s);
    est = std::fabs(beta * s[(size_t)m - 1]);
    if (!std::isfinite(theta) || !std::isfinite(beta))
      return fail(c, PPLS_E_NUMERIC, "o2m start: the cross block of S is not finite (theta = %g after %d passes)", theta,
                  passes);
    if (est <= std::ldexp(theta, -43) || m == L) break;
    if (m == CAP) {
      if (est <= std::ldexp(theta, -26)) break;   // a starting value: accepted
      return fail(c, PPLS_E_NUMERIC, "o2m start: no first singular pair after %d passes (residual estimate %g, theta %g)",
                  CAP, est, theta);
    }
    be.push_back(beta);
    Q.emplace_back((size_t)L);
    for (int i = 0; i < L; ++i) Q.back()[i] = r[i] / beta;
  }
  c->o2m_last[0] = st.side;
  c->o2m_last[1] = path;
  c->o2m_last[2] = passes;
  c->o2m_last_d[0] = est;
  c->o2m_last_d[1] = theta;
  // sigma_1 within rounding of ||X|| ||Y||: nothing of X'Y is left
  if (!(theta > std::ldexp(c->ssq_host[0], -52) * std::ldexp(c->ssq_host[1], -52)))
    return fail(c, PPLS_E_NUMERIC, "o2m start: the deflated X'Y vanishes (its largest squared singular value is %g "
                "against ssq(X) ssq(Y) = %g): no first singular pair to start from", theta,
                c->ssq_host[0] * c->ssq_host[1]);
  const int m = (int)al.size();
  std::vector<double> y((size_t)L, 0.0), x((size_t)rows);
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < L; ++i) y[i] += s[(size_t)j] * Q[(size_t)j][i];
  const double ny = std::sqrt(hdot(y.data(), y.data(), L));
  for (int i = 0; i < L; ++i) y[i] /= ny;
  // the other side: x = M y / ||M y||, M y = P_k .. P_1 A Q_1 .. Q_k y (one more pass, d = 0)
  stage(y.data());
  if ((rc = o2m_pass_host(c, S, P, st, vp.data(), nullptr, x.data(), nullptr, &path))) return rc;
  deflate(Lv, k, rows, x.data(), true);
  const double nx = std::sqrt(hdot(x.data(), x.data(), rows));
  if (!(nx > 0.0)) return fail(c, PPLS_E_NUMERIC, "o2m start: the deflated X'Y vanishes on its first right singular vector");
  for (int i = 0; i < rows; ++i) x[i] /= nx;
  t.w = st.side ? y : x;
  t.c = st.side ? x : y;
  // sign: W's entry of largest magnitude (lowest index on a tie) is positive, C follows
  int big = 0;
  for (int i = 1; i < p; ++i)
    if (std::fabs(t.w[(size_t)i]) > std::fabs(t.w[(size_t)big])) big = i;
  if (t.w[(size_t)big] < 0.0) {
    for (double& e : t.w) e = -e;
    for (double& e : t.c) e = -e;
  }
  // ssq(Tt), Tt'U, ssq(U) for Tt = Xc W., U = Yc C.: one rank-1 statistics step from S
  t.B = t.sigE = t.sigF = t.sigH = t.sigT = 1.0;
  double G[4];
  std::vector<double> SX, SY;
  const bool was = c->xp_active;
  c->xp_active = true;
  rc = rank1_sweep(c, t, Wp, Cp, k, SX, SY, G);
  c->xp_active = was;
  if (rc) return rc;
  const double N = (double)c->n_total, sst = G[0], tu = G[1], ssu = G[3];
  t.B = tu / sst;
  t.sigE = std::sqrt((ssqX - sst) / N / p);
  t.sigF = std::sqrt((ssqY - ssu) / N / q);
  t.sigH = std::sqrt((ssu - t.B * t.B * sst) / N);
  t.sigT = std::sqrt(sst / N);
  return PPLS_OK;
}

// The checks and the S every 'o2m_xprod' entry needs: data, no open stream, S formed (and kept, as
// after ppls_xprod_prepare) where the context holds rows only.
int o2m_ready(ppls_ctx* c) {
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (c->st_state == 1) return fail(c, PPLS_E_STATE, "a stream is open: call ppls_stream_end first");
  int rc;
  if (!c->xp_ready || !c->xp_S) {
    if ((rc = xprod_setup(c))) return rc;
    c->xp_explicit = true;
  }
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_o2m_start(ppls_ctx* c, const double* Wprev, const double* Cprev, int k, ppls_theta* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (c->st_state == 1) return fail(c, PPLS_E_STATE, "a stream is open: call ppls_stream_end first");
  if (!out || !out->W || !out->C || !out->B || !out->sigT) return fail(c, PPLS_E_ARG, "NULL argument");
  if (k < 0 || k > PPLS_RMAX - 1) return fail(c, PPLS_E_ARG, "k=%d earlier components outside [0,%d]", k, PPLS_RMAX - 1);
  if (k > 0 && (!Wprev || !Cprev)) return fail(c, PPLS_E_ARG, "NULL argument");
  int rc;
  if ((rc = check_fit_data(c))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, 1, 1))) return rc;
  if ((rc = o2m_ready(c))) return rc;
  const int p = c->p, q = c->q;
  std::vector<double> Wp, Cp;
  if (k > 0) {
    Wp.assign(Wprev, Wprev + (size_t)p * k);
    Cp.assign(Cprev, Cprev + (size_t)q * k);
  }
  // ||X P_1 .. P_k||^2 as the sequential loop runs it: ||A (I - w w')||^2 = ||A||^2 - (2 - w'w) ||A w||^2
  double ssqX = c->ssq_host[0], ssqY = c->ssq_host[1];
  c->xp_active = true;
  for (int j = 0; j < k && !rc; ++j) {
    Rank1 u;
    u.w.assign(Wp.begin() + (size_t)j * p, Wp.begin() + (size_t)(j + 1) * p);
    u.c.assign(Cp.begin() + (size_t)j * q, Cp.begin() + (size_t)(j + 1) * q);
    u.B = u.sigE = u.sigF = u.sigH = u.sigT = 1.0;
    double G[4];
    std::vector<double> SX, SY;
    if ((rc = rank1_sweep(c, u, Wp, Cp, j, SX, SY, G))) break;
    ssqX -= (2.0 - hdot(u.w.data(), u.w.data(), p)) * G[0];
    ssqY -= (2.0 - hdot(u.c.data(), u.c.data(), q)) * G[3];
  }
  O2mState st;
  o2m_shape(c, st);
  Rank1 t;
  if (!rc) rc = o2m_start_core(c, st, Wp, Cp, k, ssqX, ssqY, t);
  c->xp_active = false;
  if (rc) return rc;
  std::copy(t.w.begin(), t.w.end(), out->W);
  std::copy(t.c.begin(), t.c.end(), out->C);
  out->B[0] = t.B;
  out->sigT[0] = t.sigT;
  out->sigE = t.sigE;
  out->sigF = t.sigF;
  out->sigH = t.sigH;
  return PPLS_OK;
}

int ppls_ppls_o2m(ppls_ctx* c, int a, int max_steps, double atol, int crit_abs, const ppls_constraint* cons,
                  ppls_seq_fit* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (c->st_state == 1) return fail(c, PPLS_E_STATE, "a stream is open: call ppls_stream_end first");
  O2mState st;
  c->o2m_last[3] = c->seq_fits = 0;
  const int rc = seq_fit(c, a, max_steps, atol, crit_abs, cons, out,
                         [&](int k, const std::vector<double>& Wp, const std::vector<double>& Cp, double ssqX, double ssqY,
                             Rank1& t) {
                           if (k < 0) return (int)PPLS_OK;
                           int r2;
                           if (k == 0) {
                             if ((r2 = o2m_ready(c))) return r2;
                             o2m_shape(c, st);
                           }
                           return o2m_start_core(c, st, Wp, Cp, k, ssqX, ssqY, t);
                         });
  c->o2m_last[3] = c->seq_fits;   // counted by the loop after each rank1_fit_device, not by the starts
  return rc;
}

int ppls_o2m_pass(ppls_ctx* c, const double* S, int P, int ld, int row0, int col0, int rows, int L, const double* v,
                  const double* d, double* u, double* z, int* path) {
  if (!c) return PPLS_E_ARG;
  if (!S || !v || !u || !z) return fail(c, PPLS_E_ARG, "NULL argument");
  if (P < 1 || ld < 1 || rows < 1 || L < 1 || row0 < 0 || col0 < 0 || (int64_t)row0 + rows > P ||
      (int64_t)col0 + even_up(L) > ld || (ld & 1) || (col0 & 1))
    return fail(c, PPLS_E_ARG, "o2m pass: block %d x %d at (%d, %d) does not lie in %d rows of %d (even column start "
                "and row length; L is rounded up to 2)", rows, L, row0, col0, P, ld);
  HIPCHK(c, hipSetDevice(c->device));
  double* Sd = nullptr;
  int rc;
  if ((rc = dalloc(c, &Sd, (size_t)P * ld))) return rc;
  O2mState st;
  st.rows = rows;
  st.L = L;
  st.row0 = row0;
  st.col0 = col0;
  hipError_t e = hipMemcpy(Sd, S, sizeof(double) * (size_t)P * ld, hipMemcpyHostToDevice);
  if (e != hipSuccess) rc = fail(c, PPLS_E_HIP, "o2m pass upload: %s", hipGetErrorString(e));
  if (!rc) rc = o2m_pass_host(c, Sd, ld, st, v, d, u, z, path);
  (void)hipStreamSynchronize(c->stream);
  dfree(Sd);
  return rc;
}

int ppls_o2m_info(ppls_ctx* c, int* side, int* path, int* passes, double* resid, double* theta, int* fits) {
  if (!c) return PPLS_E_ARG;
  if (side) *side = c->o2m_last[0];
  if (path) *path = c->o2m_last[1];
  if (passes) *passes = c->o2m_last[2];
  if (fits) *fits = c->o2m_last[3];
  if (resid) *resid = c->o2m_last_d[0];
  if (theta) *theta = c->o2m_last_d[1];
  return PPLS_OK;
}

int ppls_o2m_pass_timing(ppls_ctx* c, int reps, double* ms, double* bytes, int* path) {
  if (!c || reps < 1 || !ms) return PPLS_E_ARG;
  if (!c->have_data || !c->xp_ready || !c->xp_S) return fail(c, PPLS_E_STATE, "the cross-products S are not formed");
  HIPCHK(c, hipSetDevice(c->device));
  O2mState st;
  o2m_shape(c, st);
  int rc;
  const int64_t P = (int64_t)c->ldx + c->ldy;
  std::vector<double> v((size_t)st.L, 1.0 / std::sqrt((double)st.L)), d((size_t)st.rows, 0.0);
  int pth = 0;
  if ((rc = o2m_pass_host(c, c->xp_S, P, st, v.data(), d.data(), nullptr, nullptr, &pth))) return rc;   // untimed
  double* dv = c->o2m_buf;
  double* dd = dv + even_up(st.L);
  double* du = dd + even_up(st.rows);
  double* dz = du + even_up(st.rows);
  double* ws = dz + even_up(st.L);
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0));
  HIPCHK(c, hipEventCreate(&e1));
  hipError_t e = hipEventRecord(e0, c->stream);
  for (int i = 0; e == hipSuccess && i < reps; ++i)
    e = ppls_launch_o2m_pass(c->xp_S, P, st.row0, st.col0, st.rows, st.L, dv, dd, du, dz, ws, c->num_cus, c->o2m_path,
                             nullptr, c->stream);
  if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float tms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&tms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIPCHK(c, e);
  *ms = (double)tms / reps;
  if (bytes) *bytes = 8.0 * st.rows * st.L;
  if (path) *path = pth;
  return PPLS_OK;
}

}  // extern "C"

namespace {

// Sums of squares of the rows [row0, row0 + nrows) of X and Y on this rank, all-reduced -> out[2].
int segment_ssq(ppls_ctx* c, int64_t row0, int64_t nrows, double out[2]) {
  int rc;
  const int nb = 1024;
  double* buf = nullptr;
  if ((rc = dalloc(c, &buf, (size_t)nb + 2))) return rc;
  hipError_t e = hipMemsetAsync(buf + nb, 0, 2 * sizeof(double), c->stream);
  for (int m = 0; m < 2 && e == hipSuccess && nrows > 0; ++m) {
    const int64_t ld = m ? c->ldy : c->ldx;
    const void* base = m ? (const void*)c->Y : (const void*)c->X;
    if (c->dtype)
      e = ppls_launch_sumsq_f32((const float*)base + row0 * ld, nrows * ld, buf, nb, buf + nb + m, c->stream);
    else
      e = ppls_launch_sumsq((const double*)base + row0 * ld, nrows * ld, buf, nb, buf + nb + m, 0, c->stream);
  }
  rc = e == hipSuccess ? allreduce(c, buf + nb, 2) : fail(c, PPLS_E_HIP, "segment ssq: %s", hipGetErrorString(e));
  if (!rc) {
    e = hipMemcpyAsync(out, buf + nb, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, PPLS_E_HIP, "segment ssq: %s", hipGetErrorString(e));
  }
  dfree(buf);
  return rc;
}

// rank1_sweep restricted to this rank's rows of one population.
int segment_sweep(ppls_ctx* c, int64_t row0, int64_t nrows, const Rank1& t, std::vector<double>& SX,
                  std::vector<double>& SY, double G[4]) {
  static const std::vector<double> none;
  c->seg_row0 = row0;
  c->seg_rows = nrows;
  const int rc = rank1_sweep(c, t, none, none, 0, SX, SY, G);
  c->seg_row0 = 0;
  c->seg_rows = -1;
  return rc;
}

struct MetaPop {
  int64_t row0 = 0, nloc = 0;   // this rank's rows of the population
  double N = 0.0;               // rows over all ranks (nrow(X[popui, ]))
  double ssq[2] = {0.0, 0.0};   // ssq(X[popui, ]), ssq(Y[popui, ])
  Rank1 t;                      // params[[j]] with the shared W., C.
  std::vector<double> SX, SY;   // X[popui, ]' mu_T, Y[popui, ]' mu_U of the last sweep
  double G[4] = {0, 0, 0, 0};
};

int meta_setup(ppls_ctx* c, int npop, const int64_t* pop_local, const int64_t* pop_total,
               std::vector<MetaPop>& pops) {
  if (npop < 1 || !pop_local || !pop_total) return fail(c, PPLS_E_ARG, "need npop >= 1 populations with row counts");
  pops.assign(npop, MetaPop());
  int64_t r0 = 0, tot = 0;
  for (int j = 0; j < npop; ++j) {
    if (pop_local[j] < 0 || pop_total[j] < 1) return fail(c, PPLS_E_ARG, "population %d has no rows", j + 1);
    pops[j].row0 = r0;
    pops[j].nloc = pop_local[j];
    pops[j].N = (double)pop_total[j];
    r0 += pop_local[j];
    tot += pop_total[j];
  }
  if (r0 != c->n_local) return fail(c, PPLS_E_ARG, "population rows on this rank sum to %lld, not n_local = %lld",
                                    (long long)r0, (long long)c->n_local);
  if (tot != c->n_total)   // stopifnot(nrow(X) == length(Ipopu)) (:448, :511)
    return fail(c, PPLS_E_ARG, "population sizes sum to %lld, not nrow(X) = %lld", (long long)tot,
                (long long)c->n_total);
  int rc;
  for (auto& pp : pops)
    if ((rc = segment_ssq(c, pp.row0, pp.nloc, pp.ssq))) return rc;
  return PPLS_OK;
}

// The M-step half of meta_EMstep (:453-484) from each population's last sweep: meta_Mstep per
// population, then W. = orth(sum_j sign(<Cxt_1, Cxt_j>) Cxt_j), C. likewise with Cyu_j.  orth of one
// column is v / ||v|| (OmicsPLS::orth semantics of Package/functions.R:252-260; unpinned).
void meta_mstep(std::vector<MetaPop>& pops, int p, int q, std::vector<double>& w, std::vector<double>& cv,
                std::vector<double>* Cxt, std::vector<double>* Cyu) {
  const int npop = (int)pops.size();
  std::vector<Rank1> nt(npop);
  for (int j = 0; j < npop; ++j) rank1_scalars(pops[j].t, pops[j].G, pops[j].ssq[0], pops[j].ssq[1], pops[j].N, p, q, &nt[j]);
  w.assign(p, 0.0);
  cv.assign(q, 0.0);
  if (Cxt) Cxt->assign((size_t)p * npop, 0.0);
  if (Cyu) Cyu->assign((size_t)q * npop, 0.0);
  const std::vector<double>& x1 = pops[0].SX;
  const double N1 = pops[0].N;
  for (int j = 0; j < npop; ++j) {
    const MetaPop& pp = pops[j];
    double d = 0.0;   // crossprod(Cxt_1, Cxt_j) = <SX_1, SX_j> / (N_1 N_j)
    for (int i = 0; i < p; ++i) d += (x1[i] / N1) * (pp.SX[i] / pp.N);
    const double sg = d > 0 ? 1.0 : (d < 0 ? -1.0 : 0.0);   // R's sign()
    for (int i = 0; i < p; ++i) w[i] += sg * (pp.SX[i] / pp.N);     // Cxt = X' mu_T / N (loglC.cpp:416)
    for (int i = 0; i < q; ++i) cv[i] += sg * (pp.SY[i] / pp.N);    // Cyu (:421)
    if (Cxt) for (int i = 0; i < p; ++i) (*Cxt)[(size_t)j * p + i] = pp.SX[i] / pp.N;
    if (Cyu) for (int i = 0; i < q; ++i) (*Cyu)[(size_t)j * q + i] = pp.SY[i] / pp.N;
  }
  double nw = 0.0, nc = 0.0;
  for (double v : w) nw += v * v;
  for (double v : cv) nc += v * v;
  nw = std::sqrt(nw);
  nc = std::sqrt(nc);
  for (double& v : w) v /= nw;
  for (double& v : cv) v /= nc;
  for (int j = 0; j < npop; ++j) {
    pops[j].t.B = nt[j].B;
    pops[j].t.sigE = nt[j].sigE;
    pops[j].t.sigF = nt[j].sigF;
    pops[j].t.sigH = nt[j].sigH;
    pops[j].t.sigT = nt[j].sigT;
  }
}

void meta_params_out(const std::vector<MetaPop>& pops, double* params) {
  const int npop = (int)pops.size();
  for (int j = 0; j < npop; ++j) rank1_to_params(pops[j].t, params, npop, j);
}

// The populations' rows (K) and sums of squares (2K: ssq(X_j), ssq(Y_j)) as meta_dev_begin takes them.
void meta_pack_counts(const std::vector<MetaPop>& pops, std::vector<double>& hN, std::vector<double>& hs) {
  const size_t K = pops.size();
  hN.resize(K);
  hs.resize(2 * K);
  for (size_t j = 0; j < K; ++j) {
    hN[j] = pops[j].N;
    hs[2 * j] = pops[j].ssq[0];
    hs[2 * j + 1] = pops[j].ssq[1];
  }
}

// What a fit's start shares: every log-likelihood slot NaN until its step is reached.
void meta_log_clear(ppls_meta_fit* out, int max_steps, int npop) {
  if (!out->log) return;
  for (size_t e = 0; e < ((size_t)max_steps + 1) * npop; ++e) out->log[e] = NAN;
}

int meta_sweep_all(ppls_ctx* c, std::vector<MetaPop>& pops, const std::vector<double>& w,
                   const std::vector<double>& cv) {
  int rc;
  for (auto& pp : pops) {
    pp.t.w = w;
    pp.t.c = cv;
    if ((rc = segment_sweep(c, pp.row0, pp.nloc, pp.t, pp.SX, pp.SY, pp.G))) return rc;
  }
  return PPLS_OK;
}

// meta_PPLSi on the device (ppls_meta_step_kernel) for every storage and shape: one segmented
// sweep per EM step -- the split sweep (fp64, p and q within its register budget) or, round 6, the
// panel sweep (fp32 storage, wide p).  Option meta_device = 0 keeps the per-population host loop.
bool meta_device_ok(const ppls_ctx* c, int npop) {
  return c->meta_device && npop >= 1 && npop <= PPLS_META_KMAX;
}

// What every device loop of meta_PPLSi keeps on the device, whatever its statistics come from: the K
// statistics blocks, the populations' rows and sums of squares, their scalars, the log-likelihoods.
struct MetaDev {
  double* stats = nullptr;
  double* N = nullptr;
  double* ssq = nullptr;
  double* log = nullptr;
  PplsRank1* st = nullptr;
  PplsScalars* sc = nullptr;
  ppls_ctx* c = nullptr;
  std::vector<hipEvent_t> evs;
  ~MetaDev() {
    dfree(stats); dfree(N); dfree(ssq); dfree(log); dfree(st); dfree(sc);
    if (c) c->sweep_stop = nullptr;
    for (auto e : evs) (void)hipEventDestroy(e);
  }
};

// Allocate and stage a fit that starts every population from t0: N (K), ssq (2K: ssq(X_j), ssq(Y_j)),
// the shared loadings into W[0], C[0].  The stop flag must be reset before.
int meta_dev_begin(ppls_ctx* c, MetaDev& d, int K, const double* N, const double* ssq, const Rank1& t0, int max_steps) {
  int rc;
  d.c = c;
  const int64_t pld = c->part_ld, lld = (int64_t)max_steps + 1;
  if ((rc = dalloc(c, &d.stats, (size_t)K * pld)) || (rc = dalloc(c, &d.N, (size_t)K)) ||
      (rc = dalloc(c, &d.ssq, (size_t)2 * K)) || (rc = dalloc(c, &d.log, (size_t)K * lld)) ||
      (rc = dalloc(c, &d.st, (size_t)K)) || (rc = dalloc(c, &d.sc, (size_t)K)))
    return rc;
  std::vector<double> hl((size_t)K * lld, NAN);
  std::vector<PplsRank1> hst((size_t)K, r1_of(t0));
  std::vector<PplsScalars> hsc((size_t)K);
  for (int j = 0; j < K; ++j) ppls_rank1_sweep_scalars(&hst[(size_t)j], &hsc[(size_t)j]);
  std::vector<double> wv((size_t)c->ldx, 0.0), cv((size_t)c->ldy, 0.0);
  std::copy(t0.w.begin(), t0.w.end(), wv.begin());
  std::copy(t0.c.begin(), t0.c.end(), cv.begin());
  HIPCHK(c, hipMemcpyAsync(d.N, N, sizeof(double) * K, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.ssq, ssq, sizeof(double) * 2 * K, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.log, hl.data(), sizeof(double) * hl.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.st, hst.data(), sizeof(PplsRank1) * K, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.sc, hsc.data(), sizeof(PplsScalars) * K, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->W[0], wv.data(), sizeof(double) * wv.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->C[0], cv.data(), sizeof(double) * cv.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host vectors go out of scope
  return PPLS_OK;
}

// The loop itself (EM_W_multi.R:551-578): per EM step stats_pass() leaves the K statistics blocks of
// the current parameters in d.stats (all-reduced where that is needed), then ppls_meta_step_kernel.
// No host round trip per step: the host enqueues at most LOOKAHEAD steps ahead and stops launching
// once the step kernel reports the end of the fit (all ranks at the same step).  ssqX, ssqY, Ntot:
// the whole data's, for logvalue[1, ].
template <class Pass>
int meta_dev_loop(ppls_ctx* c, MetaDev& d, int K, int max_steps, double atol, int crit_abs, double ssqX, double ssqY,
                  double Ntot, Pass&& stats_pass, ppls_meta_fit* out) {
  const int p = c->p, q = c->q;
  const int64_t pld = c->part_ld, lld = (int64_t)max_steps + 1;
  int rc;
  c->sweep_stop = c->stop_d;
  PplsMetaStepArgs m;
  memset(&m, 0, sizeof m);
  m.stats = d.stats; m.part_ld = pld; m.K = K; m.p = p; m.q = q; m.ldx = c->ldx; m.ldy = c->ldy;
  m.N = d.N; m.ssq = d.ssq; m.st = d.st; m.sc = d.sc; m.W = c->W[0]; m.C = c->C[0];
  m.log = d.log; m.log_ld = lld; m.max_steps = max_steps; m.crit_abs = crit_abs; m.atol = atol;
  m.stop = c->stop_d; m.stop_mirror = c->stop_mirror_dev;
  m.ssqX = ssqX; m.ssqY = ssqY; m.Ntot = Ntot;
  constexpr int LOOKAHEAD = 8;
  for (int step = 0; step <= max_steps; ++step) {
    if (step >= LOOKAHEAD) {
      HIPCHK(c, hipEventSynchronize(d.evs[(size_t)(step - LOOKAHEAD) % LOOKAHEAD]));
      const int ended = __atomic_load_n(c->stop_mirror, __ATOMIC_ACQUIRE);
      if (ended != 0 && ended <= step - LOOKAHEAD) break;   // the same break step on every rank
    }
    if ((rc = stats_pass())) return rc;
    m.step = step;
    HIPCHK(c, ppls_launch_meta_step(&m, c->stream));
    const size_t k = (size_t)step % LOOKAHEAD;
    if (d.evs.size() <= k) {
      hipEvent_t e;
      HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      d.evs.push_back(e);
    }
    HIPCHK(c, hipEventRecord(d.evs[k], c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int stop[2] = {0, 0};
  HIPCHK(c, hipMemcpy(stop, c->stop_d, sizeof stop, hipMemcpyDeviceToHost));
  if (stop[1] == 2)
    return fail(c, PPLS_E_NUMERIC, "meta_PPLSi: the log-likelihood increment of EM step %d is NaN", stop[0]);
  out->steps = stop[0] > 0 ? stop[0] : max_steps;
  std::vector<double> hl((size_t)K * lld), hw((size_t)c->ldx), hc((size_t)c->ldy);
  std::vector<PplsRank1> hst((size_t)K);
  HIPCHK(c, hipMemcpy(hl.data(), d.log, sizeof(double) * hl.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hw.data(), c->W[0], sizeof(double) * hw.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hc.data(), c->C[0], sizeof(double) * hc.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(hst.data(), d.st, sizeof(PplsRank1) * K, hipMemcpyDeviceToHost));
  if (out->log) std::copy(hl.begin(), hl.end(), out->log);
  std::copy(hw.begin(), hw.begin() + p, out->W);
  std::copy(hc.begin(), hc.begin() + q, out->C);
  for (int j = 0; j < K; ++j) rank1_to_params(hst[(size_t)j], out->params, K, j);
  return PPLS_OK;
}

// The whole meta_PPLSi loop (EM_W_multi.R:544-578) on the device.  Per EM step the statistics of
// every population from ONE segmented sweep over X and Y -- the split sweep: workgroups partitioned
// over the populations in proportion to their rows (each workgroup's rows in one population, using
// that population's scalars); the panel sweep (fp32 storage, wide p): the dots give every row its
// population's mu, and the accumulation's row chunks are partitioned like those workgroups -- then per
// population a reduction of its workgroups' partials, one all-reduce of the K statistics blocks when
// sharded, and ppls_meta_step_kernel (log-likelihoods, stop rule, M-step, the next sweep's loadings
// and scalars).  No host round trip per step: the host enqueues at most LOOKAHEAD steps ahead and
// stops launching once the step kernel reports the end of the fit (all ranks at the same step).
// logvalue[1, ] comes from the first sweep (theta0 is every population's, so the full-data Gram is
// the sum of theirs): no separate full-data sweep.
int meta_ppls_device(ppls_ctx* c, const std::vector<MetaPop>& pops, const Rank1& t0, int max_steps, double atol,
                     int crit_abs, ppls_meta_fit* out) {
  const int K = (int)pops.size();
  int rc;
  PplsSweepArgs a;
  const int plan = sweep_plan(c, 1, &a);
  if (plan != 3 && plan != 4) return fail(c, PPLS_E_STATE, "meta device path: no sweep for this shape");
  const bool panel = plan == 4;
  c->meta_path = panel ? 3 : 2;
  // workgroups per population: proportional to its local rows, at least one if it has any.  A rank
  // with no local rows (nz = 0) gets no workgroups: it launches no sweep, zeroes its K statistics
  // blocks and still joins every all-reduce (the remainder loop below never ended there).
  // Panel: the same partition of the accumulation's row chunks (a.grid: the chunk policy of a sweep of
  // every local row), so each chunk lies in one population.
  int nz = 0;
  for (const auto& pp : pops) nz += pp.nloc > 0 ? 1 : 0;
  std::vector<int> gk((size_t)K, 0);
  int G = 0;
  if (nz > 0) {
    G = std::max(a.grid, nz);
    int left = G;
    for (int j = 0; j < K; ++j) gk[(size_t)j] = pops[j].nloc > 0 ? 1 : 0;
    left -= nz;
    const double nrows = (double)std::max<int64_t>(c->n_local, 1);
    for (int j = 0; j < K && left > 0; ++j) {
      if (pops[j].nloc <= 0) continue;
      const int extra = std::min(left, (int)std::floor((double)(G - nz) * (double)pops[j].nloc / nrows));
      gk[(size_t)j] += extra;
      left -= extra;
    }
    for (int j = 0; left > 0; j = (j + 1) % K)   // the rounding remainder, one at a time (nz > 0: ends)
      if (pops[j].nloc > 0) { ++gk[(size_t)j]; --left; }
  }
  std::vector<int64_t> bnd((size_t)G + 1);
  std::vector<int> seg((size_t)G), g0((size_t)K + 1, 0);
  {
    int g = 0;
    for (int j = 0; j < K; ++j) {
      g0[(size_t)j] = g;
      for (int u = 0; u < gk[(size_t)j]; ++u, ++g) {
        bnd[(size_t)g] = pops[j].row0 + pops[j].nloc * u / gk[(size_t)j];
        seg[(size_t)g] = j;
      }
    }
    g0[(size_t)K] = g;
    bnd[(size_t)G] = c->n_local;
  }
  if ((rc = ensure_part(c, std::max(G, 1)))) return rc;
  if (panel && c->z_cols < 4) {   // Z = [Xw | Yc | mu_T | mu_U] rows + the transposed W, C
    dfree(c->Z);
    c->z_cols = 0;
    if ((rc = dalloc(c, &c->Z, (size_t)ppls_panel_z_len(c->n_local, c->ldx, c->ldy, 1)))) return rc;
    c->z_cols = 4;
  }
  if ((rc = ensure_stop(c)) || (rc = reset_stop(c))) return rc;
  struct Seg {   // the segmented sweep's own device state
    int64_t* bnd = nullptr;
    int64_t* segend = nullptr;
    int* seg = nullptr;
    ~Seg() { dfree(bnd); dfree(segend); dfree(seg); }
  } sg;
  MetaDev d;   // (destroyed before sg: nothing of sg is read once the loop has synchronised)
  const int64_t pld = c->part_ld;
  if ((rc = dalloc(c, &sg.bnd, (size_t)G + 1)) || (rc = dalloc(c, &sg.seg, (size_t)std::max(G, 1))) ||
      (rc = dalloc(c, &sg.segend, (size_t)K)))
    return rc;
  {
    std::vector<int64_t> se((size_t)K);
    for (int j = 0; j < K; ++j) se[(size_t)j] = pops[j].row0 + pops[j].nloc;
    HIPCHK(c, hipMemcpyAsync(sg.bnd, bnd.data(), sizeof(int64_t) * bnd.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(sg.seg, seg.data(), sizeof(int) * seg.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(sg.segend, se.data(), sizeof(int64_t) * K, hipMemcpyHostToDevice, c->stream));
    std::vector<double> hN, hs;
    meta_pack_counts(pops, hN, hs);
    if ((rc = meta_dev_begin(c, d, K, hN.data(), hs.data(), t0, max_steps))) return rc;   // (synchronises)
  }
  a.X = c->X;
  a.Y = c->Y;
  a.n_local = c->n_local;
  a.Wp = c->W[0];
  a.Cp = c->C[0];
  a.sc = d.sc;
  a.part = c->part;
  a.part_ld = pld;
  a.mu = nullptr;
  a.write_mu = 0;
  a.grid = G;
  a.row_bounds = sg.bnd;
  a.wg_seg = sg.seg;
  a.nt = (c->nt_loads > 0 || (c->nt_loads < 0 && 8.0 * c->n_local * (double)(c->ldx + c->ldy) > 256.0 * (1 << 20))) ? 1 : 0;
  a.stop = c->stop_d;
  a.trace = nullptr;
  c->sweep_stop = c->stop_d;
  double* tmp = c->part + (size_t)c->part_groups * pld;
  // one segmented sweep of the current parameters -> d.stats (K blocks, all-reduced)
  if (panel) {   // the dots use each row's population scalars; the accumulation's chunks are bnd
    a.row_bounds = nullptr;
    a.wg_seg = nullptr;
    a.seg_ends = sg.segend;
    a.nseg = K;
    a.chunk_bounds = sg.bnd;
  }
  auto seg_sweep = [&]() -> int {
    if (G > 0) {
      if (panel) HIPCHK(c, ppls_launch_sweep_panel(&a, c->dtype, c->Z, G, c->stream));
      else HIPCHK(c, ppls_launch_sweep_split(&a, c->stream));
    }
    for (int j = 0; j < K; ++j) {
      const int ng = g0[(size_t)j + 1] - g0[(size_t)j];
      if (ng > 0)
        HIPCHK(c, ppls_launch_reduce2(c->part + (size_t)g0[(size_t)j] * pld, ng, pld, pld, d.stats + (size_t)j * pld,
                                      tmp, c->stop_d, c->stream));
      else
        HIPCHK(c, hipMemsetAsync(d.stats + (size_t)j * pld, 0, sizeof(double) * pld, c->stream));
    }
    return allreduce(c, d.stats, (size_t)K * pld);
  };
  return meta_dev_loop(c, d, K, max_steps, atol, crit_abs, c->ssq_host[0], c->ssq_host[1], (double)c->n_total, seg_sweep,
                       out);
}

// ---- meta_* from per-population cross-products (ppls_xprod_meta.hip) -----------------

// The K statistics blocks of the loadings in W[0], C[0] and the scalars sc from the K matrices S:
// two launches, no collective (every rank holds the same S_j).  M: K x 2 P doubles of scratch.
int meta_xprod_pass(ppls_ctx* c, const double* S, int K, const PplsScalars* sc, double* stats, double* M,
                    const int* stop) {
  const int P = c->ldx + c->ldy;
  const int rw = ppls_xprod_meta_rows(K, P, c->xprod_rw, c->num_cus);
  HIPCHK(c, ppls_launch_xprod_meta(S, K, c->ldx, c->ldy, rw, c->W[0], c->C[0], sc, stats, c->part_ld, M, stop, c->stream));
  return PPLS_OK;
}

struct MetaXpScratch {
  double* M = nullptr;
  double* stats = nullptr;
  PplsScalars* sc = nullptr;
  ~MetaXpScratch() { dfree(M); dfree(stats); dfree(sc); }
};

// meta_ppls_device's loop with the segmented sweep replaced by the pass over the K matrices.
// N (K), ssq (2K) and ssqX, ssqY, Ntot as for meta_dev_loop; path: what ppls_meta_info reports.
int meta_ppls_xprod(ppls_ctx* c, const double* S, int K, const double* N, const double* ssq, double ssqX, double ssqY,
                    double Ntot, const Rank1& t0, int max_steps, double atol, int crit_abs, int path, ppls_meta_fit* out) {
  if (K < 1 || K > PPLS_META_KMAX)
    return fail(c, PPLS_E_ARG, "meta_PPLSi from cross-products: %d populations, at most %d", K, PPLS_META_KMAX);
  int rc;
  c->meta_path = path;
  if ((rc = ensure_stop(c)) || (rc = reset_stop(c))) return rc;
  MetaXpScratch x;   // (freed after d, whose loop has synchronised by then)
  MetaDev d;
  if ((rc = dalloc(c, &x.M, (size_t)K * 2 * (c->ldx + c->ldy)))) return rc;
  if ((rc = meta_dev_begin(c, d, K, N, ssq, t0, max_steps))) return rc;
  auto pass = [&]() -> int { return meta_xprod_pass(c, S, K, d.sc, d.stats, x.M, c->stop_d); };
  return meta_dev_loop(c, d, K, max_steps, atol, crit_abs, ssqX, ssqY, Ntot, pass, out);
}

// meta_sweep_all from the K matrices: every population's SX, SY, G for its scalars pops[j].t and the
// shared loadings w, cv.
int meta_xprod_all(ppls_ctx* c, const double* S, std::vector<MetaPop>& pops, const std::vector<double>& w,
                   const std::vector<double>& cv) {
  const int K = (int)pops.size(), P = c->ldx + c->ldy;
  const int64_t pld = c->part_ld;
  int rc;
  MetaXpScratch x;
  if ((rc = dalloc(c, &x.M, (size_t)K * 2 * P)) || (rc = dalloc(c, &x.stats, (size_t)K * pld)) ||
      (rc = dalloc(c, &x.sc, (size_t)K)))
    return rc;
  std::vector<PplsScalars> hsc((size_t)K);
  for (int j = 0; j < K; ++j) {
    pops[j].t.w = w;
    pops[j].t.c = cv;
    const PplsRank1 r1 = r1_of(pops[j].t);
    ppls_rank1_sweep_scalars(&r1, &hsc[(size_t)j]);
  }
  std::vector<double> wv((size_t)c->ldx, 0.0), cvv((size_t)c->ldy, 0.0);
  std::copy(w.begin(), w.end(), wv.begin());
  std::copy(cv.begin(), cv.end(), cvv.begin());
  HIPCHK(c, hipMemcpyAsync(c->W[0], wv.data(), sizeof(double) * wv.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->C[0], cvv.data(), sizeof(double) * cvv.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(x.sc, hsc.data(), sizeof(PplsScalars) * K, hipMemcpyHostToDevice, c->stream));
  if ((rc = meta_xprod_pass(c, S, K, x.sc, x.stats, x.M, nullptr))) return rc;
  std::vector<double> st((size_t)K * pld);
  HIPCHK(c, hipMemcpyAsync(st.data(), x.stats, sizeof(double) * st.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < K; ++j) {
    const double* b = st.data() + (size_t)j * pld;
    pops[j].SX.assign(b, b + c->p);
    pops[j].SY.assign(b + c->ldx, b + c->ldx + c->q);
    for (int e = 0; e < 4; ++e) pops[j].G[e] = b[(size_t)c->ldx + c->ldy + e];
  }
  return PPLS_OK;
}

// Option meta_xprod on resident rows: S_j = [X_j Y_j]'[X_j Y_j] of every population's contiguous
// local row block on the fp64 MFMA Gram (either storage type; gram_int8 does not apply), then one
// all-reduce of all K matrices (a rank without rows of a population contributes zeros).  Kept with the
// pop_local / pop_total they were formed for until the data change (xprod_free), other populations
// are passed or the option goes to 0: a second fit forms nothing.
int meta_xp_ensure(ppls_ctx* c, const std::vector<MetaPop>& pops, const int64_t* pop_local, const int64_t* pop_total) {
  const int K = (int)pops.size(), P = c->ldx + c->ldy;
  const size_t PP = (size_t)P * P;
  if (c->mx_S && c->mx_K == K && std::equal(pop_local, pop_local + K, c->mx_local.begin()) &&
      std::equal(pop_total, pop_total + K, c->mx_total.begin()))
    return PPLS_OK;
  int rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  meta_xp_free(c);
  const auto t0 = std::chrono::steady_clock::now();
  const size_t es = c->dtype ? 4 : 8;
  auto shape = [&](int j) {
    GramShape g = gram_shape(c, true, 0);
    g.X = (const char*)c->X + (size_t)pops[j].row0 * c->ldx * es;
    g.Y = (const char*)c->Y + (size_t)pops[j].row0 * c->ldy * es;
    return g;
  };
  // the K matrices and the largest population's Gram partials; when sharded the ranks agree that all
  // of them were allocated before anyone enters the all-reduce of the matrices
  size_t part_len = 0;
  for (int j = 0; j < K; ++j)
    if (pops[j].nloc > 0)
      part_len = std::max(part_len, (size_t)ppls_gram_part_doubles(P, gram_nsplit(c, shape(j), pops[j].nloc, 0)));
  double* part = nullptr;
  int rc_alloc = dalloc(c, &c->mx_S, (size_t)K * PP);
  if (!rc_alloc && part_len) rc_alloc = dalloc(c, &part, part_len);
  double tot = rc_alloc ? 1.0 : 0.0;
  if (collective(c)) {
    if (!(rc = agree(c, &tot, 1)) && tot > 0.0)
      rc = fail(c, PPLS_E_NOMEM, "meta_xprod: %d rank(s) could not allocate the %d population cross-products (%.3g GB)",
                (int)tot, K, 8.0 * K * (double)PP / 1e9);
  } else {
    rc = rc_alloc;
  }
  if (rc) {
    dfree(c->mx_S);
    dfree(part);
    return rc;
  }
  for (int j = 0; j < K && !rc; ++j) {
    if (pops[j].nloc > 0) {
      rc = gram_run(c, shape(j), pops[j].nloc, 0, c->mx_S + (size_t)j * PP, nullptr, part);
    } else if (hipMemsetAsync(c->mx_S + (size_t)j * PP, 0, sizeof(double) * PP, c->stream) != hipSuccess) {
      rc = fail(c, PPLS_E_HIP, "meta_xprod: clearing an empty population's cross-products failed");
    }
  }
  dfree(part);
  if (!rc) rc = allreduce(c, c->mx_S, (size_t)K * PP);
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, PPLS_E_HIP, "meta_xprod: the formation failed");
  if (rc) { dfree(c->mx_S); return rc; }
  c->mx_K = K;
  c->mx_local.assign(pop_local, pop_local + K);
  c->mx_total.assign(pop_total, pop_total + K);
  c->mx_form_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ++c->mx_formations;
  return PPLS_OK;
}

// meta_EMstep after the populations' statistics, from rows or from cross-products: the M-step and
// the outputs.
void meta_emstep_finish(std::vector<MetaPop>& pops, int p, int q, std::vector<double>& w, std::vector<double>& cv,
                        double* W_out, double* C_out, double* params_out, double* Cxt, double* Cyu) {
  std::vector<double> cx, cy;
  meta_mstep(pops, p, q, w, cv, Cxt ? &cx : nullptr, Cyu ? &cy : nullptr);
  std::copy(w.begin(), w.end(), W_out);
  std::copy(cv.begin(), cv.end(), C_out);
  meta_params_out(pops, params_out);
  if (Cxt) std::copy(cx.begin(), cx.end(), Cxt);
  if (Cyu) std::copy(cy.begin(), cy.end(), Cyu);
}

}  // namespace

extern "C" {

int ppls_meta_emstep(ppls_ctx* c, int npop, const int64_t* pop_local, const int64_t* pop_total, const double* W,
                     const double* C, const double* params_in, double* W_out, double* C_out, double* params_out,
                     double* Cxt, double* Cyu) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!W || !C || !params_in || !W_out || !C_out || !params_out) return fail(c, PPLS_E_ARG, "NULL argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_r(c, 1, 1))) return rc;
  std::vector<MetaPop> pops;
  if ((rc = meta_setup(c, npop, pop_local, pop_total, pops))) return rc;
  std::vector<double> w(W, W + c->p), cv(C, C + c->q);
  for (int j = 0; j < npop; ++j) pops[j].t = rank1_from_params(params_in, npop, j);
  if (c->meta_xprod) {   // the statistics from the populations' cross-products (formed once, kept)
    if ((rc = meta_xp_ensure(c, pops, pop_local, pop_total)) || (rc = meta_xprod_all(c, c->mx_S, pops, w, cv))) return rc;
  } else if ((rc = meta_sweep_all(c, pops, w, cv))) {
    return rc;
  }
  meta_emstep_finish(pops, c->p, c->q, w, cv, W_out, C_out, params_out, Cxt, Cyu);
  return PPLS_OK;
}

int ppls_meta_ppls(ppls_ctx* c, int npop, const int64_t* pop_local, const int64_t* pop_total, int max_steps,
                   double atol, int crit_abs, const ppls_theta* init, ppls_meta_fit* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!init || !init->W || !init->C || !init->B || !init->sigT || !out || !out->W || !out->C || !out->params)
    return fail(c, PPLS_E_ARG, "NULL argument");
  if (max_steps < 1) return fail(c, PPLS_E_ARG, "EMsteps must be >= 1");
  int rc;
  if ((rc = check_fit_data(c))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, 1, max_steps))) return rc;
  std::vector<MetaPop> pops;
  if ((rc = meta_setup(c, npop, pop_local, pop_total, pops))) return rc;
  const int p = c->p, q = c->q;
  const Rank1 t0 = rank1_from_init(init, p, q);
  std::vector<double> w = t0.w, cv = t0.c;
  for (auto& pp : pops) pp.t = t0;   // params = lapply(.., list(B_T = Bnw, sigX = signw[1], ...)) (:545)
  auto crit = [&](double x) { return crit_abs ? std::fabs(x) : x; };
  const size_t ld = (size_t)max_steps + 1;
  meta_log_clear(out, max_steps, npop);
  if (c->meta_xprod) {   // every step reads the K cross-product matrices (8 K P^2 bytes), not the rows
    if ((rc = meta_xp_ensure(c, pops, pop_local, pop_total))) return rc;
    std::vector<double> hN, hs;   // (the sums of squares are meta_setup's, from the rows)
    meta_pack_counts(pops, hN, hs);
    return meta_ppls_xprod(c, c->mx_S, npop, hN.data(), hs.data(), c->ssq_host[0], c->ssq_host[1], (double)c->n_total, t0,
                           max_steps, atol, crit_abs, 4, out);
  }
  if (meta_device_ok(c, npop)) return meta_ppls_device(c, pops, t0, max_steps, atol, crit_abs, out);
  c->meta_path = 1;
  // logvalue[1, ] = rep(logl_W(X, Y, Wnw, Cnw, Bnw, ...), K) (:544): one full-data sweep
  {
    std::vector<double> SX, SY;
    double G[4];
    if ((rc = rank1_sweep(c, t0, std::vector<double>(), std::vector<double>(), 0, SX, SY, G))) return rc;
    const double l0 = rank1_loglik(t0, G, c->ssq_host[0], c->ssq_host[1], (double)c->n_total, p, q);
    if (out->log)
      for (int j = 0; j < npop; ++j) out->log[(size_t)j * ld] = l0;
    out->steps = 0;
    std::vector<double> prev(npop, l0);
    if ((rc = meta_sweep_all(c, pops, w, cv))) return rc;   // meta_EMstep's E-step of step 1
    int i;
    for (i = 1; i <= max_steps; ++i) {                           // :551
      meta_mstep(pops, p, q, w, cv, nullptr, nullptr);         // fit = meta_EMstep(...) (:555-570)
      if ((rc = meta_sweep_all(c, pops, w, cv))) return rc;   // next E-step; its Gram gives logl_W
      double s_new = 0.0, s_old = 0.0;
      for (int j = 0; j < npop; ++j) {                          // logvalue[i+1, j] (:571-573)
        const double lj = rank1_loglik(pops[j].t, pops[j].G, pops[j].ssq[0], pops[j].ssq[1], pops[j].N, p, q);
        if (out->log) out->log[(size_t)j * ld + i] = lj;
        s_old += prev[j];
        s_new += lj;
        prev[j] = lj;
      }
      out->steps = i;
      if (std::isnan(s_new - s_old))                            // `if (NA < atol)` stops meta_PPLSi (:575)
        return fail(c, PPLS_E_NUMERIC, "meta_PPLSi: the log-likelihood increment of EM step %d is NaN", i);
      if (crit(s_new - s_old) < atol) break;                    // :575-578
    }
  }
  std::copy(w.begin(), w.end(), out->W);
  std::copy(cv.begin(), cv.end(), out->C);
  meta_params_out(pops, out->params);
  return PPLS_OK;
}

// variances.PPLS_simult (EM_W_multi.R:830-860).  X'X (or Y'Y) once on MFMA for all components,
// Cxt = X' mu in one HBM pass, then per component the p x p B_exp - SSt_exp on the device and its
// inverse by rocSOLVER: Cholesky potrf/potri of -(B_exp - SSt_exp), or getrf/getri (R's solve())
// when one is not positive definite.  Data-dependent sums are all-reduced over ranks.
int ppls_variances(ppls_ctx* c, const double* mu, const double* Cdiag, double sigE, int a, int xory, double* W,
                   double* B_exp, double* varMatrix, double* SSt_exp, double* SSt_star, double* seLoad) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if ((!mu && c->n_local > 0) || !Cdiag || !W || !B_exp || !seLoad) return fail(c, PPLS_E_ARG, "NULL argument");
  if (a < 1 || a > 16) return fail(c, PPLS_E_ARG, "number of components %d outside [1, 16]", a);
  if (xory != 0 && xory != 1) return fail(c, PPLS_E_ARG, "XorY must be 0 (\"X\") or 1 (\"Y\")");
  HIPCHK(c, hipSetDevice(c->device));
  const int f32 = c->dtype;
  const int p = xory ? c->q : c->p, ld = xory ? c->ldy : c->ldx;
  const void* D = xory ? (const void*)c->Y : (const void*)c->X;
  const int64_t n = c->n_local;
  const double N = (double)c->n_total;
  if (a > p) return fail(c, PPLS_E_ARG, "more components (%d) than columns (%d)", a, p);
  int rc = PPLS_OK;
  double *dmu = nullptr, *dpart = nullptr, *dS = nullptr, *dG = nullptr, *dM = nullptr, *dv = nullptr, *dMc = nullptr;
  double *dexp = nullptr, *dstar = nullptr, *dse = nullptr;
  rocblas_int *ipiv = nullptr, *info = nullptr;
  hipEvent_t evS = nullptr;
  auto done = [&](int code) {
    if (evS) (void)hipEventDestroy(evS);
    dfree(dmu); dfree(dpart); dfree(dS); dfree(dG); dfree(dM); dfree(dMc); dfree(dv); dfree(dexp); dfree(dstar); dfree(dse);
    if (ipiv) (void)hipFree(ipiv);
    if (info) (void)hipFree(info);
    return code;
  };
#define VCHK(call)                                                                              \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) return done(fail(c, PPLS_E_HIP, "%s: %s", #call, hipGetErrorString(e_))); \
  } while (0)
#define VRC(call)                  \
  do {                             \
    if ((rc = (call))) return done(rc); \
  } while (0)
  const size_t pp = (size_t)p * p;
  // ---- Cxt = D' mu (a x ld, column k contiguous) and ||mu_k||^2 (all-reduced) ----------------
  const int chunks = ppls_xtmu_chunks(std::max<int64_t>(n, 1), ld, f32);
  const int64_t sld = (int64_t)a * ld;
  VRC(dalloc(c, &dS, (size_t)sld + 16));
  std::vector<double> mu2(a, 0.0);
  if (n > 0) {
    VRC(dalloc(c, &dmu, (size_t)n * a));
    VRC(dalloc(c, &dpart, (size_t)chunks * sld + (size_t)ppls_reduce_tmp_len(chunks, sld)));
    VCHK(hipMemcpyAsync(dmu, mu, sizeof(double) * n * a, hipMemcpyHostToDevice, c->stream));
    VCHK(ppls_launch_xtmu(D, f32, n, ld, dmu, a, chunks, dpart, sld, c->stream));
    VCHK(ppls_launch_reduce2(dpart, chunks, sld, sld, dS, dpart + (size_t)chunks * sld, nullptr, c->stream));
    for (int k = 0; k < a; ++k)
      for (int64_t i = 0; i < n; ++i) mu2[k] += mu[(size_t)k * n + i] * mu[(size_t)k * n + i];   // crossprod(mu_T)
    dfree(dpart);
  } else {
    VCHK(hipMemsetAsync(dS, 0, sizeof(double) * sld, c->stream));
  }
  VCHK(hipMemcpyAsync(dS + sld, mu2.data(), sizeof(double) * a, hipMemcpyHostToDevice, c->stream));
  VRC(allreduce(c, dS, (size_t)sld + a));
  std::vector<double> S((size_t)sld + a);
  VCHK(hipMemcpyAsync(S.data(), dS, sizeof(double) * S.size(), hipMemcpyDeviceToHost, c->stream));
  VCHK(hipEventCreateWithFlags(&evS, hipEventDisableTiming));
  VCHK(hipEventRecord(evS, c->stream));   // the host's orth below overlaps the Gram
  // ---- G = D'D on MFMA, split over row ranges, all-reduced -- or, when the cross-product form
  // has formed S = [X Y]'[X Y] for this data (ppls_xprod.hip), its X'X or Y'Y block as it stands
  // (already summed over ranks; symmetric, so its row-major block is the column-major G) ------
  VRC(dalloc(c, &dG, pp));
  if (c->xp_ready) {
    const size_t P = (size_t)c->ldx + c->ldy, off = xory ? (size_t)c->ldx : 0;
    VCHK(hipMemcpy2DAsync(dG, sizeof(double) * p, c->xp_S + off * P + off, sizeof(double) * P, sizeof(double) * p, p,
                          hipMemcpyDeviceToDevice, c->stream));
  } else {
    if (n > 0) {   // (option gram_int8: the int8 CRT form, else / on its fallback the fp64 MFMA Gram)
      VRC(gram_run_s(c, gram_shape(c, false, xory), n, dG, nullptr, nullptr));
    } else {
      VCHK(hipMemsetAsync(dG, 0, sizeof(double) * pp, c->stream));
    }
    VRC(allreduce(c, dG, pp));
  }
  VCHK(hipEventSynchronize(evS));
  std::vector<double> Sp((size_t)p * a);   // t(data) %*% mu (p x a, column-major)
  for (int k = 0; k < a; ++k)
    for (int i = 0; i < p; ++i) Sp[(size_t)k * p + i] = S[(size_t)k * ld + i];
  for (int k = 0; k < a; ++k) mu2[k] = S[(size_t)sld + k];
  // W = orth(t(data) %*% mu, type = "SVD") (:831-832)
  if ((rc = host_orth(Sp.data(), p, a, PPLS_ORTH_SVD, W)))
    return done(fail(c, rc, "orth(t(data) %%*%% mu): rank-deficient"));
  // ---- per component: M = B_exp - SSt_exp, varMatrix = -solve(M), seLoad --------------------
  if (!c->blas) {
    if (rocblas_create_handle(&c->blas) != rocblas_status_success) return done(fail(c, PPLS_E_HIP, "rocblas_create_handle failed"));
  }
  if (rocblas_set_stream(c->blas, c->stream) != rocblas_status_success) return done(fail(c, PPLS_E_HIP, "rocblas_set_stream failed"));
  // all a matrices at once: one strided-batched LU and inverse (rocSOLVER's panel factorisation is
  // thousands of small launches per matrix; batching shares them -- profiles/r3_variances_*.txt)
  VRC(dalloc(c, &dM, pp * (size_t)a));
  VRC(dalloc(c, &dv, (size_t)2 * p));
  VRC(dalloc(c, &dse, (size_t)p));
  if (SSt_exp) VRC(dalloc(c, &dexp, pp));
  if (SSt_star) VRC(dalloc(c, &dstar, pp));
  VCHK(hipMalloc((void**)&ipiv, sizeof(rocblas_int) * p * a));
  VCHK(hipMalloc((void**)&info, sizeof(rocblas_int) * a));
  const double s2 = sigE * sigE, s4 = s2 * s2;
  std::vector<double> v2((size_t)2 * p);
  for (int i = 0; i < a; ++i) {
    const double ctt = N * Cdiag[i];                         // Ctt = N * t(Ctt[i, i]) (:840)
    const double Vt = ctt - mu2[i];                          // Vt = Ctt - crossprod(mu_T) (:842)
    const double k1 = ctt + 2.0 * Vt;
    const double k2 = ctt * ctt + 4.0 * mu2[i] * Vt + 2.0 * Vt * Vt;
    const double bstar = ctt / s2 / N;                       // B_star = c(Ctt)/(sigE^2) * I / nrow(X) (:844)
    B_exp[i] = bstar;
    for (int e = 0; e < p; ++e) {
      v2[e] = Sp[(size_t)i * p + e];                         // Cxt = t(X) %*% mu_T (:843)
      v2[(size_t)p + e] = W[(size_t)i * p + e];
    }
    VCHK(hipMemcpyAsync(dv, v2.data(), sizeof(double) * 2 * p, hipMemcpyHostToDevice, c->stream));
    VCHK(ppls_launch_varmat(dG, dv, dv + p, p, ctt, k1, k2, bstar, s4, N, dM + pp * i, dexp, dstar, c->stream));
    if (SSt_exp) VCHK(hipMemcpyAsync(SSt_exp + (size_t)i * pp, dexp, sizeof(double) * pp, hipMemcpyDeviceToHost, c->stream));
    if (SSt_star) VCHK(hipMemcpyAsync(SSt_star + (size_t)i * pp, dstar, sizeof(double) * pp, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipStreamSynchronize(c->stream));   // dv is reused by the next component
  }
  // varMatrix = -solve(M) = (-M)^-1, and -M = SSt_exp - B_exp is the observed information: symmetric
  // and, at a proper fit, positive definite.  Cholesky potrf + potri (half the flops of LU + inverse)
  // on a copy of -M; if any matrix is not positive definite, the batch takes R's solve() route, LU
  // getrf + getri, from the untouched M.  Either inverse is backward stable: they agree to ~kappa eps.
  std::vector<rocblas_int> inf(a, 0);
  bool chol = c->var_chol != 0;
  int chol_mode = c->var_chol;
  if (chol_mode == 1) {   // the hand-written inverse needs a p^2 scratch per matrix more than rocSOLVER
    const size_t need = sizeof(double) * (pp * (size_t)a + (size_t)ppls_spd_inverse_work(p, a));
    if (hipMalloc((void**)&dMc, need) != hipSuccess) {
      (void)hipGetLastError();   // (clear it) not enough HBM: rocSOLVER's in-place potrf/potri instead
      dMc = nullptr;
      chol_mode = 2;
    }
  }
  if (chol && chol_mode == 1) {
    // hand-written (ppls_linalg.hip): blocked Cholesky of every matrix of the batch in the same
    // launches, then T = L^-1 and T'T -- 3 nb launches (nb = p / 64) where rocSOLVER's potrf + potri
    // took 1,400 (profiles/r4_variances_c3_timeline.txt)
    VCHK(hipMemcpyAsync(dMc, dM, sizeof(double) * pp * a, hipMemcpyDeviceToDevice, c->stream));
    VCHK(ppls_launch_negate(dMc, (int64_t)pp * a, c->stream));
    VCHK(ppls_spd_inverse_batched(dMc, p, a, dMc + pp * (size_t)a, (int*)info, c->stream));
    VCHK(hipMemcpyAsync(inf.data(), info, sizeof(rocblas_int) * a, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < a; ++i) chol = chol && inf[i] == 0;
  } else if (chol) {
    VRC(dalloc(c, &dMc, pp * (size_t)a));
    VCHK(hipMemcpyAsync(dMc, dM, sizeof(double) * pp * a, hipMemcpyDeviceToDevice, c->stream));
    VCHK(ppls_launch_negate(dMc, (int64_t)pp * a, c->stream));
    if (rocsolver_dpotrf_strided_batched(c->blas, rocblas_fill_lower, p, dMc, p, (rocblas_stride)pp, info, a) !=
        rocblas_status_success)
      return done(fail(c, PPLS_E_HIP, "rocsolver potrf (strided batched) failed"));
    VCHK(hipMemcpyAsync(inf.data(), info, sizeof(rocblas_int) * a, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < a; ++i) chol = chol && inf[i] == 0;
    if (chol && rocsolver_dpotri_strided_batched(c->blas, rocblas_fill_lower, p, dMc, p, (rocblas_stride)pp, info, a) !=
                    rocblas_status_success)
      return done(fail(c, PPLS_E_HIP, "rocsolver potri (strided batched) failed"));
  }
  if (!chol) {
    if (rocsolver_dgetrf_strided_batched(c->blas, p, p, dM, p, (rocblas_stride)pp, ipiv, p, info, a) !=
            rocblas_status_success ||
        rocsolver_dgetri_strided_batched(c->blas, p, dM, p, (rocblas_stride)pp, ipiv, p, info, a) !=
            rocblas_status_success)
      return done(fail(c, PPLS_E_HIP, "rocsolver getrf/getri (strided batched) failed"));
  }
  VCHK(hipMemcpyAsync(inf.data(), info, sizeof(rocblas_int) * a, hipMemcpyDeviceToHost, c->stream));
  VCHK(hipStreamSynchronize(c->stream));
  for (int i = 0; i < a; ++i)
    if (inf[i] != 0)   // solve(): "Lapack routine dgesv: system is exactly singular"
      return done(fail(c, PPLS_E_NUMERIC, "component %d: B_exp - SSt_exp is exactly singular (U[%d,%d] = 0)", i + 1,
                       (int)inf[i], (int)inf[i]));
  if (chol) std::swap(dM, dMc);   // the inverse to copy out
  for (int i = 0; i < a; ++i) {
    if (chol) VCHK(ppls_launch_symdiag(dM + pp * i, p, dse, c->stream));
    else VCHK(ppls_launch_negdiag(dM + pp * i, p, dse, c->stream));
    if (varMatrix) VCHK(hipMemcpyAsync(varMatrix + (size_t)i * pp, dM + pp * i, sizeof(double) * pp, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipMemcpyAsync(seLoad + (size_t)i * p, dse, sizeof(double) * p, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipStreamSynchronize(c->stream));   // dse is reused by the next component
  }
  VCHK(hipStreamSynchronize(c->stream));
#undef VCHK
#undef VRC
  return done(PPLS_OK);
}

// variances.PPLS_simult from the cross-products S alone: the rows enter :830-860 through
// t(X) diag(Ctt) X = N Ctt_ii X'X (S's diagonal block), Cxt = X'mu_T and W = orth(X'mu_T) (the SX
// statistic and the polar factor of one cross-product EM step at theta) and crossprod(mu_T[, i]) (a
// quadratic form in that step's 2r x 2r Gram).  Statistics, finalize, all r observed-information
// matrices (one launch), their batched inverse and the mirror + seLoad launch stay on the device; the
// host reads 4 r^2 + 2 r doubles for the scalars and synchronises once more before the copy-out.
int ppls_variances_xprod(ppls_ctx* c, const ppls_theta* th, int r, int xory, double* W, double* Cdiag, double* B_exp,
                         double* varMatrix, double* SSt_exp, double* SSt_star, double* seLoad) {
  if (!c) return PPLS_E_ARG;
  if (c->st_state == 1) return fail(c, PPLS_E_STATE, "a stream is open: S is complete only after ppls_stream_end");
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (!th || !W || !B_exp || !seLoad) return fail(c, PPLS_E_ARG, "NULL argument");
  if (xory != 0 && xory != 1) return fail(c, PPLS_E_ARG, "XorY must be 0 (\"X\") or 1 (\"Y\")");
  if (r < 1 || r > 16) return fail(c, PPLS_E_ARG, "number of components %d outside [1, 16]", r);
  const int p = xory ? c->q : c->p, ld = xory ? c->ldy : c->ldx;
  if (r > p) return fail(c, PPLS_E_ARG, "more components (%d) than columns (%d)", r, p);
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  // ---- one cross-product EM step at theta: SX / SY, the Gram, Ctt / Cuu, the new W / C ------------
  if ((rc = ensure_r(c, r, 1))) return rc;
  if ((rc = upload_theta(c, th, r, 0))) return rc;
  HIPCHK(c, hipMemsetAsync(c->status, 0, PPLS_STATUS_INTS * sizeof(int), c->stream));
  const bool had_S = c->xp_ready;
  if ((rc = xprod_stats(c, r, 0))) return rc;   // forms S first where it is missing: the only collective
  if (!had_S) c->xp_explicit = true;            // ... and then kept, as by ppls_xprod_prepare
  if ((rc = finalize(c, r, 0, 1, -1, PPLS_ORTH_SVD))) return rc;
  const int rr = r * r;
  std::vector<double> G((size_t)4 * rr);
  PplsMoments mom;
  int st3[PPLS_STATUS_INTS];
  HIPCHK(c, hipMemcpyAsync(G.data(), c->stats + (size_t)r * (c->ldx + c->ldy), sizeof(double) * 4 * rr,
                           hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&mom, c->mom, sizeof mom, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(st3, c->status, sizeof st3, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (st3[0] == -7) {
    if (c->team_bar) HIPCHK(c, hipMemset(c->team_bar, 0, 8 * sizeof(unsigned)));
    return fail(c, PPLS_E_HIP, "finalize polar team barrier timed out (status -7)");
  }
  if (st3[0] != 0) return fail(c, PPLS_E_NUMERIC, "orth(t(data) %%*%% mu): rank-deficient");
  // ---- the scalars of :840-848, from 4 r^2 + r numbers -------------------------------------------
  const PplsScalars s = scalars_of(th, r);
  const double N = (double)c->n_total;
  const double s2 = th->sigE * th->sigE;   // sigE for "Y" too, like the reference
  PplsVarinfoArgs va;
  memset(&va, 0, sizeof va);
  std::vector<double> cd((size_t)r);
  for (int i = 0; i < r; ++i) {
    const double c1 = xory ? s.gamma[i] : s.alpha[i], c2 = xory ? s.delta[i] : s.beta[i];
    const double A = PPLS_GA(G.data(), r, i, i), D = PPLS_GD(G.data(), r, i, i), Bm = PPLS_GB(G.data(), r, i, i);
    const double mu2 = c1 * c1 * A + 2.0 * c1 * c2 * D + c2 * c2 * Bm;   // crossprod(mu[, i])
    cd[(size_t)i] = xory ? mom.Cuu[i] : mom.Ctt[i];
    const double ctt = N * cd[(size_t)i];
    const double Vt = ctt - mu2;
    va.ctt[i] = ctt;
    va.k1[i] = ctt + 2.0 * Vt;
    va.k2[i] = ctt * ctt + 4.0 * mu2 * Vt + 2.0 * Vt * Vt;
    va.bstar[i] = ctt / s2 / N;
  }
  va.S = c->xp_S;
  va.P = c->ldx + c->ldy;
  va.off = xory ? c->ldx : 0;
  va.p = p;
  va.a = r;
  va.cxt = c->stats + (xory ? (size_t)r * c->ldx : 0);
  va.ldc = ld;
  va.w = xory ? c->C[1] : c->W[1];
  va.ldw = ld;
  va.s4 = s2 * s2;
  va.N = N;
  // ---- J_i for all i in one launch, the batched inverse, mirror + seLoad --------------------------
  const size_t pp = (size_t)p * p;
  double *dJ = nullptr, *dexp = nullptr, *dstar = nullptr, *dse = nullptr;
  rocblas_int *ipiv = nullptr, *info = nullptr;
  auto done = [&](int code) {
    dfree(dJ); dfree(dexp); dfree(dstar); dfree(dse);
    if (ipiv) (void)hipFree(ipiv);
    if (info) (void)hipFree(info);
    return code;
  };
#define VCHK(call)                                                                              \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) return done(fail(c, PPLS_E_HIP, "%s: %s", #call, hipGetErrorString(e_))); \
  } while (0)
#define VRC(call)                  \
  do {                             \
    if ((rc = (call))) return done(rc); \
  } while (0)
  bool chol = c->var_chol != 0;
  int chol_mode = c->var_chol;
  if (chol_mode == 1) {   // the hand-written inverse works in a scratch behind the batch
    if (hipMalloc((void**)&dJ, sizeof(double) * (pp * (size_t)r + (size_t)ppls_spd_inverse_work(p, r))) != hipSuccess) {
      (void)hipGetLastError();   // (clear it) not enough HBM: rocSOLVER's in-place potrf/potri instead
      dJ = nullptr;
      chol_mode = 2;
    }
  }
  if (!dJ) VRC(dalloc(c, &dJ, pp * (size_t)r));
  if (SSt_exp) VRC(dalloc(c, &dexp, pp * (size_t)r));
  if (SSt_star) VRC(dalloc(c, &dstar, pp * (size_t)r));
  VRC(dalloc(c, &dse, (size_t)p * r));
  VCHK(hipMalloc((void**)&info, sizeof(rocblas_int) * 2 * r));
  va.J = dJ;
  std::vector<double> Wp((size_t)ld * r);
  std::vector<rocblas_int> inf((size_t)2 * r, 0);
  for (int pass = 0;; ++pass) {
    // pass 0: Cholesky (unless var_chol = 0); pass 1: some J_i was not positive definite, the batch
    // takes R's solve() route, LU, from J formed again (the Cholesky worked in place)
    va.sst_exp = pass == 0 ? dexp : nullptr;
    va.sst_star = pass == 0 ? dstar : nullptr;
    VCHK(ppls_launch_varinfo_batched(&va, c->stream));
    if (pass == 0) {
      if (SSt_exp) VCHK(hipMemcpyAsync(SSt_exp, dexp, sizeof(double) * pp * r, hipMemcpyDeviceToHost, c->stream));
      if (SSt_star) VCHK(hipMemcpyAsync(SSt_star, dstar, sizeof(double) * pp * r, hipMemcpyDeviceToHost, c->stream));
      VCHK(hipMemcpyAsync(Wp.data(), va.w, sizeof(double) * ld * r, hipMemcpyDeviceToHost, c->stream));
    }
    VCHK(hipMemsetAsync(info, 0, sizeof(rocblas_int) * 2 * r, c->stream));
    if (!chol || chol_mode == 2) {   // the rocSOLVER routes
      if (!c->blas && rocblas_create_handle(&c->blas) != rocblas_status_success)
        return done(fail(c, PPLS_E_HIP, "rocblas_create_handle failed"));
      if (rocblas_set_stream(c->blas, c->stream) != rocblas_status_success)
        return done(fail(c, PPLS_E_HIP, "rocblas_set_stream failed"));
    }
    if (chol && chol_mode == 1) {
      VCHK(ppls_spd_inverse_batched(dJ, p, r, dJ + pp * (size_t)r, (int*)info, c->stream));
    } else if (chol) {   // (potri of a factorisation that failed is discarded below)
      if (rocsolver_dpotrf_strided_batched(c->blas, rocblas_fill_lower, p, dJ, p, (rocblas_stride)pp, info, r) !=
              rocblas_status_success ||
          rocsolver_dpotri_strided_batched(c->blas, rocblas_fill_lower, p, dJ, p, (rocblas_stride)pp, info + r, r) !=
              rocblas_status_success)
        return done(fail(c, PPLS_E_HIP, "rocsolver potrf/potri (strided batched) failed"));
    } else {
      if (!ipiv) VCHK(hipMalloc((void**)&ipiv, sizeof(rocblas_int) * p * r));
      if (rocsolver_dgetrf_strided_batched(c->blas, p, p, dJ, p, (rocblas_stride)pp, ipiv, p, info, r) !=
              rocblas_status_success ||
          rocsolver_dgetri_strided_batched(c->blas, p, dJ, p, (rocblas_stride)pp, ipiv, p, info + r, r) !=
              rocblas_status_success)
        return done(fail(c, PPLS_E_HIP, "rocsolver getrf/getri (strided batched) failed"));
    }
    VCHK(ppls_launch_varfinish_batched(dJ, p, r, chol ? 1 : 0, dse, c->stream));
    if (varMatrix) VCHK(hipMemcpyAsync(varMatrix, dJ, sizeof(double) * pp * r, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipMemcpyAsync(seLoad, dse, sizeof(double) * p * r, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipMemcpyAsync(inf.data(), info, sizeof(rocblas_int) * 2 * r, hipMemcpyDeviceToHost, c->stream));
    VCHK(hipStreamSynchronize(c->stream));
    bool bad = false;
    for (int i = 0; i < 2 * r; ++i) bad = bad || inf[(size_t)i] != 0;
    if (!bad) break;
    if (!chol) {   // solve(): "Lapack routine dgesv: system is exactly singular"
      for (int i = 0; i < 2 * r; ++i)
        if (inf[(size_t)i] != 0)
          return done(fail(c, PPLS_E_NUMERIC, "component %d: B_exp - SSt_exp is exactly singular (U[%d,%d] = 0)",
                           i % r + 1, (int)inf[(size_t)i], (int)inf[(size_t)i]));
    }
    chol = false;
  }
#undef VCHK
#undef VRC
  for (int k = 0; k < r; ++k)
    for (int i = 0; i < p; ++i) W[(size_t)k * p + i] = Wp[(size_t)k * ld + i];
  for (int i = 0; i < r; ++i) {
    B_exp[i] = va.bstar[i];
    if (Cdiag) Cdiag[i] = cd[(size_t)i];
  }
  return done(PPLS_OK);
}

// Diagnostics / tests: ppls_varinfo_batched_kernel alone on host inputs (tests/varinfo_bar.py).
int ppls_varinfo(ppls_ctx* c, const double* S, int P, int off, int p, int a, const double* cxt, const double* w,
                 const double* ctt, const double* k1, const double* k2, const double* bstar, double sigE, double N,
                 double* J, double* sst_exp, double* sst_star) {
  if (!c || !S || !cxt || !w || !ctt || !k1 || !k2 || !bstar || !J) return PPLS_E_ARG;
  if (p < 1 || a < 1 || a > 16 || off < 0 || (P & 1) || (off & 1) || (int64_t)off + p + (p & 1) > P)
    return fail(c, PPLS_E_ARG, "varinfo: P and off must be even, off + p (+ 1 for odd p) <= P, 1 <= a <= 16");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t pp = (size_t)p * p, PP = (size_t)P * P;
  const int nout = 1 + (sst_exp ? 1 : 0) + (sst_star ? 1 : 0);
  double *dS = nullptr, *dv = nullptr, *dout = nullptr;
  auto done = [&](int code) {
    dfree(dS); dfree(dv); dfree(dout);
    return code;
  };
  int rc;
  if ((rc = dalloc(c, &dS, PP)) || (rc = dalloc(c, &dv, (size_t)2 * p * a)) || (rc = dalloc(c, &dout, pp * a * nout)))
    return done(rc);
  PplsVarinfoArgs va;
  memset(&va, 0, sizeof va);
  for (int i = 0; i < a; ++i) {
    va.ctt[i] = ctt[i];
    va.k1[i] = k1[i];
    va.k2[i] = k2[i];
    va.bstar[i] = bstar[i];
  }
  const double s2 = sigE * sigE;
  va.S = dS; va.P = P; va.off = off; va.p = p; va.a = a;
  va.cxt = dv; va.ldc = p; va.w = dv + (size_t)p * a; va.ldw = p;
  va.s4 = s2 * s2; va.N = N;
  va.J = dout;
  va.sst_exp = sst_exp ? dout + pp * a : nullptr;
  va.sst_star = sst_star ? dout + pp * a * (sst_exp ? 2 : 1) : nullptr;
  hipError_t e = hipMemcpy(dS, S, sizeof(double) * PP, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dv, cxt, sizeof(double) * p * a, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dv + (size_t)p * a, w, sizeof(double) * p * a, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(dout, 0xff, sizeof(double) * pp * a * nout, c->stream);   // unwritten reads NaN
  if (e == hipSuccess) e = ppls_launch_varinfo_batched(&va, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(J, va.J, sizeof(double) * pp * a, hipMemcpyDeviceToHost);
  if (e == hipSuccess && sst_exp) e = hipMemcpy(sst_exp, va.sst_exp, sizeof(double) * pp * a, hipMemcpyDeviceToHost);
  if (e == hipSuccess && sst_star) e = hipMemcpy(sst_star, va.sst_star, sizeof(double) * pp * a, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return done(fail(c, PPLS_E_HIP, "varinfo: %s", hipGetErrorString(e)));
  return done(PPLS_OK);
}

// Benchmark: the information kernel against the launches it replaces in ppls_variances' S path -- the
// block copy out of S, a ppls_varmat_kernel launches, the copy of the batch and the negate -- reps
// times each between HIP events, on the context's S with the statistics and loadings the last
// ppls_variances_xprod left (the times do not depend on the values; the scalars are 1).
// The matrices it forms live in its own scratch, are meaningless and are freed on return.
int ppls_varinfo_timing(ppls_ctx* c, int xory, int a, int reps, double* ms_new, double* ms_old) {
  if (!c || !ms_new || !ms_old || reps < 1 || (xory != 0 && xory != 1)) return PPLS_E_ARG;
  if (!c->have_data || !c->xp_ready || !c->xp_S) return fail(c, PPLS_E_STATE, "the cross-products S are not formed");
  if (a < 1 || a != c->r_alloc) return fail(c, PPLS_E_STATE, "call ppls_variances_xprod with %d components first", a);
  HIPCHK(c, hipSetDevice(c->device));
  const int p = xory ? c->q : c->p, ld = xory ? c->ldy : c->ldx;
  const size_t pp = (size_t)p * p, P = (size_t)c->ldx + c->ldy, off = xory ? (size_t)c->ldx : 0;
  double* buf = nullptr;   // [G | M batch | its copy]
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  auto done = [&](int code) {
    dfree(buf);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    return code;
  };
  int rc;
  if ((rc = dalloc(c, &buf, pp * (1 + 2 * (size_t)a)))) return done(rc);
  double *dG = buf, *dM = buf + pp, *dMc = dM + pp * a;
  PplsVarinfoArgs va;
  memset(&va, 0, sizeof va);
  for (int i = 0; i < a; ++i) va.ctt[i] = va.k1[i] = va.k2[i] = va.bstar[i] = 1.0;
  va.S = c->xp_S; va.P = (int)P; va.off = (int)off; va.p = p; va.a = a;
  va.cxt = c->stats + (xory ? (size_t)a * c->ldx : 0); va.ldc = ld;
  va.w = xory ? c->C[1] : c->W[1]; va.ldw = ld;
  va.s4 = 1.0; va.N = (double)c->n_total;
  va.J = dM;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
  for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {   // pass 0: warm-up
    e = hipEventRecord(ev[0], c->stream);
    for (int k = 0; k < reps && e == hipSuccess; ++k) e = ppls_launch_varinfo_batched(&va, c->stream);
    if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
    for (int k = 0; k < reps && e == hipSuccess; ++k) {
      e = hipMemcpy2DAsync(dG, sizeof(double) * p, c->xp_S + off * P + off, sizeof(double) * P, sizeof(double) * p, p,
                           hipMemcpyDeviceToDevice, c->stream);
      for (int i = 0; i < a && e == hipSuccess; ++i)
        e = ppls_launch_varmat(dG, va.cxt + (size_t)i * ld, va.w + (size_t)i * ld, p, 1.0, 1.0, 1.0, 1.0, 1.0, va.N,
                               dM + pp * i, nullptr, nullptr, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(dMc, dM, sizeof(double) * pp * a, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess) e = ppls_launch_negate(dMc, (int64_t)pp * a, c->stream);
    }
    if (e == hipSuccess) e = hipEventRecord(ev[2], c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev[2]);
  }
  float t0 = 0.f, t1 = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&t0, ev[0], ev[1]);
  if (e == hipSuccess) e = hipEventElapsedTime(&t1, ev[1], ev[2]);
  if (e != hipSuccess) return done(fail(c, PPLS_E_HIP, "varinfo_timing: %s", hipGetErrorString(e)));
  *ms_new = (double)t0 / reps;
  *ms_old = (double)t1 / reps;
  return done(PPLS_OK);
}

// Diagnostics / tests: the batched SPD inverse of variances.PPLS_simult on host matrices.
int ppls_spd_inverse(ppls_ctx* c, const double* A, int p, int a, int method, double* out, int* info, double* ms) {
  if (!c || !A || !out || !info || p < 1 || a < 1 || (method != 1 && method != 2)) return PPLS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t pp = (size_t)p * p;
  double *dA = nullptr, *dse = nullptr;
  int* dinfo = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = PPLS_OK;
  auto done = [&](int code) {
    dfree(dA); dfree(dse);
    if (dinfo) (void)hipFree(dinfo);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return code;
  };
  const size_t work = method == 1 ? (size_t)ppls_spd_inverse_work(p, a) : 0;
  if ((rc = dalloc(c, &dA, pp * a + work)) || (rc = dalloc(c, &dse, (size_t)p))) return done(rc);
  if (hipMalloc((void**)&dinfo, sizeof(int) * 2 * a) != hipSuccess) return done(fail(c, PPLS_E_HIP, "hipMalloc failed"));
  if (hipMemcpy(dA, A, sizeof(double) * pp * a, hipMemcpyHostToDevice) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return done(fail(c, PPLS_E_HIP, "spd_inverse: setup failed"));
  if (method == 2) {
    if (!c->blas && rocblas_create_handle(&c->blas) != rocblas_status_success)
      return done(fail(c, PPLS_E_HIP, "rocblas_create_handle failed"));
    if (rocblas_set_stream(c->blas, c->stream) != rocblas_status_success)
      return done(fail(c, PPLS_E_HIP, "rocblas_set_stream failed"));
  }
  (void)hipEventRecord(e0, c->stream);
  if (method == 1) {
    if (ppls_spd_inverse_batched(dA, p, a, dA + pp * a, dinfo, c->stream) != hipSuccess)
      return done(fail(c, PPLS_E_HIP, "spd_inverse: launch failed"));
  } else if (rocsolver_dpotrf_strided_batched(c->blas, rocblas_fill_lower, p, dA, p, (rocblas_stride)pp, dinfo, a) !=
                 rocblas_status_success ||
             rocsolver_dpotri_strided_batched(c->blas, rocblas_fill_lower, p, dA, p, (rocblas_stride)pp, dinfo + a, a) !=
                 rocblas_status_success) {   // (info: potrf's)
    return done(fail(c, PPLS_E_HIP, "rocsolver potrf/potri failed"));
  }
  (void)hipEventRecord(e1, c->stream);
  for (int z = 0; z < a; ++z)
    if (ppls_launch_symdiag(dA + pp * z, p, dse, c->stream) != hipSuccess)
      return done(fail(c, PPLS_E_HIP, "spd_inverse: symdiag failed"));
  if (hipStreamSynchronize(c->stream) != hipSuccess ||   // (the context stream does not block with stream 0)
      hipMemcpy(out, dA, sizeof(double) * pp * a, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(info, dinfo, sizeof(int) * a, hipMemcpyDeviceToHost) != hipSuccess)
    return done(fail(c, PPLS_E_HIP, "spd_inverse: copy-out failed"));
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  if (ms) *ms = t;
  return done(PPLS_OK);
}

// Diagnostics / benchmark: G = D'D (D = X for xory 0, Y for 1) on the MFMA Gram kernel only, with
// nsplit equal row splits (0 = the automatic halving splits, as in ppls_variances); G (p x p,
// column-major) may be NULL.
// *ms receives the Gram kernel's duration (HIP events on the context stream).
}  // extern "C"

namespace {

// ppls_gram (count NULL, weighted false), ppls_gram_weighted and ppls_gram_weighted_real (weight given).
int gram_debug(ppls_ctx* c, int xory, int nsplit, bool weighted, const int32_t* count, double* G, double* ms,
               const double* weight = nullptr, bool real = false) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (xory < 0 || xory > 2) return fail(c, PPLS_E_ARG, "xory must be 0 (X'X), 1 (Y'Y) or 2 ([X Y]'[X Y])");
  HIPCHK(c, hipSetDevice(c->device));
  const GramShape g = xory == 2 ? gram_shape(c, true, 0) : gram_shape(c, false, xory);
  const size_t pp = (size_t)g.p * g.p;
  if (c->n_local <= 0) return fail(c, PPLS_E_STATE, "no rows on this rank");
  int rc;
  struct Counts {
    int32_t* d = nullptr;
    double* w = nullptr;
    ~Counts() { dfree(d); dfree(w); }
  } cnt;
  if (real) {
    if (!weight) return fail(c, PPLS_E_ARG, "NULL weights for %lld rows", (long long)c->n_local);
    for (int64_t i = 0; i < c->n_local; ++i)
      if (!(weight[i] >= 0.0) || !std::isfinite(weight[i]))
        return fail(c, PPLS_E_ARG, "weight %g of row %lld is negative or not finite", weight[i], (long long)i);
    if ((rc = dalloc(c, &cnt.w, (size_t)c->n_local))) return rc;
    HIPCHK(c, hipMemcpy(cnt.w, weight, sizeof(double) * c->n_local, hipMemcpyHostToDevice));
  } else if (weighted) {
    if (!count) return fail(c, PPLS_E_ARG, "NULL counts for %lld rows", (long long)c->n_local);
    for (int64_t i = 0; i < c->n_local; ++i)
      if (count[i] < 0) return fail(c, PPLS_E_ARG, "count %d of row %lld is negative", (int)count[i], (long long)i);
    if ((rc = dalloc(c, &cnt.d, (size_t)c->n_local))) return rc;
    HIPCHK(c, hipMemcpy(cnt.d, count, sizeof(int32_t) * c->n_local, hipMemcpyHostToDevice));
  }
  double* dG = nullptr;
  if ((rc = dalloc(c, &dG, pp))) return rc;
  float t = 0.f;
  rc = gram_run(c, g, c->n_local, nsplit > 0 ? nsplit : 0, dG, &t, nullptr, cnt.d, cnt.w);
  if (!rc && G) {
    if (xory < 2) {
      if (hipMemcpy(G, dG, sizeof(double) * pp, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(c, PPLS_E_HIP, "gram: copy-out failed");
    } else {   // the joint Gram without the row padding between X's and Y's columns: (p + q)^2
      std::vector<double> full(pp);
      if (hipMemcpy(full.data(), dG, sizeof(double) * pp, hipMemcpyDeviceToHost) != hipSuccess) {
        rc = fail(c, PPLS_E_HIP, "gram: copy-out failed");
      } else {
        const int P = c->p + c->q;
        auto src = [&](int k) { return k < c->p ? k : c->ldx + (k - c->p); };
        for (int b = 0; b < P; ++b)
          for (int a = 0; a < P; ++a) G[(size_t)b * P + a] = full[(size_t)src(b) * g.p + src(a)];
      }
    }
  }
  dfree(dG);
  if (!rc && ms) *ms = t;
  return rc;
}

}  // namespace

extern "C" {

int ppls_gram(ppls_ctx* c, int xory, int nsplit, double* G, double* ms) {
  return gram_debug(c, xory, nsplit, false, nullptr, G, ms);
}

int ppls_gram_weighted(ppls_ctx* c, int xory, int nsplit, const int32_t* count, double* G, double* ms) {
  return gram_debug(c, xory, nsplit, true, count, G, ms);
}

int ppls_gram_weighted_real(ppls_ctx* c, int xory, int nsplit, const double* weight, double* G, double* ms) {
  return gram_debug(c, xory, nsplit, false, nullptr, G, ms, weight, true);
}

// scores.PPLS (EM_W_multi.R:411-420): T = X W, U = Y C (local rows, column-major n_local x k) in
// one pass -- the panel dots kernel with mu coefficients (1, 0; 0, 1), whose mu write-out is then
// exactly [X W | Y C].
int ppls_scores(ppls_ctx* c, const double* W, const double* C, int k, double* T, double* U) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!W || !C || k < 1 || k > PPLS_RMAX) return fail(c, PPLS_E_ARG, "W, C must be given with 1 <= k <= %d", PPLS_RMAX);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_r(c, k, 1))) return rc;
  std::vector<double> B(k, 1.0), sT(k, 1.0);
  ppls_theta th = {const_cast<double*>(W), const_cast<double*>(C), B.data(), sT.data(), 1.0, 1.0, 1.0};
  if ((rc = upload_theta(c, &th, k, 0))) return rc;
  PplsScalars s;
  memset(&s, 0, sizeof s);
  for (int j = 0; j < k; ++j) { s.alpha[j] = 1.0; s.delta[j] = 1.0; }
  HIPCHK(c, hipMemcpyAsync(c->sc[0], &s, sizeof s, hipMemcpyHostToDevice, c->stream));
  if (c->z_cols < 4 * k) {
    dfree(c->Z);
    c->z_cols = 0;
    if ((rc = dalloc(c, &c->Z, (size_t)ppls_panel_z_len(c->n_local, c->ldx, c->ldy, k)))) return rc;
    c->z_cols = 4 * k;
  }
  dfree(c->mu);
  if ((rc = dalloc(c, &c->mu, (size_t)std::max<int64_t>(c->n_local, 1) * 2 * k))) return rc;
  PplsSweepArgs a;
  memset(&a, 0, sizeof a);
  a.X = c->X; a.Y = c->Y; a.n_local = c->n_local; a.p = c->p; a.q = c->q; a.ldx = c->ldx; a.ldy = c->ldy;
  a.Wp = c->W[0]; a.Cp = c->C[0]; a.sc = c->sc[0]; a.mu = c->mu; a.write_mu = 1; a.r = k;
  a.num_cus = c->num_cus; a.dots_rows = c->dots_rows; a.dots_pair = c->dots_pair;
  HIPCHK(c, ppls_launch_panel_dots(&a, c->dtype, c->Z, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t blk = sizeof(double) * (size_t)c->n_local * k;
  if (c->n_local > 0 && T) HIPCHK(c, hipMemcpy(T, c->mu, blk, hipMemcpyDeviceToHost));
  if (c->n_local > 0 && U) HIPCHK(c, hipMemcpy(U, c->mu + (size_t)c->n_local * k, blk, hipMemcpyDeviceToHost));
  dfree(c->mu);   // sized for this k; the EM path re-allocates its own
  return PPLS_OK;
}

int ppls_em_begin(ppls_ctx* c, const ppls_theta* th, int r) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  if ((rc = check_fit_data(c))) return rc;
  if (!theta_finite(th, c->p, c->q, r)) return fail(c, PPLS_E_ARG, "theta0 has non-finite entries");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, 1 << 16))) return rc;
  std::vector<double> W(th->W, th->W + (size_t)c->p * r), C(th->C, th->C + (size_t)c->q * r);
  std::vector<double> B(th->B, th->B + r), T(th->sigT, th->sigT + r);
  ppls_theta t0 = {W.data(), C.data(), B.data(), T.data(), th->sigE, th->sigF, th->sigH};
  canonicalize(&t0, c->p, c->q, r);
  if ((rc = upload_theta(c, &t0, r, 0))) return rc;
  HIPCHK(c, hipMemsetAsync(c->status, 0, PPLS_STATUS_INTS * sizeof(int), c->stream));
  c->em_r = r;
  c->em_cur = 0;
  c->em_iter = 0;
  if ((rc = xprod_begin(c, 1 << 16, r))) return rc;
  c->em_active = true;
  return PPLS_OK;
}

int ppls_em_iterate(ppls_ctx* c, int nsteps, int type) {
  if (!c) return PPLS_E_ARG;
  if (!c->em_active || c->r_alloc != c->em_r) return fail(c, PPLS_E_STATE, "call ppls_em_begin first");
  if (nsteps < 0) return fail(c, PPLS_E_ARG, "nsteps < 0");
  if (c->em_iter + nsteps + 2 > c->loglik_cap) return fail(c, PPLS_E_ARG, "too many iterations for one run");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  for (int s = 0; s < nsteps; ++s) {
    const int nxt = c->em_cur ^ 1;
    if ((rc = stats_step(c, c->em_r, c->em_cur, false, true))) return rc;
    if ((rc = finalize(c, c->em_r, c->em_cur, nxt, c->em_iter >= 1 ? c->em_iter - 1 : -1, type))) return rc;
    c->em_cur = nxt;
    ++c->em_iter;
  }
  return PPLS_OK;
}

int ppls_em_state(ppls_ctx* c, ppls_theta* out, double* loglik, int cap, int* n_loglik) {
  if (!c) return PPLS_E_ARG;
  if (!c->em_active) return fail(c, PPLS_E_STATE, "call ppls_em_begin first");
  int rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = check_status(c))) return rc;
  if (out && (rc = download_theta(c, c->em_r, c->em_cur, out))) return rc;
  const int n = c->em_iter >= 1 ? c->em_iter - 1 : 0;
  if (n_loglik) *n_loglik = n;
  std::vector<double> l((size_t)n);
  if (n > 0) HIPCHK(c, hipMemcpy(l.data(), c->loglik, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (loglik && n > 0) std::copy(l.begin(), l.begin() + std::min(n, cap), loglik);
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(l[i]))
      return fail(c, PPLS_E_NUMERIC, "non-finite log-likelihood %g at EM iteration %d", l[i], i + 1);
  if (out && !theta_finite(out, c->p, c->q, c->em_r))
    return fail(c, PPLS_E_NUMERIC, "non-finite estimates after %d EM iterations", c->em_iter);
  return PPLS_OK;
}

int ppls_synchronize(ppls_ctx* c) {
  if (!c) return PPLS_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

int ppls_loglC_fast(ppls_ctx* c, const double* W, const double* C, const double* X, const double* Y, int64_t n,
                    int p, int q, int a, double sigX, double sigY, const double* sig2T, const double* c1,
                    const double* c2, const double* c3, const double* Kc, double* out) {
  if (!c || !W || !C || !sig2T || !c1 || !c2 || !c3 || !Kc || !out) return c ? fail(c, PPLS_E_ARG, "NULL argument") : PPLS_E_ARG;
  if (a < 1 || a > PPLS_RMAX) return fail(c, PPLS_E_ARG, "a=%d outside [1,%d]", a, PPLS_RMAX);
  int rc;
  if (X || Y) {
    if (!X || !Y) return fail(c, PPLS_E_ARG, "X and Y must both be given or both be NULL");
    if ((rc = ppls_set_data(c, X, Y, n, p, q, PPLS_LAYOUT_COLMAJOR, n))) return rc;
  } else if (!c->have_data || c->p != p || c->q != q) {
    return fail(c, PPLS_E_STATE, "no resident data of shape p=%d q=%d", p, q);
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, a, 1))) return rc;
  std::vector<double> B(a, 0.0), T(a, 1.0);
  ppls_theta th = {const_cast<double*>(W), const_cast<double*>(C), B.data(), T.data(), sigX, sigY, 0.0};
  if ((rc = upload_theta(c, &th, a, 0))) return rc;
  if ((rc = sweep(c, a, 0, false))) return rc;
  std::vector<double> cf(5 * (size_t)a);
  for (int k = 0; k < a; ++k) {
    cf[k] = sig2T[k]; cf[a + k] = c1[k]; cf[2 * a + k] = c2[k]; cf[3 * a + k] = c3[k]; cf[4 * a + k] = Kc[k];
  }
  HIPCHK(c, hipMemcpyAsync(c->coefs, cf.data(), sizeof(double) * cf.size(), hipMemcpyHostToDevice, c->stream));
  const double* G = c->stats + (int64_t)a * c->ldx + (int64_t)a * c->ldy;
  HIPCHK(c, ppls_launch_loglc(G, c->ssq, (double)c->n_total, p, q, a, sigX, sigY, c->coefs, c->loglik, c->stream));
  HIPCHK(c, hipMemcpyAsync(out, c->loglik, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

int ppls_xprod_prepare(ppls_ctx* c, double* ms, double* total_ms) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  HIPCHK(c, hipSetDevice(c->device));
  const bool was = c->xp_ready;
  int rc;
  if ((rc = xprod_setup(c))) return rc;
  c->xp_explicit = true;
  if (ms) *ms = was ? 0.0 : c->xp_setup_ms;
  if (total_ms) *total_ms = was ? 0.0 : c->xp_setup_total_ms;
  return PPLS_OK;
}

int ppls_xprod_release(ppls_ctx* c) {
  if (!c) return PPLS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  xprod_free(c);
  return PPLS_OK;
}

int ppls_xprod_get(ppls_ctx* c, double* S, int* P, int* ldx) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data || !c->xp_ready || !c->xp_S) return fail(c, PPLS_E_STATE, "no cross-products S are ready");
  const int PP = c->ldx + c->ldy;
  if (P) *P = PP;
  if (ldx) *ldx = c->ldx;
  if (S) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(S, c->xp_S, sizeof(double) * PP * PP, hipMemcpyDeviceToHost));
  }
  return PPLS_OK;
}

int ppls_xprod_setup_times(ppls_ctx* c, double* gram_ms, double* allreduce_ms, double* total_ms) {
  if (!c) return PPLS_E_ARG;
  if (gram_ms) *gram_ms = c->xp_setup_ms;
  if (allreduce_ms) *allreduce_ms = c->xp_setup_ar_ms;
  if (total_ms) *total_ms = c->xp_setup_total_ms;
  return PPLS_OK;
}

int ppls_xprod_tile_timing(ppls_ctx* c, int reps, double* ms) {
  if (!c || reps < 1 || !ms) return PPLS_E_ARG;
  if (!c->em_active || c->r_alloc != c->em_r) return fail(c, PPLS_E_STATE, "call ppls_em_begin first");
  if (!c->xp_ready || !c->xp_M) return fail(c, PPLS_E_STATE, "the cross-products S are not formed");
  HIPCHK(c, hipSetDevice(c->device));
  const int r = c->em_r, slot = c->em_cur, P = c->ldx + c->ldy;
  const int rw = ppls_xprod_tile_rows(P, r, c->xprod_rw, c->num_cus);
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0));
  HIPCHK(c, hipEventCreate(&e1));
  hipError_t e = hipEventRecord(e0, c->stream);
  for (int i = 0; e == hipSuccess && i < reps; ++i)   // the statistics of the current theta, rewritten
    e = ppls_launch_xprod_tile(c->xp_S, c->ldx, c->ldy, r, rw, c->W[slot], c->C[slot], c->sc[slot], c->stats,
                               c->xp_M, nullptr, 0, c->stream);
  if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float t = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIPCHK(c, e);
  *ms = (double)t / reps;
  return PPLS_OK;
}

int ppls_xprod_info(ppls_ctx* c, int r, int* ready, int64_t* bytes_per_pass, double* flops, int* rows_per_wave) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  const int64_t P = (int64_t)c->ldx + c->ldy;
  if (ready) *ready = c->xp_ready ? 1 : 0;
  if (bytes_per_pass) *bytes_per_pass = 8 * P * P;   // S's bytes one iteration reads
  if (flops) {   // lower 128 x 128 tiles incl. the diagonal ones, 2 flops per multiply-add
    const double nb = (double)((P + 127) / 128);
    flops[0] = 2.0 * (double)c->n_local * nb * (nb + 1) / 2.0 * 128.0 * 128.0;
  }
  if (rows_per_wave) *rows_per_wave = ppls_xprod_tile_rows((int)P, r < 1 ? 1 : r, c->xprod_rw, c->num_cus);
  return PPLS_OK;
}

int ppls_xprod_stats(ppls_ctx* c, const ppls_theta* th, int r, double* stats) {
  if (!c || !stats) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, 1))) return rc;
  if ((rc = upload_theta(c, th, r, 0))) return rc;
  if ((rc = xprod_stats(c, r, 0))) return rc;
  std::vector<double> st((size_t)c->part_ld);
  HIPCHK(c, hipMemcpyAsync(st.data(), c->stats, sizeof(double) * st.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < r; ++k) {
    for (int i = 0; i < c->p; ++i) stats[(size_t)k * c->p + i] = st[(size_t)k * c->ldx + i];
    for (int i = 0; i < c->q; ++i)
      stats[(size_t)r * c->p + (size_t)k * c->q + i] = st[(size_t)r * c->ldx + (size_t)k * c->ldy + i];
  }
  for (int e = 0; e < 4 * r * r; ++e)
    stats[(size_t)r * (c->p + c->q) + e] = st[(size_t)r * (c->ldx + c->ldy) + e];
  return PPLS_OK;
}

int ppls_sweep_stats(ppls_ctx* c, const ppls_theta* th, int r, int want_mu, double* stats, double* mu) {
  if (!c || !stats) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, 1))) return rc;
  if ((rc = upload_theta(c, th, r, 0))) return rc;
  if ((rc = sweep(c, r, 0, want_mu != 0))) return rc;
  std::vector<double> st((size_t)c->part_ld);
  HIPCHK(c, hipMemcpyAsync(st.data(), c->stats, sizeof(double) * st.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < r; ++k) {
    for (int i = 0; i < c->p; ++i) stats[(size_t)k * c->p + i] = st[(size_t)k * c->ldx + i];
    for (int i = 0; i < c->q; ++i)
      stats[(size_t)r * c->p + (size_t)k * c->q + i] = st[(size_t)r * c->ldx + (size_t)k * c->ldy + i];
  }
  for (int e = 0; e < 4 * r * r; ++e)
    stats[(size_t)r * (c->p + c->q) + e] = st[(size_t)r * (c->ldx + c->ldy) + e];
  if (want_mu && mu && c->n_local > 0)
    HIPCHK(c, hipMemcpy(mu, c->mu, sizeof(double) * (size_t)c->n_local * 2 * r, hipMemcpyDeviceToHost));
  return PPLS_OK;
}

int ppls_finalize_plan(ppls_ctx* c, int r, int type, int* templated, int* KX, int* KY, int* staged,
                       int64_t* stage_budget) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (r < 1 || r > PPLS_RMAX) return fail(c, PPLS_E_ARG, "bad r");
  HIPCHK(c, hipSetDevice(c->device));
  PplsFinalizeArgs f;
  int rc;
  if ((rc = finalize_args(c, r, 0, 1, -1, type, 0, &f))) return rc;
  PplsFinalizeGeometry g;
  HIPCHK(c, ppls_finalize_geometry(&f, &g));
  if (templated) *templated = g.templated;
  if (KX) *KX = g.KX;
  if (KY) *KY = g.KY;
  if (staged) *staged = g.staged;
  if (stage_budget) *stage_budget = (int64_t)g.stage_budget;
  return PPLS_OK;
}

int ppls_finalize_stats(ppls_ctx* c, const ppls_theta* th, int r, int type, int iter, const double* stats,
                        const double* gram_cur, const double* vstate_in, const double* xpM, int ldx, int ldy,
                        double* W_next, double* C_next, double* scalars, ppls_expect* mom, double* loglik,
                        double* gram_nxt, double* vstate_out, double* gram_stats, int* status3) {
  if (!c || !stats) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  if (type != PPLS_ORTH_SVD && type != PPLS_ORTH_QR) return fail(c, PPLS_E_ARG, "type must be SVD (0) or QR (1)");
  if (xpM && r > PPLS_FUSED_RMAX) return fail(c, PPLS_E_ARG, "the finalize forms the Gram from M for r <= 8 only");
  if (iter > (1 << 20)) return fail(c, PPLS_E_ARG, "iter too large");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, r, std::max(iter, 0) + 1))) return rc;
  if ((rc = upload_theta(c, th, r, 0))) return rc;   // W, C, scalars, their Gram; V = I
  if (ldx != c->ldx || ldy != c->ldy)
    return fail(c, PPLS_E_ARG, "the padded widths are %d and %d, not %d and %d", c->ldx, c->ldy, ldx, ldy);
  const int p = c->p, q = c->q, rr = r * r;
  {
    std::vector<double> st((size_t)c->part_ld, 0.0);   // padding rows 0, as the statistics steps leave them
    for (int k = 0; k < r; ++k) {
      for (int i = 0; i < p; ++i) st[(size_t)k * ldx + i] = stats[(size_t)k * p + i];
      for (int i = 0; i < q; ++i) st[(size_t)r * ldx + (size_t)k * ldy + i] = stats[(size_t)r * p + (size_t)k * q + i];
    }
    for (int e = 0; e < 4 * rr; ++e) st[(size_t)r * (ldx + ldy) + e] = stats[(size_t)r * (p + q) + e];
    HIPCHK(c, hipMemcpy(c->stats, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice));
  }
  if (gram_cur) HIPCHK(c, hipMemcpy(c->gram[0], gram_cur, sizeof(double) * 2 * rr, hipMemcpyHostToDevice));
  if (vstate_in) HIPCHK(c, hipMemcpy(c->vstate, vstate_in, sizeof(double) * 2 * rr, hipMemcpyHostToDevice));
  if (xpM) {
    const size_t P = (size_t)ldx + ldy;
    if (!c->xp_M && (rc = dalloc(c, &c->xp_M, P * 2 * PPLS_RMAX))) return rc;
    HIPCHK(c, hipMemcpy(c->xp_M, xpM, sizeof(double) * P * 2 * r, hipMemcpyHostToDevice));
  }
  // what the launch does not write shows: the next loadings start as NaN, the rest as 0
  HIPCHK(c, hipMemsetAsync(c->W[1], 0xff, sizeof(double) * (size_t)ldx * r, c->stream));
  HIPCHK(c, hipMemsetAsync(c->C[1], 0xff, sizeof(double) * (size_t)ldy * r, c->stream));
  HIPCHK(c, hipMemsetAsync(c->gram[1], 0, sizeof(double) * 2 * rr, c->stream));
  HIPCHK(c, hipMemsetAsync(c->status, 0, PPLS_STATUS_INTS * sizeof(int), c->stream));
  c->xp_pending_gram = xpM != nullptr;
  if ((rc = finalize(c, r, 0, 1, iter, type, 0, gram_cur == nullptr))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int st3[PPLS_STATUS_INTS];
  HIPCHK(c, hipMemcpy(st3, c->status, sizeof st3, hipMemcpyDeviceToHost));
  if (st3[0] == -7 && c->team_bar) HIPCHK(c, hipMemset(c->team_bar, 0, 8 * sizeof(unsigned)));
  if (status3) memcpy(status3, st3, sizeof st3);
  if (W_next) HIPCHK(c, hipMemcpy(W_next, c->W[1], sizeof(double) * (size_t)ldx * r, hipMemcpyDeviceToHost));
  if (C_next) HIPCHK(c, hipMemcpy(C_next, c->C[1], sizeof(double) * (size_t)ldy * r, hipMemcpyDeviceToHost));
  if (scalars) {   // [B r | sigT r | sigE sigF sigH | alpha r | beta r | gamma r | delta r]
    PplsScalars s;
    HIPCHK(c, hipMemcpy(&s, c->sc[1], sizeof s, hipMemcpyDeviceToHost));
    for (int k = 0; k < r; ++k) {
      scalars[k] = s.b[k];
      scalars[r + k] = s.t[k];
      scalars[2 * r + 3 + k] = s.alpha[k];
      scalars[3 * r + 3 + k] = s.beta[k];
      scalars[4 * r + 3 + k] = s.gamma[k];
      scalars[5 * r + 3 + k] = s.delta[k];
    }
    scalars[2 * r] = s.sigE;
    scalars[2 * r + 1] = s.sigF;
    scalars[2 * r + 2] = s.sigH;
  }
  if ((rc = download_moments(c, r, mom))) return rc;
  if (loglik && iter >= 0) HIPCHK(c, hipMemcpy(loglik, c->loglik + iter, sizeof(double), hipMemcpyDeviceToHost));
  if (gram_nxt) HIPCHK(c, hipMemcpy(gram_nxt, c->gram[1], sizeof(double) * 2 * rr, hipMemcpyDeviceToHost));
  if (vstate_out) HIPCHK(c, hipMemcpy(vstate_out, c->vstate, sizeof(double) * 2 * rr, hipMemcpyDeviceToHost));
  if (gram_stats)
    HIPCHK(c, hipMemcpy(gram_stats, c->stats + (size_t)r * (ldx + ldy), sizeof(double) * 4 * rr, hipMemcpyDeviceToHost));
  return PPLS_OK;
}

int ppls_sweep_timing(ppls_ctx* c, double* total_ms, int64_t* launches, int reset) {
  if (!c) return PPLS_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < c->ev_used; ++i) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[i].first, c->ev[i].second));
    c->timed_ms += ms;
    ++c->timed_launches;
  }
  c->ev_used = 0;
  if (total_ms) *total_ms = c->timed_ms;
  if (launches) *launches = c->timed_launches;
  if (reset) { c->timed_ms = 0.0; c->timed_launches = 0; }
  return PPLS_OK;
}

int ppls_sweep_balance(ppls_ctx* c, double* w8, int64_t* bounds, int cap, int* n_bounds) {
  if (!c) return PPLS_E_ARG;
  if (w8)
    for (int x = 0; x < 8; ++x) w8[x] = c->bal_done ? c->bal_w[x] : 1.0;
  const int nb = c->bal_done ? c->bal_grid + 1 : 0;
  if (n_bounds) *n_bounds = nb;
  if (bounds && cap > 0 && nb > 0)
    HIPCHK(c, hipMemcpy(bounds, c->bal_bounds, sizeof(int64_t) * (size_t)std::min(cap, nb), hipMemcpyDeviceToHost));
  return PPLS_OK;
}

int ppls_comm_info(ppls_ctx* c, int* nranks, int* rank, double* allreduce_ms, int64_t* allreduce_calls,
                   int reset) {
  if (!c) return PPLS_E_ARG;
  int nr = c->nranks, rk = c->rank;
  if (c->comm) {   // what RCCL itself reports for the communicator
    RCCLCHK(c, ncclCommCount(c->comm, &nr));
    RCCLCHK(c, ncclCommUserRank(c->comm, &rk));
  }
  if (nranks) *nranks = nr;
  if (rank) *rank = rk;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < c->ev_ar_used; ++i) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_ar[i].first, c->ev_ar[i].second));
    c->ar_ms += ms;
    ++c->ar_calls;
  }
  c->ev_ar_used = 0;
  if (allreduce_ms) *allreduce_ms = c->ar_ms;
  if (allreduce_calls) *allreduce_calls = c->ar_calls;
  if (reset) { c->ar_ms = 0.0; c->ar_calls = 0; }
  return PPLS_OK;
}

int ppls_sweep_info(ppls_ctx* c, int r, int64_t* bytes_per_sweep, int* variant, int* grid) {
  if (!c) return PPLS_E_ARG;
  PplsSweepArgs a;
  const int plan = sweep_plan(c, r, &a);
  if (bytes_per_sweep) *bytes_per_sweep = (int64_t)(c->dtype ? 4 : 8) * c->n_local * ((int64_t)c->p + c->q);
  if (variant) *variant = plan == 4 ? 5 : plan == 3 ? 4 : 2;
  if (grid) *grid = a.grid;
  return PPLS_OK;
}

int ppls_gram_int8(ppls_ctx* c, int which, double* G, int* nmod, int* L, double* ms) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (which < 0 || which > 2) return fail(c, PPLS_E_ARG, "which must be 0 (X), 1 (Y) or 2 (joint [X Y])");
  if (c->n_local <= 0) return fail(c, PPLS_E_STATE, "no rows on this rank");
  HIPCHK(c, hipSetDevice(c->device));
  const GramShape g = which == 2 ? gram_shape(c, true, 0) : gram_shape(c, false, which);
  const size_t pp = (size_t)g.p * g.p;
  int rc;
  double* dG = nullptr;
  if ((rc = dalloc(c, &dG, pp))) return rc;
  float t = 0.f;
  rc = gram_run_oz(c, g, c->n_local, dG, &t);
  if (nmod) *nmod = c->oz_nmod;
  if (L) *L = c->oz_L;
  if (rc == 1) rc = fail(c, PPLS_E_NUMERIC, "int8 Gram: the column spread needs L = %d bits or more than %d moduli, "
                         "or the residue planes do not fit", c->oz_L, PPLS_OZ_MAXMOD);
  if (!rc && G && hipMemcpy(G, dG, sizeof(double) * pp, hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, PPLS_E_HIP, "int8 gram: copy-out failed");
  dfree(dG);
  if (!rc && ms) for (int k = 0; k < 4; ++k) ms[k] = c->oz_ms[k];
  return rc;
}

int ppls_gram_shifts(ppls_ctx* c, int* shift, int P, int* count) {
  if (!c) return PPLS_E_ARG;
  const int k = (int)c->oz_shift.size();
  if (count) *count = k;
  if (shift) for (int j = 0; j < std::min(P, k); ++j) shift[j] = c->oz_shift[(size_t)j];
  return PPLS_OK;
}

int ppls_gram_info(ppls_ctx* c, int* int8_used, int* nmod, int* L, double* ms) {
  if (!c) return PPLS_E_ARG;
  if (int8_used) *int8_used = c->oz_used;
  if (nmod) *nmod = c->oz_nmod;
  if (L) *L = c->oz_L;
  if (ms) for (int k = 0; k < 4; ++k) ms[k] = c->oz_ms[k];
  return PPLS_OK;
}

int ppls_meta_info(ppls_ctx* c, int* path) {
  if (!c || !path) return PPLS_E_ARG;
  *path = c->meta_path;
  return PPLS_OK;
}

int ppls_sweep_kernel(ppls_ctx* c, int r, char* buf, int len) {
  if (!c || !buf || len < 1) return PPLS_E_ARG;
  if (r < 1 || r > PPLS_RMAX) return fail(c, PPLS_E_ARG, "bad r");
  PplsSweepArgs a;
  const int plan = sweep_plan(c, r, &a);
  const int nt = c->nt_loads > 0 ||
                 (c->nt_loads < 0 && 8.0 * sweep_rows(c) * (double)(c->ldx + c->ldy) > 256.0 * (1 << 20));
  char k[128];
  if (plan == 3) {
    if (ppls_split_describe(&a, k, sizeof k) != 0) return fail(c, PPLS_E_STATE, "no split instantiation for r=%d", r);
  } else {
    // as ppls_kernels.hip launch_panel_t picks them
    const bool rows64 = c->dots_rows ? c->dots_rows == 64 : sweep_rows(c) >= 32768;
    const int64_t wtiles = (sweep_rows(c) + (rows64 ? 63 : 31)) / (rows64 ? 64 : 32);
    const bool pair = c->dots_pair >= 0 ? c->dots_pair == 1 : wtiles < (int64_t)c->num_cus * 4 * (rows64 ? 2 : 3);
    snprintf(k, sizeof k, "panel<%s,%d> (mfmadots %d rows/%s + acc, %d chunks)", c->dtype ? "float" : "double", r,
             rows64 ? 64 : 32, pair ? "wave pair" : "wave", a.grid);
  }
  snprintf(buf, (size_t)len, "%s%s", k, plan == 3 && nt ? " nt" : "");
  return PPLS_OK;
}

int ppls_finalize_trace(ppls_ctx* c, int64_t* stamps, double* tick_ns) {
  if (!c || !stamps) return PPLS_E_ARG;
  if (!c->ftrace) return fail(c, PPLS_E_STATE, "finalize tracing is off (set_option ftrace 1)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(stamps, c->ftrace, PPLS_FTRACE_LEN * sizeof(long long), hipMemcpyDeviceToHost));
  if (tick_ns) {
    int khz = 0;
    HIPCHK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    *tick_ns = khz > 0 ? 1e6 / khz : 0.0;
  }
  return PPLS_OK;
}

int ppls_sweep_trace(ppls_ctx* c, int64_t* stamps, int cap, int* n, double* tick_ns) {
  if (!c || !stamps || !n) return PPLS_E_ARG;
  if (!c->strace) return fail(c, PPLS_E_STATE, "sweep tracing is off (set_option strace 1)");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int m = std::min(cap, PPLS_STRACE_MAX_WG);
  HIPCHK(c, hipMemcpy(stamps, c->strace, (size_t)m * 4 * sizeof(long long), hipMemcpyDeviceToHost));
  *n = m;
  if (tick_ns) {
    int khz = 0;
    HIPCHK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    *tick_ns = khz > 0 ? 1e6 / khz : 0.0;
  }
  return PPLS_OK;
}

int ppls_mu_coefficients(const ppls_theta* th, int r, double* coef) {
  if (!th || !th->B || !th->sigT || !coef || r < 1 || r > PPLS_RMAX) return PPLS_E_ARG;
  PplsScalars s = scalars_of(th, r);
  for (int k = 0; k < r; ++k) {
    coef[k] = s.alpha[k]; coef[r + k] = s.beta[k]; coef[2 * r + k] = s.gamma[k]; coef[3 * r + k] = s.delta[k];
  }
  return PPLS_OK;
}

int ppls_finalize_host(const double* SX, const double* SY, const double* G, double ssqX, double ssqY, double N,
                       int p, int q, int r, const ppls_theta* th, int type, ppls_theta* next,
                       ppls_expect* mom_out, double* loglik) {
  if (!G || !th || !th->W || !th->C || !th->B || !th->sigT || r < 1 || r > PPLS_RMAX || p < 1 || q < 1)
    return PPLS_E_ARG;
  PplsScalars s = scalars_of(th, r);
  double WtW[PPLS_RMAX * PPLS_RMAX], CtC[PPLS_RMAX * PPLS_RMAX];
  for (int a = 0; a < r; ++a)
    for (int b = 0; b < r; ++b) {
      double w = 0.0, cc = 0.0;
      for (int i = 0; i < p; ++i) w += th->W[(size_t)a * p + i] * th->W[(size_t)b * p + i];
      for (int i = 0; i < q; ++i) cc += th->C[(size_t)a * q + i] * th->C[(size_t)b * q + i];
      WtW[b * r + a] = w;
      CtC[b * r + a] = cc;
    }
  if (loglik) *loglik = ppls_loglik_from_gram(G, ssqX, ssqY, N, p, q, r, &s);
  PplsMoments m;
  ppls_estep_moments(G, WtW, CtC, ssqX, ssqY, N, p, q, r, &s, &m);
  if (mom_out) {
    for (int k = 0; k < r; ++k) {
      if (mom_out->Ctt) mom_out->Ctt[k] = m.Ctt[k];
      if (mom_out->Cuu) mom_out->Cuu[k] = m.Cuu[k];
      if (mom_out->Cut) mom_out->Cut[k] = m.Cut[k];
    }
    mom_out->Cee = m.Cee;
    mom_out->Cff = m.Cff;
    if (mom_out->Chh) memcpy(mom_out->Chh, m.Chh, sizeof(double) * r * r);
  }
  if (next) {
    PplsScalars nx = s;
    ppls_mstep_scalars(&m, r, &nx);
    if (next->B) for (int k = 0; k < r; ++k) next->B[k] = nx.b[k];
    if (next->sigT) for (int k = 0; k < r; ++k) next->sigT[k] = nx.t[k];
    next->sigE = nx.sigE;
    next->sigF = nx.sigF;
    next->sigH = nx.sigH;
    if (next->W && SX && host_orth(SX, p, r, type, next->W) != PPLS_OK) return PPLS_E_NUMERIC;
    if (next->C && SY && host_orth(SY, q, r, type, next->C) != PPLS_OK) return PPLS_E_NUMERIC;
  }
  return PPLS_OK;
}

}  // extern "C"

// ============================================================================ cross-validation
// predict.PPLS, cv_PPLS and crossval_PPLS (Package/PPLS/R/crossval_PPLS.R:12-114) on the device:
// a fold's training rows are gathered from the resident data into a second context (no host round
// trip), its cross-products are S - S_fold, and the held-out rows are scored where they lie.
namespace {

// Device temporaries of one call, freed on every return path.
struct CvScratch {
  std::vector<void*> ptrs;
  ~CvScratch() {
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
  }
  template <typename T>
  int get(ppls_ctx* c, T** out, size_t count) {
    *out = nullptr;
    const int rc = dalloc(c, out, count);
    if (!rc) ptrs.push_back(*out);
    return rc;
  }
};

// A HIP-event bracket on one stream; ms() after the stream was synchronised.
struct CvEvents {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~CvEvents() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  hipError_t begin(hipStream_t st) {
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    return e;
  }
  hipError_t end(hipStream_t st) { return hipEventRecord(e1, st); }
  double ms() {
    float f = 0.f;
    return hipEventElapsedTime(&f, e0, e1) == hipSuccess ? (double)f : 0.0;
  }
};

// Local row indices into a context's resident rows: in [0, limit), strictly ascending.
int cv_check_rows(ppls_ctx* c, const int64_t* rows, int64_t nrows, int64_t limit) {
  if (nrows < 0 || (nrows > 0 && !rows)) return fail(c, PPLS_E_ARG, "row list: %lld rows, NULL indices", (long long)nrows);
  for (int64_t i = 0; i < nrows; ++i) {
    if (rows[i] < 0 || rows[i] >= limit)
      return fail(c, PPLS_E_ARG, "row index %lld (entry %lld) outside [0, %lld)", (long long)rows[i], (long long)i,
                  (long long)limit);
    if (i > 0 && rows[i] <= rows[i - 1])
      return fail(c, PPLS_E_ARG, "row indices must be strictly ascending (entries %lld, %lld)", (long long)(i - 1),
                  (long long)i);
  }
  return PPLS_OK;
}

int cv_upload_rows(ppls_ctx* c, CvScratch& tmp, const int64_t* rows, int64_t nrows, int64_t** d_rows) {
  int rc;
  if ((rc = tmp.get(c, d_rows, (size_t)std::max<int64_t>(nrows, 1)))) return rc;
  if (nrows > 0) HIPCHK(c, hipMemcpy(*d_rows, rows, sizeof(int64_t) * nrows, hipMemcpyHostToDevice));
  return PPLS_OK;
}

// Rows d_rows of s's resident X, Y into X, Y (rows of ldx / ldy elements of s's storage type): the
// 16-byte units that hold real columns are copied (s's padding inside them is zero), the rest zeroed.
hipError_t cv_gather(const ppls_ctx* s, const int64_t* d_rows, int64_t nrows, void* X, void* Y, int ldx, int ldy,
                     hipStream_t st) {
  const int64_t es = s->dtype ? 4 : 8;
  hipError_t e = ppls_launch_gather_rows(s->X, s->ldx * es / 16, X, ldx * es / 16, (int)((s->p * es + 15) / 16), d_rows,
                                         nrows, st);
  if (e == hipSuccess)
    e = ppls_launch_gather_rows(s->Y, s->ldy * es / 16, Y, ldy * es / 16, (int)((s->q * es + 15) / 16), d_rows, nrows, st);
  return e;
}

double cv_gather_bytes(const ppls_ctx* s, int64_t nrows, int ldx, int ldy) {   // read + written
  const double es = s->dtype ? 4.0 : 8.0;
  return (double)nrows * es * ((double)s->p + s->q + ldx + ldy);
}

// M (rowsM x k column-major) zero-padded to ((rowsM + 3) & ~3) x k on the device.
int cv_upload_coef(ppls_ctx* c, CvScratch& tmp, const double* M, int rowsM, int k, double** out) {
  const int ld4 = (rowsM + 3) & ~3;
  std::vector<double> h((size_t)ld4 * k, 0.0);
  for (int m = 0; m < k; ++m) memcpy(&h[(size_t)m * ld4], M + (size_t)m * rowsM, sizeof(double) * rowsM);
  int rc;
  if ((rc = tmp.get(c, out, h.size()))) return rc;
  HIPCHK(c, hipMemcpy(*out, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_set_data_from(ppls_ctx* dst, ppls_ctx* src, const int64_t* rows, int64_t nrows, int64_t n_total) {
  int rc;
  if ((rc = pair_check(dst, src))) return rc;
  if (!src->have_data) return fail(dst, PPLS_E_ARG, "the source context has no data");
  if (src->st_state == 2) return fail(dst, PPLS_E_STATE, PPLS_STREAMED_MSG);
  if ((rc = cv_check_rows(dst, rows, nrows, src->n_local))) return rc;
  if (n_total > 0 && n_total < nrows) return fail(dst, PPLS_E_ARG, "n_total=%lld < %lld local rows", (long long)n_total, (long long)nrows);
  HIPCHK(dst, hipSetDevice(dst->device));
  CvScratch tmp;
  int64_t* d_rows = nullptr;
  if ((rc = cv_upload_rows(dst, tmp, rows, nrows, &d_rows))) return rc;
  dst->dtype = src->dtype;
  if ((rc = alloc_data(dst, nrows, src->p, src->q, n_total))) return rc;
  // the slack of dst's new buffers is zeroed on dst's stream, the gather reads src: it runs on src's
  // stream, behind whatever src still has queued
  HIPCHK(dst, hipStreamSynchronize(dst->stream));
  CvEvents ev;
  HIPCHK(dst, ev.begin(src->stream));
  HIPCHK(dst, cv_gather(src, d_rows, nrows, dst->X, dst->Y, dst->ldx, dst->ldy, src->stream));
  HIPCHK(dst, ev.end(src->stream));
  HIPCHK(dst, hipStreamSynchronize(src->stream));
  src->cv_ms[0] += ev.ms();
  src->cv_bytes[0] += cv_gather_bytes(src, nrows, dst->ldx, dst->ldy);
  dst->have_data = true;
  record_copy(dst, src);   // the rows keep the transform they carry in src (ppls_scale_data, ppls_adjust_data)
  if ((rc = compute_ssq(dst))) return rc;   // drops a stale S; collective when sharded (also with no rows)
  return check_finite_data(dst);
}

int ppls_xprod_downdate(ppls_ctx* dst, ppls_ctx* src, const int64_t* out_rows, int64_t n_out) {
  int rc;
  if ((rc = pair_check(dst, src))) return rc;
  if (!src->have_data || !dst->have_data) return fail(dst, PPLS_E_STATE, "no data");
  if (src->st_state == 2 || dst->st_state == 2) return fail(dst, PPLS_E_STATE, PPLS_STREAMED_MSG);
  if (dst->p != src->p || dst->q != src->q || dst->ldx != src->ldx || dst->ldy != src->ldy || dst->dtype != src->dtype)
    return fail(dst, PPLS_E_ARG, "the contexts' data differ in shape, padding or storage type");
  HIPCHK(dst, hipSetDevice(src->device));
  // S of all rows first (a collective of its own when sharded: every rank is here)
  if ((rc = xprod_setup(src))) {
    dst->err = src->err;
    return rc;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const bool coll = collective(src);
  const int P = src->ldx + src->ldy;
  const size_t PP = (size_t)P * P;
  // this rank's verdict on its arguments joins the agreement below, so that ranks return together
  int bad = cv_check_rows(dst, out_rows, n_out, src->n_local);
  if (!bad && dst->n_local != src->n_local - n_out)
    bad = fail(dst, PPLS_E_ARG, "row counts: %lld resident - %lld held out != %lld training rows on this rank",
               (long long)src->n_local, (long long)n_out, (long long)dst->n_local);
  const std::string bad_err = dst->err;
  if (bad && !coll) return bad;
  // every allocation of the call, then the ranks agree that all of them succeeded before anyone
  // enters the all-reduce of the held-out Gram (as xprod_setup does for S)
  CvScratch tmp;
  int64_t* d_rows = nullptr;
  double *gX = nullptr, *gY = nullptr, *Gout = nullptr, *part = nullptr;
  const int64_t no = bad ? 0 : n_out;
  const size_t es = src->dtype ? 4 : 8;
  const size_t xb = (size_t)std::max<int64_t>(no, 1) * src->ldx * es, yb = (size_t)std::max<int64_t>(no, 1) * src->ldy * es;
  const GramShape g{P, src->p, src->ldx, src->q, nullptr, src->ldx, nullptr, src->ldy, src->ldy};
  xprod_free(dst);
  DevGuard Snew;   // dst's S once the call has succeeded
  int rc_alloc = dalloc(dst, &Snew.p, PP);
  if (!rc_alloc) rc_alloc = tmp.get(src, &Gout, PP);
  if (!rc_alloc) rc_alloc = cv_upload_rows(src, tmp, out_rows, no, &d_rows);
  if (!rc_alloc) rc_alloc = tmp.get(src, &gX, (xb + 7) / 8 + 64);
  if (!rc_alloc) rc_alloc = tmp.get(src, &gY, (yb + 7) / 8 + 64);
  if (!rc_alloc && no > 0) {
    int* q = nullptr;
    rc_alloc = tmp.get(src, &part, (size_t)ppls_gram_part_doubles(P, gram_nsplit(src, g, no, 0)));
    if (!rc_alloc) rc_alloc = gram_queue(src, g, no, 0, &q);
  }
  if (rc_alloc && !coll && dst->err.empty()) dst->err = src->err;
  double n_out_total = (double)no;
  const AgreeSpec sp{"downdate of S", "S, the held-out rows or their Gram", "bad held-out rows", false, false};
  if ((rc = ranks_agree(dst, src, sp, rc_alloc, bad, bad_err, &n_out_total))) return rc;
  // the totals every rank shares: held out + training = all rows, and no more held out than kept
  // (beyond that S - S_out loses more than a direct Gram of the training rows: form S directly)
  if (n_out_total != (double)(src->n_total - dst->n_total) || n_out_total > (double)dst->n_total)
    return fail(dst, PPLS_E_ARG, "row counts over all ranks: %lld rows, %.0f held out, %lld training rows%s",
                (long long)src->n_total, n_out_total, (long long)dst->n_total,
                n_out_total > (double)dst->n_total ? " (more held out than kept: form S directly)" : "");
  hipError_t e = hipMemsetAsync((char*)gX + xb, 0, ((xb + 7) / 8 + 64) * 8 - xb, src->stream);
  if (e == hipSuccess) e = hipMemsetAsync((char*)gY + yb, 0, ((yb + 7) / 8 + 64) * 8 - yb, src->stream);
  CvEvents ev;
  if (e == hipSuccess) e = ev.begin(src->stream);
  if (e == hipSuccess) e = cv_gather(src, d_rows, no, gX, gY, src->ldx, src->ldy, src->stream);
  if (e == hipSuccess) e = ev.end(src->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(src->stream);
  if (e != hipSuccess) return fail(dst, PPLS_E_HIP, "held-out gather: %s", hipGetErrorString(e));
  const double gather_ms = ev.ms();
  src->cv_ms[0] += gather_ms;
  src->cv_bytes[0] += cv_gather_bytes(src, no, src->ldx, src->ldy);
  if (no > 0) {
    GramShape gs = g;
    gs.X = gX;
    gs.Y = gY;
    const int oz_used = src->oz_used;   // src's record of how its own S was formed stays
    rc = gram_run_s(src, gs, no, Gout, nullptr, part);
    src->oz_used = oz_used;
    if (rc) { dst->err = src->err; return rc; }
  } else {
    HIPCHK(dst, hipMemsetAsync(Gout, 0, sizeof(double) * PP, src->stream));
  }
  if ((rc = allreduce(src, Gout, PP))) { dst->err = src->err; return rc; }
  e = ppls_launch_downdate(src->xp_S, Gout, Snew.p, (int64_t)PP, src->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(src->stream);
  if (e != hipSuccess) return fail(dst, PPLS_E_HIP, "downdate of S: %s", hipGetErrorString(e));
  dst->xp_S = Snew.release();
  derived_publish(dst, dst->n_total, dst->mem_free_min);   // (the training rows stay as they are)
  src->cv_ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - gather_ms;
  return PPLS_OK;
}

int ppls_predict(ppls_ctx* c, const double* W, const double* C, const double* B, int k, int xory, const double* newdata,
                 int64_t n, int layout, double* pred) {
  if (!c) return PPLS_E_ARG;
  if (c->p < 1 || c->q < 1) return fail(c, PPLS_E_STATE, "no data shape: load data (p, q) first");
  if (!W || !C || !B || k < 1 || k > PPLS_RMAX) return fail(c, PPLS_E_ARG, "W, C, B must be given with 1 <= k <= %d", PPLS_RMAX);
  if (xory != 0 && xory != 1) return fail(c, PPLS_E_ARG, "xory must be 0 (newdata is X) or 1 (Y)");
  if (layout != PPLS_LAYOUT_COLMAJOR && layout != PPLS_LAYOUT_ROWMAJOR)
    return fail(c, PPLS_E_ARG, "layout must be 0 (column-major) or 1 (row-major)");
  if (n < 0 || (n > 0 && (!newdata || !pred))) return fail(c, PPLS_E_ARG, "NULL newdata or pred");
  if (n == 0) return PPLS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  // newdata W diag(B) C' (X) or newdata C diag(1/B) W' (Y), crossval_PPLS.R:19-21
  const int pa = xory ? c->q : c->p, qb = xory ? c->p : c->q;
  const int lda = (pa + 1) & ~1, ldo = (qb + 1) & ~1;
  std::vector<double> s(k);
  for (int m = 0; m < k; ++m) s[m] = xory ? 1.0 / B[m] : B[m];
  int rc;
  CvScratch tmp;
  double *A = nullptr, *Bm = nullptr, *sd = nullptr, *in = nullptr, *out = nullptr, *cm = nullptr;
  if ((rc = cv_upload_coef(c, tmp, xory ? C : W, pa, k, &A))) return rc;
  if ((rc = cv_upload_coef(c, tmp, xory ? W : C, qb, k, &Bm))) return rc;
  if ((rc = cv_upload_coef(c, tmp, s.data(), k, 1, &sd))) return rc;
  // row blocks of newdata through a staging buffer (~64 MB of input rows at a time)
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(64 << 20) / (8LL * std::max(lda, ldo))));
  if ((rc = tmp.get(c, &in, (size_t)chunk * lda))) return rc;
  if ((rc = tmp.get(c, &out, (size_t)chunk * ldo))) return rc;
  if ((rc = tmp.get(c, &cm, (size_t)chunk * std::max(pa, qb)))) return rc;
  HIPCHK(c, hipMemsetAsync(in, 0, sizeof(double) * chunk * lda, c->stream));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nc = std::min(chunk, n - r0);
    if (layout == PPLS_LAYOUT_ROWMAJOR) {
      HIPCHK(c, hipMemcpy2DAsync(in, sizeof(double) * lda, newdata + r0 * pa, sizeof(double) * pa, sizeof(double) * pa, nc,
                                 hipMemcpyHostToDevice, c->stream));
    } else {
      HIPCHK(c, hipMemcpy2DAsync(cm, sizeof(double) * nc, newdata + r0, sizeof(double) * n, sizeof(double) * nc, pa,
                                 hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, ppls_launch_to_rowmajor(cm, nc, pa, lda, in, c->stream));
    }
    HIPCHK(c, ppls_launch_cv_score(in, lda, pa, nullptr, 0, qb, 0, nullptr, nc, A, Bm, sd, k, nullptr, out, ldo,
                                   ppls_cv_grid(nc, k, c->num_cus), c->stream));
    HIPCHK(c, ppls_launch_to_colmajor(out, nc, qb, ldo, cm, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(pred + r0, sizeof(double) * n, cm, sizeof(double) * nc, sizeof(double) * nc, qb,
                          hipMemcpyDeviceToHost));
  }
  return PPLS_OK;
}

int ppls_heldout_sse(ppls_ctx* c, const double* W, const double* C, const double* B, int k, const int64_t* rows,
                     int64_t nrows, double* sse) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!W || !C || !B || !sse || k < 1 || k > PPLS_RMAX)
    return fail(c, PPLS_E_ARG, "W, C, B, sse must be given with 1 <= k <= %d", PPLS_RMAX);
  int rc;
  if ((rc = cv_check_rows(c, rows, nrows, c->n_local))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  double *A = nullptr, *Bm = nullptr, *sd = nullptr, *part = nullptr, *tot = nullptr;
  int64_t* d_rows = nullptr;
  const int grid = ppls_cv_grid(nrows, k, c->num_cus);
  const int nparts = grid * PPLS_CV_WAVES;
  if ((rc = cv_upload_coef(c, tmp, W, c->p, k, &A))) return rc;
  if ((rc = cv_upload_coef(c, tmp, C, c->q, k, &Bm))) return rc;
  if ((rc = cv_upload_coef(c, tmp, B, k, 1, &sd))) return rc;
  if ((rc = cv_upload_rows(c, tmp, rows, nrows, &d_rows))) return rc;
  if ((rc = tmp.get(c, &part, (size_t)nparts * k))) return rc;
  if ((rc = tmp.get(c, &tot, (size_t)k))) return rc;
  CvEvents ev;
  HIPCHK(c, ev.begin(c->stream));
  // (a rank with no held-out row launches too: its waves write zero partials)
  HIPCHK(c, ppls_launch_cv_score(c->X, c->ldx, c->p, c->Y, c->ldy, c->q, c->dtype, d_rows, nrows, A, Bm, sd, k, part,
                                 nullptr, 0, grid, c->stream));
  HIPCHK(c, ppls_launch_cv_sse_reduce(part, nparts, k, tot, c->stream));
  HIPCHK(c, ev.end(c->stream));
  if ((rc = allreduce(c, tot, (size_t)k))) return rc;
  HIPCHK(c, hipMemcpyAsync(sse, tot, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->cv_ms[3] += ev.ms();
  c->cv_bytes[1] += (double)nrows * (c->dtype ? 4.0 : 8.0) * ((double)c->p + c->q);
  return PPLS_OK;
}

}  // extern "C"

// ============================================================================ row diagnostics
// Per row: the squared Mahalanobis distance under the fitted covariance, split into the in-plane
// score distance and the two orthogonal distances, the log-density and Expect_M's posterior means
// (ppls_rowdiag.hip).  The kernel writes odx2, ody2, sd2 (and mu); d2 and the
// log-density follow here, O(n).
namespace {

struct RowDiagFit {
  double *W = nullptr, *C = nullptr, *coef = nullptr;   // device: padded loadings, PPLS_ROWDIAG_COEF x 16
  double sE2 = 1.0, sF2 = 1.0, cst = 0.0;               // loglik_i = cst - d2_i / 2
  double logdet = 0.0;   // (p - r) log sigE^2 + (q - r) log sigF^2 + sum_k log det_k
};

// Everything ppls_row_diagnostics{,_new} refuse about the fit, before any device work.
int rowdiag_check_fit(ppls_ctx* c, const ppls_theta* th, int r, double (&h)[PPLS_ROWDIAG_COEF * 16], RowDiagFit& f) {
  int rc;
  if ((rc = check_theta(c, th, r))) return rc;
  if (r > std::min(c->p, c->q)) return fail(c, PPLS_E_ARG, "r=%d components for %d x %d columns", r, c->p, c->q);
  if (!theta_finite(th, c->p, c->q, r)) return fail(c, PPLS_E_ARG, "theta has non-finite entries");
  const PplsScalars s = scalars_of(th, r);
  f.sE2 = th->sigE * th->sigE;
  f.sF2 = th->sigF * th->sigF;
  memset(h, 0, sizeof h);
  double logdet = 0.0;
  for (int k = 0; k < r; ++k) {
    const double t2 = th->sigT[k] * th->sigT[k], b = th->B[k];
    const double s11 = t2 + f.sE2, s12 = b * t2, s22 = b * b * t2 + th->sigH * th->sigH + f.sF2;
    // det = s11 s22 - s12^2 without the cancellation: every term is non-negative
    const double det = t2 * (th->sigH * th->sigH + f.sF2) + f.sE2 * s22;
    if (!(det > 0.0) || !std::isfinite(det))
      return fail(c, PPLS_E_ARG, "component %d: the 2 x 2 score covariance has determinant %g, not above 0", k + 1, det);
    h[0 * 16 + k] = s11; h[1 * 16 + k] = s12; h[2 * 16 + k] = s22; h[3 * 16 + k] = det;
    h[4 * 16 + k] = s.alpha[k]; h[5 * 16 + k] = s.beta[k]; h[6 * 16 + k] = s.gamma[k]; h[7 * 16 + k] = s.delta[k];
    logdet += std::log(det);
  }
  if (!(f.sE2 > 0.0) || !(f.sF2 > 0.0) || !std::isfinite(f.sE2) || !std::isfinite(f.sF2))
    return fail(c, PPLS_E_ARG, "sigE^2 = %g, sigF^2 = %g must be positive and finite", f.sE2, f.sF2);
  f.cst = -0.5 * ((double)(c->p + c->q) * std::log(6.283185307179586) + (double)(c->p - r) * std::log(f.sE2) +
                  (double)(c->q - r) * std::log(f.sF2) + logdet);
  f.logdet = ((double)(c->p - r) * std::log(f.sE2) + (double)(c->q - r) * std::log(f.sF2)) + logdet;
  return PPLS_OK;
}

int rowdiag_upload_fit(ppls_ctx* c, CvScratch& tmp, const ppls_theta* th, int r, const double (&h)[PPLS_ROWDIAG_COEF * 16],
                       RowDiagFit& f) {
  int rc;
  if ((rc = cv_upload_coef(c, tmp, th->W, c->p, r, &f.W))) return rc;
  if ((rc = cv_upload_coef(c, tmp, th->C, c->q, r, &f.C))) return rc;
  return cv_upload_coef(c, tmp, h, PPLS_ROWDIAG_COEF * 16, 1, &f.coef);
}

// Device results of `count` rows (odx2 | ody2 | sd2, `count` each, then mu_T | mu_U with leading
// dimension `count`) into the caller's arrays at row offset `at` of `n`.
int rowdiag_collect(ppls_ctx* c, const RowDiagFit& f, const double* dres, const double* dmu, int64_t count, int r,
                    int64_t at, int64_t n, ppls_row_diag* out) {
  if (count <= 0) return PPLS_OK;
  std::vector<double> h((size_t)3 * count);
  HIPCHK(c, hipMemcpy(h.data(), dres, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  const double *ox = h.data(), *oy = ox + count, *sd = oy + count;
  for (int64_t i = 0; i < count; ++i) {
    const double d2 = (ox[i] / f.sE2 + oy[i] / f.sF2) + sd[i];
    if (out->odx2) out->odx2[at + i] = ox[i];
    if (out->ody2) out->ody2[at + i] = oy[i];
    if (out->sd2) out->sd2[at + i] = sd[i];
    if (out->d2) out->d2[at + i] = d2;
    if (out->loglik) out->loglik[at + i] = f.cst - 0.5 * d2;
  }
  if (dmu) {
    if (out->mu_T)
      HIPCHK(c, hipMemcpy2D(out->mu_T + at, sizeof(double) * n, dmu, sizeof(double) * count, sizeof(double) * count, r,
                            hipMemcpyDeviceToHost));
    if (out->mu_U)
      HIPCHK(c, hipMemcpy2D(out->mu_U + at, sizeof(double) * n, dmu + (size_t)count * r, sizeof(double) * count,
                            sizeof(double) * count, r, hipMemcpyDeviceToHost));
  }
  return PPLS_OK;
}

// The device stage of ppls_row_diagnostics on the resident rows, queued on the context stream with no
// copy-out: the fit uploaded, then the kernel.  res = [odx2 | ody2 | sd2] (nrows each) and, with mu, dmu
// = [mu_T | mu_U]; both live in tmp.  d_rows: device indices or nullptr (rows 0 .. nrows - 1).
int rowdiag_device(ppls_ctx* c, CvScratch& tmp, const ppls_theta* th, int r, const double (&h)[PPLS_ROWDIAG_COEF * 16],
                   RowDiagFit& f, const int64_t* d_rows, int64_t nrows, bool mu, double** res_out, double** dmu_out) {
  int rc;
  if ((rc = rowdiag_upload_fit(c, tmp, th, r, h, f))) return rc;
  double *res = nullptr, *dmu = nullptr;
  if ((rc = tmp.get(c, &res, (size_t)3 * nrows))) return rc;
  if (mu && (rc = tmp.get(c, &dmu, (size_t)2 * nrows * r))) return rc;
  HIPCHK(c, ppls_launch_rowdiag(c->X, c->ldx, c->p, c->Y, c->ldy, c->q, c->dtype, d_rows, nrows, f.W, f.C, f.coef, r, res,
                                res + nrows, res + 2 * nrows, dmu, dmu ? dmu + (size_t)nrows * r : nullptr, nrows,
                                ppls_rowdiag_grid(nrows, c->p, c->q, c->dtype, r, c->num_cus), c->stream));
  *res_out = res;
  *dmu_out = dmu;
  return PPLS_OK;
}

// What ppls_robust_weights and ppls_po2_robust_weights do once the fit has passed its checks: §24's checks on m,
// nu and keep, every allocation, the distance pass (pass(tmp, n, &res) queues it on the context stream and
// gives res = [odx2 | ody2 | sd2], n each), the weight kernel, the all-reduce of the m + 1 sums and l_t.
template <class Pass>
int robust_weights_run(ppls_ctx* c, const double* nu, int m, int keep, double* loglik_t, double* sum_w, double sE2, double sF2,
                       double logdet, Pass&& pass) {
  int rc;
  if (m < 1 || m > PPLS_ROBUST_MAXNU) return fail(c, PPLS_E_ARG, "m=%d values of nu outside [1, %d]", m, PPLS_ROBUST_MAXNU);
  if (keep < 0 || keep >= m) return fail(c, PPLS_E_ARG, "keep=%d outside [0, %d)", keep, m);
  PplsRobustNu nus;
  memset(&nus, 0, sizeof nus);
  for (int j = 0; j < m; ++j) {
    if (!(nu[j] > 0.0) || !std::isfinite(nu[j])) return fail(c, PPLS_E_ARG, "nu[%d] = %g must be positive and finite", j, nu[j]);
    nus.nu[j] = nu[j];
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t n = c->n_local;
  // every allocation before the kept weights are touched
  CvScratch tmp;
  double *part = nullptr, *sums = nullptr, *res = nullptr;
  if ((rc = tmp.get(c, &part, (size_t)ppls_robust_blocks(n) * PPLS_ROBUST_SUMS))) return rc;
  if ((rc = tmp.get(c, &sums, (size_t)PPLS_ROBUST_SUMS))) return rc;
  if (c->rb_len < n || !c->rb_w || !c->rb_d2) {
    c->rb_kept = false;
    c->rb_len = 0;
    if ((rc = dalloc(c, &c->rb_w, (size_t)std::max<int64_t>(n, 1)))) return rc;
    if ((rc = dalloc(c, &c->rb_d2, (size_t)std::max<int64_t>(n, 1)))) return rc;
    c->rb_len = std::max<int64_t>(n, 1);
  }
  if (n > 0 && (rc = pass(tmp, n, &res))) return rc;
  c->rb_kept = false;   // from here the kept arrays are overwritten
  const double P = (double)(c->p + c->q);
  const int grid = c->rb_grid > 0 ? c->rb_grid : ppls_robust_grid(n, c->num_cus);
  HIPCHK(c, ppls_launch_robust_weights(res, res ? res + n : nullptr, res ? res + 2 * n : nullptr, n, sE2, sF2, &nus, m, keep,
                                       P, c->rb_w, c->rb_d2, part, sums, grid, c->stream));
  if ((rc = allreduce(c, sums, (size_t)PPLS_ROBUST_SUMS))) return rc;
  double hs[PPLS_ROBUST_SUMS];
  HIPCHK(c, hipMemcpyAsync(hs, sums, sizeof hs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double N = (double)c->n_total;
  for (int j = 0; j < m; ++j) {
    const double v = nu[j];
    const double cst = std::lgamma(0.5 * (v + P)) - std::lgamma(0.5 * v) - 0.5 * P * std::log(v * 3.141592653589793);
    loglik_t[j] = (N * cst - 0.5 * N * logdet) - 0.5 * (v + P) * hs[j];
  }
  if (sum_w) *sum_w = hs[PPLS_ROBUST_MAXNU];
  c->rb_kept = true;
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_row_diagnostics(ppls_ctx* c, const ppls_theta* th, int r, const int64_t* rows, int64_t nrows,
                         ppls_row_diag* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!out) return fail(c, PPLS_E_ARG, "NULL output");
  double h[PPLS_ROWDIAG_COEF * 16];
  RowDiagFit f;
  int rc;
  if ((rc = rowdiag_check_fit(c, th, r, h, f))) return rc;
  if (!rows) nrows = c->n_local;   // all local rows
  if (nrows < 0) return fail(c, PPLS_E_ARG, "row list: %lld rows", (long long)nrows);
  for (int64_t i = 0; rows && i < nrows; ++i)   // any order, repeats allowed: the kernel only reads
    if (rows[i] < 0 || rows[i] >= c->n_local)
      return fail(c, PPLS_E_ARG, "row index %lld (entry %lld) outside [0, %lld)", (long long)rows[i], (long long)i,
                  (long long)c->n_local);
  if (nrows == 0) return PPLS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  int64_t* d_rows = nullptr;
  if (rows && (rc = cv_upload_rows(c, tmp, rows, nrows, &d_rows))) return rc;
  double *res = nullptr, *dmu = nullptr;
  if ((rc = rowdiag_device(c, tmp, th, r, h, f, d_rows, nrows, out->mu_T || out->mu_U, &res, &dmu))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return rowdiag_collect(c, f, res, dmu, nrows, r, 0, nrows, out);
}

// ---------------------------------------------------------------------------- robust weights
int ppls_robust_weights(ppls_ctx* c, const ppls_theta* th, int r, const double* nu, int m, int keep, double* loglik_t,
                        double* sum_w) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!nu || !loglik_t) return fail(c, PPLS_E_ARG, "NULL argument");
  double h[PPLS_ROWDIAG_COEF * 16];
  RowDiagFit f;
  int rc;
  if ((rc = rowdiag_check_fit(c, th, r, h, f))) return rc;
  return robust_weights_run(c, nu, m, keep, loglik_t, sum_w, f.sE2, f.sF2, f.logdet, [&](CvScratch& tmp, int64_t n, double** res) {
    double* dmu = nullptr;
    return rowdiag_device(c, tmp, th, r, h, f, nullptr, n, false, res, &dmu);
  });
}

int ppls_robust_get(ppls_ctx* c, double* w, double* d2) {
  if (!c) return PPLS_E_ARG;
  if (!c->rb_kept) return fail(c, PPLS_E_STATE, "no robust weights are kept: call ppls_robust_weights first");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->n_local > 0 && w) HIPCHK(c, hipMemcpy(w, c->rb_w, sizeof(double) * c->n_local, hipMemcpyDeviceToHost));
  if (c->n_local > 0 && d2) HIPCHK(c, hipMemcpy(d2, c->rb_d2, sizeof(double) * c->n_local, hipMemcpyDeviceToHost));
  return PPLS_OK;
}

int ppls_row_diagnostics_new(ppls_ctx* c, const ppls_theta* th, int r, const double* X, const double* Y, int64_t n,
                             int layout, ppls_row_diag* out) {
  if (!c) return PPLS_E_ARG;
  if (c->p < 1 || c->q < 1) return fail(c, PPLS_E_STATE, "no data shape: load data (p, q) first");
  if (!out) return fail(c, PPLS_E_ARG, "NULL output");
  double h[PPLS_ROWDIAG_COEF * 16];
  RowDiagFit f;
  int rc;
  if ((rc = rowdiag_check_fit(c, th, r, h, f))) return rc;
  if (layout != PPLS_LAYOUT_COLMAJOR && layout != PPLS_LAYOUT_ROWMAJOR)
    return fail(c, PPLS_E_ARG, "layout must be 0 (column-major) or 1 (row-major)");
  if (n < 0 || (n > 0 && (!X || !Y))) return fail(c, PPLS_E_ARG, "NULL X or Y with %lld rows", (long long)n);
  if (n == 0) return PPLS_OK;
  const int p = c->p, q = c->q;
  for (int blk = 0; blk < 2; ++blk) {   // the whole call is refused, as ppls_set_data refuses such data
    const double* D = blk ? Y : X;
    const size_t len = (size_t)n * (blk ? q : p);
    for (size_t e = 0; e < len; ++e)
      if (!std::isfinite(D[e])) return fail(c, PPLS_E_ARG, "%c contains NaN or Inf", blk ? 'Y' : 'X');
  }
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  if ((rc = rowdiag_upload_fit(c, tmp, th, r, h, f))) return rc;
  // row blocks through a staging buffer (~64 MB of rows at a time), always staged in fp64
  const int ldx = (p + 1) & ~1, ldy = (q + 1) & ~1;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(64 << 20) / (8LL * (ldx + ldy))));
  const bool mu = out->mu_T || out->mu_U;
  double *inX = nullptr, *inY = nullptr, *cm = nullptr, *res = nullptr, *dmu = nullptr;
  if ((rc = tmp.get(c, &inX, (size_t)chunk * ldx))) return rc;
  if ((rc = tmp.get(c, &inY, (size_t)chunk * ldy))) return rc;
  if (layout == PPLS_LAYOUT_COLMAJOR && (rc = tmp.get(c, &cm, (size_t)chunk * std::max(p, q)))) return rc;
  if ((rc = tmp.get(c, &res, (size_t)3 * chunk))) return rc;
  if (mu && (rc = tmp.get(c, &dmu, (size_t)2 * chunk * r))) return rc;
  HIPCHK(c, hipMemsetAsync(inX, 0, sizeof(double) * chunk * ldx, c->stream));
  HIPCHK(c, hipMemsetAsync(inY, 0, sizeof(double) * chunk * ldy, c->stream));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nc = std::min(chunk, n - r0);
    for (int blk = 0; blk < 2; ++blk) {
      const double* D = blk ? Y : X;
      double* in = blk ? inY : inX;
      const int cols = blk ? q : p, ld = blk ? ldy : ldx;
      if (layout == PPLS_LAYOUT_ROWMAJOR) {
        HIPCHK(c, hipMemcpy2DAsync(in, sizeof(double) * ld, D + r0 * cols, sizeof(double) * cols, sizeof(double) * cols, nc,
                                   hipMemcpyHostToDevice, c->stream));
      } else {
        HIPCHK(c, hipMemcpy2DAsync(cm, sizeof(double) * nc, D + r0, sizeof(double) * n, sizeof(double) * nc, cols,
                                   hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, ppls_launch_to_rowmajor(cm, nc, cols, ld, in, c->stream));
      }
    }
    HIPCHK(c, ppls_launch_rowdiag(inX, ldx, p, inY, ldy, q, 0, nullptr, nc, f.W, f.C, f.coef, r, res, res + nc,
                                  res + 2 * nc, dmu, dmu ? dmu + (size_t)nc * r : nullptr, nc,
                                  ppls_rowdiag_grid(nc, p, q, 0, r, c->num_cus), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = rowdiag_collect(c, f, res, dmu, nc, r, r0, n, out))) return rc;
  }
  return PPLS_OK;
}

int ppls_rowdiag_timing(ppls_ctx* c, int r, int reps, double* ms) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!ms || reps < 1) return fail(c, PPLS_E_ARG, "ms must be given with reps >= 1");
  if (r < 1 || r > PPLS_RMAX || r > std::min(c->p, c->q))
    return fail(c, PPLS_E_ARG, "r=%d outside [1, min(%d, p, q)]", r, PPLS_RMAX);
  HIPCHK(c, hipSetDevice(c->device));
  // unit loadings and unit scalars: the time does not depend on the values
  std::vector<double> W((size_t)c->p * r, 0.0), C((size_t)c->q * r, 0.0), B(r, 1.0), sT(r, 1.0);
  for (int k = 0; k < r; ++k) W[(size_t)k * c->p + k] = C[(size_t)k * c->q + k] = 1.0;
  const ppls_theta th = {W.data(), C.data(), B.data(), sT.data(), 1.0, 1.0, 1.0};
  double h[PPLS_ROWDIAG_COEF * 16];
  RowDiagFit f;
  int rc;
  if ((rc = rowdiag_check_fit(c, &th, r, h, f))) return rc;
  CvScratch tmp;
  if ((rc = rowdiag_upload_fit(c, tmp, &th, r, h, f))) return rc;
  const int64_t n = c->n_local;
  double *res = nullptr, *dmu = nullptr;
  if ((rc = tmp.get(c, &res, (size_t)3 * std::max<int64_t>(n, 1)))) return rc;
  if ((rc = tmp.get(c, &dmu, (size_t)2 * std::max<int64_t>(n, 1) * r))) return rc;
  const int grid = ppls_rowdiag_grid(n, c->p, c->q, c->dtype, r, c->num_cus);
  for (int v = 0; v < 2; ++v) {
    double* m = v ? dmu : nullptr;
    CvEvents ev;
    for (int it = 0; it <= reps; ++it) {   // one untimed launch first
      if (it == 1) HIPCHK(c, ev.begin(c->stream));
      HIPCHK(c, ppls_launch_rowdiag(c->X, c->ldx, c->p, c->Y, c->ldy, c->q, c->dtype, nullptr, n, f.W, f.C, f.coef, r, res,
                                    res + n, res + 2 * n, m, m ? m + (size_t)n * r : nullptr, n, grid, c->stream));
    }
    HIPCHK(c, ev.end(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ms[v] = ev.ms() / reps;
  }
  return PPLS_OK;
}

int ppls_robust_timing(ppls_ctx* c, int reps, double* ms) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!ms || reps < 1) return fail(c, PPLS_E_ARG, "ms must be given with reps >= 1");
  HIPCHK(c, hipSetDevice(c->device));
  // distances of one component at unit loadings and scalars: real inputs, whatever the data
  std::vector<double> W((size_t)c->p, 0.0), C((size_t)c->q, 0.0);
  W[0] = C[0] = 1.0;
  double one = 1.0;
  const ppls_theta th = {W.data(), C.data(), &one, &one, 1.0, 1.0, 1.0};
  double h[PPLS_ROWDIAG_COEF * 16];
  RowDiagFit f;
  int rc;
  if ((rc = rowdiag_check_fit(c, &th, 1, h, f))) return rc;
  CvScratch tmp;
  const int64_t n = c->n_local;
  double *res = nullptr, *dmu = nullptr, *w = nullptr, *d2 = nullptr, *part = nullptr, *sums = nullptr;
  if (n < 1) return fail(c, PPLS_E_STATE, "no rows on this rank");
  if ((rc = rowdiag_device(c, tmp, &th, 1, h, f, nullptr, n, false, &res, &dmu))) return rc;
  if ((rc = tmp.get(c, &w, (size_t)n)) || (rc = tmp.get(c, &d2, (size_t)n))) return rc;
  if ((rc = tmp.get(c, &part, (size_t)ppls_robust_blocks(n) * PPLS_ROBUST_SUMS))) return rc;
  if ((rc = tmp.get(c, &sums, (size_t)PPLS_ROBUST_SUMS))) return rc;
  PplsRobustNu nus;
  for (int j = 0; j < PPLS_ROBUST_MAXNU; ++j) nus.nu[j] = 1.0 + j;
  const int grid = c->rb_grid > 0 ? c->rb_grid : ppls_robust_grid(n, c->num_cus);
  for (int v = 0; v < 2; ++v) {
    const int m = v ? PPLS_ROBUST_MAXNU : 1;
    CvEvents ev;
    for (int it = 0; it <= reps; ++it) {   // one untimed launch first
      if (it == 1) HIPCHK(c, ev.begin(c->stream));
      HIPCHK(c, ppls_launch_robust_weights(res, res + n, res + 2 * n, n, f.sE2, f.sF2, &nus, m, 0, (double)(c->p + c->q), w, d2,
                                           part, sums, grid, c->stream));
    }
    HIPCHK(c, ev.end(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ms[v] = ev.ms() / reps;
  }
  return PPLS_OK;
}

// ppls_cv_ppls (o2m = false: init holds nfolds * a starting values) and ppls_cv_ppls_o2m (o2m = true: every
// fold's fit is ppls_ppls_o2m on the training context's S).
static int cv_ppls_impl(ppls_ctx* c, int a, int nfolds, const int32_t* fold_of_row, const int64_t* fold_total, int max_steps,
                        double atol, int crit_abs, const ppls_theta* init, bool o2m, double* rmsep, int* ncomp) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!fold_total || (!o2m && !init) || !rmsep || !ncomp || (c->n_local > 0 && !fold_of_row)) return fail(c, PPLS_E_ARG, "NULL argument");
  if (a < 1 || a > PPLS_RMAX) return fail(c, PPLS_E_ARG, "nr_comp=%d outside [1,%d]", a, PPLS_RMAX);
  if (nfolds < 2) return fail(c, PPLS_E_ARG, "Cross-validation with 1 fold does not make sense, use 2 folds or more");
  int64_t tot = 0;
  for (int f = 0; f < nfolds; ++f) {
    if (fold_total[f] < 1) return fail(c, PPLS_E_ARG, "fold %d holds %lld rows", f, (long long)fold_total[f]);
    tot += fold_total[f];
  }
  if (tot != c->n_total) return fail(c, PPLS_E_ARG, "the folds hold %lld rows, the data %lld", (long long)tot, (long long)c->n_total);
  std::vector<std::vector<int64_t>> in_fold((size_t)nfolds);
  for (int64_t i = 0; i < c->n_local; ++i) {
    if (fold_of_row[i] < 0 || fold_of_row[i] >= nfolds) return fail(c, PPLS_E_ARG, "fold_of_row[%lld]=%d outside [0,%d)", (long long)i, fold_of_row[i], nfolds);
    in_fold[(size_t)fold_of_row[i]].push_back(i);
  }
  for (int f = 0; f < nfolds; ++f)
    if ((int64_t)in_fold[(size_t)f].size() > fold_total[f])
      return fail(c, PPLS_E_ARG, "fold %d: %zu local rows, %lld over all ranks", f, in_fold[(size_t)f].size(), (long long)fold_total[f]);
  for (int k = 0; !o2m && k < nfolds * a; ++k)
    if (!init[k].W || !init[k].C || !init[k].B || !init[k].sigT) return fail(c, PPLS_E_ARG, "init[%d] has NULL fields", k);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (!c->cv_train && (rc = ppls_ctx_create(c->device, &c->cv_train))) return fail(c, rc, "could not create the training context");
  ppls_ctx* t = c->cv_train;
  // c's options carry over; the communicator is borrowed (ppls_ctx_destroy(c) takes it back)
  t->xprod = c->xprod;
  t->xprod_rw = c->xprod_rw;
  t->xprod_fuse = c->xprod_fuse;
  t->o2m_path = c->o2m_path;
  if (t->gram_int8 && !c->gram_int8) {
    HIPCHK(c, hipStreamSynchronize(t->stream));
    oz_free(t);
  }
  t->gram_int8 = c->gram_int8;
  t->ldpad = c->ldpad;
  t->sweep_mode = c->sweep_mode;
  t->grid_opt = c->grid_opt;
  t->nt_loads = c->nt_loads;
  t->reducer = c->reducer;
  t->reducer_user = c->reducer_user;
  t->comm = c->comm;
  t->nranks = c->nranks;
  t->rank = c->rank;
  const int p = c->p, q = c->q;
  std::vector<double> W((size_t)p * a), C((size_t)q * a), B((size_t)a), sig((size_t)4 * a), sse((size_t)a);
  std::vector<int64_t> train;
  for (int f = 0; f < nfolds; ++f) {
    const std::vector<int64_t>& out = in_fold[(size_t)f];
    // R's X[-folds[ii], ] (crossval_PPLS.R:48): the other rows, in their order
    train.clear();
    for (int64_t i = 0; i < c->n_local; ++i)
      if (fold_of_row[i] != f) train.push_back(i);
    const int64_t n_train = c->n_total - fold_total[f];
    if (n_train < 1) return fail(c, PPLS_E_ARG, "fold %d leaves no training row", f);
    if ((rc = ppls_set_data_from(t, c, train.data(), (int64_t)train.size(), n_train))) { c->err = t->err; return rc; }
    // fits that read S get it as S - S_fold; a fold larger than its training set (2 uneven folds)
    // is past the downdate's error statement: ppls_ppls_ex then forms S from the training rows
    // (the o2m_xprod start reads S whatever the fits read)
    if ((o2m || xprod_choose(t, a * max_steps, 1)) && fold_total[f] <= n_train)
      if ((rc = ppls_xprod_downdate(t, c, out.data(), (int64_t)out.size()))) { c->err = t->err; return rc; }
    ppls_seq_fit fit;
    memset(&fit, 0, sizeof fit);
    fit.W = W.data();
    fit.C = C.data();
    fit.B = B.data();
    fit.sig = sig.data();
    const auto t0 = std::chrono::steady_clock::now();
    rc = o2m ? ppls_ppls_o2m(t, a, max_steps, atol, crit_abs, nullptr, &fit)
             : ppls_ppls_ex(t, a, max_steps, atol, crit_abs, init + (size_t)f * a, nullptr, &fit);
    c->cv_ms[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) { c->err = t->err; return rc; }
    ncomp[f] = fit.ncomp;
    for (int j = 0; j < a; ++j) rmsep[(size_t)f * a + j] = NAN;
    if (fit.ncomp < 1) continue;   // every rank alike: the fits are the same on all ranks
    if ((rc = ppls_heldout_sse(c, W.data(), C.data(), B.data(), fit.ncomp, out.data(), (int64_t)out.size(), sse.data())))
      return rc;
    // sqrt(mse(Y[fold, ], predict(fit, X[fold, ], "X"))) with mse(x, y) = mean((x - y)^2) (:49)
    for (int j = 0; j < fit.ncomp; ++j) rmsep[(size_t)f * a + j] = std::sqrt(sse[j] / ((double)fold_total[f] * q));
  }
  return PPLS_OK;
}

int ppls_cv_ppls(ppls_ctx* c, int a, int nfolds, const int32_t* fold_of_row, const int64_t* fold_total, int max_steps,
                 double atol, int crit_abs, const ppls_theta* init, double* rmsep, int* ncomp) {
  return cv_ppls_impl(c, a, nfolds, fold_of_row, fold_total, max_steps, atol, crit_abs, init, false, rmsep, ncomp);
}

int ppls_cv_ppls_o2m(ppls_ctx* c, int a, int nfolds, const int32_t* fold_of_row, const int64_t* fold_total, int max_steps,
                     double atol, int crit_abs, double* rmsep, int* ncomp) {
  return cv_ppls_impl(c, a, nfolds, fold_of_row, fold_total, max_steps, atol, crit_abs, nullptr, true, rmsep, ncomp);
}

int ppls_cv_timing(ppls_ctx* c, double* out6, int reset) {
  if (!c) return PPLS_E_ARG;
  if (out6) {
    for (int i = 0; i < 4; ++i) out6[i] = c->cv_ms[i];
    out6[4] = c->cv_bytes[0];
    out6[5] = c->cv_bytes[1];
  }
  if (reset) {
    for (int i = 0; i < 4; ++i) c->cv_ms[i] = 0.0;
    c->cv_bytes[0] = c->cv_bytes[1] = 0.0;
  }
  return PPLS_OK;
}

}  // extern "C"

// ============================================================================ scale()
// R's scale(X, center, scale) / scale(Y, center, scale) on the resident data (ppls_scale.hip): the
// column sums, then the column sums of squares of the centred values, each all-reduced once (X's p
// values and Y's q in one buffer), then the in-place update.  The statistics are formed on the host
// from the all-reduced sums, so every rank holds the same centre and scale and takes the same
// decisions.
namespace {

struct ScaleSide {
  void* data;
  int64_t ld;
  int cols, off;   // off: this block's offset in the p + q vectors (and ldc-padded device vectors)
  PplsScalePlan pl;
};

// One statistics pass over X and Y into red[0 .. p + q) (device), all-reduced.
int scale_stat_pass(ppls_ctx* c, const ScaleSide (&sd)[2], const double* centre_d, int sq, int nt, double* part,
                    double* red, std::vector<double>& host, int pass) {
  int rc;
  const int P = c->p + c->q;
  CvEvents ev;
  HIPCHK(c, hipMemsetAsync(red, 0, sizeof(double) * P, c->stream));   // a rank without rows contributes zeros
  HIPCHK(c, ev.begin(c->stream));
  if (c->n_local > 0)
    for (int m = 0; m < 2; ++m) {
      HIPCHK(c, ppls_launch_col_partials(sd[m].data, sd[m].ld, c->n_local, c->dtype, &sd[m].pl,
                                         centre_d ? centre_d + (m ? sd[0].pl.ldc : 0) : nullptr, sq, nt, part, c->stream));
      HIPCHK(c, ppls_launch_col_reduce(part, &sd[m].pl, sd[m].cols, red + sd[m].off, c->stream));
    }
  HIPCHK(c, ev.end(c->stream));
  if ((rc = allreduce(c, red, (size_t)P))) return rc;
  host.resize((size_t)P);
  HIPCHK(c, hipMemcpyAsync(host.data(), red, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double es = c->dtype ? 4.0 : 8.0;
  c->scale_ms[pass] = ev.ms();
  c->scale_bytes[pass] = (double)c->n_local * es * ((double)sd[0].pl.ldc + sd[1].pl.ldc);
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_scale_data(ppls_ctx* c, int center, int scale) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!center && !scale) return PPLS_OK;
  // n_total is the same on every rank, so this refusal needs no collective
  if (scale && c->n_total < 2)
    return fail(c, PPLS_E_ARG, "scale = TRUE needs at least 2 rows (over all ranks: %lld): the standard deviation "
                               "divides by n - 1", (long long)c->n_total);
  HIPCHK(c, hipSetDevice(c->device));
  c->rb_kept = false;   // the rows change under kept robust weights
  int rc;
  const int p = c->p, q = c->q, P = p + q;
  ScaleSide sd[2] = {{c->X, c->ldx, p, 0, ppls_scale_plan(c->n_local, p, c->dtype, c->num_cus)},
                     {c->Y, c->ldy, q, p, ppls_scale_plan(c->n_local, q, c->dtype, c->num_cus)}};
  const int L0 = sd[0].pl.ldc, L = L0 + sd[1].pl.ldc;   // device vectors: X's ldc values, then Y's
  const bool nt = c->nt_loads > 0 ||
                  (c->nt_loads < 0 && 8.0 * c->n_local * (double)(c->ldx + c->ldy) > 256.0 * (1 << 20));
  CvScratch tmp;
  double *part = nullptr, *red = nullptr, *cen_d = nullptr, *scl_d = nullptr;
  const size_t plen = std::max((size_t)sd[0].pl.nblocks * sd[0].pl.ldc, (size_t)sd[1].pl.nblocks * sd[1].pl.ldc);
  if ((rc = tmp.get(c, &part, plen))) return rc;
  if ((rc = tmp.get(c, &red, (size_t)P))) return rc;
  if ((rc = tmp.get(c, &cen_d, (size_t)L))) return rc;
  if ((rc = tmp.get(c, &scl_d, (size_t)L))) return rc;
  for (int k = 0; k < 3; ++k) c->scale_ms[k] = c->scale_bytes[k] = 0.0;

  // the p + q statistics and their ldc-padded device copies (padding: centre 0, scale 1)
  std::vector<double> cen((size_t)P, 0.0), scl((size_t)P, 1.0), host, pad((size_t)L);
  auto upload = [&](const std::vector<double>& v, double fill, double* dst) -> int {
    std::fill(pad.begin(), pad.end(), fill);
    std::copy(v.begin(), v.begin() + p, pad.begin());
    std::copy(v.begin() + p, v.end(), pad.begin() + L0);
    HIPCHK(c, hipMemcpyAsync(dst, pad.data(), sizeof(double) * L, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PPLS_OK;
  };
  if (center) {
    if ((rc = scale_stat_pass(c, sd, nullptr, 0, nt, part, red, host, 0))) return rc;
    for (int j = 0; j < P; ++j) cen[(size_t)j] = host[(size_t)j] / (double)c->n_total;
  }
  if ((rc = upload(cen, 0.0, cen_d))) return rc;
  if (scale) {
    if ((rc = scale_stat_pass(c, sd, cen_d, 1, nt, part, red, host, 1))) return rc;
    for (int j = 0; j < P; ++j) scl[(size_t)j] = std::sqrt(host[(size_t)j] / (double)(c->n_total - 1));
    // R would fill such a column with NaN (0 / 0) or Inf; decided from the all-reduced values, before
    // the data are touched
    for (int j = 0; j < P; ++j)
      if (!(scl[(size_t)j] > 0.0) || !std::isfinite(scl[(size_t)j]))
        return fail(c, PPLS_E_ARG, "%c column %d has standard deviation %g (over all ranks): scale = TRUE would fill "
                                   "it with NaN or Inf, as R's scale() does; the data are unchanged",
                    j < p ? 'X' : 'Y', (j < p ? j : j - p) + 1, scl[(size_t)j]);
  }
  // (the means are finite: resident data passed check_finite_data, so |x| < 1.3e154 and no sum overflows)
  if ((rc = upload(scl, 1.0, scl_d))) return rc;

  c->em_active = false;   // the data change: an ppls_em_begin session ends here, never a silent switch
  c->xp_active = false;
  {
    CvEvents ev;
    HIPCHK(c, ev.begin(c->stream));
    if (c->n_local > 0)
      for (int m = 0; m < 2; ++m)
        HIPCHK(c, ppls_launch_col_apply(sd[m].data, sd[m].ld, c->n_local, sd[m].cols, c->dtype, &sd[m].pl,
                                        cen_d + (m ? L0 : 0), scl_d + (m ? L0 : 0), nt, c->stream));
    HIPCHK(c, ev.end(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->scale_ms[2] = ev.ms();
    c->scale_bytes[2] = 2.0 * (double)c->n_local * (c->dtype ? 4.0 : 8.0) * (double)P;
  }
  // compose with the transform the data already carried: loaded = (new * scl + cen) * scale0 + center0
  if (c->sc_center.empty()) {
    c->sc_center.assign((size_t)P, 0.0);
    c->sc_scale.assign((size_t)P, 1.0);
  }
  for (int j = 0; j < P; ++j) {
    c->sc_center[(size_t)j] += c->sc_scale[(size_t)j] * cen[(size_t)j];
    c->sc_scale[(size_t)j] *= scl[(size_t)j];
  }
  // from here the context is what ppls_set_data of the transformed matrix would have left: ||X||^2,
  // ||Y||^2 and the free-memory slots fresh, a resident S dropped (not corrected: DESIGN), the verdict
  if ((rc = compute_ssq(c))) return rc;
  return check_finite_data(c);
}

int ppls_get_scaling(ppls_ctx* c, double* center, double* scale) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  const int P = c->p + c->q;
  for (int j = 0; j < P; ++j) {
    if (center) center[j] = c->sc_center.empty() ? 0.0 : c->sc_center[(size_t)j];
    if (scale) scale[j] = c->sc_scale.empty() ? 1.0 : c->sc_scale[(size_t)j];
  }
  return PPLS_OK;
}

int ppls_scale_timing(ppls_ctx* c, double* ms3, double* bytes3) {
  if (!c) return PPLS_E_ARG;
  for (int k = 0; k < 3; ++k) {
    if (ms3) ms3[k] = c->scale_ms[k];
    if (bytes3) bytes3[k] = c->scale_bytes[k];
  }
  return PPLS_OK;
}

}  // extern "C"

// ============================================================================ streamed data
// ppls_stream_begin / _rows / _rows_from / _end: S = [X Y]'[X Y] of the centred (and scaled) data from
// row chunks.  Per chunk, on st_stream: column means (the fixed-order column sums of
// ppls_scale.hip), the staged chunk centred about its own mean, its MFMA Gram into split partials, and
// one pass over S that sums the partials in and adds Chan's pairwise term
// (N n_c / (N + n_c)) delta delta', delta = chunk mean - running mean.  The scaling is applied to S
// at the end: S_ij / (d_i d_j).
namespace {

int stream_fail(ppls_ctx* c, int rc) {
  c->st_failed = true;
  return rc;
}

#define STREAMCHK(c, call)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return stream_fail((c), fail((c), PPLS_E_HIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__)); \
  } while (0)

int stream_open_check(ppls_ctx* c) {
  if (c->st_state != 1) return fail(c, PPLS_E_STATE, "no stream is open: call ppls_stream_begin first");
  if (c->st_failed)
    return fail(c, PPLS_E_STATE, "the stream failed earlier and is unusable until the next ppls_stream_begin");
  return PPLS_OK;
}

// Grow a device buffer the chunk work uses: wait for that work first.
int stream_grow(ppls_ctx* c, double** buf, int64_t* len, int64_t need) {
  if (*buf && *len >= need) return PPLS_OK;
  STREAMCHK(c, hipStreamSynchronize(c->st_stream));
  *len = 0;
  const int rc = dalloc(c, buf, (size_t)need);
  if (rc) return stream_fail(c, rc);
  *len = need;
  return PPLS_OK;
}

// Room for a chunk of n rows in both staging buffers (and the column-major scratch); returns with the
// buffer the chunk goes to free.
int stream_reserve(ppls_ctx* c, int64_t n, bool colmajor) {
  int rc;
  if (n > c->st_cap) {
    STREAMCHK(c, hipStreamSynchronize(c->st_stream));
    c->st_cap = 0;
    for (int b = 0; b < 2; ++b)
      if ((rc = dalloc(c, &c->st_buf[b], (size_t)n * (c->ldx + c->ldy)))) return stream_fail(c, rc);
    c->st_cap = n;
  }
  if (colmajor && (rc = stream_grow(c, &c->st_cm, &c->st_cm_len, n * std::max(c->p, c->q)))) return rc;
  // an asynchronous failure of the chunk that last used this buffer surfaces here
  STREAMCHK(c, hipEventSynchronize(c->st_done[c->st_next]));
  return PPLS_OK;
}

// The four steps of one chunk (or of one fold segment of a chunk): n staged rows Xs, Ys merged into the
// Chan state (Nprev rows, mean, S), enqueued on st_stream.  qslot: where the Gram's work queue goes (null:
// the context's kept queue, rebuilt behind a drain of st_stream when the row count changes -- a fold
// stream's segments differ in length every time, and that drain would undo the overlap with the next upload).
int stream_merge_rows(ppls_ctx* c, double* Xs, double* Ys, int64_t n, double* S, double* mean, int64_t Nprev,
                      int** qslot = nullptr, int64_t* qlen = nullptr) {
  int rc;
  const int P = c->ldx + c->ldy;
  hipStream_t s = c->st_stream;
  double *sum = c->st_vec, *mc = sum + P, *delta = mc + P, *ones = delta + 2 * P;
  const double N = (double)Nprev, nc = (double)n;
  if (c->st_center) {
    const PplsScalePlan px = ppls_scale_plan(n, c->p, 0, c->num_cus), py = ppls_scale_plan(n, c->q, 0, c->num_cus);
    const int64_t plen = std::max(px.nblocks * px.ldc, py.nblocks * py.ldc);
    if ((rc = stream_grow(c, &c->st_colpart, &c->st_colpart_len, plen))) return rc;
    STREAMCHK(c, ppls_launch_col_partials(Xs, c->ldx, n, 0, &px, nullptr, 0, 0, c->st_colpart, s));
    STREAMCHK(c, ppls_launch_col_reduce(c->st_colpart, &px, c->p, sum, s));
    STREAMCHK(c, ppls_launch_col_partials(Ys, c->ldy, n, 0, &py, nullptr, 0, 0, c->st_colpart, s));
    STREAMCHK(c, ppls_launch_col_reduce(c->st_colpart, &py, c->q, sum + c->ldx, s));
    STREAMCHK(c, ppls_launch_stream_mean(sum, P, c->p, c->ldx, c->q, nc, N, mc, delta, mean, s));
    STREAMCHK(c, ppls_launch_col_apply(Xs, c->ldx, n, c->p, 0, &px, mc, ones, 0, s));
    STREAMCHK(c, ppls_launch_col_apply(Ys, c->ldy, n, c->q, 0, &py, mc + c->ldx, ones + c->ldx, 0, s));
  }
  const GramShape g{P, c->p, c->ldx, c->q, Xs, c->ldx, Ys, c->ldy, c->ldy};
  const int nsplit = gram_nsplit(c, g, n, 0, 0);   // the staged chunk is fp64
  if ((rc = stream_grow(c, &c->st_part, &c->st_part_len, ppls_gram_part_doubles(P, nsplit)))) return rc;
  int* q = nullptr;
  if (qslot) {   // a fold segment: its own queue, free since st_done of its staging buffer was waited for
    const int64_t need = ppls_gram_queue_ints(g.p, nsplit);
    if (*qlen < need) {
      *qlen = 0;
      if ((rc = dalloc(c, qslot, (size_t)need))) return stream_fail(c, rc);
      *qlen = need;
    }
    STREAMCHK(c, ppls_gram_queue_prepare(*qslot, g.p, g.xreal, g.xcols, g.yreal, n, gram_wave_slots(c, 0), 0, c->stream));
    q = *qslot;
  } else if ((rc = gram_queue(c, g, n, 0, &q, 0, s))) {
    return stream_fail(c, rc);
  }
  STREAMCHK(c, ppls_launch_gram_joint(Xs, c->ldx, c->ldx, c->p, Ys, c->ldy, c->ldy, c->q, 0, n, P, nsplit, c->st_part, q, nullptr, nullptr, s));
  STREAMCHK(c, ppls_launch_stream_merge(S, c->p, c->ldx, c->q, c->ldy, c->st_part, nsplit,
                                        c->st_center ? delta : nullptr, N * nc / (N + nc), s));
  return PPLS_OK;
}

// The device work of the chunk staged in buffer b (n rows), enqueued on st_stream.  A fold stream
// (the chunk's stable fold order is in st_idx[b], its segment offsets in st_seg): the rows are
// gathered into fold order, then every non-empty segment is merged into its fold's state, in fold
// order; a fold absent from the chunk launches nothing.
int stream_process(ppls_ctx* c, int b, int64_t n) {
  int rc;
  const int P = c->ldx + c->ldy;
  hipStream_t s = c->st_stream;
  double* Xs = c->st_buf[b];
  double* Ys = Xs + c->st_cap * c->ldx;
  if (c->st_nfolds > 0) {
    if ((rc = stream_grow(c, &c->st_gbuf, &c->st_gbuf_len, c->st_cap * P))) return rc;
    double* Xg = c->st_gbuf;
    double* Yg = Xg + c->st_cap * c->ldx;
    STREAMCHK(c, ppls_launch_gather_rows(Xs, c->ldx / 2, Xg, c->ldx / 2, c->ldx / 2, c->st_idx[b], n, s));
    STREAMCHK(c, ppls_launch_gather_rows(Ys, c->ldy / 2, Yg, c->ldy / 2, c->ldy / 2, c->st_idx[b], n, s));
    for (int k = 0; k < c->st_nfolds; ++k) {
      const int64_t lo = c->st_seg[(size_t)k], ns = c->st_seg[(size_t)k + 1] - lo;
      if (ns == 0) continue;
      if ((rc = stream_merge_rows(c, Xg + lo * c->ldx, Yg + lo * c->ldy, ns, c->st_fS + (size_t)k * P * P,
                                  c->st_fmean + (size_t)k * P, c->st_fN[(size_t)k], &c->st_fq[(size_t)b * c->st_nfolds + k],
                                  &c->st_fq_len[(size_t)b * c->st_nfolds + k])))
        return rc;
      c->st_fN[(size_t)k] += ns;
    }
  } else if ((rc = stream_merge_rows(c, Xs, Ys, n, c->xp_S, c->st_vec + 3 * P, c->st_rows))) {
    return rc;
  }
  STREAMCHK(c, hipEventRecord(c->st_done[b], s));
  c->st_next = b ^ 1;
  c->st_rows += n;
  ++c->st_chunks;
  return PPLS_OK;
}

// The stable fold order of a chunk's rows (a counting sort) into st_idx[b] and st_seg, uploaded on
// the context's stream with the chunk.  The labels were checked.
int stream_fold_order(ppls_ctx* c, int b, const int32_t* fold, int64_t n) {
  const int K = c->st_nfolds;
  std::vector<int64_t>& seg = c->st_seg;
  seg.assign((size_t)K + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++seg[(size_t)fold[i] + 1];
  for (int k = 0; k < K; ++k) seg[(size_t)k + 1] += seg[(size_t)k];
  std::vector<int64_t> at(seg.begin(), seg.end() - 1), idx((size_t)n);
  for (int64_t i = 0; i < n; ++i) idx[(size_t)at[(size_t)fold[i]]++] = i;
  const int rc = grow(c, &c->st_idx[b], &c->st_idx_len[b], n);   // (st_done[b] was waited for: nothing reads the old list)
  if (rc) return stream_fail(c, rc);
  STREAMCHK(c, hipMemcpy(c->st_idx[b], idx.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice));
  return PPLS_OK;
}

// The calls with fold labels belong to a fold stream, those without to a plain one; labels in range.
int stream_fold_check(ppls_ctx* c, const int32_t* fold, bool labelled, int64_t n) {
  if (labelled != (c->st_nfolds > 0))
    return fail(c, PPLS_E_STATE, labelled ? "the stream was opened without folds: use the calls without fold labels"
                                          : "the stream was opened with %d folds: every chunk needs fold labels", c->st_nfolds);
  if (!labelled || n == 0) return PPLS_OK;
  if (!fold) return fail(c, PPLS_E_ARG, "NULL fold labels");
  for (int64_t i = 0; i < n; ++i)
    if (fold[i] < 0 || fold[i] >= c->st_nfolds)
      return fail(c, PPLS_E_ARG, "fold label %d of row %lld outside [0, %d)", fold[i], (long long)i, c->st_nfolds);
  return PPLS_OK;
}

// ---- ppls_stream_end: what the plain and the fold stream share -------------------------------------
// Sharded, every rank must reach every collective of the call.  A HIP error in this rank's own work
// between the collectives therefore goes into a flag the ranks agree on (agree), so every rank
// returns and none waits alone; only a failed copy of a collective's own buffer returns at once
// (that rank cannot take part in a collective over device buffers at all): REFUSECHK, which drops
// the stream.
#define REFUSECHK(c, call)                                                                                          \
  do {                                                                                                              \
    hipError_t e_ = (call);                                                                                         \
    if (e_ != hipSuccess)                                                                                           \
      return drop_to_no_data((c), fail((c), PPLS_E_HIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__)); \
  } while (0)

// A HIP error of this rank's own steps after the collectives: its verdict, which the last collective shares.
int end_hip(ppls_ctx* c, hipError_t e, const char* what) {
  return e == hipSuccess ? PPLS_OK : fail(c, PPLS_E_HIP, "ppls_stream_end, %s: %s", what, hipGetErrorString(e));
}

// The diagonal of a P x P device matrix.
hipError_t diag_to_host(const double* S, int P, std::vector<double>& diag) {
  diag.resize((size_t)P);
  return hipMemcpy2D(diag.data(), sizeof(double), S, sizeof(double) * ((size_t)P + 1), sizeof(double), (size_t)P,
                     hipMemcpyDeviceToHost);
}

// ||X||^2, ||Y||^2 = the traces of the diagonal blocks of a matrix in the joint layout, in column order.
void diag_traces(const ppls_ctx* c, const std::vector<double>& diag, double s2[2]) {
  s2[0] = s2[1] = 0.0;
  for (int j = 0; j < c->p; ++j) s2[0] += diag[(size_t)j];
  for (int j = 0; j < c->q; ++j) s2[1] += diag[(size_t)c->ldx + j];
}

// ||X||^2, ||Y||^2 of a context from the S it holds (P x P, complete on this rank): on the device and the host.
hipError_t derived_traces(ppls_ctx* c, int P) {
  std::vector<double> diag;
  double s2[2];
  hipError_t e = diag_to_host(c->xp_S, P, diag);
  if (e != hipSuccess) return e;
  diag_traces(c, diag, s2);
  if ((e = hipMemcpy(c->ssq, s2, sizeof s2, hipMemcpyHostToDevice)) != hipSuccess) return e;
  c->ssq_host[0] = s2[0];
  c->ssq_host[1] = s2[1];
  return hipSuccess;
}

int traces_finite(ppls_ctx* c, const double s2[2]) {
  for (int k = 0; k < 2; ++k)
    if (!std::isfinite(s2[k]))
      return fail(c, PPLS_E_ARG,
                  "%c contains NaN or Inf (the trace of its streamed cross-products is %g; values beyond 1.3e154 "
                  "also overflow it): the reference's svd() in orth() stops on non-finite data (EM_W_multi.R:732-733)",
                  k ? 'Y' : 'X', s2[k]);
  return PPLS_OK;
}

// The transform of a stream of N rows with mean m (joint layout) and centred sums of squares dsum:
// cen, scl over the p + q real columns as ppls_scale_get reports them, and d (joint layout, 1 where
// nothing is divided) for the kernels.  Refuses what R's scale() would fill with NaN or Inf.
int stream_transform(ppls_ctx* c, double N, const std::vector<double>& m, const std::vector<double>& dsum,
                     std::vector<double>& cen, std::vector<double>& scl, std::vector<double>& d) {
  const int p = c->p, q = c->q, ldx = c->ldx;
  d.assign((size_t)ldx + c->ldy, 1.0);
  for (int j = 0; j < p + q; ++j) {
    cen[(size_t)j] = c->st_center ? m[(size_t)(j < p ? j : ldx + j - p)] : 0.0;
    scl[(size_t)j] = 1.0;
  }
  if (!c->st_scale) return PPLS_OK;
  if (N < 2.0)
    return fail(c, PPLS_E_ARG, "scale = TRUE needs at least 2 rows (over all ranks: %lld): the standard deviation "
                               "divides by n - 1", (long long)N);
  for (int j = 0; j < p + q; ++j) {
    const int jj = j < p ? j : ldx + j - p;
    const double dj = std::sqrt(dsum[(size_t)jj] / (N - 1.0));
    if (!(dj > 0.0) || !std::isfinite(dj))
      return fail(c, PPLS_E_ARG, "%c column %d has standard deviation %g (over all ranks): scale = TRUE would fill it "
                                 "with NaN or Inf, as R's scale() does; the stream is dropped",
                  j < p ? 'X' : 'Y', (j < p ? j : j - p) + 1, dj);
    d[(size_t)jj] = scl[(size_t)j] = dj;
  }
  return PPLS_OK;
}

// ppls_stream_begin (nfolds = 0) and ppls_stream_begin_folds.
int stream_begin(ppls_ctx* c, int p, int q, int center, int scale, int nfolds) {
  if (!c) return PPLS_E_ARG;
  if ((center != 0 && center != 1) || (scale != 0 && scale != 1)) return fail(c, PPLS_E_ARG, "center and scale must be 0 or 1");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int rc;
  if ((rc = alloc_data(c, 0, p, q, 0))) return rc;   // drops resident rows, a stream, an EM session
  xprod_free(c);
  if (!c->st_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->st_stream, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b)
    if (!c->st_done[b]) HIPCHK(c, hipEventCreateWithFlags(&c->st_done[b], hipEventDisableTiming));
  const int P = c->ldx + c->ldy;
  const size_t nvec = (size_t)5 * P + (size_t)nfolds;   // (a fold stream: + the folds' weights at the end)
  auto drop = [&]() {
    dfree(c->xp_S);
    dfree(c->st_vec);
    dfree(c->st_fS);
    dfree(c->st_fmean);
  };
  if ((rc = dalloc(c, &c->xp_S, (size_t)P * P))) return rc;
  if ((rc = dalloc(c, &c->st_vec, nvec))) { drop(); return rc; }
  // the fold matrices up front, in one allocation (one collective at the end), and the fold means
  if (nfolds > 0 && ((rc = dalloc(c, &c->st_fS, (size_t)nfolds * P * P)) || (rc = dalloc(c, &c->st_fmean, (size_t)nfolds * P)))) {
    drop();
    return rc;
  }
  std::vector<double> v(nvec, 0.0);
  std::fill(v.begin() + (size_t)4 * P, v.begin() + (size_t)5 * P, 1.0);
  hipError_t e = hipMemsetAsync(c->xp_S, 0, sizeof(double) * P * P, c->stream);
  if (e == hipSuccess && nfolds > 0) e = hipMemsetAsync(c->st_fS, 0, sizeof(double) * nfolds * P * P, c->stream);
  if (e == hipSuccess && nfolds > 0) e = hipMemsetAsync(c->st_fmean, 0, sizeof(double) * nfolds * P, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(c->st_vec, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  for (int b = 0; b < 2 && e == hipSuccess; ++b) e = hipEventRecord(c->st_done[b], c->st_stream);
  if (e != hipSuccess) {
    drop();
    return fail(c, PPLS_E_HIP, "ppls_stream_begin: %s", hipGetErrorString(e));
  }
  c->st_nfolds = nfolds;
  c->st_fN.assign((size_t)nfolds, 0);
  c->st_fq.assign((size_t)2 * nfolds, nullptr);
  c->st_fq_len.assign((size_t)2 * nfolds, 0);
  c->st_sel = -1;
  c->st_center = center;
  c->st_scale = scale;
  c->st_rows = c->st_chunks = 0;
  c->st_next = 0;
  c->st_failed = false;
  c->st_state = 1;
  return PPLS_OK;
}

int stream_rows(ppls_ctx* c, const double* X, const double* Y, int64_t nrows, int layout, const int32_t* fold, bool labelled) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = stream_open_check(c))) return rc;
  if ((rc = stream_fold_check(c, fold, labelled, nrows < 0 ? 0 : nrows))) return rc;
  if (nrows == 0) return PPLS_OK;
  if (nrows < 0 || !X || !Y) return fail(c, PPLS_E_ARG, "a chunk needs nrows >= 1 and X, Y");
  if (layout != PPLS_LAYOUT_COLMAJOR && layout != PPLS_LAYOUT_ROWMAJOR)
    return fail(c, PPLS_E_ARG, "layout must be 0 (column-major) or 1 (row-major)");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = stream_reserve(c, nrows, layout == PPLS_LAYOUT_COLMAJOR))) return rc;
  const int b = c->st_next;
  if (labelled && (rc = stream_fold_order(c, b, fold, nrows))) return rc;
  for (int m = 0; m < 2; ++m) {
    const double* src = m == 0 ? X : Y;
    const int cols = m == 0 ? c->p : c->q, ld = m == 0 ? c->ldx : c->ldy;
    double* dst = c->st_buf[b] + (m == 0 ? 0 : c->st_cap * c->ldx);
    if (layout == PPLS_LAYOUT_ROWMAJOR) {
      if (ld != cols) STREAMCHK(c, hipMemset2DAsync(dst, sizeof(double) * ld, 0, sizeof(double) * ld, nrows, c->stream));
      STREAMCHK(c, hipMemcpy2DAsync(dst, sizeof(double) * ld, src, sizeof(double) * cols, sizeof(double) * cols, nrows,
                                    hipMemcpyHostToDevice, c->stream));
    } else {
      STREAMCHK(c, hipMemcpyAsync(c->st_cm, src, sizeof(double) * nrows * cols, hipMemcpyHostToDevice, c->stream));
      STREAMCHK(c, ppls_launch_to_rowmajor(c->st_cm, nrows, cols, ld, dst, c->stream));
    }
  }
  STREAMCHK(c, hipStreamSynchronize(c->stream));   // the chunk is on the device: the caller's buffers are free
  return stream_process(c, b, nrows);
}

int stream_rows_from(ppls_ctx* c, ppls_ctx* src, const int32_t* fold, bool labelled) {
  if (!c || !src) return c ? fail(c, PPLS_E_ARG, "NULL source context") : PPLS_E_ARG;
  int rc;
  if ((rc = stream_open_check(c))) return rc;
  if (src == c) return fail(c, PPLS_E_ARG, "the source must be another context");
  if (src->device != c->device) return fail(c, PPLS_E_ARG, "the source context is on device %d, this one on %d", src->device, c->device);
  if (!src->have_data) return fail(c, PPLS_E_ARG, "the source context has no data");
  if (src->st_state == 2) return fail(c, PPLS_E_STATE, PPLS_STREAMED_MSG);
  if (src->p != c->p || src->q != c->q)
    return fail(c, PPLS_E_ARG, "the source holds p=%d q=%d, the stream was begun with p=%d q=%d", src->p, src->q, c->p, c->q);
  const int64_t n = src->n_local;
  if ((rc = stream_fold_check(c, fold, labelled, n))) return rc;
  if (n == 0) return PPLS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(src->stream));
  if ((rc = stream_reserve(c, n, false))) return rc;
  const int b = c->st_next;
  if (labelled && (rc = stream_fold_order(c, b, fold, n))) return rc;
  CvScratch tmp;
  for (int m = 0; m < 2; ++m) {
    const void* sp = m == 0 ? src->X : src->Y;
    const int cols = m == 0 ? c->p : c->q, ld = m == 0 ? c->ldx : c->ldy, sld = m == 0 ? src->ldx : src->ldy;
    double* dst = c->st_buf[b] + (m == 0 ? 0 : c->st_cap * c->ldx);
    if (src->dtype) {   // fp32 storage: widen the rows, then lay them out at this context's stride
      double* wide = nullptr;
      if ((rc = tmp.get(c, &wide, (size_t)n * sld))) return stream_fail(c, rc);
      STREAMCHK(c, ppls_launch_convert(sp, 1, wide, 0, n * sld, c->stream));
      sp = wide;
    }
    if (ld != cols) STREAMCHK(c, hipMemset2DAsync(dst, sizeof(double) * ld, 0, sizeof(double) * ld, n, c->stream));
    STREAMCHK(c, hipMemcpy2DAsync(dst, sizeof(double) * ld, sp, sizeof(double) * sld, sizeof(double) * cols, n,
                                  hipMemcpyDeviceToDevice, c->stream));
  }
  STREAMCHK(c, hipStreamSynchronize(c->stream));
  return stream_process(c, b, n);
}

// xp_S = the sum of the fold matrices but `fold` (-1: all), with n_total and ||X||^2, ||Y||^2 (the
// traces of S's diagonal blocks, in column order) to match.  No state checks.
int fold_select(ppls_ctx* c, int fold) {
  const int P = c->ldx + c->ldy;
  HIPCHK(c, ppls_launch_cvs_select(c->st_fS, c->st_nfolds, fold, (int64_t)P * P, c->xp_S, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, derived_traces(c, P));
  int64_t N = 0;
  for (int k = 0; k < c->st_nfolds; ++k)
    if (k != fold) N += c->st_fN[(size_t)k];
  c->n_total = N;
  c->st_sel = fold;
  return PPLS_OK;
}

// The calls that read the fold matrices: a context streamed with folds.
int fold_state_check(ppls_ctx* c) {
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (c->st_state != 2 || c->st_nfolds < 1)
    return fail(c, PPLS_E_STATE, "the context holds no fold cross-products: stream the rows with ppls_stream_begin_folds");
  return PPLS_OK;
}

// The collectives of ppls_stream_end, over K Chan states (N_k, mean_k, S_k): a fold stream's K folds,
// or the plain stream's one state.  S: the K matrices, P x P each; mean_d: their K x P
// means on the device (overwritten); Nk: this rank's rows per state; what: the matrices' name in a
// message.  On PPLS_OK every rank holds the same matrices, Nk the rows over all ranks and mh (K x P)
// the means over all ranks.  Any other return has dropped the stream: the caller returns at once.
int stream_end_merge(ppls_ctx* c, double* S, int K, double* mean_d, std::vector<double>& Nk, std::vector<double>& mh,
                     const char* what) {
  int rc;
  const int P = c->ldx + c->ldy;
  const size_t PP = (size_t)P * P, KP = (size_t)K * P;
  mh.assign(KP, 0.0);
  if (!c->st_failed && hipMemcpy(mh.data(), mean_d, sizeof(double) * KP, hipMemcpyDeviceToHost) != hipSuccess)
    c->st_failed = true;
  if (!collective(c))
    return c->st_failed ? drop_to_no_data(c, fail(c, PPLS_E_STATE, "the stream failed before ppls_stream_end")) : PPLS_OK;
  // {failed, N_rk, N_rk m_rk for all k}: the global counts and means, and the agreement that nobody
  // failed, in one all-reduce
  const size_t nred = 1 + (size_t)K + KP;
  CvScratch tmp;
  double* red = nullptr;
  if ((rc = tmp.get(c, &red, nred))) return drop_to_no_data(c, rc);
  std::vector<double> h(nred, 0.0);
  h[0] = c->st_failed ? 1.0 : 0.0;
  for (int k = 0; k < K; ++k) {
    h[(size_t)1 + k] = Nk[(size_t)k];
    for (int j = 0; j < P; ++j)
      h[1 + (size_t)K + (size_t)k * P + j] = c->st_failed ? 0.0 : Nk[(size_t)k] * mh[(size_t)k * P + j];
  }
  REFUSECHK(c, hipMemcpyAsync(red, h.data(), sizeof(double) * nred, hipMemcpyHostToDevice, c->stream));
  if ((rc = allreduce(c, red, nred))) return drop_to_no_data(c, rc);
  REFUSECHK(c, hipMemcpyAsync(h.data(), red, sizeof(double) * nred, hipMemcpyDeviceToHost, c->stream));
  REFUSECHK(c, hipStreamSynchronize(c->stream));
  if (h[0] > 0.0)
    return drop_to_no_data(c, fail(c, PPLS_E_STATE, "the stream failed on %d rank(s) before ppls_stream_end", (int)h[0]));
  // each rank's S_k is centred about its own mean: + N_rk (m_rk - m_k)(m_rk - m_k)', the merge with
  // no partials, state by state
  std::vector<double> d(KP, 0.0);
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < P; ++j) {
      const size_t at = (size_t)k * P + j;
      const double mg = h[(size_t)1 + k] > 0.0 ? h[1 + (size_t)K + at] / h[(size_t)1 + k] : 0.0;
      d[at] = mh[at] - mg;
      mh[at] = mg;
    }
  hipError_t e = hipSuccess;
  if (c->st_center) {
    e = hipMemcpyAsync(mean_d, d.data(), sizeof(double) * KP, hipMemcpyHostToDevice, c->stream);
    for (int k = 0; k < K && e == hipSuccess; ++k)
      if (Nk[(size_t)k] > 0.0)
        e = ppls_launch_stream_merge(S + (size_t)k * PP, c->p, c->ldx, c->q, c->ldy, nullptr, 0, mean_d + (size_t)k * P,
                                     Nk[(size_t)k], c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  for (int k = 0; k < K; ++k) Nk[(size_t)k] = h[(size_t)1 + k];
  // nobody enters the all-reduce of the matrices alone (the pattern of xprod_setup)
  double bad = e == hipSuccess ? 0.0 : 1.0;
  if ((rc = agree(c, &bad, 1))) return drop_to_no_data(c, rc);
  if (bad > 0.0)
    return drop_to_no_data(c, fail(c, PPLS_E_HIP, "the cross-rank merge of %s failed on %d rank(s)", what, (int)bad));
  if ((rc = allreduce(c, S, (size_t)K * PP))) return drop_to_no_data(c, rc);
  REFUSECHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

// The finish of a plain stream of N rows with mean m (over all ranks, as every rank holds them after
// stream_end_merge), on this rank alone and with the same bits on every rank: the transform in
// cen / scl, S standardised where scale is set, ||X||^2, ||Y||^2 in s2 and on the device.  Returns
// PPLS_OK, a refusal decided from the shared values (PPLS_E_ARG: the same on every rank) or a HIP error
// of this rank, which the caller's last collective makes everybody's.
int plain_finish(ppls_ctx* c, double N, const std::vector<double>& m, std::vector<double>& cen, std::vector<double>& scl,
                 double s2[2]) {
  int rc;
  const int P = c->ldx + c->ldy;
  if (!(N >= 1.0)) return fail(c, PPLS_E_ARG, "no rows were streamed (over all ranks)");
  std::vector<double> diag, d;
  auto traces = [&]() -> int {
    const int r = end_hip(c, diag_to_host(c->xp_S, P, diag), "the diagonal of S");
    if (r) return r;
    diag_traces(c, diag, s2);
    return traces_finite(c, s2);
  };
  if ((rc = traces()) || (rc = stream_transform(c, N, m, diag, cen, scl, d))) return rc;
  if (c->st_scale) {
    hipError_t e = hipMemcpyAsync(c->st_vec, d.data(), sizeof(double) * P, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = ppls_launch_stream_standardise(c->xp_S, c->p, c->ldx, c->q, c->ldy, c->st_vec, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if ((rc = end_hip(c, e, "standardising S")) || (rc = traces())) return rc;
  }
  return end_hip(c, hipMemcpy(c->ssq, s2, sizeof(double) * 2, hipMemcpyHostToDevice), "||X||^2, ||Y||^2");
}

// The finish of a fold stream from the fold counts Nk and fold means fm of
// stream_end_merge, with plain_finish's returns.  On PPLS_OK: *N_out rows over all ranks, the
// transform in cen / scl, ||X||^2, ||Y||^2 in s2, and the context selected on all folds.
int fold_finish(ppls_ctx* c, const std::vector<double>& Nk, const std::vector<double>& fm, double* N_out,
                std::vector<double>& cen, std::vector<double>& scl, double s2[2]) {
  int rc;
  const int K = c->st_nfolds, p = c->p, q = c->q, ldx = c->ldx, P = c->ldx + c->ldy;
  const size_t KP = (size_t)K * P;
  double N = 0.0;
  for (int k = 0; k < K; ++k) {
    if (!(Nk[(size_t)k] >= 1.0))
      return fail(c, PPLS_E_ARG, "fold %d holds no row (over all ranks): every fold needs at least one; the stream is dropped", k);
    N += Nk[(size_t)k];
  }
  // the global mean, summed in fold order, and the folds' offsets from it
  std::vector<double> m((size_t)P, 0.0), ev(KP, 0.0), d, dsum((size_t)P);
  for (int j = 0; j < P; ++j) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc += Nk[(size_t)k] * fm[(size_t)k * P + j];
    m[(size_t)j] = acc / N;
  }
  if (c->st_center)
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < P; ++j) ev[(size_t)k * P + j] = fm[(size_t)k * P + j] - m[(size_t)j];
  double *vec = c->st_vec, *wd = vec + 5 * (size_t)P;   // the folds' weights N_k
  hipError_t e = hipMemcpyAsync(c->st_fmean, ev.data(), sizeof(double) * KP, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(wd, Nk.data(), sizeof(double) * K, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = ppls_launch_cvs_diag(c->st_fS, K, p, ldx, q, c->ldy, c->st_fmean, wd, vec + P, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dsum.data(), vec + P, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if ((rc = end_hip(c, e, "the diagonal of the fold matrices"))) return rc;
  double tr[2];
  diag_traces(c, dsum, tr);
  if ((rc = traces_finite(c, tr)) || (rc = stream_transform(c, N, m, dsum, cen, scl, d))) return rc;
  if (c->st_center || c->st_scale) {   // one pass over every fold matrix: recentre and standardise
    e = hipMemcpyAsync(vec, d.data(), sizeof(double) * P, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = ppls_launch_cvs_finish(c->st_fS, K, p, ldx, q, c->ldy, c->st_fmean, wd, vec, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if ((rc = end_hip(c, e, "recentring and standardising the fold matrices"))) return rc;
  }
  for (int k = 0; k < K; ++k) c->st_fN[(size_t)k] = (int64_t)Nk[(size_t)k];
  c->st_fmean_h = fm;
  if ((rc = fold_select(c, -1))) return rc;
  s2[0] = c->ssq_host[0];
  s2[1] = c->ssq_host[1];
  *N_out = N;
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_stream_begin(ppls_ctx* c, int p, int q, int center, int scale) {
  return stream_begin(c, p, q, center, scale, 0);
}

int ppls_stream_begin_folds(ppls_ctx* c, int p, int q, int center, int scale, int nfolds) {
  if (!c) return PPLS_E_ARG;
  if (nfolds < 2) return fail(c, PPLS_E_ARG, "Cross-validation with 1 fold does not make sense, use 2 folds or more");
  if (nfolds > 65535) return fail(c, PPLS_E_ARG, "nfolds=%d: at most 65535 folds", nfolds);
  return stream_begin(c, p, q, center, scale, nfolds);
}

int ppls_stream_rows(ppls_ctx* c, const double* X, const double* Y, int64_t nrows, int layout) {
  return stream_rows(c, X, Y, nrows, layout, nullptr, false);
}

int ppls_stream_rows_folds(ppls_ctx* c, const double* X, const double* Y, int64_t nrows, int layout, const int32_t* fold) {
  return stream_rows(c, X, Y, nrows, layout, fold, true);
}

int ppls_stream_rows_from(ppls_ctx* c, ppls_ctx* src) { return stream_rows_from(c, src, nullptr, false); }

int ppls_stream_rows_from_folds(ppls_ctx* c, ppls_ctx* src, const int32_t* fold) {
  return stream_rows_from(c, src, fold, true);
}

int ppls_stream_end(ppls_ctx* c) {
  if (!c) return PPLS_E_ARG;
  if (c->st_state != 1) return fail(c, PPLS_E_STATE, "no stream is open: call ppls_stream_begin first");
  HIPCHK(c, hipSetDevice(c->device));
  // Every return from here drops the stream (drop_to_no_data) or leaves the context streamed.
  int rc;
  const int p = c->p, q = c->q, P = c->ldx + c->ldy;
  // wait for the pending chunk work; a failure (now or earlier) is agreed on below when sharded
  if (hipStreamSynchronize(c->st_stream) != hipSuccess) c->st_failed = true;
  // the plain stream is one Chan state (st_rows, mean, xp_S), a fold stream one per fold
  const bool folds = c->st_nfolds > 0;
  const int K = folds ? c->st_nfolds : 1;
  std::vector<double> Nk((size_t)K, (double)c->st_rows), m;
  for (int k = 0; folds && k < K; ++k) Nk[(size_t)k] = (double)c->st_fN[(size_t)k];
  if ((rc = stream_end_merge(c, folds ? c->st_fS : c->xp_S, K, folds ? c->st_fmean : c->st_vec + 3 * P, Nk, m,
                             folds ? "the fold matrices" : "S")))
    return rc;
  // From here every rank holds the same matrices, counts and means.  The finish runs on this rank
  // alone; its outcome is PPLS_OK, a refusal decided from those shared values (PPLS_E_ARG: the same on
  // every rank) or a HIP error of this rank, which the last collective below makes everybody's.
  std::vector<double> cen((size_t)p + q, 0.0), scl((size_t)p + q, 1.0);
  double s2[2] = {0.0, 0.0}, N = Nk[0];
  int local = folds ? fold_finish(c, Nk, m, &N, cen, scl, s2) : plain_finish(c, N, m, cen, scl, s2);
  const std::string local_err = c->err;
  // the staging buffers and partials go back before the free memory is read: the smallest free HBM
  // over all ranks, as compute_ssq records it, beside the agreement on the steps above
  const int64_t rows = c->st_rows, chunks = c->st_chunks;
  stream_release(c);   // (st_state = 0: drop_to_no_data below still clears S and have_data)
  size_t mfree = 0, mtot = 0;
  if (!local) local = end_hip(c, hipMemGetInfo(&mfree, &mtot), "hipMemGetInfo");
  c->mem_free_min = (double)mfree;
  if (collective(c)) {
    CvScratch tmp;
    double* slots_d = nullptr;
    if ((rc = tmp.get(c, &slots_d, (size_t)c->nranks + 1))) return drop_to_no_data(c, rc);
    std::vector<double> slots((size_t)c->nranks + 1, 0.0);   // {HIP failures, free HBM of rank 0, 1, ...}
    slots[0] = local == PPLS_OK || local == PPLS_E_ARG ? 0.0 : 1.0;
    slots[(size_t)c->rank + 1] = (double)mfree;
    REFUSECHK(c, hipMemcpy(slots_d, slots.data(), sizeof(double) * slots.size(), hipMemcpyHostToDevice));
    if ((rc = allreduce(c, slots_d, slots.size()))) return drop_to_no_data(c, rc);
    REFUSECHK(c, hipStreamSynchronize(c->stream));
    REFUSECHK(c, hipMemcpy(slots.data(), slots_d, sizeof(double) * slots.size(), hipMemcpyDeviceToHost));
    if (slots[0] > 0.0 && (local == PPLS_OK || local == PPLS_E_ARG))
      local = fail(c, PPLS_E_HIP, "ppls_stream_end failed on %d other rank(s)", (int)slots[0]);
    else if (local)
      c->err = local_err;
    for (size_t k = 1; k < slots.size(); ++k) c->mem_free_min = std::min(c->mem_free_min, slots[k]);
  }
  if (local) return drop_to_no_data(c, local);
  c->ssq_host[0] = s2[0];
  c->ssq_host[1] = s2[1];
  c->sc_center = cen;
  c->sc_scale = scl;
  // streamed: no rows resident, S ready and kept until the data change or ppls_xprod_release
  c->st_rows = rows;
  c->st_chunks = chunks;
  c->st_state = 2;
  c->n_local = 0;
  c->xp_active = false;
  c->em_active = false;
  derived_publish(c, (int64_t)N, c->mem_free_min);
  return PPLS_OK;
}

}  // extern "C"

// ============================================================================ resampled cross-products
// A bootstrap replicate is the resident rows with row i repeated count_i times, so its cross-products
// are S_c = sum_i count_i d_i d_i': the weighted instantiation of the MFMA Gram over src's rows, no copy
// of them, into a context that holds S_c and no rows -- the streamed state.
namespace {

// ppls_xprod_resample (count; weight NULL, real false) and ppls_xprod_weighted (real: weight, or NULL for
// src's kept device weights).  One lifecycle: the agreement across ranks, dst's reused S and partials.
int reweight_impl(ppls_ctx* dst, ppls_ctx* src, const int32_t* count, const double* weight, bool real) {
  int rc;
  if ((rc = pair_check(dst, src))) return rc;
  if (!src->have_data) return fail(dst, PPLS_E_STATE, "the source context has no data");
  if (src->st_state == 2) return fail(dst, PPLS_E_STATE, PPLS_STREAMED_MSG);
  const bool kept = real && !weight;   // src's device weights, no host round trip
  if (kept && !src->rb_kept)
    return fail(dst, PPLS_E_STATE, "NULL weights and the source keeps none: call ppls_robust_weights on it first");
  HIPCHK(dst, hipSetDevice(src->device));
  const bool coll = collective(src);
  const int64_t n = src->n_local;
  const int P = src->ldx + src->ldy;
  const size_t PP = (size_t)P * P;
  // this rank's verdict on its counts joins the agreement below (with sum count), so ranks return together
  int bad = PPLS_OK;
  double sum = 0.0;
  if (kept) {
    sum = 1.0;   // kept weights are (nu + P) / (nu + d2) > 0 by construction
  } else if (real) {
    for (int64_t i = 0; i < n; ++i) {
      if (!(weight[i] >= 0.0) || !std::isfinite(weight[i])) {
        bad = fail(dst, PPLS_E_ARG, "weight %g of local row %lld is negative or not finite", weight[i], (long long)i);
        break;
      }
      sum += weight[i];
    }
  } else if (n > 0 && !count) {
    bad = fail(dst, PPLS_E_ARG, "NULL counts for %lld local rows", (long long)n);
  } else {
    for (int64_t i = 0; i < n; ++i) {
      if (count[i] < 0) {
        bad = fail(dst, PPLS_E_ARG, "count %d of local row %lld is negative", (int)count[i], (long long)i);
        break;
      }
      sum += (double)count[i];
    }
  }
  const std::string bad_err = dst->err;
  if (bad && !coll) return bad;
  // every allocation of the call before the ranks agree (as xprod_setup does for S): a new S only when
  // dst does not already hold resampled (or plainly streamed) cross-products of this shape, the kept
  // counts and partials only when they have to grow, the Gram's queue on src (kept there per shape)
  const bool reuse = derived_reuse(dst, src->p, src->q, src->ldx, src->ldy);
  const GramShape g = gram_shape(src, true, 0);
  const int64_t nrun = bad ? 0 : n;
  DevGuard Snew;
  int rc_alloc = reuse ? PPLS_OK : dalloc(dst, &Snew.p, PP);
  if (!rc_alloc && nrun > 0) {
    rc_alloc = grow(dst, &dst->rs_part, &dst->rs_part_len, ppls_gram_part_doubles(P, gram_nsplit(src, g, nrun, 0)));
    if (!rc_alloc && real && !kept) rc_alloc = grow(dst, &dst->rs_wt, &dst->rs_wt_len, nrun);
    if (!rc_alloc && !real) rc_alloc = grow(dst, &dst->rs_cnt, &dst->rs_cnt_len, nrun);
    if (!rc_alloc) {
      int* q = nullptr;
      if ((rc_alloc = gram_queue(src, g, nrun, 0, &q))) dst->err = src->err;
    }
  }
  if (bad) sum = 0.0;
  const AgreeSpec sp{"resampled S", "it", real ? "bad weights" : "bad counts", false, true};
  if ((rc = ranks_agree(dst, src, sp, rc_alloc, bad, bad_err, &sum))) return rc;
  if (real ? !(sum > 0.0) : !(sum >= 1.0))
    return fail(dst, PPLS_E_ARG, real ? "the weights are all zero over all ranks" : "the counts sum to 0 over all ranks: a replicate needs rows");
  // From here dst ends streamed on S_c, or without data.  The Gram runs on src's stream, behind whatever
  // src has queued, and the sum over ranks goes through src's communicator.
  int local = derived_begin(dst, "resample", "the source's", src->dtype, src->ldpad, src->p, src->q, src->ldx, src->ldy, Snew, reuse);
  if (!local && n > 0) {
    hipError_t e = hipSuccess;
    // (kept: src->rb_w as it stands)
    if (real && !kept) e = hipMemcpyAsync(dst->rs_wt, weight, sizeof(double) * n, hipMemcpyHostToDevice, src->stream);
    else if (!real) e = hipMemcpyAsync(dst->rs_cnt, count, sizeof(int32_t) * n, hipMemcpyHostToDevice, src->stream);
    if (e != hipSuccess) local = fail(dst, PPLS_E_HIP, "resample: upload of the counts: %s", hipGetErrorString(e));
    // always the fp64 MFMA Gram (the int8 form does not take weights); src's record of how its own S was
    // formed (oz_used) is not touched
    if (!local && (local = gram_run(src, g, n, 0, dst->xp_S, nullptr, dst->rs_part, real ? nullptr : dst->rs_cnt,
                                    kept ? src->rb_w : real ? dst->rs_wt : nullptr)))
      dst->err = src->err;
  } else if (!local) {
    if (hipMemsetAsync(dst->xp_S, 0, sizeof(double) * PP, src->stream) != hipSuccess)
      local = fail(dst, PPLS_E_HIP, "resample: zeroing S failed");
  }
  if (coll) {   // nobody enters the all-reduce of S_c alone
    double b = local ? 1.0 : 0.0;
    if ((rc = agree(src, &b, 1))) {
      dst->err = src->err;
      return drop_to_no_data(dst, rc);
    }
    if (b > 0.0 && !local) local = fail(dst, PPLS_E_HIP, "resampled S failed on %d other rank(s)", (int)b);
  }
  if (local) return drop_to_no_data(dst, local);
  if ((rc = allreduce(src, dst->xp_S, PP))) {
    dst->err = src->err;
    return drop_to_no_data(dst, rc);
  }
  // ||X||^2, ||Y||^2: the traces of S_c's diagonal blocks, in column order (as fold_select takes them)
  hipError_t e = hipStreamSynchronize(src->stream);
  if (e == hipSuccess) e = derived_traces(dst, P);
  if (e != hipSuccess) return drop_to_no_data(dst, fail(dst, PPLS_E_HIP, "resample: traces of S: %s", hipGetErrorString(e)));
  record_copy(dst, src);
  derived_publish(dst, real ? src->n_total : (int64_t)sum, src->mem_free_min);   // real weights are relative to N
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_xprod_resample(ppls_ctx* dst, ppls_ctx* src, const int32_t* count) {
  return reweight_impl(dst, src, count, nullptr, false);
}

int ppls_xprod_weighted(ppls_ctx* dst, ppls_ctx* src, const double* weight) {
  return reweight_impl(dst, src, nullptr, weight, true);
}

}  // extern "C"

// ============================================================================ permuted cross-products
// A permutation replicate pairs x_i with y_pi(i): of S = [X Y_pi]'[X Y_pi] only the p x q block
// C_pi = sum_i x_i y_pi(i)' depends on pi (ppls_permute.hip); X'X and Y'Y are src's, bit for bit.
namespace {

// perm must be a permutation of 0 .. n - 1: checked with a byte map, O(n), before any device work.
int perm_check(ppls_ctx* c, const int64_t* perm, int64_t n, std::vector<uint8_t>& seen) {
  if (n > 0x7fffffffLL)
    return fail(c, PPLS_E_ARG, "%lld local rows: the permuted cross-products take at most 2^31 - 1 per rank", (long long)n);
  if (n > 0 && !perm) return fail(c, PPLS_E_ARG, "NULL permutation for %lld local rows", (long long)n);
  try {
    seen.assign((size_t)n, 0);
  } catch (const std::bad_alloc&) {
    return fail(c, PPLS_E_NOMEM, "permutation check: no host memory for %lld bytes", (long long)n);
  }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = perm[i];
    if (v < 0 || v >= n)
      return fail(c, PPLS_E_ARG, "entry %lld of the permutation is %lld: out of range 0 .. %lld", (long long)i, (long long)v,
                  (long long)(n - 1));
    if (seen[(size_t)v])
      return fail(c, PPLS_E_ARG, "entry %lld of the permutation repeats row %lld: not a permutation", (long long)i,
                  (long long)v);
    seen[(size_t)v] = 1;
  }
  return PPLS_OK;
}

// The kernel's plan over n rows of c: splits, and the device index array [n indices | padding | bounds].
struct PermPlan {
  int nsplit;
  int64_t idx_len;   // int32 entries before the int64 bounds (even)
  int64_t ints;      // the array's whole length in int32
  int64_t part;      // doubles of split partials
};

PermPlan perm_plan(const ppls_ctx* c, int64_t n, int req) {
  PermPlan pl;
  const int slots = c->num_cus * ppls_xperm_occupancy(c->dtype) * 4;
  pl.nsplit = n > 0 ? ppls_xperm_plan(c->p, c->q, n, slots, req, nullptr) : 1;
  pl.idx_len = (n + PPLS_XPERM_PAD + 1) / 2 * 2;
  pl.ints = pl.idx_len + 2 * (PPLS_XPERM_MAXSPLIT + 1);
  pl.part = ppls_xperm_part_doubles(c->p, c->q, pl.nsplit);
  return pl;
}

// host: the staged array (pl.ints entries) for perm (validated) over c's n rows.
void perm_stage(const ppls_ctx* c, const PermPlan& pl, int64_t n, int req, const int64_t* perm, int32_t* host) {
  for (int64_t i = 0; i < n; ++i) host[i] = (int32_t)perm[i];
  for (int64_t i = n; i < pl.ints; ++i) host[i] = 0;
  const int slots = c->num_cus * ppls_xperm_occupancy(c->dtype) * 4;
  int64_t bounds[PPLS_XPERM_MAXSPLIT + 1] = {0};
  if (n > 0) ppls_xperm_plan(c->p, c->q, n, slots, req, bounds);
  memcpy(host + pl.idx_len, bounds, sizeof bounds);
}

// blk (device, ldx x ldy) = C_perm over c's n > 0 rows, on c's stream (not waited for): the MFMA kernel
// into part over the uploaded array d_idx, then the finish.  e0, e1 (may be NULL): events around the kernel.
hipError_t perm_run(ppls_ctx* c, const PermPlan& pl, int64_t n, int32_t* d_idx, double* part, double* blk, hipEvent_t e0,
                    hipEvent_t e1) {
  hipError_t e = hipSuccess;
  if (e0) e = hipEventRecord(e0, c->stream);
  if (e == hipSuccess)
    e = ppls_launch_xperm(c->X, c->ldx, c->p, c->Y, c->ldy, c->q, c->dtype, n, d_idx, (const int64_t*)(d_idx + pl.idx_len),
                          pl.nsplit, part, c->stream);
  if (e == hipSuccess && e1) e = hipEventRecord(e1, c->stream);
  if (e == hipSuccess) e = ppls_launch_xperm_finish(part, pl.nsplit, c->p, c->q, c->ldx, c->ldy, blk, c->stream);
  return e;
}

}  // namespace

extern "C" {

int ppls_xgram_permuted(ppls_ctx* c, int nsplit, const int64_t* perm, double* C, double* ms) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (nsplit < 0 || nsplit > PPLS_XPERM_MAXSPLIT)
    return fail(c, PPLS_E_ARG, "nsplit must be 0 (auto) .. %d", PPLS_XPERM_MAXSPLIT);
  if (c->n_local <= 0) return fail(c, PPLS_E_STATE, "no rows on this rank");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const int64_t n = c->n_local;
  std::vector<uint8_t> seen;
  if ((rc = perm_check(c, perm, n, seen))) return rc;
  const PermPlan pl = perm_plan(c, n, nsplit);
  struct Bufs {
    int32_t* idx = nullptr;
    double *part = nullptr, *blk = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Bufs() {
      dfree(idx); dfree(part); dfree(blk);
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } b;
  const size_t len = (size_t)c->ldx * c->ldy;
  if ((rc = dalloc(c, &b.idx, (size_t)pl.ints)) || (rc = dalloc(c, &b.part, (size_t)pl.part)) || (rc = dalloc(c, &b.blk, len)))
    return rc;
  HIPCHK(c, hipEventCreate(&b.e0));
  HIPCHK(c, hipEventCreate(&b.e1));
  std::vector<int32_t> host((size_t)pl.ints);
  perm_stage(c, pl, n, nsplit, perm, host.data());
  hipError_t e = hipMemcpy(b.idx, host.data(), sizeof(int32_t) * (size_t)pl.ints, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = perm_run(c, pl, n, b.idx, b.part, b.blk, b.e0, b.e1);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  float t = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, b.e0, b.e1);
  if (e != hipSuccess) return fail(c, PPLS_E_HIP, "permuted cross block: %s", hipGetErrorString(e));
  if (C) {
    std::vector<double> full(len);
    HIPCHK(c, hipMemcpy(full.data(), b.blk, sizeof(double) * len, hipMemcpyDeviceToHost));
    for (int j = 0; j < c->q; ++j)
      for (int a = 0; a < c->p; ++a) C[(size_t)j * c->p + a] = full[(size_t)j * c->ldx + a];
  }
  if (ms) *ms = t;
  return PPLS_OK;
}

int ppls_xprod_permute(ppls_ctx* dst, ppls_ctx* src, const int64_t* perm) {
  int rc;
  if ((rc = pair_check(dst, src))) return rc;
  if (!src->have_data) return fail(dst, PPLS_E_STATE, "the source context has no data");
  if (src->st_state == 2) return fail(dst, PPLS_E_STATE, PPLS_STREAMED_MSG);
  HIPCHK(dst, hipSetDevice(src->device));
  const bool coll = collective(src);
  const int64_t n = src->n_local;
  const int P = src->ldx + src->ldy;
  const size_t PP = (size_t)P * P, BL = (size_t)src->ldx * src->ldy;
  // this rank's verdict on its permutation joins the agreement below, so that ranks return together
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); };
  const auto t_call = Clock::now();
  const int bad = perm_check(dst, perm, n, dst->pm_seen);
  dst->pm_ms[0] = ms_since(t_call);
  dst->pm_ms[1] = dst->pm_ms[2] = dst->pm_ms[3] = 0.0;
  const std::string bad_err = dst->err;
  if (bad && !coll) return bad;
  // src's own S, formed and kept if it is not there (a collective of its own when sharded: every rank is here)
  if ((rc = xprod_setup(src))) {
    dst->err = src->err;
    return rc;
  }
  // every allocation of the call before the ranks agree: a new S only when dst does not already hold
  // streamed cross-products of this shape; the index array, the block and the partials only to grow
  const bool reuse = derived_reuse(dst, src->p, src->q, src->ldx, src->ldy);
  // (dst's diagonal blocks are already src's when its S is the one the last permute left, of this very S of src)
  const bool keep_diag = reuse && dst->pm_self_serial == dst->xp_serial && dst->pm_src_serial == src->xp_serial;
  const int64_t nrun = bad ? 0 : n;
  const PermPlan pl = perm_plan(src, nrun, 0);
  DevGuard Snew;
  int rc_alloc = reuse ? PPLS_OK : dalloc(dst, &Snew.p, PP);
  if (!rc_alloc) rc_alloc = grow(dst, &dst->pm_blk, &dst->pm_blk_len, (int64_t)BL);
  if (!rc_alloc && nrun > 0) {
    rc_alloc = grow(dst, &dst->rs_part, &dst->rs_part_len, pl.part);
    if (!rc_alloc) rc_alloc = grow(dst, &dst->pm_idx, &dst->pm_idx_len, pl.ints);
    if (!rc_alloc) {
      try {
        dst->pm_host.resize((size_t)pl.ints);
      } catch (const std::bad_alloc&) {
        rc_alloc = fail(dst, PPLS_E_NOMEM, "permuted S: no host memory for %lld row indices", (long long)pl.ints);
      }
    }
  }
  const AgreeSpec sp{"permuted S", "it", "a bad permutation", true, true};
  if ((rc = ranks_agree(dst, src, sp, rc_alloc, bad, bad_err, nullptr))) return rc;
  // From here dst ends streamed on S_pi, or without data.  Everything runs on src's stream, behind
  // whatever src has queued, and the sum over ranks goes through src's communicator.
  int local = derived_begin(dst, "permute", "the source's", src->dtype, src->ldpad, src->p, src->q, src->ldx, src->ldy, Snew, reuse);
  dst->pm_self_serial = 0;
  if (!local && !keep_diag &&
      hipMemcpyAsync(dst->xp_S, src->xp_S, sizeof(double) * PP, hipMemcpyDeviceToDevice, src->stream) != hipSuccess)
    local = fail(dst, PPLS_E_HIP, "permute: copy of the source's S failed");
  auto t_run = Clock::now();
  if (!local && n > 0) {
    perm_stage(src, pl, n, 0, perm, dst->pm_host.data());
    hipError_t e = hipMemcpyAsync(dst->pm_idx, dst->pm_host.data(), sizeof(int32_t) * (size_t)pl.ints, hipMemcpyHostToDevice,
                                  src->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(src->stream);
    dst->pm_ms[1] = ms_since(t_run);
    t_run = Clock::now();
    if (e == hipSuccess) e = perm_run(src, pl, n, dst->pm_idx, dst->rs_part, dst->pm_blk, nullptr, nullptr);
    if (e != hipSuccess) local = fail(dst, PPLS_E_HIP, "permuted cross block: %s", hipGetErrorString(e));
  } else if (!local) {
    if (hipMemsetAsync(dst->pm_blk, 0, sizeof(double) * BL, src->stream) != hipSuccess)
      local = fail(dst, PPLS_E_HIP, "permute: zeroing the block failed");
  }
  if (!local && hipStreamSynchronize(src->stream) != hipSuccess)
    local = fail(dst, PPLS_E_HIP, "permuted cross block: the kernel failed");
  dst->pm_ms[2] = ms_since(t_run);
  if (coll) {   // nobody enters the all-reduce of the block alone
    double b = local ? 1.0 : 0.0;
    if ((rc = agree(src, &b, 1))) {
      dst->err = src->err;
      return drop_to_no_data(dst, rc);
    }
    if (b > 0.0 && !local) local = fail(dst, PPLS_E_HIP, "permuted S failed on %d other rank(s)", (int)b);
  }
  if (local) return drop_to_no_data(dst, local);
  if ((rc = allreduce(src, dst->pm_blk, BL))) {   // the ldx x ldy block only: the diagonal blocks are global already
    dst->err = src->err;
    return drop_to_no_data(dst, rc);
  }
  hipError_t e = ppls_launch_xperm_scatter(dst->pm_blk, src->ldx, src->ldy, dst->xp_S, src->stream);
  // ||X||^2, ||Y||^2 are src's: a permutation of rows changes neither
  if (e == hipSuccess) e = hipMemcpyAsync(dst->ssq, src->ssq, 2 * sizeof(double), hipMemcpyDeviceToDevice, src->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(src->stream);
  if (e != hipSuccess) return drop_to_no_data(dst, fail(dst, PPLS_E_HIP, "permute: writing S: %s", hipGetErrorString(e)));
  dst->ssq_host[0] = src->ssq_host[0];
  dst->ssq_host[1] = src->ssq_host[1];
  record_copy(dst, src);
  derived_publish(dst, src->n_total, src->mem_free_min);
  dst->pm_self_serial = dst->xp_serial;
  dst->pm_src_serial = src->xp_serial;
  dst->pm_ms[3] = ms_since(t_call);
  return PPLS_OK;
}

int ppls_xperm_timing(ppls_ctx* c, double* ms4) {
  if (!c || !ms4) return PPLS_E_ARG;
  for (int i = 0; i < 4; ++i) ms4[i] = c->pm_ms[i];
  return PPLS_OK;
}

int ppls_stream_info(ppls_ctx* c, int* state, int64_t* rows_local, int64_t* n_total, int64_t* chunks) {
  if (!c) return PPLS_E_ARG;
  if (state) *state = c->st_state;
  if (rows_local) *rows_local = c->st_state ? c->st_rows : 0;
  if (n_total) *n_total = c->st_state == 2 ? c->n_total : c->st_state == 1 ? c->st_rows : 0;
  if (chunks) *chunks = c->st_state ? c->st_chunks : 0;
  return PPLS_OK;
}

int ppls_stream_fold_info(ppls_ctx* c, int* nfolds, int64_t* fold_total, int* selected) {
  if (!c) return PPLS_E_ARG;
  const int K = c->st_state ? c->st_nfolds : 0;
  if (nfolds) *nfolds = K;
  if (fold_total)
    for (int k = 0; k < K; ++k) fold_total[k] = c->st_fN[(size_t)k];
  if (selected) *selected = c->st_state == 2 && K > 0 ? c->st_sel : -1;
  return PPLS_OK;
}

int ppls_stream_select(ppls_ctx* c, int fold) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = fold_state_check(c))) return rc;
  if (c->em_active)
    return fail(c, PPLS_E_STATE, "an ppls_em_begin session is active on the selected cross-products: finish it before selecting");
  if (fold < -1 || fold >= c->st_nfolds) return fail(c, PPLS_E_ARG, "fold %d outside [-1, %d)", fold, c->st_nfolds);
  HIPCHK(c, hipSetDevice(c->device));
  return fold_select(c, fold);
}

int ppls_heldout_sse_fold(ppls_ctx* c, const double* W, const double* C, const double* B, int k, int fold, double* sse,
                          double* mag) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = fold_state_check(c))) return rc;
  if (!W || !C || !B || !sse || k < 1 || k > PPLS_RMAX)
    return fail(c, PPLS_E_ARG, "W, C, B, sse must be given with 1 <= k <= %d", PPLS_RMAX);
  if (fold < 0 || fold >= c->st_nfolds) return fail(c, PPLS_E_ARG, "fold %d outside [0, %d)", fold, c->st_nfolds);
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  double *Wd = nullptr, *Cd = nullptr, *Bd = nullptr, *work = nullptr, *out = nullptr;
  if ((rc = cv_upload_coef(c, tmp, W, c->p, k, &Wd))) return rc;
  if ((rc = cv_upload_coef(c, tmp, C, c->q, k, &Cd))) return rc;
  if ((rc = cv_upload_coef(c, tmp, B, k, 1, &Bd))) return rc;
  if ((rc = tmp.get(c, &work, (size_t)4 * c->p * k))) return rc;
  if ((rc = tmp.get(c, &out, (size_t)2 * k))) return rc;
  const size_t PP = (size_t)(c->ldx + c->ldy) * (c->ldx + c->ldy);
  std::vector<double> h((size_t)2 * k);
  HIPCHK(c, ppls_launch_cvs_heldout(c->st_fS + (size_t)fold * PP, c->p, c->ldx, c->q, c->ldy, Wd, Cd, Bd, k, work, out, out + k,
                                    c->stream));
  HIPCHK(c, hipMemcpyAsync(h.data(), out, sizeof(double) * 2 * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < k; ++j) {
    sse[j] = h[(size_t)j];
    if (mag) mag[j] = h[(size_t)k + j];
  }
  return PPLS_OK;
}

// ppls_cv_ppls_stream (o2m = false: init holds K * a starting values) and ppls_cv_ppls_stream_o2m.
static int cv_ppls_stream_impl(ppls_ctx* c, int a, int max_steps, double atol, int crit_abs, const ppls_theta* init, bool o2m,
                               double* rmsep, int* ncomp, double* cond) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = fold_state_check(c))) return rc;
  if (c->em_active)
    return fail(c, PPLS_E_STATE, "an ppls_em_begin session is active on the selected cross-products: finish it before cross-validating");
  if ((!o2m && !init) || !rmsep || !ncomp) return fail(c, PPLS_E_ARG, "NULL argument");
  if (a < 1 || a > PPLS_RMAX) return fail(c, PPLS_E_ARG, "nr_comp=%d outside [1,%d]", a, PPLS_RMAX);
  const int K = c->st_nfolds, p = c->p, q = c->q;
  for (int k = 0; !o2m && k < K * a; ++k)
    if (!init[k].W || !init[k].C || !init[k].B || !init[k].sigT) return fail(c, PPLS_E_ARG, "init[%d] has NULL fields", k);
  std::vector<double> W((size_t)p * a), C((size_t)q * a), B((size_t)a), sig((size_t)4 * a), sse((size_t)a), mag((size_t)a);
  auto run = [&]() -> int {
    int r;
    for (int f = 0; f < K; ++f) {
      if ((r = ppls_stream_select(c, f))) return r;
      if (c->n_total < 1) return fail(c, PPLS_E_ARG, "fold %d leaves no training row", f);
      ppls_seq_fit fit;
      memset(&fit, 0, sizeof fit);
      fit.W = W.data();
      fit.C = C.data();
      fit.B = B.data();
      fit.sig = sig.data();
      if ((r = o2m ? ppls_ppls_o2m(c, a, max_steps, atol, crit_abs, nullptr, &fit)
                   : ppls_ppls_ex(c, a, max_steps, atol, crit_abs, init + (size_t)f * a, nullptr, &fit)))
        return r;
      ncomp[f] = fit.ncomp;
      for (int j = 0; j < a; ++j) {
        rmsep[(size_t)f * a + j] = NAN;
        if (cond) cond[(size_t)f * a + j] = NAN;
      }
      if (fit.ncomp < 1) continue;
      if ((r = ppls_heldout_sse_fold(c, W.data(), C.data(), B.data(), fit.ncomp, f, sse.data(), mag.data()))) return r;
      for (int j = 0; j < fit.ncomp; ++j) {
        rmsep[(size_t)f * a + j] = std::sqrt(sse[(size_t)j] / ((double)c->st_fN[(size_t)f] * q));
        if (cond) cond[(size_t)f * a + j] = mag[(size_t)j] / sse[(size_t)j];
      }
    }
    return PPLS_OK;
  };
  rc = run();
  // selected on all folds again, also after an error (whose message stays)
  const std::string err = c->err;
  const int rs = fold_select(c, -1);
  if (rc) c->err = err;
  return rc ? rc : rs;
}

int ppls_cv_ppls_stream(ppls_ctx* c, int a, int max_steps, double atol, int crit_abs, const ppls_theta* init, double* rmsep,
                        int* ncomp, double* cond) {
  return cv_ppls_stream_impl(c, a, max_steps, atol, crit_abs, init, false, rmsep, ncomp, cond);
}

int ppls_cv_ppls_stream_o2m(ppls_ctx* c, int a, int max_steps, double atol, int crit_abs, double* rmsep, int* ncomp,
                            double* cond) {
  return cv_ppls_stream_impl(c, a, max_steps, atol, crit_abs, nullptr, true, rmsep, ncomp, cond);
}

int ppls_stream_fold_get(ppls_ctx* c, int fold, double* S, double* mean, int64_t* n) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = fold_state_check(c))) return rc;
  if (fold < 0 || fold >= c->st_nfolds) return fail(c, PPLS_E_ARG, "fold %d outside [0, %d)", fold, c->st_nfolds);
  const int P = c->ldx + c->ldy;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (S) HIPCHK(c, hipMemcpy(S, c->st_fS + (size_t)fold * P * P, sizeof(double) * P * P, hipMemcpyDeviceToHost));
  if (mean) memcpy(mean, c->st_fmean_h.data() + (size_t)fold * P, sizeof(double) * P);
  if (n) *n = c->st_fN[(size_t)fold];
  return PPLS_OK;
}

}  // extern "C"

namespace {

// The populations of a context streamed with folds: N_j the fold's rows, ssq(X_j), ssq(Y_j) the traces
// of S_j's diagonal blocks in column order; s2 = the whole data's ||X||^2, ||Y||^2 as fold_select(-1)
// forms them (the diagonals added in fold order, then the columns), whatever is selected now.
int stream_pops(ppls_ctx* c, std::vector<MetaPop>& pops, double s2[2]) {
  const int K = c->st_nfolds, P = c->ldx + c->ldy;
  pops.assign((size_t)K, MetaPop());
  std::vector<double> diag, dsum((size_t)P, 0.0);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < K; ++k) {
    HIPCHK(c, diag_to_host(c->st_fS + (size_t)k * P * P, P, diag));
    MetaPop& pp = pops[(size_t)k];
    pp.N = (double)c->st_fN[(size_t)k];
    diag_traces(c, diag, pp.ssq);
    for (int j = 0; j < P; ++j) dsum[(size_t)j] += diag[(size_t)j];
  }
  diag_traces(c, dsum, s2);
  return PPLS_OK;
}

int meta_stream_check(ppls_ctx* c) {
  int rc;
  if ((rc = fold_state_check(c))) return rc;
  if (c->em_active)
    return fail(c, PPLS_E_STATE, "an ppls_em_begin session is active on the selected cross-products: finish it before a meta fit");
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_meta_emstep_stream(ppls_ctx* c, const double* W, const double* C, const double* params_in, double* W_out,
                            double* C_out, double* params_out, double* Cxt, double* Cyu) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = meta_stream_check(c))) return rc;
  if (!W || !C || !params_in || !W_out || !C_out || !params_out) return fail(c, PPLS_E_ARG, "NULL argument");
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure_r(c, 1, 1))) return rc;
  std::vector<MetaPop> pops;
  double s2[2];
  if ((rc = stream_pops(c, pops, s2))) return rc;
  const int npop = (int)pops.size();
  std::vector<double> w(W, W + c->p), cv(C, C + c->q);
  for (int j = 0; j < npop; ++j) pops[j].t = rank1_from_params(params_in, npop, j);
  if ((rc = meta_xprod_all(c, c->st_fS, pops, w, cv))) return rc;
  meta_emstep_finish(pops, c->p, c->q, w, cv, W_out, C_out, params_out, Cxt, Cyu);
  return PPLS_OK;
}

int ppls_meta_ppls_stream(ppls_ctx* c, int max_steps, double atol, int crit_abs, const ppls_theta* init,
                          ppls_meta_fit* out) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = meta_stream_check(c))) return rc;
  if (!init || !init->W || !init->C || !init->B || !init->sigT || !out || !out->W || !out->C || !out->params)
    return fail(c, PPLS_E_ARG, "NULL argument");
  if (max_steps < 1) return fail(c, PPLS_E_ARG, "EMsteps must be >= 1");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<MetaPop> pops;
  double s2[2];
  if ((rc = stream_pops(c, pops, s2))) return rc;
  for (int m = 0; m < 2; ++m)   // check_fit_data's refusal, on all the streamed rows whatever is selected
    if (!(s2[m] > 0.0))
      return fail(c, PPLS_E_ARG,
                  "%c is all zero (sum of squares over all ranks = 0): the PPLS model is degenerate and the "
                  "reference's fit stops on the NA log-likelihood increment it produces (EM_W_multi.R:173,792)",
                  m ? 'Y' : 'X');
  if ((rc = ensure_r(c, 1, max_steps))) return rc;
  const int K = (int)pops.size();
  const Rank1 t0 = rank1_from_init(init, c->p, c->q);
  meta_log_clear(out, max_steps, K);
  std::vector<double> hN, hs;
  meta_pack_counts(pops, hN, hs);
  double Ntot = 0.0;
  for (int j = 0; j < K; ++j) Ntot += hN[(size_t)j];
  return meta_ppls_xprod(c, c->st_fS, K, hN.data(), hs.data(), s2[0], s2[1], Ntot, t0, max_steps, atol, crit_abs, 5, out);
}

int ppls_meta_xprod_info(ppls_ctx* c, int* npop, int64_t* formations, double* form_ms) {
  if (!c) return PPLS_E_ARG;
  if (npop) *npop = c->mx_S ? c->mx_K : 0;
  if (formations) *formations = c->mx_formations;
  if (form_ms) *form_ms = c->mx_form_ms;
  return PPLS_OK;
}

int ppls_xprod_meta_timing(ppls_ctx* c, int reps, double* ms) {
  if (!c || reps < 1 || !ms) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  const bool folds = c->st_state == 2 && c->st_nfolds > 0;
  if (!folds && !(c->st_state == 0 && c->mx_S))
    return fail(c, PPLS_E_STATE, "the context holds no population cross-products");
  const double* S = folds ? c->st_fS : c->mx_S;
  const int K = folds ? c->st_nfolds : c->mx_K, P = c->ldx + c->ldy;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_r(c, 1, 1))) return rc;
  MetaXpScratch x;
  if ((rc = dalloc(c, &x.M, (size_t)K * 2 * P)) || (rc = dalloc(c, &x.stats, (size_t)K * c->part_ld)) ||
      (rc = dalloc(c, &x.sc, (size_t)K)))
    return rc;
  HIPCHK(c, hipMemsetAsync(x.sc, 0, sizeof(PplsScalars) * K, c->stream));   // (the time does not depend on the values)
  HIPCHK(c, hipMemsetAsync(c->W[0], 0, sizeof(double) * c->ldx, c->stream));
  HIPCHK(c, hipMemsetAsync(c->C[0], 0, sizeof(double) * c->ldy, c->stream));
  if ((rc = meta_xprod_pass(c, S, K, x.sc, x.stats, x.M, nullptr))) return rc;   // warm-up
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0));
  HIPCHK(c, hipEventCreate(&e1));
  hipError_t e = hipEventRecord(e0, c->stream);
  for (int i = 0; e == hipSuccess && i < reps; ++i)
    if (meta_xprod_pass(c, S, K, x.sc, x.stats, x.M, nullptr)) e = hipErrorUnknown;
  if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float t = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIPCHK(c, e);
  *ms = (double)t / reps;
  return PPLS_OK;
}

int ppls_rank1_mu_coefficients(const double* params5, double* coef4) {
  if (!params5 || !coef4) return PPLS_E_ARG;
  const PplsRank1 t{params5[0], params5[1], params5[2], params5[3], params5[4]};
  PplsScalars s;
  ppls_rank1_sweep_scalars(&t, &s);
  coef4[0] = s.alpha[0];
  coef4[1] = s.beta[0];
  coef4[2] = s.gamma[0];
  coef4[3] = s.delta[0];
  return PPLS_OK;
}

int ppls_xprod_meta_stats(ppls_ctx* c, const double* W, const double* C, const double* params, double* stats) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (!W || !C || !params || !stats) return fail(c, PPLS_E_ARG, "NULL argument");
  const bool folds = c->st_state == 2 && c->st_nfolds > 0;
  if (!folds && !(c->st_state == 0 && c->mx_S))
    return fail(c, PPLS_E_STATE, "the context holds no population cross-products: stream the rows with "
                                 "ppls_stream_begin_folds, or make a meta_xprod = 1 call");
  const double* S = folds ? c->st_fS : c->mx_S;
  const int K = folds ? c->st_nfolds : c->mx_K;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_r(c, 1, 1))) return rc;
  std::vector<MetaPop> pops((size_t)K);
  for (int j = 0; j < K; ++j) pops[(size_t)j].t = rank1_from_params(params, K, j);
  const std::vector<double> w(W, W + c->p), cv(C, C + c->q);
  if ((rc = meta_xprod_all(c, S, pops, w, cv))) return rc;
  const size_t ld = (size_t)c->p + c->q + 4;
  for (int j = 0; j < K; ++j) {
    double* o = stats + (size_t)j * ld;
    std::copy(pops[(size_t)j].SX.begin(), pops[(size_t)j].SX.end(), o);
    std::copy(pops[(size_t)j].SY.begin(), pops[(size_t)j].SY.end(), o + c->p);
    for (int e = 0; e < 4; ++e) o[(size_t)c->p + c->q + e] = pops[(size_t)j].G[e];
  }
  return PPLS_OK;
}

}  // extern "C"

// ============================================================================ covariate adjustment
// ppls_adjust_data: the resident X, Y <- their least-squares residuals on the design [1 Z] over all
// ranks' rows.  The host holds Z: it centres and unit-scales the columns, orthonormalises
// them by two rounds of Cholesky-QR (one all-reduce of the k x k Gram each) and uploads Q; the device
// forms G = Q'[X Y] in one read of the rows and subtracts Q G in place (ppls_adjust.hip).
// ppls_xprod_adjust: the same adjustment for contexts that hold only S, as a Schur complement.
namespace {

// Sum over ranks of a small host vector (every rank calls; a no-op without other ranks).
int allreduce_hostvec(ppls_ctx* c, std::vector<double>& v) {
  if (!collective(c)) return PPLS_OK;
  int rc;
  CvScratch tmp;
  double* d = nullptr;
  if ((rc = tmp.get(c, &d, v.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(d, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, c->stream));
  if ((rc = allreduce(c, d, v.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(v.data(), d, sizeof(double) * v.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

struct AdjustSides {
  ScaleSide sd[2];
  int L0, L;   // a row of G on the device: X's ldc values, then Y's
  bool nt;
};

AdjustSides adjust_sides(ppls_ctx* c) {
  AdjustSides s{{{c->X, c->ldx, c->p, 0, ppls_scale_plan(c->n_local, c->p, c->dtype, c->num_cus)},
                 {c->Y, c->ldy, c->q, c->p, ppls_scale_plan(c->n_local, c->q, c->dtype, c->num_cus)}},
                0, 0, false};
  s.L0 = s.sd[0].pl.ldc;
  s.L = s.L0 + s.sd[1].pl.ldc;
  s.nt = c->nt_loads > 0 || (c->nt_loads < 0 && 8.0 * c->n_local * (double)(c->ldx + c->ldy) > 256.0 * (1 << 20));
  return s;
}

// The n_local x k1 row-major host Q zero-padded to kt columns, on the device.
int adjust_upload_q(ppls_ctx* c, CvScratch& tmp, const double* Q, int k1, int kt, double** Qd) {
  int rc;
  const int64_t n = c->n_local;
  std::vector<double> pad((size_t)std::max<int64_t>(n, 1) * kt, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < k1; ++a) pad[(size_t)i * kt + a] = Q[(size_t)i * k1 + a];
  if ((rc = tmp.get(c, Qd, pad.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(*Qd, pad.data(), sizeof(double) * pad.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PPLS_OK;
}

// The coefficient pass: Gd (device, kt rows of s.L doubles) = Q'[X Y], all-reduced; G (host) = its k1
// rows over the p + q real columns, row-major.
int adjust_coef_pass(ppls_ctx* c, const AdjustSides& s, CvScratch& tmp, const double* Qd, int k1, int kt, double* Gd,
                     std::vector<double>& G) {
  int rc;
  const int P = c->p + c->q;
  double *part = nullptr, *Gm = nullptr;
  const size_t plen = (size_t)kt * std::max((size_t)s.sd[0].pl.nblocks * s.sd[0].pl.ldc, (size_t)s.sd[1].pl.nblocks * s.sd[1].pl.ldc);
  if ((rc = tmp.get(c, &part, plen))) return rc;
  if ((rc = tmp.get(c, &Gm, (size_t)kt * std::max(s.L0, s.L - s.L0)))) return rc;
  HIPCHK(c, hipMemsetAsync(Gd, 0, sizeof(double) * kt * s.L, c->stream));   // a rank without rows contributes zeros
  CvEvents ev;
  HIPCHK(c, ev.begin(c->stream));
  if (c->n_local > 0)
    for (int m = 0; m < 2; ++m) {
      const ScaleSide& sd = s.sd[m];
      HIPCHK(c, ppls_launch_adjust_partials(sd.data, sd.ld, c->n_local, c->dtype, &sd.pl, Qd, kt, s.nt, part, c->stream));
      HIPCHK(c, ppls_launch_adjust_reduce(part, &sd.pl, kt, Gm, c->stream));
      // this side's kt x ldc block into its columns of the joint rows
      HIPCHK(c, hipMemcpy2DAsync(Gd + (m ? s.L0 : 0), sizeof(double) * s.L, Gm, sizeof(double) * sd.pl.ldc,
                                 sizeof(double) * sd.pl.ldc, (size_t)kt, hipMemcpyDeviceToDevice, c->stream));
    }
  HIPCHK(c, ev.end(c->stream));
  if ((rc = allreduce(c, Gd, (size_t)kt * s.L))) return rc;
  std::vector<double> h((size_t)kt * s.L);
  HIPCHK(c, hipMemcpyAsync(h.data(), Gd, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->adj_ms[0] = ev.ms();
  G.assign((size_t)k1 * P, 0.0);
  for (int a = 0; a < k1; ++a) {
    std::copy(h.begin() + (size_t)a * s.L, h.begin() + (size_t)a * s.L + c->p, G.begin() + (size_t)a * P);
    std::copy(h.begin() + (size_t)a * s.L + s.L0, h.begin() + (size_t)a * s.L + s.L0 + c->q, G.begin() + (size_t)a * P + c->p);
  }
  return PPLS_OK;
}

int adjust_state_check(ppls_ctx* c) {
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NOT_WHILE_OPEN(c, "the data");
  NEED_ROWS(c);
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_adjust_data(ppls_ctx* c, const double* Z, int k, int layout, int intercept) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = adjust_state_check(c))) return rc;
  if (c->adj_k > 0) return fail(c, PPLS_E_STATE, "the data are already adjusted for %d covariates: load them again first", c->adj_k);
  for (size_t j = 0; j < c->sc_scale.size(); ++j)
    if (c->sc_scale[j] != 1.0 || c->sc_center[j] != 0.0)
      return fail(c, PPLS_E_STATE, "the data were scaled on the device: adjust before scaling (resid(), then scale())");
  if (intercept != 0 && intercept != 1) return fail(c, PPLS_E_ARG, "intercept must be 0 or 1");
  const int k1 = k + intercept, kt = ppls_adjust_kt(k1);
  if (k < 1 || !kt) return fail(c, PPLS_E_ARG, "k = %d covariates%s: the design needs 1 .. %d columns", k,
                                intercept ? " and an intercept" : "", PPLS_ADJ_KMAX);
  if (layout != PPLS_LAYOUT_COLMAJOR && layout != PPLS_LAYOUT_ROWMAJOR) return fail(c, PPLS_E_ARG, "unknown layout %d", layout);
  // n_total is the same on every rank, so this refusal needs no collective
  if (c->n_total <= k1)
    return fail(c, PPLS_E_ARG, "%lld rows (over all ranks) for a design of %d columns: no residual degrees of freedom",
                (long long)c->n_total, k1);
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t n = c->n_local;
  const int p = c->p, q = c->q, P = p + q;
  const double N = (double)c->n_total;

  // this rank's rows of Z, row-major; a NULL or non-finite Z rides in the first all-reduce, so that
  // every rank refuses alike
  std::vector<double> A((size_t)std::max<int64_t>(n, 1) * k, 0.0), red((size_t)k + 1, 0.0);
  if (n > 0 && !Z) {
    red[(size_t)k] = 1.0;
  } else {
    for (int64_t i = 0; i < n; ++i)
      for (int j = 0; j < k; ++j) {
        const double z = layout == PPLS_LAYOUT_ROWMAJOR ? Z[(size_t)i * k + j] : Z[(size_t)j * n + i];
        if (!std::isfinite(z)) red[(size_t)k] += 1.0;
        A[(size_t)i * k + j] = z;
      }
    if (red[(size_t)k] == 0.0)
      for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) red[(size_t)j] += A[(size_t)i * k + j];
  }
  if ((rc = allreduce_hostvec(c, red))) return rc;
  if (red[(size_t)k] > 0.0)
    return fail(c, PPLS_E_ARG, "Z is NULL on a rank with rows, or holds NaN or Inf (%.0f such values or ranks): the data "
                               "are unchanged", red[(size_t)k]);
  std::vector<double> zc((size_t)k, 0.0);
  if (intercept)
    for (int j = 0; j < k; ++j) zc[(size_t)j] = red[(size_t)j] / N;
  // the design T = [1 / sqrt(N) | Z - zc], n_local x k1 row-major.  The constant column goes through the
  // Cholesky-QR rounds with the others: a centred column is orthogonal to it only up to rounding, and
  // round 1 divides that remainder by the column's pivot
  std::vector<double> Q((size_t)std::max<int64_t>(n, 1) * k1, 0.0);
  for (int64_t i = 0; i < n; ++i) {
    if (intercept) Q[(size_t)i * k1] = 1.0 / std::sqrt(N);
    for (int j = 0; j < k; ++j) Q[(size_t)i * k1 + intercept + j] = A[(size_t)i * k + j] - zc[(size_t)j];
  }

  // round 1: the Gram of T, brought to unit diagonal (= the Gram of the unit-norm columns), and
  // lm.fit's pivot rule on its Cholesky factor
  std::vector<double> G1((size_t)k1 * k1), L1((size_t)k1 * k1), L2((size_t)k1 * k1), nrm((size_t)k1, 1.0);
  ppls_adj_gram(Q.data(), n, k1, G1.data());
  if ((rc = allreduce_hostvec(c, G1))) return rc;
  for (int j = 0; j < k; ++j) {
    const double cc = G1[(size_t)(intercept + j) * k1 + intercept + j], raw = cc + N * zc[(size_t)j] * zc[(size_t)j];
    nrm[(size_t)(intercept + j)] = std::sqrt(cc);
    if (!(std::sqrt(cc) > PPLS_ADJ_TOL * std::sqrt(raw)) || !std::isfinite(cc))
      return fail(c, PPLS_E_ARG, "covariate column %d is %s (over all ranks): it is aliased and would be dropped by "
                                 "lm(); the data are unchanged", j + 1, intercept ? "constant beside the intercept" : "zero");
  }
  for (int a = 0; a < k1; ++a)
    for (int b = 0; b < k1; ++b)
      G1[(size_t)a * k1 + b] = a == b ? 1.0 : G1[(size_t)a * k1 + b] / (nrm[(size_t)a] * nrm[(size_t)b]);
  int piv = ppls_adj_chol(G1.data(), k1, PPLS_ADJ_TOL, L1.data());
  if (piv)
    return fail(c, PPLS_E_ARG, "covariate column %d is aliased: given the columns before it%s, at most %g of its norm is "
                               "left (lm.fit's tol); the data are unchanged", piv - intercept,
                intercept ? " and the intercept" : "", PPLS_ADJ_TOL);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < k1; ++j) Q[(size_t)i * k1 + j] /= nrm[(size_t)j];
  ppls_adj_solve_rows(Q.data(), n, k1, L1.data());
  // round 2 (Cholesky-QR2): the Gram of Q1 is within u kappa^2 of I
  ppls_adj_gram(Q.data(), n, k1, G1.data());
  if ((rc = allreduce_hostvec(c, G1))) return rc;
  if ((piv = ppls_adj_chol(G1.data(), k1, 0.0, L2.data())))
    return fail(c, PPLS_E_ARG, "design column %d: the second Cholesky-QR round lost positive definiteness; the data are "
                               "unchanged", piv);
  ppls_adj_solve_rows(Q.data(), n, k1, L2.data());

  const AdjustSides s = adjust_sides(c);
  CvScratch tmp;
  double *Qd = nullptr, *Gd = nullptr;
  std::vector<double> G;
  if ((rc = adjust_upload_q(c, tmp, Q.data(), k1, kt, &Qd))) return rc;
  if ((rc = tmp.get(c, &Gd, (size_t)kt * s.L))) return rc;
  c->adj_ms[0] = c->adj_ms[1] = 0.0;
  if ((rc = adjust_coef_pass(c, s, tmp, Qd, k1, kt, Gd, G))) return rc;
  for (size_t e = 0; e < G.size(); ++e)
    if (!std::isfinite(G[e])) return fail(c, PPLS_E_NUMERIC, "the coefficients Q'[X Y] are not finite; the data are unchanged");

  // from here the rows change
  c->rb_kept = false;
  c->em_active = false;
  c->xp_active = false;
  {
    CvEvents ev;
    HIPCHK(c, ev.begin(c->stream));
    if (n > 0)
      for (int m = 0; m < 2; ++m) {
        const ScaleSide& sd = s.sd[m];
        HIPCHK(c, ppls_launch_adjust_apply(sd.data, sd.ld, n, sd.cols, c->dtype, &sd.pl, Qd, Gd + (m ? s.L0 : 0), s.L, kt, s.nt,
                                           c->stream));
      }
    HIPCHK(c, ev.end(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->adj_ms[1] = ev.ms();
  }
  // the record: T diag(1 / nrm) = Q L2' L1', so the fit Q G = T diag(1 / nrm) H with H = L1^-T L2^-T G:
  // Gamma = diag(1 / nrm) H's covariate rows, and the constant's share H_0 / sqrt(N) is the column mean
  std::vector<double> H = G;
  ppls_adj_backsolve(L2.data(), k1, H.data(), P);
  ppls_adj_backsolve(L1.data(), k1, H.data(), P);
  c->adj_k = k;
  c->adj_zcenter = zc;
  c->adj_gamma.assign((size_t)k * P, 0.0);
  for (int a = 0; a < k; ++a)
    for (int j = 0; j < P; ++j) c->adj_gamma[(size_t)a * P + j] = H[(size_t)(intercept + a) * P + j] / nrm[(size_t)(intercept + a)];
  c->sc_center.assign((size_t)P, 0.0);
  c->sc_scale.assign((size_t)P, 1.0);
  if (intercept)
    for (int j = 0; j < P; ++j) c->sc_center[(size_t)j] = H[(size_t)j] / std::sqrt(N);
  c->adj_ss.assign((size_t)P, 0.0);
  for (int a = 0; a < k1; ++a)
    for (int j = 0; j < P; ++j) c->adj_ss[(size_t)j] += G[(size_t)a * P + j] * G[(size_t)a * P + j];
  // the context is what ppls_set_data of the residuals would have left (as after ppls_scale_data)
  if ((rc = compute_ssq(c))) return rc;
  return check_finite_data(c);
}

int ppls_get_adjustment(ppls_ctx* c, int* k, double* zcenter, double* Gamma) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (k) *k = c->adj_k;
  if (zcenter) std::copy(c->adj_zcenter.begin(), c->adj_zcenter.end(), zcenter);
  if (Gamma) std::copy(c->adj_gamma.begin(), c->adj_gamma.end(), Gamma);
  return PPLS_OK;
}

int ppls_adjust_explained(ppls_ctx* c, double* ss) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data || c->adj_k < 1 || c->adj_ss.size() != (size_t)(c->p + c->q))
    return fail(c, PPLS_E_STATE, "no ppls_adjust_data on these data");
  if (ss) std::copy(c->adj_ss.begin(), c->adj_ss.end(), ss);
  return PPLS_OK;
}

int ppls_adjust_coef(ppls_ctx* c, const double* Q, int k1, double* G) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = adjust_state_check(c))) return rc;
  const int kt = ppls_adjust_kt(k1);
  if (!kt) return fail(c, PPLS_E_ARG, "k1 = %d outside [1, %d]", k1, PPLS_ADJ_KMAX);
  if (!G || (c->n_local > 0 && !Q)) return fail(c, PPLS_E_ARG, "NULL argument");
  HIPCHK(c, hipSetDevice(c->device));
  const AdjustSides s = adjust_sides(c);
  CvScratch tmp;
  double *Qd = nullptr, *Gd = nullptr;
  std::vector<double> g;
  if ((rc = adjust_upload_q(c, tmp, Q, k1, kt, &Qd))) return rc;
  if ((rc = tmp.get(c, &Gd, (size_t)kt * s.L))) return rc;
  if ((rc = adjust_coef_pass(c, s, tmp, Qd, k1, kt, Gd, g))) return rc;
  std::copy(g.begin(), g.end(), G);
  return PPLS_OK;
}

int ppls_adjust_info(ppls_ctx* c, int k1, int* kt, int64_t* plans) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = adjust_state_check(c))) return rc;
  const int t = ppls_adjust_kt(k1);
  if (!t) return fail(c, PPLS_E_ARG, "k1 = %d outside [1, %d]", k1, PPLS_ADJ_KMAX);
  if (kt) *kt = t;
  if (plans) {
    const AdjustSides s = adjust_sides(c);
    for (int m = 0; m < 2; ++m) {
      const PplsScalePlan& pl = s.sd[m].pl;
      const int64_t v[5] = {pl.tx, pl.ty, pl.grid_x, pl.grid_y, pl.nblocks};
      std::copy(v, v + 5, plans + 5 * m);
    }
  }
  return PPLS_OK;
}

int ppls_adjust_timing(ppls_ctx* c, double* ms4) {
  if (!c) return PPLS_E_ARG;
  for (int k = 0; k < 4; ++k)
    if (ms4) ms4[k] = c->adj_ms[k];
  return PPLS_OK;
}

}  // extern "C"

namespace {

// What ppls_xprod_adjust and ppls_xadjust_matrix share: from the k trailing rows of src (host copy Zr,
// k x P_src: joint columns of src) F (PPLS_ADJ_KMAX x P_dst, zero where nothing is live), Gamma (k x
// (p + q), src's units) and the Schur diagonal over dst's joint columns, by the kernel's own fma chain.
struct SchurPlan {
  std::vector<double> F, gamma, diag;
};

int schur_plan(ppls_ctx* e, const std::vector<double>& Zr, const std::vector<double>& sdiag, int P_src, int p, int ldx,
               int q, int ldy_dst, int k, SchurPlan* out) {
  const int P = ldx + ldy_dst, z0 = ldx + q;   // the covariates: src's joint columns z0 .. z0 + k - 1
  std::vector<double> C((size_t)k * k), L((size_t)k * k), d((size_t)k);
  for (int a = 0; a < k; ++a) {
    d[(size_t)a] = std::sqrt(Zr[(size_t)a * P_src + z0 + a]);
    if (!(d[(size_t)a] > 0.0) || !std::isfinite(d[(size_t)a]))
      return fail(e, PPLS_E_ARG, "covariate column %d has sum of squares %g: S_zz is singular", a + 1,
                  Zr[(size_t)a * P_src + z0 + a]);
  }
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < k; ++b) {
      const double v = a >= b ? Zr[(size_t)a * P_src + z0 + b] : Zr[(size_t)b * P_src + z0 + a];   // the lower triangle
      C[(size_t)a * k + b] = a == b ? 1.0 : v / (d[(size_t)a] * d[(size_t)b]);
    }
  const int piv = ppls_adj_chol(C.data(), k, PPLS_ADJ_TOL, L.data());
  if (piv)
    return fail(e, PPLS_E_ARG, "covariate column %d is aliased: given the columns before it at most %g of its norm is left "
                               "(lm.fit's tol): S_zz is singular", piv, PPLS_ADJ_TOL);
  // F' = Lc^-1 D^-1 S_zd over dst's live joint columns
  std::vector<double> Ft((size_t)k * P, 0.0);
  auto live = [&](int c) { return c < p || (c >= ldx && c < ldx + q); };
  for (int a = 0; a < k; ++a)
    for (int c = 0; c < P; ++c)
      if (live(c)) Ft[(size_t)a * P + c] = Zr[(size_t)a * P_src + c] / d[(size_t)a];
  ppls_adj_fwdsolve(L.data(), k, Ft.data(), P);
  out->F.assign((size_t)PPLS_ADJ_KMAX * P, 0.0);
  std::copy(Ft.begin(), Ft.end(), out->F.begin());
  out->diag.assign((size_t)P, 0.0);
  for (int c = 0; c < P; ++c)
    if (live(c)) {
      double v = sdiag[(size_t)c];
      for (int a = 0; a < k; ++a) v = std::fma(-Ft[(size_t)a * P + c], Ft[(size_t)a * P + c], v);
      out->diag[(size_t)c] = v;
    }
  // Gamma = S_zz^-1 S_zd = D^-1 Lc^-T F'
  ppls_adj_backsolve(L.data(), k, Ft.data(), P);
  out->gamma.assign((size_t)k * (p + q), 0.0);
  for (int a = 0; a < k; ++a) {
    for (int j = 0; j < p; ++j) out->gamma[(size_t)a * (p + q) + j] = Ft[(size_t)a * P + j] / d[(size_t)a];
    for (int j = 0; j < q; ++j) out->gamma[(size_t)a * (p + q) + p + j] = Ft[(size_t)a * P + ldx + j] / d[(size_t)a];
  }
  return PPLS_OK;
}

// d (joint layout of dst, 1 where nothing is divided) from the Schur diagonal: sqrt(diag / denom).
int schur_scale(ppls_ctx* e, const SchurPlan& pl, int p, int ldx, int q, double denom, std::vector<double>* d) {
  d->assign(pl.diag.size(), 1.0);
  for (int j = 0; j < p + q; ++j) {
    const int c = j < p ? j : ldx + (j - p);
    const double v = std::sqrt(pl.diag[(size_t)c] / denom);
    if (!(v > 0.0) || !std::isfinite(v))
      return fail(e, PPLS_E_ARG, "%c column %d has standard deviation %g after the adjustment: scale = 1 would fill it with "
                                 "NaN or Inf", j < p ? 'X' : 'Y', (j < p ? j : j - p) + 1, v);
    (*d)[(size_t)c] = v;
  }
  return PPLS_OK;
}

}  // namespace

extern "C" {

int ppls_xprod_adjust(ppls_ctx* dst, ppls_ctx* src, int k, int scale) {
  int rc;
  if ((rc = pair_check(dst, src))) return rc;
  if (!src->have_data) return fail(dst, PPLS_E_STATE, "the source context has no data");
  if (src->st_state == 1) return fail(dst, PPLS_E_STATE, "the source's stream is open: call ppls_stream_end first");
  if (dst->st_state == 1) return fail(dst, PPLS_E_STATE, "a stream is open on the destination");
  if (src->st_state == 2 && src->st_nfolds > 0)
    return fail(dst, PPLS_E_STATE, "the source was streamed with folds: per-fold adjustment is not provided");
  if (k < 1 || k > PPLS_ADJ_KMAX || k >= src->q)
    return fail(dst, PPLS_E_ARG, "k = %d covariates: needs 1 <= k <= %d and k < the source's %d Y columns", k, PPLS_ADJ_KMAX,
                src->q);
  if (scale != 0 && scale != 1) return fail(dst, PPLS_E_ARG, "scale must be 0 or 1");
  if (scale && src->n_total < 2) return fail(dst, PPLS_E_ARG, "scale = 1 needs at least 2 rows");
  HIPCHK(dst, hipSetDevice(src->device));
  // resident rows: S of all of them first, formed and kept (a collective of its own when sharded)
  if ((rc = xprod_setup(src))) {
    dst->err = src->err;
    return rc;
  }
  if (!src->xp_ready || !src->xp_S) return fail(dst, PPLS_E_STATE, "the source holds no cross-products");
  const int p = src->p, q = src->q - k, ldx = src->ldx, P_src = src->ldx + src->ldy;
  const int ldy = ld_of(q, src->dtype, src->ldpad), P = ldx + ldy, z0 = ldx + q;
  if (P > P_src) return fail(dst, PPLS_E_STATE, "the destination's layout (%d) exceeds the source's (%d)", P, P_src);
  // host: the k trailing rows of S and its diagonal (S is the same on every rank: no collective below)
  std::vector<double> Zr((size_t)k * P_src), sdiag;
  HIPCHK(dst, hipStreamSynchronize(src->stream));
  HIPCHK(dst, hipMemcpy(Zr.data(), src->xp_S + (size_t)z0 * P_src, sizeof(double) * Zr.size(), hipMemcpyDeviceToHost));
  HIPCHK(dst, diag_to_host(src->xp_S, P_src, sdiag));
  SchurPlan pl;
  std::vector<double> d;
  if ((rc = schur_plan(dst, Zr, sdiag, P_src, p, ldx, q, ldy, k, &pl))) return rc;
  if (scale && (rc = schur_scale(dst, pl, p, ldx, q, (double)(src->n_total - 1), &d))) return rc;
  CvScratch tmp;
  double *Fd = nullptr, *dd = nullptr;
  DevGuard Snew;
  if ((rc = tmp.get(src, &Fd, pl.F.size())) || (scale && (rc = tmp.get(src, &dd, d.size())))) {
    dst->err = src->err;
    return rc;
  }
  const bool reuse = derived_reuse(dst, p, q, ldx, ldy);
  if (!reuse && (rc = dalloc(dst, &Snew.p, (size_t)P * P))) return rc;
  // the records, before dst's own are cleared (dst may be adjusted already; src's are read only)
  std::vector<double> cen((size_t)(p + q), 0.0), scl((size_t)(p + q), 1.0), zc((size_t)k, 0.0);
  for (int j = 0; j < p + q; ++j) {
    if (!src->sc_center.empty()) {
      cen[(size_t)j] = src->sc_center[(size_t)j];
      scl[(size_t)j] = src->sc_scale[(size_t)j];
    }
    if (scale) scl[(size_t)j] *= d[(size_t)(j < p ? j : ldx + (j - p))];
  }
  if (!src->sc_center.empty())
    for (int a = 0; a < k; ++a) zc[(size_t)a] = src->sc_center[(size_t)(p + q + a)];
  // From here dst ends streamed on the adjusted S, or without data.
  if ((rc = derived_begin(dst, "adjust", "the planned", src->dtype, src->ldpad, p, q, ldx, ldy, Snew, reuse)))
    return drop_to_no_data(dst, rc);
  hipError_t e = hipMemcpyAsync(Fd, pl.F.data(), sizeof(double) * pl.F.size(), hipMemcpyHostToDevice, src->stream);
  if (e == hipSuccess && scale) e = hipMemcpyAsync(dd, d.data(), sizeof(double) * d.size(), hipMemcpyHostToDevice, src->stream);
  CvEvents ev;
  if (e == hipSuccess) e = ev.begin(src->stream);
  if (e == hipSuccess) e = ppls_launch_adjust_schur(src->xp_S, P_src, dst->xp_S, p, ldx, q, ldy, Fd, k, src->stream);
  if (e == hipSuccess) e = ev.end(src->stream);
  CvEvents ev2;
  if (e == hipSuccess) e = ev2.begin(src->stream);
  if (e == hipSuccess && scale) e = ppls_launch_stream_standardise(dst->xp_S, p, ldx, q, ldy, dd, src->stream);
  if (e == hipSuccess) e = ev2.end(src->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(src->stream);
  if (e == hipSuccess) {
    dst->adj_ms[2] = ev.ms();
    dst->adj_ms[3] = scale ? ev2.ms() : 0.0;
    e = derived_traces(dst, P);
  }
  if (e != hipSuccess) return drop_to_no_data(dst, fail(dst, PPLS_E_HIP, "adjust: the Schur pass: %s", hipGetErrorString(e)));
  if ((rc = traces_finite(dst, dst->ssq_host))) return drop_to_no_data(dst, rc);
  record_set(dst, cen, scl, k, zc, pl.gamma);
  derived_publish(dst, src->n_total, src->mem_free_min);
  return PPLS_OK;
}

int ppls_xadjust_matrix(ppls_ctx* c, const double* S_src, int p, int ldx, int q_src, int ldy_src, int k, int ldy_dst,
                        int scale, double* S_dst) {
  if (!c) return PPLS_E_ARG;
  if (!S_src || !S_dst) return fail(c, PPLS_E_ARG, "NULL argument");
  const int q = q_src - k;
  if (k < 1 || k > PPLS_ADJ_KMAX || q < 1) return fail(c, PPLS_E_ARG, "k = %d outside [1, min(%d, q_src - 1)]", k, PPLS_ADJ_KMAX);
  auto shape_ok = [](int cx, int lx, int cy, int ly) {   // the joint layouts ppls_symtile.h takes
    return cx >= 1 && cy >= 1 && cx <= lx && cy <= ly && lx % 2 == 0 && ly % 2 == 0 && (int64_t)lx + ly < (1 << 30);
  };
  if (!shape_ok(p, ldx, q_src, ldy_src) || !shape_ok(p, ldx, q, ldy_dst) || ldy_dst > ldy_src)
    return fail(c, PPLS_E_ARG, "bad layout: p %d in %d, q %d in %d, %d in %d", p, ldx, q_src, ldy_src, q, ldy_dst);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const int P_src = ldx + ldy_src, P = ldx + ldy_dst, z0 = ldx + q;
  std::vector<double> Zr(S_src + (size_t)z0 * P_src, S_src + (size_t)(z0 + k) * P_src), sdiag((size_t)P_src), d;
  for (int j = 0; j < P_src; ++j) sdiag[(size_t)j] = S_src[(size_t)j * P_src + j];
  SchurPlan pl;
  if ((rc = schur_plan(c, Zr, sdiag, P_src, p, ldx, q, ldy_dst, k, &pl))) return rc;
  if (scale && (rc = schur_scale(c, pl, p, ldx, q, 1.0, &d))) return rc;
  // NaN around the output: entries the kernel must not leave (it writes all P x P) and slack behind it
  CvScratch tmp;
  double *Sd = nullptr, *Dd = nullptr, *Fd = nullptr, *dd = nullptr;
  const size_t guard = 64;
  if ((rc = tmp.get(c, &Sd, (size_t)P_src * P_src)) || (rc = tmp.get(c, &Dd, (size_t)P * P + 2 * guard)) ||
      (rc = tmp.get(c, &Fd, pl.F.size())) || (scale && (rc = tmp.get(c, &dd, d.size()))))
    return rc;
  HIPCHK(c, hipMemcpyAsync(Sd, S_src, sizeof(double) * P_src * P_src, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(Dd, 0xFF, sizeof(double) * ((size_t)P * P + 2 * guard), c->stream));
  HIPCHK(c, hipMemcpyAsync(Fd, pl.F.data(), sizeof(double) * pl.F.size(), hipMemcpyHostToDevice, c->stream));
  if (scale) HIPCHK(c, hipMemcpyAsync(dd, d.data(), sizeof(double) * d.size(), hipMemcpyHostToDevice, c->stream));
  CvEvents ev;
  HIPCHK(c, ev.begin(c->stream));
  HIPCHK(c, ppls_launch_adjust_schur(Sd, P_src, Dd + guard, p, ldx, q, ldy_dst, Fd, k, c->stream));
  HIPCHK(c, ev.end(c->stream));
  if (scale) HIPCHK(c, ppls_launch_stream_standardise(Dd + guard, p, ldx, q, ldy_dst, dd, c->stream));
  std::vector<double> h((size_t)P * P + 2 * guard);
  HIPCHK(c, hipMemcpyAsync(h.data(), Dd, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->adj_ms[2] = ev.ms();
  for (size_t g = 0; g < guard; ++g)
    if (!std::isnan(h[g]) || !std::isnan(h[guard + (size_t)P * P + g]))
      return fail(c, PPLS_E_NUMERIC, "the Schur kernel wrote outside its P x P output");
  std::copy(h.begin() + guard, h.begin() + guard + (size_t)P * P, S_dst);
  return PPLS_OK;
}

}  // extern "C"

// ============================================================================ PO2PLS
// X- and Y-specific components fitted from S (ppls_po2.hip).  Replaces the reference's loglC
// (Package/PPLS/src/loglC.cpp:36-113) and EMstepC (:116-250) and supplies the M-step it lacks (:228).
namespace {

struct Po2Shape {
  int r, rx, ry, kx, ky, k;
};

// The device side of one PO2 call: scratch that lives as long as the call, and the kernels' arguments.
struct Po2Dev {
  CvScratch tmp;
  PplsPo2Args a{};
  double *Gx0 = nullptr, *Gy0 = nullptr;   // timing: the uploaded theta, to restore it
  PplsPo2Scalars* sc0 = nullptr;
  PplsPo2Scalars hsc{};
  int rw = 0;
};

int po2_shape(ppls_ctx* c, int r, int rx, int ry, int p, int q, Po2Shape* s) {
  if (r < 1 || rx < 0 || ry < 0 || r + rx > PPLS_RMAX || r + ry > PPLS_RMAX || r + rx > p || r + ry > q)
    return fail(c, PPLS_E_ARG, "PO2PLS sizes r=%d rx=%d ry=%d outside r >= 1, rx, ry >= 0, r + rx <= min(%d, p=%d), r + ry <= min(%d, q=%d)",
                r, rx, ry, PPLS_RMAX, p, PPLS_RMAX, q);
  *s = {r, rx, ry, r + rx, r + ry, 2 * r + rx + ry};
  return PPLS_OK;
}

bool po2_sigma_ok(double v) { return std::isfinite(v) && v > 0.0; }

int po2_check_scalars(ppls_ctx* c, const ppls_po2_theta* th, const Po2Shape& s) {
  if (!th || !th->B || !th->sigT || (s.rx && !th->sigTo) || (s.ry && !th->sigUo)) return fail(c, PPLS_E_ARG, "NULL argument");
  bool ok = po2_sigma_ok(th->sigE) && po2_sigma_ok(th->sigF) && po2_sigma_ok(th->sigH);
  for (int j = 0; j < s.r; ++j) ok = ok && po2_sigma_ok(th->sigT[j]) && std::isfinite(th->B[j]);
  for (int j = 0; j < s.rx; ++j) ok = ok && po2_sigma_ok(th->sigTo[j]);
  for (int j = 0; j < s.ry; ++j) ok = ok && po2_sigma_ok(th->sigUo[j]);
  if (!ok) return fail(c, PPLS_E_ARG, "PO2PLS theta: every sigma must be finite and above 0, B finite");
  return PPLS_OK;
}

int po2_check_theta(ppls_ctx* c, const ppls_po2_theta* th, const Po2Shape& s, int p, int q) {
  int rc;
  if ((rc = po2_check_scalars(c, th, s))) return rc;
  if (!th->W || !th->C || (s.rx && !th->Wo) || (s.ry && !th->Co)) return fail(c, PPLS_E_ARG, "NULL argument");
  bool ok = true;
  for (size_t e = 0; e < (size_t)p * s.r && ok; ++e) ok = std::isfinite(th->W[e]);
  for (size_t e = 0; e < (size_t)p * s.rx && ok; ++e) ok = std::isfinite(th->Wo[e]);
  for (size_t e = 0; e < (size_t)q * s.r && ok; ++e) ok = std::isfinite(th->C[e]);
  for (size_t e = 0; e < (size_t)q * s.ry && ok; ++e) ok = std::isfinite(th->Co[e]);
  if (!ok) return fail(c, PPLS_E_ARG, "PO2PLS theta: non-finite loadings");
  return PPLS_OK;
}

void po2_pack_scalars(const ppls_po2_theta* th, const Po2Shape& s, PplsPo2Scalars* h) {
  memset(h, 0, sizeof *h);
  for (int j = 0; j < s.r; ++j) { h->b[j] = th->B[j]; h->sT[j] = th->sigT[j]; }
  for (int j = 0; j < s.rx; ++j) h->sTo[j] = th->sigTo[j];
  for (int j = 0; j < s.ry; ++j) h->sUo[j] = th->sigUo[j];
  h->sE = th->sigE; h->sF = th->sigF; h->sH = th->sigH;
}

// [A | Ao] (rows x (ca + co), column-major) into ld-padded device columns (padding rows zero).
int po2_upload_side(ppls_ctx* c, const double* A, int ca, const double* Ao, int co, int rows, int ld, double* dst) {
  std::vector<double> h((size_t)ld * (ca + co), 0.0);
  for (int j = 0; j < ca; ++j) std::copy(A + (size_t)j * rows, A + (size_t)(j + 1) * rows, h.begin() + (size_t)j * ld);
  for (int j = 0; j < co; ++j) std::copy(Ao + (size_t)j * rows, Ao + (size_t)(j + 1) * rows, h.begin() + (size_t)(ca + j) * ld);
  HIPCHK(c, hipMemcpy(dst, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
  return PPLS_OK;
}

// Scratch, arguments and theta on the device, for the context's S.
int po2_setup(ppls_ctx* c, Po2Dev& d, const ppls_po2_theta* th, const Po2Shape& s, int hist, bool keep_copy) {
  int rc;
  const int ldx = c->ldx, ldy = c->ldy, P = ldx + ldy;
  PplsPo2Args& a = d.a;
  int* ints = nullptr;
  if ((rc = d.tmp.get(c, &a.Gx, (size_t)ldx * s.kx)) || (rc = d.tmp.get(c, &a.Gy, (size_t)ldy * s.ky)) ||
      (rc = d.tmp.get(c, &a.sc, 1)) || (rc = d.tmp.get(c, &a.M, (size_t)P * s.k)) || (rc = d.tmp.get(c, &a.Q, (size_t)s.k * s.k)) ||
      (rc = d.tmp.get(c, &a.GGx, (size_t)s.kx * s.kx)) || (rc = d.tmp.get(c, &a.GGy, (size_t)s.ky * s.ky)) ||
      (rc = d.tmp.get(c, &a.sm, 1)) || (rc = d.tmp.get(c, &a.Z, (size_t)PPLS_RMAX * P)) ||
      (rc = d.tmp.get(c, &a.loglik, (size_t)hist)) || (rc = d.tmp.get(c, &ints, 4)))
    return rc;
  if (keep_copy && ((rc = d.tmp.get(c, &d.Gx0, (size_t)ldx * s.kx)) || (rc = d.tmp.get(c, &d.Gy0, (size_t)ldy * s.ky)) ||
                    (rc = d.tmp.get(c, &d.sc0, 1))))
    return rc;
  HIPCHK(c, hipMemset(ints, 0, 4 * sizeof(int)));
  a.status = ints;
  a.stop = nullptr;
  a.stop_mirror = nullptr;
  a.My = a.M + (size_t)s.kx * P;
  a.S = c->xp_S;
  a.ldx = ldx; a.ldy = ldy; a.p = c->p; a.q = c->q; a.r = s.r; a.rx = s.rx; a.ry = s.ry;
  a.N = (double)c->n_total; a.ssqX = c->ssq_host[0]; a.ssqY = c->ssq_host[1]; a.atol = 0.0;
  if ((rc = po2_upload_side(c, th->W, s.r, th->Wo, s.rx, c->p, ldx, a.Gx))) return rc;
  if ((rc = po2_upload_side(c, th->C, s.r, th->Co, s.ry, c->q, ldy, a.Gy))) return rc;
  po2_pack_scalars(th, s, &d.hsc);
  HIPCHK(c, hipMemcpy(a.sc, &d.hsc, sizeof d.hsc, hipMemcpyHostToDevice));
  if (keep_copy) {
    HIPCHK(c, hipMemcpy(d.Gx0, a.Gx, sizeof(double) * ldx * s.kx, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(d.Gy0, a.Gy, sizeof(double) * ldy * s.ky, hipMemcpyDeviceToDevice));
    HIPCHK(c, hipMemcpy(d.sc0, a.sc, sizeof d.hsc, hipMemcpyDeviceToDevice));
  }
  // rows of S per wave: the tile kernel's rule at the wider panel (option xprod_rw forces it where it fits)
  const int wmax = std::max(s.kx, s.ky);
  d.rw = ppls_xprod_tile_rows(P, wmax, c->xprod_rw, c->num_cus);
  return PPLS_OK;
}

// M = S G by the two panels (X columns with Gx, Y columns with Gy): one read of S.
int po2_panels(ppls_ctx* c, const PplsPo2Args& a, int kx, int ky, int rw) {
  const int P = a.ldx + a.ldy;
  HIPCHK(c, ppls_launch_po2_panel(a.S, P, 0, a.ldx, a.Gx, a.ldx, kx, rw, a.M, a.stop, c->stream));
  HIPCHK(c, ppls_launch_po2_panel(a.S, P, a.ldx, a.ldy, a.Gy, a.ldy, ky, rw, a.My, a.stop, c->stream));
  return PPLS_OK;
}

int po2_pass(ppls_ctx* c, Po2Dev& d, const Po2Shape& s) {
  int rc;
  if ((rc = po2_panels(c, d.a, s.kx, s.ky, d.rw))) return rc;
  HIPCHK(c, ppls_launch_po2_gram(&d.a, c->stream));
  return PPLS_OK;
}

int po2_status(ppls_ctx* c, const Po2Dev& d) {
  int st = 0;
  HIPCHK(c, hipMemcpy(&st, d.a.status, sizeof st, hipMemcpyDeviceToHost));
  switch (st) {
    case 0: return PPLS_OK;
    case PPLS_PO2_ST_SIGMA: return fail(c, PPLS_E_NUMERIC, "PO2PLS: a sigma is not finite and above 0 (status %d)", st);
    case PPLS_PO2_ST_LAMBDA: return fail(c, PPLS_E_NUMERIC, "PO2PLS: Lambda = Sigma_z^-1 + D G'G is not positive definite (status %d)", st);
    case PPLS_PO2_ST_VAR: return fail(c, PPLS_E_NUMERIC, "PO2PLS: an updated variance is not finite and above 0 (status %d)", st);
    default: return fail(c, PPLS_E_NUMERIC, "PO2PLS: rank-deficient loading update (status %d)", st);
  }
}

void po2_block(const std::vector<double>& Z, int k, int r0, int nr, int c0, int nc, double* out) {
  if (!out) return;
  for (int j = 0; j < nc; ++j)
    for (int i = 0; i < nr; ++i) out[(size_t)j * nr + i] = Z[(size_t)(c0 + j) * k + r0 + i];
}

// The moment blocks of *sm; with M (P x k, device) also C_dz = M K / N.
int po2_expect_out(ppls_ctx* c, const PplsPo2Args& a, const Po2Shape& s, bool with_M, ppls_po2_expect* out) {
  if (!out) return PPLS_OK;
  std::vector<PplsPo2Small> hv(1);
  PplsPo2Small& h = hv[0];
  HIPCHK(c, hipMemcpy(&h, a.sm, sizeof h, hipMemcpyDeviceToHost));
  const int k = s.k, r = s.r, kx = s.kx;
  std::vector<double> Z(h.Czz, h.Czz + (size_t)k * k);
  po2_block(Z, k, 0, r, 0, r, out->Ctt);
  po2_block(Z, k, r, s.rx, r, s.rx, out->Ctoto);
  po2_block(Z, k, 0, r, r, s.rx, out->Ctto);
  po2_block(Z, k, kx, r, kx, r, out->Cuu);
  po2_block(Z, k, kx + r, s.ry, kx + r, s.ry, out->Cuouo);
  po2_block(Z, k, kx, r, kx + r, s.ry, out->Cuuo);
  po2_block(Z, k, kx, r, 0, r, out->Cut);
  if (out->Chh) std::copy(h.Chh, h.Chh + (size_t)r * r, out->Chh);
  if (out->K) std::copy(h.K, h.K + (size_t)k * k, out->K);
  out->Cee = h.Cee;
  out->Cff = h.Cff;
  if (with_M && (out->Cxt || out->Cxto || out->Cyu || out->Cyuo)) {
    const int P = a.ldx + a.ldy;
    std::vector<double> M((size_t)P * k);
    HIPCHK(c, hipMemcpy(M.data(), a.M, sizeof(double) * M.size(), hipMemcpyDeviceToHost));
    auto cdz = [&](int row0, int rows, int col0, int cols, double* o) {
      if (!o) return;
      for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) {
          double acc = 0.0;
          for (int m = 0; m < k; ++m) acc += M[(size_t)m * P + row0 + i] * h.K[(size_t)(col0 + j) * k + m];
          o[(size_t)j * rows + i] = acc / a.N;
        }
    };
    cdz(0, a.p, 0, r, out->Cxt);
    cdz(0, a.p, r, s.rx, out->Cxto);
    cdz(a.ldx, a.q, kx, r, out->Cyu);
    cdz(a.ldx, a.q, kx + r, s.ry, out->Cyuo);
  }
  return PPLS_OK;
}

// What every fitting entry needs: data, no open stream, a usable S (formed and kept on resident rows).
int po2_ready(ppls_ctx* c) {
  int rc;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (c->st_state == 1) return fail(c, PPLS_E_STATE, "a stream is open: call ppls_stream_end first");
  if ((rc = check_fit_data(c))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return o2m_ready(c);
}

// Theta on the host in the ABI's layout (owned buffers), read back from the device's padded columns.
struct Po2Host {
  std::vector<double> W, Wo, C, Co, B, T, To, Uo;
  PplsPo2Scalars hs{};
  ppls_po2_theta view() {
    return {W.data(), Wo.data(), C.data(), Co.data(), B.data(), T.data(), To.data(), Uo.data(), hs.sE, hs.sF, hs.sH};
  }
};

// The device's theta of d into h; PPLS_E_NUMERIC if any of it is not finite (`after`: for the message).
int po2_pull(ppls_ctx* c, const PplsPo2Args& a, const Po2Shape& s, Po2Host& h, const char* after) {
  const int p = c->p, q = c->q, ldx = c->ldx, ldy = c->ldy;
  std::vector<double> gx((size_t)ldx * s.kx), gy((size_t)ldy * s.ky);
  PplsPo2Scalars& hs = h.hs;
  HIPCHK(c, hipMemcpy(gx.data(), a.Gx, sizeof(double) * gx.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(gy.data(), a.Gy, sizeof(double) * gy.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(&hs, a.sc, sizeof hs, hipMemcpyDeviceToHost));
  bool fin = std::isfinite(hs.sE) && std::isfinite(hs.sF) && std::isfinite(hs.sH);
  for (double v : gx) fin = fin && std::isfinite(v);
  for (double v : gy) fin = fin && std::isfinite(v);
  for (int j = 0; j < PPLS_RMAX; ++j) fin = fin && std::isfinite(hs.b[j]) && std::isfinite(hs.sT[j]) && std::isfinite(hs.sTo[j]) && std::isfinite(hs.sUo[j]);
  if (!fin) return fail(c, PPLS_E_NUMERIC, "PO2PLS: non-finite estimates after %s", after);
  h.W.assign((size_t)p * s.r, 0.0); h.Wo.assign((size_t)p * std::max(s.rx, 1), 0.0);
  h.C.assign((size_t)q * s.r, 0.0); h.Co.assign((size_t)q * std::max(s.ry, 1), 0.0);
  h.B.assign(s.r, 0.0); h.T.assign(s.r, 0.0); h.To.assign(std::max(s.rx, 1), 0.0); h.Uo.assign(std::max(s.ry, 1), 0.0);
  for (int j = 0; j < s.r; ++j) {
    std::copy(gx.begin() + (size_t)j * ldx, gx.begin() + (size_t)j * ldx + p, h.W.begin() + (size_t)j * p);
    std::copy(gy.begin() + (size_t)j * ldy, gy.begin() + (size_t)j * ldy + q, h.C.begin() + (size_t)j * q);
    h.B[j] = hs.b[j];
    h.T[j] = hs.sT[j];
  }
  for (int j = 0; j < s.rx; ++j) {
    std::copy(gx.begin() + (size_t)(s.r + j) * ldx, gx.begin() + (size_t)(s.r + j) * ldx + p, h.Wo.begin() + (size_t)j * p);
    h.To[j] = hs.sTo[j];
  }
  for (int j = 0; j < s.ry; ++j) {
    std::copy(gy.begin() + (size_t)(s.r + j) * ldy, gy.begin() + (size_t)(s.r + j) * ldy + q, h.Co.begin() + (size_t)j * q);
    h.Uo[j] = hs.sUo[j];
  }
  return PPLS_OK;
}

// Theta h into the caller's buffers.
void po2_give(const Po2Host& h, const Po2Shape& s, int p, int q, ppls_po2_theta* th) {
  std::copy(h.W.begin(), h.W.end(), th->W);
  std::copy(h.C.begin(), h.C.end(), th->C);
  if (s.rx) std::copy(h.Wo.begin(), h.Wo.begin() + (size_t)p * s.rx, th->Wo);
  if (s.ry) std::copy(h.Co.begin(), h.Co.begin() + (size_t)q * s.ry, th->Co);
  for (int j = 0; j < s.r; ++j) { th->B[j] = h.B[j]; th->sigT[j] = h.T[j]; }
  for (int j = 0; j < s.rx; ++j) th->sigTo[j] = h.To[j];
  for (int j = 0; j < s.ry; ++j) th->sigUo[j] = h.Uo[j];
  th->sigE = h.hs.sE; th->sigF = h.hs.sF; th->sigH = h.hs.sH;
}

// One E-step at theta on scratch that is set up already (its stop flag detached): theta up, pass, Gram,
// small kernel (mode 0) into loglik[0], status.
int po2_estep_again(ppls_ctx* c, Po2Dev& d, const ppls_po2_theta* th, const Po2Shape& s) {
  int rc;
  d.a.stop = nullptr;
  d.a.stop_mirror = nullptr;
  if ((rc = po2_upload_side(c, th->W, s.r, th->Wo, s.rx, c->p, c->ldx, d.a.Gx))) return rc;
  if ((rc = po2_upload_side(c, th->C, s.r, th->Co, s.ry, c->q, c->ldy, d.a.Gy))) return rc;
  po2_pack_scalars(th, s, &d.hsc);
  HIPCHK(c, hipMemcpy(d.a.sc, &d.hsc, sizeof d.hsc, hipMemcpyHostToDevice));
  if ((rc = po2_pass(c, d, s))) return rc;
  HIPCHK(c, ppls_launch_po2_small(&d.a, 1, 0, 0, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return po2_status(c, d);
}

// One E-step at theta: pass, Gram, small kernel (mode 0), status.
int po2_estep_core(ppls_ctx* c, Po2Dev& d, const ppls_po2_theta* th, const Po2Shape& s) {
  int rc;
  if ((rc = po2_setup(c, d, th, s, 1, false))) return rc;
  if ((rc = po2_pass(c, d, s))) return rc;
  HIPCHK(c, ppls_launch_po2_small(&d.a, 1, 0, 0, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return po2_status(c, d);
}

// Canonical form: the joint part by PPLS_simult's rule (:794-799), the specific components by decreasing
// sigma (stable), each column's sign so that its sum is >= 0.
void po2_canonical(ppls_po2_theta* th, const Po2Shape& s, int p, int q) {
  ppls_theta joint = {th->W, th->C, th->B, th->sigT, th->sigE, th->sigF, th->sigH};
  canonicalize(&joint, p, q, s.r);
  auto spec = [](double* L, double* sig, int rows, int n) {
    if (n == 0) return;
    std::vector<int> ord(n);
    for (int j = 0; j < n; ++j) ord[j] = j;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return sig[x] > sig[y]; });
    std::vector<double> L2((size_t)rows * n), s2(n);
    for (int j = 0; j < n; ++j) {
      double sum = 0.0;
      for (int i = 0; i < rows; ++i) sum += L[(size_t)ord[j] * rows + i];
      const double sg = sum < 0.0 ? -1.0 : 1.0;
      for (int i = 0; i < rows; ++i) L2[(size_t)j * rows + i] = sg * L[(size_t)ord[j] * rows + i];
      s2[j] = sig[ord[j]];
    }
    std::copy(L2.begin(), L2.end(), L);
    std::copy(s2.begin(), s2.end(), sig);
  };
  spec(th->Wo, th->sigTo, p, s.rx);
  spec(th->Co, th->sigUo, q, s.ry);
}

// ---- the batched iteration: m models on one S.  All models' Gx columns lie side by side in one
// ldx x sum kx buffer (Gy alike) and the X and Y parts of their M in one P x sum kx and one P x sum ky buffer,
// so one pass is ceil(sum kx / 16) + ceil(sum ky / 16) panel launches whatever m is; a chunk may straddle two
// models (the panel's output does not depend, column by column, on the width it is launched at).  Everything
// else -- stop pair, status, scalars, moments, history, Q, G'G, the update's scratch -- is per model.
struct Po2Batch {
  CvScratch tmp;
  int m = 0, sumx = 0, sumy = 0, max_entries = 0, rw = 0, hist = 0, P = 0, ldx = 0, ldy = 0;
  std::vector<Po2Shape> sh;
  std::vector<int> offx, offy;   // first column of model j in the shared X and Y buffers
  std::vector<PplsPo2Args> ha;
  PplsPo2Args* da = nullptr;
  const double* S = nullptr;
  double *Gx = nullptr, *Gy = nullptr, *Mx = nullptr, *My = nullptr, *Q = nullptr, *GGx = nullptr, *GGy = nullptr;
  size_t qstride = 0, gstride = 0;
  int* ints = nullptr;      // per model {stop[0], stop[1], status, unused}
  int* mirror = nullptr;    // host-mapped: slot j = model j's stop pass
  ~Po2Batch() {
    if (mirror) (void)hipHostFree(mirror);
  }
};

// The buffers and the device array of arguments.  guard: doubles left between the outputs (the debug entry
// fills and checks them).  loop: also what the small and update kernels need (else the pass and Gram alone).
int po2_batch_alloc(ppls_ctx* c, Po2Batch& b, const double* S, int ldx, int ldy, int p, int q, const std::vector<Po2Shape>& sh,
                    int hist, size_t guard, bool loop, int type, double atol) {
  int rc;
  const int m = (int)sh.size(), P = ldx + ldy;
  b.m = m; b.sh = sh; b.hist = hist; b.P = P; b.ldx = ldx; b.ldy = ldy; b.S = S;
  b.offx.assign(m, 0); b.offy.assign(m, 0);
  for (int j = 0; j < m; ++j) {
    b.offx[j] = b.sumx; b.offy[j] = b.sumy;
    b.sumx += sh[j].kx; b.sumy += sh[j].ky;
    b.max_entries = std::max(b.max_entries, sh[j].k * (sh[j].k + 1) / 2 + sh[j].kx * (sh[j].kx + 1) / 2 + sh[j].ky * (sh[j].ky + 1) / 2);
  }
  b.qstride = (size_t)PPLS_PO2_KMAX * PPLS_PO2_KMAX + guard;
  b.gstride = (size_t)PPLS_RMAX * PPLS_RMAX + guard;
  PplsPo2Scalars* sc = nullptr;
  PplsPo2Small* sm = nullptr;
  double *Z = nullptr, *ll = nullptr, *Mall = nullptr;
  if ((rc = b.tmp.get(c, &b.Gx, (size_t)ldx * b.sumx)) || (rc = b.tmp.get(c, &b.Gy, (size_t)ldy * b.sumy)) ||
      (rc = b.tmp.get(c, &Mall, (size_t)P * (b.sumx + b.sumy) + 3 * guard)) || (rc = b.tmp.get(c, &b.Q, b.qstride * m)) ||
      (rc = b.tmp.get(c, &b.GGx, b.gstride * m)) || (rc = b.tmp.get(c, &b.GGy, b.gstride * m)) || (rc = b.tmp.get(c, &b.da, (size_t)m)))
    return rc;
  b.Mx = Mall + guard;
  b.My = b.Mx + (size_t)P * b.sumx + guard;
  if (loop) {
    if ((rc = b.tmp.get(c, &sc, (size_t)m)) || (rc = b.tmp.get(c, &sm, (size_t)m)) || (rc = b.tmp.get(c, &Z, (size_t)m * PPLS_RMAX * P)) ||
        (rc = b.tmp.get(c, &ll, (size_t)m * hist)) || (rc = b.tmp.get(c, &b.ints, (size_t)4 * m)))
      return rc;
    HIPCHK(c, hipMemset(b.ints, 0, sizeof(int) * 4 * m));
    HIPCHK(c, hipHostMalloc((void**)&b.mirror, sizeof(int) * m, hipHostMallocMapped | hipHostMallocCoherent));
    for (int j = 0; j < m; ++j) __atomic_store_n(b.mirror + j, 0, __ATOMIC_SEQ_CST);
  }
  int* mirror_dev = nullptr;
  if (b.mirror) HIPCHK(c, hipHostGetDevicePointer((void**)&mirror_dev, b.mirror, 0));
  b.ha.assign(m, PplsPo2Args{});
  for (int j = 0; j < m; ++j) {
    PplsPo2Args& a = b.ha[j];
    a.S = S; a.ldx = ldx; a.ldy = ldy; a.p = p; a.q = q; a.r = sh[j].r; a.rx = sh[j].rx; a.ry = sh[j].ry; a.type = type;
    a.Gx = b.Gx + (size_t)b.offx[j] * ldx;
    a.Gy = b.Gy + (size_t)b.offy[j] * ldy;
    a.M = b.Mx + (size_t)b.offx[j] * P;
    a.My = b.My + (size_t)b.offy[j] * P;
    a.Q = b.Q + b.qstride * j;
    a.GGx = b.GGx + b.gstride * j;
    a.GGy = b.GGy + b.gstride * j;
    if (loop) {
      a.sc = sc + j; a.sm = sm + j; a.Z = Z + (size_t)j * PPLS_RMAX * P; a.loglik = ll + (size_t)j * hist;
      a.stop = b.ints + 4 * j; a.status = b.ints + 4 * j + 2; a.stop_mirror = mirror_dev + j;
      a.N = (double)c->n_total; a.ssqX = c->ssq_host[0]; a.ssqY = c->ssq_host[1]; a.atol = atol;
    }
  }
  HIPCHK(c, hipMemcpy(b.da, b.ha.data(), sizeof(PplsPo2Args) * m, hipMemcpyHostToDevice));
  // rows of S per wave: the tile kernel's rule at the full chunk width (the sums of a row do not depend on it)
  b.rw = ppls_xprod_tile_rows(P, PPLS_RMAX, c->xprod_rw, c->num_cus);
  return PPLS_OK;
}

// One batched pass: the shared panels in chunks of up to 16 columns, then the Gram of every model.
int po2_batch_pass(ppls_ctx* c, const Po2Batch& b) {
  for (int c0 = 0; c0 < b.sumx; c0 += PPLS_RMAX)
    HIPCHK(c, ppls_launch_po2_panel(b.S, b.P, 0, b.ldx, b.Gx + (size_t)c0 * b.ldx, b.ldx, std::min(PPLS_RMAX, b.sumx - c0), b.rw,
                                    b.Mx + (size_t)c0 * b.P, nullptr, c->stream));
  for (int c0 = 0; c0 < b.sumy; c0 += PPLS_RMAX)
    HIPCHK(c, ppls_launch_po2_panel(b.S, b.P, b.ldx, b.ldy, b.Gy + (size_t)c0 * b.ldy, b.ldy, std::min(PPLS_RMAX, b.sumy - c0), b.rw,
                                    b.My + (size_t)c0 * b.P, nullptr, c->stream));
  HIPCHK(c, ppls_launch_po2_gram_batch(b.da, b.m, b.max_entries, c->stream));
  return PPLS_OK;
}

// Theta up: the loadings into the shared padded columns, the scalars per model.
int po2_batch_upload(ppls_ctx* c, Po2Batch& b, const ppls_po2_theta* th, int p, int q) {
  const int ldx = b.ldx, ldy = b.ldy, m = b.m;
  const std::vector<Po2Shape>& sh = b.sh;
  std::vector<double> hx((size_t)ldx * b.sumx, 0.0), hy((size_t)ldy * b.sumy, 0.0);
  std::vector<PplsPo2Scalars> hs((size_t)m);
  for (int j = 0; j < m; ++j) {
    const ppls_po2_theta& t = th[j];
    for (int k = 0; k < sh[j].kx; ++k) {
      const double* src = k < sh[j].r ? t.W + (size_t)k * p : t.Wo + (size_t)(k - sh[j].r) * p;
      std::copy(src, src + p, hx.begin() + (size_t)(b.offx[j] + k) * ldx);
    }
    for (int k = 0; k < sh[j].ky; ++k) {
      const double* src = k < sh[j].r ? t.C + (size_t)k * q : t.Co + (size_t)(k - sh[j].r) * q;
      std::copy(src, src + q, hy.begin() + (size_t)(b.offy[j] + k) * ldy);
    }
    po2_pack_scalars(&t, sh[j], &hs[j]);
  }
  HIPCHK(c, hipMemcpy(b.Gx, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(b.Gy, hy.data(), sizeof(double) * hy.size(), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(b.ha[0].sc, hs.data(), sizeof(PplsPo2Scalars) * m, hipMemcpyHostToDevice));
  return PPLS_OK;
}

const char* po2_status_text(int st) {
  switch (st) {
    case PPLS_PO2_ST_SIGMA: return "a sigma is not finite and above 0";
    case PPLS_PO2_ST_LAMBDA: return "Lambda = Sigma_z^-1 + D G'G is not positive definite";
    case PPLS_PO2_ST_VAR: return "an updated variance is not finite and above 0";
    default: return "rank-deficient loading update";
  }
}

// Lower Cholesky factor of the n x n matrix A (column-major, in place); false: not positive definite.
bool po2_host_chol(std::vector<double>& A, int n) {
  for (int j = 0; j < n; ++j) {
    double d = A[(size_t)j * n + j];
    for (int m = 0; m < j; ++m) d -= A[(size_t)m * n + j] * A[(size_t)m * n + j];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    d = std::sqrt(d);
    A[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double s = A[(size_t)j * n + i];
      for (int m = 0; m < j; ++m) s -= A[(size_t)m * n + i] * A[(size_t)m * n + j];
      A[(size_t)j * n + i] = s / d;
    }
  }
  return true;
}

// Owned buffers of one theta in the ABI's layout, sized for shape s.
void po2_host_sized(Po2Host& h, const Po2Shape& s, int p, int q) {
  h.W.assign((size_t)p * s.r, 0.0); h.Wo.assign((size_t)p * std::max(s.rx, 1), 0.0);
  h.C.assign((size_t)q * s.r, 0.0); h.Co.assign((size_t)q * std::max(s.ry, 1), 0.0);
  h.B.assign(s.r, 0.0); h.T.assign(s.r, 0.0); h.To.assign(std::max(s.rx, 1), 0.0); h.Uo.assign(std::max(s.ry, 1), 0.0);
}

}  // namespace

extern "C" {

int ppls_po2_estep(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, ppls_po2_expect* out) {
  if (!c) return PPLS_E_ARG;
  if (!out) return fail(c, PPLS_E_ARG, "NULL argument");
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(c, r, rx, ry, c->p, c->q, &s)) || (rc = po2_check_theta(c, th, s, c->p, c->q))) return rc;
  if ((rc = po2_ready(c))) return rc;
  Po2Dev d;
  if ((rc = po2_estep_core(c, d, th, s))) return rc;
  return po2_expect_out(c, d.a, s, true, out);
}

int ppls_po2_loglik(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, double* out) {
  if (!c) return PPLS_E_ARG;
  if (!out) return fail(c, PPLS_E_ARG, "NULL argument");
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(c, r, rx, ry, c->p, c->q, &s)) || (rc = po2_check_theta(c, th, s, c->p, c->q))) return rc;
  if ((rc = po2_ready(c))) return rc;
  Po2Dev d;
  if ((rc = po2_estep_core(c, d, th, s))) return rc;
  HIPCHK(c, hipMemcpy(out, d.a.loglik, sizeof(double), hipMemcpyDeviceToHost));
  return PPLS_OK;
}

int ppls_po2_em_run(ppls_ctx* c, ppls_po2_theta* th, int r, int rx, int ry, int max_steps, double atol, int type,
                    double* loglik, int cap, int* n_loglik, int* negative_increment, ppls_po2_expect* eout) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(c, r, rx, ry, c->p, c->q, &s)) || (rc = po2_check_theta(c, th, s, c->p, c->q))) return rc;
  if (max_steps < 1) return fail(c, PPLS_E_ARG, "EMsteps must be >= 1");
  if (type != PPLS_ORTH_SVD && type != PPLS_ORTH_QR) return fail(c, PPLS_E_ARG, "type must be SVD (0) or QR (1)");
  if (cap < 0 || (cap > 0 && !loglik) || std::isnan(atol)) return fail(c, PPLS_E_ARG, "bad loglik buffer or atol");
  if ((rc = po2_ready(c))) return rc;
  const int p = c->p, q = c->q;
  Po2Dev d;
  if ((rc = po2_setup(c, d, th, s, max_steps + 2, false))) return rc;
  const bool do_check = !(atol == -INFINITY);
  if ((rc = ensure_stop(c)) || (rc = reset_stop(c))) return rc;
  d.a.stop = c->stop_d;
  d.a.stop_mirror = c->stop_mirror_dev;
  d.a.atol = atol;
  d.a.type = type;
  struct EvGuard {
    std::vector<hipEvent_t> evs;
    ~EvGuard() {
      for (auto e : evs) (void)hipEventDestroy(e);
    }
  } guard;
  constexpr int LOOKAHEAD = 8;   // as ppls_em_run: the host stays at most this many passes ahead of the flag
  for (int i = 1; i <= max_steps + 1; ++i) {
    if (i > LOOKAHEAD) {
      HIPCHK(c, hipEventSynchronize(guard.evs[(size_t)(i - 1 - LOOKAHEAD) % LOOKAHEAD]));
      if (__atomic_load_n(c->stop_mirror, __ATOMIC_ACQUIRE) != 0) break;
    }
    const bool last = i == max_steps + 1;
    if ((rc = po2_pass(c, d, s))) return rc;
    HIPCHK(c, ppls_launch_po2_small(&d.a, i, last ? 0 : 1, do_check ? 1 : 0, c->stream));
    if (!last) HIPCHK(c, ppls_launch_po2_update(&d.a, c->stream));
    const size_t e = (size_t)(i - 1) % LOOKAHEAD;
    if (guard.evs.size() <= e) {
      hipEvent_t ev;
      HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      guard.evs.push_back(ev);
    }
    HIPCHK(c, hipEventRecord(guard.evs[e], c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = po2_status(c, d))) return rc;
  int stopv[2] = {0, 0};
  HIPCHK(c, hipMemcpy(stopv, c->stop_d, sizeof stopv, hipMemcpyDeviceToHost));
  const int npass = stopv[0] > 0 ? stopv[0] : max_steps + 1;   // passes run = entries of the history
  if (stopv[1])
    return fail(c, PPLS_E_NUMERIC, "PO2PLS: the log-likelihood increment of EM iteration %d is NaN", npass - 1);
  std::vector<double> l((size_t)npass);
  HIPCHK(c, hipMemcpy(l.data(), d.a.loglik, sizeof(double) * npass, hipMemcpyDeviceToHost));
  for (int i = 0; i < npass; ++i)
    if (!std::isfinite(l[i])) return fail(c, PPLS_E_NUMERIC, "PO2PLS: non-finite log-likelihood %g at pass %d", l[i], i + 1);
  // the estimates, in canonical form.  The moments of the last pass belong to them as the device holds them;
  // the canonical form permutes and flips latent coordinates, so Expectations come from one more E-step at
  // the canonical estimates, on the same scratch
  Po2Host h;
  char after[48];
  snprintf(after, sizeof after, "%d EM iterations", npass - 1);
  if ((rc = po2_pull(c, d.a, s, h, after))) return rc;
  ppls_po2_theta est = h.view();
  po2_canonical(&est, s, p, q);
  h.hs.sE = est.sigE; h.hs.sF = est.sigF; h.hs.sH = est.sigH;
  if (eout) {
    if ((rc = po2_estep_again(c, d, &est, s))) return rc;
    if ((rc = po2_expect_out(c, d.a, s, true, eout))) return rc;
  }
  po2_give(h, s, p, q, th);
  for (int i = 0; i < npass && i < cap; ++i) loglik[i] = l[i];
  if (n_loglik) *n_loglik = npass;
  if (negative_increment) {
    int neg = 0;
    for (int i = 1; i < npass; ++i) neg |= (l[i] - l[i - 1] < 0);
    *negative_increment = neg;
  }
  return PPLS_OK;
}

int ppls_po2_start(ppls_ctx* c, int r, int rx, int ry, const double* V0x, const double* V0y, int steps, ppls_po2_theta* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(c, r, rx, ry, c->p, c->q, &s))) return rc;
  if (!out || !out->W || !out->C || !out->B || !out->sigT || (rx && (!out->Wo || !out->sigTo || !V0x)) ||
      (ry && (!out->Co || !out->sigUo || !V0y)))
    return fail(c, PPLS_E_ARG, "NULL argument");
  if (steps < 0) return fail(c, PPLS_E_ARG, "steps must be >= 0");
  const int p = c->p, q = c->q;
  for (size_t e = 0; e < (size_t)p * rx; ++e)
    if (!std::isfinite(V0x[e])) return fail(c, PPLS_E_ARG, "V0x has non-finite entries");
  for (size_t e = 0; e < (size_t)q * ry; ++e)
    if (!std::isfinite(V0y[e])) return fail(c, PPLS_E_ARG, "V0y has non-finite entries");
  if ((rc = po2_ready(c))) return rc;
  // the joint part: the 'o2m_xprod' sequential fit, one EM step per component (more steps of the
  // shared-only model pull a joint loading towards the strongest X-only direction)
  // The sequential fit keeps its state in its context (ensure_r: the loadings of an ppls_em_begin session, the
  // 'o2m_xprod' record), so it runs on a context of this call that holds a copy of S and nothing else: c's
  // session, options and records stay as they are.
  std::vector<double> W((size_t)p * r), C((size_t)q * r), B(r), sig((size_t)r * 4);
  ppls_seq_fit f = {W.data(), C.data(), B.data(), sig.data(), nullptr, nullptr, nullptr, nullptr, 0, 0};
  {
    struct Tmp {
      ppls_ctx* t = nullptr;
      ~Tmp() { ppls_ctx_destroy(t); }
    } tmp;
    const int Pj = c->ldx + c->ldy;
    if ((rc = ppls_ctx_create(c->device, &tmp.t))) return fail(c, rc, "PO2PLS start: no scratch context");
    ppls_ctx* t = tmp.t;
    DevGuard Snew;
    if ((rc = dalloc(t, &Snew.p, (size_t)Pj * Pj))) return fail(c, rc, "PO2PLS start: %s", t->err.c_str());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = derived_begin(t, "PO2PLS start", "the source's", c->dtype, c->ldpad, p, q, c->ldx, c->ldy, Snew, false);
    if (!rc) {
      hipError_t e = hipMemcpy(t->xp_S, c->xp_S, sizeof(double) * Pj * Pj, hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = hipMemcpy(t->ssq, c->ssq_host, sizeof c->ssq_host, hipMemcpyHostToDevice);
      if (e != hipSuccess) rc = fail(t, PPLS_E_HIP, "copy of S: %s", hipGetErrorString(e));
    }
    if (rc) return fail(c, rc, "PO2PLS start: %s", t->err.c_str());
    t->ssq_host[0] = c->ssq_host[0];
    t->ssq_host[1] = c->ssq_host[1];
    t->o2m_path = c->o2m_path;
    t->xprod_rw = c->xprod_rw;
    derived_publish(t, c->n_total, c->mem_free_min);
    if ((rc = ppls_ppls_o2m(t, r, 1, 1e-4, 0, nullptr, &f))) return fail(c, rc, "PO2PLS start, joint fit: %s", t->err.c_str());
  }
  if (f.ncomp < r) return fail(c, PPLS_E_NUMERIC, "PO2PLS start: the joint fit stopped after %d of %d components", f.ncomp, r);
  // the specific parts: orthogonal iteration on (I - P_W) S_xx (I - P_W) and (I - P_C) S_yy (I - P_C), both
  // sides in one pass over S per step (the panel kernel); the p x rx projection and QR run on the host
  const int ldx = c->ldx, ldy = c->ldy, P = ldx + ldy, wx = std::max(rx, 1), wy = std::max(ry, 1);
  struct Side {
    int n, w, ld;
    std::vector<double> Qb, V, A, sg;
  } sd[2] = {{p, rx, ldx, {}, {}, {}, {}}, {q, ry, ldy, {}, {}, {}, {}}};
  auto project_orth = [&](Side& t, const double* src) -> int {   // V <- orth((I - Qb Qb') src)
    if (t.w == 0) return PPLS_OK;
    const int jr = r;
    std::vector<double> Z(src, src + (size_t)t.n * t.w);
    for (int j = 0; j < t.w; ++j)
      for (int m = 0; m < jr; ++m) {
        const double d = hdot(&t.Qb[(size_t)m * t.n], &Z[(size_t)j * t.n], t.n);
        for (int i = 0; i < t.n; ++i) Z[(size_t)j * t.n + i] -= d * t.Qb[(size_t)m * t.n + i];
      }
    t.V.resize(Z.size());
    if (host_orth(Z.data(), t.n, t.w, PPLS_ORTH_QR, t.V.data()) != PPLS_OK)
      return fail(c, PPLS_E_NUMERIC, "PO2PLS start: rank-deficient specific block");
    return PPLS_OK;
  };
  for (int m = 0; m < 2; ++m) {
    Side& t = sd[m];
    t.Qb.resize((size_t)t.n * r);
    if (host_orth(m ? C.data() : W.data(), t.n, r, PPLS_ORTH_QR, t.Qb.data()) != PPLS_OK)
      return fail(c, PPLS_E_NUMERIC, "PO2PLS start: rank-deficient joint loadings");
    if ((rc = project_orth(t, m ? V0y : V0x))) return rc;
    t.sg.assign(t.w, 0.0);
  }
  CvScratch tmp;
  PplsPo2Args a{};
  if ((rc = tmp.get(c, &a.Gx, (size_t)ldx * wx)) || (rc = tmp.get(c, &a.Gy, (size_t)ldy * wy)) ||
      (rc = tmp.get(c, &a.M, (size_t)P * (wx + wy))))
    return rc;
  a.S = c->xp_S; a.ldx = ldx; a.ldy = ldy;
  const int rw = ppls_xprod_tile_rows(P, std::max(wx, wy), c->xprod_rw, c->num_cus);
  std::vector<double> hx((size_t)ldx * wx, 0.0), hy((size_t)ldy * wy, 0.0), hM((size_t)P * (wx + wy));
  for (int it = 0; it <= steps && (rx || ry); ++it) {   // the last pass gives V'S V alone; a side without columns is not launched
    for (int j = 0; j < rx; ++j) std::copy(&sd[0].V[(size_t)j * p], &sd[0].V[(size_t)j * p] + p, &hx[(size_t)j * ldx]);
    for (int j = 0; j < ry; ++j) std::copy(&sd[1].V[(size_t)j * q], &sd[1].V[(size_t)j * q] + q, &hy[(size_t)j * ldy]);
    HIPCHK(c, hipMemcpyAsync(a.Gx, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(a.Gy, hy.data(), sizeof(double) * hy.size(), hipMemcpyHostToDevice, c->stream));
    if (rx) HIPCHK(c, ppls_launch_po2_panel(a.S, P, 0, ldx, a.Gx, ldx, wx, rw, a.M, nullptr, c->stream));
    if (ry) HIPCHK(c, ppls_launch_po2_panel(a.S, P, ldx, ldy, a.Gy, ldy, wy, rw, a.M + (size_t)wx * P, nullptr, c->stream));
    HIPCHK(c, hipMemcpyAsync(hM.data(), a.M, sizeof(double) * hM.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int m = 0; m < 2; ++m) {
      Side& t = sd[m];
      if (t.w == 0) continue;
      t.A.resize((size_t)t.n * t.w);
      for (int j = 0; j < t.w; ++j)   // S_xx V: the X rows of the X panel; S_yy V: the Y rows of the Y panel
        std::copy(&hM[(size_t)((m ? wx : 0) + j) * P + (m ? ldx : 0)], &hM[(size_t)((m ? wx : 0) + j) * P + (m ? ldx : 0)] + t.n,
                  &t.A[(size_t)j * t.n]);
      if (it == steps) {
        for (int j = 0; j < t.w; ++j) {
          const double v = hdot(&t.V[(size_t)j * t.n], &t.A[(size_t)j * t.n], t.n) / (double)c->n_total;
          if (!(v > 0.0) || !std::isfinite(v)) return fail(c, PPLS_E_NUMERIC, "PO2PLS start: a specific variance is not above 0");
          t.sg[j] = std::sqrt(v);
        }
      } else if ((rc = project_orth(t, t.A.data()))) {
        return rc;
      }
    }
  }
  std::copy(W.begin(), W.end(), out->W);
  std::copy(C.begin(), C.end(), out->C);
  for (int k = 0; k < r; ++k) {
    out->B[k] = B[k];
    out->sigT[k] = sig[(size_t)3 * r + k];
  }
  out->sigE = sig[(size_t)0 * r + r - 1];
  out->sigF = sig[(size_t)1 * r + r - 1];
  out->sigH = sig[(size_t)2 * r + r - 1];
  if (rx) {
    std::copy(sd[0].V.begin(), sd[0].V.end(), out->Wo);
    std::copy(sd[0].sg.begin(), sd[0].sg.end(), out->sigTo);
  }
  if (ry) {
    std::copy(sd[1].V.begin(), sd[1].V.end(), out->Co);
    std::copy(sd[1].sg.begin(), sd[1].sg.end(), out->sigUo);
  }
  return PPLS_OK;
}

int ppls_po2_em_step(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, int type, ppls_po2_theta* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(c, r, rx, ry, c->p, c->q, &s)) || (rc = po2_check_theta(c, th, s, c->p, c->q))) return rc;
  if (type != PPLS_ORTH_SVD && type != PPLS_ORTH_QR) return fail(c, PPLS_E_ARG, "type must be SVD (0) or QR (1)");
  if (!out || !out->W || !out->C || !out->B || !out->sigT || (rx && (!out->Wo || !out->sigTo)) || (ry && (!out->Co || !out->sigUo)))
    return fail(c, PPLS_E_ARG, "NULL argument");
  if ((rc = po2_ready(c))) return rc;
  Po2Dev d;
  if ((rc = po2_setup(c, d, th, s, 1, false))) return rc;
  d.a.type = type;
  if ((rc = po2_pass(c, d, s))) return rc;
  HIPCHK(c, ppls_launch_po2_small(&d.a, 1, 1, 0, c->stream));
  HIPCHK(c, ppls_launch_po2_update(&d.a, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = po2_status(c, d))) return rc;
  Po2Host h;
  if ((rc = po2_pull(c, d.a, s, h, "one ECM step"))) return rc;
  po2_give(h, s, c->p, c->q, out);
  return PPLS_OK;
}

int ppls_po2_stats(ppls_ctx* c, const double* S, int P, int ldx, const double* Gx, int kx, const double* Gy, int ky,
                   int rw, double* M, double* Q, double* GG) {
  if (!c) return PPLS_E_ARG;
  if (!Gx || !Gy || !M || !Q || !GG) return fail(c, PPLS_E_ARG, "NULL argument");
  if (kx < 1 || ky < 1 || kx > PPLS_RMAX || ky > PPLS_RMAX) return fail(c, PPLS_E_ARG, "widths kx=%d ky=%d outside [1,%d]", kx, ky, PPLS_RMAX);
  const int ldy = P - ldx, k = kx + ky;
  if (ldx < 2 || ldy < 2 || (ldx & 1) || (ldy & 1) || P >= (1 << 30)) return fail(c, PPLS_E_ARG, "bad layout P=%d ldx=%d", P, ldx);
  const int wmax = std::max(kx, ky);
  if (!(rw == 0 || rw == 1 || rw == 2 || rw == 4 || (rw == 8 && wmax <= 8))) return fail(c, PPLS_E_ARG, "rw=%d", rw);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const double* Sd = nullptr;
  CvScratch tmp;
  if (S) {
    double* up = nullptr;
    if ((rc = tmp.get(c, &up, (size_t)P * P))) return rc;
    HIPCHK(c, hipMemcpy(up, S, sizeof(double) * P * P, hipMemcpyHostToDevice));
    Sd = up;
  } else {
    if (!c->have_data || !c->xp_ready || !c->xp_S) return fail(c, PPLS_E_STATE, "no cross-products S are ready");
    if (P != c->ldx + c->ldy || ldx != c->ldx) return fail(c, PPLS_E_ARG, "P=%d ldx=%d are not the context's %d, %d", P, ldx, c->ldx + c->ldy, c->ldx);
    Sd = c->xp_S;
  }
  const size_t guard = 64, nM = (size_t)P * k, nQ = (size_t)k * k, nGx = (size_t)kx * kx, nGy = (size_t)ky * ky;
  double *gxd = nullptr, *gyd = nullptr, *out = nullptr;
  const size_t nout = nM + nQ + nGx + nGy + 5 * guard;
  if ((rc = tmp.get(c, &gxd, (size_t)ldx * kx)) || (rc = tmp.get(c, &gyd, (size_t)ldy * ky)) || (rc = tmp.get(c, &out, nout))) return rc;
  HIPCHK(c, hipMemcpy(gxd, Gx, sizeof(double) * ldx * kx, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(gyd, Gy, sizeof(double) * ldy * ky, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemsetAsync(out, 0xFF, sizeof(double) * nout, c->stream));
  PplsPo2Args a{};
  a.S = Sd; a.ldx = ldx; a.ldy = ldy; a.p = ldx; a.q = ldy; a.r = 1; a.rx = kx - 1; a.ry = ky - 1;
  a.Gx = gxd; a.Gy = gyd;
  a.M = out + guard;
  a.My = a.M + (size_t)kx * P;
  a.Q = a.M + nM + guard;
  a.GGx = a.Q + nQ + guard;
  a.GGy = a.GGx + nGx + guard;
  if (rw == 0) rw = ppls_xprod_tile_rows(P, wmax, c->xprod_rw, c->num_cus);
  if (rw == 8 && wmax > 8) rw = 4;
  if ((rc = po2_panels(c, a, kx, ky, rw))) return rc;
  HIPCHK(c, ppls_launch_po2_gram(&a, c->stream));
  std::vector<double> h(nout);
  HIPCHK(c, hipMemcpyAsync(h.data(), out, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t offs[5] = {0, guard + nM, 2 * guard + nM + nQ, 3 * guard + nM + nQ + nGx, 4 * guard + nM + nQ + nGx + nGy};
  for (size_t o : offs)
    for (size_t g = 0; g < guard; ++g)
      if (!std::isnan(h[o + g])) return fail(c, PPLS_E_NUMERIC, "a PO2 statistics kernel wrote outside its output");
  std::copy(h.begin() + guard, h.begin() + guard + nM, M);
  std::copy(h.begin() + offs[1] + guard, h.begin() + offs[1] + guard + nQ, Q);
  std::copy(h.begin() + offs[2] + guard, h.begin() + offs[2] + guard + nGx, GG);
  std::copy(h.begin() + offs[3] + guard, h.begin() + offs[3] + guard + nGy, GG + nGx);
  return PPLS_OK;
}

// The PPLS_simult statistics pass alone (ppls_xprod.hip), the twin of ppls_po2_stats for the tile and Gram
// kernels of xprod_stats(): the launch goes through ppls_launch_xprod_tile.
int ppls_xprod_pass(ppls_ctx* c, const double* S, int P, int ldx, const double* W, const double* C, const double* alpha,
                    const double* beta, const double* gamma, const double* delta, int r, int rw, int with_gram, int stop,
                    double* M, double* stats, int* rw_used, int* nt_used) {
  if (!c) return PPLS_E_ARG;
  if (!W || !C || !alpha || !beta || !gamma || !delta || !M || !stats) return fail(c, PPLS_E_ARG, "NULL argument");
  if (r < 1 || r > PPLS_RMAX) return fail(c, PPLS_E_ARG, "r=%d outside [1,%d]", r, PPLS_RMAX);
  const int ldy = P - ldx;
  if (ldx < 2 || ldy < 2 || (ldx & 1) || (ldy & 1) || P >= (1 << 30)) return fail(c, PPLS_E_ARG, "bad layout P=%d ldx=%d", P, ldx);
  if (!(rw == 0 || rw == 1 || rw == 2 || rw == 4 || (rw == 8 && r <= 8))) return fail(c, PPLS_E_ARG, "rw=%d at r=%d", rw, r);
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const double* Sd = nullptr;
  CvScratch tmp;
  if (S) {
    double* up = nullptr;
    if ((rc = tmp.get(c, &up, (size_t)P * P))) return rc;
    HIPCHK(c, hipMemcpy(up, S, sizeof(double) * P * P, hipMemcpyHostToDevice));
    Sd = up;
  } else {
    if (!c->have_data || !c->xp_ready || !c->xp_S) return fail(c, PPLS_E_STATE, "no cross-products S are ready");
    if (P != c->ldx + c->ldy || ldx != c->ldx) return fail(c, PPLS_E_ARG, "P=%d ldx=%d are not the context's %d, %d", P, ldx, c->ldx + c->ldy, c->ldx);
    Sd = c->xp_S;
  }
  const size_t guard = 64, nM = (size_t)P * 2 * r, nst = (size_t)P * r + (size_t)4 * r * r, nout = nM + nst + 3 * guard;
  double *wd = nullptr, *cd = nullptr, *out = nullptr;
  PplsScalars* scd = nullptr;
  int* stopd = nullptr;
  if ((rc = tmp.get(c, &wd, (size_t)ldx * r)) || (rc = tmp.get(c, &cd, (size_t)ldy * r)) || (rc = tmp.get(c, &out, nout)) ||
      (rc = tmp.get(c, &scd, 1)) || (rc = tmp.get(c, &stopd, 2)))
    return rc;
  PplsScalars s;
  memset(&s, 0, sizeof s);
  for (int k = 0; k < r; ++k) {
    s.alpha[k] = alpha[k];
    s.beta[k] = beta[k];
    s.gamma[k] = gamma[k];
    s.delta[k] = delta[k];
  }
  const int hstop[2] = {stop ? 1 : 0, 0};
  HIPCHK(c, hipMemcpy(wd, W, sizeof(double) * ldx * r, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(cd, C, sizeof(double) * ldy * r, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(scd, &s, sizeof s, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(stopd, hstop, sizeof hstop, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemsetAsync(out, 0xFF, sizeof(double) * nout, c->stream));
  if (rw == 0) rw = ppls_xprod_tile_rows(P, r, c->xprod_rw, c->num_cus);
  if (rw_used) *rw_used = rw;
  if (nt_used) *nt_used = ppls_xprod_tile_nt(P);
  double* Md = out + guard;
  double* std_ = Md + nM + guard;
  HIPCHK(c, ppls_launch_xprod_tile(Sd, ldx, ldy, r, rw, wd, cd, scd, std_, Md, stopd, with_gram ? 1 : 0, c->stream));
  std::vector<double> h(nout);
  HIPCHK(c, hipMemcpyAsync(h.data(), out, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t offs[3] = {0, guard + nM, 2 * guard + nM + nst};
  for (size_t o : offs)
    for (size_t g = 0; g < guard; ++g)
      if (!std::isnan(h[o + g])) return fail(c, PPLS_E_NUMERIC, "a cross-product statistics kernel wrote outside its output");
  std::copy(h.begin() + guard, h.begin() + guard + nM, M);
  std::copy(h.begin() + offs[1] + guard, h.begin() + offs[1] + guard + nst, stats);
  return PPLS_OK;
}

int ppls_po2_small(ppls_ctx* c, const double* Q, const double* GG, const ppls_po2_theta* th, int r, int rx, int ry, int p,
                   int q, double N, double ssqX, double ssqY, ppls_po2_expect* out, double* loglik, int* status) {
  if (!c) return PPLS_E_ARG;
  if (!Q || !GG) return fail(c, PPLS_E_ARG, "NULL argument");
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(c, r, rx, ry, p, q, &s))) return rc;
  if (!th || !th->B || !th->sigT || (rx && !th->sigTo) || (ry && !th->sigUo)) return fail(c, PPLS_E_ARG, "NULL argument");
  if (!(N > 0.0)) return fail(c, PPLS_E_ARG, "N must be above 0");
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  PplsPo2Args a{};
  int* ints = nullptr;
  const size_t nQ = (size_t)s.k * s.k, nGx = (size_t)s.kx * s.kx, nGy = (size_t)s.ky * s.ky;
  if ((rc = tmp.get(c, &a.Q, nQ)) || (rc = tmp.get(c, &a.GGx, nGx)) || (rc = tmp.get(c, &a.GGy, nGy)) || (rc = tmp.get(c, &a.sc, 1)) ||
      (rc = tmp.get(c, &a.sm, 1)) || (rc = tmp.get(c, &a.loglik, 1)) || (rc = tmp.get(c, &ints, 4)))
    return rc;
  PplsPo2Scalars hs;
  po2_pack_scalars(th, s, &hs);
  HIPCHK(c, hipMemcpy(a.Q, Q, sizeof(double) * nQ, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(a.GGx, GG, sizeof(double) * nGx, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(a.GGy, GG + nGx, sizeof(double) * nGy, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(a.sc, &hs, sizeof hs, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemset(ints, 0, 4 * sizeof(int)));
  a.status = ints;
  a.p = p; a.q = q; a.r = r; a.rx = rx; a.ry = ry; a.N = N; a.ssqX = ssqX; a.ssqY = ssqY;
  HIPCHK(c, ppls_launch_po2_small(&a, 1, 0, 0, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int st = 0;
  HIPCHK(c, hipMemcpy(&st, ints, sizeof st, hipMemcpyDeviceToHost));
  if (status) *status = st;
  if (st != 0) return fail(c, PPLS_E_NUMERIC, "PO2PLS small kernel: status %d", st);
  if (loglik) HIPCHK(c, hipMemcpy(loglik, a.loglik, sizeof(double), hipMemcpyDeviceToHost));
  return po2_expect_out(c, a, s, false, out);
}

int ppls_po2_timing(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, int reps, double* ms6) {
  if (!c || !ms6 || reps < 1) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(c, r, rx, ry, c->p, c->q, &s)) || (rc = po2_check_theta(c, th, s, c->p, c->q))) return rc;
  if ((rc = po2_ready(c))) return rc;
  Po2Dev d;
  if ((rc = po2_setup(c, d, th, s, 2, true))) return rc;
  const size_t nx = sizeof(double) * c->ldx * s.kx, ny = sizeof(double) * c->ldy * s.ky;
  auto restore = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(d.a.Gx, d.Gx0, nx, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d.a.Gy, d.Gy0, ny, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d.a.sc, d.sc0, sizeof(PplsPo2Scalars), hipMemcpyDeviceToDevice, c->stream);
    return e;
  };
  // warm every kernel once, then time each part reps times between two events
  if ((rc = po2_pass(c, d, s))) return rc;
  HIPCHK(c, ppls_launch_po2_small(&d.a, 1, 0, 0, c->stream));
  for (int part = 0; part < 6; ++part) {
    d.a.type = part == 5 ? PPLS_ORTH_QR : PPLS_ORTH_SVD;   // part 5: the update without the polar factor
    HIPCHK(c, restore());
    if ((rc = po2_pass(c, d, s))) return rc;
    HIPCHK(c, ppls_launch_po2_small(&d.a, 1, 0, 0, c->stream));   // moments of theta for the update's inputs
    CvEvents ev;
    HIPCHK(c, ev.begin(c->stream));
    for (int i = 0; i < reps; ++i) {
      if (part == 0) { if ((rc = po2_panels(c, d.a, s.kx, s.ky, d.rw))) return rc; }
      else if (part == 1) HIPCHK(c, ppls_launch_po2_gram(&d.a, c->stream));
      else if (part == 2) HIPCHK(c, ppls_launch_po2_small(&d.a, 1, 0, 0, c->stream));
      else if (part == 3 || part == 5) HIPCHK(c, ppls_launch_po2_update(&d.a, c->stream));   // the same M, K, Czz every launch
      else {
        if ((rc = po2_pass(c, d, s))) return rc;
        HIPCHK(c, ppls_launch_po2_small(&d.a, 1, 1, 0, c->stream));
        HIPCHK(c, ppls_launch_po2_update(&d.a, c->stream));
      }
    }
    HIPCHK(c, ev.end(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ms6[part] = ev.ms() / reps;
    if ((rc = po2_status(c, d))) return rc;
  }
  return PPLS_OK;
}

// ---- batched PO2PLS: m fits on one S, prediction, cross-validation over (r, rx, ry)
int ppls_po2_em_run_batch(ppls_ctx* c, int m, ppls_po2_theta* th, const int* r, const int* rx, const int* ry, int max_steps,
                          double atol, int type, double* loglik, int cap, int* n_loglik, int* negative_increment, int* status) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (m < 1 || m > PPLS_PO2_BATCH_MAX) return fail(c, PPLS_E_ARG, "batch of %d models outside [1,%d]", m, PPLS_PO2_BATCH_MAX);
  if (!th || !r || !rx || !ry || !n_loglik || !status) return fail(c, PPLS_E_ARG, "NULL argument");
  int rc;
  const int p = c->p, q = c->q;
  std::vector<Po2Shape> sh((size_t)m);
  for (int j = 0; j < m; ++j)
    if ((rc = po2_shape(c, r[j], rx[j], ry[j], p, q, &sh[j])) || (rc = po2_check_theta(c, th + j, sh[j], p, q))) {
      c->err = "model " + std::to_string(j) + ": " + c->err;
      return rc;
    }
  if (max_steps < 1) return fail(c, PPLS_E_ARG, "EMsteps must be >= 1");
  if (type != PPLS_ORTH_SVD && type != PPLS_ORTH_QR) return fail(c, PPLS_E_ARG, "type must be SVD (0) or QR (1)");
  if (cap < 0 || (cap > 0 && !loglik) || std::isnan(atol)) return fail(c, PPLS_E_ARG, "bad loglik buffer or atol");
  if ((rc = po2_ready(c))) return rc;
  Po2Batch b;
  const int hist = max_steps + 2;
  if ((rc = po2_batch_alloc(c, b, c->xp_S, c->ldx, c->ldy, p, q, sh, hist, 0, true, type, atol))) return rc;
  if ((rc = po2_batch_upload(c, b, th, p, q))) return rc;
  const bool do_check = !(atol == -INFINITY);
  struct EvGuard {
    std::vector<hipEvent_t> evs;
    ~EvGuard() {
      for (auto e : evs) (void)hipEventDestroy(e);
    }
  } guard;
  constexpr int LOOKAHEAD = 8;   // as ppls_po2_em_run
  for (int i = 1; i <= max_steps + 1; ++i) {
    if (i > LOOKAHEAD) {
      HIPCHK(c, hipEventSynchronize(guard.evs[(size_t)(i - 1 - LOOKAHEAD) % LOOKAHEAD]));
      bool all = true;
      for (int j = 0; j < m && all; ++j) all = __atomic_load_n(b.mirror + j, __ATOMIC_ACQUIRE) != 0;
      if (all) break;
    }
    const bool last = i == max_steps + 1;
    if ((rc = po2_batch_pass(c, b))) return rc;
    HIPCHK(c, ppls_launch_po2_small_batch(b.da, m, i, last ? 0 : 1, do_check ? 1 : 0, c->stream));
    if (!last) HIPCHK(c, ppls_launch_po2_update_batch(b.da, m, c->stream));
    const size_t e = (size_t)(i - 1) % LOOKAHEAD;
    if (guard.evs.size() <= e) {
      hipEvent_t ev;
      HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      guard.evs.push_back(ev);
    }
    HIPCHK(c, hipEventRecord(guard.evs[e], c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<int> ints((size_t)4 * m);
  HIPCHK(c, hipMemcpy(ints.data(), b.ints, sizeof(int) * 4 * m, hipMemcpyDeviceToHost));
  std::string first;
  std::vector<double> l;
  for (int j = 0; j < m; ++j) {
    const int* sv = &ints[(size_t)4 * j];
    const int st = sv[2], npass = sv[0] > 0 && sv[0] <= max_steps + 1 ? sv[0] : max_steps + 1;
    rc = PPLS_OK;
    Po2Host h;
    if (st != 0) {
      rc = fail(c, PPLS_E_NUMERIC, "PO2PLS: %s (status %d)", po2_status_text(st), st);
    } else if (sv[1]) {
      rc = fail(c, PPLS_E_NUMERIC, "PO2PLS: the log-likelihood increment of EM iteration %d is NaN", npass - 1);
    } else {
      l.resize((size_t)npass);
      HIPCHK(c, hipMemcpy(l.data(), b.ha[j].loglik, sizeof(double) * npass, hipMemcpyDeviceToHost));
      for (int i = 0; i < npass && !rc; ++i)
        if (!std::isfinite(l[i])) rc = fail(c, PPLS_E_NUMERIC, "PO2PLS: non-finite log-likelihood %g at pass %d", l[i], i + 1);
      if (!rc) {
        char after[48];
        snprintf(after, sizeof after, "%d EM iterations", npass - 1);
        rc = po2_pull(c, b.ha[j], sh[j], h, after);
      }
    }
    if (rc && rc != PPLS_E_NUMERIC) return rc;
    status[j] = rc;
    if (rc) {   // theta j and its history stay as the caller gave them
      n_loglik[j] = 0;
      if (negative_increment) negative_increment[j] = 0;
      if (first.empty()) first = "model " + std::to_string(j) + ": " + c->err;
      continue;
    }
    ppls_po2_theta est = h.view();
    po2_canonical(&est, sh[j], p, q);
    h.hs.sE = est.sigE; h.hs.sF = est.sigF; h.hs.sH = est.sigH;
    po2_give(h, sh[j], p, q, th + j);
    for (int i = 0; i < npass && i < cap; ++i) loglik[(size_t)j * cap + i] = l[i];
    n_loglik[j] = npass;
    if (negative_increment) {
      int neg = 0;
      for (int i = 1; i < npass; ++i) neg |= (l[i] - l[i - 1] < 0);
      negative_increment[j] = neg;
    }
  }
  if (!first.empty()) c->err = first;
  return PPLS_OK;
}

int ppls_po2_timing_batch(ppls_ctx* c, int m, const ppls_po2_theta* th, const int* r, const int* rx, const int* ry, int steps,
                          int reps, double* ms4) {
  if (!c || !ms4 || reps < 1 || steps < 1) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  if (m < 1 || m > PPLS_PO2_BATCH_MAX) return fail(c, PPLS_E_ARG, "batch of %d models outside [1,%d]", m, PPLS_PO2_BATCH_MAX);
  if (!th || !r || !rx || !ry) return fail(c, PPLS_E_ARG, "NULL argument");
  int rc;
  const int p = c->p, q = c->q;
  std::vector<Po2Shape> sh((size_t)m);
  for (int j = 0; j < m; ++j)
    if ((rc = po2_shape(c, r[j], rx[j], ry[j], p, q, &sh[j])) || (rc = po2_check_theta(c, th + j, sh[j], p, q))) return rc;
  if ((rc = po2_ready(c))) return rc;
  Po2Batch b;
  if ((rc = po2_batch_alloc(c, b, c->xp_S, c->ldx, c->ldy, p, q, sh, 2, 0, true, PPLS_ORTH_SVD, -INFINITY))) return rc;
  std::vector<int> rws((size_t)m);
  for (int j = 0; j < m; ++j) rws[j] = ppls_xprod_tile_rows(b.P, std::max(sh[j].kx, sh[j].ky), c->xprod_rw, c->num_cus);
  auto failed = [&]() -> int {   // any model's status word
    std::vector<int> ints((size_t)4 * m);
    HIPCHK(c, hipMemcpy(ints.data(), b.ints, sizeof(int) * 4 * m, hipMemcpyDeviceToHost));
    for (int j = 0; j < m; ++j)
      if (ints[(size_t)4 * j + 2]) return fail(c, PPLS_E_NUMERIC, "model %d: PO2PLS: %s", j, po2_status_text(ints[(size_t)4 * j + 2]));
    return PPLS_OK;
  };
  for (int part = 0; part < 4; ++part) {   // every part from the same thetas; one untimed round warms the kernels
    if ((rc = po2_batch_upload(c, b, th, p, q))) return rc;
    double total = 0.0;
    for (int rep = -1; rep < reps; ++rep) {
      CvEvents ev;
      HIPCHK(c, ev.begin(c->stream));
      for (int i = 0; i < steps; ++i) {
        if (part == 0) {          // one batched iteration
          if ((rc = po2_batch_pass(c, b))) return rc;
          HIPCHK(c, ppls_launch_po2_small_batch(b.da, m, 1, 1, 0, c->stream));
          HIPCHK(c, ppls_launch_po2_update_batch(b.da, m, c->stream));
        } else if (part == 2) {   // the batched pass alone
          if ((rc = po2_batch_pass(c, b))) return rc;
        } else {                  // the models one after another through the single-model launches
          for (int j = 0; j < m; ++j) {
            if ((rc = po2_panels(c, b.ha[j], sh[j].kx, sh[j].ky, rws[j]))) return rc;
            HIPCHK(c, ppls_launch_po2_gram(&b.ha[j], c->stream));
            if (part == 1) {
              HIPCHK(c, ppls_launch_po2_small(&b.ha[j], 1, 1, 0, c->stream));
              HIPCHK(c, ppls_launch_po2_update(&b.ha[j], c->stream));
            }
          }
        }
      }
      HIPCHK(c, ev.end(c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (rep >= 0) total += ev.ms();
    }
    ms4[part] = total / ((double)reps * steps);
    if ((rc = failed())) return rc;
  }
  return PPLS_OK;
}

int ppls_po2_stats_batch(ppls_ctx* c, const double* S, int P, int ldx, int m, const int* kx, const int* ky, const double* Gx,
                         const double* Gy, double* M, double* Q, double* GG) {
  if (!c) return PPLS_E_ARG;
  if (!kx || !ky || !Gx || !Gy || !M || !Q || !GG) return fail(c, PPLS_E_ARG, "NULL argument");
  if (m < 1 || m > PPLS_PO2_BATCH_MAX) return fail(c, PPLS_E_ARG, "batch of %d models outside [1,%d]", m, PPLS_PO2_BATCH_MAX);
  const int ldy = P - ldx;
  if (ldx < 2 || ldy < 2 || (ldx & 1) || (ldy & 1) || P >= (1 << 30)) return fail(c, PPLS_E_ARG, "bad layout P=%d ldx=%d", P, ldx);
  std::vector<Po2Shape> sh((size_t)m);
  for (int j = 0; j < m; ++j) {
    if (kx[j] < 1 || ky[j] < 1 || kx[j] > PPLS_RMAX || ky[j] > PPLS_RMAX)
      return fail(c, PPLS_E_ARG, "model %d: widths kx=%d ky=%d outside [1,%d]", j, kx[j], ky[j], PPLS_RMAX);
    sh[j] = {1, kx[j] - 1, ky[j] - 1, kx[j], ky[j], kx[j] + ky[j]};
  }
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  const double* Sd = nullptr;
  CvScratch tmp;
  if (S) {
    double* up = nullptr;
    if ((rc = tmp.get(c, &up, (size_t)P * P))) return rc;
    HIPCHK(c, hipMemcpy(up, S, sizeof(double) * P * P, hipMemcpyHostToDevice));
    Sd = up;
  } else {
    if (!c->have_data || !c->xp_ready || !c->xp_S) return fail(c, PPLS_E_STATE, "no cross-products S are ready");
    if (P != c->ldx + c->ldy || ldx != c->ldx) return fail(c, PPLS_E_ARG, "P=%d ldx=%d are not the context's %d, %d", P, ldx, c->ldx + c->ldy, c->ldx);
    Sd = c->xp_S;
  }
  const size_t guard = 64;
  Po2Batch b;
  if ((rc = po2_batch_alloc(c, b, Sd, ldx, ldy, ldx, ldy, sh, 0, guard, false, 0, 0.0))) return rc;
  HIPCHK(c, hipMemcpy(b.Gx, Gx, sizeof(double) * ldx * b.sumx, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(b.Gy, Gy, sizeof(double) * ldy * b.sumy, hipMemcpyHostToDevice));
  const size_t nMall = (size_t)P * (b.sumx + b.sumy) + 3 * guard, nQ = b.qstride * m, nG = b.gstride * m;
  double* Mall = b.Mx - guard;
  HIPCHK(c, hipMemsetAsync(Mall, 0xFF, sizeof(double) * nMall, c->stream));
  HIPCHK(c, hipMemsetAsync(b.Q, 0xFF, sizeof(double) * nQ, c->stream));
  HIPCHK(c, hipMemsetAsync(b.GGx, 0xFF, sizeof(double) * nG, c->stream));
  HIPCHK(c, hipMemsetAsync(b.GGy, 0xFF, sizeof(double) * nG, c->stream));
  if ((rc = po2_batch_pass(c, b))) return rc;
  std::vector<double> hM(nMall), hQ(nQ), hX(nG), hY(nG);
  HIPCHK(c, hipMemcpyAsync(hM.data(), Mall, sizeof(double) * nMall, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hQ.data(), b.Q, sizeof(double) * nQ, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hX.data(), b.GGx, sizeof(double) * nG, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hY.data(), b.GGy, sizeof(double) * nG, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // every double outside an output must still be the fill
  const size_t oMx = guard, oMy = oMx + (size_t)P * b.sumx + guard;
  bool clean = true;
  for (size_t g = 0; g < guard && clean; ++g)
    clean = std::isnan(hM[g]) && std::isnan(hM[oMy - guard + g]) && std::isnan(hM[nMall - guard + g]);
  for (int j = 0; j < m && clean; ++j) {
    for (size_t e = (size_t)sh[j].k * sh[j].k; e < b.qstride && clean; ++e) clean = std::isnan(hQ[b.qstride * j + e]);
    for (size_t e = (size_t)sh[j].kx * sh[j].kx; e < b.gstride && clean; ++e) clean = std::isnan(hX[b.gstride * j + e]);
    for (size_t e = (size_t)sh[j].ky * sh[j].ky; e < b.gstride && clean; ++e) clean = std::isnan(hY[b.gstride * j + e]);
  }
  if (!clean) return fail(c, PPLS_E_NUMERIC, "a batched PO2 statistics kernel wrote outside its output");
  for (int j = 0; j < m; ++j) {   // per model: M (P x k), Q (k x k), GG = [kx^2 | ky^2], each packed after the one before
    const size_t nx = (size_t)P * sh[j].kx, ny = (size_t)P * sh[j].ky, k2 = (size_t)sh[j].k * sh[j].k;
    const size_t gx2 = (size_t)sh[j].kx * sh[j].kx, gy2 = (size_t)sh[j].ky * sh[j].ky;
    std::copy(hM.begin() + oMx + (size_t)b.offx[j] * P, hM.begin() + oMx + (size_t)b.offx[j] * P + nx, M);
    std::copy(hM.begin() + oMy + (size_t)b.offy[j] * P, hM.begin() + oMy + (size_t)b.offy[j] * P + ny, M + nx);
    std::copy(hQ.begin() + b.qstride * j, hQ.begin() + b.qstride * j + k2, Q);
    std::copy(hX.begin() + b.gstride * j, hX.begin() + b.gstride * j + gx2, GG);
    std::copy(hY.begin() + b.gstride * j, hY.begin() + b.gstride * j + gy2, GG + gx2);
    M += nx + ny; Q += k2; GG += gx2 + gy2;
  }
  return PPLS_OK;
}

int ppls_po2_predict_map(const ppls_po2_theta* th, int r, int rx, int ry, int p, int q, int xory, double* L, double* Bp) {
  if (!th || !L || !Bp || (xory != 0 && xory != 1)) return PPLS_E_ARG;
  int rc;
  Po2Shape s;
  if ((rc = po2_shape(nullptr, r, rx, ry, p, q, &s)) || (rc = po2_check_theta(nullptr, th, s, p, q))) return rc;
  const int n = xory ? q : p, k = xory ? s.ky : s.kx;
  const double *A = xory ? th->C : th->W, *Ao = xory ? th->Co : th->Wo, *sgo = xory ? th->sigUo : th->sigTo;
  const double sn = xory ? th->sigF : th->sigE, dn = 1.0 / (sn * sn);
  auto col = [&](int j) { return j < r ? A + (size_t)j * n : Ao + (size_t)(j - r) * n; };
  // Lambda = Sigma^-1 + G'G / sigma^2 for the side's own latent variables: (t, to) with variances sigT^2,
  // sigTo^2; (u, uo) with sigT^2 b^2 + sigH^2, sigUo^2 (the marginal of u, not its conditional given t)
  std::vector<double> Lam((size_t)k * k);
  for (int b = 0; b < k; ++b)
    for (int a = b; a < k; ++a) {
      double g = 0.0;
      const double *u = col(a), *v = col(b);
      for (int i = 0; i < n; ++i) g = std::fma(u[i], v[i], g);
      Lam[(size_t)b * k + a] = Lam[(size_t)a * k + b] = g * dn;
    }
  for (int j = 0; j < k; ++j) {
    double var;
    if (j >= r) var = sgo[j - r] * sgo[j - r];
    else if (xory) var = th->sigT[j] * th->sigT[j] * th->B[j] * th->B[j] + th->sigH * th->sigH;
    else var = th->sigT[j] * th->sigT[j];
    Lam[(size_t)j * k + j] += 1.0 / var;
  }
  if (!po2_host_chol(Lam, k)) return PPLS_E_NUMERIC;
  if (xory)
    for (int j = 0; j < r; ++j)   // 1 / beta_j must exist
      if (th->B[j] == 0.0) return PPLS_E_NUMERIC;
  std::vector<double> X((size_t)k * r, 0.0);   // Lambda X = the first r unit vectors
  for (int c0 = 0; c0 < r; ++c0) {
    double* x = &X[(size_t)c0 * k];
    x[c0] = 1.0;
    for (int i = 0; i < k; ++i) {
      double sacc = x[i];
      for (int m = 0; m < i; ++m) sacc -= Lam[(size_t)m * k + i] * x[m];
      x[i] = sacc / Lam[(size_t)i * k + i];
    }
    for (int i = k - 1; i >= 0; --i) {
      double sacc = x[i];
      for (int m = i + 1; m < k; ++m) sacc -= Lam[(size_t)i * k + m] * x[m];
      x[i] = sacc / Lam[(size_t)i * k + i];
    }
  }
  for (int c0 = 0; c0 < r; ++c0)
    for (int i = 0; i < n; ++i) {
      double acc = 0.0;
      for (int m = 0; m < k; ++m) acc = std::fma(col(m)[i], X[(size_t)c0 * k + m], acc);
      L[(size_t)c0 * n + i] = acc * dn;
    }
  for (int j = 0; j < r; ++j) {
    if (!xory) { Bp[j] = th->B[j]; continue; }
    const double vt = th->sigT[j] * th->sigT[j], b = th->B[j];
    Bp[j] = (vt * b * b + th->sigH * th->sigH) / (vt * b);   // 1 / beta_j
  }
  return PPLS_OK;
}

int ppls_po2_cv_stream(ppls_ctx* c, int ncand, const int* r, const int* rx, const int* ry, int max_steps, double atol, int type,
                       const double* V0x, const double* V0y, int start_steps, double* rmsep, double* cond, int* steps,
                       int* status, ppls_po2_theta* fits) {
  if (!c) return PPLS_E_ARG;
  int rc;
  if ((rc = fold_state_check(c))) return rc;
  if (c->em_active)
    return fail(c, PPLS_E_STATE, "an ppls_em_begin session is active on the selected cross-products: finish it before cross-validating");
  if (ncand < 1 || ncand > PPLS_PO2_BATCH_MAX) return fail(c, PPLS_E_ARG, "%d candidates outside [1,%d]", ncand, PPLS_PO2_BATCH_MAX);
  if (!r || !rx || !ry || !rmsep || !status) return fail(c, PPLS_E_ARG, "NULL argument");
  const int K = c->st_nfolds, p = c->p, q = c->q;
  std::vector<Po2Shape> sh((size_t)ncand);
  int mrx = 0, mry = 0;
  for (int j = 0; j < ncand; ++j) {
    if ((rc = po2_shape(c, r[j], rx[j], ry[j], p, q, &sh[j]))) return rc;
    mrx = std::max(mrx, rx[j]); mry = std::max(mry, ry[j]);
  }
  if ((mrx && !V0x) || (mry && !V0y)) return fail(c, PPLS_E_ARG, "NULL argument");
  for (size_t e = 0; e < (size_t)p * mrx; ++e)
    if (!std::isfinite(V0x[e])) return fail(c, PPLS_E_ARG, "V0x has non-finite entries");
  for (size_t e = 0; e < (size_t)q * mry; ++e)
    if (!std::isfinite(V0y[e])) return fail(c, PPLS_E_ARG, "V0y has non-finite entries");
  if (max_steps < 1 || start_steps < 0) return fail(c, PPLS_E_ARG, "EMsteps must be >= 1 and start_steps >= 0");
  if (type != PPLS_ORTH_SVD && type != PPLS_ORTH_QR) return fail(c, PPLS_E_ARG, "type must be SVD (0) or QR (1)");
  if (std::isnan(atol)) return fail(c, PPLS_E_ARG, "bad atol");
  if (fits)
    for (int e = 0; e < K * ncand; ++e) {
      const Po2Shape& s = sh[(size_t)(e % ncand)];
      const ppls_po2_theta& t = fits[e];
      if (!t.W || !t.C || !t.B || !t.sigT || (s.rx && (!t.Wo || !t.sigTo)) || (s.ry && (!t.Co || !t.sigUo)))
        return fail(c, PPLS_E_ARG, "fits[%d] has NULL fields", e);
    }
  auto run = [&]() -> int {
    int rr;
    std::vector<Po2Host> own((size_t)ncand);
    std::vector<ppls_po2_theta> view((size_t)ncand), bth;
    std::vector<int> idx, br, brx, bry, nl, bst;
    std::vector<double> L, Bp((size_t)PPLS_RMAX), sse((size_t)PPLS_RMAX), mag((size_t)PPLS_RMAX);
    for (int f = 0; f < K; ++f) {
      if ((rr = ppls_stream_select(c, f))) return rr;
      if (c->n_total < 1) return fail(c, PPLS_E_ARG, "fold %d leaves no training row", f);
      idx.clear(); bth.clear(); br.clear(); brx.clear(); bry.clear();
      for (int j = 0; j < ncand; ++j) {
        const size_t o = (size_t)f * ncand + j;
        rmsep[o] = NAN;
        if (cond) cond[o] = NAN;
        if (steps) steps[o] = 0;
        po2_host_sized(own[j], sh[j], p, q);
        view[j] = own[j].view();
        rr = ppls_po2_start(c, r[j], rx[j], ry[j], V0x, V0y, start_steps, &view[j]);
        if (rr && rr != PPLS_E_NUMERIC) return rr;
        status[o] = rr;
        if (rr) continue;
        idx.push_back(j); bth.push_back(view[j]); br.push_back(r[j]); brx.push_back(rx[j]); bry.push_back(ry[j]);
      }
      const int mb = (int)idx.size();
      if (mb == 0) continue;
      nl.assign(mb, 0); bst.assign(mb, 0);
      if ((rr = ppls_po2_em_run_batch(c, mb, bth.data(), br.data(), brx.data(), bry.data(), max_steps, atol, type, nullptr, 0,
                                      nl.data(), nullptr, bst.data())))
        return rr;
      for (int i = 0; i < mb; ++i) {
        const int j = idx[i];
        const size_t o = (size_t)f * ncand + j;
        status[o] = bst[i];
        if (bst[i]) continue;
        if (steps) steps[o] = nl[i] - 1;
        const ppls_po2_theta& t = bth[i];
        if (fits) {   // the caller's buffers (checked above)
          ppls_po2_theta& o_ = fits[o];
          std::copy(t.W, t.W + (size_t)p * r[j], o_.W);
          std::copy(t.C, t.C + (size_t)q * r[j], o_.C);
          std::copy(t.B, t.B + r[j], o_.B);
          std::copy(t.sigT, t.sigT + r[j], o_.sigT);
          if (rx[j]) { std::copy(t.Wo, t.Wo + (size_t)p * rx[j], o_.Wo); std::copy(t.sigTo, t.sigTo + rx[j], o_.sigTo); }
          if (ry[j]) { std::copy(t.Co, t.Co + (size_t)q * ry[j], o_.Co); std::copy(t.sigUo, t.sigUo + ry[j], o_.sigUo); }
          o_.sigE = t.sigE; o_.sigF = t.sigF; o_.sigH = t.sigH;
        }
        L.assign((size_t)p * r[j], 0.0);
        if ((rr = ppls_po2_predict_map(&t, r[j], rx[j], ry[j], p, q, 0, L.data(), Bp.data()))) {
          if (rr != PPLS_E_NUMERIC) return fail(c, rr, "PO2PLS prediction map of candidate %d refused", j);
          status[o] = rr;
          continue;
        }
        if ((rr = ppls_heldout_sse_fold(c, L.data(), t.C, Bp.data(), r[j], f, sse.data(), mag.data()))) return rr;
        const double s1 = sse[(size_t)r[j] - 1];
        rmsep[o] = std::sqrt(s1 / ((double)c->st_fN[(size_t)f] * q));
        if (cond) cond[o] = mag[(size_t)r[j] - 1] / s1;
      }
    }
    return PPLS_OK;
  };
  rc = run();
  const std::string err = c->err;   // selected on all folds again, also after an error (whose message stays)
  const int rs = fold_select(c, -1);
  if (rc) c->err = err;
  return rc ? rc : rs;
}

}  // extern "C"

// ============================================================================ PO2PLS row diagnostics
// Per row under a PO2PLS fit: the orthogonal distances to the planes of [W Wo] and [C Co], the in-plane score
// distance, the log-density and the posterior means (ppls_po2_rowdiag.hip).  The loadings need not be
// orthonormal: the host factors them (Householder QR, R's diagonal positive) and the kernel works in the
// orthonormal bases; the k x k covariance of the scores is dense.  The weights of the t model follow from the
// same three arrays by §24's kernel.
namespace {

struct Po2RowFit {
  std::vector<double> Qx, Qy, tab;   // p x kx, q x ky, PPLS_PO2_ROWDIAG_TAB
  double *dQx = nullptr, *dQy = nullptr, *dtab = nullptr;
  RowDiagFit f;   // sE2, sF2, cst, logdet (its device pointers are not used)
};

// [A | Ao] = Q R by Householder QR: Q (n x c, orthonormal columns), R (c x c column-major, upper, diagonal
// positive).  false: a pivot at or below §26's rule, R_kk^2 <= 64 c u ||column k||^2 (rank deficient).
bool po2_row_qr(const double* A, int ca, const double* Ao, int co, int n, std::vector<double>& Q, double* R) {
  const int c = ca + co;
  std::vector<double> G((size_t)n * c), floor2(c);
  for (int j = 0; j < c; ++j) {
    const double* src = j < ca ? A + (size_t)j * n : Ao + (size_t)(j - ca) * n;
    std::copy(src, src + n, &G[(size_t)j * n]);
    floor2[j] = hdot(src, src, n) * (64.0 * c * 1.1102230246251565e-16);
  }
  if (host_householder(G.data(), n, c, floor2.data(), Q, R) >= 0) return false;
  for (int k = 0; k < c; ++k)
    if (!std::isfinite(R[(size_t)k * c + k])) return false;   // |R_kk| is the pivot column's norm
  for (int k = 0; k < c; ++k)
    if (R[(size_t)k * c + k] < 0.0) {   // R's diagonal positive: row k of R and column k of Q change sign
      for (int j = k; j < c; ++j) R[(size_t)j * c + k] = -R[(size_t)j * c + k];
      for (int i = 0; i < n; ++i) Q[(size_t)k * n + i] = -Q[(size_t)k * n + i];
    }
  return true;
}

// Everything the PO2 row entries refuse about the fit, and the host algebra of §29, before any device work.
int po2_row_check_fit(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, Po2Shape& s, Po2RowFit& f) {
  int rc;
  const int p = c->p, q = c->q;
  if ((rc = po2_shape(c, r, rx, ry, p, q, &s)) || (rc = po2_check_theta(c, th, s, p, q))) return rc;
  const int kx = s.kx, k = s.k;
  std::vector<double> R((size_t)k * k, 0.0), Rx((size_t)kx * kx), Ry((size_t)s.ky * s.ky);
  if (!po2_row_qr(th->W, r, th->Wo, rx, p, f.Qx, Rx.data())) return fail(c, PPLS_E_ARG, "PO2PLS theta: [W Wo] is rank deficient");
  if (!po2_row_qr(th->C, r, th->Co, ry, q, f.Qy, Ry.data())) return fail(c, PPLS_E_ARG, "PO2PLS theta: [C Co] is rank deficient");
  auto at = [k](std::vector<double>& M, int i, int j) -> double& { return M[(size_t)j * k + i]; };
  for (int j = 0; j < kx; ++j)
    for (int i = 0; i <= j; ++i) at(R, i, j) = Rx[(size_t)j * kx + i];
  for (int j = 0; j < s.ky; ++j)
    for (int i = 0; i <= j; ++i) at(R, kx + i, kx + j) = Ry[(size_t)j * s.ky + i];
  // Sigma_z of z = (t, to | u, uo)
  std::vector<double> Sz((size_t)k * k, 0.0), T1((size_t)k * k, 0.0), Sc((size_t)k * k, 0.0);
  const double sE2 = th->sigE * th->sigE, sF2 = th->sigF * th->sigF, sH2 = th->sigH * th->sigH;
  for (int j = 0; j < r; ++j) {
    const double t2 = th->sigT[j] * th->sigT[j], b = th->B[j];
    at(Sz, j, j) = t2;
    at(Sz, j, kx + j) = at(Sz, kx + j, j) = t2 * b;
    at(Sz, kx + j, kx + j) = t2 * b * b + sH2;
  }
  for (int j = 0; j < rx; ++j) at(Sz, r + j, r + j) = th->sigTo[j] * th->sigTo[j];
  for (int j = 0; j < ry; ++j) at(Sz, kx + r + j, kx + r + j) = th->sigUo[j] * th->sigUo[j];
  // T1 = R Sigma_z; Sigma_c = T1 R' + diag(sE2 I, sF2 I), its lower triangle mirrored
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      double a = 0.0;
      for (int m = i; m < k; ++m) a += at(R, i, m) * at(Sz, m, j);
      at(T1, i, j) = a;
    }
  for (int j = 0; j < k; ++j)
    for (int i = j; i < k; ++i) {
      double a = 0.0;
      for (int m = j; m < k; ++m) a += at(T1, i, m) * at(R, j, m);
      if (i == j) a += i < kx ? sE2 : sF2;
      at(Sc, i, j) = at(Sc, j, i) = a;
    }
  // Sigma_c^-1 = Uc'Uc with Uc upper: the lower Cholesky factor of Sigma_c with its indices reversed, inverted
  std::vector<double> Lr((size_t)k * k), Li((size_t)k * k, 0.0), Uc((size_t)k * k, 0.0), UT((size_t)k * k, 0.0);
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) at(Lr, i, j) = at(Sc, k - 1 - i, k - 1 - j);
  if (!po2_host_chol(Lr, k)) return fail(c, PPLS_E_ARG, "PO2PLS theta: the covariance of the scores is not positive definite");
  double logdet_c = 0.0;
  for (int j = 0; j < k; ++j) {
    logdet_c += 2.0 * std::log(at(Lr, j, j));
    at(Li, j, j) = 1.0 / at(Lr, j, j);
    for (int i = j + 1; i < k; ++i) {
      double a = 0.0;
      for (int m = j; m < i; ++m) a += at(Lr, i, m) * at(Li, m, j);
      at(Li, i, j) = -a / at(Lr, i, i);
    }
  }
  for (int j = 0; j < k; ++j)
    for (int i = 0; i <= j; ++i) at(Uc, i, j) = at(Li, k - 1 - i, k - 1 - j);
  // Kmu = R K = Sigma_c^-1 R Sigma_z = Uc' (Uc T1): row j belongs to score j, column i to latent i
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      double a = 0.0;
      for (int m = i; m < k; ++m) a += at(Uc, i, m) * at(T1, m, j);
      at(UT, i, j) = a;
    }
  f.tab.assign(PPLS_PO2_ROWDIAG_TAB, 0.0);
  bool ok = std::isfinite(logdet_c);
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) {
      double a = 0.0;
      for (int m = 0; m <= j; ++m) a += at(Uc, m, j) * at(UT, m, i);
      f.tab[(size_t)j * 64 + i] = at(Uc, i, j);
      f.tab[(size_t)j * 64 + 32 + i] = a;
      ok = ok && std::isfinite(a) && std::isfinite(at(Uc, i, j));
    }
  if (!ok) return fail(c, PPLS_E_ARG, "PO2PLS theta: the covariance of the scores is not positive definite");
  f.f.sE2 = sE2;
  f.f.sF2 = sF2;
  f.f.logdet = ((double)(p - kx) * std::log(sE2) + (double)(q - s.ky) * std::log(sF2)) + logdet_c;
  f.f.cst = -0.5 * ((double)(p + q) * std::log(6.283185307179586) + f.f.logdet);
  return PPLS_OK;
}

int po2_row_upload_fit(ppls_ctx* c, CvScratch& tmp, const Po2Shape& s, Po2RowFit& f) {
  int rc;
  if ((rc = cv_upload_coef(c, tmp, f.Qx.data(), c->p, s.kx, &f.dQx))) return rc;
  if ((rc = cv_upload_coef(c, tmp, f.Qy.data(), c->q, s.ky, &f.dQy))) return rc;
  return cv_upload_coef(c, tmp, f.tab.data(), PPLS_PO2_ROWDIAG_TAB, 1, &f.dtab);
}

// The device stage on the resident rows, queued on the context stream with no copy-out, as rowdiag_device:
// res = [odx2 | ody2 | sd2] (nrows each) and, with mu, dmu (nrows x k); both live in tmp.
int po2_row_device(ppls_ctx* c, CvScratch& tmp, const Po2Shape& s, Po2RowFit& f, const int64_t* d_rows, int64_t nrows, bool mu,
                   double** res_out, double** dmu_out) {
  int rc;
  if ((rc = po2_row_upload_fit(c, tmp, s, f))) return rc;
  double *res = nullptr, *dmu = nullptr;
  if ((rc = tmp.get(c, &res, (size_t)3 * nrows))) return rc;
  if (mu && (rc = tmp.get(c, &dmu, (size_t)nrows * s.k))) return rc;
  HIPCHK(c, ppls_launch_po2_rowdiag(c->X, c->ldx, c->p, c->Y, c->ldy, c->q, c->dtype, d_rows, nrows, f.dQx, s.kx, f.dQy, s.ky,
                                    f.dtab, res, res + nrows, res + 2 * nrows, dmu, nrows,
                                    ppls_po2_rowdiag_grid(nrows, c->p, c->q, c->dtype, s.kx, s.ky, c->num_cus), c->stream));
  *res_out = res;
  *dmu_out = dmu;
  return PPLS_OK;
}

// rowdiag_collect with the k columns of mu in the place of mu_T.
int po2_row_collect(ppls_ctx* c, const Po2RowFit& f, const double* dres, const double* dmu, int64_t count, int k, int64_t at,
                    int64_t n, ppls_po2_row_diag* out) {
  ppls_row_diag o = {out->odx2, out->ody2, out->sd2, out->d2, out->loglik, out->mu, nullptr};
  return rowdiag_collect(c, f.f, dres, dmu, count, k, at, n, &o);
}

}  // namespace

extern "C" {

int ppls_po2_row_diagnostics(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, const int64_t* rows, int64_t nrows,
                             ppls_po2_row_diag* out) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!out) return fail(c, PPLS_E_ARG, "NULL output");
  Po2Shape s;
  Po2RowFit f;
  int rc;
  if ((rc = po2_row_check_fit(c, th, r, rx, ry, s, f))) return rc;
  if (!rows) nrows = c->n_local;   // all local rows
  if (nrows < 0) return fail(c, PPLS_E_ARG, "row list: %lld rows", (long long)nrows);
  for (int64_t i = 0; rows && i < nrows; ++i)   // any order, repeats allowed: the kernel only reads
    if (rows[i] < 0 || rows[i] >= c->n_local)
      return fail(c, PPLS_E_ARG, "row index %lld (entry %lld) outside [0, %lld)", (long long)rows[i], (long long)i,
                  (long long)c->n_local);
  if (nrows == 0) return PPLS_OK;
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  int64_t* d_rows = nullptr;
  if (rows && (rc = cv_upload_rows(c, tmp, rows, nrows, &d_rows))) return rc;
  double *res = nullptr, *dmu = nullptr;
  if ((rc = po2_row_device(c, tmp, s, f, d_rows, nrows, out->mu != nullptr, &res, &dmu))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return po2_row_collect(c, f, res, dmu, nrows, s.k, 0, nrows, out);
}

int ppls_po2_robust_weights(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, const double* nu, int m, int keep,
                            double* loglik_t, double* sum_w) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!nu || !loglik_t) return fail(c, PPLS_E_ARG, "NULL argument");
  Po2Shape s;
  Po2RowFit f;
  int rc;
  if ((rc = po2_row_check_fit(c, th, r, rx, ry, s, f))) return rc;
  return robust_weights_run(c, nu, m, keep, loglik_t, sum_w, f.f.sE2, f.f.sF2, f.f.logdet,
                            [&](CvScratch& tmp, int64_t n, double** res) {
                              double* dmu = nullptr;
                              return po2_row_device(c, tmp, s, f, nullptr, n, false, res, &dmu);
                            });
}

int ppls_po2_row_diagnostics_new(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, const double* X, const double* Y,
                                 int64_t n, int layout, ppls_po2_row_diag* out) {
  if (!c) return PPLS_E_ARG;
  if (c->p < 1 || c->q < 1) return fail(c, PPLS_E_STATE, "no data shape: load data (p, q) first");
  if (!out) return fail(c, PPLS_E_ARG, "NULL output");
  Po2Shape s;
  Po2RowFit f;
  int rc;
  if ((rc = po2_row_check_fit(c, th, r, rx, ry, s, f))) return rc;
  if (layout != PPLS_LAYOUT_COLMAJOR && layout != PPLS_LAYOUT_ROWMAJOR)
    return fail(c, PPLS_E_ARG, "layout must be 0 (column-major) or 1 (row-major)");
  if (n < 0 || (n > 0 && (!X || !Y))) return fail(c, PPLS_E_ARG, "NULL X or Y with %lld rows", (long long)n);
  if (n == 0) return PPLS_OK;
  const int p = c->p, q = c->q;
  for (int blk = 0; blk < 2; ++blk) {   // the whole call is refused, as ppls_set_data refuses such data
    const double* D = blk ? Y : X;
    const size_t len = (size_t)n * (blk ? q : p);
    for (size_t e = 0; e < len; ++e)
      if (!std::isfinite(D[e])) return fail(c, PPLS_E_ARG, "%c contains NaN or Inf", blk ? 'Y' : 'X');
  }
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  if ((rc = po2_row_upload_fit(c, tmp, s, f))) return rc;
  // row blocks through a staging buffer (~64 MB of rows at a time), always staged in fp64
  const int ldx = (p + 1) & ~1, ldy = (q + 1) & ~1;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(64 << 20) / (8LL * (ldx + ldy))));
  double *inX = nullptr, *inY = nullptr, *cm = nullptr, *res = nullptr, *dmu = nullptr;
  if ((rc = tmp.get(c, &inX, (size_t)chunk * ldx))) return rc;
  if ((rc = tmp.get(c, &inY, (size_t)chunk * ldy))) return rc;
  if (layout == PPLS_LAYOUT_COLMAJOR && (rc = tmp.get(c, &cm, (size_t)chunk * std::max(p, q)))) return rc;
  if ((rc = tmp.get(c, &res, (size_t)3 * chunk))) return rc;
  if (out->mu && (rc = tmp.get(c, &dmu, (size_t)chunk * s.k))) return rc;
  HIPCHK(c, hipMemsetAsync(inX, 0, sizeof(double) * chunk * ldx, c->stream));
  HIPCHK(c, hipMemsetAsync(inY, 0, sizeof(double) * chunk * ldy, c->stream));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t nc = std::min(chunk, n - r0);
    for (int blk = 0; blk < 2; ++blk) {
      const double* D = blk ? Y : X;
      double* in = blk ? inY : inX;
      const int cols = blk ? q : p, ld = blk ? ldy : ldx;
      if (layout == PPLS_LAYOUT_ROWMAJOR) {
        HIPCHK(c, hipMemcpy2DAsync(in, sizeof(double) * ld, D + r0 * cols, sizeof(double) * cols, sizeof(double) * cols, nc,
                                   hipMemcpyHostToDevice, c->stream));
      } else {
        HIPCHK(c, hipMemcpy2DAsync(cm, sizeof(double) * nc, D + r0, sizeof(double) * n, sizeof(double) * nc, cols,
                                   hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, ppls_launch_to_rowmajor(cm, nc, cols, ld, in, c->stream));
      }
    }
    HIPCHK(c, ppls_launch_po2_rowdiag(inX, ldx, p, inY, ldy, q, 0, nullptr, nc, f.dQx, s.kx, f.dQy, s.ky, f.dtab, res, res + nc,
                                      res + 2 * nc, dmu, nc, ppls_po2_rowdiag_grid(nc, p, q, 0, s.kx, s.ky, c->num_cus),
                                      c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = po2_row_collect(c, f, res, dmu, nc, s.k, r0, n, out))) return rc;
  }
  return PPLS_OK;
}

int ppls_po2_rowdiag_info(int p, int q, int f32, int r, int rx, int ry, int* tile_x, int* tile_y, int* rows_per_wave) {
  if (r < 1 || rx < 0 || ry < 0 || r + rx > PPLS_RMAX || r + ry > PPLS_RMAX || r + rx > p || r + ry > q) return PPLS_E_ARG;
  if (tile_x) *tile_x = ppls_po2_rowdiag_tile(r + rx);
  if (tile_y) *tile_y = ppls_po2_rowdiag_tile(r + ry);
  if (rows_per_wave) *rows_per_wave = ppls_po2_rowdiag_rows_per_wave(p, q, f32, r + rx, r + ry);
  return PPLS_OK;
}

int ppls_po2_rowdiag_timing(ppls_ctx* c, const ppls_po2_theta* th, int r, int rx, int ry, int reps, double* ms) {
  if (!c) return PPLS_E_ARG;
  if (!c->have_data) return fail(c, PPLS_E_STATE, "no data");
  NEED_ROWS(c);
  if (!ms || reps < 1) return fail(c, PPLS_E_ARG, "ms must be given with reps >= 1");
  Po2Shape s;
  Po2RowFit f;
  int rc;
  if ((rc = po2_row_check_fit(c, th, r, rx, ry, s, f))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  CvScratch tmp;
  if ((rc = po2_row_upload_fit(c, tmp, s, f))) return rc;
  const int64_t n = c->n_local;
  double *res = nullptr, *dmu = nullptr;
  if ((rc = tmp.get(c, &res, (size_t)3 * std::max<int64_t>(n, 1)))) return rc;
  if ((rc = tmp.get(c, &dmu, (size_t)std::max<int64_t>(n, 1) * s.k))) return rc;
  const int grid = ppls_po2_rowdiag_grid(n, c->p, c->q, c->dtype, s.kx, s.ky, c->num_cus);
  for (int v = 0; v < 2; ++v) {
    CvEvents ev;
    for (int it = 0; it <= reps; ++it) {   // one untimed launch first
      if (it == 1) HIPCHK(c, ev.begin(c->stream));
      HIPCHK(c, ppls_launch_po2_rowdiag(c->X, c->ldx, c->p, c->Y, c->ldy, c->q, c->dtype, nullptr, n, f.dQx, s.kx, f.dQy, s.ky,
                                        f.dtab, res, res + n, res + 2 * n, v ? dmu : nullptr, n, grid, c->stream));
    }
    HIPCHK(c, ev.end(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ms[v] = ev.ms() / reps;
  }
  return PPLS_OK;
}

}  // extern "C"
