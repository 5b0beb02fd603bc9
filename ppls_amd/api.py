"""Host-side mirror of the reference's R interface for the PPLS_simult hot path.

Same names, argument meaning, return structure and error behaviour as the R functions
(paths relative to /root/reference):

* ``PPLS_simult``  Package/PPLS/R/EM_W_multi.R:758-807
* ``Expect_M``     Package/PPLS/R/EM_W_multi.R:637-717
* ``Maximiz_M``    Package/PPLS/R/EM_W_multi.R:729-742
* ``logl_W``       Package/PPLS/R/EM_W_multi.R:297-323
* ``loglC_fast``   Package/PPLS/src/loglC.cpp:318-338 (via RcppExports.R:32-34)
* ``meta_EMstep``  Package/PPLS/R/EM_W_multi.R:446-485 (meta_Estep/meta_Mstep, src/loglC.cpp:399-474)
* ``meta_PPLSi``   Package/PPLS/R/EM_W_multi.R:509-589
* ``PPLS_to_o2m``  Package/PPLS/R/PPLS_to_o2m.R:28-80
* ``variances_PPLS_simult``  Package/PPLS/R/EM_W_multi.R:830-860 (variances.PPLS_simult)
* ``PO2PLS_Expect`` / ``PO2PLS_logl`` / ``PO2PLS``  Package/PPLS/src/loglC.cpp:116-250 (EMstepC), :36-113 (loglC), and
  the loop the reference leaves unwritten (:228)

Every call goes through the C ABI (include/ppls.h) into the HIP kernels on the GPU; matrices
are numpy arrays, R lists are dicts.  Passing ``X=None, Y=None`` uses the data already resident
in the context (no copy), which is how multi-GPU shards and large synthetic problems are driven.
"""
from __future__ import annotations

import ctypes as ct
import itertools
import math
import time
import warnings

import numpy as np

from . import _lib
from ._lib import Expect, Po2Expect, Po2Theta, PplsError, Theta, dptr
from .po2 import canonical_PO2PLS, po2_predict_map, select_grid_PO2PLS, simulate_PO2PLS, summary_PO2PLS  # noqa: F401


def pop_rows(pop_sizes, row0, n_local):
    """(local, total) rows per population for the shard [row0, row0 + n_local): population j is the
    global row block [N_1 + .. + N_{j-1}, N_1 + .. + N_j) (EM_W_multi.R:451-458, :537-541)."""
    sizes = np.asarray(pop_sizes, dtype=np.int64)
    ends = np.cumsum(sizes)
    begins = ends - sizes
    lo, hi = int(row0), int(row0) + int(n_local)
    local = np.clip(np.minimum(ends, hi) - np.maximum(begins, lo), 0, None).astype(np.int64)
    return np.ascontiguousarray(local), np.ascontiguousarray(sizes)


class Context:
    """One GPU, one HIP stream, resident X/Y (``ppls_ctx``)."""

    def __init__(self, device: int = 0):
        self._L = _lib.lib()
        h = ct.c_void_p()
        rc = self._L.ppls_ctx_create(int(device), ct.byref(h))
        if rc != 0:
            raise PplsError(rc, f"ppls_ctx_create(device={device}) failed: "
                                f"{self._L.ppls_strerror(rc).decode()} (is a GPU visible?)")
        self.h = h
        self.device = int(device)
        self.p = self.q = None
        self.n_local = self.n_total = None
        self.row0 = 0
        self._stream_folds = None     # K while the context is (being) streamed with folds
        self._reducer_fn = None       # the host reducer in place of RCCL (set_reducer)

    # -- plumbing
    def _chk(self, rc):
        if rc != 0:
            raise PplsError(rc, self._L.ppls_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self._L.ppls_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, key: str, value: int):
        self._chk(self._L.ppls_set_option(self.h, key.encode(), int(value)))

    # -- multi-GPU
    @staticmethod
    def shard_range(n_total, nranks, rank):
        L = _lib.lib()
        r0, nl = ct.c_int64(), ct.c_int64()
        L.ppls_shard_range(int(n_total), int(nranks), int(rank), ct.byref(r0), ct.byref(nl))
        return r0.value, nl.value

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = ct.create_string_buffer(128)
        rc = _lib.lib().ppls_comm_unique_id(buf)
        if rc != 0:
            raise PplsError(rc, "ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes):
        assert len(uid) == 128
        self._chk(self._L.ppls_comm_init(self.h, int(nranks), int(rank), uid))

    def set_reducer(self, fn):
        """Host-side reduction in place of RCCL (ppls_set_reducer): ``fn(buf)`` receives a float64
        numpy view of the buffer and must overwrite it in place with its sum over all ranks (e.g.
        ``torch.distributed.all_reduce`` on gloo).  ``None`` restores RCCL.  Collective when data
        is resident."""
        self._reducer_fn = fn
        if fn is None:
            self._reducer_cb = None
            self._chk(self._L.ppls_set_reducer(self.h, None, None))
            return

        def _cb(_user, buf, count):
            try:
                fn(np.ctypeslib.as_array(buf, shape=(int(count),)))
                return 0
            except Exception:   # noqa: BLE001 -- reported to the library as a reduction failure
                import traceback
                traceback.print_exc()
                return 1

        self._reducer_cb = _lib.REDUCE_FN(_cb)   # kept alive as long as the context
        self._chk(self._L.ppls_set_reducer(self.h, ct.cast(self._reducer_cb, ct.c_void_p), None))

    # -- data
    def set_data(self, X, Y, n_total=None):
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError("X and Y must be matrices with the same number of rows")
        if X.flags.f_contiguous and Y.flags.f_contiguous and not (X.flags.c_contiguous and Y.flags.c_contiguous):
            layout = _lib.PPLS_LAYOUT_COLMAJOR
        else:
            X = np.ascontiguousarray(X)
            Y = np.ascontiguousarray(Y)
            layout = _lib.PPLS_LAYOUT_ROWMAJOR
        n, p = X.shape
        q = Y.shape[1]
        nt = n if n_total is None else int(n_total)
        self._chk(self._L.ppls_set_data(self.h, dptr(X), dptr(Y), n, p, q, layout, nt))
        self.p, self.q, self.n_local, self.n_total = p, q, n, nt
        self._stream_folds = None

    def generate_synthetic(self, n_total, p, q, truth: Theta, seed: int, row0=0, n_local=None):
        nl = n_total - row0 if n_local is None else int(n_local)
        t = truth.struct()
        self._chk(self._L.ppls_generate_synthetic(self.h, int(n_total), int(row0), nl, int(p), int(q),
                                                  truth.r, ct.byref(t), ct.c_uint64(int(seed))))
        self.p, self.q, self.n_local, self.n_total, self.row0 = p, q, nl, int(n_total), int(row0)
        self._stream_folds = None

    def get_data(self, row_begin=0, nrows=None):
        nrows = self.n_local - row_begin if nrows is None else nrows
        X = np.zeros((nrows, self.p), order="F")
        Y = np.zeros((nrows, self.q), order="F")
        self._chk(self._L.ppls_get_data(self.h, dptr(X), dptr(Y), int(row_begin), int(nrows)))
        return X, Y

    def get_data_rows(self, row_begin=0, nrows=None):
        """Rows [row_begin, row_begin + nrows) of X, Y as C-ordered (row-major) float64 arrays."""
        nrows = self.n_local - row_begin if nrows is None else nrows
        X = np.empty((nrows, self.p))
        Y = np.empty((nrows, self.q))
        self._chk(self._L.ppls_get_data_rows(self.h, dptr(X), dptr(Y), int(row_begin), int(nrows)))
        return X, Y

    def philox4x32_10(self, ctr, key: int):
        """Device Philox4x32-10 block function (the generator's): ctr (count, 4) uint32 -> (count, 4)."""
        c = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
        out = np.empty_like(c)
        u32p = ct.POINTER(ct.c_uint32)
        self._chk(self._L.ppls_philox4x32_10(self.h, c.ctypes.data_as(u32p), c.shape[0], ct.c_uint64(int(key)),
                                             out.ctypes.data_as(u32p)))
        return out

    def ssq(self):
        a, b = ct.c_double(), ct.c_double()
        self._chk(self._L.ppls_data_ssq(self.h, ct.byref(a), ct.byref(b)))
        return a.value, b.value

    def scale_data(self, center=True, scale=True):
        """R's ``scale(X, center, scale)`` and ``scale(Y, center, scale)`` on the resident data, in
        place on the device (ppls_scale_data): column means and standard deviations over all
        ranks' rows.  Collective when the rows are sharded.  A column without spread under
        ``scale=True`` is an argument error and leaves the data untouched."""
        self._chk(self._L.ppls_scale_data(self.h, int(bool(center)), int(bool(scale))))

    def scaling(self):
        """The transform the resident data carry relative to what was loaded (ppls_get_scaling):
        ``loaded = resident * scale + center`` column-wise, as ``dict(centerX, scaleX, centerY,
        scaleY)`` -- R's ``attr(, "scaled:center")`` / ``"scaled:scale"`` after one ``scale_data``."""
        cen = np.zeros(self.p + self.q)
        scl = np.ones(self.p + self.q)
        self._chk(self._L.ppls_get_scaling(self.h, dptr(cen), dptr(scl)))
        return dict(centerX=cen[: self.p].copy(), scaleX=scl[: self.p].copy(),
                    centerY=cen[self.p:].copy(), scaleY=scl[self.p:].copy())

    def scale_timing(self):
        """The passes of the last ``scale_data`` (ppls_scale_timing): per pass (column sums, centred
        squares, apply) the ms between HIP events and the bytes moved on this rank."""
        ms, by = np.zeros(3), np.zeros(3)
        self._chk(self._L.ppls_scale_timing(self.h, dptr(ms), dptr(by)))
        return dict(ms=ms, bytes=by)

    # -- covariate adjustment
    @staticmethod
    def _design(Z, n):
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim == 1:
            Z = Z.reshape(-1, 1)
        if Z.ndim != 2 or Z.shape[0] != n:
            raise ValueError(f"Z must be a matrix with one row per local row ({n}), got shape {Z.shape}")
        return np.ascontiguousarray(Z)

    def adjust_data(self, Z, intercept=True):
        """R's ``resid(lm(cbind(X, Y) ~ Z))`` on the resident data, in place on the device
        (ppls_adjust_data): X and Y become their least-squares residuals on ``[1 Z]`` (or ``Z``) over all
        ranks' rows.  ``Z``: this rank's n_local x k covariate rows.  Collective when the rows are
        sharded.  An aliased or constant covariate is an argument error and leaves the data untouched;
        adjust before ``scale_data``."""
        Z = self._design(Z, self.n_local)
        self._chk(self._L.ppls_adjust_data(self.h, dptr(Z) if Z.size else None, Z.shape[1], _lib.PPLS_LAYOUT_ROWMAJOR,
                                           int(bool(intercept))))

    def adjustment(self):
        """The covariate part of the transform the data carry (ppls_get_adjustment):
        ``loaded = resident * scale + center + (z - zcenter) @ Gamma`` with ``scaling()``'s centre and
        scale, as ``dict(k, zcenter, coefX, coefY)`` (k x p and k x q, in the loaded units); k = 0 and
        empty arrays when the data are not adjusted."""
        k = ct.c_int()
        self._chk(self._L.ppls_get_adjustment(self.h, ct.byref(k), None, None))
        zc = np.zeros(k.value)
        G = np.zeros((k.value, self.p + self.q))
        if k.value:
            self._chk(self._L.ppls_get_adjustment(self.h, ct.byref(k), dptr(zc), dptr(G)))
        return dict(k=k.value, zcenter=zc, coefX=G[:, : self.p].copy(), coefY=G[:, self.p:].copy())

    def adjust_explained(self):
        """Per column of X, then of Y: the sum of squares the design explained in the last
        ``adjust_data`` (ppls_adjust_explained), sum_a G_aj^2."""
        ss = np.zeros(self.p + self.q)
        self._chk(self._L.ppls_adjust_explained(self.h, dptr(ss)))
        return ss

    def xprod_adjust(self, src: "Context", k, scale=False):
        """This context's cross-products := ``src``'s with its last ``k`` Y columns partialled out of
        the others (ppls_xprod_adjust): the Schur complement, for a ``src`` that holds S (streamed
        without folds, a resample / permute / weighted destination) or resident rows.  This context ends
        streamed (S, no rows) with shape p, q_src - k; ``scale=True`` standardises the result."""
        self._chk(self._L.ppls_xprod_adjust(self.h, src.h, int(k), int(bool(scale))))
        self.p, self.q, self.n_local, self.row0 = src.p, src.q - int(k), 0, 0
        self.n_total = self.stream_info()["n_total"]
        self._stream_folds = None

    def adjust_coef(self, Q):
        """Q'[X Y] over the resident rows by adjust_data's coefficient pass and its reduce alone
        (ppls_adjust_coef): ``Q`` is this rank's n_local x k1 rows; returns k1 x (p + q).  The data
        are not modified."""
        Q = self._design(Q, self.n_local)
        G = np.zeros((Q.shape[1], self.p + self.q))
        self._chk(self._L.ppls_adjust_coef(self.h, dptr(Q) if Q.size else None, Q.shape[1], dptr(G)))
        return G

    def adjust_info(self, k1):
        """The tile and launch shapes of the adjustment's row passes for ``k1`` design columns
        (ppls_adjust_info): ``dict(kt, X=dict(tx, ty, grid_x, grid_y, nblocks), Y=...)``."""
        kt = ct.c_int()
        pl = np.zeros(10, dtype=np.int64)
        self._chk(self._L.ppls_adjust_info(self.h, int(k1), ct.byref(kt), pl.ctypes.data_as(_lib._i64p)))
        names = ("tx", "ty", "grid_x", "grid_y", "nblocks")
        return dict(kt=kt.value, X=dict(zip(names, map(int, pl[:5]))), Y=dict(zip(names, map(int, pl[5:]))))

    def xadjust_matrix(self, S_src, p, ldx, q_src, ldy_src, k, ldy_dst, scale=False):
        """The Schur kernel of ``xprod_adjust`` alone on a host matrix in the joint padded layout
        (ppls_xadjust_matrix): returns the (ldx + ldy_dst)^2 result, padding included."""
        S = np.ascontiguousarray(S_src, dtype=np.float64)
        if S.shape != (ldx + ldy_src, ldx + ldy_src):
            raise ValueError("S_src must be (ldx + ldy_src) x (ldx + ldy_src)")
        out = np.full((ldx + ldy_dst, ldx + ldy_dst), np.nan)
        self._chk(self._L.ppls_xadjust_matrix(self.h, dptr(S), int(p), int(ldx), int(q_src), int(ldy_src), int(k),
                                              int(ldy_dst), int(bool(scale)), dptr(out)))
        return out

    def adjust_timing(self):
        """HIP-event ms of the last coefficient pass, apply pass, Schur pass and the standardise pass
        behind a scaled Schur pass (ppls_adjust_timing)."""
        ms = np.zeros(4)
        self._chk(self._L.ppls_adjust_timing(self.h, dptr(ms)))
        return dict(coef=ms[0], apply=ms[1], schur=ms[2], standardise=ms[3])

    # -- streamed data: S from row chunks, no rows resident
    def stream_begin(self, p, q, center=False, scale=False, nr_folds=None):
        """Open a stream of ``p + q`` columns (ppls_stream_begin): drops resident data and S.
        ``center`` / ``scale`` as in R's ``scale()``, applied to the streamed rows as a whole.
        ``nr_folds=K``: one cross-product matrix per fold is kept (ppls_stream_begin_folds), every
        chunk then comes with a fold label per row, and the streamed context can cross-validate."""
        if nr_folds is None:
            self._chk(self._L.ppls_stream_begin(self.h, int(p), int(q), int(bool(center)), int(bool(scale))))
        else:
            if int(nr_folds) < 2:
                raise ValueError("Cross-validation with 1 fold does not make sense, use 2 folds or more")
            self._chk(self._L.ppls_stream_begin_folds(self.h, int(p), int(q), int(bool(center)), int(bool(scale)),
                                                      int(nr_folds)))
        self.p, self.q, self.n_local, self.n_total, self.row0 = int(p), int(q), 0, 0, 0
        self._stream_folds = None if nr_folds is None else int(nr_folds)

    def stream_rows(self, X, Y, fold=None):
        """One chunk of rows (ppls_stream_rows): float64 matrices, C- or F-contiguous (both in the
        same order are passed without a copy).  Returns once the chunk is on the device.  ``fold``:
        the fold (0 .. K-1) of every row, for a stream opened with ``nr_folds=K``."""
        X, Y, layout = _chunk_arrays(X, Y, self.p, self.q)
        if fold is None:
            self._chk(self._L.ppls_stream_rows(self.h, dptr(X), dptr(Y), X.shape[0], layout))
            return
        fold = _fold_array(fold, X.shape[0], self._stream_folds)
        self._chk(self._L.ppls_stream_rows_folds(self.h, dptr(X), dptr(Y), X.shape[0], layout,
                                                 fold.ctypes.data_as(ct.POINTER(ct.c_int32))))

    def stream_rows_from(self, src: "Context", fold=None):
        """All resident rows of ``src`` as one chunk, device to device; ``src`` is left untouched.
        ``fold``: the fold of every resident row of ``src``, for a stream opened with folds."""
        if fold is None:
            self._chk(self._L.ppls_stream_rows_from(self.h, src.h))
            return
        fold = _fold_array(fold, src.n_local, self._stream_folds)
        self._chk(self._L.ppls_stream_rows_from_folds(self.h, src.h, fold.ctypes.data_as(ct.POINTER(ct.c_int32))))

    def stream_end(self):
        """Close the stream (ppls_stream_end; collective when sharded).  Returns ``dict(n, centerX,
        scaleX, centerY, scaleY)``: the rows over all ranks and the transform S carries; a stream
        with folds adds ``fold_total``, the rows per fold over all ranks."""
        try:
            self._chk(self._L.ppls_stream_end(self.h))
        except PplsError:
            self._stream_folds = None      # every error return drops the stream
            raise
        self.n_local, self.n_total = 0, self.stream_info()["n_total"]
        out = dict(n=self.n_total)
        out.update(self.scaling())
        info = self.stream_fold_info()
        if info["nr_folds"]:
            out["fold_total"] = info["fold_total"]
        return out

    def stream_fold_info(self):
        """``dict(nr_folds, fold_total, selected)`` (ppls_stream_fold_info): 0 folds for a context
        not streamed with folds; ``selected`` is the fold the working cross-products leave out."""
        K, sel = ct.c_int(), ct.c_int()
        self._chk(self._L.ppls_stream_fold_info(self.h, ct.byref(K), None, None))
        tot = np.zeros(K.value, dtype=np.int64)
        self._chk(self._L.ppls_stream_fold_info(self.h, ct.byref(K), tot.ctypes.data_as(_lib._i64p), ct.byref(sel)))
        return dict(nr_folds=K.value, fold_total=tot, selected=sel.value)

    def stream_select(self, fold=-1):
        """The working cross-products become the sum of all folds but ``fold`` (-1: all), with
        ``n_total`` and the sums of squares to match (ppls_stream_select): the fits then see the
        selected rows."""
        self._chk(self._L.ppls_stream_select(self.h, int(fold)))
        self.n_total = self.stream_info()["n_total"]

    def heldout_sse_fold(self, W, C, B, fold):
        """(sse, mag) of fold ``fold`` from its cross-products, for every prefix of the components
        (ppls_heldout_sse_fold): ``mag / sse`` tells how many digits of ``sse`` survive."""
        W, C, B = self._fit_arrays(W, C, B)
        if W.shape[0] != self.p or C.shape[0] != self.q:
            raise ValueError(f"the fit is {W.shape[0]} x {C.shape[0]}, the context's data {self.p} x {self.q}")
        sse, mag = np.zeros(W.shape[1]), np.zeros(W.shape[1])
        self._chk(self._L.ppls_heldout_sse_fold(self.h, dptr(W), dptr(C), dptr(B), W.shape[1], int(fold), dptr(sse),
                                                dptr(mag)))
        return sse, mag

    def stream_fold_get(self, fold, padded=False):
        """(S, mean, n) of one fold of a context streamed with folds (ppls_stream_fold_get), S and the
        mean over the p + q real columns unless ``padded``."""
        P, ldx = ct.c_int(), ct.c_int()
        self._chk(self._L.ppls_xprod_get(self.h, None, ct.byref(P), ct.byref(ldx)))
        S, mean, n = np.zeros((P.value, P.value)), np.zeros(P.value), ct.c_int64()
        self._chk(self._L.ppls_stream_fold_get(self.h, int(fold), dptr(S), dptr(mean), ct.byref(n)))
        if not padded:
            idx = np.r_[np.arange(self.p), ldx.value + np.arange(self.q)]
            S, mean = S[np.ix_(idx, idx)], mean[idx]
        return S, mean, n.value

    def cv_ppls_stream(self, a: int, max_steps: int, atol: float, inits, crit_abs=False):
        """cv_PPLS's loop on the folds of a context streamed with folds (ppls_cv_ppls_stream).
        ``inits`` as for ``cv_ppls``.  Returns (rmsep K x a, ncomp K, cond K x a = mag / sse)."""
        p, q = self.p, self.q
        K = self.stream_fold_info()["nr_folds"]
        if len(inits) != K or any(len(f) != a for f in inits):
            raise ValueError(f"starting values: one list of {a} per fold ({K} folds)")
        ths = [Theta(np.reshape(t["W"], (p, 1)), np.reshape(t["C"], (q, 1)), float(np.ravel(t["B"])[0]),
                     t["sigE"], t["sigF"], t["sigH"], float(np.ravel(t["sigT"])[0])) for f in inits for t in f]
        arr = (_lib.PplsTheta * (K * a))(*[t.struct() for t in ths])
        rmsep, cond = np.full((K, a), np.nan), np.full((K, a), np.nan)
        ncomp = np.zeros(K, dtype=np.int32)
        try:
            self._chk(self._L.ppls_cv_ppls_stream(self.h, int(a), int(max_steps), float(atol), int(bool(crit_abs)), arr,
                                                  dptr(rmsep), ncomp.ctypes.data_as(ct.POINTER(ct.c_int)), dptr(cond)))
        finally:
            self.n_total = self.stream_info()["n_total"]
        return rmsep, ncomp, cond

    def stream_info(self):
        st = ct.c_int()
        rows, nt, ch = ct.c_int64(), ct.c_int64(), ct.c_int64()
        self._chk(self._L.ppls_stream_info(self.h, ct.byref(st), ct.byref(rows), ct.byref(nt), ct.byref(ch)))
        return dict(state=("none", "open", "streamed")[st.value], rows_local=rows.value, n_total=nt.value,
                    chunks=ch.value)

    @property
    def streamed(self):
        """True when the context fits from streamed cross-products and holds no rows."""
        return self.stream_info()["state"] == "streamed"

    # -- hot path
    def estep(self, th: Theta, want_mu=True) -> Expect:
        e = Expect(th.r, self.n_local, want_mu)
        s = e.struct()
        t = th.struct()
        self._chk(self._L.ppls_estep(self.h, ct.byref(t), th.r, ct.byref(s)))
        e.pull(s)
        return e

    def mstep(self, fit: Expect, type_: int = _lib.PPLS_ORTH_SVD) -> Theta:
        out = Theta.empty(self.p, self.q, fit.r)
        s = fit.struct()
        o = out.struct()
        self._chk(self._L.ppls_mstep(self.h, ct.byref(s), fit.r, int(type_), ct.byref(o)))
        out.pull(o)
        return out

    def em_step(self, th: Theta, type_: int = _lib.PPLS_ORTH_SVD, want_fit=False):
        out = Theta.empty(self.p, self.q, th.r)
        fit = Expect(th.r, self.n_local, want_fit) if want_fit else None
        t, o = th.struct(), out.struct()
        fs = fit.struct() if fit is not None else None
        self._chk(self._L.ppls_em_step(self.h, ct.byref(t), th.r, int(type_), ct.byref(o),
                                       ct.byref(fs) if fs is not None else None))
        out.pull(o)
        if fit is not None:
            fit.pull(fs)
        return out, fit

    def loglik(self, th: Theta) -> float:
        out = ct.c_double()
        t = th.struct()
        self._chk(self._L.ppls_loglik(self.h, ct.byref(t), th.r, ct.byref(out)))
        return out.value

    def em_run(self, th: Theta, max_steps=10, atol=1e-4, type_=_lib.PPLS_ORTH_SVD, want_eout=True,
               want_mu=True):
        """PPLS_simult's loop from theta0 = th (copied); returns (estimates, loglik, eout, warn)."""
        est = Theta(th.W, th.C, th.B, th.sigE, th.sigF, th.sigH, th.sigT)
        ll = np.zeros(max_steps)
        steps = ct.c_int()
        neg = ct.c_int()
        eout = Expect(th.r, self.n_local, want_mu) if want_eout else None
        t = est.struct()
        es = eout.struct() if eout is not None else None
        self._chk(self._L.ppls_em_run(self.h, ct.byref(t), th.r, int(max_steps), float(atol), int(type_),
                                      dptr(ll), ct.byref(steps), ct.byref(neg),
                                      ct.byref(es) if es is not None else None))
        est.pull(t)
        if eout is not None:
            eout.pull(es)
        return est, ll[: steps.value].copy(), eout, bool(neg.value)

    def em_begin(self, th: Theta):
        t = th.struct()
        self._chk(self._L.ppls_em_begin(self.h, ct.byref(t), th.r))
        self._em_r = th.r

    def em_iterate(self, nsteps: int, type_: int = _lib.PPLS_ORTH_SVD):
        self._chk(self._L.ppls_em_iterate(self.h, int(nsteps), int(type_)))

    def em_state(self):
        out = Theta.empty(self.p, self.q, self._em_r)
        cap = 1 << 16
        ll = np.zeros(cap)
        n = ct.c_int()
        o = out.struct()
        self._chk(self._L.ppls_em_state(self.h, ct.byref(o), dptr(ll), cap, ct.byref(n)))
        out.pull(o)
        return out, ll[: n.value].copy()

    def ppls(self, a: int, max_steps: int, atol: float, inits, constraints=None, crit_abs=False):
        """Sequential PPLS fit (EM_W_multi.R:229-279) from a list of ``a`` rank-1 starting values
        (dicts W, C, B, sigE, sigF, sigH, sigT); ``constraints``: None or one fconstraint dict per
        component (fixed values, EM_W_multi.R:85-92); ``crit_abs``: critfunc = abs.  Returns the
        reference's list (W, C, B, sig, Other_output) plus the per-component logvalue traces."""
        p, q = self.p, self.q
        ths = [Theta(np.reshape(t["W"], (p, 1)), np.reshape(t["C"], (q, 1)), float(np.ravel(t["B"])[0]),
                     t["sigE"], t["sigF"], t["sigH"], float(np.ravel(t["sigT"])[0])) for t in inits]
        if len(ths) != a:
            raise ValueError(f"{len(ths)} starting values for nr_comp = {a}")
        arr = (_lib.PplsTheta * a)(*[t.struct() for t in ths])
        return self._seq_fit(a, max_steps, atol, arr, constraints, crit_abs)

    def ppls_o2m(self, a: int, max_steps: int, atol: float, constraints=None, crit_abs=False):
        """``ppls`` with ``initialGuess="o2m_xprod"`` (ppls_ppls_o2m): component k starts from the o2m
        values of the data deflated by the fitted components 1 .. k-1, read off the context's
        cross-products S on the device, and every component is fitted once.  Works wherever S is all
        there is (streamed, a fold selection, a resample destination); a resident context forms S and
        keeps it, as after ``xprod_prepare``.  Returns ``ppls``'s dict."""
        if self.p is None:   # no data: the library says so
            self._chk(self._L.ppls_ppls_o2m(self.h, int(a), int(max_steps), float(atol), 0, None, None))
        return self._seq_fit(a, max_steps, atol, None, constraints, crit_abs)

    def _seq_fit(self, a, max_steps, atol, arr, constraints, crit_abs):
        """ppls_ppls_ex from the starting values ``arr``, or ppls_ppls_o2m (``arr`` None)."""
        p, q = self.p, self.q
        W = np.zeros((p, a), order="F")
        C = np.zeros((q, a), order="F")
        B = np.zeros(a)
        sig = np.zeros((a, 4), order="F")
        lv = np.full((a, max_steps + 1), np.nan)
        last = np.zeros(a)
        nst = np.zeros(a, dtype=np.int32)
        lls = np.zeros(a)
        fit = _lib.PplsSeqFit(dptr(W), dptr(C), dptr(B), dptr(sig), dptr(lv), dptr(last),
                              nst.ctypes.data_as(ct.POINTER(ct.c_int)), dptr(lls), 0, 0)
        cons = None
        keep = []
        if constraints is not None:
            if len(constraints) != a:
                raise ValueError("There should be a list of constraints for each component, see ?PPLS.")
            cons = (_lib.PplsConstraint * a)()
            for k, cdict in enumerate(constraints):
                for key, size in (("W", p), ("C", q), ("B", 1), ("sigE", 1), ("sigF", 1), ("sigH", 1), ("sigT", 1)):
                    v = (cdict or {}).get(key)
                    if v is None:
                        continue
                    arrv = np.ascontiguousarray(np.ravel(np.asarray(v, dtype=np.float64)))
                    if arrv.shape[0] != size:
                        raise ValueError(f"constraint {key} of component {k + 1} has {arrv.shape[0]} values, not {size}")
                    keep.append(arrv)
                    setattr(cons[k], key, dptr(arrv))
        if arr is None:
            self._chk(self._L.ppls_ppls_o2m(self.h, int(a), int(max_steps), float(atol), int(bool(crit_abs)), cons,
                                            ct.byref(fit)))
        else:
            self._chk(self._L.ppls_ppls_ex(self.h, int(a), int(max_steps), float(atol), int(bool(crit_abs)), arr,
                                           cons, ct.byref(fit)))
        del keep
        k = fit.ncomp
        return dict(W=W[:, :k].copy(), C=C[:, :k].copy(), B=B[:k].copy(), sig=sig[:k].copy(),
                    Other_output=dict(Last_increment=last[:k].copy(), Number_steps=nst[:k].copy(),
                                      Loglikelihoods=lls[:k].copy(),
                                      logvalue=[lv[i, :nst[i] + 1].copy() for i in range(k)]),
                    not_monotone=[bool(fit.not_monotone >> i & 1) for i in range(k)], ncomp=k)

    def pop_rows(self, pop_sizes):
        return pop_rows(pop_sizes, self.row0, self.n_local)

    def meta_emstep(self, W, C, pop_sizes, params):
        """meta_EMstep (EM_W_multi.R:446-485) on the resident rows: per-population E- and M-step
        (meta_Estep / meta_Mstep, src/loglC.cpp:399-474) and the shared W., C.  params: npop x 5
        (B_T, sigX, sigY, sigH, sigT).  Returns (W, C, params_out, Cxt p x npop, Cyu q x npop)."""
        loc, tot = self.pop_rows(pop_sizes)
        npop = len(tot)
        W = np.ascontiguousarray(np.ravel(W), dtype=np.float64)
        C = np.ascontiguousarray(np.ravel(C), dtype=np.float64)
        pin = np.asfortranarray(np.asarray(params, dtype=np.float64).reshape(npop, 5))
        Wo, Co = np.zeros(self.p), np.zeros(self.q)
        po = np.zeros((npop, 5), order="F")
        cxt, cyu = np.zeros((self.p, npop), order="F"), np.zeros((self.q, npop), order="F")
        i64 = ct.POINTER(ct.c_int64)
        self._chk(self._L.ppls_meta_emstep(self.h, npop, loc.ctypes.data_as(i64), tot.ctypes.data_as(i64),
                                           dptr(W), dptr(C), dptr(pin), dptr(Wo), dptr(Co), dptr(po),
                                           dptr(cxt), dptr(cyu)))
        return Wo, Co, po, cxt, cyu

    def meta_ppls(self, pop_sizes, max_steps, atol, init, crit_abs=False):
        """meta_PPLSi's loop (EM_W_multi.R:544-578) from the starting values ``init`` (dict W, C, B,
        sigE, sigF, sigH, sigT, r = 1).  Returns (W, C, params npop x 5, logvalue (steps+1) x npop)."""
        loc, tot = self.pop_rows(pop_sizes)
        npop = len(tot)
        th = Theta(np.reshape(init["W"], (self.p, 1)), np.reshape(init["C"], (self.q, 1)),
                   float(np.ravel(init["B"])[0]), init["sigE"], init["sigF"], init["sigH"],
                   float(np.ravel(init["sigT"])[0]))
        t = th.struct()
        Wo, Co = np.zeros(self.p), np.zeros(self.q)
        po = np.zeros((npop, 5), order="F")
        lg = np.full((max_steps + 1, npop), np.nan, order="F")
        fit = _lib.PplsMetaFit(dptr(Wo), dptr(Co), dptr(po), dptr(lg), 0)
        i64 = ct.POINTER(ct.c_int64)
        self._chk(self._L.ppls_meta_ppls(self.h, npop, loc.ctypes.data_as(i64), tot.ctypes.data_as(i64),
                                         int(max_steps), float(atol), int(bool(crit_abs)), ct.byref(t),
                                         ct.byref(fit)))
        return Wo, Co, po, lg[: fit.steps + 1].copy()

    def meta_emstep_stream(self, W, C, params):
        """meta_EMstep on a context streamed with folds (ppls_meta_emstep_stream): the fold labels are
        the populations, every statistic comes from the fold's cross-products.  params: K x 5.
        Returns what ``meta_emstep`` returns."""
        held = self.stream_fold_info()["nr_folds"]
        W = np.ascontiguousarray(np.ravel(W), dtype=np.float64)
        C = np.ascontiguousarray(np.ravel(C), dtype=np.float64)
        pin = np.asfortranarray(np.asarray(params, dtype=np.float64).reshape(-1, 5))
        npop = pin.shape[0]
        if held and npop != held:      # (no fold stream: the call itself refuses, before it reads params)
            raise ValueError(f"{npop} parameter sets for {held} populations")
        Wo, Co = np.zeros(self.p), np.zeros(self.q)
        po = np.zeros((npop, 5), order="F")
        cxt, cyu = np.zeros((self.p, npop), order="F"), np.zeros((self.q, npop), order="F")
        self._chk(self._L.ppls_meta_emstep_stream(self.h, dptr(W), dptr(C), dptr(pin), dptr(Wo), dptr(Co), dptr(po),
                                                  dptr(cxt), dptr(cyu)))
        return Wo, Co, po, cxt, cyu

    def meta_ppls_stream(self, max_steps, atol, init, crit_abs=False):
        """meta_PPLSi's loop on a context streamed with folds (ppls_meta_ppls_stream), the whole loop
        on the device from the folds' cross-products.  Returns what ``meta_ppls`` returns."""
        npop = max(self.stream_fold_info()["nr_folds"], 1)
        th = Theta(np.reshape(init["W"], (self.p, 1)), np.reshape(init["C"], (self.q, 1)),
                   float(np.ravel(init["B"])[0]), init["sigE"], init["sigF"], init["sigH"],
                   float(np.ravel(init["sigT"])[0]))
        t = th.struct()
        Wo, Co = np.zeros(self.p), np.zeros(self.q)
        po = np.zeros((npop, 5), order="F")
        lg = np.full((max_steps + 1, npop), np.nan, order="F")
        fit = _lib.PplsMetaFit(dptr(Wo), dptr(Co), dptr(po), dptr(lg), 0)
        self._chk(self._L.ppls_meta_ppls_stream(self.h, int(max_steps), float(atol), int(bool(crit_abs)), ct.byref(t),
                                                ct.byref(fit)))
        return Wo, Co, po, lg[: fit.steps + 1].copy()

    def meta_xprod_info(self):
        """``dict(npop, formations, form_ms)`` (ppls_meta_xprod_info): the population cross-products
        option "meta_xprod" keeps on this context, how often they were formed so far, and the wall
        clock of the last formation."""
        k, n, ms = ct.c_int(), ct.c_int64(), ct.c_double()
        self._chk(self._L.ppls_meta_xprod_info(self.h, ct.byref(k), ct.byref(n), ct.byref(ms)))
        return dict(npop=k.value, formations=n.value, form_ms=ms.value)

    def xprod_meta_timing(self, reps=200):
        """Average ms of the meta statistics pass over the population matrices the context holds
        (ppls_xprod_meta_timing: HIP events around ``reps`` back-to-back passes)."""
        ms = ct.c_double()
        self._chk(self._L.ppls_xprod_meta_timing(self.h, int(reps), ct.byref(ms)))
        return ms.value

    def xprod_meta_stats(self, W, C, params):
        """The statistics pass of one meta EM step alone (ppls_xprod_meta_stats) on a context that
        holds population matrices (streamed with folds, or resident after a "meta_xprod" = 1 call):
        ``(SX K x p, SY K x q, G K x 2 x 2)`` for the shared loadings and params (K x 5)."""
        params = np.asarray(params, dtype=np.float64)
        K = params.shape[0]
        W = np.ascontiguousarray(np.ravel(W), dtype=np.float64)
        C = np.ascontiguousarray(np.ravel(C), dtype=np.float64)
        if W.shape[0] != self.p or C.shape[0] != self.q or params.shape != (K, 5):
            raise ValueError("W (p), C (q) and params (K x 5) are needed")
        held = self.stream_fold_info()["nr_folds"] or self.meta_xprod_info()["npop"]
        if held and K != held:
            raise ValueError(f"{K} parameter sets for {held} populations")
        pin = np.asfortranarray(params)
        st = np.zeros((K, self.p + self.q + 4))
        self._chk(self._L.ppls_xprod_meta_stats(self.h, dptr(W), dptr(C), dptr(pin), dptr(st)))
        return (st[:, :self.p].copy(), st[:, self.p:self.p + self.q].copy(),
                st[:, self.p + self.q:].reshape(K, 2, 2).copy())

    def variances(self, mu, Cdiag, sigE, xory, full=True):
        """variances.PPLS_simult (EM_W_multi.R:830-860) on the resident X (xory 0) or Y (xory 1):
        mu = this rank's rows of Expectations$mu_T / mu_U (n_local x a), Cdiag = diag(Ctt / Cuu).
        Returns (W, B_exp scalars, varMatrix a x p x p, seLoad p x a, SSt_exp, SSt_star) -- the
        last two (a x p x p) only with full=True."""
        # no copy when mu is already a column-major float64 n_local x a array (the fits' Expectations are)
        mu = np.asarray(mu, dtype=np.float64)
        if mu.ndim != 2 or mu.shape[0] != self.n_local:   # (a 0 x a matrix cannot be reshaped with -1)
            mu = mu.reshape(self.n_local, -1)
        mu = np.asfortranarray(mu)
        a = mu.shape[1]
        p = self.q if xory else self.p
        Cd = np.ascontiguousarray(np.ravel(Cdiag), dtype=np.float64)
        if Cd.shape[0] != a:
            raise ValueError(f"{Cd.shape[0]} variances for {a} components")
        W = np.zeros((p, a), order="F")
        Bx = np.zeros(a)
        V = np.zeros((a, p, p))            # component i: V[i] holds the column-major p x p as its transpose
        se = np.zeros((p, a), order="F")
        SE = np.zeros((a, p, p)) if full else None
        SS = np.zeros((a, p, p)) if full else None
        self._chk(self._L.ppls_variances(self.h, dptr(mu), dptr(Cd), float(sigE), int(a), int(xory), dptr(W),
                                         dptr(Bx), dptr(V), dptr(SE), dptr(SS), dptr(se)))
        # buffers hold consecutive column-major matrices: each is returned as its transposed view (no
        # copy -- a contiguous transpose of a x p x p doubles cost ~30 ms of host time at C3)
        tr = (lambda A: None if A is None else np.transpose(A, (0, 2, 1)))
        return W, Bx, tr(V), se, tr(SE), tr(SS)

    def variances_xprod(self, th: Theta, xory, full=True, want_var=True):
        """variances.PPLS_simult (EM_W_multi.R:830-860) from the cross-products S alone
        (ppls_variances_xprod): ``th`` is the theta at which the reference's Expectations are taken.
        Works on every context that holds S -- streamed, a fold stream's current selection, the
        destination of ``xprod_resample``, resident (S is formed and kept if it is not there).
        Returns (W, Cdiag, B_exp scalars, varMatrix a x p x p, seLoad p x a, SSt_exp, SSt_star):
        Cdiag = the Ctt_ii (xory 0) or Cuu_ii (xory 1) used; varMatrix only with want_var, the last
        two only with full (else None)."""
        a = th.r
        p = self.q if xory else self.p
        if p is None:
            p = 1          # no data: the library refuses before it writes
        elif th.W.shape[0] != self.p or th.C.shape[0] != self.q:
            raise ValueError(f"theta is {th.W.shape[0]} x {th.C.shape[0]}, the context's data {self.p} x {self.q}")
        W = np.zeros((p, a), order="F")
        Cd = np.zeros(a)
        Bx = np.zeros(a)
        se = np.zeros((p, a), order="F")
        V = np.zeros((a, p, p)) if want_var else None   # component i: the column-major p x p as its transpose
        SE = np.zeros((a, p, p)) if full else None
        SS = np.zeros((a, p, p)) if full else None
        s = th.struct()
        self._chk(self._L.ppls_variances_xprod(self.h, ct.byref(s), int(a), int(xory), dptr(W), dptr(Cd), dptr(Bx),
                                               dptr(V), dptr(SE), dptr(SS), dptr(se)))
        tr = (lambda A: None if A is None else np.transpose(A, (0, 2, 1)))
        return W, Cd, Bx, tr(V), se, tr(SE), tr(SS)

    def varinfo(self, S, off, p, cxt, w, ctt, k1, k2, bstar, sigE, N, full=True):
        """ppls_variances_xprod's information kernel alone on host inputs (ppls_varinfo): S (P x P), the
        p x p block at (off, off), cxt and w (p x a), the scalars ctt, k1, k2, bstar (a each) ->
        (J, SSt_exp, SSt_star), a x p x p each as stored (column-major per matrix: entry [i, b, a] is
        element (a, b)); the last two None without ``full``."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        P = S.shape[0]
        cxt = np.asfortranarray(np.asarray(cxt, dtype=np.float64).reshape(p, -1))
        w = np.asfortranarray(np.asarray(w, dtype=np.float64).reshape(p, -1))
        a = cxt.shape[1]
        sc = [np.ascontiguousarray(np.ravel(v), dtype=np.float64) for v in (ctt, k1, k2, bstar)]
        if S.shape != (P, P) or w.shape != (p, a) or any(v.shape[0] != a for v in sc):
            raise ValueError("varinfo: inconsistent shapes")
        J = np.zeros((a, p, p))
        SE = np.zeros((a, p, p)) if full else None
        SS = np.zeros((a, p, p)) if full else None
        self._chk(self._L.ppls_varinfo(self.h, dptr(S), int(P), int(off), int(p), int(a), dptr(cxt), dptr(w), dptr(sc[0]),
                                       dptr(sc[1]), dptr(sc[2]), dptr(sc[3]), float(sigE), float(N), dptr(J), dptr(SE),
                                       dptr(SS)))
        return J, SE, SS

    def varinfo_timing(self, xory, a, reps=5):
        """(ms of the information kernel, ms of the launches it replaces: block copy, ``a`` varmat
        kernels, batch copy, negate), HIP events, averages over ``reps`` (ppls_varinfo_timing); after a
        ``variances_xprod`` call with ``a`` components, whose statistics and loadings it reads; it runs with
        every scalar set to 1 (times do not depend on the values) and returns no matrix."""
        new, old = ct.c_double(), ct.c_double()
        self._chk(self._L.ppls_varinfo_timing(self.h, int(xory), int(a), int(reps), ct.byref(new), ct.byref(old)))
        return new.value, old.value

    def gram(self, xory=0, nsplit=0, want=True, count=None, weight=None):
        """D'D (D = X, Y, or xory = 2 the joint [X Y], (p + q) x (p + q)) on the fp64 MFMA Gram kernel
        alone, this rank's rows -> (G or None, kernel ms).  ``count`` (one integer >= 0 per local row):
        the weighted instantiation instead, sum_i count_i d_i d_i' (ppls_gram_weighted).  ``weight`` (one
        finite real >= 0 per local row): the real-weighted one, sum_i weight_i d_i d_i'
        (ppls_gram_weighted_real).  Giving both is an error."""
        if count is not None and weight is not None:
            raise ValueError("gram: give count or weight, not both")
        p = self.p + self.q if xory == 2 else self.q if xory else self.p
        G = np.zeros((p, p), order="F") if want else None
        ms = ct.c_double()
        if weight is not None:
            w = self._weights(weight, self.n_local)
            self._chk(self._L.ppls_gram_weighted_real(self.h, int(xory), int(nsplit), dptr(w), dptr(G), ct.byref(ms)))
        elif count is None:
            self._chk(self._L.ppls_gram(self.h, int(xory), int(nsplit), dptr(G), ct.byref(ms)))
        else:
            cnt, cp = self._counts(count, self.n_local)
            self._chk(self._L.ppls_gram_weighted(self.h, int(xory), int(nsplit), cp, dptr(G), ct.byref(ms)))
        return G, ms.value

    def gram_occupancy(self, f32=False, weighted=False):
        """Workgroups of the MFMA Gram kernel per compute unit, for fp64 or fp32 storage: the
        unweighted instantiation (it sizes the grid and the split plan), the count-weighted one
        (``weighted=True``) or the real-weighted one (``weighted="real"``)."""
        fn = (self._L.ppls_gram_occupancy_real if weighted == "real" else
              self._L.ppls_gram_occupancy_weighted if weighted else self._L.ppls_gram_occupancy)
        return int(fn(int(bool(f32))))

    def gram_int8(self, which=2, want=True):
        """The Gram by the int8-MFMA Chinese-remainder form alone (which: 0 X'X, 1 Y'Y, 2 the joint
        [X Y]'[X Y] over the padded columns) -> (G or None, dict(nmod, L, ms = [stats + residues, SYRK,
        CRT, total], shift = the per-column scalings))."""
        P = self.p if which == 0 else self.q if which == 1 else int(round(np.sqrt(self.xprod_info()["bytes_per_pass"] / 8)))
        G = np.zeros((P, P), order="F") if want else None
        nm, L, ms = ct.c_int(), ct.c_int(), np.zeros(4)
        self._chk(self._L.ppls_gram_int8(self.h, int(which), dptr(G), ct.byref(nm), ct.byref(L), dptr(ms)))
        return G, dict(nmod=nm.value, L=L.value, ms=ms.tolist(), shift=self.gram_shifts())

    def gram_shifts(self):
        """The last int8 Gram's per-column scalings: x'_kj = rint(D_kj 2^shift[j]) (int array)."""
        k = ct.c_int()
        self._chk(self._L.ppls_gram_shifts(self.h, None, 0, ct.byref(k)))
        out = (ct.c_int * max(k.value, 1))()
        self._chk(self._L.ppls_gram_shifts(self.h, out, k.value, ct.byref(k)))
        return np.array(out[:k.value], dtype=np.int64)

    def gram_info(self):
        """Which Gram ran last (forming S, or variances' X'X / Y'Y): dict(int8 (bool), nmod, L, ms =
        [stats + residues, SYRK, CRT, total])."""
        u, nm, L, ms = ct.c_int(), ct.c_int(), ct.c_int(), np.zeros(4)
        self._chk(self._L.ppls_gram_info(self.h, ct.byref(u), ct.byref(nm), ct.byref(L), dptr(ms)))
        return dict(int8=bool(u.value), nmod=nm.value, L=L.value, ms=ms.tolist())

    def spd_inverse(self, A, method=1):
        """Inverses of symmetric positive definite matrices A (a x p x p or p x p) on the device as
        variances.PPLS_simult computes them (method 1 hand-written blocked Cholesky, 2 rocSOLVER)
        -> (inverses, info per matrix: 0 or the 1-based column of the first bad pivot, device ms)."""
        A = np.asarray(A, dtype=np.float64)
        one = A.ndim == 2
        A3 = A[None] if one else A
        a, p = A3.shape[0], A3.shape[1]
        Af = np.ascontiguousarray(np.transpose(A3, (0, 2, 1)))   # column-major per matrix
        out = np.empty_like(Af)
        info = (ct.c_int * a)()
        ms = ct.c_double()
        self._chk(self._L.ppls_spd_inverse(self.h, dptr(Af), int(p), int(a), int(method), dptr(out), info,
                                            ct.byref(ms)))
        inv = np.transpose(out, (0, 2, 1))
        return (inv[0] if one else inv), np.array(list(info)), ms.value

    def xprod_prepare(self):
        """Form the cross-products S = [X Y]'[X Y] now (option "xprod") -> (Gram kernel ms, total ms);
        (0, 0) when S is already formed for the current data."""
        ms, tot = ct.c_double(), ct.c_double()
        self._chk(self._L.ppls_xprod_prepare(self.h, ct.byref(ms), ct.byref(tot)))
        return ms.value, tot.value

    def xprod_release(self):
        """Free the cross-products S now (ppls_xprod_release; 8 (p+q)^2 bytes of HBM); the next run
        that reads S forms it again."""
        self._chk(self._L.ppls_xprod_release(self.h))
        self._stream_folds = None

    def o2m_start(self, Wprev=None, Cprev=None):
        """PPLSi's 'o2m' starting values (EM_W_multi.R:126-131) for the data deflated by the loadings
        ``Wprev`` (p x k), ``Cprev`` (q x k), from the context's cross-products S (ppls_o2m_start): the
        starting-value dict (W, C, B, sigE, sigF, sigH, sigT).  The entry of W of largest magnitude is
        positive and C follows."""
        if self.p is None:   # no data: the library says so
            self._chk(self._L.ppls_o2m_start(self.h, None, None, 0, None))
        p, q = self.p, self.q
        Wp = np.zeros((p, 0)) if Wprev is None else np.asarray(Wprev, dtype=np.float64).reshape(p, -1)
        Cp = np.zeros((q, 0)) if Cprev is None else np.asarray(Cprev, dtype=np.float64).reshape(q, -1)
        if Wp.shape[1] != Cp.shape[1]:
            raise ValueError(f"{Wp.shape[1]} earlier W loadings but {Cp.shape[1]} C loadings")
        k = Wp.shape[1]
        Wp, Cp = np.asfortranarray(Wp), np.asfortranarray(Cp)
        th = Theta.empty(p, q, 1)
        s = th.struct()
        self._chk(self._L.ppls_o2m_start(self.h, dptr(Wp) if k else None, dptr(Cp) if k else None, int(k), ct.byref(s)))
        th.pull(s)
        return dict(W=th.W[:, 0].copy(), C=th.C[:, 0].copy(), B=float(th.B[0]), sigE=th.sigE, sigF=th.sigF,
                    sigH=th.sigH, sigT=float(th.sigT[0]))

    def o2m_pass(self, S, row0, col0, rows, L, v, d=None):
        """The 'o2m_xprod' pass alone (ppls_o2m_pass) on a host matrix ``S`` (row-major, an even row
        length): for the ``rows x L`` block A at (row0, col0), ``u = A v - d`` and ``z = A'u``.
        Returns (u, z, path): path 1 fused, 2 two-phase (option "o2m_path")."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        v = np.ascontiguousarray(np.ravel(v), dtype=np.float64)
        dd = None if d is None else np.ascontiguousarray(np.ravel(d), dtype=np.float64)
        if v.shape[0] != L or (dd is not None and dd.shape[0] != rows):
            raise ValueError("v has L values and d has one per row")
        u, z = np.zeros(int(rows)), np.zeros(int(L))
        path = ct.c_int()
        self._chk(self._L.ppls_o2m_pass(self.h, dptr(S), int(S.shape[0]), int(S.shape[1]), int(row0), int(col0),
                                        int(rows), int(L), dptr(v), dptr(dd), dptr(u), dptr(z), ct.byref(path)))
        return u, z, path.value

    def o2m_info(self):
        """The last 'o2m_xprod' start (ppls_o2m_info): side (0: the block's rows are X's columns),
        path of its passes, Lanczos passes, residual estimate, theta = sigma_1^2, and the rank-1
        device fits of the last ``ppls_o2m``."""
        side, path, passes, fits = ct.c_int(), ct.c_int(), ct.c_int(), ct.c_int()
        resid, theta = ct.c_double(), ct.c_double()
        self._chk(self._L.ppls_o2m_info(self.h, ct.byref(side), ct.byref(path), ct.byref(passes), ct.byref(resid),
                                        ct.byref(theta), ct.byref(fits)))
        return dict(side=side.value, path=path.value, passes=passes.value, resid=resid.value, theta=theta.value,
                    fits=fits.value)

    def o2m_pass_timing(self, reps=50):
        """Average ms of the 'o2m_xprod' pass over reps back-to-back launches on the context's S
        (HIP events around the batch, after one untimed pass) -> dict(ms, bytes, path)."""
        ms, nbytes = ct.c_double(), ct.c_double()
        path = ct.c_int()
        self._chk(self._L.ppls_o2m_pass_timing(self.h, int(reps), ct.byref(ms), ct.byref(nbytes), ct.byref(path)))
        return dict(ms=ms.value, bytes=nbytes.value, path=path.value)

    def cv_ppls_o2m(self, a: int, fold_of_row, fold_total, max_steps: int, atol: float, crit_abs=False):
        """``cv_ppls`` with ``initialGuess="o2m_xprod"`` (ppls_cv_ppls_o2m): no starting values."""
        fold_of_row = np.ascontiguousarray(np.ravel(np.asarray(fold_of_row, dtype=np.int32)))
        fold_total = np.ascontiguousarray(np.ravel(np.asarray(fold_total, dtype=np.int64)))
        K = fold_total.shape[0]
        if fold_of_row.shape[0] != self.n_local:
            raise ValueError(f"{fold_of_row.shape[0]} fold labels for {self.n_local} local rows")
        rmsep = np.full((K, a), np.nan)
        ncomp = np.zeros(K, dtype=np.int32)
        self._chk(self._L.ppls_cv_ppls_o2m(self.h, int(a), int(K), fold_of_row.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                           fold_total.ctypes.data_as(_lib._i64p), int(max_steps), float(atol),
                                           int(bool(crit_abs)), dptr(rmsep), ncomp.ctypes.data_as(ct.POINTER(ct.c_int))))
        return rmsep, ncomp

    def cv_ppls_stream_o2m(self, a: int, max_steps: int, atol: float, crit_abs=False):
        """``cv_ppls_stream`` with ``initialGuess="o2m_xprod"`` (ppls_cv_ppls_stream_o2m)."""
        K = self.stream_fold_info()["nr_folds"]
        rmsep, cond = np.full((K, a), np.nan), np.full((K, a), np.nan)
        ncomp = np.zeros(K, dtype=np.int32)
        try:
            self._chk(self._L.ppls_cv_ppls_stream_o2m(self.h, int(a), int(max_steps), float(atol), int(bool(crit_abs)),
                                                      dptr(rmsep), ncomp.ctypes.data_as(ct.POINTER(ct.c_int)), dptr(cond)))
        finally:
            self.n_total = self.stream_info()["n_total"]
        return rmsep, ncomp, cond

    def xprod_matrix(self, padded=False):
        """The cross-products S the context holds (formed, prepared, downdated or streamed):
        ``(p + q) x (p + q)``, or with ``padded=True`` ``(S, ldx)`` -- the P x P matrix in the padded
        layout (X's columns at [0, p), Y's at [ldx, ldx + q), zeros elsewhere)."""
        P, ldx = ct.c_int(), ct.c_int()
        self._chk(self._L.ppls_xprod_get(self.h, None, ct.byref(P), ct.byref(ldx)))
        S = np.zeros((P.value, P.value))
        self._chk(self._L.ppls_xprod_get(self.h, dptr(S), ct.byref(P), ct.byref(ldx)))
        if padded:
            return S, ldx.value
        live = np.r_[np.arange(self.p), ldx.value + np.arange(self.q)]
        return S[np.ix_(live, live)]

    def xprod_tile_timing(self, reps=200):
        """Average ms of the cross-product tile kernel over reps back-to-back launches (HIP events
        around the batch) for the current em_begin session's theta."""
        ms = ct.c_double()
        self._chk(self._L.ppls_xprod_tile_timing(self.h, int(reps), ct.byref(ms)))
        return ms.value

    def xprod_setup_times(self):
        """(Gram kernel ms, all-reduce of S ms, whole setup ms) of the last formation of S."""
        g, a, t = ct.c_double(), ct.c_double(), ct.c_double()
        self._chk(self._L.ppls_xprod_setup_times(self.h, ct.byref(g), ct.byref(a), ct.byref(t)))
        return g.value, a.value, t.value

    def xprod_stats(self, th: Theta):
        """One statistics step from S for theta: (X'mu_T p x r, Y'mu_U q x r, Gram 2r x 2r)."""
        r = th.r
        out = np.zeros(r * (self.p + self.q) + 4 * r * r)
        t = th.struct()
        self._chk(self._L.ppls_xprod_stats(self.h, ct.byref(t), r, dptr(out)))
        SX = out[: self.p * r].reshape(r, self.p).T
        SY = out[self.p * r: (self.p + self.q) * r].reshape(r, self.q).T
        G = out[(self.p + self.q) * r:].reshape(2 * r, 2 * r).T
        return SX, SY, G

    def xprod_pass(self, W, C, coef, S=None, rw=0, with_gram=True, stop=False):
        """The cross-product statistics pass alone (``ppls_xprod_pass``): W (ldx x r) and C (ldy x r) with
        their padding rows, coef = (alpha, beta, gamma, delta) of r values each, on a host S (row-major
        P x P, X block ldx wide) or, S = None, on the context's own.  Returns a dict: M (P x 2r), SX
        (ldx x r), SY (ldy x r) and G (2r x 2r) as the kernels left them (NaN where nothing was written),
        rw and nt (the rows per wave and the instantiation that ran: 1 non-temporal, 0 cached)."""
        W = np.asfortranarray(np.array(W, dtype=np.float64, ndmin=2))
        C = np.asfortranarray(np.array(C, dtype=np.float64, ndmin=2))
        r = W.shape[1]
        if C.shape[1] != r:
            raise ValueError("W and C need the same number of components")
        ldx, ldy = W.shape[0], C.shape[0]
        P = ldx + ldy
        cf = [np.ascontiguousarray(np.ravel(v), dtype=np.float64) for v in coef]
        if len(cf) != 4 or any(v.size != r for v in cf):
            raise ValueError("coef must be (alpha, beta, gamma, delta) of r values each")
        if S is not None:
            S = np.ascontiguousarray(S, dtype=np.float64)
            if S.shape != (P, P):
                raise ValueError(f"S must be {P} x {P}")
        M, st = np.zeros((P, 2 * r), order="F"), np.zeros(P * r + 4 * r * r)
        rwu, ntu = ct.c_int(), ct.c_int()
        self._chk(self._L.ppls_xprod_pass(self.h, dptr(S), P, ldx, dptr(W), dptr(C), dptr(cf[0]), dptr(cf[1]), dptr(cf[2]),
                                          dptr(cf[3]), r, int(rw), int(bool(with_gram)), int(bool(stop)), dptr(M), dptr(st),
                                          ct.byref(rwu), ct.byref(ntu)))
        return dict(M=M, SX=st[:ldx * r].reshape(ldx, r, order="F").copy(),
                    SY=st[ldx * r:P * r].reshape(ldy, r, order="F").copy(),
                    G=st[P * r:].reshape(2 * r, 2 * r, order="F").copy(), rw=rwu.value, nt=ntu.value)

    def sweep_stats(self, th: Theta, want_mu=False):
        """One statistics step by the sweep for theta (the kernel ``sweep_kernel(r)`` names, under the
        current options): (X'mu_T p x r, Y'mu_U q x r, Gram 2r x 2r, mu), mu = this rank's
        n_local x 2r [mu_T | mu_U] when want_mu, else None."""
        r = th.r
        out = np.zeros(r * (self.p + self.q) + 4 * r * r)
        mu = np.zeros((self.n_local, 2 * r), order="F") if want_mu else None
        t = th.struct()
        self._chk(self._L.ppls_sweep_stats(self.h, ct.byref(t), r, int(bool(want_mu)), dptr(out), dptr(mu)))
        SX = out[: self.p * r].reshape(r, self.p).T
        SY = out[self.p * r: (self.p + self.q) * r].reshape(r, self.q).T
        G = out[(self.p + self.q) * r:].reshape(2 * r, 2 * r).T
        return SX, SY, G, mu

    def finalize_plan(self, r, type=0):
        """The launch geometry of the next finalize with r components under the current options, from
        the function the launcher itself calls: {templated, KX, KY, staged, stage_budget (bytes of LDS
        left for staging S; 0 for the runtime-r kernel)}."""
        t, kx, ky, sg, bud = ct.c_int(), ct.c_int(), ct.c_int(), ct.c_int(), ct.c_int64()
        self._chk(self._L.ppls_finalize_plan(self.h, int(r), int(type), ct.byref(t), ct.byref(kx), ct.byref(ky),
                                             ct.byref(sg), ct.byref(bud)))
        return dict(templated=t.value, KX=kx.value, KY=ky.value, staged=sg.value, stage_budget=bud.value)

    def finalize_stats(self, th: Theta, SX, SY, G, type=0, iter=-1, gram_cur=None, vstate=None, xpM=None):
        """One production finalize on given statistics (``ppls_finalize_stats``): theta, X'mu_T (p x r),
        Y'mu_U (q x r), the Gram (2r x 2r), and optionally gram_cur = (W'W, C'C) (None: the scalar block
        forms them), vstate = (V_W, V_C) (None: identity) and xpM ((ldx + ldy) x 2r: the scalar block
        forms the Gram B'M itself, r <= 8).  Returns a dict: W, C (with their padding rows), B, sigT,
        sigE, sigF, sigH, alpha, beta, gamma, delta, moments (Expect), loglik (None when iter < 0),
        gram_nxt = (W'W, C'C), vstate = (V_W, V_C), gram_stats (the Gram slot after the launch), status,
        path = (code of W, code of C): 1 Cholesky-QR1, 2 Cholesky-QR2, 3 Householder, 4 QR type."""
        r = th.r
        f = lambda a: np.asfortranarray(a, dtype=np.float64).ravel(order="F")   # noqa: E731
        st = np.ascontiguousarray(np.concatenate([f(SX), f(SY), f(G)]))
        assert st.size == r * (self.p + self.q) + 4 * r * r
        pair = lambda ab: None if ab is None else np.ascontiguousarray(np.concatenate([f(ab[0]), f(ab[1])]))  # noqa: E731
        gc, vs = pair(gram_cur), pair(vstate)
        assert gc is None or gc.size == 2 * r * r
        assert vs is None or vs.size == 2 * r * r
        M = None if xpM is None else np.ascontiguousarray(f(xpM))
        t = th.struct()
        ldx, ldy = self._ld(self.p), self._ld(self.q)   # (the library refuses other widths than its own)
        Wn = np.zeros(ldx * r)
        Cn = np.zeros(ldy * r)
        assert M is None or M.size == (Wn.size + Cn.size) * 2
        sc = np.zeros(6 * r + 3)
        ex = Expect(r)
        es = ex.struct()
        ll = np.zeros(1)
        gn, vo, gs = np.zeros(2 * r * r), np.zeros(2 * r * r), np.zeros(4 * r * r)
        st3 = (ct.c_int * 3)()
        self._chk(self._L.ppls_finalize_stats(self.h, ct.byref(t), r, int(type), int(iter), dptr(st), dptr(gc),
                                              dptr(vs), dptr(M), ldx, ldy, dptr(Wn), dptr(Cn), dptr(sc), ct.byref(es), dptr(ll),
                                              dptr(gn), dptr(vo), dptr(gs), st3))
        ex.pull(es)
        sq = lambda v: v.reshape(r, r).T   # noqa: E731
        return dict(W=Wn.reshape(r, -1).T, C=Cn.reshape(r, -1).T, B=sc[:r], sigT=sc[r:2 * r], sigE=sc[2 * r],
                    sigF=sc[2 * r + 1], sigH=sc[2 * r + 2], alpha=sc[2 * r + 3:3 * r + 3],
                    beta=sc[3 * r + 3:4 * r + 3], gamma=sc[4 * r + 3:5 * r + 3], delta=sc[5 * r + 3:],
                    moments=ex, loglik=float(ll[0]) if iter >= 0 else None,
                    gram_nxt=(sq(gn[:r * r]), sq(gn[r * r:])), vstate=(sq(vo[:r * r]), sq(vo[r * r:])),
                    gram_stats=gs.reshape(2 * r, 2 * r).T, status=int(st3[0]), path=(int(st3[1]), int(st3[2])))

    @staticmethod
    def _ld(p):
        """The padded width of a p-column fp64 matrix under the default options (ld_of in ppls_capi.cpp)."""
        if p <= 2048:
            return (p + 1) & ~1
        al = 4096 if p * 8 >= 16384 else 128
        return (p * 8 + al - 1) // al * al // 8

    def xprod_info(self, r=1):
        """{ready, bytes_per_pass (8 P^2), gram_flops (as computed), rows_per_wave} of the cross-product form."""
        rd, b, f, rw = ct.c_int(), ct.c_int64(), ct.c_double(), ct.c_int()
        self._chk(self._L.ppls_xprod_info(self.h, int(r), ct.byref(rd), ct.byref(b), ct.byref(f), ct.byref(rw)))
        return dict(ready=bool(rd.value), bytes_per_pass=b.value, gram_flops=f.value, rows_per_wave=rw.value)

    def scores(self, W, C):
        """scores.PPLS (EM_W_multi.R:411-420) on the resident rows: (X W, Y C), n_local x k each."""
        W = np.asfortranarray(np.array(W, dtype=np.float64, ndmin=2).reshape(self.p, -1))
        C = np.asfortranarray(np.array(C, dtype=np.float64, ndmin=2).reshape(self.q, -1))
        k = W.shape[1]
        if C.shape[1] != k:
            raise ValueError("W and C need the same number of components")
        T = np.zeros((self.n_local, k), order="F")
        U = np.zeros((self.n_local, k), order="F")
        self._chk(self._L.ppls_scores(self.h, dptr(W), dptr(C), int(k), dptr(T), dptr(U)))
        return T, U

    # -- PO2PLS from the cross-products
    def po2_estep(self, th: Po2Theta, want_cdz=True) -> Po2Expect:
        """EMstepC's list (loglC.cpp:116-250) at theta, from the S the context holds."""
        e = Po2Expect(self.p, self.q, th.r, th.rx, th.ry, want_cdz)
        ts, es = th.struct(), e.struct()
        self._chk(self._L.ppls_po2_estep(self.h, ct.byref(ts), th.r, th.rx, th.ry, ct.byref(es)))
        e.pull(es)
        return e

    def po2_loglik(self, th: Po2Theta) -> float:
        """loglC's value (loglC.cpp:36-113) at theta, from S."""
        out = ct.c_double()
        ts = th.struct()
        self._chk(self._L.ppls_po2_loglik(self.h, ct.byref(ts), th.r, th.rx, th.ry, ct.byref(out)))
        return out.value

    def po2_em_run(self, th: Po2Theta, max_steps=100, atol=1e-4, type_=_lib.PPLS_ORTH_SVD, want_eout=True):
        """The PO2PLS EM loop on the device; returns (estimates, loglik history, Po2Expect or None,
        negative increment seen)."""
        est = th.copy()
        e = Po2Expect(self.p, self.q, th.r, th.rx, th.ry) if want_eout else None
        ll = np.zeros(int(max_steps) + 1)
        n, neg = ct.c_int(), ct.c_int()
        ts = est.struct()
        es = e.struct() if e is not None else None
        self._chk(self._L.ppls_po2_em_run(self.h, ct.byref(ts), th.r, th.rx, th.ry, int(max_steps), float(atol), int(type_),
                                          dptr(ll), len(ll), ct.byref(n), ct.byref(neg),
                                          ct.byref(es) if es is not None else None))
        est.pull(ts)
        if e is not None:
            e.pull(es)
        return est, ll[:n.value].copy(), e, bool(neg.value)

    def po2_start(self, r, rx, ry, V0x=None, V0y=None, steps=10) -> Po2Theta:
        """ppls_po2_start: the default start values -- the joint part from the one-step 'o2m_xprod' sequential
        fit, the specific loadings from ``steps`` orthogonal-iteration steps of the statistics pass started
        at V0x (p x rx) and V0y (q x ry), sigTo / sigUo from V'S V / N."""
        r, rx, ry = int(r), int(rx), int(ry)
        th = Po2Theta(np.zeros((self.p, r)), np.zeros((self.p, rx)), np.zeros((self.q, r)), np.zeros((self.q, ry)),
                      np.zeros(r), np.zeros(r), np.zeros(rx), np.zeros(ry), 1.0, 1.0, 1.0)
        vx = np.asfortranarray(np.asarray(V0x, dtype=np.float64).reshape(self.p, rx)) if rx else None
        vy = np.asfortranarray(np.asarray(V0y, dtype=np.float64).reshape(self.q, ry)) if ry else None
        ts = th.struct()
        self._chk(self._L.ppls_po2_start(self.h, r, rx, ry, dptr(vx), dptr(vy), int(steps), ct.byref(ts)))
        th.pull(ts)
        return th

    def po2_em_step(self, th: Po2Theta, type_=_lib.PPLS_ORTH_SVD) -> Po2Theta:
        """One ECM step at theta as the device leaves it (ppls_po2_em_step): no canonical form."""
        out = th.copy()
        ts, os_ = th.struct(), out.struct()
        self._chk(self._L.ppls_po2_em_step(self.h, ct.byref(ts), th.r, th.rx, th.ry, int(type_), ct.byref(os_)))
        out.pull(os_)
        return out

    def po2_stats(self, Gx, Gy, S=None, ldx=None, rw=0):
        """The PO2 statistics pass and Gram alone: (M, Q, Gx'Gx, Gy'Gy) for loadings Gx (ldx x kx), Gy
        (ldy x ky) given with their padding rows, on a host S (row-major P x P, X block ldx wide) or,
        S = None, on the context's own."""
        Gx = np.asfortranarray(np.array(Gx, dtype=np.float64, ndmin=2))
        Gy = np.asfortranarray(np.array(Gy, dtype=np.float64, ndmin=2))
        kx, ky = Gx.shape[1], Gy.shape[1]
        ldx = Gx.shape[0] if ldx is None else int(ldx)
        P = ldx + Gy.shape[0]
        if S is not None:
            S = np.ascontiguousarray(S, dtype=np.float64)
            if S.shape != (P, P):
                raise ValueError(f"S must be {P} x {P}")
        k = kx + ky
        M, Q, GG = np.zeros((P, k), order="F"), np.zeros((k, k), order="F"), np.zeros(kx * kx + ky * ky)
        self._chk(self._L.ppls_po2_stats(self.h, dptr(S) if S is not None else None, P, ldx, dptr(Gx), kx, dptr(Gy), ky,
                                         int(rw), dptr(M), dptr(Q), dptr(GG)))
        return M, Q, GG[:kx * kx].reshape(kx, kx, order="F").copy(), GG[kx * kx:].reshape(ky, ky, order="F").copy()

    def po2_small(self, Q, GGx, GGy, th: Po2Theta, p, q, N, ssqX, ssqY):
        """The small kernel alone: (Po2Expect without C_dz or None, loglik or None, status word)."""
        k = 2 * th.r + th.rx + th.ry
        Q = np.asfortranarray(np.array(Q, dtype=np.float64).reshape(k, k))
        GG = np.concatenate([np.ravel(np.asarray(GGx, dtype=np.float64), order="F"),
                             np.ravel(np.asarray(GGy, dtype=np.float64), order="F")])
        e = Po2Expect(int(p), int(q), th.r, th.rx, th.ry, want_cdz=False)
        ts, es = th.struct(), e.struct()
        ll, st = ct.c_double(float("nan")), ct.c_int()
        rc = self._L.ppls_po2_small(self.h, dptr(Q), dptr(GG), ct.byref(ts), th.r, th.rx, th.ry, int(p), int(q), float(N),
                                    float(ssqX), float(ssqY), ct.byref(es), ct.byref(ll), ct.byref(st))
        if rc == -3:   # PPLS_E_NUMERIC: the status word says why
            return None, None, st.value
        self._chk(rc)
        e.pull(es)
        return e, ll.value, st.value

    def po2_timing(self, th: Po2Theta, reps=50):
        """HIP-event ms per launch: dict(pass, gram, small, update, iteration, update_qr)."""
        ms = np.zeros(6)
        ts = th.struct()
        self._chk(self._L.ppls_po2_timing(self.h, ct.byref(ts), th.r, th.rx, th.ry, int(reps), dptr(ms)))
        return dict(zip(("pass", "gram", "small", "update", "iteration", "update_qr"), ms.tolist()))

    # -- batched PO2PLS fits and cross-validation over (r, rx, ry)
    def po2_em_run_batch(self, thetas, max_steps=100, atol=1e-4, type_=_lib.PPLS_ORTH_SVD):
        """ppls_po2_em_run_batch: the EM loop of every Po2Theta in ``thetas`` (shapes may differ or repeat)
        at once on the context's S.  Returns (estimates, histories, negative increments, status): lists with
        one entry per model; a failed model (status -3) keeps its start and an empty history."""
        ests = [t.copy() for t in thetas]
        m, cap = len(ests), int(max_steps) + 1
        structs = [t.struct() for t in ests]
        arr = (_lib.PplsPo2Theta * max(m, 1))(*structs)
        ia = lambda v: np.ascontiguousarray(v, dtype=np.int32)   # noqa: E731
        ip = lambda a: a.ctypes.data_as(_lib._ip)                # noqa: E731
        r, rx, ry = ia([t.r for t in ests]), ia([t.rx for t in ests]), ia([t.ry for t in ests])
        ll = np.zeros((max(m, 1), cap))
        n, neg, st = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.int32)
        self._chk(self._L.ppls_po2_em_run_batch(self.h, m, arr, ip(r), ip(rx), ip(ry), int(max_steps), float(atol), int(type_),
                                                dptr(ll), cap, ip(n), ip(neg), ip(st)))
        for t, s in zip(ests, arr):
            t.pull(s)
        return ests, [ll[j, :n[j]].copy() for j in range(m)], [bool(v) for v in neg[:m]], [int(v) for v in st[:m]]

    def po2_stats_batch(self, Gxs, Gys, S=None, ldx=None):
        """The batched statistics pass and Gram alone (ppls_po2_stats_batch): per model (M, Q, Gx'Gx, Gy'Gy)
        as ``po2_stats`` returns them, for lists of padded loadings Gxs[j] (ldx x kx_j), Gys[j] (ldy x ky_j)."""
        Gxs = [np.asfortranarray(np.array(G, dtype=np.float64, ndmin=2)) for G in Gxs]
        Gys = [np.asfortranarray(np.array(G, dtype=np.float64, ndmin=2)) for G in Gys]
        m = len(Gxs)
        if m < 1 or len(Gys) != m:
            raise ValueError("one Gx and one Gy per model, at least one model")
        ldx = Gxs[0].shape[0] if ldx is None else int(ldx)
        P = ldx + Gys[0].shape[0]
        if any(G.shape[0] != ldx for G in Gxs) or any(G.shape[0] != P - ldx for G in Gys):
            raise ValueError("every model's loadings need the same padded row counts")
        if S is not None:
            S = np.ascontiguousarray(S, dtype=np.float64)
            if S.shape != (P, P):
                raise ValueError(f"S must be {P} x {P}")
        kx = np.ascontiguousarray([G.shape[1] for G in Gxs], dtype=np.int32)
        ky = np.ascontiguousarray([G.shape[1] for G in Gys], dtype=np.int32)
        k = kx + ky
        Gx, Gy = np.asfortranarray(np.hstack(Gxs)), np.asfortranarray(np.hstack(Gys))
        M, Q, GG = np.zeros(int(P * k.sum())), np.zeros(int((k * k).sum())), np.zeros(int((kx * kx + ky * ky).sum()))
        ip = lambda a: a.ctypes.data_as(_lib._ip)                # noqa: E731
        self._chk(self._L.ppls_po2_stats_batch(self.h, dptr(S) if S is not None else None, P, ldx, m, ip(kx), ip(ky), dptr(Gx),
                                               dptr(Gy), dptr(M), dptr(Q), dptr(GG)))
        out, oM, oQ, oG = [], 0, 0, 0
        for j in range(m):
            a, b, kk = int(kx[j]), int(ky[j]), int(k[j])
            out.append((M[oM:oM + P * kk].reshape(P, kk, order="F").copy(), Q[oQ:oQ + kk * kk].reshape(kk, kk, order="F").copy(),
                        GG[oG:oG + a * a].reshape(a, a, order="F").copy(),
                        GG[oG + a * a:oG + a * a + b * b].reshape(b, b, order="F").copy()))
            oM, oQ, oG = oM + P * kk, oQ + kk * kk, oG + a * a + b * b
        return out

    def po2_timing_batch(self, thetas, steps=50, reps=3):
        """HIP-event ms per EM iteration (ppls_po2_timing_batch): dict(batch, sequential, batch_pass,
        sequential_pass) -- the batched iteration and pass against the same models one after another through
        the single-model launches, device time only."""
        structs = [t.struct() for t in thetas]
        arr = (_lib.PplsPo2Theta * len(thetas))(*structs)
        ia = lambda v: np.ascontiguousarray(v, dtype=np.int32)   # noqa: E731
        ip = lambda a: a.ctypes.data_as(_lib._ip)                # noqa: E731
        r, rx, ry = ia([t.r for t in thetas]), ia([t.rx for t in thetas]), ia([t.ry for t in thetas])
        ms = np.zeros(4)
        self._chk(self._L.ppls_po2_timing_batch(self.h, len(thetas), arr, ip(r), ip(rx), ip(ry), int(steps), int(reps), dptr(ms)))
        return dict(zip(("batch", "sequential", "batch_pass", "sequential_pass"), ms.tolist()))

    def po2_cv_stream(self, cands, max_steps=100, atol=1e-4, type_=_lib.PPLS_ORTH_SVD, V0x=None, V0y=None, start_steps=10,
                      want_fits=False):
        """ppls_po2_cv_stream on a context streamed with folds: ``cands`` a list of (r, rx, ry).  Returns
        dict(rmsep, cond, steps, status) of K x len(cands) arrays, with ``want_fits`` also ``fits`` (K lists of
        Po2Theta, None where the candidate failed)."""
        K = int(self.stream_fold_info()["nr_folds"])
        nc = len(cands)
        ia = lambda v: np.ascontiguousarray(v, dtype=np.int32)   # noqa: E731
        ip = lambda a: a.ctypes.data_as(_lib._ip)                # noqa: E731
        r, rx, ry = (ia([c[i] for c in cands]) for i in range(3))
        mrx, mry = int(rx.max()) if nc else 0, int(ry.max()) if nc else 0
        vx = np.asfortranarray(np.asarray(V0x, dtype=np.float64).reshape(self.p, -1)[:, :mrx]) if mrx else None
        vy = np.asfortranarray(np.asarray(V0y, dtype=np.float64).reshape(self.q, -1)[:, :mry]) if mry else None
        if (mrx and vx.shape[1] < mrx) or (mry and vy.shape[1] < mry):
            raise ValueError("V0x / V0y need max(rx) / max(ry) columns")
        Kn = max(K, 1) * max(nc, 1)
        rmsep, cond = np.full(Kn, np.nan), np.full(Kn, np.nan)
        steps, status = np.zeros(Kn, np.int32), np.zeros(Kn, np.int32)
        fits, arr = None, None
        if want_fits and K and nc:
            fits = [[Po2Theta(np.zeros((self.p, c[0])), np.zeros((self.p, c[1])), np.zeros((self.q, c[0])), np.zeros((self.q, c[2])),
                              np.zeros(c[0]), np.zeros(c[0]), np.zeros(c[1]), np.zeros(c[2]), 1.0, 1.0, 1.0) for c in cands]
                    for _ in range(K)]
            arr = (_lib.PplsPo2Theta * (K * nc))(*[t.struct() for f in fits for t in f])
        try:
            self._chk(self._L.ppls_po2_cv_stream(self.h, nc, ip(r), ip(rx), ip(ry), int(max_steps), float(atol), int(type_),
                                                 dptr(vx), dptr(vy), int(start_steps), dptr(rmsep), dptr(cond), ip(steps),
                                                 ip(status), arr))
        finally:
            if self._stream_folds:
                self.n_total = self.stream_info()["n_total"]     # selected on -1 again
        sh = (K, nc)
        out = dict(rmsep=rmsep[:K * nc].reshape(sh), cond=cond[:K * nc].reshape(sh), steps=steps[:K * nc].reshape(sh),
                   status=status[:K * nc].reshape(sh))
        if fits is not None:
            for f in range(K):
                for j in range(nc):
                    fits[f][j].pull(arr[f * nc + j])
                    if out["status"][f, j] != 0:
                        fits[f][j] = None
            out["fits"] = fits
        return out

    # -- cross-validation (crossval_PPLS.R:12-114)
    @staticmethod
    def _rows(rows):
        rows = np.ascontiguousarray(np.ravel(np.asarray(rows, dtype=np.int64)))
        return rows, rows.ctypes.data_as(_lib._i64p)

    def set_data_from(self, src: "Context", rows, n_total=None):
        """This context's data := rows ``rows`` (ascending local indices) of ``src``'s resident
        data, gathered on the device (ppls_set_data_from).  ``n_total``: the subset's rows over
        all ranks (default: ``len(rows)``)."""
        rows, rp = self._rows(rows)
        nt = rows.shape[0] if n_total is None else int(n_total)
        self._chk(self._L.ppls_set_data_from(self.h, src.h, rp, rows.shape[0], nt))
        self.p, self.q, self.n_local, self.n_total, self.row0 = src.p, src.q, rows.shape[0], nt, 0
        self._stream_folds = None

    def xprod_downdate(self, src: "Context", out_rows):
        """This context's cross-products S := ``src``'s S minus the Gram of ``src``'s rows
        ``out_rows`` (ppls_xprod_downdate); this context must hold ``src``'s other rows."""
        rows, rp = self._rows(out_rows)
        self._chk(self._L.ppls_xprod_downdate(self.h, src.h, rp, rows.shape[0]))

    @staticmethod
    def _counts(count, n):
        a = np.asarray(count)
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"counts: one per local row ({n}), got shape {a.shape}")
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("counts must be integers")
        if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
            raise ValueError("counts must fit 32 bits")
        cnt = np.ascontiguousarray(a, dtype=np.int32)
        return cnt, (cnt.ctypes.data_as(ct.POINTER(ct.c_int32)) if cnt.size else None)

    def xprod_resample(self, src: "Context", count):
        """This context's cross-products := sum_i count_i d_i d_i' over ``src``'s resident rows
        (ppls_xprod_resample): the S of ``src``'s data with row i repeated ``count[i]`` times, formed by
        the weighted MFMA Gram with no copy of the rows.  This context ends streamed (S, no rows), with
        ``src``'s shape and scaling record and ``n_total = sum(count)`` over all ranks; ``src`` is left
        as it was.  Collective over ``src``'s ranks, each passing the counts of its own rows."""
        cnt, cp = self._counts(count, src.n_local)
        self._chk(self._L.ppls_xprod_resample(self.h, src.h, cp))
        self.p, self.q, self.n_local, self.row0 = src.p, src.q, 0, 0
        self.n_total = self.stream_info()["n_total"]
        self._stream_folds = None

    @staticmethod
    def _weights(weight, n):
        w = np.ascontiguousarray(weight, dtype=np.float64)
        if w.ndim != 1 or w.shape[0] != n:
            raise ValueError(f"weights: one per local row ({n}), got shape {w.shape}")
        return w if w.size else np.zeros(1)   # (a pointer the library never reads)

    def xprod_weighted(self, src: "Context", weight=None):
        """This context's cross-products := sum_i weight_i d_i d_i' over ``src``'s resident rows
        (ppls_xprod_weighted), by the real-weighted MFMA Gram with no copy of the rows.  ``weight``: one
        finite real >= 0 per local row of ``src``, or None for the weights ``src`` keeps from
        ``robust_weights`` (they never leave the device).  This context ends streamed (S, no rows) with
        ``src``'s shape, scaling record and ``n_total``: the weights are relative to N and are not
        renormalised.  ``src`` is left as it was.  Collective over ``src``'s ranks."""
        w = None if weight is None else self._weights(weight, src.n_local)
        self._chk(self._L.ppls_xprod_weighted(self.h, src.h, dptr(w)))
        self.p, self.q, self.n_local, self.row0 = src.p, src.q, 0, 0
        self.n_total = self.stream_info()["n_total"]
        self._stream_folds = None

    def robust_weights(self, th: Theta, nu=4.0, keep=0):
        """E-step of the multivariate-t model on the resident rows (ppls_robust_weights): the distance
        pass of ``row_diagnostics`` and one small kernel.  ``nu``: a value or up to 16 of them.  Returns
        ``(loglik_t, sum_w)``: the t log-likelihood of ``th`` at every ``nu`` over all ranks' rows and
        the sum of the weights ``(nu[keep] + p + q) / (nu[keep] + d2_i)``, which stay on the device with
        their distances (``robust_get``, ``xprod_weighted(src, None)``).  Collective when sharded."""
        nus = np.ascontiguousarray(np.atleast_1d(np.asarray(nu, dtype=np.float64)))
        g = self._ROWDIAG_GUARD
        ll = np.full(nus.shape[0] + g, np.nan)
        sw = np.full(1 + g, np.nan)
        self._robust_last = (ll, sw)
        t = th.struct()
        self._chk(self._L.ppls_robust_weights(self.h, ct.byref(t), th.r, dptr(nus), nus.shape[0], int(keep), dptr(ll),
                                              dptr(sw)))
        if not (np.all(np.isnan(ll[nus.shape[0]:])) and np.all(np.isnan(sw[1:]))):
            raise PplsError(-1, "robust_weights wrote past the end of its outputs")
        return ll[: nus.shape[0]].copy(), float(sw[0])

    def robust_timing(self, reps=20):
        """The weights and t log-likelihood kernels alone over all local rows, ms between HIP events
        averaged over ``reps`` launches (ppls_robust_timing): dict(ms1, ms16) for one and for 16 nu."""
        ms = np.zeros(2)
        self._chk(self._L.ppls_robust_timing(self.h, int(reps), dptr(ms)))
        return dict(ms1=float(ms[0]), ms16=float(ms[1]))

    def robust_get(self, want_w=True, want_d2=True):
        """Host copies ``(weights, d2)`` of what the last ``robust_weights`` kept (ppls_robust_get); None
        for a part not wanted."""
        n = int(self.n_local)
        w = np.full(n, np.nan) if want_w else None
        d2 = np.full(n, np.nan) if want_d2 else None
        self._chk(self._L.ppls_robust_get(self.h, dptr(w) if n else None, dptr(d2) if n else None))
        return w, d2

    @staticmethod
    def _perm(perm, n):
        """A permutation of the ``n`` local rows as a contiguous int64 vector and its ctypes pointer (NULL
        when empty); whether it is one is checked by the library."""
        a = np.asarray(perm)
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"perm: one index per local row ({n}), got shape {a.shape}")
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("perm must hold integers")
        idx = np.ascontiguousarray(a, dtype=np.int64)
        return idx, (idx.ctypes.data_as(ct.POINTER(ct.c_int64)) if idx.size else None)

    def xprod_permute(self, src: "Context", perm):
        """This context's cross-products := [X Y_pi]'[X Y_pi] with ``Y_pi[i] = Y[perm[i]]`` over ``src``'s
        resident rows (ppls_xprod_permute): X'X and Y'Y are copied from ``src``'s S (formed and kept if it
        is not there), the p x q block sum_i x_i y_perm[i]' comes from a rectangular MFMA kernel over the
        rows where they lie.  ``perm``: a permutation of ``src``'s local rows 0 .. n_local - 1.  This
        context ends streamed (S, no rows) with ``src``'s shape, scaling record, ``n_total`` and sums of
        squares; ``src`` is left as it was.  Collective over ``src``'s ranks, each permuting its own rows."""
        idx, ip = self._perm(perm, src.n_local)
        self._chk(self._L.ppls_xprod_permute(self.h, src.h, ip))
        self.p, self.q, self.n_local, self.row0 = src.p, src.q, 0, 0
        self.n_total = self.stream_info()["n_total"]
        self._stream_folds = None

    def gram_permuted(self, perm, nsplit=0, want=True):
        """sum_i x_i y_perm[i]' (p x q) on the permuted cross-block kernel alone, this rank's rows ->
        (C or None, kernel ms) (ppls_xgram_permuted).  ``nsplit`` 0: the automatic row splits."""
        idx, ip = self._perm(perm, self.n_local)
        C = np.zeros((self.p, self.q), order="F") if want else None
        ms = ct.c_double()
        self._chk(self._L.ppls_xgram_permuted(self.h, int(nsplit), ip, dptr(C), ct.byref(ms)))
        return C, ms.value

    def xperm_timing(self):
        """Wall-clock ms of the last ``xprod_permute`` into this context: dict(check, upload, kernel, total)
        (ppls_xperm_timing)."""
        ms = np.zeros(4)
        self._chk(self._L.ppls_xperm_timing(self.h, dptr(ms)))
        return dict(check=ms[0], upload=ms[1], kernel=ms[2], total=ms[3])

    def xperm_occupancy(self, f32=False):
        """Workgroups of the permuted cross-block kernel per compute unit, for fp64 or fp32 storage."""
        return int(self._L.ppls_xperm_occupancy(int(bool(f32))))

    @staticmethod
    def _fit_arrays(W, C, B):
        W = np.asfortranarray(np.array(W, dtype=np.float64, ndmin=2))
        C = np.asfortranarray(np.array(C, dtype=np.float64, ndmin=2))
        B = np.asarray(B, dtype=np.float64)
        B = np.ascontiguousarray(np.diag(B) if B.ndim == 2 else np.ravel(B)).copy()
        if W.shape[1] != C.shape[1] or B.shape[0] != W.shape[1]:
            raise ValueError("W, C and B need the same number of components")
        return W, C, B

    def predict(self, W, C, B, newdata, xory=0):
        """predict.PPLS (crossval_PPLS.R:12-24) for a host matrix ``newdata``: xory 0 gives
        newdata W diag(B) C', xory 1 newdata C diag(1/B) W' (ppls_predict).  The context supplies the
        device and the shape (p, q) of its data; ``newdata`` is independent of the resident rows."""
        W, C, B = self._fit_arrays(W, C, B)
        if W.shape[0] != self.p or C.shape[0] != self.q:
            raise ValueError(f"the fit is {W.shape[0]} x {C.shape[0]}, the context's data {self.p} x {self.q}")
        nd = np.asarray(newdata, dtype=np.float64)
        if nd.ndim != 2 or nd.shape[1] != (self.q if xory else self.p):
            raise ValueError("Number of columns mismatch!")
        if nd.flags.f_contiguous and not nd.flags.c_contiguous:
            layout = _lib.PPLS_LAYOUT_COLMAJOR
        else:
            nd = np.ascontiguousarray(nd)
            layout = _lib.PPLS_LAYOUT_ROWMAJOR
        pred = np.zeros((nd.shape[0], self.p if xory else self.q), order="F")
        self._chk(self._L.ppls_predict(self.h, dptr(W), dptr(C), dptr(B), W.shape[1], int(xory), dptr(nd),
                                       nd.shape[0], layout, dptr(pred)))
        return pred

    def heldout_sse(self, W, C, B, rows):
        """sum_i ||y_i - yhat_i(j)||^2 over the resident rows ``rows`` for every prefix j = 1..k of
        the components, summed over ranks (ppls_heldout_sse): k values."""
        W, C, B = self._fit_arrays(W, C, B)
        if W.shape[0] != self.p or C.shape[0] != self.q:
            raise ValueError(f"the fit is {W.shape[0]} x {C.shape[0]}, the context's data {self.p} x {self.q}")
        rows, rp = self._rows(rows)
        sse = np.zeros(W.shape[1])
        self._chk(self._L.ppls_heldout_sse(self.h, dptr(W), dptr(C), dptr(B), W.shape[1], rp, rows.shape[0],
                                           dptr(sse)))
        return sse

    # -- row diagnostics
    _ROWDIAG_GUARD = 8   # doubles behind every output buffer, NaN before the call and checked after it

    def _rowdiag_out(self, n, r, want_mu):
        """The output buffers of one diagnostics call: every one ``_ROWDIAG_GUARD`` doubles longer than the
        library is told and filled with NaN, so that a refusal (nothing written) and a write past the
        end can both be seen.  Kept on the context as ``_rowdiag_last`` until the next call."""
        g = self._ROWDIAG_GUARD
        bufs = {k: np.full(n + g, np.nan) for k in ("odx2", "ody2", "sd2", "d2", "loglik")}
        if want_mu:
            bufs["mu_T"] = np.full(n * r + g, np.nan)
            bufs["mu_U"] = np.full(n * r + g, np.nan)
        self._rowdiag_last = bufs
        s = _lib.PplsRowDiag(*[dptr(bufs.get(k)) for k in ("odx2", "ody2", "sd2", "d2", "loglik", "mu_T", "mu_U")])
        return bufs, s

    def _rowdiag_result(self, bufs, n, r):
        g = self._ROWDIAG_GUARD
        out = {}
        for k, b in bufs.items():
            if not np.all(np.isnan(b[b.shape[0] - g:])):
                raise PplsError(-1, f"row diagnostics wrote past the end of {k}")
            out[k] = b[: n * r].reshape((n, r), order="F") if k in ("mu_T", "mu_U") else b[:n]
        return out

    def row_diagnostics(self, th: Theta, rows=None, want_mu=False):
        """Per resident row of this rank (ppls_row_diagnostics): the orthogonal distances ``odx2``,
        ``ody2``, the score distance ``sd2``, the squared Mahalanobis distance ``d2`` under the fitted
        covariance and the log-density ``loglik`` (its sum over all rows is ``loglik(th)``); with
        ``want_mu`` Expect_M's ``mu_T``, ``mu_U`` from the same read.  ``rows``: local indices in any
        order, repeats allowed (default: all).  No collective; a row's values are bitwise the same in
        any subset or shard."""
        if rows is None:
            n, rp = int(self.n_local), None
        else:
            rows, rp = self._rows(rows)
            n = rows.shape[0]
            if n == 0:
                rp = None
        bufs, s = self._rowdiag_out(n, th.r, want_mu)
        t = th.struct()
        if rows is not None and n == 0:   # an empty list is not "all rows"
            return self._rowdiag_result(bufs, 0, th.r)
        self._chk(self._L.ppls_row_diagnostics(self.h, ct.byref(t), th.r, rp, n, ct.byref(s)))
        return self._rowdiag_result(bufs, n, th.r)

    def row_diagnostics_new(self, th: Theta, X, Y, want_mu=False):
        """The same for host rows ``X, Y`` in the fit's units (ppls_row_diagnostics_new): staged through
        the device in blocks; the context gives the device and the shape only, so a streamed context
        or one without rows serves, and its own data are not touched."""
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError("X and Y must be matrices with the same number of rows")
        if X.shape[1] != self.p or Y.shape[1] != self.q:
            raise ValueError("Number of columns mismatch!")
        if X.flags.f_contiguous and Y.flags.f_contiguous and not (X.flags.c_contiguous and Y.flags.c_contiguous):
            layout = _lib.PPLS_LAYOUT_COLMAJOR
        else:
            X = np.ascontiguousarray(X)
            Y = np.ascontiguousarray(Y)
            layout = _lib.PPLS_LAYOUT_ROWMAJOR
        n = X.shape[0]
        bufs, s = self._rowdiag_out(n, th.r, want_mu)
        t = th.struct()
        self._chk(self._L.ppls_row_diagnostics_new(self.h, ct.byref(t), th.r, dptr(X), dptr(Y), n, layout, ct.byref(s)))
        return self._rowdiag_result(bufs, n, th.r)

    def rowdiag_timing(self, r, reps=20):
        """The diagnostics kernel alone over all local rows, ms between HIP events averaged over ``reps``
        launches (ppls_rowdiag_timing): dict(ms, ms_mu) without and with the posterior means."""
        ms = np.zeros(2)
        self._chk(self._L.ppls_rowdiag_timing(self.h, int(r), int(reps), dptr(ms)))
        return dict(ms=ms[0], ms_mu=ms[1])

    # -- PO2PLS row diagnostics and t-model weights
    def _po2_rowdiag_out(self, n, k, want_mu):
        """``_rowdiag_out`` for the PO2PLS entries: one ``mu`` of n x k."""
        g = self._ROWDIAG_GUARD
        bufs = {key: np.full(n + g, np.nan) for key in ("odx2", "ody2", "sd2", "d2", "loglik")}
        if want_mu:
            bufs["mu"] = np.full(n * k + g, np.nan)
        self._rowdiag_last = bufs
        return bufs, _lib.PplsPo2RowDiag(*[dptr(bufs.get(key)) for key in ("odx2", "ody2", "sd2", "d2", "loglik", "mu")])

    def _po2_rowdiag_result(self, bufs, n, k):
        g = self._ROWDIAG_GUARD
        out = {}
        for key, b in bufs.items():
            if not np.all(np.isnan(b[b.shape[0] - g:])):
                raise PplsError(-1, f"row diagnostics wrote past the end of {key}")
            out[key] = b[: n * k].reshape((n, k), order="F") if key == "mu" else b[:n]
        return out

    def po2_row_diagnostics(self, th: Po2Theta, rows=None, want_mu=False):
        """``row_diagnostics`` under a PO2PLS fit (ppls_po2_row_diagnostics): ``odx2``, ``ody2`` are the squared
        distances to the planes of [W Wo] and [C Co], ``sd2`` the distance of the k = 2r + rx + ry scores under
        their dense covariance, ``d2`` and ``loglik`` as there (the sum of ``loglik`` over all rows is
        ``po2_loglik(th)``); with ``want_mu`` the posterior means ``mu`` (n x k, columns t, to, u, uo).  The
        loadings need not be orthonormal.  Reads no S and forms none."""
        if rows is None:
            n, rp = int(self.n_local), None
        else:
            rows, rp = self._rows(rows)
            n = rows.shape[0]
            if n == 0:
                rp = None
        k = 2 * th.r + th.rx + th.ry
        bufs, s = self._po2_rowdiag_out(n, k, want_mu)
        t = th.struct()
        if rows is not None and n == 0:   # an empty list is not "all rows"
            return self._po2_rowdiag_result(bufs, 0, k)
        self._chk(self._L.ppls_po2_row_diagnostics(self.h, ct.byref(t), th.r, th.rx, th.ry, rp, n, ct.byref(s)))
        return self._po2_rowdiag_result(bufs, n, k)

    def po2_row_diagnostics_new(self, th: Po2Theta, X, Y, want_mu=False):
        """The same for host rows ``X, Y`` in the fit's units (ppls_po2_row_diagnostics_new), staged as
        ``row_diagnostics_new`` stages them: any context of the fit's shape serves."""
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
            raise ValueError("X and Y must be matrices with the same number of rows")
        if X.shape[1] != self.p or Y.shape[1] != self.q:
            raise ValueError("Number of columns mismatch!")
        if X.flags.f_contiguous and Y.flags.f_contiguous and not (X.flags.c_contiguous and Y.flags.c_contiguous):
            layout = _lib.PPLS_LAYOUT_COLMAJOR
        else:
            X = np.ascontiguousarray(X)
            Y = np.ascontiguousarray(Y)
            layout = _lib.PPLS_LAYOUT_ROWMAJOR
        n = X.shape[0]
        k = 2 * th.r + th.rx + th.ry
        bufs, s = self._po2_rowdiag_out(n, k, want_mu)
        t = th.struct()
        self._chk(self._L.ppls_po2_row_diagnostics_new(self.h, ct.byref(t), th.r, th.rx, th.ry, dptr(X), dptr(Y), n, layout,
                                                       ct.byref(s)))
        return self._po2_rowdiag_result(bufs, n, k)

    def po2_robust_weights(self, th: Po2Theta, nu=4.0, keep=0):
        """``robust_weights`` under a PO2PLS fit (ppls_po2_robust_weights): the distance pass of
        ``po2_row_diagnostics`` and the same weight kernel.  The weights and distances are kept where
        ``robust_weights`` keeps them: ``robust_get`` and ``xprod_weighted(src, None)`` work as they are."""
        nus = np.ascontiguousarray(np.atleast_1d(np.asarray(nu, dtype=np.float64)))
        g = self._ROWDIAG_GUARD
        ll = np.full(nus.shape[0] + g, np.nan)
        sw = np.full(1 + g, np.nan)
        self._robust_last = (ll, sw)
        t = th.struct()
        self._chk(self._L.ppls_po2_robust_weights(self.h, ct.byref(t), th.r, th.rx, th.ry, dptr(nus), nus.shape[0], int(keep),
                                                  dptr(ll), dptr(sw)))
        if not (np.all(np.isnan(ll[nus.shape[0]:])) and np.all(np.isnan(sw[1:]))):
            raise PplsError(-1, "po2_robust_weights wrote past the end of its outputs")
        return ll[: nus.shape[0]].copy(), float(sw[0])

    def po2_rowdiag_info(self, r, rx, ry, f32=False):
        """What ``po2_row_diagnostics`` runs for these sizes on this context's shape and fp64 (``f32``: fp32)
        storage (ppls_po2_rowdiag_info): dict(tile_x, tile_y, rows_per_wave)."""
        tx, ty, rw = ct.c_int(), ct.c_int(), ct.c_int()
        self._chk(self._L.ppls_po2_rowdiag_info(self.p, self.q, int(bool(f32)), int(r), int(rx), int(ry), ct.byref(tx), ct.byref(ty),
                                                ct.byref(rw)))
        return dict(tile_x=tx.value, tile_y=ty.value, rows_per_wave=rw.value)

    def po2_rowdiag_timing(self, th: Po2Theta, reps=20):
        """The PO2PLS row kernel alone over all local rows, ms between HIP events averaged over ``reps``
        launches (ppls_po2_rowdiag_timing): dict(ms, ms_mu) without and with the posterior means."""
        ms = np.zeros(2)
        t = th.struct()
        self._chk(self._L.ppls_po2_rowdiag_timing(self.h, ct.byref(t), th.r, th.rx, th.ry, int(reps), dptr(ms)))
        return dict(ms=ms[0], ms_mu=ms[1])

    def cv_ppls(self, a: int, fold_of_row, fold_total, max_steps: int, atol: float, inits, crit_abs=False):
        """cv_PPLS's loop for given folds (ppls_cv_ppls).  ``fold_of_row``: the fold of each local
        row; ``fold_total``: rows per fold over all ranks; ``inits``: per fold a list of ``a``
        starting values (dicts as for ``ppls``).  Returns (rmsep nfolds x a, ncomp nfolds): the RMSEP
        of every prefix of the components, NaN past a fold's ncomp."""
        p, q = self.p, self.q
        fold_of_row = np.ascontiguousarray(np.ravel(np.asarray(fold_of_row, dtype=np.int32)))
        fold_total = np.ascontiguousarray(np.ravel(np.asarray(fold_total, dtype=np.int64)))
        K = fold_total.shape[0]
        if fold_of_row.shape[0] != self.n_local:
            raise ValueError(f"{fold_of_row.shape[0]} fold labels for {self.n_local} local rows")
        if len(inits) != K or any(len(f) != a for f in inits):
            raise ValueError(f"starting values: one list of {a} per fold ({K} folds)")
        ths = [Theta(np.reshape(t["W"], (p, 1)), np.reshape(t["C"], (q, 1)), float(np.ravel(t["B"])[0]),
                     t["sigE"], t["sigF"], t["sigH"], float(np.ravel(t["sigT"])[0])) for f in inits for t in f]
        arr = (_lib.PplsTheta * (K * a))(*[t.struct() for t in ths])
        rmsep = np.full((K, a), np.nan)
        ncomp = np.zeros(K, dtype=np.int32)
        self._chk(self._L.ppls_cv_ppls(self.h, int(a), int(K), fold_of_row.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                       fold_total.ctypes.data_as(_lib._i64p), int(max_steps), float(atol),
                                       int(bool(crit_abs)), arr, dptr(rmsep), ncomp.ctypes.data_as(ct.POINTER(ct.c_int))))
        return rmsep, ncomp

    def cv_timing(self, reset=True):
        """Phases of the cross-validation calls on this context since the last reset
        (ppls_cv_timing): ms of the row gathers, the held-out Gram + downdate, the fits and the
        scoring kernel, and the bytes the gathers and the scoring kernel moved."""
        out = np.zeros(6)
        self._chk(self._L.ppls_cv_timing(self.h, dptr(out), int(bool(reset))))
        return dict(gather_ms=out[0], downdate_ms=out[1], fit_ms=out[2], score_ms=out[3], gather_bytes=out[4],
                    score_bytes=out[5])

    def synchronize(self):
        self._chk(self._L.ppls_synchronize(self.h))

    def loglC_fast(self, W, C, X, Y, sigX, sigY, sig2T, c1, c2, c3, Kc) -> float:
        W = np.asfortranarray(W, dtype=np.float64)
        C = np.asfortranarray(C, dtype=np.float64)
        a = W.shape[1] if W.ndim == 2 else 1
        vec = [np.ascontiguousarray(np.ravel(v), dtype=np.float64) for v in (sig2T, c1, c2, c3, Kc)]
        out = ct.c_double()
        if X is None:
            n, p, q = self.n_total, self.p, self.q
            xp = yp = None
        else:
            X = np.asfortranarray(X, dtype=np.float64)
            Y = np.asfortranarray(Y, dtype=np.float64)
            n, p = X.shape
            q = Y.shape[1]
            xp, yp = dptr(X), dptr(Y)
            self.p, self.q, self.n_local, self.n_total = p, q, n, n
        self._chk(self._L.ppls_loglC_fast(self.h, dptr(W), dptr(C), xp, yp, int(n), int(p), int(q), int(a),
                                          float(sigX), float(sigY), *[dptr(v) for v in vec],
                                          ct.byref(out)))
        return out.value

    # -- measurement
    def sweep_timing(self, reset=True):
        ms, n = ct.c_double(), ct.c_int64()
        self._chk(self._L.ppls_sweep_timing(self.h, ct.byref(ms), ct.byref(n), int(reset)))
        return ms.value, n.value

    def sweep_balance(self):
        """(weights per XCD class g % 8, row boundaries per workgroup or None) of the split sweep's
        calibrated row partition (option "balance")."""
        w = np.ones(8)
        cap = 4097
        b = np.zeros(cap, dtype=np.int64)
        nb = ct.c_int()
        self._chk(self._L.ppls_sweep_balance(self.h, dptr(w), b.ctypes.data_as(ct.POINTER(ct.c_int64)), cap,
                                             ct.byref(nb)))
        return w, (b[: nb.value].copy() if nb.value else None)

    def comm_info(self, reset=True):
        """(nranks, rank) as RCCL's communicator reports them (ncclCommCount / ncclCommUserRank; the
        context's own values without RCCL) and (total ms, calls) of the timed all-reduces."""
        nr, rk, ms, n = ct.c_int(), ct.c_int(), ct.c_double(), ct.c_int64()
        self._chk(self._L.ppls_comm_info(self.h, ct.byref(nr), ct.byref(rk), ct.byref(ms), ct.byref(n), int(reset)))
        return nr.value, rk.value, ms.value, n.value

    def sweep_trace(self, grid):
        """Per-workgroup wall-clock stamps (us, relative to the earliest entry) of the last split
        sweep: (grid, 4) = entry, ring prologue done, row loop done, partials written."""
        buf = (ct.c_int64 * (4 * grid))()
        n, tick = ct.c_int(), ct.c_double()
        self._chk(self._L.ppls_sweep_trace(self.h, buf, int(grid), ct.byref(n), ct.byref(tick)))
        a = np.array(buf[:4 * n.value], dtype=np.int64).reshape(n.value, 4)
        return (a - a[:, 0].min()) * tick.value / 1e3

    def finalize_trace(self):
        """Phase stamps of the last finalize (set_option('ftrace', 1) first): {block: [us since the
        block's first stamp, ...]} for the slots that were reached."""
        buf = (ct.c_int64 * 48)()
        tick = ct.c_double()
        self._chk(self._L.ppls_finalize_trace(self.h, buf, ct.byref(tick)))
        out = {}
        for b in range(3):
            s = [buf[16 * b + i] for i in range(16)]
            if s[0]:
                us = [round((v - s[0]) * tick.value * 1e-3, 3) if v else None for v in s]
                # 10-12 raw (Jacobi sweeps, core clock stamps); a polar team's member 0 stamps its
                # first barrier in 9 (arrived) and 10 (all arrived)
                out[b] = us[:10] + ([us[10]] if s[10] > 1000 else [s[10]]) + s[11:13] + us[13:]
        return out

    def sweep_info(self, r):
        b, v, g = ct.c_int64(), ct.c_int(), ct.c_int()
        self._chk(self._L.ppls_sweep_info(self.h, int(r), ct.byref(b), ct.byref(v), ct.byref(g)))
        return dict(bytes_per_sweep=b.value, variant={4: "split512", 5: "panel"}[v.value], grid=g.value)

    def meta_info(self):
        """The path the last meta_ppls / meta_ppls_stream took: "none", "host", "device_split",
        "device_panel", "device_xprod" (option meta_xprod) or "device_stream" (a fold stream)."""
        v = ct.c_int()
        self._chk(self._L.ppls_meta_info(self.h, ct.byref(v)))
        return ("none", "host", "device_split", "device_panel", "device_xprod", "device_stream")[v.value]

    def sweep_kernel(self, r):
        """The sweep kernel instantiation an EM iteration with r components launches (text)."""
        buf = ct.create_string_buffer(256)
        self._chk(self._L.ppls_sweep_kernel(self.h, int(r), buf, 256))
        return buf.value.decode()


# ================================================================================ R mirror
_DEFAULT_CTX = None


def default_context() -> Context:
    """The context the R-named functions use when no ``ctx`` is given: GPU 0, with the statistics
    path chosen per run by the cost model (option "xprod" = -1, as the R shim in INTEGRATION.md
    sets it: the cross-product form once a run is long enough to repay forming S).  A formed S
    stays resident for the data (8 (p+q)^2 bytes of HBM: 128 MB at p = q = 2000, 0.9 GB at
    p + q = 10,500) until new data are loaded, ``xprod`` is set to 0, or
    ``default_context().xprod_release()`` frees it."""
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = Context(0)
        _DEFAULT_CTX.set_option("xprod", -1)
    return _DEFAULT_CTX


def _orth_type(type):
    if isinstance(type, (list, tuple)):
        type = type[0]            # match.arg(type) picks the first choice, EM_W_multi.R:761
    if type not in ("SVD", "QR"):
        raise ValueError("'arg' should be one of \"SVD\", \"QR\"")
    return _lib.PPLS_ORTH_SVD if type == "SVD" else _lib.PPLS_ORTH_QR


def _ctx_with(X, Y, ctx):
    ctx = ctx or default_context()
    if X is not None:
        ctx.set_data(X, Y)
    elif ctx.n_local is None:
        raise ValueError("no data: pass X and Y or a context with resident data")
    return ctx


def Expect_M(X, Y, W, C, B, sigE, sigF, sigH, sigT, debug=False, ctx=None):
    """Expect_M (EM_W_multi.R:637-717): posterior first and second moments."""
    if debug:
        raise NotImplementedError("debug=TRUE (dense Sigma^-1, EM_W_multi.R:643-667) is an O(n(p+q)^2) "
                                  "cross-check; it lives in the test oracle, not on the GPU path")
    ctx = _ctx_with(X, Y, ctx)
    th = Theta(W, C, B, sigE, sigF, sigH, sigT)
    return ctx.estep(th, want_mu=True).as_dict()


def Maximiz_M(fit, X, Y, type=("SVD", "QR"), ctx=None):
    """Maximiz_M (EM_W_multi.R:729-742): W = orth(X'mu_T), C = orth(Y'mu_U), scalar updates."""
    ctx = _ctx_with(X, Y, ctx)
    r = np.asarray(fit["Ctt"]).shape[0]
    e = Expect(r, ctx.n_local, True)
    e.mu_T[:] = np.asarray(fit["mu_T"])
    e.mu_U[:] = np.asarray(fit["mu_U"])
    e.Ctt[:] = np.diag(np.asarray(fit["Ctt"]))
    e.Cuu[:] = np.diag(np.asarray(fit["Cuu"]))
    e.Cut[:] = np.diag(np.asarray(fit["Cut"]))
    e.Cee = float(np.trace(np.atleast_2d(fit["Cee"])) / np.atleast_2d(fit["Cee"]).shape[1])
    e.Cff = float(np.trace(np.atleast_2d(fit["Cff"])) / np.atleast_2d(fit["Cff"]).shape[1])
    e.Chh[:] = np.asarray(fit["Chh"])
    th = ctx.mstep(e, _orth_type(type))
    d = th.as_dict()
    return dict(W=d["W"], C=d["C"], B=d["B"], sigE=d["sigE"], sigF=d["sigF"], sigH=d["sigH"], sigT=d["sigT"])


def logl_W(X, Y, W, C, B_T, sigX, sigY, sigH, sigT, ctx=None):
    """logl_W (EM_W_multi.R:297-323)."""
    ctx = _ctx_with(X, Y, ctx)
    W = np.array(W, dtype=np.float64, ndmin=2)
    if W.shape[0] == 1 and ctx.p != 1:
        W = W.T
    C = np.array(C, dtype=np.float64, ndmin=2)
    if C.shape[0] == 1 and ctx.q != 1:
        C = C.T
    return ctx.loglik(Theta(W, C, B_T, sigX, sigY, sigH, sigT))


def loglC_fast(W, C, X, Y, sigX, sigY, sig2T, c1, c2, c3, Kc, ctx=None):
    """loglC_fast (src/loglC.cpp:318-338) -- the drop-in of .Call('PPLS_loglC_fast', ...)."""
    ctx = ctx or default_context()
    return ctx.loglC_fast(W, C, X, Y, sigX, sigY, sig2T, c1, c2, c3, Kc)


def random_theta0(p, q, a, seed=0):
    """Deterministic synthetic theta0: W0 = orth(N(0,1)), C0 = orth(N(0,1)), B0 = I, sigT0 = I,
    sigmas = 1 (the benchmark's starting point).  PPLS_simult's own default theta0 is
    the sequential fit PPLS(X, Y, a, 20, 1e-4, 'random') (EM_W_multi.R:762-771), which
    ``PPLS_simult`` below runs on the device."""
    rng = np.random.default_rng(seed)

    def polar(M):
        U, _, Vt = np.linalg.svd(M, full_matrices=False)
        return U @ Vt

    return dict(W=polar(rng.standard_normal((p, a))), C=polar(rng.standard_normal((q, a))),
                B=np.eye(a), sigE=1.0, sigF=1.0, sigH=1.0, sigT=np.eye(a))


def initial_guess(p, q, kind="equal", rng=None):
    """PPLSi's starting values (EM_W_multi.R:126-140): 'equal' (deterministic) or 'random' --
    orth(runif(p)), orth(runif(q)), rchisq(1,1), rchisq(2,100)/100 (sigH, sigT), rchisq(2,10)/100
    (sigE, sigF), drawn in that order (:133).

    ``rng``: an R-compatible stream (any object with R's ``runif(n)`` and ``rchisq(n, df)``, e.g. a
    restatement of R's Mersenne-Twister/Inversion defaults) reproduces R's draws after the same
    ``set.seed``; a numpy ``Generator`` draws from the same distributions.  ``orth`` of a positive
    vector is taken as v/||v|| (the QR form's -v/||v|| gives the mirrored, equivalent fit).
    'o2m' depends on the data: PPLS / PPLSi / meta_PPLSi compute it (o2m_guess_from_gram)."""
    if kind == "equal":
        return dict(W=np.ones(p) / np.sqrt(p), C=np.ones(q) / np.sqrt(q), B=1.0, sigE=1.0 / p,
                    sigF=1.0 / q, sigH=1.0, sigT=1.0)
    if kind == "random":
        rng = rng if rng is not None else np.random.default_rng()
        if hasattr(rng, "runif") and hasattr(rng, "rchisq"):      # R's own stream
            W = np.asarray(rng.runif(p), dtype=np.float64)
            C = np.asarray(rng.runif(q), dtype=np.float64)
            B = float(np.ravel(rng.rchisq(1, 1))[0])
            siglat = np.asarray(rng.rchisq(2, 100), dtype=np.float64) / 100
            sig = np.asarray(rng.rchisq(2, 10), dtype=np.float64) / 100
        else:
            W = rng.uniform(size=p)
            C = rng.uniform(size=q)
            B = rng.chisquare(1)
            siglat = rng.chisquare(100, size=2) / 100
            sig = rng.chisquare(10, size=2) / 100
        return dict(W=W / np.linalg.norm(W), C=C / np.linalg.norm(C), B=float(B), sigE=float(sig[0]),
                    sigF=float(sig[1]), sigH=float(siglat[0]), sigT=float(siglat[1]))
    if kind in ("o2m", "o2m_xprod"):
        raise ValueError(f"initialGuess={kind!r} depends on the data: PPLS / PPLSi / meta_PPLSi compute it "
                         "(o2m_guess_from_gram)")
    raise ValueError(f"unknown initialGuess {kind!r}")


def o2m_guess_from_gram(G, N, p, q, Wprev=None, Cprev=None):
    """PPLSi's 'o2m' starting values (EM_W_multi.R:126-131; meta_PPLSi :520-525) from the joint Gram
    G = [X Y]'[X Y] ((p + q) x (p + q), Context.gram(2)) of N rows, for the data PPLS deflated by the
    earlier components' loadings Wprev (p x k), Cprev (q x k): Xc = X P_1 ... P_k, P_j = I - w_j w_j'
    (:270-271, sequentially, as the reference does).  o2m(Xc, Yc, 1, 0, 0) of OmicsPLS (not vendored,
    no version pinned) with no orthogonal parts: W., C. = the first singular pair of Xc'Yc (LAPACK on
    the host, p x q: _top_singular_pair), Tt = Xc W., U = Yc C., B = Tt'U / Tt'Tt -- every sum of squares
    and product read off G (ssq(Tt) = z'X'Xz with z = P_1 ... P_k W.), so no pass over the rows.
    Returns the starting-value dict (W, C, B, sigE, sigF, sigH, sigT).  Parity unpinned against R
    (no reference file holds an o2m fit); checked against the oracle's restatement on the explicit
    deflated data (tests/test_o2m_host.py, tests/test_gpu_o2m.py)."""
    G = np.asarray(G, dtype=np.float64)
    Gxx, Gyy, Gxy = G[:p, :p], G[p:, p:], G[:p, p:]
    Wp = np.zeros((p, 0)) if Wprev is None else np.asarray(Wprev, dtype=np.float64).reshape(p, -1)
    Cp = np.zeros((q, 0)) if Cprev is None else np.asarray(Cprev, dtype=np.float64).reshape(q, -1)
    M = Gxy.copy()                          # Xc'Yc = P_k ... P_1 X'Y Q_1 ... Q_k
    for j in range(Wp.shape[1]):
        M -= np.outer(Wp[:, j], Wp[:, j] @ M)
    for j in range(Cp.shape[1]):
        M -= np.outer(M @ Cp[:, j], Cp[:, j])

    def chain(Vp, v):                       # P_1 ... P_k v
        for j in reversed(range(Vp.shape[1])):
            v = v - Vp[:, j] * (Vp[:, j] @ v)
        return v

    def ssq_deflated(Gd, Vp):               # ssq(D P_1 ... P_k): ssq(A P) = ssq(A) - (2 - w'w) ||A w||^2
        t = float(np.trace(Gd))
        for j in range(Vp.shape[1]):
            z = chain(Vp[:, :j], Vp[:, j])  # A_{j-1} w_j = D z
            t -= (2.0 - float(Vp[:, j] @ Vp[:, j])) * float(z @ Gd @ z)
        return t

    w, c = _top_singular_pair(M)
    zx, zy = chain(Wp, w), chain(Cp, c)
    sst, ssu, tu = float(zx @ Gxx @ zx), float(zy @ Gyy @ zy), float(zx @ Gxy @ zy)
    B = tu / sst
    ssx, ssy = ssq_deflated(Gxx, Wp), ssq_deflated(Gyy, Cp)
    return dict(W=w, C=c, B=B, sigE=float(np.sqrt((ssx - sst) / N / p)), sigF=float(np.sqrt((ssy - ssu) / N / q)),
                sigH=float(np.sqrt((ssu - B * B * sst) / N)), sigT=float(np.sqrt(sst / N)))


def _top_singular_pair(M):
    """The first singular pair of M (p x q) from the top eigenvector of the smaller of M'M, MM'
    (LAPACK's MRRR for that one pair: 0.3 s at 2000 x 2000 against 2.5 s for a whole svd), the
    other side as M v / ||M v||.  Its sign is LAPACK's, as the reference's svd's is."""
    import scipy.linalg
    p, q = M.shape
    if q <= p:
        _, v = scipy.linalg.eigh(M.T @ M, subset_by_index=[q - 1, q - 1])
        c = v[:, 0]
        w = M @ c
        return w / np.linalg.norm(w), c
    _, v = scipy.linalg.eigh(M @ M.T, subset_by_index=[p - 1, p - 1])
    w = v[:, 0]
    c = M.T @ w
    return w, c / np.linalg.norm(c)


def _ppls_o2m(ctx, a, steps, atol, constraints, crit_abs):
    """PPLS with 'o2m' starting values: component i starts from o2m of the data deflated by the
    fitted components 1 .. i-1 (:256-257 with :126-131), read off the joint Gram.  The device learns
    component i in a fit of i components whose first i - 1 are fixed (fconstraint, all seven values)
    to their fitted values -- the same deflation, each fixed component one EM step (its increment is
    exactly 0) -- and the result is assembled from those fits (ctx.ppls's dict)."""
    G = _joint_gram(ctx)
    p, q = ctx.p, ctx.q
    keys = ("W", "C", "B", "sig", "not_monotone")
    acc = {k: [] for k in keys}
    oo = {k: [] for k in ("Last_increment", "Number_steps", "Loglikelihoods", "logvalue")}
    inits, fixed = [], []
    Wp = Cp = None
    for i in range(a):
        inits.append(o2m_guess_from_gram(G, ctx.n_total, p, q, Wp, Cp))
        cons = fixed + [None if constraints is None else constraints[i]]
        f = ctx.ppls(i + 1, steps, atol, inits, cons, crit_abs)
        if f["ncomp"] < i + 1:   # :258-263: the fit stops at this component
            break
        for k in ("W", "C"):
            acc[k].append(f[k][:, i].copy())
        acc["B"].append(f["B"][i])
        acc["sig"].append(f["sig"][i].copy())
        acc["not_monotone"].append(f["not_monotone"][i])
        for k in ("Last_increment", "Number_steps", "Loglikelihoods"):
            oo[k].append(f["Other_output"][k][i])
        oo["logvalue"].append(f["Other_output"]["logvalue"][i])
        s = f["sig"][i]
        fixed.append(dict(W=f["W"][:, i].copy(), C=f["C"][:, i].copy(), B=f["B"][i], sigE=s[0], sigF=s[1],
                          sigH=s[2], sigT=s[3]))
        inits[i] = dict(fixed[i])
        Wp, Cp = f["W"], f["C"]
    k = len(acc["B"])
    return dict(W=np.array(acc["W"]).T.reshape(p, k), C=np.array(acc["C"]).T.reshape(q, k), B=np.array(acc["B"]),
                sig=np.array(acc["sig"]).reshape(k, 4),
                Other_output=dict(Last_increment=np.array(oo["Last_increment"]),
                                  Number_steps=np.array(oo["Number_steps"], dtype=np.int32),
                                  Loglikelihoods=np.array(oo["Loglikelihoods"]), logvalue=oo["logvalue"]),
                not_monotone=acc["not_monotone"], ncomp=k)


def _joint_gram(ctx):
    if ctx.streamed:
        raise NotImplementedError("initialGuess='o2m' on a streamed context: the rows were streamed and are not "
                                  "resident, and the joint Gram of raw rows is not kept; use 'equal', 'random' "
                                  "or 'custom'")
    if ctx.n_local != ctx.n_total:
        raise NotImplementedError("initialGuess='o2m' on row shards: all-reduce the ranks' Context.gram(2) "
                                  "and call o2m_guess_from_gram")
    G, _ = ctx.gram(2)
    return G


def fconstraint(constraints=None):
    """fconstraint (EM_W_multi.R:85-92): the seven named constraints W, C, B, sigE, sigF, sigH, sigT;
    None = estimated, a number (or vector for W, C) = fixed."""
    out = dict(W=None, C=None, B=None, sigE=None, sigF=None, sigH=None, sigT=None)
    for k, v in (constraints or {}).items():
        if k in out:
            out[k] = v
    return out


def _crit_abs(critfunc):
    if critfunc is None or getattr(critfunc, "__name__", "") == "identity":
        return False
    if critfunc in (abs, np.abs, np.fabs):
        return True
    raise NotImplementedError("critfunc must be the identity (default) or abs")


def PPLS(X, Y, nr_comp=1, EMsteps=100, atol=1e-4, initialGuess=("equal", "o2m", "random", "custom", "o2m_xprod"),
         customGuess=None, critfunc=None, constraints=None, rng=None, ctx=None):
    """PPLS (EM_W_multi.R:229-279) on the GPU: nr_comp sequential rank-1 EM fits on deflated data.
    Same return list (W, C, B, sig, Other_output); class "PPLS".  customGuess: one dict (used for
    every component, as in R) or a list of per-component dicts; critfunc: identity (default) or abs;
    constraints: None or a list of nr_comp fconstraint(...) dicts (:230, :255).

    ``initialGuess="o2m_xprod"`` takes the 'o2m' starts from the cross-products S on the
    device and fits every component once; it also runs where S is all the context holds.  On a resident
    context without S the call forms S first (one MFMA Gram pass over the rows; about 0.23 s at n = 1e6,
    p = q = 2000) and leaves it on the context -- 8 (p + q)^2 bytes of device memory, 128 MB there,
    925 MB at p = 1e4, q = 500 -- until ``ctx.xprod_release()`` or new data; with option ``xprod`` = 1
    or -1 the fits share that S."""
    ctx = _ctx_with(X, Y, ctx)
    kind = initialGuess if isinstance(initialGuess, str) else initialGuess[0]
    if customGuess is not None:
        kind = "custom"
    if constraints is not None and len(constraints) != nr_comp:
        raise ValueError("There should be a list of constraints for each component, see ?PPLS.")   # :240
    if kind == "custom":
        inits = list(customGuess) if isinstance(customGuess, (list, tuple)) else [customGuess] * nr_comp
    elif kind == "o2m":
        out = _ppls_o2m(ctx, int(nr_comp), int(EMsteps), float(atol), constraints, _crit_abs(critfunc))
        return _ppls_finish(out, nr_comp)
    elif kind == "o2m_xprod":   # the same starts from the cross-products S on the device, each component fitted once
        return _ppls_finish(ctx.ppls_o2m(int(nr_comp), int(EMsteps), float(atol), constraints, _crit_abs(critfunc)),
                            nr_comp)
    else:
        rng = rng if rng is not None else np.random.default_rng()
        inits = [initial_guess(ctx.p, ctx.q, kind, rng) for _ in range(nr_comp)]
    return _ppls_finish(ctx.ppls(int(nr_comp), int(EMsteps), float(atol), inits, constraints, _crit_abs(critfunc)),
                        nr_comp)


def _ppls_finish(out, nr_comp):
    if out["ncomp"] < nr_comp:
        warnings.warn(f"From component {out['ncomp'] + 1} on the residuals are of rank < 1e-14 and "
                      "calculations are stopped.")
    for k, bad in enumerate(out.pop("not_monotone")):
        if bad:
            warnings.warn(f"Not monotone (component {k + 1})")
    out.pop("ncomp")
    out["class"] = "PPLS"
    return out


def PPLSi(X, Y, EMsteps=100, atol=1e-4, initialGuess=("equal", "o2m", "random", "custom", "o2m_xprod"),
          customGuess=None, critfunc=None, constraints=None, rng=None, ctx=None):
    """PPLSi (EM_W_multi.R:116-180): one direction; returns W, C, B, sig, logvalue, Last_increment,
    Number_steps (W = NA when sigE or sigF collapse, :152-154).  constraints: one fconstraint dict."""
    fit = PPLS(X, Y, 1, EMsteps, atol, initialGuess, customGuess, critfunc,
               None if constraints is None else [constraints], rng, ctx)
    if len(fit["B"]) == 0:
        return dict(W=None, C=None, B=None, sig=None, logvalue=None, Last_increment=None, Number_steps=None)
    oo = fit["Other_output"]
    return dict(W=fit["W"][:, 0], C=fit["C"][:, 0], B=fit["B"][0], sig=fit["sig"][0],
                logvalue=oo["logvalue"][0], Last_increment=oo["Last_increment"][0],
                Number_steps=int(oo["Number_steps"][0]))


def _signif(x, digits):
    if x == 0 or not np.isfinite(x):
        return x
    return round(x, digits - 1 - int(np.floor(np.log10(abs(x)))))


def print_PPLS(x, perc=True, digits=3):
    """print.PPLS (EM_W_multi.R:336-354): the per-component variance table of a PPLS fit.
    Returns (rows, text): rows = n x 7 array (LV, ssq(T)/ssq(X), ssq(U)/ssq(Y), sigH^2/ssq(U),
    log LR, #steps, last incr) rounded to ``digits``; ``perc=False`` gives the absolute variances.
    As in R, sigH^2 is added once per component inside the ssq(U) sum."""
    p, q = x["W"].shape[0], x["C"].shape[0]
    sig, B, oo = np.asarray(x["sig"]), np.asarray(x["B"]), x["Other_output"]
    ll = np.asarray(oo["Loglikelihoods"], dtype=np.float64)
    dll = np.concatenate([[0.0], np.diff(ll)])
    pc = 1.0 if perc else 0.0
    rows = []
    for i in range(sig.shape[0]):
        st = float(np.sum(sig[: i + 1, 3] ** 2))
        su = float(np.sum(sig[: i + 1, 3] ** 2 * B[: i + 1] ** 2 + sig[i, 2] ** 2))
        rows.append([i + 1, st / (pc * (st + p * sig[i, 0] ** 2) + (1 - pc)),
                     su / (pc * (su + q * sig[i, 1] ** 2) + (1 - pc)),
                     sig[i, 2] ** 2 / (pc * su + (1 - pc)), dll[i], float(oo["Number_steps"][i]),
                     _signif(float(oo["Last_increment"][i]), 3)])
    rows = np.round(np.array(rows, dtype=np.float64), digits)
    names = ["LV", "ssq(T)/ssq(X)" if perc else "ssq(T)", "ssq(U)/ssq(Y)" if perc else "ssq(U)",
             "sigH^2/ssq(U)" if perc else "sigH^2", "log LR", "#steps", "last incr"]
    text = "  ".join(names) + "\n" + "\n".join(
        "  ".join(f"{v:g}" for v in row) for row in rows)
    return rows, text


def scores_PPLS(fit, X, Y, subset=None, ctx=None):
    """scores.PPLS (EM_W_multi.R:411-420): rbind(X W[, subset], Y C[, subset]) (a vector when one
    component is selected); X W and Y C are computed on the GPU in one pass.  ``fit``: a PPLS list
    (W, C) or a PPLS_simult list (estimates$W, estimates$C)."""
    ctx = _ctx_with(X, Y, ctx)
    est = fit.get("estimates", fit)
    W, C = np.asarray(est["W"]), np.asarray(est["C"])
    cols = list(range(W.shape[1])) if subset is None else [int(s) - 1 for s in np.atleast_1d(subset)]
    T, U = ctx.scores(W[:, cols], C[:, cols])
    if len(cols) == 1:
        return np.concatenate([T[:, 0], U[:, 0]])
    return np.vstack([T, U])


def PPLS_to_o2m(X_true, Y_true, fit_PPLS, ctx=None):
    """PPLS_to_o2m (PPLS_to_o2m.R:28-80): a sequential PPLS fit as an OmicsPLS "o2m" list.  The
    scores Tt = X W, U = Y C come from one device pass (ppls_scores); ssq(X), ssq(Y) from the
    context; ssq(U B_U W'), ssq(Tt B_T C') are evaluated as r x r traces (no n x p product)."""
    ctx = _ctx_with(X_true, Y_true, ctx)
    W = np.asarray(fit_PPLS["W"], dtype=np.float64).reshape(ctx.p, -1)
    C = np.asarray(fit_PPLS["C"], dtype=np.float64).reshape(ctx.q, -1)
    b = np.ravel(np.asarray(fit_PPLS["B"], dtype=np.float64))
    B_T = np.diag(b)                                          # diag(fit_PPLS$B, length(fit_PPLS$B)) (:33)
    B_U = np.linalg.inv(B_T)                                  # solve(B_T) (:34)
    Tt, U = ctx.scores(W, C)                                  # :35-36
    n = Tt.shape[0]
    ssqX, ssqY = ctx.ssq()                                    # :44-45

    def ssq(A):
        A = np.asarray(A, dtype=np.float64)
        return float(np.sum(A * A))

    def ssq_prod(S, M, L):   # ssq(S M L') = tr(M' S'S M L'L)
        return float(np.trace(M.T @ (S.T @ S) @ M @ (L.T @ L)))
    R2Xcorr, R2Ycorr = ssq(Tt) / ssqX, ssq(U) / ssqY          # :47-48
    R2Xhat = ssq_prod(U, B_U, W) / ssqX                       # :51
    R2Yhat = ssq_prod(Tt, B_T, C) / ssqY                      # :52
    z = lambda r, c: np.zeros((r, c))
    model = dict(Tt=Tt, U=U, W_=W, C_=C, P_Yosc_=z(W.shape[0], 1), P_Xosc_=z(C.shape[0], 1),
                 T_Yosc_=z(n, 1), U_Xosc_=z(n, 1), W_Yosc=z(W.shape[0], 1), C_Xosc=z(C.shape[0], 1),
                 B_T_=B_T, B_U=B_U, H_TU=0 * Tt, H_UT=U - Tt @ B_T,
                 R2X=R2Xcorr + 0.0, R2Y=R2Ycorr + 0.0, R2Xcorr=R2Xcorr, R2Ycorr=R2Ycorr, R2Xhat=R2Xhat,
                 R2Yhat=R2Yhat)                               # :60-64 (R2X_YO = R2Y_XO = 0)
    model["flags"] = dict(time=float("nan"), n=W.shape[1], nx=0, ny=0, stripped=True, highd=False, ssqX=ssqX,
                          ssqY=ssqY, varXjoint=np.sum(Tt * Tt, axis=0), varYjoint=np.sum(U * U, axis=0),
                          varXorth=np.zeros(1), varYorth=np.zeros(1))
    model["class"] = ["o2m", "o2m_stripped"]
    return model


def PPLS_simult_to_o2m(X_true, Y_true, fit_PPLS, ctx=None):
    """PPLS_simult_to_o2m (PPLS_to_o2m.R:82-140): the fit as an OmicsPLS "o2m" list.  Host-side
    bookkeeping on the fit's Expectations (mu_T, mu_U from the device Eout) and estimates; the
    only data terms, ssq(X) and ssq(Y), come from the context (computed on the device at load)."""
    ctx = _ctx_with(X_true, Y_true, ctx)
    est, E = fit_PPLS["estimates"], fit_PPLS["Expectations"]
    W, C = np.asarray(est["W"]), np.asarray(est["C"])
    r = W.shape[1]
    B_T = np.asarray(est["B"])
    Tt, U = np.asarray(E["mu_T"]), np.asarray(E["mu_U"])
    p, q = W.shape[0], C.shape[0]
    sT, B = np.asarray(est["sigT"]), np.asarray(est["B"])
    sE, sF, sH = float(est["sigE"]), float(est["sigF"]), float(est["sigH"])

    def ssq(A):
        A = np.asarray(A, dtype=np.float64)
        return float(np.sum(A * A))
    ssqX, ssqY = ctx.ssq()
    R2Xcorr = ssq(sT @ sT) / (ssq(sT @ sT) + p * sE ** 2)
    v = sT @ sT @ B @ B + np.diag(np.full(r, sH ** 2))
    R2Ycorr = ssq(v) / (ssq(v) + q * sF ** 2)
    R2Yhat = ssq(sT @ sT @ B) / (ssq(sT @ sT @ B @ B) + r * sH ** 2 + q * sF ** 2)
    P_Yosc = np.zeros((p, 1))
    P_Xosc = np.zeros((q, 1))
    model = dict(Tt=Tt, U=U, W_=W, C_=C, P_Yosc_=P_Yosc, P_Xosc_=P_Xosc, T_Yosc_=np.zeros((Tt.shape[0], 1)),
                 U_Xosc_=np.zeros((Tt.shape[0], 1)), W_Yosc=np.zeros((p, 1)), C_Xosc=np.zeros((q, 1)),
                 B_T_=B_T, B_U=np.linalg.inv(B_T), H_TU=0 * Tt, H_UT=U - Tt @ B_T,
                 R2X=R2Xcorr + 0, R2Y=R2Ycorr + 0, R2Xcorr=R2Xcorr, R2Ycorr=R2Ycorr, R2Xhat=float("nan"),
                 R2Yhat=R2Yhat)
    model["flags"] = dict(time=float("nan"), n=r, nx=0, ny=0, stripped=True, highd=False, ssqX=ssqX, ssqY=ssqY,
                          varXjoint=np.sum(Tt * Tt, axis=0), varYjoint=np.sum(U * U, axis=0),
                          varXorth=np.zeros(1), varYorth=np.zeros(1))
    model["class"] = ["o2m", "o2m_stripped"]
    return model


def _populations(Ipopu, n):
    """as.factor(Ipopu) -> level counts in level order (table(Ipopu)); R sorts the levels."""
    Ipopu = np.asarray(Ipopu)
    if Ipopu.ndim != 1 or Ipopu.shape[0] != n:
        raise ValueError("nrow(X) == length(Ipopu) is not TRUE")   # stopifnot (:448, :511)
    levels, counts = np.unique(Ipopu, return_counts=True)
    return levels, counts.astype(np.int64)


def population_labels(Ipopu):
    """``(labels int32, levels)``: every row's population as 0 .. K-1 in R's level order
    (as.factor(Ipopu), the order of ``_populations``) -- the third element of each chunk triple when
    the rows of a multi-population fit are streamed with ``stream_data(..., nr_folds=K)``.  Compute it
    from all labels at once (or pass the chunks' labels through the same ``levels``), so that every
    chunk uses the same numbering."""
    Ipopu = np.asarray(Ipopu)
    if Ipopu.ndim != 1:
        raise ValueError("Ipopu must be a vector")
    levels, inv = np.unique(Ipopu, return_inverse=True)
    return np.ascontiguousarray(inv, dtype=np.int32), levels


def rank1_mu_coefficients(params):
    """``K x 4`` (alpha, beta, gamma, delta) for ``params`` (K x 5: B_T, sigX, sigY, sigH, sigT), as
    the library stages them for a rank-1 or meta statistics pass (ppls_rank1_mu_coefficients; host
    only, no GPU)."""
    P = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, 5))
    out = np.zeros((P.shape[0], 4))
    L = _lib.lib()
    for j in range(P.shape[0]):
        if L.ppls_rank1_mu_coefficients(dptr(P[j]), dptr(out[j])) != 0:
            raise ValueError("ppls_rank1_mu_coefficients failed")
    return out


def _meta_streamed(ctx, X, Ipopu):
    """Whether a meta_* call runs on a fold stream's populations (and may: no Ipopu there)."""
    if X is not None or ctx is None or not ctx.streamed or not ctx._stream_folds:
        return False
    if Ipopu is not None:
        raise ValueError("Ipopu cannot be given: the populations are the labels the rows were streamed with")
    return True


def _params_list(levels, P):
    return [dict(B_T=float(P[j, 0]), sigX=float(P[j, 1]), sigY=float(P[j, 2]), sigH=float(P[j, 3]),
                 sigT=float(P[j, 4])) for j in range(len(levels))]


def _params_matrix(params):
    return np.array([[float(np.ravel(pp[k])[0]) for k in ("B_T", "sigX", "sigY", "sigH", "sigT")]
                     for pp in params])


def meta_EMstep(X, Y, W, C, Ipopu, params, ctx=None):
    """meta_EMstep (EM_W_multi.R:446-485) on the GPU: one EM step of the multi-population rank-1
    model.  ``params``: one dict per population (B_T, sigX, sigY, sigH, sigT), in level order.
    Returns the reference's list: per population dict(B, sighat, siglathat, Cxt, Cyu), plus
    ``W.`` and ``C.`` (shared loadings, orth of the sign-aligned sums, :481-482).

    ``meta_EMstep(None, None, W, C, None, params, ctx=ctx)`` on a context streamed with
    ``stream_data(..., nr_folds=K)`` runs on the stream's labels as populations, from their
    cross-products (ppls_meta_emstep_stream); passing an ``Ipopu`` there raises ``ValueError``."""
    if _meta_streamed(ctx, X, Ipopu):
        levels = np.arange(ctx._stream_folds)
        if len(params) != len(levels):
            raise ValueError(f"{len(params)} parameter sets for {len(levels)} populations")
        Wo, Co, P, cxt, cyu = ctx.meta_emstep_stream(W, C, _params_matrix(params))
    else:
        ctx = _ctx_with(X, Y, ctx)
        levels, counts = _populations(Ipopu, ctx.n_total)
        if len(params) != len(levels):
            raise ValueError(f"{len(params)} parameter sets for {len(levels)} populations")
        Wo, Co, P, cxt, cyu = ctx.meta_emstep(W, C, counts, _params_matrix(params))
    out = [dict(B=P[j, 0], sighat=P[j, 1:3].copy(), siglathat=P[j, 3:5].copy(), Cxt=cxt[:, j].copy(),
                Cyu=cyu[:, j].copy()) for j in range(len(levels))]
    return dict(pops=out, **{"W.": Wo.reshape(-1, 1), "C.": Co.reshape(-1, 1)})


def meta_PPLSi(X, Y, Ipopu, EMsteps=100, atol=1e-4, initialGuess=("equal", "o2m", "random", "custom", "o2m_xprod"),
               customGuess=None, critfunc=None, constraints=None, rng=None, ctx=None):
    """meta_PPLSi (EM_W_multi.R:509-589) on the GPU: a rank-1 PPLS fit with loadings shared across
    populations and per-population scalars.  Returns the reference's list (W, C, params, log) where
    ``log`` is logvalue[1:i+1, ] (rows 2..i+1 of the trace: the per-population log-likelihoods after
    each step; kept 2-D) and, additionally, ``logvalue`` (the full trace incl. the initial row).
    critfunc: None/identity or abs.  constraints: dict with numeric "W" / "C" (the only constraints
    the reference applies, :543-544).

    ``meta_PPLSi(None, None, None, ..., ctx=ctx)`` on a context streamed with
    ``stream_data(chunks, nr_folds=K)`` -- chunks of ``(X, Y, labels)`` with the labels of
    ``population_labels`` -- fits the stream's K populations from their cross-products
    (ppls_meta_ppls_stream): data larger than device memory, no rows resident; ``params`` are in label
    order 0 .. K-1.  Passing an ``Ipopu`` there raises ``ValueError``, and ``initialGuess="o2m"`` stays
    refused on streamed contexts; ``"o2m_xprod"`` takes the same start from the cross-products of all
    rows on the device (``Context.o2m_start``), resident or streamed.  One population cannot be streamed this way (a fold stream needs
    K >= 2): ``PPLSi`` on a plain stream is that fit."""
    streamed = _meta_streamed(ctx, X, Ipopu)
    if streamed:
        levels, counts = np.arange(ctx._stream_folds), None
    else:
        ctx = _ctx_with(X, Y, ctx)
        levels, counts = _populations(Ipopu, ctx.n_total)
    kind = initialGuess if isinstance(initialGuess, str) else initialGuess[0]
    if customGuess is not None:
        kind = "custom"
    if kind == "custom":
        g = customGuess
        init = dict(W=np.ravel(g["W"]), C=np.ravel(g["C"]), B=g["B"], sigE=g["sigE"], sigF=g["sigF"],
                    sigH=g["sigH"], sigT=g["sigT"])
    elif kind == "o2m":
        init = o2m_guess_from_gram(_joint_gram(ctx), ctx.n_total, ctx.p, ctx.q)   # :520-525
    elif kind == "o2m_xprod":   # :520-525 from the cross-products of all rows (a fold stream: selection -1)
        if streamed and ctx.stream_fold_info()["selected"] != -1:
            ctx.stream_select(-1)
        init = ctx.o2m_start()
    else:
        init = initial_guess(ctx.p, ctx.q, kind, rng if rng is not None else np.random.default_rng())
    if constraints:
        if constraints.get("W") is not None:
            init["W"] = np.ravel(np.asarray(constraints["W"], dtype=np.float64))
        if constraints.get("C") is not None:
            init["C"] = np.ravel(np.asarray(constraints["C"], dtype=np.float64))
    if critfunc is None or critfunc is (lambda x: x) or getattr(critfunc, "__name__", "") == "identity":
        crit_abs = False
    elif critfunc in (abs, np.abs):
        crit_abs = True
    else:
        raise NotImplementedError("critfunc must be the identity (default) or abs")
    if streamed:
        W, C, P, lg = ctx.meta_ppls_stream(int(EMsteps), float(atol), init, crit_abs)
    else:
        W, C, P, lg = ctx.meta_ppls(counts, int(EMsteps), float(atol), init, crit_abs)
    return dict(W=W, C=C, params=_params_list(levels, P), log=lg[1:], logvalue=lg)


def variances_PPLS_simult(fit, data, XorY=("X", "Y"), ctx=None, full=True, from_xprod=False):
    """variances.PPLS_simult (EM_W_multi.R:830-860) on the GPU: asymptotic standard errors of the
    loadings.  ``fit``: a PPLS_simult list (Expectations, estimates); ``data``: X (XorY = "X") or Y
    (XorY = "Y"), or None to use the context's resident X / Y.  Returns the reference's list: per
    component dict(B_exp, SSt_exp, SSt_star), then varMatrix (list of p x p) and seLoad (p x a);
    full=False skips the p x p B_exp / SSt_exp / SSt_star matrices (B_exp is then its scalar).
    The reference's t(X) %*% diag(Ctt, N) %*% X is Ctt X'X, computed once on MFMA; like the reference
    it uses estimates$sigE for XorY = "Y" as well.

    ``from_xprod=True`` (``data`` must be None): everything comes from the cross-products S that
    ``ctx`` holds (``Context.variances_xprod``), so it also serves a context without rows -- streamed,
    a fold stream's selection, a bootstrap replicate of ``xprod_resample``.  The Expectations are
    recomputed at ``fit["estimates"]`` on S (``fit["Expectations"]`` is not read), and the result
    carries the ``Ctt`` (or Cuu) diagonal used as well.  Two differences from the reference's call on
    its own fit follow from that:
      - the components come in the order of ``estimates``; the reference orders them as its
        Expectations, i.e. as the last iterate before the final rotLoad reordering;
      - the reference's final sign step flips W, C and B together, which is not a symmetry of the
        model, so where it flipped a component (a negative sigT B at the last iterate) the result is
        that of the flipped theta, not the reference's."""
    if isinstance(XorY, (list, tuple)):
        raise ValueError("the condition has length > 1")   # if(XorY=="X") with the default c("X","Y")
    if XorY not in ("X", "Y"):
        return None                                        # neither branch: W undefined in R
    xory = 0 if XorY == "X" else 1
    if from_xprod:
        if data is not None:
            raise ValueError("from_xprod=True reads the context's cross-products: data must be None")
        c = ctx or default_context()
        e = fit["estimates"]
        th = Theta(e["W"], e["C"], e["B"], e["sigE"], e["sigF"], e["sigH"], e["sigT"])
        W, Cd, Bx, V, se, SE, SS = c.variances_xprod(th, xory, full)
        p = W.shape[0]
        comps = [dict(B_exp=(Bx[i] * np.eye(p) if full else float(Bx[i])),
                      SSt_exp=(SE[i] if full else None), SSt_star=(SS[i] if full else None)) for i in range(len(Bx))]
        return dict(components=comps, varMatrix=[V[i] for i in range(len(Bx))], seLoad=se, W=W, Ctt=np.diag(Cd))
    E = fit["Expectations"]
    mu = np.asarray(E["mu_T"] if xory == 0 else E["mu_U"])
    Cd = np.diag(np.asarray(E["Ctt"] if xory == 0 else E["Cuu"]))
    sigE = float(np.ravel(fit["estimates"]["sigE"])[0])
    own = None
    if data is not None:
        D = np.asarray(data, dtype=np.float64)
        own = Context(0) if ctx is None else ctx
        dummy = np.zeros((D.shape[0], 1))
        own.set_data(D, dummy) if xory == 0 else own.set_data(dummy, D)
        c = own
    else:
        c = ctx or default_context()
    try:
        W, Bx, V, se, SE, SS = c.variances(mu, Cd, sigE, xory, full)
    finally:
        if own is not None and ctx is None:
            own.close()
    p = W.shape[0]
    comps = [dict(B_exp=(Bx[i] * np.eye(p) if full else float(Bx[i])),
                  SSt_exp=(SE[i] if full else None), SSt_star=(SS[i] if full else None)) for i in range(len(Bx))]
    return dict(components=comps, varMatrix=[V[i] for i in range(len(Bx))], seLoad=se, W=W)


def PPLS_simult(X, Y, a, EMsteps=10, atol=1e-4, type=("SVD", "QR"), init=None, ctx=None, **kw):
    """PPLS_simult (EM_W_multi.R:758-807) on the GPU.

    ``init``: dict(W, C, B, sigE, sigF, sigH, sigT) used as theta0.  Default: the reference's own
    f0 = PPLS(X, Y, a, 20, 1e-4, 'random') (:762-770, retried when it raises, up to three times),
    computed on the device; its draws come from ``rng`` (an R-compatible stream, see
    ``initial_guess``) or numpy (``seed`` keyword).  Returns dict(Expectations, loglik, estimates) like
    the R list of class "PPLS_simult"; warns "Negative increments of likelihood" where the
    reference does (:801).  ``timings`` (keyword, a dict): filled with the wall seconds of the
    initialiser (``init``) and of the loop + Expectations (``loop``) and the initialiser's steps.
    """
    if kw.get("debug"):
        raise NotImplementedError("debug=TRUE is an oracle-only cross-check")
    timings = kw.get("timings")   # optional dict: init / loop seconds and the initialiser's steps
    t0 = time.perf_counter()
    ctx = _ctx_with(X, Y, ctx)
    t = _orth_type(type)
    init_steps = []
    if init is None:
        rng = kw.get("rng")
        rng = rng if rng is not None else np.random.default_rng(kw.get("seed"))
        f0, last = None, None
        for _ in range(3):   # f0 = try(PPLS(...)): retried only when PPLS raises (:762-764)
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    f0 = PPLS(None, None, a, 20, 1e-4, "random", rng=rng, ctx=ctx)
                break
            except PplsError as e:
                f0, last = None, e
        if f0 is None:   # R: f0 is a try-error and `f0$W` stops the call (:765)
            raise PplsError(last.code, f"f0 = try(PPLS(X, Y, a, 20, 1e-4, 'random')) failed three times "
                                       f"(EM_W_multi.R:762-765): {last}")
        if len(f0["B"]) < a:
            # R carries the truncated f0 on and fails at W.[, rotLoad] (:773-776)
            raise PplsError(-1, f"subscript out of bounds: PPLS returned {len(f0['B'])} of {a} components")
        init = dict(W=f0["W"], C=f0["C"], B=np.diag(f0["B"]), sigE=f0["sig"][a - 1, 0],
                    sigF=f0["sig"][a - 1, 1], sigH=f0["sig"][a - 1, 2], sigT=np.diag(f0["sig"][:, 3]))
        init_steps = list(f0["Other_output"]["Number_steps"])
    t1 = time.perf_counter()
    th = Theta(init["W"], init["C"], init["B"], init["sigE"], init["sigF"], init["sigH"], init["sigT"])
    if th.r != a:
        raise ValueError(f"init has {th.r} components, a = {a}")
    # streamed context: no rows, so Expectations carries the moments and mu_T = mu_U = None
    est, ll, eout, neg = ctx.em_run(th, int(EMsteps), float(atol), t, want_eout=True, want_mu=not ctx.streamed)
    if neg:
        warnings.warn("Negative increments of likelihood")
    d = est.as_dict()
    estimates = dict(W=d["W"], C=d["C"], B=d["B"], sigE=d["sigE"], sigF=d["sigF"], sigH=d["sigH"],
                     sigT=d["sigT"])
    out = dict(Expectations=eout.as_dict(), loglik=ll, estimates=estimates)
    out["class"] = "PPLS_simult"
    if timings is not None:
        timings.update(init=t1 - t0, loop=time.perf_counter() - t1, init_steps=init_steps)
    return out


# ---------------------------------------------------------------------------- robust fit
def t_nu_grid(lo, hi, m=16):
    """``m`` log-spaced points from ``lo`` to ``hi``, both included."""
    return np.exp(np.linspace(np.log(lo), np.log(hi), int(m)))


def t_nu_bracket(grid, k, lo=1.0, hi=1000.0):
    """The interval the next round of the nu search covers: the neighbours of the best point ``k``."""
    return max(lo, float(grid[max(k - 1, 0)])), min(hi, float(grid[min(k + 1, len(grid) - 1)]))


def robust_PPLS_simult(X, Y, a, nu=4.0, outer=50, inner=5, atol=1e-4, type="SVD", init=None, ctx=None, work=None):
    """PPLS_simult under the multivariate-t model with ``nu`` degrees of freedom, fitted by EM: rows the
    Gaussian fit does not explain are weighted down instead of deciding the answer.

    From theta (``init``: a dict as for PPLS_simult, default the estimates of ``PPLS_simult(X, Y, a)``
    on the same context) the loop repeats: (1) ``ctx.robust_weights`` -- the distances d2_i, the weights
    u_i = (nu + p + q) / (nu + d2_i) and the t log-likelihood at theta; (2) ``work.xprod_weighted(ctx)``
    -- S_u = sum u_i d_i d_i' with ``n_total = N``, not sum u; (3) ``inner`` EM steps of PPLS_simult on
    ``work``, warm-started at theta.  It stops when the t log-likelihood rises by less than ``atol``
    (never tested on the first step) or after ``outer`` iterations.  ``nu="estimate"``: nu is re-chosen
    in step (1) to maximise the t log-likelihood of theta over [1, 1000], by four rounds of a 16-point
    log-spaced grid, each bracketing the previous best point (the ECME step).

    ``X``, ``Y``: the data, centred beforehand (no intercept is fitted), or ``None, None`` with ``ctx``
    holding the rows, ``scale_data`` output included.  ``work``: the context that holds S_u (default: a
    new one on ``ctx``'s device, closed at the end).  Sharded, every rank calls this with its own rows
    and a shared ``init``.

    Returns ``dict(estimates, loglik, nu, weights, d2, steps, converged, gaussian)``: ``estimates``
    canonicalised as PPLS_simult's; ``loglik`` the t log-likelihood at the start and after every outer
    iteration (``steps + 1`` values); ``weights`` and ``d2`` this rank's rows' at the returned estimates;
    ``gaussian`` the starting PPLS_simult fit (None when ``init`` was given)."""
    estimate = isinstance(nu, str)
    if estimate and nu != "estimate":
        raise ValueError("nu must be a positive number or 'estimate'")
    if not estimate and not (np.isfinite(nu) and nu > 0):
        raise ValueError(f"nu = {nu} must be positive and finite")
    if outer < 1 or inner < 1:
        raise ValueError(f"outer = {outer}, inner = {inner} must be at least 1")
    ctx = _ctx_with(X, Y, ctx)
    t = _orth_type(type)
    gauss = None
    if init is None:
        gauss = PPLS_simult(None, None, a, type=type, ctx=ctx)
        init = gauss["estimates"]
    th = Theta(init["W"], init["C"], init["B"], init["sigE"], init["sigF"], init["sigH"], init["sigT"])
    if th.r != a:
        raise ValueError(f"init has {th.r} components, a = {a}")

    def estep(th):
        if not estimate:
            return float(nu), float(ctx.robust_weights(th, nu)[0][0])
        lo, hi = 1.0, 1000.0
        for _ in range(4):
            grid = t_nu_grid(lo, hi)
            k = int(np.argmax(ctx.robust_weights(th, grid)[0]))
            lo, hi = t_nu_bracket(grid, k)
        return float(grid[k]), float(ctx.robust_weights(th, grid[k])[0][0])   # keeps the weights of the chosen nu

    own = work is None
    work = Context(ctx.device) if own else work
    ll, steps, converged = [], 0, False
    try:
        while True:
            nu_k, l = estep(th)
            ll.append(l)
            if len(ll) > 1 and ll[-1] - ll[-2] < atol:
                converged = True
                break
            if steps >= outer:
                break
            work.xprod_weighted(ctx)
            th = work.em_run(th, int(inner), -np.inf, t, want_eout=False, want_mu=False)[0]
            steps += 1
    finally:
        if own:
            work.close()
    w, d2 = ctx.robust_get()
    d = th.as_dict()
    estimates = dict(W=d["W"], C=d["C"], B=d["B"], sigE=d["sigE"], sigF=d["sigF"], sigH=d["sigH"], sigT=d["sigT"])
    out = dict(estimates=estimates, loglik=np.array(ll), nu=nu_k, weights=w, d2=d2, steps=steps, converged=converged,
               gaussian=gauss)
    out["class"] = "robust_PPLS_simult"
    return out


# ---------------------------------------------------------------------------- bootstrap
def bootstrap_counts(N, nboot, rng=None):
    """``nboot`` bootstrap resamples of ``N`` rows as counts: an ``(nboot, N)`` int32 array whose row b
    holds how often each row occurs in replicate b -- ``rng.multinomial(N, rep(1/N, N))``, the counts of
    R's ``sample(N, replace = TRUE)``.  ``rng``: a numpy Generator, or a seed for one."""
    N, nboot = int(N), int(nboot)
    if N < 1 or nboot < 0:
        raise ValueError(f"bootstrap_counts: N = {N}, nboot = {nboot}")
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    pv = np.full(N, 1.0 / N)
    out = np.empty((nboot, N), dtype=np.int32)
    for b in range(nboot):
        out[b] = rng.multinomial(N, pv)
    return out


def align_signs(W, W0):
    """``W`` with each column's sign set so that it points along the same column of ``W0``:
    ``W %*% diag(sign(diag(t(W) %*% W0)))``, a zero inner product counting as +1 -- the alignment the
    reference sketches in its commented mseLoadings (EM_W_multi.R:809-816).  Nothing is reordered."""
    W = np.array(W, dtype=np.float64, ndmin=2)
    W0 = np.array(W0, dtype=np.float64, ndmin=2)
    if W.shape != W0.shape:
        raise ValueError(f"align_signs: shapes {W.shape} and {W0.shape}")
    s = np.sign(np.einsum("ij,ij->j", W, W0))
    s[s == 0] = 1.0
    return W * s


_BOOT_KEYS = ("W", "C", "B", "sigE", "sigF", "sigH", "sigT")


def _boot_value(est, key):
    v = np.asarray(est[key], dtype=np.float64)
    if key in ("B", "sigT"):      # diagonal matrices in the R list: taken as their diagonals
        return np.diag(v).copy() if v.ndim == 2 else np.atleast_1d(v).astype(np.float64)
    if key in ("sigE", "sigF", "sigH"):
        return np.float64(np.ravel(v)[0])
    return v


def bootstrap_summary(replicates, level=0.95):
    """``(se, ci)`` of a list of estimate dicts (W, C, B, sigE, sigF, sigH, sigT): per key the standard
    deviation over the replicates with ``ddof = 1`` and the ``(lo, hi)`` pair of ``np.quantile`` at
    ``(1 - level) / 2`` and ``(1 + level) / 2``; B and sigT enter as their diagonals."""
    if len(replicates) < 2:
        raise ValueError(f"bootstrap: {len(replicates)} replicate(s) succeeded, a standard error needs two")
    if not 0.0 < level < 1.0:
        raise ValueError(f"level = {level} outside (0, 1)")
    se, ci = {}, {}
    for k in _BOOT_KEYS:
        A = np.stack([_boot_value(r, k) for r in replicates])
        se[k] = np.std(A, axis=0, ddof=1)
        ci[k] = (np.quantile(A, (1.0 - level) / 2.0, axis=0), np.quantile(A, (1.0 + level) / 2.0, axis=0))
    return se, ci


def bootstrap_PPLS_simult(fit, X, Y, nboot=200, EMsteps=100, atol=1e-4, type="SVD", init="fit", level=0.95, rng=None,
                          ctx=None, work=None, keep=False, counts=None):
    """Bootstrap standard errors and percentile intervals of a PPLS_simult fit: what users of the
    reference get from ``i = sample(N, replace = TRUE); PPLS_simult(X[i, ], Y[i, ], ...)`` in a loop,
    without copying a row.  Replicate b is the data with row i repeated ``counts[b, i]`` times; its
    cross-products come from the weighted MFMA Gram over the resident rows
    (``work.xprod_resample(ctx, counts[b])``) and the fit reads only them
    (``PPLS_simult(None, None, a, EMsteps, atol, type, init=..., ctx=work)``).

    ``fit``: the PPLS_simult list whose estimates are assessed.  ``X``, ``Y``: the data, or
    ``None, None`` with ``ctx`` holding the rows.  Sharded, every rank calls this with its own rows
    and passes ``counts``: this rank's columns of one draw all ranks share.  ``work``: the replicate
    context (default: a new Context on ``ctx``'s device, closed at the end).  ``init = "fit"``
    warm-starts every replicate from ``fit["estimates"]``; ``init = None`` runs the reference's own
    default initialiser per replicate, drawing from ``rng``.  ``counts`` (nboot x n_local integers):
    default ``bootstrap_counts(N, nboot, rng)``.  W and C of each replicate are aligned to the fit's
    with ``align_signs``, each against its own original; nothing is reordered.

    A warm start with few ``EMsteps`` understates the spread: a replicate that has not converged is
    still near the estimates it started from.  ``ctx``'s rows are resampled as they stand, with no
    re-centring or re-scaling per replicate, exactly like ``X[i, ]`` after ``scale()``.

    Returns ``dict(se, ci, nboot, failed, steps[, replicates])``: ``se`` and ``ci`` with the keys W, C,
    B, sigE, sigF, sigH, sigT (``bootstrap_summary``, over the replicates that succeeded); ``failed``
    the indices of replicates whose fit raised PplsError (skipped; ValueError if fewer than two
    succeed); ``steps`` the EM steps per replicate (0 for a failed one); ``replicates`` (``keep=True``)
    the aligned estimate dicts."""
    if init is not None and init != "fit":
        raise ValueError("init must be 'fit' or None")
    ctx = _ctx_with(X, Y, ctx)
    est0 = fit["estimates"]
    W0, C0 = np.array(est0["W"], dtype=np.float64, ndmin=2), np.array(est0["C"], dtype=np.float64, ndmin=2)
    a = W0.shape[1]
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    if counts is None:
        if ctx.n_local != ctx.n_total:
            raise ValueError("sharded rows: pass counts, this rank's columns of a draw all ranks share")
        counts = bootstrap_counts(ctx.n_total, nboot, rng)
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != ctx.n_local:
        raise ValueError(f"counts: nboot x {ctx.n_local} (this rank's rows), got shape {counts.shape}")
    nboot = counts.shape[0]
    theta0 = None if init is None else dict(W=W0, C=C0, B=est0["B"], sigE=est0["sigE"], sigF=est0["sigF"],
                                            sigH=est0["sigH"], sigT=est0["sigT"])
    own = work is None
    work = Context(ctx.device) if own else work
    reps, failed, steps = [], [], []
    try:
        for b in range(nboot):
            try:
                work.xprod_resample(ctx, counts[b])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")     # "Negative increments of likelihood", per replicate
                    f = PPLS_simult(None, None, a, EMsteps, atol, type, init=theta0, ctx=work, rng=rng)
            except PplsError:
                failed.append(b)
                steps.append(0)
                continue
            e = dict(f["estimates"])
            e["W"], e["C"] = align_signs(e["W"], W0), align_signs(e["C"], C0)
            reps.append(e)
            steps.append(int(len(f["loglik"])))
    finally:
        if own:
            work.close()
    if len(reps) < 2:
        raise ValueError(f"bootstrap: {len(reps)} of {nboot} replicates succeeded, a standard error needs two")
    se, ci = bootstrap_summary(reps, level)
    out = dict(se=se, ci=ci, nboot=nboot, failed=failed, steps=steps)
    if keep:
        out["replicates"] = reps
    return out


# ---------------------------------------------------------------------------- permutation test
def permutation_indices(N, nperm, rng=None):
    """``nperm`` permutations of ``N`` rows: an ``(nperm, N)`` int64 array whose row b is
    ``rng.permutation(N)``, R's ``sample(N)``.  ``rng``: a numpy Generator, or a seed for one."""
    N, nperm = int(N), int(nperm)
    if N < 1 or nperm < 0:
        raise ValueError(f"permutation_indices: N = {N}, nperm = {nperm}")
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    out = np.empty((nperm, N), dtype=np.int64)
    for b in range(nperm):
        out[b] = rng.permutation(N)
    return out


_PERM_KEYS = ("B", "cov", "loglik")


def permutation_pvalues(observed, null):
    """Per component k, ``(1 + #{b : null[b, k] >= observed[k]}) / (1 + nperm_ok[k])``, with ``nperm_ok[k]``
    the replicates whose ``null[b, k]`` is not NaN (a skipped replicate counts on neither side): the
    permutation p-value that counts the observed statistic among its own null draws, never 0; a tie
    counts against the observed value.  ``observed``: (a,), ``null``: (nperm, a).  NaN where no replicate
    has a value, or the observed one is NaN."""
    obs = np.atleast_1d(np.asarray(observed, dtype=np.float64))
    nul = np.asarray(null, dtype=np.float64).reshape(-1, obs.shape[0])
    ok = ~np.isnan(nul)
    with np.errstate(invalid="ignore"):
        ge = ok & (nul >= obs[None, :])
    n_ok = ok.sum(axis=0)
    pv = (1.0 + ge.sum(axis=0)) / (1.0 + n_ok)
    pv[(n_ok == 0) | np.isnan(obs)] = np.nan
    return pv


def _perm_stats(fit, a):
    """The sign-free statistics of a PPLS fit's first ``a`` components, NaN for components it did not reach."""
    out = {k: np.full(a, np.nan) for k in _PERM_KEYS}
    B = np.ravel(np.asarray(fit["B"], dtype=np.float64))
    k = min(a, B.shape[0])
    if k:
        sig = np.asarray(fit["sig"], dtype=np.float64).reshape(-1, 4)
        out["B"][:k] = np.abs(B[:k])
        out["cov"][:k] = np.abs(B[:k]) * sig[:k, 3] ** 2
        out["loglik"][:k] = np.asarray(fit["Other_output"]["Loglikelihoods"], dtype=np.float64)[:k]
    return out


def permutation_PPLS(fit, X, Y, nperm=199, EMsteps=100, atol=1e-4, initialGuess="o2m_xprod", rng=None, ctx=None,
                     work=None, perms=None, keep=False):
    """Permutation test of the X-Y link of a PPLS fit: is there any joint signal at all?  Replicate b
    pairs x_i with y_perm[i], which keeps both margins and destroys the link; its cross-products differ
    from the data's in the p x q block alone (``work.xprod_permute(ctx, perms[b])``, no copy of a row) and
    the fit reads only them (``PPLS(None, None, a, EMsteps, atol, initialGuess, rng=rng, ctx=work)``).

    ``fit``: the observed PPLS list, whose ``a = len(fit["B"])`` components are assessed.  ``X``, ``Y``: the
    data, or ``None, None`` with ``ctx`` holding the rows.  Sharded, every rank calls this with its own
    rows and passes ``perms``, its own permutations within its shard (still an exact test when the rows
    are exchangeable).  ``perms`` (nperm x n_local integers): default
    ``permutation_indices(N, nperm, rng)``.  ``work``: the replicate context (default: a new Context on
    ``ctx``'s device, closed at the end).

    Statistics per component k, sign-free, larger = a stronger link: ``"B"`` = |B_k|, ``"cov"`` =
    |B_k| sigT_k^2, ``"loglik"`` = the fit's log-likelihood after component k.  X'X and Y'Y are the same
    bits in every replicate, so differences in ``loglik`` come from the joint part alone.  Every
    component is tested against the global null -- X and Y unlinked -- not against a null that keeps
    the earlier components: this is not a sequential test.

    Returns ``dict(observed, null, pvalue, nperm, failed, steps[, replicates])``: ``observed[key]`` (a,),
    ``null[key]`` (nperm, a) with NaN where a replicate was skipped, ``pvalue[key]`` from
    ``permutation_pvalues`` (never 0); ``failed`` the replicates whose fit raised PplsError or stopped
    before component a (skipped for the components they did not reach; ValueError if none succeeds);
    ``steps`` the EM steps per replicate, summed over its components (0 for one that raised);
    ``replicates`` (``keep=True``) the replicate fits (None for one that raised)."""
    ctx = _ctx_with(X, Y, ctx)
    a = int(np.ravel(np.asarray(fit["B"])).shape[0])
    if a < 1:
        raise ValueError("permutation_PPLS: the fit has no component")
    kind = initialGuess if isinstance(initialGuess, str) else initialGuess[0]
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    if perms is None:
        if ctx.n_local != ctx.n_total:
            raise ValueError("sharded rows: pass perms, this rank's own permutations within its shard")
        perms = permutation_indices(ctx.n_total, nperm, rng)
    perms = np.asarray(perms)
    if perms.ndim != 2 or perms.shape[1] != ctx.n_local:
        raise ValueError(f"perms: nperm x {ctx.n_local} (this rank's rows), got shape {perms.shape}")
    nperm = perms.shape[0]
    observed = _perm_stats(fit, a)
    null = {k: np.full((nperm, a), np.nan) for k in _PERM_KEYS}
    own = work is None
    work = Context(ctx.device) if own else work
    reps, failed, steps = [], [], []
    try:
        for b in range(nperm):
            try:
                work.xprod_permute(ctx, perms[b])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")     # rank and monotonicity warnings, per replicate
                    f = PPLS(None, None, a, EMsteps, atol, kind, rng=rng, ctx=work)
            except PplsError:
                failed.append(b)
                steps.append(0)
                reps.append(None)
                continue
            st = _perm_stats(f, a)
            for k in _PERM_KEYS:
                null[k][b] = st[k]
            if len(f["B"]) < a:
                failed.append(b)
            steps.append(int(np.sum(f["Other_output"]["Number_steps"])))
            reps.append(f)
    finally:
        if own:
            work.close()
    if not np.any(~np.isnan(null["B"])):
        raise ValueError(f"permutation test: none of the {nperm} replicates succeeded")
    out = dict(observed=observed, null=null, pvalue={k: permutation_pvalues(observed[k], null[k]) for k in _PERM_KEYS},
               nperm=nperm, failed=failed, steps=steps)
    if keep:
        out["replicates"] = reps
    return out


# ---------------------------------------------------------------------------- scale()
def scale_data(X=None, Y=None, center=True, scale=True, ctx=None):
    """R's ``scale(X, center, scale)`` and ``scale(Y, center, scale)`` on the device, in place: what
    every example of the reference does before a fit (man/PPLS.Rd:57-58).  ``X``, ``Y``: loaded
    first if given, else the context's resident data are scaled.  Returns ``dict(centerX, scaleX,
    centerY, scaleY)``, R's ``attr(, "scaled:center")`` / ``"scaled:scale"`` (for data scaled more
    than once: of the composed transform).  The scaled data stay resident:
    ``scale_data(X, Y, ctx=ctx); PPLS(None, None, 3, ctx=ctx)``."""
    ctx = _ctx_with(X, Y, ctx)
    ctx.scale_data(center, scale)
    return ctx.scaling()


# ---------------------------------------------------------------------------- covariate adjustment
def _adjust_record(ctx):
    """adjust_data's result from the context's two records."""
    sc, ad = ctx.scaling(), ctx.adjustment()
    return dict(coefX=ad["coefX"], coefY=ad["coefY"], zcenter=ad["zcenter"], centerX=sc["centerX"], centerY=sc["centerY"])


def adjust_data(X=None, Y=None, Z=None, intercept=True, ctx=None):
    """R's ``X <- resid(lm(X ~ Z)); Y <- resid(lm(Y ~ Z))`` on the device, in place: age, sex, batch or
    ancestry components regressed out of both blocks before a fit, without a host round trip.  ``X``,
    ``Y``: loaded first if given, else the context's resident data are adjusted; ``Z``: the n x k
    covariates (this rank's rows).  Returns ``dict(coefX, coefY, zcenter, centerX, centerY,
    ss_explainedX, ss_explainedY)``: ``lm``'s slopes (k x p, k x q), the covariate and column means
    (0 without an intercept) and, per column, the sum of squares the design explained.  The residuals
    stay resident: ``adjust_data(X, Y, Z, ctx=ctx); scale_data(ctx=ctx); PPLS(None, None, 3, ctx=ctx)``."""
    if Z is None:
        raise ValueError("adjust_data needs the covariates Z")
    ctx = _ctx_with(X, Y, ctx)
    ctx.adjust_data(Z, intercept)
    out = _adjust_record(ctx)
    ss = ctx.adjust_explained()
    out["ss_explainedX"], out["ss_explainedY"] = ss[: ctx.p].copy(), ss[ctx.p:].copy()
    return out


def adjust_new(ctx, Xnew=None, Ynew=None, Znew=None):
    """Raw rows in the context's resident units, on the host, from its two records:
    ``(new - center - (Znew - zcenter) @ coef) / scale``.  Either of ``Xnew``, ``Ynew`` may be None;
    returns the pair.  On an adjusted context ``Znew`` is required -- the adjustment is never skipped
    silently; on any other it must be None or is ignored, and only centre and scale apply."""
    sc, ad = ctx.scaling(), ctx.adjustment()
    Zc = None
    if ad["k"]:
        if Znew is None:
            raise ValueError("the context's data were adjusted for covariates: new rows need their Z")
        Zc = np.asarray(Znew, dtype=np.float64)
        if Zc.ndim != 2:
            Zc = Zc.reshape(-1, ad["k"])      # one row of k values, or a column for k = 1
        if Zc.shape[1] != ad["k"]:
            raise ValueError(f"Znew has {Zc.shape[1]} columns, the adjustment {ad['k']}")
        Zc = Zc - ad["zcenter"]
    out = []
    for new, b in ((Xnew, "X"), (Ynew, "Y")):
        if new is None:
            out.append(None)
            continue
        new = np.asarray(new, dtype=np.float64)
        if new.ndim != 2:
            new = new.reshape(1, -1)
        if Zc is not None and Zc.shape[0] != new.shape[0]:
            raise ValueError("Znew needs one row per new row")
        fit = Zc @ ad["coef" + b] if Zc is not None else 0.0
        out.append((new - sc["center" + b] - fit) / sc["scale" + b])
    return tuple(out)


def _chunk_arrays(X, Y, p=None, q=None):
    """One chunk as float64 matrices in one memory order, and that order's layout code: F-contiguous
    pairs go as they are (column-major), everything else C-contiguous (copied only if it is not)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
        raise ValueError("a chunk is a pair of matrices X, Y with the same number of rows")
    if (p is not None and X.shape[1] != p) or (q is not None and Y.shape[1] != q):
        raise ValueError(f"chunk of {X.shape[1]} + {Y.shape[1]} columns in a stream of {p} + {q}")
    if X.flags.f_contiguous and Y.flags.f_contiguous and not (X.flags.c_contiguous and Y.flags.c_contiguous):
        return X, Y, _lib.PPLS_LAYOUT_COLMAJOR
    return np.ascontiguousarray(X), np.ascontiguousarray(Y), _lib.PPLS_LAYOUT_ROWMAJOR


def _fold_array(fold, n, K=None):
    """The fold labels of a chunk of ``n`` rows as int32, checked on the host: integers, one per row,
    in 0 .. K-1."""
    f = np.asarray(fold)
    if f.ndim != 1 or f.shape[0] != n:
        raise ValueError(f"fold labels: {f.shape} for a chunk of {n} rows (one label per row)")
    if f.dtype.kind not in "iu":
        raise TypeError(f"fold labels must be integers, not {f.dtype}")
    if n and (int(f.min()) < 0 or (K is not None and int(f.max()) >= K) or int(f.max()) > np.iinfo(np.int32).max):
        raise ValueError(f"fold labels must lie in 0 .. {'K-1' if K is None else K - 1}: found "
                         f"{int(f.min())} .. {int(f.max())}")
    return np.ascontiguousarray(f, dtype=np.int32)


def _stream_covariates(chunks, scale, ctx):
    """stream_data(covariates=True): [Y Z] streamed centred into a private source, then partialled out."""
    if isinstance(chunks, np.ndarray) or not hasattr(chunks, "__iter__"):
        raise TypeError("chunks must be an iterable of (X, Y, Z) triples")
    ctx = ctx or default_context()
    src = None
    try:
        p = q = k = None
        for tri in chunks:
            if not isinstance(tri, (tuple, list)) or len(tri) != 3:
                raise TypeError("every chunk must be an (X, Y, Z) triple")
            X = np.asarray(tri[0], dtype=np.float64)
            Z = Context._design(tri[2], X.shape[0] if X.ndim == 2 else -1)
            Y = np.asarray(tri[1], dtype=np.float64)
            if Y.ndim != 2 or Y.shape[0] != Z.shape[0]:
                raise ValueError("a chunk is a triple of matrices X, Y, Z with the same number of rows")
            if k is not None and Z.shape[1] != k:
                raise ValueError(f"chunk with {Z.shape[1]} covariates in a stream of {k}")
            YZ = np.ascontiguousarray(np.hstack([Y, Z]))
            X, YZ, _ = _chunk_arrays(X, YZ, p, None if q is None else q + k)
            if src is None:
                p, q, k = X.shape[1], Y.shape[1], Z.shape[1]
                if k < 1:
                    raise ValueError("covariates=True needs at least one column of Z")
                src = Context(ctx.device)
                if getattr(ctx, "_reducer_fn", None) is not None:
                    src.set_reducer(ctx._reducer_fn)     # the same ranks take part
                src.stream_begin(p, q + k, True, False)
            src.stream_rows(X, YZ)
        if src is None:
            raise ValueError("chunks is empty: no rows to stream")
        src.stream_end()
        ctx.xprod_adjust(src, k, scale)
    finally:
        if src is not None:
            src.close()
    out = dict(n=ctx.n_total)
    out.update(ctx.scaling())
    ad = ctx.adjustment()
    out.update(coefX=ad["coefX"], coefY=ad["coefY"], zcenter=ad["zcenter"])
    return out


def stream_data(chunks, center=True, scale=True, ctx=None, nr_folds=None, covariates=False):
    """Load data too large to hold at once: ``chunks`` is an iterable of ``(X, Y)`` row blocks (numpy
    matrices, e.g. slices of a memory-mapped file).  Their cross-products -- of the rows centred and
    scaled as R's ``scale()`` would the whole matrix -- are accumulated on the device; no rows stay
    resident.  Returns ``dict(n, centerX, scaleX, centerY, scaleY)``.  Afterwards
    ``PPLS(None, None, a, ctx=ctx)`` and ``PPLS_simult(None, None, a, ctx=ctx)`` fit from them.
    ``nr_folds=K``: every chunk is an ``(X, Y, fold)`` triple with the fold (0 .. K-1) of each row
    (``fold_labels`` gives cv_PPLS's); one cross-product matrix per fold is kept, the result gains
    ``fold_total``, and ``cv_PPLS(None, None, a, K, ctx=ctx)`` / ``crossval_PPLS`` run on them.
    ``covariates=True``: every chunk is an ``(X, Y, Z)`` triple; ``[Y Z]`` is streamed centred into a
    private context and the covariates are partialled out of the cross-products on the device
    (``Context.xprod_adjust``), which is ``adjust_data`` with an intercept followed by ``scale_data(center
    =True, scale=scale)`` for rows that are never resident; the result gains ``coefX``, ``coefY`` and
    ``zcenter``.  It needs ``center=True`` and cannot be combined with ``nr_folds``; ranks take part
    through a host reducer (``set_reducer``)."""
    if covariates:
        if nr_folds is not None:
            raise ValueError("covariates=True cannot be combined with nr_folds: per-fold adjustment is not provided")
        if not center:
            raise ValueError("covariates=True implies an intercept: center must be True")
        return _stream_covariates(chunks, scale, ctx)
    want = 2 if nr_folds is None else 3
    what = "(X, Y) pair" if nr_folds is None else "(X, Y, fold) triple"
    if nr_folds is not None and int(nr_folds) < 2:
        raise ValueError("Cross-validation with 1 fold does not make sense, use 2 folds or more")
    if isinstance(chunks, np.ndarray) or not hasattr(chunks, "__iter__"):
        raise TypeError(f"chunks must be an iterable of {what}s")
    it = iter(chunks)
    first = next(it, None)
    if first is None:
        raise ValueError("chunks is empty: no rows to stream")
    p = q = None
    for pair in itertools.chain([first], it):
        if not isinstance(pair, (tuple, list)) or len(pair) != want:
            raise TypeError(f"every chunk must be an {what}")
        X, Y, _ = _chunk_arrays(pair[0], pair[1], p, q)   # (checked before a device is touched)
        fold = None if nr_folds is None else _fold_array(pair[2], X.shape[0], int(nr_folds))
        if p is None:
            p, q = X.shape[1], Y.shape[1]
            ctx = ctx or default_context()
            ctx.stream_begin(p, q, center, scale, nr_folds)
        ctx.stream_rows(X, Y, fold)
    return ctx.stream_end()


# ---------------------------------------------------------------------------- cross-validation
# predict.PPLS, cv_PPLS, crossval_PPLS (Package/PPLS/R/crossval_PPLS.R:12-114).  Two statements below
# rest on no R run: mse(x, y) = mean((x - y)^2) is OmicsPLS's (not vendored with the reference), and
# cv_blocks restates base R's cut.default.

def cv_blocks(N, K):
    """R's ``as.numeric(cut(seq(1:N), breaks=K, labels=F))`` (crossval_PPLS.R:43) restated from
    cut.default: K equal-width intervals over [1, N] (breaks seq(1, N, length.out = K + 1)), the two
    ends moved out by (N - 1) / 1000, intervals right-closed.  Returns the 1-based block label of
    1..N (non-decreasing); N = 10, K = 3 gives sizes 4, 3, 3."""
    N, K = int(N), int(K)
    if N < 1 or K < 1:
        raise ValueError("cv_blocks needs N >= 1 and K >= 1")
    dx = float(N - 1)
    if dx == 0.0:      # cut.default's constant-x branch: dx = |x|, breaks over [x - dx/1000, x + dx/1000]
        breaks = np.linspace(1.0 - 1e-3, 1.0 + 1e-3, K + 1)
    else:
        breaks = 1.0 + np.arange(K + 1) * (dx / K)
        breaks[-1] = float(N)
        breaks[0] -= dx / 1000
        breaks[-1] += dx / 1000
    return np.searchsorted(breaks, np.arange(1, N + 1, dtype=np.float64), side="left").astype(np.int64)


_PREDICT_CTX = None


def _fit_parts(obj):
    est = obj.get("estimates", obj)
    W = np.array(est["W"], dtype=np.float64, ndmin=2)
    C = np.array(est["C"], dtype=np.float64, ndmin=2)
    return W, C, est["B"]


def predict_PPLS(object, newdata, XorY=("X", "Y"), ctx=None, rescale=False, Znew=None):
    """predict.PPLS (crossval_PPLS.R:12-24): ``newdata W diag(B) C'`` for XorY = "X" (newdata is X,
    the prediction is of Y) or ``newdata C diag(1/B) W'`` for "Y", on the GPU.  A 1-D ``newdata`` is
    one row (R's ``t(newdata)``).  ``ctx``: a context whose data have the fit's shape; by default
    the default context when its shape matches, else a private context that holds no rows.
    ``rescale=True``: ``newdata`` is in the units the data were loaded in; with a context whose data
    were scaled on the device (``scale_data``) it is brought to the fit's scale with the stored
    centre and scale of its block, on the host, and the prediction is mapped back to the loaded
    units of the other block.  With a context whose data were adjusted for covariates (``adjust_data``)
    ``Znew``, the new rows' covariates, is required then: their fitted share is taken out of
    ``newdata`` and added to the prediction (``adjust_new``)."""
    global _PREDICT_CTX
    xy = XorY if isinstance(XorY, str) else XorY[0]          # match.arg
    if xy not in ("X", "Y"):
        raise ValueError("'arg' should be one of \"X\", \"Y\"")
    W, C, B = _fit_parts(object)
    nd = np.asarray(newdata, dtype=np.float64)
    if nd.ndim != 2:
        nd = nd.reshape(1, -1)
    if nd.shape[1] != (W.shape[0] if xy == "X" else C.shape[0]):
        raise ValueError("Number of columns mismatch!")
    p, q = W.shape[0], C.shape[0]
    if ctx is None:
        ctx = _DEFAULT_CTX if _DEFAULT_CTX is not None and (_DEFAULT_CTX.p, _DEFAULT_CTX.q) == (p, q) else None
    if ctx is None:
        if _PREDICT_CTX is None:
            _PREDICT_CTX = Context(0)
        ctx = _PREDICT_CTX
        if (ctx.p, ctx.q) != (p, q):
            ctx.set_data(np.zeros((0, p)), np.zeros((0, q)))   # the shape only
    if rescale and ctx.adjustment()["k"]:
        ad, sc = ctx.adjustment(), ctx.scaling()
        other = "Y" if xy == "X" else "X"
        x = adjust_new(ctx, nd if xy == "X" else None, nd if xy == "Y" else None, Znew)[0 if xy == "X" else 1]
        Zc = np.asarray(Znew, dtype=np.float64).reshape(nd.shape[0], ad["k"]) - ad["zcenter"]
        return (ctx.predict(W, C, B, x, 0 if xy == "X" else 1) * sc["scale" + other] + sc["center" + other]
                + Zc @ ad["coef" + other])
    if rescale:
        sc = ctx.scaling()
        cin, sin, cout, sout = ((sc["centerX"], sc["scaleX"], sc["centerY"], sc["scaleY"]) if xy == "X" else
                                (sc["centerY"], sc["scaleY"], sc["centerX"], sc["scaleX"]))
        if np.any(cin != 0) or np.any(sin != 1) or np.any(cout != 0) or np.any(sout != 1):
            return ctx.predict(W, C, B, (nd - cin) / sin, 0 if xy == "X" else 1) * sout + cout
    return ctx.predict(W, C, B, nd, 0 if xy == "X" else 1)


_CV_PPLS_ARGS = ("EMsteps", "atol", "initialGuess", "customGuess", "critfunc")


def _cv_args(ppls_args):
    bad = [k for k in ppls_args if k not in _CV_PPLS_ARGS]
    if bad:
        raise TypeError(f"cv_PPLS takes PPLS's {', '.join(_CV_PPLS_ARGS)}; got {', '.join(bad)}")
    kind = ppls_args.get("initialGuess", "equal")
    kind = kind if isinstance(kind, str) else kind[0]
    custom = ppls_args.get("customGuess")
    if custom is not None:
        kind = "custom"
    if kind == "o2m":
        raise NotImplementedError("initialGuess='o2m' inside cross-validation is not implemented "
                                  "(its starting values come from per-fold SVDs of the training rows)")
    if kind not in ("equal", "random", "custom", "o2m_xprod"):
        raise ValueError(f"unknown initialGuess {kind!r}")
    if kind == "custom" and custom is None:
        raise ValueError("initialGuess='custom' needs customGuess")
    return (kind, custom, int(ppls_args.get("EMsteps", 100)), float(ppls_args.get("atol", 1e-4)),
            _crit_abs(ppls_args.get("critfunc")))


def fold_labels(N, K, folds=None, rng=None):
    """The fold (0 .. K-1, int32) of each of N rows as cv_PPLS assigns it (crossval_PPLS.R:42-44):
    ``folds`` is the permutation R's ``sample(N)`` would give, 0-based (default
    ``rng.permutation(N)``), and fold i holds rows ``folds[cv_blocks(N, K) == i + 1]``.  For callers
    who stream rows with ``nr_folds=K`` and know N beforehand."""
    N, K = int(N), int(K)
    if K < 2:
        raise ValueError("Cross-validation with 1 fold does not make sense, use 2 folds or more")
    if N < K:
        raise ValueError("nrow(X) >= nr_folds is not TRUE")
    blocks = cv_blocks(N, K)
    if folds is None:
        rng = rng if rng is not None else np.random.default_rng()
        folds = rng.permutation(N)                 # R: folds <- sample(N)
    folds = np.asarray(folds, dtype=np.int64)
    if folds.shape != (N,) or not np.array_equal(np.sort(folds), np.arange(N)):
        raise ValueError("folds must be a permutation of 0..N-1")
    fold_of = np.empty(N, dtype=np.int32)
    fold_of[folds] = blocks - 1                    # fold i holds rows folds[blocks == i]
    return fold_of


def _cv_inits(ctx, a, K, kind, custom, rng):
    if kind == "custom":
        one = list(custom) if isinstance(custom, (list, tuple)) else [custom] * a
        return [one] * K
    if kind == "equal":
        return [[initial_guess(ctx.p, ctx.q, "equal") for _ in range(a)]] * K
    rng = rng if rng is not None else np.random.default_rng()   # fold by fold, component by component
    return [[initial_guess(ctx.p, ctx.q, "random", rng) for _ in range(a)] for _ in range(K)]


def _cv_run(ctx, a, nr_folds, folds, rng, ppls_args):
    """The folds of cv_PPLS (:42-44) and one ppls_cv_ppls call with ``a`` components:
    (rmsep nr_folds x a, ncomp)."""
    kind, custom, steps, atol, crit_abs = _cv_args(ppls_args)
    N, K = int(ctx.n_total), int(nr_folds)
    fold_of = fold_labels(N, K, folds, rng)
    fold_total = np.bincount(fold_of, minlength=K).astype(np.int64)
    lo = int(ctx.row0)
    if kind == "o2m_xprod":   # the starts come from each training set's cross-products, on the device
        return ctx.cv_ppls_o2m(a, fold_of[lo: lo + ctx.n_local], fold_total, steps, atol, crit_abs)
    inits = _cv_inits(ctx, a, K, kind, custom, rng)
    return ctx.cv_ppls(a, fold_of[lo: lo + ctx.n_local], fold_total, steps, atol, inits, crit_abs)


_COND_LIMIT = 1e-6     # lost digits, not a tolerance: warn where cond 64 u exceeds it


def _cv_run_stream(ctx, a, nr_folds, folds, rng, ppls_args):
    """cv_PPLS's loop on the folds a context was streamed with (ppls_cv_ppls_stream):
    (rmsep K x a, ncomp).  The arguments are checked before any device call."""
    kind, custom, steps, atol, crit_abs = _cv_args(ppls_args)
    K = int(ctx._stream_folds)
    if int(nr_folds) != K:
        raise ValueError(f"nr_folds={int(nr_folds)}, but the rows were streamed with {K} folds")
    if folds is not None:
        raise ValueError("folds= cannot be given: the folds are those the rows were streamed with")
    if kind == "o2m_xprod":
        rmsep, ncomp, cond = ctx.cv_ppls_stream_o2m(a, steps, atol, crit_abs)
    else:
        inits = _cv_inits(ctx, a, K, kind, custom, rng)
        rmsep, ncomp, cond = ctx.cv_ppls_stream(a, steps, atol, inits, crit_abs)
    with np.errstate(invalid="ignore"):
        bad = np.argwhere(np.abs(cond) * 64 * 2.0 ** -53 > _COND_LIMIT)
    for f, j in bad:
        warnings.warn(f"fold {int(f)}, {int(j) + 1} component(s): the held-out error from cross-products keeps "
                      f"few digits (mag / sse = {cond[f, j]:.3g})")
    return rmsep, ncomp


def _cv_err(rmsep, ncomp, nr_comp):
    """Per-fold error of the nr_comp-component fit; a fold whose fit stopped early is scored with
    the components it has, as R's predict would with the truncated fit (and PPLS's warning)."""
    k = np.minimum(ncomp, nr_comp)
    if np.any(k < nr_comp):
        warnings.warn("From component %d on the residuals are of rank < 1e-14 and calculations are stopped."
                      % (int(k.min()) + 1))
    return np.array([rmsep[f, k[f] - 1] if k[f] > 0 else np.nan for f in range(rmsep.shape[0])])


def cv_PPLS(X, Y, nr_comp, nr_folds, folds=None, rng=None, ctx=None, per_fold=False, **ppls_args):
    """cv_PPLS (crossval_PPLS.R:40-52): the RMSEP of Y predicted from X by an nr_comp-component PPLS
    fit, cross-validated over nr_folds folds, averaged over the folds (``mean(err)``); with
    ``per_fold=True`` also the per-fold errors.  ``folds``: the permutation R's ``sample(N)`` would
    give, 0-based (default ``rng.permutation(N)``); fold i holds ``folds[cv_blocks(N, K) == i]``.
    ``ppls_args``: PPLS's EMsteps, atol, initialGuess ('equal', 'random', 'custom', 'o2m_xprod'),
    customGuess, critfunc; 'random' starts are drawn from ``rng`` fold by fold, component by component,
    'o2m_xprod' starts come from each training set's cross-products on the device.  The folds
    run on the device (ppls_cv_ppls).  mse(x, y) = mean((x - y)^2) as in OmicsPLS.
    ``cv_PPLS(None, None, nr_comp, K, ctx=ctx)`` on a context streamed with ``nr_folds=K`` runs on
    the stream's folds from their cross-products (ppls_cv_ppls_stream): ``nr_folds`` must be that K
    and ``folds`` None (ValueError otherwise); a warning names every fold and prefix whose held-out
    error lost digits to cancellation (mag / sse 64 u > 1e-6)."""
    _cv_args(ppls_args)
    if int(nr_folds) < 2:
        raise ValueError("Cross-validation with 1 fold does not make sense, use 2 folds or more")
    if X is None and ctx is not None and ctx._stream_folds:
        rmsep, ncomp = _cv_run_stream(ctx, int(nr_comp), nr_folds, folds, rng, ppls_args)
    else:
        ctx = _ctx_with(X, Y, ctx)
        rmsep, ncomp = _cv_run(ctx, int(nr_comp), nr_folds, folds, rng, ppls_args)
    err = _cv_err(rmsep, ncomp, int(nr_comp))
    return (float(np.mean(err)), err) if per_fold else float(np.mean(err))


def crossval_PPLS(X, Y, a, nr_folds, nr_cores=1, shared_folds=False, ctx=None, **ppls_args):
    """crossval_PPLS (crossval_PPLS.R:78-114): cv_PPLS for every number of components in ``a``.
    Returns a dict of class "cvPPLS": ``errors`` (one per entry of ``a``), ``which_error`` (index of
    the minimum into ``a``, 0-based), ``a_min`` and ``time`` (seconds).  ``nr_cores`` is checked as
    in R and otherwise ignored: the folds run on the one device.  Default: a fresh fold permutation
    per entry of ``a`` as in R, one device loop per entry.  ``shared_folds=True``: one permutation and
    one loop with max(a) components whose prefixes give every entry (PPLS is sequential): K fits
    instead of K * len(a).  ``rng`` / ``folds`` are passed on as for cv_PPLS.  On a context streamed
    with folds the folds are the stream's for every entry of ``a`` (R's fresh permutation per entry
    is impossible once the rows are gone): ``shared_folds=True`` makes K fits of max(a) components,
    ``False`` K * len(a) fits on the same folds."""
    tic = time.perf_counter()
    a = [int(v) for v in np.atleast_1d(a)]
    rng = ppls_args.pop("rng", None)
    folds = ppls_args.pop("folds", None)
    _cv_args(ppls_args)
    if X is not None:
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        if X.ndim != 2 or Y.ndim != 2:
            raise ValueError("X and Y must be matrices")
        if np.any(np.abs(X.mean(axis=0)) > 1e-5):
            warnings.warn("Data is not centered, proceeding...")
        p, q, n = X.shape[1], Y.shape[1], X.shape[0]
    else:
        if ctx is None or ctx.n_local is None:
            raise ValueError("no data: pass X and Y or a context with resident data")
        p, q, n = ctx.p, ctx.q, ctx.n_total
    if not a or min(a) < 1:
        raise ValueError("a must hold positive integers")
    if not (p > max(a) and q > max(a) and n >= nr_folds):         # stopifnot(...) :84
        raise ValueError("ncol(X) > max(a), ncol(Y) > max(a), nrow(X) >= nr_folds are not all TRUE")
    if nr_cores != abs(round(nr_cores)):                          # :85
        raise ValueError("nr_cores == abs(round(nr_cores)) is not TRUE")
    if nr_folds == 1:
        raise ValueError("Cross-validation with 1 fold does not make sense, use 2 folds or more")
    streamed = X is None and ctx is not None and bool(ctx._stream_folds)
    if streamed:     # the arguments are checked before any device call
        if int(nr_folds) != int(ctx._stream_folds):
            raise ValueError(f"nr_folds={int(nr_folds)}, but the rows were streamed with {ctx._stream_folds} folds")
        if folds is not None:
            raise ValueError("folds= cannot be given: the folds are those the rows were streamed with")
    ctx = _ctx_with(X, Y, ctx)
    if shared_folds:
        run = _cv_run_stream if streamed else _cv_run
        rmsep, ncomp = run(ctx, max(a), nr_folds, folds, rng, ppls_args)
        errors = [float(np.mean(_cv_err(rmsep, ncomp, e))) for e in a]
    else:
        rng = rng if rng is not None else np.random.default_rng()
        errors = [cv_PPLS(None, None, e, nr_folds, folds=folds, rng=rng, ctx=ctx, **ppls_args) for e in a]
    errors = np.array(errors)
    which = int(np.nanargmin(errors)) if np.any(np.isfinite(errors)) else 0
    out = dict(errors=errors, which_error=which, a_min=a[which], time=round(time.perf_counter() - tic, 2))
    out["class"] = "cvPPLS"
    return out


# ---------------------------------------------------------------------------- row diagnostics
_DIAG_STATS = ("odx2", "ody2", "sd2", "d2")


def diagnostics_df(p, q, r):
    """Degrees of freedom of the four distances under the model: odx2 / sigE^2 has p - r, ody2 / sigF^2
    q - r, sd2 2r and d2 p + q."""
    return dict(odx2=int(p) - int(r), ody2=int(q) - int(r), sd2=2 * int(r), d2=int(p) + int(q))


def chisq_upper(x, df):
    """Upper chi-square tail P(chi2_df > x) in fp64, never NaN for finite ``x``: 1 for ``df = 0`` (a
    statistic without degrees of freedom is zero up to rounding) and for ``x <= 0``."""
    import scipy.special
    x = np.asarray(x, dtype=np.float64)
    if df <= 0:
        return np.ones_like(x)
    return np.asarray(scipy.special.gammaincc(0.5 * df, 0.5 * np.maximum(x, 0.0)), dtype=np.float64)


def diagnostics_summary(res, p, q, r, sigE, sigF, alpha=0.01, adjust="none", df=None):
    """``df``, ``pvalue``, ``flag`` and ``outliers`` from the distances of one diagnostics call (the host
    part of ``diagnostics_PPLS``).  ``adjust="bonferroni"`` tests at ``alpha / n``, n the rows of this call.
    ``df``: the degrees of freedom when they are not ``diagnostics_df(p, q, r)``'s."""
    if adjust not in ("none", "bonferroni"):
        raise ValueError("adjust should be one of \"none\", \"bonferroni\"")
    n = int(np.asarray(res["d2"]).shape[0])
    level = float(alpha) / n if adjust == "bonferroni" and n > 0 else float(alpha)
    df = diagnostics_df(p, q, r) if df is None else df
    stat = dict(odx2=np.asarray(res["odx2"]) / (float(sigE) * float(sigE)),
                ody2=np.asarray(res["ody2"]) / (float(sigF) * float(sigF)), sd2=np.asarray(res["sd2"]),
                d2=np.asarray(res["d2"]))
    pv = {k: chisq_upper(stat[k], df[k]) for k in _DIAG_STATS}
    flag = {k: pv[k] < level for k in _DIAG_STATS}
    hit = np.flatnonzero(flag["d2"])
    return dict(df=df, pvalue=pv, flag=flag, outliers=hit[np.argsort(pv["d2"][hit], kind="stable")])


def _diagnostics_rows(p, q, X, Y, ctx, subset, new, rescale, Z, resident, fresh):
    """The rows of a diagnostics call and the context that scores them, as ``diagnostics_PPLS`` documents:
    ``resident(ctx, subset)`` on rows a context holds, ``fresh(ctx, X, Y)`` on new rows in the fit's units."""
    global _PREDICT_CTX
    if new:
        if X is None or Y is None:
            raise ValueError("new=True needs the rows X and Y")
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        if X.ndim != 2:
            X = X.reshape(1, -1)
        if Y.ndim != 2:
            Y = Y.reshape(1, -1)
        if X.shape[1] != p or Y.shape[1] != q:
            raise ValueError("Number of columns mismatch!")
        if ctx is None:
            ctx = _DEFAULT_CTX if _DEFAULT_CTX is not None and (_DEFAULT_CTX.p, _DEFAULT_CTX.q) == (p, q) else None
        if ctx is None:
            if _PREDICT_CTX is None:
                _PREDICT_CTX = Context(0)
            ctx = _PREDICT_CTX
            if (ctx.p, ctx.q) != (p, q):
                ctx.set_data(np.zeros((0, p)), np.zeros((0, q)))   # the shape only
        if (ctx.p, ctx.q) != (p, q):
            raise ValueError("Number of columns mismatch!")
        if subset is not None:
            idx = np.ravel(np.asarray(subset, dtype=np.int64))
            if Z is not None:
                Z = np.asarray(Z, dtype=np.float64).reshape(X.shape[0], -1)[idx]
            X, Y = X[idx], Y[idx]
        if rescale and ctx.adjustment()["k"]:
            X, Y = adjust_new(ctx, X, Y, Z)
        elif rescale:
            sc = ctx.scaling()
            X = (X - sc["centerX"]) / sc["scaleX"]
            Y = (Y - sc["centerY"]) / sc["scaleY"]
        return fresh(ctx, X, Y)
    if X is not None and (np.ndim(X) != 2 or np.ndim(Y) != 2 or np.shape(X)[1] != p or np.shape(Y)[1] != q):
        raise ValueError("Number of columns mismatch!")
    ctx = _ctx_with(X, Y, ctx)
    if (ctx.p, ctx.q) != (p, q):
        raise ValueError("Number of columns mismatch!")
    return resident(ctx, subset)


def diagnostics_PPLS(fit, X=None, Y=None, ctx=None, subset=None, new=False, rescale=False, alpha=0.01, adjust="none",
                     want_mu=False, Z=None):
    """Which rows does a ``PPLS_simult`` fit not explain?  Per row, on the GPU in one pass over the rows:
    the squared Mahalanobis distance ``d2`` under the fitted covariance, its in-plane part ``sd2`` (score
    distance) and off-plane parts ``odx2``, ``ody2`` (squared orthogonal distances in X and Y) and the
    log-density ``loglik``, which sums to ``logl_W``; with ``want_mu`` Expect_M's ``mu_T``, ``mu_U``.  On
    the host: ``df``, upper chi-square ``pvalue`` and ``flag`` (``p < alpha``, or ``p < alpha / n`` with
    ``adjust="bonferroni"``) per distance, and ``outliers``, the rows with ``flag["d2"]`` sorted by p.

    ``fit``: a ``PPLS_simult`` fit or a ``Theta``.  ``X, Y`` given: loaded into the context and scored;
    ``X=None``: the rows resident in ``ctx``; ``subset``: 0-based local row indices.  ``new=True``: ``X, Y``
    are rows scored against the fit without touching the context's data (any context of the fit's shape:
    streamed, or without rows); with ``rescale=True`` they come in the units the data were loaded in and
    are brought to the fit's with ``ctx.scaling()`` on the host, as ``predict_PPLS`` does -- called once
    per chunk this is the second pass that screens a ``stream_data`` fit.  On a context whose data were
    adjusted for covariates ``rescale=True`` needs ``Z``, the new rows' covariates (``adjust_new``)."""
    if adjust not in ("none", "bonferroni"):
        raise ValueError("adjust should be one of \"none\", \"bonferroni\"")
    if isinstance(fit, Theta):
        th = fit
    elif isinstance(fit, dict) and "estimates" in fit:
        e = fit["estimates"]
        th = Theta(e["W"], e["C"], e["B"], e["sigE"], e["sigF"], e["sigH"], e["sigT"])
    else:
        raise ValueError("diagnostics need one joint covariance: pass a PPLS_simult fit (or a Theta); the components "
                         "of a sequential PPLS / PPLSi fit carry their own sigmas")
    p, q, r = th.W.shape[0], th.C.shape[0], th.r
    res = _diagnostics_rows(p, q, X, Y, ctx, subset, new, rescale, Z,
                            lambda c, rows: c.row_diagnostics(th, rows=rows, want_mu=want_mu),
                            lambda c, Xn, Yn: c.row_diagnostics_new(th, Xn, Yn, want_mu=want_mu))
    out = dict(res)
    out.update(diagnostics_summary(res, p, q, r, th.sigE, th.sigF, alpha=alpha, adjust=adjust))
    return out


# ---------------------------------------------------------------------------- PO2PLS
def _po2_theta(W, C, P_Yosc, P_Xosc, B_T, sigX, sigY, sigH, sigT, sigTo, sigUo):
    return Po2Theta(W, P_Yosc, C, P_Xosc, B_T, sigT, sigTo if sigTo is not None else (), sigUo if sigUo is not None else (),
                    sigX, sigY, sigH)


def PO2PLS_Expect(X, Y, W, C, P_Yosc, P_Xosc, B_T, sigX, sigY, sigH, sigT, sigTo, sigUo, ctx=None):
    """EMstepC (loglC.cpp:116-250) from the cross-products: its list of expected sample covariances
    (Cxt, Cxto, Ctt, Ctto, Ctoto, Cyu, Cyuo, Cuu, Cuuo, Cuouo, Cut, Chh as full matrices), with Cee and
    Cff as the scalars tr(.)/p, tr(.)/q of its diag_Cee, diag_Cff, and K = D Lambda^-1 (the posterior
    means of the rows are [X Gx | Y Gy] K).  ``X = Y = None``: the context's data, rows or S alone."""
    ctx = _ctx_with(X, Y, ctx)
    return ctx.po2_estep(_po2_theta(W, C, P_Yosc, P_Xosc, B_T, sigX, sigY, sigH, sigT, sigTo, sigUo)).as_dict()


def PO2PLS_logl(X, Y, W, C, P_Yosc, P_Xosc, B_T, sigX, sigY, sigH, sigT, sigTo, sigUo, ctx=None):
    """loglC's value (loglC.cpp:36-113) from the cross-products, with the constant -N (p+q)/2 log 2 pi."""
    ctx = _ctx_with(X, Y, ctx)
    return ctx.po2_loglik(_po2_theta(W, C, P_Yosc, P_Xosc, B_T, sigX, sigY, sigH, sigT, sigTo, sigUo))


def PO2PLS(X, Y, r, rx, ry, EMsteps=100, atol=1e-4, type="SVD", init="ppls", rng=None, ctx=None, start_steps=10):
    """Fit the PO2PLS model -- PPLS_simult's plus rx X-specific and ry Y-specific components (the
    reference's simulC model, loglC.cpp:268-315) -- by EM on the cross-products S, on the device.

    Returns dict(Expectations, loglik, estimates, class="PO2PLS"): estimates has W, Wo, C, Co, B, sigT,
    sigTo, sigUo (diagonal matrices), sigE, sigF, sigH in canonical form; loglik has steps + 1 entries;
    Expectations is ``PO2PLS_Expect`` at the estimates.  ``X = Y = None``: the context's data -- any
    context that holds S (streamed, fold-selected, resampled, permuted, weighted, adjusted) or rows.

    ``init="ppls"`` (``ppls_po2_start``): the joint part from the 'o2m_xprod' sequential fit with ONE EM
    step per component -- the cross-covariance directions.  More steps are worse: every step of that
    shared-only model pulls a joint loading towards the strongest X-only direction (on the recovery
    problem of tests/po2_bar.py the start's loading-space error grows from 0.4-0.6 at 1 step to 1.4 at 5
    and 20 steps, and from the 20-step start the EM stays at the shared-only optimum for more than 300
    steps; from the 1-step start it recovers within 100).

    The specific loadings come from ``start_steps`` orthogonal-iteration steps of the statistics pass,
    started at normal draws from ``rng``.

    ``init=dict(W, Wo, C, Co, B, sigT, sigTo, sigUo, sigE, sigF, sigH)`` is taken as given (loadings need
    not be orthonormal).  ``type``: "SVD" (the polar factor) or "QR" (R's sign rule), as PPLS_simult.
    Warns "Negative increments of likelihood" as PPLS_simult does."""
    ctx = _ctx_with(X, Y, ctx)
    r, rx, ry = int(r), int(rx), int(ry)
    t = _orth_type(type)
    if isinstance(init, dict):
        th = Po2Theta.from_dict(init)
        if (th.r, th.rx, th.ry) != (r, rx, ry):
            raise ValueError(f"init has (r, rx, ry) = {(th.r, th.rx, th.ry)}, asked for {(r, rx, ry)}")
    elif init == "ppls":
        rng = rng if rng is not None else np.random.default_rng()
        th = ctx.po2_start(r, rx, ry, rng.standard_normal((ctx.p, rx)), rng.standard_normal((ctx.q, ry)), start_steps)
    else:
        raise ValueError("init must be 'ppls' or a dict of starting values")
    est, ll, eout, neg = ctx.po2_em_run(th, int(EMsteps), float(atol), t, want_eout=True)
    if neg:
        warnings.warn("Negative increments of likelihood")
    return {"Expectations": eout.as_dict(), "loglik": ll, "estimates": est.as_dict(), "class": "PO2PLS"}


def predict_PO2PLS(fit, newdata, XorY="X", ctx=None, rescale=False, Znew=None):
    """The PO2PLS prediction E[y | x] (``XorY="X"``) or E[x | y] ("Y") of the rows of ``newdata``, on the GPU:
    the map of ``po2_predict_map`` fed through ``predict_PPLS``'s path, so ``ctx``, ``rescale`` and ``Znew``
    mean what they mean there (scaled and covariate-adjusted contexts included).  ``fit``: a PO2PLS fit
    or its ``estimates``."""
    xy = XorY if isinstance(XorY, str) else XorY[0]
    e = fit["estimates"] if "estimates" in fit else fit
    L, Bp = po2_predict_map(e, xy)
    obj = dict(W=L, C=np.asarray(e["C"], dtype=np.float64), B=Bp) if xy == "X" else \
        dict(W=np.asarray(e["W"], dtype=np.float64), C=L, B=Bp)
    return predict_PPLS(obj, newdata, xy, ctx=ctx, rescale=rescale, Znew=Znew)


def crossval_PO2PLS(X, Y, r, rx, ry, nr_folds, folds=None, rng=None, ctx=None, EMsteps=100, atol=1e-4, type="SVD",
                    start_steps=10, return_fits=False):
    """Choose PO2PLS's component counts by cross-validated X -> Y prediction error.

    ``r``, ``rx``, ``ry``: lists; the grid is their product, in that order (list the small models first:
    ties, and cells within rounding of each other, go to the cell listed first).  Per fold all cells are
    fitted at once on the training cross-products (``ppls_po2_em_run_batch``) from ``ppls_po2_start``'s
    values (normal draws from ``rng``, the same for every fold and cell), and the held-out error comes from
    the fold's own cross-products.  Cells outside the model's size limits are refused before any device work.

    Returns dict(errors (len(r) x len(rx) x len(ry): the fold-mean RMSEP, NaN where any fold failed),
    per_fold, cond, steps (each K x grid), failed (bool, K x grid), which_error (index triple or None),
    best ((r, rx, ry) or None), time, class="cvPO2PLS"), with ``return_fits`` also ``fits`` (K lists in grid
    order of estimates dicts or None) and ``grid``.  A NaN cell never wins while a finite cell exists.

    ``X = Y = None`` with a context streamed with ``nr_folds`` folds runs on the stream's folds.  With resident
    rows (``X``, ``Y`` or a context that holds rows) the rows are streamed, device to device and as they
    are loaded (no centring or scaling), into a fold stream on a second context of the call, which then takes
    the same path; the source is left untouched.  Warns about cancellation as ``cv_PPLS`` does."""
    tic = time.perf_counter()
    rs, rxs, rys = ([int(v) for v in np.atleast_1d(a)] for a in (r, rx, ry))
    K = int(nr_folds)
    if K < 2:
        raise ValueError("Cross-validation with 1 fold does not make sense, use 2 folds or more")
    if not rs or not rxs or not rys:
        raise ValueError("r, rx and ry must each hold at least one value")
    t = _orth_type(type)
    streamed = X is None and ctx is not None and bool(ctx._stream_folds)
    if streamed:
        if K != int(ctx._stream_folds):
            raise ValueError(f"nr_folds={K}, but the rows were streamed with {ctx._stream_folds} folds")
        if folds is not None:
            raise ValueError("folds= cannot be given: the folds are those the rows were streamed with")
        src = ctx
    else:
        src = _ctx_with(X, Y, ctx)
    p, q = src.p, src.q
    grid = [(a, b, c) for a in rs for b in rxs for c in rys]
    for a, b, c in grid:     # the library's limits, checked before any device work
        if a < 1 or b < 0 or c < 0 or a + b > min(16, p) or a + c > min(16, q):
            raise ValueError(f"grid cell (r, rx, ry) = {(a, b, c)} outside r >= 1, rx, ry >= 0, r + rx <= min(16, p={p}), "
                             f"r + ry <= min(16, q={q})")
    if len(grid) > 256:
        raise ValueError(f"{len(grid)} grid cells: one batch holds at most 256")
    rng = rng if rng is not None else np.random.default_rng()
    own = None
    try:
        if streamed:
            cv = src
        else:
            fold_of = fold_labels(int(src.n_total), K, folds, rng)
            lo = int(src.row0)
            cv = own = Context(src.device)
            cv.stream_begin(p, q, False, False, nr_folds=K)
            cv.stream_rows_from(src, fold=fold_of[lo: lo + src.n_local])
            cv.stream_end()
        V0x, V0y = rng.standard_normal((p, max(rxs))), rng.standard_normal((q, max(rys)))
        res = cv.po2_cv_stream(grid, int(EMsteps), float(atol), t, V0x, V0y, int(start_steps), want_fits=return_fits)
    finally:
        if own is not None:
            own.close()
    shape = (K, len(rs), len(rxs), len(rys))
    per_fold, cond, steps = (res[k].reshape(shape) for k in ("rmsep", "cond", "steps"))
    failed = res["status"].reshape(shape) != 0
    with np.errstate(invalid="ignore"):
        lost = np.argwhere(np.abs(res["cond"]) * 64 * 2.0 ** -53 > _COND_LIMIT)
    for f, j in lost:
        warnings.warn(f"fold {int(f)}, (r, rx, ry) = {grid[int(j)]}: the held-out error from cross-products keeps "
                      f"few digits (mag / sse = {res['cond'][f, j]:.3g})")
    errors, which = select_grid_PO2PLS(per_fold, failed)
    out = {"errors": errors, "per_fold": per_fold, "cond": cond, "steps": steps, "failed": failed, "which_error": which,
           "best": None if which is None else (rs[which[0]], rxs[which[1]], rys[which[2]]),
           "time": time.perf_counter() - tic, "class": "cvPO2PLS"}
    if return_fits:
        out["grid"] = grid
        out["fits"] = [[None if th is None else th.as_dict() for th in f] for f in res["fits"]]
    return out


def cv_PO2PLS(X, Y, r, rx, ry, nr_folds, folds=None, rng=None, ctx=None, per_fold=False, **args):
    """The cross-validated RMSEP of Y predicted from X by one PO2PLS model (r, rx, ry): ``crossval_PO2PLS``
    on a grid of one cell (its ``EMsteps``, ``atol``, ``type``, ``start_steps``).  Returns the fold mean (NaN
    when a fold failed), with ``per_fold=True`` also the per-fold errors."""
    res = crossval_PO2PLS(X, Y, [int(r)], [int(rx)], [int(ry)], nr_folds, folds=folds, rng=rng, ctx=ctx, **args)
    err = float(res["errors"][0, 0, 0])
    return (err, res["per_fold"][:, 0, 0, 0].copy()) if per_fold else err


def scores_PO2PLS(fit, X=None, Y=None, ctx=None):
    """The posterior means of the latent variables of the rows, [X Gx | Y Gy] K (n_local x k, columns
    in the order t, t_o, u, u_o), by the ``ppls_scores`` pass with zero-padded columns and K on the host.
    Refused (PPLS_E_STATE) on a context that holds no rows."""
    ctx = _ctx_with(X, Y, ctx)
    e = fit["estimates"]
    Gx, Gy = np.hstack([e["W"], e["Wo"]]), np.hstack([e["C"], e["Co"]])
    kx, ky = Gx.shape[1], Gy.shape[1]
    km = max(kx, ky)
    Gxp, Gyp = np.zeros((ctx.p, km)), np.zeros((ctx.q, km))
    Gxp[:, :kx], Gyp[:, :ky] = Gx, Gy
    T, Us = ctx.scores(Gxp, Gyp)
    return np.hstack([T[:, :kx], Us[:, :ky]]) @ np.asarray(fit["Expectations"]["K"])


def _po2_fit_theta(fit):
    if isinstance(fit, Po2Theta):
        return fit
    if isinstance(fit, dict):
        return Po2Theta.from_dict(fit["estimates"] if "estimates" in fit else fit)
    raise ValueError("pass a PO2PLS fit, its estimates or a Po2Theta")


def diagnostics_PO2PLS(fit, X=None, Y=None, ctx=None, subset=None, new=False, rescale=False, alpha=0.01, adjust="none",
                       want_mu=False, Z=None):
    """``diagnostics_PPLS`` for a PO2PLS fit: per row, in one pass over the rows on the GPU, the
    squared distances ``odx2``, ``ody2`` to the planes of [W Wo] and [C Co], the distance ``sd2`` of the
    k = 2r + rx + ry scores under their dense covariance, ``d2``, the log-density ``loglik`` (it sums to
    ``PO2PLS_logl``) and, with ``want_mu``, the posterior means ``mu`` (n x k: t, to, u, uo).  ``df`` is
    p - kx, q - ky, kx + ky and p + q; ``pvalue``, ``flag``, ``outliers`` and every other argument are
    ``diagnostics_PPLS``'s.  ``fit``: a PO2PLS fit, its ``estimates`` or a ``Po2Theta``; the loadings need not
    be orthonormal."""
    if adjust not in ("none", "bonferroni"):
        raise ValueError("adjust should be one of \"none\", \"bonferroni\"")
    th = _po2_fit_theta(fit)
    p, q, kx, ky = th.W.shape[0], th.C.shape[0], th.r + th.rx, th.r + th.ry
    res = _diagnostics_rows(p, q, X, Y, ctx, subset, new, rescale, Z,
                            lambda c, rows: c.po2_row_diagnostics(th, rows=rows, want_mu=want_mu),
                            lambda c, Xn, Yn: c.po2_row_diagnostics_new(th, Xn, Yn, want_mu=want_mu))
    out = dict(res)
    out.update(diagnostics_summary(res, p, q, th.r, th.sigE, th.sigF, alpha=alpha, adjust=adjust,
                                   df=dict(odx2=p - kx, ody2=q - ky, sd2=kx + ky, d2=p + q)))
    return out


def robust_PO2PLS(X, Y, r, rx, ry, nu=4.0, outer=50, inner=5, atol=1e-4, type="SVD", init=None, ctx=None, work=None,
                  rng=None):
    """PO2PLS under the multivariate-t model with ``nu`` degrees of freedom: ``robust_PPLS_simult``'s loop
     with the PO2PLS distances and M-step.  From theta (``init``: a dict as for
    ``PO2PLS``, default the estimates of ``PO2PLS(X, Y, r, rx, ry)`` on the same context) it repeats:
    (1) ``ctx.po2_robust_weights`` -- d2_i, u_i = (nu + p + q) / (nu + d2_i) and the t log-likelihood at theta;
    (2) ``work.xprod_weighted(ctx)`` -- S_u = sum u_i d_i d_i' with ``n_total = N``; (3) ``inner`` forced ECM
    steps of ``work.po2_em_run``, warm-started at theta.  The stop rule, ``nu="estimate"``, ``X``, ``Y``,
    ``ctx`` and ``work`` are ``robust_PPLS_simult``'s; ``rng`` draws the default start's specific loadings, as
    in ``PO2PLS``.

    Returns ``dict(estimates, loglik, nu, weights, d2, steps, converged, gaussian)``: ``estimates`` in PO2PLS's
    canonical form; ``gaussian`` the starting PO2PLS fit (None when ``init`` was given)."""
    estimate = isinstance(nu, str)
    if estimate and nu != "estimate":
        raise ValueError("nu must be a positive number or 'estimate'")
    if not estimate and not (np.isfinite(nu) and nu > 0):
        raise ValueError(f"nu = {nu} must be positive and finite")
    if outer < 1 or inner < 1:
        raise ValueError(f"outer = {outer}, inner = {inner} must be at least 1")
    ctx = _ctx_with(X, Y, ctx)
    t = _orth_type(type)
    gauss = None
    if init is None:
        gauss = PO2PLS(None, None, r, rx, ry, type=type, rng=rng, ctx=ctx)
        init = gauss["estimates"]
    th = Po2Theta.from_dict(init)
    if (th.r, th.rx, th.ry) != (int(r), int(rx), int(ry)):
        raise ValueError(f"init has (r, rx, ry) = {(th.r, th.rx, th.ry)}, asked for {(int(r), int(rx), int(ry))}")

    def estep(th):
        if not estimate:
            return float(nu), float(ctx.po2_robust_weights(th, nu)[0][0])
        lo, hi = 1.0, 1000.0
        for _ in range(4):
            grid = t_nu_grid(lo, hi)
            k = int(np.argmax(ctx.po2_robust_weights(th, grid)[0]))
            lo, hi = t_nu_bracket(grid, k)
        return float(grid[k]), float(ctx.po2_robust_weights(th, grid[k])[0][0])   # keeps the weights of the chosen nu

    own = work is None
    work = Context(ctx.device) if own else work
    ll, steps, converged = [], 0, False
    try:
        while True:
            nu_k, l = estep(th)
            ll.append(l)
            if len(ll) > 1 and ll[-1] - ll[-2] < atol:
                converged = True
                break
            if steps >= outer:
                break
            work.xprod_weighted(ctx)
            th = work.po2_em_run(th, int(inner), -np.inf, t, want_eout=False)[0]
            steps += 1
    finally:
        if own:
            work.close()
    w, d2 = ctx.robust_get()
    return {"estimates": th.as_dict(), "loglik": np.array(ll), "nu": nu_k, "weights": w, "d2": d2, "steps": steps,
            "converged": converged, "gaussian": gauss, "class": "robust_PO2PLS"}
