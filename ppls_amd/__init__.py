"""ppls_amd -- MI355X-native (gfx950) EM inner loop of PPLS_simult (selbouhaddani/PPLS).

The product is the C-ABI library ``libppls_amd.so`` (include/ppls.h, HIP kernels in csrc/);
this package is its Python host binding plus the mirror of the reference's R interface.
"""
from ._lib import PPLS_ORTH_QR, PPLS_ORTH_SVD, Expect, Po2Expect, Po2Theta, PplsError, Theta  # noqa: F401
from .api import (PPLS, Context, Expect_M, Maximiz_M, PPLS_simult, PPLS_simult_to_o2m, PPLS_to_o2m, PPLSi,  # noqa: F401
                  default_context, fconstraint, initial_guess, logl_W, loglC_fast, meta_EMstep, meta_PPLSi,
                  print_PPLS, random_theta0, scores_PPLS, variances_PPLS_simult, cv_blocks, predict_PPLS, cv_PPLS,
                  crossval_PPLS, scale_data, adjust_data, adjust_new, stream_data, fold_labels, population_labels, bootstrap_counts,
                  align_signs, bootstrap_summary, bootstrap_PPLS_simult, permutation_indices, permutation_pvalues,
                  permutation_PPLS, diagnostics_PPLS, robust_PPLS_simult, PO2PLS, PO2PLS_Expect, PO2PLS_logl,
                  simulate_PO2PLS, scores_PO2PLS, summary_PO2PLS, canonical_PO2PLS, po2_predict_map, predict_PO2PLS,
                  cv_PO2PLS, crossval_PO2PLS, diagnostics_PO2PLS, robust_PO2PLS)

__all__ = ["Context", "fconstraint", "Expect_M", "Maximiz_M", "PPLS_simult", "PPLS", "PPLSi", "initial_guess", "print_PPLS", "scores_PPLS",
           "PPLS_simult_to_o2m", "PPLS_to_o2m", "meta_EMstep", "meta_PPLSi", "variances_PPLS_simult", "logl_W", "loglC_fast", "Theta",
           "Expect", "PplsError", "random_theta0", "default_context", "PPLS_ORTH_SVD", "PPLS_ORTH_QR",
           "cv_blocks", "predict_PPLS", "cv_PPLS", "crossval_PPLS", "scale_data", "adjust_data", "adjust_new", "stream_data", "fold_labels", "population_labels",
           "bootstrap_counts", "align_signs", "bootstrap_summary", "bootstrap_PPLS_simult", "permutation_indices",
           "permutation_pvalues", "permutation_PPLS", "diagnostics_PPLS", "robust_PPLS_simult", "PO2PLS", "PO2PLS_Expect",
           "PO2PLS_logl", "simulate_PO2PLS", "scores_PO2PLS", "summary_PO2PLS", "canonical_PO2PLS", "po2_predict_map",
           "predict_PO2PLS", "cv_PO2PLS", "crossval_PO2PLS", "diagnostics_PO2PLS", "robust_PO2PLS"]
