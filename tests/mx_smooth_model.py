"""The definition of dpl_mx_smooth_err / ops.mx_smooth_err (`--smooth_search`) in numpy.  For candidate c: A = the MX Q/DQ
(tests/mx_model.py) of the fp32 quotient x / s[c], B = that of the fp32 product w * s[c], C = A . B^T summed in fp64 and rounded to
fp32 — the matrix instruction's accumulator bit for bit where every partial sum is an exact fp32 number, within
tests/mx_gemm_model.py's bound of it elsewhere —, and the per-tile sums of tests/mx_mixed_model.py gemm_err_partials."""
import numpy as np

import mx_mixed_model as X
import mx_model as M


def scaled(x, w, s_row):
    s_row = np.asarray(s_row, np.float32)
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float32) / s_row, np.asarray(w, np.float32) * s_row


def product(x, w, s_row, elem):
    a, b = (M.fake_quant_mx(v, -1, elem).astype(np.float64) for v in scaled(x, w, s_row))
    with np.errstate(all="ignore"):
        return (a @ b.T).astype(np.float32)


def smooth_err_partials(x, w, s, ref, elem):
    """-> fp64 [n_cand, tiles_m, tiles_n, 2]."""
    return np.stack([X.gemm_err_partials(product(x, w, row, elem), ref) for row in np.asarray(s, np.float32)])
