"""The definition of `-A qmse` (quantisation-MSE clip search on the |x| histogram), as a numpy model.

The error-driven sibling of the percentile and the entropy search: take the centres of the bins, fake-quantise them on the
platform's own grid for every candidate clip, keep the clip of least weighted squared error.  (The reference's `mse` is OCTAV, a
per-image fixed point, not a search; this one is this project's, and its kernel — `k_hist_qmse`, csrc/calib_kernels.hip — is held
to this file.)  Per tensor: `h` = int64 [bins] |x| histogram (what `-A hist` accumulates), N = sum h; `first`, the lowest
candidate; a grid G of non-negative values whose largest is `top`:

  * uniform ("Linear"): G = {0, 1, ..., top}, top = 2 ** (bit_width - 1) - 1 (quantize._symmetric_grid's);
  * E4M3 ("Float8E4M3FN"): G = the 127 non-negative finite codes (fp8_model.e4m3_codes()), top = 448.

Everything in units of HALF a bin width: the centre of bin b is m = 2 b + 1; candidate i in [first, bins] — "clip at the centre
of bin i - 1", the value the percentile search stores for that bin — is t = 2 i - 1, its scale s = t / top.  For every bin
u = m top / t (an exact rational), Q = the point of G nearest to min(u, top) (saturation is the same formula), d = u - Q, and

    out[i] = (t / (2 top))^2 * sum_b h[b] d_b^2 / N        the mean squared error, in bin widths^2

out[i] = +inf for i < first, and everywhere when N = 0.  i* = the lowest i of least out (-1: none is finite, and then the clip is
the range); the clip is kl_model.kl_clip_from_best(i*, gmin, gmax, bins).  "Nearest" needs no tie rule: a tie needs
2 m top = (2 k + 1) t on the uniform grid — even against odd, t being odd — and 2^16 * 7 m = (2 k + 1) 2^(e + 6) t between two
E4M3 codes of binade e <= 8, where the powers of two differ.

Two statements: `qmse_curve` — exact integer arithmetic (d t on the uniform grid and 512 d t on E4M3 are integers, and so are
the comparisons that find Q; only the weighted sum is fp64) — and `qmse_curve_fp64` — plain fp64 per bin, (b + 0.5) - Q s with
fp8_model's binade / rint rule for E4M3.  tests/test_qmse_model.py holds them to each other.
"""
import numpy as np

from fp8_model import E4M3_MAX, e4m3_codes
from kl_model import kl_best, kl_clip_from_best

UNIFORM, E4M3 = "Linear", "Float8E4M3FN"


def grid_of(qtype, bit_width=8):
    """-> (grid name, top) of a platform's qi_params type."""
    if qtype == UNIFORM:
        return UNIFORM, 2 ** (int(bit_width) - 1) - 1
    if qtype == E4M3:
        return E4M3, int(E4M3_MAX)
    raise ValueError(f"no grid modelled for quantisation type {qtype!r}")


def qmse_curve(h, first, grid=UNIFORM, top=127):
    """Statement (a): out[i], i in [0, bins].  Integers throughout; the sum over the bins is fp64."""
    h = np.asarray(h, np.int64)
    bins = h.size
    N = int(h.sum())
    out = np.full(bins + 1, np.inf)
    if N == 0:
        return out
    nz = np.nonzero(h)[0]
    w = h[nz].astype(np.float64)                                   # (exact: counts stay far below 2^53)
    m = 2 * nz + 1
    if grid == UNIFORM:
        unit, a = 1, m * int(top)                                  # a = m top
    else:
        codes = np.rint(e4m3_codes().astype(np.float64) * 512).astype(np.int64)       # 512 G: integers, the last is 512 * 448
        mids = codes[:-1] + codes[1:]                              # 1024 * the midpoints of neighbouring codes
        unit, top = 512, int(E4M3_MAX)
        a = m * (512 * top)                                        # a = 512 m top
    for i in range(int(first), bins + 1):
        t = 2 * i - 1
        if grid == UNIFORM:
            q = np.minimum((2 * a + t) // (2 * t), top)            # floor(u + 1/2), saturated
        else:
            q = codes[np.searchsorted(mids * t, 2 * a)]            # codes below u: those whose midpoint to the next lies below u
        dt = a - q * t                                             # unit * d * t, exact
        out[i] = float(np.sum(w * (dt.astype(np.float64) ** 2))) / float(N * 4 * (unit * top) ** 2)
    return out


def qmse_curve_fp64(h, first, grid=UNIFORM, top=127):
    """Statement (b): the same in bin widths and plain fp64 — centre b + 0.5, scale s = (i - 0.5) / top, error (b + 0.5) - Q s."""
    h = np.asarray(h, np.int64)
    bins = h.size
    N = float(h.sum())
    out = np.full(bins + 1, np.inf)
    if N == 0:
        return out
    if grid != UNIFORM:
        top = E4M3_MAX
    c = np.arange(bins, dtype=np.float64) + 0.5
    hf = h.astype(np.float64)
    for i in range(int(first), bins + 1):
        s = (i - 0.5) / top
        v = np.minimum(c / s, top)
        if grid == UNIFORM:
            q = np.rint(v)
        else:
            _, ex = np.frexp(v)                                    # v = f * 2^ex, f in [0.5, 1): binade ex - 1
            step = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
            q = np.rint(v / step) * step
        e = c - q * s
        out[i] = np.sum(hf * e * e) / N
    return out


def qmse_clip(h, gmin, gmax, first, grid=UNIFORM, top=127):
    """-> (clip fp32 [2], i*, curve) by statement (a)."""
    curve = qmse_curve(h, first, grid, top)
    best = kl_best(curve)
    return kl_clip_from_best(best, gmin, gmax, np.asarray(h).size), best, curve
