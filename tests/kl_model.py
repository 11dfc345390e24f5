"""The definition of `-A kl` (entropy / KL-divergence clip search on the |x| histogram), as an fp64 numpy model.

The reference never shipped a KL search (its `--bins` help still reads "bins for histogram and kl"), so this project defines one
and holds its kernel (`k_hist_kl`, csrc/calib_kernels.hip) to it.  Per tensor: `h` = int64 [bins] |x| histogram (what `-A hist`
accumulates), `levels` L = 2 ** (bit_width - 1) of the platform's qi_params, eps = 1e-4.  For every candidate i in [L, bins] —
"keep bins [0, i)":

  * reference distribution p = h[:i] with the outliers h[i:] folded into the last kept bin;
  * quantised distribution q: the i bins are dealt to L groups (group j = bins [j*i // L, (j+1)*i // L)), a group's mass — WITHOUT
    the outliers — is spread evenly over its bins where p != 0;
  * both are smoothed (zeros -> eps, the mass taken evenly from the non-zeros; a candidate where that would take 1 or more from
    every non-zero bin, or that has no non-zero bin, is not admissible), normalised, and out[i] = sum P log(P / Q).

i* = the LOWEST i with minimal out[i] (NaN never wins); the clip value is the centre of the last kept bin, in fp32 exactly as the
percentile search ends (k_hist_percentile).  Two statements of the curve: `kl_curve` (vectorised) and `kl_curve_scalar` (a loop
per bin, nothing shared with the first but the definition); tests/test_kl_model.py holds them to each other.
"""
import math

import numpy as np

EPS = 1e-4


def kl_curve(h, L, eps=EPS):
    """out[i], i in [0, bins]: the divergence of candidate i; +inf where i < L or the candidate is not admissible."""
    h = np.asarray(h, np.int64)
    bins = h.size
    N = int(h.sum())
    out = np.full(bins + 1, np.inf)          # out[i]: keep bins [0, i); +inf = not admissible
    cs = np.concatenate([[0], np.cumsum(h)])
    for i in range(L, bins + 1):
        outl = N - int(cs[i])
        p = h[:i].astype(np.float64)
        p[i - 1] += outl                     # reference distribution: outliers folded into the last kept bin
        nz = p != 0
        starts = (np.arange(L + 1, dtype=np.int64) * i) // L      # group j = bins [starts[j], starts[j+1])
        gid = np.searchsorted(starts, np.arange(i), side='right') - 1      # == ((b + 1) * L - 1) // i
        G = (cs[starts[1:]] - cs[starts[:-1]]).astype(np.float64)  # group sums of h — WITHOUT the outliers
        c = np.bincount(gid, weights=nz, minlength=L)             # bins of the group where p != 0
        q = np.where(nz, G[gid] / np.maximum(c[gid], 1), 0.0)     # quantised to L levels, expanded back
        ds = []
        for d in (p, q):                                           # smoothing: zeros -> eps, the mass taken from the non-zeros
            n1 = int((d != 0).sum())
            z = i - n1
            if n1 == 0:
                break
            e1 = eps * z / n1
            if not e1 < 1.0:
                break
            ds.append(np.where(d != 0, d - e1, eps))
        if len(ds) < 2:
            continue                                               # candidate not admissible
        P = ds[0] / ds[0].sum()
        Q = ds[1] / ds[1].sum()
        with np.errstate(invalid="ignore", divide="ignore"):       # (a smoothed value below zero: NaN, which never wins)
            out[i] = np.sum(P * np.log(P / Q))
    return out


def kl_curve_scalar(h, L, eps=EPS):
    """The same definition bin by bin in plain Python floats (slow: for small histograms)."""
    h = [int(v) for v in np.asarray(h, np.int64)]
    bins = len(h)
    N = sum(h)
    out = [math.inf] * (bins + 1)
    for i in range(L, bins + 1):
        p = [float(v) for v in h[:i]]
        p[i - 1] += float(N - sum(h[:i]))
        q = [0.0] * i
        for j in range(L):
            lo, hi = (j * i) // L, ((j + 1) * i) // L
            mass, live = 0, 0
            for b in range(lo, hi):
                mass += h[b]
                live += 1 if p[b] != 0 else 0
            for b in range(lo, hi):
                if p[b] != 0:
                    q[b] = float(mass) / max(live, 1)
        smoothed = []
        for d in (p, q):
            n1 = sum(1 for v in d if v != 0)
            if n1 == 0:
                break
            e1 = eps * (i - n1) / n1
            if not e1 < 1.0:
                break
            smoothed.append([v - e1 if v != 0 else eps for v in d])
        if len(smoothed) < 2:
            continue
        sp, sq = math.fsum(smoothed[0]), math.fsum(smoothed[1])
        terms = []
        for a, b in zip(smoothed[0], smoothed[1]):
            P, Q = a / sp, b / sq
            terms.append(P * math.log(P / Q) if P / Q > 0 else math.nan)
        out[i] = math.fsum(terms) if not any(math.isnan(t) for t in terms) else math.nan
    return np.asarray(out, np.float64)


def kl_best(curve):
    """i*: the lowest index with minimal divergence (NaN never wins); -1 when no candidate is admissible."""
    c = np.where(np.isnan(curve), np.inf, np.asarray(curve, np.float64))
    i = int(np.argmin(c))                    # (the first occurrence of the minimum)
    return i if np.isfinite(c[i]) else -1


def py_max(a, b):
    return b if b > a else a                 # python max(a, b)


def py_min(a, b):
    return b if b < a else a


def kl_clip_from_best(best, gmin, gmax, bins):
    """fp32 [lo, hi] given i* (-1: none -> [gmin, gmax]): cv = fl32(i* - 1 + 0.5) * fl32(dmax / bins)."""
    gmin, gmax = np.float32(gmin), np.float32(gmax)
    if best < 0:
        return np.array([gmin, gmax], np.float32)
    dmax = py_max(np.float32(-gmin), gmax)
    cv = np.float32(np.float32(best - 1) + np.float32(0.5)) * np.float32(dmax / np.float32(bins))
    return np.array([py_max(np.float32(-cv), gmin), py_min(cv, gmax)], np.float32)


def kl_clip(h, gmin, gmax, L, eps=EPS):
    """-> (clip fp32 [2], i*, curve)."""
    curve = kl_curve(h, L, eps)
    best = kl_best(curve)
    return kl_clip_from_best(best, gmin, gmax, np.asarray(h).size), best, curve


# ------------------------------------------------------------------------------------------------ seeded fixtures
def abs_hist(x, bins):
    """(int64 [bins] histogram of |x| over (0, max |x|), gmin, gmax) — np.histogram, as `-A hist` accumulates it."""
    x = np.asarray(x, np.float32)
    gmin, gmax = np.float32(x.min()), np.float32(x.max())
    dmax = py_max(gmax, np.float32(-gmin))
    h, _ = np.histogram(np.abs(x), int(bins), (0, dmax))
    return h.astype(np.int64), gmin, gmax


def fixture_tensor(kind):
    """The tensors the definition was looked at on (seeds fixed) plus a two-level and a heavy-zero one."""
    rng = np.random.default_rng([0x4B4C, sum(kind.encode())])
    if kind == "normal":
        return rng.standard_normal(802816, dtype=np.float32)
    if kind == "relu":           # ~50 % exact zeros
        return np.maximum(rng.standard_normal(802816, dtype=np.float32), np.float32(0))
    if kind == "laplace":
        return rng.laplace(0.0, 1.0, 200704).astype(np.float32)
    if kind == "uniform":
        return rng.uniform(-1.0, 1.0, 100352).astype(np.float32)
    if kind == "outliers":       # five values far outside a normal body
        x = rng.standard_normal(401408, dtype=np.float32)
        x[:5] = np.array([78.0, -61.0, 55.5, 70.25, -66.0], np.float32)
        return x
    if kind == "lognormal":
        return rng.lognormal(0.0, 1.2, 200704).astype(np.float32)
    if kind == "small":
        return rng.standard_normal(1000, dtype=np.float32)
    if kind == "constant":
        return np.full(4096, 1.5, np.float32)
    if kind == "zeros":
        return np.zeros(4096, np.float32)
    if kind == "two_level":
        x = np.full(65536, 0.75, np.float32)
        x[::4] = np.float32(-3.0)
        return x
    if kind == "heavy_zero":     # ReLU of a shifted normal: half of the elements exactly zero, the rest a wide half-bell
        return np.maximum(rng.standard_normal(401408, dtype=np.float32) * np.float32(2.5), np.float32(0))
    raise ValueError(kind)


KINDS = ("normal", "relu", "laplace", "uniform", "outliers", "lognormal", "small", "constant", "zeros", "two_level", "heavy_zero")
DEGENERATE = ("constant", "zeros")       # exact ties at 0 (or no admissible candidate): checked by clip only
