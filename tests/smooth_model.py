"""The definition of `--smooth` (per-channel activation scales folded into MatMul weights), as a numpy model.

The reference has no such transform: this is SmoothQuant's rescaling (Xiao et al., 2023) as THIS project defines it, and
dipoorlet_amd/weight_transform/smooth.py and its kernel (`k_colwise_absmax`, csrc/side_kernels.hip) are held to it.

  * statistic: for a channels-last activation x seen as [rows, C], the running a <- np.maximum(a, np.abs(x).max(0)), started at
    zero, over every batch of the calibration set.  NaN propagates (a NaN in a column, or already in a, stays), +-inf gives inf,
    -0.0 counts as +0.0;
  * scale: s_j = a_j^alpha / w_j^(1 - alpha) in fp64, cast to fp32, where w_j is the largest |W[j, :]| over every weight the
    activation is multiplied by; s_j = 1 where a_j < 1e-6 or w_j < 1e-6 (the guard of `--we`) and where the fp32 value is not
    finite or not positive;
  * fold: g <- g / s, b <- b / s (the LayerNorm affine T = Z * g + b), W[j, :] <- W[j, :] * s_j (column j of an [N, C] weight), all
    in fp32.  In real arithmetic (T / s) @ (s * W) = T @ W.

`smooth_scales` is written one channel at a time with Python floats: it shares nothing with the package's vectorised statement
but the definition.  The helpers below it build what the tests of both files need (planted outliers, numpy statistics).
"""
import math

import numpy as np


def colwise_absmax(acc, x):
    """The statistic of one batch: x of any rank >= 1, channels last."""
    x = np.asarray(x, np.float32)
    return np.maximum(np.asarray(acc, np.float32), np.abs(x.reshape(-1, x.shape[-1])).max(0))


def smooth_scales(a, w, alpha):
    out = np.ones(len(a), np.float32)
    for j, (aj, wj) in enumerate(zip(np.asarray(a, np.float64).tolist(), np.asarray(w, np.float64).tolist())):
        if aj < 1e-6 or wj < 1e-6:
            continue                        # the guard (a NaN is not below 1e-6: the finiteness test catches it)
        try:
            v = math.pow(aj, alpha) / math.pow(wj, 1.0 - alpha)
        except (OverflowError, ZeroDivisionError, ValueError):
            continue
        with np.errstate(all="ignore"):
            s = np.float32(v)
        if np.isfinite(s) and s > 0:
            out[j] = s
    return out


def fold(g, b, weights, s):
    """-> (g / s, b / s, [W * s along its C axis]); weights: [(W, transposed)], transposed = the weight is [N, C]."""
    s = np.asarray(s, np.float32)
    g, b = np.asarray(g, np.float32), np.asarray(b, np.float32)
    return g / s.reshape(g.shape), b / s.reshape(b.shape), [np.asarray(W, np.float32) * (s[None, :] if tr else s[:, None])
                                                           for W, tr in weights]


# ---------------------------------------------------------------------------------------------- helpers of the tests
MINI_VIT = dict(depth=2, dim=64, heads=4, mlp=128, image=32, patch=8, num_classes=10)


def mini_vit(seed=0):
    from dipoorlet_amd import models
    return models.vit(seed=seed, **MINI_VIT)


def plant_outliers(graph, sites, factor=16.0, channels=(3, 17, 30, 61)):
    """A copy of `graph` computing the same function with outlier channels in every site: g_j, b_j <- * factor and W[j, :] <- / factor
    on `channels` (a power of two: exact in fp32)."""
    from dipoorlet_amd.graph import ONNXGraph
    out = ONNXGraph()
    out.copy_from(graph)
    idx = np.asarray(channels)
    for site in sites:
        for name in (site.gamma, site.beta):
            v = np.array(out.get_initializer(name), np.float32)
            v.reshape(-1)[idx] *= np.float32(factor)
            out.set_initializer(name, v)
        for r in site.readers:
            w = np.array(out.get_initializer(r.weight), np.float32)
            if r.transposed:
                w[:, idx] /= np.float32(factor)
            else:
                w[idx, :] /= np.float32(factor)
            out.set_initializer(r.weight, w)
    out.update_model()
    return out


def site_statistics(session, sites, batches):
    """{site tensor: a} by the definition above from `session` (a GraphSession on any device) over `batches` of input images."""
    import torch
    names = [s.tensor for s in sites]
    acc = {s.tensor: np.zeros(s.channels, np.float32) for s in sites}
    for x in batches:
        outs = session.run_named({session.input_names[0]: torch.as_tensor(x)}, names)
        for n, t in zip(names, outs):
            acc[n] = colwise_absmax(acc[n], t.cpu().numpy())
    return acc


def same_bits(a, b):
    """Bit for bit, any NaN pattern equal to any other."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
