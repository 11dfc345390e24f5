"""numpy model of the range pass's histogram speculation (csrc/calib_kernels.hip, K2s) — the definition the device is held to.

np.histogram(|x|, bins, (0, dmax)) depends on the shard's range through dmax alone.  The range pass histograms batch k of tensor
t against the RUNNING dmax (what batches 0 .. k-1 gave); that histogram is the final one iff the running dmax IS the final dmax,
bit for bit, and numpy accepts the range.  `valid_table` says for which (batch, tensor) pairs that holds; `partition` cuts the
element stream of the tensors that must still be read into equal shares, as dpl_build_balanced_items cuts the whole set.
"""
import numpy as np

F32 = np.float32
ALIGN = 1024        # cuts inside a tensor fall on multiples of this many elements from the tensor's start


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def running_dmax(batch_dmax):
    """[K, T] per-batch dmax (= max(max, -min) of the batch; NaN when the batch holds a NaN) -> [K, T]: the dmax of batches
    0 .. k-1, NaN for k = 0 (no data, no guess) and from the first NaN batch on (numpy's max / min propagate NaN)."""
    d = np.asarray(batch_dmax, F32)
    run = np.full(d.shape, np.nan, F32)
    for k in range(1, d.shape[0]):
        prev, cur = run[k - 1], d[k - 1]
        if k == 1:
            run[k] = cur
        else:
            with np.errstate(invalid="ignore"):
                run[k] = np.where(np.isnan(prev) | np.isnan(cur), F32(np.nan), np.where(cur > prev, cur, prev))
    return run


def valid_table(batch_dmax, final_dmax, range_ok=None):
    """valid[k, t]: the range pass's histogram of batch k, tensor t is the final one — the running dmax equals final_dmax[t] in
    every bit, is finite and non-negative, and (range_ok[t], default all True) numpy can cut the final range into the bins."""
    run = running_dmax(batch_dmax)
    fin = np.asarray(final_dmax, F32)
    ok = np.isfinite(fin) & (fin >= 0)
    if range_ok is not None:
        ok &= np.asarray(range_ok, bool)
    return (_bits(run) == _bits(fin)[None, :]) & ok[None, :] & ~np.isnan(run)


def cuts(elems, skip, n_blocks):
    """Positions of the n_blocks + 1 cuts in the stream of the tensors still to be read: cut b = floor(total * b / n_blocks),
    rounded down to a multiple of ALIGN elements from the start of the tensor it falls in; cut n_blocks = total."""
    rem = [0 if s else int(e) for e, s in zip(elems, skip)]
    P = [0]
    for r in rem:
        P.append(P[-1] + r)
    total = P[-1]
    out = []
    for b in range(n_blocks + 1):
        target = total if b == n_blocks else (total * b) // n_blocks
        if target >= total:
            out.append(total)
            continue
        t = max(i for i in range(len(rem)) if P[i] <= target and rem[i] > 0 and target < P[i + 1])
        out.append(P[t] + ((target - P[t]) // ALIGN) * ALIGN)
    return out


def partition(elems, skip, n_blocks):
    """-> per block a list of (tensor, offset, count): the pieces of [cut b, cut b + 1), split at tensor boundaries."""
    rem = [0 if s else int(e) for e, s in zip(elems, skip)]
    P = [0]
    for r in rem:
        P.append(P[-1] + r)
    c = cuts(elems, skip, n_blocks)
    blocks = []
    for b in range(n_blocks):
        pos, end, items = c[b], c[b + 1], []
        t = 0
        while pos < end:
            while P[t + 1] <= pos:
                t += 1
            stop = min(end, P[t + 1])
            items.append((t, pos - P[t], stop - pos))
            pos = stop
        blocks.append(items)
    return blocks


def skipped_share(valid, elems):
    """Share of the histogram pass's bytes that need not be read: sum over valid pairs of the tensor's elements / all pairs'."""
    v = np.asarray(valid, bool)
    e = np.asarray(elems, np.float64)
    return float((v * e[None, :]).sum() / (v.shape[0] * e.sum()))
