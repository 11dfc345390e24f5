"""The definition of `--mx_mixed` (dipoorlet_amd/mx_mixed.py): what dpl_mx_gemm_err / ops.mx_gemm_err sums, in the order it sums
it, and which nodes are promoted from MXFP4 to MXFP8 under a weight-bit budget.

gemm_err_partials   from a GIVEN fp32 C (tests/mx_gemm_model.py defines C; on the device it is k_mx_gemm's accumulator, bit for
                    bit): per 64 x 64 tile of C, [sum of d * d, sum of ref * ref] over the tile's elements inside the arrays, d =
                    (C + bias[col]) - ref in fp32 (two roundings; no bias: C - ref), each square taken in fp64, where it is exact.
                    The ORDER of the fp64 additions is part of the definition.  Wave w of the tile's four owns rows 32 (w >> 1) ..
                    and columns 32 (w & 1) .. of it.  Lane l of a wave adds its 16 terms one after the other, over (i, reg, j)
                    nested in that order, the term's row being 16 i + 4 (l >> 4) + reg and its column 16 j + (l & 15) of the
                    quadrant; a term outside the arrays is +0.0.  The 64 lane sums fold pairwise, e = e[0::2] + e[1::2], six times
                    (xor-shuffles 1, 2, 4, 8, 16, 32); the four wave sums are added as (w0 + w1) + (w2 + w3).
choose              start with every candidate at mxfp4; gain = e4 - e8, cost = 4 bits for each of the weight's elements; drop the
                    candidates whose gain is <= 0 or not finite; order by gain / cost descending, ties in graph order; walk the
                    list once and promote a node when the promoted costs so far plus its own stay <= (bits - 4) * (the elements of
                    ALL candidates); a node that does not fit is skipped and the walk goes on.
"""
import numpy as np

TILE = 64
BASE, WIDE = "mxfp4", "mxfp8"
ELEM_BITS = {BASE: 4, WIDE: 8}


def gemm_err_terms(c, ref, bias=None):
    """-> (d * d, ref * ref) as fp64 [*batch, m, n]: the terms, before any addition."""
    c, ref = np.asarray(c, np.float32), np.asarray(ref, np.float32)
    assert c.shape == ref.shape and c.ndim >= 2
    with np.errstate(invalid="ignore", over="ignore"):
        v = c if bias is None else c + np.asarray(bias, np.float32)            # one fp32 rounding
        d = (v - ref).astype(np.float64)                                       # another
        r = ref.astype(np.float64)
        return d * d, r * r


def _in_kernel_order(t):
    """fp64 [B, m, n] terms -> [B, tiles_m, tiles_n, wave 4, lane 64, term 16], +0.0 outside the arrays."""
    b, m, n = t.shape
    tm, tn = -(-m // TILE), -(-n // TILE)
    p = np.zeros((b, tm * TILE, tn * TILE), np.float64)
    p[:, :m, :n] = t
    #       b, tm, wave row, i, lane >> 4, reg, tn, wave column, j, lane & 15
    p = p.reshape(b, tm, 2, 2, 4, 4, tn, 2, 2, 16)
    #       b, tm, tn, wave row, wave column, lane >> 4, lane & 15, i, reg, j
    p = p.transpose(0, 1, 6, 2, 7, 4, 9, 3, 5, 8)
    return p.reshape(b, tm, tn, 4, 64, 16)


def _sum_in_kernel_order(t):
    e = _in_kernel_order(t)
    lane = np.zeros(e.shape[:-1], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(16):
            lane = lane + e[..., k]
        for _ in range(6):
            lane = lane[..., 0::2] + lane[..., 1::2]
        w = lane[..., 0]
        return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def gemm_err_partials(c, ref, bias=None):
    """c, ref fp32 [*batch, m, n], bias None or fp32 [n] -> fp64 [*batch, tiles_m, tiles_n, 2]."""
    dd, rr = gemm_err_terms(c, ref, bias)
    lead, (m, n) = dd.shape[:-2], dd.shape[-2:]
    out = np.stack([_sum_in_kernel_order(t.reshape((-1, m, n))) for t in (dd, rr)], axis=-1)
    return out.reshape(lead + out.shape[1:])


def relative_error(partials):
    """sum d^2 / sum ref^2 of a node from all its partials, added in fp64 (tiles in their own order)."""
    p = np.asarray(partials, np.float64).reshape(-1, 2)
    num = den = 0.0
    for a, b in p:
        num, den = num + float(a), den + float(b)
    return num / den if den > 0.0 else float("nan")


def choose(entries, bits):
    """entries: (name, e4, e8, elements) per candidate, in graph order -> {name: "mxfp4" or "mxfp8"}."""
    entries = list(entries)
    budget = (float(bits) - 4.0) * sum(int(e[3]) for e in entries)
    ranked = []
    for pos, (name, e4, e8, elements) in enumerate(entries):
        gain, cost = float(e4) - float(e8), 4 * int(elements)
        if np.isfinite(gain) and gain > 0.0:
            ranked.append((-(gain / cost), pos, name, cost))
    ranked.sort(key=lambda r: (r[0], r[1]))
    fmt = {e[0]: BASE for e in entries}
    spent = 0
    for _, _, name, cost in ranked:
        if spent + cost <= budget:
            spent += cost
            fmt[name] = WIDE
    return fmt


def average_bits(entries, fmt):
    """The element bits per weight element that a choice spends."""
    total = sum(int(e[3]) for e in entries)
    return sum(ELEM_BITS[fmt[e[0]]] * int(e[3]) for e in entries) / total if total else 4.0
