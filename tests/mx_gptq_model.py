"""The definition of `--mx_gptq` (GPTQ on the MX block-scaled grids), as a numpy model on top of tests/gptq_model.py (the recursion),
tests/mx_model.py (the floor rule, the element rounding) and tests/mx_scale_model.py (the Q/DQ under a given shared exponent).

W is [R, K], one output channel per row; MX blocks are 32 consecutive columns from column 0.  The recursion is gptq_model's with
one change: the grid of a block is fixed WHEN THE RECURSION ENTERS IT.  At every column c that is a multiple of 32, per row,
    a  = max |W[r, c : min(c + 32, K)]|        over the CURRENT values: every earlier column's compensation is already in them
    se = mx_model.shared_exponent(a)           (-127 for an all-zero block); the block's E8M0 byte is se + 127
and every column of that block is rounded as q = round_elem(w / 2^se) * 2^se, saturating at +-top * 2^se (mx_scale_model._qdq64)
— for E4M3 with one more rule, below.  A block whose entry maximum is NaN or infinite gets the byte 0xFF and every element of it
NaN, as fake_quant_mx does; nothing else is promised for such input.

Why the graph's own Q/DQ node leaves the result alone (fake_quant_mx(Wq) == Wq bit for bit): the finished block holds only
values c * 2^se with c an element value, so its own floor exponent se' is at most se.  A grid of the format under a lower
exponent is finer everywhere (subnormal codes included), so every c * 2^se is a point of it — as long as it lies within its RANGE,
+-top * 2^se'.  E2M1's largest value, 6 = 1.5 * 2^2, is the last point of its binade: nothing of the block can lie between
top * 2^se' and the end of the binade of the block's maximum, and the fixed point holds as it stands.  E4M3's largest value is
448 = 1.75 * 2^8, and the binade's last point, 1.875 * 2^8 = 480, is one the format does not have (its code is NaN): a block whose
compensation has shrunk it into a lower binade than it entered with, and whose largest finished value is 1.875 * 2^t there (120 =
1.875 * 2^6 under se = 0, say), would have that value saturated to 1.75 * 2^t by the graph's node.  So the largest value of a
finished E4M3 block must not have the significand 1.875, which is kept true column by column:
    the E4M3 rule: a column whose rounded magnitude is 1.875 * 2^t * 2^se AND exceeds every magnitude the block has been given so
    far takes the nearer of that value's two neighbours on the grid instead, 1.75 * 2^t * 2^se if |w| does not exceed it, 2 * 2^t *
    2^se otherwise (keep_top_closed).
The block's maximum is then only ever raised by a value with another significand; 1.875 * 2^t below the running maximum stays
allowed and is a point of the finer grid.  An all-zero block keeps its zeros with their signs.

  * `gptq_mx_block(W, U, c0, nb, elem, K)`: fp32, every operation a single IEEE fp32 operation in gptq_model.gptq_block's order
    (the rounding itself is exact arithmetic) — what the kernel (csrc/gptq_kernels.hip k_gptq_mx_block) is held to bit for bit, Err
    and the bytes included.  c0 % 32 == 0; nb % 32 == 0 unless c0 + nb == K; 1 <= nb <= 128.
  * `gptq_mx_layer32`: the blocks left to right with the fp32 GEMM between them, as gptq_layer32.
  * `gptq_mx_layer64`: the recursion column by column in fp64; only the block maximum and the rounding see fp32.
  * `objective`: gptq_model's.
"""
import numpy as np

import mx_model as M
import mx_scale_model as S
from gptq_model import factor, objective  # noqa: F401  (part of this definition)

BLOCK = M.BLOCK
MAX_CALL = 128


def block_entry(blk, elem):
    """blk: the current values of one MX block, [R, <= 32] (fp32 values) -> (se int64 [R], bad bool [R]: the maximum is NaN or
    infinite)."""
    with np.errstate(invalid="ignore"):
        a = np.max(np.abs(np.asarray(blk, np.float32)), axis=1)                   # np.max propagates a NaN
    bad = ~np.isfinite(a)
    return M.shared_exponent(np.where(bad, 0, a).astype(np.float32), elem), bad


def _abs_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def keep_top_closed(w, q, m):
    """The E4M3 rule.  w, q: one column and its rounding (fp32 [R]); m: the largest |q| among the block's columns rounded before
    (fp32 [R], 0 for none).  Where |q| is 1.875 * 2^t (significand 1.111b and nothing below: 15 u with u the value of |q|'s lowest
    set pattern bit) AND above m, q becomes the nearer of its two neighbours on the grid, 14 u if |w| <= |q| and 16 u otherwise —
    on bit patterns, where both are one u away (fp32 subnormals included: patterns are contiguous across 2^-126)."""
    yb, b, mb = _abs_bits(q), _abs_bits(w), _abs_bits(m)
    u = yb & (~yb + np.uint32(1))
    sig = np.where(yb >> np.uint32(23), (yb & np.uint32(0x7FFFFF)) | np.uint32(0x800000), yb)
    hit = (yb != 0) & (yb < np.uint32(0x7F800000)) & (sig == (u << np.uint32(4)) - u) & (yb > mb)
    out = np.where(hit, np.where(b > yb, yb + u, yb - u), yb) | (np.ascontiguousarray(q, np.float32).view(np.uint32) & np.uint32(0x80000000))
    return out.astype(np.uint32).view(np.float32)


def round_under(w, se, bad, elem, m):
    """One column w [R] (fp32 values) on elem_grid * 2^se, saturating, under the E4M3 rule given m (keep_top_closed) -> fp32; NaN
    where `bad`."""
    w = np.asarray(w, np.float32)
    q = S._qdq64(w.astype(np.float64), se, elem).astype(np.float32)
    if elem == "mxfp8":
        q = keep_top_closed(w, np.where(bad, 0, q).astype(np.float32), m)
    return np.where(bad, np.float32(np.nan), q).astype(np.float32)


def _raise_max(m, q):
    """m (fp32 [R]) with |q| taken in: the largest rounded magnitude of the block so far (a NaN leaves it: such a block is a NaN block)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(q) > m, np.abs(q), m).astype(np.float32)


def gptq_mx_block(W, U, c0, nb, elem, K):
    """In place on W (fp32 [R, ldw]) -> (Err fp32 [R, nb], bytes uint8 [R, ceil(nb / 32)]).  U: fp32, indexed by absolute column."""
    assert W.dtype == np.float32 and U.dtype == np.float32
    assert c0 % BLOCK == 0 and 1 <= nb <= MAX_CALL and c0 + nb <= K <= W.shape[1] and (nb % BLOCK == 0 or c0 + nb == K)
    R = W.shape[0]
    err = np.zeros((R, nb), np.float32)
    scales = np.zeros((R, -(-nb // BLOCK)), np.uint8)
    se = bad = m = None
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(nb):
            c = c0 + j
            if c % BLOCK == 0:
                se, bad = block_entry(W[:, c:min(c + BLOCK, K)], elem)
                scales[:, j // BLOCK] = np.where(bad, 0xFF, se + 127)
                m = np.zeros(R, np.float32)
            w = W[:, c].copy()
            q = round_under(w, se, bad, elem, m)
            m = _raise_max(m, q)
            e = ((w - q).astype(np.float32) / U[c, c]).astype(np.float32)
            W[:, c] = q
            err[:, j] = e
            for k in range(j + 1, nb):
                W[:, c0 + k] = (W[:, c0 + k] - (e * U[c, c0 + k]).astype(np.float32)).astype(np.float32)
    return err, scales


def gptq_mx_layer32(W, U, elem, block=MAX_CALL):
    """-> (Wq fp32 [R, K], Err fp32 [R, K], the entry bytes uint8 [R, ceil(K / 32)])"""
    assert block % BLOCK == 0 and BLOCK <= block <= MAX_CALL
    W = np.array(W, np.float32)
    U = np.asarray(U, np.float32)
    K = W.shape[1]
    err = np.zeros_like(W)
    scales = np.zeros((W.shape[0], -(-K // BLOCK)), np.uint8)
    for c0 in range(0, K, block):
        nb = min(block, K - c0)
        err[:, c0:c0 + nb], scales[:, c0 // BLOCK:c0 // BLOCK + -(-nb // BLOCK)] = gptq_mx_block(W, U, c0, nb, elem, K)
        if c0 + nb < K:
            W[:, c0 + nb:] -= (err[:, c0:c0 + nb] @ U[c0:c0 + nb, c0 + nb:]).astype(np.float32)
    return W, err, scales


def gptq_mx_layer64(W, U, elem):
    W = np.array(W, np.float64)
    U = np.asarray(U, np.float64)
    K = W.shape[1]
    se = bad = m = None
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(K):
            if c % BLOCK == 0:
                se, bad = block_entry(W[:, c:min(c + BLOCK, K)].astype(np.float32), elem)
                m = np.zeros(W.shape[0], np.float32)
            w = W[:, c].copy()
            q32 = round_under(w.astype(np.float32), se, bad, elem, m)
            m = _raise_max(m, q32)
            q = q32.astype(np.float64)
            e = (w - q) / U[c, c]
            W[:, c] = q
            W[:, c + 1:] -= np.outer(e, U[c, c + 1:])
    return W.astype(np.float32)
