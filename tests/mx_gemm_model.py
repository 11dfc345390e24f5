"""The definition of dpl_mx_gemm / ops.mx_gemm (`--mx_verify`): the product of two packed MX operands, as a numpy model on top of
tests/mx_pack_model.py (which stays the definition of the bytes).

Operands     both K-INNERMOST, as mx_pack_model.encode writes them: a_codes uint8 [*batch, m, Kp] (mxfp8) or [*batch, m, Kp / 2]
             (mxfp4), a_scales uint8 [*batch, m, Kp / 32]; b_codes / b_scales the same with n rows, under A's leading dimensions
             or none (then every batch shares B).
Product      C[.., i, j] = sum over kk < Kp of a[.., i, kk] * b[.., j, kk], a and b = mx_pack_model.decode_elements of every
             (code, scale) pair — the pad codes of a short last block included —, summed in fp64.
NaN rule     C[.., i, j] is NaN if row i of A or row j of B holds a 0xFF scale byte or an E4M3 NaN code (0x7F, 0xFF) anywhere in
             its Kp codes (whatever the other operand holds there, a zero too).
S            sum |a| * |b| per output over the finite pairs (the rows a NaN touches: NaN), the scale of the error bound
             |got - C| <= factor * Kp * 2^-23 * S + 2^-149.  factor = 1 is what fp32 additions in any order over exact products
             keep, and what MXFP4 operands keep on the MI355X (measured: no error at all).  With E4M3 operands the instruction
             does NOT add exact products: inside every run of 8 consecutive k it aligns the eight products to the largest one and
             truncates each to a multiple of 2^-14 of that one's leading power of two (448 * 448 + 1.125 * 1.125 in one run gives
             200704; in different runs 200705.265625), so up to 7 * 2^-14 * S can be lost whatever Kp is.
             HW_FACTOR is that finding in the form the bound has: twice the worst measured ratio.
"""
import numpy as np

import mx_model as M
import mx_pack_model as P

BLOCK = P.BLOCK


def decode_operand(codes, scales, elem):
    """codes / scales [..., rows, Kp (/ 2)] / [..., rows, Kp / 32] -> fp64 [..., rows, Kp] (NaN where decode says so)."""
    c = np.asarray(codes, np.uint8)
    s = np.asarray(scales, np.uint8)
    if elem == "mxfp4":
        c = P.unpack_nibbles(c)
    assert c.shape[:-1] == s.shape[:-1] and c.shape[-1] == BLOCK * s.shape[-1], (c.shape, s.shape)
    return P.decode_elements(c, np.repeat(s, BLOCK, axis=-1), elem).astype(np.float64)


def mx_gemm(a_codes, a_scales, b_codes, b_scales, elem_a, elem_b=None):
    """-> (C fp32 [*batch, m, n], S fp64 [*batch, m, n])."""
    elem_b = elem_a if elem_b is None else elem_b
    a, b = decode_operand(a_codes, a_scales, elem_a), decode_operand(b_codes, b_scales, elem_b)
    assert a.shape[-1] == b.shape[-1] and (b.ndim == 2 or b.shape[:-2] == a.shape[:-2])
    bad_a, bad_b = np.isnan(a).any(-1), np.isnan(b).any(-1)                  # [..., m], [..., n]
    a0, b0 = np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b)
    bt = np.swapaxes(b0, -1, -2)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.matmul(a0, bt)
        s = np.matmul(np.abs(a0), np.abs(bt))
        bad = bad_a[..., :, None] | bad_b[..., None, :]
        c = np.where(bad, np.nan, c).astype(np.float32)
    return c, np.where(bad, np.nan, s)


def codes_from_values(v, elem):
    """[..., Kp] numbers that are values of the element format (before the block scale) -> the packed codes of those elements."""
    v = np.asarray(v, np.float64)
    c = M.codes(elem).astype(np.float64)
    idx = np.minimum(np.searchsorted(c, np.abs(v)), c.size - 1)
    assert np.array_equal(c[idx], np.abs(v)), "not a value of the element format"
    code = (idx | (np.signbit(v).astype(np.int64) << (3 if elem == "mxfp4" else 7))).astype(np.uint8)
    return P.pack_nibbles(code) if elem == "mxfp4" else code


# max |got - C| / (Kp 2^-23 S) measured on the MI355X, random data with a few large channels through the encoder
# (tests/test_mx_gemm_gpu.py test 4): mxfp8 [34, 96] x [96, 24] 11.12, [2, 17, 64] x [64, 48] 19.51; mxfp4 0 and 0.
HW_WORST_RATIO = 19.51
HW_FACTOR = 2 * HW_WORST_RATIO


def bound(s, kp, factor=1.0):
    """|got - C| allowed: factor 1 for fp32 additions in any order, each rounded or truncated, over exact products."""
    return factor * kp * 2.0 ** -23 * s + 2.0 ** -149
