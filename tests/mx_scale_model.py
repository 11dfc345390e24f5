"""The definition of `--mx_scale_search`, as a numpy model on top of tests/mx_model.py (the values) and tests/mx_pack_model.py (the
bytes): per block of a constant MX operand, whichever of the floor-rule shared exponent se0 and se0 + 1 gives the smaller squared
Q/DQ error, and the Q/DQ and the packed bytes under GIVEN scale bytes.  Nothing here is held to a tolerance.

`scale_search(x, axis, elem)`: x viewed as [outer, K, inner], blocks of 32 along K as in mx_model.fake_quant_mx.  Per block, with
a = max |v| over the elements that exist:
    a NaN or +-inf   the byte is 0xFF, both errors are +inf
    a == 0           the byte is 0 (se = -127), both errors are 0
    otherwise        the candidates are se0 = mx_model.shared_exponent(a) and se0 + 1; se0 + 1 is dropped when it exceeds
                     127 - emax (the largest element times the scale must be an fp32 value).  Under candidate se:
                       y[k]   = round_elem(v[k] / 2^se) * 2^se, saturating, mx_model's rounding
                       e[k]   = (v[k] - y[k])^2 in fp64: the difference is exact in fp32 and its square in fp64; the elements past
                                K of a short last block are +0.0 and add 0
                       err    = the fp64 sum of the 32 terms as a balanced tree in index order, e = e[0::2] + e[1::2] five times
                     se0 + 1 is chosen iff err_1 < err_0: ties and NaN comparisons keep the floor.
The tree is part of the definition: it is what eight lanes of four, 32 lanes of one and one lane of 32 compute alike, with
xor-shuffle steps 1, 2, 4, ... across lanes.
-> (bytes uint8 [outer, nblk, inner], the order of fake_quant_mx's scales; err fp64 [outer, nblk, inner, 2]: the error at the floor
and the error at the chosen byte).

`fake_quant_mx_scaled(x, axis, elem, scales)` / `encode_scaled(x, axis, elem, scales)`: Q/DQ and packed bytes under given bytes
([outer, nblk, inner] order).  A block that holds a NaN or an infinity is a 0xFF block whatever byte was given; a given byte of 0xFF,
or one above 254 - emax, makes the block a 0xFF block too; every other block gets se = byte - 127 and mx_model's rounding under
it.  A 0xFF block has every element NaN and the packed scale byte 0xFF, its element codes 0x7F (E4M3) or 0 (E2M1) as
mx_pack_model has them.  mx_pack_model.decode(encode_scaled(x, s)) == fake_quant_mx_scaled(x, s) bit for bit, and
fake_quant_mx_scaled(x, floor bytes) == mx_model.fake_quant_mx(x) bit for bit.
"""
import numpy as np

import mx_model as M
import mx_pack_model as P

BLOCK = M.BLOCK


def _rnd(elem):
    return M.e2m1_round if elem == "mxfp4" else M._e4m3_round64


def _qdq64(v, se, elem):
    """v fp64 (fp32 values), se int64 broadcastable -> round_elem(v / 2^se) * 2^se as fp64 (an fp32 value)."""
    X = np.ldexp(1.0, se)
    with np.errstate(all="ignore"):
        return _rnd(elem)(v / X) * X


def tree_sum(e, axis):
    """The balanced tree over 32 terms along `axis`, in index order."""
    e = np.moveaxis(e, axis, -1)
    assert e.shape[-1] == BLOCK
    for _ in range(5):
        e = e[..., 0::2] + e[..., 1::2]
    return e[..., 0]


def scale_search(x, axis, elem):
    x = np.asarray(x, np.float32)
    axis, outer, K, inner = P._split(x.shape, axis)
    nblk = -(-K // BLOCK)
    x3 = x.reshape(outer, K, inner)
    scales = np.empty((outer, nblk, inner), np.uint8)
    err = np.empty((outer, nblk, inner, 2), np.float64)
    top = 127 - M.EMAX[elem]
    for b in range(nblk):
        v = np.zeros((outer, BLOCK, inner), np.float64)                       # +0.0 past K
        with np.errstate(invalid="ignore"):
            blk = x3[:, b * BLOCK:(b + 1) * BLOCK, :].astype(np.float64)
            v[:, :blk.shape[1], :] = blk
            a = np.max(np.abs(v), axis=1, keepdims=True)
        bad = ~np.isfinite(a)
        v = np.where(bad, 0.0, v)
        se0 = M.shared_exponent(np.where(bad, 0, a).astype(np.float32), elem)
        e = []
        for se in (se0, np.minimum(se0 + 1, top)):
            d = v - _qdq64(v, se, elem)
            e.append(tree_sum(d * d, 1))                                      # [outer, inner]
        up = (se0[:, 0, :] + 1 <= top) & (e[1] < e[0]) & ~bad[:, 0, :]
        scales[:, b, :] = np.where(bad[:, 0, :], 0xFF, se0[:, 0, :] + 127 + up)
        err[:, b, :, 0] = np.where(bad[:, 0, :], np.inf, e[0])
        err[:, b, :, 1] = np.where(bad[:, 0, :], np.inf, np.where(up, e[1], e[0]))
    return scales, err


def floor_scales(x, axis, elem):
    """The bytes of the floor rule, [outer, nblk, inner]."""
    return M.fake_quant_mx(x, axis, elem, return_scales=True)[1]


def fake_quant_mx_scaled(x, axis, elem, scales, return_scales=False):
    """-> y (and the bytes in effect, [outer, nblk, inner]: 0xFF wherever the block is a 0xFF block)."""
    x = np.asarray(x, np.float32)
    axis, outer, K, inner = P._split(x.shape, axis)
    nblk = -(-K // BLOCK)
    x3 = x.reshape(outer, K, inner)
    s = np.asarray(scales, np.uint8).reshape(outer, nblk, inner)
    y = np.empty_like(x3)
    eff = np.empty_like(s)
    for b in range(nblk):
        with np.errstate(invalid="ignore"):
            v = x3[:, b * BLOCK:(b + 1) * BLOCK, :].astype(np.float64)
            a = np.max(np.abs(v), axis=1, keepdims=True)
        byte = s[:, b:b + 1, :].astype(np.int64)
        bad = ~np.isfinite(a) | (byte > 254 - M.EMAX[elem])
        q = _qdq64(np.where(bad, 0.0, v), np.where(bad, 0, byte - 127), elem)
        y[:, b * BLOCK:(b + 1) * BLOCK, :] = np.where(bad, np.nan, q).astype(np.float32)
        eff[:, b, :] = np.where(bad, 0xFF, byte)[:, 0, :]
    y = y.reshape(x.shape)
    return (y, eff) if return_scales else y


def encode_scaled(x, axis, elem, scales):
    """-> (codes, scales) in mx_pack_model.packed_shapes(x.shape, axis, elem): mx_pack_model.element_codes' bytes of
    fake_quant_mx_scaled's values under the bytes in effect."""
    x = np.asarray(x, np.float32)
    axis, outer, K, inner = P._split(x.shape, axis)
    nblk = -(-K // BLOCK)
    y, s = fake_quant_mx_scaled(x, axis, elem, scales, return_scales=True)
    y3 = y.reshape(outer, K, inner)
    se = np.repeat(s.astype(np.int64) - 127, BLOCK, axis=1)[:, :K, :]
    bad = np.repeat(s == 0xFF, BLOCK, axis=1)[:, :K, :]
    w = np.ldexp(np.where(bad, 0, y3).astype(np.float64), -np.where(bad, 0, se))
    c = M.codes(elem).astype(np.float64)
    idx = np.minimum(np.searchsorted(c, np.abs(w)), c.size - 1)
    assert np.array_equal(c[idx], np.abs(w)), "a value of fake_quant_mx_scaled that is no value of the element format"
    sign = np.signbit(y3) & ~bad
    code = np.where(bad, 0, idx | (sign << 3)) if elem == "mxfp4" else np.where(bad, 0x7F, idx | (sign << 7))
    out = np.zeros((outer, inner, nblk * BLOCK), np.uint8)
    out[:, :, :K] = code.astype(np.uint8).transpose(0, 2, 1)
    if elem == "mxfp4":
        out = P.pack_nibbles(out)
    cs, ss = P.packed_shapes(x.shape, axis, elem)
    return out.reshape(cs), np.ascontiguousarray(s.transpose(0, 2, 1)).reshape(ss)
