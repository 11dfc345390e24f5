"""The definition of `--mx_pack`: an MX tensor as packed element codes and E8M0 scale bytes, as a numpy model on top of
tests/mx_model.py (which defines the values; this file defines the bytes).

Scale byte   the E8M0 code of the block, se + 127; 0xFF for a block that holds a NaN or an infinity — mx_model's own.
E4M3 element the OCP FP8 E4M3FN byte S.EEEE.MMM (bias 7) of y / 2^se, y = mx_model.fake_quant_mx(x): the sign bit of a zero is kept;
             in a 0xFF block every element that exists is 0x7F.  The 127 finite magnitudes ascend with the byte 0x00 .. 0x7E.
E2M1 element 4 bits S.EE.M (bias 1): the magnitude is the index into 0, 0.5, 1, 1.5, 2, 3, 4, 6.  Two to a byte, the element at
             the even index along K in the low nibble (ONNX FLOAT4E2M1).  In a 0xFF block the elements are 0.
Layout       x is [outer, K, inner] around the block axis.  Codes and scales are K-INNERMOST — the order a block-scaled GEMM reads
             both operands in: with Kp = 32 * ceil(K / 32), codes is uint8 [outer, inner, Kp] (E4M3) or [outer, inner, Kp / 2]
             (E2M1) and scales uint8 [outer, inner, Kp / 32].  The elements past K of a short last block have code 0.  For
             inner > 1 this transposes the element order, and the scales are NOT in fake_quant_mx's [outer, nblk, inner] order.
Decode       is defined on every (code, scale) pair: scale 0xFF -> NaN (0x7FC00000) for the whole block; E4M3 codes 0x7F and 0xFF
             -> NaN; otherwise +-value * 2^se exactly — the smallest product, 2^-9 * 2^-127 = 2^-136, is an fp32 subnormal, and a
             product above fp32's range (which encode never emits: se <= 127 - emax) is +-inf.

decode(encode(x)) == mx_model.fake_quant_mx(x) bit for bit (NaN in the same places): every value mx_model produces, scaled back
by its block's 2^se, is exactly one value of the element format.
"""
import numpy as np

import mx_model as M

BLOCK = M.BLOCK
QNAN = np.uint32(0x7FC00000)


def _split(shape, axis):
    axis = axis % len(shape)
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    return axis, outer, int(shape[axis]), inner


def packed_shapes(shape, axis, elem):
    """(codes shape, scales shape) of a tensor of `shape` blocked along `axis`: [*outer dims, *inner dims, Kp or Kp / 2 | Kp / 32]."""
    axis, _, K, _ = _split(shape, axis)
    kp = BLOCK * -(-K // BLOCK)
    lead = tuple(shape[:axis]) + tuple(shape[axis + 1:])
    return lead + (kp // 2 if elem == "mxfp4" else kp,), lead + (kp // BLOCK,)


def element_codes(x, axis, elem):
    """-> (one code per element, uint8 [outer, inner, Kp], pad = 0; scales uint8 [outer, inner, Kp / 32]) — before nibbles pair up."""
    x = np.asarray(x, np.float32)
    axis, outer, K, inner = _split(x.shape, axis)
    nblk = -(-K // BLOCK)
    y, s = M.fake_quant_mx(x, axis, elem, return_scales=True)                  # s [outer, nblk, inner]
    y3 = y.reshape(outer, K, inner)
    se = np.repeat(s.astype(np.int64) - 127, BLOCK, axis=1)[:, :K, :]
    bad = np.repeat(s == 0xFF, BLOCK, axis=1)[:, :K, :]
    w = np.ldexp(np.where(bad, 0, y3).astype(np.float64), -np.where(bad, 0, se))   # y / 2^se: exact
    c = M.codes(elem).astype(np.float64)
    idx = np.minimum(np.searchsorted(c, np.abs(w)), c.size - 1)
    assert np.array_equal(c[idx], np.abs(w)), "a value of fake_quant_mx that is no value of the element format"
    sign = np.signbit(y3) & ~bad
    if elem == "mxfp4":
        code = np.where(bad, 0, idx | (sign << 3))
    else:
        code = np.where(bad, 0x7F, idx | (sign << 7))
    out = np.zeros((outer, inner, nblk * BLOCK), np.uint8)
    out[:, :, :K] = code.astype(np.uint8).transpose(0, 2, 1)
    return out, np.ascontiguousarray(s.transpose(0, 2, 1))


def pack_nibbles(c):
    """[..., Kp] 4-bit codes -> [..., Kp / 2] bytes, the even index in the low nibble."""
    return (c[..., 0::2] | (c[..., 1::2] << 4)).astype(np.uint8)


def unpack_nibbles(b):
    out = np.empty(b.shape[:-1] + (2 * b.shape[-1],), np.uint8)
    out[..., 0::2], out[..., 1::2] = b & 0xF, b >> 4
    return out


def encode(x, axis, elem):
    """-> (codes, scales) in packed_shapes(x.shape, axis, elem)."""
    x = np.asarray(x, np.float32)
    c, s = element_codes(x, axis, elem)
    if elem == "mxfp4":
        c = pack_nibbles(c)
    cs, ss = packed_shapes(x.shape, axis, elem)
    return c.reshape(cs), s.reshape(ss)


def decode_elements(code, scale, elem):
    """One fp32 per (element code, scale byte) pair, broadcast against each other: the definition of decode on every pair."""
    code, scale = np.broadcast_arrays(np.asarray(code, np.uint8), np.asarray(scale, np.uint8))
    c = M.codes(elem).astype(np.float64)
    if elem == "mxfp4":
        mag, neg, nan = c[code & 7], (code >> 3) & 1, np.zeros(code.shape, bool)
    else:
        nan = (code & 0x7F) == 0x7F
        mag, neg = c[np.minimum(code & 0x7F, 0x7E)], code >> 7
    with np.errstate(over="ignore"):
        v = np.ldexp(np.where(neg == 1, -mag, mag), np.minimum(scale.astype(np.int64), 254) - 127).astype(np.float32)   # overflow -> +-inf
    bits = v.view(np.uint32).copy()
    bits[nan | (scale == 0xFF)] = QNAN
    return bits.view(np.float32)


def decode(codes, scales, elem, shape, axis):
    """codes / scales as encode writes them (any bytes) -> fp32 of `shape`."""
    axis, outer, K, inner = _split(tuple(shape), axis)
    nblk = -(-K // BLOCK)
    c = np.asarray(codes, np.uint8).reshape(outer, inner, -1)
    if elem == "mxfp4":
        c = unpack_nibbles(c)
    assert c.shape[2] == nblk * BLOCK
    s = np.repeat(np.asarray(scales, np.uint8).reshape(outer, inner, nblk), BLOCK, axis=2)
    y = decode_elements(c, s, elem)[:, :, :K]
    return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(shape)


def all_pairs(elem):
    """Every (element code, scale byte) pair, as blocks of a [blocks, 32] tensor along axis 1 -> (codes, scales [blocks, 1]):
    256 x 256 pairs in 2048 blocks for E4M3, 16 x 256 in 256 blocks (each code twice) for E2M1."""
    if elem == "mxfp4":
        c = pack_nibbles(np.tile(np.arange(16, dtype=np.uint8), (256, 2)))
        return c, np.arange(256, dtype=np.uint8).reshape(256, 1)
    c = np.tile(np.arange(256, dtype=np.uint8).reshape(8, 32), (256, 1))
    return c, np.repeat(np.arange(256, dtype=np.uint8), 8).reshape(2048, 1)
