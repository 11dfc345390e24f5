"""The definition of the two OCP Microscaling v1.0 FP6 formats, `--mx mxfp6_e2m3` / `--mx mxfp6_e3m2`, as a numpy model beside
tests/mx_model.py (mxfp8 / mxfp4), tests/mx_pack_model.py (their bytes) and tests/mx_scale_model.py (`--mx_scale_search`).

Elements     6 bits, no NaN and no inf codes; 32 magnitudes each, ascending with the low five bits of the code.
  mxfp6_e2m3   S.EE.MMM, bias 1: m * 2^-3 under the exponent field 0, else (1 + m / 8) * 2^(field - 1).  Largest value 7.5 (emax 2),
               subnormal step 0.125.
  mxfp6_e3m2   S.EEE.MM, bias 3: m * 2^-4 under the field 0, else (1 + m / 4) * 2^(field - 3).  Largest value 28 (emax 4), smallest
               value 0.0625.
Block rule   mx_model.fake_quant_mx's: blocks of 32 along the axis, a short last block allowed; a = max |v|; a NaN or inf -> a 0xFF
             block whose elements are all NaN; a == 0 -> se = -127 and the zeros with their signs; otherwise se = clamp(floor(log2
             a) - emax, -127, 127) and y = round_elem(v / 2^se) * 2^se — nearest, ties to the even mantissa, saturating to +-7.5
             resp. +-28.  Exact arithmetic: no tolerance anywhere.
Packed form  a block's 32 codes are ONE little-endian string of 192 bits: code i occupies bits [6 i, 6 i + 6) of the block's 24
             bytes — byte (6 i) // 8 from bit (6 i) % 8 upward, carrying into the next byte; the index along K ascends with the bit
             position.  codes uint8 [outer, inner, nblk * 24], scales uint8 [outer, inner, nblk] (K-innermost, as mx_pack_model).
             The codes past K of a short last block are 0, and so is every code of a 0xFF block.
Decode       is defined on every (code, scale byte) pair: 0xFF -> NaN (0x7FC00000), otherwise +-value * 2^(byte - 127) exactly (the
             smallest product, 2^-4 * 2^-127, is an fp32 subnormal); above fp32's range +-inf.
Scale search mx_scale_model's rule with this file's rounding: se0 + 1 where that is at most 127 - emax and its tree-summed squared
             error is smaller.  Given bytes: 0xFF, a byte above 254 - emax, or a NaN / inf in the block make a 0xFF block.
"""
import numpy as np

import mx_model as M
import mx_pack_model as P
import mx_scale_model as S

BLOCK = M.BLOCK
ELEMS = ("mxfp6_e2m3", "mxfp6_e3m2")
EMAX = {"mxfp6_e2m3": 2, "mxfp6_e3m2": 4}
EMIN = {"mxfp6_e2m3": 0, "mxfp6_e3m2": -2}              # the exponent of the smallest normal value (field 1)
MBITS = {"mxfp6_e2m3": 3, "mxfp6_e3m2": 2}
ELEM_MAX = {"mxfp6_e2m3": 7.5, "mxfp6_e3m2": 28.0}
OVER = {"mxfp6_e2m3": 7.75, "mxfp6_e3m2": 30.0}         # the tie between the largest value and the next one the format does not have
BLOCK_BYTES = 24
QNAN = P.QNAN


def codes(elem):
    """The 32 non-negative values of the format, ascending: index = the code's low five bits."""
    mb, emin = MBITS[elem], EMIN[elem]
    c = np.arange(32)
    field, m = c >> mb, c & ((1 << mb) - 1)
    return np.where(field == 0, m * 2.0 ** (emin - mb), (1 + m / 2.0 ** mb) * 2.0 ** (field - 1 + emin)).astype(np.float32)


def round_elem(v, elem):
    """fp64 in (exact for every fp32 and every fp32 / 2^se), the nearest value of the format out, as fp64: ties to the even
    mantissa, saturating, the sign of zero kept, NaN stays NaN."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        a = np.minimum(np.abs(v), ELEM_MAX[elem])
        _, ex = np.frexp(a)                                              # a = m * 2^ex, m in [0.5, 1): binade ex - 1
        step = np.ldexp(1.0, np.maximum(ex - 1, EMIN[elem]) - MBITS[elem])
        return np.copysign(np.rint(a / step) * step, v)                  # np.rint: half to even = the even mantissa


def shared_exponent(a, elem):
    a = np.asarray(a, np.float32)
    return np.where(a == 0, -127, np.clip(M.floor_log2(np.where(a == 0, 1, a)) - EMAX[elem], -127, 127)).astype(np.int64)


def _qdq64(v, se, elem):
    X = np.ldexp(1.0, se)
    with np.errstate(all="ignore"):
        return round_elem(v / X, elem) * X


def fake_quant_mx(x, axis, elem, return_scales=False, scales=None):
    """The Q/DQ; scales: None (the floor rule) or given bytes [outer, nblk, inner] (fake_quant_mx_scaled).  -> y (and the bytes in
    effect, [outer, nblk, inner])."""
    x = np.asarray(x, np.float32)
    axis, outer, K, inner = P._split(x.shape, axis)
    nblk = -(-K // BLOCK)
    x3 = x.reshape(outer, K, inner)
    y = np.empty_like(x3)
    eff = np.empty((outer, nblk, inner), np.uint8)
    given = None if scales is None else np.asarray(scales, np.uint8).reshape(outer, nblk, inner)
    for b in range(nblk):
        with np.errstate(invalid="ignore"):
            v = x3[:, b * BLOCK:(b + 1) * BLOCK, :].astype(np.float64)
            a = np.max(np.abs(v), axis=1, keepdims=True)
        bad = ~np.isfinite(a)
        if given is None:
            se = shared_exponent(np.where(bad, 0, a).astype(np.float32), elem)
        else:
            byte = given[:, b:b + 1, :].astype(np.int64)
            bad = bad | (byte > 254 - EMAX[elem])
            se = np.where(bad, 0, byte - 127)
        q = _qdq64(np.where(bad, 0.0, v), se, elem)
        y[:, b * BLOCK:(b + 1) * BLOCK, :] = np.where(bad, np.nan, q).astype(np.float32)
        eff[:, b, :] = np.where(bad, 0xFF, se + 127)[:, 0, :]
    y = y.reshape(x.shape)
    return (y, eff) if return_scales else y


def fake_quant_mx_scaled(x, axis, elem, scales, return_scales=False):
    return fake_quant_mx(x, axis, elem, return_scales, scales=scales)


def scale_search(x, axis, elem):
    """mx_scale_model.scale_search with this file's rounding -> (bytes [outer, nblk, inner], err fp64 [outer, nblk, inner, 2])."""
    x = np.asarray(x, np.float32)
    axis, outer, K, inner = P._split(x.shape, axis)
    nblk = -(-K // BLOCK)
    x3 = x.reshape(outer, K, inner)
    scales = np.empty((outer, nblk, inner), np.uint8)
    err = np.empty((outer, nblk, inner, 2), np.float64)
    top = 127 - EMAX[elem]
    for b in range(nblk):
        v = np.zeros((outer, BLOCK, inner), np.float64)
        with np.errstate(invalid="ignore"):
            blk = x3[:, b * BLOCK:(b + 1) * BLOCK, :].astype(np.float64)
            v[:, :blk.shape[1], :] = blk
            a = np.max(np.abs(v), axis=1, keepdims=True)
        bad = ~np.isfinite(a)
        v = np.where(bad, 0.0, v)
        se0 = shared_exponent(np.where(bad, 0, a).astype(np.float32), elem)
        e = []
        for se in (se0, np.minimum(se0 + 1, top)):
            d = v - _qdq64(v, se, elem)
            e.append(S.tree_sum(d * d, 1))
        up = (se0[:, 0, :] + 1 <= top) & (e[1] < e[0]) & ~bad[:, 0, :]
        scales[:, b, :] = np.where(bad[:, 0, :], 0xFF, se0[:, 0, :] + 127 + up)
        err[:, b, :, 0] = np.where(bad[:, 0, :], np.inf, e[0])
        err[:, b, :, 1] = np.where(bad[:, 0, :], np.inf, np.where(up, e[1], e[0]))
    return scales, err


def boundary_points(elem):
    """mx_model.boundary_points for these formats: every code, every tie, their fp32 neighbours, the tie above the top value."""
    c = codes(elem)
    mids = ((c[:-1].astype(np.float64) + c[1:]) / 2).astype(np.float32)
    over = np.float32(OVER[elem])
    base = np.concatenate([c, mids])
    inf = np.float32(np.inf)
    pts = np.concatenate([base, np.nextafter(base, inf), np.nextafter(base, -inf), np.array([over, np.nextafter(over, np.float32(0))], np.float32)])
    pts = pts[pts >= 0]
    return np.concatenate([pts, -pts]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the bytes
def packed_shapes(shape, axis, elem):
    axis, _, K, _ = P._split(tuple(shape), axis)
    nblk = -(-K // BLOCK)
    lead = tuple(shape[:axis]) + tuple(shape[axis + 1:])
    return lead + (nblk * BLOCK_BYTES,), lead + (nblk,)


def pack6(c):
    """[..., Kp] 6-bit codes -> [..., Kp * 3 / 4] bytes: each block of 32 one little-endian string of 192 bits."""
    c = np.asarray(c, np.uint8)
    bits = (c[..., None] >> np.arange(6, dtype=np.uint8)) & 1                  # [..., Kp, 6], the low bit first
    return np.packbits(bits.reshape(c.shape[:-1] + (-1,)), axis=-1, bitorder="little")


def unpack6(b):
    b = np.asarray(b, np.uint8)
    bits = np.unpackbits(b, axis=-1, bitorder="little").reshape(b.shape[:-1] + (-1, 6))
    return (bits << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)


def element_codes(x, axis, elem, scales=None):
    """-> (one code per element, uint8 [outer, inner, Kp], pad = 0; scales uint8 [outer, inner, nblk]) — before the codes are packed."""
    x = np.asarray(x, np.float32)
    axis, outer, K, inner = P._split(x.shape, axis)
    nblk = -(-K // BLOCK)
    y, s = fake_quant_mx(x, axis, elem, return_scales=True, scales=scales)
    y3 = y.reshape(outer, K, inner)
    se = np.repeat(s.astype(np.int64) - 127, BLOCK, axis=1)[:, :K, :]
    bad = np.repeat(s == 0xFF, BLOCK, axis=1)[:, :K, :]
    w = np.ldexp(np.where(bad, 0, y3).astype(np.float64), -np.where(bad, 0, se))
    c = codes(elem).astype(np.float64)
    idx = np.minimum(np.searchsorted(c, np.abs(w)), c.size - 1)
    assert np.array_equal(c[idx], np.abs(w)), "a value of fake_quant_mx that is no value of the element format"
    sign = np.signbit(y3) & ~bad
    code = np.where(bad, 0, idx | (sign << 5))
    out = np.zeros((outer, inner, nblk * BLOCK), np.uint8)
    out[:, :, :K] = code.astype(np.uint8).transpose(0, 2, 1)
    return out, np.ascontiguousarray(s.transpose(0, 2, 1))


def encode(x, axis, elem, scales=None):
    """-> (codes, scales) in packed_shapes(x.shape, axis, elem); scales: given bytes in x's own order (encode_scaled) or None."""
    x = np.asarray(x, np.float32)
    c, s = element_codes(x, axis, elem, scales)
    cs, ss = packed_shapes(x.shape, axis, elem)
    return pack6(c).reshape(cs), s.reshape(ss)


def encode_scaled(x, axis, elem, scales):
    return encode(x, axis, elem, scales)


def decode_elements(code, scale, elem):
    """One fp32 per (6-bit element code, scale byte) pair, broadcast against each other."""
    code, scale = np.broadcast_arrays(np.asarray(code, np.uint8), np.asarray(scale, np.uint8))
    mag, neg = codes(elem).astype(np.float64)[code & 31], (code >> 5) & 1
    with np.errstate(over="ignore"):
        v = np.ldexp(np.where(neg == 1, -mag, mag), np.minimum(scale.astype(np.int64), 254) - 127).astype(np.float32)
    bits = v.view(np.uint32).copy()
    bits[scale == 0xFF] = QNAN
    return bits.view(np.float32)


def decode(packed, scales, elem, shape, axis):
    axis, outer, K, inner = P._split(tuple(shape), axis)
    nblk = -(-K // BLOCK)
    c = unpack6(np.asarray(packed, np.uint8).reshape(outer, inner, -1))
    assert c.shape[2] == nblk * BLOCK
    s = np.repeat(np.asarray(scales, np.uint8).reshape(outer, inner, nblk), BLOCK, axis=2)
    y = decode_elements(c, s, elem)[:, :, :K]
    return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(shape)


# ---------------------------------------------------------------------------------------------- all four formats, for the MFMA tests
ALL_ELEMS = ("mxfp8", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp4")
BYTES_PER_BLOCK = {"mxfp8": 32, "mxfp6_e2m3": 24, "mxfp6_e3m2": 24, "mxfp4": 16}


def values_of(elem):
    """The non-negative finite values of any of the four element formats, ascending."""
    return codes(elem) if elem in ELEMS else M.codes(elem)


def encode_any(x, axis, elem):
    return encode(x, axis, elem) if elem in ELEMS else P.encode(x, axis, elem)


def decoded64(packed, scales, elem):
    """K-innermost packed operand [..., rows, nblk * bytes] / [..., rows, nblk] -> its values as fp64 [..., rows, Kp] (NaN for a
    0xFF block or an E4M3 NaN code)."""
    packed, scales = np.asarray(packed, np.uint8), np.asarray(scales, np.uint8)
    if elem in ELEMS:
        c = unpack6(packed)
    else:
        c = P.unpack_nibbles(packed) if elem == "mxfp4" else packed
    s = np.repeat(scales, BLOCK, axis=-1)
    fn = decode_elements if elem in ELEMS else P.decode_elements
    return fn(c, s, elem).astype(np.float64)


def gemm_ref(a, sa, b, sb, elem_a, elem_b):
    """The fp64 product of the decoded bytes: A [*batch, m, .] x B [*batch or none, n, .] -> [*batch, m, n].  A row (column) that
    holds a NaN is NaN throughout (the kernel's rule)."""
    da, db = decoded64(a, sa, elem_a), decoded64(b, sb, elem_b)
    bad_a, bad_b = np.isnan(da).any(-1), np.isnan(db).any(-1)
    c = np.matmul(np.nan_to_num(da), np.swapaxes(np.nan_to_num(db), -1, -2))
    bad = bad_a[..., :, None] | bad_b[..., None, :]
    return np.where(bad, np.nan, c)
