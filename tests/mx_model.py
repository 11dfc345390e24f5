"""The definition of the OCP Microscaling (MX) v1.0 Q/DQ of `--mx mxfp8` / `--mx mxfp4`, as a numpy model.

A block is 32 consecutive elements along one axis and shares one scale X = 2^se, an E8M0 code (se + 127; 0xFF is NaN); the
elements are OCP FP8 E4M3 (`mxfp8`: emax = 8, largest value 448, fp8_model.e4m3_round) or FP4 E2M1 (`mxfp4`: 1 sign bit, 2
exponent bits with bias 1, 1 mantissa bit — the non-negative values 0, 0.5, 1, 1.5, 2, 3, 4, 6; emax = 2).

  * `e2m1_round(v)`: fp32 -> the nearest E2M1 value as fp32, ties to the even mantissa (0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
    1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), saturating to +-6, the sign of zero kept, NaN stays NaN.
  * `fake_quant_mx(x, axis, elem)`: x viewed as [outer, K, inner] around `axis`; blocks of 32 indices along K from 0, the last
    one holding the K % 32 elements that exist (nothing is padded in).  Per block, a = max |v|:
        a NaN or +inf      every element of the block is NaN (scale code 0xFF)
        a == 0             se = -127; the outputs are the zeros, signs kept
        otherwise          se = clamp(floor(log2 a) - emax, -127, 127)       (floor(log2 a): the exponent of a, the true one
                                                                               for an fp32 subnormal)
    and y = round_elem(v / 2^se) * 2^se.

Every step is exact real arithmetic: v / 2^se is a scaling by a power of two (computed in fp64 here: nothing is flushed or
rounded), a scaled value below fp32's normal range lies far below half the smallest step of either element format, and q * 2^se
always fits fp32 (2^-9 * 2^-127 = 2^-136 is a multiple of 2^-149; 448 * 2^119 and 6 * 2^125 are below 2^128).  So there is no
tolerance anywhere: tests/test_mx_gpu.py holds the kernel (k_fake_quant_mx, csrc/mx_kernels.hip) to this file bit for bit, the
scale codes included.
"""
import numpy as np

import fp8_model

BLOCK = 32
EMAX = {"mxfp8": 8, "mxfp4": 2}
ELEM_MAX = {"mxfp8": 448.0, "mxfp4": 6.0}
E2M1_CODES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float32)


def e2m1_round(v):
    """fp64 in (exact for every fp32 and every fp32 / 2^se), the nearest E2M1 value out, as fp64."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        a = np.minimum(np.abs(v), 6.0)                                   # saturate (inf too); NaN passes through
        _, ex = np.frexp(a)                                              # a = m * 2^ex, m in [0.5, 1): binade ex - 1
        step = np.ldexp(1.0, np.maximum(ex - 1, 0) - 1)                  # one mantissa bit; below 1 the step stays 0.5
        return np.copysign(np.rint(a / step) * step, v)                  # np.rint: half to even = the even mantissa


def _e4m3_round64(w):
    """fp8_model.e4m3_round takes fp32; a scaled value w = v / 2^se is an fp32 value wherever it is not below fp32's normal
    range, and there it rounds to the zero of its sign either way (|w| < 2^-126 against a smallest step of 2^-9)."""
    with np.errstate(all="ignore"):
        tiny = np.abs(w) < 2.0 ** -126
        return np.where(tiny, np.copysign(0.0, w), fp8_model.e4m3_round(np.where(tiny, 0.0, w).astype(np.float32)).astype(np.float64))


def floor_log2(a):
    """The exponent of a positive finite fp32 `a` (the true one for a subnormal), from np.frexp."""
    _, ex = np.frexp(np.asarray(a, np.float32).astype(np.float64))
    return ex.astype(np.int64) - 1


def shared_exponent(a, elem):
    """se of a block whose max |v| is `a` (finite, >= 0)."""
    a = np.asarray(a, np.float32)
    return np.where(a == 0, -127, np.clip(floor_log2(np.where(a == 0, 1, a)) - EMAX[elem], -127, 127)).astype(np.int64)


def fake_quant_mx(x, axis, elem, return_scales=False):
    x = np.asarray(x, np.float32)
    axis = axis % x.ndim
    outer, K = int(np.prod(x.shape[:axis], dtype=np.int64)), x.shape[axis]
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    nblk = -(-K // BLOCK)
    x3 = x.reshape(outer, K, inner)
    y = np.empty_like(x3)
    scales = np.empty((outer, nblk, inner), np.uint8)
    rnd = e2m1_round if elem == "mxfp4" else _e4m3_round64
    for b in range(nblk):
        with np.errstate(invalid="ignore"):                                   # (signalling NaNs in the input)
            v = x3[:, b * BLOCK:(b + 1) * BLOCK, :].astype(np.float64)        # the elements that exist
            a = np.max(np.abs(v), axis=1, keepdims=True)                      # NaN if the block holds one (np.max propagates)
        bad = ~np.isfinite(a)
        se = shared_exponent(np.where(bad, 0, a).astype(np.float32), elem)
        X = np.ldexp(1.0, se)
        with np.errstate(all="ignore"):
            q = rnd(v / X) * X
        y[:, b * BLOCK:(b + 1) * BLOCK, :] = np.where(bad, np.nan, q).astype(np.float32)
        scales[:, b, :] = np.where(bad, 0xFF, se + 127)[:, 0, :]
    y = y.reshape(x.shape)
    return (y, scales) if return_scales else y


def codes(elem):
    """The non-negative finite values of the element format, ascending."""
    return E2M1_CODES.copy() if elem == "mxfp4" else fp8_model.e4m3_codes()


def boundary_points(elem):
    """Where a rounding to the element format can go wrong, both signs: every code and its fp32 neighbours, the midpoints of
    adjacent codes (the ties) and their fp32 neighbours, the tie between the largest code and the next one the format does not
    have (464 for E4M3, 7 for E2M1) and its lower neighbour."""
    c = codes(elem)
    mids = ((c[:-1].astype(np.float64) + c[1:]) / 2).astype(np.float32)
    over = np.float32(464.0 if elem == "mxfp8" else 7.0)
    base = np.concatenate([c, mids])
    inf = np.float32(np.inf)
    pts = np.concatenate([base, np.nextafter(base, inf), np.nextafter(base, -inf), np.array([over, np.nextafter(over, np.float32(0))], np.float32)])
    pts = pts[pts >= 0]
    return np.concatenate([pts, -pts]).astype(np.float32)
