"""The definition of the `Float8E4M3FN` quantisation type (`-D ocp_fp8`), as a numpy model.

OCP FP8 E4M3 ("e4m3fn"): 1 sign bit, 4 exponent bits with bias 7, 3 mantissa bits; no infinities; subnormal step 2^-9 (below
2^-6); largest finite value 448 = 1.75 * 2^8.  A value v of binade e = floor(log2 |v|) lies on a grid of step 2^(max(e, -6) - 3).

  * `e4m3_round(v)`: fp32 -> the nearest e4m3fn value as fp32.  Round half to even, in the subnormal range too; SATURATING —
    |v| > 448 and +-inf give +-448; NaN stays NaN; the sign of zero is kept (so -1e-9 -> -0.0).
  * `fake_quant_fp8(x, scale, axis)`: fl32(e4m3_round(fl32(x / scale[c])) * scale[c]) — the division and the product are single
    fp32 operations (the kernel's __fdiv_rn / __fmul_rn; the library is built with -ffp-contract=off), the same shape as the
    integer grid's fq_one.  Per channel, c = (i / inner) % n_channels with inner = the elements behind `axis` (dpl_fake_quant).

These are ONNX opset 19 semantics: QuantizeLinear with a float8e4m3fn zero point and saturate = 1, then DequantizeLinear.
tests/test_fp8_model.py holds `e4m3_round` to torch's CPU cast (an independent implementation, which does not saturate: the
comparison covers |v| <= 464); tests/test_fp8_gpu.py holds the kernel (fq_elem<kFqFmtE4M3>, csrc/fake_quant_kernels.hip) to this file,
bit for bit.
"""
import numpy as np

E4M3_MAX = 448.0


def e4m3_round(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):                              # (signalling NaNs in the input)
        a = np.minimum(np.abs(v.astype(np.float64)), E4M3_MAX)       # saturate (inf too); NaN passes through np.minimum
        _, ex = np.frexp(a)                                          # a = m * 2^ex, m in [0.5, 1): binade e = ex - 1
        step = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
        r = np.rint(a / step) * step                                 # (a / step is exact in fp64; np.rint: half to even)
        return np.copysign(r, v).astype(np.float32)                  # NaN stays NaN, -0 stays -0


def fake_quant_fp8(x, scale, axis=None):
    x = np.asarray(x, np.float32)
    scale = np.asarray(scale, np.float32).reshape(-1)
    if scale.size > 1:
        shape = [1] * x.ndim
        shape[axis] = scale.size
        scale = scale.reshape(shape)
    with np.errstate(all="ignore"):
        q = e4m3_round((x / scale).astype(np.float32))
        return (q * scale).astype(np.float32)


def e4m3_codes():
    """The 127 non-negative finite e4m3fn values, ascending, from the encoding itself (code 0x7f is NaN)."""
    code = np.arange(127)
    e, m = code >> 3, code & 7
    return np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7)).astype(np.float32)


def boundary_points():
    """Where a rounding to e4m3fn can go wrong, both signs: every code and its fp32 neighbours, the midpoints of adjacent codes
    (the ties) and their fp32 neighbours, 464 (the tie between 448 and the 480 the format does not have) and its lower neighbour."""
    codes = e4m3_codes()
    mids = ((codes[:-1].astype(np.float64) + codes[1:]) / 2).astype(np.float32)      # exact: one more mantissa bit
    base = np.concatenate([codes, mids])
    inf = np.float32(np.inf)
    pts = np.concatenate([base, np.nextafter(base, inf), np.nextafter(base, -inf),
                          np.array([464.0, np.nextafter(np.float32(464.0), np.float32(0))], np.float32)])
    pts = pts[pts >= 0]
    return np.concatenate([pts, -pts]).astype(np.float32)
