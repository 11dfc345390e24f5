"""The definition of `--mx_rotate`: a 32-point Hadamard rotation inside every MX block of both operands of a MatMul / Gemm, along
the reduction axis, as a numpy model.

H32 is the symmetric +-1 Sylvester matrix in natural order, H32[i][j] = (-1)^popcount(i & j), and H32 . H32 = 32 I.  With H =
blockdiag(H32, ..., H32) over a reduction length K = 32 m,

    (X . H) . (H . W / 32) = X . (H . H / 32) . W = X . W

so a network whose activation X is rotated at run time (`fwht32`, the kernel k_hadamard32 of csrc/hadamard_kernels.hip) and whose
weight W is rotated and scaled once, offline (`fold_weight`), computes the same function.  The identity is exact in real arithmetic.
What the rotation buys: an MX block has one power-of-two scale for its 32 values, and one large channel pushes the other 31 onto
the bottom codes of the element format; after the rotation the large value is spread evenly over the block (every output is a
+-1 combination of all 32 inputs).

What fp32 changes.  `fwht32` is five butterfly stages, each output of a stage one fp32 addition or subtraction: five roundings per
element, none where the values are small integers.  A stage at most doubles the largest magnitude, so the 32 outputs are bounded by
32 max |x| and overflow needs |x| > 2^122.  The 2^-5 of `fold_weight` is exact outside fp32's subnormal range.  A NaN or an
infinity anywhere in a block reaches every output of that block (inf - inf is NaN), so the whole rotated block is NaN or inf and
its MX scale code is 0xFF (mx_model.fake_quant_mx).

The pairs inside a stage are independent: the result does not depend on how a kernel maps elements to lanes, and
tests/test_mx_rotate_gpu.py holds the kernel to `fwht32` bit for bit.
"""
import numpy as np

import mx_model

BLOCK = mx_model.BLOCK


def h32():
    """H32 as int64 [32, 32]."""
    i = np.arange(BLOCK)
    pop = np.array([[bin(a & b).count("1") for b in i] for a in i])
    return np.where(pop % 2 == 0, 1, -1).astype(np.int64)


def fwht32(x):
    """x . blockdiag(H32) along the last axis (a multiple of 32), fp32, by the five stages h = 1, 2, 4, 8, 16: for every i with
    i & h == 0, (v[i], v[i | h]) <- (fl32(v[i] + v[i | h]), fl32(v[i] - v[i | h]))."""
    x = np.asarray(x, np.float32)
    if x.ndim < 1 or x.shape[-1] % BLOCK:
        raise ValueError(f"fwht32: the last axis must be a multiple of {BLOCK}, got shape {x.shape}")
    v = x.reshape(-1, BLOCK).copy()
    idx = np.arange(BLOCK)
    with np.errstate(all="ignore"):
        for h in (1, 2, 4, 8, 16):
            lo = idx[(idx & h) == 0]
            a, b = v[:, lo], v[:, lo | h]
            s, d = (a + b).astype(np.float32), (a - b).astype(np.float32)
            v[:, lo], v[:, lo | h] = s, d
    return v.reshape(x.shape)


def fold_weight(w, axis):
    """The constant operand of a rotated product: fwht32 along `axis` (the reduction axis), then * 2^-5."""
    w = np.moveaxis(np.asarray(w, np.float32), axis, -1)
    with np.errstate(all="ignore"):
        r = (fwht32(np.ascontiguousarray(w)) * np.float32(2.0 ** -5)).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(r, -1, axis))


def rotated_product(x, w, elem=None):
    """fwht32(x) @ fold_weight(w, 0) in fp64 — both operands through mx_model.fake_quant_mx along the reduction axis first when
    `elem` is 'mxfp8' / 'mxfp4'.  x: [M, K], w: [K, N]."""
    xr, wr = fwht32(x), fold_weight(w, 0)
    if elem is not None:
        xr, wr = mx_model.fake_quant_mx(xr, 1, elem), mx_model.fake_quant_mx(wr, 0, elem)
    return xr.astype(np.float64) @ wr.astype(np.float64)


def plain_product(x, w, elem=None):
    """x @ w in fp64, the operands MX-quantised first when `elem` is given."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    if elem is not None:
        x, w = mx_model.fake_quant_mx(x, 1, elem), mx_model.fake_quant_mx(w, 0, elem)
    return x.astype(np.float64) @ w.astype(np.float64)


def error_ratio(x, w, elem):
    """(rotated, plain): the relative Frobenius errors of the MX-quantised products against fp64 x @ w."""
    ref = plain_product(x, w)
    nrm = np.linalg.norm(ref)
    return (float(np.linalg.norm(rotated_product(x, w, elem) - ref) / nrm), float(np.linalg.norm(plain_product(x, w, elem) - ref) / nrm))
