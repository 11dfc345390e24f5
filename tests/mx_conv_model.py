"""The definition of dpl_mx_conv / ops.mx_conv (`--mx_conv`): a convolution (group 1) of two packed MX operands, as a numpy model on
top of tests/mx_pack_model.py (the definition of the bytes) and tests/mx_gemm_model.py (the operand decoding, the bound).

Operands     both blocked along axis 1 and K-INNERMOST, as mx_pack_model.encode(x, 1, elem) writes them:
               A  codes uint8 [n, h, w, Cb * bb], scales uint8 [n, h, w, Cb]           of an [n, c, h, w] activation (NHWC)
               B  codes uint8 [cout, kh, kw, Cb * bb], scales uint8 [cout, kh, kw, Cb] of a [cout, c, kh, kw] weight
             Cb = ceil(c / 32); bb = 32 (mxfp8) or 16 (mxfp4) bytes a block.
Product      C[b, oy, ox, co] = sum over ky, kx and ch < 32 Cb of
                 a[b, oy sh - pt + ky dh, ox sw - pl + kx dw, ch] * b[co, ky, kx, ch],      fp32 [n, oh, ow, cout] (NHWC)
             a and b = mx_pack_model.decode_elements of every (code, scale) pair — the pad codes of a short last channel block
             included —, summed in fp64.  A tap outside the image contributes nothing (and its bytes are never looked at).
NaN rule     C[b, oy, ox, co] is NaN if a block of A inside an in-image tap of that output, or any block of row co of B, holds a
             0xFF scale byte or an E4M3 NaN code (0x7F, 0xFF) — whatever the other operand holds there.  A bad pixel that no tap
             of an output reaches leaves that output finite.
S            sum |a| * |b| per output over the finite pairs (NaN where C is), the scale of mx_gemm_model.bound with
             Kp = kh * kw * 32 * Cb.
"""
import numpy as np

import mx_gemm_model as G

BLOCK = G.BLOCK


def out_size(size, k, stride, pad_begin, pad_end, dil):
    """ONNX Conv's output length along one axis under explicit pads."""
    return (size + pad_begin + pad_end - dil * (k - 1) - 1) // stride + 1


def mx_conv(a_codes, a_scales, b_codes, b_scales, elem_a, elem_b=None, *, strides, pads, dilations, out_hw):
    """pads = (top, left) -> (C fp32 [n, oh, ow, cout], S fp64 [n, oh, ow, cout])."""
    elem_b = elem_a if elem_b is None else elem_b
    a, b = G.decode_operand(a_codes, a_scales, elem_a), G.decode_operand(b_codes, b_scales, elem_b)      # [n, h, w, Cp], [cout, kh, kw, Cp]
    assert a.ndim == 4 and b.ndim == 4 and a.shape[-1] == b.shape[-1]
    n, h, w, _ = a.shape
    cout, kh, kw, _ = b.shape
    (sh, sw), (pt, pl), (dh, dw), (oh, ow) = strides, pads, dilations, out_hw
    bad_a, bad_b = np.isnan(a).any(-1), np.isnan(b).any(-1).any(-1).any(-1)                              # [n, h, w], [cout]
    a0, b0 = np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b)
    c, s = np.zeros((n, oh, ow, cout)), np.zeros((n, oh, ow, cout))
    bad = np.zeros((n, oh, ow), bool)
    oy, ox = np.arange(oh), np.arange(ow)
    with np.errstate(over="ignore", invalid="ignore"):
        for ky in range(kh):
            iy = oy * sh - pt + ky * dh
            ys = (iy >= 0) & (iy < h)
            for kx in range(kw):
                ix = ox * sw - pl + kx * dw
                xs = (ix >= 0) & (ix < w)
                if not ys.any() or not xs.any():
                    continue
                at = np.ix_(np.arange(n), np.nonzero(ys)[0], np.nonzero(xs)[0])
                px = np.ix_(np.arange(n), iy[ys], ix[xs])
                c[at] += np.matmul(a0[px], b0[:, ky, kx, :].T)
                s[at] += np.matmul(np.abs(a0[px]), np.abs(b0[:, ky, kx, :]).T)
                bad[at] |= bad_a[px]
        nan = bad[..., None] | bad_b[None, None, None, :]
        c = np.where(nan, np.nan, c).astype(np.float32)
    return c, np.where(nan, np.nan, s)


def as_gemm(a_codes, a_scales, b_codes, b_scales):
    """The operands of a 1 x 1 / stride 1 / pad 0 convolution as mx_gemm_model.mx_gemm's: A [n, h * w, ...], B [cout, ...]."""
    assert b_codes.shape[1:3] == (1, 1)
    n, h, w = a_codes.shape[:3]
    cout = b_codes.shape[0]
    return (a_codes.reshape(n, h * w, -1), a_scales.reshape(n, h * w, -1), b_codes.reshape(cout, -1), b_scales.reshape(cout, -1))
