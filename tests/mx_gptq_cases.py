"""The inputs the --mx_gptq tests share (CPU: test_mx_gptq_model.py; GPU: test_mx_gptq_gpu.py).

Layers: (R, K, N, seed) drawn exactly as gptq_cases.build draws them — A, X, W from default_rng(seed) in that order, H = X^T X / N in
fp64, U = factor(H, 0.01) — and run through the models of mx_gptq_model.py for both element formats.

Constructed single blocks (K = 32, one call): hand-made upper-triangular U with a positive diagonal (any such matrix is a legal
input) and weights chosen so that one thing happens.  Numbers per element format: `big` sits in the top binade of the block
(se = 0: [4, 8) for E2M1, [256, 512) for E4M3), `w0` is a first column whose rounding leaves the error d = w0 - Q(w0), and one
entry U[0, k] turns d into the compensation the case is about.
  shrink    the entry maximum (column 5) is compensated down into a lower binade: the result's own floor byte is below the entry byte
  saturate  a later column (3) is pushed past the largest element: it comes out as exactly +-top * 2^se
  zeros     all-zero rows, both signs of zero mixed, U >= 0: byte 0, the zeros with their signs, errors 0
  ties      U diagonal (no compensation): values exactly half-way between two codes round to the even mantissa
Rows: the values, their negation, and (shrink, saturate, ties) the values times 2^-20 — another shared exponent, the same codes.
"""
import functools

import numpy as np

import mx_gptq_model as G
import mx_model as M

ELEMS = ("mxfp4", "mxfp8")
LAYER_CASES = [(64, 288, 2048, 11), (48, 300, 64, 12), (32, 576, 16, 13)]
RAGGED = (8, 72, 512, 5)                 # K = 72: the last MX block holds 8 columns
SINGLE_CALL = (5, 128, 256, 15)          # one kernel call, no GEMM: the device must equal gptq_mx_layer32 exactly
CONSTRUCTED = ("shrink", "saturate", "zeros", "ties")


def case_id(c):
    return "x".join(str(v) for v in c[:2]) + f"-N{c[2]}"


@functools.lru_cache(maxsize=None)
def draw(case):
    R, K, N, seed = case
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, K)) * (rng.random((K, K)) < 0.1)
    X = (rng.standard_normal((N, K)) @ (np.eye(K) + 0.5 * A)).astype(np.float32)
    W = (0.05 * rng.standard_normal((R, K))).astype(np.float32)
    H = X.astype(np.float64).T @ X.astype(np.float64) / N
    U, _ = G.factor(H, 0.01)
    return W, H, U


@functools.lru_cache(maxsize=None)
def build(case, elem):
    """-> dict(W, H, U fp64, Wn = round to nearest, W64 = gptq_mx_layer64, W32 / E32 / S32 = gptq_mx_layer32) — computed once and
    shared: treat every array as read-only."""
    W, H, U = draw(case)
    W32, E32, S32 = G.gptq_mx_layer32(W, U, elem, 128)
    out = dict(W=W, H=H, U=U, Wn=M.fake_quant_mx(W, 1, elem), W64=G.gptq_mx_layer64(W, U, elem), W32=W32, E32=E32, S32=S32)
    for v in out.values():
        v.setflags(write=False)
    return out


# elem: (top, big, near_top, w0, Q(w0))
_NUM = {"mxfp4": (6.0, 4.2, 5.0, 0.7, 0.5), "mxfp8": (448.0, 300.0, 440.0, 1.03, 1.0)}
# values half-way between two codes under se = 0 -> the code with the even mantissa
TIES = {"mxfp4": [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0)],
        "mxfp8": [(2.0 ** -10, 0.0), (3 * 2.0 ** -10, 2.0 ** -8), (1.0625, 1.0), (1.1875, 1.25), (17.0, 16.0), (19.0, 20.0), (432.0, 448.0), (400.0, 384.0)]}


def constructed(name, elem):
    """-> (W fp32 [R, 32], U fp32 [32, 32])"""
    top, big, near_top, w0, q0 = _NUM[elem]
    rng = np.random.default_rng(7)
    U = np.triu(0.05 * rng.standard_normal((32, 32))).astype(np.float32)
    U[np.arange(32), np.arange(32)] = (0.5 + rng.random(32)).astype(np.float32)
    U[0, 0] = 1.0
    d = np.float32(w0) - np.float32(q0)
    row = (0.1 * top / 6.0 * rng.standard_normal(32)).astype(np.float32)         # small beside `big`
    row[0] = w0
    if name == "shrink":
        row[5] = big
        U[0, 5] = np.float32(0.6 * big / d)                    # column 5 loses 0.6 of its value before it is rounded
    elif name == "saturate":
        row[3] = near_top
        U[0, 1:3] = 0.0                                        # (columns 1 and 2 stay small: column 3 alone is pushed)
        U[1:3, 3] = 0.0
        U[0, 3] = np.float32(-(1.25 * top - near_top) / d)     # column 3 arrives at about 1.25 * top
    elif name == "zeros":
        z = np.zeros(32, np.float32)
        z[1::3] = -0.0
        # every error is +0.0 and U >= 0 here, so every update is x - (+0.0) = x: a zero keeps its sign up to its own rounding,
        # which keeps it too (under a negative U[c, k] the update -0.0 - (-0.0) is +0.0: IEEE's, not the rounding's)
        return np.stack([z, -z, np.zeros(32, np.float32)]), np.abs(U)
    elif name == "ties":
        row = np.zeros(32, np.float32)
        vals = [v for v, _ in TIES[elem]]
        row[:len(vals)] = vals
        row[31] = big                                          # se = 0
        U = np.diag(np.diag(U)).astype(np.float32)
    else:
        raise ValueError(name)
    return np.stack([row, -row, (row * np.float32(2.0 ** -20)).astype(np.float32)]), U
