"""The inputs the GPTQ tests share (CPU: test_gptq_model.py; GPU: test_gptq_gpu.py): synthetic layers with correlated inputs.

For a case (R, K, N, grid, seed), rng = default_rng(seed), drawn in this order:
    A = N(0, 1)[K, K] * (U(0, 1)[K, K] < 0.1);  X = fl32(N(0, 1)[N, K] @ (I + 0.5 A));  W = fl32(0.05 * N(0, 1)[R, K])
    H = X^T X / N in fp64
    int4: per row s = max|w| / 7 on [-7, 7];  e4m3: per row s = max|w| / 448;  uint4: ONE s = max|w| / 7, zero point 3, [0, 15]
    (an asymmetric per-tensor grid: weights below -3 s saturate)
N < K gives a singular H that only the damping makes factorisable."""
import collections
import functools

import numpy as np

import gptq_model as M

Case = collections.namedtuple("Case", "R K N grid seed")

LAYER_CASES = [Case(64, 288, 2048, "int4", 11), Case(64, 288, 2048, "e4m3", 11),
               Case(48, 300, 64, "int4", 12), Case(48, 300, 64, "e4m3", 12),
               Case(32, 576, 16, "int4", 13), Case(32, 576, 16, "e4m3", 13),
               Case(16, 200, 512, "uint4", 14)]
SINGLE_BLOCK = Case(5, 128, 256, "int4", 15)      # one block: no GEMM, the device must equal gptq_layer32 exactly
ALL_CASES = LAYER_CASES + [SINGLE_BLOCK]


def case_id(c):
    return f"{c.R}x{c.K}-N{c.N}-{c.grid}"


def make_grid(W, kind):
    a = np.abs(W).max(axis=1).astype(np.float32)
    if kind == "int4":
        return {"fmt": M.INT, "scale": (a / np.float32(7)).astype(np.float32), "zp": np.zeros(len(a), np.int32), "qlo": -7, "qhi": 7}
    if kind == "e4m3":
        return {"fmt": M.E4M3, "scale": (a / np.float32(448)).astype(np.float32)}
    if kind == "uint4":
        return {"fmt": M.INT, "scale": np.array([a.max() / np.float32(7)], np.float32), "zp": np.array([3], np.int32), "qlo": 0, "qhi": 15}
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def build(case):
    """-> dict(W, H, grid, U fp64, Wn = round to nearest, W64 = gptq_layer64, W32 / E32 = gptq_layer32) — computed once and shared:
    treat every array as read-only."""
    rng = np.random.default_rng(case.seed)
    R, K, N = case.R, case.K, case.N
    A = rng.standard_normal((K, K)) * (rng.random((K, K)) < 0.1)
    X = (rng.standard_normal((N, K)) @ (np.eye(K) + 0.5 * A)).astype(np.float32)
    W = (0.05 * rng.standard_normal((R, K))).astype(np.float32)
    H = X.astype(np.float64).T @ X.astype(np.float64) / N
    grid = make_grid(W, case.grid)
    Q = M.make_q(grid)
    U, _ = M.factor(H, 0.01)
    W32, E32 = M.gptq_layer32(W, U, Q, 128)
    out = dict(W=W, H=H, grid=grid, U=U, Wn=Q(W), W64=M.gptq_layer64(W, U, Q), W32=W32, E32=E32)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
