"""The definition of `--gptq` (GPTQ, Frantar et al., 2022: Hessian-compensated weight rounding), as a numpy model.

W is [R, K], one output channel per row.  H = X^T X / N is the [K, K] second moment of the layer's (fake-quantised) inputs.  The
weights are rounded one input column at a time, and each column's rounding error is pushed onto the columns not yet rounded along
the inverse Hessian, which keeps tr((Wq - W) H (Wq - W)^T) — the layer's output error on the calibration inputs — small.

  * `make_q(grid)`: the element quantiser Q the fake-quantised graph applies to the initializer — the integer grid's fq_one,
    fl32((clamp(rint(fl32(w / s)) + zp, qlo, qhi) - zp) * s), or FP8's fl32(e4m3_round(fl32(w / s)) * s) — with s (and zp) per row
    or one value for the tensor.
  * `factor(H, damp)` (fp64): dead columns (H[j, j] == 0) get H[j, j] = 1 and their weights stay (they end up rounded to nearest);
    H += damp * mean(diag H) * I; U = the upper Cholesky factor of H^-1 (H^-1 = U^T U).  A failed factorisation multiplies damp by
    10, at most three times; then it returns None with a warning (the layer stays at round-to-nearest).
  * `gptq_block(W, U, c0, nb, Q)`: fp32, every operation a single IEEE fp32 operation, in this order — what the kernel
    (csrc/gptq_kernels.hip) is held to bit for bit, Err included.
  * `gptq_layer32`: the blocks left to right, with the fp32 GEMM W[:, c0 + nb:] -= Err @ U[c0:c0 + nb, c0 + nb:] between them (the
    only place the device may differ from this file: by summation order).
  * `gptq_layer64`: the same recursion column by column in fp64 (only Q sees fp32).
  * `objective(Wq, W, H)`: tr((Wq - W) H (Wq - W)^T) in fp64.
"""
import warnings

import numpy as np

from fp8_model import e4m3_round

INT, E4M3 = "int", "e4m3"


def make_q(grid):
    """grid: {"fmt": INT | E4M3, "scale": fp32 [R] or [1], and for INT "zp": int [R] or [1], "qlo", "qhi"} -> Q(w) for w of
    shape [R] (one column) or [R, n]."""
    scale = np.asarray(grid["scale"], np.float32).reshape(-1)
    zp = np.asarray(grid.get("zp", 0), np.float32).reshape(-1)
    fmt = grid["fmt"]
    qlo, qhi = np.float32(grid.get("qlo", 0)), np.float32(grid.get("qhi", 0))

    def Q(w):
        w = np.asarray(w, np.float32)
        s, z = (scale, zp) if w.ndim == 1 else (scale[:, None], zp[:, None])
        with np.errstate(all="ignore"):
            t = (w / s).astype(np.float32)
            if fmt == E4M3:
                return (e4m3_round(t) * s).astype(np.float32)
            q = np.clip((np.rint(t) + z).astype(np.float32), qlo, qhi)
            return ((q - z).astype(np.float32) * s).astype(np.float32)
    return Q


def factor(H, damp=0.01, retries=3):
    """-> (U fp64 [K, K] upper with H^-1 = U^T U, the damping used), or (None, damp) when the factorisation failed."""
    H = np.array(H, np.float64)
    d = np.arange(H.shape[0])
    dead = H[d, d] == 0
    H[d[dead], d[dead]] = 1.0
    mean_diag = float(np.mean(H[d, d]))
    for _ in range(retries + 1):
        Hd = H.copy()
        Hd[d, d] += damp * mean_diag
        try:
            L = np.linalg.cholesky(Hd)
            Linv = np.linalg.solve(L, np.eye(H.shape[0]))
            U = np.linalg.cholesky(Linv.T @ Linv).T
            if np.all(np.isfinite(U)):
                return U, damp
        except np.linalg.LinAlgError:
            pass
        damp *= 10.0
    warnings.warn("gptq: the Hessian could not be factorised; the layer stays at round-to-nearest")
    return None, damp


def gptq_block(W, U, c0, nb, Q):
    """In place on W (fp32 [R, ldw]) -> Err fp32 [R, nb].  U: fp32, indexed by absolute column."""
    assert W.dtype == np.float32 and U.dtype == np.float32
    err = np.zeros((W.shape[0], nb), np.float32)
    for j in range(nb):
        c = c0 + j
        w = W[:, c].copy()
        q = Q(w)
        e = ((w - q).astype(np.float32) / U[c, c]).astype(np.float32)
        W[:, c] = q
        err[:, j] = e
        for k in range(j + 1, nb):
            W[:, c0 + k] = (W[:, c0 + k] - (e * U[c, c0 + k]).astype(np.float32)).astype(np.float32)
    return err


def gptq_layer32(W, U, Q, block=128):
    """-> (Wq fp32 [R, K], Err fp32 [R, K])"""
    W = np.array(W, np.float32)
    U = np.asarray(U, np.float32)
    K = W.shape[1]
    err = np.zeros_like(W)
    for c0 in range(0, K, block):
        nb = min(block, K - c0)
        err[:, c0:c0 + nb] = gptq_block(W, U, c0, nb, Q)
        if c0 + nb < K:
            W[:, c0 + nb:] -= (err[:, c0:c0 + nb] @ U[c0:c0 + nb, c0 + nb:]).astype(np.float32)
    return W, err


def gptq_layer64(W, U, Q):
    W = np.array(W, np.float64)
    U = np.asarray(U, np.float64)
    for c in range(W.shape[1]):
        w = W[:, c].copy()
        q = Q(w.astype(np.float32)).astype(np.float64)
        e = (w - q) / U[c, c]
        W[:, c] = q
        W[:, c + 1:] -= np.outer(e, U[c, c + 1:])
    return W.astype(np.float32)


def objective(Wq, W, H):
    d = np.asarray(Wq, np.float64) - np.asarray(W, np.float64)
    return float(np.einsum("rk,kl,rl->", d, np.asarray(H, np.float64), d))
