#!/usr/bin/env python3
"""GPTQ layer timing on one MI355X: ops.gptq_quantize (the one-wave-per-row HIP kernel per block of 128 columns + one BLAS GEMM
between blocks) against the same arithmetic as an eager torch loop (one rounding and one rank-1 update per column inside a
block, the same GEMM between blocks), on transformer / ResNet layer shapes, int8 per-channel grid.  HIP events around whole
layers: the median of --reps timed calls after one warm-up call, for every figure.  Also where a layer's time goes: the kernel calls alone, the inter-block GEMMs alone, the Hessian GEMMs (X^T X of N
input rows) and the host factorisation (fp64, CPU: download + two Cholesky factorisations + an inverse + upload).  One JSON line
per shape:  python scripts/gptq_bench.py [--reps 5] [--rows_x 4096]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(768, 3072), (3072, 768), (512, 4608)]      # R x K: a ViT-B MLP's two products, a ResNet layer4 3x3 convolution
BLOCK = 128


def _timed(fn, reps):
    """Median milliseconds of fn() by HIP events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def eager_layer(w, u, scale, qlo, qhi):
    """gptq_model.gptq_layer32 in eager torch: K roundings, K rank-1 updates, K / 128 GEMMs."""
    wq = w.clone()
    K = w.shape[1]
    s = scale
    for c0 in range(0, K, BLOCK):
        nb = min(BLOCK, K - c0)
        err = torch.empty((w.shape[0], nb), device=w.device)
        for j in range(nb):
            c = c0 + j
            col = wq[:, c]
            q = torch.clamp(torch.round(col / s), qlo, qhi) * s
            e = (col - q) / u[c, c]
            wq[:, c] = q
            err[:, j] = e
            if j + 1 < nb:
                wq[:, c + 1:c0 + nb] -= e[:, None] * u[c, c + 1:c0 + nb][None, :]
        if c0 + nb < K:
            wq[:, c0 + nb:].addmm_(err, u[c0:c0 + nb, c0 + nb:], alpha=-1.0)
    return wq


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--rows_x", type=int, default=4096, help="input rows N of the Hessian X^T X")
    a = p.parse_args()
    from dipoorlet_amd import ops
    from dipoorlet_amd.weight_transform.gptq import factor
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for R, K in SHAPES:
        w = torch.randn(R, K, device=dev) * 0.05
        x = torch.randn(a.rows_x, K, device=dev) @ (torch.eye(K, device=dev) + 0.05 * torch.randn(K, K, device=dev))
        H = (x.t() @ x).double() / a.rows_x
        t0 = time.perf_counter()
        U, _ = factor(H.cpu(), 0.01)
        u = U.to(torch.float32).contiguous().to(dev)
        torch.cuda.synchronize()
        factor_ms = (time.perf_counter() - t0) * 1e3
        scale = w.abs().max(1).values / 127.0
        grid = ops.GptqGrid("int", scale, torch.zeros(R, dtype=torch.int32, device=dev), -127, 127)
        blocks = [(c0, min(BLOCK, K - c0)) for c0 in range(0, K, BLOCK)]
        work, errs = w.clone(), [torch.empty((R, nb), device=dev) for _, nb in blocks]

        def kernels_only():
            for (c0, nb), e in zip(blocks, errs):
                ops.gptq_block(work, c0, nb, u, grid, err=e)

        def gemms_only():
            for (c0, nb), e in zip(blocks, errs):
                if c0 + nb < K:
                    work[:, c0 + nb:].addmm_(e, u[c0:c0 + nb, c0 + nb:], alpha=-1.0)

        res = {"rows": R, "cols": K, "block": BLOCK,
               "gptq_quantize_ms": round(_timed(lambda: ops.gptq_quantize(w, u, grid, BLOCK), a.reps), 3),
               "eager_ms": round(_timed(lambda: eager_layer(w, u, scale, -127.0, 127.0), a.reps), 3),
               "kernel_calls_ms": round(_timed(kernels_only, a.reps), 3),
               "interblock_gemms_ms": round(_timed(gemms_only, a.reps), 3),
               "hessian_gemm_ms": round(_timed(lambda: (x.t() @ x).double(), a.reps), 3), "hessian_rows": a.rows_x,
               "host_factor_ms": round(factor_ms, 1)}
        wq, _ = ops.gptq_quantize(w, u, grid, BLOCK)
        same = float((wq == eager_layer(w, u, scale, -127.0, 127.0)).float().mean())
        res.update(speedup=round(res["eager_ms"] / res["gptq_quantize_ms"], 1), share_equal_to_eager=round(same, 5))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
