#!/usr/bin/env python3
"""--mx_gptq layer timing on one MI355X: ops.gptq_mx_quantize (k_gptq_mx_block per 128 columns + one BLAS GEMM between calls) for
MXFP4 and MXFP8, beside ops.gptq_quantize on the static E4M3 grid (k_gptq_block<E4M3>: the same chain with a convert-style rounding
and a per-row scale instead of the block maximum and the integer rounding), on the two products of a ViT-B MLP as [rows, K]
weights.  HIP events around whole layers; the variants are timed in alternating rounds (one call of each per round, after one
warm-up round) and every figure is the median over --reps rounds.  Also the split of a layer between its kernel calls and its
inter-block GEMMs.  One JSON line per shape:  python scripts/mx_gptq_bench.py [--reps 7] [--rows_x 4096]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(768, 3072), (3072, 768)]      # R x K
BLOCK = 128


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _alternating(fns, reps):
    """{name: median ms}: one warm-up round, then `reps` rounds of one timed call of every variant in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(_once(fn))
    return {k: round(sorted(v)[len(v) // 2], 3) for k, v in ms.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
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
        U, _ = factor(H.cpu(), 0.01)
        u = U.to(torch.float32).contiguous().to(dev)
        grid = ops.GptqGrid("e4m3", w.abs().max(1).values / 448.0)
        blocks = [(c0, min(BLOCK, K - c0)) for c0 in range(0, K, BLOCK)]
        work, errs = w.clone(), [torch.empty((R, nb), device=dev) for _, nb in blocks]
        scales = torch.zeros((R, -(-K // 32)), dtype=torch.uint8, device=dev)

        def mx_kernels(elem):
            def run():
                for (c0, nb), e in zip(blocks, errs):
                    ops.gptq_mx_block(work, c0, nb, u, elem, err=e, scales=scales)
            return run

        def e4m3_kernels():
            for (c0, nb), e in zip(blocks, errs):
                ops.gptq_block(work, c0, nb, u, grid, err=e)

        def gemms_only():
            for (c0, nb), e in zip(blocks, errs):
                if c0 + nb < K:
                    work[:, c0 + nb:].addmm_(e, u[c0:c0 + nb, c0 + nb:], alpha=-1.0)

        t = _alternating({"mxfp4_quantize_ms": lambda: ops.gptq_mx_quantize(w, u, "mxfp4", BLOCK),
                          "mxfp8_quantize_ms": lambda: ops.gptq_mx_quantize(w, u, "mxfp8", BLOCK),
                          "e4m3_quantize_ms": lambda: ops.gptq_quantize(w, u, grid, BLOCK),
                          "mxfp4_kernel_calls_ms": mx_kernels("mxfp4"), "mxfp8_kernel_calls_ms": mx_kernels("mxfp8"),
                          "e4m3_kernel_calls_ms": e4m3_kernels, "interblock_gemms_ms": gemms_only}, a.reps)
        res = {"rows": R, "cols": K, "block": BLOCK, **t}
        for elem in ("mxfp4", "mxfp8"):
            res[elem + "_over_e4m3"] = round(t[elem + "_quantize_ms"] / t["e4m3_quantize_ms"], 3)
            res[elem + "_kernels_over_e4m3"] = round(t[elem + "_kernel_calls_ms"] / t["e4m3_kernel_calls_ms"], 3)
            wq, _, _ = ops.gptq_mx_quantize(w, u, elem, BLOCK)
            near = ops.gptq_mx_nearest(w, elem)
            obj = lambda q: float((((q - w).double() @ H) * (q - w).double()).sum())      # noqa: E731
            res[elem + "_objective_over_nearest"] = round(obj(wq) / obj(near), 4)
            res[elem + "_fixed_point"] = bool(torch.equal(ops.fake_quant_mx(wq, 1, elem).view(torch.int32), wq.view(torch.int32)))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
