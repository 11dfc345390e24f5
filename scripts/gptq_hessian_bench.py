#!/usr/bin/env python3
"""GPTQ's layer Hessian on one MI355X: ops.gptq_hessian (dpl_gptq_hessian: X^T X as an fp64 SYRK on v_mfma_f64_16x16x4_f64, Conv
patches gathered in the kernel) beside the path it replaces — weight_transform.gptq.input_rows (F.pad + F.unfold for a Conv), one
fp32 matmul of the BLAS library, .double() and the add onto H — on one slab of the same data: the slab weight_transform.gptq.hessian
would take (whole images, at most 256 MB of fp32 rows and 65536 rows).  The layers: ResNet-50 convolutions at batch 64 and the two
reduction lengths of a ViT-B MLP over 64 images.

Method: HIP events around each call; --buffers copies of the slab used in rotation, so no call finds its input in a cache the
previous call filled; the two paths alternate call by call within one loop (what drifts, drifts for both); one warm-up round,
then the median of --reps.  TFLOP/s: rows * K * (K + 64) — the multiply-adds of the tiles on and below the diagonal, two flops
each — over the device time.  One JSON line per layer:  python scripts/gptq_hessian_bench.py [--reps 7] [--buffers 3]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, x shape, weight shape or None, strides, ONNX pads)
LAYERS = (("resnet50 3x3 64->64 @56", (64, 64, 56, 56), (64, 64, 3, 3), [1, 1], [1, 1, 1, 1]),
          ("resnet50 1x1 256->64 @56", (64, 256, 56, 56), (64, 256, 1, 1), [1, 1], [0, 0, 0, 0]),
          ("resnet50 3x3 512->512 @7", (64, 512, 7, 7), (512, 512, 3, 3), [1, 1], [1, 1, 1, 1]),
          ("resnet50 7x7 s2 3->64 @224", (64, 3, 224, 224), (64, 3, 7, 7), [2, 2], [3, 3, 3, 3]),
          ("vit-b [64*197, 768]", (64, 197, 768), None, None, None),
          ("vit-b [64*197, 3072]", (64, 197, 3072), None, None, None))
PEAK_FP64_MATRIX_TFLOPS = 78.6       # MI355X data sheet


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--buffers", type=int, default=3)
    a = p.parse_args()
    from dipoorlet_amd import ops
    G = importlib.import_module("dipoorlet_amd.weight_transform.gptq")      # (the package's attribute of this name is the function)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for name, shape, wshape, strides, pads in LAYERS:
        if wshape is None:
            node = types.SimpleNamespace(op_type="MatMul", attrs={}, name=name)
            K = shape[-1]
        else:
            node = types.SimpleNamespace(op_type="Conv", name=name, attrs={"strides": strides, "pads": pads, "dilations": [1, 1]})
            K = wshape[1] * wshape[2] * wshape[3]
        probe = torch.empty((1,) + shape[1:], device=dev)
        per_image = G.rows_per_image(node, probe, wshape)
        images = min(shape[0], max(1, min(G._SLAB_ROWS, G._SLAB_BYTES // (4 * K)) // per_image))
        xs = [torch.randn((images,) + shape[1:], device=dev) for _ in range(a.buffers)]
        H_dev = torch.zeros((K, K), dtype=torch.float64, device=dev)
        H_blas = torch.zeros((K, K), dtype=torch.float64, device=dev)

        def device(x):
            return G._hessian_device(node, x, wshape, H_dev)

        def blas(x):
            X = G.input_rows(node, x, wshape)
            H_blas.add_(torch.matmul(X.t(), X).double())
            return X.shape[0]

        rows = device(xs[0])
        assert rows == blas(xs[0]) == images * per_image
        torch.cuda.synchronize()
        t_dev, t_blas = [], []
        for i in range(a.reps):
            x = xs[(i + 1) % a.buffers]
            t_dev.append(_event_ms(lambda: device(x)))
            t_blas.append(_event_ms(lambda: blas(x)))
        d, b = statistics.median(t_dev), statistics.median(t_blas)
        tflops = rows * K * (K + 64) / (d * 1e-3) / 1e12
        print(json.dumps({"layer": name, "K": K, "slab_images": images, "rows": rows, "splits": ops.gptq_hessian_splits(rows, K),
                          "device_ms": round(d, 3), "blas_ms": round(b, 3), "blas_over_device": round(b / d, 2),
                          "device_tflops": round(tflops, 2), "share_of_fp64_matrix_peak": round(tflops / PEAK_FP64_MATRIX_TFLOPS, 3),
                          "max_rel_diff": float((H_dev - H_blas).abs().max() / H_blas.abs().max())}), flush=True)
        del xs, H_dev, H_blas


if __name__ == "__main__":
    main()
