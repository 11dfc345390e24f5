#!/usr/bin/env python3
"""GPTQ's Hessian factorisation on one MI355X: ops.gptq_factor's kernels (dpl_gptq_factor: one blocked fp64 Cholesky factorisation
and one triangular inverse on v_mfma_f64_16x16x4_f64) beside weight_transform.gptq.factor on the host (download, two Cholesky
factorisations and an inverse in LAPACK, upload), in one process, on the Hessians scripts/gptq_bench.py builds (--rows_x correlated
input rows).  HIP events: the median of --reps timed calls after one warm-up call, for every figure; the device call is also timed
in its two parts (dpl_gptq_factor_phase).  TFLOP/s: 2 K^3 / 3 over the whole device call — a whole-call rate against the fp64
matrix peak, not a kernel's share of it.  One JSON line per K:  python scripts/gptq_factor_bench.py [--reps 5] [--rows_x 4096]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.gptq_bench import _timed  # noqa: E402

SIZES = (768, 3072, 4608)            # a ViT-B MLP's two reduction lengths, a ResNet layer4 3x3 convolution's
PEAK_FP64_MATRIX_TFLOPS = 78.6       # MI355X data sheet


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--rows_x", type=int, default=4096, help="input rows N of the Hessian X^T X")
    p.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    a = p.parse_args()
    from dipoorlet_amd import _hip, ops
    from dipoorlet_amd.weight_transform.gptq import factor
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lib = _hip.lib()
    for K in a.sizes:
        x = torch.randn(a.rows_x, K, device=dev) @ (torch.eye(K, device=dev) + 0.05 * torch.randn(K, K, device=dev))
        H = ((x.t() @ x).double() / a.rows_x).contiguous()
        nbytes = int(lib.dpl_gptq_factor_workspace(K))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        U = torch.empty((K, K), dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)

        def phase(which):
            _hip.check(lib.dpl_gptq_factor_phase(H.data_ptr(), K, 0.01, U.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, which,
                                                 torch.cuda.current_stream().cuda_stream), "dpl_gptq_factor_phase")

        def host():
            return factor(H.cpu(), 0.01)[0].to(torch.float32).contiguous().to(dev)

        res = {"K": K, "hessian_rows": a.rows_x, "workspace_mb": round(nbytes / 2 ** 20, 1),
               "device_ms": round(_timed(lambda: phase(3), a.reps), 3),
               "device_cholesky_ms": round(_timed(lambda: phase(1), a.reps), 3),
               "device_inverse_ms": round(_timed(lambda: phase(2), a.reps), 3),
               "ops_gptq_factor_ms": round(_timed(lambda: ops.gptq_factor(H, 0.01), a.reps), 3),
               "host_factor_ms": round(_timed(host, a.reps), 1)}
        phase(3)
        u_host = factor(H.cpu(), 0.01)[0].to(dev)
        res.update(status=int(status.item()), host_over_device=round(res["host_factor_ms"] / res["ops_gptq_factor_ms"], 1),
                   device_tflops=round(2 * K ** 3 / 3 / (res["device_ms"] * 1e-3) / 1e12, 3),
                   share_of_fp64_matrix_peak=round(2 * K ** 3 / 3 / (res["device_ms"] * 1e-3) / 1e12 / PEAK_FP64_MATRIX_TFLOPS, 4),
                   max_diff_over_max_u=float((U - u_host).abs().max() / u_host.abs().max()))
        print(json.dumps(res), flush=True)
        del x, H, ws, U, u_host


if __name__ == "__main__":
    main()
