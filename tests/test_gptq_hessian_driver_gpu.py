"""GPU: --gptq_hessian device in the driver.  weight_transform.hessian() with the flag off and on, on a Conv node with
asymmetric pads and stride 2 and on a MatMul node of a tiny graph: the same row count, and H within the fp32 summation bound of
the BLAS path — |H_device - H_blas| <= n 2^-24 (|X|^T |X|), n the rows of the largest slab, valid for any order the library sums
in (the device side adds exact products in fp64: its own error is 2^-29 of that).  Then one CLI run of test_gptq_e2e.py's small
ResNet with the Hessian, the factorisation and the recursion all in the library's kernels."""
import json
import types

import numpy as np
import pytest
import torch

from test_gptq_e2e import _cli, _network_error, workdir  # noqa: F401  (workdir: the module's fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]


def _graph():
    from dipoorlet_amd.models import _B
    g = _B(5)
    g.w("c.weight", (6, 5, 3, 2))
    x = g.node("Conv", ["input", "c.weight"], out="c_out", dilations=[1, 1], group=1, kernel_shape=[3, 2], pads=[0, 1, 2, 0], strides=[2, 2])
    x = g.node("Reshape", [x, g.const("shape", np.array([0, 6, -1], np.int64))], out="tokens")
    g.w("m.weight", (30, 20))
    out = g.node("MatMul", [x, "m.weight"], out="output")
    return g.finish("input", [1, 5, 11, 9], out)


@pytest.mark.parametrize("op,shape,weight_shape", [("Conv", (4, 5, 11, 9), (6, 5, 3, 2)), ("MatMul", (4, 6, 30), (30, 20))])
def test_driver_hessian_device_against_blas(op, shape, weight_shape):
    from dipoorlet_amd.weight_transform.gptq import hessian, input_rows
    node = next(n for n in _graph().graph.node if n.op_type == op)
    torch.manual_seed(1)
    chunks = [torch.randn(shape, device="cuda"), torch.randn((3,) + shape[1:], device="cuda")]
    K = 30
    blas = hessian(node, chunks, weight_shape, K, chunks[0].device)
    device = hessian(node, chunks, weight_shape, K, chunks[0].device, on_device=True)
    X = torch.cat([input_rows(node, x, weight_shape) for x in chunks]).double().abs()
    assert float(blas[-1]) == float(device[-1]) == X.shape[0]
    n = max(input_rows(node, x, weight_shape).shape[0] for x in chunks)      # (a chunk this small is one slab)
    excess = (device[:-1] - blas[:-1]).abs().view(K, K) - n * 2.0 ** -24 * (X.t() @ X)
    print(f"{op}: max |H_device - H_blas| {float((device - blas).abs().max()):.3e}, largest excess over the bound {float(excess.max()):.3e}")
    assert bool((excess <= 0).all())


def test_gptq_cli_with_hessian_factor_and_recursion_on_the_device(workdir):  # noqa: F811
    from dipoorlet_amd.utils import load_clip_val
    out = workdir / "out_hessian_device"
    assert _cli(workdir, out, "ocp_fp8", ["--gptq", "--gptq_hessian", "device", "--gptq_factor", "device"]) == 0
    report = json.load(open(out / "gptq_report.json"))
    assert report["hessian"] == "device" and report["factor"] == "device"
    assert len(report["layers"]) == 21 and all(e["kept"] == "gptq" for e in report["layers"]), report
    args = types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], output_dir=str(out))
    act, wt = load_clip_val(args)
    err_nearest = _network_error(str(workdir / "model.onnx"), workdir, act, wt, args)
    err_gptq = _network_error(str(out / "gptq.onnx"), workdir, act, wt, args)
    print(f"device Hessian: gptq / nearest output error {err_gptq / err_nearest:.4f}")
    assert err_gptq < 1.0 * err_nearest, (err_gptq, err_nearest)
