"""GPU: the branches of the --mx_gptq driver (weight_transform/gptq.py) the tiny ViT of test_mx_gptq_e2e.py does not reach — a Gemm
with transB = 0 under --mx (its weight is [K, N] with the MX blocks along axis 0: transposed on the way in and out), a weight two
MatMuls read (left, with the reason: rounding it against one reader's Hessian would change the other), and --skip_layers.  (The
reasons for a constant left operand and for a constant of rank above 2 are plain strings in _why_left / _why_left_matmul.)"""
import json
import os
import types

import numpy as np
import pytest

import mx_model as M

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]

N, IMG = 96, 8            # 96 input rows for Hessians of 192 and 64 columns: the first one singular without the damping


def _build(d):
    """flat [N, 192] -> m1 (MatMul, w1 [192, 64]) -> ma, mb (MatMul, both read ws [64, 64]) -> fc (Gemm, transB = 0, [64, 10])"""
    from dipoorlet_amd.models import _B
    g = _B(5)
    x = g.node("Flatten", ["input"], out="flat", axis=1)
    x = g.node("MatMul", [x, g.w("w1", (192, 64), fan_in=192)], out="m1_out")
    ws = g.w("ws", (64, 64), fan_in=64)
    x = g.node("MatMul", [x, ws], out="ma_out")
    x = g.node("MatMul", [x, ws], out="mb_out")
    g.w("fc.weight", (64, 10), fan_in=64)
    g.b("fc.bias", 10)
    x = g.node("Gemm", [x, "fc.weight", "fc.bias"], out="output", alpha=1.0, beta=1.0, transB=0)
    graph = g.finish("input", [1, 3, IMG, IMG], x)
    graph.output_dir = str(d)
    graph.save_onnx_model("model")
    os.makedirs(os.path.join(d, "calib", "input"))
    rng = np.random.default_rng(4)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(os.path.join(d, "calib", "input", f"{i}.bin"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("fmt", ["mxfp4", "mxfp8"])
def test_shared_weights_and_skipped_nodes_stay_and_a_transposed_gemm_is_a_fixed_point_along_axis_0(tmp_path, fmt):
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform import gptq
    d = str(tmp_path)
    _build(d)
    g = ONNXGraph.load(os.path.join(d, "model.onnx"))
    names = {n.output[0]: n.name for n in g.graph.node}
    for skip in ([], [names["m1_out"]]):
        args = types.SimpleNamespace(model=os.path.join(d, "model.onnx"), input_dir=os.path.join(d, "calib"), data_num=N, rank=0,
                                     local_rank=0, world_size=1, bins=2048, threshold=0.99999, deploy="ocp_fp8", act_quant="minmax",
                                     optim_transformer=False, merge="allreduce", calib_batch=32, output_dir=d, skip_layers=skip,
                                     mx=fmt, mx_gptq=True, gptq_block=64, gptq_damp=0.01)
        act, wt = tensor_calibration(g, args)
        g_new, report = gptq(g, g, act, wt, args)
        done = {e["node"]: e for e in report}
        left = {e["node"]: e["why"] for e in json.load(open(os.path.join(d, "gptq_report.json")))["left"]}
        want_left = {names["ma_out"]: "other nodes read its weight", names["mb_out"]: "other nodes read its weight"}
        if skip:
            want_left[names["m1_out"]] = "in --skip_layers"
        assert left == want_left
        assert set(done) == {names["output"]} | ({names["m1_out"]} if not skip else set())
        for e in report:
            assert e["grid"] == fmt and e["kept"] == "gptq" and e["objective_gptq"] <= e["objective_nearest"], e
        assert (done[names["output"]]["rows"], done[names["output"]]["cols"]) == (10, 64)
        for name in ["ws", "fc.bias"] + (["w1"] if skip else []):                        # left exactly as they are
            assert np.array_equal(g_new.get_initializer(name), g.get_initializer(name)), name
        for name in ["fc.weight"] + ([] if skip else ["w1"]):                             # [K, N]: blocks along axis 0
            w0, w1 = g.get_initializer(name), np.asarray(g_new.get_initializer(name), np.float32)
            assert w1.shape == w0.shape
            assert np.array_equal(_bits(M.fake_quant_mx(w1, 0, fmt)), _bits(w1)), name
            assert not np.array_equal(_bits(M.fake_quant_mx(w0, 0, fmt)), _bits(w1)), name
