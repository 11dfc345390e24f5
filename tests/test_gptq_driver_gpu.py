"""GPU: the branches of the --gptq driver (weight_transform/gptq.py) a ResNet does not reach — a Gemm with transB = 0 (its weight is
[K, R]: transposed on the way in and out), and the nodes that are counted and left exactly as they are: a grouped convolution, a
ConvTranspose, a node in --skip_layers, and a transB = 0 Gemm on a platform whose per-channel scales then run along K."""
import os
import types

import numpy as np
import pytest
import torch

import gptq_model as M

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]

N, IMG = 8, 12


def _build(d, trans_b):
    """c1 (plain) -> cg (group 2) -> ct (ConvTranspose) -> c2 (plain; the tests skip it) -> pool -> fc (Gemm, transB as asked; the same
    matrix either way)."""
    from dipoorlet_amd.models import _B
    g = _B(7)
    x = g.node("Relu", [g.conv("input", 3, 8, 3, 1, 1, "c1")], out="r1")
    x = g.node("Relu", [g.conv(x, 8, 8, 3, 1, 1, "cg", groups=2)], out="r2")
    g.w("ct.weight", (8, 8, 2, 2))
    g.b("ct.bias", 8)
    x = g.node("ConvTranspose", [x, "ct.weight", "ct.bias"], out="ct_out", kernel_shape=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0],
               dilations=[1, 1], group=1)
    x = g.node("Relu", [x], out="r3")
    x = g.node("Relu", [g.conv(x, 8, 24, 1, 1, 0, "c2")], out="r4")
    x = g.node("MaxPool", [x], out="pool", ceil_mode=0, kernel_shape=[4, 4], pads=[0, 0, 0, 0], strides=[4, 4])
    x = g.node("Flatten", [x], out="flat", axis=1)                       # [N, 24 * 6 * 6]
    wfc = g.w("fc.weight", (10, 864))
    if not trans_b:
        g.const("fc.weight", np.ascontiguousarray(g.init["fc.weight"].T))
    g.b("fc.bias", 10)
    x = g.node("Gemm", [x, wfc, "fc.bias"], out="output", alpha=1.0, beta=1.0, transB=int(trans_b))
    graph = g.finish("input", [1, 3, IMG, IMG], x)
    graph.output_dir = str(d)
    graph.save_onnx_model("model")
    os.makedirs(os.path.join(d, "calib", "input"))
    rng = np.random.default_rng(4)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(os.path.join(d, "calib", "input", f"{i}.bin"))


def _run(d, deploy, trans_b, skip_outputs=("c2_out",)):
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform import gptq
    _build(d, trans_b)
    g = ONNXGraph.load(os.path.join(d, "model.onnx"))
    names = {n.output[0]: n.name for n in g.graph.node}
    args = types.SimpleNamespace(model=os.path.join(d, "model.onnx"), input_dir=os.path.join(d, "calib"), data_num=N, rank=0,
                                 local_rank=0, world_size=1, bins=2048, threshold=0.99999, deploy=deploy, act_quant="minmax",
                                 optim_transformer=False, merge="allreduce", calib_batch=4, output_dir=None,
                                 skip_layers=[names[o] for o in skip_outputs], gptq=True, gptq_block=128, gptq_damp=0.01)
    act, wt = tensor_calibration(g, args)
    wt0 = {k: [np.copy(v[0]), np.copy(v[1])] for k, v in wt.items()}
    g_new, report = gptq(g, g, act, wt, args)
    return g, g_new, {names[o]: o for o in names}, report, wt0, args


def test_left_nodes_stay_and_a_transposed_gemm_is_the_untransposed_one(tmp_path):
    """-D stpu rounds weights per tensor, so both forms of the Gemm are rounded: the same inputs, the same matrix, the same grid —
    the transB = 0 result must be the transB = 1 result transposed, bit for bit."""
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.quantize import get_qnode_by_param
    res = {}
    for tb in (1, 0):
        d = tmp_path / f"tb{tb}"
        d.mkdir()
        g, g_new, out_of, report, wt, args = _run(str(d), "stpu", tb)
        done = {out_of[e["node"]]: e for e in report}
        assert set(done) == {"c1_out", "output"}                                          # what GPTQ rounded
        for e in report:
            assert e["kept"] == "gptq" and e["objective_gptq"] <= e["objective_nearest"], e
        for name in ("cg.weight", "ct.weight", "c2.weight", "c1.bias", "fc.bias"):        # left exactly as they are
            assert np.array_equal(g_new.get_initializer(name), g.get_initializer(name)), name
        assert not np.array_equal(g_new.get_initializer("c1.weight"), g.get_initializer("c1.weight"))
        w = g_new.get_initializer("fc.weight")
        assert w.shape == ((10, 864) if tb else (864, 10))
        qnode, q_min, q_max = get_qnode_by_param(platform_setting_table["stpu"]["qw_params"], "fc.weight", list(w.shape),
                                                 [np.copy(wt["fc.weight"][0]), np.copy(wt["fc.weight"][1])])
        Q = M.make_q({"fmt": M.INT, "scale": qnode.scale, "zp": np.zeros(1, np.int32), "qlo": int(np.min(q_min)), "qhi": int(np.max(q_max))})
        assert qnode.scale.size == 1 and np.array_equal(Q(w).view(np.uint32), w.view(np.uint32))      # on the graph's grid
        assert (w != Q(g.get_initializer("fc.weight"))).sum() > 10                                     # ... and not just nearest
        res[tb] = (w, done["output"])
    assert np.array_equal(res[0][0], res[1][0].T)
    assert res[0][1]["objective_gptq"] == res[1][1]["objective_gptq"] and (res[0][1]["rows"], res[0][1]["cols"]) == (10, 864)


def test_the_log_counts_what_was_left_and_why(tmp_path):
    """-D trt rounds weights per channel along axis 0 of the initializer: for a transB = 0 Gemm that is the reduction axis, which the
    kernel's per-row scales cannot express — such a node is left, with the others, and said so."""
    import json
    d = str(tmp_path)
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform import gptq
    _build(d, 0)
    g = ONNXGraph.load(os.path.join(d, "model.onnx"))
    names = {n.output[0]: n.name for n in g.graph.node}
    args = types.SimpleNamespace(model=os.path.join(d, "model.onnx"), input_dir=os.path.join(d, "calib"), data_num=N, rank=0,
                                 local_rank=0, world_size=1, bins=2048, threshold=0.99999, deploy="trt", act_quant="minmax",
                                 optim_transformer=False, merge="allreduce", calib_batch=4, output_dir=d,
                                 skip_layers=[names["c2_out"]], gptq=True, gptq_block=128, gptq_damp=0.01)
    act, wt = tensor_calibration(g, args)
    g_new, report = gptq(g, g, act, wt, args)
    assert [e["node"] for e in report] == [names["c1_out"]] and report[0]["kept"] == "gptq"
    left = {e["node"]: e["why"] for e in json.load(open(os.path.join(d, "gptq_report.json")))["left"]}
    assert left == {names["cg_out"]: "a grouped convolution", names["ct_out"]: "a ConvTranspose", names["c2_out"]: "in --skip_layers",
                    names["output"]: "its per-channel scales do not run along the output channels"}
    for name in ("cg.weight", "ct.weight", "c2.weight", "fc.weight"):
        assert np.array_equal(g_new.get_initializer(name), g.get_initializer(name)), name
    assert os.path.exists(os.path.join(d, "gptq.onnx"))
    # the walk still ran every node: the fake-quantised network with the new c1 weight computes an output
    assert torch.cuda.is_available() and not np.array_equal(g_new.get_initializer("c1.weight"), g.get_initializer("c1.weight"))
