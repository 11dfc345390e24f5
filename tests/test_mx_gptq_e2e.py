"""GPU: --mx_gptq end to end through the CLI on the tiny ViT of test_mx_pack_e2e.py (patch 8, dim 64, depth 2, heads 2, mlp 128;
32 images), once per element format, together with --mx_pack and --mx_verify.

gptq.onnx must hold, for every constant-weight MatMul and the head Gemm, a weight that the graph's own MX node leaves unchanged
(mx_model.fake_quant_mx(w) == w bit for bit) and that is not round-to-nearest of the original; the patch Conv goes through --gptq's
path on its static E4M3 grid; the products of two activations are left, with the reason.  The driver's per-layer objective must not
rise, and must fall in total.  What --mx_pack writes decodes to the very initializers, and --mx_verify finds every product within
its bound."""
import json
import os
import types

import numpy as np
import pytest
import torch

import mx_model as M

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]

N, IMG = 32, 32
FORMATS = ("mxfp4", "mxfp8")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mxgptq")
    g = models.vit(image=IMG, patch=8, dim=64, depth=2, heads=2, mlp=128, num_classes=10)     # 17 tokens, head dimension 32
    g.output_dir = str(d)
    g.save_onnx_model("vit")
    os.makedirs(d / "calib" / "input")
    rng = np.random.default_rng(12)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(d / "calib" / "input" / f"{i}.bin")
    return d


def _cli(workdir, out, extra):
    from dipoorlet_amd.__main__ import main
    return main(["-M", str(workdir / "vit.onnx"), "-I", str(workdir / "calib"), "-N", str(N), "-A", "hist", "-D", "ocp_fp8",
                 "-O", str(out), "--calib_batch", "16", "--skip_profiling", *extra])


def _network_error(model_path, workdir, act_clip, weight_clip, args):
    """Mean squared error of the fake-quantised network's output against the full-precision network's (test_gptq_e2e.py's method)."""
    from dipoorlet_amd.forward_net import load_input_batch
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.quantize import quant_graph
    g_fp = ONNXGraph.load(str(workdir / "vit.onnx"))
    g = ONNXGraph.load(model_path)
    clip = {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act_clip, **weight_clip}.items()}
    gq, _ = quant_graph(g, clip, args)
    dev = torch.device("cuda:0")
    inp = load_input_batch(str(workdir / "calib"), g_fp.network_inputs, {"input": g_fp.get_tensor_shape("input")}, 0, N, dev)
    fp = g_fp.make_session().run_named(inp, [g_fp.network_outputs[0]])[0]
    q = gq.make_session().run_named(inp, [gq.network_outputs[0]])[0]
    return float(((fp - q) ** 2).mean())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("fmt", FORMATS)
def test_mx_gptq_cli(workdir, fmt):
    from dipoorlet_amd import ops
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.utils import load_clip_val
    out = workdir / ("out_" + fmt)
    assert _cli(workdir, out, ["--mx", fmt, "--mx_gptq", "--mx_pack", "--mx_verify"]) == 0
    assert os.path.exists(out / "gptq.onnx") and os.path.exists(out / "gptq_report.json")
    g0, g1 = ONNXGraph.load(str(workdir / "vit.onnx")), ONNXGraph.load(str(out / "gptq.onnx"))
    report = json.load(open(out / "gptq_report.json"))
    by_node = {e["node"]: e for e in report["layers"]}
    left = {e["node"]: e["why"] for e in report["left"]}
    weights = {}                                                       # initializer -> (block axis | None, node)
    for node in g0.graph.node:
        if node.op_type == "Conv":
            assert by_node[node.name]["grid"] == "e4m3" and by_node[node.name]["kept"] == "gptq", node.name
            weights[node.input[1]] = (None, node)
        elif node.op_type == "Gemm":
            assert by_node[node.name]["grid"] == fmt and by_node[node.name]["kept"] == "gptq", node.name
            weights[node.input[1]] = (1, node)                         # transB = 1: [N, K]
        elif node.op_type == "MatMul":
            if node.input[1] in g0.initializer:
                assert by_node[node.name]["grid"] == fmt and by_node[node.name]["kept"] == "gptq", node.name
                weights[node.input[1]] = (0, node)                     # [K, N]
            else:
                assert node.name not in by_node and left[node.name] == "a MatMul with two activation operands", node.name
    assert len(by_node) == len(weights) == 10 and len(left) == 4
    for e in report["layers"]:
        assert e["objective_gptq"] <= e["objective_nearest"], e
    o_gptq, o_near = (sum(e[k] for e in report["layers"]) for k in ("objective_gptq", "objective_nearest"))
    assert o_gptq < o_near
    # the weights: fixed points of the graph's own node, not round-to-nearest; everything else as it was
    for name, (axis, node) in weights.items():
        w0, w1 = np.asarray(g0.get_initializer(name), np.float32), np.asarray(g1.get_initializer(name), np.float32)
        assert w0.shape == w1.shape
        if axis is None:
            assert not np.array_equal(w0, w1), name
            continue
        assert np.array_equal(_bits(M.fake_quant_mx(w1, axis, fmt)), _bits(w1)), name
        assert not np.array_equal(_bits(M.fake_quant_mx(w0, axis, fmt)), _bits(w1)), name
    for name, v in g0.initializer.items():
        if name not in weights:
            assert np.array_equal(np.asarray(v), np.asarray(g1.get_initializer(name))), name      # biases, LayerNorm affines, ...
    # --mx_pack wrote these very weights, --mx_verify multiplied them
    meta = json.load(open(out / "ocp_mx_weights.json"))
    blob = np.fromfile(out / "ocp_mx_weights.bin", dtype=np.uint8)
    dev = torch.device("cuda:0")
    assert {t["initializer"] for t in meta["tensors"].values()} == {n for n, (a, _) in weights.items() if a is not None}
    for t in meta["tensors"].values():
        w1 = np.asarray(g1.get_initializer(t["initializer"]), np.float32)
        sec = [torch.from_numpy(blob[t[p]["offset"]:t[p]["offset"] + t[p]["nbytes"]].reshape(t[p]["shape"]).copy()).to(dev) for p in ("codes", "scales")]
        got = ops.mx_decode(sec[0], sec[1], fmt, w1.shape, t["axis"]).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(w1)), t["initializer"]
    verify = json.load(open(out / "mx_verify_report.json"))
    assert verify["skipped"] == {} and len(verify["nodes"]) == 13 and all(v["within_bound"] for v in verify["nodes"].values())
    assert {n.name for _, n in weights.values() if n.op_type != "Conv"} <= set(verify["nodes"])
    # the network's output against fp32, GPTQ's weights versus round-to-nearest, under the same ranges
    args = types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], output_dir=str(out), mx=fmt)
    act, wt = load_clip_val(args)
    err_nearest = _network_error(str(workdir / "vit.onnx"), workdir, act, wt, args)
    err_gptq = _network_error(str(out / "gptq.onnx"), workdir, act, wt, args)
    print(f"--mx {fmt} --mx_gptq: output MSE gptq {err_gptq:.6g} / nearest {err_nearest:.6g} = {err_gptq / err_nearest:.4f}; "
          f"layer objectives gptq / nearest = {o_gptq / o_near:.4f}")
    assert np.isfinite(err_gptq) and np.isfinite(err_nearest)
    if fmt == "mxfp4":          # measured on this model: 0.830 for mxfp4 (0.761 for mxfp8: printed, not asserted) — DESIGN §3q
        assert err_gptq < err_nearest, (err_gptq, err_nearest)


@pytest.mark.parametrize("extra", [["--mx_gptq"], ["--mx", "mxfp4", "--mx_gptq", "--gptq"], ["--mx", "mxfp4", "--mx_gptq", "--mx_scale_search"],
                                   ["--mx", "mxfp8", "--mx_gptq", "--gptq_block", "48"]], ids=lambda e: "_".join(a.strip("-") for a in e))
def test_refused_combinations_stop_before_the_output_directory_exists(workdir, extra):
    out = workdir / "refused"
    with pytest.raises(ValueError) as e:           # (python -m dipoorlet_amd exits non-zero with this error)
        _cli(workdir, out, extra)
    assert "--mx_gptq" in str(e.value)
    assert not os.path.exists(out)
