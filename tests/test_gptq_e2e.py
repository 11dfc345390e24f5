"""GPU: --gptq end to end on a small ResNet-18 — through the CLI from a real .onnx + .bin directory, on a 4-bit integer weight
grid (-D trt, narrowed as in test_round_e2e.py so that rounding matters) and on OCP FP8 E4M3 (-D ocp_fp8), and on two ranks.

Every Conv / Gemm weight of gptq.onnx must sit on the grid the fake-quantised graph rounds it to (Q(w) == w under the ORIGINAL
ranges), biases stay, the driver's own per-layer objective must not rise, and the fake-quantised network must reproduce the
full-precision network better than with weights rounded to nearest."""
import copy
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import gptq_model as M

# (every test here re-runs or compares library forwards: deterministic algorithms, tests/conftest.py)
pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]

N, IMG, WIDTH = 16, 32, 32


def _make_workdir(d):
    from dipoorlet_amd import models
    g = models.resnet18(seed=3, image=IMG, width=WIDTH)
    g.output_dir = str(d)
    g.save_onnx_model("model")
    os.makedirs(os.path.join(d, "calib", "input"))
    rng = np.random.default_rng(9)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(os.path.join(d, "calib", "input", f"{i}.bin"))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("gptq")
    _make_workdir(str(d))
    return d


@pytest.fixture()
def four_bit_weights():
    from dipoorlet_amd.platform_settings import platform_setting_table
    saved = copy.deepcopy(platform_setting_table["trt"])
    platform_setting_table["trt"]["qw_params"]["bit_width"] = 4
    yield
    platform_setting_table["trt"].clear()
    platform_setting_table["trt"].update(saved)


def _cli(workdir, out, deploy, extra):
    from dipoorlet_amd.__main__ import main
    return main(["-M", str(workdir / "model.onnx"), "-I", str(workdir / "calib"), "-N", str(N), "-A", "minmax", "-D", deploy,
                 "-O", str(out), "--calib_batch", "8", "--skip_profiling", *extra])


def _network_error(model_path, workdir, act_clip, weight_clip, args):
    """Mean squared error of the fake-quantised network's output against the full-precision network's (original ranges)."""
    from dipoorlet_amd.forward_net import load_input_batch
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.quantize import quant_graph
    g_fp = ONNXGraph.load(str(workdir / "model.onnx"))
    g = ONNXGraph.load(model_path)
    clip = {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act_clip, **weight_clip}.items()}
    gq, _ = quant_graph(g, clip, args)
    dev = torch.device("cuda:0")
    inp = load_input_batch(str(workdir / "calib"), g_fp.network_inputs, {"input": g_fp.get_tensor_shape("input")}, 0, N, dev)
    fp = g_fp.make_session().run_named(inp, [g_fp.network_outputs[0]])[0]
    q = gq.make_session().run_named(inp, [gq.network_outputs[0]])[0]
    return float(((fp - q) ** 2).mean())


def _check_weights(model_path, workdir, weight_clip, deploy):
    """Q(w) == w bit for bit on the grid of the original ranges, for every Conv / Gemm weight; biases untouched.  -> the number of
    weights that differ from round-to-nearest."""
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.quantize import FP8_E4M3, get_qnode_by_param
    g0, g1 = ONNXGraph.load(str(workdir / "model.onnx")), ONNXGraph.load(model_path)
    moved = layers = 0
    for node in g0.graph.node:
        if node.op_type not in ("Conv", "Gemm"):
            continue
        name = node.input[1]
        w0, w1 = g0.get_initializer(name), g1.get_initializer(name)
        rng = [np.copy(weight_clip[name][0]), np.copy(weight_clip[name][1])]
        qnode, q_min, q_max = get_qnode_by_param(platform_setting_table[deploy]["qw_params"], name, list(w0.shape), rng)
        assert qnode.scale.size == w0.shape[0]                               # both platforms: per output channel
        if qnode.fmt == FP8_E4M3:
            Q = M.make_q({"fmt": M.E4M3, "scale": qnode.scale})
        else:
            Q = M.make_q({"fmt": M.INT, "scale": qnode.scale, "zp": np.zeros(qnode.scale.size, np.int32),
                          "qlo": int(np.min(q_min)), "qhi": int(np.max(q_max))})
        w1_2d, w0_2d = w1.reshape(w1.shape[0], -1).astype(np.float32), w0.reshape(w0.shape[0], -1).astype(np.float32)
        assert np.array_equal(Q(w1_2d).view(np.uint32), w1_2d.view(np.uint32)), node.name
        moved += int((w1_2d != Q(w0_2d)).sum())
        layers += 1
        if len(node.input) > 2:
            assert np.array_equal(g0.get_initializer(node.input[2]), g1.get_initializer(node.input[2])), node.name
    assert layers == 21
    return moved


def _run_and_check(workdir, out, deploy, deploy_file):
    from dipoorlet_amd.utils import load_clip_val
    assert _cli(workdir, out, deploy, ["--gptq"]) == 0
    assert os.path.exists(out / "gptq.onnx") and os.path.exists(out / deploy_file)
    args = types.SimpleNamespace(deploy=deploy, skip_layers=[], output_dir=str(out))
    act, wt = load_clip_val(args)
    moved = _check_weights(str(out / "gptq.onnx"), workdir, wt, deploy)
    assert moved > 100           # it did not just reproduce round-to-nearest
    report = json.load(open(out / "gptq_report.json"))
    assert len(report["layers"]) == 21 and report["left"] == []
    for e in report["layers"]:           # every layer: GPTQ's weights were written, and its own objective did not rise
        assert e["kept"] == "gptq" and e["objective_gptq"] <= e["objective_nearest"], e
    err_nearest = _network_error(str(workdir / "model.onnx"), workdir, act, wt, args)
    err_gptq = _network_error(str(out / "gptq.onnx"), workdir, act, wt, args)
    print(f"-D {deploy}: gptq / nearest output error: {err_gptq / err_nearest:.4f} ({moved} weights moved; layer objectives "
          f"gptq / nearest: {sum(e['objective_gptq'] for e in report['layers']) / sum(e['objective_nearest'] for e in report['layers']):.4f})")
    assert err_gptq < 1.0 * err_nearest, (err_gptq, err_nearest)


def test_gptq_cli_on_a_four_bit_integer_grid(workdir, four_bit_weights):
    _run_and_check(workdir, workdir / "out_int4", "trt", "trt_clip_val.json")


def test_gptq_cli_on_the_fp8_grid(workdir):
    _run_and_check(workdir, workdir / "out_fp8", "ocp_fp8", "ocp_fp8_scales.json")


@pytest.mark.parametrize("deploy,extra", [("trt", ["--gptq", "--adaround"]), ("ocp_fp8", ["--gptq", "--mx", "mxfp4"])])
def test_refused_combinations_stop_before_the_output_directory_exists(workdir, deploy, extra):
    out = workdir / ("refused_" + deploy)
    with pytest.raises(ValueError) as e:           # (python -m dipoorlet_amd exits non-zero with this error)
        _cli(workdir, out, deploy, extra)
    assert all(flag in str(e.value) for flag in extra if flag.startswith("--"))
    assert not os.path.exists(out)


def _worker(rank, world, port, wd):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      DPL_DIST_BACKEND="gloo")
    from dipoorlet_amd import dist_helper
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform import gptq
    platform_setting_table["trt"]["qw_params"]["bit_width"] = 4
    dist_helper.init_default()
    args = types.SimpleNamespace(model=os.path.join(wd, "model.onnx"), input_dir=os.path.join(wd, "calib"), data_num=N,
                                 rank=rank, local_rank=0, world_size=world, bins=2048, threshold=0.99999, deploy="trt",
                                 act_quant="minmax", optim_transformer=False, merge="allreduce", calib_batch=4,
                                 output_dir=os.path.join(wd, "out2"), skip_layers=[], gptq=True, gptq_block=128, gptq_damp=0.01)
    os.makedirs(args.output_dir, exist_ok=True)
    g = ONNXGraph.load(args.model, args.output_dir, "trt")
    act, wt = tensor_calibration(g, args)
    g_gptq, report = gptq(g, g, act, wt, args)
    np.savez(os.path.join(wd, f"weights{rank}.npz"), **{k: v for k, v in g_gptq.initializer.items() if v.ndim >= 2})
    assert len(report) == 21 and all(e["kept"] == "gptq" and e["objective_gptq"] <= e["objective_nearest"] for e in report), report
    np.save(os.path.join(wd, f"objective{rank}.npy"), np.array([e["objective_gptq"] for e in report]))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_end_with_the_same_weights(tmp_path):
    from dipoorlet_amd.graph import ONNXGraph
    _make_workdir(str(tmp_path))
    port = 29800 + os.getpid() % 90
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / "weights0.npz"), np.load(tmp_path / "weights1.npz")
    assert len(a.files) >= 21
    for k in a.files:       # identical models: the Hessians were summed over the ranks, not rank-local
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(np.load(tmp_path / "objective0.npy"), np.load(tmp_path / "objective1.npy"))
    assert os.path.exists(tmp_path / "out2" / "gptq.onnx")
    g0 = ONNXGraph.load(str(tmp_path / "model.onnx"))
    assert len(a.files) == 21 and all(not np.array_equal(a[k], g0.get_initializer(k)) for k in a.files)     # ... GPTQ's, every one
