"""GPU: the exported Q/DQ model — what a user deploys — executed by the ONNX definitions (tests/onnx_ref.py, through
tests/qdq_replay.py) against the device session that produced it (the fused FakeQuant nodes: k_fake_quant<PRE> / k_fake_quant_mx /
the folded weight constants).

Per case: tensor_calibration (minmax, 8 images) -> [a weight transform] -> quant_graph -> save_onnx_model -> GraphSession.  One
forward of two images that are NOT calibration images, scaled to leave the calibrated ranges, hands out every tensor; replay() walks
the file over them.  Then, per case:
  * no operator of the file is without a definition, no name of the file is unknown to the session;
  * every <t>_dq tensor — activations, and the folded weight constants — and every BlockHadamard output: bit for bit;
  * every other node inside the bound test_executor_ops_onnx.py gives its kind (op_bounds.py); the worst error per operator is printed;
  * one Conv and one Gemm / MatMul re-evaluated reading <t> instead of <t>_dq: OUTSIDE the same bound (the bound cannot hide a
    missing pair);
  * at least one activation pair with an element at the lowest code of its grid and one at the highest (counted on the
    reference's codes): the zero-point and saturation arithmetic of the file was exercised;
  * every fp32 initializer of the file is the session's constant of that name, bit for bit;
  * a second forward under the default schedule (ReLU / Add + ReLU fused into the Q/DQ kernel) that hands out only the <t>_dq
    tensors and the network outputs: bit-equal to the first.

Measured on an MI355X (torch 2.10.0+rocm7.0): every <t>_dq tensor and folded weight bit for bit in every case; Conv at most 4.85
units of 2^-24 sum |x w| (allowed 11.1), ConvTranspose 3.17, Gemm 1.61 of 218, MatMul 4.12 of 50, Add / Mul 1.0 of 27; every negative
control with ALL of its outputs outside the bound.

What these tests found: through the library's transposed convolution (F.conv_transpose2d) the ConvTranspose node — 8 -> 6, 2 x 2, stride
2, two images — was 49 to 119 units off its definition on every platform but imx (0.97: power-of-two scales leave 8 significant
bits per operand), while the file and the session agreed bit for bit around it.  Stand-alone on N(0, 1) data that call is 11.6
units off by default, 17.4 under the deterministic algorithms, 34.2 at 13 x 13, 2.5 to 2.9 on ONE image, and exactly rounded on
8-bit data: a backward-data solver, chosen by batch and shape, that spends about five bits of the operands; the hand-built cases of
test_executor_ops_onnx.py (at most 2.48) never reached it.  executor.convt_col2im — the definition as a matrix product and a
col2im — replaces it on the device for 1-D and 2-D nodes."""
import os
import types

import numpy as np
import pytest
import torch

import qdq_replay as Q

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    from dipoorlet_amd import dist_helper
    dist_helper.init_default()
    return torch.device("cuda", 0)


def _copy(clip):
    return {k: [np.copy(v[0]), np.copy(v[1])] for k, v in clip.items()}


def _workdir(d, graph):
    """graph as model.onnx in d, with 8 calibration images -> (the graph reloaded from the file, args for the library's drivers)."""
    from dipoorlet_amd.graph import ONNXGraph
    graph.output_dir = str(d)
    graph.save_onnx_model("model")
    shape = graph.get_tensor_shape("input")[1:]
    os.makedirs(os.path.join(d, "calib", "input"))
    for i, img in enumerate(Q.images(shape, Q.N_CALIB, 4)):
        img.tofile(os.path.join(d, "calib", "input", f"{i}.bin"))
    args = types.SimpleNamespace(model=os.path.join(d, "model.onnx"), input_dir=os.path.join(d, "calib"), data_num=Q.N_CALIB, rank=0,
                                 local_rank=0, world_size=1, bins=2048, threshold=0.99999, deploy=None, act_quant="minmax",
                                 optim_transformer=False, merge="allreduce", calib_batch=4, output_dir=str(d), skip_layers=[], mx=None,
                                 mx_rotate=False, smooth_alpha=0.5, gptq=False, gptq_block=128, gptq_damp=0.01, savefp=False)
    return ONNXGraph.load(args.model, str(d)), args


def _reload(args, name):
    """The model a weight transform saved, read back as the CLI reads it before it goes on (weight_transform.weight_calibration)."""
    from dipoorlet_amd.graph import ONNXGraph
    return ONNXGraph.load(os.path.join(args.output_dir, name + ".onnx"), args.output_dir)


def _replay_images(graph, dev):
    return torch.from_numpy(Q.images(graph.get_tensor_shape("input")[1:], Q.N_REPLAY, 5, Q.REPLAY_SCALE)).to(dev)


def _replay_against(session, path, x, what):
    """The file at `path` against `session` on the images x: every check of the module's docstring.  -> (results, the report)."""
    gq = session.graph
    names = list(session.input_names) + [o for n in gq.graph.node if n.name not in session._folded for o in n.output]
    first = {n: t.cpu().numpy() for n, t in zip(names, session.run_named({session.input_names[0]: x}, names))}

    def fetch(name):
        if name in first:
            return first[name]
        if name in session._folded_by_out:          # a fake-quantised weight: the constant the session folded
            return session.consts[name].cpu().numpy()
        raise KeyError(name)

    results = Q.replay(path, fetch)
    report = Q.check(results, fetch, "cuda")
    # the file's constants are the session's
    from dipoorlet_amd import onnx_io
    m = onnx_io.load_model(str(path))
    n_const = 0
    for name, arr in m.initializers.items():
        if np.asarray(arr).dtype == np.float32 and not isinstance(arr, onnx_io.Float8E4M3FNBytes):
            assert name in session.consts, f"{what}: the session has no constant {name}"
            mine = session.consts[name].cpu().numpy().reshape(np.asarray(arr).shape)
            assert Q.same_bits(mine, np.asarray(arr)), f"{what}: initializer {name} of the file is not the session's"
            n_const += 1
    # negative controls, on the host from the tensors already fetched
    controls = {}
    for ops in (("Conv",), ("Gemm", "MatMul")):
        res = next((r for r in results if r.node.op_type in ops
                    and any(p.source is not None and not p.weight and r.node.input[0] in p.node.output for p in results)), None)
        if res is not None:
            controls[res.id] = Q.negative_control(res, results, fetch, "cuda")
    # both ends of the grids
    pairs, lo, hi = Q.saturation_census(results)
    # the default schedule: only the fake-quantised activations and the outputs are handed out
    keep = [o for r in results if r.source is not None and not r.weight for o in r.node.output]
    keep += [o for o in gq.network_outputs if o not in keep]
    fused, skipped = session.fusion(keep)
    for n, t in zip(keep, session.run_named({session.input_names[0]: x}, keep)):
        assert Q.same_bits(t.cpu().numpy(), first[n]), f"{what}: {n} under the fused schedule is not the tensor of the node-by-node forward"
    report.update(nodes=len(results), unsupported=0, constants=n_const, controls=controls, pairs=pairs, at_lowest=lo, at_highest=hi,
                  fused=len(fused))
    print(f"{what}: {report['nodes']} nodes, 0 unsupported; {report['bitwise']} tensors bit for bit, {n_const} constants; worst error per "
          f"operator (units of 2^-24 sum |terms| or 2^-24 max(|ref|, 1), as op_bounds) {({k: round(v, 3) for k, v in report['worst'].items()})}; negative controls (fraction of outputs "
          f"outside the bound) {({k: round(v, 3) for k, v in controls.items()})}; {pairs} activation pairs, {lo} reach the lowest code, "
          f"{hi} the highest; {len(fused)} pairs run fused in the second forward")
    assert lo >= 1 and hi >= 1, f"{what}: saturation not reached at both ends ({lo} pairs at the lowest code, {hi} at the highest)"
    assert not report["failures"], f"{what}: " + "\n".join(report["failures"])       # (last: everything above has been looked at)
    return results, report


def _quantise_and_replay(g, act, wt, args, dev, what, name="quant_model"):
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.quantize import quant_graph
    gq, _ = quant_graph(g, _copy({**act, **wt}), args)
    gq.output_dir = args.output_dir
    path = gq.save_onnx_model(name)
    session = GraphSession(gq, device=dev)
    return _replay_against(session, path, _replay_images(g, dev), what) + (session, path)


def _platforms():
    from dipoorlet_amd.platform_settings import platform_setting_table
    return list(platform_setting_table)


@pytest.mark.parametrize("trans_b", [1, 0], ids=["transB1", "transB0"])
@pytest.mark.parametrize("deploy", _platforms())
def test_every_platform(dev, tmp_path, deploy, trans_b):
    from dipoorlet_amd.tensor_cali import tensor_calibration
    g, args = _workdir(tmp_path, Q.build_conv_net(trans_b))
    args.deploy = deploy
    act, wt = tensor_calibration(g, args)
    results, report, _, _ = _quantise_and_replay(g, act, wt, args, dev, f"{deploy} transB={trans_b}")
    ops = {r.node.op_type for r in results}
    assert {"Conv", "Gemm", "Relu", "Add", "MaxPool", "Flatten", "ConvTranspose", "DequantizeLinear"} <= ops
    assert len(report["controls"]) == 2 and report["bitwise"] >= 6


@pytest.mark.parametrize("rotate", [False, True], ids=["plain", "mx_rotate"])
@pytest.mark.parametrize("mx", ["mxfp8", "mxfp4"])
def test_mx_blocks(dev, tmp_path, mx, rotate):
    """-D ocp_fp8 --mx: both operands of the two MatMuls block-scaled, K = 48 (a full block and a short one) and K = 64; with
    --mx_rotate the K = 64 product reads a BlockHadamard output and a folded weight."""
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform import mx_rotate
    g, args = _workdir(tmp_path, Q.build_matmul_net())
    args.deploy, args.mx, args.mx_rotate = "ocp_fp8", mx, rotate
    if rotate:
        assert mx_rotate(g, args) is not g
        g = _reload(args, "rotate_model")
        assert [n.op_type for n in g.graph.node].count("BlockHadamard") == 1
    act, wt = tensor_calibration(g, args)
    results, report, _, _ = _quantise_and_replay(g, act, wt, args, dev, f"ocp_fp8 --mx {mx}{' --mx_rotate' if rotate else ''}")
    mxn = [r for r in results if r.node.op_type == "MXQuantizeDequantize"]
    assert len(mxn) == 4 and sorted(r.inputs[r.node.input[0]].shape[int(r.node.attrs["axis"])] for r in mxn) == [48, 48, 64, 64]
    assert sum(r.node.op_type == "BlockHadamard" for r in results) == int(rotate) and len(report["controls"]) == 1


def test_after_bias_correction(dev, tmp_path):
    """--bc on an asymmetric integer platform: the corrected biases are in the file and in the session, the same bits."""
    from dipoorlet_amd import onnx_io
    from dipoorlet_amd.tensor_cali import find_clip_val_minmax_weight, tensor_calibration
    from dipoorlet_amd.weight_transform import bias_correction
    g, args = _workdir(tmp_path, Q.build_conv_net(1))
    args.deploy = "snpe"
    act, wt = tensor_calibration(g, args)
    assert bias_correction(g, act, wt, args) is not g
    g_bc = _reload(args, "update_bias_model")
    wt = find_clip_val_minmax_weight(g_bc, args)
    _, _, session, path = _quantise_and_replay(g_bc, act, wt, args, dev, "snpe --bc")
    m = onnx_io.load_model(str(path))
    for b in ("c1.bias", "c2.bias", "fc.bias"):
        assert not np.array_equal(g_bc.get_initializer(b), g.get_initializer(b)), b
        assert Q.same_bits(m.initializers[b], g_bc.get_initializer(b)) and Q.same_bits(session.consts[b].cpu().numpy(), m.initializers[b]), b
    assert np.array_equal(g_bc.get_initializer("ct.bias"), g.get_initializer("ct.bias"))         # (--bc corrects Conv and Gemm)


def test_after_gptq(dev, tmp_path):
    """--gptq on trt: the rounded weights are on their pair's grid — DQ(Q(W)) of the file is the file's W, bit for bit."""
    from dipoorlet_amd import onnx_io
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform import gptq
    g, args = _workdir(tmp_path, Q.build_conv_net(1))
    args.deploy, args.gptq = "trt", True
    act, wt = tensor_calibration(g, args)
    g_new, report = gptq(g, g, act, _copy(wt), args)
    by_name = {n.name: n for n in g_new.graph.node}
    rounded = sorted(by_name[e["node"]].input[1] for e in report)
    assert rounded == ["c1.weight", "c2.weight", "fc.weight"]
    results, _, _, path = _quantise_and_replay(g_new, act, wt, args, dev, "trt --gptq")
    m = onnx_io.load_model(str(path))
    for w in rounded:
        assert not np.array_equal(g_new.get_initializer(w), g.get_initializer(w)), w
        pair = next(r for r in results if r.weight and r.source == w)
        assert Q.same_bits(pair.y[0], m.initializers[w]), f"{w}: GPTQ's weight is not a fixed point of the file's pair"
    pair = next(r for r in results if r.weight and r.source == "ct.weight")                  # (left alone: not on the grid)
    assert not Q.same_bits(pair.y[0], m.initializers["ct.weight"])


def test_after_smooth_quant(dev, tmp_path):
    """--smooth on the MatMul network (magicmind: asymmetric activations): the folded affine and weight are in the file."""
    from dipoorlet_amd.tensor_cali import tensor_calibration
    from dipoorlet_amd.weight_transform import smooth_quant
    g, args = _workdir(tmp_path, Q.build_matmul_net())
    args.deploy, args.smooth = "magicmind", True
    assert smooth_quant(g, args) is not g
    g_s = _reload(args, "smooth_model")
    assert not np.array_equal(g_s.get_initializer("fc1.weight"), g.get_initializer("fc1.weight"))
    act, wt = tensor_calibration(g_s, args)
    results, report, _, _ = _quantise_and_replay(g_s, act, wt, args, dev, "magicmind --smooth")
    assert sum(r.node.op_type == "MatMul" for r in results) == 2 and len(report["controls"]) == 1


def test_the_cli_s_quant_model(dev, tmp_path):
    """main -A hist -D trt --bc: the quant_model.onnx the CLI wrote, against a session rebuilt from the model the CLI saved
    (update_bias_model.onnx) and its act_clip_val.json / weight_clip_val.json."""
    from dipoorlet_amd.__main__ import main
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.quantize import quant_graph
    from dipoorlet_amd.utils import load_clip_val
    g, args = _workdir(tmp_path, Q.build_conv_net(1))
    out = os.path.join(tmp_path, "out")
    assert main(["-M", args.model, "-I", args.input_dir, "-N", str(Q.N_CALIB), "-A", "hist", "-D", "trt", "--bc", "-O", out,
                 "--calib_batch", "4"]) == 0
    args.deploy, args.output_dir = "trt", out
    act, wt = load_clip_val(args)                     # act_clip_val.json / weight_clip_val.json, as the CLI itself read them back
    g_bc = ONNXGraph.load(os.path.join(out, "update_bias_model.onnx"), out)
    assert not np.array_equal(g_bc.get_initializer("c1.bias"), g.get_initializer("c1.bias"))
    gq, _ = quant_graph(g_bc, {**act, **wt}, args)
    _replay_against(GraphSession(gq, device=dev), os.path.join(out, "quant_model.onnx"), _replay_images(g, dev), "the CLI, -A hist -D trt --bc")
