"""GPU: `--mx_conv` through the CLI on a small ResNet-18 (width 24, 64 x 64 images: 20 Convs with C = 3, 24, 48, 96, 192, and the
Gemm), under DPL_DETERMINISTIC=1, with --mx_pack --mx_verify: mx_verify_report.json lists all 21 nodes, none skipped — every Conv
multiplied as bytes on the block-scaled matrix instruction (ops.mx_conv), its weight read back from ocp_mx_weights.bin as [cout, kh,
kw, ...] sections — each within the bound and at cosine >= 1 - 1e-6; ocp_mx_blocks.json lists the 20 Convs and leaves none; and
quant_model.onnx replays against the session that produced it (tests/qdq_replay.py; the weight nodes
that carry searched scale bytes against tests/mx_scale_model.py).  Without --mx_conv the same command verifies
the Gemm alone."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mx_scale_model as S
import qdq_replay as Q

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, IMG = 16, 64
REPORT = "mx_verify_report.json"
CONFIGS = {"mxfp4": ["--mx", "mxfp4"], "mxfp8_search_bc": ["--mx", "mxfp8", "--mx_scale_search", "--bc"]}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mxconv")
    g = models.resnet18(width=24, image=IMG, num_classes=10)
    g.output_dir = str(d)
    g.save_onnx_model("resnet")
    os.makedirs(d / "calib" / "input")
    rng = np.random.default_rng(14)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(d / "calib" / "input" / f"{i}.bin")
    return d


def _cli(workdir, out, extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["DPL_DETERMINISTIC"] = "1"
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "resnet.onnx"), "-I", str(workdir / "calib"),
           "-N", str(N), "-A", "hist", "-D", "ocp_fp8", "-O", str(out), "--calib_batch", "8", *extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _replay(out, workdir, config):
    """quant_model.onnx of the run against a session rebuilt from the model the run saved and its clip values: every
    MXQuantizeDequantize output bit for bit, every other node inside its kind's bound (qdq_replay.check)."""
    from dipoorlet_amd import dist_helper
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.quantize import quant_graph
    from dipoorlet_amd.utils import load_clip_val
    dist_helper.init_default()
    dev = torch.device("cuda", 0)
    args = types.SimpleNamespace(deploy="ocp_fp8", output_dir=str(out), skip_layers=[], mx=CONFIGS[config][1], mx_conv=True,
                                 mx_scale_search="--mx_scale_search" in CONFIGS[config])
    saved = out / "update_bias_model.onnx"
    g = ONNXGraph.load(str(saved if "--bc" in CONFIGS[config] else workdir / "resnet.onnx"), str(out))
    act, wt = load_clip_val(args)
    gq, _ = quant_graph(g, {**act, **wt}, args)
    session = GraphSession(gq, device=dev)
    x = torch.from_numpy(Q.images(g.get_tensor_shape("input")[1:], Q.N_REPLAY, 5, Q.REPLAY_SCALE)).to(dev)
    names = list(session.input_names) + [o for n in gq.graph.node if n.name not in session._folded for o in n.output]
    first = {n: t.cpu().numpy() for n, t in zip(names, session.run_named({session.input_names[0]: x}, names))}

    def fetch(name):
        if name in first:
            return first[name]
        if name in session._folded_by_out:
            return session.consts[name].cpu().numpy()
        raise KeyError(name)

    results = Q.replay(out / "quant_model.onnx", fetch)
    mx = [r for r in results if r.node.op_type == "MXQuantizeDequantize"]
    # qdq_replay's definition of MXQuantizeDequantize is the one-input node (the floor rule).  A weight's node that carries searched
    # E8M0 bytes as its second input (--mx_scale_search) is held to tests/mx_scale_model.py under those bytes instead, bit for bit.
    searched = [r for r in mx if len(r.node.input) > 1 and r.node.input[1] != ""]
    assert len(searched) == (21 if args.mx_scale_search else 0)
    for r in searched:
        x, bytes_ = r.inputs[r.node.input[0]], r.inputs[r.node.input[1]]
        assert np.asarray(bytes_).dtype == np.uint8
        want = S.fake_quant_mx_scaled(x, int(r.node.attrs["axis"]), args.mx, bytes_)
        assert Q.same_bits(fetch(r.node.output[0]), want), r.node.name
    report = Q.check([r for r in results if not any(r is q for q in searched)], fetch, "cuda")
    print(f"{config}: replayed {len(results)} nodes, {report['bitwise']} + {len(searched)} tensors bit for bit, worst per operator {report['worst']}")
    assert not report["failures"], "\n".join(report["failures"])
    return results, mx


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_cli_block_scales_and_verifies_every_conv(workdir, config):
    elem = CONFIGS[config][1]
    out = workdir / (config + "_conv")
    _cli(workdir, out, CONFIGS[config] + ["--mx_conv", "--mx_pack", "--mx_verify"])
    rep = json.load(open(out / REPORT))
    meta = json.load(open(out / "ocp_mx_weights.json"))
    blocks = json.load(open(out / "ocp_mx_blocks.json"))
    assert rep["format"] == elem and rep["images"] == 8 and rep["skipped"] == {}
    convs = {k: v for k, v in rep["nodes"].items() if v["op"] == "Conv"}
    assert len(rep["nodes"]) == 21 and len(convs) == 20 and [v["op"] for v in rep["nodes"].values()].count("Gemm") == 1
    assert sorted(blocks["conv"]["nodes"]) == sorted(convs) and blocks["conv"]["left"] == {}
    worst = 0.0
    for name, v in rep["nodes"].items():
        t = meta["tensors"][v["constant"]]
        if v["op"] == "Conv":
            kh, kw = v["kernel"]
            cb = -(-v["c"] // 32)
            assert t["shape"] == [v["cout"], v["c"], kh, kw] and t["axis"] == 1 and t["k"] == v["c"] and v["k"] == kh * kw * v["c"]
            assert t["codes"]["shape"] == [v["cout"], kh, kw, cb * (32 if elem == "mxfp8" else 16)] and t["scales"]["shape"] == [v["cout"], kh, kw, cb]
            assert v["n"] == 8 and len(v["strides"]) == 2 and len(v["pads"]) == 4
            print(f"{config} {name}: [{v['n']} x {v['c']} x {v['h']} x {v['w']}] * [{v['cout']} x {kh} x {kw}] s {v['strides']} p {v['pads']}: max |err| "
                  f"{v['max_abs_err']:.3e}, {v['max_err_over_bound']:.4g} of the bound, 1 - cosine {1 - v['cosine']:.2e}")
        assert v["within_bound"] is True and v["max_err_over_bound"] <= 1.0 and v["cosine"] >= 1 - 1e-6, (name, v)
        worst = max(worst, v["max_err_over_bound"])
    print(f"{config}: worst max_err_over_bound {worst:.4g}")
    assert {v["c"] for v in convs.values()} >= {3, 24, 48, 96, 192}
    assert {tuple(v["kernel"]) for v in convs.values()} == {(7, 7), (3, 3), (1, 1)} and {tuple(v["strides"]) for v in convs.values()} == {(1, 1), (2, 2)}
    # the saved Q/DQ model: every Conv reads two MXQuantizeDequantize outputs along axis 1, and the file replays against the session
    results, mx = _replay(out, workdir, config)
    mx_out = {r.node.output[0]: r.node for r in mx}
    conv_nodes = [r.node for r in results if r.node.op_type == "Conv"]
    assert len(conv_nodes) == 20 and all(n.input[0] in mx_out and n.input[1] in mx_out for n in conv_nodes)
    assert all(int(mx_out[n.input[i]].attrs["axis"]) == 1 for n in conv_nodes for i in (0, 1))
    if config == "mxfp4":         # without --mx_conv: the Gemm alone, and no "conv" entry
        plain = workdir / (config + "_plain")
        _cli(workdir, plain, CONFIGS[config] + ["--mx_pack", "--mx_verify"])
        rep = json.load(open(plain / REPORT))
        assert [v["op"] for v in rep["nodes"].values()] == ["Gemm"] and rep["skipped"] == {}
        assert "conv" not in json.load(open(plain / "ocp_mx_blocks.json"))
