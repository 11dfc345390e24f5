"""GPU: `--mx_mixed` through the CLI on the mini-ViT of tests/test_mx_verify_e2e.py (patch 8, dim 64, depth 2, heads 2, mlp 128; 16
images), under DPL_DETERMINISTIC=1, every run under its own timeout.

One block's fc2 weight has planted outliers: four of its 128 input rows, one in every MX block along K, scaled by 64 — each block's
shared exponent is then the outlier's, and what E2M1 keeps of the other 31 rows is nothing.  That this weight's mxfp4 Q/DQ error
exceeds every other candidate's by a wide margin is first checked on the CPU with mx_model alone.

`--mx mxfp4 --mx_mixed 5.5 --mx_pack --mx_verify`: the report's formats are choose() of the report's own errors, within the budget,
mxfp8 better than mxfp4 on every candidate, the planted node promoted; quant_model.onnx, ocp_mx_weights.json (the per-tensor format,
the code bytes Kp resp. Kp / 2 a row) and ocp_mx_blocks.json agree with the report; --mx_verify holds every node to its own format's
bound.  `--mx_mixed 4` writes the model and the packed weights of the run without the flag, byte for byte; `--mx_mixed 8` promotes
every candidate; with `--mx_gptq` both grids are rounded on, each weight a fixed point of its own node.  The logits' cosine against
fp32 for uniform mxfp4, the mixed choice and uniform mxfp8 is printed (-s), not asserted.  Two ranks that share the images end with
one choice, the one-rank run's."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import mx_mixed_model as X
import mx_model as M

pytestmark = [pytest.mark.gpu, pytest.mark.two_forwards]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, IMG = 16, 32
PLANTED = "blocks.1.mlp.fc2.weight"
PLANTED_ROWS = (3, 40, 77, 114)            # one in each of the four MX blocks along K = 128
BITS = 5.5
ELEM_TYPE = {"mxfp4": "float4e2m1", "mxfp8": "float8e4m3fn"}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    from dipoorlet_amd.weight_transform.utils import update_weight
    d = tmp_path_factory.mktemp("mxmixed")
    g = models.vit(image=IMG, patch=8, dim=64, depth=2, heads=2, mlp=128, num_classes=10)     # 17 tokens, head dimension 32
    w = np.array(g.get_initializer(PLANTED), np.float32)
    assert w.shape == (128, 64)
    w[list(PLANTED_ROWS)] *= 64.0
    update_weight(g, w, PLANTED)
    g.update_model()
    g.output_dir = str(d)
    g.save_onnx_model("vit")
    os.makedirs(d / "calib" / "input")
    rng = np.random.default_rng(12)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(d / "calib" / "input" / f"{i}.bin")
    return d


def _cli(workdir, out, extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["DPL_DETERMINISTIC"] = "1"
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "vit.onnx"), "-I", str(workdir / "calib"),
           "-N", str(N), "-A", "hist", "-D", "ocp_fp8", "-O", str(out), "--calib_batch", "8", *extra]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _candidates(graph):
    """(node, weight name, block axis) of every MatMul / Gemm with a constant 2-D right operand, in graph order."""
    out = []
    for n in graph.graph.node:
        if n.op_type in ("MatMul", "Gemm") and n.input[1] in graph.initializer and np.asarray(graph.get_initializer(n.input[1])).ndim == 2:
            out.append((n, n.input[1], 1 if n.op_type == "Gemm" and n.attrs.get("transB", 0) else 0))
    return out


def _entries(rep):
    return [(name, v["err"]["mxfp4"], v["err"]["mxfp8"], v["elements"]) for name, v in rep["nodes"].items()]


def _logit_cosine(workdir, out, args):
    """Cosine of the fake-quantised network's logits against the fp32 network's over the calibration images (under `out`'s ranges)."""
    import torch

    from dipoorlet_amd.forward_net import load_input_batch
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.quantize import quant_graph
    from dipoorlet_amd.utils import load_clip_val
    args.output_dir = str(out)
    act, wt = load_clip_val(args)
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    gq, _ = quant_graph(g, {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act, **wt}.items()}, args)
    inp = load_input_batch(str(workdir / "calib"), g.network_inputs, {"input": g.get_tensor_shape("input")}, 0, N, torch.device("cuda:0"))
    fp = g.make_session().run_named(inp, [g.network_outputs[0]])[0].double().reshape(-1)
    q = gq.make_session().run_named(inp, [gq.network_outputs[0]])[0].double().reshape(-1)
    return float((fp * q).sum() / (fp.norm() * q.norm()))


def _rank_worker(rank, world, port, model, calib, out_dir):
    """One rank of mx_mixed.mx_mixed on the un-quantised model; every rank writes down what IT chose."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), DPL_DIST_BACKEND="gloo",
                      DPL_DETERMINISTIC="1")
    import torch

    from dipoorlet_amd import dist_helper, mx_mixed
    from dipoorlet_amd.graph import ONNXGraph
    dist_helper.init_default()
    os.makedirs(out_dir, exist_ok=True)
    args = types.SimpleNamespace(input_dir=calib, data_num=N, rank=rank, local_rank=0, world_size=world, deploy="ocp_fp8", calib_batch=8,
                                 output_dir=out_dir, skip_layers=[], mx="mxfp4", mx_mixed=BITS)
    fmt = mx_mixed.mx_mixed(ONNXGraph.load(model), args)
    assert args.mx_formats == fmt
    with open(os.path.join(out_dir, f"choice.rank{rank}.json"), "w") as f:
        json.dump(fmt, f)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.fixture(scope="module")
def mixed(workdir):
    """The run every test below reads: --mx mxfp4 --mx_mixed 5.5 --mx_pack --mx_verify."""
    out = workdir / "mixed"
    log = _cli(workdir, out, ["--mx", "mxfp4", "--mx_mixed", str(BITS), "--mx_pack", "--mx_verify"])
    return out, json.load(open(out / "mx_mixed_report.json")), log


def test_the_planted_weight_is_the_worst_on_the_cpu(workdir):
    from dipoorlet_amd.graph import ONNXGraph
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    err = {}
    for _, name, axis in _candidates(g):
        w = np.asarray(g.get_initializer(name), np.float32)
        err[name] = float(((M.fake_quant_mx(w, axis, "mxfp4").astype(np.float64) - w) ** 2).mean())       # per element
    assert len(err) == 9 and PLANTED in err
    others = max(v for k, v in err.items() if k != PLANTED)
    print(f"mxfp4 Q/DQ mean squared error: planted {err[PLANTED]:.4g}, the largest other {others:.4g} ({err[PLANTED] / others:.1f} x)")
    assert err[PLANTED] > 20.0 * others


def test_report_is_choose_of_its_own_errors(workdir, mixed):
    from dipoorlet_amd.graph import ONNXGraph
    out, rep, log = mixed
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    cands = _candidates(g)
    assert rep["base"] == "mxfp4" and rep["bits"] == BITS and rep["images"] == 8
    assert list(rep["nodes"]) == [n.name for n, _, _ in cands] and len(cands) == 9
    for (node, wname, axis), (name, v) in zip(cands, rep["nodes"].items()):
        w = np.asarray(g.get_initializer(wname))
        assert (v["op"], v["weight"], v["elements"], v["k"], v["n"]) == (node.op_type, wname, w.size, w.shape[axis], w.shape[1 - axis]), name
        assert v["m"] == (8 if node.op_type == "Gemm" else 8 * 17) and v["gain"] == v["err"]["mxfp4"] - v["err"]["mxfp8"]
        print(f"{name} [{v['m']} x {v['n']} x {v['k']}]: e4 {v['err']['mxfp4']:.4e} e8 {v['err']['mxfp8']:.4e} gain / bit "
              f"{v['gain'] / (4 * v['elements']):.3e} -> {v['format']}")
        assert 0.0 <= v["err"]["mxfp8"] < v["err"]["mxfp4"] < 1.0, name
    want = X.choose(_entries(rep), BITS)
    assert {k: v["format"] for k, v in rep["nodes"].items()} == want
    assert rep["average_bits"] == pytest.approx(X.average_bits(_entries(rep), want), rel=1e-12) and 4.0 < rep["average_bits"] <= BITS
    planted = [n.name for n, wname, _ in cands if wname == PLANTED]
    assert len(planted) == 1 and rep["nodes"][planted[0]]["format"] == "mxfp8"
    # the two-activation products stay at the base format, with the reason
    two = [n.name for n in g.graph.node if n.op_type == "MatMul" and n.input[1] not in g.initializer]
    assert len(two) == 4 and rep["left"] == {n: "a product of two activations" for n in two}
    assert all(f"--mx_mixed: {n} stays at mxfp4" in log for n in two)


def test_every_file_agrees_with_the_report(workdir, mixed):
    from dipoorlet_amd import onnx_io
    out, rep, _ = mixed
    fmt = {k: v["format"] for k, v in rep["nodes"].items()}
    model = onnx_io.load_model(str(out / "quant_model.onnx"))
    elem = {n.output[0]: (n.attrs["elem_type"], n.input[0]) for n in model.nodes if n.op_type == "MXQuantizeDequantize"}
    blocks = json.load(open(out / "ocp_mx_blocks.json"))
    meta = json.load(open(out / "ocp_mx_weights.json"))
    assert blocks["format"] == meta["format"] == "mixed" and set(meta["tensors"]) == {k for k, v in blocks["tensors"].items() if v["constant"]}
    seen = 0
    for n in model.nodes:
        if n.op_type not in ("MatMul", "Gemm") or n.input[0] not in elem:
            continue
        want = fmt.get(n.name, "mxfp4")
        assert [elem[i][0] for i in n.input[:2]] == [ELEM_TYPE[want]] * 2, n.name
        seen += 1
        if n.name in fmt:
            key = [k for k, t in meta["tensors"].items() if t["initializer"] == rep["nodes"][n.name]["weight"]]
            assert len(key) == 1
            t = meta["tensors"][key[0]]
            per_row = t["k_padded"] if want == "mxfp8" else t["k_padded"] // 2
            assert t["format"] == want == blocks["tensors"][key[0]]["format"], n.name
            assert t["codes"]["shape"] == [rep["nodes"][n.name]["n"], per_row] and t["codes"]["nbytes"] == rep["nodes"][n.name]["n"] * per_row
            assert t["scales"]["shape"] == [rep["nodes"][n.name]["n"], t["k_padded"] // 32]
    assert seen == 13 and len(meta["tensors"]) == 9
    # every entry of ocp_mx_blocks.json names the format of its node in the model
    by_tensor = {}
    for o, (e, t) in elem.items():
        by_tensor.setdefault(t, set()).add(e)
    assert all("format" in v for v in blocks["tensors"].values()) and len(blocks["tensors"]) == len(elem)
    for key, v in blocks["tensors"].items():
        assert any(key == t or key.startswith(t + "_ax") for t, es in by_tensor.items() if ELEM_TYPE[v["format"]] in es), key
    # --mx_verify: every node within its OWN format's bound
    verify = json.load(open(out / "mx_verify_report.json"))
    assert verify["format"] == "mixed" and verify["skipped"] == {} and len(verify["nodes"]) == 13
    for name, v in verify["nodes"].items():
        assert v["format"] == fmt.get(name, "mxfp4") and v["within_bound"] is True and v["max_err_over_bound"] <= 1.0, (name, v)
    assert {v["format"] for v in verify["nodes"].values()} == {"mxfp4", "mxfp8"}


def test_four_bits_is_the_run_without_the_flag(workdir):
    plain, four = workdir / "plain", workdir / "four"
    _cli(workdir, plain, ["--mx", "mxfp4", "--mx_pack"])
    _cli(workdir, four, ["--mx", "mxfp4", "--mx_mixed", "4", "--mx_pack"])
    rep = json.load(open(four / "mx_mixed_report.json"))
    assert {v["format"] for v in rep["nodes"].values()} == {"mxfp4"} and rep["average_bits"] == 4.0
    for f in ("quant_model.onnx", "ocp_mx_weights.bin"):
        assert open(plain / f, "rb").read() == open(four / f, "rb").read(), f
    assert not os.path.exists(plain / "mx_mixed_report.json")
    assert json.load(open(plain / "ocp_mx_blocks.json"))["format"] == "mxfp4" and "format" not in next(iter(json.load(open(plain / "ocp_mx_blocks.json"))["tensors"].values()))


def test_eight_bits_promotes_every_candidate(workdir, mixed):
    eight = workdir / "eight"
    _cli(workdir, eight, ["--mx", "mxfp4", "--mx_mixed", "8", "--skip_profiling"])
    rep = json.load(open(eight / "mx_mixed_report.json"))
    assert {v["format"] for v in rep["nodes"].values()} == {"mxfp8"} and rep["average_bits"] == 8.0 and len(rep["nodes"]) == 9
    # the measurement does not depend on the budget: the same errors, bit for bit
    assert {k: v["err"] for k, v in rep["nodes"].items()} == {k: v["err"] for k, v in mixed[1]["nodes"].items()}
    # uniform mxfp4, the mixed choice, uniform mxfp8: the logits against fp32 (printed, not asserted)
    uniform8 = workdir / "uniform8"
    _cli(workdir, uniform8, ["--mx", "mxfp8", "--skip_profiling"])
    ns = lambda **kw: types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], **kw)       # noqa: E731
    cos = {"uniform mxfp4": _logit_cosine(workdir, mixed[0], ns(mx="mxfp4")),
           f"--mx_mixed {BITS}": _logit_cosine(workdir, mixed[0], ns(mx="mxfp4", mx_formats={k: v["format"] for k, v in mixed[1]["nodes"].items()})),
           "--mx_mixed 8": _logit_cosine(workdir, eight, ns(mx="mxfp4", mx_formats={k: "mxfp8" for k in rep["nodes"]})),
           "uniform mxfp8": _logit_cosine(workdir, uniform8, ns(mx="mxfp8"))}
    print("logits against fp32, cosine: " + ", ".join(f"{k} {v:.6f}" for k, v in cos.items()))
    assert all(np.isfinite(v) for v in cos.values())


def test_mx_gptq_rounds_each_weight_on_its_own_grid(workdir):
    import torch

    from dipoorlet_amd import ops
    from dipoorlet_amd.graph import ONNXGraph
    out = workdir / "gptq"
    _cli(workdir, out, ["--mx", "mxfp4", "--mx_mixed", str(BITS), "--mx_gptq", "--skip_profiling"])
    rep = json.load(open(out / "mx_mixed_report.json"))
    layers = {e["node"]: e for e in json.load(open(out / "gptq_report.json"))["layers"]}
    g0, g1 = ONNXGraph.load(str(workdir / "vit.onnx")), ONNXGraph.load(str(out / "gptq.onnx"))
    dev = torch.device("cuda:0")
    assert {v["format"] for v in rep["nodes"].values()} == {"mxfp4", "mxfp8"}
    for node, wname, axis in _candidates(g0):
        fmt = rep["nodes"][node.name]["format"]
        assert layers[node.name]["grid"] == fmt and layers[node.name]["kept"] == "gptq", node.name
        w1 = torch.from_numpy(np.ascontiguousarray(g1.get_initializer(wname), dtype=np.float32)).to(dev)
        assert torch.equal(ops.fake_quant_mx(w1, axis, fmt).view(torch.int32), w1.view(torch.int32)), node.name
        assert not np.array_equal(np.asarray(g0.get_initializer(wname)), np.asarray(g1.get_initializer(wname))), node.name
    assert {e["grid"] for e in layers.values()} >= {"mxfp4", "mxfp8"}


def test_two_ranks_end_with_one_choice(workdir, mixed):
    """Each of two ranks measures four of the eight images and the sums are added over the process group: both ranks choose from the
    same numbers.  Against the one-rank run only the order of the fp64 additions and the batch shape of the fp32 forward differ."""
    import torch.multiprocessing as mp
    out = workdir / "two_ranks"
    port = 29500 + os.getpid() % 200
    mp.spawn(_rank_worker, args=(2, port, str(workdir / "vit.onnx"), str(workdir / "calib"), str(out)), nprocs=2, join=True)
    c0, c1 = (json.load(open(out / f"choice.rank{r}.json")) for r in (0, 1))
    rep, one = json.load(open(out / "mx_mixed_report.json")), mixed[1]
    assert c0 == c1 == {k: v["format"] for k, v in rep["nodes"].items()} and set(c0.values()) == {"mxfp4", "mxfp8"}
    assert rep["images"] == 8 and {k: v["m"] for k, v in rep["nodes"].items()} == {k: v["m"] for k, v in one["nodes"].items()}
    for name, v in rep["nodes"].items():
        for f in ("mxfp4", "mxfp8"):
            assert v["err"][f] == pytest.approx(one["nodes"][name]["err"][f], rel=1e-3), (name, f)
    assert c0 == {k: v["format"] for k, v in one["nodes"].items()}
