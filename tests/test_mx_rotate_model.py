"""No GPU: `--mx_rotate` — the numpy definition (tests/mx_rotate_model.py) against integer arithmetic, the site finder and the host
fold of weight_transform/rotate.py, the graph round trip, the shape rule, the CLI's checks, the ABI, and the direction of the MX
product error on the model (the table of DESIGN section 3l is what `test_error_direction_on_the_model` prints)."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import mx_rotate_model as R
from dipoorlet_amd import _hip, onnx_io, shape_infer
from dipoorlet_amd.__main__ import build_parser, check_args
from dipoorlet_amd.graph import MX_DOMAIN, ONNXGraph
from dipoorlet_amd.onnx_io import Node
from dipoorlet_amd.weight_transform.rotate import apply_rotate, find_rotate_sites, fold_weight_host, mx_rotate, rotate_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the model on small integers
def test_model_on_small_integers_is_exact():
    rng = np.random.default_rng(0)
    H = R.h32()
    assert np.array_equal(H, H.T) and np.array_equal(H @ H, 32 * np.eye(32, dtype=np.int64))
    for shape in ((1, 32), (5, 96), (3, 2, 64)):
        x = rng.integers(-8, 9, shape)
        want = (x.reshape(-1, 32) @ H).reshape(shape)                      # int64
        got = R.fwht32(x.astype(np.float32))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))
        assert np.array_equal(R.fwht32(got), (32 * x).astype(np.float32))
    with pytest.raises(ValueError):
        R.fwht32(np.zeros((2, 48), np.float32))


def test_special_values_spread_over_their_block_only():
    x = np.ones((3, 64), np.float32)
    x[0, 5] = np.nan
    x[1, 40], x[1, 41] = np.inf, -np.inf
    x[2, :32] = 0.0
    x[2, 1:32:2] = -0.0
    y = R.fwht32(x)
    assert np.isnan(y[0, :32]).all() and np.isfinite(y[0, 32:]).all()
    assert not np.isfinite(y[1, 32:]).any() and np.isfinite(y[1, :32]).all()
    assert (y[2, :32] == 0).all() and np.array_equal(y[2, 32:], y[0, 32:])


# ------------------------------------------------------------------------------------------------ 2. the product is kept
def test_product_is_kept_exactly():
    rng = np.random.default_rng(1)
    x = rng.integers(-8, 9, (7, 96)).astype(np.float32)
    w = (32 * rng.integers(-4, 5, (96, 10))).astype(np.float32)
    want = x.astype(np.float64) @ w.astype(np.float64)
    wf = R.fold_weight(w, 0)
    assert np.array_equal(R.fwht32(x).astype(np.float64) @ wf.astype(np.float64), want)
    assert np.array_equal(R.rotated_product(x, w), want) and np.array_equal(R.plain_product(x, w), want)
    assert np.array_equal(R.fold_weight(w.T.copy(), 1), wf.T)                # a transB weight: the same values, transposed


# ------------------------------------------------------------------------------------------------ 3. the site finder
def _build(nodes, init, inputs, outputs):
    m = onnx_io.Model()
    m.nodes, m.initializers = nodes, init
    m.inputs = [(n, onnx_io.FLOAT, s) for n, s in inputs]
    m.outputs = [(n, onnx_io.FLOAT, None) for n in outputs]
    return ONNXGraph(m)


def _hand_graph():
    rng = np.random.default_rng(2)
    w = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    init = {"w_mm": w(64, 10), "w_g0": w(64, 6), "w_g1": w(6, 64), "w_sh1": w(64, 4), "w_sh2": w(64, 4), "w_48": w(48, 5),
            "w_twice": w(64, 64), "w_ta": w(3, 7), "w_skip": w(64, 3), "w_3d": w(2, 64, 3), "c_left": w(3, 64), "w_cl": w(64, 2)}
    nodes = [Node("MatMul", ["x", "w_mm"], ["o_mm"], name="mm"),
             Node("Gemm", ["x", "w_g0"], ["o_g0"], name="gemm0"),
             Node("Gemm", ["x2", "w_g1"], ["o_g1"], name="gemm1", attrs={"transB": 1}),
             Node("Relu", ["x2"], ["r"], name="relu"),                                   # a reader of x2 that is no site
             Node("MatMul", ["r", "w_sh1"], ["o_sh1"], name="shared1"),
             Node("MatMul", ["r", "w_sh2"], ["o_sh2"], name="shared2"),
             Node("MatMul", ["x48", "w_48"], ["o_48"], name="k48"),
             Node("MatMul", ["x", "w_twice"], ["o_t1"], name="twice1"),
             Node("MatMul", ["o_t1", "w_twice"], ["o_t2"], name="twice2"),
             Node("Gemm", ["xt", "w_ta"], ["o_ta"], name="transa", attrs={"transA": 1}),
             Node("MatMul", ["o_sh1", "o_sh2t"], ["o_aa"], name="actact"),
             Node("Transpose", ["o_sh2"], ["o_sh2t"], name="tr", attrs={"perm": [1, 0]}),
             Node("MatMul", ["x", "w_skip"], ["o_skip"], name="skipped"),
             Node("MatMul", ["x", "w_3d"], ["o_3d"], name="w3d"),
             Node("MatMul", ["c_left", "w_cl"], ["o_cc"], name="constleft")]
    nodes[10], nodes[11] = nodes[11], nodes[10]                                          # (the Transpose in front of its reader)
    outs = ["o_mm", "o_g0", "o_g1", "o_aa", "o_48", "o_t2", "o_ta", "o_skip", "o_3d", "o_cc"]
    return _build(nodes, init, [("x", [3, 64]), ("x2", [3, 64]), ("x48", [3, 48]), ("xt", [3, 5])], outs), init


def test_site_finder():
    g, init = _hand_graph()
    sites, left = find_rotate_sites(g, ["skipped"])
    assert [tuple(s) for s in sites] == [("mm", "x", "w_mm", 0, 64), ("gemm0", "x", "w_g0", 0, 64), ("gemm1", "x2", "w_g1", 1, 64),
                                         ("shared1", "r", "w_sh1", 0, 64), ("shared2", "r", "w_sh2", 0, 64)]
    why = dict(left)
    assert set(why) == {"k48", "twice1", "twice2", "transa", "actact", "skipped", "w3d", "constleft"}
    for name, word in (("k48", "K = 48"), ("twice1", "another reader"), ("twice2", "another reader"), ("transa", "transA"),
                       ("actact", "activation x activation"), ("skipped", "--skip_layers"), ("w3d", "3 axes"), ("constleft", "operand 0 is a constant")):
        assert word in why[name], (name, why[name])
    assert [s.node for s in find_rotate_sites(g)[0]].count("skipped") == 1              # without the flag it is a site
    gr = apply_rotate(g, sites)
    had = [n for n in gr.graph.node if n.op_type == "BlockHadamard"]
    assert [(n.input[0], n.output[0]) for n in had] == [("x", "x_rot"), ("x2", "x2_rot"), ("r", "r_rot")]      # ONE node per activation
    assert all(n.domain == MX_DOMAIN and n.attrs == {"block_size": 32} for n in had)
    by = {n.name: n for n in gr.graph.node}
    assert [by[s.node].input[0] for s in sites] == ["x_rot", "x_rot", "x2_rot", "r_rot", "r_rot"]
    assert by["relu"].input[0] == "x2" and by["skipped"].input[0] == "x" and by["twice1"].input[0] == "x"      # no sites: they keep T
    order = {n.name: i for i, n in enumerate(gr.graph.node)}
    for n in had:                                        # behind the producer of T, in front of every reader of T_rot
        p = gr.get_tensor_producer(n.input[0])
        assert isinstance(p, str) or order[p.name] < order[n.name]
        assert all(order[n.name] < order[r.name] for r in gr.get_tensor_consumer(n.output[0]))
    for s in sites:                                      # 4. the host fold is the model's, bit for bit
        got = gr.get_initializer(s.weight)
        assert got.dtype == np.float32 and got.shape == init[s.weight].shape
        assert np.array_equal(got.view(np.uint32), R.fold_weight(init[s.weight], s.axis).view(np.uint32)), s.node
    for name in set(init) - {s.weight for s in sites}:
        assert gr.get_initializer(name) is g.get_initializer(name)
    assert {n.name: n for n in g.graph.node}["mm"].input[0] == "x" and not any(n.op_type == "BlockHadamard" for n in g.graph.node)
    rep = rotate_report(sites, left)
    assert rep["rotated"][2] == {"node": "gemm1", "activation": "x2_rot", "weight": "w_g1", "K": 64}
    assert {"node": "k48", "why": why["k48"]} in rep["left"]


def test_host_fold_equals_the_model_bit_for_bit():
    rng = np.random.default_rng(3)
    for shape, axis in (((96, 7), 0), ((7, 96), 1), ((32, 1), 0), ((256, 33), 0)):
        w = (rng.standard_normal(shape) * np.exp2(rng.integers(-30, 30, shape))).astype(np.float32)
        assert np.array_equal(fold_weight_host(w, axis).view(np.uint32), R.fold_weight(w, axis).view(np.uint32)), (shape, axis)


def test_a_graph_without_a_site_is_returned_unchanged(tmp_path):
    init = {"w": np.ones((48, 4), np.float32)}
    g = _build([Node("MatMul", ["x", "w"], ["y"], name="mm")], init, [("x", [2, 48])], ["y"])
    assert mx_rotate(g, types.SimpleNamespace(skip_layers=[], output_dir=str(tmp_path))) is g
    assert os.listdir(tmp_path) == []


# ------------------------------------------------------------------------------------------------ 5. round trip
def test_round_trip_keeps_node_domain_attribute_and_opset(tmp_path):
    g, _ = _hand_graph()
    gr = mx_rotate(g, types.SimpleNamespace(skip_layers=["skipped"], output_dir=str(tmp_path)))
    assert gr is not g and sorted(os.listdir(tmp_path)) == ["rotate_model.onnx", "rotate_report.json"]
    rep = json.load(open(tmp_path / "rotate_report.json"))
    assert [r["node"] for r in rep["rotated"]] == ["mm", "gemm0", "gemm1", "shared1", "shared2"] and len(rep["left"]) == 8
    m = onnx_io.load_model(str(tmp_path / "rotate_model.onnx"))
    had = [n for n in m.nodes if n.op_type == "BlockHadamard"]
    assert len(had) == 3 and all(n.domain == "dipoorlet.amd" and n.attrs["block_size"] == 32 for n in had)
    assert m.opset["dipoorlet.amd"] == 1 and m.opset[""] == g.opset[""]
    g2 = ONNXGraph.load(str(tmp_path / "rotate_model.onnx"))
    assert [(n.op_type, n.name, n.input, n.output, n.domain) for n in g2.graph.node] == \
        [(n.op_type, n.name, n.input, n.output, n.domain) for n in gr.graph.node]
    for k, v in gr.initializer.items():
        assert np.array_equal(g2.get_initializer(k), v)
    assert find_rotate_sites(g2, ["skipped"])[0] == []            # (not rotated twice)
    g2.output_dir = str(tmp_path)
    m3 = onnx_io.load_model(g2.save_onnx_model("again"))          # and a second save of the reloaded graph keeps all three
    assert m3.opset["dipoorlet.amd"] == 1 and sum(n.op_type == "BlockHadamard" and n.domain == "dipoorlet.amd" for n in m3.nodes) == 3


# ------------------------------------------------------------------------------------------------ 6. shape rule
def test_shape_rule_and_host_session():
    from dipoorlet_amd import executor as ex
    from dipoorlet_amd.executor import GraphSession
    node = Node("BlockHadamard", ["x"], ["y"], name="h", domain=MX_DOMAIN, attrs={"block_size": 32})
    host = shape_infer._HostRun(types.SimpleNamespace(opset={"": 13}), 2)
    for shape in ((64,), (5, 64), (2, 17, 96)):
        out = shape_infer._RULES["BlockHadamard"](ex, host, node, shape_infer.Spec(shape))
        assert out.shape == shape and out.dtype == torch.float32
    g, _ = _hand_graph()
    gr = apply_rotate(g, find_rotate_sites(g)[0])
    env = shape_infer.infer(gr, set(), gr.network_inputs)
    assert tuple(env["x_rot"].shape) == (3, 64) and tuple(env["r_rot"].shape) == (3, 64)
    # per-sample (the images on axis 0, the blocks along the last of two axes)
    init = {"w": np.ones((64, 4), np.float32)}
    g1 = _build([Node("MatMul", ["x", "w"], ["y"], name="mm")], init, [("x", [1, 64])], ["y"])
    g1r = apply_rotate(g1, find_rotate_sites(g1)[0])
    assert shape_infer.batch_transparent(g1r, set(), g1r.network_inputs, shape_infer.infer(g1r, set(), g1r.network_inputs))
    sess = GraphSession(gr, device="cpu")                          # the op table knows the node; on the host it is the identity
    x = torch.arange(3 * 64, dtype=torch.float32).reshape(3, 64)
    feeds = {"x": x, "x2": x, "x48": torch.ones(3, 48), "xt": torch.ones(3, 5)}
    assert torch.equal(sess.run_named(feeds, ["x_rot"])[0], x)
    assert ex.has_op("BlockHadamard") and ex.has_op("MatMul") and not ex.has_op("NoSuchOp")
    with pytest.raises(NotImplementedError, match="block_size"):
        ex.run_op(None, Node("BlockHadamard", ["x"], ["y"], attrs={"block_size": 64}), x)


# ------------------------------------------------------------------------------------------------ 7. the CLI's checks
def _parse(*extra):
    return build_parser().parse_args(["-M", "m.onnx", "-I", "d", "-N", "4", *extra])


def test_check_args():
    assert _parse("-D", "ocp_fp8").mx_rotate is False
    with pytest.raises(ValueError) as e:
        check_args(_parse("-D", "ocp_fp8", "-A", "hist", "--mx_rotate"))
    assert "--mx_rotate" in str(e.value) and "--mx " in str(e.value)
    with pytest.raises(ValueError, match="--mx_rotate"):
        check_args(_parse("-D", "trt", "--mx_rotate"))
    for mx in ("mxfp4", "mxfp8"):
        a = _parse("-D", "ocp_fp8", "-A", "hist", "--mx", mx, "--mx_rotate")
        assert a.mx_rotate is True
        check_args(a)
    check_args(_parse("-D", "ocp_fp8", "-A", "hist", "--mx", "mxfp4", "--mx_rotate", "--smooth", "--bc"))
    with pytest.raises(ValueError, match="ocp_fp8"):                # (--mx's own refusal stays)
        check_args(_parse("-D", "trt", "--mx", "mxfp4", "--mx_rotate"))
    h = build_parser().format_help()
    assert "rotate_model.onnx" in h and "rotate_report.json" in h and "X . W" in h


# ------------------------------------------------------------------------------------------------ 8. ABI
def test_abi_declares_the_kernel():
    assert _hip.ABI_VERSION >= 29
    header = open(os.path.join(ROOT, "include", "dipoorlet_hip.h")).read()
    assert int(re.search(r"#define DPL_ABI_VERSION (\d+)", header).group(1)) == _hip.ABI_VERSION
    assert "dpl_hadamard32" in _hip.SIGNATURES
    assert re.search(r"int dpl_hadamard32\(const float\* d_x, float\* d_y, uint64_t rows, uint64_t k, dpl_stream_t s\);", header)
    assert re.search(r"29: dpl_hadamard32", header)
    res, args = _hip.SIGNATURES["dpl_hadamard32"]
    assert len(args) == 5
    import dipoorlet_amd.torch_ops  # noqa: F401
    assert hasattr(torch.ops.dipoorlet, "hadamard32")
    with pytest.raises(NotImplementedError):
        torch.ops.dipoorlet.hadamard32(torch.zeros(4, 32))
    from dipoorlet_amd import ops
    with pytest.raises(_hip.DipoorletHipError):
        ops.hadamard32(torch.zeros(4, 32))                          # no CPU path


# ------------------------------------------------------------------------------------------------ 9. error direction (model only)
def _inputs(kind, rng):
    M, K = 256, 768
    if kind == "outlier":                                           # N(0,1), 2 % of the channels x 30
        x = rng.standard_normal((M, K))
        x[:, rng.choice(K, K // 50, replace=False)] *= 30.0
    elif kind == "student_t3":
        x = rng.standard_t(3, (M, K))
    elif kind == "laplace":
        x = rng.laplace(size=(M, K))
    else:
        x = rng.standard_normal((M, K))
    return x.astype(np.float32), (0.05 * rng.standard_normal((K, 256))).astype(np.float32)


def test_error_direction_on_the_model():
    """The relative Frobenius error of Q(X) . Q(W) against fp64 X . W, rotated / plain, on X = N(0,1) with 2 % of the channels
    x 30: below 1 for both formats (direction only; DESIGN section 3l quotes the printed values)."""
    for elem in ("mxfp4", "mxfp8"):
        x, w = _inputs("outlier", np.random.default_rng(2025))
        rot, plain = R.error_ratio(x, w, elem)
        print(f"MX product error, outlier channels, {elem}: rotated {rot:.5f} / plain {plain:.5f} = {rot / plain:.3f}")
        assert np.isfinite(rot) and plain > 0 and rot / plain < 1.0


def test_error_table_of_the_design_document():
    """The other rows of the table (printed; no direction is asserted for them: on N(0,1) the rotation has nothing to spread)."""
    for kind in ("student_t3", "laplace", "normal"):
        for elem in ("mxfp4", "mxfp8"):
            x, w = _inputs(kind, np.random.default_rng(2025))
            rot, plain = R.error_ratio(x, w, elem)
            print(f"MX product error, {kind}, {elem}: rotated {rot:.5f} / plain {plain:.5f} = {rot / plain:.3f}")
            assert np.isfinite(rot) and np.isfinite(plain) and plain > 0
