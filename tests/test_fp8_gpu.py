"""GPU: the OCP FP8 E4M3 Q/DQ kernels (fq_span<PRE, kFqFmtE4M3>, dpl_fake_quant_fp8 / dpl_fake_quant_fp8_items) against the numpy
definition (tests/fp8_model.py), bit for bit — no tolerance anywhere in this file —, and the `ocp_fp8` platform from the graph
session up to the CLI.  Sizes are the smallest that reach every path of fq_span: a workgroup's chunk is 3072 elements, a lane
holds four 16-byte vectors at a time (4096 elements per round of the block), rows shorter than a vector and unaligned views go
element by element, a row length that is no multiple of four makes vectors straddle two channels."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import fp8_model as M
from fp8_checks import check_saved_fp8_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1.0, 0.0123, 2.0 ** -20, 3e4)
LENGTHS = (1, 3, 1023, 1024, 1025, 4099, (1 << 20) + 5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pool():
    """NaN, +-inf, fp32 subnormals and the boundary point set of the format times each scale (a point p * s divided by s is p
    again wherever the product is exact — every power-of-two scale — and lands next to p otherwise): computed once, never changed."""
    pts = M.boundary_points()
    special = np.array([np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 0.0, -0.0, 1e9, -1e9,
                        3.4e38, -3.4e38], np.float32)
    with np.errstate(over="ignore"):
        body = np.concatenate([(pts * np.float32(s)).astype(np.float32) for s in SCALES])
    rng = np.random.default_rng(23)
    p = np.concatenate([special, rng.permutation(body)])
    p.setflags(write=False)
    return p


def _assert_same(got, want, what):
    """Equal as fp32 values, NaN in the same places, signed zeros alike: the same 32 bits wherever the value is no NaN."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32))))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _take(pool, n, start=0):
    return np.resize(np.roll(pool, -start), n).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. per tensor
@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_equals_the_model_per_tensor(dev, pool, n):
    from dipoorlet_amd import ops
    x = _take(pool, n, start=0 if n > 4 else 15)       # (the shortest tensors start at the first boundary points)
    if n == 3:
        x[:] = [np.nan, -1e-9, 464.0 * 0.0123]
    buf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    out = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    for off in (0, 1):          # a 16-byte-aligned view; a view one element in: element by element
        xv, yv = buf[off:off + n], out[off:off + n]
        assert xv.data_ptr() % 16 == 4 * off and yv.data_ptr() % 16 == 4 * off
        xv.copy_(torch.from_numpy(x))
        for s in SCALES:
            out.fill_(-77.0)
            y = ops.fake_quant_fp8(xv, torch.tensor([s], dtype=torch.float32, device=dev), out=yv)
            assert y is yv
            host = out.cpu().numpy()
            _assert_same(host[off:off + n], M.fake_quant_fp8(x, [s]), (n, off, s))
            assert (host[:off] == -77.0).all() and (host[off + n:] == -77.0).all(), (n, off, s)      # nothing written outside


# ------------------------------------------------------------------------------------------------ 2. per channel
@pytest.mark.parametrize("inner", [1, 3, 49, 64])
@pytest.mark.parametrize("C", [3, 64])
def test_kernel_equals_the_model_per_channel(dev, pool, C, inner):
    """Rows shorter than a vector (inner 1, 3), vectors that straddle two channels (49), aligned rows (64); more than two
    chunks, and an odd number of outer slices so that the 3 x 49 tensor ends in a tail."""
    from dipoorlet_amd import ops
    outer = -(-7001 // (C * inner)) | 1
    scale = (np.float32(0.0123) * (1 + np.arange(C, dtype=np.float32) / 7)).astype(np.float32)
    scale[C // 2] = 2.0 ** -20
    scale[-1] = 3e4
    assert len(set(scale.tolist())) == C
    x = _take(pool, outer * C * inner).reshape(outer, C, inner)
    xd = torch.from_numpy(x).to(dev)
    y = ops.fake_quant_fp8(xd, torch.from_numpy(scale).to(dev), axis=1)
    _assert_same(y.cpu().numpy(), M.fake_quant_fp8(x, scale, axis=1), (C, inner))
    if inner == 49:     # the same rows through an unaligned view
        buf = torch.zeros(x.size + 1, dtype=torch.float32, device=dev)
        v = buf[1:].view(outer, C, inner)
        v.copy_(xd)
        _assert_same(ops.fake_quant_fp8(v, torch.from_numpy(scale).to(dev), axis=1).cpu().numpy(), M.fake_quant_fp8(x, scale, axis=1),
                     (C, inner, "unaligned"))


def test_argument_checks_are_those_of_fake_quant(dev):
    from dipoorlet_amd import _hip, ops
    x = torch.zeros(2, 3, 4, device=dev)
    s3 = torch.ones(3, device=dev)
    with pytest.raises(_hip.DipoorletHipError, match="per-channel fake_quant needs an axis"):
        ops.fake_quant_fp8(x, s3)
    with pytest.raises(_hip.DipoorletHipError, match="axis 2 has 4 channels, scale has 3"):
        ops.fake_quant_fp8(x, s3, axis=2)
    with pytest.raises(_hip.DipoorletHipError, match="x2 must be a contiguous fp32 tensor of x's shape"):
        ops.fake_quant_fp8(x, s3, axis=1, pre="add_relu", x2=torch.zeros(2, 3, device=dev))
    assert ops.fake_quant_fp8(torch.zeros(0, device=dev), s3[:1]).numel() == 0


# ------------------------------------------------------------------------------------------------ 3. pre
def _assert_same_values(got, want, what):
    """As _assert_same, but -0 == +0: what relu makes of a -0 is the producer's business (the kernel keeps it, as torch.relu;
    np.maximum(-0.0, 0) may return either zero), and the Q/DQ pair then keeps that zero's sign."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~wn & (got != want)))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("shape,axis", [((4099,), None), ((49, 3, 49), 1), ((1025,), "unaligned")])
def test_relu_and_add_relu_on_the_way_in(dev, pool, shape, axis):
    from dipoorlet_amd import ops
    n = int(np.prod(shape))
    x = _take(pool, n).reshape(shape)
    rng = np.random.default_rng(41)
    x2 = (rng.standard_normal(n).astype(np.float32) * np.float32(3.0)).reshape(shape)
    x2.reshape(-1)[::97] = np.nan
    x2.reshape(-1)[1::97] = -x.reshape(-1)[1::97]            # sums that are exactly zero
    scale = np.array([0.0123], np.float32) if axis != 1 else np.array([0.0123, 2.0 ** -20, 0.7], np.float32)
    if axis == "unaligned":
        bx, b2 = (torch.zeros(n + 1, device=dev) for _ in range(2))
        xd, x2d = bx[1:], b2[1:]
        xd.copy_(torch.from_numpy(x))
        x2d.copy_(torch.from_numpy(x2))
    else:
        xd, x2d = torch.from_numpy(x).to(dev), torch.from_numpy(x2).to(dev)
    sd = torch.from_numpy(scale).to(dev)
    ax = axis if axis == 1 else None
    with np.errstate(all="ignore"):
        want_relu = M.fake_quant_fp8(np.maximum(x, np.float32(0)), scale, axis=ax)
        want_add = M.fake_quant_fp8(np.maximum((x + x2).astype(np.float32), np.float32(0)), scale, axis=ax)
    assert np.isnan(want_relu).any() and np.isnan(want_add).sum() > np.isnan(want_relu).sum()       # NaN stays NaN
    _assert_same_values(ops.fake_quant_fp8(xd, sd, axis=ax, pre="relu").cpu().numpy(), want_relu, (shape, "relu"))
    _assert_same_values(ops.fake_quant_fp8(xd, sd, axis=ax, pre="add_relu", x2=x2d).cpu().numpy(), want_add, (shape, "add_relu"))
    _assert_same(ops.fake_quant_fp8(xd, sd, axis=ax, pre="none").cpu().numpy(), M.fake_quant_fp8(x, scale, axis=ax), (shape, "none"))


# ------------------------------------------------------------------------------------------------ 4. the set form
def test_set_form_equals_the_per_tensor_launches(dev, pool):
    from dipoorlet_amd import ops
    shapes = [(1, 1), (1, 8, 125), (1, 3 * 1024 + 1), (1, 64, 3125)]          # 1, 1000, 3073, 200 000 elements
    assert [int(np.prod(s)) for s in shapes] == [1, 1000, 3 * 1024 + 1, 200000]
    xs = [torch.from_numpy(_take(pool, int(np.prod(s)), start=7 * i).reshape(s)).to(dev) for i, s in enumerate(shapes)]
    scales = [torch.tensor([0.0123], device=dev),
              torch.from_numpy((0.01 * (1 + np.arange(8, dtype=np.float32))).astype(np.float32)).to(dev),
              torch.tensor([2.0 ** -20], device=dev),
              torch.from_numpy((3e-3 * (1 + np.arange(64, dtype=np.float32) / 5)).astype(np.float32)).to(dev)]
    want = [ops.fake_quant_fp8(x, s, axis=1 if s.numel() > 1 else None) for x, s in zip(xs, scales)]
    for x, s, w in zip(xs, scales, want):          # (the per-tensor launches themselves: against the model)
        _assert_same(w.cpu().numpy(), M.fake_quant_fp8(x.cpu().numpy(), s.cpu().numpy(), axis=1 if s.numel() > 1 else None), tuple(x.shape))
    plan = ops.TensorSetPlan([x.numel() for x in xs], 1, dev)
    fq = ops.FakeQuantSet(plan, [(s, x.shape[-1]) for x, s in zip(xs, scales)], fmt="fp8")
    got = fq(xs)
    for g, w in zip(got, want):
        _assert_same(g.cpu().numpy(), w.cpu().numpy(), tuple(w.shape))
    inplace = [x.clone() for x in xs]
    assert fq(inplace, out=inplace) is inplace
    for g, w in zip(inplace, want):
        _assert_same(g.cpu().numpy(), w.cpu().numpy(), ("in place", tuple(w.shape)))


# ------------------------------------------------------------------------------------------------ 5. torch op
def test_torch_op(dev, pool):
    from dipoorlet_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.dipoorlet.*)
    x = torch.from_numpy(_take(pool, 5 * 3 * 49).reshape(5, 3, 49)).to(dev)
    s1, s3 = torch.tensor([0.0123], device=dev), torch.tensor([0.0123, 1.0, 3e4], device=dev)
    _assert_same(torch.ops.dipoorlet.fake_quant_fp8(x, s1, 0).cpu().numpy(), ops.fake_quant_fp8(x, s1).cpu().numpy(), "per tensor")
    _assert_same(torch.ops.dipoorlet.fake_quant_fp8(x, s3, 1).cpu().numpy(), ops.fake_quant_fp8(x, s3, axis=1).cpu().numpy(), "per channel")
    xt = x.transpose(0, 2)      # (a non-contiguous input is made contiguous, as dipoorlet::fake_quant does)
    _assert_same(torch.ops.dipoorlet.fake_quant_fp8(xt, s1, 0).cpu().numpy(), ops.fake_quant_fp8(xt.contiguous(), s1).cpu().numpy(), "strided")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        y = torch.ops.dipoorlet.fake_quant_fp8(torch.empty(5, 3, 49, device="cuda"), torch.empty(3, device="cuda"), 1)
        assert tuple(y.shape) == (5, 3, 49) and y.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 6. graph level
IMG = 32


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("fp8")
    g = models.resnet18(seed=11, image=IMG)
    g.output_dir = str(d)
    g.save_onnx_model("model")
    os.makedirs(d / "calib" / "input")
    rng = np.random.default_rng(5)
    for i in range(8):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(d / "calib" / "input" / f"{i}.bin")
    return d


@pytest.mark.two_forwards
def test_quantised_graph_runs_the_fp8_kernels(workdir, dev, monkeypatch):
    from dipoorlet_amd import dist_helper
    from dipoorlet_amd.forward_net import load_input_batch
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.quantize import quant_graph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    dist_helper.init_default()
    g = ONNXGraph.load(str(workdir / "model.onnx"))
    out = workdir / "graph"
    os.makedirs(out, exist_ok=True)
    args = types.SimpleNamespace(input_dir=str(workdir / "calib"), data_num=4, rank=0, local_rank=0, world_size=1, bins=2048,
                                 threshold=0.99999, deploy="ocp_fp8", act_quant="minmax", calib_batch=4, output_dir=str(out),
                                 skip_layers=[], savefp=False)
    a, w = tensor_calibration(g, args)
    clip = {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**a, **w}.items()}
    gq, _ = quant_graph(g, clip, args)
    assert all(q.fmt == "Float8E4M3FN" for q in gq._qdq.values()) and len(gq._qdq) > 30
    inp = load_input_batch(args.input_dir, g.network_inputs, {"input": g.get_tensor_shape("input")}, 0, 4, dev)
    x = inp["input"].cpu().numpy()
    lo, hi = float(x.min()), float(x.max())
    assert [float(v) for v in a["input"]] == [lo, hi]
    s_in = np.float32(max(abs(lo), abs(hi)) / 448)
    assert gq._qdq["input_QuantizeLinear"].scale.tolist() == [float(s_in)]
    net_out = gq.network_outputs[0]
    monkeypatch.setenv("DPL_FUSE_RELU", "1")
    sq = gq.make_session()
    fused, _ = sq.fusion([net_out])
    assert [p for p, _ in fused.values()].count("relu") >= 4       # ReLU -> Q/DQ chains run as k_fake_quant<PRE, E4M3>
    in_dq, y_fused = sq.run_named(inp, ["input_dq", net_out])
    _assert_same(in_dq.cpu().numpy(), M.fake_quant_fp8(x, [s_in]), "input_dq")
    # the first convolution's weight, folded at session build by the set form, per output channel
    wq = gq._qdq["conv1.weight_QuantizeLinear"]
    w0 = g.get_initializer("conv1.weight")
    assert wq.axis == 0 and wq.scale.size == w0.shape[0]
    assert np.array_equal(wq.scale, (np.abs(w0.reshape(w0.shape[0], -1)).max(1).astype(np.float64) / 448).astype(np.float32))
    assert "conv1.weight_QuantizeLinear" in sq._folded
    _assert_same(sq.consts["conv1.weight_dq"].cpu().numpy(), M.fake_quant_fp8(w0, wq.scale, axis=0), "conv1.weight_dq")
    monkeypatch.setenv("DPL_FUSE_RELU", "0")
    sp = gq.make_session()
    assert not sp.fusion([net_out])[0]
    (y_plain,) = sp.run_named(inp, [net_out])
    assert torch.equal(y_fused, y_plain) and torch.isfinite(y_plain).all()


# ------------------------------------------------------------------------------------------------ 7. CLI
def _cli(workdir, out, algo, *extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "model.onnx"), "-I",
           str(workdir / "calib"), "-N", "8", "-A", algo, "-D", "ocp_fp8", "-O", str(out), "--calib_batch", "4", *extra]
    return subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_cli_hist_bc_writes_scales_and_an_opset_19_model(workdir):
    from dipoorlet_amd.platform_settings import platform_setting_table
    from dipoorlet_amd.quantize import get_qnode_by_param
    out = workdir / "cli_hist"
    r = _cli(workdir, out, "hist", "--bc")
    assert r.returncode == 0, r.stdout[-3000:]
    act = json.load(open(out / "act_clip_val.json"))
    scales = json.load(open(out / "ocp_fp8_scales.json"))
    assert scales["format"] == "float8e4m3fn" and set(scales["scale"]) == set(act) and len(act) > 30
    qi = platform_setting_table["ocp_fp8"]["qi_params"]
    for name, (lo, hi) in act.items():
        q, _, _ = get_qnode_by_param(qi, name, None, [lo, hi])
        assert scales["scale"][name] == float(q.scale[0]) == float(np.float32(max(abs(lo), abs(hi)) / 448 or 1.0)), name
    assert os.path.exists(out / "update_bias_model.onnx")
    n = check_saved_fp8_model(out / "quant_model.onnx", 30, lambda t: 0)
    assert n > 30


def test_cli_refuses_mse_before_any_forward(workdir):
    out = workdir / "cli_mse"
    r = _cli(workdir, out, "mse")
    assert r.returncode not in (0, 124, 137), r.stdout[-3000:]
    assert "floating-point grid" in r.stdout and "-A mse" in r.stdout and "Supported: -A minmax, -A hist" in r.stdout
    assert not os.path.exists(out)          # nothing was set up, let alone run
