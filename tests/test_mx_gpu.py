"""GPU: the OCP Microscaling Q/DQ kernels (k_fake_quant_mx_rows / _cols, dpl_fake_quant_mx) against the numpy definition
(tests/mx_model.py), bit for bit, the E8M0 scale codes included — no tolerance anywhere in this file —, and `--mx` from the graph
session up to the CLI.  Shapes are the smallest that reach every path: inner == 1 runs 8 lanes per block on 16-byte vectors when
the bases are aligned and K % 4 == 0 and 32 lanes per block otherwise (a workgroup owns 128 or 32 blocks); inner > 1 gives a lane
four columns when inner % 4 == 0 and the bases are aligned, else one, and a workgroup is one wave."""
import gc
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mx_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMS = ("mxfp8", "mxfp4")
GUARD = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    """Sessions, calibration runs and caught exceptions hold device tensors in reference cycles, which only a pass of the cycle
    collector frees — at a moment of its own choosing, possibly inside a later test that watches torch.cuda.memory_allocated()
    (tests/test_octav_routes.py does).  Every test of this file ends with that pass."""
    yield
    gc.collect()


def _data(shape, seed):
    """Values over some forty binades, a few exact zeros of both signs and fp32 subnormals among them."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * np.exp2(rng.integers(-20, 20, shape))).astype(np.float32)
    flat = x.reshape(-1)
    flat[::37] = 0.0
    flat[5::91] = -0.0
    flat[11::113] = np.float32(1e-41)
    return x


def _same(got, want, what):
    """The same 32 bits wherever the value is no NaN, NaN in the same places."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32))))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _run(x, axis, elem, dev, misaligned=False):
    """ops.fake_quant_mx on a copy of x whose base is 16-byte aligned, or one float off -> (y, scales) on the host; the floats and
    the scale bytes around both outputs must come back untouched."""
    from dipoorlet_amd import ops
    off = 1 if misaligned else 0
    n = x.size
    nsc = (n // x.shape[axis]) * -(-x.shape[axis] // 32)
    bx = torch.zeros(n + 2 * GUARD + off, dtype=torch.float32, device=dev)
    by = torch.full((n + 2 * GUARD + off,), -77.0, dtype=torch.float32, device=dev)
    bs = torch.full((nsc + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    xv, yv = bx[GUARD + off:GUARD + off + n].view(x.shape), by[GUARD + off:GUARD + off + n].view(x.shape)
    assert xv.data_ptr() % 16 == 4 * off and yv.data_ptr() % 16 == 4 * off
    xv.copy_(torch.from_numpy(x))
    ret = ops.fake_quant_mx(xv, axis, elem, out=yv, scales=bs[GUARD:GUARD + nsc])
    assert ret is yv
    hy, hs = by.cpu().numpy(), bs.cpu().numpy()
    assert (hy[:GUARD + off] == -77.0).all() and (hy[GUARD + off + n:] == -77.0).all(), "written outside y"
    assert (hs[:GUARD] == 0xA5).all() and (hs[GUARD + nsc:] == 0xA5).all(), "written outside scales"
    return hy[GUARD + off:GUARD + off + n].reshape(x.shape), hs[GUARD:GUARD + nsc]


def _check(x, axis, dev, what, misaligned=(False, True)):
    for elem in ELEMS:
        want_y, want_s = M.fake_quant_mx(x, axis, elem, return_scales=True)
        for mis in misaligned:
            y, s = _run(x, axis, elem, dev, mis)
            _same(y, want_y, (what, elem, mis))
            assert np.array_equal(s, want_s.reshape(-1)), (what, elem, mis, np.flatnonzero(s != want_s.reshape(-1))[:5])


# ------------------------------------------------------------------------------------------------ 1. contiguous blocks
@pytest.mark.parametrize("outer", [1, 3, 197])
@pytest.mark.parametrize("K", [1, 4, 31, 32, 33, 36, 64, 100, 768])
def test_contiguous_path(dev, outer, K):
    _check(_data((outer, K), 1000 * outer + K), 1, dev, (outer, K))


# ------------------------------------------------------------------------------------------------ 2. strided blocks
@pytest.mark.parametrize("outer", [1, 3])
@pytest.mark.parametrize("inner", [2, 3, 4, 17, 64, 197])
@pytest.mark.parametrize("K", [17, 32, 40, 64])
def test_strided_path(dev, outer, K, inner):
    _check(_data((outer, K, inner), 100000 * outer + 1000 * K + inner), 1, dev, (outer, K, inner))


# ------------------------------------------------------------------------------------------------ 3. more than one workgroup's share
@pytest.mark.parametrize("shape", [(4096, 1056), (8, 1056, 520)])
def test_larger_shapes(dev, shape):
    """Past 2^22 elements and many workgroups on either path; 1056 = 33 blocks."""
    assert int(np.prod(shape)) > 1 << 22
    _check(_data(shape, 7), 1, dev, shape, misaligned=(False,))


# ------------------------------------------------------------------------------------------------ 4. rounding
@pytest.mark.parametrize("elem", ELEMS)
def test_every_code_tie_and_neighbour(dev, elem):
    """boundary_points(elem) * 2^se, 31 to a block beside a sentinel (the largest value of the format times 2^se) that pins the
    block's shared exponent to se: every code, every tie and their fp32 neighbours go through the kernel under each se — -127, where
    inputs and outputs are fp32 subnormals, and the largest one at which the sentinel is finite."""
    pts = M.boundary_points(elem)
    nb = -(-pts.size // 31)
    blocks = []
    for se in (-127, -20, 0, 30, 119):
        blk = np.zeros((nb, 32), np.float64)
        blk[:, 0] = M.ELEM_MAX[elem]
        blk[:, 1:].reshape(-1)[:pts.size] = pts
        blocks.append(np.ldexp(blk, se).astype(np.float32))
    x = np.concatenate(blocks)                                        # [5 * nb, 32]
    want_y, want_s = M.fake_quant_mx(x, 1, elem, return_scales=True)
    assert sorted(set(want_s.reshape(-1).tolist())) == [0, 107, 127, 157, 246]
    for xx, axis, wy, ws in ((x, 1, want_y, want_s.reshape(-1)), (np.ascontiguousarray(x.T), 0, want_y.T, want_s[:, 0, 0])):
        for mis in (False, True):
            y, s = _run(xx, axis, elem, dev, mis)
            _same(y, wy, (elem, axis, mis))
            assert np.array_equal(s, ws), (elem, axis, mis)


# ------------------------------------------------------------------------------------------------ 5. special values
def _special_rows():
    """[12, 64]: block 0 of every row is special, block 1 ordinary (and must come out as it does everywhere else)."""
    ordinary = np.linspace(-3, 3, 32).astype(np.float32)
    x = np.tile(ordinary, (12, 2)).astype(np.float32)
    x[0, :32] = 0
    x[0, 1:32:2] = -0.0                                    # all zero, mixed signs
    x[1, 7] = np.nan
    x.view(np.uint32)[1, 9] = 0xFFC00001                   # (and a negative NaN with a payload)
    x[2, 9] = np.inf
    x[3, 11] = -np.inf
    x[4, :32] = np.float32(2.0 ** -131)
    x[4, 0] = -np.float32(2.0 ** -130)                     # a = 2^-130, an fp32 subnormal
    x[5, :32] = np.float32(2.0 ** -127)
    x[5, 3] = np.float32(2.0 ** -120)                      # a = 2^-120: subnormal outputs under se = -127 (E4M3)
    x[6, :32] = np.float32(1.0)
    x[6, 31] = np.float32(3.4028234663852886e38)           # a = the largest finite fp32
    for r, a in ((7, np.float32(1.0)), (8, np.nextafter(np.float32(1.0), np.float32(2))), (9, np.nextafter(np.float32(1.0), np.float32(0)))):
        x[r, :32] = np.linspace(-0.9, 0.9, 32).astype(np.float32)
        x[r, 13] = -a                                      # a an exact power of two and its two fp32 neighbours
    x[10, :32] = np.float32(1e-45)                         # the smallest subnormal everywhere
    x[11, :32] = np.float32(-3.4028234663852886e38)
    return x


def test_special_values(dev):
    x = _special_rows()
    for elem in ELEMS:
        ordinary = M.fake_quant_mx(x[:1, 32:], 1, elem)[0]
        want = M.fake_quant_mx(x, 1, elem)
        assert np.isnan(want[1:4, :32]).all() and np.array_equal(want[:, 32:], np.tile(ordinary, (12, 1)))
    _check(x, 1, dev, "rows")                              # contiguous blocks
    _check(np.ascontiguousarray(x.T), 0, dev, "columns")   # the same blocks strided, 12 columns (four to a lane; one when misaligned)
    _check(np.ascontiguousarray(x[:11].T), 0, dev, "columns, 11")


# ------------------------------------------------------------------------------------------------ 6. entry points
def test_entry_points(dev):
    import ctypes as C

    import dipoorlet_amd.torch_ops  # noqa: F401
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    x = torch.from_numpy(_data((3, 40, 6), 3)).to(dev)
    y = torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert lib.dpl_fake_quant_mx(2, px, py, 3, 40, 6, None, st) == -2 and b"elem" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx(0, None, py, 3, 40, 6, None, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx(0, px, None, 3, 40, 6, None, st) == -2
    assert lib.dpl_fake_quant_mx(0, px, py, 1, 1 << 31, 1, None, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_fake_quant_mx(0, px, py, 1, 1, 1 << 31, None, st) == -2
    assert lib.dpl_fake_quant_mx(0, px, py, 1 << 40, 1 << 20, 1 << 20, None, st) == -2 and b"too large" in lib.dpl_last_error()
    for zero in ((0, 40, 6), (3, 0, 6), (3, 40, 0)):       # n == 0: a no-op, whatever the pointers
        assert lib.dpl_fake_quant_mx(1, None, None, *zero, None, st) == 0
    assert ops.fake_quant_mx(torch.empty(0, 5, device=dev), 1, "mxfp8").shape == (0, 5)
    for bad in (dict(elem="mxfp6"), dict(axis=3), dict(axis=-4), dict(axis=None)):
        kw = dict(axis=1, elem="mxfp8")
        kw.update(bad)
        with pytest.raises(_hip.DipoorletHipError):
            ops.fake_quant_mx(x, kw["axis"], kw["elem"])
    with pytest.raises(_hip.DipoorletHipError):
        ops.fake_quant_mx(x.transpose(0, 1), 1, "mxfp8")                                   # not contiguous: no silent copy
    with pytest.raises(_hip.DipoorletHipError):
        ops.fake_quant_mx(x.cpu(), 1, "mxfp8")                                             # no CPU path
    with pytest.raises(_hip.DipoorletHipError):
        ops.fake_quant_mx(x, 1, "mxfp8", out=torch.empty(3, 40, 5, device=dev))
    with pytest.raises(_hip.DipoorletHipError, match=r"\[3, 2, 6\]"):
        ops.fake_quant_mx(x, 1, "mxfp8", scales=torch.empty(3 * 6, dtype=torch.uint8, device=dev))
    with pytest.raises(_hip.DipoorletHipError):
        ops.fake_quant_mx(x, 1, "mxfp8", scales=torch.empty(36, dtype=torch.int32, device=dev))
    xh = x.cpu().numpy()
    for elem in ELEMS:
        for axis in (0, 1, 2, -1, -2, -3):
            want, want_s = M.fake_quant_mx(xh, axis, elem, return_scales=True)
            sc = torch.empty(want_s.shape, dtype=torch.uint8, device=dev)
            got = ops.fake_quant_mx(x, axis, elem, scales=sc)
            _same(got.cpu().numpy(), want, (elem, axis))
            assert np.array_equal(sc.cpu().numpy(), want_s)
            _same(torch.ops.dipoorlet.fake_quant_mx(x, axis, elem).cpu().numpy(), want, ("torch op", elem, axis))
        inplace = x.clone()
        assert ops.fake_quant_mx(inplace, 1, elem, out=inplace) is inplace                # out may be x
        _same(inplace.cpu().numpy(), M.fake_quant_mx(xh, 1, elem), ("in place", elem))
    xt = x.transpose(0, 2)              # (the torch op makes its input contiguous, as its siblings do)
    _same(torch.ops.dipoorlet.fake_quant_mx(xt, 1, "mxfp4").cpu().numpy(), M.fake_quant_mx(xt.contiguous().cpu().numpy(), 1, "mxfp4"), "strided")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.ops.dipoorlet.fake_quant_mx(torch.empty(5, 3, 49, device="cuda"), -1, "mxfp8")
        assert tuple(f.shape) == (5, 3, 49) and f.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 7. the mini-ViT
N, IMG = 16, 32


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mx")
    g = models.vit(image=IMG, patch=8, dim=64, depth=2, heads=2, mlp=128, num_classes=10)     # 17 tokens, head dimension 32
    g.output_dir = str(d)
    g.save_onnx_model("vit")
    os.makedirs(d / "calib" / "input")
    rng = np.random.default_rng(12)
    for i in range(N):
        rng.standard_normal(3 * IMG * IMG).astype(np.float32).tofile(d / "calib" / "input" / f"{i}.bin")
    return d


def _args(workdir, out, **kw):
    os.makedirs(out, exist_ok=True)
    a = dict(model=str(workdir / "vit.onnx"), input_dir=str(workdir / "calib"), data_num=N, rank=0, local_rank=0, world_size=1, bins=2048,
             threshold=0.99999, deploy="ocp_fp8", act_quant="minmax", calib_batch=8, output_dir=str(out), skip_layers=[], savefp=False,
             mx=None)
    a.update(kw)
    return types.SimpleNamespace(**a)


@pytest.fixture(scope="module")
def calibrated(workdir, dev):
    """(graph, -A minmax clip ranges, the 16 images): computed once, copied by whoever quantises."""
    from dipoorlet_amd import dist_helper
    from dipoorlet_amd.forward_net import load_input_batch
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    dist_helper.init_default()
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    act, wt = tensor_calibration(g, _args(workdir, workdir / "cal"))
    gc.collect()            # (the calibration run's session and accumulators: cycles)
    x = load_input_batch(str(workdir / "calib"), ["input"], {"input": g.get_tensor_shape("input")}, 0, N, dev)["input"]
    return g, {**act, **wt}, x


def _quantised(calibrated, mx):
    from dipoorlet_amd.quantize import quant_graph
    g, clip, _ = calibrated
    return quant_graph(g, {k: [np.copy(v[0]), np.copy(v[1])] for k, v in clip.items()}, types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx=mx))[0]


@pytest.mark.two_forwards
def test_every_mx_node_of_the_session_equals_the_model(calibrated, dev):
    from dipoorlet_amd.executor import GraphSession
    g, _, x = calibrated
    gq = _quantised(calibrated, "mxfp4")
    mx = [(n, gq._qdq[n.name]) for n in gq.graph.node if n.op_type == "FakeQuant" and gq._qdq[n.name].is_mx]
    consts = [(n, q) for n, q in mx if n.input[0] in g.initializer]
    acts = [(n, q) for n, q in mx if n.input[0] not in g.initializer]
    # per block: qkv, q.k^T (two activations), p.v (two), proj, fc1, fc2 = 4 constant operands and 8 activations; the head: 1 + 1
    assert len(consts) == 2 * 4 + 1 and len(acts) == 2 * 8 + 1 and len(mx) == sum(2 for n in g.graph.node if n.op_type in ("MatMul", "Gemm"))
    assert sorted({q.block_axis for _, q in mx}) == [-2, -1, 1]
    assert any(q.fmt == "Float8E4M3FN" for q in gq._qdq.values())                     # the patch-embedding Conv keeps E4M3
    sess = GraphSession(gq, device=dev, expose_fake_quant=True)
    assert not [k for k in sess.fusion([gq.network_outputs[0]])[0] if gq._qdq[k].is_mx]
    names = [t for n, _ in acts for t in (n.input[0], n.output[0])]
    got = dict(zip(names, sess.run_named({"input": x}, names)))
    k17 = 0
    for n, q in acts:
        xin = got[n.input[0]].cpu().numpy()
        k17 += xin.shape[q.block_axis] == 17
        _same(got[n.output[0]].cpu().numpy(), M.fake_quant_mx(xin, q.block_axis, "mxfp4"), n.name)
    assert k17 == 4                                                                   # softmax rows and V: K = 17 tokens, a short only block
    for n, q in consts:           # folded at session build, each once through its node
        assert n.name in sess._folded
        _same(sess.consts[n.output[0]].cpu().numpy(), M.fake_quant_mx(g.get_initializer(n.input[0]), q.block_axis, "mxfp4"), n.name)
    assert torch.isfinite(sess.run_named({"input": x}, [gq.network_outputs[0]])[0]).all()


@pytest.mark.two_forwards
def test_output_error_orders_the_formats(calibrated, dev):
    """Output MSE against fp32 over the 16 images: above 0 under mxfp8, larger under mxfp4.  No bound is asserted; the values, and
    plain -D ocp_fp8's, are printed (DESIGN section 3j quotes them)."""
    g, _, x = calibrated
    out = g.network_outputs[0]
    fp = g.make_session().run_named({"input": x}, [out])[0]
    mse = {}
    for mx in (None, "mxfp8", "mxfp4"):
        q = _quantised(calibrated, mx).make_session().run_named({"input": x}, [out])[0]
        mse[mx] = float(((fp.double() - q.double()) ** 2).mean())
        print(f"mini-ViT output MSE against fp32, -D ocp_fp8 --mx {mx}: {mse[mx]:.6g} (mean fp32 output^2 {float((fp.double() ** 2).mean()):.6g})")
    assert mse["mxfp8"] > 0
    assert mse["mxfp4"] > mse["mxfp8"]


# ------------------------------------------------------------------------------------------------ 8. CLI
@pytest.mark.two_forwards
def test_cli(workdir):
    from dipoorlet_amd import onnx_io
    out = workdir / "cli_mx"
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "vit.onnx"), "-I", str(workdir / "calib"),
           "-N", str(N), "-A", "hist", "-D", "ocp_fp8", "-O", str(out), "--calib_batch", "8", "--mx", "mxfp4", "--smooth", "--bc"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    for f in ("ocp_fp8_scales.json", "act_clip_val.json", "ocp_mx_blocks.json", "quant_model.onnx", "smooth_model.onnx"):
        assert os.path.exists(out / f), f
    blocks = json.load(open(out / "ocp_mx_blocks.json"))
    assert blocks["format"] == "mxfp4" and blocks["block_size"] == 32
    m = onnx_io.load_model(str(out / "quant_model.onnx"))
    nodes = [n for n in m.nodes if n.op_type == "MXQuantizeDequantize"]
    assert len(nodes) == 26 and m.opset["dipoorlet.amd"] == 1
    assert all(n.domain == "dipoorlet.amd" and n.attrs["block_size"] == 32 and n.attrs["elem_type"] == "float4e2m1" for n in nodes)
    # exactly the MX nodes of the model, with their axes: a key is the tensor's name plus the node's suffix (`_ax<k>` on a second
    # node of one tensor; none here), which is what is left of the node's name without "_QuantizeLinear"
    assert all(n.name.startswith(n.input[0] + "_QuantizeLinear") for n in nodes)
    assert {n.name.replace("_QuantizeLinear", "", 1): n.attrs["axis"] for n in nodes} == {k: v["axis"] for k, v in blocks["tensors"].items()}
    assert {k for k, v in blocks["tensors"].items() if v["constant"]} == {n.input[0] for n in nodes if n.input[0] in m.initializers}
    assert sum(v["constant"] for v in blocks["tensors"].values()) == 9
    assert any(n.op_type == "QuantizeLinear" for n in m.nodes)                        # the Conv's static E4M3 pairs beside them


# ------------------------------------------------------------------------------------------------ 9. every format in one fold
def test_session_folds_weights_of_every_format(dev):
    """A hand-made graph whose four constant weights get a node of every kind: the session's fold (GraphSession._fold_weights) leaves
    each equal, bit for bit, to that node's own apply() — one whole-set launch per static format, the MX weight through none.
    Conv [8, 3, 3, 3] on the integer grid per channel: rows of 27, not a multiple of four (a vector straddles two channels); a
    second integer weight with a single scale, asymmetric; Gemm [6, 10] on FP8 per channel; MatMul [40, 6] on MXFP4 along axis 0:
    one full block and a short one of 8 rows, inner = 6 (the unvectorised column kernel)."""
    from dipoorlet_amd import ops
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.models import _B
    from dipoorlet_amd.platform_settings import mx_setting_table, platform_setting_table
    from dipoorlet_amd.quantize import get_qnode_by_param
    b = _B(31)
    x = b.conv("input", 3, 8, 3, 1, 1, "c1")                        # c1.weight [8, 3, 3, 3]
    x = b.conv(x, 8, 10, 1, 1, 0, "c2")                             # c2.weight [10, 8, 1, 1]
    x = b.node("Flatten", [x], out="flat", axis=1)                  # [1, 10 * 2 * 2]
    b.w("mm.weight", (40, 6))
    x = b.node("MatMul", [x, "mm.weight"], out="mm_out")
    b.w("fc.weight", (6, 10))
    b.b("fc.bias", 10)
    x = b.node("Gemm", [x, "fc.weight", "fc.bias"], out="output", alpha=1.0, beta=1.0, transB=0)
    g = b.finish("input", [1, 3, 2, 2], x)
    params = {"c1.weight": platform_setting_table["trt"]["qw_params"], "c2.weight": platform_setting_table["snpe"]["qw_params"],
              "fc.weight": platform_setting_table["ocp_fp8"]["qw_params"], "mm.weight": mx_setting_table["mxfp4"]}
    for node in list(g.graph.node):
        name = node.input[1] if len(node.input) > 1 else None
        if name not in params:
            continue
        w2 = np.asarray(g.get_initializer(name), np.float64).reshape(g.get_initializer(name).shape[0], -1)
        q, _, _ = get_qnode_by_param(params[name], name, list(g.get_initializer(name).shape), [w2.min(axis=1), w2.max(axis=1)], block_axis=0)
        node.input[1] = q.output
        g.insert_qnodes_purely(q_nodes=q, node=node)
        g.topologize_graph()
    g.update_model()
    qs = {q.tensor_name: q for q in g._qdq.values()}
    assert {k: (q.fmt, q.scale.size) for k, q in qs.items()} == {"c1.weight": ("Linear", 8), "c2.weight": ("Linear", 1),
                                                                 "fc.weight": ("Float8E4M3FN", 6), "mm.weight": ("MXFP4E2M1", 1)}
    assert not qs["c2.weight"].symmetric and qs["c2.weight"].zero_point_as_stored()[0] > 0
    launches, call = [], ops.FakeQuantSet.__call__

    def counted(self, tensors, out=None):
        launches.append((self.fmt, len(tensors)))
        return call(self, tensors, out)
    ops.FakeQuantSet.__call__ = counted
    try:
        sess = GraphSession(g, device=dev)
    finally:
        ops.FakeQuantSet.__call__ = call
    assert sorted(launches) == [("fp8", 1), ("int", 2)]              # one per static format present; the MX weight in neither
    assert len(sess._folded) == 4
    for node in g.graph.node:
        if node.op_type != "FakeQuant":
            continue
        q, w = g._qdq[node.name], sess.consts[node.input[0]]
        assert node.name in sess._folded and tuple(w.shape) == tuple(g.get_initializer(node.input[0]).shape)
        one = q.apply(w.contiguous())
        assert torch.equal(sess.consts[node.output[0]], one), node.name
        assert not torch.equal(one, w), node.name                      # (the node does round)
    _same(sess.consts["mm.weight_dq"].cpu().numpy(), M.fake_quant_mx(g.get_initializer("mm.weight"), 0, "mxfp4"), "mm.weight")
    assert torch.isfinite(sess.run({"input": torch.ones(1, 3, 2, 2, device=dev)})[-1]).all()
