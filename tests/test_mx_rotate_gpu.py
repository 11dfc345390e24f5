"""GPU: `--mx_rotate` — the block-Hadamard kernel (k_hadamard32, dpl_hadamard32) against the numpy definition
(tests/mx_rotate_model.py fwht32) bit for bit, its composition with the MX Q/DQ kernel, and the rotation from the graph session up
to the CLI.  A workgroup covers 128 blocks of 32 on the 16-byte path (both bases aligned) and 32 on the element path; the shapes
are the smallest that reach one block, one workgroup's share less one, exactly and plus one on either path, several workgroups,
and a share that ends inside a row."""
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
import mx_rotate_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMS = ("mxfp8", "mxfp4")
GUARD = 8
U = 2.0 ** -24            # fp32's unit roundoff


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _leave_no_device_memory_in_cycles():
    """As tests/test_mx_gpu.py: sessions and calibration runs hold device tensors in reference cycles; every test ends with a pass of
    the cycle collector."""
    yield
    gc.collect()


def _data(shape, seed):
    """Magnitudes 2^-60 .. 2^60 (no stage of the butterfly can produce a non-zero fp32 subnormal: the smallest non-zero difference
    of two such values is 2^-84), a few exact zeros of both signs."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(1.0, 2.0, shape) * rng.choice([-1.0, 1.0], shape) * np.exp2(rng.integers(-60, 60, shape))).astype(np.float32)
    flat = x.reshape(-1)
    flat[::37] = 0.0
    flat[5::91] = -0.0
    return x


def _same(got, want, what):
    """The same 32 bits wherever the value is no NaN, NaN in the same places."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32))))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _run(x, dev, misaligned=False, inplace=False):
    """ops.hadamard32 on a copy of x whose base is 16-byte aligned, or one float off -> y on the host; the floats around the output
    must come back untouched."""
    from dipoorlet_amd import ops
    off = 1 if misaligned else 0
    n = x.size
    bx = torch.zeros(n + 2 * GUARD + off, dtype=torch.float32, device=dev)
    by = bx if inplace else torch.full((n + 2 * GUARD + off,), -77.0, dtype=torch.float32, device=dev)
    if inplace:
        bx.fill_(-77.0)
    xv, yv = bx[GUARD + off:GUARD + off + n].view(x.shape), by[GUARD + off:GUARD + off + n].view(x.shape)
    assert xv.data_ptr() % 16 == 4 * off and yv.data_ptr() % 16 == 4 * off
    xv.copy_(torch.from_numpy(x))
    ret = ops.hadamard32(xv, out=yv)
    assert ret is yv
    hy = by.cpu().numpy()
    assert (hy[:GUARD + off] == -77.0).all() and (hy[GUARD + off + n:] == -77.0).all(), "written outside y"
    if not inplace:
        _same(xv.cpu().numpy(), x, "the input was written")
    return hy[GUARD + off:GUARD + off + n].reshape(x.shape)


# ------------------------------------------------------------------------------------------------ 1. the kernel against the model
# (rows, k) -> blocks: 1 | 31, 32, 33 (the element path's share -1, =, +1) | 127, 128, 129 (the 16-byte path's) | the same counts
# from rows of 2 and 3 blocks, where 11 x 3 = 33 and 43 x 3 = 129 end a workgroup's share inside a row | several workgroups
SHAPES = [(1, 32), (31, 32), (32, 32), (33, 32), (127, 32), (128, 32), (129, 32), (16, 64), (64, 64), (11, 96), (43, 96), (300, 96),
          (2, 3072), (5, 3072)]


@pytest.mark.parametrize("rows,k", SHAPES)
def test_kernel_equals_the_model(dev, rows, k):
    x = _data((rows, k), 1000 * rows + k)
    want = R.fwht32(x)
    assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= 2.0 ** -126).all()      # (the inputs keep every stage normal)
    for mis in (False, True):
        _same(_run(x, dev, mis), want, (rows, k, mis))
        _same(_run(x, dev, mis, inplace=True), want, (rows, k, mis, "in place"))


def _special_rows():
    """[4, 96]: block 1 of rows 0 .. 2 and block 2 of row 3 are special, everything else ordinary."""
    x = _data((4, 96), 9)
    x[0, 40] = np.nan
    x[1, 35], x[1, 60] = np.inf, -np.inf
    x[2, 32:64] = -0.0                                    # all -0: element 0 of the rotated block stays -0, the others are x - x = +0
    x[3, 64:96] = 0.0
    x[3, 65:96:2] = -0.0                                  # zeros of both signs: +0 everywhere
    return x


def test_special_values(dev):
    import dipoorlet_amd.torch_ops  # noqa: F401
    x = _special_rows()
    want = R.fwht32(x)
    assert np.isnan(want[0, 32:64]).all() and np.isfinite(want[0, :32]).all() and np.isfinite(want[0, 64:]).all()
    assert not np.isfinite(want[1, 32:64]).any() and np.isnan(want[1, 32:64]).any() and np.isfinite(want[3]).all()
    assert (want[2, 32:64] == 0).all() and np.signbit(want[2, 32:64]).tolist() == [True] + 31 * [False]
    assert (want[3, 64:96] == 0).all() and not np.signbit(want[3, 64:96]).any()
    for mis in (False, True):
        _same(_run(x, dev, mis), want, ("special", mis))
        _same(_run(x, dev, mis, inplace=True), want, ("special, in place", mis))
    _same(torch.ops.dipoorlet.hadamard32(torch.from_numpy(x).to(dev)).cpu().numpy(), want, "torch op")
    x3 = _data((3, 7, 64), 4)                            # any rank: the last axis
    _same(torch.ops.dipoorlet.hadamard32(torch.from_numpy(x3).to(dev)).cpu().numpy(), R.fwht32(x3), "torch op, 3 axes")


# ------------------------------------------------------------------------------------------------ 2. entry points
def test_entry_points(dev):
    import ctypes as C

    import dipoorlet_amd.torch_ops  # noqa: F401
    from dipoorlet_amd import _hip, ops
    lib = _hip.lib()
    x = torch.from_numpy(_data((6, 64), 3)).to(dev)
    y = torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert lib.dpl_hadamard32(None, py, 6, 64, st) == -2 and b"null" in lib.dpl_last_error()
    assert lib.dpl_hadamard32(px, None, 6, 64, st) == -2
    assert lib.dpl_hadamard32(px, py, 8, 48, st) == -2 and b"multiple of 32" in lib.dpl_last_error()
    assert lib.dpl_hadamard32(px, py, 1, 1 << 31, st) == -2 and b"2^31" in lib.dpl_last_error()
    assert lib.dpl_hadamard32(px, py, 1 << 40, 1 << 30, st) == -2 and b"too large" in lib.dpl_last_error()     # 2^33 workgroups
    assert lib.dpl_hadamard32(px, py, 1 << 62, 64, st) == -2 and b"too large" in lib.dpl_last_error()          # rows * k overflows
    for zero in ((0, 64), (6, 0)):                        # n == 0: a no-op, whatever the pointers
        assert lib.dpl_hadamard32(None, None, *zero, st) == 0
    torch.cuda.synchronize()
    assert ops.hadamard32(torch.empty(0, 64, device=dev)).shape == (0, 64)
    assert ops.hadamard32(torch.empty(5, 0, device=dev)).shape == (5, 0)
    for bad in (torch.zeros(4, 48, device=dev),                                           # k = 48
                torch.zeros(64, 6, device=dev).t(),                                       # not contiguous: no silent copy
                torch.zeros(4, 64),                                                       # no CPU path
                torch.zeros(4, 64, device=dev, dtype=torch.float16),
                torch.zeros((), device=dev)):
        with pytest.raises(_hip.DipoorletHipError):
            ops.hadamard32(bad)
    with pytest.raises(_hip.DipoorletHipError):
        ops.hadamard32(x, out=torch.empty(6, 32, device=dev))
    with pytest.raises(_hip.DipoorletHipError):
        ops.hadamard32(x, out=torch.empty(6, 64))
    xt = torch.from_numpy(_data((64, 6), 5)).to(dev).t()   # (the torch op makes its input contiguous, as its siblings do)
    _same(torch.ops.dipoorlet.hadamard32(xt).cpu().numpy(), R.fwht32(xt.contiguous().cpu().numpy()), "strided")
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        f = torch.ops.dipoorlet.hadamard32(torch.empty(5, 3, 64, device="cuda"))
        assert tuple(f.shape) == (5, 3, 64) and f.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 3. composition with the MX pair
def test_rotation_then_mx_equals_the_models(dev):
    from dipoorlet_amd import ops
    rng = np.random.default_rng(11)
    x = rng.standard_normal((37, 96)).astype(np.float32)
    x[:, 5] *= 30.0
    x = np.concatenate([x, _special_rows()])
    xd = torch.from_numpy(x).to(dev)
    for elem in ELEMS:
        want, want_s = M.fake_quant_mx(R.fwht32(x), -1, elem, return_scales=True)
        sc = torch.empty(want_s.shape, dtype=torch.uint8, device=dev)
        got = ops.fake_quant_mx(ops.hadamard32(xd), -1, elem, scales=sc)
        _same(got.cpu().numpy(), want, elem)
        assert np.array_equal(sc.cpu().numpy(), want_s), elem
        assert (want_s.reshape(x.shape[0], 3)[37:39, 1] == 0xFF).all()      # the NaN and the inf block: scale code 0xFF


# ------------------------------------------------------------------------------------------------ 4. a one-MatMul graph, exactly
def test_session_keeps_an_integer_product_exactly(dev):
    from dipoorlet_amd import onnx_io
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.onnx_io import Node
    from dipoorlet_amd.weight_transform.rotate import apply_rotate, find_rotate_sites
    rng = np.random.default_rng(1)
    x = rng.integers(-8, 9, (7, 96)).astype(np.float32)
    w = (32 * rng.integers(-4, 5, (96, 10))).astype(np.float32)
    m = onnx_io.Model()
    m.nodes, m.initializers = [Node("MatMul", ["x", "w"], ["y"], name="mm")], {"w": w}
    m.inputs, m.outputs = [("x", onnx_io.FLOAT, [7, 96])], [("y", onnx_io.FLOAT, None)]
    g = ONNXGraph(m)
    sites, left = find_rotate_sites(g)
    assert len(sites) == 1 and not left
    gr = apply_rotate(g, sites)
    xd = torch.from_numpy(x).to(dev)
    y0 = GraphSession(g, device=dev).run_named({"x": xd}, ["y"])[0].cpu().numpy()
    xr, y1 = (t.cpu().numpy() for t in GraphSession(gr, device=dev).run_named({"x": xd}, ["x_rot", "y"]))
    want = x.astype(np.float64) @ w.astype(np.float64)              # every partial sum is an integer below 2^24
    assert np.array_equal(xr, R.fwht32(x)) and not np.array_equal(xr, x)
    assert np.array_equal(y0, want) and np.array_equal(y1, want)


# ------------------------------------------------------------------------------------------------ 5. / 6. the mini-ViT
N, IMG = 16, 32


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    from dipoorlet_amd import models
    d = tmp_path_factory.mktemp("mx_rotate")
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
def rotated(workdir, dev):
    """(graph, the graph reloaded from rotate_model.onnx, the sites, the 16 images): built once."""
    from dipoorlet_amd import dist_helper
    from dipoorlet_amd.forward_net import load_input_batch
    from dipoorlet_amd.graph import ONNXGraph
    from dipoorlet_amd.weight_transform.rotate import find_rotate_sites, mx_rotate
    dist_helper.init_default()
    g = ONNXGraph.load(str(workdir / "vit.onnx"))
    sites, left = find_rotate_sites(g)
    assert mx_rotate(g, _args(workdir, workdir / "rot")) is not g
    gr = ONNXGraph.load(str(workdir / "rot" / "rotate_model.onnx"))
    x = load_input_batch(str(workdir / "calib"), ["input"], {"input": g.get_tensor_shape("input")}, 0, N, dev)["input"]
    return g, gr, sites, left, x


def _block_sums_bound(t, w, axis, K):
    """(K + 12) u sum_b (sum_{k in b} |t_ik|) (sum_{k in b} |w_kj|): what fp32 may add to a rotated product.  Inside block b every
    exact rotated value is at most s_b = sum |t_ik| (and sum |w_kj| / 32 on the other side), the five roundings of a butterfly
    perturb each by at most gamma_5 times that sum, and a K-term fp32 dot product — in any order, fused or not — by gamma_K times the
    sum of |products|, which is at most 32 s_b (sum |w_kj| / 32) per block."""
    w = np.abs(np.asarray(w, np.float64))
    w = w.T if axis == 1 else w                                              # [K, N]
    tb = np.abs(t.astype(np.float64)).reshape(-1, K // 32, 32).sum(-1)       # [M, blocks]
    wb = w.reshape(K // 32, 32, -1).sum(1)                                   # [blocks, N]
    return (K + 12) * U * (tb @ wb)


@pytest.mark.two_forwards
def test_fp32_forward_of_the_rotated_vit(rotated, dev):
    """Every MatMul / Gemm with a constant right operand is a site; each rotated site's fp32 output lies within the fp32 bound of
    _block_sums_bound of the fp64 product of ITS OWN input with the ORIGINAL weight; the network output stays within 1e-4 max |y|
    of the original's — the bound tests/test_smooth_model.py accepts between two mathematically equal fp32 forms of this network (a
    wrong fold errs at order 1) —; two forwards of the rotated session are bit-identical."""
    from dipoorlet_amd.executor import GraphSession
    g, gr, sites, left, x = rotated
    const_right = [n for n in g.graph.node if n.op_type in ("MatMul", "Gemm") and n.input[1] in g.initializer]
    assert [s.node for s in sites] == [n.name for n in const_right] and len(sites) > 0
    assert sorted({s.K for s in sites}) == [64, 128]
    assert {n for n, _ in left} == {n.name for n in g.graph.node if n.op_type in ("MatMul", "Gemm")} - {s.node for s in sites}
    had = [n for n in gr.graph.node if n.op_type == "BlockHadamard"]
    assert len(had) == len({s.activation for s in sites}) and all(n.domain == "dipoorlet.amd" for n in had)
    changed = [k for k in g.initializer if not np.array_equal(g.get_initializer(k), gr.get_initializer(k))]
    assert sorted(changed) == sorted(s.weight for s in sites) and len(set(changed)) == len(sites)
    sess = GraphSession(gr, device=dev)
    by = {n.name: n for n in gr.graph.node}
    names = [t for s in sites for t in (s.activation, s.activation + "_rot", by[s.node].output[0])]
    got = dict(zip(names, (t.cpu().numpy() for t in sess.run_named({"input": x}, names))))
    worst = 0.0
    for s in sites:
        node, t = by[s.node], got[s.activation]
        _same(got[s.activation + "_rot"], R.fwht32(t), s.node)
        w0 = np.asarray(g.get_initializer(s.weight), np.float64)
        t2 = t.reshape(-1, s.K)
        ref = t2.astype(np.float64) @ (w0.T if s.axis == 1 else w0)
        bound = _block_sums_bound(t2, w0, s.axis, s.K)
        if node.op_type == "Gemm":
            assert node.attrs.get("alpha", 1.0) == 1.0 and node.attrs.get("beta", 1.0) == 1.0
            if len(node.input) > 2 and node.input[2]:
                b = np.asarray(g.get_initializer(node.input[2]), np.float64)
                ref = ref + b
                bound = bound + 2 * U * (np.abs(ref) + np.abs(b))
        err = np.abs(got[node.output[0]].reshape(ref.shape).astype(np.float64) - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (s.node, float((err / bound).max()))
        assert err.max() < 1e-3 * np.abs(ref).max(), s.node                  # (the bound cannot hide a wrong fold: that errs at order 1)
    out = g.network_outputs[0]
    y0 = GraphSession(g, device=dev).run_named({"input": x}, [out])[0]
    y1 = sess.run_named({"input": x}, [out])[0]
    e2e = float((y1 - y0).abs().max() / y0.abs().max())
    print(f"rotated mini-ViT, fp32: largest site error {worst:.4f} of its bound; output max |diff| / max |y| = {e2e:.3g} (allowed 1e-4)")
    assert torch.isfinite(y1).all() and e2e <= 1e-4
    assert torch.equal(sess.run_named({"input": x}, [out])[0], y1)           # DPL_DETERMINISTIC: bit-identical


@pytest.mark.two_forwards
def test_fake_quantised_forward_of_the_rotated_vit(workdir, rotated, dev):
    """--mx mxfp4 on the rotated graph: every MX node that reads a rotated tensor equals the model on the BlockHadamard output the
    session exposes.  Output MSE against fp32, with and without the rotation: printed, finite and > 0 (random weights: no
    direction is claimed)."""
    from dipoorlet_amd.executor import GraphSession
    from dipoorlet_amd.quantize import quant_graph
    from dipoorlet_amd.tensor_cali import tensor_calibration
    g, gr, sites, _, x = rotated
    out = g.network_outputs[0]
    fp = g.make_session().run_named({"input": x}, [out])[0]
    qargs = types.SimpleNamespace(deploy="ocp_fp8", skip_layers=[], mx="mxfp4")
    mse = {}
    for name, graph in (("plain", g), ("rotated", gr)):
        act, wt = tensor_calibration(graph, _args(workdir, workdir / ("cal_" + name)))
        gc.collect()
        if graph is gr:
            assert all(s.activation + "_rot" in act for s in sites)
        gq = quant_graph(graph, {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act, **wt}.items()}, qargs)[0]
        if graph is gr:
            rot = {s.activation + "_rot" for s in sites}
            nodes = [n for n in gq.graph.node if n.op_type == "FakeQuant" and n.input[0] in rot]
            assert len(nodes) == len(rot) and all(gq._qdq[n.name].is_mx and gq._qdq[n.name].block_axis in (-1, 1) for n in nodes)
            sess = GraphSession(gq, device=dev, expose_fake_quant=True)
            names = [t for n in nodes for t in (n.input[0], n.output[0])]
            got = dict(zip(names, sess.run_named({"input": x}, names)))
            for n in nodes:
                xin = got[n.input[0]].cpu().numpy()
                assert gq.get_tensor_producer(n.input[0]).op_type == "BlockHadamard"
                _same(got[n.output[0]].cpu().numpy(), M.fake_quant_mx(xin, -1, "mxfp4"), n.name)
        q = gq.make_session().run_named({"input": x}, [out])[0]
        mse[name] = float(((fp.double() - q.double()) ** 2).mean())
        print(f"mini-ViT output MSE against fp32, -D ocp_fp8 --mx mxfp4, {name}: {mse[name]:.6g}")
        assert np.isfinite(mse[name]) and mse[name] > 0


# ------------------------------------------------------------------------------------------------ 7. CLI
def _cli(workdir, out, *extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "dipoorlet_amd", "-M", str(workdir / "vit.onnx"), "-I", str(workdir / "calib"),
           "-N", str(N), "-A", "hist", "-D", "ocp_fp8", "-O", str(out), "--calib_batch", "8", "--mx", "mxfp4", *extra, "--smooth", "--bc"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


@pytest.mark.two_forwards
def test_cli(workdir):
    from dipoorlet_amd import onnx_io
    out = workdir / "cli_rot"
    log = _cli(workdir, out, "--mx_rotate")
    for f in ("smooth_model.onnx", "rotate_model.onnx", "rotate_report.json", "quant_model.onnx", "ocp_mx_blocks.json", "act_clip_val.json",
              "update_bias_model.onnx"):
        assert os.path.exists(out / f), f
    rep = json.load(open(out / "rotate_report.json"))
    src = onnx_io.load_model(str(out / "smooth_model.onnx"))
    const_right = [n.name for n in src.nodes if n.op_type in ("MatMul", "Gemm") and n.input[1] in src.initializers]
    assert [r["node"] for r in rep["rotated"]] == const_right and const_right
    assert {e["node"] for e in rep["left"]} == {n.name for n in src.nodes if n.op_type in ("MatMul", "Gemm")} - set(const_right)
    assert all(e["why"] for e in rep["left"]) and all(r["K"] in (64, 128) for r in rep["rotated"])
    acts, weights = sorted({r["activation"] for r in rep["rotated"]}), sorted(r["weight"] for r in rep["rotated"])
    assert "MX rotate: {} node(s) rotated over {} activation(s)".format(len(const_right), len(acts)) in log
    m = onnx_io.load_model(str(out / "quant_model.onnx"))
    assert m.opset["dipoorlet.amd"] == 1
    had = {n.output[0]: n for n in m.nodes if n.op_type == "BlockHadamard"}
    assert sorted(had) == acts and all(n.domain == "dipoorlet.amd" and n.attrs["block_size"] == 32 for n in had.values())
    mxq = [n for n in m.nodes if n.op_type == "MXQuantizeDequantize" and n.input[0] in had]
    assert sorted(n.input[0] for n in mxq) == acts                  # ONE BlockHadamard in front of the MX node of every rotated activation
    order = {n.name: i for i, n in enumerate(m.nodes)}
    assert all(order[had[n.input[0]].name] < order[n.name] for n in mxq)
    blocks = json.load(open(out / "ocp_mx_blocks.json"))
    assert blocks["rotation"] == {"block_size": 32, "activations": blocks["rotation"]["activations"], "weights": blocks["rotation"]["weights"]}
    assert sorted(blocks["rotation"]["activations"]) == acts and sorted(blocks["rotation"]["weights"]) == weights
    assert all(a in blocks["tensors"] and not blocks["tensors"][a]["constant"] for a in acts)
    assert all(blocks["tensors"][w]["constant"] for w in weights)
    clip = json.load(open(out / "act_clip_val.json"))
    assert all(a in clip for a in acts)
    # the same command without the flag: no rotate_* file, no "rotation" key
    out0 = workdir / "cli_plain"
    _cli(workdir, out0)
    assert not [f for f in os.listdir(out0) if f.startswith("rotate")]
    blocks0 = json.load(open(out0 / "ocp_mx_blocks.json"))
    assert "rotation" not in blocks0 and not any(k.endswith("_rot") for k in blocks0["tensors"])
    assert not any(n.op_type == "BlockHadamard" for n in onnx_io.load_model(str(out0 / "quant_model.onnx")).nodes)
