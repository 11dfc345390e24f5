"""Replay of a saved Q/DQ model — the file a user deploys, written by graph.to_model / insert_qnodes_purely — against the session
that produced it, node by node, through tests/onnx_ref.py.

replay(path, fetch) loads the file and walks its nodes in file order.  A node's inputs are taken by the names the FILE gives:
initializers from the file, activations from fetch(name), the device session's own tensor of that name (a numpy array) — so every
node is checked on its own and a rounding flip upstream does not propagate.  A QuantizeLinear whose output feeds only its
DequantizeLinear is evaluated as the pair (the session has no <t>_q tensor).  Nothing is skipped: an operator without a REF entry,
or a name the session does not have, is an AssertionError.

check(nodes, fetch, device_type) then holds the session to what the file defines:
  * every output of a DequantizeLinear / MXQuantizeDequantize / BlockHadamard node: bit for bit (uint32 views, NaN in the same places);
  * every other node: the bound op_bounds gives its kind (KIND below: exact, trans, sum / conv with K the reduction length).
negative_control(node, nodes, fetch, device_type): the same node evaluated with its activation read from <t> instead of <t>_dq —
the session's output must then VIOLATE the node's bound, or the bound could hide a missing pair.
"""
import numpy as np

import onnx_ref
from dipoorlet_amd import onnx_io
from onnx_ref import REF
from op_bounds import Case, _bound, _check

QDQ = ("QuantizeLinear", "DequantizeLinear")
BITWISE = ("DequantizeLinear", "MXQuantizeDequantize", "BlockHadamard")
# the kind of bound per operator, as test_executor_ops_onnx.py's cases give it (operators whose kind depends on an attribute —
# Resize, the reductions — are not listed: a file that holds one fails until it is)
KIND = {"Conv": "conv", "ConvTranspose": "conv", "Gemm": "sum", "MatMul": "sum", "AveragePool": "sum", "GlobalAveragePool": "sum"}
KIND.update({op: "exact" for op in ("Relu", "MaxPool", "GlobalMaxPool", "Flatten", "Reshape", "Transpose", "Concat", "Split", "Slice", "Gather",
                                    "Squeeze", "Unsqueeze", "Expand", "Clip", "Abs", "Neg", "Identity", "Pad", "Where") + QDQ + BITWISE})
KIND.update({op: "trans" for op in ("Add", "Sub", "Mul", "Div", "Eltwise", "Sigmoid", "Tanh", "HardSigmoid", "HardSwish", "Erf", "Exp", "Log",
                                    "Sqrt", "Pow", "Reciprocal", "Gelu", "PRelu", "LeakyRelu", "Softmax", "BatchNormalization",
                                    "LayerNormalization", "InstanceNormalization")})


class NodeResult:
    """One node of the file: `inputs` as it was evaluated ({name: array}, in input order), `y` (list) and `aux` as REF defines them,
    `codes` (the pair's quantised tensor, for a DequantizeLinear), `source` (a pair's / MX node's unquantised input name), `weight`
    (that source is an initializer of the file)."""

    def __init__(self, node, opset, inputs, y, aux, codes=None, source=None, weight=False):
        self.node, self.opset, self.inputs, self.y, self.aux, self.codes, self.source = node, opset, inputs, y, aux, codes, source
        self.weight = weight

    @property
    def id(self):
        return f"{self.node.op_type}:{self.node.name}"


def _from_file(arr):
    """An initializer as the reference takes it: a float8e4m3fn tensor becomes onnx_ref's type for it."""
    return onnx_ref.Float8E4M3FN(np.asarray(arr).view(np.uint8)) if isinstance(arr, onnx_io.Float8E4M3FNBytes) else np.asarray(arr)


def reduction_length(node, inputs):
    """K of a sum / conv kind: the number of products added up per output."""
    arrs = list(inputs.values())
    if node.op_type == "Conv":
        return int(np.prod(arrs[1].shape[1:]))
    if node.op_type == "ConvTranspose":
        w = arrs[1]
        return (w.shape[0] // int(node.attrs.get("group", 1))) * int(np.prod(w.shape[2:]))
    if node.op_type == "Gemm":
        a = arrs[0]
        return int(a.shape[0] if node.attrs.get("transA", 0) else a.shape[1])
    if node.op_type == "MatMul":
        return int(arrs[0].shape[-1])
    if node.op_type == "AveragePool":
        return int(np.prod(node.attrs["kernel_shape"]))
    if node.op_type == "GlobalAveragePool":
        return int(np.prod(arrs[0].shape[2:]))
    return 0


def _evaluate(node, opset, inputs):
    args = [None if n == "" else inputs[n] for n in node.input]
    while args and args[-1] is None:
        args.pop()
    y, aux = REF[node.op_type](args, node.attrs, opset)
    return (list(y) if isinstance(y, list) else [y]), aux


def replay(model_path, fetch):
    """-> [NodeResult] for every node of the file but the QuantizeLinear halves of the pairs (their codes are on the pair's
    DequantizeLinear result)."""
    m = onnx_io.load_model(str(model_path))
    opset = int(m.opset.get("", 13))
    init = {k: _from_file(v) for k, v in m.initializers.items()}
    unsupported = sorted({(n.domain, n.op_type) for n in m.nodes if n.op_type not in REF or n.op_type not in KIND})
    assert not unsupported, f"{model_path}: {len(unsupported)} operator(s) without a definition in onnx_ref / a kind of bound: {unsupported}"
    readers = {}
    for n in m.nodes:
        for i in n.input:
            readers.setdefault(i, []).append(n)
    declared_out = {o for o, _, _ in m.outputs}

    def take(node, name):
        if name in init:
            return init[name]
        try:
            return np.asarray(fetch(name))
        except KeyError:
            raise AssertionError(f"{node.op_type}:{node.name} reads {name!r}: neither an initializer of the file nor a tensor of the session")

    results, pending = [], {}
    for node in m.nodes:
        if node.op_type == "QuantizeLinear":
            r = readers.get(node.output[0], [])
            if len(r) == 1 and r[0].op_type == "DequantizeLinear" and r[0].input[0] == node.output[0] and node.output[0] not in declared_out:
                inputs = {n: take(node, n) for n in node.input if n != ""}
                y, _ = _evaluate(node, opset, inputs)
                pending[node.output[0]] = (node, inputs, y[0])
                continue
        inputs, codes, source = {}, None, None
        for n in node.input:
            if n == "":
                continue
            if n in pending:
                qn, q_in, codes = pending.pop(n)
                assert node.op_type == "DequantizeLinear" and list(node.input[1:]) == list(qn.input[1:]) and node.attrs == qn.attrs, \
                    f"{node.name}: does not dequantise with the scale, zero point and axis {qn.name} quantised with"
                inputs[n], source = codes, qn.input[0]
            else:
                inputs[n] = take(node, n)
        if node.op_type == "MXQuantizeDequantize":
            source = node.input[0]
        y, aux = _evaluate(node, opset, inputs)
        results.append(NodeResult(node, opset, {k: v for k, v in inputs.items() if k in node.input}, y, aux, codes, source,
                                  source in init))
    assert not pending, f"quantised tensors nothing dequantises: {sorted(pending)}"
    return results


def same_bits(got, want):
    """fp32 arrays equal bit for bit, a NaN required where the other has one (the payloads of NaNs are not compared)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all() and (got.view(np.uint32)[~gn] == want.view(np.uint32)[~wn]).all())


def _case(res):
    kind = KIND[res.node.op_type]
    return Case(res.id, res.node.op_type, [], res.node.attrs, opset=res.opset, kind=kind,
                K=reduction_length(res.node, res.inputs) if kind in ("sum", "conv") else 0)


def _session_outputs(res, fetch):
    out = []
    for o in res.node.output:
        try:
            out.append(np.asarray(fetch(o)))
        except KeyError:
            raise AssertionError(f"{res.id} writes {o!r}, which the session does not have")
    return out


def check(results, fetch, device_type):
    """Every node of the replay against the session.  -> {'bitwise': number of tensors found equal bit for bit, 'worst': {op type:
    the largest error inside the bound, in the bound's units}, 'failures': [what every node that failed said]} — the caller asserts
    that 'failures' is empty, after whatever else it wants to look at."""
    failures, worst, bitwise = [], {}, 0
    for res in results:
        got = _session_outputs(res, fetch)
        try:
            if res.node.op_type in BITWISE:
                for o, g, r in zip(res.node.output, got, res.y):
                    assert tuple(g.shape) == tuple(r.shape), f"{res.id}: {o} has shape {g.shape}, the file defines {r.shape}"
                    if not same_bits(g, r):
                        bad = ~((g == r) | (np.isnan(g) & np.isnan(r))) | (np.signbit(g) != np.signbit(r))
                        k = tuple(int(i) for i in np.argwhere(bad)[0])
                        raise AssertionError(f"{res.id}: {o} differs from the file's definition in {int(bad.sum())} of {g.size} elements; "
                                             f"first at {k}: session {g[k]!r}, file {r[k]!r}")
                    bitwise += 1
                continue
            c = _case(res)
            w = _check(c, got, res.y, res.aux, device_type)
            worst[c.op] = max(worst.get(c.op, 0.0), w)
        except AssertionError as e:
            failures.append(str(e))
    return {"bitwise": bitwise, "worst": worst, "failures": failures}


def negative_control(res, results, fetch, device_type):
    """`res` (a Conv / Gemm / MatMul whose operand 0 is a pair's output) evaluated again reading the pair's SOURCE: the session's
    output must be outside the node's bound somewhere.  -> the fraction of outputs outside it."""
    name = res.node.input[0]
    pair = next((r for r in results if name in r.node.output and r.source is not None), None)
    assert pair is not None, f"{res.id}: operand 0 ({name}) is not the output of a Q/DQ pair or an MX node"
    inputs = dict(res.inputs)
    inputs[name] = np.asarray(fetch(pair.source))
    y, aux = _evaluate(res.node, res.opset, inputs)
    c = _case(res)
    assert c.kind in ("sum", "conv")
    outside = 0.0
    for g, r in zip(_session_outputs(res, fetch), y):
        bound, _ = _bound(c, r, aux, device_type)
        outside = max(outside, float((np.abs(g.astype(np.float64) - r) > bound).mean()))
    assert outside > 0.0, f"{res.id}: reading {pair.source} instead of {name} stays inside the bound: the bound could hide a missing pair"
    return outside


def saturation_census(results):
    """Over the ACTIVATION pairs and MX nodes (source no initializer), on the reference's own codes: how many have at least one
    element at the lowest / at the highest code of their grid.  -> (pairs, at the lower end, at the upper end)."""
    n = lo = hi = 0
    for res in results:
        if res.source is None or res.weight:
            continue
        if res.node.op_type == "DequantizeLinear":
            q = res.codes
            if isinstance(q, onnx_ref.Float8E4M3FN):
                v = onnx_ref.e4m3fn_decode(q)
                at_lo, at_hi = (v == -448.0).any(), (v == 448.0).any()
            else:
                info = np.iinfo(q.dtype)
                at_lo, at_hi = (q == info.min).any(), (q == info.max).any()
        elif res.node.op_type == "MXQuantizeDequantize":
            import mx_model
            elem = onnx_ref._MX_ELEM[res.node.attrs["elem_type"]]
            x = res.y[0]
            axis = int(res.node.attrs["axis"]) % x.ndim
            x3 = x.reshape(int(np.prod(x.shape[:axis], dtype=np.int64)), x.shape[axis], -1).astype(np.float64)
            se = np.repeat(res.aux["scales"].astype(np.int64) - 127, mx_model.BLOCK, axis=1)[:, :x.shape[axis], :]
            v = x3 / np.ldexp(1.0, se)                      # the element codes' values
            top = mx_model.ELEM_MAX[elem]
            at_lo, at_hi = (v == -top).any(), (v == top).any()
        else:
            continue
        n, lo, hi = n + 1, lo + bool(at_lo), hi + bool(at_hi)
    return n, lo, hi


# ------------------------------------------------------------------------------------------------ the networks of the replay tests
IMG, N_CALIB, N_REPLAY = 12, 8, 2
SEQ, DIM, HID, OUT = 5, 48, 64, 10
# The replay images are the calibration distribution times this factor: minmax ranges of 8 x 432 standard-normal values end near
# +-3.5 sigma, so about one value in 12 of a replay image lies beyond them on either side — the input pair saturates at both ends
# in every case, and what follows it is wider than calibrated too.
REPLAY_SCALE = 2.0


def build_conv_net(trans_b):
    """input [1, 3, 12, 12] -> Conv 3->8 3x3 (weight rows of 27) -> ReLU -> Conv 8->8 3x3 -> Add (residual) -> ReLU -> ConvTranspose 8->6 2x2
    stride 2 (output channels on axis 1) -> MaxPool 4 -> Flatten -> Gemm 216->10, its weight [10, 216] (transB = 1) or the same
    matrix as [216, 10]."""
    from dipoorlet_amd.models import _B
    g = _B(23)
    r1 = g.node("Relu", [g.conv("input", 3, 8, 3, 1, 1, "c1")], out="r1")
    c2 = g.conv(r1, 8, 8, 3, 1, 1, "c2")
    r2 = g.node("Relu", [g.node("Add", [c2, r1], out="add")], out="r2")
    g.w("ct.weight", (8, 6, 2, 2))
    g.b("ct.bias", 6)
    x = g.node("ConvTranspose", [r2, "ct.weight", "ct.bias"], out="ct_out", kernel_shape=[2, 2], strides=[2, 2], pads=[0, 0, 0, 0],
               dilations=[1, 1], group=1)
    x = g.node("MaxPool", [x], out="pool", ceil_mode=0, kernel_shape=[4, 4], pads=[0, 0, 0, 0], strides=[4, 4])
    x = g.node("Flatten", [x], out="flat", axis=1)
    g.w("fc.weight", (OUT, 6 * 6 * 6))
    if not trans_b:
        g.const("fc.weight", np.ascontiguousarray(g.init["fc.weight"].T))
    g.b("fc.bias", OUT)
    x = g.node("Gemm", [x, "fc.weight", "fc.bias"], out="output", alpha=1.0, beta=1.0, transB=int(trans_b))
    return g.finish("input", [1, 3, IMG, IMG], x)


def build_matmul_net():
    """input [1, 5, 48] -> Mul gamma -> Add beta (a LayerNorm's affine: a --smooth site) -> MatMul [48, 64] (K = 48: a full MX block
    and a short one) -> Add bias -> ReLU -> MatMul [64, 10] (K = 64: rotatable by --mx_rotate)."""
    from dipoorlet_amd.models import _B
    g = _B(29)
    g.const("ln.weight", (1.0 + 0.5 * g.rng.standard_normal(DIM)).astype(np.float32))
    g.const("ln.weight", g.init["ln.weight"] * np.where(np.arange(DIM) % 11 == 3, 8.0, 1.0).astype(np.float32))     # a few large channels
    g.b("ln.bias", DIM)
    t = g.node("Add", [g.node("Mul", ["input", "ln.weight"], out="ln_mul"), "ln.bias"], out="ln_out")
    g.w("fc1.weight", (DIM, HID), fan_in=DIM)
    g.b("fc1.bias", HID)
    h = g.node("Relu", [g.node("Add", [g.node("MatMul", [t, "fc1.weight"], out="fc1_mm"), "fc1.bias"], out="fc1_out")], out="h")
    g.w("fc2.weight", (HID, OUT), fan_in=HID)
    x = g.node("MatMul", [h, "fc2.weight"], out="output")
    return g.finish("input", [1, SEQ, DIM], x)


def images(shape, n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n,) + tuple(shape)) * scale).astype(np.float32)


def reference_forward(graph, x):
    """Every tensor of an fp32 graph (no FakeQuant node) for the batch x, by the definitions in fp64: {name: fp64 array}."""
    env = {k: np.asarray(v) for k, v in graph.initializer.items()}
    env[graph.network_inputs[0]] = np.asarray(x, np.float64)
    opset = int(graph.opset.get("", 13))
    for node in graph.graph.node:
        y, _ = _evaluate(node, opset, {n: env[n] for n in node.input if n != ""})
        env.update(zip(node.output, y))
    return {k: v for k, v in env.items() if k not in graph.initializer}


def host_ranges(graph, acts):
    """(activation ranges [min, max] as -A minmax merges them, weight ranges per output channel as find_clip_val_minmax_weight takes
    them: rows of the initializer, a ConvTranspose weight's axes 0 and 1 swapped first) from host arrays."""
    from dipoorlet_amd.platform_settings import LAYER_HAS_WEIGHT
    act = {k: [np.float32(v.min()), np.float32(v.max())] for k, v in acts.items()}
    wt = {}
    for node in graph.graph.node:
        if node.op_type not in LAYER_HAS_WEIGHT:
            continue
        for j, name in enumerate(node.input[1:]):
            w = np.asarray(graph.get_initializer(name))
            if node.op_type == "ConvTranspose" and j == 0:
                w = np.swapaxes(w, 0, 1)
            w2 = w.reshape(w.shape[0], -1)
            wt[name] = [w2.min(-1), w2.max(-1)]
    return act, wt
