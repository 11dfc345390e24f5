"""Scale / zero-point derivation and the fake-quant forward — counterpart of dipoorlet/quantize.py.

The reference derives (scale, zero_point, q_min, q_max) on the host (quantize.py:111-194), wraps them
in a QuantizeLinear -> DequantizeLinear ONNX sub-graph (:197-239) and lets ONNXRuntime execute it.
Here the derivation is the same host arithmetic (numpy float64 -> float32, bit-exact against the
reference-generated golden rows) and the Q->DQ pair is ONE fused HIP kernel (k_fake_quant_*): 4 B read
+ 4 B written per element instead of a quantised intermediate tensor.

Naming follows the reference so the emitted graph / deploy files stay drop-in:
    <t>_scale, <t>_zero_point, <t>_q, <t>_dq, nodes <t>_QuantizeLinear / <t>_DequantizeLinear.

What differs between number formats is in FORMATS, one record per quantisation "type" of platform_settings' tables; a QDQNode
holds its record (`format`) and every other module asks the node ("Number formats").
"""
import numpy as np
import torch

from . import onnx_io, ops
from .graph import MX_DOMAIN, ONNXGraph
from .onnx_io import Node
from .utils import logger

QTENSORSUFFIX = "_q"
DQTENSORSUFFIX = "_dq"
QUANT_NODE_NAME_LIST = ["QuantizeLinear", "DequantizeLinear"]
FP8_E4M3 = "Float8E4M3FN"      # the quantisation type of OCP FP8 E4M3 (platform `ocp_fp8`); every other platform: "Linear"
E4M3_MAX = 448
MX_BLOCK = ops.MX_BLOCK
MX_NODES = ["MatMul", "Gemm"]
MERGE_RELU = ["Conv", "Gemm", "Eltwise", "Add"]
RELU_TYPE = ["Relu", "PRelu", "Mul"]


def _int8_wrap(zero_point, shape):
    """The reference stores the zero point through np.full(..., dtype=np.int8) (quantize.py:185): values above 127 wrap
    (191 -> -65) and are later re-read as uint8 for asymmetric grids.  Reproduced on purpose."""
    with np.errstate(all="ignore"):
        z = np.broadcast_to(np.asarray(zero_point, np.float64), shape).astype(np.int64)
    return ((z + 128) % 256 - 128).astype(np.int8)


def _symmetric_grid(top, lo, hi):
    """scale = max(|lo|, |hi|) / top per channel — the clip lands on the grid's largest value `top` (2^(b-1) - 1; 448 for E4M3) —,
    grid [-top, top], zero point 0."""
    n = lo.size if isinstance(lo, np.ndarray) else 1
    q_hi = [top] * n
    scale = np.asarray(np.max(np.abs([lo, hi]), axis=0)) / q_hi
    scale = np.where(scale == 0, 1.0, scale)          # an all-zero channel quantises with scale 1
    return scale.tolist(), [0], [-top] * n, q_hi


def _affine_grid(bits, lo, hi, tensor_name):
    """Asymmetric grid over [min(lo, 0), max(hi, 0)]: scale = span / (2^b - 1), zp = round(-lo / scale),
    q range [-zp, 2^b - 1 - zp].  Per-channel bounds are clamped IN PLACE, as the reference's caller-visible arrays are."""
    levels = 2 ** bits - 1
    if isinstance(lo, np.ndarray):
        np.minimum(lo, 0.0, out=lo)
        np.maximum(hi, 0.0, out=hi)
        scale = (hi - lo) / levels
        dead = scale == 0
        if dead.any():
            logger.warning("%d all-zero channel(s) in %s: scale set to 1", int(dead.sum()), tensor_name)
            scale = np.where(dead, 1.0, scale)
        zp = (-lo / scale).round()
        return scale.tolist(), zp, (-zp).astype(np.int32).tolist(), (levels - zp).astype(np.int32).tolist()
    lo, hi = min(0, lo), max(0, hi)
    scale = (hi - lo) / levels
    if scale == 0.0:
        scale += 1.0
    zp = np.round(-lo / scale)
    return [float(scale)], zp, [int(-zp)], [int(levels - zp)]


NO_STATIC_GRID = "its weight has no static grid"        # why --gptq leaves a layer whose weight is not on a static grid


def _in_one_transfer(arrays, dtype, device):
    """Host arrays -> their device copies, views of ONE uploaded tensor."""
    return torch.from_numpy(np.concatenate(arrays).astype(dtype)).to(device).split([a.size for a in arrays])


class NumberFormat:
    """Everything that differs between the number formats a fake-quant node rounds to.  The fields, and below them what the two
    static formats share: a scale and a zero point per tensor or per channel, saved as a QuantizeLinear -> DequantizeLinear pair."""
    static = True            # scale / zero-point initializers and, per channel, an axis to check against the tensor's shape
    takes_pre = True         # apply() has a form with the producer's ReLU / Add + ReLU inside the kernel
    block_scaled = False     # blocks along QDQNode.block_axis share a scale taken from the data: along the batch axis they mix samples
    integer = False          # a uniform grid: what -A mse, -A kl, --adaround, --brecq and --sparse assume or learn
    set_fmt = None           # ops.FakeQuantSet's fmt for a whole-set launch (set_rows); None: node by node through apply()
    zp_dtype = bounds = None     # by `symmetric` (False, True): the zero point's dtype, the (lowest, highest) value the node saturates to
    opset, ir_version = {}, 0    # what the saved nodes require of the file: {domain: operator-set version} and the IR version, at least

    def __init__(self, name):
        self.name = name

    def __deepcopy__(self, memo):       # (a copied graph's nodes share the records)
        return self

    def initializers(self, q):
        """{name: array} the node adds to a graph (utils.py:198-206): a single value as a 0-d tensor."""
        zp = self.zero_point_tensor(q)
        return {q.scale_name: q.scale if q.scale.size > 1 else q.scale.reshape(()), q.zero_point_name: zp if zp.size > 1 else zp.reshape(())}

    def onnx_nodes(self, q):
        """The nodes a FakeQuant node is saved as: the reference's 2-node form (quantize.py:208-231)."""
        attrs = {"axis": q.axis} if q.per_channel else {}
        return [Node("QuantizeLinear", [q.tensor_name, q.scale_name, q.zero_point_name], [q.q_output], name=q.q_name, attrs=attrs),
                Node("DequantizeLinear", [q.q_output, q.scale_name, q.zero_point_name], [q.output], name=q.dq_name, attrs=attrs)]


class _Linear(NumberFormat):
    """An 8-bit integer grid (every platform of the reference)."""
    integer, set_fmt = True, "int"
    # QuantizeLinear saturates to the zero-point dtype's full range (ONNX opset 13) — note: -128, not the q_min = -127 the
    # reference computes at :134 for its torch-side code
    zp_dtype, bounds = ("uint8", "int8"), ((0, 255), (-128, 127))      # :205-206

    def qnode(self, param, name, shape, range, need_transpose, block_axis, suffix):
        per_channel = bool(param.get("per_channel", False))
        symmetric = param["symmetric"]
        if not per_channel:
            range[0], range[1] = np.min(range[0]), np.max(range[1])
            if param.get("dynamic_sym", False) and np.abs(range[0] - 0.0) < 1e-6:
                symmetric = False
        if symmetric:
            scale, zero_point, q_min, q_max = _symmetric_grid(2 ** (param["bit_width"] - 1) - 1, range[0], range[1])
        else:
            scale, zero_point, q_min, q_max = _affine_grid(param["bit_width"], range[0], range[1], name)
        if param.get("log_scale", False):
            scale = 2 ** np.round(np.log2(scale))
        scale = np.array(scale, dtype=np.float32)
        return QDQNode(name, shape, scale, _int8_wrap(zero_point, scale.shape), need_transpose, per_channel, symmetric, suffix=suffix), q_min, q_max

    def apply(self, q, x, out, pre, x2):
        scale, zp = q.on_device(x.device)
        lo, hi = self.bounds[q.symmetric]
        return ops.fake_quant(x, scale, zp, lo, hi, axis=q.axis if q.scale.size > 1 else None, out=out, pre=pre, x2=x2)

    def zero_point_tensor(self, q):
        return q.zero_point if q.symmetric else q.zero_point.view(np.uint8)

    def set_rows(self, qs, inners, device):
        """ops.FakeQuantSet's parameter rows for the nodes `qs`: all scales / zero points of the set in two transfers."""
        scales = _in_one_transfer([q.scale for q in qs], np.float32, device)
        zps = _in_one_transfer([np.broadcast_to(q.zero_point_as_stored(), q.scale.shape) for q in qs], np.int32, device)
        return [(s, z, inner, *q.saturation()) for q, s, z, inner in zip(qs, scales, zps, inners)]

    def gptq_grid(self, q, q_min, q_max, dev):
        """-> (ops.GptqGrid, None) or (None, why not).  qlo / qhi: the platform's bit width (what AdaRound clamps to) inside the
        node's own saturation, so a weight on this grid passes the graph's node unchanged."""
        zp = q.zero_point_as_stored()
        lo, hi = np.asarray(q_min, np.int64).reshape(-1) + zp, np.asarray(q_max, np.int64).reshape(-1) + zp
        if not (np.all(lo == lo[0]) and np.all(hi == hi[0])):
            return None, "its channels do not share one integer range"
        sat_lo, sat_hi = q.saturation()
        return ops.GptqGrid("int", torch.from_numpy(q.scale.copy()).to(dev), torch.from_numpy(zp.astype(np.int32)).to(dev),
                            max(int(lo[0]), sat_lo), min(int(hi[0]), sat_hi)), None


class _FP8(NumberFormat):
    """OCP FP8 E4M3 (platform `ocp_fp8`): a scale only — the zero point is 0, written as a float8e4m3fn, which QuantizeLinear /
    DequantizeLinear take from opset 19 (IR version 9) on."""
    set_fmt, top = "fp8", E4M3_MAX
    zp_dtype, bounds = ("float8e4m3fn",) * 2, ((-E4M3_MAX, E4M3_MAX),) * 2       # saturate = 1: the largest finite value
    opset, ir_version = {"": 19}, 9

    def qnode(self, param, name, shape, range, need_transpose, block_axis, suffix):
        per_channel = bool(param.get("per_channel", False))
        if not per_channel:
            range[0], range[1] = np.min(range[0]), np.max(range[1])
        scale = np.array(_symmetric_grid(self.top, range[0], range[1])[0], dtype=np.float32).reshape(-1)
        return (QDQNode(name, shape, scale, np.zeros(scale.shape, np.int8), need_transpose, per_channel, True, fmt=self.name, suffix=suffix),
                -self.top, self.top)

    def apply(self, q, x, out, pre, x2):
        return ops.fake_quant_fp8(x, q.on_device(x.device)[0], axis=q.axis if q.scale.size > 1 else None, out=out, pre=pre, x2=x2)

    def zero_point_tensor(self, q):     # the zero of the format: one 0x00 byte per element (TensorProto type 17)
        return onnx_io.Float8E4M3FNBytes(np.zeros(q.scale.shape, np.uint8))

    def set_rows(self, qs, inners, device):
        return list(zip(_in_one_transfer([q.scale for q in qs], np.float32, device), inners))

    def gptq_grid(self, q, q_min, q_max, dev):
        return ops.GptqGrid("e4m3", torch.from_numpy(q.scale.copy()).to(dev)), None


class _MX(NumberFormat):
    """OCP Microscaling (`--mx`, platform_settings.mx_setting_table and mx_fp6_setting_table): blocks of MX_BLOCK along QDQNode.block_axis share a
    power-of-two scale taken from the data — no static scale, no zero point, no initializers; the clip range is ignored.  ONNX has
    no dynamic block-scaled Q/DQ pair to expand into: the node is saved as ONE node of this project's own domain.
    `--mx_scale_search`: the node of a CONSTANT operand may carry its blocks' E8M0 bytes (QDQNode.mx_scales, ops.mx_scale_search of
    the weight as it stands) — then it rounds under those (ops.fake_quant_mx_scaled), and is saved with them as a uint8 initializer,
    the node's optional second input (a block moved up to se0 + 1 is in general no fixed point of the floor rule, so the choice
    cannot be folded into the weights)."""
    static = takes_pre = False
    block_scaled = True
    opset = {MX_DOMAIN: 1}
    zp_dtype = ("int8",) * 2            # (of the placeholder zero point: never written)

    def __init__(self, name, elem, elem_type, top):
        """elem: ops.fake_quant_mx's name of the element format; elem_type: as the saved node names it; top: the largest element."""
        self.name, self.elem, self.elem_type, self.top, self.bounds = name, elem, elem_type, top, ((-top, top),) * 2

    def qnode(self, param, name, shape, range, need_transpose, block_axis, suffix):
        return (QDQNode(name, shape, np.ones(1, np.float32), np.zeros(1, np.int8), False, False, True, fmt=self.name,
                        block_axis=int(block_axis), suffix=suffix), -self.top, self.top)

    def apply(self, q, x, out, pre, x2):
        if pre is not None:
            raise ValueError(f"{q.q_name}: a block-scaled ({self.name}) fake-quant node takes no fused producer ({pre!r})")
        if q.mx_scales is not None:
            return ops.fake_quant_mx_scaled(x, q.block_axis, self.elem, q.mx_scales_on_device(x.device), out=out)
        return ops.fake_quant_mx(x, q.block_axis, self.elem, out=out)

    def initializers(self, q):
        return {} if q.mx_scales is None else {q.scale_name: q.mx_scales}

    def onnx_nodes(self, q):
        inputs = [q.tensor_name] if q.mx_scales is None else [q.tensor_name, q.scale_name]      # (the second input is optional)
        return [Node("MXQuantizeDequantize", inputs, [q.output], name=q.q_name, domain=MX_DOMAIN,
                     attrs={"axis": int(q.block_axis), "block_size": MX_BLOCK, "elem_type": self.elem_type})]

    def search_scales(self, q, w):
        """`--mx_scale_search`: give node q the error-minimising E8M0 bytes of the constant w (numpy fp32) it quantises."""
        dev = torch.device("cuda", torch.cuda.current_device())
        x = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
        q.mx_scales = ops.mx_scale_search(x, int(q.block_axis), self.elem).cpu().numpy()

    def gptq_grid(self, q, q_min, q_max, dev):
        return None, NO_STATIC_GRID


FORMATS = {f.name: f for f in (_Linear("Linear"), _FP8(FP8_E4M3), _MX("MXFP8E4M3", "mxfp8", "float8e4m3fn", 448),
                               _MX("MXFP4E2M1", "mxfp4", "float4e2m1", 6))}
MX_TYPES = {k: f for k, f in FORMATS.items() if f.block_scaled}
# The two OCP MXFP6 formats (platform_settings.mx_fp6_setting_table; tests/mx_fp6_model.py): the records of _MX's kind that
# --mx_gptq and --mx_mixed do not serve, kept beside the two they do.
MX_FP6_TYPES = {f.name: f for f in (_MX("MXFP6E2M3", "mxfp6_e2m3", "float6e2m3", 7.5), _MX("MXFP6E3M2", "mxfp6_e3m2", "float6e3m2", 28))}


def number_format(type_name):
    """The record of a quantisation "type", or None: the one lookup every reader goes through, whichever table holds the record."""
    return FORMATS.get(type_name) or MX_FP6_TYPES.get(type_name)


class QDQNode:
    """The fused fake-quant stand-in for the reference's 2-node `graph_quant` (quantize.py:197-239).  `fmt`: the number format
    of the grid, a key of FORMATS or MX_FP6_TYPES (`format`: its record, number_format).  `suffix`: appended to every name of the node — a tensor that already
    has a fake-quant node of another kind keeps that one's names for it."""

    def __init__(self, tensor_name, tensor_shape, scale, zero_point, need_transpose, per_channel, symmetric, fmt="Linear",
                 block_axis=None, suffix=""):
        self.tensor_name = tensor_name
        self.tensor_shape = list(tensor_shape) if tensor_shape is not None else None
        self.scale = np.asarray(scale, np.float32).reshape(-1)
        self.zero_point = np.asarray(zero_point, np.int8).reshape(-1)  # stored through int8 like :185
        self.per_channel = bool(per_channel)
        self.symmetric = bool(symmetric)
        self.axis = (1 if need_transpose else 0) if per_channel else None  # :214, :220
        self.fmt, self.format = fmt, number_format(fmt)
        self.block_axis = block_axis
        self.mx_scales = None           # (block-scaled nodes of constants, --mx_scale_search) uint8: one E8M0 byte per block
        self.suffix = suffix
        self.zp_dtype = self.format.zp_dtype[self.symmetric]
        self.q_name = tensor_name + "_QuantizeLinear" + suffix
        self.dq_name = tensor_name + "_DequantizeLinear" + suffix
        self.scale_name = tensor_name + "_scale" + suffix
        self.zero_point_name = tensor_name + "_zero_point" + suffix
        self.q_output = tensor_name + QTENSORSUFFIX + suffix
        self.output = tensor_name + DQTENSORSUFFIX + suffix
        self._dev = self._mx_dev = None

    @property
    def is_mx(self):
        return self.format.block_scaled

    def zero_point_as_stored(self):
        """The integers an ONNX runtime sees: int8 values, or the same bytes read as uint8."""
        return self.zero_point.astype(np.int32) if self.symmetric else self.zero_point.view(np.uint8).astype(np.int32)

    def saturation(self):
        """(lowest, highest) value of the grid the node saturates to."""
        return self.format.bounds[self.symmetric]

    def on_device(self, device):
        """(scale, zero point as stored) on `device`: uploaded once."""
        if self._dev is None or self._dev[0].device != device:
            self._dev = (torch.from_numpy(self.scale).to(device), torch.from_numpy(self.zero_point_as_stored()).to(device))
        return self._dev

    def mx_scales_on_device(self, device):
        """mx_scales on `device`: uploaded once."""
        if self._mx_dev is None or self._mx_dev.device != device:
            self._mx_dev = torch.from_numpy(self.mx_scales).to(device)
        return self._mx_dev

    def mixes_axis(self, k, nd):
        """Is axis k of the node's nd-axis tensor one along which elements do not go through the node each on its own with the same
        parameters: the per-channel axis, or the axis whose blocks share a scale?"""
        a = self.block_axis if self.format.block_scaled else self.axis
        return a is not None and (a + nd if a < 0 else a) == k

    def apply(self, x, out=None, pre=None, x2=None):
        """Fake-quantise a device tensor: QuantizeLinear -> DequantizeLinear semantics, one kernel (pre / x2: the producer's
        ReLU or Add + ReLU fused in, ops.fake_quant)."""
        return self.format.apply(self, x, out, pre, x2)


def get_qnode_by_param(param, in_tensor_name, tensor_shape, range, need_transpose=False, block_axis=-1, suffix=""):
    """quantize.py:111-194 — returns (QDQNode, q_min, q_max) for the clip range `range` = [lo, hi] (scalars, or
    per-channel arrays for weights), (None, None, None) for a type FORMATS does not hold.  Kept from the reference because callers
    rely on it: a per-tensor platform collapses `range` to its overall min / max IN PLACE (type "Float8E4M3FN" too: scale =
    max(|lo|, |hi|) / 448, zero point 0, q_min / q_max = -448 / 448); `dynamic_sym` platforms switch a non-negative activation
    (|lo| < 1e-6) to the asymmetric grid — one more bit; `log_scale` snaps scales to powers of two.  An MX type
    (mx_setting_table, mx_fp6_setting_table) ignores `range`: its node is block-scaled along `block_axis`, q_min / q_max = the element format's."""
    fmt = number_format(param["type"])
    if fmt is None:
        return None, None, None
    return fmt.qnode(param, in_tensor_name, tensor_shape, range, need_transpose, block_axis, suffix)


def quant_acti(x, scale, q_min, q_max, prob=1.0):
    """weight_transform/ada_quant_layer.py:28-36 on the device: round-half-even(x / scale), clamp to
    [q_min, q_max], * scale.  QDrop mixing (prob < 1) keeps the original value where rand >= prob."""
    sc = torch.as_tensor(scale, dtype=torch.float32, device=x.device).reshape(-1)
    zp = torch.zeros(sc.numel(), dtype=torch.int32, device=x.device)
    y = ops.fake_quant(x, sc, zp, int(q_min), int(q_max))
    if prob < 1.0:
        y = torch.where(torch.rand_like(x) < prob, y, x)
    return y


# ------------------------------------------------------------------------------------------------
# Which tensors get fake-quantised (quantize.py:20-108), on this package's ONNXGraph.  Each inserted pair is one fused
# FakeQuant node (graph.insert_qnodes_purely).  The reference decides input by input inside one loop; here the decision
# lives in a small rule object (`_NodeRules`) that the surgery consults input by input.
class _NodeRules:
    """Which platform parameter set quantises input `idx` of `node` — 'qw_params' (first constant input of a weighted
    layer), 'qb_params' (later constant inputs, only where the platform defines them), 'qi_params' (activations and
    network inputs) — or None.  Asked input by input, in order, WHILE the node is being re-wired, because two of the
    reference's rules read the live graph:
      * a ReLU-type node (Relu / PRelu / Mul) whose first input comes from outside the producer map, or a one-input one
        directly behind Conv / Gemm / Eltwise / Add, is left alone (the activation is merged into its producer).  The
        reference looks `node.input[0]` up again for every operand: once this pass has re-wired it to a fresh fake-quant
        output — not in the producer map until the node is finished — it reads as a graph input, so of Mul(a, b) only `a`
        is quantised unless `a` already had its fake-quant node (quantize.py:49-55; pinned by tests/golden/aux_level.json);
      * TensorRT: the first Conv-produced operand of an Add rides on the Conv's output scale (:80-84)."""

    def __init__(self, graph, node, plat, deploy):
        from .platform_settings import LAYER_HAS_WEIGHT
        self.graph, self.node, self.plat = graph, node, plat
        self.relu_like = node.op_type in RELU_TYPE
        self.weighted = node.op_type in LAYER_HAS_WEIGHT
        self.weight_seen = False
        self.trt_add_slot = deploy == "trt" and node.op_type == "Add"

    def role(self, name):
        graph, node = self.graph, self.node
        if name == "":
            return None
        if self.relu_like:
            producer = graph.get_tensor_producer(node.input[0])
            if isinstance(producer, str) or (len(node.input) == 1 and producer.op_type in MERGE_RELU):
                return None
        role = None
        if self.weighted and name in graph.initializer:
            if not self.weight_seen:
                self.weight_seen, role = True, "qw_params"
            elif "qb_params" in self.plat:
                role = "qb_params"
        if name in graph.network_inputs or name not in graph.input:
            producer = graph.get_tensor_producer(name)
            if self.trt_add_slot and not isinstance(producer, str) and producer.op_type == "Conv":
                self.trt_add_slot = False
                return None
            role = "qi_params"
        return role


def mx_block_axis(node, idx, shape):
    """The axis of operand `idx` (0 or 1) of a MatMul / Gemm that the product reduces over — the one MX blocks run along: MatMul
    A -1, B -2 (-1 for a 1-D B), counted from the end as MatMul's own rule is (the same answer whether or not the graph knows an
    activation's shape yet); Gemm A 0 if transA else 1, B 1 if transB else 0; Conv (`--mx_conv`) 1 for both."""
    if node.op_type == "Conv":      # (--mx_conv) channels of the [N, C, H, W] activation, input channels of the [Cout, C, kh, kw] weight
        return 1
    if node.op_type == "Gemm":
        t = int(node.attrs.get("transA" if idx == 0 else "transB", 0) or 0)
        return (0 if t else 1) if idx == 0 else (1 if t else 0)
    return -1 if idx == 0 or (shape is not None and len(shape) == 1) else -2


def mx_conv_left(graph, node):
    """`--mx_conv`: why Conv `node` of `graph` (not yet fake-quantised) keeps its static nodes — or None: both its operands take the
    MX parameter set, blocked along axis 1.  Taken: a convolution over two spatial axes (4-D input, 4-D weight), group 1, whose
    weight is a constant."""
    if len(node.input) < 2 or node.input[1] not in graph.initializer:
        return "the weight is not a constant"
    nd = np.asarray(graph.get_initializer(node.input[1])).ndim - 2
    x_shape = graph.tensor_name_shape_map.get(node.input[0])
    if nd != 2 or (x_shape is not None and len(x_shape) != 4):
        return f"a {nd}-D convolution" if nd != 2 else f"an input of {len(x_shape)} dimension(s)"
    group = int(node.attrs.get("group", 1) or 1)
    if group != 1:
        return f"group = {group}"
    return None


def mx_conv_nodes(graph, args):
    """`--mx_conv` over the Convs of `graph` (not yet fake-quantised) that quant_graph considers -> (the names of those it
    block-scales, {name: reason} of those it leaves on their static grid)."""
    from .platform_settings import platform_setting_table
    skipped = set(getattr(args, "skip_layers", None) or ())
    taken, left = [], {}
    if "Conv" not in platform_setting_table[args.deploy]["quant_nodes"]:
        return taken, left
    for node in graph.graph.node:
        if node.op_type == "Conv" and node.name not in skipped:
            why = mx_conv_left(graph, node)
            if why is None:
                taken.append(node.name)
            else:
                left[node.name] = why
    return taken, left


def _taken(act_quantized, name):
    """The entry of the first fake-quant node of tensor `name` — the one that has the usual names — or None: `name` itself for a
    static node, (name, axis) for an MX one."""
    for k in act_quantized:
        if k == name or (isinstance(k, tuple) and k[0] == name):
            return k
    return None


def insert_fake_quant_node(graph, node, act_quantized, data_range_list, args):
    """quantize.py:40-95 for one node: derive the grid of every input that has a role, re-wire the input to the
    fake-quantised tensor, and insert the FakeQuant node unless the tensor already has one (`act_quantized`).
    With args.mx ('mxfp8' / 'mxfp6_e2m3' / 'mxfp6_e3m2' / 'mxfp4': platform_settings.mx_setting; -D ocp_fp8) both operands of a MatMul / Gemm — a constant one too, whatever its role — take
    the MX parameter set instead, blocked along the operand's reduction axis (mx_block_axis); a Gemm bias is left to the platform's
    rules.  With args.mx_conv so do both operands of every Conv that mx_conv_left lets through, along axis 1; its bias too is left
    to the platform's rules.  `act_quantized` holds (name, axis) for such a node: a tensor wanted along two axes, or by a static consumer as well,
    gets one node each — the first has the usual names, a later MX one the suffix `_ax<k>`, a later static one `_static`.
    With args.mx_formats ({node name: 'mxfp8' / 'mxfp4'}, --mx_mixed: mx_mixed.py) a node named there takes that format for both
    its operands instead of args.mx; a tensor that nodes of two formats read along one axis gets a node each, entry (name, axis,
    format) and suffix `_ax<k>_<format>` for the one that is not args.mx's.
    With args.mx_scale_search the MX node of a constant operand carries error-minimising block scales (_MX.search_scales), computed
    here from the weight as it stands in `graph`; an activation's node keeps the floor rule."""
    from .platform_settings import mx_setting, platform_setting_table
    plat = platform_setting_table[args.deploy]
    mx = getattr(args, "mx", None)
    if node.op_type not in MX_NODES and not (node.op_type == "Conv" and getattr(args, "mx_conv", False) and mx_conv_left(graph, node) is None):
        mx = None
    rules = _NodeRules(graph, node, plat, args.deploy)
    for idx, name in enumerate(list(node.input)):
        role = rules.role(name)
        if mx and idx < 2 and name != "":
            shape = graph.tensor_name_shape_map.get(name)
            axis = mx_block_axis(node, idx, shape)
            fmt = (getattr(args, "mx_formats", None) or {}).get(node.name, mx)     # (--mx_mixed: this node's own format)
            key = (name, axis) if fmt == mx else (name, axis, fmt)
            first = _taken(act_quantized, name)
            q_nodes, _, _ = get_qnode_by_param(mx_setting(fmt), name, shape, None, block_axis=axis,
                                               suffix="" if first in (None, key) else f"_ax{axis}" if fmt == mx else f"_ax{axis}_{fmt}")
            node.input[idx] = q_nodes.output
            if key not in act_quantized:
                if getattr(args, "mx_scale_search", False) and name in graph.initializer:
                    q_nodes.format.search_scales(q_nodes, graph.get_initializer(name))
                graph.insert_qnodes_purely(q_nodes=q_nodes, node=node)
                act_quantized.append(key)
            continue
        if role is None:
            continue
        transposed = role == "qw_params" and node.op_type == "ConvTranspose"
        first = _taken(act_quantized, name)
        q_nodes, _, _ = get_qnode_by_param(plat[role], name, graph.tensor_name_shape_map.get(name), data_range_list[name],
                                           transposed, suffix="" if first in (None, name) else "_static")
        if q_nodes is None:
            continue
        node.input[idx] = q_nodes.output
        if name not in act_quantized:
            graph.insert_qnodes_purely(q_nodes=q_nodes, node=node)
            act_quantized.append(name)
    graph.topologize_graph()


def insert_fake_quant_node_output(graph, clip_val, args):
    """quantize.py:98-108 — platforms that quantise the network outputs: `<out>_dq` replaces every `<out>`."""
    from .platform_settings import platform_setting_table
    qi = platform_setting_table[args.deploy]["qi_params"]
    for name in tuple(graph.network_outputs):
        q_nodes, _, _ = get_qnode_by_param(qi, name, graph.tensor_name_shape_map.get(name), clip_val[name])
        graph.insert_qnodes_purely(q_nodes=q_nodes, idx=graph.index(graph.get_tensor_producer(name)) + 1)
        graph.del_network_output(name)
        graph.add_network_output(q_nodes.output)
    graph.topologize_graph()


def quant_graph(onnx_graph, clip_val, args):
    """quantize.py:20-37 -> (fake-quantised copy of the graph, the nodes whose inputs were considered): every node whose
    op type is in the platform's `quant_nodes` and whose name is not in --skip_layers, in graph order; then the network
    outputs where the platform asks for it."""
    from .platform_settings import platform_setting_table
    plat = platform_setting_table[args.deploy]
    skipped = set(getattr(args, "skip_layers", None) or ())
    graph_q = ONNXGraph()
    graph_q.copy_from(onnx_graph)
    quant_node_list = [n for n in graph_q.graph.node if n.op_type in plat["quant_nodes"] and n.name not in skipped]
    done = []
    for node in quant_node_list:
        insert_fake_quant_node(graph_q, node, done, clip_val, args)
    if plat["quantize_network_output"]:
        insert_fake_quant_node_output(graph_q, clip_val, args)
    graph_q.update_model()
    return graph_q, quant_node_list
