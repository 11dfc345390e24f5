"""--gptq (not in the reference): GPTQ (Frantar et al., 2022) — Hessian-compensated weight rounding, one pass per layer, on whatever
grid the platform's fake-quant nodes round weights to (an integer grid or OCP FP8 E4M3).  tests/gptq_model.py is the definition.

The fake-quantised network is walked once, node-major, exactly as AdaRound's driver walks it (walk.QuantWalk).  For every
Conv (group 1, two spatial axes) and Gemm whose weight the graph fake-quantises:
  * H = sum X^T X / rows over the node's fake-quantised input — a Gemm's input rows, a Conv's unfolded patches (pads applied
    explicitly, so asymmetric ONNX pads are right) — fp32 GEMMs per slab summed in fp64, one fp64 SUM all-reduce per node;
  * U = the upper Cholesky factor of (H + damp * mean(diag H) * I)^-1, on the host in fp64 (factor(): every rank computes the same
    matrix, whatever device solver the torch build ships);
  * ops.gptq_quantize rounds the weight column by column (csrc/gptq_kernels.hip) under the grid of the very get_qnode_by_param call
    insert_fake_quant_node makes for that initializer: the graph's own Q/DQ node leaves the result unchanged;
  * the new weight goes into the result, the fake-quantised graph and its session before the node runs, so everything downstream is
    rounded against GPTQ's weights upstream.
Profiling and deployment go on with the ORIGINAL ranges, as after AdaRound.

--mx_gptq (with --mx): the same walk over a second kind of layer.  Every Gemm without transA and every MatMul whose second input is
a constant 2-D initializer, where the graph's own node block-scales the weight (QDQNode.is_mx — asked of the node quant_graph built,
not of the format's gptq_grid, which has no static grid to give), goes to ops.gptq_mx_quantize as [N, K] with the blocks along K
(tests/mx_gptq_model.py is the definition): a block's shared exponent is fixed when the recursion enters it, and the finished
weight is a fixed point of the graph's MXQuantizeDequantize node, so no scale byte has to travel.  Every Conv / Gemm whose weight
has a static grid (the patch embedding's E4M3 scales) takes the path above.  Report entries carry "grid" then."""
import json
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

from .. import ops
from ..dist_helper import barrier, shard_range
from ..executor import conv_padding
from ..platform_settings import platform_setting_table
from ..quantize import NO_STATIC_GRID, get_qnode_by_param
from ..utils import logger
from .walk import QuantWalk

__all__ = ["gptq", "factor", "layer_grid"]

GPTQ_NODE_TYPES = ("Conv", "Gemm")
MX_GPTQ_NODE_TYPES = GPTQ_NODE_TYPES + ("MatMul",)     # what --mx_gptq visits
LEFT_NODE_TYPES = ("ConvTranspose",)       # counted in the log, left as they are
_SLAB_BYTES = 256 << 20                    # bytes of X (fp32 rows) per GEMM; unfold holds a second copy of a slab while it is reshaped
_SLAB_ROWS = 1 << 16                       # ... and rows of X per fp32 GEMM at the most: longer sums are split and added in fp64
_DAMP_RETRIES = 3


def factor(H, damp=0.01):
    """H: fp64 CPU tensor [K, K] (not modified) -> (U fp64 [K, K] upper with (H')^-1 = U^T U, the damping used), H' = H with dead
    columns' (H[j, j] == 0) diagonal set to 1 plus damp * mean(diag H') * I — or (None, damp) when the factorisation still fails
    after the damping has been multiplied by 10 three times."""
    H = H.detach().to(device="cpu", dtype=torch.float64).clone()
    d = H.diagonal()
    d[d == 0] = 1.0
    mean_diag = float(d.mean())
    for _ in range(_DAMP_RETRIES + 1):
        Hd = H.clone()
        Hd.diagonal().add_(damp * mean_diag)
        L, info = torch.linalg.cholesky_ex(Hd)
        if int(info) == 0 and bool(torch.isfinite(L).all()):
            U, info = torch.linalg.cholesky_ex(torch.cholesky_inverse(L), upper=True)
            if int(info) == 0 and bool(torch.isfinite(U).all()):
                return U, damp
        damp *= 10.0
    return None, damp


def layer_grid(graph, node, clip_val, args, dev):
    """The grid the fake-quantised graph rounds `node`'s weight to -> (ops.GptqGrid, None) or (None, why not).  From the same
    get_qnode_by_param call as quantize.insert_fake_quant_node's; qlo / qhi: the platform's bit width (what AdaRound clamps to)
    inside the Q/DQ node's own saturation, so a weight on this grid passes the graph's node unchanged."""
    name = node.input[1]
    param = platform_setting_table[args.deploy]["qw_params"]
    rng = [np.copy(clip_val[name][0]), np.copy(clip_val[name][1])]
    qnode, q_min, q_max = get_qnode_by_param(param, name, graph.tensor_name_shape_map.get(name), rng, False)
    return (None, NO_STATIC_GRID) if qnode is None else qnode.format.gptq_grid(qnode, q_min, q_max, dev)


def _why_left(node, weight):
    """Why GPTQ does not touch `node` (None: it does)."""
    if node.op_type == "Conv":
        if int(node.attrs.get("group", 1)) != 1:
            return "a grouped convolution"
        if weight.ndim != 4:
            return "not a convolution over two spatial axes"
    elif node.op_type == "MatMul":
        if weight.ndim > 2:
            return "a constant of rank above 2"
        if weight.ndim < 2:
            return "a constant of rank below 2"
    elif node.attrs.get("transA", 0):
        return "a Gemm with transA"
    return None


def _why_left_matmul(graph, node):
    """Why --mx_gptq leaves a MatMul whose second input is no initializer."""
    return "a constant left operand" if node.input[0] in graph.initializer else "a MatMul with two activation operands"


def _mx_elem(graph_q, node, ori, weight):
    """The element format of the MX node quant_graph put on the weight of `node` (graph_q's; `ori`: the same node before) ->
    (elem, None); (None, None) where the weight's node is a static one; (None, why) where the MX node is not one GPTQ can serve."""
    producer = graph_q.get_tensor_producer(node.input[1])
    q = None if isinstance(producer, str) else graph_q._qdq.get(producer.name)
    if q is None or not q.is_mx:
        return None, None
    if q.mx_scales is not None:
        return None, "its MX node carries searched scales"
    k_axis = 1 if ori.op_type == "Gemm" and ori.attrs.get("transB", 0) else 0
    if weight.ndim != 2 or int(q.block_axis) % 2 != k_axis:
        return None, "its MX blocks do not run along the reduction axis"
    return q.format.elem, None


def input_rows(node, x, weight_shape):
    """The rows X [n, K] of the product the node computes as X @ W^T, W = weight.reshape(C_out, K): a Gemm's input, a Conv's patches
    in (C_in, kh, kw) order; a MatMul's left operand [..., K] row by row."""
    if node.op_type == "Gemm":
        return x.reshape(x.shape[0], -1)
    if node.op_type == "MatMul":
        return x.reshape(-1, x.shape[-1])
    kernel = list(weight_shape[2:])
    strides = node.attrs.get("strides", [1, 1])
    dil = node.attrs.get("dilations", [1, 1])
    _, fpad = conv_padding(node, x, kernel, strides, dil)
    if any(fpad):
        x = F.pad(x, fpad)
    cols = F.unfold(x, tuple(kernel), dilation=tuple(dil), padding=0, stride=tuple(strides))     # [B, K, L]
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def rows_per_image(node, x, weight_shape):
    """Rows of input_rows() one image contributes, from the shapes alone: 1 for a Gemm, the output positions of a Conv, the product
    of a MatMul operand's axes between the first and the last."""
    if node.op_type == "Gemm":
        return 1
    if node.op_type == "MatMul":
        return int(np.prod(x.shape[1:-1], dtype=np.int64))
    kernel = list(weight_shape[2:])
    strides = node.attrs.get("strides", [1, 1])
    dil = node.attrs.get("dilations", [1, 1])
    _, fpad = conv_padding(node, x, kernel, strides, dil)       # F.pad order: last axis first, (begin, end) per axis
    n = 1
    for ax in range(2):
        size = x.shape[2 + ax] + fpad[2 * (1 - ax)] + fpad[2 * (1 - ax) + 1]
        n *= (size - dil[ax] * (kernel[ax] - 1) - 1) // strides[ax] + 1
    return n


def hessian(node, chunks, weight_shape, K, dev):
    """sum X^T X over this rank's chunks of the node's input, and the number of rows, in ONE fp64 device vector [K * K + 1] (what is
    all-reduced).  A chunk is taken in slabs of whole images of at most _SLAB_BYTES of fp32 rows (and _SLAB_ROWS rows; one image
    at the least)."""
    acc = torch.zeros(K * K + 1, dtype=torch.float64, device=dev)
    H = acc[:K * K].view(K, K)
    for x in chunks:
        per_image = max(1, rows_per_image(node, x, weight_shape))
        step = max(1, min(_SLAB_ROWS, _SLAB_BYTES // (4 * K)) // per_image)
        for i in range(0, x.shape[0], step):
            X = input_rows(node, x[i:i + step], weight_shape)
            if X.shape[1] != K or X.shape[0] != per_image * min(step, x.shape[0] - i):
                raise ValueError(f"--gptq: {node.name}: input rows of shape {tuple(X.shape)}, expected {per_image} per image and {K} columns")
            H += torch.matmul(X.t(), X).double()
            acc[K * K] += X.shape[0]
    return acc


def _objective(wq, w, H):
    d = (wq - w).double()
    return float(((d @ H) * d).sum())


def gptq(graph_ori, graph, act_clip_val, weight_clip_val, args):
    """-> (the graph with GPTQ's weights — rank 0 saves it as gptq.onnx —, the per-layer report: a list of {node, rows, cols, damp,
    objective_nearest, objective_gptq, kept}); objective = tr((Wq - W) H (Wq - W)^T) under the layer's own H; `kept`: 'gptq', or
    'nearest' where the factorisation failed (objective_gptq is None; the weight is left as it is: the graph's Q/DQ node rounds it
    to nearest).  Rank 0 also writes the report, and the nodes left as they are with the reason, to gptq_report.json."""
    barrier()
    walk = QuantWalk(graph, act_clip_val, weight_clip_val, args)
    graph_new, graph_q, dev, rank = walk.graph_new, walk.graph_q, walk.dev, walk.rank
    qf = walk.start(*shard_range(args.data_num, rank, walk.world))
    skip = set(getattr(args, "skip_layers", None) or ())
    block = int(getattr(args, "gptq_block", ops.GPTQ_MAX_BLOCK) or ops.GPTQ_MAX_BLOCK)
    damp0 = float(getattr(args, "gptq_damp", 0.01) or 0.01)
    ori_nodes = {n.name: n for n in graph.graph.node}
    mx_gptq = bool(getattr(args, "mx_gptq", False))
    flag = "--mx_gptq" if mx_gptq else "--gptq"
    visited = (MX_GPTQ_NODE_TYPES if mx_gptq else GPTQ_NODE_TYPES) + LEFT_NODE_TYPES
    report, left = [], []
    with torch.no_grad():
        for node in graph_q.graph.node:
            ori = ori_nodes.get(node.name)
            if ori is None or ori.op_type not in visited or len(ori.input) < 2:
                qf.run(node)
                continue
            wname = ori.input[1]
            weight = graph_new.get_initializer(wname) if wname in graph_new.initializer else None
            why = ("in --skip_layers" if node.name in skip else "a ConvTranspose" if ori.op_type in LEFT_NODE_TYPES else
                   _why_left_matmul(graph_new, ori) if ori.op_type == "MatMul" and weight is None else
                   "its weight is not a constant" if weight is None else
                   "the graph does not fake-quantise its weight" if node.input[1] == wname else _why_left(ori, weight))
            if why is None and mx_gptq and len(graph_new.get_tensor_consumer(wname)) > 1:
                why = "other nodes read its weight"
            grid = elem = None
            if why is None and mx_gptq:
                elem, why = _mx_elem(graph_q, node, ori, weight)
            if why is None and elem is None:
                if ori.op_type == "MatMul":
                    why = NO_STATIC_GRID
                else:
                    grid, why = layer_grid(graph_new, ori, walk.clip_val, args, dev)
            rows_first = ori.op_type == "Conv" or (ori.op_type == "Gemm" and bool(ori.attrs.get("transB", 0)))
            if why is None and grid is not None and grid.scale.numel() > 1 and not (rows_first and grid.scale.numel() == weight.shape[0]):
                why = "its per-channel scales do not run along the output channels"
            if why is not None:
                left.append((node.name, why))
                qf.run(node)
                continue
            w_host = np.ascontiguousarray(weight, dtype=np.float32)
            w2d = torch.from_numpy(w_host.reshape(w_host.shape[0], -1) if rows_first else np.ascontiguousarray(w_host.T)).to(dev)
            R, K = w2d.shape
            acc = hessian(ori, qf.env[node.input[0]], w_host.shape, K, dev)
            if walk.world > 1:
                dist.all_reduce(acc)
            H = acc[:K * K].view(K, K) / acc[K * K]
            U, damp = factor(H.cpu(), damp0)
            w_near = ops.gptq_nearest(w2d, grid) if elem is None else ops.gptq_mx_nearest(w2d, elem)
            entry = {"node": node.name, "rows": int(R), "cols": int(K), "damp": damp, "kept": "nearest",
                     "objective_nearest": _objective(w_near, w2d, H), "objective_gptq": None}
            if mx_gptq:
                entry["grid"] = grid.fmt if elem is None else elem
            if U is None:       # the only fall-back: the weight stays as it is, the graph's Q/DQ node rounds it to nearest
                logger.warning("%s: the Hessian of %s could not be factorised (damping up to %g): left at round-to-nearest", flag, node.name, damp)
            else:
                u32 = U.to(torch.float32).contiguous().to(dev)
                wq = ops.gptq_quantize(w2d, u32, grid, block)[0] if elem is None else ops.gptq_mx_quantize(w2d, u32, elem, block)[0]
                entry.update(objective_gptq=_objective(wq, w2d, H), kept="gptq")
                if entry["objective_gptq"] > entry["objective_nearest"]:       # (reported, not acted on)
                    logger.warning("%s: %s: the compensated rounding did not lower the objective (%g against %g)", flag, node.name,
                                   entry["objective_gptq"], entry["objective_nearest"])
                w_new = wq if rows_first else wq.t().contiguous()
                walk.set_const(wname, w_new.reshape(w_host.shape))
            report.append(entry)
            if rank == 0:
                logger.info("GPTQ for: {} [{} x {}] objective nearest {:.6g} -> gptq {} ({})".format(
                    node.name, R, K, entry["objective_nearest"],
                    "-" if entry["objective_gptq"] is None else "{:.6g}".format(entry["objective_gptq"]), entry["kept"]))
            del acc, H, U, w_near
            qf.run(node)
    if rank == 0:
        logger.info("GPTQ: {} layer(s) rounded, {} left as they are{}".format(
            sum(e["kept"] == "gptq" for e in report), len(left) + sum(e["kept"] != "gptq" for e in report),
            "".join("\n  {}: {}".format(n, w) for n, w in left)))
        if getattr(args, "output_dir", None):
            with open(os.path.join(args.output_dir, "gptq_report.json"), "w") as f:
                json.dump({"layers": report, "left": [{"node": n, "why": w} for n, w in left]}, f, indent=1)
    return walk.finish("gptq"), report
