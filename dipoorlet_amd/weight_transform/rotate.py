"""`--mx_rotate` — a 32-point Hadamard rotation inside every MX block of both operands of a MatMul / Gemm with a constant weight
(not in the reference; with `--mx` only; the definition in numpy is tests/mx_rotate_model.py).

An MX block has one power-of-two scale for 32 values along the reduction axis: one large channel pushes the other 31 onto the
bottom codes of the element format.  With H32 the symmetric +-1 Sylvester matrix (H32 . H32 = 32 I) and H = blockdiag(H32, ...),

    (X . H) . (H . W / 32) = X . W

in real arithmetic, so the network computes the same function while every value of a rotated block is a +-1 combination of all
32.  For every *site* — a MatMul / Gemm (transA = 0), not in --skip_layers, whose operand 0 is an activation T, whose operand 1 is
a 2-D initializer nothing else reads, and whose reduction length K is a multiple of 32 — the graph gets ONE node `BlockHadamard`
(domain graph.MX_DOMAIN, block_size 32; executor: ops.hadamard32, k_hadamard32) per activation, T -> T_rot, shared by every site
that reads T; the site reads T_rot, and its weight is replaced by H . W / 32 along the reduction axis.  Readers of T that are no
sites keep reading T.  The weight side is a handful of fp32 array operations on the host, as in `--smooth` and `--we`.  Saved as
rotate_model.onnx, with rotate_report.json.  A runtime applies H32 per block in front of its MX quantiser of every tensor listed.
"""
import collections
import json
import os

import numpy as np
from .. import dist_helper
from ..graph import MX_DOMAIN, ONNXGraph
from ..onnx_io import Node
from ..utils import logger
from .utils import update_weight

__all__ = ["RotateSite", "BLOCK", "ROT_SUFFIX", "find_rotate_sites", "fold_weight_host", "apply_rotate", "rotate_report", "mx_rotate"]

BLOCK = 32
ROT_SUFFIX = "_rot"
# node: the MatMul / Gemm's name; activation: its operand 0; weight: its initializer; axis: the weight's reduction axis; K: its length
RotateSite = collections.namedtuple("RotateSite", "node activation weight axis K")


def _why_left(graph, node, skipped):
    """None if `node` (a MatMul / Gemm) is a site, else the reason it is left alone."""
    if node.name in skipped:
        return "in --skip_layers"
    if len(node.input) < 2 or node.input[0] == "" or node.input[1] == "":
        return "fewer than two operands"
    if node.op_type == "Gemm" and node.attrs.get("transA", 0):
        return "transA: the activation's reduction axis is not its last"
    a, w = node.input[0], node.input[1]
    if a in graph.initializer:
        return "operand 0 is a constant"
    producer = graph.get_tensor_producer(a)
    if not isinstance(producer, str) and producer.op_type == "BlockHadamard":
        return "operand 0 is rotated already (the output of a BlockHadamard node)"
    if w not in graph.initializer:
        return "operand 1 is an activation (activation x activation products are out of scope)"
    wv = np.asarray(graph.initializer[w])
    if wv.ndim != 2:
        return f"the weight has {wv.ndim} axes, not 2"
    if len(graph.input_map.get(w, ())) != 1:
        return "the weight has another reader"
    k = int(wv.shape[1 if node.op_type == "Gemm" and node.attrs.get("transB", 0) else 0])
    if k == 0 or k % BLOCK:
        return f"K = {k} is not a multiple of {BLOCK}"
    if a + ROT_SUFFIX in graph.initializer or not isinstance(graph.get_tensor_producer(a + ROT_SUFFIX), str) \
            or a + ROT_SUFFIX in graph.network_inputs:
        return f"the graph already has a tensor {a + ROT_SUFFIX}"
    return None


def find_rotate_sites(graph, skip_layers=()):
    """-> (sites in graph order, [(node name, why)] for every other MatMul / Gemm)."""
    skipped = set(skip_layers or ())
    sites, left = [], []
    for node in graph.graph.node:
        if node.op_type not in ("MatMul", "Gemm"):
            continue
        why = _why_left(graph, node, skipped)
        if why is not None:
            left.append((node.name, why))
            continue
        trans = node.op_type == "Gemm" and bool(node.attrs.get("transB", 0))
        w = np.asarray(graph.initializer[node.input[1]])
        sites.append(RotateSite(node.name, node.input[0], node.input[1], 1 if trans else 0, int(w.shape[1 if trans else 0])))
    return sites, left


def fold_weight_host(w, axis):
    """H . W / 32 along `axis` of a 2-D fp32 weight (tests/mx_rotate_model.py fold_weight, bit for bit): per run of 32 along the
    axis the five butterfly stages h = 1, 2, 4, 8, 16 — (v[i], v[i | h]) <- (v[i] + v[i | h], v[i] - v[i | h]) for i & h == 0,
    each a single fp32 operation — then * 2^-5."""
    w = np.asarray(w, np.float32)
    v = np.ascontiguousarray(np.moveaxis(w, axis, -1))
    shape = v.shape
    v = v.reshape(-1, BLOCK).copy()
    idx = np.arange(BLOCK)
    with np.errstate(all="ignore"):
        for h in (1, 2, 4, 8, 16):
            lo = idx[(idx & h) == 0]
            a, b = v[:, lo], v[:, lo | h]
            v[:, lo], v[:, lo | h] = a + b, a - b            # (fp32 arrays: numpy rounds every sum to fp32)
        v *= np.float32(2.0 ** -5)
    return np.ascontiguousarray(np.moveaxis(v.reshape(shape), -1, axis))


def apply_rotate(graph, sites):
    """-> a copy of `graph` with every site rotated: one BlockHadamard node per activation in front of its first site, the sites
    re-wired to its output, their weights folded."""
    out = ONNXGraph()
    out.copy_from(graph)
    by_name = {n.name: n for n in out.graph.node}
    rotated = {}
    for site in sites:
        node = by_name[site.node]
        t = site.activation
        if t not in rotated:
            rotated[t] = t + ROT_SUFFIX
            had = Node("BlockHadamard", [t], [rotated[t]], name=t + "_BlockHadamard", domain=MX_DOMAIN, attrs={"block_size": BLOCK})
            out.insert_node_purely(had, out.graph.node.index(node))
            if t in out.tensor_name_shape_map:
                out.set_tensor_shape(rotated[t], out.tensor_name_shape_map[t])
            if rotated[t] not in out.output:
                out.output.append(rotated[t])
        node.input[0] = rotated[t]
        update_weight(out, fold_weight_host(out.get_initializer(site.weight), site.axis), site.weight)
    out.opset[MX_DOMAIN] = 1
    out.update_model()
    return out


def rotate_report(sites, left):
    return {"rotated": [{"node": s.node, "activation": s.activation + ROT_SUFFIX, "weight": s.weight, "K": s.K} for s in sites],
            "left": [{"node": n, "why": w} for n, w in left]}


def mx_rotate(graph, args):
    """-> the rotated graph (rank 0 saves it as rotate_model.onnx and writes rotate_report.json); `graph` itself, nothing written,
    where it has no site.  Host work only: every rank ends with the same model."""
    sites, left = find_rotate_sites(graph, getattr(args, "skip_layers", None) or ())
    rank = dist_helper.rank()
    if not sites:
        if rank == 0:
            logger.info("--mx_rotate: no MatMul / Gemm with a constant weight and K a multiple of {} in this graph: nothing to do{}".format(
                BLOCK, "".join("\n  {}: {}".format(n, w) for n, w in left)))
        return graph
    graph_r = apply_rotate(graph, sites)
    if rank == 0:
        logger.info("MX rotate: {} node(s) rotated over {} activation(s), {} left as they are{}".format(
            len(sites), len({s.activation for s in sites}), len(left), "".join("\n  {}: {}".format(n, w) for n, w in left)))
        if getattr(args, "output_dir", None):
            graph_r.output_dir = args.output_dir
            graph_r.save_onnx_model("rotate_model")
            with open(os.path.join(args.output_dir, "rotate_report.json"), "w") as f:
                json.dump(rotate_report(sites, left), f, indent=1)
    return graph_r
