"""`--smooth` — SmoothQuant-style folding of per-channel activation scales into MatMul weights (not in the reference; the
definition in numpy is tests/smooth_model.py).

A transformer's LayerNorm outputs have a few channels tens of times larger than the rest; a platform that quantises the
activation going into a MatMul per tensor (`magicmind`, `ocp_fp8`) spends its levels on those channels.  For every *site* — a
decomposed LayerNorm affine `T = Mul(Z, g) + b` whose every reader is a MatMul / Gemm with a constant weight — channel j of the
affine is divided by s_j and row j of every reader's weight is multiplied by s_j:

    s_j = a_j^alpha / w_j^(1 - alpha)        a_j = max |T[..., j]| over the calibration images, w_j = max |W[j, :]| over the readers

In real arithmetic the network computes the same function; T becomes flat.  `--we` is the same idea between two convolutions,
where both sides are weights; here one side is an activation, so its per-channel max |x| is swept over the calibration set on the
GPU (k_colwise_absmax: one read of the tensor, a running maximum per channel, no host synchronisation until the single read-back).
The folding itself is a handful of fp32 array operations on weights of a few MB: host work, as in `--we`.  Saved as
smooth_model.onnx.
"""
import collections

import numpy as np
import torch
import torch.distributed as dist

from .. import dist_helper, ops
from ..executor import GraphSession, load_chunks
from ..graph import ONNXGraph
from ..utils import logger
from .utils import update_weight

__all__ = ["SmoothSite", "SmoothReader", "find_smooth_sites", "smooth_scales", "apply_smooth", "smooth_statistics", "smooth_quant"]

# tensor: the site T; gamma / beta: the initializers g and b of the affine; channels: C; readers: every consumer of T
SmoothSite = collections.namedtuple("SmoothSite", "tensor gamma beta channels readers")
# node: the MatMul / Gemm's name; weight: its initializer; transposed: the weight is [N, C] (Gemm, transB = 1), else [C, N]
SmoothReader = collections.namedtuple("SmoothReader", "node weight transposed")


def _last_axis_vector(graph, name):
    """Elements of initializer `name` if its shape broadcasts along the last axis only ([C] or [1, ..., 1, C]); else 0."""
    if name not in graph.initializer:
        return 0
    shape = tuple(np.asarray(graph.initializer[name]).shape)
    if len(shape) < 1 or any(d != 1 for d in shape[:-1]):
        return 0
    return int(shape[-1])


def _affine_operands(graph, node):
    """(activation, initializer, C) of a two-input node one of whose operands (either) is a last-axis vector; else None."""
    if len(node.input) != 2:
        return None
    for act, init in (tuple(node.input), tuple(node.input)[::-1]):
        c = _last_axis_vector(graph, init)
        if c and act not in graph.initializer:
            return act, init, c
    return None


def _reader(graph, node, tensor, channels):
    """The SmoothReader of `node` if it is a MatMul / Gemm that multiplies `tensor` (on the left) by a constant [C, N] matrix."""
    if node.op_type == "MatMul":
        if len(node.input) != 2 or node.input[0] != tensor or node.input[1] not in graph.initializer:
            return None
        w = np.asarray(graph.initializer[node.input[1]])
        return SmoothReader(node.name, node.input[1], False) if w.ndim == 2 and w.shape[0] == channels else None
    if node.op_type == "Gemm":
        if len(node.input) < 2 or node.input[0] != tensor or node.attrs.get("transA", 0) or node.input[1] not in graph.initializer:
            return None
        if tensor in node.input[1:]:
            return None
        w = np.asarray(graph.initializer[node.input[1]])
        trans = bool(node.attrs.get("transB", 0))
        return SmoothReader(node.name, node.input[1], trans) if w.ndim == 2 and w.shape[1 if trans else 0] == channels else None
    return None


def find_smooth_sites(graph):
    """Every site of `graph`, in graph order (the rule: the module's docstring and DESIGN; anything else is left alone)."""
    def read_once(name):
        return len(graph.input_map.get(name, ())) == 1

    sites = []
    for add in graph.graph.node:
        if add.op_type != "Add":
            continue
        top = _affine_operands(graph, add)
        if top is None:
            continue
        y, beta, c = top
        mul = graph.get_tensor_producer(y)
        if isinstance(mul, str) or mul.op_type != "Mul":
            continue
        inner = _affine_operands(graph, mul)
        if inner is None or inner[2] != c:
            continue
        gamma = inner[1]
        after = graph.get_tensor_consumer(y)       # Y feeds that Add and nothing else (by name: a copied graph's maps hold copies)
        if len(after) != 1 or isinstance(after[0], str) or after[0].name != add.name or y in graph.network_outputs:
            continue
        t = add.output[0]
        if t in graph.network_outputs:
            continue
        readers = []
        for node in graph.get_tensor_consumer(t):
            r = None if isinstance(node, str) else _reader(graph, node, t, c)
            if r is None:
                readers = None
                break
            readers.append(r)
        if not readers:
            continue
        if gamma == beta or not all(read_once(n) for n in [gamma, beta] + [r.weight for r in readers]):
            continue
        sites.append(SmoothSite(t, gamma, beta, c, tuple(readers)))
    return sites


def smooth_scales(a, w, alpha):
    """s = a^alpha / w^(1 - alpha) per channel, computed in fp64 and cast to fp32; 1 where a < 1e-6 or w < 1e-6 (`--we`'s guard) and
    where the value is not a positive finite fp32 number."""
    a, w = np.asarray(a, np.float64).reshape(-1), np.asarray(w, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        s = (np.power(a, float(alpha)) / np.power(w, 1.0 - float(alpha))).astype(np.float32)
    bad = (a < 1e-6) | (w < 1e-6) | ~np.isfinite(s) | ~(s > 0)
    return np.where(bad, np.float32(1.0), s).astype(np.float32)


def _weight_rows_absmax(graph, site):
    """w_j: the largest |W[j, :]| over the site's readers, fp32 [C]."""
    w = np.zeros(site.channels, np.float32)
    for r in site.readers:
        m = np.abs(np.asarray(graph.get_initializer(r.weight), np.float32))
        w = np.maximum(w, m.max(0 if r.transposed else 1))
    return w


def apply_smooth(graph, sites, stats, alpha):
    """-> (a copy of `graph` with every site folded, {site tensor: s fp32 [C]}).  stats: {site tensor: a fp32 [C]}."""
    out = ONNXGraph()
    out.copy_from(graph)
    scales = {}
    for site in sites:
        s = smooth_scales(stats[site.tensor], _weight_rows_absmax(out, site), alpha)
        scales[site.tensor] = s
        for name in (site.gamma, site.beta):
            v = np.asarray(out.get_initializer(name), np.float32)
            update_weight(out, v / s.reshape(v.shape), name)
        for r in site.readers:
            w = np.asarray(out.get_initializer(r.weight), np.float32)
            update_weight(out, w * (s[None, :] if r.transposed else s[:, None]), r.weight)
    out.update_model()
    return out, scales


@torch.no_grad()
def smooth_statistics(graph, sites, args, session=None):
    """{site tensor: max |T[..., j]| over the calibration images, fp32 [C]}: one forward per chunk of this rank's shard exposing
    the site tensors only, ops.colwise_absmax of each into its slice of ONE [sum C] device buffer, one read-back at the end.  With
    several ranks the buffer is all-reduced (MAX, on the bit patterns like the kernel: order-free, NaN kept) first, so every rank
    returns the same values.  session: a GraphSession of `graph` on the current device to run the forwards on (default: a new one)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    world = int(getattr(args, "world_size", 1) or 1)
    world = world if dist_helper.active(world) else 1
    st, ed = dist_helper.balanced_shard(args.data_num, int(getattr(args, "rank", 0)) if world > 1 else 0, world)
    names = [s.tensor for s in sites]
    offs = np.concatenate([[0], np.cumsum([s.channels for s in sites])]).astype(np.int64)
    buf = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
    if ed > st:
        sess = session if session is not None else GraphSession(graph, device=dev)
        bounds, inputs = load_chunks(graph, args, st, ed, dev)
        for c in range(len(bounds)):
            outs = sess.run_named({n: v[c] for n, v in inputs.items()}, names)
            for k, t in enumerate(outs):
                ops.colwise_absmax(t, acc=buf[offs[k]:offs[k + 1]])
    if world > 1:
        dist.all_reduce(buf.view(torch.int32), op=dist.ReduceOp.MAX)
    host = buf.cpu().numpy()
    return {n: host[offs[k]:offs[k + 1]].copy() for k, n in enumerate(names)}


def smooth_quant(graph, args):
    """-> the smoothed graph (rank 0 saves it as smooth_model.onnx); `graph` itself, nothing written, where it has no site.
    Every rank calls it (the statistics are shared over the process group) and ends with the same model."""
    sites = find_smooth_sites(graph)
    rank = dist_helper.rank()
    if not sites:
        if rank == 0:
            logger.info("--smooth: no LayerNorm affine feeding only MatMul / Gemm weights in this graph: nothing to do")
        return graph
    alpha = float(getattr(args, "smooth_alpha", 0.5))
    stats = smooth_statistics(graph, sites, args)
    graph_s, scales = apply_smooth(graph, sites, stats, alpha)
    if rank == 0:
        for site in sites:
            a, s = stats[site.tensor], scales[site.tensor]
            with np.errstate(all="ignore"):
                logger.info("Smooth: {} ({} channels, {} readers)  max|x| {:.4g} -> {:.4g}".format(
                    site.gamma, site.channels, len(site.readers), float(np.max(a)), float(np.max(a / s))))
        if getattr(args, "output_dir", None):
            graph_s.output_dir = args.output_dir
            graph_s.save_onnx_model("smooth_model")
    return graph_s
