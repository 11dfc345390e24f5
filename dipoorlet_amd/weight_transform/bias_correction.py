"""`--bc` bias correction on the GPU — counterpart of dipoorlet/weight_transform/bias_correction.py:9-55
(and its call site weight_trans_base.py:21-29).

Reference: for every Conv / Gemm node in topological order it re-builds the fake-quantised graph,
creates one ONNXRuntime session per node through the host-side ActivationCache (forward_net.py:23-190),
pulls the node's fp and quantised outputs for ALL N images to the host and adds mean(fp - q) over
(N, H, W) to the bias, so that later nodes see the corrected upstream biases.

Here the whole calibration set's frontier stays resident in HBM and the two networks (fp and
fake-quantised) are walked ONCE, node-major: each node is executed for all images before the next one
starts (executor.Frontier: activations are kept as lists of per-chunk device tensors and freed by reference count), so the
sequential dependence "correct bias k, then everything downstream sees it" costs O(nodes) node
executions instead of O(nodes^2).  The bias enters a Conv / Gemm output linearly, so after the update the
already computed quantised output is fixed up in place (q_out += diff) instead of being recomputed.
The fake-quant structure does not depend on bias values, so the quantised graph is built once.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from .. import ops
from ..dist_helper import active, balanced_shard as bc_shard
from ..executor import Frontier, GraphSession, frontier_peak_elems
from ..utils import logger
from .walk import QuantWalk

BIAS_CORRECTION_NODE_TYPE = ["Conv", "Gemm"]


def _channel_mean_diff(fp_chunks, q_chunks, is_conv, world_size=1, n_ch=None):
    """bias_correction.py:10-13 — mean(fp - q) over every axis but the channel one (axis 1 of a Conv output
    [n, C, spatial...]; the last axis of a Gemm output [n, C]): one fused kernel per chunk pair, fp64 sums.
    world_size > 1: the chunks are this rank's shard of the images; the per-channel fp64 sums and the count are added up over
    the ranks (ONE all-reduce of [C + 1] doubles per node), so every rank returns the mean over the whole set."""
    acc, cnt = None, 0
    dev = torch.device("cuda", torch.cuda.current_device())
    if n_ch is not None:        # (a rank whose shard is empty still joins the all-reduce)
        acc = torch.zeros(int(n_ch), dtype=torch.float64, device=dev)
    for a, b in zip(fp_chunks, q_chunks):
        a, b = a.to(dev, non_blocking=True), b.to(dev, non_blocking=True)   # (no-ops unless the frontier is kept on the host)
        if not is_conv:
            a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
        acc = ops.channel_diff_sum(a.contiguous(), b.contiguous(), acc)
        cnt += a.numel() // a.shape[1]
    if world_size > 1:
        packed = torch.cat([acc, torch.tensor([float(cnt)], dtype=torch.float64, device=acc.device)])
        dist.all_reduce(packed, op=dist.ReduceOp.SUM)
        return (packed[:-1] / packed[-1]).float()
    return (acc / cnt).float()


def update_conv_node_bias(graph_bc, node, fp_activations, q_activations, world_size=1):
    """bias_correction.py:9-31 on device tensors: bias += mean(fp - q) over every axis but the channel one (Conv output
    chunks [n, C, H, W], Gemm output chunks [n, C]); a node without a bias input gets `<node>_bias`.  Returns the
    per-channel difference (fp32 device tensor) that was added.  `*_activations`: lists of per-chunk device tensors
    (world_size > 1: of this rank's shard; the mean is over all ranks' images)."""
    bc_node = next(n for n in graph_bc.graph.node if n.name == node.name)
    n_ch = None
    if world_size > 1:          # the channel count from the weights: [C_out, ...] (Conv; Gemm with transB), [K, C_out] (Gemm)
        w = graph_bc.get_initializer(bc_node.input[1])
        n_ch = w.shape[0] if (node.op_type == "Conv" or bc_node.attrs.get("transB", 0)) else w.shape[1]
    diff = _channel_mean_diff(fp_activations, q_activations, node.op_type == "Conv", world_size, n_ch)
    if len(bc_node.input) > 2:
        bname = bc_node.input[2]
        new_bias = graph_bc.get_initializer(bname).astype(np.float32) + diff.cpu().numpy()
    else:
        bname = node.name + "_bias"
        new_bias = diff.cpu().numpy()
        bc_node.input.append(bname)
        graph_bc.input.append(bname)
    graph_bc.set_initializer(bname, new_bias.astype(np.float32))
    return diff


@torch.no_grad()
def bias_correction(graph, act_clip_val, weight_clip_val, args):
    """bias_correction.py:34-55 -> the bias-corrected graph (also saved as update_bias_model.onnx)."""
    walk = QuantWalk(graph, act_clip_val, weight_clip_val, args)
    graph_bc, graph_q, s_q = walk.graph_new, walk.graph_q, walk.s_q
    s_fp = GraphSession(graph, device=walk.dev)
    # The reference lets rank 0 walk ALL images while the others wait (weight_trans_base.py:21-29, forward_net.py:50-52).  The
    # correction is a per-channel SUM over images, so with several ranks each walks its shard of the images node-major as
    # before and the sums are all-reduced per Conv / Gemm node (RCCL): every rank holds the same corrected biases, and its
    # frontier is 1 / world of the set.  args.merge == 'reference' keeps the reference's schedule.
    world = int(getattr(args, "world_size", 1) or 1)
    sharded = getattr(args, "merge", "allreduce") != "reference" and active(world)
    st, ed = bc_shard(args.data_num, int(getattr(args, "rank", 0)), world) if sharded else (0, args.data_num)
    world = world if sharded else 1
    N = ed - st
    # HBM budget: the two frontiers hold the WHOLE set's live activations.  Refuse up front with a plain message rather than
    # die in the allocator halfway through (the other ranks would be left at the next barrier).
    need = 4.0 * N * (frontier_peak_elems(s_fp) + frontier_peak_elems(s_q))
    budget = float(getattr(args, "resident_gb", 160.0) or 160.0) * 1e9
    on_host = need > budget
    if on_host:
        logger.warning("--bc: the live activations of all %d images of both networks are about %.0f GB at the widest point of "
                       "this graph, over the %.0f GB budget (--resident_gb): keeping them in host memory between nodes",
                       N, need / 1e9, budget / 1e9)
    qf = walk.start(st, ed, on_host)
    fp = Frontier(s_fp, walk.bounds, qf.env, on_host)       # (the same input chunks)
    fp_nodes = {n.name: n for n in graph.graph.node}
    # DPL_BC_RECOMPUTE=1 (a testing aid): a corrected node's quantised output is computed AGAIN with the corrected bias instead of
    # being fixed up in place (q_out + diff).  The two are the same value up to one fp32 rounding — conv(x, w, b) + d against
    # conv(x, w, b + d) — but a last-bit difference flips a rounding step of a fake-quantised layer downstream now and then; with
    # the recomputation the walk IS the reference's definition evaluated node-major (tests/test_cli_e2e.py compares them exactly).
    recompute = os.environ.get("DPL_BC_RECOMPUTE") == "1"
    for node in graph_q.graph.node:
        if node.name not in fp_nodes:
            qf.run(node)
            continue  # a FakeQuant node
        fp_node = fp_nodes[node.name]
        corrected = node.op_type in BIAS_CORRECTION_NODE_TYPE
        out = node.output[0]
        if corrected:
            fp.hold(fp_node.output[0])      # hold both outputs for the diff BEFORE the nodes run: an output nobody consumes is
            qf.hold(out)                    # dropped at once
            if recompute:                   # (... and the inputs for the second run)
                for i in qf.inputs_of(node):
                    qf.hold(i)
        qf.run(node)
        fp.run(fp_node)
        if not corrected:
            continue
        logger.info("Update bias for node: {}".format(node.name))
        bc_node = next(n for n in graph_bc.graph.node if n.name == node.name)
        diff = update_conv_node_bias(graph_bc, node, fp.env[out], qf.env[out], world)
        if recompute:
            bname = bc_node.input[2]
            if len(node.input) < 3:       # (a node without a bias has just been given one)
                node.input.append(bname)
            walk.set_const(bname, torch.from_numpy(np.ascontiguousarray(graph_bc.get_initializer(bname), dtype=np.float32)))
            qf.run(node)
        elif qf.env[out]:
            shape = [1, -1] + [1] * (qf.env[out][0].dim() - 2)
            d_host = diff.reshape(shape).cpu() if on_host else None
            for t in qf.env[out]:  # the bias is additive in the output: fix the computed q output in place
                t.add_(d_host if on_host else diff.reshape(shape))
        fp.drop(fp_node.output[0])
        qf.drop(out)
    return walk.finish("update_bias_model")
