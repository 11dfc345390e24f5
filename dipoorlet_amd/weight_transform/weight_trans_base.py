"""weight_calibration — counterpart of dipoorlet/weight_transform/weight_trans_base.py:15-68: the order in which
the weight transforms run and what is re-derived after each."""
import os

import torch.distributed as dist

from ..graph import ONNXGraph
from ..tensor_cali import find_clip_val_minmax_weight, tensor_calibration
from ..utils import load_clip_val, logger, reduce_clip_val, save_clip_val
from .adaround import adaround
from .bias_correction import bias_correction
from .brecq import brecq
from .gptq import gptq
from .rotate import mx_rotate
from .smooth import smooth_quant
from .sparse_quant import sparse_quant
from .update_bn import update_bn
from .weight_equalization import weight_equalization


def _reload(name, args):
    args.model = os.path.join(args.output_dir, name + ".onnx")        # utils.update_model_path
    return ONNXGraph.load(args.model, args.output_dir, args.deploy, getattr(args, "model_type", None))


def _recalibrate(graph, args):
    """Re-derive the ranges of a changed model on every rank and pass them through the same per-rank files ->
    rank-0 reduce -> load sequence as __main__ (so all ranks end with identical, JSON-rounded values)."""
    rank, world = dist.get_rank(), dist.get_world_size()
    act, weight = tensor_calibration(graph, args)
    save_clip_val(act, weight, args, act_fname=f"act_clip_val.json.rank{rank}",
                  weight_fname=f"weight_clip_val.json.rank{rank}")
    dist.barrier()
    if rank == 0:   # (as __main__: with the statistics merged over RCCL every rank already holds the whole set's clips)
        reduce_clip_val(world, args, already_merged=(getattr(args, "merge", "allreduce") != "reference"))
    dist.barrier()
    return load_clip_val(args)


def weight_calibration(onnx_graph, act_clip_val, weight_clip_val, args):
    """Returns (graph_after_wt, onnx_graph, act_clip_val, weight_clip_val) like the reference; every rank ends
    with the same model and ranges."""
    graph_after_wt = ONNXGraph()
    graph_after_wt.copy_from(onnx_graph)
    rank = dist.get_rank()

    def stage(flag, message, every_rank, run, saved, rederive, remark=None):
        """One transform that writes a model every rank goes on with: rank 0 says `message`; every rank — or rank 0 alone — runs
        `run(graph)`; barrier; everyone reloads <saved>.onnx and re-derives 'all' ranges or the 'weight' ranges (rank 0 says
        `remark` first).  A transform that hands back the graph it was given wrote nothing: that graph and its ranges stay."""
        nonlocal graph_after_wt, act_clip_val, weight_clip_val
        if not getattr(args, flag, False):
            return
        if rank == 0:
            logger.info(message)
        out = run(graph_after_wt) if every_rank or rank == 0 else None
        dist.barrier()
        if out is graph_after_wt:
            return
        graph_after_wt = _reload(saved, args)
        if remark and rank == 0:
            logger.info(remark)
        if rederive == "all":
            act_clip_val, weight_clip_val = _recalibrate(graph_after_wt, args)
        else:
            weight_clip_val = find_clip_val_minmax_weight(graph_after_wt, args)

    # --smooth, --mx_rotate (not in the reference): first, so that everything below sees their model, as after --we; the rotation
    # keeps --smooth's scales.  Every rank runs them (--smooth sweeps its statistics in shards; the rotation is host work).
    # --bc (:21-29): every rank corrects over its shard of the images (bias_correction); --merge reference: rank 0 alone, over all
    # images, as the reference.  Only biases change: the weight ranges alone are refreshed.  --we (:31-38), --update_bn (:40-53).
    bc_sharded = dist.get_world_size() > 1 and getattr(args, "merge", "allreduce") != "reference"
    stage("smooth", "Weight transform: smoothing MatMul inputs...", True, lambda g: smooth_quant(g, args), "smooth_model", "all")
    stage("mx_rotate", "Weight transform: rotating MX blocks...", True, lambda g: mx_rotate(g, args), "rotate_model", "all")
    if getattr(args, "mx_mixed", None) is not None:
        # --mx_mixed (not in the reference): on the model as --smooth / --mx_rotate leave it and before anything that runs the
        # fake-quantised graph, whose MX nodes take the chosen formats from here on (args.mx_formats).  Every rank runs it.
        from ..mx_mixed import mx_mixed
        if rank == 0:
            logger.info("Choosing MXFP4 or MXFP8 per node...")
        mx_mixed(graph_after_wt, args)
        dist.barrier()
    stage("bc", "Weight transform: bias correction...", bc_sharded,
          lambda g: bias_correction(g, act_clip_val, weight_clip_val, args), "update_bias_model", "weight")
    stage("we", "Weight transform: cross-layer equalisation...", False, lambda g: weight_equalization(g, args), "weight_equal_model", "all")
    stage("update_bn", "Weight transform: BN statistics of the quantised network...", False,
          lambda g: update_bn(g, act_clip_val, weight_clip_val, args, recalibrate=False), "update_bn_model", "all", "Re calibration...")
    if getattr(args, "sparse", False):     # :65-66 — instead of AdaRound / BRECQ
        args.acti_quant = False
        graph_after_wt = sparse_quant(onnx_graph, graph_after_wt, act_clip_val, weight_clip_val, args)
        return graph_after_wt, onnx_graph, act_clip_val, weight_clip_val
    if getattr(args, "adaround", False):   # :55-57
        args.acti_quant = False
        graph_after_wt = adaround(onnx_graph, graph_after_wt, act_clip_val, weight_clip_val, args)
    if getattr(args, "brecq", False):      # :59-64
        args.acti_quant = bool(getattr(args, "drop", False))
        graph_after_wt = brecq(onnx_graph, graph_after_wt, act_clip_val, weight_clip_val, args)
    if getattr(args, "gptq", False) or getattr(args, "mx_gptq", False):
        # (not in the reference) where AdaRound runs, instead of it; the ORIGINAL ranges stay.  --mx_gptq: the same driver over the
        # block-scaled MatMul / Gemm weights as well
        if dist.get_rank() == 0:
            logger.info("Weight transform: GPTQ{}...".format(" on the MX grids" if getattr(args, "mx_gptq", False) else ""))
        graph_after_wt, _ = gptq(onnx_graph, graph_after_wt, act_clip_val, weight_clip_val, args)
    return graph_after_wt, onnx_graph, act_clip_val, weight_clip_val
