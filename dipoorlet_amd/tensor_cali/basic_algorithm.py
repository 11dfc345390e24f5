"""Activation clip-range search: the three registry algorithms of the reference
(dipoorlet/tensor_cali/basic_algorithm.py:8-69) plus the per-channel weight ranges (:72-91), computed
on the MI355X — and, in registries of their own, the entropy search `kl` the reference never shipped
(tensor_cali_extensions) and the quantisation-MSE search `qmse` on the platform's own grid (tensor_cali_grid_aware).

Registry keys, call form and return type are the reference's: `tensor_cali_dispatcher(key, graph, args)`
-> {tensor_name: [lo, hi]} with numpy scalars (they must support .tolist(), utils.py:314-316); an
unknown key logs "Calibration Algorithm Not Found!" and returns None.

Multi-rank: with args.world_size > 1 and args.merge != 'reference' (default) the per-rank statistics
are merged with RCCL collectives (dist_helper.merge_*), so every rank returns the clip ranges of the
WHOLE calibration set — equal to the reference run with world_size = 1.  args.merge == 'reference'
keeps the reference's behaviour: per-rank ranges / histograms / means, to be averaged afterwards by
utils.reduce_clip_val exactly as __main__.py:121-128 does.
"""
import numpy as np
import torch

from .. import ops
from ..dist_helper import gather_rows, merge_hist, merge_ranges
from ..forward_net import (CalibrationRun, forward_get_minmax, forward_net_octav, hist_pass)
from ..platform_settings import LAYER_HAS_WEIGHT, platform_setting_table
from ..utils import dispatch_functool, logger


@dispatch_functool
def tensor_cali_dispatcher(*args, **kwargs):
    logger.info("Calibration Algorithm Not Found!")


@dispatch_functool
def tensor_cali_extensions(*args, **kwargs):
    """Algorithms beyond the reference's three: same call form as tensor_cali_dispatcher, a registry of its own (the reference
    answers their keys with "Calibration Algorithm Not Found!", and tensor_cali_dispatcher keeps doing so)."""
    logger.info("Calibration Algorithm Not Found!")


@dispatch_functool
def tensor_cali_grid_aware(*args, **kwargs):
    """Algorithms whose answer depends on the platform's number format (its qi_params): same call form, a registry of its own —
    tensor_cali_extensions holds the format-blind additions."""
    logger.info("Calibration Algorithm Not Found!")


def _merged(args):
    return getattr(args, "world_size", 1) > 1 and getattr(args, "merge", "allreduce") != "reference"


def _as_clip_dict(names, lo, hi):
    lo = lo.detach().cpu().numpy().astype(np.float32, copy=False)
    hi = hi.detach().cpu().numpy().astype(np.float32, copy=False)
    return {n: [lo[t], hi[t]] for t, n in enumerate(names)}


@tensor_cali_dispatcher.register("minmax")
def find_clip_val_minmax(onnx_graph, args, run=None, **kwargs):
    """basic_algorithm.py:13-22 — [min over images, max over images] per tensor.
    run: a CalibrationRun over (onnx_graph, args) to sweep with (tensor_calibration builds one); default: a new one."""
    run = run or CalibrationRun(onnx_graph, args)
    forward_get_minmax(onnx_graph, args, run=run)
    gmin, gmax = run.acc.gmin, run.acc.gmax
    if _merged(args):
        merge_ranges(gmin, gmax, args.world_size)
    return _as_clip_dict(run.names, gmin, gmax)


def _hist_statistics(onnx_graph, args, store_stats=None, run=None):
    """The two sweeps of the histogram algorithms (ranges, then |x| histograms over them) and their merge over ranks
    -> (acc, names): ops.CalibAccumulators with gmin / gmax / hist of every tensor, and the tensors' names.

    store_stats = {'minmax': {name: {'min': [...], 'max': [...]}}, 'hist': {name: int64[bins]}} skips the
    sweeps (the reference's unused hook, basic_algorithm.py:26-29): the statistics are installed as given."""
    bins = int(args.bins)  # the reference leaves a CLI --bins as str and crashes at :47; int() is the fix
    if store_stats:
        names = list(store_stats["hist"].keys())
        dev = torch.device("cuda", torch.cuda.current_device())
        acc = ops.CalibAccumulators(len(names), dev, bins)
        mm = store_stats["minmax"]
        acc.set_minmax(torch.tensor([float(np.min(mm[n]["min"])) for n in names], dtype=torch.float32, device=dev),
                       torch.tensor([float(np.max(mm[n]["max"])) for n in names], dtype=torch.float32, device=dev))
        acc.hist_prepare()
        acc.hist.copy_(torch.from_numpy(np.stack([np.asarray(store_stats["hist"][n], np.int64) for n in names])))
    else:
        run = run or CalibrationRun(onnx_graph, args)
        forward_get_minmax(onnx_graph, args, run=run, keep_resident=True)   # pass 1
        gmin, gmax = run.acc.gmin.clone(), run.acc.gmax.clone()
        if _merged(args):
            merge_ranges(gmin, gmax, args.world_size)
        acc = hist_pass(run, gmin, gmax, bins)                                # pass 2
        if _merged(args):
            merge_hist(acc.hist, args.world_size)
        names = run.names
    return acc, names


@tensor_cali_dispatcher.register("hist")
def find_clip_val_hist(onnx_graph, args, store_stats=None, run=None, **kwargs):
    """basic_algorithm.py:25-54 — percentile (cumulative mass >= args.threshold) of the |x| histogram.

    store_stats: _hist_statistics — only the percentile search runs on the device."""
    acc, names = _hist_statistics(onnx_graph, args, store_stats, run)
    clip = acc.hist_percentile(float(args.threshold))
    return _as_clip_dict(names, clip[:, 0], clip[:, 1])


def kl_levels(deploy):
    """Quantisation levels per sign of the platform's activations: 2 ** (bit_width - 1) of its qi_params."""
    return 2 ** (int(platform_setting_table[deploy]["qi_params"]["bit_width"]) - 1)


@tensor_cali_extensions.register("kl")
def find_clip_val_kl(onnx_graph, args, store_stats=None, run=None, **kwargs):
    """Entropy calibration — not in the reference, which names "kl" in its --bins help and never shipped one: the clip that
    loses the least information (KL divergence) when the |x| histogram is cut at a candidate bin and quantised to the platform's
    levels.  The definition is this project's (tests/kl_model.py), searched on the device in one launch (k_hist_kl)
    over the very histograms `-A hist` accumulates — same sweeps, same merge over ranks, same store_stats hook.
    args.threshold is not used; args.bins must be at least the platform's levels (128)."""
    levels = kl_levels(args.deploy)
    if int(args.bins) < levels:
        raise ValueError(f"-A kl needs --bins >= {levels} (the quantisation levels of '{args.deploy}'), got {int(args.bins)}")
    acc, names = _hist_statistics(onnx_graph, args, store_stats, run)
    clip, _, _ = acc.hist_kl(levels)
    return _as_clip_dict(names, clip[:, 0], clip[:, 1])


@tensor_cali_grid_aware.register("qmse")
def find_clip_val_qmse(onnx_graph, args, store_stats=None, run=None, **kwargs):
    """Quantisation-MSE calibration — not in the reference, whose `mse` is OCTAV (a per-image fixed point, for a uniform grid):
    the clip of least mean squared error when the centres of the |x| histogram's bins are fake-quantised on the platform's own
    activation grid — the integers of its bit width, or the OCP FP8 E4M3 codes of `-D ocp_fp8` — for every candidate bin.  The
    definition is this project's (tests/qmse_model.py), searched on the device in one launch (k_hist_qmse) over the
    very histograms `-A hist` accumulates — same sweeps, same merge over ranks, same store_stats hook.
    args.threshold is not used; the lowest candidate is the platform's level count (128), which args.bins must reach."""
    first = kl_levels(args.deploy)
    if int(args.bins) < first:
        raise ValueError(f"-A qmse needs --bins >= {first} (the quantisation levels of '{args.deploy}'), got {int(args.bins)}")
    qi = platform_setting_table[args.deploy]["qi_params"]
    acc, names = _hist_statistics(onnx_graph, args, store_stats, run)
    clip, _, _ = acc.hist_qmse(qi["type"], qi["bit_width"], first)
    return _as_clip_dict(names, clip[:, 0], clip[:, 1])


@tensor_cali_dispatcher.register("mse")
def find_clip_val_octav(onnx_graph, args, run=None, **kwargs):
    """basic_algorithm.py:57-69 — OCTAV scale per image, then [max(min_all, -mean s), min(max_all, mean s)].
    The mean is taken with numpy in fp32 over the per-image list exactly as the reference does, so it is
    reproduced bit for bit given the per-image scales (python max/min: a NaN mean falls back to the range)."""
    run = run or CalibrationRun(onnx_graph, args)
    forward_net_octav(onnx_graph, args, run=run, as_dict=False)
    rows = run.octav_rows
    if _merged(args):
        rows = gather_rows(rows, args.world_size)
    r = rows.detach().cpu().numpy().astype(np.float32, copy=False)
    # [3, T, n] contiguous: row [k, t] is what the reference's np.array(list_of_per_image_values) holds — a contiguous fp32
    # vector in image order — so numpy's mean / max / min over it are the reference's, bit for bit
    cols = np.ascontiguousarray(r.transpose(2, 1, 0))
    clip_val = {}
    for t, name in enumerate(run.names):
        with np.errstate(all="ignore"):
            mean_s = cols[0, t].mean()
        data_max = cols[2, t].max()
        data_min = cols[1, t].min()
        clip_val[name] = [max(data_min, -mean_s), min(data_max, mean_s)]
    return clip_val


def find_clip_val_minmax_weight(onnx_graph, args, session=None):
    """basic_algorithm.py:72-91 — per output channel [min, max] of every initializer input (node.input[1:])
    of Conv / Gemm / ConvTranspose / PRelu / BatchNormalization; ConvTranspose weights are viewed
    [1,0,2,3]-transposed; 0-d initializers are skipped.  Row reductions run in k_rowwise_minmax.

    session: an executor session of THIS graph — its initializers are on the device already (one transfer at session
    build) and are reduced where they lie; without one every initializer is uploaded here."""
    weight_tensor, need_transpose = {}, []
    for node in onnx_graph.graph.node:
        if node.op_type in LAYER_HAS_WEIGHT:
            for in_tensor in list(node.input)[1:]:
                weight_tensor[in_tensor] = onnx_graph.get_initializer(in_tensor)
            if node.op_type == "ConvTranspose":
                need_transpose.append(node.input[1])
    dev = torch.device("cuda", torch.cuda.current_device())
    resident = getattr(session, "consts", None) or {}
    todo = [(name, np.asarray(t)) for name, t in weight_tensor.items() if np.asarray(t).ndim >= 1]
    if not todo:
        return {}
    # every row's (min, max) into ONE device buffer, read back in one transfer (a round trip per initializer — 161 of them for
    # ResNet-50 — was a tenth of a second of a run)
    rows = [t.shape[1] if name in need_transpose else t.shape[0] for name, t in todo]
    res = torch.empty(2, sum(rows), dtype=torch.float32, device=dev)
    off = 0
    for (name, tensor), c in zip(todo, rows):
        w = resident.get(name)
        if w is not None and w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == tuple(tensor.shape):
            if name in need_transpose:
                w = w.permute(1, 0, 2, 3)
            w2 = w.reshape(c, -1).contiguous()
        else:
            if name in need_transpose:
                tensor = tensor.transpose([1, 0, 2, 3])
            w2 = torch.from_numpy(np.ascontiguousarray(tensor.reshape(c, -1), dtype=np.float32)).to(dev, non_blocking=True)
        ops.rowwise_minmax(w2, out=(res[0, off:off + c], res[1, off:off + c]))
        off += c
    flat = res.cpu().numpy()
    out, off = {}, 0
    for (name, _), c in zip(todo, rows):
        out[name] = [flat[0, off:off + c].copy(), flat[1, off:off + c].copy()]
        off += c
    return out
