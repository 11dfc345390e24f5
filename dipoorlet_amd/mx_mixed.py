"""`--mx_mixed BITS` — MXFP4 or MXFP8 per node under a weight-bit budget (not in the reference; with `--mx mxfp4` only; the
definition is tests/mx_mixed_model.py).

`--mx` takes one element format for the whole network.  MXFP4 everywhere is the format worth having for weight bytes and
matrix-core rate, and most of what it costs sits in a few layers; this says which layers to keep at MXFP8, given how many bits
may be spent: BITS in [4, 8], the average element bits over the weights of the candidate nodes.

Candidates   every Gemm with no transA, alpha = beta = 1 and a bias that is absent or a constant 1-D [n], and every MatMul, whose
             right operand is a constant 2-D weight that nothing else reads.  Everything else that `--mx` block-scales stays at the
             base format and is listed with its reason (LEFT_*).
Measurement  the first --calib_batch images through the UN-quantised graph as it stands after --smooth / --mx_rotate.  Per
             candidate: the activation its MX node would read (under --mx_rotate the BlockHadamard output), encoded along K as
             E2M1 and as E4M3 (ops.mx_encode); its weight as it stands, encoded once in each format; ops.mx_gemm_err of the two
             same-format pairs against the node's own fp32 output, with its bias — the product on the block-scaled matrix
             instruction, its error summed in the kernel's epilogue, C never written.  The partials are added in
             fp64: e4 = sum d^2 / sum ref^2, e8 likewise.  Several ranks take a balanced share of the images each and add their
             sums over the process group (as --smooth shares its statistics), so every rank ends with the same numbers.
Choice       choose(): every candidate starts at mxfp4; gain = e4 - e8, cost = 4 bits for each of the weight's K * N elements;
             candidates whose gain is <= 0 or not finite are dropped; the rest go by gain / cost, descending, ties in graph order;
             one walk promotes a node when the promoted costs stay <= (BITS - 4) * (the elements of all candidates) — a node that
             does not fit is skipped and the walk goes on.  Both operands of a promoted node become mxfp8.
-> {node name: format} of the candidates, which quantize.insert_fake_quant_node consults (args.mx_formats) in place of
platform_settings.mx_setting(args.mx); rank 0 writes mx_mixed_report.json.
"""
import json
import math
import os

import numpy as np

from .utils import logger

REPORT = "mx_mixed_report.json"
BASE, WIDE = "mxfp4", "mxfp8"
ELEM_BITS = {BASE: 4, WIDE: 8}
LEFT_TWO_ACTIVATIONS = "a product of two activations"
LEFT_CONSTANT_LEFT = "a constant left operand"
LEFT_SHARED = "other nodes read its weight"
LEFT_RANK = "a constant of rank {}, not 2"
LEFT_CONV = "a Conv (--mx_conv block-scales it at the base format)"
LEFT_GEMM = "a Gemm with {}"


def why_left(graph, node):
    """None if `node` (a MatMul / Gemm of the un-quantised graph) is a candidate, else the reason it stays at the base format."""
    if len(node.input) < 2 or node.input[0] == "" or node.input[1] == "":
        return "fewer than two operands"
    a, w = node.input[0], node.input[1]
    if node.op_type == "Gemm":
        if int(node.attrs.get("transA", 0) or 0):
            return LEFT_GEMM.format("transA")
        if float(node.attrs.get("alpha", 1.0)) != 1.0 or float(node.attrs.get("beta", 1.0)) != 1.0:
            return LEFT_GEMM.format("alpha or beta other than 1")
    if a in graph.initializer:
        return LEFT_CONSTANT_LEFT
    if w not in graph.initializer:
        return LEFT_TWO_ACTIVATIONS
    wv = np.asarray(graph.initializer[w])
    if wv.ndim != 2:
        return LEFT_RANK.format(wv.ndim)
    if len(graph.input_map.get(w, ())) != 1:
        return LEFT_SHARED
    if node.op_type == "Gemm" and len(node.input) > 2 and node.input[2] != "":
        n = int(wv.shape[0 if int(node.attrs.get("transB", 0) or 0) else 1])
        if node.input[2] not in graph.initializer or tuple(np.asarray(graph.initializer[node.input[2]]).shape) != (n,):
            return LEFT_GEMM.format("a bias that is no constant [n]")
    return None


def find_candidates(graph, args):
    """-> (the candidate nodes in graph order, {name: reason} of every other node that --mx block-scales)."""
    from .platform_settings import platform_setting_table
    from .quantize import MX_NODES, mx_conv_nodes
    quant_nodes = platform_setting_table[args.deploy]["quant_nodes"]
    skipped = set(getattr(args, "skip_layers", None) or ())
    taken, left = [], {}
    conv = set(mx_conv_nodes(graph, args)[0]) if getattr(args, "mx_conv", False) else set()
    for node in graph.graph.node:
        if node.name in skipped or node.op_type not in quant_nodes:
            continue
        if node.name in conv:
            left[node.name] = LEFT_CONV
        elif node.op_type in MX_NODES:
            why = why_left(graph, node)
            if why is None:
                taken.append(node)
            else:
                left[node.name] = why
    return taken, left


def choose(entries, bits):
    """entries: (name, e4, e8, elements) per candidate in graph order -> {name: "mxfp4" | "mxfp8"} (tests/mx_mixed_model.py choose)."""
    entries = list(entries)
    budget = (float(bits) - 4.0) * sum(int(e[3]) for e in entries)
    ranked = []
    for pos, (name, e4, e8, elements) in enumerate(entries):
        gain, cost = float(e4) - float(e8), 4 * int(elements)
        if math.isfinite(gain) and gain > 0.0:
            ranked.append((-(gain / cost), pos, name, cost))
    ranked.sort(key=lambda r: (r[0], r[1]))
    fmt = {e[0]: BASE for e in entries}
    spent = 0
    for _, _, name, cost in ranked:
        if spent + cost <= budget:
            spent += cost
            fmt[name] = WIDE
    return fmt


def measure(graph, nodes, args):
    """-> fp64 [len(nodes), 5] on the host: per candidate sum d^2 and sum ref^2 under mxfp4, the same under mxfp8, and the rows of
    its product, over the first --calib_batch images (every rank its share; summed over the process group)."""
    import torch
    import torch.distributed as dist

    from . import dist_helper, ops
    from .forward_net import ActivationCache
    from .quantize import mx_block_axis
    images = max(1, min(int(args.data_num), int(getattr(args, "calib_batch", None) or 16)))
    world = int(getattr(args, "world_size", 1) or 1)
    world = world if dist_helper.active(world) else 1
    st, ed = dist_helper.balanced_shard(images, int(getattr(args, "rank", 0)) if world > 1 else 0, world)
    dev = torch.device("cuda", torch.cuda.current_device())
    sums = torch.zeros((len(nodes), 5), dtype=torch.float64, device=dev)
    if ed > st and nodes:
        cache = ActivationCache(graph, args, st, ed)
        for i, node in enumerate(nodes):
            w = torch.from_numpy(np.ascontiguousarray(graph.get_initializer(node.input[1]), dtype=np.float32)).to(dev)
            axis = mx_block_axis(node, 1, tuple(w.shape)) % 2
            k, n = int(w.shape[axis]), int(w.shape[1 - axis])
            bias = None
            if node.op_type == "Gemm" and len(node.input) > 2 and node.input[2] != "":
                bias = torch.from_numpy(np.ascontiguousarray(graph.get_initializer(node.input[2]), dtype=np.float32)).to(dev)
            packed_w = {elem: ops.mx_encode(w, axis, elem) for elem in (BASE, WIDE)}
            for x, ref in zip(cache.chunks(node.input[0]), cache.chunks(node.output[0])):
                if x.dim() < 2 or int(x.shape[-1]) != k or ref.numel() != (x.numel() // k) * n:
                    raise ValueError(f"--mx_mixed: {node.name}: an input of shape {list(x.shape)} and an output of {list(ref.shape)} "
                                     f"for a [{k}, {n}] weight")
                x2, ref2 = x.reshape(-1, k).contiguous(), ref.reshape(-1, n).contiguous()
                for j, elem in enumerate((BASE, WIDE)):
                    part = ops.mx_gemm_err(*ops.mx_encode(x2, -1, elem), *packed_w[elem], ref2, elem, bias=bias)
                    sums[i, 2 * j:2 * j + 2] += part.sum(dim=(0, 1))
                sums[i, 4] += x2.shape[0]
        cache.reset()
    if world > 1:
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    return sums.cpu().numpy(), images


def mx_mixed(graph, args):
    """-> {node name: "mxfp4" | "mxfp8"} for every candidate of `graph` (also kept as args.mx_formats); rank 0 writes
    mx_mixed_report.json.  Every rank calls it and ends with the same choice."""
    from . import dist_helper
    bits = float(args.mx_mixed)
    nodes, left = find_candidates(graph, args)
    sums, images = measure(graph, nodes, args)
    entries, report = [], {}
    for node, (d4, r4, d8, r8, rows) in zip(nodes, sums.tolist()):
        w = np.asarray(graph.initializer[node.input[1]])
        k_axis = 1 if node.op_type == "Gemm" and int(node.attrs.get("transB", 0) or 0) else 0
        e4, e8 = (d / r if r > 0.0 else float("nan") for d, r in ((d4, r4), (d8, r8)))
        entries.append((node.name, e4, e8, int(w.size)))
        report[node.name] = {"op": node.op_type, "m": int(rows), "n": int(w.shape[1 - k_axis]), "k": int(w.shape[k_axis]), "weight": node.input[1],
                             "elements": int(w.size), "err": {BASE: e4, WIDE: e8}, "gain": e4 - e8}
    fmt = choose(entries, bits)
    total = sum(e[3] for e in entries)
    average = sum(ELEM_BITS[fmt[e[0]]] * e[3] for e in entries) / total if total else float(ELEM_BITS[BASE])
    for name, f in fmt.items():
        report[name]["format"] = f
    args.mx_formats = dict(fmt)
    if dist_helper.rank() == 0:
        for name, why in left.items():
            logger.info("--mx_mixed: {} stays at {}: {}".format(name, args.mx, why))
        for name, e in report.items():
            logger.info("--mx_mixed: {} {} [{} x {} x {}] relative error mxfp4 {:.4e}, mxfp8 {:.4e} -> {}".format(
                e["op"], name, e["m"], e["n"], e["k"], e["err"][BASE], e["err"][WIDE], e["format"]))
        logger.info("--mx_mixed {:g}: {} of {} candidate(s) at mxfp8, {:.4f} bits per weight element; {} node(s) left at {}".format(
            bits, sum(f == WIDE for f in fmt.values()), len(fmt), average, len(left), args.mx))
        if getattr(args, "output_dir", None):
            with open(os.path.join(args.output_dir, REPORT), "w") as f:
                json.dump({"base": args.mx, "bits": bits, "images": images, "average_bits": average, "nodes": report, "left": left}, f, indent=1)
    return fmt
