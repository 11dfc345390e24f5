"""`--mx_verify` — the packed MX files checked by the hardware that reads them (not in the reference; with `--mx_pack` only).

ocp_mx_weights.bin holds "the bytes a block-scaled GEMM reads"; this runs that GEMM.  After deploy has written the files, rank 0
takes the first --calib_batch images through the fake-quantised graph and, for every MatMul / Gemm whose two operands carry MX
nodes, multiplies the operands as BYTES on CDNA4's block-scaled matrix instruction (ops.mx_gemm):
  the activation operand   the tensor its MX node reads (under --mx_rotate the BlockHadamard output), encoded on the device along
                           its block axis (ops.mx_encode) — the same values the graph's MX node produces, as codes and scales;
  the constant operand     its codes and scales READ BACK from ocp_mx_weights.bin by the offsets of ocp_mx_weights.json — the file
                           has to be sufficient on its own; an operand that is itself an activation (Q . K^T, attention . V) is
                           encoded on the fly;
then alpha / beta / bias as the node defines them, in torch, and compares with the node's own output in the same forward: an fp32
product of dequantised values.  The bound is that of ops.mx_gemm against its definition, BOUND_FACTOR[format] * Kp * 2^-23 * S
(S = |A^| . |B^|, computed in the run from the decoded bytes), taken twice because the node's side carries an fp32 summation too —
plus, for a Gemm with a bias, the same factor on |beta . C|.  The factor is 1 for mxfp4 and mxfp6_e2m3, where the instruction adds exact products
(measured: no error), and twice the worst measured ratio, 10.38, for mxfp6_e3m2.  For mxfp8 it is twice the worst ratio measured on random data (tests/test_mx_gemm_gpu.py test 4): the
instruction truncates the E4M3 products of every run of 8 consecutive k to 2^-14 of the run's largest before it adds them, which
loses up to 7 * 2^-14 * S whatever Kp is.  The element format is the node's own, read from its two MX nodes (they
agree; under --mx_mixed ocp_mx_weights.json says "mixed", every tensor's entry names its format, and so does every node's entry of
the report), and the factor that format's.  -> mx_verify_report.json; no other file changes.

`--mx_conv`: a Conv whose two inputs are MX outputs goes through ops.mx_conv the same way — the activation encoded along axis 1 on
the device (NHWC codes), the weight's [cout, kh, kw, Cp ...] sections of ocp_mx_weights.bin as they stand, the explicit pads from
executor.conv_padding, the bias added in torch — and is compared with the node's output permuted to NHWC under the same bound with
Kp = kh * kw * 32 * ceil(C / 32); S = |A^| * |B^| in fp64 as unfold + matmul of the decoded bytes.
"""
import json
import os

import numpy as np
import torch

from .utils import logger

REPORT = "mx_verify_report.json"
BOUND_FACTOR = {"mxfp4": 1.0, "mxfp8": 2 * 19.51,      # on Kp * 2^-23 * S; mxfp8: twice the worst measured ratio, 19.51
                # the two MXFP6 formats on the same data and shapes (tests/test_mx_fp6_gemm_gpu.py test 5): E2M3 x E2M3
                # measured 0 and 0 — its products, about 12 bits wide, are added exactly — so factor 1 as for mxfp4; E3M2 x E3M2
                # measured 5.007 on [34, 96] x [96, 24] and 10.38 on [2, 17, 64] x [64, 48]: twice the worst
                "mxfp6_e2m3": 1.0, "mxfp6_e3m2": 2 * 10.38}


def _packed_from_file(entry, blob, dev):
    out = []
    for part in ("codes", "scales"):
        sec = entry[part]
        raw = blob[sec["offset"]:sec["offset"] + sec["nbytes"]]
        if raw.size != sec["nbytes"]:
            raise ValueError(f"ocp_mx_weights.bin ends inside a section ({part} at {sec['offset']}, {sec['nbytes']} bytes)")
        out.append(torch.from_numpy(np.ascontiguousarray(raw).reshape(sec["shape"])).to(dev))
    return out


def mx_verify(graph, act_clip_val, weight_clip_val, args):
    """-> the report (also written to mx_verify_report.json in args.output_dir)."""
    from . import ops
    from .forward_net import ActivationCache
    from .quantize import MX_BLOCK, quant_graph
    clip = {k: [np.copy(v[0]), np.copy(v[1])] for k, v in {**act_clip_val, **weight_clip_val}.items()}
    graph_q, _ = quant_graph(graph, clip, args)
    with open(os.path.join(args.output_dir, "ocp_mx_weights.json")) as f:
        meta = json.load(f)
    blob = np.fromfile(os.path.join(args.output_dir, "ocp_mx_weights.bin"), dtype=np.uint8)
    mixed = meta["format"] == "mixed"       # (--mx_mixed) every tensor's entry then names its own format
    images = max(1, min(int(args.data_num), int(getattr(args, "calib_batch", None) or 16)))
    cache = ActivationCache(graph_q, args, 0, images)
    sess = cache._session()
    dev = sess.device
    by_out = {q.output: q for q in graph_q._qdq.values() if q.is_mx}
    nodes, skipped = {}, {}

    def activation(name):
        return torch.cat(list(cache.chunks(name))).contiguous()

    def operand(q, last_two, elem):
        """(codes, scales, key or None) of the operand behind MX node q, K-innermost: [*lead, rows, Kp ...]."""
        if q.tensor_name in graph_q.initializer:
            key = q.tensor_name + q.suffix
            if key not in meta["tensors"]:
                raise KeyError(f"{key} is not in ocp_mx_weights.json")
            if meta["tensors"][key].get("format", meta["format"]) != elem:
                raise ValueError(f"{key} is {meta['tensors'][key].get('format', meta['format'])} in ocp_mx_weights.json and {elem} in the graph")
            return (*_packed_from_file(meta["tensors"][key], blob, dev), key, int(meta["tensors"][key]["k"]))
        x = activation(q.tensor_name)
        axis = int(q.block_axis)
        if x.dim() < 2 or axis % x.dim() != x.dim() + last_two:
            raise ValueError(f"blocks along axis {axis} of a tensor of {x.dim()} dimension(s)")
        return (*ops.mx_encode(x, last_two, elem), None, int(x.shape[last_two]))

    def conv(node, qa, qb, elem):
        """A Conv (`--mx_conv`) whose two inputs are MX outputs, blocked along axis 1 -> its report entry."""
        from .executor import conv_padding
        if qa.tensor_name in graph_q.initializer or qb.tensor_name not in graph_q.initializer:
            raise ValueError("not an activation convolved with a constant weight")
        if int(node.attrs.get("group", 1) or 1) != 1:
            raise ValueError("a grouped convolution")
        x = activation(qa.tensor_name)
        if x.dim() != 4 or int(qa.block_axis) % 4 != 1 or int(qb.block_axis) % 4 != 1:
            raise ValueError(f"blocks along axes {int(qa.block_axis)} and {int(qb.block_axis)} of a {x.dim()}-D convolution's operands")
        a_codes, a_scales = ops.mx_encode(x, 1, elem)                                        # [n, h, w, Cp ...]: NHWC
        b_codes, b_scales, key, c_b = operand(qb, None, elem)                                    # [cout, kh, kw, Cp ...] as the file holds it
        n, c, h, w = (int(d) for d in x.shape)
        if b_codes.dim() != 4 or c_b != c:
            raise ValueError(f"the weight's packed codes are {list(b_codes.shape)} over {c_b} channels, the input has {c}")
        cout, kh, kw = (int(d) for d in b_codes.shape[:3])
        strides = tuple(int(v) for v in node.attrs.get("strides", [1, 1]))
        dil = tuple(int(v) for v in node.attrs.get("dilations", [1, 1]))
        _, fpad = conv_padding(node, x, (kh, kw), strides, dil)                              # F.pad's order: left, right, top, bottom
        want = activation(node.output[0]).double()
        if want.dim() != 4 or int(want.shape[0]) != n or int(want.shape[1]) != cout:
            raise ValueError(f"the node's output is {list(want.shape)}")
        oh, ow = int(want.shape[2]), int(want.shape[3])
        got = ops.mx_conv(a_codes, a_scales, b_codes, b_scales, elem, strides=strides, pads=(int(fpad[2]), int(fpad[0])), dilations=dil,
                          out_hw=(oh, ow)).double()
        cb = int(a_scales.shape[-1])
        kp = kh * kw * MX_BLOCK * cb
        # S from the bytes themselves: |A^| * |B^| in fp64 — the patches of |A^| (unfold) times |B^| as a matrix
        a_hat = ops.mx_decode(a_codes, a_scales, elem, (n, MX_BLOCK * cb, h, w), 1).double().abs()
        b_hat = ops.mx_decode(b_codes, b_scales, elem, (cout, MX_BLOCK * cb, kh, kw), 1).double().abs()
        cols = torch.nn.functional.unfold(torch.nn.functional.pad(a_hat, [int(v) for v in fpad]), (kh, kw), dilation=dil, stride=strides)
        if int(cols.shape[-1]) != oh * ow:
            raise ValueError(f"{int(cols.shape[-1])} patches for an output of {oh} x {ow}")
        s = torch.matmul(b_hat.reshape(cout, -1), cols).reshape(n, cout, oh, ow).permute(0, 2, 3, 1)
        if len(node.input) > 2 and node.input[2] != "":
            bias = sess.consts[node.input[2]] if node.input[2] in sess.consts else activation(node.input[2])
            bias = torch.as_tensor(bias, device=dev).double().reshape(-1)
            got, s = got + bias, s + bias.abs()
        want = want.permute(0, 2, 3, 1)
        bound = 2.0 * BOUND_FACTOR[elem] * kp * 2.0 ** -23 * s + 2.0 ** -149
        err = (got - want).abs()
        ratio = float((err / bound).max())
        cos = float((got * want).sum() / (got.norm() * want.norm()).clamp_min(1e-300))
        logger.info("--mx_verify: Conv {} [{} x {} x {} x {}] * [{} x {} x {}] ({} from the file): max |err| {:.3e}, {:.3e} of the bound, cosine "
                    "{:.9f}".format(node.name, n, c, h, w, cout, kh, kw, key, float(err.max()), ratio, cos))
        return {"op": "Conv", "n": n, "c": c, "h": h, "w": w, "cout": cout, "kernel": [kh, kw], "strides": list(strides),
                "pads": [int(fpad[2]), int(fpad[0]), int(fpad[3]), int(fpad[1])], "dilations": list(dil), "k": kh * kw * c, "constant": key,
                "max_abs_err": float(err.max()), "max_err_over_bound": ratio, "cosine": cos,
                "within_bound": bool(ratio <= 1.0 and bool(torch.isfinite(got).all()))}

    for node in graph_q.graph.node:
        if node.op_type not in ("MatMul", "Gemm", "Conv") or len(node.input) < 2:
            continue
        qa, qb = by_out.get(node.input[0]), by_out.get(node.input[1])
        if qa is None and qb is None:
            continue
        try:
            if qa is None or qb is None:
                raise ValueError("only one operand is block-scaled")
            if qa.format.elem != qb.format.elem:
                raise ValueError(f"its operands are {qa.format.elem} and {qb.format.elem}")
            elem = qa.format.elem               # the node's own format, from its MX nodes
            if node.op_type == "Conv":
                nodes[node.name] = conv(node, qa, qb, elem)
                if mixed:
                    nodes[node.name]["format"] = elem
                continue
            trans_b = 0
            if node.op_type == "Gemm":
                if int(node.attrs.get("transA", 0) or 0):
                    raise ValueError("transA = 1")
                trans_b = int(node.attrs.get("transB", 0) or 0)
            if qa.tensor_name in graph_q.initializer:
                raise ValueError("the first operand is a constant")
            a_codes, a_scales, _, k = operand(qa, -1, elem)
            b_codes, b_scales, key, k_b = operand(qb, -1 if trans_b else -2, elem)
            if k_b != k:
                raise ValueError(f"the operands reduce over {k} and {k_b} elements")
            lead, lead_b = tuple(a_codes.shape[:-2]), tuple(b_codes.shape[:-2])
            if lead_b not in ((), lead):
                if int(np.prod(lead_b, dtype=np.int64)) != 1:
                    raise ValueError(f"leading dimensions {list(lead)} and {list(lead_b)} need a broadcast")
                b_codes, b_scales = b_codes.reshape(b_codes.shape[-2:]), b_scales.reshape(b_scales.shape[-2:])
            got = ops.mx_gemm(a_codes, a_scales, b_codes, b_scales, elem)
            m, n, kp = int(a_codes.shape[-2]), int(b_codes.shape[-2]), MX_BLOCK * int(a_scales.shape[-1])
            # S from the bytes themselves: |A^| . |B^|^T in fp64
            a_hat = ops.mx_decode(a_codes, a_scales, elem, tuple(a_scales.shape[:-1]) + (kp,), -1).double().abs()
            b_hat = ops.mx_decode(b_codes, b_scales, elem, tuple(b_scales.shape[:-1]) + (kp,), -1).double().abs()
            s = torch.matmul(a_hat, b_hat.transpose(-1, -2))
            got = got.double()
            if node.op_type == "Gemm":
                alpha, beta = float(node.attrs.get("alpha", 1.0)), float(node.attrs.get("beta", 1.0))
                got, s = got * alpha, s * abs(alpha)
                if len(node.input) > 2 and node.input[2] != "":
                    c = sess.consts[node.input[2]] if node.input[2] in sess.consts else activation(node.input[2])
                    c = torch.as_tensor(c, device=dev).double() * beta
                    got, s = got + c, s + c.abs()
            want = activation(node.output[0]).double()
            if want.numel() != got.numel():
                raise ValueError(f"the node's output has {want.numel()} elements, the product {got.numel()}")
            want = want.reshape(got.shape)
            bound = 2.0 * BOUND_FACTOR[elem] * kp * 2.0 ** -23 * s + 2.0 ** -149
            err = (got - want).abs()
            ratio = float((err / bound).max())
            cos = float((got * want).sum() / (got.norm() * want.norm()).clamp_min(1e-300))
            nodes[node.name] = {"op": node.op_type, "m": m, "n": n, "k": k, "constant": key,
                                "max_abs_err": float(err.max()), "max_err_over_bound": ratio, "cosine": cos,
                                "within_bound": bool(ratio <= 1.0 and bool(torch.isfinite(got).all()))}
            if mixed:
                nodes[node.name]["format"] = elem
            logger.info("--mx_verify: {} {} [{} x {} x {}]{}: max |err| {:.3e}, {:.3e} of the bound, cosine {:.9f}".format(
                node.op_type, node.name, m, n, kp, "" if key is None else " (" + key + " from the file)", float(err.max()), ratio, cos))
        except (ValueError, KeyError) as e:
            skipped[node.name] = str(e)
            logger.warning("--mx_verify: {} {} skipped: {}".format(node.op_type, node.name, e))
    report = {"format": meta["format"], "images": images, "nodes": nodes, "skipped": skipped}
    with open(os.path.join(args.output_dir, REPORT), "w") as f:
        json.dump(report, f, indent=4)
    bad = [k for k, v in nodes.items() if not v["within_bound"]]
    if bad:
        logger.warning("--mx_verify: {} node(s) outside the bound: {}".format(len(bad), ", ".join(bad)))
    else:
        logger.info("--mx_verify: {} node(s) within the bound, {} skipped".format(len(nodes), len(skipped)))
    return report
