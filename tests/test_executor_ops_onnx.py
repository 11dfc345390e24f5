"""The executor's op table — one small function per operator that translates ONNX attributes into a torch call — against the ONNX
definitions (tests/onnx_ref.py: numpy fp64, held to hand-worked values by test_onnx_ref.py), node by node: hand-built
onnx_io.Nodes with the attribute combinations exporters other than torch's write (auto_pad, asymmetric pads, output_shape,
coordinate_transformation_mode, axes inputs, opset-dependent defaults), called as executor._OPS[op](session, node, *tensors).

Every case runs on the CPU, and again on the device in the test marked gpu.  Tolerances are derived, not tuned:

  exact  operators that move or select values: bit for bit against the model's result cast to fp32.
  sum    a K-term sum in any order of fp32 accumulation is within (K + 2) 2^-24 sum |terms| of the exact value; the model supplies
         sum |terms| per output (AveragePool, ReduceSum / ReduceMean, GlobalAveragePool, linear Resize with K = 2^axes).
  conv   Conv / ConvTranspose, K = Cin / g * prod(k): the same bound on the CPU.  On the device MIOpen may choose Winograd or split-K
         solvers the bound does not describe: there the bound is DEVICE_CONV_RATIO * 2^-24 * sum |x w|, four times the largest ratio
         |got - ref| / (2^-24 sum |x w|) measured over the convolution cases on an MI355X (the margin is for solver choice, which
         varies with the library build).  The measured ratios are in CONV_MEASURED (op_bounds.py), per case, largest first: 2.779
         (conv_2d_k1) at most, so the device bound is 11.1 * 2^-24 * sum |x w|.
         For every convolution case the bound — on either device — stays below 1 % of the smallest |x w| product that reaches the
         output (asserted from the model's numbers): a dropped kernel position or pad row cannot hide inside it.  Inputs are
         |N(0, 1)| + 0.5 with random signs for that reason.
  trans  normalisations, Softmax, Sigmoid, Tanh, Gelu, Erf, Exp, Log, Pow and the other elementwise arithmetic go through library
         functions: against the fp64 model, in units of 2^-24 max(|ref|, 1).  Largest error measured per operator: TRANS_MEASURED
         in op_bounds.py (CPU, MI355X) — 4.462 on the CPU and 6.74 on the device, both LayerNormalization; the bound is four times the larger
         of the two maxima: 26.96 units.

The tables, the bounds and the comparison itself live in op_bounds.py (tests/qdq_replay.py holds the nodes of a saved Q/DQ model to
the same bounds).

A case the executor refuses is asserted as a refusal that names the attribute (cubic and tf_crop_and_resize Resize)."""
import functools
import types

import numpy as np
import pytest
import torch

from dipoorlet_amd import executor as ex
from dipoorlet_amd import shape_infer
from dipoorlet_amd.executor import _OPS, GraphSession
from dipoorlet_amd.graph import ONNXGraph
from dipoorlet_amd.onnx_io import Node
from onnx_ref import INT64_MAX, INT64_MIN, REF

from op_bounds import (CONV_MEASURED, DEVICE_CONV_RATIO, TRANS_MEASURED, TRANS_RATIO, U, Case, _bound, _check,  # noqa: F401
                       _one_tap_condition)


def _away(rng, *shape):
    """|N(0, 1)| + 0.5 with random signs: no value near zero, so that every product of a convolution is worth noticing."""
    return ((np.abs(rng.standard_normal(shape)) + 0.5) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def _c(a):
    return np.array(a, order="C")       # (np.ascontiguousarray would turn a 0-d scalar into shape (1,))


def _i64(*v):
    return np.array(v, np.int64)


def _f32(*v):
    return np.array(v, np.float32)


def _cases():
    rng = np.random.default_rng(20261)
    cs = []

    def add(id, op, inputs, attrs=None, **kw):
        cs.append(Case(id, op, inputs, attrs, **kw))

    # ------------------------------------------------------------------------------------------------ Conv
    def conv(id, xs, ws, attrs, bias=True):
        g = attrs.get("group", 1)
        inputs = [_away(rng, *xs), _away(rng, *ws)] + ([_away(rng, ws[0])] if bias else [])
        add("conv_" + id, "Conv", inputs, attrs, kind="conv", K=ws[1] * int(np.prod(ws[2:])))
        assert xs[1] == ws[1] * g

    conv("1d_s2_d2_asym", (2, 4, 9), (5, 4, 3), {"strides": [2], "dilations": [2], "pads": [2, 1]})
    conv("2d_s2_d2_asym", (2, 3, 9, 8), (4, 3, 3, 3), {"strides": [2, 2], "dilations": [2, 2], "pads": [1, 2, 2, 0]})
    conv("2d_asym_nobias", (2, 3, 7, 10), (5, 3, 3, 2), {"pads": [0, 1, 2, 0]}, bias=False)
    conv("2d_sym", (2, 4, 8, 7), (4, 4, 3, 3), {"pads": [1, 1, 1, 1], "kernel_shape": [3, 3]})
    conv("2d_group2", (2, 6, 7, 10), (4, 3, 3, 2), {"group": 2, "pads": [1, 0, 1, 1]}, bias=False)
    conv("2d_group3_k5x1", (2, 6, 11, 9), (6, 2, 5, 1), {"group": 3, "pads": [2, 0, 1, 0], "strides": [2, 1]})
    conv("2d_depthwise", (2, 6, 8, 7), (6, 1, 3, 3), {"group": 6, "pads": [1, 0, 0, 1]})
    conv("2d_k1", (2, 8, 5, 4), (3, 8, 1, 1), {}, bias=False)
    for ap in ("SAME_UPPER", "SAME_LOWER", "VALID"):   # in 8, k 3, s 2: total 1; in 7, k 4, s 2: total 3 — both odd
        conv("2d_" + ap.lower(), (2, 3, 8, 7), (4, 3, 3, 4), {"auto_pad": ap, "strides": [2, 2]}, bias=ap != "SAME_LOWER")
    conv("2d_same_upper_dilated", (2, 3, 8, 7), (4, 3, 3, 2), {"auto_pad": "SAME_UPPER", "dilations": [2, 3]})
    conv("3d_asym", (2, 3, 5, 6, 4), (4, 3, 2, 3, 2), {"pads": [1, 0, 1, 0, 1, 1], "strides": [1, 2, 1]})
    conv("3d_group_same_lower", (2, 4, 4, 5, 6), (4, 2, 3, 2, 3), {"group": 2, "auto_pad": "SAME_LOWER", "strides": [2, 2, 2]}, bias=False)

    # ------------------------------------------------------------------------------------------------ ConvTranspose
    def convt(id, xs, ws, attrs, bias=True):
        g = attrs.get("group", 1)
        inputs = [_away(rng, *xs), _away(rng, *ws)] + ([_away(rng, ws[1] * g)] if bias else [])
        add("convt_" + id, "ConvTranspose", inputs, attrs, kind="conv", K=(ws[0] // g) * int(np.prod(ws[2:])))
        assert xs[1] == ws[0]

    convt("1d_asym", (2, 4, 6), (4, 3, 3), {"strides": [2], "pads": [1, 0]})
    convt("2d_s2_opad", (2, 4, 5, 6), (4, 3, 3, 3), {"strides": [2, 2], "pads": [1, 1, 1, 1], "output_padding": [1, 0]})
    convt("2d_dilated", (2, 3, 5, 7), (3, 4, 3, 2), {"dilations": [2, 3], "pads": [1, 0, 1, 0]}, bias=False)
    convt("2d_group3", (2, 6, 5, 4), (6, 2, 3, 3), {"group": 3, "strides": [2, 1], "pads": [0, 1, 0, 1]})
    convt("2d_asym", (2, 3, 6, 5), (3, 4, 3, 4), {"strides": [2, 2], "pads": [1, 0, 2, 1]})
    convt("2d_asym_opad", (2, 3, 4, 5), (3, 2, 3, 3), {"strides": [3, 2], "pads": [0, 2, 1, 0], "output_padding": [2, 1]}, bias=False)
    convt("2d_output_shape", (2, 3, 5, 5), (3, 4, 3, 3), {"strides": [2, 2], "output_shape": [10, 10]})
    convt("2d_output_shape_opad", (2, 3, 5, 4), (3, 2, 3, 2), {"strides": [2, 2], "output_shape": [10, 7], "output_padding": [1, 0]})
    convt("2d_same_upper", (2, 3, 5, 4), (3, 4, 3, 3), {"strides": [2, 2], "auto_pad": "SAME_UPPER"})
    convt("2d_same_lower", (2, 3, 5, 4), (3, 4, 3, 3), {"strides": [2, 2], "auto_pad": "SAME_LOWER"}, bias=False)
    convt("2d_valid", (2, 3, 5, 4), (3, 4, 2, 3), {"strides": [2, 1], "auto_pad": "VALID"})
    convt("3d_asym", (2, 2, 3, 4, 3), (2, 3, 2, 3, 2), {"strides": [2, 1, 2], "pads": [1, 0, 0, 0, 1, 1]})

    # ------------------------------------------------------------------------------------------------ pools
    x4 = _away(rng, 2, 3, 9, 8)
    neg = -np.abs(_away(rng, 2, 3, 7, 6))
    for op, kind in (("MaxPool", "exact"), ("AveragePool", "sum")):
        p = "maxpool_" if op == "MaxPool" else "avgpool_"
        cips = (None,) if op == "MaxPool" else (0, 1)
        for cip in cips:
            tag = "" if cip is None else f"_cip{cip}"
            extra = {} if cip is None else {"count_include_pad": cip}

            def pool(id, x, attrs):
                add(p + id + tag, op, [x], dict(attrs, **extra), kind=kind, K=int(np.prod(attrs["kernel_shape"])))

            pool("sym", x4, {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]})
            pool("asym", x4, {"kernel_shape": [3, 2], "strides": [2, 1], "pads": [1, 0, 0, 1]})
            pool("nopad_default_stride", x4, {"kernel_shape": [2, 3]})
            # ceil mode: H in 5, k 2, s 2, no pads: the third window starts at 4 < 5: kept.  W in 3, pads 1 1: the third would start
            # at 4 >= 3 + 1: dropped
            pool("ceil_kept_dropped", _away(rng, 2, 3, 5, 3), {"kernel_shape": [2, 2], "strides": [2, 2], "pads": [0, 1, 0, 1], "ceil_mode": 1})
            # asymmetric pads in ceil mode: H in 5, pads 0 2: the fourth window would start at 6 >= 5, INSIDE the end padding:
            # dropped; W in 6, pads 1 0: the fourth starts at 6 < 7: kept
            pool("asym_ceil", _away(rng, 2, 3, 5, 6), {"kernel_shape": [2, 2], "strides": [2, 2], "pads": [0, 1, 2, 0], "ceil_mode": 1})
            pool("same_upper_even", _away(rng, 2, 3, 8, 6), {"kernel_shape": [3, 3], "strides": [2, 2], "auto_pad": "SAME_UPPER"})
            pool("same_lower_even", _away(rng, 2, 3, 8, 6), {"kernel_shape": [2, 3], "strides": [1, 2], "auto_pad": "SAME_LOWER"})
            pool("1d_asym", _away(rng, 2, 4, 10), {"kernel_shape": [4], "strides": [3], "pads": [2, 1]})
            pool("3d_asym", _away(rng, 2, 3, 4, 5, 6), {"kernel_shape": [2, 2, 3], "strides": [1, 2, 2], "pads": [1, 0, 0, 0, 1, 1]})
            pool("all_negative_sym", neg, {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]})
            pool("all_negative_asym", neg, {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 0, 0, 1]})
    add("maxpool_dilated", "MaxPool", [x4], {"kernel_shape": [3, 2], "dilations": [2, 3], "pads": [1, 1, 1, 1], "strides": [1, 2]})
    add("maxpool_dilated_asym_ceil", "MaxPool", [x4], {"kernel_shape": [2, 2], "dilations": [2, 2], "pads": [1, 0, 0, 2], "strides": [2, 2],
                                                       "ceil_mode": 1})
    xn = x4.copy()
    xn[0, 1, 4, 3] = np.nan
    xn[1, 2, 0, 0] = np.nan
    add("maxpool_nan", "MaxPool", [xn], {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]})
    add("global_average_pool", "GlobalAveragePool", [x4], kind="sum", K=72)
    add("global_max_pool", "GlobalMaxPool", [x4])
    add("global_max_pool_negative_3d", "GlobalMaxPool", [-np.abs(_away(rng, 2, 3, 4, 5, 3))])

    # ------------------------------------------------------------------------------------------------ Resize / Upsample
    xr = _away(rng, 2, 3, 5, 7)
    none = None
    targets = (("scale2", _f32(1, 1, 2, 2), none), ("scale1p6", _f32(1, 1, 1.6, 1.6), none),
               ("sizes_up", none, _i64(2, 3, 9, 10)), ("sizes_down", none, _i64(2, 3, 3, 4)))
    for coord in ("half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric"):
        for tname, scales, sizes in targets:
            inputs = [xr, none, scales] if sizes is None else [xr, none, none, sizes]
            for nearest in ("round_prefer_floor", "round_prefer_ceil", "floor", "ceil"):
                add(f"resize_nearest_{coord}_{nearest}_{tname}", "Resize", inputs,
                    {"mode": "nearest", "coordinate_transformation_mode": coord, "nearest_mode": nearest})
            add(f"resize_linear_{coord}_{tname}", "Resize", inputs, {"mode": "linear", "coordinate_transformation_mode": coord},
                kind="sum", K=4)
    add("resize_default_attrs_scale1p6", "Resize", [xr, none, _f32(1, 1, 1.6, 1.6)])
    add("resize_default_attrs_sizes", "Resize", [xr, _f32(), _f32(), _i64(2, 3, 8, 11)], opset=11)
    add("resize_default_attrs_5_to_8", "Resize", [_away(rng, 2, 3, 5), none, none, _i64(2, 3, 8)])
    add("resize_linear_default_coord_5_to_10", "Resize", [_away(rng, 2, 3, 5), none, _f32(1, 1, 2)], {"mode": "linear"}, kind="sum", K=2)
    add("resize_linear_align_corners_5_to_10", "Resize", [_away(rng, 2, 3, 5), none, _f32(1, 1, 2)],
        {"mode": "linear", "coordinate_transformation_mode": "align_corners"}, kind="sum", K=2)
    add("resize_linear_3d_half_pixel", "Resize", [_away(rng, 2, 3, 4, 5, 3), none, none, _i64(2, 3, 6, 4, 7)], {"mode": "linear"},
        kind="sum", K=8)
    add("resize_linear_to_one_pytorch_half_pixel", "Resize", [xr, none, none, _i64(2, 3, 1, 1)],
        {"mode": "linear", "coordinate_transformation_mode": "pytorch_half_pixel"}, kind="sum", K=4)
    add("resize_linear_one_axis_only", "Resize", [xr, none, _f32(1, 1, 1, 1.6)], {"mode": "linear"}, kind="sum", K=2)
    for op, opset in (("Upsample", 9), ("Resize", 10)):
        for tname, scales in (("scale2", _f32(1, 1, 2, 2)), ("scale1p6", _f32(1, 1, 1.6, 2.5))):
            add(f"{op.lower()}{opset}_nearest_{tname}", op, [xr, scales], {"mode": "nearest"}, opset=opset)
            add(f"{op.lower()}{opset}_linear_{tname}", op, [xr, scales], {"mode": "linear"}, opset=opset, kind="sum", K=4)
    add("resize_cubic_refused", "Resize", [xr, none, _f32(1, 1, 2, 2)], {"mode": "cubic"}, refuse="mode=cubic")
    add("resize_tf_crop_and_resize_refused", "Resize", [xr, _f32(0, 0, 0, 0, 1, 1, 1, 1), none, _i64(2, 3, 4, 4)],
        {"mode": "linear", "coordinate_transformation_mode": "tf_crop_and_resize"}, refuse="coordinate_transformation_mode=tf_crop_and_resize")

    # ------------------------------------------------------------------------------------------------ Pad
    xp = _away(rng, 2, 3, 5, 4)
    for mode in ("constant", "reflect", "edge"):
        add(f"pad_{mode}_trailing", "Pad", [xp, _i64(0, 0, 2, 1, 0, 0, 1, 3)], {"mode": mode})
        add(f"pad_{mode}_negative", "Pad", [xp, _i64(0, 0, -1, 2, 0, 0, 1, -2)], {"mode": mode})
        add(f"pad_{mode}_channel_axis", "Pad", [xp, _i64(0, 1, 0, 2, 0, 2, 1, 0)], {"mode": mode})
        add(f"pad_{mode}_axes_last", "Pad", [xp, _i64(1, 2), none, _i64(-1)], {"mode": mode}, opset=18)
        add(f"pad_{mode}_axes_two", "Pad", [xp, _i64(2, 1, 0, 3), none, _i64(3, -3)], {"mode": mode}, opset=18)
        add(f"pad_{mode}_3d_tensor", "Pad", [_away(rng, 2, 4, 6), _i64(0, 1, 2, 0, 0, 3)], {"mode": mode})
    add("pad_default_mode", "Pad", [xp, _i64(0, 0, 1, 1, 0, 0, 1, 1)])
    add("pad_value_input", "Pad", [xp, _i64(0, 0, 1, 2, 0, 0, 0, 1), _f32(-3.5).reshape(())])
    add("pad_value_input_axes", "Pad", [xp, _i64(1, 2), _f32(1.25).reshape(()), _i64(2)], opset=18)
    add("pad_attrs_opset2", "Pad", [xp], {"pads": [0, 0, 1, 0, 0, 0, 2, 1], "value": 2.5}, opset=2)
    add("pad_batch_axis_axes", "Pad", [xp, _i64(1, 0), none, _i64(0)], opset=18, session=False)

    # ------------------------------------------------------------------------------------------------ elementwise
    xe = _away(rng, 2, 3, 5, 4)
    xnan = xe.copy()
    xnan[0, 0, 0, 0] = np.nan
    xnan[1, 2, 3, 1] = np.nan
    add("relu", "Relu", [xe])
    add("relu_nan", "Relu", [xnan])
    add("clip_inputs", "Clip", [xe, _f32(-0.75).reshape(()), _f32(1.5).reshape(())])
    add("clip_min_only", "Clip", [xe, _f32(0.25).reshape(())])
    add("clip_max_only", "Clip", [xe, none, _f32(0.75).reshape(())])
    add("clip_no_bounds", "Clip", [xe])
    add("clip_attrs_opset6", "Clip", [xe], {"min": -1.0, "max": 0.5}, opset=6)
    add("clip_attr_max_only_opset6", "Clip", [xe], {"max": 0.5}, opset=6)
    add("clip_nan", "Clip", [xnan, _f32(-1).reshape(()), _f32(1).reshape(())])
    for name in ("Abs", "Neg", "Floor", "Ceil", "Identity", "Dropout"):
        add(name.lower(), name, [xe * np.float32(1.7)])
    for name in ("Sigmoid", "Tanh", "HardSwish", "Erf", "Exp", "Reciprocal"):
        add(name.lower(), name, [xe * np.float32(1.7)], kind="trans")
    add("leakyrelu_default", "LeakyRelu", [xe], kind="trans")
    add("leakyrelu_alpha", "LeakyRelu", [xe], {"alpha": 0.3}, kind="trans")
    add("hardsigmoid_default", "HardSigmoid", [xe * np.float32(2)], kind="trans")
    add("hardsigmoid_alpha_beta", "HardSigmoid", [xe], {"alpha": 0.4, "beta": 0.3}, kind="trans")
    add("gelu", "Gelu", [xe], kind="trans", opset=20)
    add("gelu_tanh", "Gelu", [xe], {"approximate": "tanh"}, kind="trans", opset=20)
    add("sqrt", "Sqrt", [np.abs(xe)], kind="trans")
    add("log", "Log", [np.abs(xe)], kind="trans")
    add("prelu_channel_slope", "PRelu", [xe, _away(rng, 3, 1, 1)], kind="trans")
    add("prelu_scalar_slope", "PRelu", [xe, _f32(0.2)], kind="trans")
    ye = _away(rng, 2, 3, 5, 4)
    for name in ("Add", "Sub", "Mul", "Div"):
        add(name.lower(), name, [xe, ye], kind="trans", feeds=(0, 1))
        add(name.lower() + "_broadcast_const", name, [xe, _away(rng, 3, 1, 1)], kind="trans")
    add("eltwise", "Eltwise", [xe, ye], kind="trans", feeds=(0, 1))
    add("pow", "Pow", [np.abs(xe), ye], kind="trans", feeds=(0, 1))
    add("pow_scalar", "Pow", [xe, _f32(2.0).reshape(())], kind="trans")
    add("where", "Where", [rng.random((3, 1, 4)) < 0.5, xe, ye], feeds=(1, 2))
    add("equal", "Equal", [np.round(xe), np.round(ye)], feeds=(0, 1), session=False)
    add("cast_int64", "Cast", [xe * np.float32(3)], {"to": 7}, session=False)
    add("cast_float16", "Cast", [xe], {"to": 10}, session=False)
    add("cast_bool_to_float", "Cast", [rng.random((2, 3)) < 0.5], {"to": 1}, session=False)

    # ------------------------------------------------------------------------------------------------ Softmax, normalisations
    xs = _away(rng, 2, 3, 4)
    add("softmax13_default", "Softmax", [xs], kind="trans")
    add("softmax13_axis1", "Softmax", [xs], {"axis": 1}, kind="trans")
    add("softmax13_axis_neg2", "Softmax", [xe], {"axis": -2}, kind="trans")
    add("softmax11_default", "Softmax", [xs], opset=11, kind="trans")
    add("softmax11_axis2", "Softmax", [xs], {"axis": 2}, opset=11, kind="trans")
    add("softmax11_axis_neg1_4d", "Softmax", [xe], {"axis": -1}, opset=11, kind="trans")
    add("softmax1_axis0", "Softmax", [xs], {"axis": 0}, opset=1, kind="trans", session=False)
    add("softmax11_2d", "Softmax", [_away(rng, 2, 7)], opset=11, kind="trans")
    var = (np.abs(_away(rng, 3)) + 0.1).astype(np.float32)
    add("batchnorm", "BatchNormalization", [xe, _away(rng, 3), _away(rng, 3), _away(rng, 3), var], {"epsilon": 1e-3}, kind="trans")
    add("batchnorm_default_eps_3d", "BatchNormalization", [xs, _away(rng, 3), _away(rng, 3), _away(rng, 3), var], kind="trans")
    add("layernorm_last", "LayerNormalization", [xe, _away(rng, 4), _away(rng, 4)], kind="trans", opset=17)
    add("layernorm_axis2_nobias", "LayerNormalization", [xe, _away(rng, 5, 4)], {"axis": 2, "epsilon": 1e-3}, kind="trans", opset=17)
    add("layernorm_axis_neg3", "LayerNormalization", [xe, _away(rng, 3, 5, 4), _away(rng, 3, 5, 4)], {"axis": -3}, kind="trans", opset=17)
    add("instancenorm", "InstanceNormalization", [xe, _away(rng, 3), _away(rng, 3)], {"epsilon": 1e-3}, kind="trans")
    add("instancenorm_1d", "InstanceNormalization", [_away(rng, 2, 4, 9), _away(rng, 4), _away(rng, 4)], kind="trans")

    # ------------------------------------------------------------------------------------------------ reductions
    for name, kind in (("ReduceSum", "sum"), ("ReduceMean", "sum"), ("ReduceMax", "exact"), ("ReduceMin", "exact")):
        p = name.lower()
        add(p + "_axes_input", name, [xe, _i64(1, 3)], kind=kind, K=12)
        add(p + "_axes_attr_nokeep", name, [xe], {"axes": [2], "keepdims": 0}, kind=kind, K=5, opset=11)
        add(p + "_negative_axes", name, [xe, _i64(-1, -3)], {"keepdims": 0}, kind=kind, K=12)
        add(p + "_no_axes", name, [xe], kind=kind, K=60, session=False)
        add(p + "_no_axes_nokeep", name, [xe], {"keepdims": 0}, kind=kind, K=60, session=False)
        add(p + "_empty_axes", name, [xe, _i64()], kind=kind, K=60, session=False)
        add(p + "_empty_axes_noop", name, [xe, _i64()], {"noop_with_empty_axes": 1}, kind=kind, K=1)
        add(p + "_absent_axes_noop", name, [xe], {"noop_with_empty_axes": 1, "keepdims": 0}, kind=kind, K=1)

    # ------------------------------------------------------------------------------------------------ shape and index operators
    xi = _away(rng, 2, 3, 4, 5)
    for ax in (0, 1, 2, -1, -4, 4):
        add(f"flatten_axis{ax}", "Flatten", [xi], {"axis": ax}, session=ax not in (0, -4))
    add("flatten_default", "Flatten", [xi])
    add("reshape_zero_and_minus1", "Reshape", [xi, _i64(0, -1, 5)])
    add("reshape_allowzero", "Reshape", [xi, _i64(2, 12, 5)], {"allowzero": 1}, opset=14, session=False)
    add("transpose_default", "Transpose", [xi], session=False)
    add("transpose_perm", "Transpose", [xi], {"perm": [0, 2, 3, 1]})
    add("transpose_perm_batch_moves", "Transpose", [xi], {"perm": [2, 0, 3, 1]})
    add("concat_axis1", "Concat", [xi, _away(rng, 2, 2, 4, 5), _away(rng, 2, 1, 4, 5)], {"axis": 1}, feeds=(0, 1, 2))
    add("concat_axis_neg1", "Concat", [xi, _away(rng, 2, 3, 4, 2)], {"axis": -1}, feeds=(0, 1))
    add("split_input", "Split", [xi, _i64(1, 3, 1)], {"axis": 3}, n_out=3)
    add("split_attr_opset11", "Split", [xi], {"axis": 1, "split": [2, 1]}, n_out=2, opset=11)
    add("split_equal_by_outputs", "Split", [xi], {"axis": 2}, n_out=2)
    add("split_num_outputs_uneven", "Split", [xi], {"axis": 3, "num_outputs": 3}, n_out=3, opset=18)
    add("split_num_outputs_negative_axis", "Split", [xi], {"axis": -1, "num_outputs": 2}, n_out=2, opset=18)
    add("slice_positive_steps", "Slice", [xi, _i64(1, 0), _i64(4, INT64_MAX), _i64(2, 3), _i64(1, 2)])
    add("slice_negative_bounds", "Slice", [xi, _i64(-3, -4), _i64(-1, 100), _i64(-1, -2)])
    add("slice_negative_step_int64_min", "Slice", [xi, _i64(-1, INT64_MAX), _i64(INT64_MIN, 0), _i64(3, 2), _i64(-1, -2)])
    add("slice_negative_step_empty", "Slice", [xi, _i64(1), _i64(3), _i64(2), _i64(-1)])
    add("slice_default_axes_steps", "Slice", [xi, _i64(0, 1), _i64(2, 3)])
    add("slice_attrs_opset1", "Slice", [xi], {"starts": [1, 1], "ends": [3, 1000], "axes": [2, 3]}, opset=1)
    add("gather_negative_indices", "Gather", [xi, _i64(-1, 0, -3, 2)], {"axis": 2})
    add("gather_2d_indices", "Gather", [xi, _i64(4, -5, 0, 2, -1, 1).reshape(2, 3)], {"axis": 3})
    add("gather_scalar_negative", "Gather", [xi, _i64(-2).reshape(())], {"axis": 1})
    add("gather_negative_axis", "Gather", [xi, _i64(1, -1)], {"axis": -1})
    add("gather_axis0", "Gather", [xi, _i64(-1, 0)], session=False)
    x1 = _away(rng, 2, 1, 4, 1)
    add("squeeze_axes_input", "Squeeze", [x1, _i64(1, -1)])
    add("squeeze_axes_attr", "Squeeze", [x1], {"axes": [3]}, opset=11)
    add("squeeze_no_axes", "Squeeze", [x1], session=False)
    add("unsqueeze_axes_input", "Unsqueeze", [xs, _i64(1, -1)])
    add("unsqueeze_axes_attr", "Unsqueeze", [xs], {"axes": [4, 2]}, opset=11)
    add("expand", "Expand", [x1, _i64(1, 3, 1, 5)])
    add("expand_to_higher_rank", "Expand", [_away(rng, 2, 1, 4), _i64(3, 1, 1, 1)], session=False)
    add("shape", "Shape", [xi], session=False)
    add("constantofshape_default", "ConstantOfShape", [_i64(2, 3, 4)], session=False, feeds=())
    add("constantofshape_value", "ConstantOfShape", [_i64(3, 2)], {"value": _f32(1.5)}, session=False, feeds=())
    add("constantofshape_int64", "ConstantOfShape", [_i64(4)], {"value": _i64(-7)}, session=False, feeds=())
    return cs


CASES = _cases()
RUN = [c for c in CASES if c.refuse is None]
assert len({c.id for c in CASES}) == len(CASES)


def test_every_op_of_the_table_has_a_case():
    covered = {c.op for c in CASES}
    assert set(_OPS) - covered == {"FakeQuant", "Gemm", "MatMul"}     # (held to their definitions in test_hip_parity.py)


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    """The model's answer for a case: computed once, shared by every test, never written to."""
    c = next(c for c in CASES if c.id == case_id)
    # (Split before opset 18 has no num_outputs: the node's number of outputs says it)
    y, aux = REF[c.op](c.inputs, dict(c.attrs, num_outputs=c.n_out) if c.op == "Split" else c.attrs, c.opset)
    ys = list(y) if isinstance(y, list) else [y]
    for a in ys + ([] if aux is None else list(aux.values())):
        a.setflags(write=False)
    return ys, aux


def _session(c, device):
    return types.SimpleNamespace(batch=2, device=torch.device(device), match_batch=lambda a, b: (a, b),
                                 graph=types.SimpleNamespace(opset={"": c.opset}))


def _node(c):
    names = ["" if a is None else f"i{j}" for j, a in enumerate(c.inputs)]
    while names and names[-1] == "":
        names.pop()
    return Node(c.op, names, [f"y{k}" for k in range(c.n_out)], name="n", attrs=c.attrs)


def _call(c, device):
    args = [None if a is None else torch.from_numpy(_c(a)).to(device) for a in c.inputs]
    while args and args[-1] is None:
        args.pop()
    with torch.no_grad():
        out = _OPS[c.op](_session(c, device), _node(c), *args)
    return [o.cpu().numpy() for o in (out if isinstance(out, (list, tuple)) else [out])]


@pytest.mark.parametrize("c", RUN, ids=lambda c: c.id)
def test_op_follows_the_onnx_definition_cpu(c):
    ref, aux = _reference(c.id)
    if c.kind == "conv":
        _one_tap_condition(c, aux, "cpu")
    _check(c, _call(c, "cpu"), ref, aux, "cpu")


@pytest.mark.parametrize("c", [c for c in CASES if c.refuse is not None], ids=lambda c: c.id)
def test_out_of_scope_attributes_are_refused_by_name(c):
    with pytest.raises(NotImplementedError, match=c.refuse):
        _call(c, "cpu")
    with pytest.raises(NotImplementedError, match=c.refuse):
        _shape_rule(c)


def test_a_bare_call_without_a_session_means_opset_13():
    """Existing callers pass s = None: the opset-13 meaning (Softmax along one axis, Resize with the opset-11+ defaults)."""
    x = torch.from_numpy(_away(np.random.default_rng(3), 2, 3, 5))
    y = _OPS["Softmax"](None, Node("Softmax", ["x"], ["y"]), x).numpy()
    np.testing.assert_allclose(y, REF["Softmax"]([x.numpy()], {}, 13)[0], rtol=0, atol=TRANS_RATIO * U)
    y = _OPS["Resize"](None, Node("Resize", ["x", "", "", "s"], ["y"]), x, None, None, torch.tensor([2, 3, 8])).numpy()
    assert np.array_equal(y, REF["Resize"]([x.numpy(), None, None, _i64(2, 3, 8)], {}, 13)[0].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------- shape rules
def _shape_rule(c):
    args = []
    for j, a in enumerate(c.inputs):
        if a is None:
            args.append(None)
        elif j in c.feeds:
            args.append(shape_infer.Spec(a.shape))
        else:
            args.append(ex._host_ints(torch.from_numpy(_c(a))))
    while args and args[-1] is None:
        args.pop()
    host = shape_infer._HostRun(types.SimpleNamespace(opset={"": c.opset}), 2)
    return shape_infer._RULES[c.op](ex, host, _node(c), *args)


@pytest.mark.parametrize("c", RUN, ids=lambda c: c.id)
def test_host_shape_rule_gives_the_defined_shape_or_declines(c):
    """shape_infer's rule for the node: the model's output shape, or Unsupported / NotImplementedError (the session then takes the
    shapes from a forward) — never another shape, never another exception."""
    ref, _ = _reference(c.id)
    try:
        out = _shape_rule(c)
    except (shape_infer.Unsupported, NotImplementedError):
        return
    out = out if isinstance(out, (list, tuple)) else [out]
    assert [tuple(o.shape) for o in out] == [tuple(r.shape) for r in ref], c.id


# ---------------------------------------------------------------------------------------------------------- batching
def _one_node_graph(c):
    g = ONNXGraph()
    node = _node(c)
    g.graph.node = [node]
    feeds = [f"i{j}" for j in c.feeds]
    g.initializer = {f"i{j}": _c(a) for j, a in enumerate(c.inputs) if a is not None and j not in c.feeds}
    g.network_inputs, g.network_outputs = feeds, list(node.output)
    g.input = [n for n in node.input if n]
    g.tensor_name_shape_map = {f"i{j}": [1] + list(c.inputs[j].shape[1:]) for j in c.feeds}
    g.opset = {"": c.opset}
    g.topologize_graph()
    g.set_index()
    return g


@pytest.mark.parametrize("c", [c for c in RUN if c.session], ids=lambda c: c.id)
def test_batch_of_two_through_a_session_is_two_single_images(c):
    """The case at batch 2 through a GraphSession of the one-node graph, and as two batch-1 runs: every image follows the definition,
    and the two runs agree — exactly for the selection operators, within the case's bound for the rest."""
    ref, aux = _reference(c.id)
    s = GraphSession(_one_node_graph(c), device="cpu")
    outs = [f"y{k}" for k in range(c.n_out)]
    feeds = {f"i{j}": torch.from_numpy(_c(c.inputs[j].astype(np.float32))) for j in c.feeds}
    both = s.run_named(feeds, outs)
    for k in range(2):
        one = s.run_named({n: v[k:k + 1] for n, v in feeds.items()}, outs)
        for o, (tb, t1, r) in enumerate(zip(both, one, ref)):
            axis = _batch_axis(c, o, r, t1)                 # the images are stacked in blocks along it
            rk = np.split(r, 2, axis)[k]
            a1 = {n: np.split(v, 2, axis)[k] for n, v in aux.items()} if aux is not None else None
            # (a session hands a batch on image-major: [B, per-image ...] in memory)
            g2, g1 = tb.reshape(2, -1)[k].numpy().reshape(rk.shape), t1.numpy().reshape(rk.shape)
            _check(c, [g2], [rk], a1, "cpu", f" image {k} of a batch")
            _check(c, [g1], [rk], a1, "cpu", f" image {k} alone")
            bound, _ = _bound(c, rk, a1, "cpu")
            if bound is None:
                assert np.array_equal(g2, g1, equal_nan=True), c.id
            else:
                assert (np.abs(g2.astype(np.float64) - g1) <= bound).all(), c.id


@pytest.mark.parametrize("op,inputs,attrs,opset", [
    ("Softmax", [_away(np.random.default_rng(5), 2, 3, 4)], {"axis": 0}, 11),       # flattened at axis 0: one row over the whole batch
    ("ReduceSum", [_away(np.random.default_rng(6), 2, 3, 4), _i64()], {}, 13),      # empty axes: every axis, the images' too
    ("ReduceMax", [_away(np.random.default_rng(7), 2, 3, 4)], {"keepdims": 0}, 13),
], ids=["softmax11_axis0", "reducesum_empty_axes", "reducemax_no_axes"])
def test_a_node_that_mixes_the_images_is_not_batched(op, inputs, attrs, opset):
    """Where the definition at this opset reads across the batch axis, the session must not take the batch for per-image work: no
    proof from shape_infer.batch_transparent, the batch-2 self-check notices, and every image gets its single-image answer."""
    c = Case("mixing", op, inputs, attrs, opset=opset, kind="trans" if op == "Softmax" else "sum" if op == "ReduceSum" else "exact", K=12)
    s = GraphSession(_one_node_graph(c), device="cpu")
    x = torch.from_numpy(inputs[0])
    both = s.run_named({"i0": x}, ["y0"])[0]
    assert s._batched_ok is False
    for k in range(2):
        y, aux = REF[op]([inputs[0][k:k + 1]] + inputs[1:], attrs, opset)
        _check(c, [both.reshape(2, -1)[k].numpy().reshape(y.shape)], [y], aux, "cpu", f" image {k}")


def _batch_axis(c, o, r, t1):
    """Where the images sit in output o of the model's batch-2 answer: the axis on which it is twice a single image's."""
    shape1 = tuple(t1.shape[1:]) if t1.dim() == r.ndim + 1 else tuple(t1.shape)
    if len(shape1) != r.ndim:
        shape1 = tuple(t1.shape)
    diff = [d for d in range(r.ndim) if r.shape[d] != shape1[d]]
    assert len(diff) == 1 and r.shape[diff[0]] == 2 * shape1[diff[0]], (c.id, r.shape, tuple(t1.shape))
    return diff[0]


# ---------------------------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def device():
    assert torch.cuda.is_available(), "needs the MI355X"
    return "cuda:0"


@pytest.mark.gpu
def test_ops_follow_the_onnx_definition_on_the_device(device):
    """Every case of the CPU list on the device, under the same bounds except the convolutions' (DEVICE_CONV_RATIO).  Prints the
    largest convolution ratio per case and the largest transcendental error per operator: what CONV_MEASURED / TRANS_MEASURED
    record from an MI355X — convolutions 0.87 (conv_2d_valid) to 2.779 (conv_2d_k1; convt_2d_asym 2.48, conv_2d_sym 2.086), every
    case listed there; transcendentals 6.74 at most (LayerNormalization; InstanceNormalization 6.318, HardSwish 2.495)."""
    failures, conv, trans = [], {}, {}
    for c in RUN:
        ref, aux = _reference(c.id)
        try:
            if c.kind == "conv":
                _one_tap_condition(c, aux, "cuda")
            worst = _check(c, _call(c, device), ref, aux, "cuda")
        except AssertionError as e:
            failures.append(f"{c.id}: {e}")
            continue
        if c.kind == "conv":
            conv[c.id] = worst
        elif c.kind == "trans":
            trans[c.op] = max(trans.get(c.op, 0.0), worst)
    print("convolution ratios:", {k: round(v, 3) for k, v in sorted(conv.items(), key=lambda kv: -kv[1])})
    print("transcendental units:", {k: round(v, 3) for k, v in sorted(trans.items(), key=lambda kv: -kv[1])})
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_refusals_hold_on_the_device(device):
    for c in CASES:
        if c.refuse is not None:
            with pytest.raises(NotImplementedError, match=c.refuse):
                _call(c, device)
