"""CPU: tests/onnx_ref.py — the numpy fp64 model of the ONNX operator definitions that test_executor_ops_onnx.py holds the
executor's op table to — against values worked out by hand from the definitions (the arithmetic is in the comments)."""
import numpy as np
import pytest

import onnx_ref
from onnx_ref import REF

X22 = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32).reshape(1, 1, 2, 2)


def _resize(x, attrs, sizes=None, scales=None, opset=13):
    inputs = [x, None, None if scales is None else np.asarray(scales, np.float32), None if sizes is None else np.asarray(sizes, np.int64)]
    return REF["Resize"](inputs, attrs, opset)[0]


@pytest.mark.parametrize("coord,row0,at11,at21", [
    # x_orig(o) = (o + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25, clamped to [0, 1]: weights 0, 0.25, 0.75, 1 on each axis.
    # row 0 (weight 0 down): 1 + t = 1, 1.25, 1.75, 2.  (1, 1): top 1.25, bottom 3.25, 0.25 down: 1.25 + 0.25 * 2 = 1.75.
    # (2, 1): 0.75 down: 1.25 + 0.75 * 2 = 2.75
    ("half_pixel", [1.0, 1.25, 1.75, 2.0], 1.75, 2.75),
    ("pytorch_half_pixel", [1.0, 1.25, 1.75, 2.0], 1.75, 2.75),            # (out > 1: the same coordinates)
    # x_orig(o) = o * (2 - 1) / (4 - 1) = 0, 1/3, 2/3, 1.  row 0: 1, 4/3, 5/3, 2.  (1, 1): 1 + 1/3 * 1 + 1/3 * 2 = 2.
    # (2, 1): 1 + 1/3 * 1 + 2/3 * 2 = 8/3
    ("align_corners", [1.0, 4 / 3, 5 / 3, 2.0], 2.0, 8 / 3),
    # x_orig(o) = o / 2 = 0, 0.5, 1, 1.5 -> 1 (clamped).  row 0: 1, 1.5, 2, 2.  (1, 1): 1 + 0.5 * 1 + 0.5 * 2 = 2.5.
    # (2, 1): weight 1 down: 3 + 0.5 = 3.5
    ("asymmetric", [1.0, 1.5, 2.0, 2.0], 2.5, 3.5),
])
def test_linear_resize_2x2_to_4x4_per_coordinate_mode(coord, row0, at11, at21):
    y = _resize(X22, {"mode": "linear", "coordinate_transformation_mode": coord}, sizes=[1, 1, 4, 4])
    assert y.shape == (1, 1, 4, 4)
    np.testing.assert_allclose(y[0, 0, 0], row0, rtol=0, atol=1e-15)
    np.testing.assert_allclose([y[0, 0, 1, 1], y[0, 0, 2, 1], y[0, 0, 3, 3]], [at11, at21, 4.0], rtol=0, atol=1e-15)
    # the same by scales = 2: out = floor(2 * 2), the coordinates divide by the given scale
    np.testing.assert_array_equal(_resize(X22, {"mode": "linear", "coordinate_transformation_mode": coord}, scales=[1, 1, 2, 2]), y)


def test_resize_to_one_pixel_pytorch_half_pixel_reads_the_origin():
    # out = 1: pytorch_half_pixel -> x_orig = 0 on both axes -> x[0, 0] = 1; half_pixel -> (0 + 0.5) / 0.5 - 0.5 = 0.5 on both
    # axes -> the mean of the four = 2.5
    assert _resize(X22, {"mode": "linear", "coordinate_transformation_mode": "pytorch_half_pixel"}, sizes=[1, 1, 1, 1]).item() == 1.0
    assert _resize(X22, {"mode": "linear", "coordinate_transformation_mode": "half_pixel"}, sizes=[1, 1, 1, 1]).item() == 2.5


@pytest.mark.parametrize("coord,nearest,index", [
    # half_pixel, scale 8 / 5: x_orig = (o + 0.5) / 1.6 - 0.5 = -0.1875 0.4375 1.0625 1.6875 2.3125 2.9375 3.5625 4.1875
    ("half_pixel", "round_prefer_floor", [0, 0, 1, 2, 2, 3, 4, 4]),     # ceil(x - 0.5): o = 2: ceil(0.5625) = 1; o = 3: ceil(1.1875) = 2
    ("half_pixel", "round_prefer_ceil", [0, 0, 1, 2, 2, 3, 4, 4]),      # floor(x + 0.5): o = 2: floor(1.5625) = 1; o = 6: floor(4.0625) = 4
    ("half_pixel", "floor", [0, 0, 1, 1, 2, 2, 3, 4]),                  # o = 0: floor(-0.1875) = -1 -> clamped to 0; o = 3: floor(1.6875) = 1
    ("half_pixel", "ceil", [0, 1, 2, 2, 3, 3, 4, 4]),                   # o = 1: ceil(0.4375) = 1; o = 7: ceil(4.1875) = 5 -> clamped to 4
    # asymmetric: x_orig = o / 1.6 = 0 0.625 1.25 1.875 2.5 3.125 3.75 4.375 — o = 4 is a tie
    ("asymmetric", "round_prefer_floor", [0, 1, 1, 2, 2, 3, 4, 4]),     # o = 4: ceil(2.5 - 0.5) = 2 (the tie goes down); o = 1: ceil(0.125) = 1
    ("asymmetric", "round_prefer_ceil", [0, 1, 1, 2, 3, 3, 4, 4]),      # o = 4: floor(2.5 + 0.5) = 3 (the tie goes up); o = 6: floor(4.25) = 4
    ("asymmetric", "floor", [0, 0, 1, 1, 2, 3, 3, 4]),                  # o = 1: floor(0.625) = 0; o = 5: floor(3.125) = 3
    ("asymmetric", "ceil", [0, 1, 2, 2, 3, 4, 4, 4]),                   # o = 2: ceil(1.25) = 2; o = 7: ceil(4.375) = 5 -> clamped to 4
])
def test_nearest_resize_5_to_8_under_each_nearest_mode(coord, nearest, index):
    x = np.arange(10, 15, dtype=np.float32).reshape(1, 1, 5)
    y = _resize(x, {"mode": "nearest", "coordinate_transformation_mode": coord, "nearest_mode": nearest}, sizes=[1, 1, 8])
    np.testing.assert_array_equal(y.reshape(-1) - 10, index)


def test_resize_defaults_by_opset():
    x = np.arange(10, 15, dtype=np.float32).reshape(1, 1, 5)
    # opset 11+, no attributes: half_pixel / round_prefer_floor (the first row of the table above)
    np.testing.assert_array_equal(_resize(x, {}, sizes=[1, 1, 8]).reshape(-1) - 10, [0, 0, 1, 2, 2, 3, 4, 4])
    # Resize-10 and Upsample: (X, scales), x_orig = o / 1.6, floor — out = floor(5 * 1.6) = 8 (fp32 1.6 is a little above 1.6)
    for op, opset in (("Resize", 10), ("Upsample", 9)):
        y = REF[op]([x, np.array([1, 1, 1.6], np.float32)], {"mode": "nearest"}, opset)[0]
        np.testing.assert_array_equal(y.reshape(-1) - 10, [0, 0, 1, 1, 2, 3, 3, 4])
        # linear: x_orig(1) = 1 / 1.6 = 0.625 -> 10.625; x_orig(7) = 4.375 -> clamped to 4 -> 14
        y = REF[op]([x, np.array([1, 1, 1.6], np.float32)], {"mode": "linear"}, opset)[0].reshape(-1)
        np.testing.assert_allclose([y[1], y[7]], [10.625, 14.0], rtol=0, atol=1e-6)


def test_conv_1d_asymmetric_pads():
    x = np.array([1, 2, 3, 4], np.float32).reshape(1, 1, 4)
    w = np.array([1, 10, 100], np.float32).reshape(1, 1, 3)
    # pads [2, 0]: the taps read 0 0 1 2 3 4.  y[0] = 0 + 0 + 1 * 100 = 100; y[1] = 0 + 1 * 10 + 2 * 100 = 210;
    # y[2] = 1 + 20 + 300 = 321; y[3] = 2 + 30 + 400 = 432
    y, aux = REF["Conv"]([x, w], {"pads": [2, 0]}, 13)
    np.testing.assert_array_equal(y.reshape(-1), [100, 210, 321, 432])
    np.testing.assert_array_equal(aux["mag"].reshape(-1), [100, 210, 321, 432])
    np.testing.assert_array_equal(aux["min_tap"].reshape(-1), [100, 10, 1, 2])      # the smallest product that reaches each output
    # pads [0, 2]: 1 2 3 4 0 0.  y[2] = 3 + 40 + 0 = 43; y[3] = 4
    np.testing.assert_array_equal(REF["Conv"]([x, w], {"pads": [0, 2]}, 13)[0].reshape(-1), [321, 432, 43, 4])
    # auto_pad on a size where total is odd: in 4, k 3, stride 2: out = 2, total = (2 - 1) * 2 + 3 - 4 = 1.
    # SAME_UPPER: begin 0, end 1: windows 1 2 3 | 3 4 0 -> 321, 43.  SAME_LOWER: begin 1: 0 1 2 | 2 3 4 -> 210, 432
    np.testing.assert_array_equal(REF["Conv"]([x, w], {"auto_pad": "SAME_UPPER", "strides": [2]}, 13)[0].reshape(-1), [321, 43])
    np.testing.assert_array_equal(REF["Conv"]([x, w], {"auto_pad": "SAME_LOWER", "strides": [2]}, 13)[0].reshape(-1), [210, 432])


def test_conv_transpose_1d_asymmetric_pads_output_shape_and_auto_pad():
    x = np.array([1, 2, 3], np.float32).reshape(1, 1, 3)
    w = np.array([1, 10, 100], np.float32).reshape(1, 1, 3)
    # stride 2: input cell i lands on 2 i + t.  full length 2 * 2 + 2 + 1 = 7: 1, 10, 100 + 2, 20, 200 + 3, 30, 300
    full = [1, 10, 102, 20, 203, 30, 300]
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2]}, 13)[0].reshape(-1), full)
    # pads [1, 0] crop one in front; [0, 1] one behind
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "pads": [1, 0]}, 13)[0].reshape(-1), full[1:])
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "pads": [0, 1]}, 13)[0].reshape(-1), full[:-1])
    # output_shape 6 = in * stride: total = 7 - 6 = 1.  SAME_UPPER: begin 1 // 2 = 0, end 1; anything else: begin 1 - 0 = 1, end 0
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "auto_pad": "SAME_UPPER"}, 13)[0].reshape(-1), full[:-1])
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "auto_pad": "SAME_LOWER"}, 13)[0].reshape(-1), full[1:])
    np.testing.assert_array_equal(REF["ConvTranspose"]([x, w], {"strides": [2], "output_shape": [6]}, 13)[0].reshape(-1), full[1:])
    # output_padding 1 lengthens the full output by a zero: output_shape 6 then has total 2: one cropped on each side
    y = REF["ConvTranspose"]([x, w], {"strides": [2], "output_padding": [1], "output_shape": [6]}, 13)[0]
    np.testing.assert_array_equal(y.reshape(-1), full[1:])


def test_ceil_mode_last_window_kept_and_dropped():
    x5 = np.arange(1, 6, dtype=np.float32).reshape(1, 1, 5)
    # in 5, k 2, stride 2, no pads: ceil((5 - 2) / 2) + 1 = 3; the last window starts at 4 < 5: kept, it holds cell 4 alone
    attrs = {"kernel_shape": [2], "strides": [2], "ceil_mode": 1}
    np.testing.assert_array_equal(REF["MaxPool"]([x5], attrs, 13)[0].reshape(-1), [2, 4, 5])
    np.testing.assert_array_equal(REF["MaxPool"]([x5], dict(attrs, ceil_mode=0), 13)[0].reshape(-1), [2, 4])
    # in 3, pads [1, 1], k 2, stride 2: ceil((5 - 2) / 2) + 1 = 3; the third window would start at 2 * 2 = 4 >= in + pb = 4: dropped.
    # windows: cells -1 0 -> 1; cells 1 2 -> 3
    x3 = np.arange(1, 4, dtype=np.float32).reshape(1, 1, 3)
    attrs = {"kernel_shape": [2], "strides": [2], "pads": [1, 1], "ceil_mode": 1}
    np.testing.assert_array_equal(REF["MaxPool"]([x3], attrs, 13)[0].reshape(-1), [1, 3])
    # the same windows averaged: count_include_pad 0: 1 / 1, (2 + 3) / 2; 1: (0 + 1) / 2, 2.5
    np.testing.assert_array_equal(REF["AveragePool"]([x3], attrs, 13)[0].reshape(-1), [1, 2.5])
    np.testing.assert_array_equal(REF["AveragePool"]([x3], dict(attrs, count_include_pad=1), 13)[0].reshape(-1), [0.5, 2.5])


def test_count_include_pad_pair():
    x = np.arange(1, 6, dtype=np.float32).reshape(1, 1, 5)
    # in 5, k 3, stride 2, pads [1, 1]: (7 - 3) / 2 + 1 = 3 windows over cells {-1 0 1}, {1 2 3}, {3 4 5}
    attrs = {"kernel_shape": [3], "strides": [2], "pads": [1, 1]}
    # 0: (1 + 2) / 2 = 1.5, (2 + 3 + 4) / 3 = 3, (4 + 5) / 2 = 4.5
    y, aux = REF["AveragePool"]([x], dict(attrs, count_include_pad=0), 13)
    np.testing.assert_array_equal(y.reshape(-1), [1.5, 3, 4.5])
    np.testing.assert_array_equal(aux["mag"].reshape(-1), [1.5, 3, 4.5])
    # 1: 3 / 3 = 1, 3, 9 / 3 = 3
    np.testing.assert_array_equal(REF["AveragePool"]([x], dict(attrs, count_include_pad=1), 13)[0].reshape(-1), [1, 3, 3])
    # a cell that exists only because of ceil mode is never counted: k 2, stride 2, no pads, ceil: {0 1} {2 3} {4 (5)} -> 5 / 1
    attrs = {"kernel_shape": [2], "strides": [2], "ceil_mode": 1, "count_include_pad": 1}
    np.testing.assert_array_equal(REF["AveragePool"]([x], attrs, 13)[0].reshape(-1), [1.5, 3.5, 5])


def test_softmax_before_opset_13_flattens_at_axis():
    x = np.log(np.array([[[1, 2], [3, 4], [5, 5]], [[1, 1], [2, 2], [2, 2]]], np.float64)).astype(np.float32)    # [2, 3, 2]
    # opset 11, default axis 1: rows of 3 * 2 = 6.  image 0: exp sums to 1 + 2 + 3 + 4 + 5 + 5 = 20: [0, 0, 1] = 2 / 20,
    # [0, 2, 0] = 5 / 20; image 1: sum 10: [1, 1, 0] = 2 / 10
    y = REF["Softmax"]([x], {}, 11)[0]
    np.testing.assert_allclose([y[0, 0, 1], y[0, 2, 0], y[1, 1, 0]], [0.1, 0.25, 0.2], rtol=0, atol=1e-7)
    # axis 2 at opset 11: rows of 2: [0, 0, 1] = 2 / 3; axis 0: one row of 12, sum 30: [0, 0, 1] = 2 / 30
    assert abs(REF["Softmax"]([x], {"axis": 2}, 11)[0][0, 0, 1] - 2 / 3) < 1e-7
    assert abs(REF["Softmax"]([x], {"axis": 0}, 11)[0][0, 0, 1] - 2 / 30) < 1e-7
    # opset 13: along one axis, default the last: [0, 0, 1] = 2 / 3, [0, 2, 0] = 5 / 10; axis 1: [0, 0, 1] = 2 / (2 + 4 + 5)
    y = REF["Softmax"]([x], {}, 13)[0]
    np.testing.assert_allclose([y[0, 0, 1], y[0, 2, 0]], [2 / 3, 0.5], rtol=0, atol=1e-7)
    assert abs(REF["Softmax"]([x], {"axis": 1}, 13)[0][0, 0, 1] - 2 / 11) < 1e-7


def test_pad_with_axes_modes_and_negative_pads():
    x = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    axes = np.array([-1], np.int64)

    def pad(pads, mode="constant", value=None):
        return REF["Pad"]([x, np.array(pads, np.int64), value, axes], {"mode": mode}, 18)[0]
    # pads [1, 2] on the LAST axis only: position 0 is padding, position 1 is x[:, 0]
    np.testing.assert_array_equal(pad([1, 2]), [[0, 1, 2, 3, 0, 0], [0, 4, 5, 6, 0, 0]])
    np.testing.assert_array_equal(pad([1, 0], value=np.array(7, np.float32)), [[7, 1, 2, 3], [7, 4, 5, 6]])
    # reflect [2, 1]: positions -2 -1 | 0 1 2 | 3 mirror about the ends without repeating them: 3 2 | 1 2 3 | 2
    np.testing.assert_array_equal(pad([2, 1], "reflect")[0], [3, 2, 1, 2, 3, 2])
    # edge [1, 2]: 1 | 1 2 3 | 3 3
    np.testing.assert_array_equal(pad([1, 2], "edge")[0], [1, 1, 2, 3, 3, 3])
    # a negative pad crops: [-1, 1]: position 0 is x[:, 1]: 2 3 0
    np.testing.assert_array_equal(pad([-1, 1]), [[2, 3, 0], [5, 6, 0]])
    # without axes the pads cover every axis: [b0, b1, e0, e1] = [1, 0, 0, 1] -> a row in front, a column behind
    y = REF["Pad"]([x, np.array([1, 0, 0, 1], np.int64)], {}, 13)[0]
    np.testing.assert_array_equal(y, [[0, 0, 0, 0], [1, 2, 3, 0], [4, 5, 6, 0]])


def test_small_definitions():
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    # Gather: index -1 on an axis of 3 is 2
    np.testing.assert_array_equal(REF["Gather"]([x, np.array([-1, 0], np.int64)], {"axis": 1}, 13)[0], x[:, [2, 0]])
    # Split, num_outputs 3 of an axis of 5: chunks of ceil(5 / 3) = 2, the last one smaller: 2, 2, 1
    x5 = np.arange(10, dtype=np.float32).reshape(2, 5)
    parts = REF["Split"]([x5], {"axis": 1, "num_outputs": 3}, 18)[0]
    assert [p.shape[1] for p in parts] == [2, 2, 1] and parts[2][1, 0] == 9
    # Reduce with absent / empty axes: everything, or identity with noop_with_empty_axes = 1
    assert REF["ReduceSum"]([x], {"keepdims": 0}, 13)[0] == 276
    np.testing.assert_array_equal(REF["ReduceSum"]([x, np.array([], np.int64)], {"noop_with_empty_axes": 1}, 13)[0], x)
    assert REF["ReduceSum"]([x, np.array([], np.int64)], {"keepdims": 0}, 13)[0] == 276
    # Slice: INT64 bounds clamp; a negative step walks down to (not including) the clamped end
    big = onnx_ref.INT64_MAX
    y = REF["Slice"]([x, np.array([-1], np.int64), np.array([onnx_ref.INT64_MIN], np.int64), np.array([2], np.int64), np.array([-1], np.int64)], {}, 13)[0]
    np.testing.assert_array_equal(y, x[:, :, ::-1])
    y = REF["Slice"]([x, np.array([1], np.int64), np.array([big], np.int64), np.array([2], np.int64), np.array([2], np.int64)], {}, 13)[0]
    np.testing.assert_array_equal(y, x[:, :, 1::2])
    # Flatten at axis 0 and at a negative axis
    assert REF["Flatten"]([x], {"axis": 0}, 13)[0].shape == (1, 24) and REF["Flatten"]([x], {"axis": -1}, 13)[0].shape == (6, 4)
    # Relu, Clip and MaxPool keep a NaN
    n = np.array([[[np.nan, 1.0, -2.0, 3.0]]], np.float32)
    assert np.isnan(REF["Relu"]([n], {}, 13)[0][0, 0, 0]) and np.isnan(REF["Clip"]([n, np.float32(-1), np.float32(1)], {}, 13)[0][0, 0, 0])
    y = REF["MaxPool"]([n], {"kernel_shape": [2], "strides": [2]}, 13)[0].reshape(-1)
    assert np.isnan(y[0]) and y[1] == 3


# ------------------------------------------------------------------------------------------------ QuantizeLinear / DequantizeLinear
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f8zero(shape=()):
    return onnx_ref.Float8E4M3FN(np.zeros(shape, np.uint8))


def test_quantize_linear_by_hand():
    # scale 0.5: x / scale = 1, 3, 5, -1, -3 halves -> 0.5 1.5 2.5 -0.5 -1.5: ties go to the even integer: 0 2 2 -0 -2
    x = np.array([0.25, 0.75, 1.25, -0.25, -0.75, -0.0, 100.0, -100.0], np.float32)
    s = np.float32(0.5)
    # int8, zero point -5: 0 2 2 0 -2 0 -> -5 -3 -3 -5 -7 -5; 200 - 5 saturates to 127, -200 - 5 to -128
    q, _ = REF["QuantizeLinear"]([x, s, np.array(-5, np.int8)], {}, 13)
    assert q.dtype == np.int8 and q.tolist() == [-5, -3, -3, -5, -7, -5, 127, -128]
    # back: (q + 5) * 0.5 = 0 1 1 0 -1 0 66 -61.5, and the zero of a -0.0 is +0.0 (an integer difference has no sign)
    y, _ = REF["DequantizeLinear"]([q, s, np.array(-5, np.int8)], {}, 13)
    assert y.dtype == np.float32 and y.tolist() == [0, 1, 1, 0, -1, 0, 66, -61.5] and not np.signbit(y[5])
    # uint8, zero point 200 (above 127): 200 202 202 200 198 200, saturating to 255 and 0; no zero point at all: uint8 zero
    q, _ = REF["QuantizeLinear"]([x, s, np.array(200, np.uint8)], {}, 13)
    assert q.dtype == np.uint8 and q.tolist() == [200, 202, 202, 200, 198, 200, 255, 0]
    assert REF["DequantizeLinear"]([q, s, np.array(200, np.uint8)], {}, 13)[0].tolist() == [0, 1, 1, 0, -1, 0, 27.5, -100]
    q, _ = REF["QuantizeLinear"]([x, s], {}, 13)
    assert q.dtype == np.uint8 and q.tolist() == [0, 2, 2, 0, 0, 0, 200, 0]
    # x / y_scale is an fp32 division: 0.35 / 0.1 is 3.5 in fp32 (a tie -> 4) and 3.4999999 in fp64 (-> 3)
    assert np.float32(0.35) / np.float32(0.1) == np.float32(3.5) and np.float64(np.float32(0.35)) / np.float64(np.float32(0.1)) < 3.5
    assert REF["QuantizeLinear"]([np.array([0.35], np.float32), np.float32(0.1), np.array(0, np.int8)], {}, 13)[0].tolist() == [4]
    # types must match at DequantizeLinear; a NaN has no integer code in the text: the lower end here
    with pytest.raises(ValueError, match="differ in type"):
        REF["DequantizeLinear"]([q, s, np.array(0, np.int8)], {}, 13)
    assert REF["QuantizeLinear"]([np.array([np.nan], np.float32), s, np.array(3, np.int8)], {}, 13)[0].tolist() == [-128]


def test_quantize_linear_per_axis():
    x = np.arange(-6, 6, dtype=np.float32).reshape(2, 3, 2)          # [[-6 -5] [-4 -3] [-2 -1]] [[0 1] [2 3] [4 5]]
    s3, z3 = np.array([1, 2, 4], np.float32), np.array([0, 10, -10], np.int8)
    # axis 1 (the default): rows scaled by 1, 2, 4: -6 -5 | -2 -1.5 | -0.5 -0.25 -> -6 -5 | -2 -2 | -0 -0, plus 0, 10, -10
    q, _ = REF["QuantizeLinear"]([x, s3, z3], {}, 13)
    assert q[0].tolist() == [[-6, -5], [8, 8], [-10, -10]] and q[1].tolist() == [[0, 1], [11, 12], [-9, -9]]
    y, _ = REF["DequantizeLinear"]([q, s3, z3], {"axis": 1}, 13)
    assert y[0].tolist() == [[-6, -5], [-4, -4], [0, 0]] and y[1].tolist() == [[0, 1], [2, 4], [4, 4]]
    # axis 0 and axis -1, two scales; a number of scales that is not the axis' extent is refused, at either operator
    s2 = np.array([1, 4], np.float32)
    q0, _ = REF["QuantizeLinear"]([x, s2, np.zeros(2, np.int8)], {"axis": 0}, 13)
    assert q0[0].tolist() == [[-6, -5], [-4, -3], [-2, -1]] and q0[1].tolist() == [[0, 0], [0, 1], [1, 1]]
    assert np.array_equal(REF["QuantizeLinear"]([x, s2, np.zeros(2, np.int8)], {"axis": -1}, 13)[0][1], [[0, 0], [2, 1], [4, 1]])
    with pytest.raises(ValueError, match="y_scale"):
        REF["QuantizeLinear"]([x, s2, np.zeros(2, np.int8)], {"axis": 1}, 13)
    with pytest.raises(ValueError, match="x_scale"):
        REF["DequantizeLinear"]([q, s2, np.zeros(2, np.int8)], {"axis": 1}, 13)
    # one element, whatever the axis says: the whole tensor
    assert np.array_equal(REF["QuantizeLinear"]([x, np.array([2], np.float32), np.array([1], np.int8)], {"axis": 1}, 13)[0][1],
                          [[1, 1], [2, 3], [3, 3]])


def test_float8e4m3fn_codes_by_hand():
    enc, dec = onnx_ref.e4m3fn_encode, onnx_ref.e4m3fn_decode
    # 1 = 2^(7 - 7): exponent field 7, mantissa 0: 0x38; 448 = 1.75 * 2^8: 0x7e; the smallest subnormal 2^-9: 0x01; -0.0: 0x80
    assert enc(np.array([1.0, 448.0, 2.0 ** -9, -0.0, -1.5], np.float32)).tolist() == [0x38, 0x7E, 0x01, 0x80, 0xBC]
    assert dec(np.array([0x38, 0x7E, 0x01, 0xBC], np.uint8)).tolist() == [1.0, 448.0, 2.0 ** -9, -1.5] and np.isnan(dec(np.array([0x7F, 0xFF], np.uint8))).all()
    # ties go to the even mantissa: 1.0625 between 1 (0x38) and 1.125 (0x39) -> 0x38; 1.1875 between 0x39 and 1.25 (0x3a) -> 0x3a;
    # 2^-10, half the smallest subnormal, between 0x00 and 0x01 -> 0x00; 464 between 448 and the 480 the format lacks -> 448
    assert enc(np.array([1.0625, 1.1875, 2.0 ** -10, 464.0], np.float32)).tolist() == [0x38, 0x3A, 0x00, 0x7E]
    # out of range: saturate = 1 (the default) gives +-448, saturate = 0 NaN; NaN stays NaN either way
    big = np.array([465.0, -1e9, np.inf, -np.inf, np.nan], np.float32)
    assert enc(big).tolist() == [0x7E, 0xFE, 0x7E, 0xFE, 0x7F] and (enc(big, saturate=False) & 0x7F).tolist() == [0x7F] * 5
    q, _ = REF["QuantizeLinear"]([big, np.float32(1), _f8zero()], {"saturate": 0}, 19)
    assert isinstance(q, onnx_ref.Float8E4M3FN) and (np.asarray(q) & 0x7F).tolist() == [0x7F] * 5
    with pytest.raises(ValueError, match="opset 13"):
        REF["QuantizeLinear"]([big, np.float32(1), _f8zero()], {}, 13)
    # every code decodes and encodes back to itself
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    assert np.array_equal(np.asarray(enc(dec(codes))), codes)


@pytest.mark.parametrize("signed", [True, False], ids=["int8", "uint8"])
def test_integer_pair_is_the_oracle_bit_for_bit(signed):
    """DequantizeLinear(QuantizeLinear(x)) against oracle.np_oracle.fake_quant_qdq (the model the k_fake_quant kernels are held to),
    per tensor and per channel on axes 0 and 1, stored zero points above 127 included: exact .5 ties under power-of-two scales,
    both saturation ends and one step inside them, -0.0, and random values under arbitrary scales."""
    from oracle import np_oracle as O
    rng = np.random.default_rng(7)
    zps = [0, -128, 127, -65, 5] if signed else [0, 255, 128, 191, 37]                      # (191 is stored as int8 -65)
    k = np.arange(-300, 301, dtype=np.float32)
    for zp in zps:
        stored = np.array(zp, np.int8 if signed else np.uint8)
        for scale in (0.5, 0.0625, 4.0, 0.1, 0.0371):
            s = np.float32(scale)
            x = np.concatenate([(k + 0.5) * s, k * s, np.nextafter((k + 0.5) * s, np.float32(np.inf)), np.array([-0.0, 0.0, 1e30, -1e30, np.inf, -np.inf], np.float32),
                                (rng.standard_normal(500) * 100 * scale).astype(np.float32)]).astype(np.float32)
            y, q = onnx_ref.qdq_pair(x, s, stored, {}, 13)
            want = O.fake_quant_qdq(x, s, stored.view(np.int8), signed=signed)
            assert np.array_equal(_bits(y), _bits(want)), (zp, scale)
            info = np.iinfo(stored.dtype)
            assert (q == info.min).any() and (q == info.max).any()
    x = (rng.standard_normal((6, 5, 4)) * 40).astype(np.float32)
    x[0, 0, 0], x[1, 1, 1] = -0.0, 1e9
    for axis in (0, 1):
        n = x.shape[axis]
        s = (2.0 ** rng.integers(-3, 2, n)).astype(np.float32) * np.where(np.arange(n) % 2, np.float32(1), np.float32(0.3))
        z = rng.integers(-128, 128, n).astype(np.int8) if signed else rng.integers(0, 256, n).astype(np.uint8)
        y, _ = onnx_ref.qdq_pair(x, s, z, {"axis": axis}, 13)
        assert np.array_equal(_bits(y), _bits(O.fake_quant_qdq(x, s, z.view(np.int8), axis=axis, signed=signed))), axis


def test_fp8_pair_is_the_fp8_model_bit_for_bit():
    """Opset 19 with a float8e4m3fn zero point against tests/fp8_model.py fake_quant_fp8 (held to torch's cast; the k_fake_quant
    FP8 kernels are held to it): every boundary point of the format and the special values, per tensor and per channel."""
    import fp8_model
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-9, -1e-9, 2.0 ** -10, -2.0 ** -10, 1e30, -1e30, 2.0 ** -149], np.float32)
    pts = np.concatenate([fp8_model.boundary_points(), special])
    for scale in (1.0, 0.5, 0.0371, 3.0, 2.0 ** -20):
        y, q = onnx_ref.qdq_pair((pts.astype(np.float64) * np.float32(scale)).astype(np.float32), np.float32(scale), _f8zero(), {}, 19)
        want = fp8_model.fake_quant_fp8((pts.astype(np.float64) * np.float32(scale)).astype(np.float32), scale)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(y), nan) and nan.sum() == 1 and np.array_equal(_bits(y)[~nan], _bits(want)[~nan]), scale
        v = onnx_ref.e4m3fn_decode(q)
        assert (v == 448).any() and (v == -448).any()
    x = np.resize(pts, (4, 6, 50)).copy()
    for axis in (0, 1):
        s = np.array([1.0, 0.25, 0.0371, 3.0, 0.5, 7.0][:x.shape[axis]], np.float32)
        y, _ = onnx_ref.qdq_pair(x, s, _f8zero(s.shape), {"axis": axis}, 19)
        want = fp8_model.fake_quant_fp8(x, s, axis)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(y), nan) and np.array_equal(_bits(y)[~nan], _bits(want)[~nan]), axis


def test_project_domain_entries_defer_to_their_models():
    import mx_model
    import mx_rotate_model
    x = (np.random.default_rng(3).standard_normal((3, 48, 2)) * 5).astype(np.float32)
    for elem, name in (("mxfp8", "float8e4m3fn"), ("mxfp4", "float4e2m1")):
        y, aux = REF["MXQuantizeDequantize"]([x], {"axis": 1, "block_size": 32, "elem_type": name}, 13)
        want, scales = mx_model.fake_quant_mx(x, 1, elem, return_scales=True)
        assert np.array_equal(_bits(y), _bits(want)) and np.array_equal(aux["scales"], scales) and scales.shape == (3, 2, 2)
    with pytest.raises(ValueError, match="block_size"):
        REF["MXQuantizeDequantize"]([x], {"axis": 1, "block_size": 16, "elem_type": "float4e2m1"}, 13)
    x = np.random.default_rng(4).standard_normal((5, 64)).astype(np.float32)
    assert np.array_equal(_bits(REF["BlockHadamard"]([x], {"block_size": 32}, 13)[0]), _bits(mx_rotate_model.fwht32(x)))


def test_gemm_and_matmul_by_hand():
    a = np.array([[1, -2], [3, 4]], np.float32)
    b = np.array([[5, 6], [-7, 8]], np.float32)
    # a b = [[5 + 14, 6 - 16], [15 - 28, 18 + 32]]; the magnitudes add up without signs
    y, aux = REF["MatMul"]([a, b], {}, 13)
    assert y.tolist() == [[19, -10], [-13, 50]] and aux["mag"].tolist() == [[19, 22], [43, 50]]
    # Gemm: 2 a^T b^T + 3 c, c = [10, -20] along N.  a^T = [[1, 3], [-2, 4]], b^T = [[5, -7], [6, 8]]: a^T b^T = [[23, 17], [14, 46]]
    y, aux = REF["Gemm"]([a, b, np.array([10, -20], np.float32)], {"transA": 1, "transB": 1, "alpha": 2.0, "beta": 3.0}, 13)
    assert y.tolist() == [[76, -26], [58, 32]] and aux["mag"].tolist() == [[2 * 23 + 30, 2 * 31 + 60], [2 * 34 + 30, 2 * 46 + 60]]
    assert REF["Gemm"]([a, b], {}, 13)[0].tolist() == [[19, -10], [-13, 50]]
